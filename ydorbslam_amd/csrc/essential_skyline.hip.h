// gfx950 HIP kernels of the essential graph's block-skyline Cholesky: H + lambda I stored as the envelope of
// 7x7 blocks that skyline_plan.h lays out, factorised in place and solved, in fp64 with every entry summed in a fixed order.
//
// Storage: row i (a position of the plan's order) holds the blocks of columns first[i] .. i, each [r][c] row-major, block (i, j) at
// 49 * (rowOff[i] + j - first[i]).  Of a diagonal block the lower triangle is read.  b is held by position, x goes out by free vertex.
//
// Shared with the dense path (essential_kernels.hip.h): ess_vertex_sums, the sums of one free vertex.  Shared with the BA's skyline
// solver (sky_blocks.hip.h): the Cholesky of a diagonal block, the row substitutions against it and the packed-triangle index.  The
// walk over the block columns is this kernel's own.
//
// k_ess_assemble_sky  one wave per free vertex clears its row of the envelope and runs ess_vertex_sums over it: the diagonal block in
//                     edge order and one block per neighbour in edge order, a neighbour's block written only when the neighbour comes
//                     earlier in the order (the other endpoint's wave writes it otherwise, from its own side of the same edges: the
//                     transposed block).  No atomics.
// k_ess_sky_solve     one workgroup walks the block columns: every thread factorises the 7x7 diagonal block in registers (the same
//                     arithmetic 256 times costs no more time than once and saves a barrier), the rows of the column's panel and b,
//                     as one more row, are solved against it, barrier, the blocks of every pair of rows in the column's list take
//                     their rank-7 update, barrier.  Then the rows are walked downwards for the back substitution.  Every barrier is
//                     reached by every thread: the loop bounds are the plan's, and a non-positive pivot is replaced by 1 and reported
//                     in status[0] at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "essential_kernels.hip.h"
#include "sky_blocks.hip.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace ess {

// Row pos of the envelope: the diagonal block, which ends the row, a neighbour's block only when the neighbour comes earlier in the
// order (the other endpoint's wave writes it otherwise, from its own side of the same edges: the transposed block); b by free vertex
// and by position
struct EssEnvelopeDst {
  R* row; size_t off; const int* inv; int pos, f0, a; R *bkeep, *bwork;   // off: the blocks before the diagonal one
  __device__ void diag(int r, int c, R v) const { row[off + 7 * r + c] = v; }
  __device__ void nbr(int o, int r, int c, R v) const { if (inv[o] < pos) row[49 * (size_t)(inv[o] - f0) + 7 * r + c] = v; }
  __device__ void b(int r, R v) const { bkeep[7 * (size_t)a + r] = v; bwork[7 * (size_t)pos + r] = v; }
};

__global__ __launch_bounds__(64) void k_ess_assemble_sky(int nF, R lambda, const int* __restrict__ incStart, const int* __restrict__ incE,
                                                         const int* __restrict__ incN, const int* __restrict__ incO, const R* __restrict__ Hb,
                                                         const R* __restrict__ bb, const int* __restrict__ inv, const int* __restrict__ first,
                                                         const long long* __restrict__ rowOff, R* __restrict__ A, R* __restrict__ bkeep,
                                                         R* __restrict__ bwork, int* __restrict__ status) {
  const int a = blockIdx.x, lane = threadIdx.x;
  if (a >= nF) {   // the status word of this trial's factorisation
    if (lane == 0) status[0] = 0;
    return;
  }
  const int pos = inv[a], f0 = first[pos];
  R* row = A + 49 * (size_t)rowOff[pos];
  const size_t off = 49 * (size_t)(pos - f0);   // the blocks before the diagonal one, which is written whole below
  for (size_t i = lane; i < off; i += 64) row[i] = 0;
  __syncthreads();   // the cleared row is in memory before the blocks go over it
  ess_vertex_sums(a, lane, lambda, incStart, incE, incN, incO, Hb, bb, EssEnvelopeDst{row, off, inv, pos, f0, a, bkeep, bwork});
}

// One entry of the rank-7 update of column j: *dst -= a[0..6] . b[0..6].  Item w of the column addresses, from the plan alone,
//   w < 49 pairs: entry e = w % 49 of block (i, k) for the pair p = w / 49 = ia (ia + 1) / 2 + ik of list members, k <= i: rows r of L_ij and c of L_kj
//   else:         b_i[r] for the list member (w - 49 pairs) / 7: row r of L_ij and y_j
struct UpdateItem { const R *a, *b; R* dst; };
__device__ __forceinline__ UpdateItem updateItem(long long w, long long pairs, int j, long long cs, const int* __restrict__ colRows,
                                                 const long long* __restrict__ colBlk, R* A, R* bw) {
  UpdateItem u;
  if (w < 49 * pairs) {
    const long long p = w / 49;
    const int e = (int)(w - 49 * p), r = e / 7, c = e - 7 * r;
    const int ia = sky::triRow(p);
    const int ik = (int)(p - (long long)ia * (ia + 1) / 2);
    const long long bi = colBlk[cs + ia], bk = colBlk[cs + ik];
    u.a = A + 49 * (size_t)bi + 7 * r;
    u.b = A + 49 * (size_t)bk + 7 * c;
    u.dst = A + 49 * (size_t)(bi - j + colRows[cs + ik]) + e;   // block (i, k) lies k - j blocks after block (i, j)
  } else {
    const int t = (int)(w - 49 * pairs), ia = t / 7, r = t - 7 * ia;
    u.a = A + 49 * (size_t)colBlk[cs + ia] + 7 * r;
    u.b = bw + 7 * (size_t)j;
    u.dst = bw + 7 * (size_t)colRows[cs + ia] + r;
  }
  return u;
}
__device__ __forceinline__ void applyUpdate(const UpdateItem& u) {
  R s = *u.dst;
#pragma unroll
  for (int q = 0; q < 7; q++) s -= u.a[q] * u.b[q];
  *u.dst = s;
}

// A, bw and x are read and written by different threads across the barriers: no __restrict__ on them.  Every column is a chain of
// dependent global-memory round trips, so each thread's first item of a phase is addressed (and, where the data are final, loaded)
// before the step it would otherwise wait behind; items past the first 256 take the plain loop.
__global__ __launch_bounds__(256) void k_ess_sky_solve(int nF, const int* __restrict__ first, const long long* __restrict__ rowOff,
                                                       const long long* __restrict__ colStart, const int* __restrict__ colRows,
                                                       const long long* __restrict__ colBlk, const int* __restrict__ perm, R* A, R* bw, R* x,
                                                       R* dinv, int* status) {
  const int tid = threadIdx.x;
  bool bad = false;
  for (int j = 0; j < nF; j++) {
    R l[28], inv[7];
    R* D = A + 49 * (size_t)(rowOff[j + 1] - 1);   // the diagonal block ends its row
    const long long cs = colStart[j];
    const int m = (int)(colStart[j + 1] - cs), nPanel = 7 * m + 1;
    // the panel: row t % 7 of the block of the list's row t / 7, and b_j as the last row
    auto panelRow = [&](int t) -> R* { return t < 7 * m ? A + 49 * (size_t)colBlk[cs + t / 7] + 7 * (t % 7) : bw + 7 * (size_t)j; };
    R* row = nullptr;
    R v[7];
    if (tid < nPanel) {   // final since the last barrier: loaded while the diagonal block is factorised
      row = panelRow(tid);
#pragma unroll
      for (int c = 0; c < 7; c++) v[c] = row[c];
    }
    if (!sky::factorBlock<7>(D, l, inv)) bad = true;
    if (tid < nPanel) {
      sky::solveRow<7>(v, l, inv);
#pragma unroll
      for (int c = 0; c < 7; c++) row[c] = v[c];
    }
    for (int t = tid + 256; t < nPanel; t += 256) {
      row = panelRow(t);
#pragma unroll
      for (int c = 0; c < 7; c++) v[c] = row[c];
      sky::solveRow<7>(v, l, inv);
#pragma unroll
      for (int c = 0; c < 7; c++) row[c] = v[c];
    }
    // the rank-7 update: block (i, k) -= L_ij L_kj^T for every pair k <= i of the list, and b_i -= L_ij y_j
    const long long pairs = (long long)m * (m + 1) / 2, items = 49 * pairs + 7 * (long long)m;
    UpdateItem u0{nullptr, nullptr, nullptr};
    if (tid < items) u0 = updateItem(tid, pairs, j, cs, colRows, colBlk, A, bw);
    __syncthreads();   // the panel and y_j are written, and every thread has read D
    if (tid == 0) sky::storeFactor<7>(D, dinv, j, l, inv);
    if (tid < items) applyUpdate(u0);
    for (long long w = tid + 256; w < items; w += 256) applyUpdate(updateItem(w, pairs, j, cs, colRows, colBlk, A, bw));
    __syncthreads();   // column j + 1 and b_{j+1} are final
  }
  // L^T x = y, the rows downwards: x_i from the diagonal block, then y_j -= L_ij^T x_i along the row
  for (int i = nF - 1; i >= 0; i--) {
    const int f0 = first[i];
    const R* rowp = A + 49 * (size_t)rowOff[i];
    const R* D = rowp + 49 * (size_t)(i - f0);
    const int items = 7 * (i - f0);
    R bcol[7], s0 = 0;
    if (tid < items) {   // column c of block tid / 7 and its y entry: final, loaded while x_i is solved
      const int jb = tid / 7, c = tid - 7 * jb;
#pragma unroll
      for (int r = 0; r < 7; r++) bcol[r] = rowp[49 * (size_t)jb + 7 * r + c];
      s0 = bw[7 * (size_t)f0 + tid];
    }
    R xv[7];
    sky::solveDiagBack<7>(D, dinv, bw, i, xv);
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < 7; c++) x[7 * (size_t)perm[i] + c] = xv[c];
    }
    if (tid < items) {
#pragma unroll
      for (int r = 0; r < 7; r++) s0 -= bcol[r] * xv[r];
      bw[7 * (size_t)f0 + tid] = s0;
    }
    for (int t = tid + 256; t < items; t += 256) {
      const int jb = t / 7, c = t - 7 * jb;
      const R* B = rowp + 49 * (size_t)jb;
      R s = bw[7 * (size_t)f0 + t];
#pragma unroll
      for (int r = 0; r < 7; r++) s -= B[7 * r + c] * xv[r];
      bw[7 * (size_t)f0 + t] = s;
    }
    __syncthreads();   // y_{i-1} is final
  }
  if (bad && tid == 0) status[0] = 1;
}

}  // namespace ess
}  // namespace ydorb
