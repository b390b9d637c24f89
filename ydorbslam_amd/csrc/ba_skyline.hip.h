// gfx950 HIP kernels of the BA's block-skyline reduced camera solve: the Schur complement S stored as the
// envelope of 6x6 blocks that ba_pairs.h / skyline_plan.h lay out, factorised in place and solved, in fp64 with every entry summed in
// a fixed order.  The dense kernels of ba_kernels.hip.h are not touched; these take their place when the solver is SKYLINE.
//
// Buckets: one per covisible pair of free poses and one per free pose (ba_pairs.h, PairList), ordered by (i2, i1) like the dense
// path's triangular index, so that bucket q of row i2 is found by a binary search for i1 in pairI1[rowStart[i2] .. rowStart[i2 + 1]).
// Storage: row i (a position of the plan's order) holds the blocks of columns first[i] .. i, each [r][c] row-major, block (i, j) at
// 36 * (rowOff[i] + j - first[i]).  Of a diagonal block the lower triangle is read.
//
// Shared with the dense path (ba_kernels.hip.h): pair_walk, the loop over a landmark's pairs of free poses, and schur_block, the sum
// of one bucket on the matrix core.  Shared with the essential graph's solver (sky_blocks.hip.h): the Cholesky of a diagonal block,
// the row substitutions against it and the packed-triangle index.  The walk over the block columns is this kernel's own.
//
// k_sky_pair_count / k_sky_pair_fill   pair_walk with the bucket looked up in the pair table (k_excl_scan and k_pair_sort are used
//                     as they are)
// k_sky_schur_pairs   schur_block, stored to the block's place in the envelope, transposed when the order puts i1 after i2
// k_sky_solve         one workgroup of 1024 walks the block columns: every thread factorises the 6x6 diagonal block in registers, the
//                     rows of the column's panel and b, as one more row, are solved against it (and kept in LDS when the panel fits),
//                     barrier, the blocks of every pair of rows in the column's list take their rank-6 update, barrier.  Then the rows
//                     are walked downwards for the back substitution.  Every barrier is reached by every thread: the loop bounds are
//                     the plan's, and a non-positive pivot is replaced by 1 and reported in status[0] at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ba_kernels.hip.h"
#include "sky_blocks.hip.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace ba {

__device__ __forceinline__ int sky_bucket(const int* __restrict__ rowStart, const int* __restrict__ pairI1, int i1, int i2) {  // i1 <= i2
  int lo = rowStart[i2], hi = rowStart[i2 + 1] - 1;   // the row ends with its diagonal bucket, i1 == i2
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pairI1[mid] < i1) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_sky_pair_count(EdgeSoA Ed, const int* __restrict__ ptStart, int nL, const int* __restrict__ rowStart,
                                                        const int* __restrict__ pairI1, int* __restrict__ cnt) {
  pair_walk(Ed, ptStart, nL, [&](int, int, int i1, int i2) { atomicAdd(&cnt[sky_bucket(rowStart, pairI1, i1, i2)], 1); });
}
__global__ __launch_bounds__(256) void k_sky_pair_fill(EdgeSoA Ed, const int* __restrict__ ptStart, int nL, const int* __restrict__ rowStart,
                                                       const int* __restrict__ pairI1, int* __restrict__ cursor, int2* __restrict__ items) {
  pair_walk(Ed, ptStart, nL, [&](int a, int b, int i1, int i2) { items[atomicAdd(&cursor[sky_bucket(rowStart, pairI1, i1, i2)], 1)] = make_int2(a, b); });
}

// One workgroup per bucket: schur_block's sum into the block's place in the envelope, transposed when the order puts i1 after i2.
__global__ __launch_bounds__(64 * kSchurWaves) void k_sky_schur_pairs(const int* __restrict__ start, const int2* __restrict__ items, int nBuckets,
                                                                      const int* __restrict__ pairI1, const int* __restrict__ pairI2,
                                                                      const long long* __restrict__ pairDst, const R* __restrict__ BD,
                                                                      const R* __restrict__ Hpl, const R* __restrict__ Hpp, R lambda,
                                                                      R* __restrict__ env) {
  const int bkt = blockIdx.x;
  if (bkt >= nBuckets) return;
  const int i1 = pairI1[bkt], i2 = pairI2[bkt];
  // contrib = 1.0: the dense path's of a single rank
  schur_block(items, start[bkt], start[bkt + 1], i1, i2, BD, Hpl, Hpp, lambda, 1.0, [&](int q, int r, R v) {
    const long long d = pairDst[bkt];
    env[36 * (size_t)(d >> 1) + ((d & 1) ? r * 6 + q : q * 6 + r)] = v;
  });
}

constexpr int kSkyThreads = 1024;
constexpr int kSkyPanelLds = 128;   // a column whose list has at most this many rows keeps its solved panel in LDS (36.9 KB)

// A, bw and x are read and written by different threads across the barriers: no __restrict__ on them.  bs is the right-hand side by
// free pose, bw [12 nF] the work area: b by position, then the reciprocal pivots.  x goes out by free pose.
__global__ __launch_bounds__(kSkyThreads) void k_sky_solve(int nF, const int* __restrict__ first, const long long* __restrict__ rowOff,
                                                           const long long* __restrict__ colStart, const int* __restrict__ colRows,
                                                           const long long* __restrict__ colBlk, const int* __restrict__ perm,
                                                           const R* __restrict__ bs, R* A, R* bw, R* x, int* status) {
  __shared__ R pan[6 * (6 * kSkyPanelLds + 1)];
  const int tid = threadIdx.x;
  R* dinv = bw + 6 * (size_t)nF;
  for (int t = tid; t < 6 * nF; t += kSkyThreads) bw[t] = bs[6 * (size_t)perm[t / 6] + t % 6];
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < nF; j++) {
    R l[21], inv[6];
    R* D = A + 36 * (size_t)(rowOff[j + 1] - 1);   // the diagonal block ends its row
    const long long cs = colStart[j];
    const int m = (int)(colStart[j + 1] - cs), nPanel = 6 * m + 1;
    const bool inLds = m <= kSkyPanelLds;
    if (!sky::factorBlock<6>(D, l, inv)) bad = true;
    // the panel: row t % 6 of the block of the list's row t / 6, and b_j as the last row
    for (int t = tid; t < nPanel; t += kSkyThreads) {
      R* row = t < 6 * m ? A + 36 * (size_t)colBlk[cs + t / 6] + 6 * (t % 6) : bw + 6 * (size_t)j;
      R v[6];
#pragma unroll
      for (int c = 0; c < 6; c++) v[c] = row[c];
      sky::solveRow<6>(v, l, inv);
#pragma unroll
      for (int c = 0; c < 6; c++) row[c] = v[c];
      if (inLds) {
#pragma unroll
        for (int c = 0; c < 6; c++) pan[6 * t + c] = v[c];
      }
    }
    __syncthreads();   // the panel and y_j are written, and every thread has read D
    if (tid == 0) sky::storeFactor<6>(D, dinv, j, l, inv);
    // the rank-6 update: block (i, k) -= L_ij L_kj^T for every pair k <= i of the list, and b_i -= L_ij y_j.  Item w:
    //   w < 36 pairs: entry e = w % 36 of block (i, k) for the pair p = w / 36 = ia (ia + 1) / 2 + ik of list members
    //   else:         b_i[r] for the list member (w - 36 pairs) / 6
    const long long pairs = (long long)m * (m + 1) / 2, items = 36 * pairs + 6 * (long long)m;
    for (long long w = tid; w < items; w += kSkyThreads) {
      int ra, rb;   // panel rows of the two operands
      R* dst;
      if (w < 36 * pairs) {
        const long long p = w / 36;
        const int e = (int)(w - 36 * p), r = e / 6, c = e - 6 * r;
        const int ia = sky::triRow(p);
        const int ik = (int)(p - (long long)ia * (ia + 1) / 2);
        ra = 6 * ia + r; rb = 6 * ik + c;
        dst = A + 36 * (size_t)(colBlk[cs + ia] - j + colRows[cs + ik]) + e;   // block (i, k) lies k - j blocks after block (i, j)
      } else {
        const int t = (int)(w - 36 * pairs), ia = t / 6, r = t - 6 * ia;
        ra = 6 * ia + r; rb = 6 * m;
        dst = bw + 6 * (size_t)colRows[cs + ia] + r;
      }
      const R* a;
      const R* b;
      if (inLds) {
        a = pan + 6 * ra; b = pan + 6 * rb;
      } else {
        a = A + 36 * (size_t)colBlk[cs + ra / 6] + 6 * (ra % 6);
        b = rb < 6 * m ? A + 36 * (size_t)colBlk[cs + rb / 6] + 6 * (rb % 6) : bw + 6 * (size_t)j;
      }
      R s = *dst;
#pragma unroll
      for (int q = 0; q < 6; q++) s -= a[q] * b[q];
      *dst = s;
    }
    __syncthreads();   // column j + 1 and b_{j+1} are final, and pan is free
  }
  // L^T x = y, the rows downwards: x_i from the diagonal block, then y_j -= L_ij^T x_i along the row
  for (int i = nF - 1; i >= 0; i--) {
    const int f0 = first[i];
    const R* rowp = A + 36 * (size_t)rowOff[i];
    const R* D = rowp + 36 * (size_t)(i - f0);
    const int items = 6 * (i - f0);
    R xv[6];
    sky::solveDiagBack<6>(D, dinv, bw, i, xv);
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < 6; c++) x[6 * (size_t)perm[i] + c] = xv[c];
    }
    for (int t = tid; t < items; t += kSkyThreads) {
      const int jb = t / 6, c = t - 6 * jb;
      const R* B = rowp + 36 * (size_t)jb;
      R s = bw[6 * (size_t)f0 + t];
#pragma unroll
      for (int r = 0; r < 6; r++) s -= B[6 * r + c] * xv[r];
      bw[6 * (size_t)f0 + t] = s;
    }
    __syncthreads();   // y_{i-1} is final
  }
  if (bad && tid == 0) status[0] = 1;
}

}  // namespace ba
}  // namespace ydorb
