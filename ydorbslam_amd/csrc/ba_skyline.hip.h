// gfx950 HIP kernels of the BA's block-skyline reduced camera solve: the Schur complement S stored as the
// envelope of 6x6 blocks that ba_pairs.h / skyline_plan.h lay out, factorised in place and solved, in fp64 with every entry summed in
// a fixed order.  The dense kernels of ba_kernels.hip.h are not touched; these take their place when the solver is SKYLINE.
//
// Buckets: one per covisible pair of free poses and one per free pose (ba_pairs.h, PairList), ordered by (i2, i1) like the dense
// path's triangular index, so that bucket q of row i2 is found by a binary search for i1 in pairI1[rowStart[i2] .. rowStart[i2 + 1]).
// Storage: row i (a position of the plan's order) holds the blocks of columns first[i] .. i, each [r][c] row-major, block (i, j) at
// 36 * (rowOff[i] + j - first[i]).  Of a diagonal block the lower triangle is read.
//
// k_sky_pair_count / k_sky_pair_fill   k_pair_count / k_pair_fill with the bucket looked up in the pair table (k_excl_scan and
//                     k_pair_sort are used as they are)
// k_sky_schur_pairs   b_schur_pairs' accumulation, item for item; only the destination differs: the block's place in the envelope,
//                     transposed when the order puts i1 after i2
// k_sky_solve         one workgroup of 1024 walks the block columns: every thread factorises the 6x6 diagonal block in registers, the
//                     rows of the column's panel and b, as one more row, are solved against it (and kept in LDS when the panel fits),
//                     barrier, the blocks of every pair of rows in the column's list take their rank-6 update, barrier.  Then the rows
//                     are walked downwards for the back substitution.  Every barrier is reached by every thread: the loop bounds are
//                     the plan's, and a non-positive pivot is replaced by 1 and reported in status[0] at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ba_kernels.hip.h"

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
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= nL) return;
  for (int a = ptStart[l]; a < ptStart[l + 1]; a++) {
    const int i1 = Ed.pidx[a];
    if (i1 < 0) continue;
    for (int b = a; b < ptStart[l + 1]; b++) {
      const int i2 = Ed.pidx[b];  // edges of a landmark are sorted by pose index: i2 >= i1
      if (i2 >= 0) atomicAdd(&cnt[sky_bucket(rowStart, pairI1, i1, i2)], 1);
    }
  }
}
__global__ __launch_bounds__(256) void k_sky_pair_fill(EdgeSoA Ed, const int* __restrict__ ptStart, int nL, const int* __restrict__ rowStart,
                                                       const int* __restrict__ pairI1, int* __restrict__ cursor, int2* __restrict__ items) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= nL) return;
  for (int a = ptStart[l]; a < ptStart[l + 1]; a++) {
    const int i1 = Ed.pidx[a];
    if (i1 < 0) continue;
    for (int b = a; b < ptStart[l + 1]; b++) {
      const int i2 = Ed.pidx[b];
      if (i2 >= 0) items[atomicAdd(&cursor[sky_bucket(rowStart, pairI1, i1, i2)], 1)] = make_int2(a, b);
    }
  }
}

// One workgroup per bucket.  The loop over the items, the split over the waves and the sum of the partials are b_schur_pairs' (see
// there for the operand layout): the two must give the same bits.
__global__ __launch_bounds__(64 * kSchurWaves) void k_sky_schur_pairs(const int* __restrict__ start, const int2* __restrict__ items, int nBuckets,
                                                                      const int* __restrict__ pairI1, const int* __restrict__ pairI2,
                                                                      const long long* __restrict__ pairDst, const R* __restrict__ BD,
                                                                      const R* __restrict__ Hpl, const R* __restrict__ Hpp, R lambda,
                                                                      R* __restrict__ env) {
  __shared__ R part[kSchurWaves][36];
  const int bkt = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (bkt >= nBuckets) return;
  const int i1 = pairI1[bkt], i2 = pairI2[bkt];
  const int i16 = lane & 15, kq = lane >> 4;
  const bool live = i16 < 6;
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  const int b0 = start[bkt], b1 = start[bkt + 1];
  const int per = (((b1 - b0) + kSchurWaves - 1) / kSchurWaves + 3) & ~3;
  const int s0 = min(b0 + wv * per, b1), s1 = min(s0 + per, b1);
  for (int base = s0; base < s1; base += 32) {
    R av[8][3], bv[8][3];
#pragma unroll
    for (int g = 0; g < 8; g++) {
      const int idx = base + 4 * g + kq;
      const bool on = live && idx < s1;
      const int2 it = on ? items[idx] : make_int2(0, 0);
      const R* pa = Hpl + (size_t)18 * it.y + i16 * 3;
      const R* pb = BD + (size_t)18 * it.x + i16 * 3;
#pragma unroll
      for (int c = 0; c < 3; c++) { av[g][c] = on ? pa[c] : 0.0; bv[g][c] = on ? pb[c] : 0.0; }
    }
#pragma unroll
    for (int g = 0; g < 8; g++)
      if (base + 4 * g < s1) {
#pragma unroll
        for (int c = 0; c < 3; c++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[g][c], bv[g][c], acc, 0, 0, 0);
      }
  }
  if (live) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int q = kq + 4 * reg;
      if (q < 6) part[wv][q * 6 + i16] = acc[reg];
    }
  }
  __syncthreads();
  if (threadIdx.x < 36) {
    const int q = threadIdx.x / 6, r = threadIdx.x - 6 * q;
    R v = 0;
#pragma unroll
    for (int w = 0; w < kSchurWaves; w++) v -= part[w][threadIdx.x];
    if (i1 == i2) v += 1.0 * (Hpp[(size_t)36 * i1 + q * 6 + r] + (q == r ? lambda : 0.0));   // the dense path's `contrib` of a single rank
    const long long d = pairDst[bkt];
    env[36 * (size_t)(d >> 1) + ((d & 1) ? r * 6 + q : q * 6 + r)] = v;
  }
}

__device__ __forceinline__ constexpr int tri6(int r, int c) { return r * (r + 1) / 2 + c; }

// L L^T of the lower triangle of D ([6][6]) into l (packed rows) and the reciprocals of its diagonal into inv; false when a pivot was
// not positive (it is then taken as 1).  Every division by a pivot is a product with inv, as in the essential graph's factor7.
__device__ __forceinline__ bool factor6(const R* D, R* l, R* inv) {
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c <= r; c++) {
      R s = D[6 * r + c];
#pragma unroll
      for (int q = 0; q < c; q++) s -= l[tri6(r, q)] * l[tri6(c, q)];
      if (c == r) {
        if (!(s > 0)) { ok = false; s = 1.0; }
        l[tri6(r, r)] = sqrt(s);
        inv[r] = 1.0 / l[tri6(r, r)];
      } else {
        l[tri6(r, c)] = s * inv[c];
      }
    }
  return ok;
}

// One row of a panel (or b_j) against the factor of the diagonal block: v L^T = row, in place
__device__ __forceinline__ void solveRow6(R* v, const R* l, const R* inv) {
#pragma unroll
  for (int c = 0; c < 6; c++) {
    R s = v[c];
#pragma unroll
    for (int q = 0; q < c; q++) s -= v[q] * l[tri6(c, q)];
    v[c] = s * inv[c];
  }
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
    if (!factor6(D, l, inv)) bad = true;
    // the panel: row t % 6 of the block of the list's row t / 6, and b_j as the last row
    for (int t = tid; t < nPanel; t += kSkyThreads) {
      R* row = t < 6 * m ? A + 36 * (size_t)colBlk[cs + t / 6] + 6 * (t % 6) : bw + 6 * (size_t)j;
      R v[6];
#pragma unroll
      for (int c = 0; c < 6; c++) v[c] = row[c];
      solveRow6(v, l, inv);
#pragma unroll
      for (int c = 0; c < 6; c++) row[c] = v[c];
      if (inLds) {
#pragma unroll
        for (int c = 0; c < 6; c++) pan[6 * t + c] = v[c];
      }
    }
    __syncthreads();   // the panel and y_j are written, and every thread has read D
    if (tid == 0) {
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c <= r; c++) D[6 * r + c] = l[tri6(r, c)];
#pragma unroll
      for (int c = 0; c < 6; c++) dinv[6 * (size_t)j + c] = inv[c];
    }
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
        int ia = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);   // the two loops make the rounded root exact
        while ((long long)ia * (ia + 1) / 2 > p) ia--;
        while ((long long)(ia + 1) * (ia + 2) / 2 <= p) ia++;
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
#pragma unroll
    for (int c = 5; c >= 0; c--) {
      R s = bw[6 * (size_t)i + c];
#pragma unroll
      for (int q = c + 1; q < 6; q++) s -= D[6 * q + c] * xv[q];
      xv[c] = s * dinv[6 * (size_t)i + c];
    }
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
