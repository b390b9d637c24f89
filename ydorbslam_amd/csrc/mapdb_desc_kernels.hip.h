// gfx950 HIP kernel of the distinctive-descriptor query on the resident table's descriptor blocks and point views (include/ydorb/c_api.h,
// "Resident descriptors").  The blocks and the views themselves are kept by the span kernels of
// mapdb_span_kernels.hip.h.
//   k_mapdb_distinctive   MapPoint::computeDistinctiveDescriptors for the named point slots: one wave per point, four per workgroup, as
//                         k_distinctive (match_kernels.hip.h), whose bisection it runs.  Three passes over the point's views, 64 at
//                         a time, a lane per view:
//                           A  reads no descriptor: each view's block start and length; a view without a block is skipped, one with
//                              idx >= length flags the point (status 3) and the wave leaves.  Counts the collected rows, m.
//                           B  copies the first kStageRows collected rows to the wave's LDS, in collected order (ballot prefix), and
//                              notes the span position where the collected rows past them begin.
//                           C  the lane of collected row c holds that row and bisects its median: the count over the other rows
//                              reads the staged rows from LDS (wave-uniform addresses broadcast) and the rows past the staging
//                              limit through the indirection from global memory, view by view (wave-uniform, scalar loads).
//                         The winner is the wave-min of (median << 16 | collected row); the lane that holds it writes its span
//                         position, its view and its row.
// Every index is bounded by the host before the launch or checked here: a point slot is below n_points (the query's validation) and
// read against the view headers' capacity, a view's keyframe slot is below n_keyframes (validated when staged) and read against the
// block headers' capacity, its keypoint index is checked against the device's block length before any row is read.  Integers only.
// No inline assembly, no device-side assert / printf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapdb_desc_host.h"

namespace ydorb {
namespace mapdb {

constexpr int kDescThreads = 256;
constexpr int kDescWaves = kDescThreads / 64;
// Rows staged in LDS per wave: 128 x 32 B = 4 KiB, 16 KiB per workgroup.  A CU holds 32 waves = 8 such workgroups = 128 KiB of its
// 160 KiB: occupancy stays bound by the wave cap, not by LDS.
constexpr int kStageRows = 128;

struct DistinctiveArgs {
  int n, nViewHdr, nBlockHdr;
  const int* slots;        // [n] below n_points
  const uint8_t* bad;      // [pointCap]
  const int* viewStart;    // [nViewHdr] in int32 entries of viewPool
  const int* viewLen;      // [nViewHdr] 2 x the number of views
  const int* viewPool;
  const int* blockStart;   // [nBlockHdr] in descriptors
  const int* blockLen;     // [nBlockHdr]
  const uint4* blockPool;
  int* best;               // [n]
  int* bestView;           // [n][2]
  uint4* descOut;          // [n][2]
  uint8_t* status;         // [n]
};

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
         __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

static __global__ __launch_bounds__(kDescThreads) void k_mapdb_distinctive(DistinctiveArgs g) {
  __shared__ uint4 staged[kDescWaves][2 * kStageRows];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = blockIdx.x * kDescWaves + wave;
  if (q >= g.n) return;   // uniform over the wave; no workgroup barrier below
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  int st = -1;
  const int slot = g.slots[q];
  int vb = 0, nv = 0;
  if (g.bad[slot]) st = YDORB_MAPDESC_BAD;
  else if (slot < g.nViewHdr) { vb = g.viewStart[slot]; nv = g.viewLen[slot] >> 1; }
  // pass A: no descriptor is read before every view's index is known to lie inside its block
  int m = 0;
  if (st < 0) {
    bool outside = false;
    for (int v0 = 0; v0 < nv; v0 += 64) {
      const int v = v0 + lane;
      bool has = false;
      if (v < nv) {
        const int kf = g.viewPool[vb + 2 * v], idx = g.viewPool[vb + 2 * v + 1];
        const int len = kf < g.nBlockHdr ? g.blockLen[kf] : 0;
        has = len > 0;
        outside = outside || (has && idx >= len);
      }
      m += __popcll(__ballot(has));
    }
    if (__ballot(outside) != 0ull) st = YDORB_MAPDESC_VIEW_OUT_OF_RANGE;
    else if (m == 0) st = YDORB_MAPDESC_NO_DESCRIPTORS;
  }
  if (st >= 0) {
    if (lane == 0) { g.best[q] = -1; g.bestView[2 * q] = 0; g.bestView[2 * q + 1] = 0; g.status[q] = (uint8_t)st; }
    if (lane < 2) g.descOut[2 * (size_t)q + lane] = zero;
    return;
  }
  // pass B: the first kStageRows collected rows, in collected order
  uint4* S = staged[wave];
  int resume = nv;   // the span position of collected row kStageRows
  for (int v0 = 0, c0 = 0; v0 < nv && (c0 < kStageRows || (m > kStageRows && resume == nv)); v0 += 64) {
    const int v = v0 + lane;
    bool has = false;
    size_t row = 0;
    if (v < nv) {
      const int kf = g.viewPool[vb + 2 * v], idx = g.viewPool[vb + 2 * v + 1];
      has = kf < g.nBlockHdr && g.blockLen[kf] > 0;
      if (has) row = (size_t)g.blockStart[kf] + (size_t)idx;
    }
    const unsigned long long mask = __ballot(has);
    const int c = c0 + __popcll(mask & below);
    if (has && c < kStageRows) { S[2 * c] = g.blockPool[2 * row]; S[2 * c + 1] = g.blockPool[2 * row + 1]; }
    const unsigned long long first = __ballot(has && c == kStageRows);
    if (first != 0ull) resume = v0 + (__ffsll((long long)first) - 1);
    c0 += __popcll(mask);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // pass C
  const int inLds = min(m, kStageRows), kth = (int)(0.5 * m);
  unsigned win = 0xFFFFFFFFu;
  int winV = 0, winKf = 0, winIdx = 0;
  uint4 w0 = zero, w1 = zero;
  for (int v0 = 0, c0 = 0; v0 < nv; v0 += 64) {
    const int v = v0 + lane;
    bool has = false;
    int kf = 0, idx = 0;
    size_t row = 0;
    if (v < nv) {
      kf = g.viewPool[vb + 2 * v]; idx = g.viewPool[vb + 2 * v + 1];
      has = kf < g.nBlockHdr && g.blockLen[kf] > 0;
      if (has) row = (size_t)g.blockStart[kf] + (size_t)idx;
    }
    const unsigned long long mask = __ballot(has);
    if (has) {
      const int c = c0 + __popcll(mask & below);
      const uint4 a0 = g.blockPool[2 * row], a1 = g.blockPool[2 * row + 1];
      int lo = 0, hi = 256;   // smallest t with count(d <= t) > kth
      while (lo < hi) {
        const int t = (lo + hi) >> 1;
        int cnt = 0;
        for (int j = 0; j < inLds; j++) cnt += hamming256(a0, a1, S[2 * j], S[2 * j + 1]) <= t;
        for (int u = resume; u < nv; u++) {   // past the staging limit: through the indirection, wave-uniform
          const int kfu = g.viewPool[vb + 2 * u], len = kfu < g.nBlockHdr ? g.blockLen[kfu] : 0;
          if (len == 0) continue;
          const size_t r = (size_t)g.blockStart[kfu] + (size_t)g.viewPool[vb + 2 * u + 1];
          cnt += hamming256(a0, a1, g.blockPool[2 * r], g.blockPool[2 * r + 1]) <= t;
        }
        if (cnt > kth) hi = t; else lo = t + 1;
      }
      const unsigned key = ((unsigned)lo << 16) | (unsigned)c;   // c <= 65534: a span holds at most 65535 views
      if (key < win) { win = key; winV = v; winKf = kf; winIdx = idx; w0 = a0; w1 = a1; }
    }
    c0 += __popcll(mask);
  }
  unsigned least = win;
  for (int d = 32; d > 0; d >>= 1) least = min(least, (unsigned)__shfl_xor((int)least, d));
  if (win == least) {   // one lane: the collected row is part of the key
    g.best[q] = winV; g.bestView[2 * q] = winKf; g.bestView[2 * q + 1] = winIdx; g.status[q] = YDORB_MAPDESC_UPDATED;
    g.descOut[2 * (size_t)q] = w0; g.descOut[2 * (size_t)q + 1] = w1;
  }
}

}  // namespace mapdb
}  // namespace ydorb
