// gfx950 HIP kernels of the local-BA graph query on the resident table (include/ydorb/c_api.h, "Local BA graph"; DESIGN.md section 2
// "Local BA graph on the resident table: the integer contract", section 6u).  They follow the unchanged k_rowset_mark / _count / _emit
// of mapdb_rows_kernels.hip.h, whose result (the local points in order, and their count) stays on the device.
//   k_lba_rank     one lane per keyframe of the call: poseOf[kf_slots[i]] = i.  The host refused a repeated slot, so no two lanes store
//                  to one address.
//   k_lba_mark     one lane per local point walks the point's view span (the shape of k_normal_depth).  It counts the usable views,
//                  gathers the status bits and, for every view of a usable keyframe that is not local (poseOf < 0), whatever the view's
//                  idx, takes a 64-bit integer atomicMin(&first[kf], rank << 16 | view position): an integer min does not depend on
//                  the order the atomics land in.
//                  A span holds at most 65 535 views (mapdb_desc_host.h), so the key orders by (rank, position).
//   k_lba_count    per point the number of "wins", the views of usable keyframes whose key equals first[kf]: each fixed keyframe wins exactly once, at its
//                  first occurrence in the walk.  Per workgroup the totals of edges and of wins.
//   k_lba_scan     each workgroup takes its two bases from the totals before it (as k_rowset_emit does) and writes the exclusive
//                  offsets of its points by a wave prefix sum and the wave totals: no arrival-order cursor anywhere.  Workgroup 0
//                  writes the three counts the host reads back.
//   k_lba_fixed    the winners write pose_kf / pose_fixed at n_local + offset and poseOf[kf] = n_local + offset; lanes below n_local
//                  write the local part of the two arrays.  A winner is the only lane that stores to its keyframe's entries.
//   k_lba_edges    one lane per point writes its edges at its offset, in span order, reading the view pool, both arrays of the feature
//                  pool and the position through the resident span offsets; also points, point_slot, point_status, edge_kf, edge_idx.
//   k_lba_reset    one lane per keyframe slot of the table: poseOf = -1, first = its maximum.
// Invariant: between calls poseOf is -1 and first is UINT64_MAX for every keyframe slot, as `first` of the rows header is INT32_MAX.
// The driver launches k_lba_reset at the end of every call that launched k_lba_rank; a call that failed in between leaves a flag that
// makes the next call fill both tables before it starts.
// The mark, count and scan kernels are launched over the host's bound of the point count (the kept entries cannot outnumber the row
// entries or the points); a lane at or past the device-side count contributes nothing.  Every index is validated by the host when it
// was staged (a row entry and a view's keyframe are below the table's counts, an octave is 0..7) or checked here against the device's
// span lengths before it is used: a view whose keyframe has no features, or whose idx is not below their length, reads nothing.
// Plain vector stores, no LDS beyond the wave totals, no inline assembly, no device-side assert / printf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapdb_lba_host.h"

namespace ydorb {
namespace mapdb {

constexpr int kLbaThreads = 256;
constexpr int kLbaWaves = kLbaThreads / 64;
constexpr unsigned long long kLbaNoFirst = ~0ull;

struct LbaArgs {
  int nLocal, nKfAll, bound, nBlocks;   // bound: the most points the call can have; nBlocks = ceil(bound / kLbaThreads)
  int nViewHdr, nFeatHdr;
  const float* invLevelSigma2; // [8]
  const int* kfSlots;          // [nLocal]
  const int* nPoints;          // [1] device-side count: k_rowset_emit's total
  const int* pointSlot;        // [bound] k_rowset_emit's result
  const int *viewStart, *viewLen, *viewPool;     // the handle's tables
  const int *featStart, *featLen;
  const YdKeyPoint* kps;
  const float* rightX;
  const float* pos;
  int* poseOf;                 // [>= nKfAll] -1 between calls
  unsigned long long* first;   // [>= nKfAll] kLbaNoFirst between calls
  // scratch, per point
  uint8_t* status;
  int *edgeCount, *winCount, *edgeOff, *winOff;
  int *blockEdge, *blockWin;   // [nBlocks]
  int* counts;                 // [4] n_points, n_edges, n_fixed
  // the result area
  uint8_t* outPoseFixed;
  int *outPoseKf, *outPointSlot, *outEdgePose, *outEdgePoint, *outEdgeKf, *outEdgeIdx;
  uint8_t* outStatus;
  double *outPoints, *outMeas, *outInfo;
};

struct LbaSpan { int at, m; };

__device__ inline LbaSpan lbaViews(const LbaArgs& g, int slot) {
  LbaSpan s{0, 0};
  if (slot < g.nViewHdr) { s.at = g.viewStart[slot]; s.m = g.viewLen[slot] >> 1; }
  return s;
}
// The feature length of a keyframe; 0: no feature span, the keyframe is unusable (isBad())
__device__ inline int lbaFeatLen(const LbaArgs& g, int kf) {
  return (unsigned)kf < (unsigned)g.nKfAll && kf < g.nFeatHdr ? g.featLen[kf] : 0;
}
// Whether a view is usable, else the status bit
__device__ inline bool lbaUsable(const LbaArgs& g, int kf, int idx, unsigned& status) {
  const int flen = lbaFeatLen(g, kf);
  if (flen <= 0) { status |= YDORB_LBA_POINT_SKIPPED_VIEWS; return false; }
  if ((unsigned)idx >= (unsigned)flen) { status |= YDORB_LBA_POINT_VIEW_OUT_OF_RANGE; return false; }
  return true;
}
__device__ inline unsigned long long lbaKey(int rank, int j) { return ((unsigned long long)(unsigned)rank << 16) | (unsigned)j; }

static __global__ __launch_bounds__(kLbaThreads) void k_lba_rank(LbaArgs g) {
  const int i = blockIdx.x * kLbaThreads + threadIdx.x;
  if (i < g.nLocal) g.poseOf[g.kfSlots[i]] = i;
}

static __global__ __launch_bounds__(kLbaThreads) void k_lba_mark(LbaArgs g) {
  const int p = blockIdx.x * kLbaThreads + threadIdx.x;
  if (p >= g.bound || p >= *g.nPoints) return;
  const LbaSpan s = lbaViews(g, g.pointSlot[p]);
  unsigned status = 0;
  int edges = 0;
  for (int j = 0; j < s.m; j++) {
    const int kf = g.viewPool[s.at + 2 * j], idx = g.viewPool[s.at + 2 * j + 1];
    if (lbaFeatLen(g, kf) > 0 && g.poseOf[kf] < 0) atomicMin(&g.first[kf], lbaKey(p, j));   // an occurrence, whatever its idx
    if (!lbaUsable(g, kf, idx, status)) continue;
    edges++;
  }
  if (edges == 0) status |= YDORB_LBA_POINT_NO_EDGES;
  g.status[p] = (uint8_t)status;
  g.edgeCount[p] = edges;
}

static __global__ __launch_bounds__(kLbaThreads) void k_lba_count(LbaArgs g) {
  __shared__ int waveEdge[kLbaWaves], waveWin[kLbaWaves];
  const int p = blockIdx.x * kLbaThreads + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int edges = 0, wins = 0;
  if (p < g.bound && p < *g.nPoints) {
    edges = g.edgeCount[p];
    const LbaSpan s = lbaViews(g, g.pointSlot[p]);
    for (int j = 0; j < s.m; j++) {
      const int kf = g.viewPool[s.at + 2 * j];
      if (lbaFeatLen(g, kf) > 0 && g.first[kf] == lbaKey(p, j)) wins++;
    }
    g.winCount[p] = wins;
  }
  for (int d = 32; d > 0; d >>= 1) { edges += __shfl_xor(edges, d); wins += __shfl_xor(wins, d); }
  if (lane == 0) { waveEdge[wave] = edges; waveWin[wave] = wins; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int e = 0, w = 0;
    for (int v = 0; v < kLbaWaves; v++) { e += waveEdge[v]; w += waveWin[v]; }
    g.blockEdge[blockIdx.x] = e; g.blockWin[blockIdx.x] = w;
  }
}

static __global__ __launch_bounds__(kLbaThreads) void k_lba_scan(LbaArgs g) {
  __shared__ int part[4][kLbaWaves], waveEdge[kLbaWaves], waveWin[kLbaWaves];
  const int tid = threadIdx.x, p = blockIdx.x * kLbaThreads + tid, lane = tid & 63, wave = tid >> 6;
  int beforeE = 0, allE = 0, beforeW = 0, allW = 0;
  for (int b = tid; b < g.nBlocks; b += kLbaThreads) {
    const int e = g.blockEdge[b], w = g.blockWin[b];
    allE += e; allW += w;
    if (b < (int)blockIdx.x) { beforeE += e; beforeW += w; }
  }
  for (int d = 32; d > 0; d >>= 1) {
    beforeE += __shfl_xor(beforeE, d); allE += __shfl_xor(allE, d); beforeW += __shfl_xor(beforeW, d); allW += __shfl_xor(allW, d);
  }
  const bool live = p < g.bound && p < *g.nPoints;
  const int myE = live ? g.edgeCount[p] : 0, myW = live ? g.winCount[p] : 0;
  int incE = myE, incW = myW;   // inclusive prefix sums over the wave
  for (int d = 1; d < 64; d <<= 1) {
    const int e = __shfl_up(incE, d), w = __shfl_up(incW, d);
    if (lane >= d) { incE += e; incW += w; }
  }
  if (lane == 0) { part[0][wave] = beforeE; part[1][wave] = allE; part[2][wave] = beforeW; part[3][wave] = allW; }
  if (lane == 63) { waveEdge[wave] = incE; waveWin[wave] = incW; }
  __syncthreads();
  int baseE = 0, totalE = 0, baseW = 0, totalW = 0;
  for (int v = 0; v < kLbaWaves; v++) {
    baseE += part[0][v]; totalE += part[1][v]; baseW += part[2][v]; totalW += part[3][v];
    if (v < wave) { baseE += waveEdge[v]; baseW += waveWin[v]; }
  }
  if (blockIdx.x == 0 && tid == 0) { g.counts[0] = *g.nPoints; g.counts[1] = totalE; g.counts[2] = totalW; g.counts[3] = 0; }
  if (!live) return;
  g.edgeOff[p] = baseE + incE - myE;
  g.winOff[p] = baseW + incW - myW;
}

static __global__ __launch_bounds__(kLbaThreads) void k_lba_fixed(LbaArgs g) {
  const int p = blockIdx.x * kLbaThreads + threadIdx.x;
  if (p < g.nLocal) { g.outPoseKf[p] = g.kfSlots[p]; g.outPoseFixed[p] = 0; }
  if (p >= g.bound || p >= *g.nPoints) return;
  if (g.winCount[p] == 0) return;
  const LbaSpan s = lbaViews(g, g.pointSlot[p]);
  int at = g.nLocal + g.winOff[p];
  for (int j = 0; j < s.m; j++) {
    const int kf = g.viewPool[s.at + 2 * j];
    if (lbaFeatLen(g, kf) <= 0 || g.first[kf] != lbaKey(p, j)) continue;
    g.outPoseKf[at] = kf; g.outPoseFixed[at] = 1;
    g.poseOf[kf] = at;
    at++;
  }
}

static __global__ __launch_bounds__(kLbaThreads) void k_lba_edges(LbaArgs g) {
  const int p = blockIdx.x * kLbaThreads + threadIdx.x;
  if (p >= g.bound || p >= *g.nPoints) return;
  const int slot = g.pointSlot[p];
  g.outPointSlot[p] = slot;
  g.outStatus[p] = g.status[p];
  for (int d = 0; d < 3; d++) g.outPoints[3 * (size_t)p + d] = (double)g.pos[3 * (size_t)slot + d];
  const LbaSpan s = lbaViews(g, slot);
  unsigned ignored = 0;
  size_t e = (size_t)g.edgeOff[p];
  for (int j = 0; j < s.m; j++) {
    const int kf = g.viewPool[s.at + 2 * j], idx = g.viewPool[s.at + 2 * j + 1];
    if (!lbaUsable(g, kf, idx, ignored)) continue;
    const size_t f = (size_t)g.featStart[kf] + (size_t)idx;
    const YdKeyPoint kp = g.kps[f];
    const float ur = g.rightX[f];
    g.outEdgePose[e] = g.poseOf[kf]; g.outEdgePoint[e] = p;
    g.outMeas[3 * e] = (double)kp.x; g.outMeas[3 * e + 1] = (double)kp.y; g.outMeas[3 * e + 2] = ur < 0 ? -1.0 : (double)ur;
    g.outInfo[e] = (double)g.invLevelSigma2[kp.octave];   // 0..7: validated when the features were staged (mapdb_feat_host.h)
    g.outEdgeKf[e] = kf; g.outEdgeIdx[e] = idx;
    e++;
  }
}

static __global__ __launch_bounds__(kLbaThreads) void k_lba_reset(int nKfAll, int* poseOf, unsigned long long* first) {
  const int k = blockIdx.x * kLbaThreads + threadIdx.x;
  if (k >= nKfAll) return;
  poseOf[k] = -1;
  first[k] = kLbaNoFirst;
}

}  // namespace mapdb
}  // namespace ydorb
