// gfx950 HIP kernels of Tracking::searchLocalPoints' geometry: Frame::isInCameraFrustum with MapPoint::predictScaleLevel (ORB-SLAM2
// Frame::isInFrustum / MapPoint::PredictScale, which YDORBSLAM renames), in fp32 under the written-order contract
// of DESIGN.md section 2 ("isInCameraFrustum"): +, -, *, / and sqrt only, every op a single IEEE operation (-ffp-contract=off), so the
// kernels equal the CPU restatement tests/frustum_ref/frustum_ref.cpp bit for bit.  The predicted level needs no log on the device: the
// view carries the nLevels - 1 ratio thresholds the host found with the reference's own log, and the level is the number of thresholds
// strictly below maxDistance / dist.
// Layout: one lane per list entry.  k_frustum_cull runs over the concatenated point lists of all views; a lane finds its view by a
// binary search of the CSR starts (wave-uniform loads except in the waves that straddle two views).  k_frustum_queries is the one-view
// form over the points 0 .. n-1 that also writes the projection search's query rows, so that they never exist on the host.  Both
// share frustum_test.  The map-point table is two float4 arrays and one float array, read through the list's point index.  No LDS.
// Two translation units include this header (frustum.hip launches the first kernel, orb_matcher.hip the second): the kernels are static.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ydorb/c_api.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace frustum {

constexpr int kThreads = 256;

typedef YdFrustumView ViewDev;   // plain floats and ints: the ABI struct travels as it is

struct Args {
  int nViews, nEntries;
  const int* start;            // [nViews + 1]
  const ViewDev* views;
  const float4* posMin;        // [nPoints] (P, minDistInv)
  const float4* normalMax;     // [nPoints] (Pn, maxDistInv)
  const float* maxDistance;    // [nPoints]
  const int* pointIdx;         // [nEntries]
  const uint8_t* skip;         // [nEntries]
  YdTrackView* rows;           // [nEntries]
  uint8_t* status;             // [nEntries]
};

// row r of Rcw times P plus tcw[r]: products exact in double, the four terms summed in double in ascending index, rounded once
__device__ __forceinline__ float row_rt(const ViewDev& V, int r, float x, float y, float z) {
  return (float)((((double)V.Rcw[3 * r] * (double)x + (double)V.Rcw[3 * r + 1] * (double)y) + (double)V.Rcw[3 * r + 2] * (double)z) + (double)V.tcw[r]);
}

// Frame::isInCameraFrustum for one map point: the exit code, and the track fields when it is 0 (all zero otherwise)
__device__ __forceinline__ int frustum_test(const ViewDev& V, float4 a, float4 b, float maxDistance, bool skip, YdTrackView& T) {
  T.u = 0.f; T.v = 0.f; T.ur = 0.f; T.view_cos = 0.f; T.level = 0;
  if (skip) return YDORB_FRUSTUM_SKIPPED;
  const float PcX = row_rt(V, 0, a.x, a.y, a.z), PcY = row_rt(V, 1, a.x, a.y, a.z), PcZ = row_rt(V, 2, a.x, a.y, a.z);
  if (PcZ < 0.0f) return YDORB_FRUSTUM_BEHIND;
  const float invz = 1.0f / PcZ;
  const float u = V.fx * PcX * invz + V.cx;
  const float v = V.fy * PcY * invz + V.cy;
  if (u < V.min_x || u > V.max_x) return YDORB_FRUSTUM_OUT_U;
  if (v < V.min_y || v > V.max_y) return YDORB_FRUSTUM_OUT_V;
  const float POx = a.x - V.Ow[0], POy = a.y - V.Ow[1], POz = a.z - V.Ow[2];
  const float dist = (float)sqrt(((double)POx * (double)POx + (double)POy * (double)POy) + (double)POz * (double)POz);
  if (dist < a.w || dist > b.w) return YDORB_FRUSTUM_DISTANCE;
  const float viewCos = (float)((((double)POx * (double)b.x + (double)POy * (double)b.y) + (double)POz * (double)b.z) / (double)dist);
  if (viewCos < V.viewing_cos_limit) return YDORB_FRUSTUM_VIEW_ANGLE;
  const float ratio = maxDistance / dist;
  int level = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) level += (k < V.n_levels - 1 && V.level_ratio[k] < ratio) ? 1 : 0;
  T.u = u; T.v = v; T.ur = u - V.bf * invz; T.view_cos = viewCos; T.level = level;
  return YDORB_FRUSTUM_IN_VIEW;
}

static __global__ __launch_bounds__(kThreads) void k_frustum_cull(Args g) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= g.nEntries) return;
  // the view whose range holds e: the last f with start[f] <= e (empty views share a start and are skipped by "last")
  int lo = 0, hi = g.nViews - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (g.start[mid] <= e) lo = mid; else hi = mid - 1;
  }
  const ViewDev& V = g.views[lo];
  const int p = g.pointIdx[e];
  YdTrackView T;
  const int code = frustum_test(V, g.posMin[p], g.normalMax[p], g.maxDistance[p], g.skip[e] != 0, T);
  g.rows[e] = T;
  g.status[e] = (uint8_t)code;
}

// The query row of searchByProjectionInFrameAndMapPoint (orbMatcher.cpp:28-38) for one tested point where k_gather_projection reads it
// (QueryT = match_kernels' QueryDev): all zero, flags 0, unless the point is in view.
template <class QueryT>
__device__ __forceinline__ QueryT query_of(const ViewDev& V, const YdTrackView& T, int code, float th, bool hasObs) {
  QueryT Q;
  Q.u = 0.f; Q.v = 0.f; Q.r = 0.f; Q.minLevel = 0; Q.maxLevel = 0; Q.ur = 0.f; Q.rs = 0.f; Q.angle = 0.f; Q.level = 0; Q.flags = 0;
  if (code == YDORB_FRUSTUM_IN_VIEW) {
    const float radius = th * ((double)T.view_cos > 0.998 ? 2.5f : 4.0f);   // getRadiusByViewCos, orbMatcher.cpp:820-826
    float sf = V.scale_factors[0];
#pragma unroll
    for (int k = 1; k < 8; k++) sf = T.level == k ? V.scale_factors[k] : sf;
    Q.u = T.u; Q.v = T.v; Q.r = radius * sf;
    Q.minLevel = T.level - 1; Q.maxLevel = T.level;
    Q.ur = T.ur; Q.rs = Q.r; Q.level = T.level;
    Q.flags = 1 | (hasObs ? 2 : 0);
  }
  return Q;
}

// One view over the points 0 .. n-1: the track rows and status bytes of k_frustum_cull plus the query rows of the projection search.
template <class QueryT>
static __global__ __launch_bounds__(kThreads) void k_frustum_queries(ViewDev V, int n, const float4* __restrict__ posMin, const float4* __restrict__ normalMax,
                                                              const float* __restrict__ maxDistance, const uint8_t* __restrict__ skip,
                                                              const uint8_t* __restrict__ hasObs, float th, QueryT* __restrict__ queries,
                                                              YdTrackView* __restrict__ rows, uint8_t* __restrict__ status) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  YdTrackView T;
  const int code = frustum_test(V, posMin[i], normalMax[i], maxDistance[i], skip[i] != 0, T);
  queries[i] = query_of<QueryT>(V, T, code, th, hasObs[i] != 0);
  rows[i] = T;
  status[i] = (uint8_t)code;
}

}  // namespace frustum
}  // namespace ydorb
