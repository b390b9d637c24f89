// gfx950 HIP kernels of Tracking::searchLocalPoints on the resident map table (include/ydorb/c_api.h, "Resident point attributes";
// DESIGN.md section 2 "Local map on the resident table", section 6q): frustum_kernels.hip.h's two kernels with the slot indirection.
// A lane loads its listed slot's resident record (mapdb_resident_points.h), forms the operands frustum::frustum_test takes and calls it
// unchanged, so a result equals the flat kernels' on a table gathered from the resident values bit for bit.
// Layout: one lane per list entry, no LDS.  A lane reads 4 bytes of slot, 1 of skip and, through the slot, 12 + 12 + 4 + 4 + 8 + 2
// bytes of the record (k_mapdb_local_queries: 32 more of descriptor, as two 16-byte loads); the loads through the slot are gathers from
// eight arrays (pos, bad, span start and end, normal, the two distances, flags; the descriptor is a ninth): a cache line per array and
// lane, ten when both 12-byte triples straddle one, one more for the descriptor.  Both kernels are bound by those gathers and by launch latency, not by arithmetic.
// Slots were validated on the host against n_points; every array covers the point table's capacity.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frustum_kernels.hip.h"
#include "mapdb_attr_host.h"
#include "mapdb_resident_points.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace frustum {

// The record of `slot` against view V.  need: the flag bits a listed point must carry (the geometry; the fused search: and the
// descriptor).  Effective skip = the caller's byte OR the resident bad flag (a slot never set reads as bad).  A point that is not
// skipped and lacks a needed flag is YDORB_FRUSTUM_NO_ATTRIBUTES with a zero track row.  0.8f * minDistance and 1.2f * maxDistance
// are one fp32 multiply each: the bits of getMinDistanceInvariance() / getMaxDistanceInvariance().
__device__ __forceinline__ int resident_test(const ViewDev& V, const mapdb::ResidentPoints& R, int slot, bool callerSkip, unsigned need, YdTrackView& T,
                                             bool& hasObs) {
  const bool skip = callerSkip || R.bad[slot] != 0;
  hasObs = R.obsEnd[slot] > R.obsStart[slot];
  if (!skip && (R.flags[slot] & need) != need) {
    T.u = 0.f; T.v = 0.f; T.ur = 0.f; T.view_cos = 0.f; T.level = 0;
    return YDORB_FRUSTUM_NO_ATTRIBUTES;
  }
  const float maxDistance = R.maxDistance[slot];
  const float4 a = make_float4(R.pos[3 * slot], R.pos[3 * slot + 1], R.pos[3 * slot + 2], 0.8f * R.minDistance[slot]);
  const float4 b = make_float4(R.normal[3 * slot], R.normal[3 * slot + 1], R.normal[3 * slot + 2], 1.2f * maxDistance);
  return frustum_test(V, a, b, maxDistance, skip, T);
}

struct ResidentCullArgs {
  int nViews, nEntries;
  const int* start;            // [nViews + 1]
  const ViewDev* views;
  const int* slots;            // [nEntries]
  const uint8_t* skip;         // [nEntries]
  YdTrackView* rows;           // [nEntries]
  uint8_t* status;             // [nEntries]
  mapdb::ResidentPoints R;
};

// k_frustum_cull over listed slots
static __global__ __launch_bounds__(kThreads) void k_mapdb_frustum_cull(ResidentCullArgs g) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= g.nEntries) return;
  int lo = 0, hi = g.nViews - 1;   // the last view f with start[f] <= e, as k_frustum_cull finds it
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (g.start[mid] <= e) lo = mid; else hi = mid - 1;
  }
  YdTrackView T;
  bool hasObs;
  const int code = resident_test(g.views[lo], g.R, g.slots[e], g.skip[e] != 0, mapdb::kAttrGeometry, T, hasObs);
  g.rows[e] = T;
  g.status[e] = (uint8_t)code;
}

// k_frustum_queries over listed slots; it also copies each listed point's descriptor to the matcher's query-descriptor area
template <class QueryT>
static __global__ __launch_bounds__(kThreads) void k_mapdb_local_queries(ViewDev V, int n, const int* __restrict__ slots, const uint8_t* __restrict__ skip,
                                                                         mapdb::ResidentPoints R, float th, QueryT* __restrict__ queries,
                                                                         uint4* __restrict__ qdesc, YdTrackView* __restrict__ rows,
                                                                         uint8_t* __restrict__ status) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int slot = slots[i];
  YdTrackView T;
  bool hasObs;
  const int code = resident_test(V, R, slot, skip[i] != 0, mapdb::kAttrGeometry | mapdb::kAttrDescriptor, T, hasObs);
  const uint4* d = reinterpret_cast<const uint4*>(R.desc);
  qdesc[2 * i] = d[2 * slot]; qdesc[2 * i + 1] = d[2 * slot + 1];
  queries[i] = frustum::query_of<QueryT>(V, T, code, th, hasObs);
  rows[i] = T;
  status[i] = (uint8_t)code;
}

}  // namespace frustum
}  // namespace ydorb
