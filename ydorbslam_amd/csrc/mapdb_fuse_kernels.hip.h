// gfx950 HIP kernel of the batched fuse search on the resident map table (include/ydorb/c_api.h, "Resident keyframe features"; DESIGN.md
// section 2 "Fuse search on the resident table", section 6r): pass 1 of OrbMatcher::fuseByProjection / fuseBySim3 for every (target
// keyframe, listed point) of a call, in fp32 under the written-order contract of DESIGN.md section 2: +, -, *, / and sqrt only, every op
// a single IEEE operation (fp contract off), so the kernel equals the CPU restatement tests/fuse_ref/fuse_ref.cpp bit for bit.
// fuse_test is a sibling of frustum::frustum_test, not a caller of it: the adapter divides by zc where the frustum test multiplies by
// 1 / zc, the image test is half open, and the predicates are one conjunction of positive comparisons, so a NaN is rejected where the
// frustum test lets it pass every exit.  The two share row_rt and the level count over the view's ratio table.
// Layout: one lane per list entry, no LDS.  A lane finds its target by a binary search of the CSR starts (wave-uniform loads except in
// the waves that straddle two targets), loads its slot's resident record through eight gathers (mapdb_frustum_kernels.hip.h says what
// they cost), walks the point's observation span when the target asks for isInKeyFrame, and writes one query row, one status byte
// and the point's 32-byte descriptor (two uint4) where k_gather_projection reads them: the rows of all targets lie in list order, and call t
// points at row start[t].  Bound by those gathers and by launch latency, not by arithmetic.
// Slots were validated on the host against n_points, keyframe slots against n_keyframes; every per-slot array covers the point
// table's capacity; an observation span lies inside the pool (the table's own invariant).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frustum_kernels.hip.h"
#include "mapdb_attr_host.h"
#include "mapdb_resident_points.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace fuse {

constexpr int kThreads = 256;

typedef YdFuseTarget TargetDev;   // plain floats and ints: the ABI struct travels as it is

// Pass 1 for one point against one target: true when every predicate holds; the query fields either way
struct FuseRow { float u, v, ur, r; int level; };
__device__ __forceinline__ bool fuse_test(const TargetDev& G, float x, float y, float z, float nx, float ny, float nz, float minDistance, float maxDistance,
                                          FuseRow& Q) {
  const frustum::ViewDev& V = G.view;
  const float xc = frustum::row_rt(V, 0, x, y, z), yc = frustum::row_rt(V, 1, x, y, z), zc = frustum::row_rt(V, 2, x, y, z);
  const float u = V.fx * xc / zc + V.cx;
  const float v = V.fy * yc / zc + V.cy;
  const float ur = u - V.bf / zc;
  const float POx = x - V.Ow[0], POy = y - V.Ow[1], POz = z - V.Ow[2];
  const float dist = (float)sqrt(((double)POx * (double)POx + (double)POy * (double)POy) + (double)POz * (double)POz);
  const float ratio = maxDistance / dist;
  int level = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) level += (k < V.n_levels - 1 && V.level_ratio[k] < ratio) ? 1 : 0;
  float sf = V.scale_factors[0];
#pragma unroll
  for (int k = 1; k < 8; k++) sf = level == k ? V.scale_factors[k] : sf;
  const bool inImage = u >= V.min_x && u < V.max_x && v >= V.min_y && v < V.max_y;
  const double dot = ((double)POx * (double)nx + (double)POy * (double)ny) + (double)POz * (double)nz;
  Q.u = u; Q.v = v; Q.ur = ur; Q.level = level; Q.r = G.th * sf;
  return zc >= 0.0f && inImage && dist >= 0.8f * minDistance && dist <= 1.2f * maxDistance && dot >= 0.5 * (double)dist;
}

struct QueryArgs {
  int nTargets, nEntries;
  const int* start;            // [nTargets + 1]
  const TargetDev* targets;    // [nTargets]
  const int* slots;            // [nEntries]
  const uint8_t* skip;         // [nEntries]
  mapdb::ResidentPoints R;
  const int* obsKf;            // the observation pool
  uint4* qdesc;                // [nEntries][2]
  uint8_t* status;             // [nEntries]
};

template <class QueryT>
static __global__ __launch_bounds__(kThreads) void k_mapdb_fuse_queries(QueryArgs g, QueryT* __restrict__ queries /* [nEntries] */) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= g.nEntries) return;
  int lo = 0, hi = g.nTargets - 1;   // the last target t with start[t] <= e, as k_frustum_cull finds its view
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (g.start[mid] <= e) lo = mid; else hi = mid - 1;
  }
  const TargetDev& G = g.targets[lo];
  const size_t at = (size_t)e;
  const int slot = g.slots[e];
  const mapdb::ResidentPoints& R = g.R;
  QueryT Q;
  Q.u = 0.f; Q.v = 0.f; Q.r = 0.f; Q.minLevel = 0; Q.maxLevel = 0; Q.ur = 0.f; Q.rs = 0.f; Q.angle = 0.f; Q.level = 0; Q.flags = 0;
  int st;
  if (g.skip[e]) st = YDORB_FUSE_SKIPPED;
  else if (R.bad[slot]) st = YDORB_FUSE_BAD;
  else {
    bool observed = false;
    if (G.flags & YDORB_FUSE_SKIP_OBSERVED)
      for (int o = R.obsStart[slot], end = R.obsEnd[slot]; o < end; o++) observed = observed || g.obsKf[o] == G.kf_slot;
    const unsigned need = mapdb::kAttrGeometry | mapdb::kAttrDescriptor;
    if (observed) st = YDORB_FUSE_OBSERVED;
    else if ((R.flags[slot] & need) != need) st = YDORB_FUSE_NO_ATTRIBUTES;
    else {
      FuseRow F;
      const bool ok = fuse_test(G, R.pos[3 * slot], R.pos[3 * slot + 1], R.pos[3 * slot + 2], R.normal[3 * slot], R.normal[3 * slot + 1],
                                R.normal[3 * slot + 2], R.minDistance[slot], R.maxDistance[slot], F);
      st = ok ? YDORB_FUSE_SEARCHED : YDORB_FUSE_REJECTED;
      if (ok) { Q.u = F.u; Q.v = F.v; Q.ur = F.ur; Q.level = F.level; Q.minLevel = -1; Q.maxLevel = -1; Q.r = F.r; Q.flags = 1; }
    }
  }
  const uint4* d = reinterpret_cast<const uint4*>(R.desc);
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  g.qdesc[2 * at] = st == YDORB_FUSE_SEARCHED ? d[2 * (size_t)slot] : zero;
  g.qdesc[2 * at + 1] = st == YDORB_FUSE_SEARCHED ? d[2 * (size_t)slot + 1] : zero;
  queries[at] = Q;
  g.status[e] = (uint8_t)st;
}

}  // namespace fuse
}  // namespace ydorb
