// gfx950 HIP kernels of ydorb_mapdb_create_new_points (orb_matcher.hip; DESIGN.md section 2 "createNewMapPoints on the resident table",
// section 6t): LocalMapping::createNewMapPoints for all neighbours of one keyframe on the resident map table.  The order-free part runs
// once over all neighbours, the order-dependent part is a chain of two small launches per neighbour on one stream:
//   k_mapdb_tri_join      one lane per (neighbour, entry of the first keyframe's BoW span): two binary searches over the second span's
//                         node ids give the bucket [begin, end) of the entry's node; an entry whose feature has a map point at call time
//                         (row entry >= 0), or fails stereo_only, or whose node the second span lacks, gets an empty range.  Queries are
//                         not compacted: query q of every neighbour is the first span's entry q, which is the order of the reference's
//                         merge-join.  This replaces the host merge-join of ydorb_search_for_triangulation.
//   k_mapdb_tri_gather    the body of k_gather_bow (match_kernels.hip.h) with blockIdx.y as the neighbour: one wave per query, Hamming
//                         distance and epipolar test of every bucket member, records appended to the neighbour's part of the pool.
//                         tri_pair_ok and hamming256 are the flat search's.  A query that does not fit sets the overflow word and
//                         keeps count 0; nothing is written past the pool.
//   k_resolve             unchanged (match_kernels.hip.h), mode 5, one launch per neighbour.
//   k_mapdb_tri_geometry  one lane per query of one neighbour: a matched query builds f1 / f2 / lv from the resident keypoints and
//                         right_x, the uploaded depths and the level tables, runs triangulate_match (triangulate_kernels.hip.h) and
//                         writes the three dense outputs at idx1.  An accepted match zeroes the record count of its query in every
//                         later neighbour's qInfo: the claim of idx1, which the next k_resolve sees as an empty query.
// All wave64, plain vector stores, no LDS; the one atomic is the pool head k_gather_bow also takes.  Every index is bounded by the
// host: a usable keyframe's row, block and depth have its feature count and its BoW feature indices lie below it (lockResidentTri).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.hip.h"
#include "triangulate_kernels.hip.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace mapdbtri {

constexpr int kThreads = 256;

struct Spans { int featStart, n, blockStart, rowStart, bowStart, bowLen; };   // == mapdb::ResidentTriSpans
struct Pools {
  const int* rowPool; const int2* bowPool; const KeyPointDev* kps; const float* rightX; const uint8_t* blockPool;
};
struct NbDev {             // one neighbour, in device memory
  Spans k2;
  int usable;              // 0: every query of this neighbour is empty
  int depthAt;             // where the second keyframe's depths begin in the uploaded depth array
  float ratioFactor;
  int pad;
  BowCallDev geom;         // F, the epipole and the second keyframe's level tables as tri_pair_ok reads them; the pointers stay null
  tri::ViewDev view;
};
struct FirstDev {          // the first keyframe, in device memory: the level tables are indexed by octave
  Spans k1;
  tri::ViewDev view;
  float sigma2[8], sf[8];
};
struct SearchArgs {
  Pools R;
  Spans k1;
  int nq, stereoOnly;      // nq == k1.bowLen
  const NbDev* nb;
  int2* qRange;            // [nNb][nq] into bowPool
  int* qFeat;              // [nq] the feature of the first keyframe behind query q, the same for every neighbour
  float* qAngle;           // [nq] its angle
  int2* qInfo;             // [nNb][nq]
  uint32_t* pool; unsigned* heads; unsigned poolPerNb; int* overflow;
};

static __global__ __launch_bounds__(kThreads) void k_mapdb_tri_join(SearchArgs g) {
  const int q = blockIdx.x * kThreads + threadIdx.x, nb = blockIdx.y;
  if (q >= g.nq) return;
  const int2 e = g.R.bowPool[g.k1.bowStart + q];   // (node, feature)
  const int i1 = e.y;
  if (nb == 0) { g.qFeat[q] = i1; g.qAngle[q] = g.R.kps[g.k1.featStart + i1].angle; }
  const NbDev& N = g.nb[nb];
  int2 range = make_int2(0, 0);
  if (N.usable && g.R.rowPool[g.k1.rowStart + i1] < 0 && (!g.stereoOnly || g.R.rightX[g.k1.featStart + i1] >= 0)) {
    const int2* B = g.R.bowPool + N.k2.bowStart;
    int lo = 0, hi = N.k2.bowLen;   // the first entry whose node is not below e.x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (B[mid].x < e.x) lo = mid + 1; else hi = mid;
    }
    const int begin = lo;
    hi = N.k2.bowLen;               // the first entry whose node is above e.x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (B[mid].x <= e.x) lo = mid + 1; else hi = mid;
    }
    range = make_int2(N.k2.bowStart + begin, N.k2.bowStart + lo);
  }
  g.qRange[(size_t)nb * g.nq + q] = range;
}

static __global__ __launch_bounds__(kThreads) void k_mapdb_tri_gather(SearchArgs g) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wv, nb = blockIdx.y;
  if (q >= g.nq) return;
  const size_t at = (size_t)nb * g.nq + q;
  const int2 rg = g.qRange[at];
  const int total = rg.y - rg.x;
  int2 info = make_int2(0, 0);
  if (total > 0) {
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(g.heads + nb, (unsigned)total);
    base = __shfl(base, 0, 64);
    if (base + (unsigned)total > g.poolPerNb) {
      if (lane == 0) *g.overflow = 1;   // every writer stores the same word
    } else {
      const NbDev& N = g.nb[nb];
      uint32_t* pool = g.pool + (size_t)nb * g.poolPerNb;
      const int i1 = g.qFeat[q];
      const uint8_t* qd = g.R.blockPool + (size_t)(g.k1.blockStart + i1) * 32;
      const KeyPointDev k1 = g.R.kps[g.k1.featStart + i1];
      const bool good1 = g.R.rightX[g.k1.featStart + i1] >= 0;
      int written = 0;
      for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        bool pass = false;
        int idx = 0, dist = 0;
        if (t < total) {
          idx = g.R.bowPool[rg.x + t].y;
          const bool good2 = g.R.rightX[N.k2.featStart + idx] >= 0;
          pass = g.R.rowPool[N.k2.rowStart + idx] < 0 && (!g.stereoOnly || good2);
          if (pass) dist = hamming256(qd, g.R.blockPool + (size_t)(N.k2.blockStart + idx) * 32);
          if (pass) pass = dist <= kThLow && tri_pair_ok(N.geom, k1, good1, g.R.kps[N.k2.featStart + idx], good2);
        }
        const unsigned long long m = __ballot(pass);
        if (pass) pool[base + written + __popcll(m & ((1ull << lane) - 1ull))] = ((uint32_t)dist << 16) | (uint32_t)idx;
        written += __popcll(m);
      }
      info = make_int2((int)((size_t)nb * g.poolPerNb + base), written);
    }
  }
  if (lane == 0) g.qInfo[at] = info;
}

struct GeometryArgs {
  Pools R;
  const FirstDev* first;
  int nNb, nq, nb;         // nb: the neighbour k_resolve has just resolved
  const NbDev* nbs;
  const float* depth;      // the first keyframe's [n] at 0, then each neighbour's at its depthAt
  const int* qFeat;
  const int* assigned;     // [nNb][nq] k_resolve's result per query: the second keyframe's feature or -1
  int2* qInfo;             // [nNb][nq]
  int* matched;            // [nNb][n] out
  float* x3d;              // [nNb][n][3] out
  uint8_t* status;         // [nNb][n] out
};

static __global__ __launch_bounds__(kThreads) void k_mapdb_tri_geometry(GeometryArgs g) {
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= g.nq) return;
  const int i2 = g.assigned[(size_t)g.nb * g.nq + q];
  if (i2 < 0) return;
  const NbDev& N = g.nbs[g.nb];
  const FirstDev& A = *g.first;
  const int i1 = g.qFeat[q];
  const KeyPointDev k1 = g.R.kps[A.k1.featStart + i1], k2 = g.R.kps[N.k2.featStart + i2];
  const float4 f1 = make_float4(k1.x, k1.y, g.R.rightX[A.k1.featStart + i1], g.depth[i1]);
  const float4 f2 = make_float4(k2.x, k2.y, g.R.rightX[N.k2.featStart + i2], g.depth[N.depthAt + i2]);
  const float4 lv = make_float4(A.sigma2[k1.octave], N.geom.sf2B[k2.octave], A.sf[k1.octave], N.geom.sfB[k2.octave]);
  float X, Y, Z;
  const uint8_t st = tri::triangulate_match(A.view, N.view, f1, f2, lv, N.ratioFactor, X, Y, Z);
  const size_t o = (size_t)g.nb * A.k1.n + i1;
  g.matched[o] = i2;
  g.x3d[3 * o] = X; g.x3d[3 * o + 1] = Y; g.x3d[3 * o + 2] = Z;
  g.status[o] = st;
  if ((st & 15) == 0)   // accepted: idx1 has a map point for every later neighbour
    for (int j = g.nb + 1; j < g.nNb; j++) g.qInfo[(size_t)j * g.nq + q].y = 0;
}

}  // namespace mapdbtri
}  // namespace ydorb
