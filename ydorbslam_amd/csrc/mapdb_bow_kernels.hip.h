// gfx950 HIP kernels of ydorb_mapdb_search_by_bow_keyframes and ydorb_mapdb_search_by_bow_frame (orb_matcher.hip; DESIGN.md section 2
// "BoW searches on the resident table", section 6v): OrbMatcher::searchByBowInTwoKeyFrames (mode 4) and searchByBowInKeyFrameAndFrame
// (mode 3) for all candidate keyframes of one call.  The pairs do not depend on each other, so every step runs once over all of them:
//   k_mapdb_bow_join    one lane per (pair, entry of the A side's BoW span in map order).  Two binary searches over the B side's
//                       (node, feature) pairs give the bucket [begin, end) of the entry's node.  The range is empty when A's feature has
//                       no good map point or B lacks the node.  Queries are not compacted: query q is the span's entry q, which is the
//                       order of the reference's merge-join.  Mode 4: A is the first keyframe, the same for every pair (qFeat / qAngle
//                       are written once, by the first usable pair), B the pair's resident span.  Mode 3: A is the pair's keyframe (its queries start at
//                       the host's prefix sum), B the frame's feature vector, uploaded once per call.
//   k_mapdb_bow_gather  the body of k_gather_bow (match_kernels.hip.h) without the triangulation test: one wave per query, Hamming
//                       distances of the bucket 64 at a time, records appended in ballot order behind one atomicAdd on the pair's pool
//                       head.  A candidate counts when it has a good map point (mode 4) or its uploaded valid byte is set (mode 3).  A
//                       query that does not fit sets the overflow word and keeps count 0; nothing is written past the pool.
//   k_resolve           unchanged (match_kernels.hip.h), one launch with one workgroup per pair.
//   k_mapdb_bow_emit    one lane per (pair, query) in mode 4, per (pair, frame feature) in mode 3: k_resolve's result becomes the two
//                       dense outputs, the matched feature and the point slot of the keyframe's row at it.
// "Has a good map point": the row entry p is >= 0, below the point table's capacity, and the resident bad flag of p is clear (a slot
// never set reads as bad).  All wave64, plain vector stores, no LDS; the one atomic is the pool head.  Bounds: a usable keyframe's row
// and block have its feature count and the feature indices of its BoW span lie below it (the host's lock checks this), the frame's
// feature indices lie below its n (checkBowFrame), a row entry is compared with the capacity here before the bad flag is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.hip.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace mapdbbow {

constexpr int kThreads = 256;

struct Spans { int featStart, n, blockStart, rowStart, bowStart, bowLen; };   // == mapdb::ResidentTriSpans
struct Pools {
  const int* rowPool; const int2* bowPool; const KeyPointDev* kps; const uint8_t* blockPool;
  const uint8_t* bad; int pointCap;
};
struct PairDev {           // one candidate keyframe, in device memory
  Spans kf;
  int usable;              // 0: the pair has no query
  int qStart;              // where its queries begin in qRange / qInfo (mode 4: pair * nq, mode 3: the prefix sum)
};
struct SearchArgs {
  Pools R;
  int mode;                // 4 or 3
  Spans first;             // mode 4: the A side of every pair
  int nq;                  // mode 4: first.bowLen; mode 3: the longest span of a usable pair (the grid's extent)
  int nOut;                // the outputs' row length: mode 4 first.n, mode 3 the frame's n
  int writer;              // mode 4: the first usable pair, whose lanes write qFeat / qAngle
  const PairDev* pairs;
  const int2* frameBow; int frameBowLen;                 // mode 3: the B side
  const uint8_t *frameDesc, *frameValid;                 // frameValid null: every feature
  int2* qRange;            // into bowPool (mode 4) or frameBow (mode 3)
  int* qFeat;              // the feature of the A side behind a query: [nq] (mode 4) or at the pair's qStart (mode 3)
  float* qAngle;           // its angle, alike
  int2* qInfo;
  const int* assigned;     // k_resolve's result: mode 4 [pair][nq] feature of B per query, mode 3 [pair][nOut] query per frame feature
  int *matched, *point;    // [pair][nOut] out
  uint32_t* pool; unsigned* heads; unsigned poolPerPair; int* overflow;
};

__device__ __forceinline__ bool good_point(const Pools& R, int p) { return p >= 0 && p < R.pointCap && !R.bad[p]; }

// the pair's A side and how many queries it has
__device__ __forceinline__ const Spans& a_side(const SearchArgs& g, const PairDev& P) { return g.mode == 4 ? g.first : P.kf; }

static __global__ __launch_bounds__(kThreads) void k_mapdb_bow_join(SearchArgs g) {
  const int q = blockIdx.x * kThreads + threadIdx.x, pr = blockIdx.y;
  const PairDev& P = g.pairs[pr];
  if (!P.usable) return;
  const Spans& A = a_side(g, P);
  if (q >= A.bowLen) return;
  const int2 e = g.R.bowPool[A.bowStart + q];   // (node, feature)
  const int i1 = e.y;
  const int aAt = g.mode == 4 ? q : P.qStart + q;
  if (g.mode == 3 || pr == g.writer) {   // mode 4: once
    g.qFeat[aAt] = i1;
    g.qAngle[aAt] = g.R.kps[A.featStart + i1].angle;
  }
  int2 range = make_int2(0, 0);
  if (good_point(g.R, g.R.rowPool[A.rowStart + i1])) {
    const int2* B = g.mode == 4 ? g.R.bowPool + P.kf.bowStart : g.frameBow;
    const int nB = g.mode == 4 ? P.kf.bowLen : g.frameBowLen, off = g.mode == 4 ? P.kf.bowStart : 0;
    const unsigned node = (unsigned)e.x;
    int lo = 0, hi = nB;   // the first entry whose node is not below e.x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((unsigned)B[mid].x < node) lo = mid + 1; else hi = mid;
    }
    const int begin = lo;
    hi = nB;               // the first entry whose node is above e.x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((unsigned)B[mid].x <= node) lo = mid + 1; else hi = mid;
    }
    range = make_int2(off + begin, off + lo);
  }
  g.qRange[P.qStart + q] = range;
}

static __global__ __launch_bounds__(kThreads) void k_mapdb_bow_gather(SearchArgs g) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wv, pr = blockIdx.y;
  const PairDev& P = g.pairs[pr];
  if (!P.usable) return;
  const Spans& A = a_side(g, P);
  if (q >= A.bowLen) return;
  const int at = P.qStart + q;
  const int2 rg = g.qRange[at];
  const int total = rg.y - rg.x;
  int2 info = make_int2(0, 0);
  if (total > 0) {
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(g.heads + pr, (unsigned)total);
    base = __shfl(base, 0, 64);
    if (base + (unsigned)total > g.poolPerPair) {
      if (lane == 0) *g.overflow = 1;   // every writer stores the same word
    } else {
      uint32_t* pool = g.pool + (size_t)pr * g.poolPerPair;
      const int i1 = g.qFeat[g.mode == 4 ? q : at];
      const uint8_t* qd = g.R.blockPool + (size_t)(A.blockStart + i1) * 32;
      const int2* B = g.mode == 4 ? g.R.bowPool : g.frameBow;
      int written = 0;
      for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        bool pass = false;
        int idx = 0, dist = 0;
        if (t < total) {
          idx = B[rg.x + t].y;
          if (g.mode == 4) {
            pass = good_point(g.R, g.R.rowPool[P.kf.rowStart + idx]);
            if (pass) dist = hamming256(qd, g.R.blockPool + (size_t)(P.kf.blockStart + idx) * 32);
          } else {
            pass = !g.frameValid || g.frameValid[idx];
            if (pass) dist = hamming256(qd, g.frameDesc + (size_t)idx * 32);
          }
        }
        const unsigned long long m = __ballot(pass);
        if (pass) pool[base + written + __popcll(m & ((1ull << lane) - 1ull))] = ((uint32_t)dist << 16) | (uint32_t)idx;
        written += __popcll(m);
      }
      info = make_int2((int)((size_t)pr * g.poolPerPair + base), written);
    }
  }
  if (lane == 0) g.qInfo[at] = info;
}

// The outputs are -1 everywhere before this kernel; it writes the matches.  Mode 4: a feature index occurs once in a BoW span, so no two
// queries of a pair write the same element.
static __global__ __launch_bounds__(kThreads) void k_mapdb_bow_emit(SearchArgs g) {
  const int e = blockIdx.x * kThreads + threadIdx.x, pr = blockIdx.y;
  const PairDev& P = g.pairs[pr];
  if (!P.usable) return;
  if (g.mode == 4) {
    if (e >= g.nq) return;
    const int i2 = g.assigned[(size_t)pr * g.nq + e];
    if (i2 < 0) return;
    const size_t o = (size_t)pr * g.nOut + g.qFeat[e];
    g.matched[o] = i2;
    g.point[o] = g.R.rowPool[P.kf.rowStart + i2];
  } else {
    if (e >= g.nOut) return;
    const int q = g.assigned[(size_t)pr * g.nOut + e];
    if (q < 0) return;
    const int f = g.R.bowPool[P.kf.bowStart + q].y;
    const size_t o = (size_t)pr * g.nOut + e;
    g.matched[o] = f;
    g.point[o] = g.R.rowPool[P.kf.rowStart + f];
  }
}

}  // namespace mapdbbow
}  // namespace ydorb
