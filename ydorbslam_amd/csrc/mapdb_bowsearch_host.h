// Host half of the batched BoW searches over the resident map table (include/ydorb/c_api.h, ydorb_mapdb_search_by_bow_keyframes and
// ydorb_mapdb_search_by_bow_frame): what the entries decide before any device work and a plain-C++ execution of
// one pair of the search.
//   checkBowFrame      the refusals of the frame form's YdBowSide, first offender named
//   flattenFrameBow    the frame's feature vector as (node, feature) pairs in map order: what the kernels' binary searches walk
//   bowQueryStarts     where the queries of each pair begin (mode 3: a prefix sum of the usable keyframes' span lengths)
//   goodMapPoint       the rule "has a good map point" of every resident side
//   bowSearchOnHost    the reference's sequential loops (orbMatcher.cpp:303-462) over host copies of the pools: merge-join of the two
//                      node lists, validity, best / second over the bucket, ratio test, the rotation histogram.  It is not a
//                      transcription of the kernels: there is no binary search, no record pool and no query table in it.
// No HIP here: a plain host compiler builds it (tests/cpu_harness/mapdb_bowsearch_check.cpp).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "map_table.h"
#include "mapdb_bow_host.h"

namespace ydorb {
namespace mapdb {

constexpr int32_t kMaxBowFrameFeatures = 65535;   // a candidate record packs its feature index in 16 bits

// The frame side of ydorb_mapdb_search_by_bow_frame.  valid may be null: every feature is a candidate.
inline bool checkBowFrame(const YdBowSide* f, std::string& err) {
  if (!f) return fail(err, "null frame");
  if (f->n < 0 || f->n > kMaxBowFrameFeatures) return fail(err, "frame: n %lld outside 0..65535", f->n);
  if (f->n > 0 && (!f->kps || !f->desc)) return fail(err, "frame: null kps or desc");
  const YdFeatureVector& v = f->fv;
  if (v.n_nodes < 0) return fail(err, "frame: negative number of nodes: %lld", v.n_nodes);
  if (!v.node_start) return fail(err, "frame: null node_start");
  if (v.node_start[0] != 0) return fail(err, "frame: node_start[0] is %lld, not 0", v.node_start[0]);
  if (v.n_nodes > 0 && !v.node_ids) return fail(err, "frame: null node_ids");
  for (int32_t a = 0; a < v.n_nodes; a++) {
    if (v.node_start[a + 1] < v.node_start[a]) return fail(err, "frame: node_start decreases at %lld", a + 1);
    if (a > 0 && v.node_ids[a] <= v.node_ids[a - 1])
      return fail(err, "frame: node id %lld after %lld, the node ids ascend strictly", (long long)v.node_ids[a], (long long)v.node_ids[a - 1]);
  }
  const int32_t total = v.node_start[v.n_nodes];
  if (total > 0 && !v.feat) return fail(err, "frame: null feat");
  for (int32_t q = 0; q < total; q++)
    if (v.feat[q] < 0 || v.feat[q] >= f->n) return fail(err, "frame: entry %lld: feature index %lld outside 0..%lld", q, v.feat[q], f->n - 1);
  return true;
}

// (node, feature) in map order.  A node id of 2^31 or more keeps its bits: the kernels compare ids as unsigned, and no resident id
// reaches it (mapdb_bow_host.h refuses one).
inline void flattenFrameBow(const YdFeatureVector& v, std::vector<BowRec>& out) {
  out.clear();
  for (int32_t a = 0; a < v.n_nodes; a++)
    for (int32_t q = v.node_start[a]; q < v.node_start[a + 1]; q++) out.push_back(BowRec{(int32_t)v.node_ids[a], v.feat[q]});
}

// start [n + 1]: the queries of pair i are [start[i], start[i + 1]); an unusable pair has none.  False past INT32_MAX.
inline bool bowQueryStarts(const int32_t* len, const uint8_t* status, int32_t n, std::vector<int32_t>& start) {
  start.assign((size_t)n + 1, 0);
  int64_t at = 0;
  for (int32_t i = 0; i < n; i++) {
    if (!status[i]) at += len[i];
    if (at > INT32_MAX) return false;
    start[(size_t)i + 1] = (int32_t)at;
  }
  return true;
}

// The row entry names a point slot below the table's capacity whose bad flag is clear; a slot never set reads as bad.
inline bool goodMapPoint(int32_t p, const uint8_t* bad, int32_t pointCap) { return p >= 0 && p < pointCap && !bad[p]; }

struct BowSearchSide {
  const BowRec* bow; int32_t bowLen;   // the feature vector in map order
  const YdKeyPoint* kps; const uint8_t* desc; int32_t n;
  const int32_t* row;                  // resident side: the keyframe's row [n]; null for the frame
  const uint8_t* valid;                // the frame only: null = every feature
};

namespace bowsearch_detail {
inline int hamming(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i += 8) {
    uint64_t x, y;
    memcpy(&x, a + i, 8);
    memcpy(&y, b + i, 8);
    d += __builtin_popcountll(x ^ y);
  }
  return d;
}
inline int rotBin(float a1, float a2) {   // orbMatcher.cpp:121-130
  const float factor = 1.0 / 30;
  float rot = a1 - a2;
  if (rot < 0.0) rot += 360.0;
  int bin = (int)round(rot * factor);
  if (bin == 30) bin = 0;
  return bin;
}
}  // namespace bowsearch_detail

// One pair.  mode 4: A = the first keyframe, B = the second; matched / point [A.n]: the second keyframe's feature and its row entry.
// mode 3: A = the keyframe, B = the frame; matched / point [B.n]: the keyframe's feature and its row entry.  -1 where there is no
// match.  Returns the reference's count.
inline int bowSearchOnHost(int mode, const BowSearchSide& A, const BowSearchSide& B, const uint8_t* bad, int32_t pointCap, float ratio, int checkOrientation,
                           int32_t* matched, int32_t* point) {
  using namespace bowsearch_detail;
  const int32_t nOut = mode == 3 ? B.n : A.n;
  for (int32_t i = 0; i < nOut; i++) { matched[i] = -1; point[i] = -1; }
  std::vector<uint8_t> matchedB((size_t)B.n, 0);
  std::vector<std::vector<int32_t>> rotHist(30);
  int matchNum = 0;
  int32_t a = 0, b = 0;
  while (a < A.bowLen && b < B.bowLen) {
    const uint32_t na = (uint32_t)A.bow[a].node, nb = (uint32_t)B.bow[b].node;
    if (na < nb) { a++; continue; }
    if (nb < na) { b++; continue; }
    int32_t aEnd = a, bEnd = b;
    while (aEnd < A.bowLen && (uint32_t)A.bow[aEnd].node == na) aEnd++;
    while (bEnd < B.bowLen && (uint32_t)B.bow[bEnd].node == na) bEnd++;
    for (int32_t ia = a; ia < aEnd; ia++) {
      const int32_t idxA = A.bow[ia].feat;
      if (!goodMapPoint(A.row[idxA], bad, pointCap)) continue;
      int bestDist = 256, secondDist = 256;
      int32_t bestIdx = -1;
      for (int32_t ib = b; ib < bEnd; ib++) {
        const int32_t idxB = B.bow[ib].feat;
        if (matchedB[(size_t)idxB]) continue;
        if (B.row ? !goodMapPoint(B.row[idxB], bad, pointCap) : (B.valid && !B.valid[idxB])) continue;
        const int dist = hamming(A.desc + (size_t)idxA * 32, B.desc + (size_t)idxB * 32);
        if (dist < bestDist) { secondDist = bestDist; bestDist = dist; bestIdx = idxB; }
        else if (dist < secondDist) secondDist = dist;
      }
      if (bestDist <= 50 && static_cast<float>(bestDist) < ratio * static_cast<float>(secondDist)) {
        matchedB[(size_t)bestIdx] = 1;
        const int32_t o = mode == 3 ? bestIdx : idxA;
        matched[o] = mode == 3 ? idxA : bestIdx;
        point[o] = mode == 3 ? A.row[idxA] : B.row[bestIdx];
        if (checkOrientation) rotHist[(size_t)rotBin(A.kps[idxA].angle, B.kps[bestIdx].angle)].push_back(o);
        matchNum++;
      }
    }
    a = aEnd; b = bEnd;
  }
  if (checkOrientation) {   // computeThreeMaxima, orbMatcher.cpp:827-854
    int i1 = -1, i2 = -1, i3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < 30; i++) {
      const int s = (int)rotHist[(size_t)i].size();
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
      else if (s > max3) { max3 = s; i3 = i; }
    }
    if (max2 < max1 / 10) { i3 = -1; i2 = -1; }
    else if (max3 < max1 / 10) { i3 = -1; }
    for (int i = 0; i < 30; i++)
      if (i != i1 && i != i2 && i != i3)
        for (int32_t o : rotHist[(size_t)i]) { matched[o] = -1; point[o] = -1; matchNum--; }
  }
  return matchNum;
}

}  // namespace mapdb
}  // namespace ydorb
