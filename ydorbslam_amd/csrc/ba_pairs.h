// Host plan of the BA's block-skyline reduced camera solve (ba_skyline.hip.h): the list of covisible free-pose
// pairs, which takes the place of the nPf (nPf + 1) / 2 bucket space of the dense path, and the envelope of S under the order
// skyline_plan.h picks for those pairs.  S has one 6x6 block per free pose and one per pair of free poses that share a landmark.
// Nothing here is sized by nPf^2 and every offset is 64-bit.  No HIP here: a plain host compiler builds it
// (tests/cpu_harness/ba_pairs_check.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "skyline_plan.h"

namespace ydorb {
namespace bapairs {

constexpr int64_t kBlockBytes = 36 * 8;   // one 6x6 block of the envelope (sky::kBlockBytes is the essential graph's 7x7)
constexpr int kDenseMaxRows = 19200;      // ba::kCholSolveMaxN (ba_solver.hip asserts that the two agree)
constexpr int64_t kDefaultFactorBytes = (int64_t)kDenseMaxRows * kDenseMaxRows * 8;   // the largest dense S
// One workgroup walks the columns in one launch: a block update is 36 entries x 6 multiply-subtracts = 432 flop, so this many of them
// are 7.2e9 flop, under the 1.2e10 flop DESIGN.md section 6j allows one launch that nothing can interrupt.
constexpr int64_t kMaxPairUpdates = (int64_t)1 << 24;
constexpr int64_t kMaxBuckets = (int64_t)1 << 30;   // bucket and item indices on the device are 32-bit

// The buckets of the Schur complement: for every free pose i2 the free poses i1 <= i2 that share a landmark with it, ascending, the
// diagonal (i1 == i2) last.  Bucket q is block (i2[q], i1[q]); the buckets of row i are rowStart[i] .. rowStart[i + 1] - 1.
struct PairList {
  int nPf = 0;
  int64_t covisiblePairs = 0;   // buckets off the diagonal
  std::vector<int> rowStart, i1, i2;
  int64_t buckets() const { return (int64_t)i1.size(); }
  // the bucket of (a, b), a <= b, or -1: what the device's binary search returns
  int64_t find(int a, int b) const {
    const int* lo = i1.data() + rowStart[b];
    const int* hi = i1.data() + rowStart[b + 1];
    const int* at = std::lower_bound(lo, hi, a);
    return at != hi && *at == a ? at - i1.data() : -1;
  }
};

// The edges grouped by landmark: ptStart [nL + 1] and, per edge in that order, the free-pose index of its pose (negative = fixed).
// The free poses of one landmark need not be sorted and may repeat.
inline PairList buildPairs(int nPf, int nL, const int* ptStart, const int* pidx) {
  PairList L;
  L.nPf = nPf;
  std::vector<uint64_t> keys;   // i2 << 32 | i1, i1 < i2
  std::vector<int> mine;
  size_t compactAt = (size_t)1 << 24;
  for (int l = 0; l < nL; l++) {
    mine.clear();
    for (int q = ptStart[l]; q < ptStart[l + 1]; q++)
      if (pidx[q] >= 0) mine.push_back(pidx[q]);
    std::sort(mine.begin(), mine.end());
    mine.erase(std::unique(mine.begin(), mine.end()), mine.end());
    for (size_t b = 1; b < mine.size(); b++)
      for (size_t a = 0; a < b; a++) keys.push_back((uint64_t)mine[b] << 32 | (uint32_t)mine[a]);
    if (keys.size() > compactAt) {   // keep the work list within a factor of the result's size
      std::sort(keys.begin(), keys.end());
      keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
      compactAt = std::max(compactAt, 2 * keys.size());
    }
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  L.covisiblePairs = (int64_t)keys.size();
  L.rowStart.assign((size_t)nPf + 1, 0);
  L.i1.reserve(keys.size() + (size_t)nPf);
  L.i2.reserve(keys.size() + (size_t)nPf);
  size_t k = 0;
  for (int i = 0; i < nPf; i++) {
    L.rowStart[i] = (int)L.i1.size();
    for (; k < keys.size() && (int)(keys[k] >> 32) == i; k++) { L.i1.push_back((int)(uint32_t)keys[k]); L.i2.push_back(i); }
    L.i1.push_back(i); L.i2.push_back(i);
  }
  L.rowStart[nPf] = (int)L.i1.size();
  return L;
}

// The same from a flat problem: free poses numbered as the driver numbers them (in the caller's order, a pose counts when it is not
// fixed and, unless `allPoses`, has an edge).  Returns the number of free poses.
inline PairList buildPairsFromEdges(int K, int NP, int E, const uint8_t* fixed, const int* edgePose, const int* edgePoint, bool allPoses) {
  std::vector<int> poseIdx((size_t)K, -1), start((size_t)NP + 1, 0), pidx((size_t)E);
  std::vector<uint8_t> used((size_t)K, allPoses ? 1 : 0);
  for (int e = 0; e < E; e++) used[edgePose[e]] = 1;
  int nPf = 0;
  for (int k = 0; k < K; k++) if (used[k] && !fixed[k]) poseIdx[k] = nPf++;
  for (int e = 0; e < E; e++) start[edgePoint[e] + 1]++;
  for (int p = 0; p < NP; p++) start[p + 1] += start[p];
  std::vector<int> fill(start.begin(), start.end() - 1);
  for (int e = 0; e < E; e++) pidx[fill[edgePoint[e]]++] = poseIdx[edgePose[e]];
  return buildPairs(nPf, NP, start.data(), pidx.data());
}

// The envelope for a pair list: the order, first[], the row offsets and the sizes; refused with both figures in `err` when the
// envelope is larger than maxFactorBytes (0 = kDefaultFactorBytes) or the factorisation takes more than kMaxPairUpdates block
// updates.  Both checks come before the column lists are built.
inline bool planEnvelope(const PairList& L, int ordering, int64_t maxFactorBytes, bool columns, sky::Plan& P, std::string& err) {
  const int nOff = (int)L.covisiblePairs;
  std::vector<int> a((size_t)nOff), b((size_t)nOff);
  for (size_t q = 0, k = 0; q < L.i1.size(); q++)
    if (L.i1[q] != L.i2[q]) { a[k] = L.i1[q]; b[k] = L.i2[q]; k++; }
  P = sky::makePlan(L.nPf, nOff, a.data(), b.data(), ordering);
  const long long limit = maxFactorBytes ? (long long)maxFactorBytes : (long long)kDefaultFactorBytes;
  const long long bytes = (long long)(P.envBlocks * kBlockBytes);
  const char* order = P.orderingUsed == sky::kOrderRcm ? "RCM" : "natural";
  char text[320];
  if (bytes > limit) {
    snprintf(text, sizeof(text), "BA: the skyline envelope takes %lld bytes (%lld blocks, %s order), max_factor_bytes is %lld", bytes,
             (long long)P.envBlocks, order, limit);
    err = text;
    return false;
  }
  if (P.pairUpdates > kMaxPairUpdates) {
    snprintf(text, sizeof(text), "BA: the skyline factorisation takes %lld block updates per trial (%lld envelope blocks, %s order), at most "
             "%lld are run in one launch", (long long)P.pairUpdates, (long long)P.envBlocks, order, (long long)kMaxPairUpdates);
    err = text;
    return false;
  }
  if (columns) sky::buildColumns(P);
  return true;
}

// Where bucket q's block goes: 2 * (block index in the envelope) + 1 when it is stored transposed (the order puts i1 after i2)
inline std::vector<int64_t> bucketDestinations(const PairList& L, const sky::Plan& P) {
  std::vector<int64_t> dst(L.i1.size());
  for (size_t q = 0; q < L.i1.size(); q++) {
    const int p1 = P.inv[L.i1[q]], p2 = P.inv[L.i2[q]];
    const int row = std::max(p1, p2), col = std::min(p1, p2);
    dst[q] = 2 * (P.rowOff[row] + (col - P.first[row])) + (p1 > p2 ? 1 : 0);
  }
  return dst;
}

}  // namespace bapairs
}  // namespace ydorb
