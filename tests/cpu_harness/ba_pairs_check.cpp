// Stand-alone check of the BA skyline's host plan (ydorbslam_amd/csrc/ba_pairs.h over skyline_plan.h): the covisible pair list and the
// envelope on small graphs, against a brute-force statement in this file.  Built with -fsanitize=address,undefined by
// tests/test_ba_skyline_cpu.py; it has its own main and loads nothing else.
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../ydorbslam_amd/csrc/ba_pairs.h"

using namespace ydorb;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                             \
  do {                                                                          \
    if (!(cond)) { printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
  } while (0)

struct Graph {
  int K = 0;
  std::vector<uint8_t> fixed;
  std::vector<int> edgePose, edgePoint;
  int nPoints = 0;
  void point(const std::vector<int>& seenBy) {
    for (int k : seenBy) { edgePose.push_back(k); edgePoint.push_back(nPoints); }
    nPoints++;
  }
};

Graph chain(int K, int span, bool loop) {
  Graph g;
  g.K = K; g.fixed.assign(K, 0); g.fixed[0] = 1;
  for (int k = 0; k < K; k++) {
    std::vector<int> seen;
    for (int j = 0; j < span; j++)
      if (k + j < K) seen.push_back(k + j);
    if (loop && k < 2)   // the loop closure: the last three keyframes see the first points
      for (int c = K - 3; c < K; c++) seen.push_back(c);
    g.point(seen);
  }
  return g;
}

struct Checked { bapairs::PairList L; sky::Plan P; bool ok; std::string err; };

Checked check(const char* name, const Graph& g, int ordering, int64_t maxBytes = 0) {
  Checked c;
  c.L = bapairs::buildPairsFromEdges(g.K, g.nPoints, (int)g.edgePose.size(), g.fixed.data(), g.edgePose.data(), g.edgePoint.data(), false);
  const bapairs::PairList& L = c.L;
  // brute force: free index, then every pair of free poses of every point
  std::vector<int> idx(g.K, -1);
  std::vector<char> used(g.K, 0);
  for (int k : g.edgePose) used[k] = 1;
  int nPf = 0;
  for (int k = 0; k < g.K; k++) if (used[k] && !g.fixed[k]) idx[k] = nPf++;
  std::set<std::pair<int, int>> want;
  for (int p = 0; p < g.nPoints; p++)
    for (size_t a = 0; a < g.edgePose.size(); a++)
      for (size_t b = 0; b < g.edgePose.size(); b++)
        if (g.edgePoint[a] == p && g.edgePoint[b] == p && idx[g.edgePose[a]] >= 0 && idx[g.edgePose[a]] < idx[g.edgePose[b]])
          want.insert({idx[g.edgePose[a]], idx[g.edgePose[b]]});
  CHECK(L.nPf == nPf);
  CHECK(L.covisiblePairs == (int64_t)want.size());
  CHECK(L.buckets() == (int64_t)want.size() + nPf);
  CHECK((int)L.rowStart.size() == nPf + 1 && L.rowStart[nPf] == (int)L.buckets());
  for (int i = 0; i < nPf; i++) {   // every row ascending, each pair once, the diagonal last
    CHECK(L.rowStart[i] < L.rowStart[i + 1]);
    for (int q = L.rowStart[i]; q < L.rowStart[i + 1]; q++) {
      CHECK(L.i2[q] == i && L.i1[q] <= i);
      if (q + 1 < L.rowStart[i + 1]) CHECK(L.i1[q] < L.i1[q + 1]);
      if (L.i1[q] != i) CHECK(want.count({L.i1[q], i}) == 1);
      CHECK(L.find(L.i1[q], i) == q);
    }
    CHECK(L.i1[L.rowStart[i + 1] - 1] == i);
  }
  c.ok = bapairs::planEnvelope(L, ordering, maxBytes, true, c.P, c.err);
  const sky::Plan& P = c.P;
  if (c.ok) {
    CHECK((int)P.perm.size() == nPf && (int)P.first.size() == nPf);
    std::vector<char> seen(nPf, 0);
    for (int k = 0; k < nPf; k++) { CHECK(P.perm[k] >= 0 && P.perm[k] < nPf && !seen[P.perm[k]]); seen[P.perm[k]] = 1; CHECK(P.inv[P.perm[k]] == k); }
    std::vector<int> first(nPf);
    for (int k = 0; k < nPf; k++) first[k] = k;
    for (const auto& pr : want) {
      const int a = P.inv[pr.first], b = P.inv[pr.second], hi = std::max(a, b), lo = std::min(a, b);
      first[hi] = std::min(first[hi], lo);
    }
    int64_t blocks = 0;
    for (int k = 0; k < nPf; k++) { CHECK(P.first[k] == first[k] && P.first[k] <= k); blocks += k - first[k] + 1; }
    CHECK(blocks == P.envBlocks && P.rowOff[nPf] == blocks);
    // every bucket's destination lies in its row of the envelope, transposed exactly when the order swaps the pair
    const std::vector<int64_t> dst = bapairs::bucketDestinations(L, P);
    std::set<int64_t> blocksHit;
    for (size_t q = 0; q < dst.size(); q++) {
      const int p1 = P.inv[L.i1[q]], p2 = P.inv[L.i2[q]], row = std::max(p1, p2);
      const int64_t blk = dst[q] >> 1;
      CHECK(blk >= P.rowOff[row] && blk < P.rowOff[row + 1]);
      CHECK((dst[q] & 1) == (p1 > p2 ? 1 : 0));
      CHECK(blocksHit.insert(blk).second);
    }
    // the column lists: ascending rows, as many entries as blocks off the diagonal
    CHECK(P.colStart[nPf] == blocks - nPf);
    for (int j = 0; j < nPf; j++)
      for (int64_t q = P.colStart[j]; q < P.colStart[j + 1]; q++) {
        CHECK(P.colRows[q] > j && P.first[P.colRows[q]] <= j);
        CHECK(P.colBlk[q] == P.rowOff[P.colRows[q]] + j - P.first[P.colRows[q]]);
        if (q + 1 < P.colStart[j + 1]) CHECK(P.colRows[q] < P.colRows[q + 1]);
      }
  }
  printf("%s: %d free, %lld pairs, %lld blocks, widest row %d, %s\n", name, nPf, (long long)L.covisiblePairs, (long long)P.envBlocks, P.maxRowBlocks,
         !c.ok ? "refused" : P.orderingUsed == sky::kOrderRcm ? "rcm" : "natural");
  return c;
}

}  // namespace

int main() {
  {
    const Checked c = check("chain, span 3", chain(30, 3, false), sky::kOrderSmaller);
    CHECK(c.ok && c.P.maxRowBlocks == 3 && c.P.orderingUsed == sky::kOrderNatural && c.L.covisiblePairs == 28 + 27);
  }
  {
    const Graph g = chain(40, 3, true);
    const Checked nat = check("loop, natural", g, sky::kOrderNatural), rcm = check("loop, rcm", g, sky::kOrderRcm), sm = check("loop, smaller", g, sky::kOrderSmaller);
    CHECK(nat.P.maxRowBlocks == 39 && rcm.P.maxRowBlocks <= 6 && sm.P.orderingUsed == sky::kOrderRcm && sm.P.envBlocks == rcm.P.envBlocks);
    CHECK(sm.P.envBlocks < nat.P.envBlocks);
  }
  {
    Graph g;   // keyframe 1 sees every point, each other keyframe one of them
    g.K = 12; g.fixed.assign(12, 0); g.fixed[0] = 1;
    for (int k = 2; k < 12; k++) g.point({1, k});
    const Checked c = check("star, hub first", g, sky::kOrderNatural);
    CHECK(c.P.envBlocks == 11 * 12 / 2 && c.L.covisiblePairs == 10);
    CHECK(check("star, smaller", g, sky::kOrderSmaller).P.envBlocks == 2 * 11 - 1);
  }
  {
    Graph g;   // two components: 1-2-3 and 4-5-6
    g.K = 7; g.fixed.assign(7, 0); g.fixed[0] = 1;
    g.point({0, 1}); g.point({1, 2}); g.point({2, 3}); g.point({4, 5}); g.point({5, 6}); g.point({4, 6});
    const Checked c = check("two components", g, sky::kOrderNatural);
    CHECK(c.P.first[3] == 3 && c.P.first[2] == 1);
  }
  {
    Graph g;   // keyframe 3 shares points with fixed keyframes only; keyframe 5 has no edge; point 0 is seen twice by keyframe 1
    g.K = 6; g.fixed.assign(6, 0); g.fixed[0] = g.fixed[4] = 1;
    g.point({1, 2, 1}); g.point({0, 3, 4}); g.point({2, 1});
    const Checked c = check("fixed-only and idle", g, sky::kOrderSmaller);
    CHECK(c.L.nPf == 3 && c.L.covisiblePairs == 1 && c.P.first[2] == 2);
  }
  {
    Graph g;
    g.K = 3; g.fixed.assign(3, 1);
    g.point({0, 1, 2});
    const Checked c = check("all fixed", g, sky::kOrderSmaller);
    CHECK(c.ok && c.L.nPf == 0 && c.L.buckets() == 0 && c.P.envBlocks == 0);
  }
  {
    Graph g;   // no edges at all
    g.K = 2; g.fixed.assign(2, 0);
    CHECK(check("no edges", g, sky::kOrderRcm).L.nPf == 0);
  }
  {
    const Graph g = chain(30, 3, false);
    const Checked c = check("tiny limit", g, sky::kOrderNatural, 1000);
    CHECK(!c.ok && c.err.find("takes 24192 bytes") != std::string::npos && c.err.find("max_factor_bytes is 1000") != std::string::npos);
  }
  {
    Graph g;   // a dense envelope of 601 block rows: 600 * 601 * 602 / 6 block updates, above 2^24
    g.K = 603; g.fixed.assign(603, 0); g.fixed[0] = 1;
    for (int k = 2; k < 603; k++) g.point({1, k});
    bapairs::PairList L = bapairs::buildPairsFromEdges(g.K, g.nPoints, (int)g.edgePose.size(), g.fixed.data(), g.edgePose.data(), g.edgePoint.data(), false);
    sky::Plan P;
    std::string err;
    CHECK(!bapairs::planEnvelope(L, sky::kOrderNatural, 0, true, P, err));
    CHECK(err.find("takes 36361101 block updates") != std::string::npos && err.find("at most 16777216") != std::string::npos);
    CHECK(P.colRows.empty());   // refused before the column lists
    CHECK(bapairs::planEnvelope(L, sky::kOrderSmaller, 0, true, P, err) && P.envBlocks == 2 * 602 - 1);
    printf("work bound: %s\n", err.c_str());
  }
  printf("%d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
