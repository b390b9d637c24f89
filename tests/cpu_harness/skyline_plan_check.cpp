// Stand-alone check of ydorbslam_amd/csrc/skyline_plan.h (no HIP, no GPU): the order and the envelope of the block-skyline Cholesky on
// small graphs whose difficulties are known.  tests/test_essgraph_skyline_cpu.py builds it with -fsanitize=address,undefined and runs it
// as its own process.  Prints one line per graph and ordering; the exit status is the number of failed properties.  Then the two
// directions between an envelope and the dense matrix (expandEnvelope, packEnvelope) for both block sizes, which print failures only.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/skyline_plan.h"

namespace {

using ydorb::sky::Plan;
int g_failed = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { g_failed++; printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct TestGraph {
  std::string name;
  int nV;
  std::vector<int> fixed;
  std::vector<std::pair<int, int>> edges;
};

std::vector<std::pair<int, int>> ring(int n) {
  std::vector<std::pair<int, int>> e;
  for (int i = 0; i + 1 < n; i++) e.push_back({i, i + 1});
  e.push_back({n - 1, 0});
  return e;
}

std::vector<TestGraph> graphs() {
  std::vector<TestGraph> out;
  out.push_back({"two", 2, {0}, {{0, 1}}});
  {
    auto e = ring(6); e.push_back({1, 4});
    out.push_back({"six", 6, {0}, e});
  }
  {
    auto e = ring(12); e.push_back({3, 4}); e.push_back({4, 3});
    out.push_back({"ring12 with repeated pairs", 12, {0}, e});
  }
  {
    std::vector<std::pair<int, int>> e = {{39, 0}, {31, 16}};
    for (int v = 1; v < 40; v++) e.push_back({v, (v - 1) / 2});
    for (int v = 1; v < 39; v += 2) e.push_back({v, v + 1});
    for (int v = 3; v < 30; v += 7) e.push_back({v, v + 5});
    out.push_back({"tree40", 40, {0}, e});
  }
  {
    std::vector<std::pair<int, int>> e = {{0, 1}};
    for (int v = 2; v < 10; v++) e.push_back({1, v});
    out.push_back({"star, hub first", 10, {0}, e});
  }
  {
    std::vector<std::pair<int, int>> e = {{0, 9}};
    for (int v = 1; v < 9; v++) e.push_back({v, 9});
    out.push_back({"star, hub last", 10, {0}, e});
  }
  out.push_back({"two components off one fixed vertex", 8, {0}, {{0, 1}, {1, 2}, {2, 3}, {3, 1}, {0, 4}, {4, 5}, {5, 6}, {6, 7}, {7, 4}}});
  {
    auto e = ring(9); e.push_back({2, 6});
    out.push_back({"fixed vertex in the middle", 9, {4}, e});
  }
  {
    auto e = ring(11); e.push_back({1, 8}); e.push_back({5, 0}); e.push_back({5, 7});
    out.push_back({"two fixed vertices", 11, {0, 7}, e});
  }
  for (int n : {12, 101}) out.push_back({"free ring " + std::to_string(n), n + 1, {n}, ring(n)});   // the fixed vertex hangs off nothing
  return out;
}

void freePairs(const TestGraph& g, int& nF, std::vector<int>& a, std::vector<int>& b) {
  std::vector<int> freeOf(g.nV, 0);
  for (int f : g.fixed) freeOf[f] = -1;
  nF = 0;
  for (int v = 0; v < g.nV; v++)
    if (freeOf[v] == 0) freeOf[v] = nF++;
  for (auto& e : g.edges) { a.push_back(freeOf[e.first]); b.push_back(freeOf[e.second]); }
}

bool sameArrays(const Plan& p, const Plan& q) {
  return p.perm == q.perm && p.inv == q.inv && p.first == q.first && p.rowOff == q.rowOff && p.colStart == q.colStart && p.colRows == q.colRows && p.colBlk == q.colBlk &&
         p.envBlocks == q.envBlocks && p.orderingUsed == q.orderingUsed && p.maxRowBlocks == q.maxRowBlocks;
}

void checkPlan(const TestGraph& g, int ordering, int nF, const std::vector<int>& a, const std::vector<int>& b, Plan& P) {
  using namespace ydorb::sky;
  P = makePlan(nF, (int)a.size(), a.data(), b.data(), ordering);
  buildColumns(P);
  const char* nm = g.name.c_str();
  EXPECT((int)P.perm.size() == nF && (int)P.inv.size() == nF && (int)P.first.size() == nF && (int)P.rowOff.size() == nF + 1, "%s", nm);
  std::vector<int> seen(nF, 0);
  for (int k = 0; k < nF; k++) {
    EXPECT(P.perm[k] >= 0 && P.perm[k] < nF, "%s: perm[%d] = %d", nm, k, P.perm[k]);
    if (P.perm[k] >= 0 && P.perm[k] < nF) { seen[P.perm[k]]++; EXPECT(P.inv[P.perm[k]] == k, "%s: inv is not perm's inverse at %d", nm, k); }
  }
  for (int f = 0; f < nF; f++) EXPECT(seen[f] == 1, "%s: free vertex %d placed %d times", nm, f, seen[f]);
  if (ordering == kOrderNatural)
    for (int k = 0; k < nF; k++) EXPECT(P.perm[k] == k, "%s: the natural order moved %d", nm, k);
  // every edge between free vertices lies inside the envelope, and first[] is attained by some edge (or is the diagonal)
  std::vector<int> lowest(nF);
  for (int k = 0; k < nF; k++) lowest[k] = k;
  for (size_t e = 0; e < a.size(); e++) {
    if (a[e] < 0 || b[e] < 0) continue;
    const int i = std::max(P.inv[a[e]], P.inv[b[e]]), j = std::min(P.inv[a[e]], P.inv[b[e]]);
    EXPECT(P.first[i] <= j, "%s: edge %zu at (%d, %d) lies before first = %d", nm, e, i, j, P.first[i]);
    lowest[i] = std::min(lowest[i], j);
  }
  int64_t blocks = 0;
  int longest = 0;
  for (int k = 0; k < nF; k++) {
    EXPECT(P.first[k] <= k && P.first[k] >= 0, "%s: first[%d] = %d", nm, k, P.first[k]);
    EXPECT(P.first[k] == lowest[k], "%s: first[%d] = %d, the lowest neighbour is %d", nm, k, P.first[k], lowest[k]);
    EXPECT(P.rowOff[k] == blocks, "%s: rowOff[%d]", nm, k);
    blocks += k - P.first[k] + 1;
    longest = std::max(longest, k - P.first[k] + 1);
  }
  EXPECT(P.rowOff[nF] == blocks && P.envBlocks == blocks && P.maxRowBlocks == longest, "%s: sizes", nm);
  EXPECT(P.envBlocks == (P.orderingUsed == kOrderRcm ? P.envRcm : P.envNatural), "%s: envelope of the order used", nm);
  // the column lists: ascending, and exactly the rows i > j with first[i] <= j
  EXPECT((int)P.colStart.size() == nF + 1 && P.colStart[0] == 0 && P.colStart[nF] == blocks - nF && (int64_t)P.colRows.size() == blocks - nF && P.colBlk.size() == P.colRows.size(), "%s: column sizes", nm);
  int64_t work = 0;
  for (int j = 0; j < nF; j++) {
    const int64_t m = P.colStart[j + 1] - P.colStart[j];
    work += m * (m + 1) / 2;
  }
  EXPECT(P.pairUpdates == work, "%s: pairUpdates %lld, the lists give %lld", nm, (long long)P.pairUpdates, (long long)work);
  for (int j = 0; j < nF; j++) {
    std::vector<int> want;
    for (int i = j + 1; i < nF; i++)
      if (P.first[i] <= j) want.push_back(i);
    const std::vector<int> got(P.colRows.begin() + P.colStart[j], P.colRows.begin() + P.colStart[j + 1]);
    EXPECT(got == want, "%s: column %d", nm, j);
    for (int64_t p = P.colStart[j]; p < P.colStart[j + 1] && got == want; p++) {
      const int i = P.colRows[(size_t)p];
      EXPECT(P.colBlk[(size_t)p] == P.rowOff[i] + (j - P.first[i]) && P.colBlk[(size_t)p] < P.rowOff[i + 1] - 1, "%s: block of (%d, %d)", nm, i, j);
    }
  }
  Plan again = makePlan(nF, (int)a.size(), a.data(), b.data(), ordering);
  buildColumns(again);
  EXPECT(sameArrays(P, again), "%s: two calls differ", nm);
}

// expandEnvelope / packEnvelope on plan P of B x B blocks.  The envelope holds distinct values, the upper triangle of a diagonal block
// mirroring its lower one, so that both conventions for the diagonal have to give the same symmetric matrix and packing returns the bytes.
template <int B> void checkEnvelope(const char* nm, const Plan& P) {
  using namespace ydorb::sky;
  const size_t N = (size_t)B * P.nF;
  std::vector<double> env(B * B * (size_t)P.envBlocks);
  for (size_t k = 0; k < env.size(); k++) env[k] = 1.0 + (double)k;
  for (int i = 0; i < P.nF; i++) {
    double* D = &env[B * B * (size_t)(P.rowOff[i + 1] - 1)];
    for (int r = 0; r < B; r++)
      for (int c = r + 1; c < B; c++) D[B * r + c] = D[B * c + r];
  }
  std::vector<double> whole(N * N, -1.0), lower(N * N, -2.0), back(env.size(), -3.0);
  expandEnvelope<B>(P, env.data(), whole.data(), kDiagWhole);
  expandEnvelope<B>(P, env.data(), lower.data(), kDiagLower);
  EXPECT(whole == lower, "%s B = %d: the two diagonal conventions differ on symmetric diagonal blocks", nm, B);
  size_t asym = 0, outside = 0, inside = 0;
  for (size_t r = 0; r < N; r++)
    for (size_t c = 0; c < N; c++) {
      asym += whole[r * N + c] != whole[c * N + r];
      const int pi = P.inv[r / B], pj = P.inv[c / B], i = std::max(pi, pj), j = std::min(pi, pj);
      if (j < P.first[i]) outside += whole[r * N + c] != 0.0; else inside += whole[r * N + c] == 0.0;
    }
  EXPECT(asym == 0 && outside == 0 && inside == 0, "%s B = %d: %zu asymmetric, %zu set outside the envelope, %zu left zero inside", nm, B, asym, outside, inside);
  packEnvelope<B>(P, whole.data(), back.data());
  EXPECT(back == env, "%s B = %d: packing the expansion does not return the envelope", nm, B);
  // where the conventions part: with a diagonal block's upper triangle spoilt, kDiagWhole copies it and kDiagLower does not read it
  std::vector<double> spoilt = env;
  spoilt[B * B * (size_t)(P.rowOff[1] - 1) + 1] = -7.0;   // entry (0, 1) of the first diagonal block
  expandEnvelope<B>(P, spoilt.data(), whole.data(), kDiagWhole);
  EXPECT(whole != lower, "%s B = %d: kDiagWhole did not copy the stored upper triangle", nm, B);
  expandEnvelope<B>(P, spoilt.data(), whole.data(), kDiagLower);
  EXPECT(whole == lower, "%s B = %d: kDiagLower read the upper triangle", nm, B);
}

void checkEnvelopes() {
  using namespace ydorb::sky;
  std::vector<std::pair<int, int>> star;
  for (int v = 1; v < 5; v++) star.push_back({0, v});
  const TestGraph gs[] = {{"closed ring 12", 12, {}, ring(12)}, {"star 5, hub first", 5, {}, star}};
  for (const TestGraph& g : gs)
    for (int ordering : {kOrderNatural, kOrderRcm}) {
      int nF;
      std::vector<int> a, b;
      freePairs(g, nF, a, b);
      Plan P = makePlan(nF, (int)a.size(), a.data(), b.data(), ordering);
      buildColumns(P);
      EXPECT(P.orderingUsed == ordering && nF == g.nV, "%s", g.name.c_str());
      checkEnvelope<6>(g.name.c_str(), P);
      checkEnvelope<7>(g.name.c_str(), P);
    }
}

}  // namespace

int main() {
  using namespace ydorb::sky;
  for (const TestGraph& g : graphs()) {
    int nF;
    std::vector<int> a, b;
    freePairs(g, nF, a, b);
    Plan nat, rcm, smaller;
    checkPlan(g, kOrderNatural, nF, a, b, nat);
    checkPlan(g, kOrderRcm, nF, a, b, rcm);
    checkPlan(g, kOrderSmaller, nF, a, b, smaller);
    EXPECT(nat.orderingUsed == kOrderNatural && rcm.orderingUsed == kOrderRcm, "%s", g.name.c_str());
    EXPECT(smaller.envBlocks <= nat.envBlocks && smaller.envBlocks <= rcm.envBlocks, "%s: SMALLER is not the smaller", g.name.c_str());
    if (rcm.envBlocks >= nat.envBlocks) EXPECT(smaller.orderingUsed == kOrderNatural, "%s: natural on a tie", g.name.c_str());
    else EXPECT(sameArrays(smaller, rcm), "%s: SMALLER is not the RCM plan", g.name.c_str());
    EXPECT(nat.envNatural == rcm.envNatural && nat.envRcm == rcm.envRcm, "%s: both sizes in every plan", g.name.c_str());
    if (g.name.rfind("free ring", 0) == 0) {
      EXPECT(nat.maxRowBlocks == nF, "%s: the natural order's last row is full", g.name.c_str());
      EXPECT(rcm.maxRowBlocks <= 3, "%s: RCM leaves a row of %d blocks", g.name.c_str(), rcm.maxRowBlocks);
    }
    printf("%-36s free %3d  envelope natural %5lld  rcm %5lld  longest row %3d / %3d  smaller -> %s\n", g.name.c_str(), nF, (long long)nat.envBlocks,
           (long long)rcm.envBlocks, nat.maxRowBlocks, rcm.maxRowBlocks, smaller.orderingUsed == kOrderRcm ? "rcm" : "natural");
  }
  checkEnvelopes();
  printf("%d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
