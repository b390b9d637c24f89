// Host plan of the essential graph's block-skyline Cholesky (essential_skyline.hip.h): the order of the free
// vertices and the envelope of H under it.  H has one 7x7 block per free vertex and one per connected pair; a Cholesky factor keeps its
// fill between a row's first non-zero and the diagonal, so the plan is that first block per row, the 64-bit offsets of the rows and,
// per column, the rows below it that reach it.  No symbolic elimination.  No HIP here: a plain host compiler builds it
// (tests/cpu_harness/skyline_plan_check.cpp).
//
// Positions: perm[k] = the free vertex (caller's numbering) at position k, inv = its inverse.  first, rowOff, colStart and colRows are
// indexed by position.  Row i stores the blocks of columns first[i] .. i, block (i, j) at rowOff[i] + (j - first[i]).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace ydorb {
namespace sky {

enum { kOrderSmaller = 0, kOrderNatural = 1, kOrderRcm = 2 };   // YDORB_ESS_ORDER_*
constexpr int64_t kBlockBytes = 49 * 8;

struct Plan {
  int nF = 0, orderingUsed = kOrderNatural, maxRowBlocks = 0;
  int64_t envBlocks = 0, envNatural = 0, envRcm = 0;
  int64_t pairUpdates = 0;         // the factorisation's work: sum over the columns of m (m + 1) / 2 block updates, m = the column's list
  std::vector<int> perm, inv, first;
  std::vector<int64_t> rowOff;     // [nF + 1]
  std::vector<int64_t> colStart;   // [nF + 1], filled by buildColumns
  std::vector<int> colRows;        // column j: the rows i > j with first[i] <= j, ascending
  std::vector<int64_t> colBlk;     // beside colRows: where that row's block of column j lies, rowOff[i] + j - first[i]
};

// The free vertices' adjacency without repeats, neighbours ascending.  a[e], b[e]: free indices of edge e's ends, negative = fixed.
struct Adjacency {
  std::vector<int> start, nbr;
  Adjacency(int nF, int nE, const int* a, const int* b) : start(nF + 1, 0) {
    std::vector<std::pair<int, int>> pairs;
    pairs.reserve(2 * (size_t)nE);
    for (int e = 0; e < nE; e++)
      if (a[e] >= 0 && b[e] >= 0 && a[e] != b[e]) { pairs.emplace_back(a[e], b[e]); pairs.emplace_back(b[e], a[e]); }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    nbr.resize(pairs.size());
    for (size_t k = 0; k < pairs.size(); k++) { start[pairs[k].first + 1]++; nbr[k] = pairs[k].second; }
    for (int f = 0; f < nF; f++) start[f + 1] += start[f];
  }
  int degree(int v) const { return start[v + 1] - start[v]; }
};

// first[] by position under `inv`, and the envelope's size in blocks
inline int64_t envelopeOf(const Adjacency& A, const std::vector<int>& inv, std::vector<int>& first) {
  const int nF = (int)inv.size();
  first.resize(nF);
  int64_t blocks = 0;
  for (int v = 0; v < nF; v++) {
    int lo = inv[v];
    for (int q = A.start[v]; q < A.start[v + 1]; q++) lo = std::min(lo, inv[A.nbr[q]]);
    first[inv[v]] = lo;
    blocks += inv[v] - lo + 1;
  }
  return blocks;
}

// Reverse Cuthill-McKee.  Components in the order of their lowest vertex; inside one, breadth first from a pseudo-peripheral vertex
// (George & Liu: from the lowest vertex, move to a vertex of least degree in the last level while that deepens the level structure),
// neighbours by (degree, index), the component's order reversed.  Every tie is broken by the vertex index.
inline std::vector<int> rcmOrder(const Adjacency& A) {
  const int nF = (int)A.start.size() - 1;
  std::vector<int> order, mark(nF, -1), queue;
  std::vector<char> placed(nF, 0);
  order.reserve(nF);
  int stamp = 0;
  auto lessDeg = [&](int x, int y) { return A.degree(x) != A.degree(y) ? A.degree(x) < A.degree(y) : x < y; };
  // breadth-first levels from r; returns the depth and leaves the last level in `last`
  auto levels = [&](int r, std::vector<int>& last) {
    queue.clear(); queue.push_back(r); mark[r] = ++stamp;
    size_t levelBegin = 0;
    int depth = 0;
    for (;;) {
      const size_t levelEnd = queue.size();
      for (size_t h = levelBegin; h < levelEnd; h++)
        for (int q = A.start[queue[h]]; q < A.start[queue[h] + 1]; q++)
          if (mark[A.nbr[q]] != stamp) { mark[A.nbr[q]] = stamp; queue.push_back(A.nbr[q]); }
      if (queue.size() == levelEnd) { last.assign(queue.begin() + levelBegin, queue.end()); return depth; }
      levelBegin = levelEnd; depth++;
    }
  };
  std::vector<int> last, fresh;
  for (int s0 = 0; s0 < nF; s0++) {
    if (placed[s0]) continue;
    int r = s0, depth = levels(r, last);
    for (;;) {
      const int cand = *std::min_element(last.begin(), last.end(), lessDeg);
      std::vector<int> candLast;
      const int d = levels(cand, candLast);
      if (d <= depth) break;
      r = cand; depth = d; last.swap(candLast);
    }
    const size_t begin = order.size();
    order.push_back(r); placed[r] = 1;
    for (size_t h = begin; h < order.size(); h++) {
      const int v = order[h];
      fresh.clear();
      for (int q = A.start[v]; q < A.start[v + 1]; q++)
        if (!placed[A.nbr[q]]) { placed[A.nbr[q]] = 1; fresh.push_back(A.nbr[q]); }
      std::sort(fresh.begin(), fresh.end(), lessDeg);
      order.insert(order.end(), fresh.begin(), fresh.end());
    }
    std::reverse(order.begin() + begin, order.end());
  }
  return order;
}

// Order, first, row offsets and the sizes.  `ordering` is kOrderSmaller / Natural / Rcm; Smaller takes the natural order on a tie.
inline Plan makePlan(int nF, int nE, const int* a, const int* b, int ordering) {
  Plan P;
  P.nF = nF;
  const Adjacency A(nF, nE, a, b);
  std::vector<int> natural(nF), invRcm(nF), firstNat, firstRcm;
  for (int f = 0; f < nF; f++) natural[f] = f;
  const std::vector<int> rcm = rcmOrder(A);
  for (int k = 0; k < nF; k++) invRcm[rcm[k]] = k;
  P.envNatural = envelopeOf(A, natural, firstNat);
  P.envRcm = envelopeOf(A, invRcm, firstRcm);
  const bool useRcm = ordering == kOrderRcm || (ordering == kOrderSmaller && P.envRcm < P.envNatural);
  P.orderingUsed = useRcm ? kOrderRcm : kOrderNatural;
  P.envBlocks = useRcm ? P.envRcm : P.envNatural;
  P.perm = useRcm ? rcm : natural;
  P.inv = useRcm ? invRcm : natural;
  P.first = useRcm ? firstRcm : firstNat;
  P.rowOff.assign(nF + 1, 0);
  for (int i = 0; i < nF; i++) {
    P.rowOff[i + 1] = P.rowOff[i] + (i - P.first[i] + 1);
    P.maxRowBlocks = std::max(P.maxRowBlocks, i - P.first[i] + 1);
  }
  std::vector<int64_t> delta(nF + 1, 0);   // +1 at first[i], -1 at i: the prefix sum at j counts the rows that reach column j
  for (int i = 0; i < nF; i++) { delta[P.first[i]]++; delta[i]--; }
  int64_t reach = 0;
  for (int j = 0; j < nF; j++) { reach += delta[j]; P.pairUpdates += reach * (reach + 1) / 2; }
  return P;
}

// The column lists: as many entries as the envelope has blocks off the diagonal, so the caller checks the envelope's size first.
inline void buildColumns(Plan& P) {
  const int nF = P.nF;
  P.colStart.assign(nF + 1, 0);
  std::vector<int64_t> delta(nF + 1, 0);   // +1 at first[i], -1 at i: the prefix sum at j counts the rows that reach column j
  for (int i = 0; i < nF; i++) { delta[P.first[i]]++; delta[i]--; }
  int64_t reach = 0;
  for (int j = 0; j < nF; j++) { reach += delta[j]; P.colStart[j + 1] = P.colStart[j] + reach; }
  P.colRows.resize((size_t)P.colStart[nF]);
  P.colBlk.resize((size_t)P.colStart[nF]);
  std::vector<int64_t> cursor(P.colStart.begin(), P.colStart.end() - 1);
  for (int i = 0; i < nF; i++)   // rows ascending, so every column's list comes out ascending
    for (int j = P.first[i]; j < i; j++) {
      P.colBlk[(size_t)cursor[j]] = P.rowOff[i] + (j - P.first[i]);
      P.colRows[(size_t)cursor[j]++] = i;
    }
}

// An envelope of B x B blocks ([r][c] row-major, block (i, j) of positions j <= i at B B (rowOff[i] + j - first[i])) against the dense
// symmetric M ([N][N], N = B nF) in the caller's numbering.  expandEnvelope clears M and writes every stored block with its mirror
// image; of a diagonal block it copies either what is stored or the lower triangle, mirrored.  packEnvelope reads the blocks back out
// of M, whole.
enum DiagBlock { kDiagWhole, kDiagLower };
template <int B> void expandEnvelope(const Plan& P, const double* env, double* M, DiagBlock diag) {
  const size_t N = (size_t)B * P.nF;
  std::fill(M, M + N * N, 0.0);
  for (int i = 0; i < P.nF; i++)
    for (int j = P.first[i]; j <= i; j++) {
      const double* blk = env + B * B * (size_t)(P.rowOff[i] + (j - P.first[i]));
      const size_t a = (size_t)B * P.perm[i], o = (size_t)B * P.perm[j];
      for (int r = 0; r < B; r++)
        for (int c = 0; c < B; c++) {
          if (i == j && c > r && diag == kDiagLower) continue;
          M[(a + r) * N + o + c] = blk[B * r + c];
          if (i != j || diag == kDiagLower) M[(o + c) * N + a + r] = blk[B * r + c];
        }
    }
}
template <int B> void packEnvelope(const Plan& P, const double* M, double* env) {
  const size_t N = (size_t)B * P.nF;
  for (int i = 0; i < P.nF; i++)
    for (int j = P.first[i]; j <= i; j++) {
      double* blk = env + B * B * (size_t)(P.rowOff[i] + (j - P.first[i]));
      for (int r = 0; r < B; r++)
        for (int c = 0; c < B; c++) blk[B * r + c] = M[((size_t)B * P.perm[i] + r) * N + (size_t)B * P.perm[j] + c];
    }
}

}  // namespace sky
}  // namespace ydorb
