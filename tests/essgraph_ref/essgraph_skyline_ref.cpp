// TEST-ONLY: essref_optimize (essgraph_ref.cpp) with H and its Cholesky factor stored as a scalar skyline in natural order - first[i],
// row pointers, contiguous rows from a row's first structural non-zero to the diagonal - so that its memory grows with the envelope
// and graphs above the dense solver's limit fit.  The operations and their order are solveDense's (which already skips a row's leading
// zeros), so below the limit essref_sky_optimize returns the bytes essref_optimize returns; tests/test_essgraph_skyline_cpu.py checks
// that.  The per-edge arithmetic is not restated a second time: the restatement's own translation unit is included, and its
// linearizeEdge / chi2Of / oplus / mapPoint are called.
#include "essgraph_ref.cpp"

namespace {

struct Skyline {
  int n = 0;
  std::vector<int> first;        // structural: the first column of row i's envelope
  std::vector<size_t> ptr;       // row i at ptr[i], entry (i, j) at ptr[i] + j - first[i]
  std::vector<size_t> colStart;  // column j: the rows i > j with first[i] <= j, ascending
  std::vector<int> colRows;
  double& at(std::vector<double>& M, int i, int j) const { return M[ptr[i] + (size_t)(j - first[i])]; }
  double at(const std::vector<double>& M, int i, int j) const { return M[ptr[i] + (size_t)(j - first[i])]; }
};

Skyline envelope(const Graph& G) {
  Skyline S;
  S.n = 7 * G.nF;
  std::vector<int> lowest(G.nF);
  for (int f = 0; f < G.nF; f++) lowest[f] = f;
  for (int e = 0; e < G.nE; e++) {
    const int a = G.freeOf[G.v0[e]], b = G.freeOf[G.v1[e]];
    if (a < 0 || b < 0) continue;
    lowest[std::max(a, b)] = std::min(lowest[std::max(a, b)], std::min(a, b));
  }
  S.first.resize(S.n); S.ptr.assign(S.n + 1, 0);
  for (int i = 0; i < S.n; i++) { S.first[i] = 7 * lowest[i / 7]; S.ptr[i + 1] = S.ptr[i] + (size_t)(i - S.first[i] + 1); }
  S.colStart.assign(S.n + 1, 0);
  for (int i = 0; i < S.n; i++)
    for (int j = S.first[i]; j < i; j++) S.colStart[j + 1]++;
  for (int j = 0; j < S.n; j++) S.colStart[j + 1] += S.colStart[j];
  S.colRows.resize(S.colStart[S.n]);
  std::vector<size_t> cursor(S.colStart.begin(), S.colStart.end() - 1);
  for (int i = 0; i < S.n; i++)
    for (int j = S.first[i]; j < i; j++) S.colRows[cursor[j]++] = i;
  return S;
}

// build(): the lower triangle of H into the skyline, b; the edges in order, every sum as there
void buildSky(const Graph& G, const Skyline& S, const double* est, std::vector<double>& H, std::vector<double>& b) {
  std::fill(H.begin(), H.end(), 0.0);
  std::fill(b.begin(), b.end(), 0.0);
  for (int e = 0; e < G.nE; e++) {
    double ev[7], J[98];
    linearizeEdge<double>(est, G.fixed, G.v0[e], G.v1[e], G.meas + 8 * (size_t)e, G.fix, ev, J);
    const int f[2] = {G.freeOf[G.v0[e]], G.freeOf[G.v1[e]]};
    for (int sa = 0; sa < 2; sa++) {
      if (f[sa] < 0) continue;
      for (int r = 0; r < 7; r++) {
        double s = 0;
        for (int k = 0; k < 7; k++) s += J[49 * sa + 7 * k + r] * (-ev[k]);
        b[7 * f[sa] + r] += s;
      }
      for (int sb = sa; sb < 2; sb++) {
        if (f[sb] < 0) continue;
        for (int r = 0; r < 7; r++)
          for (int c = 0; c < 7; c++) {
            double s = 0;
            for (int k = 0; k < 7; k++) s += J[49 * sa + 7 * k + r] * J[49 * sb + 7 * k + c];
            const int row = 7 * f[sa] + r, col = 7 * f[sb] + c;
            if (sa == sb) { if (col <= row) S.at(H, row, col) += s; }
            else if (row > col) S.at(H, row, col) += s;
            else S.at(H, col, row) += s;
          }
      }
    }
  }
}

// solveDense over the skyline: the same first[] (the first numerical non-zero of a row), the same sums in the same order
bool solveSky(const Skyline& S, const std::vector<double>& H, double lambda, const std::vector<double>& b, std::vector<double>& x, std::vector<double>& L) {
  const int n = S.n;
  std::vector<int> first(n);
  for (int i = 0; i < n; i++) {
    int c = S.first[i];
    while (c < i && S.at(H, i, c) == 0) c++;
    first[i] = c;
  }
  for (int i = 0; i < n; i++) {
    for (int j = S.first[i]; j < first[i]; j++) S.at(L, i, j) = 0.0;
    for (int j = first[i]; j <= i; j++) {
      double s = S.at(H, i, j) + (i == j ? lambda : 0.0);
      for (int q = std::max(first[i], first[j]); q < j; q++) s -= S.at(L, i, q) * S.at(L, j, q);
      if (i == j) {
        if (!(s > 0)) return false;
        S.at(L, i, i) = std::sqrt(s);
      } else {
        S.at(L, i, j) = s / S.at(L, j, j);
      }
    }
  }
  std::vector<double> y(n);
  for (int i = 0; i < n; i++) {
    double s = b[i];
    for (int q = first[i]; q < i; q++) s -= S.at(L, i, q) * y[q];
    y[i] = s / S.at(L, i, i);
  }
  for (int i = n - 1; i >= 0; i--) {
    double s = y[i];
    for (size_t p = S.colStart[i]; p < S.colStart[i + 1]; p++) {
      const int q = S.colRows[p];
      if (first[q] <= i) s -= S.at(L, q, i) * y[q];
    }
    y[i] = s / S.at(L, i, i);
  }
  x = y;
  return true;
}

}  // namespace

extern "C" {

// essref_optimize's arguments and results; in addition sizes[0] = the skyline's entries (doubles held for H, and again for L)
int essref_sky_optimize(int nV, double* sim3, const uint8_t* fixed, int nE, const int* v0, const int* v1, const double* meas, int fix_scale,
                        int iterations, int max_trials, double lambda_init, int nP, const float* pts, const int* pref, float* pts_out,
                        double* pts_out_d, double* log_chi2, double* log_lambda, int* log_trials, int* counts, long long* sizes) {
  Graph G{nV, nE, 0, fixed, v0, v1, meas, fix_scale != 0, std::vector<int>(nV, -1)};
  for (int v = 0; v < nV; v++)
    if (!fixed[v]) G.freeOf[v] = G.nF++;
  if (G.nF == 0 || G.nF == nV) return -1;
  const int n = 7 * G.nF;
  const Skyline S = envelope(G);
  if (sizes) sizes[0] = (long long)S.ptr[n];
  std::vector<double> est(sim3, sim3 + 8 * (size_t)nV), est0 = est, backup, H(S.ptr[n]), L(S.ptr[n]), b(n), x(n, 0.0);
  counts[0] = counts[1] = counts[2] = 0;
  double lambda = 0, ni = 2;
  for (int it = 0; it < iterations; it++) {
    double currentChi = chi2Of(G, est.data());
    buildSky(G, S, est.data(), H, b);
    if (it == 0) lambda = lambda_init;
    double rho = 0;
    int qmax = 0;
    bool broke = false;
    do {
      backup = est;
      const bool ok = solveSky(S, H, lambda, b, x, L);
      for (int v = 0; v < nV; v++)
        if (G.freeOf[v] >= 0) store(oplus(load<double>(est.data() + 8 * (size_t)v), x.data() + 7 * G.freeOf[v], G.fix), est.data() + 8 * (size_t)v);
      double tempChi = chi2Of(G, est.data());
      if (!ok) tempChi = 1.7976931348623157e308;
      double scale = 0;
      for (int j = 0; j < n; j++) scale += x[j] * (lambda * x[j] + b[j]);
      scale += 1e-3;
      rho = (currentChi - tempChi) / scale;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - std::pow(2 * rho - 1, 3);
        alpha = std::fmin(alpha, 2. / 3.);
        lambda *= std::fmax(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
      } else {
        lambda *= ni; ni *= 2;
        est = backup;
        if (!std::isfinite(lambda)) broke = true;
      }
      qmax++; counts[0]++;
    } while (!broke && rho < 0 && qmax < max_trials);
    if (counts[2] < 32) { log_chi2[counts[2]] = currentChi; log_lambda[counts[2]] = lambda; log_trials[counts[2]] = qmax; counts[2]++; }
    counts[1]++;
    if (qmax == max_trials || rho == 0 || !std::isfinite(lambda)) break;
  }
  std::memcpy(sim3, est.data(), sizeof(double) * 8 * (size_t)nV);
  for (int p = 0; p < nP; p++) {
    const double X[3] = {(double)pts[3 * p], (double)pts[3 * p + 1], (double)pts[3 * p + 2]};
    double c[3], w[3];
    mapPoint(load<double>(est0.data() + 8 * (size_t)pref[p]), X, c);
    mapPoint(inverse(load<double>(est.data() + 8 * (size_t)pref[p])), c, w);
    for (int k = 0; k < 3; k++) { pts_out_d[3 * p + k] = w[k]; pts_out[3 * p + k] = (float)w[k]; }
  }
  return 0;
}

}  // extern "C"
