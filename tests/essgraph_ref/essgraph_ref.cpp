// CPU restatement of the essential-graph optimisation (ydorb_essential_graph_optimize), independent of the product's headers.
// ORB-SLAM2 Optimizer::OptimizeEssentialGraph over g2o's VertexSim3Expmap / EdgeSim3 (types_seven_dof_expmap.h, sim3.h), the numeric
// Jacobians of BaseBinaryEdge::linearizeOplus (delta 1e-9), constructQuadraticForm, a dense LL^T and the trial loop of
// OptimizationAlgorithmLevenberg with a user lambda, in plain C++ under the contract of DESIGN.md section 2 ("Essential graph: the
// arithmetic contract").  Built with the oracle's flags (-ffp-contract=off).  The Sim3 algebra is a template on the scalar so that the
// error chain can also run in long double: the gap between the two is what sets the tolerances of the GPU tests (section 6i).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

template <class T> struct S3 { T q[4], t[3], s; };   // q = x y z w

template <class T> void qmul(const T* a, const T* b, T* o) {
  const T ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
  o[0] = aw * bx + ax * bw + ay * bz - az * by;
  o[1] = aw * by + ay * bw + az * bx - ax * bz;
  o[2] = aw * bz + az * bw + ax * by - ay * bx;
  o[3] = aw * bw - ax * bx - ay * by - az * bz;
}
template <class T> void qrot(const T* q, const T* v, T* o) {   // Eigen quaternion * vector
  T uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
  for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
  const T c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int k = 0; k < 3; k++) o[k] = (v[k] + uv[k] * q[3]) + c[k];
}
template <class T> void qToR(const T* q, T m[3][3]) {
  const T tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
  const T twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1],
          tzz = tz * q[2];
  m[0][0] = 1 - (tyy + tzz); m[0][1] = txy - twz; m[0][2] = txz + twy;
  m[1][0] = txy + twz; m[1][1] = 1 - (txx + tzz); m[1][2] = tyz - twx;
  m[2][0] = txz - twy; m[2][1] = tyz + twx; m[2][2] = 1 - (txx + tyy);
}
template <class T> void rToQ(const T a[3][3], T* q) {   // Eigen Quaternion(Matrix3)
  T t = a[0][0] + a[1][1] + a[2][2];
  if (t > 0) {
    t = std::sqrt(t + T(1));
    q[3] = T(0.5) * t;
    t = T(0.5) / t;
    q[0] = (a[2][1] - a[1][2]) * t; q[1] = (a[0][2] - a[2][0]) * t; q[2] = (a[1][0] - a[0][1]) * t;
  } else {
    int i = 0;
    if (a[1][1] > a[0][0]) i = 1;
    if (a[2][2] > a[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(a[i][i] - a[j][j] - a[k][k] + T(1));
    q[i] = T(0.5) * t;
    t = T(0.5) / t;
    q[3] = (a[k][j] - a[j][k]) * t;
    q[j] = (a[j][i] + a[i][j]) * t;
    q[k] = (a[k][i] + a[i][k]) * t;
  }
}

// Sim3(const Vector7d&): the exponential map
template <class T> S3<T> sim3Exp(const T* u) {
  const T ox = u[0], oy = u[1], oz = u[2], sigma = u[6];
  const T theta = std::sqrt(ox * ox + oy * oy + oz * oz);
  const T Om[3][3] = {{0, -oz, oy}, {oz, 0, -ox}, {-oy, ox, 0}};
  T Om2[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) Om2[a][b] = Om[a][0] * Om[0][b] + Om[a][1] * Om[1][b] + Om[a][2] * Om[2][b];
  const T s = std::exp(sigma), eps = T(0.00001);
  T A, B, C, ca, cb;
  const bool small = theta < eps;
  if (small) { ca = 1; cb = 1; }
  else { ca = std::sin(theta) / theta; cb = (1 - std::cos(theta)) / (theta * theta); }
  if (std::fabs(sigma) < eps) {
    C = 1;
    if (small) { A = T(1.) / T(2.); B = T(1.) / T(6.); }
    else { const T th2 = theta * theta; A = (1 - std::cos(theta)) / th2; B = (theta - std::sin(theta)) / (th2 * theta); }
  } else {
    C = (s - 1) / sigma;
    if (small) {
      const T sg2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sg2;
      B = ((T(0.5) * sg2 - sigma + 1) * s - 1) / (sg2 * sigma);   // with the - 1: DESIGN.md section 2
    } else {
      const T a = s * std::sin(theta), b = s * std::cos(theta), th2 = theta * theta, sg2 = sigma * sigma, c = th2 + sg2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * T(1.) / th2;
    }
  }
  T Rm[3][3], W[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      const T I = a == b ? T(1) : T(0);
      Rm[a][b] = (I + ca * Om[a][b]) + cb * Om2[a][b];
      W[a][b] = (A * Om[a][b] + B * Om2[a][b]) + C * I;
    }
  S3<T> r;
  rToQ(Rm, r.q);
  for (int a = 0; a < 3; a++) r.t[a] = W[a][0] * u[3] + W[a][1] * u[4] + W[a][2] * u[5];
  r.s = s;
  return r;
}
template <class T> S3<T> compose(const S3<T>& a, const S3<T>& b) {
  S3<T> r;
  qmul(a.q, b.q, r.q);
  T rt[3];
  qrot(a.q, b.t, rt);
  for (int k = 0; k < 3; k++) r.t[k] = rt[k] * a.s + a.t[k];
  r.s = a.s * b.s;
  return r;
}
template <class T> S3<T> inverse(const S3<T>& a) {
  S3<T> r;
  r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
  const T f = T(-1.) / a.s;
  const T v[3] = {a.t[0] * f, a.t[1] * f, a.t[2] * f};
  qrot(r.q, v, r.t);
  r.s = T(1.) / a.s;
  return r;
}
template <class T> S3<T> oplus(const S3<T>& S, const T* x, bool fix) {   // VertexSim3Expmap::oplusImpl
  T u[7];
  for (int k = 0; k < 7; k++) u[k] = x[k];
  if (fix) u[6] = 0;
  return compose(sim3Exp(u), S);
}
template <class T> void mapPoint(const S3<T>& S, const T* p, T* o) {
  T r[3];
  qrot(S.q, p, r);
  for (int k = 0; k < 3; k++) o[k] = r[k] * S.s + S.t[k];
}

// Sim3::log(); the 3x3 solve as Eigen's PartialPivLU
template <class T> void sim3Log(const S3<T>& S, T* res) {
  const T sigma = std::log(S.s), eps = T(0.00001);
  T Rm[3][3];
  qToR(S.q, Rm);
  const T d = T(0.5) * (Rm[0][0] + Rm[1][1] + Rm[2][2] - 1);
  const T dR[3] = {Rm[2][1] - Rm[1][2], Rm[0][2] - Rm[2][0], Rm[1][0] - Rm[0][1]};
  T om[3], A, B, C;
  if (std::fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) {
      for (int k = 0; k < 3; k++) om[k] = T(0.5) * dR[k];
      A = T(1.) / T(2.); B = T(1.) / T(6.);
    } else {
      const T theta = std::acos(d), th2 = theta * theta, f = theta / (2 * std::sqrt(1 - d * d));
      for (int k = 0; k < 3; k++) om[k] = f * dR[k];
      A = (1 - std::cos(theta)) / th2;
      B = (theta - std::sin(theta)) / (th2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (d > 1 - eps) {
      const T sg2 = sigma * sigma;
      for (int k = 0; k < 3; k++) om[k] = T(0.5) * dR[k];
      A = ((sigma - 1) * S.s + 1) / sg2;
      B = ((T(0.5) * sg2 - sigma + 1) * S.s - 1) / (sg2 * sigma);   // with the - 1: DESIGN.md section 2
    } else {
      const T theta = std::acos(d), f = theta / (2 * std::sqrt(1 - d * d));
      for (int k = 0; k < 3; k++) om[k] = f * dR[k];
      const T th2 = theta * theta, a = S.s * std::sin(theta), b = S.s * std::cos(theta), c = th2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) / th2;
    }
  }
  const T Om[3][3] = {{0, -om[2], om[1]}, {om[2], 0, -om[0]}, {-om[1], om[0], 0}};
  T W[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      const T o2 = Om[a][0] * Om[0][b] + Om[a][1] * Om[1][b] + Om[a][2] * Om[2][b];
      W[a][b] = (A * Om[a][b] + B * o2) + (a == b ? C : T(0));
    }
  T y[3] = {S.t[0], S.t[1], S.t[2]};
  for (int k = 0; k < 3; k++) {
    int piv = k;
    for (int r = k + 1; r < 3; r++)
      if (std::fabs(W[r][k]) > std::fabs(W[piv][k])) piv = r;
    if (piv != k) {
      for (int c = 0; c < 3; c++) { const T tmp = W[k][c]; W[k][c] = W[piv][c]; W[piv][c] = tmp; }
      const T tmp = y[k]; y[k] = y[piv]; y[piv] = tmp;
    }
    for (int r = k + 1; r < 3; r++) {
      W[r][k] = W[r][k] / W[k][k];
      for (int c = k + 1; c < 3; c++) W[r][c] -= W[r][k] * W[k][c];
    }
  }
  y[1] -= W[1][0] * y[0];
  y[2] -= W[2][0] * y[0]; y[2] -= W[2][1] * y[1];
  y[2] = y[2] / W[2][2];
  y[1] = (y[1] - W[1][2] * y[2]) / W[1][1];
  y[0] = ((y[0] - W[0][1] * y[1]) - W[0][2] * y[2]) / W[0][0];
  for (int k = 0; k < 3; k++) { res[k] = om[k]; res[3 + k] = y[k]; }
  res[6] = sigma;
}

template <class T> S3<T> load(const double* p) {
  S3<T> S;
  for (int k = 0; k < 4; k++) S.q[k] = T(p[k]);
  for (int k = 0; k < 3; k++) S.t[k] = T(p[4 + k]);
  S.s = T(p[7]);
  return S;
}
void store(const S3<double>& S, double* p) {
  for (int k = 0; k < 4; k++) p[k] = S.q[k];
  for (int k = 0; k < 3; k++) p[4 + k] = S.t[k];
  p[7] = S.s;
}

// EdgeSim3::computeError in T, rounded to double: log(C * v0 * v1^-1)
template <class T> void edgeError(const S3<T>& C, const S3<T>& Vi, const S3<T>& Vj, double* e) {
  T r[7];
  sim3Log(compose(compose(C, Vi), inverse(Vj)), r);
  for (int k = 0; k < 7; k++) e[k] = (double)r[k];
}
double dot7(const double* e) {
  double s = 0;
  for (int k = 0; k < 7; k++) s += e[k] * e[k];
  return s;
}

// computeError + linearizeOplus of one edge with the error chain (oplus and the error) in T; J[side][k][d], zero for a fixed vertex
template <class T> void linearizeEdge(const double* est, const uint8_t* fixed, int vi, int vj, const double* meas, bool fix, double* e, double* J) {
  const S3<T> C = load<T>(meas), Vi = load<T>(est + 8 * (size_t)vi), Vj = load<T>(est + 8 * (size_t)vj);
  edgeError(C, Vi, Vj, e);
  const double dlt = 1e-9, scalar = 1.0 / (2 * dlt);
  for (int side = 0; side < 2; side++)
    for (int d = 0; d < 7; d++) {
      double col[7] = {0, 0, 0, 0, 0, 0, 0};
      if (!fixed[side ? vj : vi]) {
        T u[7] = {0, 0, 0, 0, 0, 0, 0};
        double ep[7], em[7];
        u[d] = T(dlt);
        const S3<T> Pp = oplus(side ? Vj : Vi, u, fix);
        edgeError(C, side ? Vi : Pp, side ? Pp : Vj, ep);
        u[d] = T(-dlt);
        const S3<T> Pm = oplus(side ? Vj : Vi, u, fix);
        edgeError(C, side ? Vi : Pm, side ? Pm : Vj, em);
        for (int k = 0; k < 7; k++) col[k] = scalar * (ep[k] - em[k]);
      }
      for (int k = 0; k < 7; k++) J[49 * side + 7 * k + d] = col[k];
    }
}

struct Graph {
  int nV, nE, nF;
  const uint8_t* fixed;
  const int *v0, *v1;
  const double* meas;
  bool fix;
  std::vector<int> freeOf;
};

double chi2Of(const Graph& G, const double* est) {   // activeChi2: the edges in order
  double chi = 0;
  for (int e = 0; e < G.nE; e++) {
    double ev[7];
    edgeError(load<double>(G.meas + 8 * (size_t)e), load<double>(est + 8 * (size_t)G.v0[e]), load<double>(est + 8 * (size_t)G.v1[e]), ev);
    chi += dot7(ev);
  }
  return chi;
}

// buildSystem: H (lower and upper, [n][n]) and b from the edges in order
void build(const Graph& G, const double* est, std::vector<double>& H, std::vector<double>& b) {
  const int n = 7 * G.nF;
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
            H[(size_t)(7 * f[sa] + r) * n + 7 * f[sb] + c] += s;
            if (sa != sb) H[(size_t)(7 * f[sb] + c) * n + 7 * f[sa] + r] += s;
          }
      }
    }
  }
}

// LL^T of H + lambda I and both substitutions; false on a non-positive pivot (x is then left as it was).  Leading zeros of a row are
// skipped (they stay zero in the factor), which changes no bit of the result.
bool solveDense(const std::vector<double>& H, int n, double lambda, const std::vector<double>& b, std::vector<double>& x, std::vector<double>& L) {
  std::vector<int> first(n);
  for (int i = 0; i < n; i++) {
    int c = 0;
    while (c < i && H[(size_t)i * n + c] == 0) c++;
    first[i] = c;
  }
  for (int i = 0; i < n; i++) {
    for (int j = first[i]; j <= i; j++) {
      double s = H[(size_t)i * n + j] + (i == j ? lambda : 0.0);
      for (int q = std::max(first[i], first[j]); q < j; q++) s -= L[(size_t)i * n + q] * L[(size_t)j * n + q];
      if (i == j) {
        if (!(s > 0)) return false;
        L[(size_t)i * n + i] = std::sqrt(s);
      } else {
        L[(size_t)i * n + j] = s / L[(size_t)j * n + j];
      }
    }
  }
  std::vector<double> y(n);
  for (int i = 0; i < n; i++) {
    double s = b[i];
    for (int q = first[i]; q < i; q++) s -= L[(size_t)i * n + q] * y[q];
    y[i] = s / L[(size_t)i * n + i];
  }
  for (int i = n - 1; i >= 0; i--) {
    double s = y[i];
    for (int q = i + 1; q < n; q++)
      if (first[q] <= i) s -= L[(size_t)q * n + i] * y[q];
    y[i] = s / L[(size_t)i * n + i];
  }
  x = y;
  return true;
}

}  // namespace

extern "C" {

void essref_exp(const double* u, double* S8) { store(sim3Exp<double>(u), S8); }
void essref_log(const double* S8, double* u) { sim3Log(load<double>(S8), u); }
// which branches log() takes: bit 0 = |sigma| < 1e-5, bit 1 = d > 1 - 1e-5
int essref_log_branch(const double* S8) {
  const S3<double> S = load<double>(S8);
  double Rm[3][3];
  qToR(S.q, Rm);
  const double d = 0.5 * (Rm[0][0] + Rm[1][1] + Rm[2][2] - 1);
  return (std::fabs(std::log(S.s)) < 0.00001 ? 1 : 0) | (d > 1 - 0.00001 ? 2 : 0);
}
void essref_compose(const double* a, const double* b, double* o) { store(compose(load<double>(a), load<double>(b)), o); }
void essref_inverse(const double* a, double* o) { store(inverse(load<double>(a)), o); }

// err [E][7], J0 / J1 [E][7][7], chi2 [E]; long_double != 0: the error chain in long double
void essref_linearize(int nV, const double* est, const uint8_t* fixed, int nE, const int* v0, const int* v1, const double* meas, int fix_scale,
                      int long_double, double* err, double* J0, double* J1, double* chi2) {
  (void)nV;
  for (int e = 0; e < nE; e++) {
    double ev[7], J[98];
    if (long_double) linearizeEdge<long double>(est, fixed, v0[e], v1[e], meas + 8 * (size_t)e, fix_scale != 0, ev, J);
    else linearizeEdge<double>(est, fixed, v0[e], v1[e], meas + 8 * (size_t)e, fix_scale != 0, ev, J);
    std::memcpy(err + 7 * (size_t)e, ev, sizeof ev);
    std::memcpy(J0 + 49 * (size_t)e, J, 49 * sizeof(double));
    std::memcpy(J1 + 49 * (size_t)e, J + 49, 49 * sizeof(double));
    chi2[e] = dot7(ev);
  }
}

// The whole call.  sim3 in/out; counts = n_trials, n_iterations, n_log; logs hold 32 rows; pts_out_d: the corrected points before the
// rounding to float.  Returns 0, or -1 when the graph has no free or no fixed vertex.
int essref_optimize(int nV, double* sim3, const uint8_t* fixed, int nE, const int* v0, const int* v1, const double* meas, int fix_scale,
                    int iterations, int max_trials, double lambda_init, int nP, const float* pts, const int* pref, float* pts_out,
                    double* pts_out_d, double* log_chi2, double* log_lambda, int* log_trials, int* counts) {
  Graph G{nV, nE, 0, fixed, v0, v1, meas, fix_scale != 0, std::vector<int>(nV, -1)};
  for (int v = 0; v < nV; v++)
    if (!fixed[v]) G.freeOf[v] = G.nF++;
  if (G.nF == 0 || G.nF == nV) return -1;
  const int n = 7 * G.nF;
  std::vector<double> est(sim3, sim3 + 8 * (size_t)nV), est0 = est, backup, H((size_t)n * n), L((size_t)n * n), b(n), x(n, 0.0);
  counts[0] = counts[1] = counts[2] = 0;
  double lambda = 0, ni = 2;
  for (int it = 0; it < iterations; it++) {
    double currentChi = chi2Of(G, est.data());
    build(G, est.data(), H, b);
    if (it == 0) lambda = lambda_init;   // setUserLambdaInit
    double rho = 0;
    int qmax = 0;
    bool broke = false;
    do {
      backup = est;   // push
      const bool ok = solveDense(H, n, lambda, b, x, L);
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
        est = backup;   // pop
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

double essref_chi2(int nV, const double* est, int nE, const int* v0, const int* v1, const double* meas) {
  Graph G{nV, nE, 0, nullptr, v0, v1, meas, false, {}};
  return chi2Of(G, est);
}

}  // extern "C"
