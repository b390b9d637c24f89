// TEST ORACLE — not part of the product path.  Built by tests/sim3_support.py with oracle/Makefile's flags.
//
// Dependency-free CPU restatement of the loop-closure Sim3 check of ORB-SLAM2 (which YDORBSLAM renames):
//   Sim3Solver (src/Sim3Solver.cc): setRansacParameters, iterate, ComputeSim3 (Horn 1987), CheckInliers, Project
//   Optimizer::OptimizeSim3 (src/Optimizer.cc) over g2o's VertexSim3Expmap (types/sim3.h exp map, types_seven_dof_expmap.h edges),
//   BaseBinaryEdge's central-difference linearizeOplus (delta 1e-9), Huber, and the Levenberg-Marquardt trial loop
//   (core/optimization_algorithm_levenberg.cpp).
// The RANSAC follows the fp32 contract written in DESIGN.md section 2 ("Sim3 RANSAC"): only +, -, *, / and sqrt in a fixed order, so
// the GPU result must match this file bit for bit.  The LM is fp64 with libm transcendentals and matches the GPU to a tolerance.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

namespace {

// ---------------------------------------------------------------------------------------------------------------- RANSAC (fp32)
inline float dot3f(const float* a, const float* b) {   // cv::Mat float products: each product exact in double, summed in double
  return (float)(((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2]);
}

// T = [sR (3x3 row-major) | t]
struct Tf { float A[9], t[3]; };

struct Hyp { float R[9], t[3], s; Tf T12, T21; };

void horn(const float* X1, const float* X2, const int* idx, bool fixScale, Hyp& h) {
  float P1[3][3], P2[3][3];   // [coordinate][point]: the reference's 3x3 cv::Mat of column points
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) { P1[r][c] = X1[3 * idx[c] + r]; P2[r][c] = X2[3 * idx[c] + r]; }
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
  for (int r = 0; r < 3; r++) {
    O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) / 3.0f;
    O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) / 3.0f;
    for (int c = 0; c < 3; c++) { Pr1[r][c] = P1[r][c] - O1[r]; Pr2[r][c] = P2[r][c] - O2[r]; }
  }
  float M[3][3];   // M = Pr2 * Pr1^T
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) M[i][j] = dot3f(Pr2[i], Pr1[j]);
  float A[4][4];
  A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
  A[0][1] = M[1][2] - M[2][1];
  A[0][2] = M[2][0] - M[0][2];
  A[0][3] = M[0][1] - M[1][0];
  A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
  A[1][2] = M[0][1] + M[1][0];
  A[1][3] = M[2][0] + M[0][2];
  A[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
  A[2][3] = M[1][2] + M[2][1];
  A[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < i; j++) A[i][j] = A[j][i];
  // cyclic Jacobi, 8 sweeps of the 6 (p, q) pairs in order, every rotation applied even when tiny
  float V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 8; sweep++)
    for (int p = 0; p < 3; p++)
      for (int q = p + 1; q < 4; q++) {
        const float apq = A[p][q];
        if (apq == 0.0f) continue;
        const float theta = (A[q][q] - A[p][p]) / (2.0f * apq);
        float t = 1.0f / (std::fabs(theta) + std::sqrt(theta * theta + 1.0f));
        if (theta < 0.0f) t = -t;
        const float c = 1.0f / std::sqrt(t * t + 1.0f), s = t * c;
        for (int k = 0; k < 4; k++) {
          const float akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; k++) {
          const float apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; k++) {
          const float vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  int im = 0;
  for (int i = 1; i < 4; i++) if (A[i][i] > A[im][im]) im = i;
  float w = V[0][im], x = V[1][im], y = V[2][im], z = V[3][im];
  if (w < 0.0f) { w = -w; x = -x; y = -y; z = -z; }
  const float n = std::sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / n; x = x / n; y = y / n; z = z / n;
  float* R = h.R;
  R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - w * z); R[2] = 2.0f * (x * z + w * y);
  R[3] = 2.0f * (x * y + w * z); R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - w * x);
  R[6] = 2.0f * (x * z - w * y); R[7] = 2.0f * (y * z + w * x); R[8] = 1.0f - 2.0f * (x * x + y * y);
  float P3[3][3];   // R * Pr2
  for (int i = 0; i < 3; i++)
    for (int c = 0; c < 3; c++) { const float col[3] = {Pr2[0][c], Pr2[1][c], Pr2[2][c]}; P3[i][c] = dot3f(R + 3 * i, col); }
  float s = 1.0f;
  if (!fixScale) {
    double nom = 0, den = 0;
    for (int i = 0; i < 3; i++)
      for (int c = 0; c < 3; c++) { nom += (double)Pr1[i][c] * (double)P3[i][c]; den += (double)(P3[i][c] * P3[i][c]); }
    s = (float)(nom / den);
  }
  h.s = s;
  for (int i = 0; i < 3; i++) h.t[i] = O1[i] - s * dot3f(R + 3 * i, O2);
  for (int k = 0; k < 9; k++) h.T12.A[k] = s * R[k];
  for (int i = 0; i < 3; i++) h.T12.t[i] = h.t[i];
  const double inv = 1.0 / (double)s;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) h.T21.A[3 * i + j] = (float)(inv * (double)R[3 * j + i]);
  for (int i = 0; i < 3; i++) h.T21.t[i] = -dot3f(h.T21.A + 3 * i, h.t);
}

inline float reproj(const Tf& T, const float* X, const float* K, const float* P) {
  const float c0 = dot3f(T.A, X) + T.t[0], c1 = dot3f(T.A + 3, X) + T.t[1], c2 = dot3f(T.A + 6, X) + T.t[2];
  const float invz = 1.0f / c2;
  const float u = K[0] * (c0 * invz) + K[2], v = K[1] * (c1 * invz) + K[3];
  const float d0 = P[0] - u, d1 = P[1] - v;
  return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}

struct Prob {
  int N, fix, minInl, maxIts;
  const float *X1, *X2, *P1, *P2, *me1, *me2, *K1, *K2;
};

int checkInliers(const Prob& p, const Hyp& h, uint8_t* mask) {
  int n = 0;
  for (int i = 0; i < p.N; i++) {
    const float e1 = reproj(h.T12, p.X2 + 3 * i, p.K1, p.P1 + 2 * i);
    const float e2 = reproj(h.T21, p.X1 + 3 * i, p.K2, p.P2 + 2 * i);
    const bool in = e1 < p.me1[i] && e2 < p.me2[i];
    if (mask) mask[i] = in;
    n += in;
  }
  return n;
}

// ------------------------------------------------------------------------------------------------------------------ Sim3 LM (fp64)
struct V3 { double x, y, z; };
struct Q4 { double x, y, z, w; };
struct S3 { Q4 r; V3 t; double s; };

inline V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline V3 scl(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline V3 qrot(Q4 q, V3 v) {   // Eigen quaternion * vector
  V3 qv{q.x, q.y, q.z};
  V3 uv = cross(qv, v);
  uv = add(uv, uv);
  return add(add(v, scl(uv, q.w)), cross(qv, uv));
}
inline Q4 qmul(Q4 a, Q4 b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
          a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
Q4 rToQ(const double a[3][3]) {   // Eigen Quaternion(Matrix3)
  Q4 q;
  double t = a[0][0] + a[1][1] + a[2][2];
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (a[2][1] - a[1][2]) * t; q.y = (a[0][2] - a[2][0]) * t; q.z = (a[1][0] - a[0][1]) * t;
  } else {
    int i = 0;
    if (a[1][1] > a[0][0]) i = 1;
    if (a[2][2] > a[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(a[i][i] - a[j][j] - a[k][k] + 1.0);
    double c[3];
    c[i] = 0.5 * t;
    t = 0.5 / t;
    q.w = (a[k][j] - a[j][k]) * t;
    c[j] = (a[j][i] + a[i][j]) * t;
    c[k] = (a[k][i] + a[i][k]) * t;
    q.x = c[0]; q.y = c[1]; q.z = c[2];
  }
  return q;
}
// g2o Sim3(const Vector7d& update): omega, upsilon, sigma and the A, B, C branches of sim3.h
S3 sim3Exp(const double* u) {
  const double ox = u[0], oy = u[1], oz = u[2], sigma = u[6];
  const double theta = std::sqrt(ox * ox + oy * oy + oz * oz);
  const double Om[3][3] = {{0, -oz, oy}, {oz, 0, -ox}, {-oy, ox, 0}};
  double Om2[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) Om2[a][b] = Om[a][0] * Om[0][b] + Om[a][1] * Om[1][b] + Om[a][2] * Om[2][b];
  const double s = std::exp(sigma), eps = 0.00001;
  double A, B, C, ca, cb;
  const bool small = theta < eps;
  if (small) { ca = 1; cb = 1; }
  else { ca = std::sin(theta) / theta; cb = (1 - std::cos(theta)) / (theta * theta); }
  if (std::fabs(sigma) < eps) {
    C = 1;
    if (small) { A = 1. / 2.; B = 1. / 6.; }
    else { const double th2 = theta * theta; A = (1 - std::cos(theta)) / th2; B = (theta - std::sin(theta)) / (th2 * theta); }
  } else {
    C = (s - 1) / sigma;
    if (small) {
      const double sg2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sg2;
      B = ((0.5 * sg2 - sigma + 1) * s) / (sg2 * sigma);
    } else {
      const double a = s * std::sin(theta), b = s * std::cos(theta), th2 = theta * theta, sg2 = sigma * sigma, c = th2 + sg2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / th2;
    }
  }
  double Rm[3][3], W[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      const double I = a == b ? 1.0 : 0.0;
      Rm[a][b] = (I + ca * Om[a][b]) + cb * Om2[a][b];
      W[a][b] = (A * Om[a][b] + B * Om2[a][b]) + C * I;
    }
  S3 r;
  r.r = rToQ(Rm);
  r.t = {W[0][0] * u[3] + W[0][1] * u[4] + W[0][2] * u[5], W[1][0] * u[3] + W[1][1] * u[4] + W[1][2] * u[5],
         W[2][0] * u[3] + W[2][1] * u[4] + W[2][2] * u[5]};
  r.s = s;
  return r;
}
inline S3 compose(const S3& a, const S3& b) { return {qmul(a.r, b.r), add(scl(qrot(a.r, b.t), a.s), a.t), a.s * b.s}; }
inline S3 inverse(const S3& a) {
  const Q4 rc{-a.r.x, -a.r.y, -a.r.z, a.r.w};
  return {rc, qrot(rc, scl(a.t, -1. / a.s)), 1. / a.s};
}
inline void projErr(const S3& S, const double* X, const double* K, const double* obs, double* e) {
  const V3 p = add(scl(qrot(S.r, V3{X[0], X[1], X[2]}), S.s), S.t);
  e[0] = obs[0] - ((p.x / p.z) * K[0] + K[2]);
  e[1] = obs[1] - ((p.y / p.z) * K[1] + K[3]);
}
inline void huber(double e, double delta, double* rho0, double* rho1) {
  const double dsqr = delta * delta;
  if (e <= dsqr) { *rho0 = e; *rho1 = 1.; }
  else { const double s = std::sqrt(e); *rho0 = 2 * s * delta - dsqr; *rho1 = delta / s; }
}
inline double chi2(const double* e, double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

bool solve7(const double (&Hs)[28], double lambda, const double (&b)[7], double (&x)[7]) {   // LL^T, false if not positive definite
  double L[7][7];
  int k = 0;
  for (int r = 0; r < 7; r++)
    for (int c = r; c < 7; c++, k++) L[c][r] = Hs[k] + (r == c ? lambda : 0.0);
  for (int j = 0; j < 7; j++) {
    double d = L[j][j];
    for (int q = 0; q < j; q++) d -= L[j][q] * L[j][q];
    if (!(d > 0)) return false;
    d = std::sqrt(d);
    L[j][j] = d;
    for (int i = j + 1; i < 7; i++) {
      double s2 = L[i][j];
      for (int q = 0; q < j; q++) s2 -= L[i][q] * L[j][q];
      L[i][j] = s2 / d;
    }
  }
  for (int i = 0; i < 7; i++) {
    double s2 = b[i];
    for (int q = 0; q < i; q++) s2 -= L[i][q] * x[q];
    x[i] = s2 / L[i][i];
  }
  for (int i = 6; i >= 0; i--) {
    double s2 = x[i];
    for (int q = i + 1; q < 7; q++) s2 -= L[q][i] * x[q];
    x[i] = s2 / L[i][i];
  }
  return true;
}

struct Opt {
  int E;
  const double *X1, *X2, *o1, *o2, *w1, *w2, *K1, *K2;
  bool fix;
  double delta;
  uint8_t* active;   // 1 = pair in the graph
  double* err;       // [E][4] last computed e12, e21 (g2o's _error)
  int trials;
};

S3 oplus(const S3& S, const double* x, bool fix) {
  double u[7];
  for (int k = 0; k < 7; k++) u[k] = x[k];
  if (fix) u[6] = 0;
  return compose(sim3Exp(u), S);
}
double robustChi(Opt& o, const S3& S) {   // computeActiveErrors + activeRobustChi2
  const S3 Si = inverse(S);
  double chi = 0;
  for (int i = 0; i < o.E; i++) {
    if (!o.active[i]) continue;
    double* e = o.err + 4 * i;
    projErr(S, o.X2 + 3 * i, o.K1, o.o1 + 2 * i, e);
    projErr(Si, o.X1 + 3 * i, o.K2, o.o2 + 2 * i, e + 2);
    double r0, r1;
    huber(chi2(e, o.w1[i]), o.delta, &r0, &r1); chi += r0;
    huber(chi2(e + 2, o.w2[i]), o.delta, &r0, &r1); chi += r0;
  }
  return chi;
}
// optimize(iters): returns the robust chi2 after the last iteration (g2o's currentChi)
double optimize(Opt& o, S3& S, int iters) {
  const double dlt = 1e-9, scalar = 1.0 / (2 * dlt);
  double lambda = 0, ni = 2, currentChi = 0;
  for (int it = 0; it < iters; it++) {
    currentChi = robustChi(o, S);
    // the 14 perturbed estimates of the numeric Jacobian, and their inverses
    S3 Sp[7][2], Sip[7][2];
    for (int d = 0; d < 7; d++)
      for (int sg = 0; sg < 2; sg++) {
        double u[7] = {0, 0, 0, 0, 0, 0, 0};
        u[d] = sg ? -dlt : dlt;
        Sp[d][sg] = oplus(S, u, o.fix);
        Sip[d][sg] = inverse(Sp[d][sg]);
      }
    double Hs[28] = {0}, b[7] = {0};
    for (int i = 0; i < o.E; i++) {
      if (!o.active[i]) continue;
      for (int side = 0; side < 2; side++) {
        const double* e = o.err + 4 * i + 2 * side;
        const double w = side ? o.w2[i] : o.w1[i];
        double J[2][7];
        for (int d = 0; d < 7; d++) {
          double ep[2], em[2];
          if (side == 0) { projErr(Sp[d][0], o.X2 + 3 * i, o.K1, o.o1 + 2 * i, ep); projErr(Sp[d][1], o.X2 + 3 * i, o.K1, o.o1 + 2 * i, em); }
          else { projErr(Sip[d][0], o.X1 + 3 * i, o.K2, o.o2 + 2 * i, ep); projErr(Sip[d][1], o.X1 + 3 * i, o.K2, o.o2 + 2 * i, em); }
          J[0][d] = scalar * (ep[0] - em[0]);
          J[1][d] = scalar * (ep[1] - em[1]);
        }
        double r0, r1;
        huber(chi2(e, w), o.delta, &r0, &r1);
        const double W = r1 * w, om0 = -(w * e[0]) * r1, om1 = -(w * e[1]) * r1;
        int k = 0;
        for (int r = 0; r < 7; r++)
          for (int c = r; c < 7; c++, k++) Hs[k] += J[0][r] * W * J[0][c] + J[1][r] * W * J[1][c];
        for (int r = 0; r < 7; r++) b[r] += J[0][r] * om0 + J[1][r] * om1;
      }
    }
    if (it == 0) {   // computeLambdaInit
      double mx = 0;
      int k = 0;
      for (int r = 0; r < 7; r++) { mx = std::fmax(std::fabs(Hs[k]), mx); k += 7 - r; }
      lambda = 1e-5 * mx; ni = 2;
    }
    double rho = 0, x[7] = {0, 0, 0, 0, 0, 0, 0};
    int qmax = 0;
    do {
      const S3 Sb = S;
      const bool ok = solve7(Hs, lambda, b, x);
      S = oplus(S, x, o.fix);   // g2o applies _x even after a failed solve
      double tempChi = robustChi(o, S);
      if (!ok) tempChi = std::numeric_limits<double>::max();
      rho = currentChi - tempChi;
      double sc = 1e-3;
      for (int j = 0; j < 7; j++) sc += x[j] * (lambda * x[j] + b[j]);
      rho /= sc;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - std::pow((2 * rho - 1), 3.0);
        alpha = std::fmin(alpha, 2. / 3.);
        lambda *= std::fmax(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
      } else {
        lambda *= ni; ni *= 2;
        S = Sb;
        if (!std::isfinite(lambda)) { qmax++; o.trials++; break; }
      }
      qmax++; o.trials++;
    } while (rho < 0 && qmax < 10);
    if (qmax == 10 || rho == 0 || !std::isfinite(lambda)) break;
  }
  return currentChi;
}

}  // namespace

extern "C" {

// setRansacParameters' iteration count
int sim3ref_ransac_its(int N, double probability, int minInliers, int maxIterations) {
  const float epsilon = (float)minInliers / N;
  int nIterations;
  if (minInliers == N) nIterations = 1;
  else {
    const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
    nIterations = std::isfinite(v) && std::fabs(v) < 2147483647.0 ? (int)v : std::numeric_limits<int>::min();   // x86's conversion of NaN / overflow
  }
  return std::max(1, std::min(nIterations, maxIterations));
}

// g2o's Sim3(update) as [qx qy qz qw tx ty tz s]
void sim3ref_exp(const double* u, double* out) {
  const S3 r = sim3Exp(u);
  const double v[8] = {r.r.x, r.r.y, r.r.z, r.r.w, r.t.x, r.t.y, r.t.z, r.s};
  for (int k = 0; k < 8; k++) out[k] = v[k];
}

// ComputeSim3 of one triple: R [9], t [3], s, T12 [12], T21 [12]
void sim3ref_horn(const float* X1, const float* X2, const int* idx, int fixScale, float* out) {
  Hyp h;
  horn(X1, X2, idx, fixScale != 0, h);
  std::memcpy(out, h.R, 9 * 4); std::memcpy(out + 9, h.t, 3 * 4); out[12] = h.s;
  std::memcpy(out + 13, h.T12.A, 9 * 4); std::memcpy(out + 22, h.T12.t, 3 * 4);
  std::memcpy(out + 25, h.T21.A, 9 * 4); std::memcpy(out + 34, h.T21.t, 3 * 4);
}

// the reference's rotation: ang = atan2(|v|, w), Rodrigues(2 ang v / |v|), as cv::Rodrigues evaluates it (double inside, float out)
void sim3ref_rodrigues(const float* q /* w x y z */, float* R) {
  const float vn = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float ang = std::atan2(vn, q[0]);
  float r[3];
  for (int k = 0; k < 3; k++) r[k] = q[k + 1] * (2 * ang) / vn;
  const double rx = r[0], ry = r[1], rz = r[2], th = std::sqrt(rx * rx + ry * ry + rz * rz);
  const double c = std::cos(th), s = std::sin(th), c1 = 1. - c, it = th ? 1. / th : 0.;
  const double x = rx * it, y = ry * it, z = rz * it;
  const double M[9] = {c + c1 * x * x, c1 * x * y - s * z, c1 * x * z + s * y, c1 * x * y + s * z, c + c1 * y * y, c1 * y * z - s * x,
                       c1 * x * z - s * y, c1 * y * z + s * x, c + c1 * z * z};
  for (int k = 0; k < 9; k++) R[k] = (float)M[k];
}

// iterate(chunk) called repeatedly, as LoopClosing::computeSim3 does, from state[0] = mnIterations, state[1] = mnBestInliers until
// a call returns, bNoMore is set, or the triples run out.  out = {ret hypothesis or -1, bNoMore, calls}.  best13 in/out.
void sim3ref_ransac(int N, const float* X1, const float* X2, const float* P1, const float* P2, const float* me1, const float* me2,
                    const float* K1, const float* K2, int fixScale, int minInliers, int maxIts, const int* triples, int nTriples, int chunk,
                    int* state, float* best13, int* out, uint8_t* inliers, int* hypCounts) {
  const Prob p{N, fixScale, minInliers, maxIts, X1, X2, P1, P2, me1, me2, K1, K2};
  for (int i = 0; i < N; i++) inliers[i] = 0;
  for (int k = 0; hypCounts && k < nTriples; k++) hypCounts[k] = -1;
  int& its = state[0];
  int& best = state[1];
  const int first = its;
  int used = 0, calls = 0;
  out[0] = -1;
  for (;;) {   // one iterate(chunk) per pass
    calls++;
    bool noMore = false;
    if (N < minInliers) { out[1] = 1; break; }
    int cur = 0, ret = -1;
    while (its < maxIts && cur < chunk && used < nTriples) {
      cur++; its++;
      const int* tri = triples + 3 * used;
      Hyp h;
      horn(X1, X2, tri, fixScale != 0, h);
      const int n = checkInliers(p, h, nullptr);
      if (hypCounts) hypCounts[used] = n;
      used++;
      if (n >= best) {
        best = n;
        std::memcpy(best13, h.R, 9 * 4); std::memcpy(best13 + 9, h.t, 3 * 4); best13[12] = h.s;
        if (n > minInliers) { checkInliers(p, h, inliers); ret = first + used - 1; break; }
      }
    }
    if (ret >= 0) { out[0] = ret; out[1] = 0; break; }
    if (its >= maxIts) noMore = true;
    out[1] = noMore;
    if (noMore || used >= nTriples) break;
  }
  out[2] = calls;
}

// OptimizeSim3 on one problem.  S12 = qx qy qz qw tx ty tz s (in/out), chi2[2], returns nIn
int sim3ref_optimize(int E, const double* X1c, const double* X2c, const double* obs1, const double* obs2, const double* w1, const double* w2,
                     const double* K1, const double* K2, int fixScale, double th2, double* S12, uint8_t* outlier, double* chi2log, int* trials) {
  const float th2f = (float)th2;
  const double thr = th2f, delta = (double)std::sqrt(th2f);
  chi2log[0] = chi2log[1] = std::numeric_limits<double>::quiet_NaN();
  *trials = 0;
  for (int i = 0; i < E; i++) outlier[i] = 0;
  if (E == 0) return 0;
  uint8_t* active = new uint8_t[E];
  double* err = new double[4 * E];
  for (int i = 0; i < E; i++) active[i] = 1;
  Opt o{E, X1c, X2c, obs1, obs2, w1, w2, K1, K2, fixScale != 0, delta, active, err, 0};
  S3 S{{S12[0], S12[1], S12[2], S12[3]}, {S12[4], S12[5], S12[6]}, S12[7]};
  chi2log[0] = optimize(o, S, 5);
  int nBad = 0;
  for (int i = 0; i < E; i++)
    if (chi2(err + 4 * i, w1[i]) > thr || chi2(err + 4 * i + 2, w2[i]) > thr) { active[i] = 0; outlier[i] = 1; nBad++; }
  const int nMore = nBad > 0 ? 10 : 5;
  int nIn = 0;
  if (E - nBad >= 10) {
    chi2log[1] = optimize(o, S, nMore);
    for (int i = 0; i < E; i++) {
      if (!active[i]) continue;
      if (chi2(err + 4 * i, w1[i]) > thr || chi2(err + 4 * i + 2, w2[i]) > thr) outlier[i] = 1;
      else nIn++;
    }
    S12[0] = S.r.x; S12[1] = S.r.y; S12[2] = S.r.z; S12[3] = S.r.w;
    S12[4] = S.t.x; S12[5] = S.t.y; S12[6] = S.t.z; S12[7] = S.s;
  }
  *trials = o.trials;
  delete[] active;
  delete[] err;
  return nIn;
}

}  // extern "C"
