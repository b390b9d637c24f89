// TEST ORACLE — not part of the product path.  Built by tests/pnp_support.py with oracle/Makefile's flags.
//
// Dependency-free CPU restatement of the relocalisation EPnP RANSAC of ORB-SLAM2 (which YDORBSLAM renames to pnpSolver.*):
//   PnPsolver (src/PnPsolver.cc): SetRansacParameters, iterate, Refine, CheckInliers, and Lepetit's EPnP (compute_pose,
//   choose_control_points, compute_barycentric_coordinates, fill_M, compute_L_6x10, compute_rho, find_betas_approx_1/2/3,
//   gauss_newton, qr_solve, compute_R_and_t, solve_for_sign, estimate_R_and_t, reprojection_error).
// OpenCV's cvMulTransposed / cvSVD / cvInvert / cvSolve are replaced by the written-order double arithmetic of DESIGN.md section 2
// ("EPnP RANSAC"): only +, -, *, / and sqrt, every operation a single IEEE double operation, so the GPU must match this file bit for
// bit.  Every loop has a fixed upper bound; NaN / inf input runs through to a NaN pose that counts no inlier.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int kSymSweeps = 16;     // cyclic Jacobi sweeps (12x12 and 3x3 symmetric)
constexpr int kSvdSweeps = 16;     // one-sided Jacobi sweeps (6xk and 3x3)
constexpr double kSvdTol = 1e-15;  // one-sided Jacobi: skip a pair when |gamma| <= tol * sqrt(alpha * beta)
constexpr double kEps = 2.220446049250313e-16;

// Symmetric cyclic Jacobi on A (n x n, row-major, n <= 12).  Out: d[k] = |eigenvalue| sorted descending (ties keep the lower index),
// ut rows = the matching eigenvectors, each signed so that its largest-magnitude component (first on ties) is positive.
void jacobiSym(int n, double* A, double* d, double* ut) {
  double V[144];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kSymSweeps; sweep++) {
    int rotated = 0;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = A[p * n + q], app = A[p * n + p], aqq = A[q * n + q];
        const double g = 100.0 * fabs(apq);
        if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) continue;   // negligible against both diagonals
        rotated = 1;
        const double theta = (aqq - app) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; k++) {   // columns p, q
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {   // rows p, q
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; k++) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
    if (!rotated) break;
  }
  int order[12];
  double ev[12];
  for (int i = 0; i < n; i++) { order[i] = i; ev[i] = fabs(A[i * n + i]); }
  for (int i = 0; i < n; i++) {   // selection sort, descending; strict > keeps the first of equal values
    int m = i;
    for (int j = i + 1; j < n; j++)
      if (ev[j] > ev[m]) m = j;
    const double tv = ev[i]; ev[i] = ev[m]; ev[m] = tv;
    const int to = order[i]; order[i] = order[m]; order[m] = to;
  }
  for (int i = 0; i < n; i++) {
    d[i] = ev[i];
    const int c = order[i];
    int big = 0;
    for (int k = 1; k < n; k++)
      if (fabs(V[k * n + c]) > fabs(V[big * n + c])) big = k;
    const bool neg = V[big * n + c] < 0.0;
    for (int k = 0; k < n; k++) ut[i * n + k] = neg ? -V[k * n + c] : V[k * n + c];
  }
}

// One-sided (Hestenes) Jacobi SVD of A (m x k row-major, m <= 12, k <= 5): A = U diag(w) V^T.  A is overwritten by A V; w sorted
// descending (ties keep the lower index); U[:, j] = (A V)[:, j] / w[j] (0 where w[j] == 0); V [k x k] row-major.
void svdOneSided(int m, int k, double* A, double* w, double* U, double* V) {
  for (int i = 0; i < k; i++)
    for (int j = 0; j < k; j++) V[i * k + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kSvdSweeps; sweep++) {
    int rotated = 0;
    for (int p = 0; p < k - 1; p++)
      for (int q = p + 1; q < k; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int i = 0; i < m; i++) {
          alpha = alpha + A[i * k + p] * A[i * k + p];
          beta = beta + A[i * k + q] * A[i * k + q];
          gamma = gamma + A[i * k + p] * A[i * k + q];
        }
        if (!(fabs(gamma) > kSvdTol * sqrt(alpha * beta))) continue;
        rotated = 1;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        if (zeta < 0.0) t = -t;
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < m; i++) {
          const double aip = A[i * k + p], aiq = A[i * k + q];
          A[i * k + p] = c * aip - s * aiq;
          A[i * k + q] = s * aip + c * aiq;
        }
        for (int i = 0; i < k; i++) {
          const double vip = V[i * k + p], viq = V[i * k + q];
          V[i * k + p] = c * vip - s * viq;
          V[i * k + q] = s * vip + c * viq;
        }
      }
    if (!rotated) break;
  }
  double sv[5];
  int order[5];
  for (int j = 0; j < k; j++) {
    double ss = 0.0;
    for (int i = 0; i < m; i++) ss = ss + A[i * k + j] * A[i * k + j];
    sv[j] = sqrt(ss);
    order[j] = j;
  }
  for (int i = 0; i < k; i++) {
    int mx = i;
    for (int j = i + 1; j < k; j++)
      if (sv[j] > sv[mx]) mx = j;
    const double tv = sv[i]; sv[i] = sv[mx]; sv[mx] = tv;
    const int to = order[i]; order[i] = order[mx]; order[mx] = to;
  }
  double Vs[25];
  for (int j = 0; j < k; j++) {
    const int c = order[j];
    w[j] = sv[j];
    for (int i = 0; i < m; i++) U[i * k + j] = sv[j] == 0.0 ? 0.0 : A[i * k + c] / sv[j];
    for (int i = 0; i < k; i++) Vs[i * k + j] = V[i * k + c];
  }
  for (int i = 0; i < k * k; i++) V[i] = Vs[i];
}

// cvSolve(A, b, x, CV_SVD): x = V diag(1/w) U^T b over the singular values above kEps * max(m, k) * w[0]
void lstsqSvd(int m, int k, const double* Ain, const double* b, double* x) {
  double A[60], U[60], w[5], V[25];
  for (int i = 0; i < m * k; i++) A[i] = Ain[i];
  svdOneSided(m, k, A, w, U, V);
  const double thr = kEps * (double)(m > k ? m : k) * w[0];
  double c[5];
  for (int j = 0; j < k; j++) {
    double s = 0.0;
    for (int i = 0; i < m; i++) s = s + U[i * k + j] * b[i];
    c[j] = w[j] > thr ? s / w[j] : 0.0;
  }
  for (int i = 0; i < k; i++) {
    double s = 0.0;
    for (int j = 0; j < k; j++) s = s + V[i * k + j] * c[j];
    x[i] = s;
  }
}

// 3x3 ABt = U diag(w) V^T.  When w[2] <= 1e-10 * w[0] (numerically rank 2, e.g. a planar point set) U's last column is completed as
// det(V) * (u0 x u1), which makes U V^T the rotation that maps V's frame onto U's.
void svd3(const double* abt, double* U, double* V) {
  double A[9], w[3];
  for (int i = 0; i < 9; i++) A[i] = abt[i];
  svdOneSided(3, 3, A, w, U, V);
  if (!(w[2] > 1e-10 * w[0])) {
    const double detV = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) + V[2] * (V[3] * V[7] - V[4] * V[6]);
    const double sg = detV < 0.0 ? -1.0 : 1.0;
    U[2] = sg * (U[3] * U[7] - U[6] * U[4]);
    U[5] = sg * (U[6] * U[1] - U[0] * U[7]);
    U[8] = sg * (U[0] * U[4] - U[3] * U[1]);
  }
}

inline double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline double dist2(const double* a, const double* b) {
  return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

struct Epnp {
  double fu, fv, uc, vc;
  int n = 0;
  std::vector<double> pws, us, alphas, pcs;
  double cws[4][3], ccs[4][3];

  void add(double X, double Y, double Z, double u, double v) {
    pws.push_back(X); pws.push_back(Y); pws.push_back(Z);
    us.push_back(u); us.push_back(v);
    n++;
  }

  void chooseControlPoints() {
    cws[0][0] = cws[0][1] = cws[0][2] = 0;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < 3; j++) cws[0][j] += pws[3 * i + j];
    for (int j = 0; j < 3; j++) cws[0][j] /= n;
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dc[3], uct[9];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        double s = 0.0;
        for (int i = 0; i < n; i++) s = s + (pws[3 * i + a] - cws[0][a]) * (pws[3 * i + b] - cws[0][b]);
        m[3 * a + b] = s;
      }
    jacobiSym(3, m, dc, uct);
    for (int i = 1; i < 4; i++) {
      const double k = sqrt(dc[i - 1] / n);
      for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * uct[3 * (i - 1) + j];
    }
    kc[0] = sqrt(dc[0] / n); kc[1] = sqrt(dc[1] / n); kc[2] = sqrt(dc[2] / n);
    std::memcpy(ucts, uct, sizeof uct);
  }
  double kc[3], ucts[9];

  // CC = [c1 - c0, c2 - c0, c3 - c0] = Uct^T diag(k) (columns k_j * u_j), so its inverse is diag(1 / k) Uct: row j of CC^-1 is
  // u_j / k_j, and 0 when k_j <= 3 * eps * k_0 (cvInvert(CV_SVD)'s pseudo-inverse drops such a singular value).
  void computeBarycentric() {
    double ci[9];
    const double thr = 3.0 * kEps * kc[0];
    for (int j = 0; j < 3; j++)
      for (int c = 0; c < 3; c++) ci[3 * j + c] = kc[j] > thr ? ucts[3 * j + c] / kc[j] : 0.0;
    alphas.assign(4 * (size_t)n, 0.0);
    for (int i = 0; i < n; i++) {
      const double* pi = &pws[3 * i];
      double* a = &alphas[4 * i];
      for (int j = 0; j < 3; j++)
        a[1 + j] = ci[3 * j] * (pi[0] - cws[0][0]) + ci[3 * j + 1] * (pi[1] - cws[0][1]) + ci[3 * j + 2] * (pi[2] - cws[0][2]);
      a[0] = 1.0 - a[1] - a[2] - a[3];
    }
  }

  // element (r, c) of M (2n x 12), fill_M's values
  double Mrc(int r, int c) const {
    const int i = r >> 1, j = c / 3, w = c % 3;
    const double a = alphas[4 * i + j];
    if ((r & 1) == 0) return w == 0 ? a * fu : w == 1 ? 0.0 : a * (uc - us[2 * i]);
    return w == 0 ? 0.0 : w == 1 ? a * fv : a * (vc - us[2 * i + 1]);
  }

  void computeCcs(const double* betas, const double* ut) {
    for (int i = 0; i < 4; i++) ccs[i][0] = ccs[i][1] = ccs[i][2] = 0.0;
    for (int i = 0; i < 4; i++) {
      const double* v = ut + 12 * (11 - i);
      for (int j = 0; j < 4; j++)
        for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * v[3 * j + k];
    }
  }
  void computePcs() {
    pcs.assign(3 * (size_t)n, 0.0);
    for (int i = 0; i < n; i++) {
      const double* a = &alphas[4 * i];
      for (int j = 0; j < 3; j++) pcs[3 * i + j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
    }
  }
  void solveForSign() {
    if (n > 0 && pcs[2] < 0.0) {
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 3; j++) ccs[i][j] = -ccs[i][j];
      for (int i = 0; i < 3 * n; i++) pcs[i] = -pcs[i];
    }
  }
  void estimateRt(double R[3][3], double t[3]) {
    double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
    for (int i = 0; i < n; i++)
      for (int j = 0; j < 3; j++) { pc0[j] += pcs[3 * i + j]; pw0[j] += pws[3 * i + j]; }
    for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
    double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, U[9], V[9];
    for (int i = 0; i < n; i++) {
      const double* pc = &pcs[3 * i];
      const double* pw = &pws[3 * i];
      for (int j = 0; j < 3; j++) {
        abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
        abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
        abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
      }
    }
    svd3(abt, U, V);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) R[i][j] = dot(U + 3 * i, V + 3 * j);
    const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
                       R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
    if (det < 0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
    t[0] = pc0[0] - dot(R[0], pw0);
    t[1] = pc0[1] - dot(R[1], pw0);
    t[2] = pc0[2] - dot(R[2], pw0);
  }
  double reprojError(const double R[3][3], const double t[3]) const {
    double sum2 = 0.0;
    for (int i = 0; i < n; i++) {
      const double* pw = &pws[3 * i];
      const double Xc = dot(R[0], pw) + t[0], Yc = dot(R[1], pw) + t[1];
      const double invZc = 1.0 / (dot(R[2], pw) + t[2]);
      const double ue = uc + fu * Xc * invZc, ve = vc + fv * Yc * invZc;
      const double u = us[2 * i], v = us[2 * i + 1];
      sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    return sum2 / n;
  }
  double computeRt(const double* ut, const double* betas, double R[3][3], double t[3]) {
    computeCcs(betas, ut);
    computePcs();
    solveForSign();
    estimateRt(R, t);
    return reprojError(R, t);
  }

  static void computeL(const double* ut, double* l) {
    const double* v[4] = {ut + 12 * 11, ut + 12 * 10, ut + 12 * 9, ut + 12 * 8};
    double dv[4][6][3];
    for (int i = 0; i < 4; i++) {
      int a = 0, b = 1;
      for (int j = 0; j < 6; j++) {
        dv[i][j][0] = v[i][3 * a] - v[i][3 * b];
        dv[i][j][1] = v[i][3 * a + 1] - v[i][3 * b + 1];
        dv[i][j][2] = v[i][3 * a + 2] - v[i][3 * b + 2];
        b++;
        if (b > 3) { a++; b = a + 1; }
      }
    }
    for (int i = 0; i < 6; i++) {
      double* row = l + 10 * i;
      row[0] = dot(dv[0][i], dv[0][i]);
      row[1] = 2.0 * dot(dv[0][i], dv[1][i]);
      row[2] = dot(dv[1][i], dv[1][i]);
      row[3] = 2.0 * dot(dv[0][i], dv[2][i]);
      row[4] = 2.0 * dot(dv[1][i], dv[2][i]);
      row[5] = dot(dv[2][i], dv[2][i]);
      row[6] = 2.0 * dot(dv[0][i], dv[3][i]);
      row[7] = 2.0 * dot(dv[1][i], dv[3][i]);
      row[8] = 2.0 * dot(dv[2][i], dv[3][i]);
      row[9] = dot(dv[3][i], dv[3][i]);
    }
  }
  void computeRho(double* rho) const {
    rho[0] = dist2(cws[0], cws[1]); rho[1] = dist2(cws[0], cws[2]); rho[2] = dist2(cws[0], cws[3]);
    rho[3] = dist2(cws[1], cws[2]); rho[4] = dist2(cws[1], cws[3]); rho[5] = dist2(cws[2], cws[3]);
  }

  static void betas1(const double* L, const double* rho, double* betas) {
    double l[24], b4[4];
    for (int i = 0; i < 6; i++) { l[4 * i] = L[10 * i]; l[4 * i + 1] = L[10 * i + 1]; l[4 * i + 2] = L[10 * i + 3]; l[4 * i + 3] = L[10 * i + 6]; }
    lstsqSvd(6, 4, l, rho, b4);
    if (b4[0] < 0) {
      betas[0] = sqrt(-b4[0]);
      betas[1] = -b4[1] / betas[0]; betas[2] = -b4[2] / betas[0]; betas[3] = -b4[3] / betas[0];
    } else {
      betas[0] = sqrt(b4[0]);
      betas[1] = b4[1] / betas[0]; betas[2] = b4[2] / betas[0]; betas[3] = b4[3] / betas[0];
    }
  }
  static void betas2(const double* L, const double* rho, double* betas) {
    double l[18], b3[3];
    for (int i = 0; i < 6; i++) { l[3 * i] = L[10 * i]; l[3 * i + 1] = L[10 * i + 1]; l[3 * i + 2] = L[10 * i + 2]; }
    lstsqSvd(6, 3, l, rho, b3);
    if (b3[0] < 0) {
      betas[0] = sqrt(-b3[0]);
      betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
    } else {
      betas[0] = sqrt(b3[0]);
      betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) betas[0] = -betas[0];
    betas[2] = 0.0; betas[3] = 0.0;
  }
  static void betas3(const double* L, const double* rho, double* betas) {
    double l[30], b5[5];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 5; j++) l[5 * i + j] = L[10 * i + j];
    lstsqSvd(6, 5, l, rho, b5);
    if (b5[0] < 0) {
      betas[0] = sqrt(-b5[0]);
      betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
    } else {
      betas[0] = sqrt(b5[0]);
      betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) betas[0] = -betas[0];
    betas[2] = b5[3] / betas[0];
    betas[3] = 0.0;
  }

  // the reference's Householder qr_solve on A (6 x 4) and b (6); returns false (X untouched) on its "A is singular" exit
  static bool qrSolve(double* A, double* b, double* X) {
    const int nr = 6, nc = 4;
    double A1[4], A2[4];
    for (int k = 0; k < nc; k++) {
      double eta = fabs(A[k * nc + k]);
      for (int i = k + 1; i < nr; i++) {
        const double elt = fabs(A[i * nc + k]);
        if (eta < elt) eta = elt;
      }
      if (eta == 0) return false;
      double sum = 0.0;
      const double inv_eta = 1. / eta;
      for (int i = k; i < nr; i++) {
        A[i * nc + k] *= inv_eta;
        sum += A[i * nc + k] * A[i * nc + k];
      }
      double sigma = sqrt(sum);
      if (A[k * nc + k] < 0) sigma = -sigma;
      A[k * nc + k] += sigma;
      A1[k] = sigma * A[k * nc + k];
      A2[k] = -eta * sigma;
      for (int j = k + 1; j < nc; j++) {
        double s = 0;
        for (int i = k; i < nr; i++) s += A[i * nc + k] * A[i * nc + j];
        const double tau = s / A1[k];
        for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
      }
    }
    for (int j = 0; j < nc; j++) {
      double tau = 0;
      for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
      tau /= A1[j];
      for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
      double s = 0;
      for (int j = i + 1; j < nc; j++) s += A[i * nc + j] * X[j];
      X[i] = (b[i] - s) / A2[i];
    }
    return true;
  }
  // five steps; x starts at 0 and a singular step leaves it as it was (the reference reads an uninitialised x there)
  static void gaussNewton(const double* L, const double* rho, double* betas) {
    double x[4] = {0, 0, 0, 0};
    for (int it = 0; it < 5; it++) {
      double A[24], b[6];
      for (int i = 0; i < 6; i++) {
        const double* r = L + 10 * i;
        A[4 * i] = 2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3];
        A[4 * i + 1] = r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3];
        A[4 * i + 2] = r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3];
        A[4 * i + 3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3];
        b[i] = rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] + r[3] * betas[0] * betas[2] +
                         r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] + r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] +
                         r[8] * betas[2] * betas[3] + r[9] * betas[3] * betas[3]);
      }
      qrSolve(A, b, x);
      for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
  }

  double computePose(double R[3][3], double t[3]) {
    chooseControlPoints();
    computeBarycentric();
    double mtm[144], d[12], ut[144];
    for (int a = 0; a < 12; a++)
      for (int b = a; b < 12; b++) {
        double s = 0.0;
        for (int r = 0; r < 2 * n; r++) s = s + Mrc(r, a) * Mrc(r, b);
        mtm[12 * a + b] = s;
        mtm[12 * b + a] = s;
      }
    jacobiSym(12, mtm, d, ut);
    double L[60], rho[6];
    computeL(ut, L);
    computeRho(rho);
    double Betas[4][4], err[4], Rs[4][3][3], ts[4][3];
    betas1(L, rho, Betas[1]);
    gaussNewton(L, rho, Betas[1]);
    err[1] = computeRt(ut, Betas[1], Rs[1], ts[1]);
    betas2(L, rho, Betas[2]);
    gaussNewton(L, rho, Betas[2]);
    err[2] = computeRt(ut, Betas[2], Rs[2], ts[2]);
    betas3(L, rho, Betas[3]);
    gaussNewton(L, rho, Betas[3]);
    err[3] = computeRt(ut, Betas[3], Rs[3], ts[3]);
    int N = 1;
    if (err[2] < err[1]) N = 2;
    if (err[3] < err[N]) N = 3;
    std::memcpy(R, Rs[N], sizeof Rs[N]);
    std::memcpy(t, ts[N], sizeof ts[N]);
    return err[N];
  }
};

struct Prob {
  int N;
  const float *Xw, *P2D, *maxErr;
  float K[4];
};

// CheckInliers with its mixed float / double types
int checkInliers(const Prob& p, const double R[3][3], const double t[3], uint8_t* mask) {
  const double fu = p.K[0], fv = p.K[1], uc = p.K[2], vc = p.K[3];
  int cnt = 0;
  for (int i = 0; i < p.N; i++) {
    const float x = p.Xw[3 * i], y = p.Xw[3 * i + 1], z = p.Xw[3 * i + 2];
    const float Xc = R[0][0] * x + R[0][1] * y + R[0][2] * z + t[0];
    const float Yc = R[1][0] * x + R[1][1] * y + R[1][2] * z + t[1];
    const float invZc = 1 / (R[2][0] * x + R[2][1] * y + R[2][2] * z + t[2]);
    const double ue = uc + fu * Xc * invZc, ve = vc + fv * Yc * invZc;
    const float distX = p.P2D[2 * i] - ue, distY = p.P2D[2 * i + 1] - ve;
    const float error2 = distX * distX + distY * distY;
    const bool in = error2 < p.maxErr[i];
    mask[i] = in;
    cnt += in;
  }
  return cnt;
}

void poseFromPoints(const Prob& p, const int* idx, int n, double R[3][3], double t[3]) {
  Epnp e;
  e.fu = p.K[0]; e.fv = p.K[1]; e.uc = p.K[2]; e.vc = p.K[3];
  for (int i = 0; i < n; i++) {
    const int k = idx[i];
    e.add(p.Xw[3 * k], p.Xw[3 * k + 1], p.Xw[3 * k + 2], p.P2D[2 * k], p.P2D[2 * k + 1]);
  }
  e.computePose(R, t);
}

void toTcw(const double R[3][3], const double t[3], float* T) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[r][c];
    T[4 * r + 3] = (float)t[r];
  }
}

}  // namespace

extern "C" {

// SetRansacParameters' arithmetic.  out: [nMinInliers, maxIts]; epsilon out as float
void pnpref_params(int N, double probability, int minInliers, int maxIterations, int minSet, float epsilon, int* out, float* epsOut) {
  int nMinInliers = N * epsilon;
  if (nMinInliers < minInliers) nMinInliers = minInliers;
  if (nMinInliers < minSet) nMinInliers = minSet;
  if (epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
  int nIterations;
  if (nMinInliers == N) nIterations = 1;
  else nIterations = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
  int its = nIterations < maxIterations ? nIterations : maxIterations;
  out[0] = nMinInliers;
  out[1] = its > 1 ? its : 1;
  *epsOut = epsilon;
}

void pnpref_eig_sym(int n, const double* A, double* d, double* ut) {
  double a[144];
  std::memcpy(a, A, sizeof(double) * n * n);
  jacobiSym(n, a, d, ut);
}
void pnpref_svd(int m, int k, const double* A, double* w, double* U, double* V) {
  double a[60];
  std::memcpy(a, A, sizeof(double) * m * k);
  svdOneSided(m, k, a, w, U, V);
}
void pnpref_lstsq(int m, int k, const double* A, const double* b, double* x) { lstsqSvd(m, k, A, b, x); }
void pnpref_qr_solve(const double* A, const double* b, double* x) {
  double a[24], bb[6];
  std::memcpy(a, A, sizeof a);
  std::memcpy(bb, b, sizeof bb);
  Epnp::qrSolve(a, bb, x);
}

// EPnP on points idx[0..n-1]: out = R (9, row-major), t (3), mean reprojection error
void pnpref_epnp(const float* Xw, const float* P2D, const float* K, const int* idx, int n, double* out) {

  Epnp e;
  e.fu = K[0]; e.fv = K[1]; e.uc = K[2]; e.vc = K[3];
  for (int i = 0; i < n; i++) e.add(Xw[3 * idx[i]], Xw[3 * idx[i] + 1], Xw[3 * idx[i] + 2], P2D[2 * idx[i]], P2D[2 * idx[i] + 1]);
  double R[3][3], t[3];
  out[12] = e.computePose(R, t);

  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) out[3 * r + c] = R[r][c];
  for (int r = 0; r < 3; r++) out[9 + r] = t[r];
}

// iterate(chunk) repeated from state[0] = mnIterations until a return, bNoMore, or the quads run out.
// state in/out: [next_hyp, best_inliers]; bestMask [N] in/out; bestTcw [12] in/out.
// out: [ret_hyp, how (0 none, 1 refined, 2 best at exhaustion), no_more, n_calls, n_inliers]; Tcw [12]; inliers [N]; hyp [n_hyp]
void pnpref_ransac(int N, const float* Xw, const float* P2D, const float* maxErr, const float* K, int minInliers, int maxIts, int loopOr,
                   const int* quads, int nHyp, int chunk, int* state, uint8_t* bestMask, float* bestTcw, int* out, float* Tcw,
                   uint8_t* inliers, int* hyp) {
  Prob p{N, Xw, P2D, maxErr, {K[0], K[1], K[2], K[3]}};
  for (int k = 0; k < nHyp; k++) hyp[k] = -1;
  std::memset(inliers, 0, N);
  std::memset(Tcw, 0, 12 * sizeof(float));
  out[0] = -1; out[1] = 0; out[2] = 0; out[3] = 0; out[4] = 0;
  int mnIterations = state[0], mnBest = state[1], used = 0;
  std::vector<uint8_t> mask(N), refMask(N);
  while (true) {   // one iterate(chunk) call per pass
    out[3]++;
    bool noMore = false;
    if (N < minInliers) { out[2] = 1; break; }
    int cur = 0;
    bool ran_out = false;
    while (loopOr ? (mnIterations < maxIts || cur < chunk) : (mnIterations < maxIts && cur < chunk)) {
      if (used == nHyp) {   // out of quads: a call that ran nothing does not count
        ran_out = true;
        if (cur == 0) out[3]--;
        break;
      }
      cur++;
      mnIterations++;
      const int h = used++;
      double R[3][3], t[3];
      poseFromPoints(p, quads + 4 * h, 4, R, t);
      const int cnt = checkInliers(p, R, t, mask.data());
      hyp[h] = cnt;
      if (cnt >= minInliers) {
        if (cnt > mnBest) {
          std::memcpy(bestMask, mask.data(), N);
          mnBest = cnt;
          toTcw(R, t, bestTcw);
        }
        // Refine(): EPnP over the best inliers in ascending index, then CheckInliers; succeeds when the count > minInliers
        std::vector<int> idx;
        for (int i = 0; i < N; i++)
          if (bestMask[i]) idx.push_back(i);
        double Rr[3][3], tr[3];
        poseFromPoints(p, idx.data(), (int)idx.size(), Rr, tr);
        const int rc = checkInliers(p, Rr, tr, refMask.data());
        if (rc > minInliers) {
          out[0] = mnIterations - 1; out[1] = 1; out[4] = rc;
          toTcw(Rr, tr, Tcw);
          std::memcpy(inliers, refMask.data(), N);
          state[0] = mnIterations; state[1] = mnBest;
          return;
        }
      }
    }
    if (ran_out) break;
    if (mnIterations >= maxIts) {
      noMore = true;
      if (mnBest >= minInliers) {
        out[1] = 2; out[4] = mnBest;
        std::memcpy(Tcw, bestTcw, 12 * sizeof(float));
        std::memcpy(inliers, bestMask, N);
      }
    }
    if (noMore) { out[2] = 1; break; }
  }
  state[0] = mnIterations; state[1] = mnBest;
}

}  // extern "C"
