// gfx950 HIP kernels of the relocalisation EPnP RANSAC (ydorb_pnp_ransac).
//
// Restated from ORB-SLAM2's PnPsolver.cc (iterate, Refine, CheckInliers and Lepetit's EPnP), which YDORBSLAM renames to pnpSolver.*
// (DESIGN.md section 6d), in fp64 under the written-order contract of DESIGN.md section 2 ("EPnP RANSAC"): +, -, *, / and sqrt only,
// every op a single IEEE operation (-ffp-contract=off), so the kernels equal the CPU restatement tests/pnp_ref bit for bit.
// Layout: one single-wave workgroup per hypothesis.  The EPnP state (MtM, its eigenvectors, the control points) lives in LDS; the 78
// entries of MtM and every row / column / eigenvector update of a Jacobi rotation are spread over the lanes, each element computed by
// exactly the expression of the serial restatement, so the bits do not depend on the split.  The short serial steps (3x3 PCA, the
// 6xk least-squares solves, Gauss-Newton, R and t) run on lane 0.  Inliers are counted 64 points per step with a ballot.
// The commit kernel, one 256-thread workgroup per problem, walks the counts in iterate()'s order and runs Refine (EPnP over the best
// inliers) with the same device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace ydorb {
namespace pnp {

constexpr int kSymSweeps = 16;
constexpr int kSvdSweeps = 16;
constexpr double kSvdTol = 1e-15;
constexpr double kEps = 2.220446049250313e-16;
constexpr int kCommitThreads = 256;

struct ProbDev {        // one problem; offsets in elements of the packed arrays
  int n, minInl, maxIts, nEval;
  int bestIn;           // mnBestInliers on entry
  int ptOff;            // first point in Xw (x3), P2D (x2), maxErr, masks, refine scratch
  int hypOff;           // first hypothesis in quads (x4), counts, poses (x12)
  int seqLen;           // hypotheses the iterate() sequence runs without a return
  float K[4];           // fu fv uc vc
};
struct ProbOut { int ret, how, best, bestHyp, nInl, pad[3]; float T[12], bestT[12]; };

// ------------------------------------------------------------------------------------------------------------ serial pieces
__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ inline double dist2(const double* a, const double* b) {
  return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// rotation (c, s) of the symmetric cyclic Jacobi; false when apq is negligible against both diagonals
__device__ inline bool jacobiRot(double app, double aqq, double apq, double& c, double& s) {
  const double g = 100.0 * fabs(apq);
  if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  c = 1.0 / sqrt(t * t + 1.0);
  s = t * c;
  return true;
}

// |eigenvalues| descending (strict > keeps the first of equal values) and sign-normalised eigenvector rows
__device__ inline void sortEig(int n, const double* A, const double* V, double* d, double* ut) {
  int order[12];
  double ev[12];
  for (int i = 0; i < n; i++) { order[i] = i; ev[i] = fabs(A[i * n + i]); }
  for (int i = 0; i < n; i++) {
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

__device__ inline void jacobiSym3(double* A, double* d, double* ut) {   // one thread
  const int n = 3;
  double V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int sweep = 0; sweep < kSymSweeps; sweep++) {
    int rotated = 0;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        double c, s;
        if (!jacobiRot(A[p * n + p], A[q * n + q], A[p * n + q], c, s)) continue;
        rotated = 1;
        for (int k = 0; k < n; k++) {
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {
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
  sortEig(3, A, V, d, ut);
}

__device__ inline void svdOneSided(int m, int k, double* A, double* w, double* U, double* V) {   // one thread; m <= 6, k <= 5
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

__device__ inline void lstsqSvd(int m, int k, const double* Ain, const double* b, double* x) {
  double A[30], U[30], w[5], V[25];
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

__device__ inline void svd3(const double* abt, double* U, double* V) {
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

__device__ inline void betas1(const double* L, const double* rho, double* betas) {
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
__device__ inline void betas2(const double* L, const double* rho, double* betas) {
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
__device__ inline void betas3(const double* L, const double* rho, double* betas) {
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

__device__ inline bool qrSolve(double* A, double* b, double* X) {   // the reference's Householder qr_solve, 6 x 4
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
__device__ inline void gaussNewton(const double* L, const double* rho, double* betas) {
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

__device__ inline void computeL(const double* ut, double* l) {
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
    row[0] = dot3(dv[0][i], dv[0][i]);
    row[1] = 2.0 * dot3(dv[0][i], dv[1][i]);
    row[2] = dot3(dv[1][i], dv[1][i]);
    row[3] = 2.0 * dot3(dv[0][i], dv[2][i]);
    row[4] = 2.0 * dot3(dv[1][i], dv[2][i]);
    row[5] = dot3(dv[2][i], dv[2][i]);
    row[6] = 2.0 * dot3(dv[0][i], dv[3][i]);
    row[7] = 2.0 * dot3(dv[1][i], dv[3][i]);
    row[8] = 2.0 * dot3(dv[2][i], dv[3][i]);
    row[9] = dot3(dv[3][i], dv[3][i]);
  }
}

// ------------------------------------------------------------------------------------------------------------ EPnP, one workgroup
struct Shared {          // LDS of one EPnP solve
  double A[144], V[144], ut[144], d[12];
  double cws[4][3], ccs[4][3], kc[3], uct[9];
  double L[60], rho[6], betas[4];
  double Rs[4][9], ts[4][3], err[4];
  double R[9], t[3];
  double al4[16], pcs4[12];   // the hypothesis kernel's 4 points
  int idx4[4];
  int cnt;
};

// a point of the problem, as the reference's double pws / us
struct Pts {
  const float* Xw;
  const float* P2D;
  const int* idx;
  __device__ double pw(int i, int c) const { return (double)Xw[3 * idx[i] + c]; }
  __device__ double u(int i, int c) const { return (double)P2D[2 * idx[i] + c]; }
};

// compute_pose over the n points pts (n >= 0), run by all nthr threads of the workgroup; al [n][4] and pcs [n][3] are scratch
// (LDS or global).  Result in S.R, S.t.  Ends with a barrier.
__device__ void epnp(const Pts& P, int n, const float* K, double* al, double* pcs, Shared& S, int tid, int nthr) {
  const double fu = K[0], fv = K[1], uc = K[2], vc = K[3];
  if (tid == 0) {   // choose_control_points, and CC^-1
    double (*cws)[3] = S.cws;
    cws[0][0] = cws[0][1] = cws[0][2] = 0;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < 3; j++) cws[0][j] += P.pw(i, j);
    for (int j = 0; j < 3; j++) cws[0][j] /= n;
    double m[9], dc[3];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        double s = 0.0;
        for (int i = 0; i < n; i++) s = s + (P.pw(i, a) - cws[0][a]) * (P.pw(i, b) - cws[0][b]);
        m[3 * a + b] = s;
      }
    jacobiSym3(m, dc, S.uct);
    for (int i = 1; i < 4; i++) {
      const double k = sqrt(dc[i - 1] / n);
      for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * S.uct[3 * (i - 1) + j];
    }
    S.kc[0] = sqrt(dc[0] / n); S.kc[1] = sqrt(dc[1] / n); S.kc[2] = sqrt(dc[2] / n);
  }
  __syncthreads();
  {   // compute_barycentric_coordinates, a point per thread
    const double thr = 3.0 * kEps * S.kc[0];
    double ci[9];
    for (int j = 0; j < 3; j++)
      for (int c = 0; c < 3; c++) ci[3 * j + c] = S.kc[j] > thr ? S.uct[3 * j + c] / S.kc[j] : 0.0;
    for (int i = tid; i < n; i += nthr) {
      const double p0 = P.pw(i, 0), p1 = P.pw(i, 1), p2 = P.pw(i, 2);
      double* a = al + 4 * i;
      double a1[3];
      for (int j = 0; j < 3; j++) a1[j] = ci[3 * j] * (p0 - S.cws[0][0]) + ci[3 * j + 1] * (p1 - S.cws[0][1]) + ci[3 * j + 2] * (p2 - S.cws[0][2]);
      a[1] = a1[0]; a[2] = a1[1]; a[3] = a1[2];
      a[0] = 1.0 - a1[0] - a1[1] - a1[2];
    }
  }
  __syncthreads();
  // MtM: the 78 entries a <= b over the lanes, each an ascending-row sum of fill_M's products
  for (int e = tid; e < 78; e += nthr) {
    int a = 0, r0 = e;
    while (r0 >= 12 - a) { r0 -= 12 - a; a++; }
    const int b = a + r0;
    const int ja = a / 3, wa = a % 3, jb = b / 3, wb = b % 3;
    double s = 0.0;
    for (int i = 0; i < n; i++) {
      const double aa = al[4 * i + ja], ab = al[4 * i + jb];
      const double ui = P.u(i, 0), vi = P.u(i, 1);
      const double m0a = wa == 0 ? aa * fu : wa == 1 ? 0.0 : aa * (uc - ui);
      const double m0b = wb == 0 ? ab * fu : wb == 1 ? 0.0 : ab * (uc - ui);
      s = s + m0a * m0b;
      const double m1a = wa == 0 ? 0.0 : wa == 1 ? aa * fv : aa * (vc - vi);
      const double m1b = wb == 0 ? 0.0 : wb == 1 ? ab * fv : ab * (vc - vi);
      s = s + m1a * m1b;
    }
    S.A[12 * a + b] = s;
    S.A[12 * b + a] = s;
  }
  for (int e = tid; e < 144; e += nthr) S.V[e] = (e / 12) == (e % 12) ? 1.0 : 0.0;
  __syncthreads();
  // 12x12 cyclic Jacobi: every thread takes the same (uniform) decision; thread k updates row / column / eigenvector element k
  for (int sweep = 0; sweep < kSymSweeps; sweep++) {
    int rotated = 0;
    for (int p = 0; p < 11; p++)
      for (int q = p + 1; q < 12; q++) {
        double c, s;
        const bool rot = jacobiRot(S.A[p * 12 + p], S.A[q * 12 + q], S.A[p * 12 + q], c, s);
        __syncthreads();
        if (!rot) continue;
        rotated = 1;
        if (tid < 12) {
          const int k = tid;
          const double akp = S.A[k * 12 + p], akq = S.A[k * 12 + q];
          S.A[k * 12 + p] = c * akp - s * akq;
          S.A[k * 12 + q] = s * akp + c * akq;
          const double vkp = S.V[k * 12 + p], vkq = S.V[k * 12 + q];
          S.V[k * 12 + p] = c * vkp - s * vkq;
          S.V[k * 12 + q] = s * vkp + c * vkq;
        }
        __syncthreads();
        if (tid < 12) {
          const int k = tid;
          const double apk = S.A[p * 12 + k], aqk = S.A[q * 12 + k];
          S.A[p * 12 + k] = c * apk - s * aqk;
          S.A[q * 12 + k] = s * apk + c * aqk;
        }
        __syncthreads();
      }
    if (!rotated) break;
  }
  if (tid == 0) {
    sortEig(12, S.A, S.V, S.d, S.ut);
    computeL(S.ut, S.L);
    const double (*cws)[3] = S.cws;
    S.rho[0] = dist2(cws[0], cws[1]); S.rho[1] = dist2(cws[0], cws[2]); S.rho[2] = dist2(cws[0], cws[3]);
    S.rho[3] = dist2(cws[1], cws[2]); S.rho[4] = dist2(cws[1], cws[3]); S.rho[5] = dist2(cws[2], cws[3]);
  }
  __syncthreads();
  for (int ap = 1; ap <= 3; ap++) {
    if (tid == 0) {   // find_betas_approx_<ap>, gauss_newton, compute_ccs
      double betas[4];
      if (ap == 1) betas1(S.L, S.rho, betas);
      else if (ap == 2) betas2(S.L, S.rho, betas);
      else betas3(S.L, S.rho, betas);
      gaussNewton(S.L, S.rho, betas);
      for (int i = 0; i < 4; i++) S.ccs[i][0] = S.ccs[i][1] = S.ccs[i][2] = 0.0;
      for (int i = 0; i < 4; i++) {
        const double* v = S.ut + 12 * (11 - i);
        for (int j = 0; j < 4; j++)
          for (int k = 0; k < 3; k++) S.ccs[j][k] += betas[i] * v[3 * j + k];
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += nthr) {   // compute_pcs
      const double* a = al + 4 * i;
      for (int j = 0; j < 3; j++) pcs[3 * i + j] = a[0] * S.ccs[0][j] + a[1] * S.ccs[1][j] + a[2] * S.ccs[2][j] + a[3] * S.ccs[3][j];
    }
    __syncthreads();
    // solve_for_sign: every thread takes the decision before any thread negates pcs[2] (the workgroup may span several waves)
    const bool flip = n > 0 && pcs[2] < 0.0;
    __syncthreads();
    if (flip)
      for (int i = tid; i < 3 * n; i += nthr) pcs[i] = -pcs[i];
    __syncthreads();
    if (tid == 0) {   // estimate_R_and_t and reprojection_error
      double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
      for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) { pc0[j] += pcs[3 * i + j]; pw0[j] += P.pw(i, j); }
      for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
      double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, U[9], V[9];
      for (int i = 0; i < n; i++) {
        const double* pc = pcs + 3 * i;
        const double pw[3] = {P.pw(i, 0), P.pw(i, 1), P.pw(i, 2)};
        for (int j = 0; j < 3; j++) {
          abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
          abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
          abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
        }
      }
      svd3(abt, U, V);
      double R[3][3], t[3];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i][j] = dot3(U + 3 * i, V + 3 * j);
      const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
                         R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
      if (det < 0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
      t[0] = pc0[0] - dot3(R[0], pw0);
      t[1] = pc0[1] - dot3(R[1], pw0);
      t[2] = pc0[2] - dot3(R[2], pw0);
      double sum2 = 0.0;
      for (int i = 0; i < n; i++) {
        const double pw[3] = {P.pw(i, 0), P.pw(i, 1), P.pw(i, 2)};
        const double Xc = dot3(R[0], pw) + t[0], Yc = dot3(R[1], pw) + t[1];
        const double invZc = 1.0 / (dot3(R[2], pw) + t[2]);
        const double ue = uc + fu * Xc * invZc, ve = vc + fv * Yc * invZc;
        const double u = P.u(i, 0), v = P.u(i, 1);
        sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
      }
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) S.Rs[ap][3 * i + j] = R[i][j];
      for (int i = 0; i < 3; i++) S.ts[ap][i] = t[i];
      S.err[ap] = sum2 / n;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int N = 1;
    if (S.err[2] < S.err[1]) N = 2;
    if (S.err[3] < S.err[N]) N = 3;
    for (int i = 0; i < 9; i++) S.R[i] = S.Rs[N][i];
    for (int i = 0; i < 3; i++) S.t[i] = S.ts[N][i];
  }
  __syncthreads();
}

// CheckInliers' test of point i (the reference's float / double mix)
__device__ inline bool inlier(const double* Rm, const double* tv, const float* Xw, const float* P2D, const float* maxErr, const float* K, int i) {
  const double fu = K[0], fv = K[1], uc = K[2], vc = K[3];
  const double R[3][3] = {{Rm[0], Rm[1], Rm[2]}, {Rm[3], Rm[4], Rm[5]}, {Rm[6], Rm[7], Rm[8]}};
  const double t[3] = {tv[0], tv[1], tv[2]};
  const float x = Xw[3 * i], y = Xw[3 * i + 1], z = Xw[3 * i + 2];
  const float Xc = R[0][0] * x + R[0][1] * y + R[0][2] * z + t[0];
  const float Yc = R[1][0] * x + R[1][1] * y + R[1][2] * z + t[1];
  const float invZc = 1 / (R[2][0] * x + R[2][1] * y + R[2][2] * z + t[2]);
  const double ue = uc + fu * Xc * invZc, ve = vc + fv * Yc * invZc;
  const float distX = P2D[2 * i] - ue, distY = P2D[2 * i + 1] - ve;
  const float error2 = distX * distX + distY * distY;
  return error2 < maxErr[i];
}

// ------------------------------------------------------------------------------------------------------------ kernels
// counts[hypOff + h], poses[hypOff + h][12] (R row-major, t) of hypothesis h of problem blockIdx.y: one single-wave workgroup each
__global__ __launch_bounds__(64) void k_pnp_hypotheses(const ProbDev* __restrict__ probs, const float* __restrict__ Xw,
                                                       const float* __restrict__ P2D, const float* __restrict__ maxErr,
                                                       const int* __restrict__ quads, int* __restrict__ counts,
                                                       double* __restrict__ poses) {
  __shared__ Shared S;
  const ProbDev& pr = probs[blockIdx.y];
  const int h = blockIdx.x, tid = threadIdx.x;
  if (h >= pr.nEval) return;   // uniform over the workgroup
  const int o = pr.ptOff;
  const float *xw = Xw + 3 * o, *p2 = P2D + 2 * o, *me = maxErr + o;
  if (tid < 4) S.idx4[tid] = quads[4 * (size_t)(pr.hypOff + h) + tid];
  __syncthreads();
  const Pts P{xw, p2, S.idx4};
  epnp(P, 4, pr.K, S.al4, S.pcs4, S, tid, 64);
  int cnt = 0;
  for (int base = 0; base < pr.n; base += 64) {
    const int i = base + tid;
    const bool in = i < pr.n && inlier(S.R, S.t, xw, p2, me, pr.K, i);
    cnt += __popcll(__ballot(in));
  }
  if (tid == 0) counts[pr.hypOff + h] = cnt;
  if (tid < 9) poses[12 * (size_t)(pr.hypOff + h) + tid] = S.R[tid];
  else if (tid < 12) poses[12 * (size_t)(pr.hypOff + h) + tid] = S.t[tid - 9];
}

struct CommitArgs {
  const ProbDev* probs;
  const float *Xw, *P2D, *maxErr;
  const int* counts;
  const double* poses;
  const uint8_t* bestMaskIn;
  uint8_t* bestMask;      // out: the best mask (from bestMaskIn or the best hypothesis)
  uint8_t* inliers;       // out: the returned mask
  int* idx;               // scratch [points]: Refine's best-inlier list
  double *al, *pcs;       // scratch [points][4], [points][3]
  ProbOut* out;
};

__device__ inline void toTcw(const double* R, const double* t, float* T) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
    T[4 * r + 3] = (float)t[r];
  }
}

// iterate()'s ordered commit, one workgroup per problem.  Refine's input (the best mask) changes only when the best does, so its
// outcome is recomputed only then; that equals calling it at every qualifying hypothesis.
__global__ __launch_bounds__(kCommitThreads) void k_pnp_commit(CommitArgs a) {
  __shared__ Shared S;
  __shared__ int sRefCnt, sM;
  const ProbDev& pr = a.probs[blockIdx.x];
  const int tid = threadIdx.x, o = pr.ptOff, N = pr.n;
  const float *xw = a.Xw + 3 * o, *p2 = a.P2D + 2 * o, *me = a.maxErr + o;
  uint8_t* bmask = a.bestMask + o;
  uint8_t* inl = a.inliers + o;
  for (int i = tid; i < N; i += kCommitThreads) { bmask[i] = a.bestMaskIn[o + i]; inl[i] = 0; }
  __syncthreads();
  int best = pr.bestIn, bestHyp = -1, ret = -1;
  bool dirty = true, lastOk = false;
  for (int h = 0; h < pr.nEval; h++) {
    const int c = a.counts[pr.hypOff + h];
    if (c < pr.minInl) continue;
    if (c > best) {   // mvbBestInliers = mvbInliersi of hypothesis h
      best = c; bestHyp = h; dirty = true;
      const double* ps = a.poses + 12 * (size_t)(pr.hypOff + h);
      for (int i = tid; i < N; i += kCommitThreads) bmask[i] = inlier(ps, ps + 9, xw, p2, me, pr.K, i);
      __syncthreads();
    }
    if (dirty) {   // Refine()
      if (tid == 0) {
        int m = 0;
        for (int i = 0; i < N; i++)
          if (bmask[i]) a.idx[o + m++] = i;
        sM = m;
        sRefCnt = 0;
      }
      __syncthreads();
      const int m = sM;
      const Pts P{xw, p2, a.idx + o};
      epnp(P, m, pr.K, a.al + 4 * (size_t)o, a.pcs + 3 * (size_t)o, S, tid, kCommitThreads);
      int cnt = 0;
      for (int i = tid; i < N; i += kCommitThreads) {
        const bool in = inlier(S.R, S.t, xw, p2, me, pr.K, i);
        inl[i] = in;
        cnt += in;
      }
      atomicAdd(&sRefCnt, cnt);
      __syncthreads();
      dirty = false;
      lastOk = sRefCnt > pr.minInl;
    }
    if (lastOk) { ret = h; break; }
  }
  const bool complete = pr.nEval == pr.seqLen;
  int how = ret >= 0 ? 1 : (complete && best >= pr.minInl && N >= pr.minInl) ? 2 : 0;
  if (how == 2)
    for (int i = tid; i < N; i += kCommitThreads) inl[i] = bmask[i];
  else if (how == 0)
    for (int i = tid; i < N; i += kCommitThreads) inl[i] = 0;
  if (tid == 0) {
    ProbOut& r = a.out[blockIdx.x];
    r.ret = ret; r.how = how; r.best = best; r.bestHyp = bestHyp;
    r.nInl = how == 1 ? sRefCnt : how == 2 ? best : 0;
    if (bestHyp >= 0) {
      const double* ps = a.poses + 12 * (size_t)(pr.hypOff + bestHyp);
      toTcw(ps, ps + 9, r.bestT);
    }
    if (how == 1) toTcw(S.R, S.t, r.T);
  }
}

}  // namespace pnp
}  // namespace ydorb
