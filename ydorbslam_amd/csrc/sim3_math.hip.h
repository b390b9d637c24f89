// The g2o Sim3 algebra in double (types/sim3.h), once: the exponential and logarithm maps with their A, B, C branches, product, inverse,
// the point map and VertexSim3Expmap::oplusImpl.  Shared by the Sim3 check (sim3_kernels.hip.h) and the essential-graph optimisation
// (essential_kernels.hip.h).  Functions and one type only - no kernel and no device variable - so any translation unit includes it.
#pragma once
#include <hip/hip_runtime.h>
#include "g2o_math.hip.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace sim3 {

using g2o::R; using g2o::V3; using g2o::Q4;
using g2o::add; using g2o::cross; using g2o::scale; using g2o::qrot; using g2o::qmul; using g2o::rToQ; using g2o::qToR;
using g2o::huber; using g2o::block_sums; using g2o::block_sum1; using g2o::dense_solve; using g2o::lambda_init; using g2o::lm_judge;

struct S3 { Q4 r; V3 t; R s; };

// g2o Sim3(const Vector7d& update) (types/sim3.h): omega, upsilon, sigma and its A, B, C branches.
// limitB: the branch theta < eps <= |sigma| takes B = (s (sigma^2 / 2 - sigma + 1) - 1) / sigma^3, the limit of the general branch for
// theta -> 0, instead of the bundled form without the - 1 (which is about 1 / sigma^3 and multiplies Omega^2).  Off for the Sim3 check,
// whose results stay as they are; on for the essential graph.
__device__ __forceinline__ S3 sim3Exp(const R* u, bool limitB = false) {
  const R ox = u[0], oy = u[1], oz = u[2], sigma = u[6];
  const R theta = sqrt(ox * ox + oy * oy + oz * oz);
  const R Om[3][3] = {{0, -oz, oy}, {oz, 0, -ox}, {-oy, ox, 0}};
  R Om2[3][3];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) Om2[a][b] = Om[a][0] * Om[0][b] + Om[a][1] * Om[1][b] + Om[a][2] * Om[2][b];
  const R s = exp(sigma), eps = 0.00001;
  R A, B, C, ca, cb;
  const bool small = theta < eps;
  if (small) { ca = 1; cb = 1; }
  else { ca = sin(theta) / theta; cb = (1 - cos(theta)) / (theta * theta); }
  if (fabs(sigma) < eps) {
    C = 1;
    if (small) { A = 1. / 2.; B = 1. / 6.; }
    else { const R th2 = theta * theta; A = (1 - cos(theta)) / th2; B = (theta - sin(theta)) / (th2 * theta); }
  } else {
    C = (s - 1) / sigma;
    if (small) {
      const R sg2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sg2;
      B = limitB ? ((0.5 * sg2 - sigma + 1) * s - 1) / (sg2 * sigma) : ((0.5 * sg2 - sigma + 1) * s) / (sg2 * sigma);
    } else {
      const R a = s * sin(theta), b = s * cos(theta), th2 = theta * theta, sg2 = sigma * sigma, c = th2 + sg2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / th2;
    }
  }
  R Rm[3][3], W[3][3];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) {
      const R I = a == b ? 1.0 : 0.0;
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
__device__ __forceinline__ S3 compose(const S3& a, const S3& b) { return {qmul(a.r, b.r), add(scale(qrot(a.r, b.t), a.s), a.t), a.s * b.s}; }
__device__ __forceinline__ S3 inverse(const S3& a) {
  const Q4 rc{-a.r.x, -a.r.y, -a.r.z, a.r.w};
  return {rc, qrot(rc, scale(a.t, -1. / a.s)), 1. / a.s};
}
__device__ __forceinline__ S3 oplus(const S3& S, const R* x, bool fix, bool limitB = false) {   // VertexSim3Expmap::oplusImpl
  R u[7];
#pragma unroll
  for (int k = 0; k < 7; k++) u[k] = x[k];
  if (fix) u[6] = 0;
  return compose(sim3Exp(u, limitB), S);
}
__device__ __forceinline__ V3 sim3Map(const S3& S, V3 p) { return add(scale(qrot(S.r, p), S.s), S.t); }   // Sim3::map: s * (r * xyz) + t

// Sim3::log() (types/sim3.h): sigma = log(s), d = (trace(R) - 1) / 2, omega from deltaR(R) = (R21 - R12, R02 - R20, R10 - R01), the four
// branches on |sigma| < 1e-5 and d > 1 - 1e-5, W = A Omega + B Omega^2 + C I and upsilon = W.lu().solve(t) in the order of Eigen's
// PartialPivLU for a 3x3: per column the row of the largest |entry| from the diagonal down (the first one on a tie) is swapped up, the
// column below the pivot is divided by it, the trailing block takes the rank-1 update; then the unit-lower and the upper substitution.
__device__ __forceinline__ void sim3Log(const S3& S, R* res) {
  const R sigma = log(S.s), eps = 0.00001;
  R Rm[3][3];
  qToR(S.r, Rm);
  const R d = 0.5 * (Rm[0][0] + Rm[1][1] + Rm[2][2] - 1);
  const R dR[3] = {Rm[2][1] - Rm[1][2], Rm[0][2] - Rm[2][0], Rm[1][0] - Rm[0][1]};
  R om[3], A, B, C;
  if (fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) {
#pragma unroll
      for (int k = 0; k < 3; k++) om[k] = 0.5 * dR[k];
      A = 1. / 2.; B = 1. / 6.;
    } else {
      const R theta = acos(d), th2 = theta * theta, f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
      for (int k = 0; k < 3; k++) om[k] = f * dR[k];
      A = (1 - cos(theta)) / th2;
      B = (theta - sin(theta)) / (th2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (d > 1 - eps) {
      const R sg2 = sigma * sigma;
#pragma unroll
      for (int k = 0; k < 3; k++) om[k] = 0.5 * dR[k];
      A = ((sigma - 1) * S.s + 1) / sg2;
      B = ((0.5 * sg2 - sigma + 1) * S.s - 1) / (sg2 * sigma);   // the limit form, as under limitB in sim3Exp
    } else {
      const R theta = acos(d), f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
      for (int k = 0; k < 3; k++) om[k] = f * dR[k];
      const R th2 = theta * theta, a = S.s * sin(theta), b = S.s * cos(theta), c = th2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) / th2;
    }
  }
  const R Om[3][3] = {{0, -om[2], om[1]}, {om[2], 0, -om[0]}, {-om[1], om[0], 0}};
  R W[3][3];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) {
      const R o2 = Om[a][0] * Om[0][b] + Om[a][1] * Om[1][b] + Om[a][2] * Om[2][b];
      W[a][b] = (A * Om[a][b] + B * o2) + (a == b ? C : 0.0);
    }
  R y[3] = {S.t.x, S.t.y, S.t.z};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int piv = k;
#pragma unroll
    for (int r = k + 1; r < 3; r++)
      if (fabs(W[r][k]) > fabs(W[piv][k])) piv = r;
#pragma unroll
    for (int r = k + 1; r < 3; r++)
      if (piv == r) {   // written per candidate row so that every index stays a compile-time constant
#pragma unroll
        for (int c = 0; c < 3; c++) { const R tmp = W[k][c]; W[k][c] = W[r][c]; W[r][c] = tmp; }
        const R tmp = y[k]; y[k] = y[r]; y[r] = tmp;
      }
#pragma unroll
    for (int r = k + 1; r < 3; r++) {
      W[r][k] = W[r][k] / W[k][k];
#pragma unroll
      for (int c = k + 1; c < 3; c++) W[r][c] -= W[r][k] * W[k][c];
    }
  }
  y[1] -= W[1][0] * y[0];
  y[2] -= W[2][0] * y[0]; y[2] -= W[2][1] * y[1];
  y[2] = y[2] / W[2][2];
  y[1] = (y[1] - W[1][2] * y[2]) / W[1][1];
  y[0] = ((y[0] - W[0][1] * y[1]) - W[0][2] * y[2]) / W[0][0];
#pragma unroll
  for (int k = 0; k < 3; k++) { res[k] = om[k]; res[3 + k] = y[k]; }
  res[6] = sigma;
}

}  // namespace sim3
}  // namespace ydorb
