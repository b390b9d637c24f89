// The g2o / Eigen pieces that every Levenberg-Marquardt back-end here restates, once: local and global BA and the pose-only
// optimisation (ba_kernels.hip.h, ba_solver.hip) and the Sim3 check (sim3_kernels.hip.h).  Quaternion algebra of Eigen and
// types/slam3d/se3quat.h, Huber of core/robust_kernel_impl.cpp, the fixed-order workgroup sums the bit-exact contract rests on,
// LinearSolverDense for a handful of unknowns, and the lambda control of core/optimization_algorithm_levenberg.cpp (lm_judge, which
// comes from the HIP-free lm_schedule.h so that the host schedule of BA shares it).
// Functions and types only - no __device__ / __constant__ variable and no kernel - so any translation unit includes it freely.
// The oracle and tests/*_ref stay independent restatements and do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "lm_schedule.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace g2o {

typedef double R;
struct V3 { R x, y, z; };
struct Q4 { R x, y, z, w; };

__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 scale(V3 a, R s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 qrot(Q4 q, V3 v) {  // Eigen quaternion * vector
  V3 qv{q.x, q.y, q.z};
  V3 uv = cross(qv, v);
  uv = add(uv, uv);
  return add(add(v, scale(uv, q.w)), cross(qv, uv));
}
__device__ __forceinline__ Q4 qmul(Q4 a, Q4 b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
          a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
__device__ __forceinline__ void qToR(Q4 q, R m[3][3]) {
  const R tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const R twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x, tyy = ty * q.y,
          tyz = tz * q.y, tzz = tz * q.z;
  m[0][0] = 1 - (tyy + tzz); m[0][1] = txy - twz; m[0][2] = txz + twy;
  m[1][0] = txy + twz; m[1][1] = 1 - (txx + tzz); m[1][2] = tyz - twx;
  m[2][0] = txz - twy; m[2][1] = tyz + twx; m[2][2] = 1 - (txx + tyy);
}
__device__ __forceinline__ Q4 rToQ(const R a[3][3]) {  // Eigen Quaternion(Matrix3)
  Q4 q;
  R t = a[0][0] + a[1][1] + a[2][2];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (a[2][1] - a[1][2]) * t;
    q.y = (a[0][2] - a[2][0]) * t;
    q.z = (a[1][0] - a[0][1]) * t;
  } else {
    int i = 0;
    if (a[1][1] > a[0][0]) i = 1;
    if (a[2][2] > a[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(a[i][i] - a[j][j] - a[k][k] + 1.0);
    R c[3];
    c[i] = 0.5 * t;
    t = 0.5 / t;
    q.w = (a[k][j] - a[j][k]) * t;
    c[j] = (a[j][i] + a[i][j]) * t;
    c[k] = (a[k][i] + a[i][k]) * t;
    q.x = c[0]; q.y = c[1]; q.z = c[2];
  }
  return q;
}
__device__ __forceinline__ void qnormalize(Q4& q) {  // se3quat.h:280-285
  if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
  const R n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  q.x /= n; q.y /= n; q.z /= n; q.w /= n;
}
__device__ __forceinline__ void huber(R e, R delta, R* rho0, R* rho1) {  // robust_kernel_impl.cpp:65-78
  const R dsqr = delta * delta;
  if (e <= dsqr) { *rho0 = e; *rho1 = 1.; }
  else { const R s = sqrt(e); *rho0 = 2 * s * delta - dsqr; *rho1 = delta / s; }
}

// Sums of a 4-wave workgroup in a fixed order (wave butterfly, then the wave partials 0..3), every thread gets every sum.
// `part` is LDS of the caller, rows at least K wide.
template <int K, int Stride>
__device__ __forceinline__ void block_sums(R (&v)[K], R (*part)[Stride], R (&out)[K]) {
  static_assert(K <= Stride, "a wave's partial sums do not fit its row of part");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  }
  __syncthreads();                       // the previous reduction's readers are done with `part`
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) part[wv][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) out[k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
}
template <int Stride>
__device__ __forceinline__ R block_sum1(R v, R (*part)[Stride]) {
  R a[1] = {v}, o[1];
  block_sums<1>(a, part, o);
  return o[0];
}

// LL^T of the NxN system (Hs = packed upper triangle, row by row) + lambda*I and both substitutions (LinearSolverDense,
// linear_solver_dense.h:66-109); false when not positive definite, and x is then left as it was.
template <int N>
__device__ __forceinline__ bool dense_solve(const R (&Hs)[N * (N + 1) / 2], R lambda, const R (&b)[N], R (&x)[N]) {
  R L[N][N];
  int k = 0;
#pragma unroll
  for (int r = 0; r < N; r++)
#pragma unroll
    for (int c = r; c < N; c++, k++) L[c][r] = Hs[k] + (r == c ? lambda : 0.0);   // lower triangle
#pragma unroll
  for (int j = 0; j < N; j++) {
    R d = L[j][j];
#pragma unroll
    for (int q = 0; q < j; q++) d -= L[j][q] * L[j][q];
    if (!(d > 0)) return false;
    d = sqrt(d);
    L[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < N; i++) {
      R s2 = L[i][j];
#pragma unroll
      for (int q = 0; q < j; q++) s2 -= L[i][q] * L[j][q];
      L[i][j] = s2 / d;
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) {
    R s2 = b[i];
#pragma unroll
    for (int q = 0; q < i; q++) s2 -= L[i][q] * x[q];
    x[i] = s2 / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    R s2 = x[i];
#pragma unroll
    for (int q = i + 1; q < N; q++) s2 -= L[q][i] * x[q];
    x[i] = s2 / L[i][i];
  }
  return true;
}

// computeLambdaInit (optimization_algorithm_levenberg.cpp) over a packed upper triangle: tau * max |diagonal|
template <int N>
__device__ __forceinline__ R lambda_init(const R (&Hs)[N * (N + 1) / 2]) {
  R mx = 0;
  int k = 0;
#pragma unroll
  for (int r = 0; r < N; r++) { mx = fmax(fabs(Hs[k]), mx); k += N - r; }
  return 1e-5 * mx;
}

}  // namespace g2o
}  // namespace ydorb
