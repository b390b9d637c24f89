// gfx950 HIP kernels of the loop-closure Sim3 check (ydorb_sim3_ransac / ydorb_sim3_optimize).
//
// Restated from ORB-SLAM2, which YDORBSLAM renames:
//   * Sim3Solver::iterate / ComputeSim3 (Horn 1987) / CheckInliers / Project (src/Sim3Solver.cc), in fp32 under the written-order
//     contract of DESIGN.md section 2 ("Sim3 RANSAC"): +, -, *, / and sqrt only, every op a single IEEE operation
//     (-ffp-contract=off), so the kernels equal a CPU restatement bit for bit.  The eigenvector of Horn's 4x4 comes from a fixed-sweep
//     cyclic Jacobi and R from the normalised quaternion, which equals the reference's atan2 -> Rodrigues in exact arithmetic.
//   * Optimizer::OptimizeSim3 (src/Optimizer.cc) over g2o's VertexSim3Expmap (types/sim3.h) with EdgeSim3ProjectXYZ /
//     EdgeInverseSim3ProjectXYZ (types_seven_dof_expmap.h), BaseBinaryEdge's central-difference Jacobian (delta 1e-9), Huber and the
//     Levenberg-Marquardt trial loop of core/optimization_algorithm_levenberg.cpp: k_pose_optimize's structure (ba_kernels.hip.h)
//     with a 7-vector and two edges per pair, in fp64.  The quaternion algebra, Huber, the fixed-order sums, the dense LL^T solve
//     and the lambda control are those of g2o_math.hip.h, shared with the BA kernels.
// Layout of the RANSAC: one wave per hypothesis (DESIGN.md section 6c has the comparison with a lane per hypothesis).  Every lane of
// the wave solves Horn redundantly on the same three pairs (wave-uniform values: no broadcast, no divergence), then the wave strides
// over the problem's pairs in global memory 64 at a time and counts inliers with a ballot, so a problem of any size needs no LDS.
// The ordered replay of iterate() is one wave per problem that reads the counts back in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "g2o_math.hip.h"
#include "sim3_math.hip.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace sim3 {

// ------------------------------------------------------------------------------------------------------------ RANSAC (fp32)
struct RansacDev {      // one problem; offsets in elements of the packed arrays
  int n, fix, minInl, maxIts;
  int nEval;            // hypotheses to evaluate (from next_hyp on, at most max_its - next_hyp)
  int bestIn;           // mnBestInliers on entry
  int pairOff;          // first pair in X1 / X2 (x3), P1 / P2 (x2), maxErr1 / maxErr2, mask
  int hypOff;           // first hypothesis in triples (x3) and counts
  float K1[4], K2[4];
};
struct RansacOut { int ret, best, bestIdx, pad; float T[13]; };   // T = R, t, s of hypothesis bestIdx

__device__ __forceinline__ float dot3f(const float* a, const float* b) {   // products exact in double, summed in double
  return (float)(((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2]);
}

struct Hyp { float R[9], t[3], s, A12[9], A21[9], t21[3]; };   // T12 = [A12 | t], T21 = [A21 | t21]

// ComputeSim3 on pairs idx[0..2]
__device__ __forceinline__ void horn(const float* __restrict__ X1, const float* __restrict__ X2, const int* idx, bool fixScale, Hyp& h) {
  float P1[3][3], P2[3][3];
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int r = 0; r < 3; r++) { P1[r][c] = X1[3 * idx[c] + r]; P2[r][c] = X2[3 * idx[c] + r]; }
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) / 3.0f;
    O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) / 3.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) { Pr1[r][c] = P1[r][c] - O1[r]; Pr2[r][c] = P2[r][c] - O2[r]; }
  }
  float M[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
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
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < i; j++) A[i][j] = A[j][i];
  float V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 8; sweep++)
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        const float apq = A[p][q];
        if (apq == 0.0f) continue;
        const float theta = (A[q][q] - A[p][p]) / (2.0f * apq);
        float t = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
        if (theta < 0.0f) t = -t;
        const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  int im = 0;
#pragma unroll
  for (int i = 1; i < 4; i++) if (A[i][i] > A[im][im]) im = i;
  float w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
  for (int i = 1; i < 4; i++)
    if (im == i) { w = V[0][i]; x = V[1][i]; y = V[2][i]; z = V[3][i]; }
  if (w < 0.0f) { w = -w; x = -x; y = -y; z = -z; }
  const float n = sqrtf(((w * w + x * x) + y * y) + z * z);
  w = w / n; x = x / n; y = y / n; z = z / n;
  float* R = h.R;
  R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - w * z); R[2] = 2.0f * (x * z + w * y);
  R[3] = 2.0f * (x * y + w * z); R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - w * x);
  R[6] = 2.0f * (x * z - w * y); R[7] = 2.0f * (y * z + w * x); R[8] = 1.0f - 2.0f * (x * x + y * y);
  float s = 1.0f;
  if (!fixScale) {
    double nom = 0, den = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float col[3] = {Pr2[0][c], Pr2[1][c], Pr2[2][c]};
        const float p3 = dot3f(R + 3 * i, col);
        nom += (double)Pr1[i][c] * (double)p3;
        den += (double)(p3 * p3);
      }
    s = (float)(nom / den);
  }
  h.s = s;
#pragma unroll
  for (int i = 0; i < 3; i++) h.t[i] = O1[i] - s * dot3f(R + 3 * i, O2);
#pragma unroll
  for (int k = 0; k < 9; k++) h.A12[k] = s * R[k];
  const double inv = 1.0 / (double)s;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) h.A21[3 * i + j] = (float)(inv * (double)R[3 * j + i]);
#pragma unroll
  for (int i = 0; i < 3; i++) h.t21[i] = -dot3f(h.A21 + 3 * i, h.t);
}

// squared pixel error of X mapped by [A | t] and projected through K against P (Project + CheckInliers)
__device__ __forceinline__ float reproj(const float* A, const float* t, const float* X, const float* K, const float* P) {
  const float c0 = dot3f(A, X) + t[0], c1 = dot3f(A + 3, X) + t[1], c2 = dot3f(A + 6, X) + t[2];
  const float invz = 1.0f / c2;
  const float u = K[0] * (c0 * invz) + K[2], v = K[1] * (c1 * invz) + K[3];
  const float d0 = P[0] - u, d1 = P[1] - v;
  return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}
__device__ __forceinline__ bool inlier(const Hyp& h, const float* __restrict__ X1, const float* __restrict__ X2, const float* __restrict__ P1,
                                       const float* __restrict__ P2, const float* __restrict__ me1, const float* __restrict__ me2,
                                       const float* K1, const float* K2, int i) {
  const float e1 = reproj(h.A12, h.t, X2 + 3 * i, K1, P1 + 2 * i);
  const float e2 = reproj(h.A21, h.t21, X1 + 3 * i, K2, P2 + 2 * i);
  return e1 < me1[i] && e2 < me2[i];
}

constexpr int kHypWaves = 4;   // hypotheses per workgroup

// counts[hypOff + h] = inliers of hypothesis h of problem blockIdx.y
__global__ __launch_bounds__(64 * kHypWaves) void k_sim3_hypotheses(const RansacDev* __restrict__ probs, const float* __restrict__ X1,
                                                                    const float* __restrict__ X2, const float* __restrict__ P1,
                                                                    const float* __restrict__ P2, const float* __restrict__ me1,
                                                                    const float* __restrict__ me2, const int* __restrict__ triples,
                                                                    int* __restrict__ counts) {
  const RansacDev& pr = probs[blockIdx.y];
  const int h = blockIdx.x * kHypWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (h >= pr.nEval) return;
  const int o = pr.pairOff;
  const float *x1 = X1 + 3 * o, *x2 = X2 + 3 * o, *p1 = P1 + 2 * o, *p2 = P2 + 2 * o, *m1 = me1 + o, *m2 = me2 + o;
  const int* tri = triples + 3 * (pr.hypOff + h);
  const int idx[3] = {tri[0], tri[1], tri[2]};
  Hyp hy;
  horn(x1, x2, idx, pr.fix != 0, hy);
  int cnt = 0;
  for (int base = 0; base < pr.n; base += 64) {
    const int i = base + lane;
    const bool in = i < pr.n && inlier(hy, x1, x2, p1, p2, m1, m2, pr.K1, pr.K2, i);
    cnt += __popcll(__ballot(in));
  }
  if (lane == 0) counts[pr.hypOff + h] = cnt;
}

// iterate()'s ordered commit, one wave per problem: the first hypothesis with count >= the running best and > minInliers returns;
// the best state is the last hypothesis up to there with count >= the running best.  Recomputes the winner's mask.
__global__ __launch_bounds__(64) void k_sim3_replay(const RansacDev* __restrict__ probs, const float* __restrict__ X1,
                                                   const float* __restrict__ X2, const float* __restrict__ P1, const float* __restrict__ P2,
                                                   const float* __restrict__ me1, const float* __restrict__ me2,
                                                   const int* __restrict__ triples, const int* __restrict__ counts,
                                                   RansacOut* __restrict__ out, uint8_t* __restrict__ mask) {
  const RansacDev& pr = probs[blockIdx.x];
  const int lane = threadIdx.x;
  int best = pr.bestIn, ret = -1, bestIdx = -1;
  for (int base = 0; base < pr.nEval && ret < 0; base += 64) {
    const int c = base + lane < pr.nEval ? counts[pr.hypOff + base + lane] : -1;
    const int m = min(64, pr.nEval - base);
    for (int j = 0; j < m; j++) {
      const int cj = __shfl(c, j, 64);
      if (cj >= best) {
        best = cj; bestIdx = base + j;
        if (cj > pr.minInl) { ret = base + j; break; }
      }
    }
  }
  const int o = pr.pairOff;
  const float *x1 = X1 + 3 * o, *x2 = X2 + 3 * o, *p1 = P1 + 2 * o, *p2 = P2 + 2 * o, *m1 = me1 + o, *m2 = me2 + o;
  Hyp hy;
  if (bestIdx >= 0) {
    const int* tri = triples + 3 * (pr.hypOff + bestIdx);
    const int idx[3] = {tri[0], tri[1], tri[2]};
    horn(x1, x2, idx, pr.fix != 0, hy);
  }
  for (int i = lane; i < pr.n; i += 64) mask[o + i] = ret >= 0 && inlier(hy, x1, x2, p1, p2, m1, m2, pr.K1, pr.K2, i);
  if (lane == 0) {
    RansacOut& r = out[blockIdx.x];
    r.ret = ret; r.best = best; r.bestIdx = bestIdx;
    if (bestIdx >= 0) {
#pragma unroll
      for (int k = 0; k < 9; k++) r.T[k] = hy.R[k];
#pragma unroll
      for (int k = 0; k < 3; k++) r.T[9 + k] = hy.t[k];
      r.T[12] = hy.s;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ Sim3 LM (fp64)
// obs - cam_map(project(S.map(X)))
__device__ __forceinline__ void projErr(const S3& S, const R* X, const R* K, const R* obs, R* e) {
  const V3 p = add(scale(qrot(S.r, V3{X[0], X[1], X[2]}), S.s), S.t);
  e[0] = obs[0] - ((p.x / p.z) * K[0] + K[2]);
  e[1] = obs[1] - ((p.y / p.z) * K[1] + K[3]);
}
__device__ __forceinline__ R chi2(const R* e, R w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

constexpr int kOptThreads = 256;   // 4 waves
constexpr int kAcc = 36;           // packed upper 7x7 (28) + b (7) + robust chi2

struct OptArgs {
  const int* start;
  R* S12;
  const R *K1, *K2;
  const uint8_t* fix;
  const R *X1, *X2, *o1, *o2, *w1, *w2;
  R thr, delta;
  R* err;            // [pairs][4] g2o's _error of both edges as last computed
  uint8_t* active;   // [pairs] 1 = pair in the graph
  uint8_t* outlier;
  int* nIn;
  R* chi2Log;        // [n][2]
  int* trials;
};

struct OptLds {
  R part[4][kAcc];
  S3 pert[7][2][2];  // [dim][+delta, -delta][estimate, its inverse] of the numeric Jacobian
};

// computeActiveErrors + robust chi2 of the pairs in the graph at estimate S (every edge's error stored)
__device__ __forceinline__ R active_chi(const OptArgs& a, int e0, int E, const S3& S, const S3& Si, const R* K1, const R* K2, OptLds& L) {
  R chi = 0;
  for (int i = threadIdx.x; i < E; i += kOptThreads) {
    const int e = e0 + i;
    if (!a.active[e]) continue;
    R* er = a.err + 4 * e;
    projErr(S, a.X2 + 3 * e, K1, a.o1 + 2 * e, er);
    projErr(Si, a.X1 + 3 * e, K2, a.o2 + 2 * e, er + 2);
    R r0, r1;
    huber(chi2(er, a.w1[e]), a.delta, &r0, &r1); chi += r0;
    huber(chi2(er + 2, a.w2[e]), a.delta, &r0, &r1); chi += r0;
  }
  return block_sum1(chi, L.part);
}

// SparseOptimizer::optimize(iters) with OptimizationAlgorithmLevenberg; returns currentChi of the last iteration
__device__ R lm_optimize(const OptArgs& a, int e0, int E, S3& S, const R* K1, const R* K2, bool fix, int iters, int& trials, OptLds& L) {
  const R dlt = 1e-9, scalar = 1.0 / (2 * dlt);
  R lambda = 0, ni = 2, currentChi = 0;
  const int tid = threadIdx.x;
  for (int it = 0; it < iters; it++) {
    __syncthreads();   // the previous iteration's readers of L.pert are done
    if (tid < 14) {
      const int d = tid >> 1, sg = tid & 1;
      R u[7] = {0, 0, 0, 0, 0, 0, 0};
      u[d] = sg ? -dlt : dlt;
      const S3 P = oplus(S, u, fix);
      L.pert[d][sg][0] = P;
      L.pert[d][sg][1] = inverse(P);
    }
    __syncthreads();
    const S3 Si = inverse(S);
    R acc[kAcc];
#pragma unroll
    for (int k = 0; k < kAcc; k++) acc[k] = 0;
    for (int i = tid; i < E; i += kOptThreads) {
      const int e = e0 + i;
      if (!a.active[e]) continue;
      R* er = a.err + 4 * e;
      projErr(S, a.X2 + 3 * e, K1, a.o1 + 2 * e, er);
      projErr(Si, a.X1 + 3 * e, K2, a.o2 + 2 * e, er + 2);
#pragma unroll
      for (int side = 0; side < 2; side++) {
        const R* ev = er + 2 * side;
        const R w = side ? a.w2[e] : a.w1[e];
        const R* X = side ? a.X1 + 3 * e : a.X2 + 3 * e;
        const R* K = side ? K2 : K1;
        const R* ob = side ? a.o2 + 2 * e : a.o1 + 2 * e;
        R J[2][7];
#pragma unroll
        for (int d = 0; d < 7; d++) {
          R ep[2], em[2];
          projErr(L.pert[d][0][side], X, K, ob, ep);
          projErr(L.pert[d][1][side], X, K, ob, em);
          J[0][d] = scalar * (ep[0] - em[0]);
          J[1][d] = scalar * (ep[1] - em[1]);
        }
        R r0, r1;
        huber(chi2(ev, w), a.delta, &r0, &r1);
        acc[35] += r0;
        const R W = r1 * w, om0 = -(w * ev[0]) * r1, om1 = -(w * ev[1]) * r1;
        int k = 0;
#pragma unroll
        for (int r = 0; r < 7; r++)
#pragma unroll
          for (int c = r; c < 7; c++, k++) acc[k] += J[0][r] * W * J[0][c] + J[1][r] * W * J[1][c];
#pragma unroll
        for (int r = 0; r < 7; r++) acc[28 + r] += J[0][r] * om0 + J[1][r] * om1;
      }
    }
    R Sm[kAcc];
    block_sums<kAcc>(acc, L.part, Sm);
    R Hs[28], b[7];
#pragma unroll
    for (int k = 0; k < 28; k++) Hs[k] = Sm[k];
#pragma unroll
    for (int k = 0; k < 7; k++) b[k] = Sm[28 + k];
    currentChi = Sm[35];
    if (it == 0) { lambda = lambda_init<7>(Hs); ni = 2; }   // computeLambdaInit
    R rho = 0, x[7] = {0, 0, 0, 0, 0, 0, 0};
    int qmax = 0;
    do {
      const S3 Sb = S;   // push()
      const bool ok = dense_solve<7>(Hs, lambda, b, x);
      S = oplus(S, x, fix);   // g2o applies _x even after a failed solve
      const R tempChi = active_chi(a, e0, E, S, inverse(S), K1, K2, L);
      R sc = 1e-3;   // computeScale() + 1e-3
#pragma unroll
      for (int j = 0; j < 7; j++) sc += x[j] * (lambda * x[j] + b[j]);
      if (!lm_judge(lambda, ni, currentChi, rho, tempChi, sc, ok)) {
        S = Sb;   // pop()
        if (!isfinite(lambda)) { qmax++; trials++; break; }
      }
      qmax++; trials++;
    } while (rho < 0 && qmax < 10);
    if (qmax == 10 || rho == 0 || !isfinite(lambda)) break;
  }
  return currentChi;
}

// the pairs in the graph with chi2 > th2 on either edge (their g2o _error as last computed): leave the graph, become outliers
__device__ __forceinline__ int cull(const OptArgs& a, int e0, int E, OptLds& L) {
  int bad = 0;
  for (int i = threadIdx.x; i < E; i += kOptThreads) {
    const int e = e0 + i;
    if (!a.active[e]) continue;
    const R* er = a.err + 4 * e;
    if (chi2(er, a.w1[e]) > a.thr || chi2(er + 2, a.w2[e]) > a.thr) { a.active[e] = 0; a.outlier[e] = 1; bad++; }
  }
  const int n = (int)block_sum1((R)bad, L.part);
  __syncthreads();   // active[] of this cull is visible to the next pass
  return n;
}

__global__ __launch_bounds__(kOptThreads) void k_sim3_optimize(int nProb, OptArgs a) {
  __shared__ OptLds L;
  const int p = blockIdx.x, tid = threadIdx.x;
  if (p >= nProb) return;
  const int e0 = a.start[p], E = a.start[p + 1] - e0;
  if (tid < 2) a.chi2Log[2 * p + tid] = __longlong_as_double(0x7ff8000000000000ll);
  for (int i = tid; i < E; i += kOptThreads) { a.active[e0 + i] = 1; a.outlier[e0 + i] = 0; }
  if (E == 0) {   // no edge: g2o has no vertex to optimise and nCorr - nBad < 10
    if (tid == 0) { a.nIn[p] = 0; a.trials[p] = 0; }
    return;
  }
  __syncthreads();
  const R* s12 = a.S12 + 8 * p;
  S3 S{{s12[0], s12[1], s12[2], s12[3]}, {s12[4], s12[5], s12[6]}, s12[7]};
  const R K1[4] = {a.K1[4 * p], a.K1[4 * p + 1], a.K1[4 * p + 2], a.K1[4 * p + 3]};
  const R K2[4] = {a.K2[4 * p], a.K2[4 * p + 1], a.K2[4 * p + 2], a.K2[4 * p + 3]};
  const bool fix = a.fix[p] != 0;
  int trials = 0;
  const R chi1 = lm_optimize(a, e0, E, S, K1, K2, fix, 5, trials, L);
  const int nBad = cull(a, e0, E, L);
  int nIn = 0;
  R chi2s = __longlong_as_double(0x7ff8000000000000ll);
  if (E - nBad >= 10) {
    chi2s = lm_optimize(a, e0, E, S, K1, K2, fix, nBad > 0 ? 10 : 5, trials, L);
    nIn = E - nBad - cull(a, e0, E, L);
  }
  if (tid == 0) {
    a.chi2Log[2 * p] = chi1;
    a.chi2Log[2 * p + 1] = chi2s;
    a.nIn[p] = nIn;
    a.trials[p] = trials;
    if (E - nBad >= 10) {
      R* o = a.S12 + 8 * p;
      o[0] = S.r.x; o[1] = S.r.y; o[2] = S.r.z; o[3] = S.r.w; o[4] = S.t.x; o[5] = S.t.y; o[6] = S.t.z; o[7] = S.s;
    }
  }
}

}  // namespace sim3
}  // namespace ydorb
