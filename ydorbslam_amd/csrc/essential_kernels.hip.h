// gfx950 HIP kernels of the essential-graph optimisation (ydorb_essential_graph_optimize).
//
// Restated from ORB-SLAM2 Optimizer::OptimizeEssentialGraph (src/Optimizer.cc) over g2o's VertexSim3Expmap / EdgeSim3
// (types/types_seven_dof_expmap.h, types/sim3.h), BaseBinaryEdge's central-difference Jacobians (core/base_binary_edge.hpp, delta 1e-9)
// and its constructQuadraticForm, in fp64 under the contract of DESIGN.md section 2 ("Essential graph: the arithmetic contract").  The
// Sim3 algebra is sim3_math.hip.h's, the fixed-order sums are g2o_math.hip.h's, the dense factorisation is the BA's (ba_solver.hip
// exports its launch sequence), and the Levenberg-Marquardt schedule runs on the host (lm_schedule.h).
//
// k_ess_linearize  one wave per edge: lanes 0..27 each evaluate the error at one perturbed estimate (vertex side x dimension x sign),
//                  lane 28 evaluates the error itself; the Jacobian columns are the pairwise differences, the 7x7 blocks J^T J and the
//                  two J^T e go to per-edge slots.  A lane-per-edge form (not built) would keep 2 x 49 Jacobian doubles next to the Sim3
//                  temporaries of an evaluation; here a lane holds one 7-vector (DESIGN.md section 6i has the resource figures).
// k_ess_assemble   one wave per free vertex: clears the vertex's 7 rows of the dense S, then sums the stored blocks of its incident
//                  edges in edge order (diagonal) and per neighbour in edge order (off-diagonal), adds lambda, writes b.  No atomics.
//                  The sums are ess_vertex_sums, which the skyline's k_ess_assemble_sky runs over the envelope.
// k_ess_update     one lane per free vertex: trial estimate oplus(estimate, x) and the vertex's term of computeScale.
// k_ess_chi2       one lane per edge: chi2 of the trial estimate.
// k_ess_sum        one workgroup: the chi2 and scale sums in a fixed order, plus the factorisation's status, for the one read-back.
// k_ess_points     one lane per map point: correctedSwr.map(Srw.map(p)).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sim3_math.hip.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace ess {

using g2o::R; using g2o::V3; using g2o::Q4; using g2o::block_sums;
using sim3::S3; using sim3::compose; using sim3::inverse; using sim3::sim3Log; using sim3::sim3Map;

// oplusImpl with the limit form of the exponential's B (sim3_math.hip.h): exp and log are then inverses of each other in every branch
__device__ __forceinline__ S3 essOplus(const S3& S, const R* x, bool fix) { return sim3::oplus(S, x, fix, true); }

__device__ __forceinline__ S3 loadS3(const R* p) { return {{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}, p[7]}; }
__device__ __forceinline__ void storeS3(R* p, const S3& S) {
  p[0] = S.r.x; p[1] = S.r.y; p[2] = S.r.z; p[3] = S.r.w; p[4] = S.t.x; p[5] = S.t.y; p[6] = S.t.z; p[7] = S.s;
}
// EdgeSim3::computeError: log(C * v0 * v1^-1)
__device__ __forceinline__ void essError(const S3& C, const S3& Vi, const S3& Vj, R* e) { sim3Log(compose(compose(C, Vi), inverse(Vj)), e); }
__device__ __forceinline__ R dot7(const R* e) {   // chi2 with information = identity, k ascending
  R s = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) s += e[k] * e[k];
  return s;
}

constexpr int kJ = 98;    // per edge: Jacobians [side][row k][column d]
constexpr int kH = 147;   // per edge: J0^T J0, J0^T J1, J1^T J1, each [r][c]
constexpr int kB = 14;    // per edge: -J0^T e, -J1^T e

// linearizeOplus + constructQuadraticForm of edge blockIdx.x.  freeOf[v] < 0: the vertex is fixed; g2o does not differentiate with
// respect to it, its Jacobian is stored as zero and nothing of it is assembled.
__global__ __launch_bounds__(64) void k_ess_linearize(int E, const R* __restrict__ est, const int* __restrict__ freeOf, const int* __restrict__ v0,
                                                      const int* __restrict__ v1, const R* __restrict__ meas, int fixScale, R* __restrict__ err,
                                                      R* __restrict__ chiE, R* __restrict__ Jout, R* __restrict__ Hb, R* __restrict__ bb) {
  __shared__ R Jl[2][7][7];
  __shared__ R e0[7];
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= E) return;
  const int vi = v0[e], vj = v1[e];
  const S3 C = loadS3(meas + 8 * (size_t)e);
  S3 Vi = loadS3(est + 8 * (size_t)vi), Vj = loadS3(est + 8 * (size_t)vj);
  const int side = lane >= 14 ? 1 : 0, d = (lane - 14 * side) >> 1, sg = lane & 1;
  const R dlt = 1e-9, scalar = 1.0 / (2 * dlt);
  if (lane < 28) {
    R u[7];
#pragma unroll
    for (int k = 0; k < 7; k++) u[k] = k == d ? (sg ? -dlt : dlt) : 0.0;
    const S3 P = essOplus(side ? Vj : Vi, u, fixScale != 0);
    if (side) Vj = P; else Vi = P;
  }
  R ev[7];
  essError(C, Vi, Vj, ev);
  const bool fixedSide = freeOf[side ? vj : vi] < 0;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const R minus = __shfl_xor(ev[k], 1, 64);   // lane + 1 holds the error at -delta
    if (lane < 28 && !sg) Jl[side][k][d] = fixedSide ? 0.0 : scalar * (ev[k] - minus);
  }
  if (lane == 28) {
#pragma unroll
    for (int k = 0; k < 7; k++) { e0[k] = ev[k]; err[7 * (size_t)e + k] = ev[k]; }
    chiE[e] = dot7(ev);
  }
  __syncthreads();
  const R* Jf = &Jl[0][0][0];
  for (int idx = lane; idx < kJ; idx += 64) Jout[kJ * (size_t)e + idx] = Jf[idx];
  for (int idx = lane; idx < kH + kB; idx += 64) {
    if (idx < kH) {
      const int blk = idx / 49, rc = idx - 49 * blk, r = rc / 7, c = rc - 7 * r;
      const int sa = blk == 2 ? 1 : 0, sb = blk == 0 ? 0 : 1;
      R s = 0;
#pragma unroll
      for (int k = 0; k < 7; k++) s += Jl[sa][k][r] * Jl[sb][k][c];
      Hb[kH * (size_t)e + idx] = s;
    } else {
      const int t = idx - kH, sd = t / 7, r = t - 7 * sd;
      R s = 0;
#pragma unroll
      for (int k = 0; k < 7; k++) s += Jl[sd][k][r] * (-e0[k]);
      bb[kB * (size_t)e + t] = s;
    }
  }
}

// The three sums of free vertex a, one wave: lanes 0 .. 48 sum entry (r, c) of the diagonal block over the incident edges in edge order
// (plus lambda) and of one block per free neighbour in edge order, lanes 49 .. 55 an entry of b.  incStart / incE: per free vertex its
// incident edges as (edge << 1 | side) in edge order; incN / incO: the same entries ordered by the neighbour's free index (fixed
// neighbours, -1, first), edge order kept inside a neighbour.  Where the sums go is the destination's business: dst.diag(r, c, v),
// dst.nbr(o, r, c, v) for neighbour o's block (a destination may skip it), dst.b(r, v).  k_ess_assemble and k_ess_assemble_sky
// (essential_skyline.hip.h) are this body over their own storage.
template <class Dst> __device__ __forceinline__ void ess_vertex_sums(int a, int lane, R lambda, const int* __restrict__ incStart,
                                                                     const int* __restrict__ incE, const int* __restrict__ incN,
                                                                     const int* __restrict__ incO, const R* __restrict__ Hb,
                                                                     const R* __restrict__ bb, const Dst& dst) {
  const int q0 = incStart[a], q1 = incStart[a + 1];
  if (lane < 49) {
    const int r = lane / 7, c = lane - 7 * r;
    R s = 0;
    for (int q = q0; q < q1; q++) {
      const int ent = incE[q];
      s += Hb[kH * (size_t)(ent >> 1) + ((ent & 1) ? 98 : 0) + lane];
    }
    if (r == c) s += lambda;
    dst.diag(r, c, s);
    int cur = -1;
    R acc = 0;
    for (int q = q0; q < q1; q++) {
      const int o = incO[q];
      if (o < 0) continue;
      if (o != cur) {
        if (cur >= 0) dst.nbr(cur, r, c, acc);
        cur = o; acc = 0;
      }
      const int ent = incN[q];
      acc += Hb[kH * (size_t)(ent >> 1) + 49 + ((ent & 1) ? 7 * c + r : lane)];   // side 1: the block of (j, i) is the transpose
    }
    if (cur >= 0) dst.nbr(cur, r, c, acc);
  } else if (lane < 56) {
    const int r = lane - 49;
    R s = 0;
    for (int q = q0; q < q1; q++) {
      const int ent = incE[q];
      s += bb[kB * (size_t)(ent >> 1) + 7 * (ent & 1) + r];
    }
    dst.b(r, s);
  }
}

// Vertex a's 7 rows of the dense S, every neighbour's block, and b by free vertex (twice)
struct EssDenseDst {
  R* rows; int n, a; R *bkeep, *bwork;
  __device__ void diag(int r, int c, R v) const { rows[(size_t)r * n + 7 * a + c] = v; }
  __device__ void nbr(int o, int r, int c, R v) const { rows[(size_t)r * n + 7 * o + c] = v; }
  __device__ void b(int r, R v) const { bkeep[7 * a + r] = v; bwork[7 * a + r] = v; }
};

// H + lambda I into the dense S ([n][n] row-major, n = 7 nF padded to the factorisation's tile with a unit diagonal) and b (twice: the
// factorisation's forward substitution consumes bwork).  The whole of S is written on every call: the factorisation overwrites it, and
// the arena keeps earlier calls' contents.
__global__ __launch_bounds__(64) void k_ess_assemble(int nF, int n, R lambda, const int* __restrict__ incStart, const int* __restrict__ incE,
                                                     const int* __restrict__ incN, const int* __restrict__ incO, const R* __restrict__ Hb,
                                                     const R* __restrict__ bb, R* __restrict__ S, R* __restrict__ bkeep, R* __restrict__ bwork,
                                                     int* __restrict__ status) {
  const int a = blockIdx.x, lane = threadIdx.x;
  if (a >= nF) {   // the padding rows, and the status word of this trial's factorisation
    if (lane == 0) status[0] = 0;
    for (int r = 7 * nF; r < n; r++) {
      for (int c = lane; c < n; c += 64) S[(size_t)r * n + c] = r == c ? 1.0 : 0.0;
      if (lane == 0) { bkeep[r] = 0; bwork[r] = 0; }
    }
    return;
  }
  R* rows = S + (size_t)7 * a * n;
  for (size_t i = lane; i < (size_t)7 * n; i += 64) rows[i] = 0;
  __syncthreads();   // the cleared rows are in memory before the blocks go over them
  ess_vertex_sums(a, lane, lambda, incStart, incE, incN, incO, Hb, bb, EssDenseDst{rows, n, a, bkeep, bwork});
}

// push + update(x): next[v] = oplus(cur[v], x_v) for every free vertex; sv[f] = sum_k x[k] (lambda x[k] + b[k]), its part of computeScale
__global__ __launch_bounds__(256) void k_ess_update(int nF, const int* __restrict__ vertOf, const R* __restrict__ cur, R* __restrict__ next,
                                                    const R* __restrict__ x, const R* __restrict__ b, R lambda, int fixScale, R* __restrict__ sv) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nF) return;
  const int v = vertOf[f];
  R xv[7], s = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) { xv[k] = x[7 * f + k]; s += xv[k] * (lambda * xv[k] + b[7 * f + k]); }
  storeS3(next + 8 * (size_t)v, essOplus(loadS3(cur + 8 * (size_t)v), xv, fixScale != 0));
  sv[f] = s;
}

__global__ __launch_bounds__(256) void k_ess_chi2(int E, const R* __restrict__ est, const int* __restrict__ v0, const int* __restrict__ v1,
                                                  const R* __restrict__ meas, R* __restrict__ chiE) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  R ev[7];
  essError(loadS3(meas + 8 * (size_t)e), loadS3(est + 8 * (size_t)v0[e]), loadS3(est + 8 * (size_t)v1[e]), ev);
  chiE[e] = dot7(ev);
}

// scal[0] = sum chiE, scal[1] = sum sv, scal[2] = status[0]: every thread sums its stride of 256 in ascending order, then the workgroup
// sums of g2o_math.hip.h.  nS == 0 leaves the scale at 0 (the chi2 at the top of an iteration).
__global__ __launch_bounds__(256) void k_ess_sum(const R* __restrict__ chiE, int nE, const R* __restrict__ sv, int nS, const int* __restrict__ status,
                                                 R* __restrict__ scal) {
  __shared__ R part[4][2];
  R a[2] = {0, 0}, o[2];
  for (int i = threadIdx.x; i < nE; i += 256) a[0] += chiE[i];
  for (int i = threadIdx.x; i < nS; i += 256) a[1] += sv[i];
  block_sums<2>(a, part, o);
  if (threadIdx.x == 0) { scal[0] = o[0]; scal[1] = o[1]; scal[2] = (R)status[0]; }
}

// MapPoint correction of OptimizeEssentialGraph: Srw = the reference keyframe's estimate before, correctedSwr = the inverse of its
// estimate after; float in, float out, the chain in double
__global__ __launch_bounds__(256) void k_ess_points(int nP, const float* __restrict__ pts, const int* __restrict__ ref, const R* __restrict__ estIn,
                                                    const R* __restrict__ estOut, float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nP) return;
  const int v = ref[p];
  const V3 X{(R)pts[3 * (size_t)p], (R)pts[3 * (size_t)p + 1], (R)pts[3 * (size_t)p + 2]};
  const V3 Y = sim3Map(inverse(loadS3(estOut + 8 * (size_t)v)), sim3Map(loadS3(estIn + 8 * (size_t)v), X));
  out[3 * (size_t)p] = (float)Y.x; out[3 * (size_t)p + 1] = (float)Y.y; out[3 * (size_t)p + 2] = (float)Y.z;
}

}  // namespace ess
}  // namespace ydorb
