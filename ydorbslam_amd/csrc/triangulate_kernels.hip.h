// gfx950 HIP kernel of ydorb_triangulate_matches: the geometry of LocalMapping::createNewMapPoints between the match list and the new
// MapPoints (ORB-SLAM2 LocalMapping::CreateNewMapPoints' loop body, which YDORBSLAM renames), in fp32 under the
// written-order contract of DESIGN.md section 2 ("createNewMapPoints"): +, -, *, / and sqrt only, every op a single IEEE operation
// (-ffp-contract=off), so the kernel equals the CPU restatement tests/triangulate_ref/triangulate_ref.cpp bit for bit.
// Layout: one lane per match over the concatenated matches of all problems; a lane finds its problem by a binary search of the CSR
// starts.  The host has gathered each match's two features (12 floats), so every per-match load is a coalesced 16-byte load; the two
// views' constants are wave-uniform loads except in the waves that straddle two problems.  A (as its four columns) and V of the
// one-sided Jacobi are 16 floats each and stay in registers: every index below is a compile-time constant.  No LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace ydorb {
namespace tri {

constexpr int kThreads = 256;
constexpr int kSweeps = 30;   // OpenCV's max_iter = max(m, 30); a bound, so NaN input terminates too

struct ViewDev {   // one keyframe's constants: 32 floats
  float Tcw[12], Rwc[9], Ow[3];
  float fx, fy, cx, cy, invfx, invfy, b, bf;
};
struct ProblemDev { int first, second; float ratioFactor; int pad; };
// one match as the host gathered it: f1 / f2 = (x, y, right_x, depth) of the two features, lv = (levelSigma2[octave1],
// levelSigma2[octave2], scaleFactors[octave1], scaleFactors[octave2])
struct Args {
  int nProblems, nMatches;
  const int* start;            // [nProblems + 1]
  const ProblemDev* problems;
  const ViewDev* views;
  const float4* f1; const float4* f2; const float4* lv;
  float* x3d;                  // [nMatches][3]
  uint8_t* status;             // [nMatches]
};

__device__ __forceinline__ float dot3(const float* a, float x, float y, float z) {   // products exact in double, summed in double
  return (float)(((double)a[0] * (double)x + (double)a[1] * (double)y) + (double)a[2] * (double)z);
}
__device__ __forceinline__ double dot3d(const float* a, float x, float y, float z) {
  return ((double)a[0] * (double)x + (double)a[1] * (double)y) + (double)a[2] * (double)z;
}
// row r of [R | t] times (x, y, z, 1): four terms summed in double, rounded once
__device__ __forceinline__ float row4(const float* T, int r, float x, float y, float z) {
  return (float)(dot3d(T + 4 * r, x, y, z) + (double)T[4 * r + 3]);
}

// cos(2 atan2(b / 2, d)) as (d^2 - h^2) / (d^2 + h^2), h = b / 2: one libm-free form for both sides
__device__ __forceinline__ float cos_stereo(float b, float d) {
  const float h = b / 2.0f;
  const double d2 = (double)d * (double)d, h2 = (double)h * (double)h;
  return (float)((d2 - h2) / (d2 + h2));
}

// One pair (I, J) of the one-sided Jacobi, OpenCV's JacobiSVDImpl_<float> with sqrt(p^2 + beta^2) for hypot.  a[i] is column i of A.
template <int I, int J>
__device__ __forceinline__ bool jacobi_pair(float (&a)[4][4], float (&v)[4][4], double (&w)[4]) {
  double p = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) p += (double)a[I][k] * (double)a[J][k];
  const double eps = (double)2.384185791015625e-07f;   // FLT_EPSILON * 2
  if (fabs(p) <= eps * sqrt(w[I] * w[J])) return false;
  p *= 2;
  const double beta = w[I] - w[J], gamma = sqrt(p * p + beta * beta);
  float c, s;
  if (beta < 0) {
    const double delta = (gamma - beta) * 0.5;
    s = (float)sqrt(delta / gamma);
    c = (float)(p / (gamma * (double)s * 2));
  } else {
    c = (float)sqrt((gamma + beta) / (gamma * 2));
    s = (float)(p / (gamma * (double)c * 2));
  }
  double na = 0, nb = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float t0 = c * a[I][k] + s * a[J][k];
    const float t1 = -s * a[I][k] + c * a[J][k];
    a[I][k] = t0; a[J][k] = t1;
    na += (double)t0 * (double)t0; nb += (double)t1 * (double)t1;
  }
  w[I] = na; w[J] = nb;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float t0 = c * v[I][k] + s * v[J][k];
    const float t1 = -s * v[I][k] + c * v[J][k];
    v[I][k] = t0; v[J][k] = t1;
  }
  return true;
}

// Right singular vector of A's smallest singular value; rows[r] = row r of A.  Ties go to the higher index.
__device__ __forceinline__ void null_vector(const float (&rows)[4][4], float (&x)[4]) {
  float a[4][4], v[4][4];
  double w[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { a[i][k] = rows[k][i]; sd += (double)a[i][k] * (double)a[i][k]; v[i][k] = i == k ? 1.0f : 0.0f; }
    w[i] = sd;
  }
  for (int it = 0; it < kSweeps; it++) {
    const bool c01 = jacobi_pair<0, 1>(a, v, w), c02 = jacobi_pair<0, 2>(a, v, w), c03 = jacobi_pair<0, 3>(a, v, w);
    const bool c12 = jacobi_pair<1, 2>(a, v, w), c13 = jacobi_pair<1, 3>(a, v, w), c23 = jacobi_pair<2, 3>(a, v, w);
    if (!(c01 | c02 | c03 | c12 | c13 | c23)) break;
  }
  double best = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) sd += (double)a[i][k] * (double)a[i][k];
    const double sv = sqrt(sd);
    // i == 0 starts; later columns replace it unless strictly larger (NaN compares false and replaces: fixed either way)
    if (i == 0 || !(sv > best)) {
      best = sv;
#pragma unroll
      for (int k = 0; k < 4; k++) x[k] = v[i][k];
    }
  }
}

// reprojection chi-square of (x, y, z) in one camera; true = the reference's `continue`
__device__ __forceinline__ bool reproj_rejects(const ViewDev& V, float x, float y, float z, float4 f, bool stereo, float sigma2) {
  const float invz = 1.0f / z;
  const float u = V.fx * x * invz + V.cx;
  const float v = V.fy * y * invz + V.cy;
  const float ex = u - f.x, ey = v - f.y;
  if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
  const float ur = u - V.bf * invz;
  const float er = ur - f.z;
  return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

__device__ __forceinline__ float dist3(float x, float y, float z, const float* O) {
  const float nx = x - O[0], ny = y - O[1], nz = z - O[2];
  return (float)sqrt(((double)nx * (double)nx + (double)ny * (double)ny) + (double)nz * (double)nz);
}

// The geometry of one match, shared by k_triangulate_matches and k_mapdb_tri_geometry (mapdb_tri_kernels.hip.h): f1 / f2 = (x, y, right_x,
// depth) of the two features, lv = (levelSigma2[octave1], levelSigma2[octave2], scaleFactors[octave1], scaleFactors[octave2]).  Writes the
// point where a source produced one (0 0 0 otherwise) and returns the status byte of c_api.h.
__device__ __forceinline__ uint8_t triangulate_match(const ViewDev& V1, const ViewDev& V2, const float4 f1, const float4 f2, const float4 lv,
                                                     const float ratioFactor, float& X, float& Y, float& Z) {
  const bool stereo1 = f1.z >= 0, stereo2 = f2.z >= 0;

  const float xn1x = (f1.x - V1.cx) * V1.invfx, xn1y = (f1.y - V1.cy) * V1.invfy;
  const float xn2x = (f2.x - V2.cx) * V2.invfx, xn2y = (f2.y - V2.cy) * V2.invfy;
  float r1[3], r2[3];
#pragma unroll
  for (int r = 0; r < 3; r++) { r1[r] = dot3(V1.Rwc + 3 * r, xn1x, xn1y, 1.0f); r2[r] = dot3(V2.Rwc + 3 * r, xn2x, xn2y, 1.0f); }
  const double n1 = sqrt(dot3d(r1, r1[0], r1[1], r1[2])), n2 = sqrt(dot3d(r2, r2[0], r2[1], r2[2]));
  const float cosRays = (float)(dot3d(r1, r2[0], r2[1], r2[2]) / (n1 * n2));
  float cosS1 = cosRays + 1.0f, cosS2 = cosS1;
  if (stereo1) cosS1 = cos_stereo(V1.b, f1.w);
  else if (stereo2) cosS2 = cos_stereo(V2.b, f2.w);
  const float cosS = cosS2 < cosS1 ? cosS2 : cosS1;   // std::min(cosS1, cosS2) literally: a NaN cosS1 stays

  X = 0; Y = 0; Z = 0;
  int src = 0, code = -1;
  if (cosRays < cosS && cosRays > 0 && (stereo1 || stereo2 || (double)cosRays < 0.9998)) {
    src = 1;
    float A[4][4], x[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      A[0][k] = xn1x * V1.Tcw[8 + k] - V1.Tcw[k];
      A[1][k] = xn1y * V1.Tcw[8 + k] - V1.Tcw[4 + k];
      A[2][k] = xn2x * V2.Tcw[8 + k] - V2.Tcw[k];
      A[3][k] = xn2y * V2.Tcw[8 + k] - V2.Tcw[4 + k];
    }
    null_vector(A, x);
    if (x[3] == 0) code = 2;
    else { X = x[0] / x[3]; Y = x[1] / x[3]; Z = x[2] / x[3]; }
  } else if (stereo1 && cosS1 < cosS2) {
    src = 2;
    if (f1.w > 0) {
      const float cx = (f1.x - V1.cx) * f1.w * V1.invfx, cy = (f1.y - V1.cy) * f1.w * V1.invfy;
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const float c = (float)(dot3d(V1.Rwc + 3 * r, cx, cy, f1.w) + (double)V1.Ow[r]);
        if (r == 0) X = c; else if (r == 1) Y = c; else Z = c;
      }
    } else code = 9;
  } else if (stereo2 && cosS2 < cosS1) {
    src = 3;
    if (f2.w > 0) {
      const float cx = (f2.x - V2.cx) * f2.w * V2.invfx, cy = (f2.y - V2.cy) * f2.w * V2.invfy;
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const float c = (float)(dot3d(V2.Rwc + 3 * r, cx, cy, f2.w) + (double)V2.Ow[r]);
        if (r == 0) X = c; else if (r == 1) Y = c; else Z = c;
      }
    } else code = 9;
  } else code = 1;

  int notFinite = 0;
  if (code < 0) {
    notFinite = !(fabsf(X) <= 3.402823466e+38f && fabsf(Y) <= 3.402823466e+38f && fabsf(Z) <= 3.402823466e+38f);
    const float z1 = row4(V1.Tcw, 2, X, Y, Z), z2 = row4(V2.Tcw, 2, X, Y, Z);
    if (z1 <= 0) code = 3;
    else if (z2 <= 0) code = 4;
    else if (reproj_rejects(V1, row4(V1.Tcw, 0, X, Y, Z), row4(V1.Tcw, 1, X, Y, Z), z1, f1, stereo1, lv.x)) code = 5;
    else if (reproj_rejects(V2, row4(V2.Tcw, 0, X, Y, Z), row4(V2.Tcw, 1, X, Y, Z), z2, f2, stereo2, lv.y)) code = 6;
    else {
      const float d1 = dist3(X, Y, Z, V1.Ow), d2 = dist3(X, Y, Z, V2.Ow);
      if (d1 == 0 || d2 == 0) code = 7;
      else {
        const float ratioDist = d2 / d1, ratioOctave = lv.z / lv.w;
        code = (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) ? 8 : 0;
      }
    }
  }
  return (uint8_t)(code | (src << 4) | (notFinite ? 0x80 : 0));
}

static __global__ __launch_bounds__(kThreads) void k_triangulate_matches(Args g) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= g.nMatches) return;
  // the problem whose range holds m: the last p with start[p] <= m (empty problems share a start and are skipped by "last")
  int lo = 0, hi = g.nProblems - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (g.start[mid] <= m) lo = mid; else hi = mid - 1;
  }
  const ProblemDev P = g.problems[lo];
  const ViewDev& V1 = g.views[P.first];
  const ViewDev& V2 = g.views[P.second];
  float X, Y, Z;
  const uint8_t st = triangulate_match(V1, V2, g.f1[m], g.f2[m], g.lv[m], P.ratioFactor, X, Y, Z);
  g.x3d[3 * (size_t)m] = X; g.x3d[3 * (size_t)m + 1] = Y; g.x3d[3 * (size_t)m + 2] = Z;
  g.status[m] = st;
}

}  // namespace tri
}  // namespace ydorb
