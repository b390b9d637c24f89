// CPU restatement of LocalMapping::createNewMapPoints' loop body (ORB-SLAM2 LocalMapping::CreateNewMapPoints, which YDORBSLAM
// renames): test infrastructure, the checker of ydorb_triangulate_matches.  Written the reference's way - one match after the other,
// small matrices in loops - under the arithmetic contract of DESIGN.md section 2 ("createNewMapPoints"): float inputs, products of a
// small float gemm / Mat::dot / cv::norm exact in double and summed in ascending index, the SVD as OpenCV's JacobiSVDImpl_<float>
// with sqrt(p^2 + beta^2) for hypot.  Built with oracle/Makefile's flags (-ffp-contract=off) by tests/triangulate_support.py.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/ydorb/c_api.h"

namespace {

struct Vec3 { float v[3]; };

// cv::Mat(3x3, float) * (3x1): GEMMSingleMul<float, double>
Vec3 mul3(const float* R, const Vec3& x) {
  Vec3 o;
  for (int r = 0; r < 3; r++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s = k == 0 ? (double)R[3 * r] * (double)x.v[0] : s + (double)R[3 * r + k] * (double)x.v[k];
    o.v[r] = (float)s;
  }
  return o;
}
// Mat::dot and the sum of cv::norm: double accumulation in ascending index
double dotd(const float* a, const float* b, int n) {
  double s = (double)a[0] * (double)b[0];
  for (int k = 1; k < n; k++) s = s + (double)a[k] * (double)b[k];
  return s;
}
double norm3(const Vec3& a) { return std::sqrt(dotd(a.v, a.v, 3)); }

// cos(2 * atan2(b / 2, depth)) in the libm-free form of the contract
float cosStereo(float b, float depth) {
  const float h = b / 2.0f;
  const double d2 = (double)depth * (double)depth, h2 = (double)h * (double)h;
  return (float)((d2 - h2) / (d2 + h2));
}

// cv::SVD::compute(A, w, u, vt): JacobiSVDImpl_<float> on At (row i of At = column i of A), Vt accumulated; returns vt.row(3) after
// the descending sort, i.e. the row of the smallest singular value, the last one on ties.
int jacobiNullVector(const float* A, float* x) {
  const int n = 4, m = 4;
  float At[4][4], Vt[4][4];
  double W[4];
  const float eps = 1.1920928955078125e-07f * 2;   // FLT_EPSILON * 2
  for (int i = 0; i < n; i++) {
    double sd = 0;
    for (int k = 0; k < m; k++) {
      At[i][k] = A[k * 4 + i];
      const float t = At[i][k];
      sd += (double)t * t;
    }
    W[i] = sd;
    for (int k = 0; k < n; k++) Vt[i][k] = 0;
    Vt[i][i] = 1;
  }
  int iter;
  const int maxIter = 30;   // std::max(m, 30)
  for (iter = 0; iter < maxIter; iter++) {
    bool changed = false;
    for (int i = 0; i < n - 1; i++)
      for (int j = i + 1; j < n; j++) {
        float *Ai = At[i], *Aj = At[j];
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
        if (std::abs(p) <= eps * std::sqrt((double)a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = std::sqrt(p * p + beta * beta);   // hypot((double)p, beta)
        float c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = (float)std::sqrt(delta / gamma);
          c = (float)(p / (gamma * s * 2));
        } else {
          c = (float)std::sqrt((gamma + beta) / (gamma * 2));
          s = (float)(p / (gamma * c * 2));
        }
        a = b = 0;
        for (int k = 0; k < m; k++) {
          const float t0 = c * Ai[k] + s * Aj[k];
          const float t1 = -s * Ai[k] + c * Aj[k];
          Ai[k] = t0; Aj[k] = t1;
          a += (double)t0 * t0; b += (double)t1 * t1;
        }
        W[i] = a; W[j] = b;
        changed = true;
        float *Vi = Vt[i], *Vj = Vt[j];
        for (int k = 0; k < n; k++) {
          const float t0 = c * Vi[k] + s * Vj[k];
          const float t1 = -s * Vi[k] + c * Vj[k];
          Vi[k] = t0; Vj[k] = t1;
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < n; i++) {
    double sd = 0;
    for (int k = 0; k < m; k++) {
      const float t = At[i][k];
      sd += (double)t * t;
    }
    W[i] = std::sqrt(sd);
  }
  int last = 0;   // where the descending sort puts the last row: the smallest value, the highest index among equals
  for (int i = 1; i < n; i++)
    if (!(W[i] > W[last])) last = i;
  for (int k = 0; k < n; k++) x[k] = Vt[last][k];
  return iter;
}

struct Feature { float x, y, ur, depth; int octave; };

Feature feature(const YdTriView& V, int i) { return Feature{V.kps[i].x, V.kps[i].y, V.right_x[i], V.depth[i], V.kps[i].octave}; }

// KeyFrame::unprojectStereo: false = the empty Mat
bool unprojectStereo(const YdTriView& V, const Feature& f, Vec3& out) {
  const float z = f.depth;
  if (z > 0) {
    const float x = (f.x - V.cx) * z * V.invfx;
    const float y = (f.y - V.cy) * z * V.invfy;
    const float c[3] = {x, y, z};
    for (int r = 0; r < 3; r++) out.v[r] = (float)(dotd(V.Rwc + 3 * r, c, 3) + (double)V.Ow[r]);   // Twc.R * x3Dc + Twc.t as one gemm
    return true;
  }
  return false;
}

// true = `continue`
bool reprojectionFails(const YdTriView& V, const Feature& f, bool stereo, float x, float y, float z) {
  const float sigmaSquare = V.level_sigma2[f.octave];
  const float invz = 1.0 / z;
  if (!stereo) {
    const float u = V.fx * x * invz + V.cx;
    const float v = V.fy * y * invz + V.cy;
    const float errX = u - f.x;
    const float errY = v - f.y;
    if ((errX * errX + errY * errY) > 5.991 * sigmaSquare) return true;
  } else {
    const float u = V.fx * x * invz + V.cx;
    const float u_r = u - V.bf * invz;
    const float v = V.fy * y * invz + V.cy;
    const float errX = u - f.x;
    const float errY = v - f.y;
    const float errX_r = u_r - f.ur;
    if ((errX * errX + errY * errY + errX_r * errX_r) > 7.8 * sigmaSquare) return true;
  }
  return false;
}

uint8_t oneMatch(const YdTriView& V1, const YdTriView& V2, int idx1, int idx2, float ratioFactor, float* out) {
  out[0] = out[1] = out[2] = 0;
  const Feature kp1 = feature(V1, idx1), kp2 = feature(V2, idx2);
  const bool bStereo1 = kp1.ur >= 0, bStereo2 = kp2.ur >= 0;
  const Vec3 xn1 = {{(kp1.x - V1.cx) * V1.invfx, (kp1.y - V1.cy) * V1.invfy, 1.0f}};
  const Vec3 xn2 = {{(kp2.x - V2.cx) * V2.invfx, (kp2.y - V2.cy) * V2.invfy, 1.0f}};
  const Vec3 ray1 = mul3(V1.Rwc, xn1), ray2 = mul3(V2.Rwc, xn2);
  const float cosParallaxRays = dotd(ray1.v, ray2.v, 3) / (norm3(ray1) * norm3(ray2));
  float cosParallaxStereo = cosParallaxRays + 1;
  float cosParallaxStereo1 = cosParallaxStereo;
  float cosParallaxStereo2 = cosParallaxStereo;
  if (bStereo1) cosParallaxStereo1 = cosStereo(V1.b, kp1.depth);
  else if (bStereo2) cosParallaxStereo2 = cosStereo(V2.b, kp2.depth);
  cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min(1, 2)

  Vec3 x3D = {{0, 0, 0}};
  int src;
  if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < 0.9998)) {
    src = YDORB_TRI_SRC_LINEAR;
    float A[16];
    for (int k = 0; k < 4; k++) {
      A[k] = xn1.v[0] * V1.Tcw[8 + k] - V1.Tcw[k];
      A[4 + k] = xn1.v[1] * V1.Tcw[8 + k] - V1.Tcw[4 + k];
      A[8 + k] = xn2.v[0] * V2.Tcw[8 + k] - V2.Tcw[k];
      A[12 + k] = xn2.v[1] * V2.Tcw[8 + k] - V2.Tcw[4 + k];
    }
    float h[4];
    jacobiNullVector(A, h);
    if (h[3] == 0) return YDORB_TRI_W_ZERO | (src << 4);
    for (int k = 0; k < 3; k++) x3D.v[k] = h[k] / h[3];
  } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
    src = YDORB_TRI_SRC_UNPROJECT_FIRST;
    if (!unprojectStereo(V1, kp1, x3D)) return YDORB_TRI_BAD_STEREO_DEPTH | (src << 4);
  } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
    src = YDORB_TRI_SRC_UNPROJECT_SECOND;
    if (!unprojectStereo(V2, kp2, x3D)) return YDORB_TRI_BAD_STEREO_DEPTH | (src << 4);
  } else
    return YDORB_TRI_NO_METHOD;
  std::memcpy(out, x3D.v, sizeof x3D.v);
  uint8_t bits = (uint8_t)(src << 4);
  if (!(std::isfinite(x3D.v[0]) && std::isfinite(x3D.v[1]) && std::isfinite(x3D.v[2]))) bits |= YDORB_TRI_NOT_FINITE;

  // Rcw.row(r).dot(x3Dt) + tcw(r): a double dot plus a float, rounded when assigned
  const float z1 = dotd(V1.Tcw + 8, x3D.v, 3) + V1.Tcw[11];
  if (z1 <= 0) return bits | YDORB_TRI_DEPTH_FIRST;
  const float z2 = dotd(V2.Tcw + 8, x3D.v, 3) + V2.Tcw[11];
  if (z2 <= 0) return bits | YDORB_TRI_DEPTH_SECOND;
  const float x1 = dotd(V1.Tcw, x3D.v, 3) + V1.Tcw[3];
  const float y1 = dotd(V1.Tcw + 4, x3D.v, 3) + V1.Tcw[7];
  if (reprojectionFails(V1, kp1, bStereo1, x1, y1, z1)) return bits | YDORB_TRI_REPROJ_FIRST;
  const float x2 = dotd(V2.Tcw, x3D.v, 3) + V2.Tcw[3];
  const float y2 = dotd(V2.Tcw + 4, x3D.v, 3) + V2.Tcw[7];
  if (reprojectionFails(V2, kp2, bStereo2, x2, y2, z2)) return bits | YDORB_TRI_REPROJ_SECOND;

  Vec3 normal1, normal2;
  for (int k = 0; k < 3; k++) { normal1.v[k] = x3D.v[k] - V1.Ow[k]; normal2.v[k] = x3D.v[k] - V2.Ow[k]; }
  const float dist1 = norm3(normal1);
  const float dist2 = norm3(normal2);
  if (dist1 == 0 || dist2 == 0) return bits | YDORB_TRI_ZERO_DISTANCE;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = V1.scale_factors[kp1.octave] / V2.scale_factors[kp2.octave];
  if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return bits | YDORB_TRI_SCALE_RATIO;
  return bits | YDORB_TRI_ACCEPTED;
}

}  // namespace

extern "C" {

// same arguments as ydorb_triangulate_matches; indices are trusted (the tests hand over valid batches)
int triref_triangulate(const YdTriBatch* B, float* x3d, uint8_t* status, int32_t* n_accepted) {
  for (int p = 0; p < B->n_problems; p++) {
    const YdTriView &V1 = B->views[B->first_view[p]], &V2 = B->views[B->second_view[p]];
    int acc = 0;
    for (int m = B->match_start[p]; m < B->match_start[p + 1]; m++) {
      status[m] = oneMatch(V1, V2, B->idx1[m], B->idx2[m], B->ratio_factor[p], x3d + 3 * (size_t)m);
      acc += (status[m] & 15) == YDORB_TRI_ACCEPTED;
    }
    if (n_accepted) n_accepted[p] = acc;
  }
  return 0;
}

// the null vector of a row-major 4x4 float matrix; returns the sweeps used
int triref_null_vector(const float* A, float* x) { return jacobiNullVector(A, x); }

float triref_cos_stereo(float b, float depth) { return cosStereo(b, depth); }

}
