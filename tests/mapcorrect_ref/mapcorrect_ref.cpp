// CPU restatement of ydorb_mapdb_correct (include/ydorb/c_api.h, "Map correction") on a flat table, written the way ORB-SLAM2 writes
// the three loops: sequential, one point after the other, each point's updateNormalAndDepth() at once with whatever the centre array
// holds at that moment, and - in the interleaved mode - the keyframe's centre overwritten in place after its points, as setPose follows
// the point loop in LoopClosing::CorrectLoop.  Nothing here speaks of ranks "below r": the product's visibility rule is checked against
// the order of events it abbreviates.  It shares nothing with the product but the ABI structs, and is built by
// tests/mapcorrect_support.py with oracle/Makefile's flags (-ffp-contract=off).  The arithmetic is DESIGN.md section 2, "Map correction".
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ydorb/c_api.h"

namespace {

struct Vec3 { double x, y, z; };
struct Quat { double x, y, z, w; };
struct Sim3 { Quat r; Vec3 t; double s; };

Vec3 cross(const Vec3& a, const Vec3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
Vec3 operator+(const Vec3& a, const Vec3& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
Vec3 operator*(double s, const Vec3& a) { return {s * a.x, s * a.y, s * a.z}; }
// Eigen's Quaternion * Vector3: uv = q.vec x v; uv += uv; v + w uv + q.vec x uv
Vec3 operator*(const Quat& q, const Vec3& v) {
  const Vec3 u{q.x, q.y, q.z};
  Vec3 uv = cross(u, v);
  uv = uv + uv;
  return (v + q.w * uv) + cross(u, uv);
}
Quat conjugate(const Quat& q) { return {-q.x, -q.y, -q.z, q.w}; }
Sim3 read(const double* p) { return {{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}, p[7]}; }
Sim3 inverse(const Sim3& S) { return {conjugate(S.r), conjugate(S.r) * ((-1. / S.s) * S.t), 1. / S.s}; }   // g2o Sim3::inverse
Vec3 map(const Sim3& S, const Vec3& xyz) { return S.s * (S.r * xyz) + S.t; }                             // g2o Sim3::map

// one row of a CV_32F 3x3 times 3x1 plus 3x1: cv::gemm accumulates the products in double, adds the addend, and stores a float
float gemmRow(const float* M, const float* t, int r, const float* x) {
  double s = (double)M[3 * r] * (double)x[0];
  for (int k = 1; k < 3; k++) s += (double)M[3 * r + k] * (double)x[k];
  return (float)(s + (double)t[r]);
}

double norm3(const float d[3]) {
  double s = 0.0;
  for (int i = 0; i < 3; i++) s += (double)d[i] * (double)d[i];
  return std::sqrt(s);
}

struct Map {
  const YdObservationTable* T;
  float* pos;
  float* centre;
  const int32_t* refKf;
  const uint8_t* refLevel;
};

// MapPoint::UpdateNormalAndDepth past its two early returns, as tests/mapmaint_ref/mapmaint_ref.cpp states it
void updateNormalAndDepth(const Map& m, int p, const float* sf, int nLevels, float* normal, float* minD, float* maxD) {
  const int b = m.T->obs_start[p], e = m.T->obs_start[p + 1];
  const float* P = m.pos + 3 * p;
  float nrm[3] = {0.f, 0.f, 0.f};
  int n = 0;
  for (int q = b; q < e; q++) {
    const float* Owi = m.centre + 3 * m.T->obs_kf[q];
    float normali[3];
    for (int i = 0; i < 3; i++) normali[i] = P[i] - Owi[i];
    const float inv = (float)(1.0 / norm3(normali));
    for (int i = 0; i < 3; i++) { const float t = normali[i] * inv; nrm[i] = nrm[i] + t; }
    n++;
  }
  float PC[3];
  const float* Owr = m.centre + 3 * m.refKf[p];
  for (int i = 0; i < 3; i++) PC[i] = P[i] - Owr[i];
  const float dist = (float)norm3(PC);
  *maxD = dist * sf[m.refLevel[p]];
  *minD = *maxD / sf[nLevels - 1];
  const float invn = (float)(1.0 / (double)n);
  for (int i = 0; i < 3; i++) normal[i] = nrm[i] * invn;
}

}  // namespace

extern "C" {

// The table is (T, pos, centre, ref_kf, ref_level); pos and centre are corrected in place.  Returns 0.  Inputs are taken as valid.
int mapcorrect_ref(const YdObservationTable* T, float* pos, float* centre, const int32_t* ref_kf, const uint8_t* ref_level,
                   const YdMapCorrection* c) {
  const Map m{T, pos, centre, ref_kf, ref_level};
  const bool normals = c->normal != nullptr;
  const int n = c->n, K = c->n_kf;
  std::memset(c->pos_out, 0, 12 * (size_t)n);
  if (normals) { std::memset(c->normal, 0, 12 * (size_t)n); std::memset(c->min_distance, 0, 4 * (size_t)n); std::memset(c->max_distance, 0, 4 * (size_t)n); }

  // who corrects what: the walk over the entries in order with the mnCorrectedByKF mark
  std::vector<uint8_t> corrected((size_t)T->n_points, 0);
  std::vector<std::vector<int>> listOf((size_t)K);      // per keyframe of the call, the entries it corrects, in order
  std::vector<int> inCall((size_t)T->n_keyframes, -1);  // keyframe slot -> its place in the call (the reference holds a pointer instead)
  for (int j = 0; j < K; j++) inCall[(size_t)c->kf_slots[j]] = j;
  for (int i = 0; i < n; i++) {
    const int p = c->slots ? c->slots[i] : i;
    if (T->bad[p]) { c->status[i] = YDORB_MAPCORR_BAD; continue; }                 // if(!pMPi || pMPi->isBad()) continue;
    if (corrected[p]) { c->status[i] = YDORB_MAPCORR_CLAIMED; continue; }          // if(pMPi->mnCorrectedByKF==mpCurrentKF->mnId) continue;
    corrected[p] = 1;                                                            // pMPi->mnCorrectedByKF = mpCurrentKF->mnId;
    int k = c->corrector ? c->corrector[i] : -1;
    if (k < 0) {                                                                 // the point's reference keyframe, if the call has it
      k = inCall[(size_t)ref_kf[p]];
      if (k < 0) { c->status[i] = YDORB_MAPCORR_NOT_COVERED; continue; }
    }
    c->status[i] = YDORB_MAPCORR_DONE;
    listOf[(size_t)k].push_back(i);
  }

  auto correct = [&](int i, int k) {
    const int p = c->slots ? c->slots[i] : i;
    float* P = pos + 3 * p;
    if (c->arithmetic == YDORB_MAPCORR_SIM3) {
      const Sim3 Siw = read(static_cast<const double*>(c->before) + 8 * k);
      const Sim3 correctedSwi = inverse(read(static_cast<const double*>(c->after) + 8 * k));
      const Vec3 eigP3Dw{(double)P[0], (double)P[1], (double)P[2]};
      const Vec3 eigCorrectedP3Dw = map(correctedSwi, map(Siw, eigP3Dw));        // correctedSwi.map(Siw.map(eigP3Dw))
      P[0] = (float)eigCorrectedP3Dw.x; P[1] = (float)eigCorrectedP3Dw.y; P[2] = (float)eigCorrectedP3Dw.z;   // SetWorldPos
    } else {
      const float* Tcw = static_cast<const float*>(c->before) + 12 * k;
      const float* Twc = static_cast<const float*>(c->after) + 12 * k;
      float Xc[3], Xw[3];
      for (int r = 0; r < 3; r++) Xc[r] = gemmRow(Tcw, Tcw + 9, r, P);           // Xc = Rcw*pMP->GetWorldPos()+tcw;
      for (int r = 0; r < 3; r++) Xw[r] = gemmRow(Twc, Twc + 9, r, Xc);          // pMP->SetWorldPos(Rwc*Xc+twc);
      std::memcpy(P, Xw, 12);
    }
    std::memcpy(c->pos_out + 3 * i, P, 12);
    if (T->obs_start[p] == T->obs_start[p + 1]) { c->status[i] = YDORB_MAPCORR_DONE_NO_OBSERVATIONS; return; }   // if(observations.empty()) return;
    if (normals)                                                                 // pMPi->UpdateNormalAndDepth();
      updateNormalAndDepth(m, p, c->scale_factors, c->n_levels, c->normal + 3 * i, c->min_distance + i, c->max_distance + i);
  };
  auto setPose = [&](int k) { if (c->centre_after) std::memcpy(centre + 3 * c->kf_slots[k], c->centre_after + 3 * k, 12); };

  if (c->centres == YDORB_MAPCORR_INTERLEAVED) {
    for (int k = 0; k < K; k++) {                                                // for(mit=CorrectedSim3.begin(); ...)
      for (const int i : listOf[(size_t)k]) correct(i, k);
      setPose(k);                                                                // pKFi->SetPose(correctedTiw);
    }
    return 0;
  }
  if (c->centres == YDORB_MAPCORR_POSES_FIRST)
    for (int k = 0; k < K; k++) setPose(k);                                      // every pose is set before the first point moves
  std::vector<int> of((size_t)n, -1);
  for (int k = 0; k < K; k++) for (const int i : listOf[(size_t)k]) of[(size_t)i] = k;
  for (int i = 0; i < n; i++) if (of[(size_t)i] >= 0) correct(i, of[(size_t)i]); // for(size_t i=0; i<vpMPs.size(); i++)
  if (c->centres == YDORB_MAPCORR_RESIDENT)
    for (int k = 0; k < K; k++) setPose(k);
  return 0;
}

}  // extern "C"
