// TEST-ONLY: executes the three map-correction methods of ydorb::adapter::MapMirror (include/ydorb/mapMirror.hpp) beside the
// reference's loops on the same stand-ins of KeyFrame / MapPoint in one program, linked against libydorb.so:
//   mapcorrect_run in.bin
// in.bin is mapmaint_run.cpp's scene format (the keyframes' centres in it are replaced by poses made here).  The loops are written
// plainly, as ORB-SLAM2 writes them:
//   A  LoopClosing::CorrectLoop's point correction over CorrectedSim3 in the map's own (address) order, with the per-point
//      UpdateNormalAndDepth() and the keyframe's SetPose after its points;
//   B  the tail of Optimizer::OptimizeEssentialGraph: every pose set, then every point through mnCorrectedReference or its reference
//      keyframe, with UpdateNormalAndDepth();
//   C  the map update of RunGlobalBundleAdjustment: mPosGBA for the points the BA held, the pose pair of the reference keyframe for
//      the others, the points of keyframes that were not reached skipped.
// UpdateNormalAndDepth() of one point goes through the flattening adapter (mapPoint.hpp), one point per call: its arithmetic is the
// map-maintenance contract.  cv::Mat products the loops need are written out with cv::gemm's arithmetic (products exact in double,
// summed in ascending index, rounded once): the stand-in cv::Mat accumulates in float.
// For each loop: the adapter method runs on the mirror, the objects' state is recorded and put back, the reference loop runs, and the
// two states are compared exactly (positions, normals, distances, marks, poses, centres).  The objects then hold what the table
// holds, so the next loop starts in step with no touch.  One line per figure, "<name> <value>"; tests/test_mapcorrect_adapter_gpu.py
// reads them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include <opencv2/core.hpp>

#include "ydorb/mapMirror.hpp"
#include "ydorb/mapPoint.hpp"

struct KeyFrame;
struct MapPoint {
  int id = 0;
  bool bad = false;
  cv::Mat pos, normal, posGBA;
  float minDistance = 0.f, maxDistance = 0.f;
  long unsigned int m_int_correctedByKeyFrameID = 0, m_int_correctedReference = 0, BAGlobalForKF = 0;
  std::shared_ptr<KeyFrame> ref;
  std::map<std::shared_ptr<KeyFrame>, size_t> observations;
  bool isBad() { return bad; }
  std::map<std::shared_ptr<KeyFrame>, size_t> getObservations() { return observations; }
  cv::Mat getPosInWorld() { return pos.clone(); }
  void setPosInWorld(const cv::Mat& P) { P.copyTo(pos); }
  void setNormalAndDepth(const cv::Mat& n, float mn, float mx) { n.copyTo(normal); minDistance = mn; maxDistance = mx; }
  std::shared_ptr<KeyFrame> getReferenceKeyFrame() { return ref; }
};

// Rwc * x + t of 3x3 | 3x1 blocks, cv::gemm's arithmetic
static cv::Mat gemm3(const cv::Mat& R, const cv::Mat& x, const cv::Mat& t) {
  cv::Mat o(3, 1, CV_32F);
  for (int r = 0; r < 3; r++) {
    double s = (double)R.at<float>(r, 0) * (double)x.at<float>(0);
    for (int k = 1; k < 3; k++) s += (double)R.at<float>(r, k) * (double)x.at<float>(k);
    o.at<float>(r) = (float)(s + (double)t.at<float>(r));
  }
  return o;
}

struct KeyFrame {
  long unsigned int m_int_keyFrameID = 0, BAGlobalForKF = 0;
  cv::Mat Tcw, Twc, centre, TcwBefGBA;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  std::vector<std::shared_ptr<MapPoint>> mapPoints;
  std::vector<std::shared_ptr<KeyFrame>> covisible;
  cv::Mat getCameraOriginInWorld() { return centre.clone(); }
  cv::Mat getPose() { return Tcw.clone(); }
  cv::Mat getPoseInverse() { return Twc.clone(); }
  std::vector<std::shared_ptr<MapPoint>> getMapPointMatches() { return mapPoints; }
  std::vector<std::shared_ptr<KeyFrame>> getVectorCovisibleKeyFrames() { return covisible; }
  void setBadFlag() {}
  bool isBad() { return false; }
  void setPose(const cv::Mat& T) {   // KeyFrame::SetPose: Rwc = Rcw.t(); Ow = -Rwc*tcw; Twc = [Rwc | Ow]
    Tcw = T.clone();
    const cv::Mat Rwc = Tcw.rowRange(0, 3).colRange(0, 3).t(), tcw = Tcw.rowRange(0, 3).colRange(3, 4);
    const cv::Mat zero(3, 1, CV_32F);
    centre = -gemm3(Rwc, tcw, zero);
    Twc = cv::Mat::eye(4, 4, CV_32F);
    Rwc.copyTo(Twc.rowRange(0, 3).colRange(0, 3));
    centre.copyTo(Twc.rowRange(0, 3).colRange(3, 4));
  }
};
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
typedef ydorb::adapter::MapMirror<KF, MP> Mirror;
namespace ya = ydorb::adapter;

// g2o::Sim3 as far as the loops use it
struct Quat { double qx, qy, qz, qw; double x() const { return qx; } double y() const { return qy; } double z() const { return qz; } double w() const { return qw; } };
struct Vec3 { double v[3]; double operator[](int i) const { return v[i]; } };
struct Sim3 {
  Quat r{0, 0, 0, 1}; Vec3 t{{0, 0, 0}}; double s = 1;
  Quat rotation() const { return r; }
  Vec3 translation() const { return t; }
  double scale() const { return s; }
  static Vec3 rot(const Quat& q, const Vec3& p) {   // Eigen: uv = q.vec x p; uv += uv; p + w uv + q.vec x uv
    Vec3 uv{{q.qy * p.v[2] - q.qz * p.v[1], q.qz * p.v[0] - q.qx * p.v[2], q.qx * p.v[1] - q.qy * p.v[0]}};
    for (int k = 0; k < 3; k++) uv.v[k] = uv.v[k] + uv.v[k];
    const Vec3 c{{q.qy * uv.v[2] - q.qz * uv.v[1], q.qz * uv.v[0] - q.qx * uv.v[2], q.qx * uv.v[1] - q.qy * uv.v[0]}};
    return Vec3{{(p.v[0] + q.qw * uv.v[0]) + c.v[0], (p.v[1] + q.qw * uv.v[1]) + c.v[1], (p.v[2] + q.qw * uv.v[2]) + c.v[2]}};
  }
  Sim3 inverse() const {
    Sim3 o;
    o.r = Quat{-r.qx, -r.qy, -r.qz, r.qw};
    const double f = -1. / s;
    o.t = rot(o.r, Vec3{{f * t.v[0], f * t.v[1], f * t.v[2]}});
    o.s = 1. / s;
    return o;
  }
  Vec3 map(const Vec3& xyz) const { const Vec3 p = rot(r, xyz); return Vec3{{s * p.v[0] + t.v[0], s * p.v[1] + t.v[1], s * p.v[2] + t.v[2]}}; }
  cv::Mat toCvSE3() const {   // Converter::toCvSE3(rotation().toRotationMatrix(), translation() * (1. / s))
    const double tx = 2 * r.qx, ty = 2 * r.qy, tz = 2 * r.qz, twx = tx * r.qw, twy = ty * r.qw, twz = tz * r.qw, txx = tx * r.qx, txy = ty * r.qx,
                 txz = tz * r.qx, tyy = ty * r.qy, tyz = tz * r.qy, tzz = tz * r.qz;
    const double R[3][3] = {{1 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1 - (txx + tzz), tyz - twx}, {txz - twy, tyz + twx, 1 - (txx + tyy)}};
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    const double inv = 1. / s;
    for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) T.at<float>(a, b) = (float)R[a][b]; T.at<float>(a, 3) = (float)(t.v[a] * inv); }
    return T;
  }
};
typedef std::map<KF, Sim3> KeyFrameAndPose;

static FILE* g_in;
static int32_t geti() { int32_t v = 0; if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static float getf() { float v = 0; if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static cv::Mat vec3() { cv::Mat m(3, 1, CV_32F); for (int r = 0; r < 3; r++) m.at<float>(r) = getf(); return m; }

static uint32_t g_rng = 12345u;
static double uni(double lo, double hi) { g_rng = g_rng * 1664525u + 1013904223u; return lo + (hi - lo) * ((g_rng >> 8) * (1.0 / 16777216.0)); }
static Quat unit(double x, double y, double z, double w) { const double n = std::sqrt(x * x + y * y + z * z + w * w); return Quat{x / n, y / n, z / n, w / n}; }
static Sim3 randomPose() { Sim3 S; S.r = unit(uni(-1, 1), uni(-1, 1), uni(-1, 1), uni(-1, 1)); S.t = Vec3{{uni(-4, 4), uni(-4, 4), uni(-4, 4)}}; return S; }
static Sim3 nudged(const Sim3& S, double scaleSpan) {
  Sim3 o;
  o.r = unit(S.r.qx + uni(-0.05, 0.05), S.r.qy + uni(-0.05, 0.05), S.r.qz + uni(-0.05, 0.05), S.r.qw + uni(-0.05, 0.05));
  o.t = Vec3{{S.t.v[0] + uni(-0.4, 0.4), S.t.v[1] + uni(-0.4, 0.4), S.t.v[2] + uni(-0.4, 0.4)}};
  o.s = 1.0 + uni(-scaleSpan, scaleSpan);
  return o;
}

struct Scene { std::vector<KF> kfs; std::vector<MP> mps; int current = 0; };

static std::vector<int32_t> snapshot(const Scene& S) {
  std::vector<int32_t> o;
  auto putf = [&o](float v) { int32_t b; memcpy(&b, &v, 4); o.push_back(b); };
  for (const MP& m : S.mps) {
    for (int r = 0; r < 3; r++) putf(m->pos.at<float>(r));
    for (int r = 0; r < 3; r++) putf(m->normal.at<float>(r));
    putf(m->minDistance); putf(m->maxDistance);
    o.push_back((int32_t)m->m_int_correctedByKeyFrameID); o.push_back((int32_t)m->m_int_correctedReference);
  }
  for (const KF& k : S.kfs) {
    for (int r = 0; r < 3; r++) putf(k->centre.at<float>(r));
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) putf(k->Tcw.at<float>(r, c));
  }
  return o;
}
static void restore(Scene& S, const std::vector<int32_t>& o) {
  size_t at = 0;
  auto getF = [&o, &at]() { float v; memcpy(&v, &o[at++], 4); return v; };
  for (const MP& m : S.mps) {
    for (int r = 0; r < 3; r++) m->pos.at<float>(r) = getF();
    for (int r = 0; r < 3; r++) m->normal.at<float>(r) = getF();
    m->minDistance = getF(); m->maxDistance = getF();
    m->m_int_correctedByKeyFrameID = (long unsigned int)o[at++]; m->m_int_correctedReference = (long unsigned int)o[at++];
  }
  for (const KF& k : S.kfs) {
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    at += 3;
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) T.at<float>(r, c) = getF();
    k->setPose(T);
  }
}
static int moved(const std::vector<int32_t>& a, const std::vector<int32_t>& b, size_t nPts) {
  int n = 0;
  for (size_t p = 0; p < nPts; p++) n += memcmp(&a[10 * p], &b[10 * p], 12) != 0;
  return n;
}

static void updateNormalAndDepth(const MP& mp) {   // MapPoint::UpdateNormalAndDepth of one point, through the flattening adapter
  ya::updateNormalAndDepthBatch<KF, MP>(std::vector<MP>{mp}, [](const MP& p, const cv::Mat& n, float mn, float mx) { p->setNormalAndDepth(n, mn, mx); });
}
static const auto applyNormals = [](const MP& p, const cv::Mat&, const cv::Mat& normal, float mn, float mx) {
  if (!normal.empty()) p->setNormalAndDepth(normal, mn, mx);
};

static void report(const char* tag, Scene& S, Mirror& mirror, const std::vector<int32_t>& base, const std::vector<int32_t>& got, const std::vector<int32_t>& want,
                   int corrected, int verifyDifferences) {
  printf("%s_same %d\n%s_corrected %d\n%s_points_moved %d\n%s_verify_differences %d\n", tag, (int)(got == want), tag, corrected, tag,
         moved(base, want, S.mps.size()), tag, verifyDifferences);
  const Mirror::Difference d = mirror.verify();   // the objects hold the reference loop's state now: still what the table holds
  printf("%s_verify_after_reference %d\n", tag, (int)(d.pointSlots.size() + d.keyFrameSlots.size()));
}

int main(int argc, char** argv) {
  if (argc < 2 || !(g_in = fopen(argv[1], "rb"))) { fprintf(stderr, "usage: mapcorrect_run in.bin\n"); return 2; }
  Scene S;
  const int nKf = geti(), nPts = geti(), nLevels = geti();
  std::vector<float> sf(nLevels);
  for (float& s : sf) s = getf();
  (void)getf();
  S.current = geti();
  std::vector<int> covisible(geti());
  for (int& c : covisible) c = geti();
  for (int q = geti(); q > 0; q--) (void)geti();
  S.kfs.resize(nKf); S.mps.resize(nPts);
  for (int k = nKf - 1; k >= 0; k--) if (k % 2 == 1) S.kfs[k] = std::make_shared<KeyFrame>();   // addresses out of id order
  for (int k = 0; k < nKf; k++) if (k % 2 == 0) S.kfs[k] = std::make_shared<KeyFrame>();
  for (int p = 0; p < nPts; p++) { S.mps[p] = std::make_shared<MapPoint>(); S.mps[p]->id = p; S.mps[p]->normal = cv::Mat(3, 1, CV_32F); }
  std::vector<Sim3> pose(nKf);
  for (int k = 0; k < nKf; k++) {
    KeyFrame& K = *S.kfs[k];
    K.m_int_keyFrameID = (long unsigned int)k;
    (void)vec3(); (void)geti();
    pose[k] = randomPose();
    K.setPose(pose[k].toCvSE3());
    const int n = geti();
    K.m_v_keyPoints.resize(n); K.m_v_rightXcords.resize(n); K.m_v_depth.resize(n); K.mapPoints.resize(n);
    K.m_v_scaleFactors = sf;
    for (int i = 0; i < n; i++) { K.m_v_keyPoints[i] = cv::KeyPoint(); K.m_v_keyPoints[i].octave = geti(); }
    for (int i = 0; i < n; i++) K.m_v_rightXcords[i] = getf();
    for (int i = 0; i < n; i++) K.m_v_depth[i] = getf();
    for (int i = 0; i < n; i++) { const int p = geti(); if (p >= 0) K.mapPoints[i] = S.mps[p]; }
  }
  for (int p = 0; p < nPts; p++) {
    MapPoint& M = *S.mps[p];
    M.pos = vec3();
    M.bad = geti() != 0;
    M.ref = S.kfs[geti()];
    const int n = geti();
    for (int i = 0; i < n; i++) { const int k = geti(), idx = geti(); M.observations[S.kfs[k]] = (size_t)idx; }
  }
  // a map-point vector and the observation maps disagree after a fuse or a replace: every fifth entry leaves its keyframe's vector
  // while the point keeps the observation.  With complete vectors the first observer in the order always claims a point, and no
  // corrected point has an observer whose pose was already set.
  { int at = 0; for (const KF& k : S.kfs) for (MP& m : k->mapPoints) if (m && at++ % 5 == 0) m = MP(); }
  const KF cur = S.kfs[S.current];

  Mirror mirror(0, 64, 4, 256);
  for (const KF& k : S.kfs) mirror.touch(k);
  for (const MP& m : S.mps) mirror.touch(m);
  for (const MP& m : S.mps) updateNormalAndDepth(m);   // the map's normals before anything is corrected
  { const Mirror::Difference d = mirror.verify(); printf("loaded_verify_differences %d\n", (int)(d.pointSlots.size() + d.keyFrameSlots.size())); }

  // ---------------------------------------------------------------------------------------------------------------- loop A
  KeyFrameAndPose CorrectedSim3, NonCorrectedSim3;
  for (int c : covisible) { NonCorrectedSim3[S.kfs[c]] = pose[c]; CorrectedSim3[S.kfs[c]] = nudged(pose[c], 0.08); }
  NonCorrectedSim3[cur] = pose[S.current]; CorrectedSim3[cur] = nudged(pose[S.current], 0.08);
  {
    const std::vector<int32_t> base = snapshot(S);
    const int corrected = mirror.correctLoopPoints(CorrectedSim3, NonCorrectedSim3, cur, applyNormals);
    for (const auto& kv : CorrectedSim3) kv.first->setPose(kv.second.toCvSE3());
    const Mirror::Difference d = mirror.verify();
    const std::vector<int32_t> got = snapshot(S);
    restore(S, base);
    for (const auto& mit : CorrectedSim3) {
      const KF pKFi = mit.first;
      const Sim3 g2oCorrectedSiw = mit.second, g2oCorrectedSwi = g2oCorrectedSiw.inverse(), g2oSiw = NonCorrectedSim3[pKFi];
      for (const MP& pMPi : pKFi->getMapPointMatches()) {
        if (!pMPi) continue;
        if (pMPi->isBad()) continue;
        if (pMPi->m_int_correctedByKeyFrameID == cur->m_int_keyFrameID) continue;
        const cv::Mat P3Dw = pMPi->getPosInWorld();
        const Vec3 eigP3Dw{{(double)P3Dw.at<float>(0), (double)P3Dw.at<float>(1), (double)P3Dw.at<float>(2)}};
        const Vec3 eigCorrectedP3Dw = g2oCorrectedSwi.map(g2oSiw.map(eigP3Dw));
        cv::Mat cvCorrectedP3Dw(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) cvCorrectedP3Dw.at<float>(r) = (float)eigCorrectedP3Dw.v[r];
        pMPi->setPosInWorld(cvCorrectedP3Dw);
        pMPi->m_int_correctedByKeyFrameID = cur->m_int_keyFrameID;
        pMPi->m_int_correctedReference = pKFi->m_int_keyFrameID;
        updateNormalAndDepth(pMPi);
      }
      pKFi->setPose(g2oCorrectedSiw.toCvSE3());
    }
    report("A", S, mirror, base, got, snapshot(S), corrected, (int)(d.pointSlots.size() + d.keyFrameSlots.size()));
  }

  // ---------------------------------------------------------------------------------------------------------------- loop B
  {
    std::vector<Sim3> vScw(nKf), vCorrectedScw(nKf);
    for (int k = 0; k < nKf; k++) {
      const auto it = NonCorrectedSim3.find(S.kfs[k]);
      vScw[k] = it != NonCorrectedSim3.end() ? it->second : pose[k];
      vCorrectedScw[k] = nudged(vScw[k], 0.05);
    }
    const std::vector<int32_t> base = snapshot(S);
    for (int k = 0; k < nKf; k++) { S.kfs[k]->setPose(vCorrectedScw[k].toCvSE3()); mirror.touch(S.kfs[k]); }   // the poses first, by the caller
    const std::vector<int32_t> posed = snapshot(S);
    const int corrected = mirror.correctAfterEssentialGraph(S.kfs, S.mps, cur, [&](const KF& k) { return vScw[k->m_int_keyFrameID]; },
                                                            [&](const KF& k) { return vCorrectedScw[k->m_int_keyFrameID]; }, applyNormals);
    const Mirror::Difference d = mirror.verify();
    const std::vector<int32_t> got = snapshot(S);
    restore(S, posed);
    for (const MP& pMP : S.mps) {
      if (pMP->isBad()) continue;
      const long unsigned int nIDr = pMP->m_int_correctedByKeyFrameID == cur->m_int_keyFrameID ? pMP->m_int_correctedReference
                                                                                               : pMP->getReferenceKeyFrame()->m_int_keyFrameID;
      const Sim3 Srw = vScw[nIDr], correctedSwr = vCorrectedScw[nIDr].inverse();
      const cv::Mat P3Dw = pMP->getPosInWorld();
      const Vec3 eigCorrectedP3Dw = correctedSwr.map(Srw.map(Vec3{{(double)P3Dw.at<float>(0), (double)P3Dw.at<float>(1), (double)P3Dw.at<float>(2)}}));
      cv::Mat cvCorrectedP3Dw(3, 1, CV_32F);
      for (int r = 0; r < 3; r++) cvCorrectedP3Dw.at<float>(r) = (float)eigCorrectedP3Dw.v[r];
      pMP->setPosInWorld(cvCorrectedP3Dw);
      updateNormalAndDepth(pMP);
    }
    report("B", S, mirror, base, got, snapshot(S), corrected, (int)(d.pointSlots.size() + d.keyFrameSlots.size()));
    for (int k = 0; k < nKf; k++) pose[k] = vCorrectedScw[k];
  }

  // ---------------------------------------------------------------------------------------------------------------- loop C
  {
    const long unsigned int nLoopKF = cur->m_int_keyFrameID + 1000;
    std::vector<Sim3> after(nKf);
    for (int k = 0; k < nKf; k++) { after[k] = nudged(pose[k], 0.0); after[k].s = 1; }
    std::vector<KF> reached;
    for (int k = 0; k < nKf; k++) if (k % 5 != 3) reached.push_back(S.kfs[k]);       // the spanning tree did not reach every fifth
    for (const MP& m : S.mps) if (m->id % 7 == 2) {                                  // the points the BA held
      m->BAGlobalForKF = nLoopKF;
      m->posGBA = cv::Mat(3, 1, CV_32F);
      for (int r = 0; r < 3; r++) m->posGBA.at<float>(r) = m->pos.at<float>(r) + (float)uni(-0.2, 0.2);
    }
    const std::vector<int32_t> base = snapshot(S);
    auto setPoses = [&](bool touch) {
      for (const KF& k : reached) {
        k->TcwBefGBA = k->getPose();
        k->setPose(after[k->m_int_keyFrameID].toCvSE3());
        k->BAGlobalForKF = nLoopKF;
        if (touch) mirror.touch(k);
      }
    };
    setPoses(true);
    std::vector<MP> others;
    for (const MP& m : S.mps) {
      if (m->isBad()) continue;
      if (m->BAGlobalForKF == nLoopKF) { m->setPosInWorld(m->posGBA); mirror.touchPosition(m); }
      else others.push_back(m);
    }
    const int corrected = mirror.correctAfterGlobalBA(reached, others, [](const KF& k) { return k->TcwBefGBA; }, [](const KF& k) { return k->getPoseInverse(); },
                                                      applyNormals);
    const Mirror::Difference d = mirror.verify();
    const std::vector<int32_t> got = snapshot(S);
    restore(S, base);
    setPoses(false);
    for (const MP& pMP : S.mps) {
      if (pMP->isBad()) continue;
      if (pMP->BAGlobalForKF == nLoopKF) {
        pMP->setPosInWorld(pMP->posGBA);
      } else {
        const KF pRefKF = pMP->getReferenceKeyFrame();
        if (pRefKF->BAGlobalForKF != nLoopKF) continue;
        const cv::Mat Rcw = pRefKF->TcwBefGBA.rowRange(0, 3).colRange(0, 3), tcw = pRefKF->TcwBefGBA.rowRange(0, 3).colRange(3, 4);
        const cv::Mat Xc = gemm3(Rcw, pMP->getPosInWorld(), tcw);
        const cv::Mat Twc = pRefKF->getPoseInverse();
        pMP->setPosInWorld(gemm3(Twc.rowRange(0, 3).colRange(0, 3), Xc, Twc.rowRange(0, 3).colRange(3, 4)));
      }
    }
    report("C", S, mirror, base, got, snapshot(S), corrected, (int)(d.pointSlots.size() + d.keyFrameSlots.size()));
    printf("C_not_reached %d\n", nKf - (int)reached.size());
  }
  YdMapDbStats st;
  ydorb_mapdb_stats(mirror.handle(), &st);
  printf("stats_point_table_growths %d\n", st.point_table_growths);
  return 0;
}
