// TEST-ONLY: EXECUTES the resident forms of the two fuse adapters on the GPU - fuseByProjection(Mirror&, ...) / fuseBySim3(Mirror&, ...)
// of include/ydorb/orbMatcher.hpp and both directions of searchInNeighborsImpl(Mirror&, ...) of include/ydorb/localMapping.hpp over a
// MapMirror with enableAttributes(), enableFeatures() and enableDescriptors() - beside the flat fuseByProjection / fuseBySim3, one call
// per target, on a second copy of the same scene, with stand-ins of Frame / KeyFrame / MapPoint that carry real data.  The scene is
// made here from a seed: a new keyframe and 4 neighbours a few centimetres apart, each with features that hold its own map points,
// and for many points a twin feature in another keyframe, just outside the search radius in x as the reference's window wants it
// (frame.cpp:353), that is empty (the point is added there), holds another point (one replaces the other) or holds the point itself
// (shared: skipped).  The program compares the two copies exactly - every point's observations, bad flag and replaced-by link, every
// keyframe's map-point vector, the return values - and prints one line per figure, "<name> <value>".  The stand-in's beReplacedBy moves
// the observations as MapPoint::replace does and leaves the survivor's descriptor alone (orbMatcher.hpp says why that matters).
// OpenCV is the functional mock of tests/cpu_harness/mockrt, whose float gemm sums in float where the contract of DESIGN.md section 2
// sums exact products in double: the flat copy's projections may differ from the device's in the last bit, which no comparison here
// is sensitive to unless a projection falls on a window or cell boundary to within that bit.
//   localmapping_resident_run
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "ydorb/localMapping.hpp"
#include "ydorb/mapMirror.hpp"

namespace {

struct KeyFrame;
struct MapPoint;
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;

struct Frame {
  static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLine, m_flt_baseLineTimesFx;
};
float Frame::m_flt_fx = 500.f, Frame::m_flt_fy = 500.f, Frame::m_flt_cx = 320.f, Frame::m_flt_cy = 240.f, Frame::m_flt_baseLine = 0.08f,
      Frame::m_flt_baseLineTimesFx = 40.f;

struct KeyFrame : std::enable_shared_from_this<KeyFrame> {
  long m_int_keyFrameID = 0, m_int_fuseTargetForKeyFrameID = -1;
  cv::Mat R, t, O, m_cvMat_descriptors;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors, m_v_invScaleFactorSquares;
  float m_flt_logScaleFactor = 0.f;
  std::vector<MP> mps;
  std::vector<KF> best;
  static float m_flt_minX, m_flt_maxX, m_flt_minY, m_flt_maxY;
  cv::Mat getRotation_c2w() { return R.clone(); }
  cv::Mat getTranslation_c2w() { return t.clone(); }
  cv::Mat getCameraOriginInWorld() { return O.clone(); }
  bool isInImage(const float& x, const float& y) const { return x >= m_flt_minX && x < m_flt_maxX && y >= m_flt_minY && y < m_flt_maxY; }
  bool isBad() { return false; }
  MP getMapPoint(int idx) { return mps[(size_t)idx]; }
  void addMapPoint(const MP& mp, int idx) { mps[(size_t)idx] = mp; }
  void replaceMapPointMatch(size_t idx, const MP& mp) { mps[idx] = mp; }
  void eraseMapPointMatch(size_t idx) { mps[idx].reset(); }
  std::vector<MP> getMapPointMatches() { return mps; }
  std::set<MP> getMatchedMapPointsSet() { std::set<MP> s; for (const MP& mp : mps) if (mp) s.insert(mp); return s; }
  std::vector<KF> getBestCovisibilityKeyFrames(int n) { return std::vector<KF>(best.begin(), best.begin() + std::min<size_t>((size_t)n, best.size())); }
  std::vector<KF> getVectorCovisibleKeyFrames() { return best; }
  void setBadFlag() {}
};
float KeyFrame::m_flt_minX = 0.f, KeyFrame::m_flt_maxX = 640.f, KeyFrame::m_flt_minY = 0.f, KeyFrame::m_flt_maxY = 480.f;

struct MapPoint : std::enable_shared_from_this<MapPoint> {
  int index = -1;
  cv::Mat pos, normal, desc;
  float minDist = 0.f, maxDist = 0.f;
  bool bad = false;
  std::map<KF, size_t> obs;
  KF ref;
  MP replacedBy;
  long m_int_fuseCandidateForKeyFrameID = -1;
  bool isBad() { return bad; }
  int getObservationsNum() { return (int)obs.size(); }
  std::map<KF, size_t> getObservations() { return obs; }
  KF getReferenceKeyFrame() { return ref; }
  cv::Mat getDescriptor() { return desc.clone(); }
  cv::Mat getPosInWorld() { return pos.clone(); }
  cv::Mat getNormal() { return normal.clone(); }
  float getMinDistanceInvariance() { return 0.8f * minDist; }
  float getMaxDistanceInvariance() { return 1.2f * maxDist; }
  float getMinDistance() { return minDist; }
  float getMaxDistance() { return maxDist; }
  bool isInKeyFrame(const KF& kf) { return obs.count(kf) != 0; }
  void addObservation(const KF& kf, size_t idx) { if (!obs.count(kf)) obs[kf] = idx; }
  int predictScaleLevel(const float& dist, const KF& kf) { return ydorb::adapter::predictScaleLevelFormula(maxDist / dist, kf->m_flt_logScaleFactor, (int)kf->m_v_scaleFactors.size()); }
  void beReplacedBy(const MP& by) {   // MapPoint::replace without its last line, the survivor's computeDistinctiveDescriptors()
    if (by.get() == this) return;
    const std::map<KF, size_t> held = obs;
    obs.clear();
    bad = true;
    replacedBy = by;
    for (const auto& ob : held) {
      if (!by->isInKeyFrame(ob.first)) { ob.first->replaceMapPointMatch(ob.second, by); by->addObservation(ob.first, ob.second); }
      else ob.first->eraseMapPointMatch(ob.second);
    }
  }
};
typedef ydorb::adapter::MapMirror<KF, MP> Mirror;

struct World { std::vector<KF> kfs; std::vector<MP> points; };

cv::Mat vec3(double x, double y, double z) { cv::Mat m(3, 1, CV_32F); m.at<float>(0) = (float)x; m.at<float>(1) = (float)y; m.at<float>(2) = (float)z; return m; }

// the same seed gives the same world: the two copies are built independently and share no object
World build(unsigned seed, int nKf, int nFeat) {
  std::mt19937 rng(seed);
  auto uni = [&rng](double lo, double hi) { return lo + (hi - lo) * (double)(rng() >> 8) / (double)(1u << 24); };
  World W;
  std::vector<float> sf(8, 1.f), inv2(8, 1.f);
  for (int l = 1; l < 8; l++) sf[l] = sf[l - 1] * 1.2f;
  for (int l = 0; l < 8; l++) inv2[l] = 1.0f / (sf[l] * sf[l]);
  const float th = 1.0f;
  for (int k = 0; k < nKf; k++) {
    KF kf = std::make_shared<KeyFrame>();
    kf->m_int_keyFrameID = k;
    kf->R = cv::Mat::eye(3, 3, CV_32F);
    kf->O = vec3(0.04 * k, 0.02 * (k % 2), 0.03 * (k % 3));
    kf->t = -kf->O;
    kf->m_v_scaleFactors = sf; kf->m_v_invScaleFactorSquares = inv2;
    kf->m_flt_logScaleFactor = std::log(1.2f);
    kf->m_cvMat_descriptors.create(8 * nFeat, 32, CV_8U);   // trimmed to the feature count below
    W.kfs.push_back(kf);
  }
  auto addFeature = [&](const KF& kf, float x, float y, int octave, float rightX, const unsigned char* d) {
    cv::KeyPoint kp;
    kp.pt.x = x; kp.pt.y = y; kp.size = 31.f; kp.angle = 0.f; kp.response = 1.f; kp.octave = octave; kp.class_id = -1;
    const int idx = (int)kf->m_v_keyPoints.size();
    kf->m_v_keyPoints.push_back(kp); kf->m_v_rightXcords.push_back(rightX); kf->m_v_depth.push_back(-1.f); kf->mps.push_back(MP());
    std::memcpy(kf->m_cvMat_descriptors.ptr<unsigned char>(idx), d, 32);
    return idx;
  };
  auto project = [&](const KF& kf, const cv::Mat& P, float& u, float& v, float& z) {
    const float x = P.at<float>(0) - kf->O.at<float>(0), y = P.at<float>(1) - kf->O.at<float>(1);
    z = P.at<float>(2) - kf->O.at<float>(2);
    u = Frame::m_flt_fx * x / z + Frame::m_flt_cx; v = Frame::m_flt_fy * y / z + Frame::m_flt_cy;
  };
  for (int k = 0; k < nKf; k++) {
    const KF& kf = W.kfs[(size_t)k];
    for (int j = 0; j < nFeat; j++) {
      unsigned char d[32];
      for (int b = 0; b < 32; b++) d[b] = (unsigned char)rng();
      const int octave = (int)(rng() % 6);
      const float x = (float)uni(60, 580), y = (float)uni(60, 420);
      const double z = uni(3.0, 8.0);
      const int idx = addFeature(kf, x, y, octave, -1.f, d);
      if (rng() % 4 == 0) continue;   // a feature without a map point
      MP mp = std::make_shared<MapPoint>();
      mp->index = (int)W.points.size();
      mp->pos = vec3(kf->O.at<float>(0) + (x - Frame::m_flt_cx) * z / Frame::m_flt_fx, kf->O.at<float>(1) + (y - Frame::m_flt_cy) * z / Frame::m_flt_fy,
                     kf->O.at<float>(2) + z);
      const cv::Mat PO = mp->pos - kf->O;
      const float dist = (float)cv::norm(PO);
      mp->normal = PO / (double)dist;
      mp->maxDist = dist * std::pow(1.2f, (float)octave - 0.5f);
      mp->minDist = mp->maxDist / sf[7];
      mp->desc.create(1, 32, CV_8U);
      std::memcpy(mp->desc.data, d, 32);
      for (int f = (int)(rng() % 6); f > 0; f--) mp->desc.data[rng() % 32] ^= (unsigned char)(1u << (rng() % 8));
      mp->ref = kf;
      mp->obs[kf] = (size_t)idx;
      kf->mps[(size_t)idx] = mp;
      kf->m_v_depth[(size_t)idx] = (float)z;
      W.points.push_back(mp);
      // a twin feature in another keyframe, just outside the search radius in x, at the level the point predicts there
      if (rng() % 3 == 0) continue;
      const KF& other = W.kfs[(size_t)((k + 1 + (int)(rng() % (unsigned)(nKf - 1))) % nKf)];
      float u, v, zc;
      project(other, mp->pos, u, v, zc);
      const float side = rng() % 2 ? 1.f : -1.f;
      const float tx = u + side * (th * sf[octave] + (float)uni(0.1, 0.6) * sf[octave]), ty = v + (float)uni(-0.3, 0.3);
      if (tx < 20 || tx > 620 || ty < 20 || ty > 460) continue;
      const int kind = (int)(rng() % 3);
      const int tidx = addFeature(other, tx, ty, octave, kind == 1 ? tx - Frame::m_flt_baseLineTimesFx / zc : -1.f, mp->desc.data);
      if (kind == 2) {   // the twin holds the point itself: shared, isInKeyFrame
        mp->obs[other] = (size_t)tidx;
        other->mps[(size_t)tidx] = mp;
      } else if (rng() % 2) {   // the twin holds another point: one of the two replaces the other
        MP q = std::make_shared<MapPoint>(*mp);
        q->index = (int)W.points.size();
        q->pos = mp->pos.clone(); q->normal = mp->normal.clone(); q->desc = mp->desc.clone();
        q->obs.clear();
        q->ref = other;
        q->obs[other] = (size_t)tidx;
        if (rng() % 2) {   // with more observations than the searched point: it survives
          const KF& third = W.kfs[(size_t)((k + 2) % nKf)];
          if (third != other && third != kf) {
            unsigned char e[32];
            for (int b = 0; b < 32; b++) e[b] = (unsigned char)rng();
            float u3, v3, z3;
            project(third, q->pos, u3, v3, z3);
            const int i3 = addFeature(third, u3 + 30.f, v3, octave, -1.f, e);   // far from the projection: never a candidate
            q->obs[third] = (size_t)i3;
            third->mps[(size_t)i3] = q;
          }
        }
        other->mps[(size_t)tidx] = q;
        W.points.push_back(q);
      }
    }
  }
  for (const KF& kf : W.kfs) {
    if (kf->m_v_keyPoints.size() > (size_t)kf->m_cvMat_descriptors.rows) { fprintf(stderr, "scene: too many features\n"); exit(2); }
    kf->m_cvMat_descriptors = kf->m_cvMat_descriptors.rowRange(0, (int)kf->m_v_keyPoints.size()).clone();   // one row per feature
    for (const KF& o : W.kfs) if (o != kf) kf->best.push_back(o);
  }
  return W;
}

// what the comparison reads of a world, as integers
std::vector<long> stateOf(const World& W) {
  std::vector<long> s;
  for (const MP& mp : W.points) {
    s.push_back(mp->bad ? 1 : 0);
    s.push_back(mp->replacedBy ? mp->replacedBy->index : -1);
    s.push_back((long)mp->obs.size());
    std::vector<std::pair<long, long> > o;
    for (const auto& ob : mp->obs) o.push_back(std::make_pair(ob.first->m_int_keyFrameID, (long)ob.second));
    std::sort(o.begin(), o.end());
    for (const auto& p : o) { s.push_back(p.first); s.push_back(p.second); }
  }
  for (const KF& kf : W.kfs)
    for (const MP& mp : kf->mps) s.push_back(mp ? mp->index : -1);
  return s;
}

Mirror* mirrorOf(World& W) {
  Mirror* mirror = new Mirror(0, 64, 2, 256);   // small: every table grows while the scene is loaded
  mirror->enableAttributes();
  mirror->enableFeatures();
  mirror->enableDescriptors();
  for (const KF& kf : W.kfs) { mirror->touch(kf); mirror->touchRow(kf); mirror->touchDescriptors(kf); mirror->touchFeatures(kf); }
  for (const MP& mp : W.points) { mirror->touch(mp); mirror->touchAttributes(mp); }
  mirror->flush();
  return mirror;
}

int differences(Mirror& mirror) {
  const Mirror::Difference a = mirror.verify(), d = mirror.verifyDescriptors();
  return (int)(a.pointSlots.size() + a.keyFrameSlots.size() + mirror.verifyRows().size() + d.pointSlots.size() + d.keyFrameSlots.size() +
               mirror.verifyAttributes().size() + mirror.verifyFeatures().size());
}

cv::Mat sim3Of(const KF& kf, float scale) {   // [sR | t] with R = I: the keyframe's own pose, scaled
  cv::Mat S = cv::Mat::eye(4, 4, CV_32F);
  for (int r = 0; r < 3; r++) { S.at<float>(r, r) = scale; S.at<float>(r, 3) = kf->t.at<float>(r); }
  return S;
}

}  // namespace

int main() {
  namespace ya = ydorb::adapter;
  const int nKf = 5, nFeat = 60;
  const float th = 1.0f;
  try {
    // ---- searchInNeighbors: flat, one fuseByProjection call per target and one more; resident, two batched calls
    World A = build(7, nKf, nFeat), B = build(7, nKf, nFeat);
    printf("worlds_equal_before %d\npoints %d\n", stateOf(A) == stateOf(B) ? 1 : 0, (int)A.points.size());
    const KF curA = A.kfs[0], curB = B.kfs[0];
    std::vector<int> flat1;
    const std::vector<MP> ownA = curA->getMapPointMatches();
    for (size_t k = 1; k < A.kfs.size(); k++) flat1.push_back(ya::fuseByProjection<KF, MP, Frame>(ya::matcher(), A.kfs[k], ownA, th));
    std::vector<MP> candA;
    for (size_t k = 1; k < A.kfs.size(); k++)
      for (const MP& mp : A.kfs[k]->getMapPointMatches()) {
        if (!mp || mp->isBad() || mp->m_int_fuseCandidateForKeyFrameID == curA->m_int_keyFrameID) continue;
        mp->m_int_fuseCandidateForKeyFrameID = curA->m_int_keyFrameID;
        candA.push_back(mp);
      }
    const int flat2 = ya::fuseByProjection<KF, MP, Frame>(ya::matcher(), curA, candA, th);

    Mirror* mirror = mirrorOf(B);
    printf("verify_before %d\n", differences(*mirror));
    curB->best = std::vector<KF>(B.kfs.begin() + 1, B.kfs.end());
    for (size_t k = 1; k < B.kfs.size(); k++) B.kfs[k]->best.clear();   // the targets are the four neighbours, in order
    const std::pair<std::vector<int>, int> res = ya::searchInNeighborsImpl<Frame, KF, MP>(*mirror, ya::matcher(), curB, 10,
        [](const MP& mp, const KF&, size_t, const cv::Mat& row) { mp->desc = row.clone(); },
        [](const MP& mp, const cv::Mat& normal, float minD, float maxD) { mp->normal = normal.clone(); mp->minDist = minD; mp->maxDist = maxD; }, th);
    int sum1 = 0, replaced = 0, added = 0;
    for (const int n : flat1) sum1 += n;
    for (const MP& mp : A.points) replaced += mp->replacedBy ? 1 : 0;
    for (size_t i = 0; i < A.points.size(); i++) added += A.points[i]->replacedBy ? 0 : (int)A.points[i]->obs.size();
    printf("direction1_counts_same %d\ndirection1_fused %d\ndirection2_flat %d\ndirection2_resident %d\n", res.first == flat1 ? 1 : 0, sum1, flat2, res.second);
    printf("state_same %d\nreplaced %d\nobservations_after %d\n", stateOf(A) == stateOf(B) ? 1 : 0, replaced, added);
    printf("verify_after %d\n", differences(*mirror));
    YdMapDbFeatStats fs;
    ydorb_mapdb_feat_stats(mirror->handle(), &fs);
    printf("features_resident %lld\nlast_feat_sync_bytes %lld\n", (long long)fs.n_features, (long long)fs.last_feat_sync_bytes);
    delete mirror;

    // ---- LoopClosing::searchAndFuse: fuseBySim3 per keyframe against the overload, every keyframe with a Sim3 of its own
    World C = build(11, nKf, nFeat), D = build(11, nKf, nFeat);
    std::vector<MP> loopC, loopD;
    for (size_t i = 0; i < C.points.size(); i += 2) { loopC.push_back(C.points[i]); loopD.push_back(D.points[i]); }
    std::vector<int> simFlat;
    std::vector<cv::Mat> sims;
    for (size_t k = 0; k < C.kfs.size(); k++) {
      sims.push_back(sim3Of(C.kfs[k], 1.0f + 0.002f * (float)k));
      simFlat.push_back(ya::fuseBySim3<KF, MP, Frame>(ya::matcher(), C.kfs[k], sims[k], loopC, th));
    }
    Mirror* m2 = mirrorOf(D);
    const std::vector<int> simRes = ya::fuseBySim3<KF, MP, Frame>(*m2, ya::matcher(), D.kfs, sims, std::vector<std::vector<MP> >(D.kfs.size(), loopD), th);
    int simSum = 0;
    for (const int n : simFlat) simSum += n;
    printf("sim3_counts_same %d\nsim3_fused %d\nsim3_state_same %d\nsim3_verify_after %d\n", simRes == simFlat ? 1 : 0, simSum, stateOf(C) == stateOf(D) ? 1 : 0,
           differences(*m2));
    delete m2;
  } catch (const std::exception& e) {
    fprintf(stderr, "localmapping_resident_run: %s\n", e.what());
    return 1;
  }
  return 0;
}
