// TEST-ONLY: EXECUTES the resident overload localBundleAdjustImpl<Frame>(mirror, ...) of include/ydorb/optimizer.hpp on the GPU beside
// the flat localBundleAdjustImpl on a second copy of the same scene, with stand-ins of KeyFrame / MapPoint / Map that carry real data,
// once with the stop flag clear and once with it set before the solve.  The scene is made here from a seed: 10 keyframes along x
// looking down z (id 0 among the connected ones, one connected keyframe bad, four seen only through the points), 260 points projected
// into the keyframes that see them with a little noise and, for some observations, a gross error that the solve marks as an outlier;
// mono and stereo features mixed.  The observation container is ordered by keyframe id, so that both copies walk it alike (the
// reference's order by pointer would differ between two copies).  The flat copy's MapPoint::updateNormalAndDepth is the flat
// batched adapter of mapPoint.hpp on the one point.  The program compares the two copies exactly - poses, positions, observations,
// map-point vectors, normals and distances as bit patterns - and prints one line per figure, "<name> <value>".
//   localba_resident_run
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <vector>

#include "ydorb/mapMirror.hpp"
#include "ydorb/mapPoint.hpp"
#include "ydorb/optimizer.hpp"

namespace {

struct KeyFrame;
struct MapPoint;
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
struct ById { bool operator()(const KF& a, const KF& b) const; };
typedef std::map<KF, size_t, ById> Observations;

struct Frame { static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLineTimesFx; };
float Frame::m_flt_fx = 500.f, Frame::m_flt_fy = 500.f, Frame::m_flt_cx = 320.f, Frame::m_flt_cy = 240.f, Frame::m_flt_baseLineTimesFx = 40.f;

struct KeyFrame {
  long int m_int_keyFrameID = 0, m_int_localBAForKeyFrameID = -1, m_int_fixedBAForKeyFrameID = -1;
  bool bad = false;
  cv::Mat pose, m_cvMat_descriptors;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_scaleFactors, m_v_invScaleFactorSquares;
  std::vector<MP> mps;
  std::vector<KF> connected;
  std::vector<MP> getMatchedMapPointsVec() { return mps; }
  std::vector<MP> getMapPointMatches() { return mps; }
  std::vector<KF> getOrderedConnectedKeyFrames() { return connected; }
  bool isBad() { return bad; }
  cv::Mat getCameraPoseByTransform_c2w() { return pose.clone(); }
  void setCameraPoseByTransform_c2w(cv::Mat T) { pose = T.clone(); }
  cv::Mat getCameraOriginInWorld() {   // -R^T t, one rounded operation at a time
    cv::Mat O(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
      float acc = 0.f;
      for (int k = 0; k < 3; k++) { const float p = pose.at<float>(k, r) * pose.at<float>(k, 3); acc = acc + p; }
      O.at<float>(r) = -acc;
    }
    return O;
  }
  void eraseMatchedMapPoint(const MP& mp) { for (MP& p : mps) if (p == mp) p.reset(); }
};
bool ById::operator()(const KF& a, const KF& b) const { return a->m_int_keyFrameID < b->m_int_keyFrameID; }

struct MapPoint : std::enable_shared_from_this<MapPoint> {
  int index = -1;
  bool bad = false;
  cv::Mat pos, normal, desc;
  float minDist = 0.f, maxDist = 0.f;
  Observations obs;
  KF ref;
  long int m_int_localBAForKeyFrameID = -1;
  bool isBad() { return bad; }
  Observations getObservations() { return obs; }
  KF getReferenceKeyFrame() { return ref; }
  cv::Mat getPosInWorld() { return pos.clone(); }
  cv::Mat getNormal() { return normal.clone(); }
  cv::Mat getDescriptor() { return desc.clone(); }
  float getMinDistance() { return minDist; }
  float getMaxDistance() { return maxDist; }
  void setPosInWorld(const cv::Mat& p) { pos = p.clone(); }
  void eraseObservation(const KF& kf) {
    obs.erase(kf);
    if (ref == kf && !obs.empty()) ref = obs.begin()->first;
  }
  void store(const cv::Mat& n, float mn, float mx) { normal = n.clone(); minDist = mn; maxDist = mx; }
  void updateNormalAndDepth() {   // the flat copy: the batched flat adapter on this one point
    const std::vector<MP> self(1, shared_from_this());
    ydorb::adapter::updateNormalAndDepthBatch<KF, MP>(self, [](const MP& mp, const cv::Mat& n, float mn, float mx) { mp->store(n, mn, mx); });
  }
};
struct Map { std::mutex m_mutex_updateMap; };
typedef ydorb::adapter::MapMirror<KF, MP> Mirror;

struct World { std::vector<KF> kfs; std::vector<MP> points; KF kf0; };

World build(unsigned seed) {
  std::mt19937 rng(seed);
  auto uni = [&rng](double lo, double hi) { return lo + (hi - lo) * (double)(rng() >> 8) / (double)(1u << 24); };
  World W;
  const int nKf = 10, nPts = 260;
  std::vector<float> sf(8, 1.f), inv2(8, 1.f);
  for (int l = 1; l < 8; l++) sf[(size_t)l] = sf[(size_t)l - 1] * 1.2f;
  for (int l = 0; l < 8; l++) inv2[(size_t)l] = 1.0f / (sf[(size_t)l] * sf[(size_t)l]);
  std::vector<double> cx((size_t)nKf);
  for (int k = 0; k < nKf; k++) {
    KF kf = std::make_shared<KeyFrame>();
    kf->m_int_keyFrameID = k;
    cx[(size_t)k] = 0.3 * k;
    kf->pose = cv::Mat::eye(4, 4, CV_32F);
    kf->pose.at<float>(0, 3) = (float)(-cx[(size_t)k] + (k ? uni(-0.02, 0.02) : 0.0));   // a little off the truth: the solve moves it
    kf->pose.at<float>(1, 3) = (float)(k ? uni(-0.02, 0.02) : 0.0);
    kf->m_v_scaleFactors = sf; kf->m_v_invScaleFactorSquares = inv2;
    W.kfs.push_back(kf);
  }
  for (int p = 0; p < nPts; p++) {
    MP mp = std::make_shared<MapPoint>();
    mp->index = p;
    const double X = uni(-1.5, 4.5), Y = uni(-1.5, 1.5), Z = uni(4.0, 9.0);
    mp->pos = cv::Mat(3, 1, CV_32F);
    mp->pos.at<float>(0) = (float)(X + uni(-0.03, 0.03)); mp->pos.at<float>(1) = (float)(Y + uni(-0.03, 0.03)); mp->pos.at<float>(2) = (float)(Z + uni(-0.03, 0.03));
    mp->bad = rng() % 40 == 0;
    mp->desc.create(1, 32, CV_8U);
    for (int b = 0; b < 32; b++) mp->desc.data[b] = (unsigned char)(7 * p + b);
    for (int k = 0; k < nKf; k++) {
      if (rng() % 5 < 2) continue;
      const KF& kf = W.kfs[(size_t)k];
      double u = 500.0 * (X - cx[(size_t)k]) / Z + 320.0 + uni(-0.4, 0.4), v = 500.0 * Y / Z + 240.0 + uni(-0.4, 0.4);
      if (rng() % 25 == 0) u += 30.0;   // a gross error: an outlier edge
      cv::KeyPoint kp;
      kp.pt.x = (float)u; kp.pt.y = (float)v; kp.size = 31.f; kp.angle = 0.f; kp.response = 1.f; kp.octave = (int)(rng() % 8); kp.class_id = -1;
      const size_t idx = kf->m_v_keyPoints.size();
      kf->m_v_keyPoints.push_back(kp);
      kf->m_v_rightXcords.push_back(rng() % 2 ? (float)(u - 40.0 / Z) : -1.f);
      kf->mps.push_back(mp);
      mp->obs[kf] = idx;
      if (rng() % 4 == 0) {   // a feature without a map point beside it
        kf->m_v_keyPoints.push_back(kp); kf->m_v_rightXcords.push_back(-1.f); kf->mps.push_back(MP());
      }
    }
    if (!mp->obs.empty()) mp->ref = mp->obs.begin()->first;
    else mp->ref = W.kfs[0];
    W.points.push_back(mp);
  }
  for (const KF& kf : W.kfs) kf->m_cvMat_descriptors.create((int)kf->m_v_keyPoints.size(), 32, CV_8U);
  W.kf0 = W.kfs[2];
  for (const int k : {1, 0, 3, 4, 5}) W.kf0->connected.push_back(W.kfs[(size_t)k]);   // id 0 is local: fixed by its id
  W.kfs[4]->bad = true;                                                              // a bad connected keyframe: left out everywhere
  // the normals and distances both copies start from
  ydorb::adapter::updateNormalAndDepthBatch<KF, MP>(W.points, [](const MP& mp, const cv::Mat& n, float mn, float mx) { mp->store(n, mn, mx); });
  return W;
}

void putf(std::vector<int32_t>& s, float v) { int32_t b; std::memcpy(&b, &v, 4); s.push_back(b); }
std::vector<int32_t> stateOf(const World& W) {
  std::vector<int32_t> s;
  for (const KF& kf : W.kfs) {
    for (int i = 0; i < 16; i++) putf(s, kf->pose.ptr<float>()[i]);
    for (const MP& mp : kf->mps) s.push_back(mp ? mp->index : -1);
  }
  for (const MP& mp : W.points) {
    for (int r = 0; r < 3; r++) putf(s, mp->pos.at<float>(r));
    for (int r = 0; r < 3; r++) putf(s, mp->normal.empty() ? 0.f : mp->normal.at<float>(r));
    putf(s, mp->minDist); putf(s, mp->maxDist);
    s.push_back((int32_t)mp->obs.size());
    for (const auto& ob : mp->obs) { s.push_back((int32_t)ob.first->m_int_keyFrameID); s.push_back((int32_t)ob.second); }
    s.push_back(mp->ref ? (int32_t)mp->ref->m_int_keyFrameID : -1);
  }
  return s;
}
int observations(const World& W) { int n = 0; for (const MP& mp : W.points) n += (int)mp->obs.size(); return n; }

Mirror* mirrorOf(World& W, bool descriptors, bool features) {
  Mirror* mirror = new Mirror(0, 64, 2, 256);   // small: every table grows while the scene is loaded
  mirror->enableAttributes();
  if (features) mirror->enableFeatures();
  if (descriptors) mirror->enableDescriptors();
  for (const KF& kf : W.kfs) {
    mirror->touch(kf); mirror->touchRow(kf);
    if (descriptors) mirror->touchDescriptors(kf);
    if (features) mirror->touchFeatures(kf);
  }
  for (const MP& mp : W.points) { mirror->touch(mp); mirror->touchAttributes(mp); }
  mirror->flush();
  return mirror;
}
int differences(Mirror& mirror) {
  const Mirror::Difference a = mirror.verify(), d = mirror.verifyDescriptors();
  return (int)(a.pointSlots.size() + a.keyFrameSlots.size() + mirror.verifyRows().size() + d.pointSlots.size() + d.keyFrameSlots.size() +
               mirror.verifyFeatures().size() + mirror.verifyAttributes().size());
}
const auto storeNormal = [](const MP& mp, const cv::Mat& n, float mn, float mx) { mp->store(n, mn, mx); };

bool refuses(World& W, bool descriptors, bool features, const char* needle) {
  Mirror* m = mirrorOf(W, descriptors, features);
  bool refused = false;
  try { m->localBaGraph(std::vector<KF>(1, W.kf0)); }
  catch (const std::exception& e) { refused = std::strstr(e.what(), needle) != nullptr; }
  delete m;
  return refused;
}

}  // namespace

int main() {
  namespace ya = ydorb::adapter;
  try {
    for (int pass = 0; pass < 2; pass++) {
      const char* tag = pass ? "stopped" : "solved";
      bool stop = pass == 1;
      World A = build(21), B = build(21);
      const std::vector<int32_t> before = stateOf(A);
      printf("%s_worlds_equal_before %d\n", tag, before == stateOf(B) ? 1 : 0);
      const int obsBefore = observations(A);
      auto mapA = std::make_shared<Map>(), mapB = std::make_shared<Map>();
      ya::localBundleAdjustImpl<KF, std::shared_ptr<Map>, Frame>(A.kf0, mapA, &stop);
      Mirror* mirror = mirrorOf(B, true, true);
      printf("%s_verify_before %d\n", tag, differences(*mirror));
      ya::localBundleAdjustImpl<Frame>(*mirror, B.kf0, mapB, &stop, storeNormal);
      const std::vector<int32_t> a = stateOf(A), b = stateOf(B);
      int moved = 0;
      for (size_t i = 0; i < a.size(); i++) moved += a[i] != before[i];
      printf("%s_state_same %d\n%s_values_changed %d\n%s_observations_erased %d\n", tag, a == b ? 1 : 0, tag, moved, tag, obsBefore - observations(A));
      printf("%s_verify_after %d\n", tag, differences(*mirror));
      if (!pass) {
        YdMapDbLbaStats st;
        ydorb_mapdb_lba_stats(mirror->handle(), &st);
        printf("graph_local %lld\ngraph_fixed %lld\ngraph_points %lld\ngraph_edges %lld\n", (long long)st.last_n_local, (long long)st.last_n_fixed,
               (long long)st.last_n_points, (long long)st.last_n_edges);
      }
      delete mirror;
    }
    World C = build(21);
    printf("refused_without_descriptors %d\n", refuses(C, false, true, "without enableDescriptors()") ? 1 : 0);
    printf("refused_without_features %d\n", refuses(C, true, false, "without enableFeatures()") ? 1 : 0);
  } catch (const std::exception& e) {
    fprintf(stderr, "localba_resident_run: %s\n", e.what());
    return 1;
  }
  return 0;
}
