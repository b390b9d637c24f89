// TEST-ONLY: executes the map-maintenance adapters (include/ydorb/mapPoint.hpp, keyFrame.hpp, keyFrameCullingImpl of localMapping.hpp)
// on stand-ins of KeyFrame / MapPoint that carry data, linked against libydorb.so:   mapmaint_run in.bin out.bin
// The observation containers are std::maps keyed by the stand-in pointer, so their iteration order is the allocator's; the program
// dumps it and the Python side (tests/test_mapmaint_adapter_gpu.py) replays in that order.  It also times the three flattenings on the
// host (printed as "flatten_<name>_us <microseconds>"), which tools/map_maintenance_bench.py reports beside the entries' own times.
// in.bin (int32 / float32, little endian):
//   n_kf n_points n_levels | scale_factors[n_levels] | thDepth | current | n_covisible covisible[] | n_queries queries[]
//   per keyframe: centre[3] not_erase n_kp | octave[n_kp] | right_x[n_kp] | depth[n_kp] | map_point[n_kp] (-1 = null)
//   per point: pos[3] bad ref_kf n_obs | (kf idx)[n_obs]
// out.bin: per point n_obs kf[n_obs] (iteration order) | per point applied normal[3] min max | per query n (kf weight)[n] |
//   n_flagged flagged[] | bad[n_kf]
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <vector>

#include <opencv2/core.hpp>

#include "ydorb/keyFrame.hpp"
#include "ydorb/localMapping.hpp"
#include "ydorb/mapPoint.hpp"

struct KeyFrame;
struct MapPoint {
  int id = 0;
  bool bad = false, applied = false;
  cv::Mat pos, normal;
  float minD = 0.f, maxD = 0.f;
  std::shared_ptr<KeyFrame> ref;
  std::map<std::shared_ptr<KeyFrame>, size_t> observations;
  bool isBad() { return bad; }
  std::map<std::shared_ptr<KeyFrame>, size_t> getObservations() { return observations; }
  cv::Mat getPosInWorld() { return pos.clone(); }
  std::shared_ptr<KeyFrame> getReferenceKeyFrame() { return ref; }
};
struct KeyFrame {
  long unsigned int m_int_keyFrameID = 0;
  bool bad = false, notErase = false;
  cv::Mat centre;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  std::vector<std::shared_ptr<MapPoint>> mapPoints;
  std::vector<std::shared_ptr<KeyFrame>> covisible;
  cv::Mat getCameraOriginInWorld() { return centre.clone(); }
  std::vector<std::shared_ptr<MapPoint>> getMapPointMatches() { return mapPoints; }
  std::vector<std::shared_ptr<KeyFrame>> getVectorCovisibleKeyFrames() { return covisible; }
  void setBadFlag() { if (!notErase) bad = true; }   // a protected keyframe is only marked (mbToBeErased)
  bool isBad() { return bad; }
};
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;

static FILE* g_in;
static FILE* g_out;
static int32_t geti() { int32_t v = 0; if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static float getf() { float v = 0; if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static void puti(int32_t v) { fwrite(&v, 4, 1, g_out); }
static void putf(float v) { fwrite(&v, 4, 1, g_out); }
static cv::Mat vec3() { cv::Mat m(3, 1, CV_32F); for (int r = 0; r < 3; r++) m.at<float>(r) = getf(); return m; }

template <class F> static void timed(const char* name, F f) {
  const auto t0 = std::chrono::steady_clock::now();
  f();
  const auto t1 = std::chrono::steady_clock::now();
  printf("flatten_%s_us %.1f\n", name, std::chrono::duration<double, std::micro>(t1 - t0).count());
}

int main(int argc, char** argv) {
  if (argc != 3 || !(g_in = fopen(argv[1], "rb")) || !(g_out = fopen(argv[2], "wb"))) { fprintf(stderr, "usage: mapmaint_run in.bin out.bin\n"); return 2; }
  namespace ya = ydorb::adapter;
  const int nKf = geti(), nPts = geti(), nLevels = geti();
  std::vector<float> sf(nLevels);
  for (float& s : sf) s = getf();
  const float thDepth = getf();
  const int current = geti();
  std::vector<int> covisible(geti());
  for (int& c : covisible) c = geti();
  std::vector<int> queries(geti());
  for (int& q : queries) q = geti();
  std::vector<KF> kfs(nKf);
  std::vector<MP> mps(nPts);
  // allocated odd ids downwards, then even ids upwards: the pointer-keyed containers then do not iterate by id
  for (int k = nKf - 1; k >= 0; k--) if (k % 2 == 1) kfs[k] = std::make_shared<KeyFrame>();
  for (int k = 0; k < nKf; k++) if (k % 2 == 0) kfs[k] = std::make_shared<KeyFrame>();
  for (int p = 0; p < nPts; p++) { mps[p] = std::make_shared<MapPoint>(); mps[p]->id = p; }
  for (int k = 0; k < nKf; k++) {
    KeyFrame& K = *kfs[k];
    K.m_int_keyFrameID = (long unsigned int)k;
    K.centre = vec3();
    K.notErase = geti() != 0;
    const int n = geti();
    K.m_v_keyPoints.resize(n); K.m_v_rightXcords.resize(n); K.m_v_depth.resize(n); K.mapPoints.resize(n);
    K.m_v_scaleFactors = sf;
    for (int i = 0; i < n; i++) { K.m_v_keyPoints[i] = cv::KeyPoint(); K.m_v_keyPoints[i].octave = geti(); }
    for (int i = 0; i < n; i++) K.m_v_rightXcords[i] = getf();
    for (int i = 0; i < n; i++) K.m_v_depth[i] = getf();
    for (int i = 0; i < n; i++) { const int p = geti(); if (p >= 0) K.mapPoints[i] = mps[p]; }
  }
  for (int c : covisible) kfs[current]->covisible.push_back(kfs[c]);
  for (int p = 0; p < nPts; p++) {
    MapPoint& M = *mps[p];
    M.pos = vec3();
    M.bad = geti() != 0;
    M.ref = kfs[geti()];
    const int n = geti();
    for (int i = 0; i < n; i++) { const int k = geti(), idx = geti(); M.observations[kfs[k]] = (size_t)idx; }
  }
  for (int p = 0; p < nPts; p++) {
    puti((int32_t)mps[p]->observations.size());
    for (const auto& ob : mps[p]->observations) puti((int32_t)ob.first->m_int_keyFrameID);
  }
  // the flattenings alone, host time (the adapters below flatten again)
  timed("normal_depth", [&] { ya::NormalDepthFlat<KF, MP> F; ya::flattenNormalDepth<KF, MP>(mps, F); });
  timed("covisibility", [&] { for (int q : queries) { ya::CovisibilityFlat<KF, MP> F; ya::flattenCovisibility(kfs[q], F); } });
  timed("culling", [&] { ya::CullingFlat<KF, MP> F; ya::flattenCulling(kfs[current], thDepth, F); });

  ya::updateNormalAndDepthBatch<KF, MP>(mps, [](const MP& mp, const cv::Mat& normal, float mn, float mx) {
    mp->normal = normal.clone(); mp->minD = mn; mp->maxD = mx; mp->applied = true;
  });
  for (int p = 0; p < nPts; p++) {
    puti(mps[p]->applied ? 1 : 0);
    for (int r = 0; r < 3; r++) putf(mps[p]->applied ? mps[p]->normal.at<float>(r) : 0.f);
    putf(mps[p]->minD); putf(mps[p]->maxD);
  }
  for (int q : queries) {
    const std::map<KF, int> counter = ya::covisibilityCounter<KF, MP>(kfs[q]);
    puti((int32_t)counter.size());
    for (const auto& kv : counter) { puti((int32_t)kv.first->m_int_keyFrameID); puti(kv.second); }
  }
  const std::vector<KF> flagged = ya::keyFrameCullingImpl<KF, MP>(kfs[current], thDepth, 0);
  puti((int32_t)flagged.size());
  for (const KF& k : flagged) puti((int32_t)k->m_int_keyFrameID);
  for (int k = 0; k < nKf; k++) puti(kfs[k]->bad ? 1 : 0);
  fclose(g_out);
  return 0;
}
