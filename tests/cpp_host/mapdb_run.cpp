// TEST-ONLY: executes ydorb::adapter::MapMirror (include/ydorb/mapMirror.hpp) beside the three flattening adapters (mapPoint.hpp,
// keyFrame.hpp, keyFrameCullingImpl) on the same stand-ins of KeyFrame / MapPoint in one program, linked against libydorb.so:
//   mapdb_run in.bin [reps]
// in.bin is mapmaint_run.cpp's scene format.  The program touches everything, compares (phase A), mutates the stand-ins with the touch
// each mutation needs (observations added and erased, a point set bad, positions written back as a BA does, a pose moved, a keyframe
// erased and forgotten) and compares again (phase B), forgets a point and lets a new one take its slot (phase C), and at the end makes
// one mutation without its touch.  It prints one line per figure, "<name> <value>"; tests/test_mapdb_adapter_gpu.py reads them.  A
// comparison is exact: applied flags, float bit patterns, counter maps, the flagged keyframes in order.  With reps it also times the
// adapter-level work both ways, alternating (tools/map_maintenance_bench.py --resident).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <opencv2/core.hpp>

#include "ydorb/keyFrame.hpp"
#include "ydorb/localMapping.hpp"
#include "ydorb/mapMirror.hpp"
#include "ydorb/mapPoint.hpp"

struct KeyFrame;
struct MapPoint {
  int id = 0;
  bool bad = false;
  cv::Mat pos;
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
  void setBadFlag() { if (!notErase) bad = true; }
  bool isBad() { return bad; }
};
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
typedef ydorb::adapter::MapMirror<KF, MP> Mirror;
namespace ya = ydorb::adapter;

static FILE* g_in;
static int32_t geti() { int32_t v = 0; if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static float getf() { float v = 0; if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static cv::Mat vec3() { cv::Mat m(3, 1, CV_32F); for (int r = 0; r < 3; r++) m.at<float>(r) = getf(); return m; }

struct Scene {
  std::vector<KF> kfs;
  std::vector<MP> mps;
  std::vector<int> queries;
  int current = 0;
  float thDepth = 0.f;
};

struct Applied {   // what an apply callback saw, per point id
  std::vector<int32_t> rec;   // applied, normal bits x3, min bits, max bits
  explicit Applied(size_t n) : rec(6 * n, 0) {}
  void operator()(const MP& mp, const cv::Mat& normal, float mn, float mx) {
    int32_t* r = &rec[6 * (size_t)mp->id];
    r[0] = 1;
    for (int i = 0; i < 3; i++) { const float v = normal.at<float>(i); memcpy(&r[1 + i], &v, 4); }
    memcpy(&r[4], &mn, 4); memcpy(&r[5], &mx, 4);
  }
};

static std::vector<int> ids(const std::vector<KF>& v) { std::vector<int> o; for (const KF& k : v) o.push_back((int)k->m_int_keyFrameID); return o; }
static void resetBad(Scene& S, const std::vector<KF>& flagged) { for (const KF& k : flagged) k->bad = false; (void)S; }

// the three adapters both ways, exactly
static void compare(const char* tag, Scene& S, Mirror& mirror) {
  Applied flat(S.mps.size()), res(S.mps.size());
  const int nFlat = ya::updateNormalAndDepthBatch<KF, MP>(S.mps, [&](const MP& mp, const cv::Mat& n, float a, float b) { flat(mp, n, a, b); });
  const int nRes = mirror.updateNormalAndDepth(S.mps, [&](const MP& mp, const cv::Mat& n, float a, float b) { res(mp, n, a, b); });
  printf("%s_normal_same %d\n%s_normal_updated %d\n", tag, (int)(nFlat == nRes && flat.rec == res.rec), tag, nRes);
  int same = 1, total = 0;
  for (int q : S.queries) {
    if (S.kfs[q]->bad) continue;
    const std::map<KF, int> a = ya::covisibilityCounter<KF, MP>(S.kfs[q]), b = mirror.covisibilityCounter(S.kfs[q]);
    same = same && a == b;
    total += (int)b.size();
  }
  printf("%s_covisibility_same %d\n%s_covisibility_connections %d\n", tag, same, tag, total);
  const std::vector<KF> fa = ya::keyFrameCullingImpl<KF, MP>(S.kfs[S.current], S.thDepth, 0);
  resetBad(S, fa);
  const std::vector<KF> fb = mirror.keyFrameCulling(S.kfs[S.current], S.thDepth);
  resetBad(S, fb);
  printf("%s_culling_same %d\n%s_culling_flagged %d\n", tag, (int)(ids(fa) == ids(fb)), tag, (int)fb.size());
  const Mirror::Difference d = mirror.verify();
  printf("%s_verify_differences %d\n", tag, (int)(d.pointSlots.size() + d.keyFrameSlots.size()));
}

static void eraseObservation(const MP& mp, const KF& kf) {
  const auto it = mp->observations.find(kf);
  if (it == mp->observations.end()) return;
  kf->mapPoints[it->second] = MP();
  mp->observations.erase(it);
  if (mp->ref == kf && !mp->observations.empty()) mp->ref = mp->observations.begin()->first;
}
static bool addObservation(const MP& mp, const KF& kf) {
  if (mp->observations.count(kf)) return false;
  for (size_t i = 0; i < kf->mapPoints.size(); i++)
    if (!kf->mapPoints[i]) { kf->mapPoints[i] = mp; mp->observations[kf] = i; return true; }
  return false;
}

template <class F> static double once(F f) {
  const auto t0 = std::chrono::steady_clock::now();
  f();
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
static void report(const char* name, std::vector<double> t) {
  std::sort(t.begin(), t.end());
  printf("time_%s_ms %.4f %.4f %.4f\n", name, t[t.size() / 2], t.front(), t.back());
}

int main(int argc, char** argv) {
  if (argc < 2 || !(g_in = fopen(argv[1], "rb"))) { fprintf(stderr, "usage: mapdb_run in.bin [reps]\n"); return 2; }
  const int reps = argc > 2 ? atoi(argv[2]) : 0;
  Scene S;
  const int nKf = geti(), nPts = geti(), nLevels = geti();
  std::vector<float> sf(nLevels);
  for (float& s : sf) s = getf();
  S.thDepth = getf();
  S.current = geti();
  std::vector<int> covisible(geti());
  for (int& c : covisible) c = geti();
  S.queries.resize(geti());
  for (int& q : S.queries) q = geti();
  S.kfs.resize(nKf); S.mps.resize(nPts);
  for (int k = nKf - 1; k >= 0; k--) if (k % 2 == 1) S.kfs[k] = std::make_shared<KeyFrame>();
  for (int k = 0; k < nKf; k++) if (k % 2 == 0) S.kfs[k] = std::make_shared<KeyFrame>();
  for (int p = 0; p < nPts; p++) { S.mps[p] = std::make_shared<MapPoint>(); S.mps[p]->id = p; }
  for (int k = 0; k < nKf; k++) {
    KeyFrame& K = *S.kfs[k];
    K.m_int_keyFrameID = (long unsigned int)k;
    K.centre = vec3();
    K.notErase = geti() != 0;
    const int n = geti();
    K.m_v_keyPoints.resize(n); K.m_v_rightXcords.resize(n); K.m_v_depth.resize(n); K.mapPoints.resize(n);
    K.m_v_scaleFactors = sf;
    for (int i = 0; i < n; i++) { K.m_v_keyPoints[i] = cv::KeyPoint(); K.m_v_keyPoints[i].octave = geti(); }
    for (int i = 0; i < n; i++) K.m_v_rightXcords[i] = getf();
    for (int i = 0; i < n; i++) K.m_v_depth[i] = getf();
    for (int i = 0; i < n; i++) { const int p = geti(); if (p >= 0) K.mapPoints[i] = S.mps[p]; }
  }
  for (int c : covisible) S.kfs[S.current]->covisible.push_back(S.kfs[c]);
  for (int p = 0; p < nPts; p++) {
    MapPoint& M = *S.mps[p];
    M.pos = vec3();
    M.bad = geti() != 0;
    M.ref = S.kfs[geti()];
    const int n = geti();
    for (int i = 0; i < n; i++) { const int k = geti(), idx = geti(); M.observations[S.kfs[k]] = (size_t)idx; }
  }

  Mirror mirror(0, 64, 4, 256);   // small on purpose: every table grows while the scene is loaded
  for (const KF& k : S.kfs) mirror.touch(k);
  for (const MP& m : S.mps) mirror.touch(m);
  compare("A", S, mirror);

  if (reps > 0) {   // the adapter-level work both ways, alternating; culling's flags are reset outside the clock
    std::vector<double> tf[3], tr[3], tt[2];
    const KF cur = S.kfs[S.current];
    auto sink = [](const MP&, const cv::Mat&, float, float) {};
    for (int r = 0; r < reps + 1; r++) {
      double a = once([&] { ya::updateNormalAndDepthBatch<KF, MP>(S.mps, sink); });
      double b = once([&] { mirror.updateNormalAndDepth(S.mps, sink); });
      if (r) { tf[0].push_back(a); tr[0].push_back(b); }
      a = once([&] { for (int q : S.queries) ya::covisibilityCounter<KF, MP>(S.kfs[q]); });
      b = once([&] { for (int q : S.queries) mirror.covisibilityCounter(S.kfs[q]); });
      if (r) { tf[1].push_back(a); tr[1].push_back(b); }
      std::vector<KF> f;
      a = once([&] { f = ya::keyFrameCullingImpl<KF, MP>(cur, S.thDepth, 0); });
      resetBad(S, f);
      b = once([&] { f = mirror.keyFrameCulling(cur, S.thDepth); });
      resetBad(S, f);
      if (r) { tf[2].push_back(a); tr[2].push_back(b); }
      // the price of the touches: 300 points re-read and flushed, and every point
      for (int p = 0; p < std::min(300, nPts); p++) mirror.touch(S.mps[p]);
      a = once([&] { mirror.flush(); });
      for (const MP& m : S.mps) mirror.touch(m);
      b = once([&] { mirror.flush(); });
      if (r) { tt[0].push_back(a); tt[1].push_back(b); }
    }
    const char* names[3] = {"normal_depth", "covisibility", "culling"};
    for (int i = 0; i < 3; i++) { report((std::string("flat_") + names[i]).c_str(), tf[i]); report((std::string("mirror_") + names[i]).c_str(), tr[i]); }
    report("mirror_flush_300_touched", tt[0]); report("mirror_flush_all_touched", tt[1]);
  }

  // ---- mutations, each with its touch
  int added = 0, erased = 0;
  for (int p = 0; p < nPts && added < 40; p += 7)       // addObservation
    for (int k = 1; k < nKf; k += 3)
      if (addObservation(S.mps[p], S.kfs[k])) { mirror.touch(S.mps[p]); added++; break; }
  for (int p = 3; p < nPts && erased < 40; p += 11) {   // eraseObservation
    if (S.mps[p]->observations.size() < 2) continue;
    eraseObservation(S.mps[p], S.mps[p]->observations.begin()->first);
    mirror.touch(S.mps[p]);
    erased++;
  }
  for (int p = 5; p < nPts; p += 97) { S.mps[p]->bad = true; mirror.touch(S.mps[p]); }   // setBadFlag
  for (int p = 0; p < std::min(200, nPts); p++) {                                          // a BA write-back
    for (int r = 0; r < 3; r++) S.mps[p]->pos.at<float>(r) += 0.03125f * (float)(1 + r);
    mirror.touchPosition(S.mps[p]);
  }
  for (int k : {2, 9}) { S.kfs[k]->centre.at<float>(0) += 0.5f; S.kfs[k]->centre.at<float>(2) -= 0.25f; mirror.touch(S.kfs[k]); }   // setPose
  {   // a keyframe erased from the map: its observations go from every point, the covisibility list drops it, the mirror forgets it
    const KF gone = S.kfs[covisible[1] == S.current ? covisible[2] : covisible[1]];
    for (const MP& mp : std::vector<MP>(gone->mapPoints)) if (mp) { eraseObservation(mp, gone); mirror.touch(mp); }
    std::vector<KF>& list = S.kfs[S.current]->covisible;
    list.erase(std::remove(list.begin(), list.end(), gone), list.end());
    gone->bad = true;
    mirror.forget(gone);
    printf("erased_keyframe %d\n", (int)gone->m_int_keyFrameID);
  }
  printf("mutations_added %d\nmutations_erased %d\n", added, erased);
  compare("B", S, mirror);

  {   // a point leaves the map and a new one takes its slot
    const MP old = S.mps[17];
    const int32_t slot = mirror.slotOf(old);
    for (const auto& ob : std::map<KF, size_t>(old->observations)) eraseObservation(old, ob.first);
    mirror.forget(old);
    MP fresh = std::make_shared<MapPoint>();
    fresh->id = 17; fresh->pos = old->pos.clone(); fresh->ref = S.kfs[4];
    addObservation(fresh, S.kfs[4]); addObservation(fresh, S.kfs[6]); addObservation(fresh, S.kfs[8]);
    S.mps[17] = fresh;
    mirror.touch(fresh);
    printf("slot_reused %d\n", (int)(mirror.slotOf(fresh) == slot && mirror.slotOf(old) == -1));
  }
  compare("C", S, mirror);

  {   // one mutation without its touch: verify() names exactly that slot, results differ, nothing fails
    MP victim;
    for (int p = 100; p < nPts && !victim; p++) if (!S.mps[p]->bad && S.mps[p]->observations.size() >= 3) victim = S.mps[p];
    KF which = victim->observations.begin()->first;
    if (which == victim->ref) which = (++victim->observations.begin())->first;
    eraseObservation(victim, which);
    const Mirror::Difference d = mirror.verify();
    printf("missed_touch_slot %d\nverify_named %d\nverify_named_slot %d\n", (int)mirror.slotOf(victim), (int)(d.pointSlots.size() + d.keyFrameSlots.size()),
           d.pointSlots.empty() ? -1 : (int)d.pointSlots[0]);
    Applied flat(S.mps.size()), res(S.mps.size());
    ya::updateNormalAndDepthBatch<KF, MP>(S.mps, [&](const MP& mp, const cv::Mat& n, float a, float b) { flat(mp, n, a, b); });
    mirror.updateNormalAndDepth(S.mps, [&](const MP& mp, const cv::Mat& n, float a, float b) { res(mp, n, a, b); });
    int differ = 0;
    for (size_t p = 0; p < S.mps.size(); p++) differ += memcmp(&flat.rec[6 * p], &res.rec[6 * p], 24) != 0;
    printf("missed_touch_points_that_differ %d\nmissed_touch_differs_at_victim %d\n", differ,
           (int)(memcmp(&flat.rec[6 * (size_t)victim->id], &res.rec[6 * (size_t)victim->id], 24) != 0));
    mirror.touch(victim);
    const Mirror::Difference after = mirror.verify();
    printf("verify_after_the_touch %d\n", (int)(after.pointSlots.size() + after.keyFrameSlots.size()));
  }
  YdMapDbStats st;
  ydorb_mapdb_stats(mirror.handle(), &st);
  printf("stats_point_table_growths %d\nstats_keyframe_table_growths %d\nstats_repacks %d\n", st.point_table_growths, st.keyframe_table_growths,
         st.repacks_kept + st.repacks_grown);
  return 0;
}
