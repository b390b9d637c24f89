// TEST-ONLY: executes updateLocalKeyFramesImpl / updateLocalPointsImpl (include/ydorb/tracking.hpp) over ydorb::adapter::MapMirror's
// keyframe rows (include/ydorb/mapMirror.hpp) beside the two reference loops written out on the same stand-ins of Frame / KeyFrame /
// MapPoint (those of mapdb_run.cpp, with the members the local map reads added), in one program linked against libydorb.so:
//   localmap_run [reps]
// It builds a seeded scene (140 keyframes in a chain with a spanning tree and covisibility lists, 4 000 points), and compares the two
// ways for four frames - a window whose expansion meets the parent `break`, one whose counter alone holds more than 80 keyframes, one
// that passes 80 inside the expansion, one around bad keyframes - in four states: after touching everything (A), after addMapPoint /
// erase / replace mutations, a new keyframe and a point set bad, each with its touches (B), after a keyframe was forgotten and its
// slot reused (C), and after a mutation made without its touch (D: verifyRows() names that keyframe).  It prints one line per figure,
// "<name> <value>"; tests/test_localmap_adapter_gpu.py reads them.  A comparison is exact: the local keyframe vector, the reference
// keyframe, the local point vector in order, the seen flags, the nulled frame entries.  With reps it also times, in state A, the two
// reference loops and the two adapters over all frames, alternating (tools/map_maintenance_bench.py --local-map).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include <opencv2/core.hpp>

#include "ydorb/mapMirror.hpp"
#include "ydorb/tracking.hpp"

struct KeyFrame;
struct MapPoint {
  int id = 0;
  bool bad = false;
  cv::Mat pos;
  std::shared_ptr<KeyFrame> ref;
  std::map<std::shared_ptr<KeyFrame>, size_t> observations;
  long unsigned int m_int_trackReferenceForFrameID = 0;
  bool isBad() { return bad; }
  std::map<std::shared_ptr<KeyFrame>, size_t> getObservations() { return observations; }
  cv::Mat getPosInWorld() { return pos.clone(); }
  std::shared_ptr<KeyFrame> getReferenceKeyFrame() { return ref; }
};
struct KeyFrame {
  long unsigned int m_int_keyFrameID = 0, m_int_trackReferenceForFrameID = 0;
  bool bad = false, notErase = false;
  cv::Mat centre;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  std::vector<std::shared_ptr<MapPoint>> mapPoints;
  std::vector<std::shared_ptr<KeyFrame>> covisible;
  std::set<std::shared_ptr<KeyFrame>> children;
  std::shared_ptr<KeyFrame> parent;
  cv::Mat getCameraOriginInWorld() { return centre.clone(); }
  std::vector<std::shared_ptr<MapPoint>> getMapPointMatches() { return mapPoints; }
  std::vector<std::shared_ptr<KeyFrame>> getVectorCovisibleKeyFrames() { return covisible; }
  std::vector<std::shared_ptr<KeyFrame>> getBestCovisibilityKeyFrames(const int& n) {
    return std::vector<std::shared_ptr<KeyFrame>>(covisible.begin(), covisible.begin() + std::min<size_t>((size_t)n, covisible.size()));
  }
  std::set<std::shared_ptr<KeyFrame>> getChildren() { return children; }
  std::shared_ptr<KeyFrame> getParent() { return parent; }
  void setBadFlag() { if (!notErase) bad = true; }
  bool isBad() { return bad; }
};
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
struct Frame {
  long unsigned int m_int_ID = 0;
  std::vector<MP> m_v_sptrMapPoints;
  KF m_sptr_referenceKeyFrame;
};
typedef ydorb::adapter::MapMirror<KF, MP> Mirror;
namespace ya = ydorb::adapter;

static uint32_t g_rng = 12345u;
static int rnd(int n) { g_rng = g_rng * 1664525u + 1013904223u; return (int)((g_rng >> 8) % (uint32_t)n); }

// ---- the two reference loops, as ORB-SLAM2 writes them
static void refUpdateLocalKeyFrames(Frame& frame, std::vector<KF>& localKeyFrames, KF& referenceKeyFrame) {
  std::map<KF, int> keyframeCounter;
  for (size_t i = 0; i < frame.m_v_sptrMapPoints.size(); i++) {
    if (frame.m_v_sptrMapPoints[i]) {
      const MP mp = frame.m_v_sptrMapPoints[i];
      if (!mp->isBad()) {
        const std::map<KF, size_t> observations = mp->getObservations();
        for (const auto& ob : observations) keyframeCounter[ob.first]++;
      } else {
        frame.m_v_sptrMapPoints[i] = MP();
      }
    }
  }
  if (keyframeCounter.empty()) return;
  int max = 0;
  KF kfMax;
  localKeyFrames.clear();
  localKeyFrames.reserve(3 * keyframeCounter.size());
  for (const auto& it : keyframeCounter) {
    const KF kf = it.first;
    if (kf->isBad()) continue;
    if (it.second > max) { max = it.second; kfMax = kf; }
    localKeyFrames.push_back(it.first);
    kf->m_int_trackReferenceForFrameID = frame.m_int_ID;
  }
  for (std::vector<KF>::const_iterator itKF = localKeyFrames.begin(), itEndKF = localKeyFrames.end(); itKF != itEndKF; itKF++) {
    if (localKeyFrames.size() > 80) break;
    const KF kf = *itKF;
    const std::vector<KF> neighs = kf->getBestCovisibilityKeyFrames(10);
    for (const KF& n : neighs) {
      if (!n->isBad()) {
        if (n->m_int_trackReferenceForFrameID != frame.m_int_ID) { localKeyFrames.push_back(n); n->m_int_trackReferenceForFrameID = frame.m_int_ID; break; }
      }
    }
    const std::set<KF> childs = kf->getChildren();
    for (const KF& c : childs) {
      if (!c->isBad()) {
        if (c->m_int_trackReferenceForFrameID != frame.m_int_ID) { localKeyFrames.push_back(c); c->m_int_trackReferenceForFrameID = frame.m_int_ID; break; }
      }
    }
    const KF parent = kf->getParent();
    if (parent) {
      if (parent->m_int_trackReferenceForFrameID != frame.m_int_ID) { localKeyFrames.push_back(parent); parent->m_int_trackReferenceForFrameID = frame.m_int_ID; break; }
    }
  }
  if (kfMax) { referenceKeyFrame = kfMax; frame.m_sptr_referenceKeyFrame = referenceKeyFrame; }
}

static void refUpdateLocalPoints(Frame& frame, const std::vector<KF>& localKeyFrames, std::vector<MP>& localMapPoints) {
  localMapPoints.clear();
  for (const KF& kf : localKeyFrames) {
    const std::vector<MP> mps = kf->getMapPointMatches();
    for (const MP& mp : mps) {
      if (!mp) continue;
      if (mp->m_int_trackReferenceForFrameID == frame.m_int_ID) continue;
      if (!mp->isBad()) { localMapPoints.push_back(mp); mp->m_int_trackReferenceForFrameID = frame.m_int_ID; }
    }
  }
}

struct Scene {
  std::vector<KF> kfs;
  std::vector<MP> mps;
  std::vector<std::vector<int>> frames;   // per test frame: point ids, -1 = no map point
};
static long unsigned int g_frameId = 100;

static KF makeKeyFrame(Scene& S, int id, int centrePoint, int nEntries) {
  KF kf = std::make_shared<KeyFrame>();
  kf->m_int_keyFrameID = (long unsigned int)id;
  kf->centre = cv::Mat(3, 1, CV_32F);
  for (int r = 0; r < 3; r++) kf->centre.at<float>(r) = 0.25f * (float)(id + r);
  kf->m_v_keyPoints.resize((size_t)nEntries); kf->m_v_rightXcords.assign((size_t)nEntries, -1.f); kf->m_v_depth.assign((size_t)nEntries, 1.f);
  kf->m_v_scaleFactors = {1.f, 1.2f};
  kf->mapPoints.resize((size_t)nEntries);
  for (int i = 0; i < nEntries; i++) {
    kf->m_v_keyPoints[(size_t)i].octave = i % 2;
    if (rnd(5) == 0) continue;
    const MP& mp = S.mps[(size_t)((centrePoint + rnd(360)) % (int)S.mps.size())];
    if (mp->observations.count(kf)) continue;   // a keyframe holds a point once
    kf->mapPoints[(size_t)i] = mp;
    mp->observations[kf] = (size_t)i;
    if (!mp->ref) mp->ref = kf;
  }
  return kf;
}

static std::vector<int> frameAround(const Scene& S, int firstKf, int lastKf, int n) {
  std::vector<int> f;
  const int lo = firstKf * 28, span = (lastKf - firstKf) * 28 + 360;
  for (int i = 0; i < n; i++) f.push_back(rnd(6) == 0 ? -1 : (lo + rnd(span)) % (int)S.mps.size());
  return f;
}

static std::vector<int> kfIds(const std::vector<KF>& v) { std::vector<int> o; for (const KF& k : v) o.push_back((int)k->m_int_keyFrameID); return o; }
static std::vector<int> mpIds(const std::vector<MP>& v) { std::vector<int> o; for (const MP& m : v) o.push_back(m->id); return o; }

// every test frame both ways, exactly
static void compare(const char* tag, Scene& S, Mirror& mirror) {
  int sameKfs = 1, sameRef = 1, samePoints = 1, sameSeen = 1, sameNulled = 1, stopped80 = 0, totalKfs = 0, totalPoints = 0, nulled = 0, seenCount = 0;
  for (const std::vector<int>& ids : S.frames) {
    Frame fa, fb;
    for (int p : ids) { fa.m_v_sptrMapPoints.push_back(p < 0 ? MP() : S.mps[(size_t)p]); fb.m_v_sptrMapPoints.push_back(p < 0 ? MP() : S.mps[(size_t)p]); }
    std::vector<KF> ka, kb;
    std::vector<MP> pa, pb;
    KF ra, rb;
    fa.m_int_ID = ++g_frameId;
    refUpdateLocalKeyFrames(fa, ka, ra);
    refUpdateLocalPoints(fa, ka, pa);
    std::vector<uint8_t> seenA;   // searchLocalPoints: the frame's own matches carry m_int_lastSeenInFrameID
    { std::set<MP> own; for (const MP& m : fa.m_v_sptrMapPoints) if (m) own.insert(m); for (const MP& m : pa) seenA.push_back(own.count(m) ? 1 : 0); }
    fb.m_int_ID = ++g_frameId;
    ya::updateLocalKeyFramesImpl(mirror, fb, kb, rb);
    const std::vector<uint8_t> seenB = ya::updateLocalPointsImpl(mirror, fb, kb, pb);
    sameKfs = sameKfs && kfIds(ka) == kfIds(kb) && ka == kb;
    sameRef = sameRef && ra == rb && fa.m_sptr_referenceKeyFrame == fb.m_sptr_referenceKeyFrame;
    samePoints = samePoints && pa == pb && mpIds(pa) == mpIds(pb);
    sameSeen = sameSeen && seenA == seenB;
    sameNulled = sameNulled && fa.m_v_sptrMapPoints == fb.m_v_sptrMapPoints;
    for (size_t i = 0; i < ids.size(); i++) nulled += ids[i] >= 0 && !fb.m_v_sptrMapPoints[i];
    stopped80 += kb.size() > 80;
    totalKfs += (int)kb.size(); totalPoints += (int)pb.size();
    for (uint8_t s : seenB) seenCount += s;
  }
  printf("%s_local_keyframes_same %d\n%s_reference_keyframe_same %d\n%s_local_points_same %d\n%s_seen_same %d\n%s_nulled_same %d\n", tag, sameKfs, tag, sameRef,
         tag, samePoints, tag, sameSeen, tag, sameNulled);
  printf("%s_frames_past_80 %d\n%s_local_keyframes %d\n%s_local_points %d\n%s_nulled %d\n%s_seen %d\n", tag, stopped80, tag, totalKfs, tag, totalPoints, tag, nulled,
         tag, seenCount);
  const std::vector<int32_t> rows = mirror.verifyRows();
  const Mirror::Difference d = mirror.verify();
  printf("%s_verify_rows_differences %d\n%s_verify_differences %d\n", tag, (int)rows.size(), tag, (int)(d.pointSlots.size() + d.keyFrameSlots.size()));
}

static void eraseMatch(Mirror& mirror, const KF& kf, size_t idx) {   // eraseMapPointMatch + eraseObservation, with their touches
  const MP mp = kf->mapPoints[idx];
  if (!mp) return;
  kf->mapPoints[idx] = MP();
  mp->observations.erase(kf);
  if (mp->ref == kf && !mp->observations.empty()) mp->ref = mp->observations.begin()->first;
  mirror.touch(mp); mirror.touchEntry(kf, idx);
}
static bool addMatch(Mirror& mirror, const KF& kf, size_t idx, const MP& mp) {   // addMapPoint + addObservation
  if (kf->mapPoints[idx] || mp->observations.count(kf)) return false;
  kf->mapPoints[idx] = mp;
  mp->observations[kf] = idx;
  mirror.touch(mp); mirror.touchEntry(kf, idx);
  return true;
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
static std::vector<Frame> makeFrames(const Scene& S) {
  std::vector<Frame> out;
  for (const std::vector<int>& ids : S.frames) {
    Frame f;
    for (int p : ids) f.m_v_sptrMapPoints.push_back(p < 0 ? MP() : S.mps[(size_t)p]);
    f.m_int_ID = ++g_frameId;
    out.push_back(f);
  }
  return out;
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 0;
  Scene S;
  const int nKf = 140, nPts = 4000;
  S.mps.resize((size_t)nPts);
  for (int p = 0; p < nPts; p++) {
    S.mps[(size_t)p] = std::make_shared<MapPoint>();
    S.mps[(size_t)p]->id = p;
    S.mps[(size_t)p]->pos = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) S.mps[(size_t)p]->pos.at<float>(r) = 0.125f * (float)(p % 97 + r);
  }
  S.kfs.resize((size_t)nKf);
  {   // allocation order differs from id order, so that the pointer-ordered containers do not iterate by id
    std::vector<int> order;
    for (int k = nKf - 1; k >= 0; k--) if (k % 2 == 1) order.push_back(k);
    for (int k = 0; k < nKf; k++) if (k % 2 == 0) order.push_back(k);
    for (int k : order) S.kfs[(size_t)k] = makeKeyFrame(S, k, k * 28, 140 + k % 31);
  }
  for (int k = 0; k < nKf; k++) {   // covisibility lists k+-1 .. k+-5, a chain as spanning tree; keyframe 60 hangs under keyframe 5
    for (int d = 1; d <= 5; d++) for (int s : {-1, 1}) if (k + s * d >= 0 && k + s * d < nKf) S.kfs[(size_t)k]->covisible.push_back(S.kfs[(size_t)(k + s * d)]);
    const int parent = k == 60 ? 5 : k - 1;
    if (parent >= 0) { S.kfs[(size_t)k]->parent = S.kfs[(size_t)parent]; S.kfs[(size_t)parent]->children.insert(S.kfs[(size_t)k]); }
  }
  for (int p = 0; p < nPts; p++) {
    if (!S.mps[(size_t)p]->ref) S.mps[(size_t)p]->ref = S.kfs[0];
    if (p % 37 == 11) S.mps[(size_t)p]->bad = true;
  }
  for (int k : {20, 23, 27}) S.kfs[(size_t)k]->bad = true;
  S.frames.push_back(frameAround(S, 55, 66, 500));    // the expansion reaches keyframe 60, whose parent is far away: the parent break
  S.frames.push_back(frameAround(S, 30, 125, 900));   // the counter alone holds more than 80 keyframes
  S.frames.push_back(frameAround(S, 70, 132, 700));   // passes 80 inside the expansion
  S.frames.push_back(frameAround(S, 17, 30, 400));    // bad keyframes in the counter and among the neighbours
  S.frames.push_back(std::vector<int>(50, -1));       // no map point at all: both leave the local map as it was

  Mirror mirror(0, 256, 16, 2048);   // small on purpose: every table grows while the scene is loaded
  for (const KF& k : S.kfs) { mirror.touch(k); mirror.touchRow(k); }
  for (const MP& m : S.mps) mirror.touch(m);
  compare("A", S, mirror);

  if (reps > 0) {   // updateLocalMap's two halves over every frame, both ways, alternating; the frames are built outside the clock
    std::vector<double> ta, tb;
    for (int r = 0; r < reps + 1; r++) {
      std::vector<Frame> fa = makeFrames(S), fb = makeFrames(S);
      std::vector<KF> ka, kb;
      std::vector<MP> pa, pb;
      KF ra, rb;
      const double a = once([&] { for (Frame& f : fa) { refUpdateLocalKeyFrames(f, ka, ra); refUpdateLocalPoints(f, ka, pa); } });
      const double b = once([&] { for (Frame& f : fb) { ya::updateLocalKeyFramesImpl(mirror, f, kb, rb); ya::updateLocalPointsImpl(mirror, f, kb, pb); } });
      if (r) { ta.push_back(a); tb.push_back(b); }
    }
    report("reference_loops_update_local_map", ta);
    report("mirror_update_local_map", tb);
  }

  // ---- mutations, each with its touches
  int added = 0, erased = 0, replaced = 0;
  for (int k = 56; k < 64; k++) {
    const KF& kf = S.kfs[(size_t)k];
    for (size_t i = 0; i < kf->mapPoints.size() && erased < 60; i += 9) if (kf->mapPoints[i]) { eraseMatch(mirror, kf, i); erased++; }
    for (size_t i = 1; i < kf->mapPoints.size() && added < 60; i += 7) added += addMatch(mirror, kf, i, S.mps[(size_t)((k * 28 + 400 + (int)i) % nPts)]) ? 1 : 0;
    for (size_t i = 2; i < kf->mapPoints.size() && replaced < 40; i += 13) {   // replaceMapPointMatch
      const MP other = S.mps[(size_t)((k * 28 + 900 + (int)i) % nPts)];
      if (!kf->mapPoints[i] || other->observations.count(kf)) continue;
      eraseMatch(mirror, kf, i);
      replaced += addMatch(mirror, kf, i, other) ? 1 : 0;
    }
  }
  for (int p = 1600; p < 1700; p += 9) { S.mps[(size_t)p]->bad = true; mirror.touch(S.mps[(size_t)p]); }   // setBadFlag of points
  {   // keyframe creation
    const KF fresh = makeKeyFrame(S, nKf, 61 * 28, 150);
    fresh->covisible = S.kfs[61]->covisible; fresh->parent = S.kfs[61]; S.kfs[61]->children.insert(fresh);
    S.kfs[62]->covisible.insert(S.kfs[62]->covisible.begin(), fresh);
    S.kfs.push_back(fresh);
    mirror.touch(fresh); mirror.touchRow(fresh);
    for (const MP& mp : fresh->mapPoints) if (mp) mirror.touch(mp);
  }
  printf("mutations_added %d\nmutations_erased %d\nmutations_replaced %d\n", added, erased, replaced);
  compare("B", S, mirror);

  {   // a keyframe leaves the map (setBadFlag -> forget) and a new one takes its slot
    const KF gone = S.kfs[58];
    const int32_t slot = mirror.slotOf(gone);
    for (size_t i = 0; i < gone->mapPoints.size(); i++) eraseMatch(mirror, gone, i);
    gone->bad = true;
    if (gone->parent) gone->parent->children.erase(gone);
    mirror.forget(gone);
    const KF fresh = makeKeyFrame(S, nKf + 1, 59 * 28, 133);
    fresh->covisible = S.kfs[59]->covisible; fresh->parent = S.kfs[59]; S.kfs[59]->children.insert(fresh);
    S.kfs[57]->covisible.insert(S.kfs[57]->covisible.begin(), fresh);
    S.kfs.push_back(fresh);
    mirror.touch(fresh); mirror.touchRow(fresh);
    for (const MP& mp : fresh->mapPoints) if (mp) mirror.touch(mp);
    printf("slot_reused %d\n", (int)(mirror.slotOf(fresh) == slot && mirror.slotOf(gone) == -1));
  }
  compare("C", S, mirror);

  {   // one mutation without its row touch: verifyRows() names exactly that keyframe, nothing fails
    const KF kf = S.kfs[61];
    size_t idx = 0;
    while (!kf->mapPoints[idx] || kf->mapPoints[idx]->bad) idx++;
    const MP mp = kf->mapPoints[idx];
    kf->mapPoints[idx] = MP();
    mp->observations.erase(kf);
    if (mp->ref == kf && !mp->observations.empty()) mp->ref = mp->observations.begin()->first;
    mirror.touch(mp);                                  // the point's side is told, the row is not
    const std::vector<int32_t> rows = mirror.verifyRows();
    printf("missed_touch_slot %d\nverify_rows_named %d\nverify_rows_named_slot %d\n", (int)mirror.slotOf(kf), (int)rows.size(), rows.empty() ? -1 : (int)rows[0]);
    mirror.touchEntry(kf, idx);
    printf("verify_rows_after_the_touch %d\n", (int)mirror.verifyRows().size());
  }
  compare("D", S, mirror);
  YdMapDbRowStats rs;
  ydorb_mapdb_row_stats(mirror.handle(), &rs);
  printf("row_stats_header_growths %d\nrow_stats_repacks %d\n", rs.header_growths, rs.repacks_kept + rs.repacks_grown);
  return 0;
}
