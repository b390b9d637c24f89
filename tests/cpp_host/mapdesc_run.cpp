// TEST-ONLY: executes the resident-descriptor methods of ydorb::adapter::MapMirror (include/ydorb/mapMirror.hpp) on stand-ins of
// KeyFrame / MapPoint in one program, linked against libydorb.so:
//   mapdesc_run
// The scene is seeded here: 30 keyframes of 64 keypoints whose descriptors are four base rows with a few flipped bits (equal medians
// are common), 300 map points seen by 0 .. 8 keyframes.  The stand-in MapPoint carries the reference's own sequential
// computeDistinctiveDescriptors (restated from ORB-SLAM2: a bad point returns, observations of bad keyframes are skipped, the median
// is v[(int)(0.5 m)] of the sorted distance row, the first least median wins).  The program runs the mirror with descriptors enabled
// through four steps - everything touched; one keyframe inserted; a fuse that replaces points; a keyframe culled and one merely set
// bad - and after each compares, for every touched point, what the mirror's apply received with what the sequential function leaves
// in m_descriptor, and calls verifyDescriptors().  It prints one line per figure, "<name> <value>"; tests/test_mapdesc_adapter_gpu.py
// reads them.  Every comparison is exact.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include <opencv2/core.hpp>

#include "ydorb/mapMirror.hpp"

struct KeyFrame;
struct MapPoint;
typedef std::shared_ptr<KeyFrame> KF;
struct KeyFrame {
  long unsigned int m_int_keyFrameID = 0;
  bool bad = false;
  cv::Mat centre, m_cvMat_descriptors;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  std::vector<std::shared_ptr<MapPoint>> mapPoints;
  cv::Mat getCameraOriginInWorld() { return centre.clone(); }
  std::vector<std::shared_ptr<MapPoint>> getMapPointMatches() { return mapPoints; }
  std::vector<KF> getVectorCovisibleKeyFrames() { return std::vector<KF>(); }
  void setBadFlag() { bad = true; }
  bool isBad() { return bad; }
};
struct MapPoint {
  int id = 0;
  bool bad = false;
  cv::Mat pos, m_descriptor;
  KF ref;
  std::map<KF, size_t> observations;
  bool isBad() { return bad; }
  std::map<KF, size_t> getObservations() { return observations; }
  cv::Mat getPosInWorld() { return pos.clone(); }
  KF getReferenceKeyFrame() { return ref; }
  // the reference's member function; returns whether m_descriptor was written
  bool computeDistinctiveDescriptors() {
    if (bad) return false;
    std::vector<cv::Mat> rows;
    for (const auto& ob : observations)
      if (!ob.first->isBad()) rows.push_back(ob.first->m_cvMat_descriptors.row((int)ob.second));
    if (rows.empty()) return false;
    const size_t m = rows.size();
    std::vector<std::vector<int>> dist(m, std::vector<int>(m, 0));
    for (size_t i = 0; i < m; i++)
      for (size_t j = i + 1; j < m; j++) {
        int d = 0;
        for (int b = 0; b < 32; b++) d += __builtin_popcount((unsigned)(rows[i].ptr<unsigned char>()[b] ^ rows[j].ptr<unsigned char>()[b]));
        dist[i][j] = dist[j][i] = d;
      }
    int bestMedian = INT32_MAX;
    size_t bestIdx = 0;
    for (size_t i = 0; i < m; i++) {
      std::vector<int> v(dist[i]);
      std::sort(v.begin(), v.end());
      const int median = v[(size_t)(0.5 * (double)m)];
      if (median < bestMedian) { bestMedian = median; bestIdx = i; }
    }
    m_descriptor = rows[bestIdx].clone();
    return true;
  }
};
typedef std::shared_ptr<MapPoint> MP;
typedef ydorb::adapter::MapMirror<KF, MP> Mirror;

static std::mt19937 g_rng(20240917);
static int uni(int lo, int hi) { return lo + (int)(g_rng() % (uint32_t)(hi - lo + 1)); }
static unsigned char g_base[4][32];

static KF makeKeyFrame(int id, int nKeyPoints) {
  KF k = std::make_shared<KeyFrame>();
  k->m_int_keyFrameID = (long unsigned int)id;
  k->centre = cv::Mat(3, 1, CV_32F);
  for (int r = 0; r < 3; r++) k->centre.at<float>(r) = 0.25f * (float)uni(-16, 16);
  k->m_cvMat_descriptors = cv::Mat(nKeyPoints, 32, CV_8U);
  for (int i = 0; i < nKeyPoints; i++) {
    unsigned char* row = k->m_cvMat_descriptors.ptr<unsigned char>(i);
    memcpy(row, g_base[uni(0, 3)], 32);
    for (int f = uni(0, 2); f > 0; f--) row[uni(0, 31)] ^= (unsigned char)(1 << uni(0, 7));
  }
  k->m_v_keyPoints.resize((size_t)nKeyPoints);
  for (cv::KeyPoint& kp : k->m_v_keyPoints) { kp = cv::KeyPoint(); kp.octave = uni(0, 7); }
  k->m_v_rightXcords.assign((size_t)nKeyPoints, -1.f);
  k->m_v_depth.assign((size_t)nKeyPoints, 1.f);
  k->m_v_scaleFactors.assign(8, 1.f);
  k->mapPoints.resize((size_t)nKeyPoints);
  return k;
}
static MP makePoint(int id) {
  MP p = std::make_shared<MapPoint>();
  p->id = id;
  p->pos = cv::Mat(3, 1, CV_32F);
  for (int r = 0; r < 3; r++) p->pos.at<float>(r) = 0.125f * (float)uni(-40, 40);
  return p;
}
static bool observe(const MP& p, const KF& k) {   // at a free keypoint; several points may share a keyframe, none a keypoint
  if (p->observations.count(k)) return false;
  std::vector<size_t> free;
  for (size_t i = 0; i < k->mapPoints.size(); i++) if (!k->mapPoints[i]) free.push_back(i);
  if (free.empty()) return false;
  const size_t i = free[(size_t)uni(0, (int)free.size() - 1)];
  k->mapPoints[i] = p; p->observations[k] = i;
  if (!p->ref) p->ref = k;
  return true;
}
static void unobserve(const MP& p, const KF& k) {
  const auto it = p->observations.find(k);
  if (it == p->observations.end()) return;
  k->mapPoints[it->second] = MP();
  p->observations.erase(it);
  if (p->ref == k && !p->observations.empty()) p->ref = p->observations.begin()->first;
}

// For the touched points: the mirror's batch against the sequential member function, then verifyDescriptors()
static void compare(const char* tag, Mirror& mirror, const std::vector<MP>& touched) {
  std::map<int, std::vector<unsigned char>> applied;
  int viewsAgree = 1;
  const int n = mirror.computeDistinctiveDescriptors(touched, [&](const MP& p, const KF& k, size_t idx, const cv::Mat& row) {
    applied[p->id].assign(row.ptr<unsigned char>(), row.ptr<unsigned char>() + 32);
    const auto it = p->observations.find(k);   // the view the winner came from is one of the point's own
    viewsAgree = viewsAgree && it != p->observations.end() && it->second == idx && !memcmp(k->m_cvMat_descriptors.ptr<unsigned char>((int)idx), row.ptr<unsigned char>(), 32);
  });
  int same = 1, updated = 0;
  std::set<int> seen;
  for (const MP& p : touched) {
    if (!p || !seen.insert(p->id).second) continue;
    const bool wrote = p->computeDistinctiveDescriptors();
    updated += wrote ? 1 : 0;
    const auto it = applied.find(p->id);
    same = same && wrote == (it != applied.end()) && (!wrote || !memcmp(it->second.data(), p->m_descriptor.ptr<unsigned char>(), 32));
  }
  const Mirror::Difference d = mirror.verifyDescriptors();
  const Mirror::Difference t = mirror.verify();
  printf("%s_same %d\n%s_updated %d\n%s_applied %d\n%s_views_agree %d\n%s_verify_differences %d\n", tag, same, tag, updated, tag, n, tag, viewsAgree, tag,
         (int)(d.pointSlots.size() + d.keyFrameSlots.size() + t.pointSlots.size() + t.keyFrameSlots.size()));
}

int main() {
  for (auto& row : g_base) for (unsigned char& b : row) b = (unsigned char)g_rng();
  std::vector<KF> kfs;
  std::vector<MP> mps;
  for (int k = 0; k < 30; k++) kfs.push_back(makeKeyFrame(k, 64));
  for (int p = 0; p < 300; p++) {
    mps.push_back(makePoint(p));
    for (int o = uni(0, 8); o > 0; o--) observe(mps.back(), kfs[(size_t)uni(0, 29)]);
    if (!mps.back()->ref) mps.back()->ref = kfs[0];
    if (p % 37 == 5) mps.back()->bad = true;
  }

  Mirror mirror(0, 64, 4, 256);   // small on purpose: every table grows while the scene is loaded
  mirror.enableDescriptors(64, 64);
  for (const KF& k : kfs) { mirror.touch(k); mirror.touchDescriptors(k); }
  for (const MP& p : mps) mirror.touch(p);
  compare("A", mirror, mps);

  {   // processNewKeyFrame: a keyframe enters, points it matched gain an observation, new points are made in it
    const KF k = makeKeyFrame(30, 64);
    kfs.push_back(k);
    std::vector<MP> touched;
    for (int j = 0; j < 6; j++) { const MP p = mps[(size_t)uni(0, 299)]; if (!p->bad && observe(p, k)) { mirror.touch(p); touched.push_back(p); } }
    for (int j = 0; j < 5; j++) {
      const MP p = makePoint((int)mps.size());
      mps.push_back(p);
      observe(p, k); observe(p, kfs[(size_t)uni(0, 29)]);
      mirror.touch(p); touched.push_back(p);
    }
    mirror.touch(k); mirror.touchDescriptors(k);
    printf("B_touched %d\n", (int)touched.size());
    compare("B", mirror, touched);
  }

  {   // searchInNeighbors / searchAndFuse: point a is replaced by point b, which takes a's observations where it has none
    std::vector<MP> touched;
    int replaced = 0;
    for (int a = 1; a < 300 && replaced < 20; a += 7) {
      const MP pa = mps[(size_t)a], pb = mps[(size_t)a + 1];
      if (pa->bad || pb->bad || pa->observations.empty()) continue;
      for (const auto& ob : std::map<KF, size_t>(pa->observations)) {
        const size_t idx = ob.second;
        unobserve(pa, ob.first);
        if (!pb->observations.count(ob.first)) { ob.first->mapPoints[idx] = pb; pb->observations[ob.first] = idx; }
      }
      pa->bad = true;
      mirror.touch(pa); mirror.touch(pb);
      touched.push_back(pb); touched.push_back(pa);
      replaced++;
    }
    mirror.forget(mps[8]);   // one of the replaced points leaves the map altogether
    touched.erase(std::remove(touched.begin(), touched.end(), mps[8]), touched.end());
    printf("C_replaced %d\n", replaced);
    compare("C", mirror, touched);
  }

  {   // keyFrameCulling: keyframe 3 is erased from the map; keyframe 11 is only flagged bad and stays in the observations
    std::vector<MP> touched;
    const KF gone = kfs[3], flagged = kfs[11];
    for (const MP& p : std::vector<MP>(gone->mapPoints)) if (p) { unobserve(p, gone); mirror.touch(p); touched.push_back(p); }
    gone->setBadFlag();
    mirror.forget(gone);
    flagged->setBadFlag();
    mirror.touchDescriptors(flagged);
    for (const MP& p : flagged->mapPoints) if (p) touched.push_back(p);   // their views are unchanged: no touch
    printf("D_touched %d\n", (int)touched.size());
    compare("D", mirror, touched);
    compare("E", mirror, mps);   // and every point again
  }

  {   // a missed touch: a point loses an observation and the mirror is not told
    MP victim;
    for (size_t p = 100; p < 300 && !victim; p++) if (!mps[p]->bad && mps[p]->observations.size() >= 3) victim = mps[p];
    unobserve(victim, victim->observations.begin()->first);
    const Mirror::Difference d = mirror.verifyDescriptors();
    printf("missed_touch_slot %d\nverify_named %d\nverify_named_slot %d\n", (int)mirror.slotOf(victim), (int)(d.pointSlots.size() + d.keyFrameSlots.size()),
           d.pointSlots.empty() ? -1 : (int)d.pointSlots[0]);
    mirror.touch(victim);
    const Mirror::Difference after = mirror.verifyDescriptors();
    printf("verify_after_the_touch %d\n", (int)(after.pointSlots.size() + after.keyFrameSlots.size()));
  }
  YdMapDbDescStats ds;
  ydorb_mapdb_desc_stats(mirror.handle(), &ds);
  printf("stats_views %lld\nstats_descriptors %lld\nstats_repacks %d\n", (long long)ds.n_views, (long long)ds.n_descriptors,
         ds.view_repacks_kept + ds.view_repacks_grown + ds.desc_repacks_kept + ds.desc_repacks_grown);
  return 0;
}
