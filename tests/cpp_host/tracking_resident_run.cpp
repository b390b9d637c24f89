// TEST-ONLY: EXECUTES the resident form of Tracking::searchLocalPoints on the GPU - updateLocalPointsImpl and then
// searchLocalPointsImpl(Mirror&, ...) of include/ydorb/tracking.hpp over a MapMirror with enableAttributes() (include/ydorb/mapMirror.hpp)
// - beside the flat searchLocalPointsImpl on a second copy of the same scene, with stand-ins of Frame / KeyFrame / MapPoint that carry
// real data.  It reads the scenario of tests/cpp_host/tracking_run.cpp (tests/test_tracking_resident_adapter_gpu.py writes it), gives the
// resident copy six keyframes whose map-point vectors list the local points in order and observe those the scenario calls observed,
// and compares exactly: the frame's map-point vector, every point's track members, visibility counter and last-seen frame, the
// return value; then a forget() whose slot is taken again by a point without a descriptor.  It prints one line per figure, "<name> <value>".  OpenCV is the functional mock of tests/cpu_harness/mockrt.
//   tracking_resident_run scenario.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "ydorb/mapMirror.hpp"
#include "ydorb/tracking.hpp"

namespace {

struct Reader {
  FILE* f;
  explicit Reader(const char* path) : f(fopen(path, "rb")) { if (!f) { perror(path); exit(2); } }
  ~Reader() { fclose(f); }
  template <class T> T get() { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "scenario truncated\n"); exit(2); } return v; }
  template <class T> void get(T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scenario truncated\n"); exit(2); } }
};

cv::Mat readMat32(Reader& R, int rows, int cols) { cv::Mat m(rows, cols, CV_32F); R.get(m.ptr<float>(), (size_t)rows * cols); return m; }

struct KeyFrame;
struct MapPoint {
  int index = -1;
  cv::Mat pos, normal, desc;
  float minDist = 0, maxDist = 0;      // m_flt_minDistance / m_flt_maxDistance
  bool bad = false;
  int nObs = 0, visible = 0;
  std::shared_ptr<KeyFrame> ref;
  std::map<std::shared_ptr<KeyFrame>, size_t> observations;   // the resident copy only; the flat overload reads nObs
  long int m_int_lastSeenInFrameID = -1;
  long unsigned int m_int_trackReferenceForFrameID = 0;
  bool m_b_isTrackInView = false;
  int m_int_trackScaleLevel = -7;
  float m_flt_trackViewCos = -7.f, m_flt_trackProjX = -7.f, m_flt_trackProjY = -7.f, m_flt_trackProjRightX = -7.f;
  bool isBad() { return bad; }
  int getObservationsNum() { return nObs; }
  std::map<std::shared_ptr<KeyFrame>, size_t> getObservations() { return observations; }
  std::shared_ptr<KeyFrame> getReferenceKeyFrame() { return ref; }
  cv::Mat getDescriptor() { return desc.clone(); }
  cv::Mat getPosInWorld() { return pos.clone(); }
  cv::Mat getNormal() { return normal.clone(); }
  float getMinDistanceInvariance() { return 0.8f * minDist; }
  float getMaxDistanceInvariance() { return 1.2f * maxDist; }
  float getMinDistance() { return minDist; }
  float getMaxDistance() { return maxDist; }
  void increaseVisible(int n = 1) { visible += n; }
};
struct KeyFrame {
  long unsigned int m_int_keyFrameID = 0, m_int_trackReferenceForFrameID = 0;
  cv::Mat centre;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  std::vector<std::shared_ptr<MapPoint>> mapPoints;
  cv::Mat getCameraOriginInWorld() { return centre.clone(); }
  std::vector<std::shared_ptr<MapPoint>> getMapPointMatches() { return mapPoints; }
  std::vector<std::shared_ptr<KeyFrame>> getVectorCovisibleKeyFrames() { return std::vector<std::shared_ptr<KeyFrame>>(); }
  void setBadFlag() {}
  bool isBad() { return false; }
};
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
struct Frame {
  std::vector<cv::KeyPoint> m_v_keyPoints;
  cv::Mat m_cvMat_descriptors, m_cvMat_T_c2w, origin;
  std::vector<float> m_v_rightXcords, m_v_scaleFactors;
  std::vector<MP> m_v_sptrMapPoints;
  long int m_int_ID = 0;
  float m_flt_logScaleFactor = 0;
  cv::Mat getCameraOriginInWorld() { return origin.clone(); }
  static float m_flt_minX, m_flt_maxX, m_flt_minY, m_flt_maxY, m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLine, m_flt_baseLineTimesFx;
};
float Frame::m_flt_minX, Frame::m_flt_maxX, Frame::m_flt_minY, Frame::m_flt_maxY, Frame::m_flt_fx, Frame::m_flt_fy, Frame::m_flt_cx, Frame::m_flt_cy,
    Frame::m_flt_baseLine, Frame::m_flt_baseLineTimesFx;
typedef ydorb::adapter::MapMirror<KF, MP> Mirror;

struct World {   // one copy of the scene: the flat and the resident run must not see each other's writes
  Frame frame;
  std::vector<MP> all, local;
};

bool sameTrack(const MapPoint& a, const MapPoint& b) {
  return memcmp(&a.m_flt_trackProjX, &b.m_flt_trackProjX, 4) == 0 && memcmp(&a.m_flt_trackProjY, &b.m_flt_trackProjY, 4) == 0 &&
         memcmp(&a.m_flt_trackProjRightX, &b.m_flt_trackProjRightX, 4) == 0 && memcmp(&a.m_flt_trackViewCos, &b.m_flt_trackViewCos, 4) == 0 &&
         a.m_int_trackScaleLevel == b.m_int_trackScaleLevel && a.m_b_isTrackInView == b.m_b_isTrackInView;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: tracking_resident_run scenario.bin\n"); return 2; }
  Reader R(argv[1]);
  float cam[9];
  R.get(cam, 9);
  Frame::m_flt_fx = cam[0]; Frame::m_flt_fy = cam[1]; Frame::m_flt_cx = cam[2]; Frame::m_flt_cy = cam[3]; Frame::m_flt_baseLineTimesFx = cam[4];
  Frame::m_flt_minX = cam[5]; Frame::m_flt_maxX = cam[6]; Frame::m_flt_minY = cam[7]; Frame::m_flt_maxY = cam[8];
  Frame::m_flt_baseLine = 0.f;
  World A;
  Frame& frame = A.frame;
  const int nLevels = R.get<int32_t>();
  frame.m_v_scaleFactors.resize(nLevels);
  R.get(frame.m_v_scaleFactors.data(), nLevels);
  frame.m_flt_logScaleFactor = R.get<float>();
  frame.m_int_ID = R.get<int32_t>();
  const float th = R.get<float>(), ratio = R.get<float>();
  frame.m_cvMat_T_c2w = readMat32(R, 4, 4);
  frame.origin = readMat32(R, 3, 1);
  const int n = R.get<int32_t>();
  frame.m_v_keyPoints.resize(n);
  R.get(reinterpret_cast<unsigned char*>(frame.m_v_keyPoints.data()), (size_t)n * sizeof(cv::KeyPoint));
  frame.m_cvMat_descriptors.create(std::max(n, 1), 32, CV_8U);
  R.get(frame.m_cvMat_descriptors.data, (size_t)n * 32);
  frame.m_v_rightXcords.resize(n);
  R.get(frame.m_v_rightXcords.data(), n);
  const int nAll = R.get<int32_t>();
  for (int i = 0; i < nAll; i++) {
    auto mp = std::make_shared<MapPoint>();
    mp->index = i;
    mp->pos = readMat32(R, 3, 1); mp->normal = readMat32(R, 3, 1);
    mp->minDist = R.get<float>(); mp->maxDist = R.get<float>();
    mp->desc.create(1, 32, CV_8U);
    R.get(mp->desc.data, 32);
    const int32_t rec[4] = {R.get<int32_t>(), R.get<int32_t>(), R.get<int32_t>(), R.get<int32_t>()};
    mp->bad = rec[0] != 0; mp->nObs = rec[1]; mp->m_int_lastSeenInFrameID = rec[2]; mp->visible = rec[3];
    A.all.push_back(mp);
  }
  std::vector<int32_t> slot(n);
  R.get(slot.data(), n);
  frame.m_v_sptrMapPoints.resize(n);
  for (int i = 0; i < n; i++) if (slot[i] >= 0) frame.m_v_sptrMapPoints[i] = A.all[slot[i]];
  const int nLocal = R.get<int32_t>();
  std::vector<int32_t> localIdx(nLocal);
  R.get(localIdx.data(), nLocal);
  for (int i : localIdx) A.local.push_back(A.all[i]);

  World B;   // a deep copy of the points; the frame's matrices are only read
  B.frame = A.frame;
  for (const MP& mp : A.all) B.all.push_back(std::make_shared<MapPoint>(*mp));
  for (int i = 0; i < n; i++) B.frame.m_v_sptrMapPoints[i] = slot[i] >= 0 ? B.all[slot[i]] : MP();

  namespace ya = ydorb::adapter;
  const int matchesFlat = ya::searchLocalPointsImpl(ya::matcher(), A.frame, A.local, th, ratio);

  // the resident copy: six keyframes list the local points in order; a point the scenario calls observed is observed by its keyframe
  const int nKf = 6;
  std::vector<KF> kfs;
  for (int k = 0; k < nKf; k++) {
    KF kf = std::make_shared<KeyFrame>();
    kf->m_int_keyFrameID = (long unsigned int)k;
    kf->centre = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) kf->centre.at<float>(r) = 0.1f * (float)(k + r);
    kf->m_v_scaleFactors = frame.m_v_scaleFactors;
    kfs.push_back(kf);
  }
  const int per = (nLocal + nKf - 1) / nKf;
  for (int i = 0; i < nLocal; i++) {
    const MP& mp = B.all[localIdx[i]];
    KeyFrame& kf = *kfs[i / per];
    mp->ref = kfs[i / per];
    if (mp->nObs > 0) mp->observations[kfs[i / per]] = kf.mapPoints.size();
    kf.mapPoints.push_back(mp);
    kf.m_v_keyPoints.push_back(cv::KeyPoint());
    kf.m_v_rightXcords.push_back(-1.f);
  }
  for (const MP& mp : B.all) if (!mp->ref) mp->ref = kfs[0];

  Mirror mirror(0, 64, 4, 256);   // small: the point table grows while the scene is loaded
  mirror.enableAttributes();
  for (const KF& kf : kfs) { mirror.touch(kf); mirror.touchRow(kf); }
  for (const MP& mp : B.all) { mirror.touch(mp); mirror.touchAttributes(mp); }
  mirror.flush();
  const Mirror::Difference diff = mirror.verify();
  printf("verify_differences %d\n", (int)(diff.pointSlots.size() + diff.keyFrameSlots.size()));
  printf("verify_attributes_differences %d\n", (int)mirror.verifyAttributes().size());

  std::vector<MP> localB;
  const std::vector<uint8_t> seen = ya::updateLocalPointsImpl(mirror, B.frame, kfs, localB);
  int nSeen = 0;
  for (const uint8_t s : seen) nSeen += s;
  int nLive = 0;
  for (const MP& mp : A.local) nLive += !mp->bad;
  bool sameOrder = (int)localB.size() == nLive;
  for (size_t i = 0, j = 0; sameOrder && i < A.local.size(); i++) {
    if (A.local[i]->bad) continue;
    sameOrder = localB[j++]->index == A.local[i]->index;
  }
  printf("local_points %d\nlocal_points_in_order %d\nseen %d\n", (int)localB.size(), sameOrder ? 1 : 0, nSeen);
  const int matchesResident = ya::searchLocalPointsImpl(mirror, ya::matcher(), B.frame, localB, th, ratio, &seen);

  int sameSlots = 1, sameTracks = 1, sameCounts = 1, inView = 0;
  for (int i = 0; i < n; i++) {
    const int a = A.frame.m_v_sptrMapPoints[i] ? A.frame.m_v_sptrMapPoints[i]->index : -1, b = B.frame.m_v_sptrMapPoints[i] ? B.frame.m_v_sptrMapPoints[i]->index : -1;
    if (a != b) sameSlots = 0;
  }
  for (int i = 0; i < nAll; i++) {
    if (!sameTrack(*A.all[i], *B.all[i])) sameTracks = 0;
    if (A.all[i]->visible != B.all[i]->visible || A.all[i]->m_int_lastSeenInFrameID != B.all[i]->m_int_lastSeenInFrameID) sameCounts = 0;
    inView += B.all[i]->m_b_isTrackInView ? 1 : 0;
  }
  YdMapDbAttrStats as;
  YdMapDbStats st;
  ydorb_mapdb_attr_stats(mirror.handle(), &as);
  ydorb_mapdb_stats(mirror.handle(), &st);
  printf("matches_flat %d\nmatches_resident %d\nframe_map_points_same %d\ntrack_members_same %d\nvisible_and_last_seen_same %d\nin_view %d\n", matchesFlat,
         matchesResident, sameSlots, sameTracks, sameCounts, inView);
  printf("attr_growths %d\nattr_capacity_is_point_capacity %d\nlast_attr_sync_bytes %lld\nlast_sync_bytes %lld\n", as.growths, as.capacity == st.point_capacity ? 1 : 0,
         (long long)as.last_attr_sync_bytes, (long long)st.last_sync_bytes);

  // a host-side change without its touch is named by verifyAttributes, and mended by the touch
  const MP& changed = localB[3];
  changed->maxDist *= 2.f;
  const std::vector<int32_t> named = mirror.verifyAttributes();
  printf("verify_attributes_named %d\n", named.size() == 1 && named[0] == mirror.slotOf(changed) ? 1 : 0);
  mirror.touchAttributes(changed);
  printf("verify_attributes_after_the_touch %d\n", (int)mirror.verifyAttributes().size());

  // forget(), then the slot taken again before the next flush by a point made from a keyframe, whose descriptor is still unset (an
  // empty matrix): the slot reads as "no attributes", the touch stages the geometry alone, the search answers status 7 until the
  // descriptor is set and touched
  MP gone;
  for (const MP& mp : localB) if (mp->m_b_isTrackInView && mp != changed) { gone = mp; break; }
  const int32_t freed = mirror.slotOf(gone);
  for (const KF& kf : kfs)
    for (size_t i = 0; i < kf->mapPoints.size(); i++)
      if (kf->mapPoints[i] == gone) { kf->mapPoints[i].reset(); mirror.touchEntry(kf, i); }
  mirror.forget(gone);
  MP fresh = std::make_shared<MapPoint>(*gone);
  fresh->index = nAll; fresh->desc = cv::Mat(); fresh->observations.clear(); fresh->nObs = 0;
  mirror.touch(fresh);
  const auto flagsOf = [&](int32_t s) {
    mirror.flush();
    YdMapDbStats now;
    ydorb_mapdb_stats(mirror.handle(), &now);
    const size_t np = (size_t)now.n_points;
    std::vector<float> nrm(3 * np), mn(np), mx(np);
    std::vector<uint8_t> d(32 * np), fl(np);
    if (ydorb_mapdb_export_attributes(mirror.handle(), nrm.data(), mn.data(), mx.data(), d.data(), fl.data()) != YDORB_OK) return -1;
    return (int)fl[(size_t)s];
  };
  const auto statusOf = [&](const MP& mp) {
    const YdFrameView fv = ya::frameView(B.frame);
    const YdFrustumView view = ya::frustumView(B.frame, 0.5f);
    std::vector<uint8_t> taken, status;
    ya::takenMask(B.frame, false, taken);
    std::vector<int32_t> assigned(taken.size(), -1);
    std::vector<YdTrackView> rows;
    int32_t nToMatch = 0;
    mirror.searchLocalPoints(ya::matcher(), fv, view, std::vector<MP>(1, mp), std::vector<uint8_t>(1, 0), th, ratio, taken, assigned, rows, status, nToMatch);
    return (int)status[0];
  };
  printf("slot_reused %d\n", mirror.slotOf(fresh) == freed ? 1 : 0);
  printf("reused_slot_flags_before_a_touch %d\n", flagsOf(freed));
  printf("reused_slot_status_before_a_touch %d\n", statusOf(fresh));
  mirror.touchAttributes(fresh);
  printf("reused_slot_flags_with_an_empty_descriptor %d\n", flagsOf(freed));
  printf("reused_slot_status_with_an_empty_descriptor %d\n", statusOf(fresh));
  const std::vector<int32_t> lacking = mirror.verifyAttributes();
  printf("verify_attributes_names_the_missing_group %d\n", lacking.size() == 1 && lacking[0] == freed ? 1 : 0);
  fresh->desc = gone->desc.clone();
  mirror.touchAttributes(fresh);
  printf("reused_slot_flags_after_the_descriptor %d\n", flagsOf(freed));
  printf("reused_slot_status_after_the_descriptor %d\n", statusOf(fresh));
  printf("verify_attributes_at_the_end %d\n", (int)mirror.verifyAttributes().size());
  return 0;
}
