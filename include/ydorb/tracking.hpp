// Drop-in body of Tracking::searchLocalPoints (tracking.cpp:570-604; ORB-SLAM2 Tracking::SearchLocalPoints, which YDORBSLAM renames;
// SURVEY 3.2) and a batched Frame::isInCameraFrustum (frame.cpp:295-326) on top of the ydorb C ABI.  Function
// templates over the reference's own Frame / MapPoint types (included by the translation unit that instantiates them), so the member
// function becomes a forward ("Local map tracking"):
//   void Tracking::searchLocalPoints() {
//     float th = m_sensor == RGBD ? 3.f : 1.f;                                       // the caller keeps choosing th
//     if (m_frame_currentFrame.m_int_ID < m_int_lastRelocFrameID + 2) th = 5.f;
//     ydorb::adapter::searchLocalPointsImpl(ydorb::adapter::matcher(), m_frame_currentFrame, m_v_sptrLocalMapPoints, th, 0.8f);
//   }
// The first loop over the frame's own map points and the visibility counters stay on the host; the frustum test of every local map
// point, the query build and the projection search are ONE ydorb_search_local_points call.
//
// REQUIRED in the reference: a one-line getter on MapPoint,  float getMaxDistance() { lock; return m_flt_maxDistance; }  -
// predictScaleLevel divides the RAW maximum distance by the distance, and the reference only exposes 1.2f * it
// (getMaxDistanceInvariance).
// Assumed spellings, as in the other adapters: Frame m_cvMat_T_c2w (Rcw / tcw are its blocks, which is what updatePoseMatrices copies
// out of it), getCameraOriginInWorld(), m_int_ID, m_v_scaleFactors, m_flt_logScaleFactor, m_v_sptrMapPoints, the static m_flt_fx ..
// m_flt_cy, m_flt_baseLineTimesFx, m_flt_minX .. m_flt_maxY; MapPoint isBad(), increaseVisible(), m_int_lastSeenInFrameID,
// getPosInWorld(), getNormal(), getMinDistanceInvariance(), getMaxDistanceInvariance(), getDescriptor(), getObservationsNum(),
// m_b_isTrackInView, m_flt_trackProjX, m_flt_trackProjY, m_flt_trackProjRightX, m_int_trackScaleLevel, m_flt_trackViewCos.
#ifndef YDORB_ADAPTER_TRACKING_HPP
#define YDORB_ADAPTER_TRACKING_HPP

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core.hpp>

#include "c_api.h"
#include "orbMatcher.hpp"

namespace ydorb {
namespace adapter {

// MapPoint::predictScaleLevel's formula, ceil(log(ratio) / logScaleFactor) clamped to [0, nLevels - 1], with the clamp taken before the
// conversion to int (the same value wherever the reference's conversion is defined)
inline int predictScaleLevelFormula(float ratio, float logScaleFactor, int nLevels) {
  const float q = std::ceil(std::log(ratio) / logScaleFactor);
  if (!(q >= 0.0f)) return 0;
  if (q >= (float)nLevels) return nLevels - 1;
  return (int)q;
}

// YdFrustumView::level_ratio: out[k], k = 0 .. nLevels - 2, = the largest float ratio for which the formula gives <= k, found by
// bisection over the bit patterns of the positive floats with the very std::log(float) the reference calls.  The device then needs no
// log: the level is the number of entries strictly below the ratio (NaN -> 0, +inf -> nLevels - 1).
inline void levelRatioTable(float logScaleFactor, int nLevels, float* out) {
  auto value = [](uint32_t bits) { float f; std::memcpy(&f, &bits, 4); return f; };
  for (int k = 0; k + 1 < nLevels; k++) {
    uint32_t lo = 1u, hi = 0x7F7FFFFFu;   // the smallest positive float gives level 0; FLT_MAX normally more than k
    if (predictScaleLevelFormula(value(hi), logScaleFactor, nLevels) <= k) { out[k] = value(hi); continue; }
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (predictScaleLevelFormula(value(mid), logScaleFactor, nLevels) <= k) lo = mid; else hi = mid;
    }
    out[k] = value(lo);
  }
}

// one frame as the frustum test reads it; the level table is rebuilt only when the scale factor changes
template <class FrameT>
inline YdFrustumView frustumView(FrameT& f, float viewingCosLimit) {
  YdFrustumView v;
  std::memset(&v, 0, sizeof v);
  const cv::Mat O = f.getCameraOriginInWorld();
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) v.Rcw[3 * r + c] = f.m_cvMat_T_c2w.template at<float>(r, c);
    v.tcw[r] = f.m_cvMat_T_c2w.template at<float>(r, 3);
    v.Ow[r] = O.at<float>(r);
  }
  v.fx = FrameT::m_flt_fx; v.fy = FrameT::m_flt_fy; v.cx = FrameT::m_flt_cx; v.cy = FrameT::m_flt_cy; v.bf = FrameT::m_flt_baseLineTimesFx;
  v.min_x = FrameT::m_flt_minX; v.max_x = FrameT::m_flt_maxX; v.min_y = FrameT::m_flt_minY; v.max_y = FrameT::m_flt_maxY;
  v.viewing_cos_limit = viewingCosLimit;
  v.n_levels = (int32_t)f.m_v_scaleFactors.size();
  if (v.n_levels < 1 || v.n_levels > 8) throw std::runtime_error("ydorb: 1..8 pyramid levels are supported");
  thread_local float cachedLog = 0.f, cachedTable[7];
  thread_local int cachedLevels = 0;
  if (cachedLevels != v.n_levels || cachedLog != f.m_flt_logScaleFactor) {
    levelRatioTable(f.m_flt_logScaleFactor, v.n_levels, cachedTable);
    cachedLog = f.m_flt_logScaleFactor; cachedLevels = v.n_levels;
  }
  for (int k = 0; k + 1 < v.n_levels; k++) v.level_ratio[k] = cachedTable[k];
  for (int k = 0; k < v.n_levels; k++) v.scale_factors[k] = f.m_v_scaleFactors[k];
  return v;
}

// the map points as the shared table of the ABI; withDescriptors for the search
template <class MapPointPtr>
struct MapPointTableHost {
  std::vector<float> posMin, normalMax, maxDistance;
  std::vector<uint8_t> desc;
  YdMapPointTable table;
  MapPointTableHost(const std::vector<MapPointPtr>& mps, bool withDescriptors) {
    const size_t n = mps.size();
    posMin.resize(4 * n + 4); normalMax.resize(4 * n + 4); maxDistance.resize(n + 1);
    if (withDescriptors) desc.resize(32 * n + 32);
    for (size_t i = 0; i < n; i++) {
      const cv::Mat P = mps[i]->getPosInWorld(), N = mps[i]->getNormal();
      for (int k = 0; k < 3; k++) { posMin[4 * i + k] = P.at<float>(k); normalMax[4 * i + k] = N.at<float>(k); }
      posMin[4 * i + 3] = mps[i]->getMinDistanceInvariance();
      normalMax[4 * i + 3] = mps[i]->getMaxDistanceInvariance();
      maxDistance[i] = mps[i]->getMaxDistance();
      if (withDescriptors) { const cv::Mat d = mps[i]->getDescriptor(); std::memcpy(desc.data() + 32 * i, d.template ptr<uint8_t>(), 32); }
    }
    table.pos_min = posMin.data(); table.normal_max = normalMax.data(); table.max_distance = maxDistance.data();
    table.desc = withDescriptors ? desc.data() : nullptr;
    table.n = (int32_t)n;
  }
};

template <class MapPointPtr>
inline void writeTrackFields(const MapPointPtr& mp, uint8_t status, const YdTrackView& row) {
  mp->m_b_isTrackInView = status == YDORB_FRUSTUM_IN_VIEW;
  if (status != YDORB_FRUSTUM_IN_VIEW) return;   // the reference leaves the other members as they were
  mp->m_flt_trackProjX = row.u; mp->m_flt_trackProjY = row.v; mp->m_flt_trackProjRightX = row.ur;
  mp->m_int_trackScaleLevel = row.level; mp->m_flt_trackViewCos = row.view_cos;
}

// Frame::isInCameraFrustum(mp, viewingCosLimit) for every map point of a list in ONE ydorb_frustum_cull call; inView[i] = its return
// value.  Null or bad points are the caller's business in the reference too: pass the points it would have passed.
template <class FrameT, class MapPointPtr>
inline std::vector<bool> isInCameraFrustumBatch(FrameT& frame, const std::vector<MapPointPtr>& mapPoints, float viewingCosLimit, int device = 0) {
  const int n = (int)mapPoints.size();
  std::vector<bool> inView(n, false);
  if (n == 0) return inView;
  const YdFrustumView view = frustumView(frame, viewingCosLimit);
  MapPointTableHost<MapPointPtr> host(mapPoints, false);
  std::vector<int32_t> idx(n);
  for (int i = 0; i < n; i++) idx[i] = i;
  std::vector<uint8_t> skip(n, 0), status(n);
  std::vector<YdTrackView> rows(n);
  const int32_t start[2] = {0, n};
  YdFrustumBatch B;
  B.device = device; B.n_views = 1; B.views = &view; B.table = host.table; B.list_start = start; B.point_idx = idx.data(); B.skip = skip.data();
  if (ydorb_frustum_cull(&B, rows.data(), status.data(), nullptr) != YDORB_OK) throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
  for (int i = 0; i < n; i++) { writeTrackFields(mapPoints[i], status[i], rows[i]); inView[i] = status[i] == YDORB_FRUSTUM_IN_VIEW; }
  return inView;
}

// Tracking::searchLocalPoints' body.  Returns what searchByProjectionInFrameAndMapPoint returns (0 when no point is in view: the
// reference then does not search).
template <class FrameT, class MapPointPtr>
inline int searchLocalPointsImpl(ydorb_matcher_t* m, FrameT& frame, const std::vector<MapPointPtr>& localMapPoints, float th, float ratio) {
  for (auto& mp : frame.m_v_sptrMapPoints) {      // the points the frame already tracks are not searched again
    if (!mp) continue;
    if (mp->isBad()) { mp.reset(); continue; }
    mp->increaseVisible();
    mp->m_int_lastSeenInFrameID = frame.m_int_ID;
    mp->m_b_isTrackInView = false;
  }
  const int n = (int)localMapPoints.size();
  if (n == 0) return 0;
  std::vector<uint8_t> skip(n), hasObs(n), status(n);
  for (int i = 0; i < n; i++) {
    skip[i] = (localMapPoints[i]->m_int_lastSeenInFrameID == frame.m_int_ID || localMapPoints[i]->isBad()) ? 1 : 0;
    hasObs[i] = localMapPoints[i]->getObservationsNum() > 0 ? 1 : 0;
  }
  const YdFrustumView view = frustumView(frame, 0.5f);
  MapPointTableHost<MapPointPtr> host(localMapPoints, true);
  std::vector<YdTrackView> rows(n);
  std::vector<uint8_t> taken;
  takenMask(frame, false, taken);
  std::vector<int32_t> assigned(taken.size(), -1);
  int32_t nToMatch = 0, nMatches = 0;
  const YdFrameView fv = frameView(frame);
  if (ydorb_search_local_points(m, &fv, &view, &host.table, skip.data(), hasObs.data(), th, ratio, taken.data(), assigned.data(), rows.data(),
                                status.data(), &nToMatch, &nMatches) != YDORB_OK)
    throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
  for (int i = 0; i < n; i++) {
    if (status[i] == YDORB_FRUSTUM_SKIPPED) continue;   // the reference does not call isInCameraFrustum for these
    writeTrackFields(localMapPoints[i], status[i], rows[i]);
    if (status[i] == YDORB_FRUSTUM_IN_VIEW) localMapPoints[i]->increaseVisible();
  }
  for (size_t i = 0; i < assigned.size(); i++)
    if (assigned[i] >= 0) frame.m_v_sptrMapPoints[i] = localMapPoints[assigned[i]];
  return nToMatch > 0 ? nMatches : 0;
}

// Tracking::searchLocalPoints' body over a MapMirror with enableAttributes() (mapMirror.hpp): the same pre-loop
// and post-loop, but position, normal, distances and descriptor of every local point are read on the device by slot and only the slot
// list and a skip byte per point go up (ydorb_mapdb_search_local_points).  isBad() and getObservationsNum() are not asked per point:
// the table's bad flag and observation span answer them.  seen (updateLocalPointsImpl's return value) may be given; a point it flags is
// skipped as one whose m_int_lastSeenInFrameID is this frame's.  A point the table holds no complete attributes for comes back as
// YDORB_FRUSTUM_NO_ATTRIBUTES and is handled as not in view (mirror.verifyAttributes() names it).
template <class Mirror, class FrameT, class MapPointPtr>
inline int searchLocalPointsImpl(Mirror& mirror, ydorb_matcher_t* m, FrameT& frame, const std::vector<MapPointPtr>& localMapPoints, float th, float ratio,
                                 const std::vector<uint8_t>* seen = nullptr) {
  for (auto& mp : frame.m_v_sptrMapPoints) {      // the points the frame already tracks are not searched again
    if (!mp) continue;
    if (mp->isBad()) { mp.reset(); continue; }
    mp->increaseVisible();
    mp->m_int_lastSeenInFrameID = frame.m_int_ID;
    mp->m_b_isTrackInView = false;
  }
  const int n = (int)localMapPoints.size();
  if (n == 0) return 0;
  std::vector<uint8_t> skip(n), status;
  for (int i = 0; i < n; i++) skip[i] = (localMapPoints[i]->m_int_lastSeenInFrameID == frame.m_int_ID || (seen && (*seen)[i])) ? 1 : 0;
  const YdFrustumView view = frustumView(frame, 0.5f);
  std::vector<YdTrackView> rows;
  std::vector<uint8_t> taken;
  takenMask(frame, false, taken);
  std::vector<int32_t> assigned(taken.size(), -1);
  int32_t nToMatch = 0;
  const YdFrameView fv = frameView(frame);
  const int nMatches = mirror.searchLocalPoints(m, fv, view, localMapPoints, skip, th, ratio, taken, assigned, rows, status, nToMatch);
  for (int i = 0; i < n; i++) {
    if (status[i] == YDORB_FRUSTUM_SKIPPED) continue;   // the reference does not call isInCameraFrustum for these
    writeTrackFields(localMapPoints[i], status[i], rows[i]);   // YDORB_FRUSTUM_NO_ATTRIBUTES: not in view
    if (status[i] == YDORB_FRUSTUM_IN_VIEW) localMapPoints[i]->increaseVisible();
  }
  for (size_t i = 0; i < assigned.size(); i++)
    if (assigned[i] >= 0) frame.m_v_sptrMapPoints[i] = localMapPoints[assigned[i]];
  return nToMatch > 0 ? nMatches : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Tracking::updateLocalMap's two halves over a MapMirror's keyframe rows (mapMirror.hpp), restated from
// ORB-SLAM2's Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (the reference source is absent from this repository).  The member
// functions become forwards ("Local map"):
//   void Tracking::updateLocalKeyFrames() { ydorb::adapter::updateLocalKeyFramesImpl(mirror, m_frame_currentFrame, m_v_sptrLocalKeyFrames, m_sptr_referenceKeyFrame); }
//   void Tracking::updateLocalPoints()    { ydorb::adapter::updateLocalPointsImpl(mirror, m_frame_currentFrame, m_v_sptrLocalKeyFrames, m_v_sptrLocalMapPoints); }
// Assumed spellings beyond those above: Frame m_sptr_referenceKeyFrame; KeyFrame isBad(), m_int_trackReferenceForFrameID,
// getBestCovisibilityKeyFrames(int), getChildren() (a std::set of keyframes), getParent(); MapPoint m_int_trackReferenceForFrameID.

// The counter comes from the mirror (one query, no observation map is walked); the frame entries whose point is bad are nulled here;
// then the reference's tail as written: the keyframes of the counter in the container's order, the reference keyframe by the largest
// count (the first of equals), and one neighbour, one child and the parent per keyframe until more than 80 are held.  The `break`
// after the parent leaves the outer loop, as in the reference.
template <class Mirror, class FrameT, class KeyFramePtr>
inline void updateLocalKeyFramesImpl(Mirror& mirror, FrameT& frame, std::vector<KeyFramePtr>& localKeyFrames, KeyFramePtr& referenceKeyFrame) {
  std::vector<size_t> badIndices;
  const std::map<KeyFramePtr, int> keyFrameCounter = mirror.keyFrameCounter(frame.m_v_sptrMapPoints, &badIndices);
  for (const size_t i : badIndices) frame.m_v_sptrMapPoints[i].reset();
  if (keyFrameCounter.empty()) return;
  int max = 0;
  KeyFramePtr keyFrameMax;
  localKeyFrames.clear();
  localKeyFrames.reserve(3 * keyFrameCounter.size());
  for (const auto& kv : keyFrameCounter) {
    const KeyFramePtr& kf = kv.first;
    if (kf->isBad()) continue;
    if (kv.second > max) { max = kv.second; keyFrameMax = kf; }
    localKeyFrames.push_back(kf);
    kf->m_int_trackReferenceForFrameID = frame.m_int_ID;
  }
  const size_t nFirst = localKeyFrames.size();   // the reference's end iterator is taken before the loop pushes
  for (size_t i = 0; i < nFirst; i++) {
    if (localKeyFrames.size() > 80) break;
    const KeyFramePtr kf = localKeyFrames[i];
    for (const KeyFramePtr& neighbour : kf->getBestCovisibilityKeyFrames(10)) {
      if (neighbour->isBad()) continue;
      if (neighbour->m_int_trackReferenceForFrameID != frame.m_int_ID) {
        localKeyFrames.push_back(neighbour);
        neighbour->m_int_trackReferenceForFrameID = frame.m_int_ID;
        break;
      }
    }
    for (const KeyFramePtr& child : kf->getChildren()) {
      if (child->isBad()) continue;
      if (child->m_int_trackReferenceForFrameID != frame.m_int_ID) {
        localKeyFrames.push_back(child);
        child->m_int_trackReferenceForFrameID = frame.m_int_ID;
        break;
      }
    }
    const KeyFramePtr parent = kf->getParent();
    if (parent && parent->m_int_trackReferenceForFrameID != frame.m_int_ID) {
      localKeyFrames.push_back(parent);
      parent->m_int_trackReferenceForFrameID = frame.m_int_ID;
      break;   // leaves the outer loop
    }
  }
  if (keyFrameMax) {
    referenceKeyFrame = keyFrameMax;
    frame.m_sptr_referenceKeyFrame = referenceKeyFrame;
  }
}

// One query in place of the walk over every local keyframe's map-point vector.  Returns, per local map point, whether it is one of the
// frame's own matches: what searchLocalPoints' first loop marks m_int_lastSeenInFrameID for, and its `skip`.
template <class Mirror, class FrameT, class KeyFramePtr, class MapPointPtr>
inline std::vector<uint8_t> updateLocalPointsImpl(Mirror& mirror, FrameT& frame, const std::vector<KeyFramePtr>& localKeyFrames,
                                                  std::vector<MapPointPtr>& localMapPoints) {
  std::vector<uint8_t> seen;
  localMapPoints = mirror.localPoints(localKeyFrames, frame.m_v_sptrMapPoints, &seen);
  for (const MapPointPtr& mp : localMapPoints) mp->m_int_trackReferenceForFrameID = frame.m_int_ID;
  return seen;
}

// The search of Tracking::trackReferenceKeyFrame over a resident map table: searchByBowInKeyFrameAndFrame(refKF, frame) as the
// one-keyframe case of orbMatcher.hpp's batched overload.  Optional: with one keyframe there is no round trip to save, only the
// keyframe's side of the upload (DESIGN.md section 6v has what was measured); Tracking::relocalize, which names every candidate in one
// call, is where the batched form pays.
//   int nmatches = ydorb::adapter::trackReferenceKeyFrameSearchImpl(mirror, ydorb::adapter::matcher(), m_frame_currentFrame,
//                                                                   m_sptr_referenceKeyFrame, vpMapPointMatches);   // ratio 0.7, orientation check on
template <class Mirror, class FrameT, class KeyFramePtr, class MapPointPtr>
inline int trackReferenceKeyFrameSearchImpl(Mirror& mirror, ydorb_matcher_t* m, FrameT& frame, const KeyFramePtr& referenceKeyFrame,
                                            std::vector<MapPointPtr>& matched, float ratio = 0.7f, bool checkOrientation = true) {
  std::vector<std::vector<MapPointPtr>> all;
  const std::vector<int> n = searchByBowInKeyFrameAndFrame(mirror, m, std::vector<KeyFramePtr>{referenceKeyFrame}, frame, all, ratio, checkOrientation);
  matched = std::move(all[0]);
  return n[0];
}

}  // namespace adapter
}  // namespace ydorb
#endif
