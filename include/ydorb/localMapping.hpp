// Drop-in body of LocalMapping::createNewMapPoints (ORB-SLAM2 LocalMapping::CreateNewMapPoints, which YDORBSLAM renames; SURVEY 3.3,
// DESIGN.md section 6f) on top of the ydorb C ABI.  A function template over the reference's own KeyFrame / MapPoint / Map / Frame
// types (included by the translation unit that instantiates it), so the member function becomes a one-line forward:
//   void LocalMapping::createNewMapPoints()
//   { ydorb::adapter::createNewMapPointsImpl<Frame, std::shared_ptr<KeyFrame>, MapPoint>(ydorb::adapter::matcher(), m_sptr_currentKeyFrame,
//       m_sptr_map, m_list_recentAddedMapPoints, [this] { return checkNewKeyFrames(); }); }
// Per neighbour of getBestCovisibilityKeyFrames(10), in the reference's order: abortCheck() for i > 0, the baseline test, F12 on the host,
// the searchForTriangulation adapter (GPU), ONE ydorb_triangulate_matches call for the neighbour's matches (GPU), then the reference's
// bookkeeping for the accepted matches in match order.  This flat loop is one call per neighbour because a point accepted with
// neighbour i sets the current keyframe's map point at idx1 and so changes what searchForTriangulation may match with neighbour i + 1;
// the overload over a MapMirror below makes one call for all neighbours and carries that claim on the device.
// Assumed spellings, as in the other adapters: m_v_keyPoints, m_v_rightXcords, m_v_depth, m_v_scaleFactors, m_v_scaleFactorSquares,
// getRotation_c2w / getTranslation_c2w / getCameraOriginInWorld, FrameT::m_flt_fx .. m_flt_baseLineTimesFx; invfx = 1.0f / fx as the
// reference stores it; the MapPoint constructor MapPoint(pos, keyFrame, map).
#ifndef YDORB_ADAPTER_LOCALMAPPING_HPP
#define YDORB_ADAPTER_LOCALMAPPING_HPP

#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <opencv2/core.hpp>

#include "c_api.h"
#include "mapPoint.hpp"
#include "orbMatcher.hpp"
#include "tracking.hpp"   // levelRatioTable, which orbMatcher.hpp's fuse overloads over a mirror call

namespace ydorb {
namespace adapter {

// one keyframe as ydorb_triangulate_matches reads it; Rwc = Rcw^T in plain loops (a transpose rounds nothing)
template <class FrameT, class KeyFramePtr>
inline YdTriView triView(const KeyFramePtr& kf) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(YdKeyPoint), "cv::KeyPoint layout");
  YdTriView v;
  std::memset(&v, 0, sizeof v);
  v.kps = reinterpret_cast<const YdKeyPoint*>(kf->m_v_keyPoints.data());
  v.right_x = kf->m_v_rightXcords.data();
  v.depth = kf->m_v_depth.data();
  v.n = (int32_t)kf->m_v_keyPoints.size();
  const cv::Mat R = kf->getRotation_c2w(), t = kf->getTranslation_c2w(), O = kf->getCameraOriginInWorld();
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) { v.Tcw[4 * r + c] = R.at<float>(r, c); v.Rwc[3 * c + r] = R.at<float>(r, c); }
    v.Tcw[4 * r + 3] = t.at<float>(r);
    v.Ow[r] = O.at<float>(r);
  }
  v.fx = FrameT::m_flt_fx; v.fy = FrameT::m_flt_fy; v.cx = FrameT::m_flt_cx; v.cy = FrameT::m_flt_cy;
  v.invfx = 1.0f / FrameT::m_flt_fx; v.invfy = 1.0f / FrameT::m_flt_fy;
  v.b = FrameT::m_flt_baseLine; v.bf = FrameT::m_flt_baseLineTimesFx;
  v.level_sigma2 = kf->m_v_scaleFactorSquares.data();
  v.scale_factors = kf->m_v_scaleFactors.data();
  v.n_levels = (int32_t)kf->m_v_scaleFactors.size();
  return v;
}

// LocalMapping::computeF12: F12 = K^-T [t12]x R12 K^-1 with R12 = R1w R2w^T, t12 = -R12 t2w + t1w, in plain 3x3 float loops (each
// product rounded, sums in ascending k); K^-1 in closed form from fx, fy, cx, cy
template <class FrameT, class KeyFramePtr>
inline cv::Mat computeF12(const KeyFramePtr& kf1, const KeyFramePtr& kf2) {
  const cv::Mat R1 = kf1->getRotation_c2w(), t1 = kf1->getTranslation_c2w(), R2 = kf2->getRotation_c2w(), t2 = kf2->getTranslation_c2w();
  float R12[3][3], t12[3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      float s = 0.f;
      for (int k = 0; k < 3; k++) s = s + R1.at<float>(r, k) * R2.at<float>(c, k);
      R12[r][c] = s;
    }
  for (int r = 0; r < 3; r++) {
    float s = 0.f;
    for (int k = 0; k < 3; k++) s = s + R12[r][k] * t2.at<float>(k);
    t12[r] = -s + t1.at<float>(r);
  }
  const float tx[3][3] = {{0.f, -t12[2], t12[1]}, {t12[2], 0.f, -t12[0]}, {-t12[1], t12[0], 0.f}};
  const float ifx = 1.0f / FrameT::m_flt_fx, ify = 1.0f / FrameT::m_flt_fy;
  const float Kinv[3][3] = {{ifx, 0.f, -FrameT::m_flt_cx * ifx}, {0.f, ify, -FrameT::m_flt_cy * ify}, {0.f, 0.f, 1.f}};
  float M[3][3], N[3][3];
  auto mul = [](const float (*A)[3], const float (*B)[3], float (*C)[3], bool transposeA) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        float s = 0.f;
        for (int k = 0; k < 3; k++) s = s + (transposeA ? A[k][r] : A[r][k]) * B[k][c];
        C[r][c] = s;
      }
  };
  mul(Kinv, tx, M, true);    // K^-T [t12]x
  mul(M, R12, N, false);
  mul(N, Kinv, M, false);
  cv::Mat F(3, 3, CV_32F);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) F.at<float>(r, c) = M[r][c];
  return F;
}

// Returns the number of MapPoints created.  MapPointT is the pointee (std::make_shared<MapPointT>(pos, keyFrame, map)).  `device` is
// the device that `m` was created on (matcher(device)), so that the search and the triangulation of a neighbour run on the same GPU.
template <class FrameT, class KeyFramePtr, class MapPointT, class MapPtr, class RecentList, class AbortCheck>
int createNewMapPointsImpl(ydorb_matcher_t* m, KeyFramePtr current, MapPtr map, RecentList& recentAddedMapPoints, AbortCheck abortCheck,
                           int device = 0) {
  const std::vector<KeyFramePtr> neighbours = current->getBestCovisibilityKeyFrames(10);
  const cv::Mat Ow1 = current->getCameraOriginInWorld();
  const float ratioFactor = 1.5f * current->m_v_scaleFactors[1];   // 1.5f * mfScaleFactor
  YdTriView views[2];
  views[0] = triView<FrameT>(current);   // pose and intrinsics of the current keyframe, read once before the loop as the reference does
  int created = 0;
  for (size_t i = 0; i < neighbours.size(); i++) {
    if (i > 0 && abortCheck()) return created;
    KeyFramePtr kf2 = neighbours[i];
    const cv::Mat baselineVec = kf2->getCameraOriginInWorld() - Ow1;
    const float baseline = (float)cv::norm(baselineVec);
    if (baseline < FrameT::m_flt_baseLine) continue;
    const cv::Mat F12 = computeF12<FrameT>(current, kf2);
    std::vector<std::pair<int, int>> pairs;
    searchForTriangulation<KeyFramePtr, FrameT>(m, current, kf2, F12, pairs, false, false);   // ORBmatcher(0.6, false)
    const int32_t n = (int32_t)pairs.size();
    if (n == 0) continue;
    views[1] = triView<FrameT>(kf2);
    std::vector<int32_t> idx1(n), idx2(n);
    for (int32_t k = 0; k < n; k++) { idx1[k] = pairs[k].first; idx2[k] = pairs[k].second; }
    const int32_t first = 0, second = 1, start[2] = {0, n};
    YdTriBatch B;
    std::memset(&B, 0, sizeof B);
    B.device = device; B.n_views = 2; B.n_problems = 1; B.views = views; B.first_view = &first; B.second_view = &second;
    B.match_start = start; B.idx1 = idx1.data(); B.idx2 = idx2.data(); B.ratio_factor = &ratioFactor;
    std::vector<float> x3d(3 * (size_t)n);
    std::vector<uint8_t> status(n);
    if (ydorb_triangulate_matches(&B, x3d.data(), status.data(), nullptr) != YDORB_OK)
      throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
    for (int32_t k = 0; k < n; k++) {
      if ((status[k] & 15) != YDORB_TRI_ACCEPTED) continue;
      cv::Mat pos(3, 1, CV_32F);
      for (int r = 0; r < 3; r++) pos.at<float>(r) = x3d[3 * (size_t)k + r];
      auto mp = std::make_shared<MapPointT>(pos, current, map);
      mp->addObservation(current, idx1[k]);
      mp->addObservation(kf2, idx2[k]);
      current->addMapPoint(mp, idx1[k]);
      kf2->addMapPoint(mp, idx2[k]);
      mp->computeDistinctiveDescriptors();
      mp->updateNormalAndDepth();
      map->addMapPoint(mp);
      recentAddedMapPoints.push_back(mp);
      created++;
    }
  }
  return created;
}

// one keyframe as ydorb_mapdb_create_new_points reads it: triView's constants; kf_slot, n and depth are the mirror's to set
template <class FrameT, class KeyFramePtr>
inline YdCreateView createView(const KeyFramePtr& kf) {
  const YdTriView t = triView<FrameT>(kf);
  if (t.n_levels < 1 || t.n_levels > 8) throw std::runtime_error("ydorb: createNewMapPoints: a scale pyramid outside 1..8 levels");
  YdCreateView v;
  std::memset(&v, 0, sizeof v);
  std::memcpy(v.Tcw, t.Tcw, sizeof v.Tcw); std::memcpy(v.Rwc, t.Rwc, sizeof v.Rwc); std::memcpy(v.Ow, t.Ow, sizeof v.Ow);
  v.fx = t.fx; v.fy = t.fy; v.cx = t.cx; v.cy = t.cy; v.invfx = t.invfx; v.invfy = t.invfy; v.b = t.b; v.bf = t.bf;
  for (int l = 0; l < t.n_levels; l++) { v.level_sigma2[l] = t.level_sigma2[l]; v.scale_factors[l] = t.scale_factors[l]; }
  v.n_levels = t.n_levels;
  return v;
}

// createNewMapPoints over a resident map table (mapMirror.hpp with enableDescriptors(), enableFeatures() and enableBow(); DESIGN.md
// section 6t):
//   void LocalMapping::createNewMapPoints()
//   { ydorb::adapter::createNewMapPointsImpl<Frame, std::shared_ptr<KeyFrame>, MapPoint>(*m_mirror, ydorb::adapter::matcher(),
//       m_sptr_currentKeyFrame, m_sptr_map, m_list_recentAddedMapPoints, [this] { return checkNewKeyFrames(); }); }
// The same neighbour list, baseline test, computeF12, epipole and ratioFactor as the flat body above, computed for every neighbour
// up front; then ONE createNewPoints call, whose device side carries the claim of an accepted idx1 from neighbour to neighbour; then the
// walk, neighbour by neighbour with abortCheck() for i > 0 (over ALL neighbours, as the flat loop asks before its baseline test) and
// per neighbour the accepted idx1 in ascending order with the flat body's bookkeeping.  Results of neighbour i do not depend on later
// neighbours, so an abort after neighbour k drops the tail unread.  The new points, both row entries and the points' views are
// registered with the mirror (touch, touchEntry), as searchInNeighborsImpl registers its changes.
template <class FrameT, class KeyFramePtr, class MapPointT, class Mirror, class MapPtr, class RecentList, class AbortCheck>
int createNewMapPointsImpl(Mirror& mirror, ydorb_matcher_t* m, KeyFramePtr current, MapPtr map, RecentList& recentAddedMapPoints, AbortCheck abortCheck) {
  const std::vector<KeyFramePtr> neighbours = current->getBestCovisibilityKeyFrames(10);
  const cv::Mat Ow1 = current->getCameraOriginInWorld();
  const float ratioFactor = 1.5f * current->m_v_scaleFactors[1];   // 1.5f * mfScaleFactor
  std::vector<KeyFramePtr> searched;
  std::vector<int> callOf(neighbours.size(), -1);                  // the call's neighbour of each listed one; -1: the baseline test skips it
  std::vector<YdCreateNeighbour> records;
  for (size_t i = 0; i < neighbours.size(); i++) {
    const KeyFramePtr& kf2 = neighbours[i];
    const cv::Mat baselineVec = kf2->getCameraOriginInWorld() - Ow1;
    const float baseline = (float)cv::norm(baselineVec);
    if (baseline < FrameT::m_flt_baseLine) continue;
    YdCreateNeighbour G;
    std::memset(&G, 0, sizeof G);
    G.view = createView<FrameT>(kf2);
    const cv::Mat F12 = computeF12<FrameT>(current, kf2);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) G.F[r * 3 + c] = F12.at<float>(r, c);
    const cv::Mat C2 = kf2->getRotation_c2w() * Ow1 + kf2->getTranslation_c2w();   // searchForTriangulation's epipole (orbMatcher.hpp)
    G.ex = FrameT::m_flt_fx * C2.at<float>(0) / C2.at<float>(2) + FrameT::m_flt_cx;
    G.ey = FrameT::m_flt_fy * C2.at<float>(1) / C2.at<float>(2) + FrameT::m_flt_cy;
    G.ratio_factor = ratioFactor;
    callOf[i] = (int)searched.size();
    searched.push_back(kf2);
    records.push_back(G);
  }
  if (searched.empty()) return 0;
  const typename Mirror::CreateResult r = mirror.createNewPoints(m, current, searched, createView<FrameT>(current), records, false, false);   // ORBmatcher(0.6, false)
  int created = 0;
  for (size_t i = 0; i < neighbours.size(); i++) {
    if (i > 0 && abortCheck()) return created;
    if (callOf[i] < 0) continue;
    const KeyFramePtr& kf2 = neighbours[i];
    const size_t row = (size_t)callOf[i] * (size_t)r.n;
    if (r.neighbourStatus[(size_t)callOf[i]] != YDORB_CREATE_NB_OK)
      throw std::runtime_error("ydorb: createNewMapPoints: the resident table cannot search a neighbour (status " +
                               std::to_string((int)r.neighbourStatus[(size_t)callOf[i]]) + ")");
    for (int32_t idx1 = 0; idx1 < r.n; idx1++) {
      if ((r.status[row + (size_t)idx1] & 15) != YDORB_TRI_ACCEPTED) continue;
      const int32_t idx2 = r.matchedSecond[row + (size_t)idx1];
      cv::Mat pos(3, 1, CV_32F);
      for (int k = 0; k < 3; k++) pos.at<float>(k) = r.x3d[3 * (row + (size_t)idx1) + (size_t)k];
      auto mp = std::make_shared<MapPointT>(pos, current, map);
      mp->addObservation(current, idx1);
      mp->addObservation(kf2, idx2);
      current->addMapPoint(mp, idx1);
      kf2->addMapPoint(mp, idx2);
      mp->computeDistinctiveDescriptors();
      mp->updateNormalAndDepth();
      map->addMapPoint(mp);
      recentAddedMapPoints.push_back(mp);
      mirror.touch(mp);
      mirror.touchEntry(current, (size_t)idx1);
      mirror.touchEntry(kf2, (size_t)idx2);
      created++;
    }
  }
  return created;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Drop-in body of LocalMapping::keyFrameCulling (ORB-SLAM2 LocalMapping::KeyFrameCulling):
//   void LocalMapping::keyFrameCulling()
//   { ydorb::adapter::keyFrameCullingImpl<std::shared_ptr<KeyFrame>, std::shared_ptr<MapPoint>>(m_sptr_currentKeyFrame, thDepth); }
// One flatten of the covisible keyframes' map points and one ydorb_map_keyframe_redundancy call judge every candidate; the walk then
// follows the reference's order.  The first candidate with `cull` gets setBadFlag(); when that made it isBad(), its observations are
// gone from every map point, so its byte in `removed` is set and the candidates after it are asked for again over the same table (no
// second flatten).  A keyframe that setNotErase() protects is only marked by setBadFlag(): it stays unmasked and the walk goes on.
// Additional assumed spellings: KeyFrame getVectorCovisibleKeyFrames(), m_int_keyFrameID (0 = the first keyframe of the map, never
// culled), m_v_depth, setBadFlag(), isBad(); the depth test !(depth > thDepth || depth < 0) is always made (stereo / RGB-D).
template <class KeyFramePtr, class MapPointPtr>
struct CullingFlat {
  ObservationFlat<KeyFramePtr, MapPointPtr> obs;
  std::vector<KeyFramePtr> candidates;
  std::vector<int32_t> candKf, listStart{0}, pointIdx;
  std::vector<uint8_t> ownLevel;
};

template <class KeyFramePtr, class MapPointPtr>
inline void flattenCulling(const KeyFramePtr& current, float thDepth, CullingFlat<KeyFramePtr, MapPointPtr>& F) {
  for (const KeyFramePtr& kf : current->getVectorCovisibleKeyFrames()) {
    if (kf->m_int_keyFrameID == 0) continue;
    F.candidates.push_back(kf);
    F.candKf.push_back(F.obs.slot(kf));
    const std::vector<MapPointPtr> mps = kf->getMapPointMatches();
    for (size_t i = 0; i < mps.size(); i++) {
      if (!mps[i]) continue;
      if (kf->m_v_depth[i] > thDepth || kf->m_v_depth[i] < 0) continue;   // the caller's float test (a bad point is skipped either way)
      F.pointIdx.push_back(F.obs.point(mps[i]));
      F.ownLevel.push_back((uint8_t)kf->m_v_keyPoints[i].octave);
    }
    if (F.pointIdx.size() > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX culling entries");
    F.listStart.push_back((int32_t)F.pointIdx.size());
  }
}

// Returns the keyframes setBadFlag() was called on, in order.
template <class KeyFramePtr, class MapPointPtr>
inline std::vector<KeyFramePtr> keyFrameCullingImpl(const KeyFramePtr& current, float thDepth, int device = 0) {
  CullingFlat<KeyFramePtr, MapPointPtr> F;
  flattenCulling(current, thDepth, F);
  std::vector<KeyFramePtr> flagged;
  const int32_t K = (int32_t)F.candidates.size();
  if (K == 0) return flagged;
  const YdObservationTable T = F.obs.table();
  std::vector<uint8_t> removed((size_t)T.n_keyframes, 0), cull(K);
  std::vector<int32_t> nCounted(K), nRedundant(K), start;
  bool masked = false;
  int32_t at = 0;
  while (at < K) {
    const int32_t n = K - at, base = F.listStart[at];
    start.assign((size_t)n + 1, 0);
    for (int32_t k = 0; k <= n; k++) start[k] = F.listStart[at + k] - base;
    mapCheck(ydorb_map_keyframe_redundancy(&T, F.candKf.data() + at, n, start.data(), F.pointIdx.data() + base, F.ownLevel.data() + base,
                                           masked ? removed.data() : nullptr, 3, device, nCounted.data(), nRedundant.data(), cull.data()));
    int32_t k = 0;
    for (; k < n; k++) {
      if (!cull[k]) continue;
      const KeyFramePtr& kf = F.candidates[at + k];
      kf->setBadFlag();
      flagged.push_back(kf);
      if (kf->isBad()) {   // erased: the verdicts after it are stale
        removed[F.candKf[at + k]] = 1;
        masked = true;
        k++;
        break;
      }
    }
    at += k;
  }
  return flagged;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Drop-in body of LocalMapping::searchInNeighbors (ORB-SLAM2 LocalMapping::SearchInNeighbors) over a resident map table (mapMirror.hpp
// with enableAttributes(), enableFeatures() and enableDescriptors()):
//   void LocalMapping::searchInNeighbors()
//   { ydorb::adapter::searchInNeighborsImpl<Frame, std::shared_ptr<KeyFrame>, std::shared_ptr<MapPoint>>(*m_mirror, ydorb::adapter::matcher(),
//       m_sptr_currentKeyFrame, m_b_isMonocular ? 20 : 10, storeDescriptor, storeNormalAndDepth); }
// The targets are collected as the reference collects them (the best covisible keyframes and five of each one's, marked with
// m_int_fuseTargetForKeyFrameID).  Then TWO batched calls where the reference makes one fuse call per target and one more:
//   direction 1  the current keyframe's map points into every target: fuseByProjection(mirror, m, targets, ...), one list per target;
//   direction 2  the targets' map points (each once, marked with m_int_fuseCandidateForKeyFrameID, bad ones left out) into the
//                current keyframe: the same overload with one target.  Its flush carries what direction 1 changed.
// The tail - computeDistinctiveDescriptors() and updateNormalAndDepth() of the current keyframe's points - goes through the mirror's
// two methods, whose write-through keeps the resident attributes current; storeDescriptor(mp, kf, idx, row) and
// storeNormalAndDepth(mp, normal, minDistance, maxDistance) store the results in the objects (INTEGRATION.md shows both).  The
// keyframe's updateConnections() stays the caller's last line.  Returns the fuse counts of direction 1 (per target) and direction 2.
// Additional assumed spellings: KeyFrame getBestCovisibilityKeyFrames(n), m_int_fuseTargetForKeyFrameID, m_int_keyFrameID, isBad(),
// getMapPointMatches(), m_flt_logScaleFactor, the static m_flt_minX .. m_flt_maxY; MapPoint m_int_fuseCandidateForKeyFrameID.
template <class FrameT, class KeyFramePtr, class MapPointPtr, class Mirror, class StoreDescriptor, class StoreNormalDepth>
inline std::pair<std::vector<int>, int> searchInNeighborsImpl(Mirror& mirror, ydorb_matcher_t* m, KeyFramePtr current, int nn, StoreDescriptor storeDescriptor,
                                                              StoreNormalDepth storeNormalAndDepth, float th = 3.0f) {
  std::vector<KeyFramePtr> targets;
  for (const KeyFramePtr& kf : current->getBestCovisibilityKeyFrames(nn)) {
    if (kf->isBad() || kf->m_int_fuseTargetForKeyFrameID == current->m_int_keyFrameID) continue;
    targets.push_back(kf);
    kf->m_int_fuseTargetForKeyFrameID = current->m_int_keyFrameID;
    for (const KeyFramePtr& kf2 : kf->getBestCovisibilityKeyFrames(5)) {
      if (kf2->isBad() || kf2->m_int_fuseTargetForKeyFrameID == current->m_int_keyFrameID || kf2->m_int_keyFrameID == current->m_int_keyFrameID) continue;
      targets.push_back(kf2);
      kf2->m_int_fuseTargetForKeyFrameID = current->m_int_keyFrameID;   // ORB-SLAM2 leaves this mark out and may list a keyframe twice; a second pass over it fuses nothing new
    }
  }
  std::pair<std::vector<int>, int> fused(std::vector<int>(), 0);
  if (targets.empty()) return fused;
  const std::vector<MapPointPtr> own = current->getMapPointMatches();
  fused.first = fuseByProjection<KeyFramePtr, MapPointPtr, FrameT>(mirror, m, targets, std::vector<std::vector<MapPointPtr> >(targets.size(), own), th);
  std::vector<MapPointPtr> candidates;
  for (const KeyFramePtr& kf : targets)
    for (const MapPointPtr& mp : kf->getMapPointMatches()) {
      if (!mp || mp->isBad() || mp->m_int_fuseCandidateForKeyFrameID == current->m_int_keyFrameID) continue;
      mp->m_int_fuseCandidateForKeyFrameID = current->m_int_keyFrameID;
      candidates.push_back(mp);
    }
  fused.second = fuseByProjection<KeyFramePtr, MapPointPtr, FrameT>(mirror, m, std::vector<KeyFramePtr>(1, current),
                                                                     std::vector<std::vector<MapPointPtr> >(1, candidates), th)[0];
  std::vector<MapPointPtr> live;
  for (const MapPointPtr& mp : current->getMapPointMatches())
    if (mp && !mp->isBad()) live.push_back(mp);
  mirror.computeDistinctiveDescriptors(live, storeDescriptor);
  mirror.updateNormalAndDepth(live, storeNormalAndDepth);
  return fused;
}

}  // namespace adapter
}  // namespace ydorb
#endif
