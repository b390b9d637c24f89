// Batched MapPoint::updateNormalAndDepth (ORB-SLAM2 MapPoint::UpdateNormalAndDepth) on top of the ydorb C ABI,
// and the flattening of the observation containers that the three map-maintenance adapters share (this file, keyFrame.hpp,
// localMapping.hpp).  Function templates over the reference's own KeyFrame / MapPoint types, included by the translation unit that
// instantiates them.  The loops that call updateNormalAndDepth() once per point (after a BA, in searchInNeighbors) become
//   ydorb::adapter::updateNormalAndDepthBatch(points, [](const std::shared_ptr<MapPoint>& mp, const cv::Mat& normal, float minD, float maxD)
//     { mp->setNormalAndDepth(normal, minD, maxD); });
// with the three-line setter INTEGRATION.md lists ("Map maintenance").  One flatten, one ydorb_map_update_normal_depth call.
// The observers of a point are passed in the iteration order of its own container (the float sum over them is ordered).
// Assumed spellings, as in the other adapters: MapPoint isBad(), getObservations() -> std::map<KeyFramePtr, size_t>, getPosInWorld(),
// getReferenceKeyFrame(); KeyFrame m_v_keyPoints (octave), m_v_rightXcords (>= 0 marks a stereo observation), m_v_scaleFactors (one
// pyramid for all keyframes), getCameraOriginInWorld().
#ifndef YDORB_ADAPTER_MAPPOINT_HPP
#define YDORB_ADAPTER_MAPPOINT_HPP

#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core.hpp>

#include "c_api.h"

namespace ydorb {
namespace adapter {

// The flattened observation table of a call: keyframes get slots in the order they are first met, map points an index in the order
// they are added (each distinct point once).
template <class KeyFramePtr, class MapPointPtr>
struct ObservationFlat {
  std::map<KeyFramePtr, int32_t> slotOf;
  std::vector<KeyFramePtr> keyFrames;
  std::map<MapPointPtr, int32_t> indexOf;
  std::vector<MapPointPtr> points;
  std::vector<int32_t> obsStart{0}, obsKf;
  std::vector<uint8_t> obsLevel, bad;

  int32_t slot(const KeyFramePtr& kf) {
    const auto it = slotOf.find(kf);
    if (it != slotOf.end()) return it->second;
    const int32_t s = (int32_t)keyFrames.size();
    slotOf[kf] = s;
    keyFrames.push_back(kf);
    return s;
  }
  int32_t point(const MapPointPtr& mp) {
    const auto it = indexOf.find(mp);
    if (it != indexOf.end()) return it->second;
    const int32_t p = (int32_t)points.size();
    indexOf[mp] = p;
    points.push_back(mp);
    bad.push_back(mp->isBad() ? 1 : 0);
    for (const auto& ob : mp->getObservations()) {   // the container's own order
      obsKf.push_back(slot(ob.first));
      const int octave = ob.first->m_v_keyPoints[ob.second].octave;
      obsLevel.push_back((uint8_t)((octave & 0x7f) | (ob.first->m_v_rightXcords[ob.second] >= 0 ? 0x80 : 0)));
    }
    if (obsKf.size() > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX observations in one table");
    obsStart.push_back((int32_t)obsKf.size());
    return p;
  }
  int32_t span(int32_t p) const { return obsStart[p + 1] - obsStart[p]; }
  YdObservationTable table() const {
    YdObservationTable T;
    T.n_points = (int32_t)points.size(); T.n_keyframes = (int32_t)keyFrames.size();
    T.obs_start = obsStart.data(); T.obs_kf = obsKf.data(); T.obs_level = obsLevel.data(); T.bad = bad.data();
    return T;
  }
};

inline void mapCheck(int rc) {
  if (rc != YDORB_OK) throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
}

// The inputs of ydorb_map_update_normal_depth for `points` (each distinct point once, in order)
template <class KeyFramePtr, class MapPointPtr>
struct NormalDepthFlat {
  ObservationFlat<KeyFramePtr, MapPointPtr> obs;
  std::vector<float> pos, centre, scaleFactors;
  std::vector<int32_t> refKf;
  std::vector<uint8_t> refLevel;
};

template <class KeyFramePtr, class MapPointPtr, class Points>
inline void flattenNormalDepth(const Points& points, NormalDepthFlat<KeyFramePtr, MapPointPtr>& F) {
  for (const MapPointPtr& mp : points) {
    if (!mp || F.obs.indexOf.count(mp)) continue;
    const int32_t p = F.obs.point(mp);
    const cv::Mat P = mp->getPosInWorld();
    for (int r = 0; r < 3; r++) F.pos.push_back(P.template at<float>(r));
    int32_t slot = 0;
    uint8_t level = 0;
    if (!F.obs.bad[p] && F.obs.span(p) > 0) {   // the reference reads its reference keyframe only past both early returns
      const KeyFramePtr ref = mp->getReferenceKeyFrame();
      const auto observations = mp->getObservations();
      const auto it = observations.find(ref);
      const size_t idx = it != observations.end() ? it->second : 0;   // observations[pRefKF] on the reference's copy
      slot = F.obs.slot(ref);
      level = (uint8_t)ref->m_v_keyPoints[idx].octave;
    }
    F.refKf.push_back(slot);
    F.refLevel.push_back(level);
  }
  for (const KeyFramePtr& kf : F.obs.keyFrames) {
    const cv::Mat O = kf->getCameraOriginInWorld();
    for (int r = 0; r < 3; r++) F.centre.push_back(O.template at<float>(r));
  }
  if (!F.obs.keyFrames.empty()) F.scaleFactors = F.obs.keyFrames[0]->m_v_scaleFactors;
  else F.scaleFactors.assign(1, 1.0f);          // no observation anywhere: nothing is updated, the entry still wants a pyramid
}

// apply(mp, normal (3x1 CV_32F), minDistance, maxDistance) for every point the reference would have updated (not bad, observed), in
// the order of `points`.  Returns their number.
template <class KeyFramePtr, class MapPointPtr, class Points, class Apply>
inline int updateNormalAndDepthBatch(const Points& points, Apply apply, int device = 0) {
  NormalDepthFlat<KeyFramePtr, MapPointPtr> F;
  flattenNormalDepth<KeyFramePtr, MapPointPtr>(points, F);
  const size_t n = F.obs.points.size();
  if (n == 0) return 0;
  const YdObservationTable T = F.obs.table();
  std::vector<float> normal(3 * n), minD(n), maxD(n);
  std::vector<uint8_t> status(n);
  mapCheck(ydorb_map_update_normal_depth(&T, F.pos.data(), F.centre.data(), F.refKf.data(), F.refLevel.data(), F.scaleFactors.data(),
                                         (int32_t)F.scaleFactors.size(), device, normal.data(), minD.data(), maxD.data(), status.data()));
  int updated = 0;
  for (size_t p = 0; p < n; p++) {
    if (status[p] != YDORB_MAP_UPDATED) continue;
    cv::Mat nrm(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) nrm.template at<float>(r) = normal[3 * p + r];
    apply(F.obs.points[p], nrm, minD[p], maxD[p]);
    updated++;
  }
  return updated;
}

}  // namespace adapter
}  // namespace ydorb
#endif
