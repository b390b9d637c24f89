// TEST-ONLY: type-checks the keyframe-row methods of ydorb::adapter::MapMirror (include/ydorb/mapMirror.hpp) and
// updateLocalKeyFramesImpl / updateLocalPointsImpl (include/ydorb/tracking.hpp) against mock declarations of the reference's Frame /
// KeyFrame / MapPoint members they touch (names as in mapmirror_syntax_check.cpp and the headers' "assumed spellings" lists).
#include <map>
#include <memory>
#include <set>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/mapMirror.hpp"
#include "../../include/ydorb/tracking.hpp"

struct KeyFrame;
struct MapPoint {
  long unsigned int m_int_trackReferenceForFrameID;
  bool isBad(); std::map<std::shared_ptr<KeyFrame>, size_t> getObservations(); cv::Mat getPosInWorld();
  std::shared_ptr<KeyFrame> getReferenceKeyFrame();
};
struct KeyFrame {
  long unsigned int m_int_keyFrameID, m_int_trackReferenceForFrameID;
  std::vector<cv::KeyPoint> m_v_keyPoints; std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  cv::Mat getCameraOriginInWorld(); std::vector<std::shared_ptr<MapPoint>> getMapPointMatches();
  std::vector<std::shared_ptr<KeyFrame>> getVectorCovisibleKeyFrames(); void setBadFlag(); bool isBad();
  std::vector<std::shared_ptr<KeyFrame>> getBestCovisibilityKeyFrames(const int& n); std::set<std::shared_ptr<KeyFrame>> getChildren();
  std::shared_ptr<KeyFrame> getParent();
};
struct Frame {
  long unsigned int m_int_ID;
  std::vector<std::shared_ptr<MapPoint>> m_v_sptrMapPoints;
  std::shared_ptr<KeyFrame> m_sptr_referenceKeyFrame;
};

namespace ya = ydorb::adapter;
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
int check(KF kf, Frame& frame, std::vector<KF>& localKeyFrames, std::vector<MP>& localMapPoints, KF& referenceKeyFrame) {
  ya::MapMirror<KF, MP> mirror(0);
  mirror.touchRow(kf); mirror.touchEntry(kf, 3);
  mirror.flush();
  std::vector<size_t> badIndices;
  const std::map<KF, int> counter = mirror.keyFrameCounter(frame.m_v_sptrMapPoints, &badIndices);
  std::vector<uint8_t> seen;
  const std::vector<MP> points = mirror.localPoints(localKeyFrames, frame.m_v_sptrMapPoints, &seen);
  const std::vector<int32_t> differ = mirror.verifyRows();
  ya::updateLocalKeyFramesImpl(mirror, frame, localKeyFrames, referenceKeyFrame);
  const std::vector<uint8_t> flags = ya::updateLocalPointsImpl(mirror, frame, localKeyFrames, localMapPoints);
  mirror.forget(kf);
  return (int)(counter.size() + points.size() + differ.size() + flags.size() + seen.size() + badIndices.size());
}
