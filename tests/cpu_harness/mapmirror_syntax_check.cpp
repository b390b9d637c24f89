// TEST-ONLY: type-checks ydorb::adapter::MapMirror (include/ydorb/mapMirror.hpp) against mock declarations of the reference's
// KeyFrame / MapPoint members it touches (names as in mapmaint_syntax_check.cpp).
#include <map>
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/mapMirror.hpp"

struct KeyFrame;
struct MapPoint {
  bool isBad(); std::map<std::shared_ptr<KeyFrame>, size_t> getObservations(); cv::Mat getPosInWorld();
  std::shared_ptr<KeyFrame> getReferenceKeyFrame(); void setNormalAndDepth(const cv::Mat&, float, float);
};
struct KeyFrame {
  long unsigned int m_int_keyFrameID;
  std::vector<cv::KeyPoint> m_v_keyPoints; std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  cv::Mat getCameraOriginInWorld(); std::vector<std::shared_ptr<MapPoint>> getMapPointMatches();
  std::vector<std::shared_ptr<KeyFrame>> getVectorCovisibleKeyFrames(); void setBadFlag(); bool isBad();
};

namespace ya = ydorb::adapter;
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
int check(KF kf, MP mp, const std::vector<MP>& points, float thDepth) {
  ya::MapMirror<KF, MP> mirror(0);
  mirror.touch(kf); mirror.touch(mp); mirror.touchPosition(mp);
  mirror.flush();
  const int n = mirror.updateNormalAndDepth(points, [](const MP& p, const cv::Mat& normal, float mn, float mx) { p->setNormalAndDepth(normal, mn, mx); });
  const std::map<KF, int> counter = mirror.covisibilityCounter(kf);
  const std::vector<KF> flagged = mirror.keyFrameCulling(kf, thDepth);
  const ya::MapMirror<KF, MP>::Difference d = mirror.verify();
  mirror.forget(mp); mirror.forget(kf);
  mirror.clear();
  return n + (int)counter.size() + (int)flagged.size() + (int)d.pointSlots.size() + mirror.slotOf(kf) + mirror.slotOf(mp);
}
