// TEST-ONLY: type-checks the map-maintenance adapters (include/ydorb/mapPoint.hpp, keyFrame.hpp and keyFrameCullingImpl of
// localMapping.hpp) against mock declarations of the reference's KeyFrame / MapPoint members they touch (names as in the other
// adapters' checks).
#include <map>
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/keyFrame.hpp"
#include "../../include/ydorb/localMapping.hpp"
#include "../../include/ydorb/mapPoint.hpp"

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
int check(KF kf, const std::vector<MP>& points, float thDepth) {
  const int n = ya::updateNormalAndDepthBatch<KF, MP>(points, [](const MP& mp, const cv::Mat& normal, float mn, float mx) { mp->setNormalAndDepth(normal, mn, mx); });
  const std::map<KF, int> counter = ya::covisibilityCounter<KF, MP>(kf);
  const std::vector<KF> flagged = ya::keyFrameCullingImpl<KF, MP>(kf, thDepth, 0);
  return n + (int)counter.size() + (int)flagged.size();
}
