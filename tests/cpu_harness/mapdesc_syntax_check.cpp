// TEST-ONLY: type-checks the resident-descriptor methods of ydorb::adapter::MapMirror (include/ydorb/mapMirror.hpp) against mock
// declarations of the reference's KeyFrame / MapPoint members they touch (names as in mapmirror_syntax_check.cpp, plus
// m_cvMat_descriptors and the m_descriptor a caller's apply sets).
#include <map>
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/mapMirror.hpp"

struct KeyFrame;
struct MapPoint {
  cv::Mat m_descriptor;
  bool isBad(); std::map<std::shared_ptr<KeyFrame>, size_t> getObservations(); cv::Mat getPosInWorld();
  std::shared_ptr<KeyFrame> getReferenceKeyFrame();
};
struct KeyFrame {
  long unsigned int m_int_keyFrameID;
  cv::Mat m_cvMat_descriptors;
  std::vector<cv::KeyPoint> m_v_keyPoints; std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  cv::Mat getCameraOriginInWorld(); std::vector<std::shared_ptr<MapPoint>> getMapPointMatches();
  std::vector<std::shared_ptr<KeyFrame>> getVectorCovisibleKeyFrames(); void setBadFlag(); bool isBad();
};

namespace ya = ydorb::adapter;
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
int check(KF kf, MP mp, const std::vector<MP>& points) {
  ya::MapMirror<KF, MP> mirror(0);
  mirror.enableDescriptors(1 << 16, 1 << 18);
  mirror.touch(kf); mirror.touchDescriptors(kf); mirror.touch(mp);
  mirror.flush();
  const int n = mirror.computeDistinctiveDescriptors(points, [](const MP& p, const KF& k, size_t idx, const cv::Mat& row) {
    p->m_descriptor = row.clone();
    (void)k; (void)idx;
  });
  const ya::MapMirror<KF, MP>::Difference d = mirror.verifyDescriptors();
  mirror.forget(mp); mirror.forget(kf);
  mirror.clear();
  return n + (int)d.pointSlots.size() + (int)d.keyFrameSlots.size() + (mirror.descriptorsEnabled() ? 1 : 0);
}
