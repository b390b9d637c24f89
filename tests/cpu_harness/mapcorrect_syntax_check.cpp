// TEST-ONLY: type-checks the three map-correction methods of ydorb::adapter::MapMirror (include/ydorb/mapMirror.hpp) against mock
// declarations of the reference's KeyFrame / MapPoint members and of a Sim3 type they touch (names as in mapmirror_syntax_check.cpp
// and essgraph_syntax_check.cpp).
#include <map>
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/mapMirror.hpp"

struct KeyFrame;
struct MapPoint {
  long unsigned int m_int_correctedByKeyFrameID, m_int_correctedReference;
  bool isBad(); std::map<std::shared_ptr<KeyFrame>, size_t> getObservations(); cv::Mat getPosInWorld(); void setPosInWorld(const cv::Mat&);
  std::shared_ptr<KeyFrame> getReferenceKeyFrame(); void setNormalAndDepth(const cv::Mat&, float, float);
};
struct KeyFrame {
  long unsigned int m_int_keyFrameID;
  std::vector<cv::KeyPoint> m_v_keyPoints; std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  cv::Mat getCameraOriginInWorld(); std::vector<std::shared_ptr<MapPoint>> getMapPointMatches();
  std::vector<std::shared_ptr<KeyFrame>> getVectorCovisibleKeyFrames(); void setBadFlag(); bool isBad();
  cv::Mat getCameraPoseByTransform_c2w(); cv::Mat getCameraPoseByTransform_w2c();
};
struct Quat { double x() const; double y() const; double z() const; double w() const; };
struct Vec { double operator[](int) const; };
struct Sim3 { Quat rotation() const; Vec translation() const; double scale() const; };   // g2o::Sim3's readers

namespace ya = ydorb::adapter;
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
typedef std::map<KF, Sim3> KeyFrameAndPose;

int check(KF currentKF, const KeyFrameAndPose& corrected, const KeyFrameAndPose& nonCorrected, const std::vector<KF>& kfs, const std::vector<MP>& points,
          const std::vector<Sim3>& vScw, std::map<KF, cv::Mat>& tcwBefGBA) {
  ya::MapMirror<KF, MP> mirror(0);
  const auto apply = [](const MP& p, const cv::Mat& pos, const cv::Mat& normal, float mn, float mx) {
    (void)pos;
    if (!normal.empty()) p->setNormalAndDepth(normal, mn, mx);
  };
  int n = mirror.correctLoopPoints(corrected, nonCorrected, currentKF, apply);
  n += mirror.correctAfterEssentialGraph(kfs, points, currentKF, [&](const KF& kf) { return vScw[kf->m_int_keyFrameID]; },
                                         [&](const KF& kf) { return vScw[kf->m_int_keyFrameID]; }, apply);
  n += mirror.correctAfterGlobalBA(kfs, points, [&](const KF& kf) { return tcwBefGBA[kf]; }, [](const KF& kf) { return kf->getCameraPoseByTransform_w2c(); },
                                   apply);
  return n + (int)mirror.verify().pointSlots.size();
}
