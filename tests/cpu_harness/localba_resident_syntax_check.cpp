// TEST-ONLY: type-checks the resident overload localBundleAdjustImpl<Frame>(mirror, ...) of include/ydorb/optimizer.hpp and
// MapMirror::localBaGraph (include/ydorb/mapMirror.hpp) against mock declarations of the reference's KeyFrame / MapPoint / Map / Frame
// members they touch (names as in adapter_syntax_check.cpp and mapmirror_syntax_check.cpp, plus m_v_invScaleFactorSquares for the
// sigma table and the setter a caller's apply uses).  Built with the declaration-only OpenCV mock and the Eigen stand-in of mockrt.
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/mapMirror.hpp"
#include "../../include/ydorb/optimizer.hpp"

struct KeyFrame;
struct MapPoint {
  bool isBad(); std::map<std::shared_ptr<KeyFrame>, size_t> getObservations(); cv::Mat getPosInWorld(); void setPosInWorld(const cv::Mat&);
  std::shared_ptr<KeyFrame> getReferenceKeyFrame(); void eraseObservation(std::shared_ptr<KeyFrame>);
  void setNormalAndDepth(const cv::Mat&, float, float);
};
struct Frame { static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLineTimesFx; };
struct KeyFrame {
  long int m_int_keyFrameID, m_int_localBAForKeyFrameID;
  std::vector<cv::KeyPoint> m_v_keyPoints; std::vector<float> m_v_rightXcords, m_v_scaleFactors, m_v_invScaleFactorSquares; cv::Mat m_cvMat_descriptors;
  cv::Mat getCameraOriginInWorld(); cv::Mat getCameraPoseByTransform_c2w(); void setCameraPoseByTransform_c2w(cv::Mat);
  std::vector<std::shared_ptr<MapPoint>> getMapPointMatches(); std::vector<std::shared_ptr<KeyFrame>> getOrderedConnectedKeyFrames();
  void eraseMatchedMapPoint(std::shared_ptr<MapPoint>); bool isBad();
};
struct Map { std::mutex m_mutex_updateMap; };

namespace ya = ydorb::adapter;
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
int check(KF kf, std::shared_ptr<Map> map, bool& stop) {
  ya::MapMirror<KF, MP> mirror(0);
  mirror.enableDescriptors(); mirror.enableFeatures();
  const ya::MapMirror<KF, MP>::LocalBaGraph G = mirror.localBaGraph(std::vector<KF>(1, kf));
  ya::localBundleAdjustImpl<Frame>(mirror, kf, map, &stop, [](const MP& p, const cv::Mat& normal, float mn, float mx) { p->setNormalAndDepth(normal, mn, mx); });
  return (int)G.poseKF.size() + (int)G.pointMP.size() + (int)G.edgeKF.size() + G.graph.n_fixed;
}
