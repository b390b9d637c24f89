// TEST-ONLY: type-checks optimizeEssentialGraphImpl of include/ydorb/optimizer.hpp against declarations of the KeyFrame / MapPoint / Map
// members it touches (spellings as listed at the adapter; ORB-SLAM2's names in the project's lowerCamelCase) and a Sim3 type with the
// three accessors of g2o::Sim3.  Built with -fsyntax-only against tests/cpu_harness/mock (OpenCV declarations) and mockrt (Eigen).
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/optimizer.hpp"

struct KeyFrame;
typedef std::shared_ptr<KeyFrame> KFP;
struct MapPoint {
  long int m_int_correctedByKeyFrameID, m_int_correctedReference;
  bool isBad(); cv::Mat getPosInWorld(); void setPosInWorld(const cv::Mat&); void updateNormalAndDepth(); KFP getReferenceKeyFrame();
};
typedef std::shared_ptr<MapPoint> MPP;
struct KeyFrame {
  long int m_int_keyFrameID;
  bool isBad(); cv::Mat getRotation_c2w(); cv::Mat getTranslation_c2w(); void setCameraPoseByTransform_c2w(const cv::Mat&);
  KFP getParent(); bool hasChild(KFP); std::set<KFP> getLoopEdges(); std::vector<KFP> getCovisiblesByWeight(const int&); int getWeight(KFP);
};
struct Map {
  std::mutex m_mutex_updateMap;
  std::vector<KFP> getAllKeyFrames(); std::vector<MPP> getAllMapPoints();
};
struct Frame {};

// the accessors of g2o::Sim3
struct Quat { double x() const; double y() const; double z() const; double w() const; };
struct Vec3 { double operator[](int) const; };
struct Sim3 { const Quat& rotation() const; const Vec3& translation() const; const double& scale() const; };

typedef std::map<KFP, Sim3> KeyFrameAndPose;

void correctLoopTail(std::shared_ptr<Map> map, KFP loopKF, KFP curKF, const KeyFrameAndPose& nonCorrected, const KeyFrameAndPose& corrected,
                     const std::map<KFP, std::set<KFP>>& loopConnections, const bool& fixScale) {
  ydorb::adapter::optimizeEssentialGraphImpl<Frame>(map, loopKF, curKF, nonCorrected, corrected, loopConnections, fixScale);
}
