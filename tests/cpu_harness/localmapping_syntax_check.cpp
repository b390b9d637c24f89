// TEST-ONLY: type-checks include/ydorb/localMapping.hpp against mock declarations of the reference's KeyFrame / MapPoint / Map / Frame
// members it touches (names as in the other adapters' checks).
#include <list>
#include <map>
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/localMapping.hpp"

struct KeyFrame;
struct Map;
struct MapPoint {
  MapPoint(const cv::Mat&, std::shared_ptr<KeyFrame>, std::shared_ptr<Map>);
  void addObservation(std::shared_ptr<KeyFrame>, int); void computeDistinctiveDescriptors(); void updateNormalAndDepth();
};
typedef std::map<unsigned, std::vector<unsigned>> FeatureVector;
struct Frame {
  static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLine, m_flt_baseLineTimesFx;
};
struct KeyFrame {
  std::vector<cv::KeyPoint> m_v_keyPoints; cv::Mat m_cvMat_descriptors; FeatureVector m_bow_keyPointsVec;
  std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors, m_v_scaleFactorSquares; int m_int_keyPointsNum;
  std::shared_ptr<MapPoint> getMapPoint(const int&); void addMapPoint(std::shared_ptr<MapPoint>, const int&);
  cv::Mat getCameraOriginInWorld(); cv::Mat getRotation_c2w(); cv::Mat getTranslation_c2w();
  std::vector<std::shared_ptr<KeyFrame>> getBestCovisibilityKeyFrames(const int&);
};
struct Map { void addMapPoint(std::shared_ptr<MapPoint>); };

namespace ya = ydorb::adapter;
int check(std::shared_ptr<KeyFrame> kf, std::shared_ptr<Map> map, std::list<std::shared_ptr<MapPoint>>& recent) {
  return ya::createNewMapPointsImpl<Frame, std::shared_ptr<KeyFrame>, MapPoint>(ya::matcher(), kf, map, recent, [] { return false; });
}
