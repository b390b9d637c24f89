// TEST-ONLY: type-checks include/ydorb/tracking.hpp against mock declarations of the reference's Frame / MapPoint members it touches
// (names as in the other adapters' checks; getMaxDistance() is the one-line getter the header asks the reference to add).
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/tracking.hpp"

struct MapPoint {
  bool m_b_isTrackInView; int m_int_trackScaleLevel; float m_flt_trackViewCos, m_flt_trackProjX, m_flt_trackProjY, m_flt_trackProjRightX;
  long int m_int_lastSeenInFrameID;
  bool isBad(); int getObservationsNum(); cv::Mat getDescriptor(); cv::Mat getPosInWorld(); cv::Mat getNormal();
  float getMaxDistanceInvariance(); float getMinDistanceInvariance(); float getMaxDistance(); void increaseVisible(int n = 1);
};
struct Frame {
  std::vector<cv::KeyPoint> m_v_keyPoints; cv::Mat m_cvMat_descriptors; std::vector<float> m_v_rightXcords, m_v_scaleFactors;
  std::vector<std::shared_ptr<MapPoint>> m_v_sptrMapPoints; cv::Mat m_cvMat_T_c2w; long int m_int_ID; float m_flt_logScaleFactor;
  cv::Mat getCameraOriginInWorld();
  static float m_flt_minX, m_flt_maxX, m_flt_minY, m_flt_maxY, m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLine, m_flt_baseLineTimesFx;
};

namespace ya = ydorb::adapter;
int check(Frame& f, std::vector<std::shared_ptr<MapPoint>>& local) {
  float table[7];
  ya::levelRatioTable(f.m_flt_logScaleFactor, 8, table);
  const std::vector<bool> in = ya::isInCameraFrustumBatch(f, local, 0.5f);
  return ya::searchLocalPointsImpl(ya::matcher(), f, local, 1.0f, 0.8f) + (int)in.size();
}
