// TEST-ONLY: type-checks the RGB-D constructor bodies of include/ydorb/frame.hpp against mock declarations of the reference's Frame
// members they touch (names as the header lists them).
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/orbExtractor.hpp"
#include "../../include/ydorb/frame.hpp"

struct Frame {
  std::vector<cv::KeyPoint> m_v_keyPoints, m_v_rightKeyPoints; cv::Mat m_cvMat_descriptors, m_cvMat_rightDescriptors, m_cvMat_distCoef;
  std::vector<float> m_v_rightXcords, m_v_depth; int m_int_keyPointsNum;
  std::vector<std::size_t> m_v_grid[64][48];
  std::shared_ptr<YDORBSLAM::OrbExtractor> m_sptr_leftOrbExtractor, m_sptr_rightOrbExtractor;
  static float m_flt_minX, m_flt_maxX, m_flt_minY, m_flt_maxY, m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLine, m_flt_baseLineTimesFx;
};

namespace ya = ydorb::adapter;
int check(Frame& f, const cv::Mat& gray, const cv::Mat& imDepth) {
  std::vector<cv::KeyPoint> raw;
  ya::computeImageBoundsImpl(f, gray);
  int st = ya::undistortKeyPointsImpl(f, &raw);
  st |= ya::computeStereoFromRGBDImpl(f, imDepth, &raw);
  st |= ya::computeStereoFromRGBDImpl(f, imDepth, nullptr, 1.0f, false);
  ya::assignKeyPointsToGridImpl(f);
  st |= ya::finishRGBDFrameImpl(f, gray, imDepth, true, &raw, 1.0f, YDORB_FRAME_DEPTH_AT_UNDISTORTED);
  return st + ya::computeStereoMatchesImpl(f);
}
