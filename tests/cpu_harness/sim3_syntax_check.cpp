// TEST-ONLY: type-checks include/ydorb/sim3Solver.hpp and optimizeSim3Impl of include/ydorb/optimizer.hpp against declarations of the
// KeyFrame / MapPoint / Frame members they touch (names as the other adapters use them: reference src/keyFrame.hpp, mapPoint.hpp,
// frame.hpp).  Built with -fsyntax-only against tests/cpu_harness/mock (OpenCV declarations) and mockrt (Eigen).
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/optimizer.hpp"
#include "../../include/ydorb/sim3Solver.hpp"

struct KeyFrame;
struct MapPoint {
  bool isBad(); cv::Mat getPosInWorld(); int getIdxInKeyFrame(std::shared_ptr<KeyFrame>);
};
struct KeyFrame {
  std::vector<cv::KeyPoint> m_v_keyPoints; std::vector<float> m_v_scaleFactorSquares, m_v_invScaleFactorSquares;
  cv::Mat getRotation_c2w(); cv::Mat getTranslation_c2w(); std::vector<std::shared_ptr<MapPoint>> getMatchedMapPointsVec();
};
struct Frame { static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy; };

typedef std::shared_ptr<KeyFrame> KFP;
typedef std::shared_ptr<MapPoint> MPP;

int loopClosingCheck(KFP kf1, KFP kf2, std::vector<MPP>& matched12) {
  ydorb::adapter::Sim3Solver<KFP, MPP, Frame> solver(kf1, kf2, matched12, true);
  solver.setRansacParameters(0.99, 20, 300);
  bool noMore = false;
  std::vector<bool> inliers;
  int nInliers = 0;
  cv::Mat T12 = solver.iterate(5, noMore, inliers, nInliers);
  cv::Mat R = solver.getEstimatedRotation(), t = solver.getEstimatedTranslation();
  float s = solver.getEstimatedScale();
  double S12[8] = {0, 0, 0, 1, t.at<float>(0), t.at<float>(1), t.at<float>(2), s};
  (void)R; (void)T12;
  return ydorb::adapter::optimizeSim3Impl<Frame>(kf1, kf2, matched12, S12, 10.0f, true);
}
