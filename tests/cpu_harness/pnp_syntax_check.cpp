// TEST-ONLY: type-checks include/ydorb/pnpSolver.hpp against declarations of the Frame / MapPoint members it touches (names as
// optimizePoseImpl uses them: reference src/frame.hpp, mapPoint.hpp).  Built with -fsyntax-only against tests/cpu_harness/mock
// (OpenCV declarations) and mockrt.
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/pnpSolver.hpp"

struct MapPoint {
  bool isBad(); cv::Mat getPosInWorld();
};
struct Frame {
  std::vector<cv::KeyPoint> m_v_keyPoints; std::vector<float> m_v_scaleFactorSquares;
  static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy;
};

typedef std::shared_ptr<MapPoint> MPP;
typedef ydorb::adapter::PnPsolver<Frame, MPP> PnPsolver;

int relocalizeSketch(const Frame& F, std::vector<std::vector<MPP>>& matches) {
  std::vector<PnPsolver*> solvers;
  for (auto& m : matches) {
    PnPsolver* s = new PnPsolver(F, m);
    s->setRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
    solvers.push_back(s);
  }
  std::vector<cv::Mat> Tcw;
  std::vector<char> noMore;
  std::vector<std::vector<bool>> inliers;
  std::vector<int> nInliers;
  ydorb::adapter::pnpIterateBatch(solvers, 5, Tcw, noMore, inliers, nInliers);
  bool bNoMore = false;
  std::vector<bool> vbInliers;
  int n = 0;
  cv::Mat T = solvers[0]->iterate(5, bNoMore, vbInliers, n);
  int found = T.empty() ? 0 : 1;
  for (PnPsolver* s : solvers) delete s;
  return found + n;
}
