// Drop-in adapter for the relocalisation PnPsolver (ORB-SLAM2 src/PnPsolver.cc, which YDORBSLAM renames to pnpSolver.*; DESIGN.md
// section 6d) on top of ydorb_pnp_ransac.  A class template over the reference's Frame / MapPoint types with the reference's public
// members:
//   PnPsolver(const Frame& F, const vector<MapPoint*>& vpMapPointMatches)
//   void setRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
//                            float epsilon = 0.4, float th2 = 5.991)
//   cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)   (4x4 float Tcw, or an empty Mat)
// The constructor reads F.m_v_keyPoints (the undistorted keypoints), F.m_v_scaleFactorSquares[octave] as the level sigma^2
// (mvLevelSigma2), the static m_flt_fx / m_flt_fy / m_flt_cx / m_flt_cy, and each kept map point's getPosInWorld(); null and bad map
// points are skipped and mvKeyPointIndices kept.  The loop condition defaults to ORB-SLAM2's
//   while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)
// (setLoopOr(false) selects the && variant).
// iterate(n) draws all the 4-point sets of its call with the reference's RandomInt (process-global rand(), available-index copy,
// swap-remove) BEFORE the call, because the GPU evaluates them in parallel: with ||, a call draws max(maxIts - mnIterations, n) sets,
// with && min(n, maxIts - mnIterations).  The reference draws inside its loop and stops at the hypothesis whose Refine succeeds, so when a call returns at hypothesis k
// of the H it drew, this adapter has consumed 4 * (H - 1 - k) more rand() values than the reference.  Everything else - the
// hypotheses, the returned pose, bNoMore, the inliers, the best state carried between calls - is the reference's.
// pnpIterateBatch() runs iterate(n) on several solvers (the relocalisation candidates) in ONE ydorb_pnp_ransac call.
#ifndef YDORB_ADAPTER_PNPSOLVER_HPP
#define YDORB_ADAPTER_PNPSOLVER_HPP

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core.hpp>

#include "c_api.h"

namespace ydorb {
namespace adapter {

// DUtils::Random::RandomInt
inline int pnpRandomInt(int min, int max) {
  const int d = max - min + 1;
  return int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}

template <class FrameT, class MapPointPtr>
class PnPsolver {
 public:
  PnPsolver(const FrameT& F, const std::vector<MapPointPtr>& vpMapPointMatches, int device = 0)
      : device_(device), nMatches_((int)vpMapPointMatches.size()) {
    for (int i = 0; i < nMatches_; i++) {
      const MapPointPtr& mp = vpMapPointMatches[i];
      if (!mp) continue;
      if (mp->isBad()) continue;
      const cv::KeyPoint& kp = F.m_v_keyPoints[i];
      P2D.push_back(kp.pt.x); P2D.push_back(kp.pt.y);
      sigma2_.push_back(F.m_v_scaleFactorSquares[kp.octave]);
      const cv::Mat Pos = mp->getPosInWorld();
      Xw.push_back(Pos.at<float>(0)); Xw.push_back(Pos.at<float>(1)); Xw.push_back(Pos.at<float>(2));
      mvKeyPointIndices.push_back(i);
    }
    K_[0] = FrameT::m_flt_fx; K_[1] = FrameT::m_flt_fy; K_[2] = FrameT::m_flt_cx; K_[3] = FrameT::m_flt_cy;
    setRansacParameters();
  }

  void setRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                           float th2 = 5.991f) {
    const int N = (int)mvKeyPointIndices.size();
    int nMinInliers = N * epsilon;
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    minInliers_ = nMinInliers;
    if (epsilon < (float)minInliers_ / N) epsilon = (float)minInliers_ / N;
    int nIterations;
    if (minInliers_ == N) nIterations = 1;
    else nIterations = (int)std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));
    maxIts_ = std::max(1, std::min(nIterations, maxIterations));
    maxErr.resize(sigma2_.size());
    for (size_t i = 0; i < sigma2_.size(); i++) maxErr[i] = sigma2_[i] * th2;
    iterations_ = 0; bestInliers_ = 0;
    bestMask.assign(std::max(N, 1), 0);
    std::fill(bestTcw_, bestTcw_ + 12, 0.f);
  }
  void setLoopOr(bool loopOr) { loopOr_ = loopOr; }

  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    std::vector<PnPsolver*> one(1, this);
    std::vector<cv::Mat> T;
    std::vector<char> noMore;
    std::vector<std::vector<bool>> inl;
    std::vector<int> nInl;
    pnpIterate(one, nIterations, T, noMore, inl, nInl, device_);
    bNoMore = noMore[0] != 0;
    vbInliers = inl[0];
    nInliers = nInl[0];
    return T[0];
  }

  // draws this solver's sets for one iterate(n) call and fills the problem; finish() reads it back
  void prepare(int nIterations, YdPnpProblem& P) {
    const int N = (int)mvKeyPointIndices.size();
    const int chunk = std::max(1, nIterations);
    lastQuads.clear();
    if (N >= minInliers_ && N >= 4) {
      // one iterate(n) call: with ||, until mnIterations >= maxIts and n have run; with &&, n or what maxIts leaves
      const int H = loopOr_ ? std::max(maxIts_ - iterations_, chunk) : std::min(chunk, std::max(0, maxIts_ - iterations_));
      std::vector<int> avail;
      for (int h = 0; h < H; h++) {
        avail.resize(N);
        for (int i = 0; i < N; i++) avail[i] = i;   // mvAllIndices
        for (int i = 0; i < 4; i++) {
          const int r = pnpRandomInt(0, (int)avail.size() - 1);
          lastQuads.push_back(avail[r]);
          avail[r] = avail.back();
          avail.pop_back();
        }
      }
    }
    mask_.assign(std::max(N, 1), 0);
    std::memset(&P, 0, sizeof P);
    P.n = N; P.min_inliers = minInliers_; P.max_its = maxIts_; P.loop_or = loopOr_ ? 1 : 0;
    P.Xw = Xw.data(); P.P2D = P2D.data(); P.max_err = maxErr.data();
    std::memcpy(P.K, K_, sizeof K_);
    P.n_hyp = (int)lastQuads.size() / 4; P.quads = lastQuads.data();
    P.next_hyp = iterations_; P.best_inliers = bestInliers_; P.best_mask = bestMask.data();
    std::memcpy(P.best_Tcw, bestTcw_, sizeof bestTcw_);
    P.inliers = mask_.data();
  }
  cv::Mat finish(const YdPnpProblem& P, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    const int N = (int)mvKeyPointIndices.size();
    iterations_ = P.next_hyp; bestInliers_ = P.best_inliers;
    std::memcpy(bestTcw_, P.best_Tcw, sizeof bestTcw_);
    bNoMore = P.no_more != 0 || (N >= minInliers_ && N < 4);   // fewer than four matches: no set can be drawn
    vbInliers.clear();
    nInliers = 0;
    if (P.ret_how == YDORB_PNP_NONE) return cv::Mat();
    vbInliers.assign(nMatches_, false);
    for (int i = 0; i < N; i++)
      if (mask_[i]) vbInliers[mvKeyPointIndices[i]] = true;
    nInliers = P.n_inliers;
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 4; c++) T.at<float>(r, c) = P.Tcw[4 * r + c];
      T.at<float>(3, r) = 0.f;
    }
    T.at<float>(3, 3) = 1.f;
    return T;
  }

  // runs iterate(nIterations) on every solver in one ydorb_pnp_ransac call
  static void pnpIterate(const std::vector<PnPsolver*>& solvers, int nIterations, std::vector<cv::Mat>& Tcw, std::vector<char>& bNoMore,
                         std::vector<std::vector<bool>>& vbInliers, std::vector<int>& nInliers, int device = 0) {
    const size_t n = solvers.size();
    std::vector<YdPnpProblem> P(n);
    for (size_t i = 0; i < n; i++) solvers[i]->prepare(nIterations, P[i]);
    if (n && ydorb_pnp_ransac(P.data(), (int32_t)n, std::max(1, nIterations), device) != YDORB_OK)
      throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
    Tcw.assign(n, cv::Mat()); bNoMore.assign(n, 0); vbInliers.assign(n, std::vector<bool>()); nInliers.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
      bool nm = false;
      Tcw[i] = solvers[i]->finish(P[i], nm, vbInliers[i], nInliers[i]);
      bNoMore[i] = nm;
    }
  }

  // the flat problem ydorb_pnp_ransac receives, and the sets the last iterate() drew
  std::vector<float> Xw, P2D, maxErr;
  std::vector<int> mvKeyPointIndices, lastQuads;
  std::vector<uint8_t> bestMask;
  int maxIterations() const { return maxIts_; }
  int minInliers() const { return minInliers_; }

 private:
  int device_, nMatches_;
  float K_[4];
  std::vector<float> sigma2_;
  std::vector<uint8_t> mask_;
  bool loopOr_ = true;
  int minInliers_ = 8, maxIts_ = 1, iterations_ = 0, bestInliers_ = 0;
  float bestTcw_[12] = {0};
};

// Tracking::relocalize's batch: iterate(n) on every candidate's solver in one GPU call
template <class Solver>
void pnpIterateBatch(const std::vector<Solver*>& solvers, int nIterations, std::vector<cv::Mat>& Tcw, std::vector<char>& bNoMore,
                     std::vector<std::vector<bool>>& vbInliers, std::vector<int>& nInliers, int device = 0) {
  Solver::pnpIterate(solvers, nIterations, Tcw, bNoMore, vbInliers, nInliers, device);
}

}  // namespace adapter
}  // namespace ydorb
#endif
