// Drop-in adapter for the loop-closure Sim3Solver (ORB-SLAM2 src/Sim3Solver.cc, which YDORBSLAM renames) on top
// of ydorb_sim3_ransac.  A class template over the reference's KeyFrame / MapPoint types with the reference's public members:
//   Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*>& vpMatched12, const bool bFixScale = true)
//   void setRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
//   cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)
//   cv::Mat getEstimatedRotation(), getEstimatedTranslation(); float getEstimatedScale()
// The constructor keeps the reference's pair predicates and does its float camera-frame transforms on the host, in the written order of
// DESIGN.md section 2 ("Sim3 RANSAC"): each product exact in double, the three terms summed in double, rounded once to float.
// iterate(n) draws its n triples with the reference's RandomInt (process-global rand(), available-index copy, swap-remove) BEFORE the
// call, because the GPU evaluates them in parallel.  The reference draws inside its loop and stops at the hypothesis that returns, so
// when a call returns at hypothesis k of n, this adapter has consumed 3 * (n - 1 - k) more rand() values than the reference.  Everything
// else - the hypotheses, the returned one, bNoMore, the inliers, the best state carried between calls - is the reference's.
#ifndef YDORB_ADAPTER_SIM3SOLVER_HPP
#define YDORB_ADAPTER_SIM3SOLVER_HPP

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core.hpp>

#include "c_api.h"

namespace ydorb {
namespace adapter {

// DUtils::Random::RandomInt
inline int randomInt(int min, int max) {
  const int d = max - min + 1;
  return int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}

// rows of a 3x3 float cv::Mat times a 3-vector plus t, in the contract's order
inline void cameraPoint(const cv::Mat& R, const cv::Mat& t, const cv::Mat& Xw, float* out) {
  for (int r = 0; r < 3; r++) {
    const double s = ((double)R.at<float>(r, 0) * (double)Xw.at<float>(0) + (double)R.at<float>(r, 1) * (double)Xw.at<float>(1)) +
                     (double)R.at<float>(r, 2) * (double)Xw.at<float>(2);
    out[r] = (float)s + t.at<float>(r);
  }
}

template <class KeyFramePtr, class MapPointPtr, class FrameT>
class Sim3Solver {
 public:
  Sim3Solver(KeyFramePtr kf1, KeyFramePtr kf2, const std::vector<MapPointPtr>& matched12, const bool fixScale = true, int device = 0)
      : fixScale_(fixScale), device_(device), n1_((int)matched12.size()) {
    const std::vector<MapPointPtr> mps1 = kf1->getMatchedMapPointsVec();
    const cv::Mat R1 = kf1->getRotation_c2w(), t1 = kf1->getTranslation_c2w(), R2 = kf2->getRotation_c2w(), t2 = kf2->getTranslation_c2w();
    K_[0] = FrameT::m_flt_fx; K_[1] = FrameT::m_flt_fy; K_[2] = FrameT::m_flt_cx; K_[3] = FrameT::m_flt_cy;
    for (int i1 = 0; i1 < n1_; i1++) {
      if (!matched12[i1]) continue;
      const MapPointPtr mp1 = mps1[i1], mp2 = matched12[i1];
      if (!mp1) continue;
      if (mp1->isBad() || mp2->isBad()) continue;
      const int idx1 = mp1->getIdxInKeyFrame(kf1), idx2 = mp2->getIdxInKeyFrame(kf2);
      if (idx1 < 0 || idx2 < 0) continue;
      const float sigma1 = kf1->m_v_scaleFactorSquares[kf1->m_v_keyPoints[idx1].octave];
      const float sigma2 = kf2->m_v_scaleFactorSquares[kf2->m_v_keyPoints[idx2].octave];
      maxErr1.push_back((float)(size_t)(9.210 * sigma1));   // mvnMaxError is a vector<size_t>
      maxErr2.push_back((float)(size_t)(9.210 * sigma2));
      indices1.push_back(i1);
      float c[3];
      cameraPoint(R1, t1, mp1->getPosInWorld(), c);
      X1.insert(X1.end(), c, c + 3);
      cameraPoint(R2, t2, mp2->getPosInWorld(), c);
      X2.insert(X2.end(), c, c + 3);
    }
    toImage(X1, P1);
    toImage(X2, P2);
    setRansacParameters();
  }

  void setRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    minInliers_ = minInliers;
    const int N = (int)indices1.size();
    const float epsilon = (float)minInliers / N;
    int n;
    if (minInliers == N) n = 1;
    else {
      const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
      n = std::isfinite(v) && std::fabs(v) < 2147483647.0 ? (int)v : std::numeric_limits<int>::min();
    }
    maxIts_ = std::max(1, std::min(n, maxIterations));
    iterations_ = 0; bestInliers_ = 0;
    std::fill(best_, best_ + 13, 0.f);
  }

  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers.assign(n1_, false);
    nInliers = 0;
    const int N = (int)indices1.size();
    lastTriples.clear();
    if (N >= minInliers_ && N >= 3) {
      const int n = std::max(0, std::min(nIterations, maxIts_ - iterations_));
      std::vector<int> avail;
      for (int h = 0; h < n; h++) {
        avail.resize(N);
        for (int i = 0; i < N; i++) avail[i] = i;   // mvAllIndices
        for (int i = 0; i < 3; i++) {
          const int r = randomInt(0, (int)avail.size() - 1);
          lastTriples.push_back(avail[r]);
          avail[r] = avail.back();
          avail.pop_back();
        }
      }
    }
    YdSim3Problem P;
    std::memset(&P, 0, sizeof P);
    std::vector<uint8_t> mask(std::max(N, 1));
    P.n = N; P.fix_scale = fixScale_; P.min_inliers = minInliers_; P.max_its = maxIts_;
    P.X1 = X1.data(); P.X2 = X2.data(); P.P1 = P1.data(); P.P2 = P2.data(); P.max_err1 = maxErr1.data(); P.max_err2 = maxErr2.data();
    std::memcpy(P.K1, K_, sizeof K_); std::memcpy(P.K2, K_, sizeof K_);
    P.n_hyp = (int)lastTriples.size() / 3; P.triples = lastTriples.data();
    P.next_hyp = iterations_; P.best_inliers = bestInliers_;
    std::memcpy(P.best_T12, best_, sizeof best_);
    P.inliers = mask.data();
    if (ydorb_sim3_ransac(&P, 1, std::max(1, nIterations), device_) != YDORB_OK) throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
    iterations_ = P.next_hyp; bestInliers_ = P.best_inliers;
    std::memcpy(best_, P.best_T12, sizeof best_);
    bNoMore = P.no_more != 0 || (N >= minInliers_ && N < 3);   // fewer than three pairs: no triple can be drawn
    if (P.ret_hyp < 0) return cv::Mat();
    for (int i = 0; i < N; i++)
      if (mask[i]) { vbInliers[indices1[i]] = true; nInliers++; }
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) T.at<float>(r, c) = best_[12] * best_[3 * r + c];   // sR, as ComputeSim3 forms it
      T.at<float>(r, 3) = best_[9 + r];
      T.at<float>(3, r) = 0.f;
    }
    T.at<float>(3, 3) = 1.f;
    return T;
  }

  cv::Mat getEstimatedRotation() const {
    cv::Mat R(3, 3, CV_32F);
    for (int k = 0; k < 9; k++) R.at<float>(k / 3, k % 3) = best_[k];
    return R;
  }
  cv::Mat getEstimatedTranslation() const {
    cv::Mat t(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) t.at<float>(k) = best_[9 + k];
    return t;
  }
  float getEstimatedScale() const { return best_[12]; }

  // the flat problem ydorb_sim3_ransac receives, and the triples the last iterate() drew
  std::vector<float> X1, X2, P1, P2, maxErr1, maxErr2;
  std::vector<int> indices1, lastTriples;
  int maxIterations() const { return maxIts_; }

 private:
  void toImage(const std::vector<float>& X, std::vector<float>& P) const {   // FromCameraToImage
    P.resize(X.size() / 3 * 2);
    for (size_t i = 0; i < X.size() / 3; i++) {
      const float invz = 1.0f / X[3 * i + 2];
      P[2 * i] = K_[0] * (X[3 * i] * invz) + K_[2];
      P[2 * i + 1] = K_[1] * (X[3 * i + 1] * invz) + K_[3];
    }
  }
  bool fixScale_;
  int device_, n1_;
  float K_[4];
  int minInliers_ = 6, maxIts_ = 1, iterations_ = 0, bestInliers_ = 0;
  float best_[13] = {0};
};

}  // namespace adapter
}  // namespace ydorb
#endif
