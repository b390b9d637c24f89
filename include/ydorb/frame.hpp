// Drop-in body for YDORBSLAM::Frame::computeStereoMatches() (reference src/frame.cpp:362-477) on top of the ydorb C ABI.
// In src/frame.cpp the member function becomes
//     void Frame::computeStereoMatches(){ ydorb::adapter::computeStereoMatchesImpl(*this); }
// with m_sptr_leftOrbExtractor / m_sptr_rightOrbExtractor being the adapter class of include/ydorb/orbExtractor.hpp (their
// pyramids stay in HBM: setPyramidDownload(false) is enough for this path).  Everything the function read is passed as it
// is: the undistorted keypoints of both images, both descriptor matrices, baseline and baseline x fx.
//
// Drop-in bodies for the tail of the RGB-D constructor (reference src/frame.cpp:99-100,134-145; ORB-SLAM2's Frame::UndistortKeyPoints,
// ComputeStereoFromRGBD, ComputeImageBounds, AssignFeaturesToGrid, which YDORBSLAM renames; DESIGN.md sections 2 "Frame tail" and 6h):
// computeImageBoundsImpl, undistortKeyPointsImpl, computeStereoFromRGBDImpl, assignKeyPointsToGridImpl, each one call of the C ABI's
// "Frame construction" section, and finishRGBDFrameImpl, which replaces extractOrb and all four with ONE ydorb_extract_rgbd call
// ("RGB-D frame construction").
// Assumed spellings, as in the other adapters: Frame m_v_keyPoints (the undistorted keypoints once undistortKeyPoints has run: the
// frame keeps one vector, so the raw ones go to a vector the caller names), m_int_keyPointsNum, m_cvMat_descriptors, m_v_rightXcords,
// m_v_depth, m_cvMat_distCoef (CV_32F, k1 k2 p1 p2 [k3]), m_v_grid[64][48] (per-cell index vectors with clear() / push_back()),
// m_sptr_leftOrbExtractor (include/ydorb/orbExtractor.hpp), the static m_flt_fx .. m_flt_cy, m_flt_baseLineTimesFx and m_flt_minX ..
// m_flt_maxY.  The grid element sizes (frame.cpp:99-100) stay where the constructor computes them from the bounds.
#ifndef YDORB_ADAPTER_FRAME_HPP
#define YDORB_ADAPTER_FRAME_HPP

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core.hpp>

#include "c_api.h"
#include "orbMatcher.hpp"

namespace ydorb {
namespace adapter {

// flags = 0 reproduces the reference as written (including the left index that lags behind from the first keypoint that
// leaves the loop body early, frame.cpp:462); YDORB_STEREO_INDEX_BY_KEYPOINT indexes descriptor row and output slot by the
// keypoint itself.  Returns the status bits of ydorb_stereo_matches.
template <class FrameT>
int computeStereoMatchesImpl(FrameT& f, int flags = 0, ydorb_matcher_t* m = matcher()) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(YdKeyPoint), "cv::KeyPoint must be the 28-byte POD the ABI mirrors");
  const int nl = (int)f.m_v_keyPoints.size(), nr = (int)f.m_v_rightKeyPoints.size();
  f.m_v_rightXcords.assign(f.m_int_keyPointsNum, -1.0f);   // :363-364
  f.m_v_depth.assign(f.m_int_keyPointsNum, -1.0f);
  if (nl == 0 || nr == 0) return 0;
  if (nl != f.m_int_keyPointsNum) throw std::runtime_error("ydorb: m_int_keyPointsNum differs from m_v_keyPoints.size()");   // frame.cpp:88 sets it so
  cv::Mat dl = f.m_cvMat_descriptors.isContinuous() ? f.m_cvMat_descriptors : f.m_cvMat_descriptors.clone();
  cv::Mat dr = f.m_cvMat_rightDescriptors.isContinuous() ? f.m_cvMat_rightDescriptors : f.m_cvMat_rightDescriptors.clone();
  const int32_t cl = nl, cr = nr;
  YdStereoSide L{f.m_sptr_leftOrbExtractor->handle(), 0, 1, reinterpret_cast<const YdKeyPoint*>(f.m_v_keyPoints.data()), dl.data, &cl, nl, 0};
  YdStereoSide R{f.m_sptr_rightOrbExtractor->handle(), 0, 1, reinterpret_cast<const YdKeyPoint*>(f.m_v_rightKeyPoints.data()), dr.data, &cr, nr, 0};
  int32_t kept = 0, status = 0;
  if (ydorb_stereo_matches(m, &L, &R, 1, FrameT::m_flt_baseLineTimesFx, FrameT::m_flt_baseLine, flags, f.m_v_rightXcords.data(), f.m_v_depth.data(),
                           &kept, &status, nullptr) != YDORB_OK)
    throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
  return status;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The RGB-D constructor's tail
// ---------------------------------------------------------------------------------------------------------------------------------
inline void frameCheck(int rc) {
  if (rc != YDORB_OK) throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
}

// K and the distortion coefficients as the ABI reads them; pinhole = true leaves the coefficients zero (keypoints that are
// undistorted already pass through the tail unchanged: k1 == 0 is the copy exit)
template <class FrameT>
inline YdCamera frameCamera(const FrameT& f, bool pinhole = false, int nIter = 5) {
  YdCamera c;
  std::memset(&c, 0, sizeof c);
  c.fx = FrameT::m_flt_fx; c.fy = FrameT::m_flt_fy; c.cx = FrameT::m_flt_cx; c.cy = FrameT::m_flt_cy;
  c.n_iter = nIter;
  if (!pinhole) {
    const int n = (int)f.m_cvMat_distCoef.total();
    for (int i = 0; i < n && i < 5; i++) c.dist[i] = f.m_cvMat_distCoef.template at<float>(i);
  }
  return c;
}

inline int depthTypeOf(const cv::Mat& d) {
  if (d.empty()) return YDORB_DEPTH_NONE;
  if (d.type() == CV_32F) return YDORB_DEPTH_F32;
#ifdef CV_16UC1
  if (d.type() == CV_16UC1) return YDORB_DEPTH_U16;
#endif
  throw std::runtime_error("ydorb: the depth image must be CV_32F (or CV_16UC1 with its factor)");
}

// the fields of a YdFrameTail that do not depend on the step: one frame of n keypoints
template <class FrameT>
inline YdFrameTail frameTailOf(const FrameT& f, const std::vector<cv::KeyPoint>& kps, const int32_t* n, bool pinhole, int device) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(YdKeyPoint), "cv::KeyPoint must be the 28-byte POD the ABI mirrors");
  YdFrameTail t;
  std::memset(&t, 0, sizeof t);
  t.kps = reinterpret_cast<const YdKeyPoint*>(kps.data()); t.n = n; t.n_frames = 1; t.cap = *n;
  t.cam = frameCamera(f, pinhole); t.bf = FrameT::m_flt_baseLineTimesFx; t.device = device;
  t.bounds[0] = FrameT::m_flt_minX; t.bounds[1] = FrameT::m_flt_maxX; t.bounds[2] = FrameT::m_flt_minY; t.bounds[3] = FrameT::m_flt_maxY;
  return t;
}

// Frame::computeImageBounds (frame.cpp:99-100): the four image corners through the undistortion, on the device
template <class FrameT>
void computeImageBoundsImpl(FrameT& f, const cv::Mat& image, int device = 0) {
  const YdCamera c = frameCamera(f);
  float b[4];
  frameCheck(ydorb_image_bounds(&c, image.cols, image.rows, b, device));
  FrameT::m_flt_minX = b[0]; FrameT::m_flt_maxX = b[1]; FrameT::m_flt_minY = b[2]; FrameT::m_flt_maxY = b[3];
}

// Frame::undistortKeyPoints (frame.cpp:134-145): m_v_keyPoints become the undistorted ones; `raw`, when given, receives what they were.
// Returns the status bits of ydorb_frame_tail.
template <class FrameT>
int undistortKeyPointsImpl(FrameT& f, std::vector<cv::KeyPoint>* raw = nullptr, int device = 0) {
  if (raw) *raw = f.m_v_keyPoints;
  const int32_t n = (int32_t)f.m_v_keyPoints.size();
  if (n == 0) return 0;
  const YdFrameTail t = frameTailOf(f, f.m_v_keyPoints, &n, false, device);
  std::vector<cv::KeyPoint> un(n);
  int32_t status = 0;
  frameCheck(ydorb_frame_tail(&t, reinterpret_cast<YdKeyPoint*>(un.data()), nullptr, nullptr, nullptr, nullptr, &status, nullptr));
  f.m_v_keyPoints.swap(un);
  return status;
}

// Frame::computeStereoFromRGBD (frame.cpp:134-145) behind undistortKeyPoints.  raw != nullptr: the depth pixel is the RAW keypoint's
// (ORB-SLAM2's mvKeys), and the undistorted x of right_x is recomputed from it on the device; raw == nullptr: the frame's one
// vector indexes the image (YDORB_FRAME_DEPTH_AT_UNDISTORTED's result).  gather = true reads the (at most n) depth pixels on the host and
// uploads n floats instead of the image.  depthFactor applies to a CV_16UC1 image only.  Returns the status bits.
template <class FrameT>
int computeStereoFromRGBDImpl(FrameT& f, const cv::Mat& imDepth, const std::vector<cv::KeyPoint>* raw = nullptr, float depthFactor = 1.0f,
                              bool gather = true, int device = 0) {
  const std::vector<cv::KeyPoint>& idx = raw ? *raw : f.m_v_keyPoints;
  const int32_t n = (int32_t)idx.size();
  f.m_v_rightXcords.assign(n, -1.0f);
  f.m_v_depth.assign(n, -1.0f);
  if (n == 0) return 0;
  YdFrameTail t = frameTailOf(f, idx, &n, raw == nullptr, device);
  const int type = depthTypeOf(imDepth);
  std::vector<float> samples;
  int32_t hostStatus = 0;
  if (type != YDORB_DEPTH_NONE && gather) {
    samples.assign(n, -1.0f);
    for (int i = 0; i < n; i++) {
      const float px = idx[i].pt.x, py = idx[i].pt.y;
      if (!(px > -1.0f && px < (float)imDepth.cols && py > -1.0f && py < (float)imDepth.rows)) { hostStatus |= YDORB_FRAME_STATUS_DEPTH_INDEX; continue; }
      const unsigned char* row = imDepth.data + (size_t)(int)py * imDepth.step;
      samples[i] = type == YDORB_DEPTH_U16 ? (float)reinterpret_cast<const uint16_t*>(row)[(int)px] * depthFactor
                                           : reinterpret_cast<const float*>(row)[(int)px];
    }
    t.depth = samples.data(); t.depth_type = YDORB_DEPTH_SAMPLES;
  } else if (type != YDORB_DEPTH_NONE) {
    t.depth = imDepth.data; t.depth_type = type; t.depth_w = imDepth.cols; t.depth_h = imDepth.rows;
    t.depth_row_stride = (int64_t)imDepth.step; t.depth_factor = depthFactor;
  }
  int32_t status = 0;
  frameCheck(ydorb_frame_tail(&t, nullptr, f.m_v_rightXcords.data(), f.m_v_depth.data(), nullptr, nullptr, &status, nullptr));
  return status | hostStatus;
}

// the per-cell vectors from the CSR: indices ascend in a cell, as push_back left them
template <class FrameT>
inline void fillGridFromCsr(FrameT& f, const int32_t* cellStart, const int32_t* cellIdx) {
  for (int ix = 0; ix < 64; ix++)
    for (int iy = 0; iy < 48; iy++) {
      auto& cell = f.m_v_grid[ix][iy];
      cell.clear();
      for (int k = cellStart[ix * 48 + iy]; k < cellStart[ix * 48 + iy + 1]; k++) cell.push_back(cellIdx[k]);
    }
}

// Frame::assignKeyPointsToGrid (frame.cpp:134-145, cell rule :249-264,327-336) over the undistorted m_v_keyPoints
template <class FrameT>
void assignKeyPointsToGridImpl(FrameT& f, int device = 0) {
  const int32_t n = (int32_t)f.m_v_keyPoints.size();
  std::vector<int32_t> cellStart(64 * 48 + 1, 0), cellIdx(n > 0 ? n : 1);
  if (n > 0) {
    const YdFrameTail t = frameTailOf(f, f.m_v_keyPoints, &n, true, device);
    frameCheck(ydorb_frame_tail(&t, nullptr, nullptr, nullptr, cellStart.data(), cellIdx.data(), nullptr, nullptr));
  }
  fillGridFromCsr(f, cellStart.data(), cellIdx.data());
}

// extractOrb + undistortKeyPoints + computeStereoFromRGBD + assignKeyPointsToGrid of the RGB-D constructor as ONE ydorb_extract_rgbd
// call (upload, extraction, tail, one read-back, one synchronise).  firstFrame = true computes the image bounds before it, as the
// constructor does for its first frame.  An empty imDepth gives the monocular tail.  `raw`, when given, receives the keypoints as
// extracted; flags: YDORB_FRAME_DEPTH_AT_UNDISTORTED.  Returns the status bits.
template <class FrameT>
int finishRGBDFrameImpl(FrameT& f, const cv::Mat& gray, const cv::Mat& imDepth, bool firstFrame = false, std::vector<cv::KeyPoint>* raw = nullptr,
                        float depthFactor = 1.0f, int flags = 0, int device = 0) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(YdKeyPoint), "cv::KeyPoint must be the 28-byte POD the ABI mirrors");
  CV_Assert(gray.type() == CV_8UC1);
  if (firstFrame) computeImageBoundsImpl(f, gray, device);
  ydorb_extractor_t* ex = f.m_sptr_leftOrbExtractor->handle();
  const int cap = ydorb_extractor_max_keypoints(ex);
  const YdCamera cam = frameCamera(f);
  const float bounds[4] = {FrameT::m_flt_minX, FrameT::m_flt_maxX, FrameT::m_flt_minY, FrameT::m_flt_maxY};
  std::vector<cv::KeyPoint> kr(cap), ku(cap);
  cv::Mat desc(cap, 32, CV_8U);
  std::vector<float> rx(cap), dz(cap);
  std::vector<int32_t> cellStart(64 * 48 + 1, 0), cellIdx(cap);
  int32_t n = 0, status = 0;
  const int type = depthTypeOf(imDepth);
  frameCheck(ydorb_extract_rgbd(ex, gray.data, gray.cols, gray.rows, (int32_t)gray.step, type == YDORB_DEPTH_NONE ? nullptr : imDepth.data, type,
                                (int32_t)imDepth.step, depthFactor, &cam, FrameT::m_flt_baseLineTimesFx, bounds, flags,
                                reinterpret_cast<YdKeyPoint*>(kr.data()), reinterpret_cast<YdKeyPoint*>(ku.data()), desc.data, rx.data(), dz.data(),
                                cellStart.data(), cellIdx.data(), cap, &n, &status));
  kr.resize(n); ku.resize(n); rx.resize(n); dz.resize(n);
  f.m_int_keyPointsNum = n;
  f.m_v_keyPoints.swap(ku);
  if (raw) raw->swap(kr);
  if (n == 0) f.m_cvMat_descriptors = cv::Mat();
  else f.m_cvMat_descriptors = desc.rowRange(0, n).clone();
  f.m_v_rightXcords.swap(rx);
  f.m_v_depth.swap(dz);
  fillGridFromCsr(f, cellStart.data(), cellIdx.data());
  return status;
}

}  // namespace adapter
}  // namespace ydorb
#endif
