// gfx950 HIP kernels of the Frame constructor's tail (reference src/frame.cpp:99-100,134-145; ORB-SLAM2's Frame::UndistortKeyPoints,
// ComputeStereoFromRGBD, ComputeImageBounds and AssignFeaturesToGrid, which YDORBSLAM renames; DESIGN.md sections 2 "Frame tail" and 6h).
//   k_frame_tail        one lane per (frame, keypoint): undistortion in fp64, depth look-up, right x;
//   k_undistort_points  the same undistortion for a bare list of points (ydorb_undistort_points, the corners of ydorb_image_bounds);
//   k_frame_grid        one workgroup per frame: the 64x48 grid of the undistorted keypoints as a CSR, with the matcher's cell rule.
// Arithmetic contract: +, -, *, / only, every operation a single IEEE operation in the written order (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grid_build.hip.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace frame {

constexpr int kThreads = 256;
enum { kDepthNone = 0, kDepthU16 = 1, kDepthF32 = 2, kDepthSamples = 3 };   // == YDORB_DEPTH_*
enum { kStatusDepthIndex = 1, kStatusIcdist = 4 };                          // == YDORB_FRAME_STATUS_*
enum { kFlagDepthAtUndistorted = 1 };                                       // == YDORB_FRAME_DEPTH_AT_UNDISTORTED

struct CamDev {   // == YdCamera
  float fx, fy, cx, cy, k1, k2, p1, p2, k3;
  int nIter;
};

// cv::undistortPoints(mat, mat, K, D, Mat(), K) for one point: n_iter fixed iterations, no epsilon test.  False when 1 + k1 r2 + k2 r4
// + k3 r6 turned negative: the normalised point is then the undistorted one's start value, as in cvUndistortPointsInternal.
__device__ __forceinline__ bool undistort_point(const CamDev& c, float u, float v, float& ou, float& ov) {
  if (c.k1 == 0.0f) { ou = u; ov = v; return true; }   // the reference's early exit looks at k1 alone
  const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy, k1 = c.k1, k2 = c.k2, p1 = c.p1, p2 = c.p2, k3 = c.k3;
  const double ifx = 1.0 / fx, ify = 1.0 / fy;
  const double x0 = ((double)u - cx) * ifx, y0 = ((double)v - cy) * ify;
  double x = x0, y = y0;
  bool ok = true;
  for (int it = 0; it < c.nIter; it++) {
    const double r2 = x * x + y * y;
    const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
    if (icdist < 0) { x = x0; y = y0; ok = false; break; }
    const double dX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
    const double dY = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
    x = (x0 - dX) * icdist;
    y = (y0 - dY) * icdist;
  }
  ou = (float)(fx * x + cx);
  ov = (float)(fy * y + cy);
  return ok;
}

struct TailArgs {
  const KeyPointDev* kps;   // [nFrames][cap] as extracted
  const int* n;             // [nFrames] device counts
  int nFrames, cap;
  const void* depth;        // image of frame f at depth + f * frameStride bytes, row r at + r * rowStride bytes; samples: float [nFrames][cap]
  int depthType, w, h;
  long long rowStride, frameStride;
  float factor;
  CamDev cam;
  float bf;
  int flags;
  KeyPointDev* kpsUn;       // outputs, each may be null
  float* rightX;
  float* depthOut;
  int* status;              // [nFrames], cleared by the driver
};

__global__ __launch_bounds__(kThreads) void k_frame_tail(const TailArgs a) {
  const int f = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= min(a.n[f], a.cap)) return;
  const size_t slot = (size_t)f * a.cap + i;
  const KeyPointDev kp = a.kps[slot];
  float ux, uy;   // plain registers: a keypoint record whose fields are written through references goes to LDS
  int st = 0;
  if (!undistort_point(a.cam, kp.x, kp.y, ux, uy)) st |= kStatusIcdist;
  if (a.kpsUn) a.kpsUn[slot] = KeyPointDev{ux, uy, kp.size, kp.angle, kp.response, kp.octave, kp.class_id};
  if (a.rightX || a.depthOut) {
    float d = -1.0f;
    if (a.depthType == kDepthSamples) {
      d = static_cast<const float*>(a.depth)[slot];
    } else if (a.depthType != kDepthNone) {
      // (int) truncates toward zero, so everything above -1 lands on pixel 0; NaN fails both comparisons
      const float px = (a.flags & kFlagDepthAtUndistorted) ? ux : kp.x, py = (a.flags & kFlagDepthAtUndistorted) ? uy : kp.y;
      if (px > -1.0f && px < (float)a.w && py > -1.0f && py < (float)a.h) {
        const uint8_t* row = static_cast<const uint8_t*>(a.depth) + (size_t)f * a.frameStride + (size_t)(int)py * a.rowStride;
        d = a.depthType == kDepthU16 ? __fmul_rn((float)reinterpret_cast<const uint16_t*>(row)[(int)px], a.factor)
                                     : reinterpret_cast<const float*>(row)[(int)px];
      } else {
        st |= kStatusDepthIndex;
      }
    }
    const bool has = d > 0.0f;
    if (a.depthOut) a.depthOut[slot] = has ? d : -1.0f;
    if (a.rightX) a.rightX[slot] = has ? __fsub_rn(ux, __fdiv_rn(a.bf, d)) : -1.0f;
  }
  if (st && a.status) atomicOr(&a.status[f], st);
}

// xy / out: [n][2] floats; status (may be null, cleared by the driver): one word, the OR of kStatusIcdist over the points
__global__ __launch_bounds__(kThreads) void k_undistort_points(const CamDev cam, const float2* __restrict__ xy, int n, float2* __restrict__ out,
                                                               int* __restrict__ status) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float2 p = xy[i];
  float2 q;
  const bool ok = undistort_point(cam, p.x, p.y, q.x, q.y);
  out[i] = q;
  if (!ok && status) atomicOr(status, kStatusIcdist);
}

struct GridArgs {
  const KeyPointDev* kpsUn;   // [nFrames][cap]
  const int* n;
  int cap;
  float minX, gridWInv, gridHInv;
  int* cellStart;             // [nFrames][kGridCells + 1]
  int* cellIdx;               // [nFrames][cap]
};

__global__ __launch_bounds__(256) void k_frame_grid(const GridArgs a) {
  __shared__ int hist[kGridCells];
  __shared__ int wsum[4];
  extern __shared__ int16_t cellOf[];  // [cap]
  const int f = blockIdx.x;
  FrameDev F{};
  F.kps = a.kpsUn + (size_t)f * a.cap; F.nPtr = a.n + f;
  F.minX = a.minX; F.gridWInv = a.gridWInv; F.gridHInv = a.gridHInv;
  F.cellStart = a.cellStart + (size_t)f * (kGridCells + 1); F.cellIdx = a.cellIdx + (size_t)f * a.cap;
  grid_build<false>(F, a.cap, hist, wsum, cellOf);
}

}  // namespace frame
}  // namespace ydorb
