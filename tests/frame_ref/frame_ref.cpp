// CPU restatement of the Frame constructor's tail (reference src/frame.cpp:99-100,134-145; ORB-SLAM2's Frame::UndistortKeyPoints,
// ComputeStereoFromRGBD, ComputeImageBounds, AssignFeaturesToGrid, which YDORBSLAM renames) under the arithmetic contract of DESIGN.md
// section 2 ("Frame tail"): the loop of cv::undistortPoints in fp64 with +, -, *, / only, every operation in the written order, built
// with -ffp-contract=off.  TEST INFRASTRUCTURE ONLY: the product never links it.  One keypoint after the other, the grid as the
// per-cell vectors the reference keeps, flattened to a CSR at the end.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ydorb/c_api.h"

namespace {

// returns false when icdist < 0 ended the loop (x0, y0 restored)
bool undistort(const YdCamera& c, float u, float v, float& ou, float& ov) {
  if (c.dist[0] == 0.0f) { ou = u; ov = v; return true; }
  const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
  const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3], k3 = c.dist[4];
  const double ifx = 1.0 / fx, ify = 1.0 / fy;
  double x, y, x0, y0;
  x0 = x = (u - cx) * ifx;
  y0 = y = (v - cy) * ify;
  bool ok = true;
  for (int j = 0; j < c.n_iter; j++) {
    double r2 = x * x + y * y;
    double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
    if (icdist < 0) { x = x0; y = y0; ok = false; break; }
    double deltaX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
    double deltaY = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  ou = (float)(fx * x + cx);
  ov = (float)(fy * y + cy);
  return ok;
}

}  // namespace

extern "C" {

// xy, out [n][2]; status (may be null): OR of YDORB_FRAME_STATUS_ICDIST over the points
void frameref_undistort_points(const YdCamera* cam, const float* xy, int n, float* out, int* status) {
  int st = 0;
  for (int i = 0; i < n; i++)
    if (!undistort(*cam, xy[2 * i], xy[2 * i + 1], out[2 * i], out[2 * i + 1])) st |= YDORB_FRAME_STATUS_ICDIST;
  if (status) *status = st;
}

void frameref_image_bounds(const YdCamera* cam, int w, int h, float* b) {
  if (cam->dist[0] == 0.0f) { b[0] = 0.f; b[1] = (float)w; b[2] = 0.f; b[3] = (float)h; return; }
  const float c[8] = {0.f, 0.f, (float)w, 0.f, 0.f, (float)h, (float)w, (float)h};
  float u[8];
  frameref_undistort_points(cam, c, 4, u, nullptr);
  b[0] = std::fmin(u[0], u[4]); b[1] = std::fmax(u[2], u[6]);
  b[2] = std::fmin(u[1], u[3]); b[3] = std::fmax(u[5], u[7]);
}

// ydorb_frame_tail's host form on host arrays; every output may be null
void frameref_frame_tail(const YdFrameTail* B, YdKeyPoint* kpsUn, float* rightX, float* depth, int32_t* cellStart, int32_t* cellIdx, int32_t* status) {
  const int cap = B->cap;
  for (int f = 0; f < B->n_frames; f++) {
    const int n = B->n[f];
    int st = 0;
    std::vector<YdKeyPoint> un(n);
    for (int i = 0; i < n; i++) {
      const YdKeyPoint kp = B->kps[(size_t)f * cap + i];
      un[i] = kp;
      if (!undistort(B->cam, kp.x, kp.y, un[i].x, un[i].y)) st |= YDORB_FRAME_STATUS_ICDIST;
      float d = -1.0f;
      if (B->depth_type == YDORB_DEPTH_SAMPLES) {
        d = static_cast<const float*>(B->depth)[(size_t)f * cap + i];
      } else if (B->depth_type != YDORB_DEPTH_NONE) {
        const float px = (B->flags & YDORB_FRAME_DEPTH_AT_UNDISTORTED) ? un[i].x : kp.x;
        const float py = (B->flags & YDORB_FRAME_DEPTH_AT_UNDISTORTED) ? un[i].y : kp.y;
        if (px > -1.0f && px < (float)B->depth_w && py > -1.0f && py < (float)B->depth_h) {
          const int col = (int)px, row = (int)py;
          const uint8_t* r = static_cast<const uint8_t*>(B->depth) + (size_t)f * B->depth_frame_stride + (size_t)row * B->depth_row_stride;
          if (B->depth_type == YDORB_DEPTH_U16) d = (float)reinterpret_cast<const uint16_t*>(r)[col] * B->depth_factor;
          else d = reinterpret_cast<const float*>(r)[col];
        } else {
          st |= YDORB_FRAME_STATUS_DEPTH_INDEX;
        }
      }
      float dz = -1.0f, rx = -1.0f;
      if (d > 0) { dz = d; rx = un[i].x - B->bf / d; }
      if (depth) depth[(size_t)f * cap + i] = dz;
      if (rightX) rightX[(size_t)f * cap + i] = rx;
      if (kpsUn) kpsUn[(size_t)f * cap + i] = un[i];
    }
    if (status) status[f] = st;
    if (cellStart && cellIdx) {
      // frame.cpp:249-264,327-336: rounds, and offsets y by min_x
      const float minX = B->bounds[0];
      const float gridWInv = static_cast<float>(64) / (B->bounds[1] - B->bounds[0]);
      const float gridHInv = static_cast<float>(48) / (B->bounds[3] - B->bounds[2]);
      std::vector<std::vector<int>> grid(64 * 48);
      for (int i = 0; i < n; i++) {
        const int lx = (int)roundf((un[i].x - minX) * gridWInv);
        const int ly = (int)roundf((un[i].y - minX) * gridHInv);
        if (lx < 0 || lx >= 64 || ly < 0 || ly >= 48) continue;
        grid[lx * 48 + ly].push_back(i);
      }
      int32_t* cs = cellStart + (size_t)f * (64 * 48 + 1);
      int at = 0;
      for (int c = 0; c < 64 * 48; c++) {
        cs[c] = at;
        for (int idx : grid[c]) cellIdx[(size_t)f * cap + at++] = idx;
      }
      cs[64 * 48] = at;
    }
  }
}

}  // extern "C"
