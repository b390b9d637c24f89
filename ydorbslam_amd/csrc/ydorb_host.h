// Shared host helpers of the C-ABI library (error text, device guard).
#pragma once
#include <cstdint>
struct ydorb_extractor;
namespace ydorb {
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
// YDORB_OK if `device` is a usable gfx950 HIP device and is now current; YDORB_ERR_NO_DEVICE otherwise.
// The product has no CPU path: callers propagate the error.
int require_device(int device);
// Device view of the image pyramid an extractor built in its last call (m_v_imagePyramid, read by Frame::computeStereoMatches,
// reference src/frame.cpp:366,412-427): ROI origin of every level in frame 0, the distance between frames, level geometry and
// the scale tables.  Defined in orb_extractor.hip.
struct PyramidView {
  int device, nLevels, frames;
  long long frameStride;
  const uint8_t* roi[8];
  int w[8], h[8], pitch[8];
  float scale[8], invScale[8];
  int quota[8];   // keypoints per level the extractor returns at most (m_v_keyPointsNumsPerLevel)
  void* stream;
};
int extractor_pyramid_view(const ydorb_extractor* e, PyramidView* out);
// The BA's blocked dense Cholesky for another driver's system (defined in ba_solver.hip, whose translation unit holds the kernels):
// queues on `stream` (a hipStream_t) the factorisation of S + the forward substitution and the backward solve, over device memory the
// caller owns.  S is [n][n] row-major, n a multiple of kCholTile, lower tiles and whole diagonal tiles set; it is overwritten by the
// factor.  diagL / diagInv hold n * kCholTile doubles each, b / yv / x hold n; b is consumed.  status[0] must be 0 on entry and is raised
// when a pivot is not positive (x is then not a solution).  Nothing is synchronised.  YDORB_ERR_UNSUPPORTED past chol_max_rows().
constexpr int kCholTile = 32;
int chol_max_rows();
int chol_factor_solve(void* stream, double* S, double* diagL, double* diagInv, int n, int* status, double* b, double* yv, double* x);
}  // namespace ydorb
