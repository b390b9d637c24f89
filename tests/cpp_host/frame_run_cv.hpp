// TEST-ONLY additions to the storage-carrying OpenCV stand-in (tests/cpu_harness/mockrt/opencv2/core.hpp) for frame_run.cpp: the 16-bit
// depth type, which the stand-in's element-size table does not know, as a matrix built by hand.
#pragma once
#include <opencv2/core.hpp>
#define CV_16UC1 2
namespace frame_run {
inline cv::Mat mat16(int rows, int cols) {
  cv::Mat m;
  m.rows = rows; m.cols = cols; m.type_ = CV_16UC1; m.step = (size_t)cols * 2;
  m.buf = std::make_shared<std::vector<unsigned char>>((size_t)rows * m.step + 64, 0);
  m.data = m.buf->data();
  return m;
}
}  // namespace frame_run
