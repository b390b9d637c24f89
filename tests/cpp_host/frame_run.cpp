// TEST-ONLY: EXECUTES the RGB-D constructor bodies of include/ydorb/frame.hpp on the GPU against a stand-in Frame that carries data
// (tests/test_frame_adapter_gpu.py builds it against the storage-carrying OpenCV stand-in and libydorb.so).
//   frame_run <in> <out>
// in:  int32 w, h, depth kind (0 none, 1 uint16, 2 float), n_features; float K[4], dist[5], bf, depth factor; gray [h][w]; depth [h][w]
// out: two records, (1) finishRGBDFrameImpl, (2) extractAndCompute + the four separate bodies with the sample-gather path, followed by
//      right_x / depth of the image path.  A record: int32 n, status; raw keypoints, undistorted keypoints [n][28]; descriptors
//      [n][32]; right_x, depth [n]; bounds [4]; cell_start [3073]; cell_idx [cell_start[3072]].
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "frame_run_cv.hpp"
#include "../../include/ydorb/orbExtractor.hpp"
#include "../../include/ydorb/frame.hpp"

struct Frame {
  std::vector<cv::KeyPoint> m_v_keyPoints, m_v_rawKeyPoints;
  cv::Mat m_cvMat_descriptors, m_cvMat_distCoef;
  std::vector<float> m_v_rightXcords, m_v_depth;
  int m_int_keyPointsNum = 0;
  std::vector<std::size_t> m_v_grid[64][48];
  std::shared_ptr<YDORBSLAM::OrbExtractor> m_sptr_leftOrbExtractor;
  static float m_flt_minX, m_flt_maxX, m_flt_minY, m_flt_maxY, m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLineTimesFx;
};
float Frame::m_flt_minX, Frame::m_flt_maxX, Frame::m_flt_minY, Frame::m_flt_maxY, Frame::m_flt_fx, Frame::m_flt_fy, Frame::m_flt_cx, Frame::m_flt_cy,
    Frame::m_flt_baseLineTimesFx;

namespace ya = ydorb::adapter;

static void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
static void wr(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { fprintf(stderr, "short output\n"); exit(2); } }

static void dump(FILE* o, const Frame& f, int status) {
  const int32_t n = (int32_t)f.m_v_keyPoints.size(), st = status;
  if (f.m_int_keyPointsNum != n || (int)f.m_v_rawKeyPoints.size() != n || (int)f.m_v_rightXcords.size() != n || (int)f.m_v_depth.size() != n ||
      f.m_cvMat_descriptors.rows != n) { fprintf(stderr, "inconsistent frame\n"); exit(3); }
  wr(o, &n, 4); wr(o, &st, 4);
  wr(o, f.m_v_rawKeyPoints.data(), sizeof(cv::KeyPoint) * n);
  wr(o, f.m_v_keyPoints.data(), sizeof(cv::KeyPoint) * n);
  for (int r = 0; r < n; r++) wr(o, f.m_cvMat_descriptors.ptr<unsigned char>(r), 32);
  wr(o, f.m_v_rightXcords.data(), 4 * (size_t)n); wr(o, f.m_v_depth.data(), 4 * (size_t)n);
  const float b[4] = {Frame::m_flt_minX, Frame::m_flt_maxX, Frame::m_flt_minY, Frame::m_flt_maxY};
  wr(o, b, sizeof b);
  std::vector<int32_t> cs(64 * 48 + 1, 0), ci;
  for (int ix = 0; ix < 64; ix++)
    for (int iy = 0; iy < 48; iy++) {
      cs[ix * 48 + iy] = (int32_t)ci.size();
      for (std::size_t k : f.m_v_grid[ix][iy]) ci.push_back((int32_t)k);
    }
  cs[64 * 48] = (int32_t)ci.size();
  wr(o, cs.data(), 4 * cs.size()); wr(o, ci.data(), 4 * ci.size());
}

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 1;
  int32_t hd[4];
  float par[11];
  rd(in, hd, sizeof hd); rd(in, par, sizeof par);
  const int w = hd[0], h = hd[1], kind = hd[2];
  cv::Mat gray(h, w, CV_8U), depth;
  rd(in, gray.data, (size_t)w * h);
  if (kind == 1) { depth = frame_run::mat16(h, w); rd(in, depth.data, (size_t)w * h * 2); }
  if (kind == 2) { depth = cv::Mat(h, w, CV_32F); rd(in, depth.data, (size_t)w * h * 4); }
  fclose(in);
  Frame::m_flt_fx = par[0]; Frame::m_flt_fy = par[1]; Frame::m_flt_cx = par[2]; Frame::m_flt_cy = par[3]; Frame::m_flt_baseLineTimesFx = par[9];
  const float factor = par[10];
  try {
    Frame f;
    f.m_cvMat_distCoef = cv::Mat(5, 1, CV_32F);
    for (int i = 0; i < 5; i++) f.m_cvMat_distCoef.at<float>(i) = par[4 + i];
    f.m_sptr_leftOrbExtractor = std::make_shared<YDORBSLAM::OrbExtractor>(hd[3], 1.2f, 8, 20, 7);
    f.m_sptr_leftOrbExtractor->setPyramidDownload(false);
    // (1) the single call; the bounds start out wrong and the first-frame flag must repair them
    Frame::m_flt_minX = Frame::m_flt_minY = -1.f; Frame::m_flt_maxX = Frame::m_flt_maxY = -1.f;
    int st = ya::finishRGBDFrameImpl(f, gray, depth, true, &f.m_v_rawKeyPoints, factor);
    dump(out, f, st);
    // (2) the reference's own sequence, one body after the other
    Frame g;
    g.m_cvMat_distCoef = f.m_cvMat_distCoef;
    g.m_sptr_leftOrbExtractor = f.m_sptr_leftOrbExtractor;
    Frame::m_flt_minX = Frame::m_flt_minY = -1.f; Frame::m_flt_maxX = Frame::m_flt_maxY = -1.f;
    g.m_sptr_leftOrbExtractor->extractAndCompute(gray, g.m_v_keyPoints, g.m_cvMat_descriptors);
    g.m_int_keyPointsNum = (int)g.m_v_keyPoints.size();
    st = ya::undistortKeyPointsImpl(g, &g.m_v_rawKeyPoints);
    st |= ya::computeStereoFromRGBDImpl(g, depth, &g.m_v_rawKeyPoints, factor, true);
    ya::computeImageBoundsImpl(g, gray);
    ya::assignKeyPointsToGridImpl(g);
    dump(out, g, st);
    (void)ya::computeStereoFromRGBDImpl(g, depth, &g.m_v_rawKeyPoints, factor, false);   // the image path
    wr(out, g.m_v_rightXcords.data(), 4 * g.m_v_rightXcords.size()); wr(out, g.m_v_depth.data(), 4 * g.m_v_depth.size());
  } catch (const std::exception& e) {
    fprintf(stderr, "frame_run: %s\n", e.what());
    return 4;
  }
  fclose(out);
  return 0;
}
