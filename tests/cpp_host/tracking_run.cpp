// TEST-ONLY: EXECUTES include/ydorb/tracking.hpp (searchLocalPointsImpl) on the GPU against stand-ins of the reference's Frame / MapPoint
// classes that carry real data, and dumps every map point's track fields, visibility counter and last-seen frame and the frame's
// map-point slots.  tests/test_tracking_adapter_gpu.py builds the scenario and replays it through the ctypes path.  OpenCV is the
// functional mock of tests/cpu_harness/mockrt.
//   tracking_run scenario.bin out.bin
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/ydorb/tracking.hpp"

namespace {

struct Reader {
  FILE* f;
  explicit Reader(const char* path) : f(fopen(path, "rb")) { if (!f) { perror(path); exit(2); } }
  ~Reader() { fclose(f); }
  template <class T> T get() { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "scenario truncated\n"); exit(2); } return v; }
  template <class T> void get(T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scenario truncated\n"); exit(2); } }
};

cv::Mat readMat32(Reader& R, int rows, int cols) { cv::Mat m(rows, cols, CV_32F); R.get(m.ptr<float>(), (size_t)rows * cols); return m; }

struct MapPoint {
  int index = -1;
  cv::Mat pos, normal, desc;
  float minDist = 0, maxDist = 0;      // m_flt_minDistance / m_flt_maxDistance
  bool bad = false;
  int nObs = 0, visible = 0;
  long int m_int_lastSeenInFrameID = -1;
  bool m_b_isTrackInView = false;
  int m_int_trackScaleLevel = -7;
  float m_flt_trackViewCos = -7.f, m_flt_trackProjX = -7.f, m_flt_trackProjY = -7.f, m_flt_trackProjRightX = -7.f;
  bool isBad() { return bad; }
  int getObservationsNum() { return nObs; }
  cv::Mat getDescriptor() { return desc.clone(); }
  cv::Mat getPosInWorld() { return pos.clone(); }
  cv::Mat getNormal() { return normal.clone(); }
  float getMinDistanceInvariance() { return 0.8f * minDist; }
  float getMaxDistanceInvariance() { return 1.2f * maxDist; }
  float getMaxDistance() { return maxDist; }
  void increaseVisible(int n = 1) { visible += n; }
};
struct Frame {
  std::vector<cv::KeyPoint> m_v_keyPoints;
  cv::Mat m_cvMat_descriptors, m_cvMat_T_c2w, origin;
  std::vector<float> m_v_rightXcords, m_v_scaleFactors;
  std::vector<std::shared_ptr<MapPoint>> m_v_sptrMapPoints;
  long int m_int_ID = 0;
  float m_flt_logScaleFactor = 0;
  cv::Mat getCameraOriginInWorld() { return origin.clone(); }
  static float m_flt_minX, m_flt_maxX, m_flt_minY, m_flt_maxY, m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLine, m_flt_baseLineTimesFx;
};
float Frame::m_flt_minX, Frame::m_flt_maxX, Frame::m_flt_minY, Frame::m_flt_maxY, Frame::m_flt_fx, Frame::m_flt_fy, Frame::m_flt_cx, Frame::m_flt_cy,
    Frame::m_flt_baseLine, Frame::m_flt_baseLineTimesFx;

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: tracking_run scenario.bin out.bin\n"); return 2; }
  Reader R(argv[1]);
  float cam[9];
  R.get(cam, 9);
  Frame::m_flt_fx = cam[0]; Frame::m_flt_fy = cam[1]; Frame::m_flt_cx = cam[2]; Frame::m_flt_cy = cam[3]; Frame::m_flt_baseLineTimesFx = cam[4];
  Frame::m_flt_minX = cam[5]; Frame::m_flt_maxX = cam[6]; Frame::m_flt_minY = cam[7]; Frame::m_flt_maxY = cam[8];
  Frame::m_flt_baseLine = 0.f;
  Frame frame;
  const int nLevels = R.get<int32_t>();
  frame.m_v_scaleFactors.resize(nLevels);
  R.get(frame.m_v_scaleFactors.data(), nLevels);
  frame.m_flt_logScaleFactor = R.get<float>();
  frame.m_int_ID = R.get<int32_t>();
  const float th = R.get<float>(), ratio = R.get<float>();
  frame.m_cvMat_T_c2w = readMat32(R, 4, 4);
  frame.origin = readMat32(R, 3, 1);
  const int n = R.get<int32_t>();
  frame.m_v_keyPoints.resize(n);
  R.get(reinterpret_cast<unsigned char*>(frame.m_v_keyPoints.data()), (size_t)n * sizeof(cv::KeyPoint));
  frame.m_cvMat_descriptors.create(std::max(n, 1), 32, CV_8U);
  R.get(frame.m_cvMat_descriptors.data, (size_t)n * 32);
  frame.m_v_rightXcords.resize(n);
  R.get(frame.m_v_rightXcords.data(), n);
  const int nAll = R.get<int32_t>();
  std::vector<std::shared_ptr<MapPoint>> all;
  for (int i = 0; i < nAll; i++) {
    auto mp = std::make_shared<MapPoint>();
    mp->index = i;
    mp->pos = readMat32(R, 3, 1); mp->normal = readMat32(R, 3, 1);
    mp->minDist = R.get<float>(); mp->maxDist = R.get<float>();
    mp->desc.create(1, 32, CV_8U);
    R.get(mp->desc.data, 32);
    const int32_t rec[4] = {R.get<int32_t>(), R.get<int32_t>(), R.get<int32_t>(), R.get<int32_t>()};
    mp->bad = rec[0] != 0; mp->nObs = rec[1]; mp->m_int_lastSeenInFrameID = rec[2]; mp->visible = rec[3];
    all.push_back(mp);
  }
  std::vector<int32_t> slot(n);
  R.get(slot.data(), n);
  frame.m_v_sptrMapPoints.resize(n);
  for (int i = 0; i < n; i++) if (slot[i] >= 0) frame.m_v_sptrMapPoints[i] = all[slot[i]];
  const int nLocal = R.get<int32_t>();
  std::vector<int32_t> localIdx(nLocal);
  R.get(localIdx.data(), nLocal);
  std::vector<std::shared_ptr<MapPoint>> local;
  for (int i : localIdx) local.push_back(all[i]);

  namespace ya = ydorb::adapter;
  const int32_t matches = ya::searchLocalPointsImpl(ya::matcher(), frame, local, th, ratio);

  FILE* f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  fwrite(&matches, 4, 1, f);
  for (const auto& mp : all) {
    const float fl[4] = {mp->m_flt_trackProjX, mp->m_flt_trackProjY, mp->m_flt_trackProjRightX, mp->m_flt_trackViewCos};
    const int32_t in[4] = {mp->m_int_trackScaleLevel, mp->m_b_isTrackInView ? 1 : 0, mp->visible, (int32_t)mp->m_int_lastSeenInFrameID};
    fwrite(fl, 4, 4, f); fwrite(in, 4, 4, f);
  }
  for (int i = 0; i < n; i++) { const int32_t s = frame.m_v_sptrMapPoints[i] ? frame.m_v_sptrMapPoints[i]->index : -1; fwrite(&s, 4, 1, f); }
  fclose(f);
  return 0;
}
