// TEST-ONLY: EXECUTES include/ydorb/localMapping.hpp (createNewMapPointsImpl) on the GPU against stand-ins of the reference's KeyFrame /
// MapPoint / Map classes that carry real data, and dumps the MapPoints it created with their observation pairs, in creation order.
// tests/test_triangulate_adapter_gpu.py builds the scenario and replays the loop through the ctypes path.  OpenCV is the functional mock
// of tests/cpu_harness/mockrt.
//   localmapping_run scenario.bin out.bin
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <memory>
#include <vector>

#include "../../include/ydorb/localMapping.hpp"

namespace {

struct Reader {
  FILE* f;
  explicit Reader(const char* path) : f(fopen(path, "rb")) { if (!f) { perror(path); exit(2); } }
  ~Reader() { fclose(f); }
  template <class T> T get() { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "scenario truncated\n"); exit(2); } return v; }
  template <class T> void get(T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scenario truncated\n"); exit(2); } }
};

struct KeyFrame;
struct Map;
struct MapPoint {
  cv::Mat pos;
  std::vector<std::pair<int, int>> obs;   // (keyframe index, keypoint index) in addObservation order
  int distinctive = 0, updates = 0;
  MapPoint(const cv::Mat& p, std::shared_ptr<KeyFrame>, std::shared_ptr<Map>) : pos(p.clone()) {}
  void addObservation(std::shared_ptr<KeyFrame> kf, int idx);
  void computeDistinctiveDescriptors() { distinctive++; }
  void updateNormalAndDepth() { updates++; }
};
typedef std::map<unsigned, std::vector<unsigned>> FeatureVector;
struct Frame {
  static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLine, m_flt_baseLineTimesFx;
};
float Frame::m_flt_fx, Frame::m_flt_fy, Frame::m_flt_cx, Frame::m_flt_cy, Frame::m_flt_baseLine, Frame::m_flt_baseLineTimesFx;
struct KeyFrame {
  int index = -1;
  cv::Mat R, t, O, m_cvMat_descriptors;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors, m_v_scaleFactorSquares;
  int m_int_keyPointsNum = 0;
  FeatureVector m_bow_keyPointsVec;
  std::vector<std::shared_ptr<MapPoint>> mps;
  std::vector<std::shared_ptr<KeyFrame>> neighbours;
  std::shared_ptr<MapPoint> getMapPoint(const int& i) { return mps[i]; }
  void addMapPoint(std::shared_ptr<MapPoint> mp, const int& i) { mps[i] = mp; }
  cv::Mat getRotation_c2w() { return R.clone(); }
  cv::Mat getTranslation_c2w() { return t.clone(); }
  cv::Mat getCameraOriginInWorld() { return O.clone(); }
  std::vector<std::shared_ptr<KeyFrame>> getBestCovisibilityKeyFrames(const int& n) {
    return std::vector<std::shared_ptr<KeyFrame>>(neighbours.begin(), neighbours.begin() + std::min<size_t>(n, neighbours.size()));
  }
};
void MapPoint::addObservation(std::shared_ptr<KeyFrame> kf, int idx) { obs.push_back(std::make_pair(kf->index, idx)); }
struct Map {
  std::vector<std::shared_ptr<MapPoint>> points;
  void addMapPoint(std::shared_ptr<MapPoint> mp) { points.push_back(mp); }
};

cv::Mat readMat32(Reader& R, int rows, int cols) { cv::Mat m(rows, cols, CV_32F); R.get(m.ptr<float>(), (size_t)rows * cols); return m; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: localmapping_run scenario.bin out.bin\n"); return 2; }
  Reader R(argv[1]);
  float cam[6];
  R.get(cam, 6);
  Frame::m_flt_fx = cam[0]; Frame::m_flt_fy = cam[1]; Frame::m_flt_cx = cam[2]; Frame::m_flt_cy = cam[3];
  Frame::m_flt_baseLine = cam[4]; Frame::m_flt_baseLineTimesFx = cam[5];
  const int nLevels = R.get<int32_t>();
  std::vector<float> sf(nLevels), sf2(nLevels);
  R.get(sf.data(), nLevels); R.get(sf2.data(), nLevels);
  const int nKF = R.get<int32_t>(), abortAfter = R.get<int32_t>();
  std::vector<std::shared_ptr<KeyFrame>> kfs;
  for (int k = 0; k < nKF; k++) {
    auto kf = std::make_shared<KeyFrame>();
    kf->index = k;
    kf->R = readMat32(R, 3, 3); kf->t = readMat32(R, 3, 1); kf->O = readMat32(R, 3, 1);
    const int n = R.get<int32_t>();
    kf->m_int_keyPointsNum = n;
    kf->m_v_keyPoints.resize(n);
    R.get(reinterpret_cast<unsigned char*>(kf->m_v_keyPoints.data()), (size_t)n * sizeof(cv::KeyPoint));
    kf->m_cvMat_descriptors.create(std::max(n, 1), 32, CV_8U);
    R.get(kf->m_cvMat_descriptors.data, (size_t)n * 32);
    kf->m_v_rightXcords.resize(n); R.get(kf->m_v_rightXcords.data(), n);
    kf->m_v_depth.resize(n); R.get(kf->m_v_depth.data(), n);
    const int nodes = R.get<int32_t>();
    for (int i = 0; i < nodes; i++) {
      const unsigned id = R.get<uint32_t>();
      const int m = R.get<int32_t>();
      std::vector<unsigned> f(m);
      R.get(f.data(), m);
      kf->m_bow_keyPointsVec[id] = f;
    }
    kf->m_v_scaleFactors = sf; kf->m_v_scaleFactorSquares = sf2;
    kf->mps.resize(n);
    kfs.push_back(kf);
  }
  for (int k = 1; k < nKF; k++) kfs[0]->neighbours.push_back(kfs[k]);
  auto map = std::make_shared<Map>();
  std::list<std::shared_ptr<MapPoint>> recent;
  int abortCalls = 0;
  namespace ya = ydorb::adapter;
  const int created = ya::createNewMapPointsImpl<Frame, std::shared_ptr<KeyFrame>, MapPoint>(
      ya::matcher(), kfs[0], map, recent, [&] { abortCalls++; return abortAfter >= 0 && abortCalls >= abortAfter; });
  FILE* f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  const int32_t head[4] = {created, abortCalls, (int32_t)map->points.size(), (int32_t)recent.size()};
  fwrite(head, 4, 4, f);
  auto it = recent.begin();
  for (size_t i = 0; i < map->points.size(); i++, ++it) {
    const MapPoint& mp = *map->points[i];
    // one record per point: position, its two observations in order, the call counts, and whether the lists and the keyframes agree
    const bool consistent = *it == map->points[i] && mp.obs.size() == 2 && mp.obs[0].first == 0 && kfs[0]->mps[mp.obs[0].second] == map->points[i] &&
                            kfs[mp.obs[1].first]->mps[mp.obs[1].second] == map->points[i];
    fwrite(mp.pos.ptr<float>(), 4, 3, f);
    const int32_t rec[6] = {mp.obs.size() > 0 ? mp.obs[0].second : -1, mp.obs.size() > 1 ? mp.obs[1].first : -1,
                            mp.obs.size() > 1 ? mp.obs[1].second : -1, mp.distinctive, mp.updates, consistent ? 1 : 0};
    fwrite(rec, 4, 6, f);
  }
  fclose(f);
  return 0;
}
