// TEST-ONLY: EXECUTES the resident overload createNewMapPointsImpl(Mirror&, ...) of include/ydorb/localMapping.hpp on the GPU, over a
// MapMirror with enableDescriptors(), enableFeatures() and enableBow(), beside the flat createNewMapPointsImpl on a second copy of the
// same stand-in keyframes (KeyFrame / MapPoint / Map stand-ins that carry real data).  The scenario is the file of
// tests/cpp_host/localmapping_run.cpp (tests/test_createpoints_resident_adapter_gpu.py writes it).  The program compares the two copies
// exactly - the created points in order: position bits, both observations, the call counts, the keyframes' map-point vectors - and
// prints one line per figure, "<name> <value>".  OpenCV is the functional mock of tests/cpu_harness/mockrt.
//   createpoints_resident_run scenario.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <vector>

#include "../../include/ydorb/localMapping.hpp"
#include "../../include/ydorb/mapMirror.hpp"

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
typedef std::shared_ptr<KeyFrame> KF;
struct MapPoint {
  cv::Mat pos;
  KF ref;
  std::vector<std::pair<int, int>> obs;   // (keyframe index, keypoint index) in addObservation order
  std::map<KF, size_t> held;              // the same, as the reference's container
  int distinctive = 0, updates = 0;
  MapPoint(const cv::Mat& p, KF kf, std::shared_ptr<Map>) : pos(p.clone()), ref(kf) {}
  void addObservation(KF kf, int idx);
  void computeDistinctiveDescriptors() { distinctive++; }
  void updateNormalAndDepth() { updates++; }
  bool isBad() { return false; }
  std::map<KF, size_t> getObservations() { return held; }
  KF getReferenceKeyFrame() { return ref; }
  cv::Mat getPosInWorld() { return pos.clone(); }
};
typedef std::shared_ptr<MapPoint> MP;
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
  std::vector<MP> mps;
  std::vector<KF> neighbours;
  MP getMapPoint(const int& i) { return mps[i]; }
  void addMapPoint(MP mp, const int& i) { mps[i] = mp; }
  std::vector<MP> getMapPointMatches() { return mps; }
  bool isBad() { return false; }
  cv::Mat getRotation_c2w() { return R.clone(); }
  cv::Mat getTranslation_c2w() { return t.clone(); }
  cv::Mat getCameraOriginInWorld() { return O.clone(); }
  std::vector<KF> getBestCovisibilityKeyFrames(const int& n) { return std::vector<KF>(neighbours.begin(), neighbours.begin() + std::min<size_t>(n, neighbours.size())); }
};
void MapPoint::addObservation(KF kf, int idx) { obs.push_back(std::make_pair(kf->index, idx)); held[kf] = (size_t)idx; }
struct Map {
  std::vector<MP> points;
  void addMapPoint(MP mp) { points.push_back(mp); }
};
typedef ydorb::adapter::MapMirror<KF, MP> Mirror;

cv::Mat readMat32(Reader& R, int rows, int cols) { cv::Mat m(rows, cols, CV_32F); R.get(m.ptr<float>(), (size_t)rows * cols); return m; }

struct World {
  std::vector<KF> kfs;
  std::shared_ptr<Map> map = std::make_shared<Map>();
  std::list<MP> recent;
  int abortAfter = -1, abortCalls = 0, created = 0;
};

// the same file gives the same world: the two copies are read independently and share no object
World load(const char* path) {
  Reader R(path);
  World W;
  float cam[6];
  R.get(cam, 6);
  Frame::m_flt_fx = cam[0]; Frame::m_flt_fy = cam[1]; Frame::m_flt_cx = cam[2]; Frame::m_flt_cy = cam[3];
  Frame::m_flt_baseLine = cam[4]; Frame::m_flt_baseLineTimesFx = cam[5];
  const int nLevels = R.get<int32_t>();
  std::vector<float> sf(nLevels), sf2(nLevels);
  R.get(sf.data(), nLevels); R.get(sf2.data(), nLevels);
  const int nKF = R.get<int32_t>();
  W.abortAfter = R.get<int32_t>();
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
    W.kfs.push_back(kf);
  }
  for (int k = 1; k < nKF; k++) W.kfs[0]->neighbours.push_back(W.kfs[k]);
  return W;
}

// the created points in order, as integers: position bits, both observations, call counts, then every keyframe's map-point vector
std::vector<long> stateOf(const World& W) {
  std::vector<long> s;
  std::map<const MapPoint*, long> order;
  auto it = W.recent.begin();
  for (size_t i = 0; i < W.map->points.size(); i++, ++it) {
    const MapPoint& mp = *W.map->points[i];
    order[&mp] = (long)i;
    for (int r = 0; r < 3; r++) { uint32_t b; std::memcpy(&b, mp.pos.ptr<float>() + r, 4); s.push_back((long)b); }
    s.push_back((long)mp.obs.size());
    for (const auto& o : mp.obs) { s.push_back(o.first); s.push_back(o.second); }
    s.push_back(mp.distinctive); s.push_back(mp.updates);
    s.push_back(it != W.recent.end() && *it == W.map->points[i] ? 1 : 0);
  }
  for (const KF& kf : W.kfs)
    for (const MP& mp : kf->mps) s.push_back(mp ? order[mp.get()] : -1);
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: createpoints_resident_run scenario.bin\n"); return 2; }
  namespace ya = ydorb::adapter;
  try {
    World A = load(argv[1]), B = load(argv[1]);
    A.created = ya::createNewMapPointsImpl<Frame, KF, MapPoint>(ya::matcher(), A.kfs[0], A.map, A.recent,
                                                                [&] { A.abortCalls++; return A.abortAfter >= 0 && A.abortCalls >= A.abortAfter; });
    Mirror mirror(0, 64, 2, 256);   // small: every table grows while the scene is loaded
    mirror.enableDescriptors();
    mirror.enableFeatures();
    mirror.enableBow();
    // the current keyframe is touched as LocalMapping would have it; the neighbours are met by the call for the first time
    mirror.touch(B.kfs[0]); mirror.touchRow(B.kfs[0]); mirror.touchDescriptors(B.kfs[0]); mirror.touchFeatures(B.kfs[0]); mirror.touchBow(B.kfs[0]);
    B.created = ya::createNewMapPointsImpl<Frame, KF, MapPoint>(mirror, ya::matcher(), B.kfs[0], B.map, B.recent,
                                                                [&] { B.abortCalls++; return B.abortAfter >= 0 && B.abortCalls >= B.abortAfter; });
    int perNb[16] = {0};
    for (const MP& mp : B.map->points) if (mp->obs.size() == 2 && mp->obs[1].first < 16) perNb[mp->obs[1].first]++;
    printf("created_flat %d\ncreated_resident %d\nabort_calls_flat %d\nabort_calls_resident %d\n", A.created, B.created, A.abortCalls, B.abortCalls);
    printf("state_same %d\nmap_points %d\nrecent %d\n", stateOf(A) == stateOf(B) ? 1 : 0, (int)B.map->points.size(), (int)B.recent.size());
    for (size_t k = 1; k < B.kfs.size(); k++) printf("created_with_%zu %d\n", k, perNb[k]);
    const Mirror::Difference d = mirror.verify();
    printf("verify_after %d\n", (int)(d.pointSlots.size() + d.keyFrameSlots.size() + mirror.verifyRows().size() + mirror.verifyBow().size() +
                                      mirror.verifyFeatures().size()));
    YdMapDbBowStats bs;
    ydorb_mapdb_bow_stats(mirror.handle(), &bs);
    printf("bow_entries_resident %lld\n", (long long)bs.n_entries);
    // a second keyframe's worth: the call again finds every accepted idx1 taken by its row and creates nothing from those
    const int again = ya::createNewMapPointsImpl<Frame, KF, MapPoint>(mirror, ya::matcher(), B.kfs[0], B.map, B.recent, [] { return false; });
    int againFlat = ya::createNewMapPointsImpl<Frame, KF, MapPoint>(ya::matcher(), A.kfs[0], A.map, A.recent, [] { return false; });
    printf("second_call_same %d\nsecond_call_created %d\n", again == againFlat && stateOf(A) == stateOf(B) ? 1 : 0, again);
  } catch (const std::exception& e) {
    fprintf(stderr, "createpoints_resident_run: %s\n", e.what());
    return 1;
  }
  return 0;
}
