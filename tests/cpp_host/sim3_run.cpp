// TEST-ONLY: EXECUTES include/ydorb/sim3Solver.hpp and optimizeSim3Impl (include/ydorb/optimizer.hpp) on the GPU against stand-ins of the
// reference's KeyFrame / MapPoint that carry real data, and dumps what they did; tests/test_sim3_adapter_gpu.py builds the scenario and
// compares with the ctypes path on the same flat problem.  OpenCV / Eigen are the functional mocks of tests/cpu_harness/mockrt.
//
//   sim3_run ransac scenario.bin out.bin    Sim3Solver(kf1, kf2, matched12) + setRansacParameters + iterate(5) until a return or bNoMore
//   sim3_run opt    scenario.bin out.bin    optimizeSim3Impl(kf1, kf2, matched12, S12, th2, fixScale)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ydorb/optimizer.hpp"
#include "../../include/ydorb/sim3Solver.hpp"

namespace {

struct Reader {
  FILE* f;
  explicit Reader(const char* path) : f(fopen(path, "rb")) { if (!f) { perror(path); exit(2); } }
  ~Reader() { fclose(f); }
  template <class T> T get() { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "scenario truncated\n"); exit(2); } return v; }
  template <class T> void get(T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scenario truncated\n"); exit(2); } }
};
struct Writer {
  FILE* f;
  explicit Writer(const char* path) : f(fopen(path, "wb")) { if (!f) { perror(path); exit(2); } }
  ~Writer() { fclose(f); }
  template <class T> void put(const T& v) { fwrite(&v, sizeof(T), 1, f); }
  template <class T> void put(const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
};

struct KeyFrame;
struct MapPoint {
  cv::Mat pos;
  bool bad = false;
  std::shared_ptr<KeyFrame> kf1, kf2;
  int idx1 = -1, idx2 = -1;
  int index = -1;
  bool isBad() { return bad; }
  cv::Mat getPosInWorld() { return pos.clone(); }
  int getIdxInKeyFrame(std::shared_ptr<KeyFrame> kf) { return kf == kf1 ? idx1 : kf == kf2 ? idx2 : -1; }
};
struct KeyFrame {
  cv::Mat R, t;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_scaleFactorSquares, m_v_invScaleFactorSquares;
  std::vector<std::shared_ptr<MapPoint>> mps;
  cv::Mat getRotation_c2w() { return R.clone(); }
  cv::Mat getTranslation_c2w() { return t.clone(); }
  std::vector<std::shared_ptr<MapPoint>> getMatchedMapPointsVec() { return mps; }
};
struct Frame { static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy; };
float Frame::m_flt_fx, Frame::m_flt_fy, Frame::m_flt_cx, Frame::m_flt_cy;

typedef std::shared_ptr<KeyFrame> KFP;
typedef std::shared_ptr<MapPoint> MPP;

struct Scene {
  KFP kf[2];
  std::vector<MPP> mps, matched12;
};

Scene readScene(Reader& R) {
  Scene S;
  const int nMP = R.get<int32_t>(), nKP1 = R.get<int32_t>(), nKP2 = R.get<int32_t>();
  Frame::m_flt_fx = R.get<float>(); Frame::m_flt_fy = R.get<float>(); Frame::m_flt_cx = R.get<float>(); Frame::m_flt_cy = R.get<float>();
  const int nKP[2] = {nKP1, nKP2};
  for (int k = 0; k < 2; k++) {
    KFP kf = std::make_shared<KeyFrame>();
    kf->R = cv::Mat(3, 3, CV_32F); kf->t = cv::Mat(3, 1, CV_32F);
    for (int i = 0; i < 9; i++) kf->R.at<float>(i / 3, i % 3) = R.get<float>();
    for (int i = 0; i < 3; i++) kf->t.at<float>(i) = R.get<float>();
    kf->m_v_scaleFactorSquares.resize(8); kf->m_v_invScaleFactorSquares.resize(8);
    R.get(kf->m_v_scaleFactorSquares.data(), 8); R.get(kf->m_v_invScaleFactorSquares.data(), 8);
    kf->m_v_keyPoints.resize(nKP[k]);
    for (auto& kp : kf->m_v_keyPoints) { kp = cv::KeyPoint(); kp.pt.x = R.get<float>(); kp.pt.y = R.get<float>(); kp.octave = R.get<int32_t>(); }
    S.kf[k] = kf;
  }
  for (int m = 0; m < nMP; m++) {
    MPP p = std::make_shared<MapPoint>();
    p->pos = cv::Mat(3, 1, CV_32F);
    for (int i = 0; i < 3; i++) p->pos.at<float>(i) = R.get<float>();
    p->bad = R.get<int32_t>() != 0; p->idx1 = R.get<int32_t>(); p->idx2 = R.get<int32_t>();
    p->kf1 = S.kf[0]; p->kf2 = S.kf[1]; p->index = m;
    S.mps.push_back(p);
  }
  S.kf[0]->mps.resize(nKP1); S.matched12.resize(nKP1);
  for (int i = 0; i < nKP1; i++) { const int m = R.get<int32_t>(); if (m >= 0) S.kf[0]->mps[i] = S.mps[m]; }
  for (int i = 0; i < nKP1; i++) { const int m = R.get<int32_t>(); if (m >= 0) S.matched12[i] = S.mps[m]; }
  return S;
}

int runRansac(Reader& R, Writer& W) {
  Scene S = readScene(R);
  const unsigned seed = R.get<int32_t>();
  const int minInliers = R.get<int32_t>(), maxIts = R.get<int32_t>(), fix = R.get<int32_t>();
  ydorb::adapter::Sim3Solver<KFP, MPP, Frame> solver(S.kf[0], S.kf[1], S.matched12, fix != 0);
  solver.setRansacParameters(0.99, minInliers, maxIts);
  const int N = (int)solver.indices1.size();
  W.put<int32_t>(N); W.put(solver.indices1.data(), N);
  W.put(solver.X1.data(), 3 * N); W.put(solver.X2.data(), 3 * N); W.put(solver.P1.data(), 2 * N); W.put(solver.P2.data(), 2 * N);
  W.put(solver.maxErr1.data(), N); W.put(solver.maxErr2.data(), N);
  W.put<int32_t>(solver.maxIterations());
  {   // the HIP runtime's lazy initialisation (first call on the device) may itself use rand(): let it happen before the seed
    ydorb::adapter::Sim3Solver<KFP, MPP, Frame> warm(S.kf[0], S.kf[1], S.matched12, fix != 0);
    bool nm;
    std::vector<bool> v;
    int k;
    warm.iterate(5, nm, v, k);
  }
  std::srand(seed);
  std::vector<int> all;
  std::vector<bool> inl;
  bool noMore = false;
  int nInl = 0, calls = 0;
  cv::Mat T;
  for (; calls < 200; calls++) {   // LoopClosing::computeSim3's repeated iterate(5)
    T = solver.iterate(5, noMore, inl, nInl);
    all.insert(all.end(), solver.lastTriples.begin(), solver.lastTriples.end());
    if (!T.empty() || noMore) { calls++; break; }
  }
  W.put<int32_t>(calls); W.put<int32_t>((int32_t)all.size()); W.put(all.data(), all.size());
  W.put<int32_t>(T.empty() ? 0 : 1); W.put<int32_t>(noMore ? 1 : 0); W.put<int32_t>(nInl);
  for (size_t i = 0; i < S.matched12.size(); i++) W.put<uint8_t>(i < inl.size() && inl[i] ? 1 : 0);
  float t16[16] = {0};
  if (!T.empty()) for (int i = 0; i < 16; i++) t16[i] = T.at<float>(i / 4, i % 4);
  W.put(t16, 16);
  const cv::Mat Rb = solver.getEstimatedRotation(), tb = solver.getEstimatedTranslation();
  for (int i = 0; i < 9; i++) W.put<float>(Rb.at<float>(i / 3, i % 3));
  for (int i = 0; i < 3; i++) W.put<float>(tb.at<float>(i));
  W.put<float>(solver.getEstimatedScale());
  return 0;
}

int runOpt(Reader& R, Writer& W) {
  Scene S = readScene(R);
  double S12[8];
  R.get(S12, 8);
  const float th2 = R.get<float>();
  const int fix = R.get<int32_t>();
  std::vector<MPP> matches = S.matched12;
  const int n = ydorb::adapter::optimizeSim3Impl<Frame>(S.kf[0], S.kf[1], matches, S12, th2, fix != 0);
  W.put<int32_t>(n); W.put(S12, 8);
  for (auto& m : matches) W.put<int32_t>(m ? m->index : -1);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: sim3_run ransac|opt scenario.bin out.bin\n"); return 2; }
  try {
    Reader R(argv[2]);
    Writer W(argv[3]);
    const std::string what = argv[1];
    if (what == "ransac") return runRansac(R, W);
    if (what == "opt") return runOpt(R, W);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  fprintf(stderr, "unknown mode\n");
  return 2;
}
