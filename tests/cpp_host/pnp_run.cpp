// TEST-ONLY: EXECUTES include/ydorb/pnpSolver.hpp on the GPU against stand-ins of the reference's Frame / MapPoint that carry real
// data, and dumps what it did; tests/test_pnp_adapter_gpu.py builds the scenario and replays every call through the ctypes path.
// OpenCV is the functional mock of tests/cpu_harness/mockrt.
//
//   pnp_run seq   scenario.bin out.bin   PnPsolver(F, matches[0]) + setRansacParameters + iterate(5) until a return or bNoMore
//   pnp_run batch scenario.bin out.bin   one PnPsolver per match vector; pnpIterateBatch(live solvers, 5) rounds, the relocalisation
//                                        loop: a solver leaves the batch at a return or bNoMore
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ydorb/pnpSolver.hpp"

namespace {

struct Reader {
  FILE* f;
  explicit Reader(const char* path) : f(fopen(path, "rb")) { if (!f) { perror(path); exit(2); } }
  ~Reader() { fclose(f); }
  template <class T> T get() { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "scenario truncated\n"); exit(2); } return v; }
};
struct Writer {
  FILE* f;
  explicit Writer(const char* path) : f(fopen(path, "wb")) { if (!f) { perror(path); exit(2); } }
  ~Writer() { fclose(f); }
  template <class T> void put(const T& v) { fwrite(&v, sizeof(T), 1, f); }
  template <class T> void put(const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
};

struct MapPoint {
  cv::Mat pos;
  bool bad = false;
  bool isBad() { return bad; }
  cv::Mat getPosInWorld() { return pos.clone(); }
};
struct Frame {
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_scaleFactorSquares;
  static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy;
};
float Frame::m_flt_fx, Frame::m_flt_fy, Frame::m_flt_cx, Frame::m_flt_cy;

typedef std::shared_ptr<MapPoint> MPP;
typedef ydorb::adapter::PnPsolver<Frame, MPP> Solver;

struct Scene {
  Frame F;
  std::vector<MPP> mps;
  std::vector<std::vector<MPP>> matches;
  int loopOr, seed;
};

Scene readScene(Reader& R) {
  Scene S;
  const int nKP = R.get<int32_t>(), nMP = R.get<int32_t>(), nSol = R.get<int32_t>();
  S.loopOr = R.get<int32_t>(); S.seed = R.get<int32_t>();
  Frame::m_flt_fx = R.get<float>(); Frame::m_flt_fy = R.get<float>(); Frame::m_flt_cx = R.get<float>(); Frame::m_flt_cy = R.get<float>();
  S.F.m_v_scaleFactorSquares.resize(8);
  for (auto& v : S.F.m_v_scaleFactorSquares) v = R.get<float>();
  S.F.m_v_keyPoints.resize(nKP);
  for (auto& kp : S.F.m_v_keyPoints) { kp = cv::KeyPoint(); kp.pt.x = R.get<float>(); kp.pt.y = R.get<float>(); kp.octave = R.get<int32_t>(); }
  for (int m = 0; m < nMP; m++) {
    MPP p = std::make_shared<MapPoint>();
    p->pos = cv::Mat(3, 1, CV_32F);
    for (int i = 0; i < 3; i++) p->pos.at<float>(i) = R.get<float>();
    p->bad = R.get<int32_t>() != 0;
    S.mps.push_back(p);
  }
  S.matches.resize(nSol);
  for (auto& v : S.matches) {
    v.resize(nKP);
    for (int i = 0; i < nKP; i++) { const int m = R.get<int32_t>(); if (m >= 0) v[i] = S.mps[m]; }
  }
  return S;
}

Solver* makeSolver(const Scene& S, int k) {
  Solver* s = new Solver(S.F, S.matches[k]);
  s->setRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);   // Tracking::relocalize's parameters
  s->setLoopOr(S.loopOr != 0);
  return s;
}

void putSolver(Writer& W, const Solver& s) {
  const int N = (int)s.mvKeyPointIndices.size();
  W.put<int32_t>(N); W.put(s.mvKeyPointIndices.data(), N);
  W.put(s.Xw.data(), 3 * N); W.put(s.P2D.data(), 2 * N); W.put(s.maxErr.data(), N);
  W.put<int32_t>(s.minInliers()); W.put<int32_t>(s.maxIterations());
}

// one record per iterate() a solver ran: solver, its quads, and what iterate returned
void putCall(Writer& W, int k, const Solver& s, const cv::Mat& T, bool noMore, const std::vector<bool>& inl, int nInl, int nKP) {
  W.put<int32_t>(k);
  W.put<int32_t>((int32_t)s.lastQuads.size() / 4); W.put(s.lastQuads.data(), s.lastQuads.size());
  W.put<int32_t>(T.empty() ? 0 : 1); W.put<int32_t>(noMore ? 1 : 0); W.put<int32_t>(nInl);
  W.put<int32_t>((int32_t)inl.size());
  for (int i = 0; i < nKP; i++) W.put<uint8_t>(i < (int)inl.size() && inl[i] ? 1 : 0);
  float t16[16] = {0};
  if (!T.empty()) for (int i = 0; i < 16; i++) t16[i] = T.at<float>(i / 4, i % 4);
  W.put(t16, 16);
}

void warmUp(const Scene& S) {   // the HIP runtime's lazy initialisation may itself use rand(): let it happen before the seed
  Solver* w = makeSolver(S, 0);
  bool nm;
  std::vector<bool> v;
  int k;
  w->iterate(5, nm, v, k);
  delete w;
}

int runSeq(Reader& R, Writer& W) {
  Scene S = readScene(R);
  const int nKP = (int)S.F.m_v_keyPoints.size();
  warmUp(S);
  Solver* s = makeSolver(S, 0);
  putSolver(W, *s);
  std::srand(S.seed);
  std::vector<bool> inl;
  bool noMore = false;
  int nInl = 0;
  for (int call = 0; call < 400; call++) {   // the relocalisation loop's repeated iterate(5) on one candidate
    const cv::Mat T = s->iterate(5, noMore, inl, nInl);
    putCall(W, 0, *s, T, noMore, inl, nInl, nKP);
    if (!T.empty() || noMore) break;
  }
  delete s;
  return 0;
}

int runBatch(Reader& R, Writer& W) {
  Scene S = readScene(R);
  const int nKP = (int)S.F.m_v_keyPoints.size(), nSol = (int)S.matches.size();
  warmUp(S);
  std::vector<Solver*> solvers;
  for (int k = 0; k < nSol; k++) { solvers.push_back(makeSolver(S, k)); putSolver(W, *solvers.back()); }
  std::srand(S.seed);
  std::vector<char> done(nSol, 0);
  for (int round = 0; round < 400; round++) {
    std::vector<Solver*> live;
    std::vector<int> ids;
    for (int k = 0; k < nSol; k++) if (!done[k]) { live.push_back(solvers[k]); ids.push_back(k); }
    if (live.empty()) break;
    std::vector<cv::Mat> T;
    std::vector<char> noMore;
    std::vector<std::vector<bool>> inl;
    std::vector<int> nInl;
    ydorb::adapter::pnpIterateBatch(live, 5, T, noMore, inl, nInl);
    for (size_t j = 0; j < live.size(); j++) {
      putCall(W, ids[j], *live[j], T[j], noMore[j] != 0, inl[j], nInl[j], nKP);
      if (!T[j].empty() || noMore[j]) done[ids[j]] = 1;
    }
  }
  for (Solver* s : solvers) delete s;
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: pnp_run seq|batch scenario.bin out.bin\n"); return 2; }
  try {
    Reader R(argv[2]);
    Writer W(argv[3]);
    const std::string what = argv[1];
    if (what == "seq") return runSeq(R, W);
    if (what == "batch") return runBatch(R, W);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  fprintf(stderr, "unknown mode\n");
  return 2;
}
