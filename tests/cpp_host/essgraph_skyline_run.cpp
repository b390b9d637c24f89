// TEST-ONLY: EXECUTES optimizeEssentialGraphImpl (include/ydorb/optimizer.hpp) with a chosen solver on a stand-in map that may hold more
// keyframes than the dense solver takes, and dumps the graph it built and what it wrote back;
// tests/test_essgraph_skyline_adapter_gpu.py builds the scenario and compares with the ctypes path on the dumped graph.  The scenario
// file is essgraph_run.cpp's.  OpenCV / Eigen are the functional mocks of tests/cpu_harness/mockrt.
//
//   essgraph_skyline_run scenario.bin out.bin auto|dense|skyline        exit status 1 and the text on stderr when the adapter throws
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <vector>

#include "../../include/ydorb/optimizer.hpp"

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
typedef std::shared_ptr<KeyFrame> KFP;
struct KeyFrame {
  long int m_int_keyFrameID = 0;
  bool bad = false;
  cv::Mat R, t, written;
  KFP parent;
  std::set<KFP> children, loopEdges;
  std::vector<std::pair<int, KFP>> covisibles;   // (weight, keyframe), ordered by weight, largest first
  bool isBad() { return bad; }
  cv::Mat getRotation_c2w() { return R.clone(); }
  cv::Mat getTranslation_c2w() { return t.clone(); }
  void setCameraPoseByTransform_c2w(const cv::Mat& T) { written = T.clone(); }
  KFP getParent() { return parent; }
  bool hasChild(KFP k) { return children.count(k) != 0; }
  std::set<KFP> getLoopEdges() { return loopEdges; }
  std::vector<KFP> getCovisiblesByWeight(const int& w) {
    std::vector<KFP> out;
    for (auto& c : covisibles) if (c.first >= w) out.push_back(c.second);
    return out;
  }
  int getWeight(KFP k) {
    for (auto& c : covisibles) if (c.second == k) return c.first;
    return 0;
  }
};
struct MapPoint {
  cv::Mat pos;
  bool bad = false;
  KFP ref;
  long int m_int_correctedByKeyFrameID = -1, m_int_correctedReference = -1;
  int set = 0, updated = 0;
  bool isBad() { return bad; }
  cv::Mat getPosInWorld() { return pos.clone(); }
  void setPosInWorld(const cv::Mat& X) { pos = X.clone(); set++; }
  void updateNormalAndDepth() { updated++; }
  KFP getReferenceKeyFrame() { return ref; }
};
typedef std::shared_ptr<MapPoint> MPP;
struct Map {
  std::mutex m_mutex_updateMap;
  std::vector<KFP> kfs;
  std::vector<MPP> mps;
  std::vector<KFP> getAllKeyFrames() { return kfs; }
  std::vector<MPP> getAllMapPoints() { return mps; }
};
struct Frame {};

struct Quat { double v[4]; double x() const { return v[0]; } double y() const { return v[1]; } double z() const { return v[2]; } double w() const { return v[3]; } };
struct Vec3 { double v[3]; double operator[](int i) const { return v[i]; } };
struct Sim3 {
  Quat r; Vec3 t; double s;
  const Quat& rotation() const { return r; }
  const Vec3& translation() const { return t; }
  const double& scale() const { return s; }
};
typedef std::map<KFP, Sim3> KeyFrameAndPose;

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: essgraph_skyline_run scenario.bin out.bin auto|dense|skyline\n"); return 2; }
  const int solver = !strcmp(argv[3], "auto") ? YDORB_ESS_SOLVER_AUTO : !strcmp(argv[3], "dense") ? YDORB_ESS_SOLVER_DENSE
                     : !strcmp(argv[3], "skyline") ? YDORB_ESS_SOLVER_SKYLINE : -1;
  if (solver < 0) { fprintf(stderr, "unknown solver %s\n", argv[3]); return 2; }
  try {
    Reader R(argv[1]);
    Writer W(argv[2]);
    const int nKF = R.get<int32_t>();
    std::vector<KeyFrame> pool(nKF);   // one block: the pointer order of std::map<KFP, ...> is the order of the list
    std::map<long int, KFP> byId;
    auto map = std::make_shared<Map>();
    std::vector<int> parentId(nKF);
    for (int i = 0; i < nKF; i++) {
      KFP kf(&pool[i], [](KeyFrame*) {});
      kf->m_int_keyFrameID = R.get<int32_t>(); kf->bad = R.get<int32_t>() != 0; parentId[i] = R.get<int32_t>();
      kf->R = cv::Mat(3, 3, CV_32F); kf->t = cv::Mat(3, 1, CV_32F);
      for (int k = 0; k < 9; k++) kf->R.at<float>(k / 3, k % 3) = R.get<float>();
      for (int k = 0; k < 3; k++) kf->t.at<float>(k) = R.get<float>();
      byId[kf->m_int_keyFrameID] = kf;
      map->kfs.push_back(kf);
    }
    for (int i = 0; i < nKF; i++)
      if (parentId[i] >= 0) { map->kfs[i]->parent = byId.at(parentId[i]); byId.at(parentId[i])->children.insert(map->kfs[i]); }
    const int nCov = R.get<int32_t>();
    for (int i = 0; i < nCov; i++) {
      const int a = R.get<int32_t>(), b = R.get<int32_t>(), w = R.get<int32_t>();
      byId.at(a)->covisibles.push_back({w, byId.at(b)});
      byId.at(b)->covisibles.push_back({w, byId.at(a)});
    }
    const int nLoop = R.get<int32_t>();
    for (int i = 0; i < nLoop; i++) {
      const int a = R.get<int32_t>(), b = R.get<int32_t>();
      byId.at(a)->loopEdges.insert(byId.at(b)); byId.at(b)->loopEdges.insert(byId.at(a));
    }
    KeyFrameAndPose pose[2];   // corrected, non-corrected
    for (int m = 0; m < 2; m++) {
      const int n = R.get<int32_t>();
      for (int i = 0; i < n; i++) {
        const int id = R.get<int32_t>();
        Sim3 S;
        R.get(S.r.v, 4); R.get(S.t.v, 3); S.s = R.get<double>();
        pose[m][byId.at(id)] = S;
      }
    }
    std::map<KFP, std::set<KFP>> loopConnections;
    const int nConn = R.get<int32_t>();
    for (int i = 0; i < nConn; i++) {
      const int id = R.get<int32_t>(), n = R.get<int32_t>();
      for (int k = 0; k < n; k++) loopConnections[byId.at(id)].insert(byId.at(R.get<int32_t>()));
    }
    const int nMP = R.get<int32_t>();
    for (int i = 0; i < nMP; i++) {
      auto mp = std::make_shared<MapPoint>();
      mp->pos = cv::Mat(3, 1, CV_32F);
      for (int k = 0; k < 3; k++) mp->pos.at<float>(k) = R.get<float>();
      mp->bad = R.get<int32_t>() != 0;
      mp->ref = byId.at(R.get<int32_t>());
      mp->m_int_correctedByKeyFrameID = R.get<int32_t>(); mp->m_int_correctedReference = R.get<int32_t>();
      map->mps.push_back(mp);
    }
    const KFP loopKF = byId.at(R.get<int32_t>()), curKF = byId.at(R.get<int32_t>());
    const bool fixScale = R.get<int32_t>() != 0;

    const auto G = ydorb::adapter::buildEssentialGraph(map, loopKF, curKF, pose[1], pose[0], loopConnections);
    const int V = (int)G.vertexKF.size(), E = (int)G.v0.size();
    W.put<int32_t>(V);
    W.put(G.sim3.data(), G.sim3.size()); W.put(G.fixed.data(), G.fixed.size());
    W.put<int32_t>(E); W.put(G.v0.data(), E); W.put(G.v1.data(), E); W.put(G.meas.data(), G.meas.size());

    ydorb::adapter::optimizeEssentialGraphImpl<Frame>(map, loopKF, curKF, pose[1], pose[0], loopConnections, fixScale, 0, solver);
    for (const KFP& k : map->kfs) {
      W.put<int32_t>(k->written.empty() ? 0 : 1);
      float T[16] = {0};
      if (!k->written.empty()) for (int i = 0; i < 16; i++) T[i] = k->written.at<float>(i / 4, i % 4);
      W.put(T, 16);
    }
    for (const MPP& p : map->mps) {
      W.put<int32_t>(p->set); W.put<int32_t>(p->updated);
      for (int k = 0; k < 3; k++) W.put<float>(p->pos.at<float>(k));
    }
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
