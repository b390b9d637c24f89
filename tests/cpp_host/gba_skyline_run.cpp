// TEST-ONLY: EXECUTES globalBundleAdjustImpl (include/ydorb/optimizer.hpp) with a chosen solver on a stand-in map that may hold more
// keyframes than the dense reduced camera solve takes, and dumps what it wrote back;
// tests/test_gba_skyline_adapter_gpu.py builds the scenario and compares with the ctypes path on the same graph.  OpenCV / Eigen are
// the functional mocks of tests/cpu_harness/mockrt.
//
//   gba_skyline_run scenario.bin out.bin auto|dense|skyline|default loopKeyFrameID     exit status 1 and the text on stderr when the adapter throws
//
// scenario: camera fx fy cx cy bf (float); iterations, robust (int32); nKF, then per keyframe its id (int32) and T_c2w (16 float);
// nMP, then per map point its position (3 float), nObs (int32) and per observation keyframe index (int32), u, v, u_right (float).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
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

struct KeyFrame {
  long int m_int_keyFrameID = 0, m_int_globalBAForKeyFrameID = 0;
  cv::Mat pose, m_cvMat_T_c2w_GlobalBA;
  int poseWrites = 0;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_invScaleFactorSquares;
  bool isBad() { return false; }
  cv::Mat getCameraPoseByTransform_c2w() { return pose.clone(); }
  void setCameraPoseByTransform_c2w(cv::Mat T) { pose = T.clone(); poseWrites++; }
};
typedef std::shared_ptr<KeyFrame> KFP;
struct MapPoint {
  cv::Mat pos, m_cvMat_posGlobalBA;
  long int m_int_globalBAforKeyFrameID = 0;
  int sets = 0, updates = 0;
  std::map<KFP, size_t> obs;
  bool isBad() { return false; }
  cv::Mat getPosInWorld() { return pos.clone(); }
  std::map<KFP, size_t> getObservations() { return obs; }
  void setPosInWorld(const cv::Mat& p) { pos = p.clone(); sets++; }
  void updateNormalAndDepth() { updates++; }
};
typedef std::shared_ptr<MapPoint> MPP;
struct Map {
  std::mutex m_mutex_updateMap;
  std::vector<KFP> kfs;
  std::vector<MPP> mps;
  std::vector<KFP> getAllKeyFrames() { return kfs; }
  std::vector<MPP> getAllMapPoints() { return mps; }
};
struct Frame { static float m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLineTimesFx; };
float Frame::m_flt_fx, Frame::m_flt_fy, Frame::m_flt_cx, Frame::m_flt_cy, Frame::m_flt_baseLineTimesFx;

}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: gba_skyline_run scenario.bin out.bin auto|dense|skyline|default loopKeyFrameID\n"); return 2; }
  const bool byDefault = !strcmp(argv[3], "default");
  const int solver = !strcmp(argv[3], "auto") ? YDORB_BA_SOLVER_AUTO : !strcmp(argv[3], "dense") ? YDORB_BA_SOLVER_DENSE
                     : !strcmp(argv[3], "skyline") ? YDORB_BA_SOLVER_SKYLINE : byDefault ? 0 : -1;
  if (solver < 0) { fprintf(stderr, "unknown solver %s\n", argv[3]); return 2; }
  const long int loopId = atol(argv[4]);
  try {
    Reader R(argv[1]);
    Writer W(argv[2]);
    float cam[5];
    R.get(cam, 5);
    Frame::m_flt_fx = cam[0]; Frame::m_flt_fy = cam[1]; Frame::m_flt_cx = cam[2]; Frame::m_flt_cy = cam[3]; Frame::m_flt_baseLineTimesFx = cam[4];
    const int iterations = R.get<int32_t>();
    const bool robust = R.get<int32_t>() != 0;
    auto map = std::make_shared<Map>();
    const int nKF = R.get<int32_t>();
    for (int i = 0; i < nKF; i++) {
      auto kf = std::make_shared<KeyFrame>();
      kf->m_int_keyFrameID = R.get<int32_t>();
      kf->pose = cv::Mat(4, 4, CV_32F);
      R.get(kf->pose.ptr<float>(), 16);
      kf->m_v_invScaleFactorSquares.assign(8, 1.0f);
      map->kfs.push_back(kf);
    }
    const int nMP = R.get<int32_t>();
    for (int i = 0; i < nMP; i++) {
      auto mp = std::make_shared<MapPoint>();
      mp->pos = cv::Mat(3, 1, CV_32F);
      R.get(mp->pos.ptr<float>(), 3);
      const int nObs = R.get<int32_t>();
      for (int o = 0; o < nObs; o++) {
        const KFP& kf = map->kfs.at(R.get<int32_t>());
        cv::KeyPoint kp;
        kp.pt.x = R.get<float>(); kp.pt.y = R.get<float>(); kp.octave = 0;
        mp->obs[kf] = kf->m_v_keyPoints.size();
        kf->m_v_keyPoints.push_back(kp);
        kf->m_v_rightXcords.push_back(R.get<float>());
      }
      map->mps.push_back(mp);
    }
    if (byDefault) ydorb::adapter::globalBundleAdjustImpl<Frame>(map, iterations, nullptr, loopId, robust);
    else ydorb::adapter::globalBundleAdjustImpl<Frame>(map, iterations, nullptr, loopId, robust, solver);
    for (const KFP& k : map->kfs) {
      W.put<int32_t>(k->poseWrites); W.put<int32_t>((int32_t)k->m_int_globalBAForKeyFrameID);
      W.put(k->pose.ptr<float>(), 16);
      float G[16] = {0};
      if (!k->m_cvMat_T_c2w_GlobalBA.empty()) for (int i = 0; i < 16; i++) G[i] = k->m_cvMat_T_c2w_GlobalBA.at<float>(i / 4, i % 4);
      W.put(G, 16);
    }
    for (const MPP& p : map->mps) {
      W.put<int32_t>(p->sets); W.put<int32_t>(p->updates); W.put<int32_t>((int32_t)p->m_int_globalBAforKeyFrameID);
      W.put(p->pos.ptr<float>(), 3);
      float G[3] = {0, 0, 0};
      if (!p->m_cvMat_posGlobalBA.empty()) for (int i = 0; i < 3; i++) G[i] = p->m_cvMat_posGlobalBA.at<float>(i);
      W.put(G, 3);
    }
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
