// TEST-ONLY: EXECUTES the matcher and stereo adapter bodies of include/ydorb/orbMatcher.hpp and include/ydorb/frame.hpp that
// adapter_run.cpp does not reach, on the GPU, against stand-ins of the reference's Frame / KeyFrame / MapPoint that carry real data,
// and dumps what each adapter returned and the full object state it left behind.  tests/matcher_adapters_support.py builds the
// scenarios, states the host side of every adapter independently (float32, one rounded operation at a time, in the arithmetic of the
// mock cv::Mat of tests/cpu_harness/mockrt), pushes the flat problem through the ctypes mirror and replays the bookkeeping;
// tests/test_matcher_adapters_gpu.py requires identical state.
//
//   matcher_adapters_run mappoint scenario.bin out.bin   searchByProjectionInFrameAndMapPoint        (orbMatcher.cpp:24-64)
//   matcher_adapters_run reloc    scenario.bin out.bin   searchByProjectionInKeyFrameAndCurrentFrame (orbMatcher.cpp:156-239)
//   matcher_adapters_run sim      scenario.bin out.bin   searchByProjectionInSim                     (orbMatcher.cpp:240-302)
//   matcher_adapters_run sim3     scenario.bin out.bin   searchBySim3                                (orbMatcher.cpp:566-681)
//   matcher_adapters_run fuse     scenario.bin out.bin   fuseByProjection, flat form                 (orbMatcher.cpp:682-745)
//   matcher_adapters_run fusesim  scenario.bin out.bin   fuseBySim3, flat form                       (orbMatcher.cpp:746-807)
//   matcher_adapters_run tri      scenario.bin out.bin   searchForTriangulation, flat form           (orbMatcher.cpp:463-565)
//   matcher_adapters_run stereo   scenario.bin out.bin   Frame::computeStereoMatches                 (frame.cpp:362-477)
//
// Every sub-command but `stereo` reads the same world (camera, pyramid, map points, keyframes, observations, one frame) followed by
// its own arguments, and writes: the return value, one result vector (the frame's or the caller's map-point vector as point indices,
// or the pairs), then every point's bad flag, replaced-by link and sorted observations and every keyframe's map-point vector.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ydorb/orbExtractor.hpp"
#include "../../include/ydorb/tracking.hpp"
#include "../../include/ydorb/frame.hpp"

namespace {

struct Reader {
  FILE* f;
  explicit Reader(const char* path) : f(fopen(path, "rb")) { if (!f) { perror(path); exit(2); } }
  ~Reader() { fclose(f); }
  template <class T> T get() { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "scenario truncated\n"); exit(2); } return v; }
  template <class T> void get(T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scenario truncated\n"); exit(2); } }
  bool atEnd() { const int c = fgetc(f); if (c == EOF) return true; ungetc(c, f); return false; }
};
struct Writer {
  FILE* f;
  explicit Writer(const char* path) : f(fopen(path, "wb")) { if (!f) { perror(path); exit(2); } }
  ~Writer() { fclose(f); }
  template <class T> void put(const T& v) { fwrite(&v, sizeof(T), 1, f); }
  template <class T> void put(const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
};

struct KeyFrame;
struct MapPoint;
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
typedef std::map<unsigned, std::vector<unsigned>> FeatureVector;

// ---- stand-ins with real storage: only the members the adapters touch (names as in reference src/*.hpp) -------------------------
struct Frame {
  std::vector<cv::KeyPoint> m_v_keyPoints, m_v_rightKeyPoints;
  cv::Mat m_cvMat_descriptors, m_cvMat_rightDescriptors, m_cvMat_T_c2w;
  std::vector<float> m_v_rightXcords, m_v_depth, m_v_scaleFactors;
  float m_flt_logScaleFactor = 0.f;
  std::vector<MP> m_v_sptrMapPoints;
  int m_int_keyPointsNum = 0;
  std::shared_ptr<YDORBSLAM::OrbExtractor> m_sptr_leftOrbExtractor, m_sptr_rightOrbExtractor;
  static float m_flt_minX, m_flt_maxX, m_flt_minY, m_flt_maxY, m_flt_fx, m_flt_fy, m_flt_cx, m_flt_cy, m_flt_baseLine, m_flt_baseLineTimesFx;
  bool isInImage(const float& x, const float& y) const { return x >= m_flt_minX && x < m_flt_maxX && y >= m_flt_minY && y < m_flt_maxY; }   // frame.cpp:291-294
};
float Frame::m_flt_minX, Frame::m_flt_maxX, Frame::m_flt_minY, Frame::m_flt_maxY, Frame::m_flt_fx, Frame::m_flt_fy, Frame::m_flt_cx, Frame::m_flt_cy,
    Frame::m_flt_baseLine, Frame::m_flt_baseLineTimesFx;

struct KeyFrame : std::enable_shared_from_this<KeyFrame> {
  int index = -1;
  cv::Mat R, t, O, m_cvMat_descriptors;      // the pose parts and the camera centre as the keyframe stores them (keyFrame.cpp setPose)
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords, m_v_scaleFactors, m_v_scaleFactorSquares, m_v_invScaleFactorSquares;
  float m_flt_logScaleFactor = 0.f;
  int m_int_keyPointsNum = 0;
  FeatureVector m_bow_keyPointsVec;
  std::vector<MP> mps;
  static float m_flt_minX, m_flt_maxX, m_flt_minY, m_flt_maxY;
  cv::Mat getRotation_c2w() { return R.clone(); }
  cv::Mat getTranslation_c2w() { return t.clone(); }
  cv::Mat getCameraOriginInWorld() { return O.clone(); }
  bool isInImage(const float& x, const float& y) const { return x >= m_flt_minX && x < m_flt_maxX && y >= m_flt_minY && y < m_flt_maxY; }
  MP getMapPoint(int idx) { return mps[(size_t)idx]; }
  void addMapPoint(const MP& mp, int idx) { mps[(size_t)idx] = mp; }
  std::vector<MP> getMatchedMapPointsVec() { return mps; }
  std::set<MP> getMatchedMapPointsSet() { std::set<MP> s; for (const MP& mp : mps) if (mp) s.insert(mp); return s; }
};
float KeyFrame::m_flt_minX, KeyFrame::m_flt_maxX, KeyFrame::m_flt_minY, KeyFrame::m_flt_maxY;

struct MapPoint : std::enable_shared_from_this<MapPoint> {
  int index = -1;
  cv::Mat pos, normal, desc;                 // 3x1 CV_32F twice, 1x32 CV_8U
  float minDist = 0.f, maxDist = 0.f;
  bool bad = false;
  std::map<KF, size_t> obs;
  MP replacedBy;
  bool m_b_isTrackInView = false;
  float m_flt_trackProjX = 0.f, m_flt_trackProjY = 0.f, m_flt_trackProjRightX = 0.f, m_flt_trackViewCos = 0.f;
  int m_int_trackScaleLevel = 0;
  bool isBad() { return bad; }
  int getObservationsNum() { return (int)obs.size(); }
  cv::Mat getDescriptor() { return desc.clone(); }           // mapPoint.hpp:63-66 returns a clone
  cv::Mat getPosInWorld() { return pos.clone(); }
  cv::Mat getNormal() { return normal.clone(); }
  float getMinDistanceInvariance() { return 0.8f * minDist; }
  float getMaxDistanceInvariance() { return 1.2f * maxDist; }
  bool isInKeyFrame(const KF& kf) { return obs.count(kf) != 0; }
  int getIdxInKeyFrame(const KF& kf) { auto it = obs.find(kf); return it == obs.end() ? -1 : (int)it->second; }
  void addObservation(const KF& kf, size_t idx) { if (!obs.count(kf)) obs[kf] = idx; }
  int predictScaleLevel(const float& dist, const KF& kf) { return ydorb::adapter::predictScaleLevelFormula(maxDist / dist, kf->m_flt_logScaleFactor, (int)kf->m_v_scaleFactors.size()); }
  int predictScaleLevel(const float& dist, const Frame& f) { return ydorb::adapter::predictScaleLevelFormula(maxDist / dist, f.m_flt_logScaleFactor, (int)f.m_v_scaleFactors.size()); }
  void beReplacedBy(const MP& by) {   // MapPoint::replace without its last line, the survivor's computeDistinctiveDescriptors()
    if (by.get() == this) return;
    const std::map<KF, size_t> held = obs;
    obs.clear();
    bad = true;
    replacedBy = by;
    for (const auto& ob : held) {
      if (!by->isInKeyFrame(ob.first)) { ob.first->mps[ob.second] = by; by->addObservation(ob.first, ob.second); }
      else ob.first->mps[ob.second].reset();
    }
  }
};

cv::Mat readMat32(Reader& R, int rows, int cols) { cv::Mat m(rows, cols, CV_32F); R.get(m.ptr<float>(), (size_t)rows * cols); return m; }
void readKeypoints(Reader& R, int n, std::vector<cv::KeyPoint>& kps, cv::Mat& desc, std::vector<float>& rightX) {
  kps.resize(n);
  R.get(reinterpret_cast<unsigned char*>(kps.data()), (size_t)n * sizeof(cv::KeyPoint));
  desc.create(std::max(n, 1), 32, CV_8U);
  R.get(desc.data, (size_t)n * 32);
  rightX.resize(n);
  R.get(rightX.data(), n);
}
void readFeatureVector(Reader& R, FeatureVector& fv) {
  const int nodes = R.get<int32_t>();
  for (int i = 0; i < nodes; i++) {
    const unsigned id = R.get<uint32_t>();
    const int m = R.get<int32_t>();
    std::vector<unsigned> f(m);
    R.get(f.data(), m);
    fv[id] = f;
  }
}
std::vector<MP> readPointList(Reader& R, const std::vector<MP>& mps) {
  const int n = R.get<int32_t>();
  std::vector<MP> out(n);
  for (int i = 0; i < n; i++) { const int k = R.get<int32_t>(); if (k >= 0) out[i] = mps[(size_t)k]; }
  return out;
}

struct World {
  std::vector<MP> points;
  std::vector<KF> kfs;
  Frame frame;
};

void readWorld(Reader& R, World& W) {
  float c[10];
  R.get(c, 10);
  Frame::m_flt_fx = c[0]; Frame::m_flt_fy = c[1]; Frame::m_flt_cx = c[2]; Frame::m_flt_cy = c[3]; Frame::m_flt_baseLine = c[4]; Frame::m_flt_baseLineTimesFx = c[5];
  Frame::m_flt_minX = KeyFrame::m_flt_minX = c[6]; Frame::m_flt_maxX = KeyFrame::m_flt_maxX = c[7];
  Frame::m_flt_minY = KeyFrame::m_flt_minY = c[8]; Frame::m_flt_maxY = KeyFrame::m_flt_maxY = c[9];
  std::vector<float> sf(8), sf2(8), inv2(8);
  R.get(sf.data(), 8);
  const float logSf = R.get<float>();
  for (int l = 0; l < 8; l++) { sf2[l] = sf[l] * sf[l]; inv2[l] = 1.0f / sf2[l]; }
  const int nMP = R.get<int32_t>();
  W.points.resize(nMP);
  for (int i = 0; i < nMP; i++) {
    MP mp = std::make_shared<MapPoint>();
    mp->index = i;
    mp->pos = readMat32(R, 3, 1);
    mp->normal = readMat32(R, 3, 1);
    mp->minDist = R.get<float>(); mp->maxDist = R.get<float>();
    mp->m_flt_trackProjX = R.get<float>(); mp->m_flt_trackProjY = R.get<float>(); mp->m_flt_trackProjRightX = R.get<float>(); mp->m_flt_trackViewCos = R.get<float>();
    mp->bad = R.get<int32_t>() != 0; mp->m_b_isTrackInView = R.get<int32_t>() != 0; mp->m_int_trackScaleLevel = R.get<int32_t>();
    mp->desc.create(1, 32, CV_8U);
    R.get(mp->desc.data, 32);
    W.points[i] = mp;
  }
  const int nKF = R.get<int32_t>();
  for (int k = 0; k < nKF; k++) {
    KF kf = std::make_shared<KeyFrame>();
    kf->index = k;
    kf->R = readMat32(R, 3, 3); kf->t = readMat32(R, 3, 1); kf->O = readMat32(R, 3, 1);
    kf->m_v_scaleFactors = sf; kf->m_v_scaleFactorSquares = sf2; kf->m_v_invScaleFactorSquares = inv2; kf->m_flt_logScaleFactor = logSf;
    const int n = R.get<int32_t>();
    kf->m_int_keyPointsNum = n;
    readKeypoints(R, n, kf->m_v_keyPoints, kf->m_cvMat_descriptors, kf->m_v_rightXcords);
    kf->mps.resize(n);
    for (int i = 0; i < n; i++) { const int p = R.get<int32_t>(); if (p >= 0) kf->mps[i] = W.points[(size_t)p]; }
    readFeatureVector(R, kf->m_bow_keyPointsVec);
    W.kfs.push_back(kf);
  }
  for (int i = 0; i < nMP; i++) {
    const int nobs = R.get<int32_t>();
    for (int o = 0; o < nobs; o++) { const int k = R.get<int32_t>(), idx = R.get<int32_t>(); W.points[i]->obs[W.kfs[(size_t)k]] = (size_t)idx; }
  }
  Frame& f = W.frame;
  f.m_cvMat_T_c2w = readMat32(R, 4, 4);
  f.m_v_scaleFactors = sf; f.m_flt_logScaleFactor = logSf;
  const int n = R.get<int32_t>();
  f.m_int_keyPointsNum = n;
  readKeypoints(R, n, f.m_v_keyPoints, f.m_cvMat_descriptors, f.m_v_rightXcords);
  f.m_v_sptrMapPoints.resize(n);
  for (int i = 0; i < n; i++) { const int p = R.get<int32_t>(); if (p >= 0) f.m_v_sptrMapPoints[i] = W.points[(size_t)p]; }
}

void writeResult(Writer& Wr, const World& W, int ret, const std::vector<int32_t>& vec) {
  Wr.put<int32_t>(ret);
  Wr.put<int32_t>((int32_t)vec.size());
  Wr.put(vec.data(), vec.size());
  for (const MP& mp : W.points) {
    Wr.put<int32_t>(mp->bad ? 1 : 0);
    Wr.put<int32_t>(mp->replacedBy ? mp->replacedBy->index : -1);
    std::vector<std::pair<int, int>> o;
    for (const auto& kv : mp->obs) o.push_back({kv.first->index, (int)kv.second});
    std::sort(o.begin(), o.end());
    Wr.put<int32_t>((int32_t)o.size());
    for (const auto& p : o) { Wr.put<int32_t>(p.first); Wr.put<int32_t>(p.second); }
  }
  for (const KF& kf : W.kfs) {
    Wr.put<int32_t>((int32_t)kf->mps.size());
    for (const MP& mp : kf->mps) Wr.put<int32_t>(mp ? mp->index : -1);
  }
}
std::vector<int32_t> indicesOf(const std::vector<MP>& v) {
  std::vector<int32_t> out;
  for (const MP& mp : v) out.push_back(mp ? mp->index : -1);
  return out;
}

int runWorld(const std::string& what, const char* in, const char* out) {
  namespace ya = ydorb::adapter;
  Reader R(in);
  World W;
  readWorld(R, W);
  ydorb_matcher_t* m = ya::matcher();
  int ret = 0;
  std::vector<int32_t> vec;
  if (what == "mappoint") {
    const std::vector<MP> list = readPointList(R, W.points);
    const float thd = R.get<float>(), ratio = R.get<float>();
    ret = ya::searchByProjectionInFrameAndMapPoint(m, W.frame, list, thd, ratio);
    vec = indicesOf(W.frame.m_v_sptrMapPoints);
  } else if (what == "reloc") {
    const KF kf = W.kfs[(size_t)R.get<int32_t>()];
    const std::vector<MP> foundList = readPointList(R, W.points);
    const std::set<MP> found(foundList.begin(), foundList.end());
    const float thd = R.get<float>();
    const int orbDist = R.get<int32_t>(), checkOri = R.get<int32_t>();
    ret = ya::searchByProjectionInKeyFrameAndCurrentFrame(m, W.frame, kf, found, thd, orbDist, checkOri != 0);
    vec = indicesOf(W.frame.m_v_sptrMapPoints);
  } else if (what == "sim") {
    const KF kf = W.kfs[(size_t)R.get<int32_t>()];
    const cv::Mat S = readMat32(R, 4, 4);
    const std::vector<MP> list = readPointList(R, W.points);
    std::vector<MP> matched = readPointList(R, W.points);
    const int th = R.get<int32_t>();
    ret = ya::searchByProjectionInSim<KF, MP, Frame>(m, kf, S, list, matched, th);
    vec = indicesOf(matched);
  } else if (what == "sim3") {
    const KF kf1 = W.kfs[(size_t)R.get<int32_t>()], kf2 = W.kfs[(size_t)R.get<int32_t>()];
    std::vector<MP> matched12 = readPointList(R, W.points);
    const float th = R.get<float>();
    ret = ya::searchBySim3<KF, MP, Frame>(m, kf1, kf2, matched12, th);
    vec = indicesOf(matched12);
  } else if (what == "fuse") {
    const KF kf = W.kfs[(size_t)R.get<int32_t>()];
    const std::vector<MP> list = readPointList(R, W.points);
    const float th = R.get<float>();
    ret = ya::fuseByProjection<KF, MP, Frame>(m, kf, list, th);
  } else if (what == "fusesim") {
    const KF kf = W.kfs[(size_t)R.get<int32_t>()];
    const cv::Mat S = readMat32(R, 4, 4);
    const std::vector<MP> list = readPointList(R, W.points);
    const float th = R.get<float>();
    ret = ya::fuseBySim3<KF, MP, Frame>(m, kf, S, list, th);
  } else if (what == "tri") {
    const KF kf1 = W.kfs[(size_t)R.get<int32_t>()], kf2 = W.kfs[(size_t)R.get<int32_t>()];
    const cv::Mat F12 = readMat32(R, 3, 3);
    const int stereoOnly = R.get<int32_t>(), checkOri = R.get<int32_t>();
    std::vector<std::pair<int, int>> pairs;
    pairs.push_back({-7, -7});   // the adapter clears what the caller left in it
    ret = ya::searchForTriangulation<KF, Frame>(m, kf1, kf2, F12, pairs, stereoOnly != 0, checkOri != 0);
    for (const auto& p : pairs) { vec.push_back(p.first); vec.push_back(p.second); }
  } else {
    return 2;
  }
  if (!R.atEnd()) { fprintf(stderr, "scenario has bytes the sub-command did not read\n"); return 2; }
  Writer Wr(out);
  writeResult(Wr, W, ret, vec);
  return 0;
}

// stereo: two images -> the adapter's two extractors -> computeStereoMatchesImpl.  variant 0: as is; 1: the right image yields no keypoints
// (an all-zero image is sent by the caller); 2: m_int_keyPointsNum is off by one (the adapter throws); 3: both descriptor matrices are
// column views of wider ones (not continuous).  Output: threw, status, n, m_v_rightXcords and m_v_depth as raw bits, then the left and
// right keypoints and descriptors the extractors gave, for the caller's own call on the same data.
int runStereo(const char* in, const char* out) {
  Reader R(in);
  const int w = R.get<int32_t>(), h = R.get<int32_t>(), nf = R.get<int32_t>(), flags = R.get<int32_t>(), variant = R.get<int32_t>();
  Frame::m_flt_baseLine = R.get<float>(); Frame::m_flt_baseLineTimesFx = R.get<float>();
  cv::Mat left(h, w, CV_8UC1), right(h, w, CV_8UC1);
  R.get(left.data, (size_t)w * h);
  R.get(right.data, (size_t)w * h);
  Frame f;
  f.m_sptr_leftOrbExtractor = std::make_shared<YDORBSLAM::OrbExtractor>(nf, 1.2f, 8, 20, 7);
  f.m_sptr_rightOrbExtractor = std::make_shared<YDORBSLAM::OrbExtractor>(nf, 1.2f, 8, 20, 7);
  f.m_sptr_leftOrbExtractor->extractAndCompute(left, f.m_v_keyPoints, f.m_cvMat_descriptors);
  f.m_sptr_rightOrbExtractor->extractAndCompute(right, f.m_v_rightKeyPoints, f.m_cvMat_rightDescriptors);
  f.m_int_keyPointsNum = (int)f.m_v_keyPoints.size() + (variant == 2 ? 1 : 0);
  const cv::Mat dl = f.m_cvMat_descriptors.clone(), dr = f.m_cvMat_rightDescriptors.clone();
  if (variant == 3) {
    auto widen = [](const cv::Mat& d) {
      cv::Mat wide(std::max(d.rows, 1), 48, CV_8U);
      for (int r = 0; r < wide.rows; r++) std::memset(wide.ptr<unsigned char>(r), 0xA5, 48);
      if (d.rows) d.copyTo(wide.rowRange(0, d.rows).colRange(8, 40));
      return wide.rowRange(0, d.rows).colRange(8, 40);
    };
    f.m_cvMat_descriptors = widen(dl);
    f.m_cvMat_rightDescriptors = widen(dr);
    if (f.m_cvMat_descriptors.isContinuous() || f.m_cvMat_rightDescriptors.isContinuous()) { fprintf(stderr, "the column views are continuous\n"); return 2; }
  }
  int threw = 0, status = 0;
  try {
    status = ydorb::adapter::computeStereoMatchesImpl(f, flags);
  } catch (const std::runtime_error&) {
    threw = 1;
  }
  Writer W(out);
  W.put<int32_t>(threw); W.put<int32_t>(status);
  W.put<int32_t>((int32_t)f.m_v_rightXcords.size());
  W.put(f.m_v_rightXcords.data(), f.m_v_rightXcords.size());
  W.put<int32_t>((int32_t)f.m_v_depth.size());
  W.put(f.m_v_depth.data(), f.m_v_depth.size());
  const int nl = (int)f.m_v_keyPoints.size(), nr = (int)f.m_v_rightKeyPoints.size();
  W.put<int32_t>(nl);
  W.put(reinterpret_cast<const unsigned char*>(f.m_v_keyPoints.data()), (size_t)nl * sizeof(cv::KeyPoint));
  for (int i = 0; i < nl; i++) W.put(dl.ptr<unsigned char>(i), 32);
  W.put<int32_t>(nr);
  W.put(reinterpret_cast<const unsigned char*>(f.m_v_rightKeyPoints.data()), (size_t)nr * sizeof(cv::KeyPoint));
  for (int i = 0; i < nr; i++) W.put(dr.ptr<unsigned char>(i), 32);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: matcher_adapters_run mappoint|reloc|sim|sim3|fuse|fusesim|tri|stereo scenario.bin out.bin\n"); return 2; }
  try {
    const std::string what = argv[1];
    if (what == "stereo") return runStereo(argv[2], argv[3]);
    return runWorld(what, argv[2], argv[3]);
  } catch (const std::exception& e) {
    fprintf(stderr, "matcher_adapters_run: %s\n", e.what());
    return 1;
  }
}
