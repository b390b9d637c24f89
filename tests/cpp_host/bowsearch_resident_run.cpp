// TEST-ONLY: EXECUTES the resident overloads searchByBowInTwoKeyFrames(Mirror&, ...) / searchByBowInKeyFrameAndFrame(Mirror&, ...) of
// include/ydorb/orbMatcher.hpp and trackReferenceKeyFrameSearchImpl of include/ydorb/tracking.hpp on the GPU, over a MapMirror with
// enableDescriptors(), enableFeatures() and enableBow(), beside the flat adapters called once per candidate on a second copy of the same
// stand-in keyframes (KeyFrame / MapPoint / Frame stand-ins that carry real data).  The flat side does what LoopClosing::computeSim3
// and Tracking::relocalize do around the search: a bad candidate keyframe is skipped and has no matches.  The scenario is the file
// tests/test_bowsearch_resident_adapter_gpu.py writes.  The program compares the two copies exactly - per candidate the ids of the
// matched map points and the count - and prints one line per figure, "<name> <value>".  OpenCV is the functional mock of
// tests/cpu_harness/mockrt.
//   bowsearch_resident_run scenario.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "../../include/ydorb/mapMirror.hpp"
#include "../../include/ydorb/orbMatcher.hpp"
#include "../../include/ydorb/tracking.hpp"

namespace {

struct Reader {
  FILE* f;
  explicit Reader(const char* path) : f(fopen(path, "rb")) { if (!f) { perror(path); exit(2); } }
  ~Reader() { fclose(f); }
  template <class T> T get() { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "scenario truncated\n"); exit(2); } return v; }
  template <class T> void get(T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scenario truncated\n"); exit(2); } }
};

struct KeyFrame;
typedef std::shared_ptr<KeyFrame> KF;
struct MapPoint {
  int id = -1;
  bool bad = false;
  cv::Mat pos;
  KF ref;
  std::map<KF, size_t> held;
  bool isBad() { return bad; }
  std::map<KF, size_t> getObservations() { return held; }
  KF getReferenceKeyFrame() { return ref; }
  cv::Mat getPosInWorld() { return pos.clone(); }
};
typedef std::shared_ptr<MapPoint> MP;
typedef std::map<unsigned, std::vector<unsigned>> FeatureVector;
struct Frame {
  int m_int_keyPointsNum = 0;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  cv::Mat m_cvMat_descriptors;
  FeatureVector m_bow_keyPointsVec;
};
struct KeyFrame {
  int index = -1;
  long int m_int_keyFrameID = 0;
  bool bad = false;
  cv::Mat O, m_cvMat_descriptors;
  std::vector<cv::KeyPoint> m_v_keyPoints;
  std::vector<float> m_v_rightXcords;
  int m_int_keyPointsNum = 0;
  FeatureVector m_bow_keyPointsVec;
  std::vector<MP> mps;
  std::vector<MP> getMapPointMatches() { return mps; }
  std::vector<MP> getMatchedMapPointsVec() { return mps; }
  bool isBad() { return bad; }
  cv::Mat getCameraOriginInWorld() { return O.clone(); }
};
typedef ydorb::adapter::MapMirror<KF, MP> Mirror;

template <class T> void readFeatures(Reader& R, T& x) {
  const int n = R.get<int32_t>();
  x.m_int_keyPointsNum = n;
  x.m_v_keyPoints.resize(n);
  R.get(reinterpret_cast<unsigned char*>(x.m_v_keyPoints.data()), (size_t)n * sizeof(cv::KeyPoint));
  x.m_cvMat_descriptors.create(std::max(n, 1), 32, CV_8U);
  R.get(x.m_cvMat_descriptors.data, (size_t)n * 32);
  const int nodes = R.get<int32_t>();
  for (int i = 0; i < nodes; i++) {
    const unsigned id = R.get<uint32_t>();
    const int m = R.get<int32_t>();
    std::vector<unsigned> f(m);
    R.get(f.data(), m);
    x.m_bow_keyPointsVec[id] = f;
  }
}

struct World {
  std::vector<MP> points;
  std::vector<KF> kfs;   // kfs[0] is the current keyframe, the rest the candidates
  Frame frame;
};

// the same file gives the same world: the two copies are read independently and share no object
World load(const char* path) {
  Reader R(path);
  World W;
  const int nPoints = R.get<int32_t>();
  std::vector<uint8_t> bad(nPoints);
  R.get(bad.data(), nPoints);
  for (int p = 0; p < nPoints; p++) {
    auto mp = std::make_shared<MapPoint>();
    mp->id = p; mp->bad = bad[p] != 0;
    mp->pos = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) mp->pos.ptr<float>()[r] = (float)(p + r);
    W.points.push_back(mp);
  }
  const int nKF = R.get<int32_t>();
  for (int k = 0; k < nKF; k++) {
    auto kf = std::make_shared<KeyFrame>();
    kf->index = k; kf->m_int_keyFrameID = k;
    kf->bad = R.get<int32_t>() != 0;
    kf->O = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) kf->O.ptr<float>()[r] = (float)k;
    readFeatures(R, *kf);
    const int n = kf->m_int_keyPointsNum;
    kf->m_v_rightXcords.assign(n, -1.0f);
    std::vector<int32_t> row(n);
    R.get(row.data(), n);
    kf->mps.resize(n);
    for (int i = 0; i < n; i++)
      if (row[i] >= 0) {
        kf->mps[i] = W.points[row[i]];
        W.points[row[i]]->held[kf] = (size_t)i;
        if (!W.points[row[i]]->ref) W.points[row[i]]->ref = kf;
      }
    W.kfs.push_back(kf);
  }
  readFeatures(R, W.frame);
  return W;
}

std::vector<int> ids(const std::vector<MP>& v) {
  std::vector<int> out;
  for (const MP& mp : v) out.push_back(mp ? mp->id : -1);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: bowsearch_resident_run scenario.bin\n"); return 2; }
  namespace ya = ydorb::adapter;
  try {
    World A = load(argv[1]), B = load(argv[1]);
    const float ratio = 0.75f;
    const std::vector<KF> candA(A.kfs.begin() + 1, A.kfs.end()), candB(B.kfs.begin() + 1, B.kfs.end());
    const size_t nc = candA.size();
    // the flat side, one call per candidate that is not bad
    std::vector<std::vector<MP>> loopA(nc), relocA(nc);
    std::vector<int> nLoopA(nc, 0), nRelocA(nc, 0);
    for (size_t i = 0; i < nc; i++) {
      loopA[i].assign(A.kfs[0]->mps.size(), MP());
      relocA[i].assign(A.frame.m_v_keyPoints.size(), MP());
      if (candA[i]->isBad()) continue;
      nLoopA[i] = ya::searchByBowInTwoKeyFrames(ya::matcher(), A.kfs[0], candA[i], loopA[i], ratio, true);
      nRelocA[i] = ya::searchByBowInKeyFrameAndFrame(ya::matcher(), candA[i], A.frame, relocA[i], ratio, true);
    }
    std::vector<MP> refA;
    const int nRefA = ya::searchByBowInKeyFrameAndFrame(ya::matcher(), A.kfs[0], A.frame, refA, 0.7f, true);
    // the resident side: one call per form
    Mirror mirror(0, 64, 2, 256);   // small: every table grows while the scene is loaded
    mirror.enableDescriptors();
    mirror.enableFeatures();
    mirror.enableBow();
    // the current keyframe is touched as LocalMapping would have it; the candidates are met by the call for the first time
    mirror.touch(B.kfs[0]); mirror.touchRow(B.kfs[0]); mirror.touchDescriptors(B.kfs[0]); mirror.touchFeatures(B.kfs[0]); mirror.touchBow(B.kfs[0]);
    std::vector<std::vector<MP>> loopB, relocB;
    const std::vector<int> nLoopB = ya::searchByBowInTwoKeyFrames(mirror, ya::matcher(), B.kfs[0], candB, loopB, ratio, true);
    const std::vector<int> nRelocB = ya::searchByBowInKeyFrameAndFrame(mirror, ya::matcher(), candB, B.frame, relocB, ratio, true);
    std::vector<MP> refB;
    const int nRefB = ya::trackReferenceKeyFrameSearchImpl(mirror, ya::matcher(), B.frame, B.kfs[0], refB);
    int loopSame = nLoopB.size() == nc && loopB.size() == nc, relocSame = nRelocB.size() == nc && relocB.size() == nc, bad = 0, loopAll = 0, relocAll = 0, loopMin = 1 << 30,
        relocMin = 1 << 30;
    for (size_t i = 0; i < nc && loopSame && relocSame; i++) {
      loopSame = loopSame && nLoopA[i] == nLoopB[i] && ids(loopA[i]) == ids(loopB[i]);
      relocSame = relocSame && nRelocA[i] == nRelocB[i] && ids(relocA[i]) == ids(relocB[i]);
      loopAll += nLoopB[i]; relocAll += nRelocB[i];
      if (candB[i]->isBad()) { bad++; continue; }
      loopMin = std::min(loopMin, nLoopB[i]); relocMin = std::min(relocMin, nRelocB[i]);
    }
    printf("candidates %d\nbad_candidates %d\nloop_same %d\nreloc_same %d\nloop_matches %d\nreloc_matches %d\nloop_min %d\nreloc_min %d\n", (int)nc, bad, loopSame, relocSame,
           loopAll, relocAll, loopMin, relocMin);
    printf("reference_same %d\nreference_matches %d\n", nRefA == nRefB && ids(refA) == ids(refB) ? 1 : 0, nRefB);
    const auto st = mirror.searchByBowKeyFrames(ya::matcher(), B.kfs[0], candB, ratio, true).pairStatus;
    int unusable = 0;
    for (size_t i = 0; i < st.size(); i++) unusable += st[i] != 0 && candB[i]->isBad();
    printf("bad_candidates_unusable %d\n", unusable);
    const Mirror::Difference d = mirror.verify(), dd = mirror.verifyDescriptors();
    printf("verify_after %d\n", (int)(d.pointSlots.size() + d.keyFrameSlots.size() + dd.pointSlots.size() + dd.keyFrameSlots.size() + mirror.verifyRows().size() +
                                      mirror.verifyFeatures().size() + mirror.verifyBow().size()));
    // a point goes bad and a row entry is cleared: with the touches the reference's bookkeeping already makes, the next call follows
    MP gone;
    for (size_t j = 0; j < loopB[0].size() && !gone; j++) gone = loopB[0][j];
    int followed = -1;
    if (gone) {
      gone->bad = true; mirror.touch(gone);
      A.points[gone->id]->bad = true;
      std::vector<std::vector<MP>> l2;
      const std::vector<int> n2 = ya::searchByBowInTwoKeyFrames(mirror, ya::matcher(), B.kfs[0], candB, l2, ratio, true);
      std::vector<MP> f2(A.kfs[0]->mps.size());
      const int nf2 = ya::searchByBowInTwoKeyFrames(ya::matcher(), A.kfs[0], candA[0], f2, ratio, true);
      followed = n2[0] == nf2 && ids(l2[0]) == ids(f2);
      for (const MP& mp : l2[0]) followed = followed && mp != gone;
    }
    printf("bad_point_followed %d\n", followed);
    // a mirror without enableBow() refuses
    Mirror plain(0, 64, 2, 256);
    plain.enableDescriptors();
    plain.enableFeatures();
    int refused = 0;
    try { std::vector<std::vector<MP>> x; ya::searchByBowInTwoKeyFrames(plain, ya::matcher(), B.kfs[0], candB, x, ratio, true); } catch (const std::runtime_error& e) {
      refused += std::strstr(e.what(), "without enableDescriptors(), enableFeatures() and enableBow()") != nullptr;
    }
    try { std::vector<std::vector<MP>> x; ya::searchByBowInKeyFrameAndFrame(plain, ya::matcher(), candB, B.frame, x, ratio, true); } catch (const std::runtime_error& e) {
      refused += std::strstr(e.what(), "without enableDescriptors(), enableFeatures() and enableBow()") != nullptr;
    }
    printf("refused_without_bow %d\n", refused);
    // the current keyframe itself goes bad, touched as setBadFlag's lines say: the table holds no features of it any more, and the
    // call answers with a status per candidate and all-null vectors of the keyframe's length, it does not throw
    B.kfs[0]->bad = true;
    mirror.touchDescriptors(B.kfs[0]); mirror.touchFeatures(B.kfs[0]); mirror.touchBow(B.kfs[0]);
    std::vector<std::vector<MP>> l3;
    const std::vector<int> n3 = ya::searchByBowInTwoKeyFrames(mirror, ya::matcher(), B.kfs[0], candB, l3, ratio, true);
    const auto st3 = mirror.searchByBowKeyFrames(ya::matcher(), B.kfs[0], candB, ratio, true).pairStatus;
    int answered = n3.size() == nc && l3.size() == nc && st3.size() == nc;
    for (size_t i = 0; i < nc && answered; i++) {
      answered = n3[i] == 0 && st3[i] == YDORB_BOW_PAIR_NO_FEATURES && l3[i].size() == B.kfs[0]->mps.size();
      for (const MP& mp : l3[i]) answered = answered && !mp;
    }
    printf("bad_first_answers %d\n", answered);
  } catch (const std::exception& e) {
    fprintf(stderr, "bowsearch_resident_run: %s\n", e.what());
    return 1;
  }
  return 0;
}
