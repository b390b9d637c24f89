// CPU restatement of the graph assembly of localBundleAdjust (include/ydorb/optimizer.hpp:59-113; the reference's
// src/optimizer.cpp:140-283) on flat arrays, for the tests of ydorb_mapdb_local_ba_graph.  The loops are the adapter's, one for one:
// the m_int_localBAForKeyFrameID / m_int_fixedBAForKeyFrameID tags are arrays per keyframe and per point, getMatchedMapPointsVec() is
// a keyframe's row, getObservations() is a point's view span in span order (the order of the std::map), isBad() of a keyframe is "no
// features", m_v_keyPoints / m_v_rightXcords are the feature arrays.  It shares no code with ydorbslam_amd/csrc.
//   keyframe k: row = rowSlot[rowStart[k] .. rowStart[k+1]), features = kps / rightX [featStart[k] .. featStart[k+1])
//   point p:    views = (viewKf, viewIdx)[viewStart[p] .. viewStart[p+1])
// The one thing the reference cannot hold is a view whose idx is not below the keyframe's feature count: it is skipped with status 2.
#include <stddef.h>

#include <cstdint>
#include <list>
#include <map>
#include <vector>

namespace {
struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };
static_assert(sizeof(KeyPoint) == 28, "cv::KeyPoint-compatible");
}  // namespace

// counts [4] = n_local, n_fixed, n_points, n_edges.  The output arrays hold nKfAll poses, nPoints points and viewStart[nPoints] edges.
extern "C" int localbaref_graph(int nKfAll, int nPoints, const int32_t* rowStart, const int32_t* rowSlot, const uint8_t* bad, const float* pos,
                                const int32_t* viewStart, const int32_t* viewKf, const int32_t* viewIdx, const int32_t* featStart, const void* kps_,
                                const float* rightX, const int32_t* kfSlots, int nKf, const float* invScaleFactorSquares, int32_t* counts,
                                int32_t* poseKf, uint8_t* poseFixed, int32_t* pointSlot, uint8_t* pointStatus, double* points, int32_t* edgePose,
                                int32_t* edgePoint, int32_t* edgeKf, int32_t* edgeIdx, double* edgeMeas, double* edgeInfo) {
  const KeyPoint* kps = static_cast<const KeyPoint*>(kps_);
  const auto isBadKf = [&](int k) { return featStart[k + 1] == featStart[k]; };
  std::vector<uint8_t> localTag((size_t)nKfAll, 0), fixedTag((size_t)nKfAll, 0), pointTag((size_t)nPoints, 0);
  // local keyframes: the caller's list (the covisibility walk stays on the host and leaves bad keyframes out)
  std::list<int> localKFs;
  for (int i = 0; i < nKf; i++) { localKFs.push_back(kfSlots[i]); localTag[(size_t)kfSlots[i]] = 1; }
  std::list<int> localMPs;
  for (const int k : localKFs)
    for (int q = rowStart[k]; q < rowStart[k + 1]; q++) {
      const int mp = rowSlot[q];
      if (mp >= 0 && !bad[mp] && !pointTag[(size_t)mp]) { localMPs.push_back(mp); pointTag[(size_t)mp] = 1; }
    }
  std::list<int> fixedKFs;
  for (const int mp : localMPs)
    for (int v = viewStart[mp]; v < viewStart[mp + 1]; v++) {
      const int k = viewKf[v];
      if (!localTag[(size_t)k] && !fixedTag[(size_t)k]) {
        fixedTag[(size_t)k] = 1;
        if (!isBadKf(k)) fixedKFs.push_back(k);
      }
    }
  // flat graph
  std::map<long, int> poseIndex;
  int nPoses = 0;
  long maxKFid = 0;
  const auto addPose = [&](int k, bool fix) {
    poseIndex[k] = nPoses;
    poseKf[nPoses] = k; poseFixed[nPoses] = fix ? 1 : 0;
    nPoses++;
    if (k > maxKFid) maxKFid = k;
  };
  for (const int k : localKFs) addPose(k, false);
  const int nLocal = nPoses;
  for (const int k : fixedKFs) addPose(k, true);
  int nP = 0, nE = 0;
  for (const int mp : localMPs) {
    const int p = nP++;
    pointSlot[p] = mp;
    for (int d = 0; d < 3; d++) points[3 * p + d] = pos[3 * mp + d];
    uint8_t status = 0;
    int emitted = 0;
    for (int v = viewStart[mp]; v < viewStart[mp + 1]; v++) {
      const int k = viewKf[v], idx = viewIdx[v];
      if (isBadKf(k)) { status |= 1; continue; }
      if (idx >= featStart[k + 1] - featStart[k]) { status |= 2; continue; }
      if (k > maxKFid) continue;
      const auto it = poseIndex.find(k);
      if (it == poseIndex.end()) continue;
      const KeyPoint& kp = kps[featStart[k] + idx];
      const float ur = rightX[featStart[k] + idx];
      edgePose[nE] = it->second; edgePoint[nE] = p;
      edgeMeas[3 * nE] = kp.x; edgeMeas[3 * nE + 1] = kp.y; edgeMeas[3 * nE + 2] = ur < 0 ? -1.0 : (double)ur;
      edgeInfo[nE] = invScaleFactorSquares[kp.octave];
      edgeKf[nE] = k; edgeIdx[nE] = idx;
      nE++; emitted++;
    }
    if (!emitted) status |= 4;
    pointStatus[p] = status;
  }
  counts[0] = nLocal; counts[1] = nPoses - nLocal; counts[2] = nP; counts[3] = nE;
  return 0;
}
