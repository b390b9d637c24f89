// Host side of the local-BA graph query on the resident table (include/ydorb/c_api.h, "Local BA graph"; DESIGN.md section 2 "Local BA
// graph on the resident table: the integer contract", section 6u): the validation of ydorb_mapdb_local_ba_graph, the layout of its
// result in the handle's pinned memory, and the whole contract executed on host arrays in the layout the kernels read, as the
// reference's sequential loops (optimizer.hpp:59-113).  The driver runs the kernels of mapdb_lba_kernels.hip.h; the stand-alone check
// (tests/cpu_harness/mapdb_lba_check.cpp) runs lbaOnHost against a std::map model.  No HIP here: a plain host compiler builds it.
//   result    one area, every array 16-byte aligned, the same offsets on the device and in the pinned copy.  It is laid out once the
//             three counts (points, edges, fixed keyframes) have been read back, so nothing in it is sized by a bound; the poses, which
//             the caller fills, lie behind what the device writes and exist in the pinned copy only.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "layout.h"
#include "map_table.h"
#include "mapdb_desc_host.h"
#include "mapdb_feat_host.h"
#include "mapdb_rows_host.h"

namespace ydorb {
namespace mapdb {

// Refusals of ydorb_mapdb_local_ba_graph, in the order the header lists them.  nKfAll: the table's n_keyframes, staged slots included.
// mark [nKfAll] is scratch for the repeat test; it is all zero before and after.
inline bool checkLbaArgs(const int32_t* kfSlots, int32_t nKf, const float* invLevelSigma2, const void* out, int32_t nKfAll, bool featuresEnabled,
                         std::vector<uint8_t>& mark, std::string& err) {
  if (!out) return fail(err, "null out");
  if (nKf < 0) return fail(err, "negative number of keyframe slots: %lld", nKf);
  if (nKf > 0 && !kfSlots) return fail(err, "null kf_slots");
  if (!invLevelSigma2) return fail(err, "null inv_level_sigma2");
  if (!FeatHost::checkEnabled(featuresEnabled, err)) return false;
  if (!RowsHost::checkKfSlots(kfSlots, nKf, nKfAll, err)) return false;
  mark.resize((size_t)nKfAll, 0);
  int32_t repeatAt = -1;
  for (int32_t i = 0; i < nKf && repeatAt < 0; i++) {
    if (mark[(size_t)kfSlots[i]]) repeatAt = i;
    else mark[(size_t)kfSlots[i]] = 1;
  }
  for (int32_t i = 0; i < nKf; i++) mark[(size_t)kfSlots[i]] = 0;
  if (repeatAt >= 0) return fail(err, "kf_slots[%lld]: keyframe slot %lld is named twice", repeatAt, kfSlots[repeatAt]);
  return true;
}

// Where the arrays of a result lie.  maxPoses / maxPoints / maxEdges: what the area is sized for.
struct LbaLayout {
  size_t oPoseFixed = 0, oPoseKf = 0, oPointSlot = 0, oStatus = 0, oPoints = 0, oEdgePose = 0, oEdgePoint = 0, oEdgeKf = 0, oEdgeIdx = 0, oMeas = 0,
         oInfo = 0, devBytes = 0, oPoses = 0, bytes = 0;
  LbaLayout() = default;
  LbaLayout(size_t nPoses, size_t nPoints, size_t nEdges) {
    Layout L;
    oPoseFixed = L.add(nPoses); oPoseKf = L.add(4 * nPoses);
    oPointSlot = L.add(4 * nPoints); oStatus = L.add(nPoints); oPoints = L.add(24 * nPoints);
    oEdgePose = L.add(4 * nEdges); oEdgePoint = L.add(4 * nEdges); oEdgeKf = L.add(4 * nEdges); oEdgeIdx = L.add(4 * nEdges);
    oMeas = L.add(24 * nEdges); oInfo = L.add(8 * nEdges);
    L.add(16);             // never an empty area
    devBytes = L.bytes;    // what the device writes and the one read-back copies
    oPoses = L.add(56 * nPoses);   // the caller's: in the pinned copy only
    bytes = L.bytes;
  }
};

// Points *out at the arrays of `L` in `base` (the pinned copy)
inline void lbaPointResult(const LbaLayout& L, uint8_t* base, int32_t nLocal, int32_t nFixed, int32_t nPoints, int32_t nEdges, YdLocalBaGraph* out) {
  *out = YdLocalBaGraph{};
  YdBaProblem& P = out->problem;
  P.n_poses = nLocal + nFixed; P.n_points = nPoints; P.n_edges = nEdges;
  P.poses = reinterpret_cast<double*>(base + L.oPoses); P.pose_fixed = base + L.oPoseFixed; P.points = reinterpret_cast<double*>(base + L.oPoints);
  P.edge_pose = reinterpret_cast<const int32_t*>(base + L.oEdgePose); P.edge_point = reinterpret_cast<const int32_t*>(base + L.oEdgePoint);
  P.edge_meas = reinterpret_cast<const double*>(base + L.oMeas); P.edge_inv_sigma2 = reinterpret_cast<const double*>(base + L.oInfo);
  out->n_local = nLocal; out->n_fixed = nFixed;
  out->pose_kf = reinterpret_cast<const int32_t*>(base + L.oPoseKf); out->point_slot = reinterpret_cast<const int32_t*>(base + L.oPointSlot);
  out->edge_kf = reinterpret_cast<const int32_t*>(base + L.oEdgeKf); out->edge_idx = reinterpret_cast<const int32_t*>(base + L.oEdgeIdx);
  out->point_status = base + L.oStatus;
}

struct LbaHostGraph {
  int32_t nLocal = 0, nFixed = 0;
  std::vector<int32_t> poseKf, pointSlot, edgePose, edgePoint, edgeKf, edgeIdx;
  std::vector<uint8_t> poseFixed, pointStatus;
  std::vector<double> points, meas, info;
};

// The contract on host tables, written as the reference's loops.  bad [nPoints] / pos [nPoints][3]: the point table's columns.  A slot
// at or past a header table's size has no span.  The arguments are valid (checkLbaArgs).
inline void lbaOnHost(const RowTables& R, const ViewTables& V, const FeatTables& F, const uint8_t* bad, const float* pos, int32_t nKfAll, const int32_t* kfSlots,
                      int32_t nKf, const float* invLevelSigma2, LbaHostGraph& G) {
  G = LbaHostGraph{};
  const auto spanLen = [](const std::vector<int32_t>& len, int32_t k) { return (size_t)k < len.size() ? len[(size_t)k] : 0; };
  std::vector<int32_t> poseOf((size_t)nKfAll, -1);
  std::vector<uint8_t> fixedTag((size_t)nKfAll, 0);
  for (int32_t i = 0; i < nKf; i++) { poseOf[(size_t)kfSlots[i]] = i; G.poseKf.push_back(kfSlots[i]); G.poseFixed.push_back(0); }
  G.nLocal = nKf;
  // local points: the rows in the order given, null and bad entries skipped, every slot at its first occurrence (:66-69)
  std::vector<uint8_t> tagged;
  for (int32_t i = 0; i < nKf; i++) {
    const int32_t k = kfSlots[i], len = spanLen(R.rowLen, k);
    for (int32_t q = 0; q < len; q++) {
      const int32_t s = R.pool.at((size_t)(R.rowStart[(size_t)k] + q));
      if (s < 0 || bad[s]) continue;
      if ((size_t)s >= tagged.size()) tagged.resize((size_t)s + 1, 0);
      if (tagged[(size_t)s]) continue;
      tagged[(size_t)s] = 1;
      G.pointSlot.push_back(s);
    }
  }
  // a view is usable when its keyframe has features (= !isBad()) and idx lies inside them
  const auto usable = [&](int32_t kf, int32_t idx, uint8_t& status) {
    const int32_t flen = spanLen(F.len, kf);
    if (flen == 0) { status |= YDORB_LBA_POINT_SKIPPED_VIEWS; return false; }
    if (idx >= flen) { status |= YDORB_LBA_POINT_VIEW_OUT_OF_RANGE; return false; }
    return true;
  };
  const size_t nP = G.pointSlot.size();
  G.pointStatus.assign(nP, 0);
  // fixed keyframes: the other usable observers, at their first occurrence in the walk (:70-76)
  for (size_t p = 0; p < nP; p++) {
    const int32_t s = G.pointSlot[p], m = spanLen(V.rowLen, s) / 2;
    for (int32_t j = 0; j < m; j++) {
      const int32_t kf = V.pool.at((size_t)(V.rowStart[(size_t)s] + 2 * j)), idx = V.pool.at((size_t)(V.rowStart[(size_t)s] + 2 * j + 1));
      (void)idx;   // an occurrence whatever its idx: a view past the features still names a keyframe that is not bad
      if (poseOf[(size_t)kf] >= 0 || fixedTag[(size_t)kf] || spanLen(F.len, kf) == 0) continue;
      fixedTag[(size_t)kf] = 1;
      poseOf[(size_t)kf] = (int32_t)G.poseKf.size();
      G.poseKf.push_back(kf); G.poseFixed.push_back(1);
      G.nFixed++;
    }
  }
  // edges (:99-113): every usable observer is local or fixed by now, so the pose lookup never misses
  G.points.resize(3 * nP);
  for (size_t p = 0; p < nP; p++) {
    const int32_t s = G.pointSlot[p], m = spanLen(V.rowLen, s) / 2;
    for (int d = 0; d < 3; d++) G.points[3 * p + (size_t)d] = (double)pos[3 * (size_t)s + (size_t)d];
    uint8_t status = 0;
    int32_t emitted = 0;
    for (int32_t j = 0; j < m; j++) {
      const int32_t kf = V.pool.at((size_t)(V.rowStart[(size_t)s] + 2 * j)), idx = V.pool.at((size_t)(V.rowStart[(size_t)s] + 2 * j + 1));
      if (!usable(kf, idx, status)) continue;
      const size_t at = (size_t)F.start[(size_t)kf] + (size_t)idx;
      const YdKeyPoint& kp = F.kps.at(at);
      const float ur = F.rightX.at(at);
      G.edgePose.push_back(poseOf[(size_t)kf]); G.edgePoint.push_back((int32_t)p);
      G.meas.push_back((double)kp.x); G.meas.push_back((double)kp.y); G.meas.push_back(ur < 0 ? -1.0 : (double)ur);
      G.info.push_back((double)invLevelSigma2[kp.octave]);
      G.edgeKf.push_back(kf); G.edgeIdx.push_back(idx);
      emitted++;
    }
    if (emitted == 0) status |= YDORB_LBA_POINT_NO_EDGES;
    G.pointStatus[p] = status;
  }
}

}  // namespace mapdb
}  // namespace ydorb
