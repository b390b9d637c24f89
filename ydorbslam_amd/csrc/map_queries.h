// The host body of the three map queries (normal and depth, covisibility, keyframe redundancy), one per query, run by the flat
// entries of map_maintenance.hip and the resident entries of map_resident.hip alike.  A body lays the upload and read-back areas
// out, stages the caller's arrays, uploads in one copy, runs the one kernel of map_kernels.hip.h, reads back in one copy,
// synchronises and copies out.  What differs between the two routes is where the table (and, for normal and depth, the point
// attributes) comes from: a MapSource says so.  The caller has validated, holds c.mu, has made the device current and, on the
// resident route, has applied what was staged.  Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/ydorb/c_api.h"
#include "host_buffers.h"
#include "map_kernels.hip.h"
#include "map_table.h"

namespace ydorb {
namespace mapmaint {

// where a flat table's arrays sit in the upload area
struct TableAt {
  size_t start, kf, level, bad, nObs;
  void lay(Layout& U, const YdObservationTable* T) {
    nObs = (size_t)T->obs_start[T->n_points];
    start = U.add(4 * ((size_t)T->n_points + 1)); kf = U.add(4 * nObs); level = U.add(nObs); bad = U.add((size_t)T->n_points);
  }
  void stage(Mem& h, const YdObservationTable* T) const {
    std::memcpy(at<void>(h, start), T->obs_start, 4 * ((size_t)T->n_points + 1));
    if (nObs) { std::memcpy(at<void>(h, kf), T->obs_kf, 4 * nObs); std::memcpy(at<void>(h, level), T->obs_level, nObs); }
    if (T->n_points) std::memcpy(at<void>(h, bad), T->bad, (size_t)T->n_points);
  }
  Table device(Mem& d, const YdObservationTable* T) const {
    Table t;
    t.nPoints = T->n_points; t.nKeyframes = T->n_keyframes;
    t.obsStart = at<int>(d, start); t.obsEnd = t.obsStart + 1; t.obsKf = at<int>(d, kf); t.obsLevel = at<uint8_t>(d, level); t.bad = at<uint8_t>(d, bad);
    return t;
  }
};

// Where a query's table comes from.  Flat (`flat` set): the caller's table travels in the query's one upload, ahead of the query's
// own arrays.  Resident (`flat` null): `resident` already points into the handle's arenas and no table byte moves.
// Normal and depth reads point attributes too.  Flat: pos, refKf, refLevel [n_points] and centre [n_keyframes] are host arrays and
// go up behind the table, and every point is updated.  Resident: they are the handle's device arrays, and `slots` [n], a host
// array, is what goes up.
struct MapSource {
  const YdObservationTable* flat = nullptr;
  Table resident{};
  const float *pos = nullptr, *centre = nullptr;
  const int32_t* refKf = nullptr;
  const uint8_t* refLevel = nullptr;
  const int32_t* slots = nullptr;
  TableAt ta{};
  size_t oPos = 0, oCen = 0, oRef = 0, oLvl = 0, oSlots = 0;

  void lay(Layout& U) { if (flat) ta.lay(U, flat); }
  void stage(Mem& hUp) const { if (flat) ta.stage(hUp, flat); }
  Table device(Mem& up) const { return flat ? ta.device(up, flat) : resident; }   // only after the buffers have grown
  size_t nKeyframes() const { return (size_t)(flat ? flat->n_keyframes : resident.nKeyframes); }

  void layPoints(Layout& U, size_t n) {
    if (flat) { oPos = U.add(12 * n); oCen = U.add(12 * nKeyframes()); oRef = U.add(4 * n); oLvl = U.add(n); }
    else oSlots = U.add(4 * n);
  }
  void stagePoints(Mem& hUp, size_t n) const {
    if (!flat) { std::memcpy(at<void>(hUp, oSlots), slots, 4 * n); return; }
    const size_t nk = nKeyframes();
    std::memcpy(at<void>(hUp, oPos), pos, 12 * n);
    if (nk) std::memcpy(at<void>(hUp, oCen), centre, 12 * nk);
    std::memcpy(at<void>(hUp, oRef), refKf, 4 * n);
    std::memcpy(at<void>(hUp, oLvl), refLevel, n);
  }
  void devicePoints(Mem& up, NormalArgs& a) const {
    if (flat) { a.pos = at<float>(up, oPos); a.centre = at<float>(up, oCen); a.refKf = at<int>(up, oRef); a.refLevel = at<uint8_t>(up, oLvl); a.slots = nullptr; }
    else { a.pos = pos; a.centre = centre; a.refKf = refKf; a.refLevel = refLevel; a.slots = at<int>(up, oSlots); }
  }
};

// Where runNormalDepth left the slots it was given and its results on the device; they stay until the context's buffers are used again
struct NormalDepthOnDevice {
  const int* slots = nullptr;
  const float *normal = nullptr, *minDistance = nullptr, *maxDistance = nullptr;
  const uint8_t* status = nullptr;
};

// n > 0 points: all of a flat table's, or the resident table's `slots`
inline int runNormalDepth(StagedCtx& c, MapSource& src, int32_t n, const float* scale_factors, int32_t n_levels, float* normal,
                          float* min_distance, float* max_distance, uint8_t* status, NormalDepthOnDevice* where = nullptr) {
  const size_t np = (size_t)n;
  Layout U;
  src.lay(U);
  src.layPoints(U, np);
  Layout D;
  const size_t dNrm = D.add(12 * np), dMin = D.add(4 * np), dMax = D.add(4 * np), dSt = D.add(np);
  int rc;
  if ((rc = c.ensure(U.bytes, D.bytes))) return rc;
  src.stage(c.hUp);
  src.stagePoints(c.hUp, np);
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  NormalArgs a;
  a.t = src.device(c.up);
  src.devicePoints(c.up, a);
  for (int i = 0; i < 8; i++) a.scaleFactors[i] = i < n_levels ? scale_factors[i] : 0.f;
  a.nLevels = n_levels;
  a.n = n;
  a.normal = at<float>(c.down, dNrm); a.minDistance = at<float>(c.down, dMin); a.maxDistance = at<float>(c.down, dMax);
  a.status = at<uint8_t>(c.down, dSt);
  hipLaunchKernelGGL(k_normal_depth, dim3((unsigned)((np + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(normal, at<void>(c.hDown, dNrm), 12 * np);
  std::memcpy(min_distance, at<void>(c.hDown, dMin), 4 * np);
  std::memcpy(max_distance, at<void>(c.hDown, dMax), 4 * np);
  std::memcpy(status, at<void>(c.hDown, dSt), np);
  if (where) { where->slots = a.slots; where->normal = a.normal; where->minDistance = a.minDistance; where->maxDistance = a.maxDistance; where->status = a.status; }
  return YDORB_OK;
}

// n_queries > 0
inline int runCovisibility(StagedCtx& c, MapSource& src, const int32_t* query_kf, int32_t n_queries, const int32_t* list_start,
                           const int32_t* point_idx, const int32_t* out_start, int32_t* conn_kf, int32_t* conn_weight, int32_t* counts,
                           uint8_t* status) {
  const size_t nq = (size_t)n_queries, L = (size_t)list_start[nq], cap = (size_t)out_start[nq];
  Layout U;
  src.lay(U);
  const size_t oQ = U.add(4 * nq), oLs = U.add(4 * (nq + 1)), oIdx = U.add(4 * L), oOs = U.add(4 * (nq + 1));
  Layout D;
  const size_t dKf = D.add(4 * cap), dW = D.add(4 * cap), dCnt = D.add(4 * nq), dSt = D.add(nq);
  int rc;
  if ((rc = c.ensure(U.bytes, D.bytes))) return rc;
  src.stage(c.hUp);
  std::memcpy(at<void>(c.hUp, oQ), query_kf, 4 * nq);
  std::memcpy(at<void>(c.hUp, oLs), list_start, 4 * (nq + 1));
  if (L) std::memcpy(at<void>(c.hUp, oIdx), point_idx, 4 * L);
  std::memcpy(at<void>(c.hUp, oOs), out_start, 4 * (nq + 1));
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  CovisArgs a;
  a.t = src.device(c.up);
  a.nQueries = n_queries;
  a.queryKf = at<int>(c.up, oQ); a.listStart = at<int>(c.up, oLs); a.pointIdx = at<int>(c.up, oIdx); a.outStart = at<int>(c.up, oOs);
  a.connKf = at<int>(c.down, dKf); a.connWeight = at<int>(c.down, dW); a.counts = at<int>(c.down, dCnt); a.status = at<uint8_t>(c.down, dSt);
  hipLaunchKernelGGL(k_covisibility, dim3((unsigned)nq), dim3(kThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(counts, at<void>(c.hDown, dCnt), 4 * nq);
  std::memcpy(status, at<void>(c.hDown, dSt), nq);
  const int32_t* hKf = at<int32_t>(c.hDown, dKf);
  const int32_t* hW = at<int32_t>(c.hDown, dW);
  for (size_t q = 0; q < nq; q++) {   // only what a query wrote: the rest of its range, and all of an overflowing query's, stays the caller's
    if (status[q] != 0 || counts[q] == 0) continue;
    std::memcpy(conn_kf + out_start[q], hKf + out_start[q], 4 * (size_t)counts[q]);
    std::memcpy(conn_weight + out_start[q], hW + out_start[q], 4 * (size_t)counts[q]);
  }
  return YDORB_OK;
}

// n_candidates > 0 and list_start[n_candidates] > 0: the entries answer the empty cases themselves, before they touch a device
inline int runRedundancy(StagedCtx& c, MapSource& src, const int32_t* cand_kf, int32_t n_candidates, const int32_t* list_start,
                         const int32_t* point_idx, const uint8_t* own_level, const uint8_t* removed, int32_t th_obs, int32_t* n_counted,
                         int32_t* n_redundant, uint8_t* cull) {
  const size_t nc = (size_t)n_candidates, nk = src.nKeyframes(), L = (size_t)list_start[nc];
  Layout U;
  src.lay(U);
  const size_t oC = U.add(4 * nc), oLs = U.add(4 * (nc + 1)), oIdx = U.add(4 * L), oOwn = U.add(L), oRem = U.add(nk);
  Layout D;
  const size_t dCnt = D.add(4 * nc), dRed = D.add(4 * nc);
  int rc;
  if ((rc = c.ensure(U.bytes, D.bytes))) return rc;
  src.stage(c.hUp);
  std::memcpy(at<void>(c.hUp, oC), cand_kf, 4 * nc);
  std::memcpy(at<void>(c.hUp, oLs), list_start, 4 * (nc + 1));
  std::memcpy(at<void>(c.hUp, oIdx), point_idx, 4 * L);
  std::memcpy(at<void>(c.hUp, oOwn), own_level, L);
  if (removed) std::memcpy(at<void>(c.hUp, oRem), removed, nk);
  else std::memset(at<void>(c.hUp, oRem), 0, nk);
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(c.down.p, 0, D.bytes, s));
  RedundancyArgs a;
  a.t = src.device(c.up);
  a.nCand = n_candidates; a.nEntries = (int)L; a.thObs = th_obs;
  a.candKf = at<int>(c.up, oC); a.listStart = at<int>(c.up, oLs); a.pointIdx = at<int>(c.up, oIdx); a.ownLevel = at<uint8_t>(c.up, oOwn);
  a.removed = at<uint8_t>(c.up, oRem);
  a.nCounted = at<int>(c.down, dCnt); a.nRedundant = at<int>(c.down, dRed);
  hipLaunchKernelGGL(k_redundancy, dim3((unsigned)((L + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(n_counted, at<void>(c.hDown, dCnt), 4 * nc);
  std::memcpy(n_redundant, at<void>(c.hDown, dRed), 4 * nc);
  for (size_t k = 0; k < nc; k++) cull[k] = maptable::cullVerdict(n_redundant[k], n_counted[k]);
  return YDORB_OK;
}

}  // namespace mapmaint
}  // namespace ydorb
