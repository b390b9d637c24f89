// Host driver of map maintenance + its C ABI (include/ydorb/c_api.h, "Map maintenance"): ydorb_map_update_normal_depth,
// ydorb_map_covisibility, ydorb_map_keyframe_redundancy, ydorb_map_release.  A call checks everything on the host (map_table.h), copies
// the observation table and its own arrays into one pinned staging area, uploads it in one copy, runs one kernel and reads the results
// back in one copy.  The culling verdict is the reference's double compare, made here on the host.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>

#include "../../include/ydorb/c_api.h"
#include "host_buffers.h"
#include "map_kernels.hip.h"
#include "map_table.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::mapmaint;

namespace {

StagedCtx g_ctx[16];   // this solver's own: nothing is shared with the other staged solvers

int invalid(const std::string& what) { set_error("map maintenance: %s", what.c_str()); return YDORB_ERR_INVALID_ARG; }

// where the table's arrays sit in the upload area
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

int ensure(StagedCtx& c, const Layout& U, const Layout& D) {
  int rc;
  if ((rc = c.up.ensure(U.bytes)) || (rc = c.hUp.ensure(U.bytes)) || (rc = c.down.ensure(D.bytes)) || (rc = c.hDown.ensure(D.bytes))) return rc;
  return YDORB_OK;
}

}  // namespace

extern "C" int ydorb_map_update_normal_depth(const YdObservationTable* T, const float* pos, const float* centre, const int32_t* ref_kf,
                                             const uint8_t* ref_level, const float* scale_factors, int32_t n_levels, int32_t device,
                                             float* normal, float* min_distance, float* max_distance, uint8_t* status) {
  std::string err;
  if (!maptable::checkNormalDepth(T, pos, centre, ref_kf, ref_level, scale_factors, n_levels, device, normal, min_distance, max_distance,
                                  status, err))
    return invalid(err);
  int rc = require_device(device);
  if (rc) return rc;
  const size_t np = (size_t)T->n_points, nk = (size_t)T->n_keyframes;
  if (np == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  Layout U;
  TableAt ta;
  ta.lay(U, T);
  const size_t oPos = U.add(12 * np), oCen = U.add(12 * nk), oRef = U.add(4 * np), oLvl = U.add(np);
  Layout D;
  const size_t dNrm = D.add(12 * np), dMin = D.add(4 * np), dMax = D.add(4 * np), dSt = D.add(np);
  if ((rc = ensure(c, U, D))) return rc;
  ta.stage(c.hUp, T);
  std::memcpy(at<void>(c.hUp, oPos), pos, 12 * np);
  if (nk) std::memcpy(at<void>(c.hUp, oCen), centre, 12 * nk);
  std::memcpy(at<void>(c.hUp, oRef), ref_kf, 4 * np);
  std::memcpy(at<void>(c.hUp, oLvl), ref_level, np);
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  NormalArgs a;
  a.t = ta.device(c.up, T);
  a.pos = at<float>(c.up, oPos); a.centre = at<float>(c.up, oCen); a.refKf = at<int>(c.up, oRef); a.refLevel = at<uint8_t>(c.up, oLvl);
  for (int i = 0; i < 8; i++) a.scaleFactors[i] = i < n_levels ? scale_factors[i] : 0.f;
  a.nLevels = n_levels;
  a.slots = nullptr; a.n = T->n_points;
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
  return YDORB_OK;
}

extern "C" int ydorb_map_covisibility(const YdObservationTable* T, const int32_t* query_kf, int32_t n_queries, const int32_t* list_start,
                                      const int32_t* point_idx, const int32_t* out_start, int32_t device, int32_t* conn_kf,
                                      int32_t* conn_weight, int32_t* counts, uint8_t* status) {
  std::string err;
  if (!maptable::checkCovisibility(T, query_kf, n_queries, list_start, point_idx, out_start, device, conn_kf, conn_weight, counts, status, err))
    return invalid(err);
  int rc = require_device(device);
  if (rc) return rc;
  const size_t nq = (size_t)n_queries;
  if (nq == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  const size_t L = (size_t)list_start[nq], cap = (size_t)out_start[nq];
  Layout U;
  TableAt ta;
  ta.lay(U, T);
  const size_t oQ = U.add(4 * nq), oLs = U.add(4 * (nq + 1)), oIdx = U.add(4 * L), oOs = U.add(4 * (nq + 1));
  Layout D;
  const size_t dKf = D.add(4 * cap), dW = D.add(4 * cap), dCnt = D.add(4 * nq), dSt = D.add(nq);
  if ((rc = ensure(c, U, D))) return rc;
  ta.stage(c.hUp, T);
  std::memcpy(at<void>(c.hUp, oQ), query_kf, 4 * nq);
  std::memcpy(at<void>(c.hUp, oLs), list_start, 4 * (nq + 1));
  if (L) std::memcpy(at<void>(c.hUp, oIdx), point_idx, 4 * L);
  std::memcpy(at<void>(c.hUp, oOs), out_start, 4 * (nq + 1));
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  CovisArgs a;
  a.t = ta.device(c.up, T);
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

extern "C" int ydorb_map_keyframe_redundancy(const YdObservationTable* T, const int32_t* cand_kf, int32_t n_candidates,
                                             const int32_t* list_start, const int32_t* point_idx, const uint8_t* own_level,
                                             const uint8_t* removed, int32_t th_obs, int32_t device, int32_t* n_counted,
                                             int32_t* n_redundant, uint8_t* cull) {
  std::string err;
  if (!maptable::checkRedundancy(T, cand_kf, n_candidates, list_start, point_idx, own_level, device, n_counted, n_redundant, cull, err))
    return invalid(err);
  int rc = require_device(device);
  if (rc) return rc;
  const size_t nc = (size_t)n_candidates, nk = (size_t)T->n_keyframes;
  if (nc == 0) return YDORB_OK;
  const size_t L = (size_t)list_start[nc];
  std::memset(n_counted, 0, 4 * nc);
  std::memset(n_redundant, 0, 4 * nc);
  std::memset(cull, 0, nc);               // an empty list: 0 > 0.9 * 0 is false
  if (L == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  Layout U;
  TableAt ta;
  ta.lay(U, T);
  const size_t oC = U.add(4 * nc), oLs = U.add(4 * (nc + 1)), oIdx = U.add(4 * L), oOwn = U.add(L), oRem = U.add(nk);
  Layout D;
  const size_t dCnt = D.add(4 * nc), dRed = D.add(4 * nc);
  if ((rc = ensure(c, U, D))) return rc;
  ta.stage(c.hUp, T);
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
  a.t = ta.device(c.up, T);
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

extern "C" int ydorb_map_release(int32_t device) {
  if (device < 0 || device >= 16) { set_error("invalid device"); return YDORB_ERR_INVALID_ARG; }
  int rc = require_device(device);
  if (rc) return rc;
  return release_staged(g_ctx[device], device);
}
