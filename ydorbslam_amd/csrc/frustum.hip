// Host driver of the batched Frame::isInCameraFrustum + its C ABI (include/ydorb/c_api.h, "Local map tracking"): ydorb_frustum_cull,
// ydorb_frustum_release.  A call checks the lists and every point index, copies views, lists and the shared map-point table into one
// pinned staging area, uploads it in one copy, runs k_frustum_cull once and reads track rows and status bytes back in one copy.
// (ydorb_search_local_points, the one-view form fused with the projection search, lives with the matcher in orb_matcher.hip.)
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "../../include/ydorb/c_api.h"
#include "frustum_kernels.hip.h"
#include "host_buffers.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::frustum;

namespace {

StagedCtx g_ctx[16];   // this solver's own: nothing is shared with the other staged solvers

int invalid(const char* what) { set_error("frustum: %s", what); return YDORB_ERR_INVALID_ARG; }

}  // namespace

extern "C" int ydorb_frustum_cull(const YdFrustumBatch* B, YdTrackView* rows, uint8_t* status, int32_t* n_in_view) {
  if (!B || B->n_views < 0 || B->table.n < 0 || B->device < 0 || B->device >= 16) return invalid("invalid batch");
  const int nv = B->n_views, np = B->table.n;
  if (nv > 0 && (!B->views || !B->list_start)) return invalid("null views or list_start");
  if (np > 0 && (!B->table.pos_min || !B->table.normal_max || !B->table.max_distance)) return invalid("null map-point table arrays");
  for (int f = 0; f < nv; f++)
    if (B->views[f].n_levels < 1 || B->views[f].n_levels > 8) {
      set_error("frustum: view %d: n_levels %d outside 1..8", f, B->views[f].n_levels);
      return YDORB_ERR_INVALID_ARG;
    }
  if (nv > 0 && B->list_start[0] != 0) return invalid("list_start[0] must be 0");
  for (int f = 0; f < nv; f++)
    if (B->list_start[f + 1] < B->list_start[f]) return invalid("list_start must be non-decreasing");
  const int L = nv > 0 ? B->list_start[nv] : 0;
  if (L > 0 && (!B->point_idx || !B->skip || !rows || !status)) return invalid("null list or output arrays");
  for (int e = 0; e < L; e++)
    if (B->point_idx[e] < 0 || B->point_idx[e] >= np) {
      set_error("frustum: list entry %d: point index %d outside the table of %d", e, B->point_idx[e], np);
      return YDORB_ERR_INVALID_ARG;
    }
  int rc = require_device(B->device);
  if (rc) return rc;
  if (n_in_view) std::memset(n_in_view, 0, sizeof(int32_t) * (size_t)nv);
  if (L == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[B->device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(B->device))) return rc;
  const size_t l = L;
  Layout U;
  const size_t oStart = U.add(4 * (size_t)(nv + 1)), oView = U.add(sizeof(ViewDev) * nv), oPos = U.add(16 * (size_t)np), oNrm = U.add(16 * (size_t)np),
               oMax = U.add(4 * (size_t)np), oIdx = U.add(4 * l), oSkip = U.add(l);
  Layout D;
  const size_t dRows = D.add(sizeof(YdTrackView) * l), dSt = D.add(l);
  if ((rc = c.ensure(U.bytes, D.bytes))) return rc;
  std::memcpy(at<void>(c.hUp, oStart), B->list_start, 4 * (size_t)(nv + 1));
  std::memcpy(at<void>(c.hUp, oView), B->views, sizeof(ViewDev) * nv);
  std::memcpy(at<void>(c.hUp, oPos), B->table.pos_min, 16 * (size_t)np);
  std::memcpy(at<void>(c.hUp, oNrm), B->table.normal_max, 16 * (size_t)np);
  std::memcpy(at<void>(c.hUp, oMax), B->table.max_distance, 4 * (size_t)np);
  std::memcpy(at<void>(c.hUp, oIdx), B->point_idx, 4 * l);
  std::memcpy(at<void>(c.hUp, oSkip), B->skip, l);
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  Args a;
  a.nViews = nv; a.nEntries = L;
  a.start = at<int>(c.up, oStart); a.views = at<ViewDev>(c.up, oView);
  a.posMin = at<float4>(c.up, oPos); a.normalMax = at<float4>(c.up, oNrm); a.maxDistance = at<float>(c.up, oMax);
  a.pointIdx = at<int>(c.up, oIdx); a.skip = at<uint8_t>(c.up, oSkip);
  a.rows = at<YdTrackView>(c.down, dRows); a.status = at<uint8_t>(c.down, dSt);
  hipLaunchKernelGGL(k_frustum_cull, dim3((L + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(rows, at<void>(c.hDown, dRows), sizeof(YdTrackView) * l);
  std::memcpy(status, at<void>(c.hDown, dSt), l);
  if (n_in_view)
    for (int f = 0; f < nv; f++)
      for (int e = B->list_start[f]; e < B->list_start[f + 1]; e++) n_in_view[f] += status[e] == YDORB_FRUSTUM_IN_VIEW;
  return YDORB_OK;
}

extern "C" int ydorb_frustum_release(int32_t device) { return release_staged(g_ctx, device); }
