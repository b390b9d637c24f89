// Host driver of createNewMapPoints' geometry + its C ABI (include/ydorb/c_api.h, "LocalMapping::createNewMapPoints"):
// ydorb_triangulate_matches, ydorb_triangulate_release.  A call checks every index, gathers each match's two features into one pinned
// staging area (so the upload grows with the matches, not with the keyframes' feature counts), uploads it in one copy, runs
// k_triangulate_matches once and reads points and status bytes back in one copy.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "../../include/ydorb/c_api.h"
#include "host_buffers.h"
#include "triangulate_kernels.hip.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::tri;

namespace {

StagedCtx g_ctx[16];   // this solver's own: nothing is shared with the other staged solvers

int invalid(const char* what) { set_error("triangulate: %s", what); return YDORB_ERR_INVALID_ARG; }

}  // namespace

extern "C" int ydorb_triangulate_matches(const YdTriBatch* B, float* x3d, uint8_t* status, int32_t* n_accepted) {
  if (!B || B->n_views < 0 || B->n_problems < 0 || B->device < 0 || B->device >= 16) return invalid("invalid batch");
  const int n = B->n_problems, nv = B->n_views;
  if (nv > 0 && !B->views) return invalid("null views");
  if (n > 0 && (!B->first_view || !B->second_view || !B->match_start || !B->ratio_factor)) return invalid("null problem arrays");
  for (int v = 0; v < nv; v++) {
    const YdTriView& V = B->views[v];
    if (V.n < 0 || V.n_levels < 0 || (V.n > 0 && (!V.kps || !V.right_x || !V.depth)) || (V.n_levels > 0 && (!V.level_sigma2 || !V.scale_factors))) {
      set_error("triangulate: view %d: invalid sizes or null arrays", v);
      return YDORB_ERR_INVALID_ARG;
    }
  }
  if (n > 0 && B->match_start[0] != 0) return invalid("match_start[0] must be 0");
  for (int p = 0; p < n; p++) {
    if (B->match_start[p + 1] < B->match_start[p]) return invalid("match_start must be non-decreasing");
    if (B->first_view[p] < 0 || B->first_view[p] >= nv || B->second_view[p] < 0 || B->second_view[p] >= nv) {
      set_error("triangulate: problem %d: view index out of range", p);
      return YDORB_ERR_INVALID_ARG;
    }
  }
  const int M = n > 0 ? B->match_start[n] : 0;
  if (M > 0 && (!B->idx1 || !B->idx2 || !x3d || !status)) return invalid("null match or output arrays");
  for (int p = 0; p < n; p++) {
    const YdTriView &V1 = B->views[B->first_view[p]], &V2 = B->views[B->second_view[p]];
    for (int m = B->match_start[p]; m < B->match_start[p + 1]; m++) {
      const int i1 = B->idx1[m], i2 = B->idx2[m];
      if (i1 < 0 || i1 >= V1.n || i2 < 0 || i2 >= V2.n) {
        set_error("triangulate: problem %d match %d: keypoint index (%d, %d) out of range", p, m - B->match_start[p], i1, i2);
        return YDORB_ERR_INVALID_ARG;
      }
      const int o1 = V1.kps[i1].octave, o2 = V2.kps[i2].octave;
      if (o1 < 0 || o1 >= V1.n_levels || o2 < 0 || o2 >= V2.n_levels) {
        set_error("triangulate: problem %d match %d: octave (%d, %d) outside the level tables", p, m - B->match_start[p], o1, o2);
        return YDORB_ERR_INVALID_ARG;
      }
    }
  }
  int rc = require_device(B->device);
  if (rc) return rc;
  if (n_accepted) std::memset(n_accepted, 0, sizeof(int32_t) * (size_t)n);
  if (M == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[B->device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(B->device))) return rc;
  const size_t m = M;
  Layout U;
  const size_t oStart = U.add(4 * (size_t)(n + 1)), oProb = U.add(sizeof(ProblemDev) * n), oView = U.add(sizeof(ViewDev) * nv),
               oF1 = U.add(16 * m), oF2 = U.add(16 * m), oLv = U.add(16 * m);
  Layout D;
  const size_t dX = D.add(12 * m), dSt = D.add(m);
  if ((rc = c.ensure(U.bytes, D.bytes))) return rc;
  std::memcpy(at<void>(c.hUp, oStart), B->match_start, 4 * (size_t)(n + 1));
  ProblemDev* prob = at<ProblemDev>(c.hUp, oProb);
  for (int p = 0; p < n; p++) prob[p] = ProblemDev{B->first_view[p], B->second_view[p], B->ratio_factor[p], 0};
  ViewDev* view = at<ViewDev>(c.hUp, oView);
  for (int v = 0; v < nv; v++) {
    const YdTriView& V = B->views[v];
    ViewDev& d = view[v];
    std::memcpy(d.Tcw, V.Tcw, sizeof d.Tcw); std::memcpy(d.Rwc, V.Rwc, sizeof d.Rwc); std::memcpy(d.Ow, V.Ow, sizeof d.Ow);
    d.fx = V.fx; d.fy = V.fy; d.cx = V.cx; d.cy = V.cy; d.invfx = V.invfx; d.invfy = V.invfy; d.b = V.b; d.bf = V.bf;
  }
  float4 *f1 = at<float4>(c.hUp, oF1), *f2 = at<float4>(c.hUp, oF2), *lv = at<float4>(c.hUp, oLv);
  for (int p = 0; p < n; p++) {
    const YdTriView &V1 = B->views[B->first_view[p]], &V2 = B->views[B->second_view[p]];
    for (int k = B->match_start[p]; k < B->match_start[p + 1]; k++) {
      const int i1 = B->idx1[k], i2 = B->idx2[k];
      const YdKeyPoint &k1 = V1.kps[i1], &k2 = V2.kps[i2];
      f1[k] = make_float4(k1.x, k1.y, V1.right_x[i1], V1.depth[i1]);
      f2[k] = make_float4(k2.x, k2.y, V2.right_x[i2], V2.depth[i2]);
      lv[k] = make_float4(V1.level_sigma2[k1.octave], V2.level_sigma2[k2.octave], V1.scale_factors[k1.octave], V2.scale_factors[k2.octave]);
    }
  }
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  Args a;
  a.nProblems = n; a.nMatches = M;
  a.start = at<int>(c.up, oStart); a.problems = at<ProblemDev>(c.up, oProb); a.views = at<ViewDev>(c.up, oView);
  a.f1 = at<float4>(c.up, oF1); a.f2 = at<float4>(c.up, oF2); a.lv = at<float4>(c.up, oLv);
  a.x3d = at<float>(c.down, dX); a.status = at<uint8_t>(c.down, dSt);
  hipLaunchKernelGGL(k_triangulate_matches, dim3((M + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(x3d, at<void>(c.hDown, dX), 12 * m);
  std::memcpy(status, at<void>(c.hDown, dSt), m);
  if (n_accepted)
    for (int p = 0; p < n; p++)
      for (int k = B->match_start[p]; k < B->match_start[p + 1]; k++) n_accepted[p] += (status[k] & 15) == YDORB_TRI_ACCEPTED;
  return YDORB_OK;
}

extern "C" int ydorb_triangulate_release(int32_t device) { return release_staged(g_ctx, device); }
