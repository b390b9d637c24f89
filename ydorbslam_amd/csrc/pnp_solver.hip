// Host driver of the relocalisation EPnP RANSAC + its C ABI (include/ydorb/c_api.h, "EPnP RANSAC"): ydorb_pnp_ransac,
// ydorb_pnp_release.  A call packs the batch into one pinned staging area, uploads it in one copy, runs the kernels of
// pnp_kernels.hip.h and reads back O(problems) bytes, the per-hypothesis counts and the masks in one copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "host_buffers.h"
#include "pnp_kernels.hip.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::pnp;

namespace {

StagedCtx g_ctx[16];   // this solver's own: nothing is shared with the other staged solvers

}  // namespace

extern "C" int ydorb_pnp_ransac(YdPnpProblem* probs, int32_t n, int32_t chunk, int32_t device) {
  if (n < 0 || (n > 0 && !probs) || chunk < 1 || device < 0 || device >= 16) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  for (int p = 0; p < n; p++) {
    const YdPnpProblem& q = probs[p];
    if (q.n < 0 || q.n_hyp < 0 || q.next_hyp < 0 ||
        (q.n > 0 && (!q.Xw || !q.P2D || !q.max_err || !q.best_mask || !q.inliers)) || (q.n_hyp > 0 && !q.quads)) {
      set_error("pnp problem %d: invalid sizes or null arrays", p);
      return YDORB_ERR_INVALID_ARG;
    }
    for (int k = 0; k < 4 * q.n_hyp; k++)
      if (q.quads[k] < 0 || q.quads[k] >= q.n) { set_error("pnp problem %d: quad index %d out of range", p, q.quads[k]); return YDORB_ERR_INVALID_ARG; }
  }
  int rc = require_device(device);
  if (rc) return rc;
  if (n == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  // H: hypotheses the iterate(chunk) sequence runs without a return.  With ||, the first call runs until mnIterations >= maxIts and
  // it has run chunk; with &&, calls of chunk run up to maxIts.  Either way the sequence ends with bNoMore after H.
  std::vector<int> seq(n), nEval(n), ptOff(n), hypOff(n);
  size_t nPts = 0, nHyp = 0;
  int maxEval = 0;
  for (int p = 0; p < n; p++) {
    const YdPnpProblem& q = probs[p];
    seq[p] = q.n < q.min_inliers ? 0 : q.loop_or ? std::max(q.max_its - q.next_hyp, chunk) : std::max(0, q.max_its - q.next_hyp);
    nEval[p] = std::min(seq[p], q.n_hyp);
    ptOff[p] = (int)nPts; hypOff[p] = (int)nHyp;
    nPts += q.n; nHyp += nEval[p];
    maxEval = std::max(maxEval, nEval[p]);
  }
  Layout U;
  const size_t oDev = U.add(sizeof(ProbDev) * n), oX = U.add(12 * nPts), oP = U.add(8 * nPts), oM = U.add(4 * nPts),
               oBm = U.add(nPts), oQ = U.add(16 * nHyp);
  Layout D;
  const size_t oOut = D.add(sizeof(ProbOut) * n), oCnt = D.add(4 * nHyp), oBest = D.add(nPts), oInl = D.add(nPts);
  Layout W;
  const size_t wPose = W.add(96 * nHyp), wIdx = W.add(4 * nPts), wAl = W.add(32 * nPts), wPc = W.add(24 * nPts);
  if ((rc = c.ensure(U.bytes, D.bytes, W.bytes))) return rc;
  ProbDev* dev = at<ProbDev>(c.hUp, oDev);
  for (int p = 0; p < n; p++) {
    const YdPnpProblem& q = probs[p];
    ProbDev& d = dev[p];
    d.n = q.n; d.minInl = q.min_inliers; d.maxIts = q.max_its; d.nEval = nEval[p]; d.bestIn = q.best_inliers;
    d.ptOff = ptOff[p]; d.hypOff = hypOff[p]; d.seqLen = seq[p];
    std::memcpy(d.K, q.K, sizeof d.K);
    const size_t o = ptOff[p];
    if (q.n) {
      std::memcpy(at<float>(c.hUp, oX) + 3 * o, q.Xw, 12 * (size_t)q.n);
      std::memcpy(at<float>(c.hUp, oP) + 2 * o, q.P2D, 8 * (size_t)q.n);
      std::memcpy(at<float>(c.hUp, oM) + o, q.max_err, 4 * (size_t)q.n);
      std::memcpy(at<uint8_t>(c.hUp, oBm) + o, q.best_mask, q.n);
    }
    if (nEval[p]) std::memcpy(at<int>(c.hUp, oQ) + 4 * (size_t)hypOff[p], q.quads, 16 * (size_t)nEval[p]);
  }
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  const ProbDev* dDev = at<ProbDev>(c.up, oDev);
  const float *dX = at<float>(c.up, oX), *dP = at<float>(c.up, oP), *dM = at<float>(c.up, oM);
  // problems go in gridDim.y, which holds at most 65535: larger batches take several launches
  for (int p0 = 0; maxEval > 0 && p0 < n; p0 += 65535) {
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3(maxEval, std::min(65535, n - p0)), dim3(64), 0, s, dDev + p0, dX, dP, dM,
                       at<const int>(c.up, oQ), at<int>(c.down, oCnt), at<double>(c.scratch, wPose));
    HIPCHK(hipGetLastError());
  }
  CommitArgs a;
  a.probs = dDev; a.Xw = dX; a.P2D = dP; a.maxErr = dM; a.counts = at<const int>(c.down, oCnt); a.poses = at<const double>(c.scratch, wPose);
  a.bestMaskIn = at<const uint8_t>(c.up, oBm); a.bestMask = at<uint8_t>(c.down, oBest); a.inliers = at<uint8_t>(c.down, oInl);
  a.idx = at<int>(c.scratch, wIdx); a.al = at<double>(c.scratch, wAl); a.pcs = at<double>(c.scratch, wPc); a.out = at<ProbOut>(c.down, oOut);
  hipLaunchKernelGGL(k_pnp_commit, dim3(n), dim3(kCommitThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const ProbOut* out = at<ProbOut>(c.hDown, oOut);
  for (int p = 0; p < n; p++) {
    YdPnpProblem& q = probs[p];
    const ProbOut& r = out[p];
    const int evaluated = r.ret >= 0 ? r.ret + 1 : nEval[p];
    if (q.hyp_inliers)
      for (int k = 0; k < q.n_hyp; k++) q.hyp_inliers[k] = k < evaluated ? at<int>(c.hDown, oCnt)[hypOff[p] + k] : -1;
    if (q.n) {
      std::memcpy(q.inliers, at<uint8_t>(c.hDown, oInl) + ptOff[p], q.n);
      std::memcpy(q.best_mask, at<uint8_t>(c.hDown, oBest) + ptOff[p], q.n);
    }
    if (r.bestHyp >= 0) std::memcpy(q.best_Tcw, r.bestT, sizeof q.best_Tcw);
    q.best_inliers = r.best;
    q.ret_how = r.how;
    q.ret_hyp = r.ret >= 0 ? q.next_hyp + r.ret : -1;
    q.n_inliers = r.nInl;
    if (r.how == YDORB_PNP_REFINED) std::memcpy(q.Tcw, r.T, sizeof q.Tcw);
    else if (r.how == YDORB_PNP_BEST) std::memcpy(q.Tcw, q.best_Tcw, sizeof q.Tcw);
    else std::memset(q.Tcw, 0, sizeof q.Tcw);
    if (q.n < q.min_inliers) {
      q.no_more = 1; q.n_calls = 1;
    } else if (r.ret >= 0) {
      q.no_more = 0; q.n_calls = q.loop_or ? 1 : r.ret / chunk + 1;
    } else if (nEval[p] == seq[p]) {
      q.no_more = 1; q.n_calls = q.loop_or ? 1 : std::max(1, (seq[p] + chunk - 1) / chunk);
    } else {   // the quads ran out before the sequence ended
      q.no_more = 0; q.n_calls = q.loop_or ? (nEval[p] > 0) : (nEval[p] + chunk - 1) / chunk;
    }
    q.next_hyp += evaluated;
  }
  return YDORB_OK;
}

extern "C" int ydorb_pnp_release(int32_t device) { return release_staged(g_ctx, device); }
