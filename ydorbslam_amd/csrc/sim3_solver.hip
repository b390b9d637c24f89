// Host driver of the loop-closure Sim3 check + its C ABI (include/ydorb/c_api.h, "Sim3 RANSAC"): ydorb_sim3_ransac,
// ydorb_sim3_optimize, ydorb_sim3_release.  A call packs the batch into one pinned staging area, uploads it in one copy, runs the
// kernels of sim3_kernels.hip.h and reads back O(problems) bytes plus the masks in one copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "host_buffers.h"
#include "sim3_kernels.hip.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::sim3;

namespace {

StagedCtx g_ctx[16];   // this solver's own: nothing is shared with the other staged solvers

}  // namespace

extern "C" int ydorb_sim3_ransac(YdSim3Problem* probs, int32_t n, int32_t chunk, int32_t device) {
  if (n < 0 || (n > 0 && !probs) || chunk < 1 || device < 0 || device >= 16) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  for (int p = 0; p < n; p++) {
    const YdSim3Problem& q = probs[p];
    if (q.n < 0 || q.n_hyp < 0 || q.next_hyp < 0 || (q.n > 0 && (!q.X1 || !q.X2 || !q.P1 || !q.P2 || !q.max_err1 || !q.max_err2 || !q.inliers)) ||
        (q.n_hyp > 0 && !q.triples)) {
      set_error("sim3 problem %d: invalid sizes or null arrays", p);
      return YDORB_ERR_INVALID_ARG;
    }
    for (int k = 0; k < 3 * q.n_hyp; k++)
      if (q.triples[k] < 0 || q.triples[k] >= q.n) { set_error("sim3 problem %d: triple index %d out of range", p, q.triples[k]); return YDORB_ERR_INVALID_ARG; }
  }
  int rc = require_device(device);
  if (rc) return rc;
  if (n == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  // hypotheses each problem evaluates: none when N < minInliers (iterate returns at once), at most max_its - next_hyp
  std::vector<int> nEval(n), pairOff(n), hypOff(n);
  int nPairs = 0, nHyp = 0, maxEval = 0;
  for (int p = 0; p < n; p++) {
    const YdSim3Problem& q = probs[p];
    nEval[p] = q.n < q.min_inliers ? 0 : std::max(0, std::min(q.n_hyp, q.max_its - q.next_hyp));
    pairOff[p] = nPairs; hypOff[p] = nHyp;
    nPairs += q.n; nHyp += nEval[p];
    maxEval = std::max(maxEval, nEval[p]);
  }
  Layout U;
  const size_t oDev = U.add(sizeof(RansacDev) * n), oX1 = U.add(12 * (size_t)nPairs), oX2 = U.add(12 * (size_t)nPairs),
               oP1 = U.add(8 * (size_t)nPairs), oP2 = U.add(8 * (size_t)nPairs), oM1 = U.add(4 * (size_t)nPairs),
               oM2 = U.add(4 * (size_t)nPairs), oTri = U.add(12 * (size_t)nHyp);
  Layout D;
  const size_t oOut = D.add(sizeof(RansacOut) * n), oCnt = D.add(4 * (size_t)nHyp), oMask = D.add(nPairs);
  if ((rc = c.ensure(U.bytes, D.bytes))) return rc;
  RansacDev* dev = at<RansacDev>(c.hUp, oDev);
  for (int p = 0; p < n; p++) {
    const YdSim3Problem& q = probs[p];
    RansacDev& d = dev[p];
    d.n = q.n; d.fix = q.fix_scale; d.minInl = q.min_inliers; d.maxIts = q.max_its; d.nEval = nEval[p]; d.bestIn = q.best_inliers;
    d.pairOff = pairOff[p]; d.hypOff = hypOff[p];
    std::memcpy(d.K1, q.K1, sizeof d.K1); std::memcpy(d.K2, q.K2, sizeof d.K2);
    const size_t o = pairOff[p];
    if (q.n) {
      std::memcpy(at<float>(c.hUp, oX1) + 3 * o, q.X1, 12 * (size_t)q.n);
      std::memcpy(at<float>(c.hUp, oX2) + 3 * o, q.X2, 12 * (size_t)q.n);
      std::memcpy(at<float>(c.hUp, oP1) + 2 * o, q.P1, 8 * (size_t)q.n);
      std::memcpy(at<float>(c.hUp, oP2) + 2 * o, q.P2, 8 * (size_t)q.n);
      std::memcpy(at<float>(c.hUp, oM1) + o, q.max_err1, 4 * (size_t)q.n);
      std::memcpy(at<float>(c.hUp, oM2) + o, q.max_err2, 4 * (size_t)q.n);
    }
    if (nEval[p]) std::memcpy(at<int>(c.hUp, oTri) + 3 * (size_t)hypOff[p], q.triples, 12 * (size_t)nEval[p]);
  }
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  const RansacDev* dDev = at<RansacDev>(c.up, oDev);
  const float *dX1 = at<float>(c.up, oX1), *dX2 = at<float>(c.up, oX2), *dP1 = at<float>(c.up, oP1), *dP2 = at<float>(c.up, oP2),
              *dM1 = at<float>(c.up, oM1), *dM2 = at<float>(c.up, oM2);
  const int* dTri = at<int>(c.up, oTri);
  // problems go in gridDim.y, which holds at most 65535: larger batches take several launches
  for (int p0 = 0; maxEval > 0 && p0 < n; p0 += 65535) {
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3((maxEval + kHypWaves - 1) / kHypWaves, std::min(65535, n - p0)), dim3(64 * kHypWaves), 0, s,
                       dDev + p0, dX1, dX2, dP1, dP2, dM1, dM2, dTri, at<int>(c.down, oCnt));
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_sim3_replay, dim3(n), dim3(64), 0, s, dDev, dX1, dX2, dP1, dP2, dM1, dM2, dTri, at<const int>(c.down, oCnt),
                     at<RansacOut>(c.down, oOut), at<uint8_t>(c.down, oMask));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const RansacOut* out = at<RansacOut>(c.hDown, oOut);
  for (int p = 0; p < n; p++) {
    YdSim3Problem& q = probs[p];
    const RansacOut& r = out[p];
    const int evaluated = r.ret >= 0 ? r.ret + 1 : nEval[p];
    if (q.hyp_inliers) {
      for (int k = 0; k < q.n_hyp; k++) q.hyp_inliers[k] = k < evaluated ? at<int>(c.hDown, oCnt)[hypOff[p] + k] : -1;
    }
    if (q.n) std::memcpy(q.inliers, at<uint8_t>(c.hDown, oMask) + pairOff[p], q.n);
    if (r.bestIdx >= 0) std::memcpy(q.best_T12, r.T, sizeof q.best_T12);
    q.best_inliers = r.best;
    q.ret_hyp = r.ret >= 0 ? q.next_hyp + r.ret : -1;
    if (q.n < q.min_inliers) {
      q.no_more = 1; q.n_calls = 1;
    } else if (r.ret >= 0) {
      q.no_more = 0; q.n_calls = r.ret / chunk + 1;
    } else {
      q.no_more = q.next_hyp + evaluated >= q.max_its;
      q.n_calls = std::max(1, (evaluated + chunk - 1) / chunk);
    }
    q.next_hyp += evaluated;
  }
  return YDORB_OK;
}

extern "C" int ydorb_sim3_optimize(const YdSim3Batch* B, uint8_t* outlier, int32_t* n_in, double* chi2_log, int32_t* trials) {
  if (!B || B->n_problems < 0 || (B->n_problems && (!B->corr_start || !B->S12 || !B->K1 || !B->K2 || !B->fix_scale || !n_in)) ||
      B->device < 0 || B->device >= 16) {
    set_error("invalid sim3 batch");
    return YDORB_ERR_INVALID_ARG;
  }
  const int n = B->n_problems;
  if (n > 0) {
    if (B->corr_start[0] != 0) { set_error("corr_start[0] must be 0"); return YDORB_ERR_INVALID_ARG; }
    for (int p = 0; p < n; p++)
      if (B->corr_start[p + 1] < B->corr_start[p]) { set_error("corr_start must be non-decreasing"); return YDORB_ERR_INVALID_ARG; }
  }
  const int E = n > 0 ? B->corr_start[n] : 0;
  if (E > 0 && (!B->X1c || !B->X2c || !B->obs1 || !B->obs2 || !B->inv_sigma2_1 || !B->inv_sigma2_2 || !outlier)) {
    set_error("null pair arrays");
    return YDORB_ERR_INVALID_ARG;
  }
  int rc = require_device(B->device);
  if (rc) return rc;
  if (n == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[B->device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(B->device))) return rc;
  const size_t e = E;
  Layout U;
  const size_t oStart = U.add(4 * (size_t)(n + 1)), oS = U.add(64 * (size_t)n), oK1 = U.add(32 * (size_t)n), oK2 = U.add(32 * (size_t)n),
               oFix = U.add(n), oX1 = U.add(24 * e), oX2 = U.add(24 * e), oO1 = U.add(16 * e), oO2 = U.add(16 * e), oW1 = U.add(8 * e),
               oW2 = U.add(8 * e);
  Layout D;   // S12 first: it goes down with the results
  const size_t dS = D.add(64 * (size_t)n), dChi = D.add(16 * (size_t)n), dIn = D.add(4 * (size_t)n), dTr = D.add(4 * (size_t)n), dOut = D.add(e);
  Layout W;
  const size_t wErr = W.add(32 * e), wAct = W.add(e);
  if ((rc = c.ensure(U.bytes, D.bytes, W.bytes))) return rc;
  std::memcpy(at<void>(c.hUp, oStart), B->corr_start, 4 * (size_t)(n + 1));
  std::memcpy(at<void>(c.hUp, oS), B->S12, 64 * (size_t)n);
  std::memcpy(at<void>(c.hUp, oK1), B->K1, 32 * (size_t)n);
  std::memcpy(at<void>(c.hUp, oK2), B->K2, 32 * (size_t)n);
  std::memcpy(at<void>(c.hUp, oFix), B->fix_scale, n);
  if (E) {
    std::memcpy(at<void>(c.hUp, oX1), B->X1c, 24 * e);
    std::memcpy(at<void>(c.hUp, oX2), B->X2c, 24 * e);
    std::memcpy(at<void>(c.hUp, oO1), B->obs1, 16 * e);
    std::memcpy(at<void>(c.hUp, oO2), B->obs2, 16 * e);
    std::memcpy(at<void>(c.hUp, oW1), B->inv_sigma2_1, 8 * e);
    std::memcpy(at<void>(c.hUp, oW2), B->inv_sigma2_2, 8 * e);
  }
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(at<void>(c.down, dS), at<void>(c.up, oS), 64 * (size_t)n, hipMemcpyDeviceToDevice, s));
  const float th2f = (float)B->th2;
  OptArgs a;
  a.start = at<int>(c.up, oStart); a.S12 = at<double>(c.down, dS); a.K1 = at<double>(c.up, oK1); a.K2 = at<double>(c.up, oK2);
  a.fix = at<uint8_t>(c.up, oFix); a.X1 = at<double>(c.up, oX1); a.X2 = at<double>(c.up, oX2); a.o1 = at<double>(c.up, oO1);
  a.o2 = at<double>(c.up, oO2); a.w1 = at<double>(c.up, oW1); a.w2 = at<double>(c.up, oW2);
  a.thr = (double)th2f; a.delta = (double)sqrtf(th2f);   // the reference's float th2 and deltaHuber = sqrt(th2)
  a.err = at<double>(c.scratch, wErr); a.active = at<uint8_t>(c.scratch, wAct); a.outlier = at<uint8_t>(c.down, dOut);
  a.nIn = at<int>(c.down, dIn); a.chi2Log = at<double>(c.down, dChi); a.trials = at<int>(c.down, dTr);
  hipLaunchKernelGGL(k_sim3_optimize, dim3(n), dim3(kOptThreads), 0, s, n, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(B->S12, at<void>(c.hDown, dS), 64 * (size_t)n);
  std::memcpy(n_in, at<void>(c.hDown, dIn), 4 * (size_t)n);
  if (E) std::memcpy(outlier, at<void>(c.hDown, dOut), e);
  if (chi2_log) std::memcpy(chi2_log, at<void>(c.hDown, dChi), 16 * (size_t)n);
  if (trials) std::memcpy(trials, at<void>(c.hDown, dTr), 4 * (size_t)n);
  return YDORB_OK;
}

extern "C" int ydorb_sim3_release(int32_t device) { return release_staged(g_ctx, device); }
