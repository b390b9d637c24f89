// Host driver of the essential-graph optimisation + its C ABI (include/ydorb/c_api.h, "Essential-graph optimisation"):
// ydorb_essential_graph_optimize, ydorb_essential_graph_linearize, ydorb_essential_graph_trial_step, ydorb_essential_graph_set_profiling,
// ydorb_essential_graph_release, and ydorb_essential_graph_plan / _optimize_with / _trial_step_with, which choose the solver.
// A call checks its arguments, builds the per-vertex lists of incident edges, lays its device memory out once (three arenas of the
// per-device StagedCtx: the uploaded graph, the work area, the results), uploads in one copy and steps g2o's Levenberg-Marquardt
// schedule (lm_schedule.h) with one read-back of three scalars per trial.  The kernels are essential_kernels.hip.h's; the dense
// factorisation is the BA's, queued through chol_factor_solve (ydorb_host.h); the block-skyline one (essential_skyline.hip.h, planned
// on the host by skyline_plan.h) differs in the assemble and solve phases of a trial only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "essential_kernels.hip.h"
#include "essential_skyline.hip.h"
#include "host_buffers.h"
#include "lm_schedule.h"
#include "skyline_dev.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::ess;

namespace {

struct EssCtx : StagedCtx {
  bool profiling = false;
  hipEvent_t ev[10] = {};   // one pair per phase of a trial, reused: every trial ends in a synchronise
};
EssCtx g_ctx[16];   // this driver's own: nothing is shared with the other staged solvers

enum { PH_LIN = 0, PH_ASM, PH_SOLVE, PH_UPD, PH_CHI, PH_COUNT };

// The graph as the kernels index it: free vertices numbered in vertex order, every free vertex's incident edges twice.
struct Graph {
  int nV = 0, nE = 0, nP = 0, nF = 0, n = 0;
  std::vector<int> freeOf, vertOf, incStart, incE, incN, incO;
  bool sky = false;   // the block-skyline solver: P is planned, n = 7 nF
  sky::Plan P;
};

int fail(const char* what) { set_error("essential graph: %s", what); return YDORB_ERR_INVALID_ARG; }

// Every check of the ABI but the solver's size limit (chooseSolver), before any device work.
int checkGraph(const YdEssentialGraph* g, bool optimise, Graph& G) {
  if (!g) return fail("null graph");
  if (g->device < 0 || g->device >= 16) return fail("invalid device");
  if (g->n_vertices < 1 || g->n_edges < 0 || g->n_points < 0) return fail("negative or empty sizes");
  if (!g->sim3 || !g->fixed || (g->n_edges && (!g->edge_v0 || !g->edge_v1 || !g->edge_meas)) || (g->n_points && (!g->points || !g->point_ref)))
    return fail("null array");
  if (optimise && (g->iterations < 1 || g->max_trials < 1)) return fail("iterations and max_trials must be positive");
  if (optimise && !(g->lambda_init > 0 && std::isfinite(g->lambda_init))) return fail("lambda_init must be positive and finite");
  G.nV = g->n_vertices; G.nE = g->n_edges; G.nP = g->n_points;
  G.freeOf.assign(G.nV, -1);
  for (int v = 0; v < G.nV; v++) {
    if (!(g->sim3[8 * (size_t)v + 7] > 0)) { set_error("essential graph: vertex %d has a non-positive scale", v); return YDORB_ERR_INVALID_ARG; }
    if (!g->fixed[v]) { G.freeOf[v] = G.nF++; G.vertOf.push_back(v); }
  }
  if (G.nF == G.nV) return fail("no fixed vertex: the gauge is free");
  if (G.nF == 0) return fail("every vertex is fixed");
  for (int e = 0; e < G.nE; e++) {
    const int i = g->edge_v0[e], j = g->edge_v1[e];
    if (i < 0 || i >= G.nV || j < 0 || j >= G.nV) { set_error("essential graph: edge %d references a vertex out of range", e); return YDORB_ERR_INVALID_ARG; }
    if (i == j) { set_error("essential graph: edge %d joins vertex %d to itself", e, i); return YDORB_ERR_INVALID_ARG; }
    if (!(g->edge_meas[8 * (size_t)e + 7] > 0)) { set_error("essential graph: edge %d has a non-positive scale", e); return YDORB_ERR_INVALID_ARG; }
  }
  for (int p = 0; p < G.nP; p++)
    if (g->point_ref[p] < 0 || g->point_ref[p] >= G.nV) { set_error("essential graph: point %d references a vertex out of range", p); return YDORB_ERR_INVALID_ARG; }
  // incident edges per free vertex, in edge order; then the same entries ordered by neighbour (stable: edge order inside a neighbour)
  G.incStart.assign(G.nF + 1, 0);
  for (int e = 0; e < G.nE; e++) {
    const int fi = G.freeOf[g->edge_v0[e]], fj = G.freeOf[g->edge_v1[e]];
    if (fi >= 0) G.incStart[fi + 1]++;
    if (fj >= 0) G.incStart[fj + 1]++;
  }
  for (int f = 0; f < G.nF; f++) G.incStart[f + 1] += G.incStart[f];
  const int nInc = G.incStart[G.nF];
  G.incE.resize(nInc); G.incN.resize(nInc); G.incO.resize(nInc);
  std::vector<int> cursor(G.incStart.begin(), G.incStart.end() - 1), other(nInc);
  for (int e = 0; e < G.nE; e++) {
    const int fi = G.freeOf[g->edge_v0[e]], fj = G.freeOf[g->edge_v1[e]];
    if (fi >= 0) { other[cursor[fi]] = fj; G.incE[cursor[fi]++] = 2 * e; }
    if (fj >= 0) { other[cursor[fj]] = fi; G.incE[cursor[fj]++] = 2 * e + 1; }
  }
  std::vector<int> order;
  for (int f = 0; f < G.nF; f++) {
    const int q0 = G.incStart[f], q1 = G.incStart[f + 1];
    order.resize(q1 - q0);
    for (int q = q0; q < q1; q++) order[q - q0] = q;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return other[a] < other[b]; });
    for (int q = q0; q < q1; q++) { G.incN[q] = G.incE[order[q - q0]]; G.incO[q] = other[order[q - q0]]; }
  }
  return YDORB_OK;
}

const YdEssentialSolverOptions kDenseOptions = {YDORB_ESS_SOLVER_DENSE, YDORB_ESS_ORDER_SMALLER, 0};
constexpr long long kSkyMaxPairUpdates = 1LL << 24;   // 1.2e10 flop per trial; a dense envelope of 465 block rows, or a band of 6 over a million keyframes

// The solver of this call and its size limit; for SKYLINE, and whenever `info` is asked for, the plan.  Host only.
int chooseSolver(const YdEssentialGraph* g, const YdEssentialSolverOptions* opt, Graph& G, YdEssentialSolverInfo* info) {
  const YdEssentialSolverOptions O = opt ? *opt : YdEssentialSolverOptions{};
  if (O.solver < YDORB_ESS_SOLVER_AUTO || O.solver > YDORB_ESS_SOLVER_SKYLINE) return fail("unknown solver");
  if (O.ordering < YDORB_ESS_ORDER_SMALLER || O.ordering > YDORB_ESS_ORDER_RCM) return fail("unknown ordering");
  if (O.max_factor_bytes < 0) return fail("negative max_factor_bytes");
  const int maxFree = chol_max_rows() / 7;
  G.sky = O.solver == YDORB_ESS_SOLVER_SKYLINE || (O.solver == YDORB_ESS_SOLVER_AUTO && G.nF > maxFree);
  if (!G.sky && G.nF > maxFree) {
    set_error("essential graph: %d free vertices, the dense solve takes at most %d (%d rows)", G.nF, maxFree, chol_max_rows());
    return YDORB_ERR_UNSUPPORTED;
  }
  G.n = G.sky ? 7 * G.nF : (7 * G.nF + kCholTile - 1) / kCholTile * kCholTile;
  if (G.sky || info) {
    std::vector<int> fa(G.nE), fb(G.nE);
    for (int e = 0; e < G.nE; e++) { fa[e] = G.freeOf[g->edge_v0[e]]; fb[e] = G.freeOf[g->edge_v1[e]]; }
    G.P = sky::makePlan(G.nF, G.nE, fa.data(), fb.data(), O.ordering);
  }
  if (G.sky) {
    const long long limit = O.max_factor_bytes ? (long long)O.max_factor_bytes : (long long)chol_max_rows() * chol_max_rows() * 8;
    const long long bytes = (long long)(G.P.envBlocks * sky::kBlockBytes);
    if (bytes > limit) {
      set_error("essential graph: the skyline envelope takes %lld bytes (%lld blocks, %s order), max_factor_bytes is %lld", bytes,
                (long long)G.P.envBlocks, G.P.orderingUsed == YDORB_ESS_ORDER_RCM ? "RCM" : "natural", limit);
      return YDORB_ERR_UNSUPPORTED;
    }
    // The bytes bound the memory, not the time: one workgroup walks the columns, and a dense envelope within the default bytes would
    // keep it busy for tens of minutes in one launch that nothing can interrupt.  kSkyMaxPairUpdates block updates (686 flop each)
    // are a few seconds of that walk per trial at the rate measured on a band; a map's envelope stays orders below.
    if (G.P.pairUpdates > kSkyMaxPairUpdates) {
      set_error("essential graph: the skyline factorisation takes %lld block updates per trial (%lld envelope blocks, %s order), at most %lld "
                "are run in one workgroup", (long long)G.P.pairUpdates, (long long)G.P.envBlocks,
                G.P.orderingUsed == YDORB_ESS_ORDER_RCM ? "RCM" : "natural", (long long)kSkyMaxPairUpdates);
      return YDORB_ERR_UNSUPPORTED;
    }
    sky::buildColumns(G.P);
  }
  if (info) {
    info->solver_used = G.sky ? YDORB_ESS_SOLVER_SKYLINE : YDORB_ESS_SOLVER_DENSE;
    info->ordering_used = G.P.orderingUsed; info->n_free = G.nF; info->max_row_blocks = G.P.maxRowBlocks;
    info->envelope_blocks = G.P.envBlocks; info->envelope_blocks_natural = G.P.envNatural; info->envelope_blocks_rcm = G.P.envRcm;
    info->factor_bytes = G.sky ? G.P.envBlocks * sky::kBlockBytes : (int64_t)G.n * G.n * 8;
  }
  return YDORB_OK;
}

// The plan's arrays on the device (SKYLINE only; null otherwise)
using SkyPtrs = sky::PlanArrays;
struct UpPtrs { double *est0, *meas; int *v0, *v1, *freeOf, *vertOf, *incStart, *incE, *incN, *incO, *pref; float* pts; SkyPtrs k; };
size_t layUp(const Graph& G, void* base, UpPtrs& u) {
  Carve a(base);
  const size_t nInc = std::max<size_t>(G.incE.size(), 1), E = std::max(G.nE, 1), P = std::max(G.nP, 1);
  a.take(u.est0, 8 * (size_t)G.nV); a.take(u.meas, 8 * E); a.take(u.v0, E); a.take(u.v1, E); a.take(u.freeOf, G.nV); a.take(u.vertOf, G.nF);
  a.take(u.incStart, G.nF + 1); a.take(u.incE, nInc); a.take(u.incN, nInc); a.take(u.incO, nInc); a.take(u.pts, 3 * P); a.take(u.pref, P);
  u.k = SkyPtrs{};
  if (G.sky) u.k.take(a, G.P, true, 1);
  return a.L.bytes;
}
// The work area.  It keeps what earlier, differently sized calls left, so every array has a first writer inside the call:
//   est[0], est[1]  copies of the upload;  err, chiE, J, Hb, bb: k_ess_linearize, every edge (chiE again by k_ess_chi2)
//   S, bkeep, bwork k_ess_assemble, every element, every trial;  status: k_ess_assemble, every trial
//   diagInv         one memset per call (a panel that meets a non-positive pivot leaves its tile as it was: see ba_solver.hip)
//   diagL           write-only;  yv: [0, n - 32) by the factorisation's forward substitution, all the solve reads;  x: the solve, [0, n)
//   sv              k_ess_update, every free vertex
// SKYLINE: S is the envelope (49 doubles per block), written whole by k_ess_assemble_sky every trial with bkeep, bwork and status;
// x and diagInv (here the 7 nF reciprocal pivots) by k_ess_sky_solve, every free vertex; diagL and yv are not used and take no room.
struct WorkPtrs { double *est[2], *err, *chiE, *J, *Hb, *bb, *S, *bkeep, *bwork, *diagInv, *diagL, *yv, *x, *sv; int* status; };
size_t layWork(const Graph& G, void* base, WorkPtrs& w) {
  Carve a(base);
  const size_t E = std::max(G.nE, 1), n = G.n, nS = G.sky ? 49 * (size_t)G.P.envBlocks : n * n, nT = G.sky ? 0 : n * kCholTile, nI = G.sky ? n : nT, nY = G.sky ? 0 : n;
  a.take(w.est[0], 8 * (size_t)G.nV); a.take(w.est[1], 8 * (size_t)G.nV); a.take(w.err, 7 * E); a.take(w.chiE, E); a.take(w.J, kJ * E);
  a.take(w.Hb, kH * E); a.take(w.bb, kB * E); a.take(w.S, nS); a.take(w.bkeep, n); a.take(w.bwork, n); a.take(w.diagInv, nI);
  a.take(w.diagL, nT); a.take(w.yv, nY); a.take(w.x, n); a.take(w.sv, G.nF); a.take(w.status, 2);
  return a.L.bytes;
}
struct DownPtrs { double *scal, *est; float* pts; };
size_t layDown(const Graph& G, void* base, DownPtrs& d) {
  Carve a(base);
  a.take(d.scal, 4); a.take(d.est, 8 * (size_t)G.nV); a.take(d.pts, 3 * (size_t)std::max(G.nP, 1));
  return a.L.bytes;
}

struct Run {
  EssCtx& c;
  const YdEssentialGraph* g;
  Graph G;
  UpPtrs u, hu;   // device / pinned views of the upload arena
  WorkPtrs w;
  DownPtrs d, hd;
  float ms[PH_COUNT] = {};
  int pending[PH_COUNT] = {};
  explicit Run(EssCtx& ctx, const YdEssentialGraph* graph) : c(ctx), g(graph) {}
};

int begin(Run& R_) {
  EssCtx& c = R_.c;
  const Graph& G = R_.G;
  const YdEssentialGraph* g = R_.g;
  int rc;
  UpPtrs tmpU; WorkPtrs tmpW; DownPtrs tmpD;
  const size_t ub = layUp(G, nullptr, tmpU), wb = layWork(G, nullptr, tmpW), db = layDown(G, nullptr, tmpD);
  if ((rc = c.ensure(ub, db, wb))) return rc;
  layUp(G, c.up.p, R_.u); layUp(G, c.hUp.p, R_.hu); layWork(G, c.scratch.p, R_.w); layDown(G, c.down.p, R_.d); layDown(G, c.hDown.p, R_.hd);
  UpPtrs& h = R_.hu;
  const size_t E = G.nE, P = G.nP, nInc = G.incE.size();
  std::memcpy(h.est0, g->sim3, 64 * (size_t)G.nV);
  if (E) { std::memcpy(h.meas, g->edge_meas, 64 * E); std::memcpy(h.v0, g->edge_v0, 4 * E); std::memcpy(h.v1, g->edge_v1, 4 * E); }
  std::memcpy(h.freeOf, G.freeOf.data(), 4 * (size_t)G.nV);
  std::memcpy(h.vertOf, G.vertOf.data(), 4 * (size_t)G.nF);
  std::memcpy(h.incStart, G.incStart.data(), 4 * (size_t)(G.nF + 1));
  if (nInc) { std::memcpy(h.incE, G.incE.data(), 4 * nInc); std::memcpy(h.incN, G.incN.data(), 4 * nInc); std::memcpy(h.incO, G.incO.data(), 4 * nInc); }
  if (P) { std::memcpy(h.pts, g->points, 12 * P); std::memcpy(h.pref, g->point_ref, 4 * P); }
  if (G.sky) h.k.fill(G.P, [](void* dst, const void* src, size_t bytes) { if (bytes) std::memcpy(dst, src, bytes); });
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, ub, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(R_.w.est[0], R_.u.est0, 64 * (size_t)G.nV, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(R_.w.est[1], R_.u.est0, 64 * (size_t)G.nV, hipMemcpyDeviceToDevice, s));
  if (!G.sky) HIPCHK(hipMemsetAsync(R_.w.diagInv, 0, sizeof(double) * (size_t)G.n * kCholTile, s));
  return YDORB_OK;
}

// Event pair around the launches of one phase when profiling is on; the elapsed time is collected after the trial's synchronise.
struct Phase {
  Run& R_;
  int ph;
  Phase(Run& r, int phase) : R_(r), ph(phase) { if (R_.c.profiling) (void)hipEventRecord(R_.c.ev[2 * ph], R_.c.stream); }
  ~Phase() { if (R_.c.profiling) { (void)hipEventRecord(R_.c.ev[2 * ph + 1], R_.c.stream); R_.pending[ph] = 1; } }
};
void collect(Run& R_) {
  for (int ph = 0; ph < PH_COUNT; ph++)
    if (R_.pending[ph]) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, R_.c.ev[2 * ph], R_.c.ev[2 * ph + 1]) == hipSuccess) R_.ms[ph] += ms;
      R_.pending[ph] = 0;
    }
}

void linearize(Run& R_, const double* est) {
  const Graph& G = R_.G;
  if (G.nE)
    hipLaunchKernelGGL(k_ess_linearize, dim3(G.nE), dim3(64), 0, R_.c.stream, G.nE, est, R_.u.freeOf, R_.u.v0, R_.u.v1, R_.u.meas, R_.g->fix_scale,
                       R_.w.err, R_.w.chiE, R_.w.J, R_.w.Hb, R_.w.bb);
}

// H + lambda I and b of the linearised graph, into the solver's storage
void assemble(Run& R_, double lambda) {
  const Graph& G = R_.G;
  WorkPtrs& w = R_.w;
  const UpPtrs& u = R_.u;
  if (G.sky)
    hipLaunchKernelGGL(k_ess_assemble_sky, dim3(G.nF + 1), dim3(64), 0, R_.c.stream, G.nF, lambda, u.incStart, u.incE, u.incN, u.incO, w.Hb, w.bb, u.k.inv,
                       u.k.first, u.k.rowOff, w.S, w.bkeep, w.bwork, w.status);
  else
    hipLaunchKernelGGL(k_ess_assemble, dim3(G.nF + 1), dim3(64), 0, R_.c.stream, G.nF, G.n, lambda, u.incStart, u.incE, u.incN, u.incO, w.Hb, w.bb, w.S,
                       w.bkeep, w.bwork, w.status);
}

// factorise and solve what assemble() left: x, and status[0] raised on a non-positive pivot
int solve(Run& R_) {
  const Graph& G = R_.G;
  WorkPtrs& w = R_.w;
  if (!G.sky) return chol_factor_solve(R_.c.stream, w.S, w.diagL, w.diagInv, G.n, w.status, w.bwork, w.yv, w.x);
  const SkyPtrs& k = R_.u.k;
  hipLaunchKernelGGL(k_ess_sky_solve, dim3(1), dim3(256), 0, R_.c.stream, G.nF, k.first, k.rowOff, k.colStart, k.colRows, k.colBlk, k.perm, w.S, w.bwork, w.x,
                     w.diagInv, w.status);
  return YDORB_OK;
}

int readScal(Run& R_) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(R_.hd.scal, R_.d.scal, sizeof(double) * 4, hipMemcpyDeviceToHost, R_.c.stream));
  HIPCHK(hipStreamSynchronize(R_.c.stream));
  collect(R_);
  return YDORB_OK;
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg and a user lambda; returns the buffer that holds the result
int optimize(Run& R_, YdBaResult* res, int* curOut) {
  const Graph& G = R_.G;
  const YdEssentialGraph* g = R_.g;
  WorkPtrs& w = R_.w;
  hipStream_t s = R_.c.stream;
  int rc, cur = 0;
  YdBaOptions O;
  std::memset(&O, 0, sizeof O);
  O.iters1 = g->iterations; O.max_trials = g->max_trials; O.flags = YDORB_BA_SINGLE_STAGE;
  LmSchedule lm;
  lm.begin(O, res);
  lm.userLambdaInit = g->lambda_init;
  for (bool more = lm.firstIteration(nullptr); more;) {
    {  // computeActiveErrors + buildSystem: errors, chi2 and the blocks of every edge
      Phase t(R_, PH_LIN);
      linearize(R_, w.est[cur]);
    }
    if (lm.needChi2()) {
      hipLaunchKernelGGL(k_ess_sum, dim3(1), dim3(256), 0, s, w.chiE, G.nE, w.sv, 0, w.status, R_.d.scal);
      if ((rc = readScal(R_))) return rc;
      lm.setChi2(R_.hd.scal[0]);
    }
    if (lm.needLambdaInit()) lm.setMaxDiag(0);   // the user lambda: no diagonal is looked at
    LmSchedule::Next next;
    do {
      const int nxt = cur ^ 1;
      {
        Phase t(R_, PH_ASM);
        assemble(R_, lm.lambda);
      }
      {
        Phase t(R_, PH_SOLVE);
        if ((rc = solve(R_))) return rc;
      }
      {
        Phase t(R_, PH_UPD);
        hipLaunchKernelGGL(k_ess_update, dim3((G.nF + 255) / 256), dim3(256), 0, s, G.nF, R_.u.vertOf, w.est[cur], w.est[nxt], w.x, w.bkeep, lm.lambda,
                           g->fix_scale, w.sv);
      }
      {
        Phase t(R_, PH_CHI);
        if (G.nE) hipLaunchKernelGGL(k_ess_chi2, dim3((G.nE + 255) / 256), dim3(256), 0, s, G.nE, w.est[nxt], R_.u.v0, R_.u.v1, R_.u.meas, w.chiE);
        hipLaunchKernelGGL(k_ess_sum, dim3(1), dim3(256), 0, s, w.chiE, G.nE, w.sv, G.nF, w.status, R_.d.scal);
      }
      if ((rc = readScal(R_))) return rc;
      next = lm.trial(R_.hd.scal[0], R_.hd.scal[1], R_.hd.scal[2] == 0, nullptr);
      if (lm.lastAccepted) cur = nxt;
    } while (next == LmSchedule::Retry);
    more = next == LmSchedule::NextIteration;
  }
  *curOut = cur;
  return YDORB_OK;
}

}  // namespace

extern "C" int ydorb_essential_graph_plan(const YdEssentialGraph* g, const YdEssentialSolverOptions* opt, YdEssentialSolverInfo* info, int32_t* perm,
                                          int32_t* first) {
  if (!info) return fail("null info");
  std::memset(info, 0, sizeof *info);
  Graph G;
  int rc = checkGraph(g, true, G);
  if (rc) return rc;
  if ((rc = chooseSolver(g, opt, G, info))) return rc;
  if (perm) std::memcpy(perm, G.P.perm.data(), 4 * (size_t)G.nF);
  if (first) std::memcpy(first, G.P.first.data(), 4 * (size_t)G.nF);
  return YDORB_OK;
}

extern "C" int ydorb_essential_graph_optimize_with(const YdEssentialGraph* g, const YdEssentialSolverOptions* opt, float* points_out, YdBaResult* res,
                                                   YdEssentialSolverInfo* info) {
  if (!res) return fail("null result");
  std::memset(res, 0, sizeof *res);
  if (info) std::memset(info, 0, sizeof *info);
  EssCtx* ctx = g && g->device >= 0 && g->device < 16 ? &g_ctx[g->device] : &g_ctx[0];
  Run R_(*ctx, g);
  int rc = checkGraph(g, true, R_.G);
  if (rc) return rc;
  if ((rc = chooseSolver(g, opt, R_.G, info))) return rc;
  if (g->n_points && !points_out) return fail("null points_out");
  if ((rc = require_device(g->device))) return rc;
  EssCtx& c = *ctx;
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(g->device))) return rc;
  if (c.profiling)
    for (hipEvent_t& e : c.ev)
      if (!e) HIPCHK(hipEventCreate(&e));
  if ((rc = begin(R_))) return rc;
  int cur = 0;
  if ((rc = optimize(R_, res, &cur))) return rc;
  const Graph& G = R_.G;
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(R_.d.est, R_.w.est[cur], 64 * (size_t)G.nV, hipMemcpyDeviceToDevice, s));
  if (G.nP) hipLaunchKernelGGL(k_ess_points, dim3((G.nP + 255) / 256), dim3(256), 0, s, G.nP, R_.u.pts, R_.u.pref, R_.u.est0, R_.d.est, R_.d.pts);
  HIPCHK(hipGetLastError());
  DownPtrs tmp;
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, layDown(G, nullptr, tmp), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(g->sim3, R_.hd.est, 64 * (size_t)G.nV);
  if (G.nP) std::memcpy(points_out, R_.hd.pts, 12 * (size_t)G.nP);
  res->ms_build = R_.ms[PH_LIN]; res->ms_schur = R_.ms[PH_ASM]; res->ms_solve = R_.ms[PH_SOLVE]; res->ms_update = R_.ms[PH_UPD]; res->ms_errors = R_.ms[PH_CHI];
  res->ms_total = res->ms_build + res->ms_schur + res->ms_solve + res->ms_update + res->ms_errors;
  return YDORB_OK;
}

extern "C" int ydorb_essential_graph_optimize(const YdEssentialGraph* g, float* points_out, YdBaResult* res) {
  return ydorb_essential_graph_optimize_with(g, &kDenseOptions, points_out, res, nullptr);
}

extern "C" int ydorb_essential_graph_linearize(const YdEssentialGraph* g, double* err, double* J0, double* J1, double* chi2) {
  EssCtx* ctx = g && g->device >= 0 && g->device < 16 ? &g_ctx[g->device] : &g_ctx[0];
  Run R_(*ctx, g);
  int rc = checkGraph(g, false, R_.G);
  if (rc) return rc;
  if ((rc = chooseSolver(g, &kDenseOptions, R_.G, nullptr))) return rc;
  if ((rc = require_device(g->device))) return rc;
  EssCtx& c = *ctx;
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(g->device))) return rc;
  if ((rc = begin(R_))) return rc;
  const bool was = c.profiling;
  c.profiling = false;
  linearize(R_, R_.w.est[0]);
  c.profiling = was;
  HIPCHK(hipGetLastError());
  const size_t E = R_.G.nE;
  std::vector<double> J(kJ * E);
  if (E) {
    if (err) HIPCHK(hipMemcpyAsync(err, R_.w.err, 56 * E, hipMemcpyDeviceToHost, c.stream));
    if (chi2) HIPCHK(hipMemcpyAsync(chi2, R_.w.chiE, 8 * E, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(J.data(), R_.w.J, 8 * kJ * E, hipMemcpyDeviceToHost, c.stream));
  }
  HIPCHK(hipStreamSynchronize(c.stream));
  for (size_t e = 0; e < E; e++) {
    if (J0) std::memcpy(J0 + 49 * e, J.data() + kJ * e, 49 * 8);
    if (J1) std::memcpy(J1 + 49 * e, J.data() + kJ * e + 49, 49 * 8);
  }
  return YDORB_OK;
}

extern "C" int ydorb_essential_graph_trial_step(const YdEssentialGraph* g, double lambda, double* x, int32_t* solved) {
  {   // the order of the checks as ever: the graph, the dense limit, then the outputs and lambda
    Graph G;
    int rc = checkGraph(g, false, G);
    if (rc || (rc = chooseSolver(g, &kDenseOptions, G, nullptr))) return rc;
    if (!x || !solved || !(lambda > 0)) return fail("trial step: null output or non-positive lambda");
  }
  return ydorb_essential_graph_trial_step_with(g, &kDenseOptions, lambda, x, solved, nullptr, nullptr);
}

// The assembled system (lambda = 0) out of the solver's storage, expanded to dense in the caller's vertex order.
int copySystem(Run& R_, double* H_out, double* b_out) {
  const Graph& G = R_.G;
  hipStream_t s = R_.c.stream;
  const size_t N = 7 * (size_t)G.nF;
  if (b_out) HIPCHK(hipMemcpyAsync(b_out, R_.w.bkeep, 8 * N, hipMemcpyDeviceToHost, s));
  if (!H_out) { HIPCHK(hipStreamSynchronize(s)); return YDORB_OK; }
  std::vector<double> S(G.sky ? 49 * (size_t)G.P.envBlocks : (size_t)G.n * G.n);
  HIPCHK(hipMemcpyAsync(S.data(), R_.w.S, 8 * S.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (!G.sky) {
    for (size_t r = 0; r < N; r++) std::memcpy(H_out + r * N, S.data() + r * G.n, 8 * N);
    return YDORB_OK;
  }
  sky::expandEnvelope<7>(G.P, S.data(), H_out, sky::kDiagWhole);
  return YDORB_OK;
}

extern "C" int ydorb_essential_graph_trial_step_with(const YdEssentialGraph* g, const YdEssentialSolverOptions* opt, double lambda, double* x,
                                                     int32_t* solved, double* H_out, double* b_out) {
  EssCtx* ctx = g && g->device >= 0 && g->device < 16 ? &g_ctx[g->device] : &g_ctx[0];
  Run R_(*ctx, g);
  int rc = checkGraph(g, false, R_.G);
  if (rc) return rc;
  if (!x || !solved) return fail("trial step: null output or non-positive lambda");
  if ((rc = chooseSolver(g, opt, R_.G, nullptr))) return rc;
  if ((H_out || b_out) && 7 * R_.G.nF > 4096) return fail("trial step: H_out / b_out are copied for at most 4096 rows");
  if ((rc = require_device(g->device))) return rc;
  EssCtx& c = *ctx;
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(g->device))) return rc;
  if ((rc = begin(R_))) return rc;
  const Graph& G = R_.G;
  WorkPtrs& w = R_.w;
  const bool was = c.profiling;
  c.profiling = false;
  linearize(R_, w.est[0]);
  c.profiling = was;
  if (H_out || b_out) {
    assemble(R_, 0.0);
    if ((rc = copySystem(R_, H_out, b_out))) return rc;
  }
  assemble(R_, lambda);
  if ((rc = solve(R_))) return rc;
  int status[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(x, w.x, sizeof(double) * 7 * (size_t)G.nF, hipMemcpyDeviceToHost, c.stream));
  HIPCHK(hipMemcpyAsync(status, w.status, sizeof(int), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(hipStreamSynchronize(c.stream));
  *solved = status[0] == 0;
  return YDORB_OK;
}

extern "C" int ydorb_essential_graph_set_profiling(int32_t device, int32_t on) {
  if (device < 0 || device >= 16) { set_error("invalid device"); return YDORB_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lock(g_ctx[device].mu);
  g_ctx[device].profiling = on != 0;
  return YDORB_OK;
}

extern "C" int ydorb_essential_graph_release(int32_t device) {
  const int rc = release_staged(g_ctx, device);   // waits for the stream: no event is in flight behind it
  if (rc) return rc;
  EssCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  for (hipEvent_t& e : c.ev)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  return YDORB_OK;
}
