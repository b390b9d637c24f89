// Host driver of the MI355X local-BA back-end + its C ABI (include/ydorb/c_api.h, "Local bundle adjustment").
// Sequencing restated from the reference: two-stage schedule of Optimizer::localBundleAdjust
// (src/optimizer.cpp:284-334), SparseOptimizer::initializeOptimization/optimize
// (thirdParty/g2o/g2o/core/sparse_optimizer.cpp:208-280, 366-440) and the Levenberg-Marquardt trial loop
// (core/optimization_algorithm_levenberg.cpp:57-173).  All arithmetic on the graph runs in ba_kernels.hip.h;
// the host only sorts the edge list, steps the LM schedule (lm_schedule.h), and reads three scalars per trial.
#include <hip/hip_runtime.h>
#include <chrono>

#include <algorithm>
#include <string>
#include <thread>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <numeric>
#include <optional>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "ba_kernels.hip.h"
#include "ba_pairs.h"
#include "ba_skyline.hip.h"
#include "host_buffers.h"
#include "lm_schedule.h"
#include "skyline_dev.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::ba;

namespace {

enum { PH_ERR = 0, PH_BUILD, PH_SCHUR, PH_SOLVE, PH_UPDATE, PH_COUNT };

// The reduced system of one optimize() call: stage 1 sizes it, stage 2 re-uses it (and the arenas laid out for it) as it is.
// sky: the block-skyline solver (ba_skyline.hip.h).  n = 6 nPf then, nBuckets = the covisible pairs + nPf, and `plan` holds the envelope.
struct Sys {
  std::vector<int> act; int nL = 0, nPf = 0, Ea = 0, n = 0, nb = 0, nBlkE = 0, nBuckets = 0, nPoseEdges = 0; size_t nItems = 0;
  bool sky = false;
  sky::Plan plan;
  size_t envDoubles() const { return 36 * (size_t)plan.envBlocks; }
};
static_assert(bapairs::kDenseMaxRows == kCholSolveMaxN, "ba_pairs.h states the dense limit for the host-only plan");

// `state`: both copies of the estimate (LM push / pop is a swap of the index).  beginSolve uploads [0]; prepareStage copies cur -> cur ^ 1
// whole before the first k_update of a stage, which writes the free poses and the active landmarks only.
struct StatePtrs { double *poses[2], *pts[2]; };
size_t layState(int K, int NP, void* base, StatePtrs& st) {
  Carve a(base);
  for (int i = 0; i < 2; i++) { a.take(st.poses[i], (size_t)7 * K); a.take(st.pts[i], (size_t)3 * NP); }
  return a.L.bytes;
}

// `up`: what the host orders and uploads for a stage, through the pinned staging area at the same offsets and with ONE copy (twelve
// before: with 16 set-up threads of a batch the runtime's lock was the cost).  Written whole by that copy; k_cull later rewrites eInfo / eRobust.
// SKYLINE adds the pair table (PairList: rowStart, i1, i2 and each bucket's place in the envelope) and the plan's arrays.
struct SkyPtrs : sky::PlanArrays { int *pairRow, *pairI1, *pairI2; long long* pairDst; };
struct UpPtrs { int *ePose, *ePidx, *ePt, *eLm, *ptStart, *poseStart, *ptOf, *poseEdges, *poseOf; double *eMeas, *eInfo; uint8_t* eRobust; SkyPtrs k; };
size_t layUp(const Sys& Y, void* base, UpPtrs& u) {
  Carve a(base);
  const size_t Ea = Y.Ea;
  a.take(u.ePose, Ea); a.take(u.ePidx, Ea); a.take(u.ePt, Ea); a.take(u.eLm, Ea); a.take(u.eMeas, 3 * Ea); a.take(u.eInfo, Ea); a.take(u.eRobust, Ea);
  a.take(u.ptStart, Y.nL + 1); a.take(u.poseStart, Y.nPf + 1); a.take(u.ptOf, Y.nL); a.take(u.poseEdges, Y.nPoseEdges); a.take(u.poseOf, Y.nPf);
  u.k = SkyPtrs{};
  if (Y.sky) {
    const size_t nB = Y.nBuckets, nF = Y.nPf;
    a.take(u.k.pairRow, nF + 1); a.take(u.k.pairI1, nB); a.take(u.k.pairI2, nB); a.take(u.k.pairDst, nB);
    u.k.take(a, Y.plan, false);
  }
  return a.L.bytes;
}

// `work`: everything the device itself writes during a stage.  Nothing is cleared at allocation and the arena keeps whatever an earlier,
// differently laid out solve left, so every array needs a first writer inside the stage.  Who that is ("free edge" = pidx >= 0; the
// lock-step kb_* wrappers leave before the body when blockIdx.x is past the member's OWN count, so a member smaller than the grid reads
// and writes exactly what its single solve does; it keeps scal / status in the pool's dScal, with the same writers):
//   eInfo0    copy of eInfo right after the upload;  eOutlier: k_cull(final), every edge, before the read-back
//   err       memset at stage 1 (an edge that is never evaluated has error 0), then k_errors for every edge with information != 0
//   pair*     pairCnt: memset, then k_pair_count;  pairStart: k_excl_scan, [0 .. nBuckets];  pairCursor: copy of pairStart;  pairA: k_pair_fill,
//             pairB: k_pair_sort, all nItems entries each.  With nBuckets == 0 none of the five is written or read.
//   partial   [0, nBlkE) k_errors and [nBlkE, ..) k_scale, one per workgroup; k_sum_partials reads exactly those counts
//   Hll, bl   k_build_points, every landmark;  Hpl: k_build_points, every free edge (zeros for a culled one), the only ones read
//   Hpp | bp  k_build_poses, every free pose;  Dinv, db: k_dinv, every landmark;  BD: k_bd, every free edge
//   status    k_dinv, the first kernel of every trial, before k_chol_step / k_sum_partials touch it
//   S | bs | diagInv   ONE memset at the start of every stage.  Per trial k_schur_pairs writes the lower 6x6 blocks and the padding, k_bs bs;
//             the diagonal 32x32 tiles above the block diagonal are only written by the rank-32 updates and loaded (not used) by the next
//             factorisation: hence the clear of S.  diagInv[kb] is written by launch kb of k_chol_step UNLESS a pivot is not positive: the
//             panel then leaves early, and the later launches and k_chol_solve read diagInv[kb ..] as the last trial left it.  That step is
//             rejected, yet its scale sum decides the sign of rho: before diagInv was cleared with S, a failed first factorisation of a
//             solve read whatever the memory held.  diagL is write-only.
//   yv        [0, n - 32) by the forward-substitution workgroup of k_chol_step launches 1 .. nb - 1, all k_chol_solve reads
//   xp        k_chol_solve, [0, n);  xl: k_backsub, every landmark
//   SKYLINE   S is the envelope (36 doubles per block) | bs: the envelope is cleared and then written by k_sky_schur_pairs in EVERY trial
//             (the factorisation overwrites it, and the blocks no pair writes are its fill), bs by k_bs as above.  skyW [12 nPf]: b by
//             position, then the reciprocal pivots, both written whole by k_sky_solve before it reads them.  diagInv, diagL and yv take
//             no room.  pair*: as above with the pair table's buckets.
//   scal      [0] and [2] k_sum_partials, [1] k_max_diag (first iteration), [6], [7] the status copies; [3 .. 5] are never written: they
//             travel to the host with every read-back and nothing there reads them
struct WorkPtrs {
  double *eInfo0, *err, *partial, *Hll, *bl, *Hpl, *BD, *Hpp, *S, *diagInv, *diagL, *Dinv, *db, *xp, *xl, *yv, *skyW, *scal;
  uint8_t* eOutlier;
  int *status, *pairCnt, *pairStart, *pairCursor;
  int2 *pairA, *pairB;
  double* bp(const Sys& Y) const { return Hpp + (size_t)36 * Y.nPf; }   // Hpp | bp: one all-reduce covers both
  double* bs(const Sys& Y) const { return S + (Y.sky ? Y.envDoubles() : (size_t)Y.n * Y.n); }      // S | bs likewise
};
size_t layWork(const Sys& Y, void* base, WorkPtrs& w) {
  Carve a(base);
  const size_t Ea = Y.Ea, nL = Y.nL, nPf = Y.nPf, n = Y.n, tiles = Y.sky ? 0 : (size_t)Y.nb * NB * NB, nBk = (size_t)Y.nBuckets + 1, items = std::max<size_t>(Y.nItems, 1);
  a.take(w.eInfo0, Ea); a.take(w.eOutlier, Ea); a.take(w.err, 3 * Ea); a.take(w.partial, Y.nBlkE + (6 * nPf + 3 * nL + 255) / 256 + 1);
  a.take(w.Hll, 6 * nL); a.take(w.bl, 3 * nL); a.take(w.Hpl, 18 * Ea); a.take(w.BD, 18 * Ea); a.take(w.Hpp, 42 * std::max<size_t>(nPf, 1));
  const size_t nS = Y.sky ? Y.envDoubles() : n * n;
  a.take(w.S, nS + n + tiles); w.diagInv = w.S + nS + n;   // one array on purpose: cleared together
  a.take(w.diagL, tiles); a.take(w.Dinv, 6 * nL); a.take(w.db, 3 * nL); a.take(w.xp, n); a.take(w.yv, Y.sky ? 0 : n); a.take(w.skyW, Y.sky ? 2 * n : 0);
  a.take(w.xl, 3 * nL);
  a.take(w.scal, 8); a.take(w.status, 2); a.take(w.pairCnt, nBk); a.take(w.pairStart, nBk); a.take(w.pairCursor, nBk); a.take(w.pairA, items); a.take(w.pairB, items);
  return a.L.bytes;
}

// `pose`: the arrays of one ydorb_pose_optimize batch; the first five are uploaded, the rest written by k_pose_optimize.
struct PosePtrs { int *start, *inl, *trials; double *poses, *X, *meas, *info, *err, *chi; uint8_t *flags, *outlier; };
size_t layPose(int n, size_t E, void* base, PosePtrs& q) {
  Carve a(base);
  a.take(q.start, n + 1); a.take(q.poses, (size_t)7 * n); a.take(q.X, 3 * E); a.take(q.meas, 3 * E); a.take(q.info, E);
  a.take(q.err, 3 * E); a.take(q.flags, E); a.take(q.outlier, E); a.take(q.inl, n); a.take(q.chi, (size_t)4 * n); a.take(q.trials, n);
  return a.L.bytes;
}

// The device memory and staging of ONE solve: a single solve's context and a lock-step batch member hold one each.  An arena grows
// with 25 % slack when a solve needs more than it has and is otherwise re-laid out in place.
struct SolveMem {
  int device = -1;
  hipStream_t stream = nullptr;   // a batch member: the set-up or the batch's stream (not owned)
  Mem state, up, work;
  StatePtrs st{};   // where the arrays of the three arenas are (layState / layUp / layWork)
  UpPtrs u{};
  WorkPtrs w{};
  PinnedMem hStage;   // pinned staging of the ordered edge arrays on their way up and of the results on their way down: an asynchronous
                      // copy out of / into pageable memory runs at ~8 GB/s and makes the host wait for the stream
  int stage(size_t bytes) { return bytes <= hStage.cap ? YDORB_OK : hStage.alloc(bytes + bytes / 4 + 4096); }
  void releaseBuffers() { for (Mem* m : {&state, &up, &work, static_cast<Mem*>(&hStage)}) m->release(); }
};

struct Ctx {  // per-device context of the single solves and the pose batches, reused across calls (localBundleAdjust runs on one thread, localMapping.cpp:29)
  SolveMem mem;
  Mem pose;   // pose-only batches (layPose)
  hipEvent_t ev[2 * PH_COUNT + 2]{};
  PinnedMem hPin;   // read-back area: scal[8] (one stream sync per LM trial); lives as long as the stream and the events
  // ydorb_ba_release: device scratch and pinned staging back to the system (stream, events and hPin stay)
  void releaseBuffers() { mem.releaseBuffers(); pose.release(); }
};
// A small pool of contexts per device: one localBundleAdjust at a time is the reference's use (LocalMapping thread), but the solve
// is a latency chain that leaves most of the GPU idle, so several host threads (several maps / sessions) may solve concurrently,
// each on its own stream and scratch.
constexpr int kCtxPool = 8;
std::mutex g_mu[16][kCtxPool];
Ctx g_ctx[16][kCtxPool];
std::mutex g_pick;

// Locks a free context of the device's pool (all busy: queues behind slot 0) and creates its stream, events and read-back area on first
// use.  Null when that failed; the error text is set.
Ctx* acquireCtx(int device, std::unique_lock<std::mutex>& lock) {
  int slot = -1;
  {
    std::lock_guard<std::mutex> pick(g_pick);
    for (int i = 0; i < kCtxPool && slot < 0; i++)
      if (g_mu[device][i].try_lock()) slot = i;
  }
  if (slot < 0) { slot = 0; g_mu[device][0].lock(); }
  lock = std::unique_lock<std::mutex>(g_mu[device][slot], std::adopt_lock);
  Ctx& c = g_ctx[device][slot];
  auto init = [&]() -> int {
    c.mem.device = device;
    HIPCHK(hipStreamCreateWithFlags(&c.mem.stream, hipStreamNonBlocking));
    for (auto& e : c.ev) HIPCHK(hipEventCreate(&e));
    return c.hPin.alloc(sizeof(double) * 16);
  };
  if (!c.mem.stream && init() != YDORB_OK) return nullptr;
  return &c;
}

struct Run {
  SolveMem* c;
  const YdBaProblem* P;
  const YdBaOptions* O;
  YdBaResult* res;
  int cur = 0;  // which of poses[2]/pts[2] holds the current estimate
  bool noRobust = false;   // YDORB_BA_NO_ROBUST
  Cam cam;
  bool phaseTimes = false;   // YDORB_BA_PHASE_TIMES
  double phaseMs[PH_COUNT] = {0, 0, 0, 0, 0};
  bool pending[PH_COUNT] = {false, false, false, false, false};
  Sys sys;
  hipEvent_t* ev = nullptr;   // Ctx::ev and Ctx::hPin of a single solve (optimize()); a lock-step batch member has neither
  double* hPin = nullptr;
  LmSchedule lm;   // lambda, nu, the counters and every decision on them
  const YdBaSolverOptions* SO = nullptr;   // null: DENSE (ydorb_ba_solve, the lock-step batch)
  YdBaSolverInfo* info = nullptr;
  bool stopped() const { return LmSchedule::raised(P->stop); }
};

int tooWideForSolve(int n) {
  set_error("reduced camera system of %d rows is wider than the solve kernel's LDS (max %d)", n, kCholSolveMaxN);
  return YDORB_ERR_UNSUPPORTED;
}

int denseRows(int nPf) { return std::max(NB, (6 * nPf + NB - 1) / NB * NB); }

// The solver of a problem with nPf free poses, host only.  For SKYLINE, and whenever `info` is asked for, `pairs` is built by
// makePairs() and the envelope planned (with the column lists when `columns`).  Nothing here touches a device: a refusal comes before the
// stage's arenas are sized and before any of its kernels.
template <class MakePairs>
int chooseSolver(const YdBaSolverOptions* opt, int world, int nPf, MakePairs makePairs, bool columns, bapairs::PairList& pairs, sky::Plan& plan,
                 bool& sky, YdBaSolverInfo* info) {
  const YdBaSolverOptions O = opt ? *opt : YdBaSolverOptions{YDORB_BA_SOLVER_DENSE, YDORB_ESS_ORDER_SMALLER, 0};
  if (O.solver < YDORB_BA_SOLVER_AUTO || O.solver > YDORB_BA_SOLVER_SKYLINE) { set_error("BA: unknown solver"); return YDORB_ERR_INVALID_ARG; }
  if (O.ordering < YDORB_ESS_ORDER_SMALLER || O.ordering > YDORB_ESS_ORDER_RCM) { set_error("BA: unknown ordering"); return YDORB_ERR_INVALID_ARG; }
  if (O.max_factor_bytes < 0) { set_error("BA: negative max_factor_bytes"); return YDORB_ERR_INVALID_ARG; }
  if (O.solver == YDORB_BA_SOLVER_SKYLINE && world > 1) {
    set_error("BA: the skyline solver runs on one rank (the all-reduce of S is dense only)");
    return YDORB_ERR_UNSUPPORTED;
  }
  const bool over = 6 * (long long)nPf > kCholSolveMaxN;
  sky = O.solver == YDORB_BA_SOLVER_SKYLINE || (O.solver == YDORB_BA_SOLVER_AUTO && over && world <= 1);
  if (!sky && over) return tooWideForSolve(denseRows(nPf));
  if (info) memset(info, 0, sizeof(*info));
  if (sky || info) {
    pairs = makePairs();
    std::string err;
    if (pairs.buckets() > bapairs::kMaxBuckets) { set_error("BA: %lld pose-pair buckets, at most %lld", (long long)pairs.buckets(), (long long)bapairs::kMaxBuckets); return YDORB_ERR_UNSUPPORTED; }
    if (!bapairs::planEnvelope(pairs, O.ordering, O.max_factor_bytes, sky && columns, plan, err) && sky) {
      set_error("%s", err.c_str());
      return YDORB_ERR_UNSUPPORTED;
    }
  }
  if (info) {
    info->solver_used = sky ? YDORB_BA_SOLVER_SKYLINE : YDORB_BA_SOLVER_DENSE;
    info->ordering_used = plan.orderingUsed; info->n_free = nPf; info->max_row_blocks = plan.maxRowBlocks; info->dense_max_rows = kCholSolveMaxN;
    info->covisible_pairs = pairs.covisiblePairs; info->envelope_blocks = plan.envBlocks; info->envelope_blocks_natural = plan.envNatural;
    info->envelope_blocks_rcm = plan.envRcm; info->pair_updates = plan.pairUpdates;
    info->factor_bytes = sky ? plan.envBlocks * bapairs::kBlockBytes : (int64_t)denseRows(nPf) * denseRows(nPf) * 8;
  }
  return YDORB_OK;
}

int allreduce(Run& R_, void* d_buf, int64_t count, int op) {
  const YdBaOptions* O = R_.O;
  if (!O->allreduce || O->world <= 1) return YDORB_OK;
  if (count > O->comm_doubles || !O->d_comm_buf) { set_error("BA comm buffer too small (%lld doubles needed)", (long long)count); return YDORB_ERR_CAPACITY; }
  HIPCHK(hipMemcpyAsync(O->d_comm_buf, d_buf, sizeof(double) * count, hipMemcpyDeviceToDevice, R_.c->stream));
  HIPCHK(hipStreamSynchronize(R_.c->stream));
  if (O->allreduce(O->allreduce_user, O->d_comm_buf, count, op) != 0) { set_error("BA all-reduce callback failed"); return YDORB_ERR_HIP; }
  HIPCHK(hipMemcpyAsync(d_buf, O->d_comm_buf, sizeof(double) * count, hipMemcpyDeviceToDevice, R_.c->stream));
  return YDORB_OK;
}

// YDORB_BA_TRACE=1: host wall-clock marks of the solve on stderr (where the time between device phases goes)
static bool g_trace = getenv("YDORB_BA_TRACE") != nullptr && getenv("YDORB_BA_TRACE")[0] == '1';
static std::chrono::steady_clock::time_point g_t0;
static void trace(const char* what) {
  if (!g_trace) return;
  fprintf(stderr, "[ba %8.3f ms] %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_t0).count(), what);
}

struct PhaseTimer {
  Run& r; int ph; hipEvent_t a, b; bool on;
  PhaseTimer(Run& r_, int ph_) : r(r_), ph(ph_), a(r_.ev[2 * ph_]), b(r_.ev[2 * ph_ + 1]), on(r_.phaseTimes) {
    if (!on) return;   // YDORB_BA_PHASE_TIMES not asked for: no events on the stream
    collect(r_, ph_);  // an earlier recording of this phase's events must be read before they are re-recorded
    (void)hipEventRecord(a, r.c->stream);
  }
  void stop() { if (on) { (void)hipEventRecord(b, r.c->stream); on = false; r.pending[ph] = true; } }
  static void collect(Run& r_, int ph_) {
    if (!r_.pending[ph_]) return;
    float ms = 0;
    if (hipEventSynchronize(r_.ev[2 * ph_ + 1]) == hipSuccess && hipEventElapsedTime(&ms, r_.ev[2 * ph_], r_.ev[2 * ph_ + 1]) == hipSuccess)
      r_.phaseMs[ph_] += ms;
    r_.pending[ph_] = false;
  }
};

// initializeOptimization(0) for one optimize() call: host ordering of the level-0 edges, uploads, pose-pair buckets (stage 1), or the
// refreshed information / robust flags on stage 1's structures (stage 2); leaves S cleared and both estimate buffers in agreement.
// R_.sys.Ea == 0 afterwards means there is nothing to optimise.
int prepareStage(Run& R_, bool reuse) {
  SolveMem& c = *R_.c;
  const YdBaProblem& P = *R_.P;
  const YdBaOptions& O = *R_.O;
  hipStream_t s = c.stream;
  const int K = P.n_poses, NP = P.n_points, E = P.n_edges;
  trace("optimize: begin");
  Sys& Y = R_.sys;
  // Stage 2 (after the chi2 cull) re-uses stage 1's device structures: a culled edge keeps its slot with information 0, which
  // every kernel treats as "skip" — no second host ordering, upload or pair-bucket build.  Landmarks / poses that lose all their
  // edges stay in the system with H = lambda*I, b = 0, i.e. dx = 0: the same estimate g2o keeps by leaving them out.
  auto prepare = [&]() -> int {
    std::vector<int> act;
    for (int e = 0; e < E; e++) act.push_back(e);   // every edge starts at level 0 (optimizer.cpp:239-280)
    if (act.empty()) { Y.Ea = 0; return YDORB_OK; }
    // index mapping (buildIndexMapping, sparse_optimizer.cpp:168-192): free poses first, then landmarks, active ones only
    std::vector<int> poseIdx(K, -1), ptIdx(NP, -1), poseOf, ptOf;
    {
      std::vector<uint8_t> pu(K, 0), qu(NP, 0);
      for (int e : act) { pu[P.edge_pose[e]] = 1; qu[P.edge_point[e]] = 1; }
      for (int k = 0; k < K; k++) if (pu[k] && !P.pose_fixed[k]) { poseIdx[k] = (int)poseOf.size(); poseOf.push_back(k); }
      for (int p = 0; p < NP; p++) if (qu[p]) { ptIdx[p] = (int)ptOf.size(); ptOf.push_back(p); }
    }
    const int nL = (int)ptOf.size(), Ea = (int)act.size();
    if (O.world > 1) {
      // every rank must factorise the same reduced system: the free-pose set comes from the caller's fixed mask only
      poseOf.clear();
      for (int k = 0; k < K; k++) { poseIdx[k] = -1; if (!P.pose_fixed[k]) { poseIdx[k] = (int)poseOf.size(); poseOf.push_back(k); } }
    }
    const int nPf = (int)poseOf.size();
    {  // order by (landmark index, free-pose index, caller's pose index): counting sort by landmark, then a tiny insertion sort per
       // landmark.  The fixed poses all have free-pose index -1, so the caller's index orders them: the device order, and with it every
       // summation order, depends on the SET of edges and not on the order the caller lists them in.
      std::vector<int> start(nL + 1, 0), sorted(Ea);
      for (int e : act) start[ptIdx[P.edge_point[e]] + 1]++;
      for (int l = 0; l < nL; l++) start[l + 1] += start[l];
      std::vector<int> fill(start.begin(), start.end() - 1);
      for (int e : act) sorted[fill[ptIdx[P.edge_point[e]]]++] = e;
      auto after = [&](int x, int y) {   // edge x belongs behind edge y of the same landmark
        const int px = poseIdx[P.edge_pose[x]], py = poseIdx[P.edge_pose[y]];
        return px != py ? px > py : P.edge_pose[x] > P.edge_pose[y];
      };
      for (int l = 0; l < nL; l++)
        for (int a = start[l] + 1; a < start[l + 1]; a++) {
          const int e = sorted[a];
          int b = a - 1;
          while (b >= start[l] && after(sorted[b], e)) { sorted[b + 1] = sorted[b]; b--; }
          sorted[b + 1] = e;
          // One edge per (pose, landmark), fixed poses included (c_api.h, YdBaProblem): e now follows the edge it does not sort behind, and
          // that one is of the same pose exactly when the pair repeats.  k_pair_sort ranks the items of a pose-pair bucket by their first
          // edge; two items with one key would share a slot of its output and leave another slot unwritten.
          if (b >= start[l] && P.edge_pose[sorted[b]] == P.edge_pose[e]) {
            set_error("edges %d and %d are both the observation of point %d by pose %d", sorted[b], e, P.edge_point[e], P.edge_pose[e]);
            return YDORB_ERR_INVALID_ARG;
          }
        }
      act.swap(sorted);
    }
    std::vector<int> hPose(Ea), hPidx(Ea), hPt(Ea), hLm(Ea), hPtStart(nL + 1, 0), hPoseStart(nPf + 1, 0), hPoseEdges;
    std::vector<double> hMeas((size_t)3 * Ea), hInfo(Ea);
    std::vector<uint8_t> hRobust(Ea);
    for (int i = 0; i < Ea; i++) {
      const int e = act[i];
      hPose[i] = P.edge_pose[e]; hPidx[i] = poseIdx[P.edge_pose[e]]; hPt[i] = P.edge_point[e]; hLm[i] = ptIdx[P.edge_point[e]];
      for (int d = 0; d < 3; d++) hMeas[3 * i + d] = P.edge_meas[3 * e + d];
      hInfo[i] = P.edge_inv_sigma2[e];
      hRobust[i] = R_.noRobust ? 0 : 1;
      hPtStart[hLm[i] + 1]++;
      if (hPidx[i] >= 0) hPoseStart[hPidx[i] + 1]++;
    }
    for (int l = 0; l < nL; l++) hPtStart[l + 1] += hPtStart[l];
    for (int i = 0; i < nPf; i++) hPoseStart[i + 1] += hPoseStart[i];
    hPoseEdges.resize(hPoseStart[nPf]);
    {
      std::vector<int> fill(hPoseStart.begin(), hPoseStart.end() - 1);
      for (int i = 0; i < Ea; i++) if (hPidx[i] >= 0) hPoseEdges[fill[hPidx[i]]++] = i;
    }
    Sys Z;
    Z.nL = nL; Z.nPf = nPf; Z.Ea = Ea; Z.nPoseEdges = (int)hPoseEdges.size();
    Z.n = std::max(NB, (6 * nPf + NB - 1) / NB * NB); Z.nb = Z.n / NB;
    Z.nBlkE = (Ea + 255) / 256;
    Z.nBuckets = (int)std::min<long long>((long long)nPf * (nPf + 1) / 2, std::numeric_limits<int>::max());   // pose-pair buckets of the Schur complement (structure is fixed for this optimize() call); SKYLINE sets its own below
    for (int l = 0; l < nL; l++) {
      size_t m = 0;
      for (int i = hPtStart[l]; i < hPtStart[l + 1]; i++) m += hPidx[i] >= 0;
      Z.nItems += m * (m + 1) / 2;
    }
    bapairs::PairList pairs;
    std::vector<int64_t> pairDst;
    {
      int rc = chooseSolver(R_.SO, O.world, nPf, [&] { return bapairs::buildPairs(nPf, nL, hPtStart.data(), hPidx.data()); }, true, pairs, Z.plan, Z.sky, R_.info);
      if (rc) return rc;
      if (Z.sky) {   // nothing on this path is sized by nPf^2
        Z.n = 6 * nPf; Z.nb = 0; Z.nBuckets = (int)pairs.buckets();
        pairDst = bapairs::bucketDestinations(pairs, Z.plan);
      }
    }
    trace("optimize: host ordering done");
    // the two arenas of the stage: sized, grown if need be (at most two hipMalloc where every array had its own), then laid out
    const size_t upBytes = layUp(Z, nullptr, c.u);
    int rc;
    if ((rc = c.stage(upBytes)) || (rc = c.up.ensure(upBytes)) || (rc = c.work.ensure(layWork(Z, nullptr, c.w)))) return rc;
    layUp(Z, c.up.p, c.u);
    layWork(Z, c.work.p, c.w);
    const UpPtrs& u = c.u;
    const WorkPtrs& w = c.w;
    {  // through the context's pinned staging area (true asynchronous copies at PCIe rate; the area is free again at the sync below)
      auto up = [&](const void* dst, const void* src, size_t bytes) {   // into the staging area at the array's offset in the arena
        if (bytes) memcpy(c.hStage.as<uint8_t>() + (static_cast<const uint8_t*>(dst) - c.up.as<uint8_t>()), src, bytes);
      };
      auto upv = [&](const auto* dst, const auto& vec) { up(dst, vec.data(), sizeof(vec[0]) * vec.size()); };
      upv(u.ePose, hPose); upv(u.ePidx, hPidx); upv(u.ePt, hPt); upv(u.eLm, hLm); upv(u.eMeas, hMeas); upv(u.eInfo, hInfo);
      upv(u.eRobust, hRobust); upv(u.ptStart, hPtStart); upv(u.poseStart, hPoseStart); upv(u.ptOf, ptOf);
      upv(u.poseEdges, hPoseEdges); upv(u.poseOf, poseOf);
      if (Z.sky) {
        upv(u.k.pairRow, pairs.rowStart); upv(u.k.pairI1, pairs.i1); upv(u.k.pairI2, pairs.i2); upv(u.k.pairDst, pairDst);
        u.k.fill(Z.plan, up);
      }
      HIPCHK(hipMemcpyAsync(c.up.p, c.hStage.p, upBytes, hipMemcpyHostToDevice, s));
      // the original information: the chi2 tests between and after the stages use it (k_cull)
      HIPCHK(hipMemcpyAsync(w.eInfo0, u.eInfo, sizeof(double) * Ea, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemsetAsync(w.err, 0, sizeof(double) * 3 * Ea, s));   // an edge that is never evaluated (stop flag) has error 0
    }
    trace("optimize: uploads enqueued");
    if (Z.nBuckets > 0) {
      const int nBuckets = Z.nBuckets;
      EdgeSoA Ed{u.ePose, u.ePidx, u.ePt, u.eMeas, u.eInfo, u.eRobust, Ea};
      HIPCHK(hipMemsetAsync(w.pairCnt, 0, sizeof(int) * (nBuckets + 1), s));
      if (Z.sky) hipLaunchKernelGGL(k_sky_pair_count, dim3((nL + 255) / 256), dim3(256), 0, s, Ed, u.ptStart, nL, u.k.pairRow, u.k.pairI1, w.pairCnt);
      else hipLaunchKernelGGL(k_pair_count, dim3((nL + 255) / 256), dim3(256), 0, s, Ed, u.ptStart, nL, w.pairCnt);
      hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(256), 0, s, w.pairCnt, nBuckets, w.pairStart);
      HIPCHK(hipMemcpyAsync(w.pairCursor, w.pairStart, sizeof(int) * (nBuckets + 1), hipMemcpyDeviceToDevice, s));
      if (Z.sky) hipLaunchKernelGGL(k_sky_pair_fill, dim3((nL + 255) / 256), dim3(256), 0, s, Ed, u.ptStart, nL, u.k.pairRow, u.k.pairI1, w.pairCursor, w.pairA);
      else hipLaunchKernelGGL(k_pair_fill, dim3((nL + 255) / 256), dim3(256), 0, s, Ed, u.ptStart, nL, w.pairCursor, w.pairA);
      hipLaunchKernelGGL(k_pair_sort, dim3((nBuckets + 3) / 4), dim3(256), 0, s, w.pairStart, nBuckets, w.pairA, w.pairB);
    }
    HIPCHK(hipStreamSynchronize(s));   // the host staging vectors above die with this scope
    Z.act.swap(act);
    Y = std::move(Z);
    return YDORB_OK;
  };
  int rc;
  if (!reuse || Y.Ea == 0) {
    if ((rc = prepare())) return rc;
  }
  // (stage 2 re-uses stage 1's device structures as they are: k_cull already zeroed the information of the culled edges and
  // cleared the robust flags on the device.  The host does not learn how many edges survived; a cull that left NONE shows at the
  // stage's first iteration as a system whose largest diagonal entry is exactly 0, see LmSchedule::setMaxDiag)
  if (Y.Ea == 0) return YDORB_OK;
  // the two estimate buffers must agree on everything the update kernel does not write (fixed poses, points without edges)
  HIPCHK(hipMemcpyAsync(c.st.poses[R_.cur ^ 1], c.st.poses[R_.cur], sizeof(double) * 7 * K, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(c.st.pts[R_.cur ^ 1], c.st.pts[R_.cur], sizeof(double) * 3 * NP, hipMemcpyDeviceToDevice, s));
  if (!Y.sky) HIPCHK(hipMemsetAsync(c.w.S, 0, sizeof(double) * ((size_t)Y.n * Y.n + Y.n + (size_t)Y.nb * NB * NB), s));   // S | bs | diagInv (see WorkPtrs)
  return YDORB_OK;
}

// The Schur complement of one LM trial, S | bs from Hpp, Hpl, Hll and lambda, and its solve into xp: the two phases that differ
// between the solvers.  optimize() and ydorb_ba_reduced_system_with queue the same launches.
int launchSchur(Run& R_, double lambda, double contrib) {
  SolveMem& c = *R_.c;
  const Sys& Y = R_.sys;
  const UpPtrs& u = c.u;
  const WorkPtrs& w = c.w;
  hipStream_t s = c.stream;
  EdgeSoA Ed{u.ePose, u.ePidx, u.ePt, u.eMeas, u.eInfo, u.eRobust, Y.Ea};
  double *dbp = w.bp(Y), *dbs = w.bs(Y);
  hipLaunchKernelGGL(k_dinv, dim3((Y.nL + 255) / 256), dim3(256), 0, s, w.Hll, w.bl, Y.nL, lambda, w.Dinv, w.db, w.status);
  hipLaunchKernelGGL(k_bd, dim3(Y.nBlkE), dim3(256), 0, s, Ed, u.eLm, w.Hpl, w.Dinv, w.BD);
  if (Y.nPf)
    hipLaunchKernelGGL(k_bs, dim3(Y.nPf), dim3(256), 0, s, Ed, u.poseStart, u.poseEdges, u.eLm, w.Hpl, w.db, dbp, contrib, dbs);
  if (!Y.sky) {
    hipLaunchKernelGGL(k_schur_pairs, dim3(Y.nBuckets + 1), dim3(64 * kSchurWaves), 0, s, w.pairStart, w.pairB, Y.nPf, Y.nBuckets, w.BD, w.Hpl, w.Hpp, lambda, contrib, Y.n, w.S, dbs);
  } else if (Y.nBuckets) {
    HIPCHK(hipMemsetAsync(w.S, 0, sizeof(double) * Y.envDoubles(), s));   // the fill: blocks of the envelope that no bucket writes
    hipLaunchKernelGGL(k_sky_schur_pairs, dim3(Y.nBuckets), dim3(64 * kSchurWaves), 0, s, w.pairStart, w.pairB, Y.nBuckets, u.k.pairI1, u.k.pairI2, u.k.pairDst, w.BD, w.Hpl, w.Hpp, lambda, w.S);
  }
  return YDORB_OK;
}
int launchSolve(Run& R_) {
  SolveMem& c = *R_.c;
  const Sys& Y = R_.sys;
  const WorkPtrs& w = c.w;
  hipStream_t s = c.stream;
  if (Y.sky) {
    const SkyPtrs& k = c.u.k;
    if (Y.nPf)
      hipLaunchKernelGGL(k_sky_solve, dim3(1), dim3(kSkyThreads), 0, s, Y.nPf, k.first, k.rowOff, k.colStart, k.colRows, k.colBlk, k.perm, w.bs(Y), w.S, w.skyW, w.xp, w.status);
    return YDORB_OK;
  }
  for (int kb = 0; kb < Y.nb; kb++)
    hipLaunchKernelGGL(k_chol_step, dim3((Y.nb - kb) * (Y.nb - kb + 1) / 2 + (kb > 0)), dim3(256), 0, s, w.S, w.diagL, w.diagInv, Y.n, kb, w.status, w.bs(Y), w.yv);
  if (!launch_chol_solve(s, w.S, w.diagInv, Y.n, w.yv, w.bs(Y), w.xp)) return tooWideForSolve(Y.n);
  return YDORB_OK;
}

// one SparseOptimizer::optimize(iterations) on the level-0 edges: the stage R_.lm is at
int optimize(Run& R_) {
  LmSchedule& lm = R_.lm;
  int rc = prepareStage(R_, lm.stage == 2);
  if (rc) return rc;
  SolveMem& c = *R_.c;
  const YdBaOptions& O = *R_.O;
  hipStream_t s = c.stream;
  const Sys& Y = R_.sys;
  if (Y.Ea == 0) return YDORB_OK;
  const int nL = Y.nL, nPf = Y.nPf, Ea = Y.Ea, n = Y.n, nBlkE = Y.nBlkE;
  const UpPtrs& u = c.u;
  const WorkPtrs& w = c.w;
  double* const* poses = c.st.poses;
  double* const* pts = c.st.pts;
  double *dHpp = w.Hpp, *dbp = w.bp(Y), *dS = w.S;
  EdgeSoA Ed{u.ePose, u.ePidx, u.ePt, u.eMeas, u.eInfo, u.eRobust, Ea};
  const double dM = O.delta_mono, dSt = O.delta_stereo;
  double* hscal = R_.hPin;
  const bool multi = O.world > 1 && O.allreduce;

  auto computeChi2 = [&](int buf, bool withStatus) -> int {   // into hscal[0]
    PhaseTimer t(R_, PH_ERR);
    hipLaunchKernelGGL(k_errors, dim3(nBlkE), dim3(256), 0, s, Ed, poses[buf], pts[buf], R_.cam, dM, dSt, w.err, w.partial);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, s, w.partial, nBlkE, w.scal, 0, withStatus ? w.status : nullptr);
    t.stop();
    if (multi) { int r2 = allreduce(R_, w.scal, 1, 0); if (r2) return r2; }
    HIPCHK(hipMemcpyAsync(hscal, w.scal, sizeof(double) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return YDORB_OK;
  };

  trace("optimize: pair buckets enqueued");
  const double& lambda = lm.lambda;
  for (bool more = lm.firstIteration(R_.P->stop); more;) {
    if (lm.needChi2()) {
      if ((rc = computeChi2(R_.cur, false))) return rc;
      lm.setChi2(hscal[0]);
    }
    {  // buildSystem
      PhaseTimer t(R_, PH_BUILD);
      hipLaunchKernelGGL(k_build_points, dim3((nL + 127) / 128), dim3(128), 0, s, Ed, u.ptStart, nL, poses[R_.cur], pts[R_.cur], R_.cam, dM, dSt, w.err, w.Hll, w.bl, w.Hpl);
      if (nPf)
        hipLaunchKernelGGL(k_build_poses, dim3(nPf), dim3(256), 0, s, Ed, u.poseStart, u.poseEdges, poses[R_.cur], pts[R_.cur], R_.cam, dM, dSt, w.err, dHpp, dbp);
      t.stop();
      if (multi && nPf) { if ((rc = allreduce(R_, dHpp, (int64_t)42 * nPf, 0))) return rc; }
    }
    if (lm.needLambdaInit()) {
      hipLaunchKernelGGL(k_max_diag, dim3(1), dim3(256), 0, s, dHpp, nPf, w.Hll, nL, w.scal, 1);
      if (multi) { if ((rc = allreduce(R_, w.scal + 1, 1, 1))) return rc; }
      HIPCHK(hipMemcpyAsync(hscal, w.scal, sizeof(double) * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (!lm.setMaxDiag(hscal[1])) break;
    }
    LmSchedule::Next next;
    do {
      const int nxt = R_.cur ^ 1;
      {
        PhaseTimer t(R_, PH_SCHUR);
        const double contrib = (!multi || O.rank == 0) ? 1.0 : 0.0;
        if ((rc = launchSchur(R_, lambda, contrib))) return rc;
        t.stop();
      }
      if (multi) {  // sum of the per-rank landmark contributions (+ rank 0's Hpp, lambda, bp)
        if ((rc = allreduce(R_, dS, (int64_t)n * n + n, 0))) return rc;
      }
      {
        PhaseTimer t(R_, PH_SOLVE);
        if ((rc = launchSolve(R_))) return rc;
        hipLaunchKernelGGL(k_backsub, dim3((nL + 127) / 128), dim3(128), 0, s, Ed, u.ptStart, nL, w.Hpl, w.Dinv, w.bl, w.xp, w.xl);
        t.stop();
        HIPCHK(hipGetLastError());
      }
      {
        PhaseTimer t(R_, PH_UPDATE);
        hipLaunchKernelGGL(k_update, dim3((std::max(nPf, nL) + 255) / 256), dim3(256), 0, s, poses[R_.cur], pts[R_.cur], poses[nxt], pts[nxt], u.poseOf, nPf, u.ptOf, nL, w.xp, w.xl);
        // computeScale: pose part once (rank 0), landmark part per rank
        {
          const int np6 = (!multi || O.rank == 0) ? 6 * nPf : 0;
          const int nb2 = (np6 + 3 * nL + 255) / 256;
          hipLaunchKernelGGL(k_scale, dim3(nb2), dim3(256), 0, s, w.xp, dbp, np6, w.xl, w.bl, 3 * nL, lambda, w.partial + nBlkE);
          hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, s, w.partial + nBlkE, nb2, w.scal, 2, nullptr);
        }
        t.stop();
        if (multi) { if ((rc = allreduce(R_, w.scal + 2, 1, 0))) return rc; }
      }
      if ((rc = computeChi2(nxt, true))) return rc;  // also brings back scal[2], the factorisation status, and leaves err = errors of the trial state
      next = lm.trial(hscal[0], hscal[2], (int)hscal[6] == 0, R_.P->stop);
      if (lm.lastAccepted) R_.cur = nxt;
    } while (next == LmSchedule::Retry);
    more = next == LmSchedule::NextIteration;
  }
  trace("optimize: LM loop done");
  for (int ph = 0; ph < PH_COUNT; ph++) PhaseTimer::collect(R_, ph);
  trace("optimize: errors read back");
  return YDORB_OK;
}

// validation shared by the single and the batched entry points; fills *Oout with the effective options
int checkProblem(const YdBaProblem* P, const YdBaOptions* optIn, YdBaResult* res, YdBaOptions* Oout) {
  if (!P || !res) { set_error("null argument"); return YDORB_ERR_INVALID_ARG; }
  YdBaOptions O;
  if (optIn) O = *optIn; else ydorb_ba_default_options(&O);
  uint8_t* outlier = res->edge_outlier;
  memset(res, 0, sizeof(*res));
  res->edge_outlier = outlier;
  const int K = P->n_poses, NP = P->n_points, E = P->n_edges;
  if (K < 0 || NP < 0 || E < 0 || (K && (!P->poses || !P->pose_fixed)) || (NP && !P->points) ||
      (E && (!P->edge_pose || !P->edge_point || !P->edge_meas || !P->edge_inv_sigma2)) || O.device < 0 || O.device >= 16 || O.max_trials < 1) {
    set_error("invalid BA problem");
    return YDORB_ERR_INVALID_ARG;
  }
  for (int e = 0; e < E; e++)
    if (P->edge_pose[e] < 0 || P->edge_pose[e] >= K || P->edge_point[e] < 0 || P->edge_point[e] >= NP) {
      set_error("edge %d references a vertex out of range", e);
      return YDORB_ERR_INVALID_ARG;
    }
  if (outlier) memset(outlier, 0, E);
  *Oout = O;
  return YDORB_OK;
}

// state upload at the start of a solve (the vertices g2o is handed at optimizer.cpp:185-230)
int beginSolve(Run& R_) {
  SolveMem& c = *R_.c;
  const YdBaProblem* P = R_.P;
  const YdBaOptions& O = *R_.O;
  const int K = P->n_poses, NP = P->n_points;
  int rc;
  R_.noRobust = (O.flags & YDORB_BA_NO_ROBUST) != 0;
  R_.phaseTimes = (O.flags & YDORB_BA_PHASE_TIMES) != 0;
  R_.cam = Cam{P->fx, P->fy, P->cx, P->cy, P->bf};
  R_.lm.begin(O, R_.res);
  if ((rc = c.state.ensure(layState(K, NP, nullptr, c.st)))) return rc;
  layState(K, NP, c.state.p, c.st);
  {  // SE3Quat's 7-vector constructor normalises the rotation (se3quat.h:80-86)
    std::vector<double> hp(P->poses, P->poses + (size_t)7 * K);
    for (int k = 0; k < K; k++) {
      double* q = &hp[7 * k + 3];
      if (q[3] < 0) for (int d = 0; d < 4; d++) q[d] = -q[d];
      const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int d = 0; d < 4; d++) q[d] /= nrm;
    }
    HIPCHK(hipMemcpyAsync(c.st.poses[0], hp.data(), sizeof(double) * 7 * K, hipMemcpyHostToDevice, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));   // hp dies here
  }
  HIPCHK(hipMemcpyAsync(c.st.pts[0], P->points, sizeof(double) * 3 * NP, hipMemcpyHostToDevice, c.stream));
  return YDORB_OK;
}

// final == 0, optimizer.cpp:290-311: edges whose chi2 exceeds the threshold or whose depth is not positive leave the second stage
int launchCull(Run& R_, int final) {
  SolveMem& c = *R_.c;
  const YdBaOptions& O = *R_.O;
  const int Ea = R_.sys.Ea;
  if (Ea == 0) return YDORB_OK;
  hipLaunchKernelGGL(k_cull, dim3((Ea + 255) / 256), dim3(256), 0, c.stream, c.u.ePose, c.u.ePt, c.u.eMeas, Ea, c.w.eInfo0, c.w.err,
                     c.st.poses[R_.cur], c.st.pts[R_.cur], O.chi2_mono, O.chi2_stereo, final, c.u.eInfo, c.u.eRobust, c.w.eOutlier);
  HIPCHK(hipGetLastError());
  return YDORB_OK;
}

// optimizer.cpp:315-351 up to the write-back: the final outlier list and the estimates
int endSolve(Run& R_) {
  SolveMem& c = *R_.c;
  const YdBaProblem* P = R_.P;
  const Sys& Y = R_.sys;
  int rc = launchCull(R_, 1);
  if (rc) return rc;
  uint8_t* outlier = R_.res->edge_outlier;
  // down through the pinned staging area, then into the caller's (pageable) arrays
  const size_t bPoses = sizeof(double) * 7 * P->n_poses, bPts = sizeof(double) * 3 * P->n_points, oPts = (bPoses + 255) & ~(size_t)255,
               oOut = oPts + ((bPts + 255) & ~(size_t)255);
  if ((rc = c.stage(oOut + Y.Ea))) return rc;
  if (outlier && Y.Ea) HIPCHK(hipMemcpyAsync(c.hStage.as<uint8_t>() + oOut, c.w.eOutlier, Y.Ea, hipMemcpyDeviceToHost, c.stream));
  HIPCHK(hipMemcpyAsync(c.hStage.as<uint8_t>(), c.st.poses[R_.cur], bPoses, hipMemcpyDeviceToHost, c.stream));
  HIPCHK(hipMemcpyAsync(c.hStage.as<uint8_t>() + oPts, c.st.pts[R_.cur], bPts, hipMemcpyDeviceToHost, c.stream));
  HIPCHK(hipStreamSynchronize(c.stream));
  memcpy(P->poses, c.hStage.as<uint8_t>(), bPoses);
  memcpy(P->points, c.hStage.as<uint8_t>() + oPts, bPts);
  if (outlier) for (int i = 0; i < Y.Ea; i++) outlier[Y.act[i]] = c.hStage.as<uint8_t>()[oOut + i];   // device edges are in (landmark, pose) order
  if (R_.stopped()) R_.res->stopped = 1;
  return YDORB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// ydorb_ba_solve_batch: independent problems advance in LOCK STEP through one set of launches per phase (blockIdx.z = problem,
// ba_kernels.hip.h "Lock-step batch").  The host keeps one LmSchedule per problem - the one optimize() above steps -
// and every round (a) builds the system of the problems that start an iteration, (b) runs one LM trial of every unfinished
// problem, (c) reads all problems' three scalars back with ONE copy and decides accept / retry / terminate per problem.  A problem
// that is done with a stage goes through the same cull / second stage / read-back steps as a single solve while the others go on.
// ---------------------------------------------------------------------------------------------------------------------------
struct Job {
  SolveMem mem;            // its own arenas; mem.stream is a set-up stream or the batch's (not owned)
  BaDev dev{};             // its record of the stage at hand (offsets, sizes); both upload images of a round start from it
  YdBaOptions O;
  std::optional<Run> run;  // of the call at hand; none for a member that was invalid, empty or stopped on arrival
  bool needBuild = false;  // at the start of an iteration: phase (a) of the next round is for it
  bool done = false;
  bool pendingEnd = false;   // finished its LM schedule: final cull + read-back still to do (all of a group together, on the set-up threads)
  int rc = YDORB_OK;
  std::string errText;
};
// A pinned area that an enqueued copy reads is not written again until the stream has been waited on past that copy.
struct BatchPool {   // per device: contexts, stream and staging of the lock-step batches (one batch at a time per device)
  std::mutex mu;
  hipStream_t stream = nullptr;
  std::vector<Job*> jobs;          // grown on demand; buffers are kept between calls
  std::vector<hipStream_t> setupStreams;
  Mem dDev, dScal;                 // BaDev[B]; per problem 8 doubles (chi2, max diag, scale sum, ..., status copies) + 2 ints of status
  PinnedMem hDev, hScal;           // two images of BaDev[B], the one phase (a) of a round uploads and the one phase (b) uploads: (a) does not
                                   // always wait before the host goes on to (b); the read-back of dScal's doubles
};
BatchPool g_batch[16];
constexpr int kSetupThreads = 16;  // host threads of a batch's set-up phase
constexpr int kBatchGroup = 64;    // problems per lock-step group (C5-sized problems take ~40 MB each)

// YDORB_BA_TEST_LATE_UPLOADS: enqueued in front of a BaDev upload, so that the copy reads its pinned source 200 us after the host went on
void lateUpload(void*) { std::this_thread::sleep_for(std::chrono::microseconds(200)); }

void fillDev(Job& J, BaDev& D, const BaDev* dDevBase, double* dScal, int* dStatus) {
  const UpPtrs& u = J.mem.u;
  const WorkPtrs& w = J.mem.w;
  const StatePtrs& st = J.mem.st;
  const Sys& Y = J.run->sys;
  memset(&D, 0, sizeof(D));
  auto off = [&](const void* p) { return (long long)(reinterpret_cast<const char*>(p) - reinterpret_cast<const char*>(dDevBase)); };   // see BaDev
  D.ePose = off(u.ePose); D.ePidx = off(u.ePidx); D.ePt = off(u.ePt); D.eMeas = off(u.eMeas); D.eInfo = off(u.eInfo); D.eRobust = off(u.eRobust);
  D.ptStart = off(u.ptStart); D.poseStart = off(u.poseStart); D.poseEdges = off(u.poseEdges); D.eLm = off(u.eLm);
  D.poseOf = off(u.poseOf); D.ptOf = off(u.ptOf); D.pairStart = off(w.pairStart); D.pairItems = off(w.pairB);
  for (int i = 0; i < 2; i++) { D.poses[i] = off(st.poses[i]); D.pts[i] = off(st.pts[i]); }
  D.err = off(w.err); D.partial = off(w.partial); D.Hll = off(w.Hll); D.bl = off(w.bl); D.Hpl = off(w.Hpl);
  D.BD = off(w.BD); D.Hpp = off(w.Hpp); D.S = off(w.S); D.diagL = off(w.diagL); D.diagInv = off(w.diagInv);
  D.Dinv = off(w.Dinv); D.db = off(w.db); D.xp = off(w.xp); D.yv = off(w.yv); D.xl = off(w.xl);
  D.scal = off(dScal); D.status = off(dStatus);
  D.cam = J.run->cam; D.dM = J.O.delta_mono; D.dSt = J.O.delta_stereo;
  D.nL = Y.nL; D.nPf = Y.nPf; D.Ea = Y.Ea; D.n = Y.n; D.nb = Y.nb; D.nBlkE = Y.nBlkE; D.nBuckets = Y.nBuckets;
}

int solveGroup(BatchPool& B, const YdBaProblem* probs, const YdBaOptions& Oin, YdBaResult* res, int n, int* rcEach) {
  hipStream_t s = B.stream;
  const bool lateUploads = (Oin.flags & YDORB_BA_TEST_LATE_UPLOADS) != 0;
  int rc;
  if ((rc = B.dDev.ensure(sizeof(BaDev) * n)) || (rc = B.dScal.ensure((sizeof(double) * 8 + sizeof(int) * 2) * n))) return rc;
  BaDev* hDevA = B.hDev.as<BaDev>();   // phase (a)'s image: next written in the following round, after the wait that ends phase (b)
  BaDev* hDevB = hDevA + n;            // phase (b)'s image: uploaded and waited on within phase (b)
  double* hScal = B.hScal.as<double>();
  double* dScalAll = B.dScal.as<double>();
  int* dStatusAll = reinterpret_cast<int*>(dScalAll + (size_t)8 * n);
  std::vector<Job*> J(B.jobs.begin(), B.jobs.begin() + n);
  auto fail = [&](int j, int code) { J[j]->rc = code; J[j]->done = true; if (rcEach) rcEach[j] = code; };

  // Stage transitions (per problem, on its stream).  over == false: the member enters the stage its schedule is at; true: that stage is
  // over and the schedule says what follows.  Finished members wait for the final cull, read-back and outlier scatter (~0.1 ms each,
  // mostly host) until the rounds have ended, see below.
  auto nextStage = [&](int j, bool over) {
    Job& X = *J[j];
    Run& R_ = *X.run;
    X.needBuild = false;
    for (int r;; over = true) {
      if (over) {
        if (!R_.lm.handOver(R_.P->stop)) { X.pendingEnd = X.done = true; return; }
        if ((r = launchCull(R_, 0))) { fail(j, r); return; }
      }
      if ((r = prepareStage(R_, R_.lm.stage == 2))) { fail(j, r); return; }
      if (R_.sys.Ea == 0) continue;
      if (R_.sys.n > kCholSolveMaxN) { fail(j, tooWideForSolve(R_.sys.n)); return; }
      fillDev(X, X.dev, B.dDev.as<BaDev>(), dScalAll + (size_t)8 * j, dStatusAll + (size_t)2 * j);
      if (R_.lm.firstIteration(R_.P->stop)) { X.needBuild = true; return; }
    }
  };
  // fn(j, stream) for every member, spread over a few host threads, each with a set-up stream of its own; then the error text of a
  // member that failed becomes the calling thread's
  auto spread = [&](auto fn) {
    const int nt = std::max(1, std::min(n, kSetupThreads));
    std::atomic<int> next{0};
    auto worker = [&](int t) {
      (void)hipSetDevice(Oin.device);
      for (int j = next.fetch_add(1); j < n; j = next.fetch_add(1)) fn(j, B.setupStreams[t]);
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(worker, t);
    worker(0);
    for (std::thread& th : pool) th.join();
    for (int j = 0; j < n; j++) if (J[j]->rc != YDORB_OK && !J[j]->errText.empty()) set_error("%s", J[j]->errText.c_str());
  };

  // Set-up of every problem (validation, edge ordering, uploads, pose-pair buckets): ~2 ms of host work and pageable copies per C5-sized
  // problem, independent of the others, so it is spread over a few host threads, each on its own set-up stream; the lock-step
  // rounds below then run on the batch's one stream.
  while ((int)B.setupStreams.size() < std::min(n, kSetupThreads)) {
    hipStream_t st = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    B.setupStreams.push_back(st);
  }
  spread([&](int j, hipStream_t st) {
    Job& X = *J[j];
    X.done = false; X.pendingEnd = false; X.rc = YDORB_OK; X.errText.clear();
    X.run.reset();
    if (rcEach) rcEach[j] = YDORB_OK;
    int r = checkProblem(&probs[j], &Oin, &res[j], &X.O);
    const YdBaProblem* P = &probs[j];
    if (!r) {
      if (P->stop && *P->stop) { res[j].stopped = 1; X.done = true; return; }
      if (P->n_edges == 0 || P->n_poses == 0 || P->n_points == 0) { X.done = true; return; }
      X.mem.device = Oin.device; X.mem.stream = st;
      X.run.emplace(Run{&X.mem, P, &X.O, &res[j]});
      r = beginSolve(*X.run);
    }
    if (!r) {
      nextStage(j, false);
      r = X.rc;
    }
    if (r) { X.errText = ydorb_last_error(); fail(j, r); }
    if (hipStreamSynchronize(st) != hipSuccess && !r) { X.errText = "hipStreamSynchronize failed"; fail(j, YDORB_ERR_HIP); }
    X.mem.stream = s;
  });
  trace("batch: set-up done");

  auto maxOver = [&](auto fn) { int m = 0; for (int j = 0; j < n; j++) if (!J[j]->done) m = std::max(m, fn(J[j]->run->sys)); return m; };
  auto rounds = [&]() -> int {
    while (true) {
      bool any = false;
      for (int j = 0; j < n; j++) any = any || !J[j]->done;
      if (!any) break;
      trace("batch: round begins");
      // (a) iteration starts: chi2 of the current estimate where needed, H and b, initial lambda -----------------------------------
      bool anyBuild = false, anyChi = false, anyDiag = false;
      for (int j = 0; j < n; j++) {
        Job& X = *J[j];
        BaDev& D = hDevA[j];
        D = X.dev;
        D.trial = 0;
        D.build = !X.done && X.needBuild;
        D.chi2 = D.build && X.run->lm.needChi2();
        D.maxdiag = D.build && X.run->lm.needLambdaInit();
        D.cur = X.done ? 0 : X.run->cur;
        D.lambda = X.run ? X.run->lm.lambda : 0;
        anyBuild = anyBuild || D.build; anyChi = anyChi || D.chi2; anyDiag = anyDiag || D.maxdiag;
      }
      const int gE = maxOver([](const Sys& Y) { return Y.nBlkE; }), gL128 = maxOver([](const Sys& Y) { return (Y.nL + 127) / 128; }),
                gL256 = maxOver([](const Sys& Y) { return (Y.nL + 255) / 256; }), gP = maxOver([](const Sys& Y) { return Y.nPf; }),
                gBk = maxOver([](const Sys& Y) { return Y.nBuckets + 1; }), gNb = maxOver([](const Sys& Y) { return Y.nb; }),
                gUpd = maxOver([](const Sys& Y) { return (std::max(Y.nPf, Y.nL) + 255) / 256; }),
                gScale = maxOver([](const Sys& Y) { return (6 * Y.nPf + 3 * Y.nL + 255) / 256; }), gN = maxOver([](const Sys& Y) { return Y.n; });
      const BaDev* dDev = B.dDev.as<BaDev>();
      if (anyBuild) {
        if (lateUploads) HIPCHK(hipLaunchHostFunc(s, lateUpload, nullptr));
        HIPCHK(hipMemcpyAsync(B.dDev.p, hDevA, sizeof(BaDev) * n, hipMemcpyHostToDevice, s));
        if (anyChi) {
          hipLaunchKernelGGL(kb_errors, dim3(gE, 1, n), dim3(256), 0, s, dDev, 0);
          hipLaunchKernelGGL(kb_sum_partials, dim3(1, 1, n), dim3(256), 0, s, dDev, 0);
        }
        hipLaunchKernelGGL(kb_build_points, dim3(gL128, 1, n), dim3(128), 0, s, dDev);
        if (gP) hipLaunchKernelGGL(kb_build_poses, dim3(gP, 1, n), dim3(256), 0, s, dDev);
        if (anyDiag) hipLaunchKernelGGL(kb_max_diag, dim3(1, 1, n), dim3(256), 0, s, dDev);
        HIPCHK(hipGetLastError());
        if (anyChi || anyDiag) {
          HIPCHK(hipMemcpyAsync(hScal, dScalAll, sizeof(double) * 8 * n, hipMemcpyDeviceToHost, s));
          HIPCHK(hipStreamSynchronize(s));
        }
        for (int j = 0; j < n; j++) {
          Job& X = *J[j];
          const BaDev& D = hDevA[j];
          if (!D.build) continue;
          if (D.chi2) X.run->lm.setChi2(hScal[8 * j + 0]);
          X.needBuild = false;
          if (D.maxdiag && !X.run->lm.setMaxDiag(hScal[8 * j + 1])) nextStage(j, true);
        }
      }
      // (b) one LM trial of every unfinished problem ----------------------------------------------------------------------------------
      for (int j = 0; j < n; j++) {
        Job& X = *J[j];
        BaDev& D = hDevB[j];
        D = X.dev;
        D.build = D.chi2 = D.maxdiag = 0;
        D.trial = !X.done;
        D.lambda = X.run ? X.run->lm.lambda : 0;
        D.cur = X.done ? 0 : X.run->cur;
      }
      if (lateUploads) HIPCHK(hipLaunchHostFunc(s, lateUpload, nullptr));
      HIPCHK(hipMemcpyAsync(B.dDev.p, hDevB, sizeof(BaDev) * n, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(kb_dinv, dim3(gL256, 1, n), dim3(256), 0, s, dDev);
      hipLaunchKernelGGL(kb_bd, dim3(gE, 1, n), dim3(256), 0, s, dDev);
      if (gP) hipLaunchKernelGGL(kb_bs, dim3(gP, 1, n), dim3(256), 0, s, dDev);
      hipLaunchKernelGGL(kb_schur_pairs, dim3(gBk, 1, n), dim3(64 * kSchurWaves), 0, s, dDev);
      for (int kb = 0; kb < gNb; kb++)
        hipLaunchKernelGGL(kb_chol_step, dim3((gNb - kb) * (gNb - kb + 1) / 2 + (kb > 0), 1, n), dim3(256), 0, s, dDev, kb);
      {
        const size_t dyn = sizeof(double) * (size_t)gN;
        if (dyn > 48 * 1024)
          HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kb_chol_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
        hipLaunchKernelGGL(kb_chol_solve, dim3(1, 1, n), dim3(1024), dyn, s, dDev);
      }
      hipLaunchKernelGGL(kb_backsub, dim3(gL128, 1, n), dim3(128), 0, s, dDev);
      hipLaunchKernelGGL(kb_update, dim3(gUpd, 1, n), dim3(256), 0, s, dDev);
      hipLaunchKernelGGL(kb_scale, dim3(gScale, 1, n), dim3(256), 0, s, dDev);
      hipLaunchKernelGGL(kb_sum_partials, dim3(1, 1, n), dim3(256), 0, s, dDev, 2);
      hipLaunchKernelGGL(kb_errors, dim3(gE, 1, n), dim3(256), 0, s, dDev, 1);
      hipLaunchKernelGGL(kb_sum_partials, dim3(1, 1, n), dim3(256), 0, s, dDev, 1);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(hScal, dScalAll, sizeof(double) * 8 * n, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      trace("batch: round synchronised");
      // (c) the LM decision of every problem (optimization_algorithm_levenberg.cpp:95-146, as in optimize()) -----------------------------------
      for (int j = 0; j < n; j++) {
        Job& X = *J[j];
        if (X.done) continue;
        const double* hs = hScal + (size_t)8 * j;
        const LmSchedule::Next next = X.run->lm.trial(hs[0], hs[2], (int)hs[6] == 0, X.run->P->stop);
        if (X.run->lm.lastAccepted) X.run->cur ^= 1;
        X.needBuild = next == LmSchedule::NextIteration;
        if (next == LmSchedule::StageOver) nextStage(j, true);
      }
    }
    return YDORB_OK;
  };
  {
    // a HIP error inside the rounds ends the group: every member that has not been read back reports it (its poses / points / outlier
    // list were not written), members that failed earlier keep their own status
    int rr = rounds();
    if (rr == YDORB_OK && hipStreamSynchronize(s) != hipSuccess) { set_error("hipStreamSynchronize failed after the lock-step rounds"); rr = YDORB_ERR_HIP; }
    if (rr != YDORB_OK) {
      const std::string text = ydorb_last_error();
      for (int j = 0; j < n; j++)
        if (J[j]->rc == YDORB_OK && J[j]->run && (!J[j]->done || J[j]->pendingEnd)) { J[j]->pendingEnd = false; J[j]->errText = text; fail(j, rr); }
      set_error("%s", text.c_str());
      return rr;
    }
  }
  spread([&](int j, hipStream_t st) {   // endSolve of every finished problem (the lock-step stream has drained)
    Job& X = *J[j];
    if (!X.pendingEnd) return;
    X.pendingEnd = false;
    X.mem.stream = st;
    const int r = endSolve(*X.run);
    X.mem.stream = s;
    if (r) { X.errText = ydorb_last_error(); fail(j, r); }
  });
  trace("batch: done");
  int first = YDORB_OK;
  for (int j = 0; j < n; j++) if (J[j]->rc != YDORB_OK && first == YDORB_OK) first = J[j]->rc;
  return first;
}

}  // namespace

// ydorb_host.h: the factorisation's launch sequence for a system another driver assembled (ydorb_ba_dense_solve, essential_graph.hip)
static_assert(ydorb::kCholTile == NB, "ydorb_host.h states the tile of the blocked Cholesky");
int ydorb::chol_max_rows() { return kCholSolveMaxN; }
int ydorb::chol_factor_solve(void* stream, double* S, double* diagL, double* diagInv, int n, int* status, double* b, double* yv, double* x) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = n / NB;
  for (int kb = 0; kb < nb; kb++)
    hipLaunchKernelGGL(k_chol_step, dim3((nb - kb) * (nb - kb + 1) / 2 + (kb > 0)), dim3(256), 0, s, S, diagL, diagInv, n, kb, status, b, yv);
  if (!launch_chol_solve(s, S, diagInv, n, yv, b, x)) {
    set_error("system of %d rows is wider than the solve kernel's LDS (max %d)", n, kCholSolveMaxN);
    return YDORB_ERR_UNSUPPORTED;
  }
  HIPCHK(hipGetLastError());
  return YDORB_OK;
}

extern "C" {

void ydorb_ba_default_options(YdBaOptions* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->iters1 = 5; o->iters2 = 10;
  o->chi2_mono = 5.991; o->chi2_stereo = 7.815;
  o->delta_mono = (double)(float)sqrt(5.991);   // `const float monoDelta = sqrt(5.991)`, optimizer.cpp:223
  o->delta_stereo = (double)(float)sqrt(7.815);
  o->max_trials = 10;
  o->device = 0;
  o->rank = 0; o->world = 1;
}

int ydorb_ba_solve(const YdBaProblem* P, const YdBaOptions* optIn, YdBaResult* res) {
  const YdBaSolverOptions dense = {YDORB_BA_SOLVER_DENSE, YDORB_ESS_ORDER_SMALLER, 0};
  return ydorb_ba_solve_with(P, optIn, &dense, res, nullptr);
}

int ydorb_ba_solve_with(const YdBaProblem* P, const YdBaOptions* optIn, const YdBaSolverOptions* sopt, YdBaResult* res, YdBaSolverInfo* info) {
  const YdBaSolverOptions SO = sopt ? *sopt : YdBaSolverOptions{YDORB_BA_SOLVER_AUTO, YDORB_ESS_ORDER_SMALLER, 0};
  if (info) memset(info, 0, sizeof(*info));
  YdBaOptions O;
  int rc = checkProblem(P, optIn, res, &O);
  if (rc) return rc;
  const int K = P->n_poses, NP = P->n_points, E = P->n_edges;
  if (P->stop && *P->stop) { res->stopped = 1; return YDORB_OK; }  // optimizer.cpp:284-286
  if (E == 0 || K == 0 || NP == 0) return YDORB_OK;
  if ((rc = require_device(O.device))) return rc;
  g_t0 = std::chrono::steady_clock::now();
  trace("solve: begin");
  std::unique_lock<std::mutex> lock;
  Ctx* ctx = acquireCtx(O.device, lock);
  if (!ctx) return YDORB_ERR_HIP;
  Ctx& c = *ctx;
  Run R_{&c.mem, P, &O, res};
  R_.ev = c.ev; R_.hPin = c.hPin.as<double>();
  R_.SO = &SO; R_.info = info;
  if ((rc = beginSolve(R_))) return rc;
  trace("solve: state uploaded");
  hipEvent_t t0 = c.ev[2 * PH_COUNT], t1 = c.ev[2 * PH_COUNT + 1];
  HIPCHK(hipEventRecord(t0, c.mem.stream));

  for (;;) {   // bundleAdjust: one optimize() call, nothing culled; localBundleAdjust: two, unless stopped in between
    if ((rc = optimize(R_))) return rc;
    if (!R_.lm.handOver(P->stop)) break;
    if ((rc = launchCull(R_, 0))) return rc;
    trace("solve: depths read");
  }
  HIPCHK(hipEventRecord(t1, c.mem.stream));
  if ((rc = endSolve(R_))) return rc;
  (void)hipEventElapsedTime(&res->ms_total, t0, t1);
  trace("solve: results read back");
  res->ms_errors = (float)R_.phaseMs[PH_ERR]; res->ms_build = (float)R_.phaseMs[PH_BUILD]; res->ms_schur = (float)R_.phaseMs[PH_SCHUR];
  res->ms_solve = (float)R_.phaseMs[PH_SOLVE]; res->ms_update = (float)R_.phaseMs[PH_UPDATE];
  return YDORB_OK;
}

int ydorb_pose_optimize(const YdPoseBatch* B, uint8_t* outlier, int32_t* n_inliers, double* chi2_log, int32_t* trials) {
  if (!B || B->n_frames < 0 || (B->n_frames && (!B->edge_start || !B->poses || !n_inliers)) || B->device < 0 || B->device >= 16) {
    set_error("invalid pose batch");
    return YDORB_ERR_INVALID_ARG;
  }
  const int n = B->n_frames;
  if (n == 0) return YDORB_OK;
  if (B->edge_start[0] != 0) { set_error("edge_start[0] must be 0"); return YDORB_ERR_INVALID_ARG; }
  for (int f = 0; f < n; f++)
    if (B->edge_start[f + 1] < B->edge_start[f]) { set_error("edge_start must be non-decreasing"); return YDORB_ERR_INVALID_ARG; }
  const int E = B->edge_start[n];
  if (E > 0 && (!B->points || !B->meas || !B->inv_sigma2 || !outlier)) { set_error("null edge arrays"); return YDORB_ERR_INVALID_ARG; }
  int rc = require_device(B->device);
  if (rc) return rc;
  std::unique_lock<std::mutex> lock;
  Ctx* c = acquireCtx(B->device, lock);
  if (!c) return YDORB_ERR_HIP;
  hipStream_t s = c->mem.stream;
  const size_t Ez = (size_t)std::max(E, 1);
  PosePtrs q;
  if ((rc = c->pose.ensure(layPose(n, Ez, nullptr, q)))) return rc;
  layPose(n, Ez, c->pose.p, q);
  HIPCHK(hipMemcpyAsync(q.start, B->edge_start, sizeof(int) * (n + 1), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(q.poses, B->poses, sizeof(double) * 7 * n, hipMemcpyHostToDevice, s));
  if (E) {
    HIPCHK(hipMemcpyAsync(q.X, B->points, sizeof(double) * 3 * E, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(q.meas, B->meas, sizeof(double) * 3 * E, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(q.info, B->inv_sigma2, sizeof(double) * E, hipMemcpyHostToDevice, s));
  }
  const Cam cam{B->fx, B->fy, B->cx, B->cy, B->bf};
  const double dM = (double)(float)sqrt(5.991), dS = (double)(float)sqrt(7.815);   // optimizer.cpp:381-382
  hipLaunchKernelGGL(k_pose_optimize, dim3(n), dim3(kPoseThreads), 0, s, n, q.start, q.poses, q.X, q.meas, q.info, cam, dM, dS, q.err, q.flags, q.outlier, q.inl, q.chi, q.trials);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(B->poses, q.poses, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(n_inliers, q.inl, sizeof(int) * n, hipMemcpyDeviceToHost, s));
  if (E) HIPCHK(hipMemcpyAsync(outlier, q.outlier, E, hipMemcpyDeviceToHost, s));
  if (chi2_log) HIPCHK(hipMemcpyAsync(chi2_log, q.chi, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, s));
  if (trials) HIPCHK(hipMemcpyAsync(trials, q.trials, sizeof(int) * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return YDORB_OK;
}

int ydorb_ba_solve_batch(const YdBaProblem* probs, int32_t n, const YdBaOptions* opt, YdBaResult* res, int32_t threads, int32_t* rcEach) {
  if (n < 0 || (n > 0 && (!probs || !res))) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  if (opt && opt->world > 1) { set_error("the batched form solves whole problems: no landmark sharding"); return YDORB_ERR_INVALID_ARG; }
  if (n == 0) return YDORB_OK;
  YdBaOptions O;
  if (opt) O = *opt; else ydorb_ba_default_options(&O);
  if (O.device < 0 || O.device >= 16) { set_error("invalid device"); return YDORB_ERR_INVALID_ARG; }
  int rc = require_device(O.device);
  if (rc) return rc;
  BatchPool& B = g_batch[O.device];
  std::lock_guard<std::mutex> lock(B.mu);
  g_t0 = std::chrono::steady_clock::now();
  HIPCHK(hipSetDevice(O.device));
  if (!B.stream) HIPCHK(hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking));
  // `threads` is the number of problems advanced together (0 = as many as fit one group); the lock-step batch needs no host threads
  const int group = std::max(1, std::min<int>(threads > 0 ? threads : kBatchGroup, kBatchGroup));
  if ((rc = B.hDev.ensure(sizeof(BaDev) * 2 * group)) || (rc = B.hScal.ensure(sizeof(double) * 8 * group))) return rc;
  while ((int)B.jobs.size() < group) B.jobs.push_back(new Job());
  int first = YDORB_OK;
  std::string firstText;
  for (int at = 0; at < n; at += group) {
    const int m = std::min(group, n - at);
    rc = solveGroup(B, probs + at, O, res + at, m, rcEach ? rcEach + at : nullptr);
    if (rc != YDORB_OK && first == YDORB_OK) { first = rc; firstText = ydorb_last_error(); }
  }
  if (first != YDORB_OK) set_error("%s", firstText.c_str());
  return first;
}

int ydorb_ba_release(int32_t device) {
  if (device < 0 || device >= 16) { set_error("invalid device"); return YDORB_ERR_INVALID_ARG; }
  int rc = require_device(device);
  if (rc) return rc;
  HIPCHK(hipSetDevice(device));
  for (int i = 0; i < kCtxPool; i++) {          // waits for a solve that holds the context
    std::lock_guard<std::mutex> lock(g_mu[device][i]);
    Ctx& c = g_ctx[device][i];
    if (c.mem.stream) (void)hipStreamSynchronize(c.mem.stream);
    c.releaseBuffers();
  }
  BatchPool& B = g_batch[device];
  std::lock_guard<std::mutex> lock(B.mu);
  if (B.stream) (void)hipStreamSynchronize(B.stream);
  for (Job* j : B.jobs) { j->mem.releaseBuffers(); delete j; }
  B.jobs.clear();
  for (Mem* m : {&B.dDev, &B.dScal, static_cast<Mem*>(&B.hDev), static_cast<Mem*>(&B.hScal)}) m->release();
  return YDORB_OK;
}

int ydorb_ba_dense_solve(int32_t device, const double* A, int32_t n0, const double* b, double* x, int32_t* ok) {
  if (!A || !b || !x || !ok || n0 < 1 || device < 0 || device >= 16) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  int rc = require_device(device);
  if (rc) return rc;
  const int n = (n0 + NB - 1) / NB * NB, nb = n / NB;
  std::vector<double> hA((size_t)n * n, 0.0), hb(n, 0.0);
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) hA[(size_t)i * n + j] = (i < n0 && j < n0) ? A[(size_t)i * n0 + j] : (i == j ? 1.0 : 0.0);
    if (i < n0) hb[i] = b[i];
  }
  Layout L;
  const size_t tiles = sizeof(double) * nb * NB * NB;
  const size_t oA = L.add(sizeof(double) * n * n), oD = L.add(tiles), oI = L.add(tiles), ob = L.add(sizeof(double) * n), ox = L.add(sizeof(double) * n),
               oy = L.add(sizeof(double) * n), ost = L.add(sizeof(int) * 2);
  ScopedMem m;   // exact size; freed on every return
  if ((rc = m.alloc(L.bytes))) return rc;
  double *dA = m.at<double>(oA), *dD = m.at<double>(oD), *dI = m.at<double>(oI), *db = m.at<double>(ob), *dx = m.at<double>(ox), *dy = m.at<double>(oy);
  int* dst = m.at<int>(ost);
  HIPCHK(hipMemcpy(dA, hA.data(), sizeof(double) * n * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(db, hb.data(), sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dst, 0, sizeof(int) * 2));
  if ((rc = chol_factor_solve(nullptr, dA, dD, dI, n, dst, db, dy, dx))) return rc;
  std::vector<double> hx(n);
  int hst[2];
  HIPCHK(hipMemcpy(hx.data(), dx, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hst, dst, sizeof(hst), hipMemcpyDeviceToHost));
  *ok = hst[0] == 0;
  for (int i = 0; i < n0; i++) x[i] = hx[i];
#ifdef CHOL_TIMING
  {
    static long long clk[2][32][12];
    HIPCHK(hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_cholClk), sizeof(clk)));
    for (int w = 0; w < 2; w++)
      for (int kb = 0; kb < nb && kb < 32; kb += 6) {
        fprintf(stderr, "chol wg%d kb=%d:", w, kb);
        for (int p2 = 1; p2 < 11; p2++) fprintf(stderr, " %.2f", clk[w][kb][p2] ? (clk[w][kb][p2] - clk[w][kb][0]) / 100.0 : -1.0);
        fprintf(stderr, " us\n");
      }
    for (int kb = 1; kb < nb && kb < 32; kb++) fprintf(stderr, "%.1f ", (clk[0][kb][0] - clk[0][kb - 1][0]) / 100.0);
    fprintf(stderr, "us between step starts\n");
  }
#endif
  return YDORB_OK;
}

int ydorb_ba_plan(const YdBaProblem* P, const YdBaOptions* optIn, const YdBaSolverOptions* sopt, YdBaSolverInfo* info, int32_t* perm, int32_t* first) {
  if (!P || !info) { set_error("null argument"); return YDORB_ERR_INVALID_ARG; }
  YdBaResult res{};
  YdBaOptions O;
  int rc = checkProblem(P, optIn, &res, &O);
  if (rc) return rc;
  const YdBaSolverOptions SO = sopt ? *sopt : YdBaSolverOptions{YDORB_BA_SOLVER_AUTO, YDORB_ESS_ORDER_SMALLER, 0};
  // the free poses as prepareStage numbers them: not fixed and, on one rank, seen by an edge
  int nPf = 0;
  {
    std::vector<uint8_t> used(P->n_poses, O.world > 1 ? 1 : 0);
    for (int e = 0; e < P->n_edges; e++) used[P->edge_pose[e]] = 1;
    for (int k = 0; k < P->n_poses; k++) nPf += used[k] && !P->pose_fixed[k];
  }
  bapairs::PairList pairs;
  sky::Plan plan;
  bool sky = false;
  rc = chooseSolver(&SO, O.world, nPf, [&] { return bapairs::buildPairsFromEdges(P->n_poses, P->n_points, P->n_edges, P->pose_fixed, P->edge_pose, P->edge_point, O.world > 1); },
                    false, pairs, plan, sky, info);
  if (rc) return rc;
  for (int i = 0; i < nPf && (int)plan.perm.size() == nPf; i++) {
    if (perm) perm[i] = plan.perm[i];
    if (first) first[i] = plan.first[i];
  }
  return YDORB_OK;
}

int ydorb_ba_reduced_system_with(const YdBaProblem* P, const YdBaOptions* optIn, const YdBaSolverOptions* sopt, double lambda, double* S_out,
                                 double* bs_out, double* x_out, int32_t* solved) {
  if (!S_out || !bs_out || !x_out || !solved) { set_error("null argument"); return YDORB_ERR_INVALID_ARG; }
  const YdBaSolverOptions SO = sopt ? *sopt : YdBaSolverOptions{YDORB_BA_SOLVER_AUTO, YDORB_ESS_ORDER_SMALLER, 0};
  YdBaResult res{};
  YdBaOptions O;
  int rc = checkProblem(P, optIn, &res, &O);
  if (rc) return rc;
  if (P->n_edges == 0 || O.world > 1) { set_error("reduced system: needs edges and a single rank"); return YDORB_ERR_INVALID_ARG; }
  if ((rc = require_device(O.device))) return rc;
  std::unique_lock<std::mutex> lock;
  Ctx* ctx = acquireCtx(O.device, lock);
  if (!ctx) return YDORB_ERR_HIP;
  Ctx& c = *ctx;
  Run R_{&c.mem, P, &O, &res};
  R_.ev = c.ev; R_.hPin = c.hPin.as<double>();
  R_.SO = &SO;
  if ((rc = beginSolve(R_))) return rc;
  if ((rc = prepareStage(R_, false))) return rc;
  const Sys& Y = R_.sys;
  const int F = Y.nPf, n6 = 6 * F;
  if (Y.Ea == 0 || F == 0) { set_error("reduced system: no free pose"); return YDORB_ERR_INVALID_ARG; }
  if (n6 > 4096) { set_error("reduced system: %d rows, at most 4096 are expanded", n6); return YDORB_ERR_UNSUPPORTED; }
  hipStream_t s = c.mem.stream;
  const UpPtrs& u = c.mem.u;
  const WorkPtrs& w = c.mem.w;
  EdgeSoA Ed{u.ePose, u.ePidx, u.ePt, u.eMeas, u.eInfo, u.eRobust, Y.Ea};
  const double *poses = c.mem.st.poses[R_.cur], *pts = c.mem.st.pts[R_.cur];
  hipLaunchKernelGGL(k_errors, dim3(Y.nBlkE), dim3(256), 0, s, Ed, poses, pts, R_.cam, O.delta_mono, O.delta_stereo, w.err, w.partial);
  hipLaunchKernelGGL(k_build_points, dim3((Y.nL + 127) / 128), dim3(128), 0, s, Ed, u.ptStart, Y.nL, poses, pts, R_.cam, O.delta_mono, O.delta_stereo, w.err, w.Hll, w.bl, w.Hpl);
  hipLaunchKernelGGL(k_build_poses, dim3(F), dim3(256), 0, s, Ed, u.poseStart, u.poseEdges, poses, pts, R_.cam, O.delta_mono, O.delta_stereo, w.err, w.Hpp, w.bp(Y));
  if ((rc = launchSchur(R_, lambda, 1.0))) return rc;
  const size_t nS = Y.sky ? Y.envDoubles() : (size_t)Y.n * Y.n;
  std::vector<double> hS(nS), hx(Y.n);
  int hst[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hS.data(), w.S, sizeof(double) * nS, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(bs_out, w.bs(Y), sizeof(double) * n6, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));   // the factorisation overwrites S
  if ((rc = launchSolve(R_))) return rc;
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(hx.data(), w.xp, sizeof(double) * Y.n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hst, w.status, sizeof(hst), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *solved = hst[0] == 0;
  for (int i = 0; i < n6; i++) x_out[i] = hx[i];
  // the lower triangle of either storage, mirrored
  if (!Y.sky) {
    for (int r = 0; r < n6; r++)
      for (int cc = 0; cc <= r; cc++) S_out[(size_t)r * n6 + cc] = S_out[(size_t)cc * n6 + r] = hS[(size_t)r * Y.n + cc];
  } else {
    sky::expandEnvelope<6>(Y.plan, hS.data(), S_out, sky::kDiagLower);
  }
  return YDORB_OK;
}

int ydorb_ba_skyline_solve(int32_t device, const double* A, int32_t n, const double* b, int32_t ordering, double* x, int32_t* ok) {
  if (!A || !b || !x || !ok || n < 6 || n % 6 || n > 4096 || device < 0 || device >= 16 || ordering < YDORB_ESS_ORDER_SMALLER || ordering > YDORB_ESS_ORDER_RCM) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  int rc = require_device(device);
  if (rc) return rc;
  const int F = n / 6;
  // every non-zero block off the diagonal as a landmark that its two poses share
  std::vector<int> start(1, 0), pidx;
  for (int i = 0; i < F; i++)
    for (int j = 0; j < i; j++) {
      bool any = false;
      for (int r = 0; r < 6 && !any; r++)
        for (int cc = 0; cc < 6; cc++)
          if (A[(size_t)(6 * i + r) * n + 6 * j + cc] != 0.0 || A[(size_t)(6 * j + cc) * n + 6 * i + r] != 0.0) { any = true; break; }
      if (any) { pidx.push_back(j); pidx.push_back(i); start.push_back((int)pidx.size()); }
    }
  const bapairs::PairList pairs = bapairs::buildPairs(F, (int)start.size() - 1, start.data(), pidx.data());
  sky::Plan K;
  std::string err;
  if (!bapairs::planEnvelope(pairs, ordering, 0, true, K, err)) { set_error("%s", err.c_str()); return YDORB_ERR_UNSUPPORTED; }
  std::vector<double> env(36 * (size_t)K.envBlocks, 0.0);
  sky::packEnvelope<6>(K, A, env.data());
  struct { double *A, *b, *w, *x; int* status; sky::PlanArrays k; } d;
  auto lay = [&](void* base) {
    Carve a(base);
    a.take(d.A, env.size()); a.take(d.b, n); a.take(d.w, 2 * (size_t)n); a.take(d.x, n); a.take(d.status, 2);
    d.k.take(a, K, false);
    return a.L.bytes;
  };
  ScopedMem m;   // exact size; freed on every return
  if ((rc = m.alloc(lay(nullptr)))) return rc;
  lay(m.p);
  hipError_t upErr = hipSuccess;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    if (bytes && upErr == hipSuccess) upErr = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  };
  up(d.A, env.data(), sizeof(double) * env.size()); up(d.b, b, sizeof(double) * n);
  d.k.fill(K, up);
  HIPCHK(upErr);
  HIPCHK(hipMemset(d.status, 0, sizeof(int) * 2));
  hipLaunchKernelGGL(k_sky_solve, dim3(1), dim3(kSkyThreads), 0, nullptr, F, d.k.first, d.k.rowOff, d.k.colStart, d.k.colRows, d.k.colBlk, d.k.perm, d.b, d.A, d.w,
                     d.x, d.status);
  HIPCHK(hipGetLastError());
  int hst[2];
  HIPCHK(hipMemcpy(x, d.x, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hst, d.status, sizeof(hst), hipMemcpyDeviceToHost));
  *ok = hst[0] == 0;
  return YDORB_OK;
}

}  // extern "C"
