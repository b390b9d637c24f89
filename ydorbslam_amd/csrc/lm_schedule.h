// g2o's Levenberg-Marquardt schedule of one local / global BA solve, stated once for the host: the outer-iteration loop of
// SparseOptimizer::optimize (core/sparse_optimizer.cpp:366-440), the trial loop and SolverResult::Terminate of
// OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:57-173) and the two-stage hand-over of
// Optimizer::localBundleAdjust (src/optimizer.cpp:284-314).  The single solve and every member of a lock-step batch (ba_solver.hip)
// step one LmSchedule each; they differ only in how the launches between two questions are issued.  No HIP here: a plain host
// compiler builds it (tests/cpu_harness/lm_schedule_check.cpp), and g2o_math.hip.h takes lm_judge from here for the device loops.
#pragma once
#include <stdint.h>
#include <cmath>

#include "../../include/ydorb/c_api.h"

#if defined(__HIPCC__)
#define YD_HD_INLINE __host__ __device__ inline __attribute__((always_inline))
#else
#define YD_HD_INLINE inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ydorb {
namespace g2o {

// The verdict on one LM trial (optimization_algorithm_levenberg.cpp:95-146), for the device loops and the host schedule alike.
// tempChi is the chi2 of the trial estimate - g2o applies _x and evaluates it even when the solve failed (solved == false) and then
// overrides it with DBL_MAX.  scale is computeScale() + 1e-3, formed by the caller in the order its results have always had (the dense
// device loops start their sum from the 1e-3, LmSchedule adds it to the device's sum), because results are compared bit for bit.
// Accept: lambda shrinks, ni = 2, currentChi = tempChi; reject: lambda *= ni, ni doubles.  The caller keeps its own push / pop, trial
// counters and the non-finite-lambda break.
YD_HD_INLINE bool lm_judge(double& lambda, double& ni, double& currentChi, double& rho, double tempChi, double scale, bool solved) {
  if (!solved) tempChi = 1.7976931348623157e308;   // DBL_MAX
  rho = currentChi - tempChi;
  rho /= scale;
  if (rho > 0 && std::isfinite(tempChi)) {
    double alpha = 1. - pow((2 * rho - 1), 3.0);
    alpha = fmin(alpha, 2. / 3.);
    lambda *= fmax(1. / 3., alpha);
    ni = 2;
    currentChi = tempChi;
    return true;
  }
  lambda *= ni; ni *= 2;
  return false;
}

}  // namespace g2o

// The driver asks in this order; `stop` is the caller's flag (NULL: never raised), read only where the reference polls it:
//   begin()  then per stage:  firstIteration(stop)                               - false: the stage has no iteration
//     per iteration:  needChi2() -> setChi2();  build;  needLambdaInit() -> setMaxDiag()   - false: the stage is over
//       per trial:    trial(tempChi, scaleSum, solved, stop) -> Retry | NextIteration | StageOver;  `lastAccepted`: flip the estimate
//   a stage over:  handOver(stop)  - true: cull, then the second stage from firstIteration();  false: the solve is finished
struct LmSchedule {
  enum Next { Retry, NextIteration, StageOver };
  typedef const volatile uint8_t* Stop;

  int stage = 1, it = 0, iterations = 0, qmax = 0, iters2 = 0, maxTrials = 0;
  bool singleStage = false, lastAccepted = true;
  double lambda = 0, ni = 2, currentChi = 0, rho = 0;
  double userLambdaInit = 0;   // setUserLambdaInit: > 0 replaces computeLambdaInit's 1e-5 * maxDiag; off by default, set after begin()
  YdBaResult* res = nullptr;

  static bool raised(Stop stop) { return stop && *stop; }

  void begin(const YdBaOptions& O, YdBaResult* r) {
    *this = LmSchedule();
    res = r; iterations = O.iters1; iters2 = O.iters2; maxTrials = O.max_trials; singleStage = (O.flags & YDORB_BA_SINGLE_STAGE) != 0;
  }
  // `for (it = 0; it < iterations && !terminate(); ...)` at it == 0
  bool firstIteration(Stop stop) const { return it < iterations && !raised(stop); }

  // computeActiveErrors + activeRobustChi2 at the top of an iteration: after the first iteration the state is the trial that was just
  // accepted, whose errors and chi2 are already there - same kernel, same inputs, same bits.  A trial can also end rejected without
  // terminating the loop (rho = NaN: `rho < 0` and `rho == 0` are both false); then they belong to the rejected state and are
  // recomputed on the kept one, as g2o does at the top of every iteration.
  bool needChi2() const { return it == 0 || !lastAccepted; }
  void setChi2(double chi2) { currentChi = chi2; }
  bool needLambdaInit() const { return it == 0; }
  // computeLambdaInit from the largest diagonal entry of H.  False ends a second stage that has no edge left: initializeOptimization(0)
  // finds no level-0 edge when the cull removed them all, and optimize() returns without an iteration ("0 vertices to optimize"; the
  // oracle's `if (act.empty()) return`).  The driver's culled edges keep their slots with information 0, so the stage is entered; its
  // first buildSystem then gives H = 0, whereas one surviving edge puts fx^2 / z^2 * information > 0 on its landmark's diagonal.
  // Nothing is logged and no trial runs: the stage did not take place.
  bool setMaxDiag(double maxDiag) {
    if (stage == 2 && maxDiag == 0) return false;
    lambda = userLambdaInit > 0 ? userLambdaInit : 1e-5 * maxDiag; ni = 2;
    return true;
  }

  // One trial's read-back.  Accepted (lastAccepted): discardTop(), the caller keeps the updated estimate; else pop(), the previous one
  // stays.  An iteration that ends is logged (32 rows at most) and counted, then SolverResult::Terminate and the loop condition decide.
  Next trial(double tempChi, double scaleSum, bool solved, Stop stop) {
    lastAccepted = g2o::lm_judge(lambda, ni, currentChi, rho, tempChi, scaleSum + 1e-3, solved);
    qmax++;
    res->n_trials++;
    const bool lambdaBroke = !lastAccepted && !std::isfinite(lambda);   // `break` out of the trial loop, after counting the trial
    if (!lambdaBroke && rho < 0 && qmax < maxTrials && !raised(stop)) return Retry;
    if (res->n_log < 32) {
      res->log_chi2[res->n_log] = currentChi; res->log_lambda[res->n_log] = lambda; res->log_trials[res->n_log] = qmax; res->log_stage[res->n_log] = stage;
      res->n_log++;
    }
    res->n_iterations++;
    const bool terminate = qmax == maxTrials || rho == 0 || !std::isfinite(lambda);
    it++; qmax = 0; rho = 0;
    return terminate || !(it < iterations && !raised(stop)) ? StageOver : NextIteration;
  }

  // optimizer.cpp:290-314 after the first optimize() call, nothing after the second or after bundleAdjust's only one.  True: the caller
  // culls the edges over the chi2 threshold and goes through the second stage, which starts here.  A stop seen here is reported.
  bool handOver(Stop stop) {
    if (stage != 1 || singleStage) return false;
    if (raised(stop)) { res->stopped = 1; return false; }
    stage = 2; it = 0; iterations = iters2; qmax = 0; rho = 0; lastAccepted = true; lambda = 0; ni = 2; currentChi = 0;
    return true;
  }
};

}  // namespace ydorb
