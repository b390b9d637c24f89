// Stand-alone check of ydorbslam_amd/csrc/lm_schedule.h (no HIP, no GPU): the product's LM schedule against a literal nested-loop
// transcription of g2o's, both fed the same scripted scalar stream.  tests/test_ba_lm_schedule_cpu.py builds it with
// -fsanitize=address,undefined and runs it as its own process:  lm_schedule_check [streams]
//
// The reference below is the shape of the reference code itself - SparseOptimizer::optimize (sparse_optimizer.cpp:366-440) around
// OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:57-173), called twice by Optimizer::localBundleAdjust
// (optimizer.cpp:284-314) - with the three device results of the BA driver (chi2, largest diagonal, one trial's tempChi / scale sum /
// solved) drawn from the script in place of the kernels.  It restates the lambda control too and includes nothing of the product.
// The product side steps LmSchedule the two ways ba_solver.hip does: as loops (the single solve) and as a state machine that is asked
// one question per round (a lock-step batch member).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ydorbslam_amd/csrc/lm_schedule.h"

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double u() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
  bool chance(double p) { return u() < p; }
};

const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

// One solve's inputs: the options and, on demand, the scalars the device would return.  A draw depends on the seed and on how many
// draws came before it only, so two control flows see the same values exactly as long as they ask for the same things in the same order;
// `asked` records that order.
struct Script {
  Rng rng;
  int iters1, iters2, maxTrials, stopAfter, nTrials = 0;
  bool singleStage, calm;
  volatile uint8_t stop = 0;
  double lastChi = 1;
  std::vector<char> asked;

  explicit Script(uint64_t seed) : rng{seed} {
    calm = rng.chance(0.08);   // every step accepted: the only runs that get past 32 iterations
    iters1 = calm ? 15 + rng.below(15) : rng.chance(0.1) ? 0 : 1 + rng.below(7);
    iters2 = calm ? 15 + rng.below(15) : rng.chance(0.1) ? 0 : 1 + rng.below(12);
    maxTrials = 1 + rng.below(10);
    singleStage = rng.chance(0.2);
    stopAfter = calm || rng.chance(0.5) ? -1 : rng.below(25);   // the flag rises once this many trials have run (0: before the first)
    stop = stopAfter == 0;
  }
  double chi2() {
    asked.push_back('c');
    if (!calm && rng.chance(0.02)) return rng.chance(0.5) ? kNaN : kInf;
    return lastChi = 1e6 + 100 * rng.u();
  }
  double maxDiag() {
    asked.push_back('d');
    const double v = 1 + 1000 * rng.u();
    if (calm) return v;
    if (rng.chance(0.12)) return 0;   // a second stage whose cull left no edge
    if (rng.chance(0.10)) { const double big[4] = {kInf, kNaN, 1e308, 1.7e308}; return big[rng.below(4)]; }   // lambda not finite at once or after a few rejections
    return v;
  }
  void trial(double* tempChi, double* scaleSum, bool* solved) {
    asked.push_back('t');
    *solved = true;
    *scaleSum = 1e-2 + rng.u();
    const double u = calm ? 1 : rng.u(), step = 0.1 * rng.u();
    if (u < 0.05) *tempChi = lastChi;                    // rho == 0 where the last chi2 drawn is the current one
    else if (u < 0.09) *tempChi = rng.chance(0.5) ? kNaN : kInf;
    else *tempChi = lastChi = calm || rng.chance(0.45) ? lastChi * (1 - step) : lastChi * (1 + step);
    if (u >= 0.09 && u < 0.13) *scaleSum = rng.chance(0.3) ? kNaN : rng.chance(0.5) ? -1e-3 : -1 - rng.u();   // scale NaN, 0 or negative
    if (u >= 0.13 && u < 0.23) *solved = false;
    if (++nTrials == stopAfter) stop = 1;
  }
};

struct Outcome {
  YdBaResult res;
  std::vector<uint8_t> accepts;
  int culls = 0;
  Outcome() { memset(&res, 0, sizeof(res)); }
};

// what the reference side saw, so that a branch no stream reaches fails the run
struct Coverage {
  long streams = 0, trials = 0, retries = 0, endMaxTrials = 0, endRhoZero = 0, endLambda = 0, rhoNaN = 0, failedSolves = 0, noEdgesLeft = 0,
       emptyStages = 0, stopBeforeIteration = 0, stopAfterTrial = 0, stopAtHandOver = 0, stopAtStageStart = 0, singleStage = 0, pastLogCap = 0,
       chi2Recomputed = 0;
} cov;

bool stopped(const Script& S, long& seen) { seen += S.stop; return S.stop; }   // the flag, polled; and where a raised one was seen

// ---- the reference ---------------------------------------------------------------------------------------------------------------
void refOptimize(Script& S, Outcome& out, int iterations, int stage) {
  double lambda = 0, ni = 2, currentChi = 0;
  bool lastAccepted = true;
  if (iterations == 0) cov.emptyStages++;
  for (int it = 0; it < iterations && !stopped(S, it == 0 ? cov.stopAtStageStart : cov.stopBeforeIteration); it++) {
    if (it == 0 || !lastAccepted) {   // computeActiveErrors + activeRobustChi2 (the driver skips what an accepted trial left in place)
      if (it) cov.chi2Recomputed++;
      currentChi = S.chi2();
    }
    if (it == 0) {   // computeLambdaInit
      const double maxDiagonal = S.maxDiag();
      if (stage == 2 && maxDiagonal == 0) { cov.noEdgesLeft++; break; }   // "0 vertices to optimize": the stage does not take place
      lambda = 1e-5 * maxDiagonal;
      ni = 2;
    }
    double rho = 0;
    int qmax = 0;
    do {
      if (qmax) cov.retries++;
      double tempChi, scaleSum;
      bool solved;
      S.trial(&tempChi, &scaleSum, &solved);
      cov.trials++;
      if (!solved) { tempChi = std::numeric_limits<double>::max(); cov.failedSolves++; }
      rho = (currentChi - tempChi);
      double scale = scaleSum + 1e-3;
      rho /= scale;
      if (rho > 0 && std::isfinite(tempChi)) {   // last step was good
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = (std::min)(alpha, 2. / 3.);
        double scaleFactor = (std::max)(1. / 3., alpha);
        lambda *= scaleFactor;
        ni = 2;
        currentChi = tempChi;
        lastAccepted = true;
        out.accepts.push_back(1);
      } else {
        lambda *= ni;
        ni *= 2;
        lastAccepted = false;
        out.accepts.push_back(0);
        if (!std::isfinite(lambda)) { qmax++; out.res.n_trials++; break; }
      }
      qmax++;
      out.res.n_trials++;
      if (std::isnan(rho)) cov.rhoNaN++;
    } while (rho < 0 && qmax < S.maxTrials && !stopped(S, cov.stopAfterTrial));
    YdBaResult& r = out.res;
    if (r.n_log < 32) {
      r.log_chi2[r.n_log] = currentChi; r.log_lambda[r.n_log] = lambda; r.log_trials[r.n_log] = qmax; r.log_stage[r.n_log] = stage;
      r.n_log++;
    }
    r.n_iterations++;
    if (qmax == S.maxTrials || rho == 0 || !std::isfinite(lambda)) {   // SolverResult::Terminate
      if (!std::isfinite(lambda)) cov.endLambda++; else if (rho == 0) cov.endRhoZero++; else cov.endMaxTrials++;
      break;
    }
  }
}
void refSolve(Script& S, Outcome& out) {
  refOptimize(S, out, S.iters1, 1);
  if (S.singleStage) {
    cov.singleStage++;
  } else if (!stopped(S, cov.stopAtHandOver)) {   // optimizer.cpp:290-314
    out.culls++;
    refOptimize(S, out, S.iters2, 2);
  } else {
    out.res.stopped = 1;
  }
  cov.streams++;
  if (out.res.n_iterations > 32) cov.pastLogCap++;
}

// ---- the product, stepped as ba_solver.hip steps it -----------------------------------------------------------------------------
YdBaOptions options(const Script& S) {
  YdBaOptions O;
  memset(&O, 0, sizeof(O));
  O.iters1 = S.iters1; O.iters2 = S.iters2; O.max_trials = S.maxTrials; O.flags = S.singleStage ? YDORB_BA_SINGLE_STAGE : 0;
  return O;
}
void stepTrial(ydorb::LmSchedule& lm, Script& S, Outcome& out, ydorb::LmSchedule::Next* next) {
  double tempChi, scaleSum;
  bool solved;
  S.trial(&tempChi, &scaleSum, &solved);
  *next = lm.trial(tempChi, scaleSum, solved, &S.stop);
  out.accepts.push_back(lm.lastAccepted);
}
void loopSolve(Script& S, Outcome& out) {   // optimize() and ydorb_ba_solve
  typedef ydorb::LmSchedule L;
  L lm;
  lm.begin(options(S), &out.res);
  for (;;) {
    for (bool more = lm.firstIteration(&S.stop); more;) {
      if (lm.needChi2()) lm.setChi2(S.chi2());
      if (lm.needLambdaInit() && !lm.setMaxDiag(S.maxDiag())) break;
      L::Next next;
      do stepTrial(lm, S, out, &next); while (next == L::Retry);
      more = next == L::NextIteration;
    }
    if (!lm.handOver(&S.stop)) break;
    out.culls++;
  }
}
void roundSolve(Script& S, Outcome& out) {   // one member of solveGroup: phases (a) and (c) of its rounds
  typedef ydorb::LmSchedule L;
  L lm;
  lm.begin(options(S), &out.res);
  bool needBuild = false, done = false;
  auto nextStage = [&](bool over) {
    needBuild = false;
    for (;; over = true) {
      if (over) {
        if (!lm.handOver(&S.stop)) { done = true; return; }
        out.culls++;
      }
      if (lm.firstIteration(&S.stop)) { needBuild = true; return; }
    }
  };
  nextStage(false);
  while (!done) {
    if (needBuild) {
      const bool chi2 = lm.needChi2(), maxdiag = lm.needLambdaInit();
      if (chi2) lm.setChi2(S.chi2());
      needBuild = false;
      if (maxdiag && !lm.setMaxDiag(S.maxDiag())) nextStage(true);
    }
    if (done) break;
    L::Next next;
    stepTrial(lm, S, out, &next);
    needBuild = next == L::NextIteration;
    if (next == L::StageOver) nextStage(true);
  }
}

bool same(double a, double b) { return a == b || (std::isnan(a) && std::isnan(b)); }
bool equal(const Outcome& a, const Script& sa, const Outcome& b, const Script& sb, const char* what, uint64_t seed) {
  const YdBaResult &x = a.res, &y = b.res;
  bool ok = x.n_trials == y.n_trials && x.n_iterations == y.n_iterations && x.n_log == y.n_log && x.stopped == y.stopped && a.culls == b.culls &&
            a.accepts == b.accepts && sa.asked == sb.asked;
  for (int i = 0; ok && i < x.n_log; i++)
    ok = same(x.log_chi2[i], y.log_chi2[i]) && same(x.log_lambda[i], y.log_lambda[i]) && x.log_trials[i] == y.log_trials[i] && x.log_stage[i] == y.log_stage[i];
  if (!ok)
    printf("MISMATCH %s, seed %llu: trials %d / %d, iterations %d / %d, log rows %d / %d, stopped %d / %d, culls %d / %d, scalars asked %zu / %zu\n", what,
           (unsigned long long)seed, x.n_trials, y.n_trials, x.n_iterations, y.n_iterations, x.n_log, y.n_log, x.stopped, y.stopped, a.culls, b.culls,
           sa.asked.size(), sb.asked.size());
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  const long streams = argc > 1 ? atol(argv[1]) : 20000;
  long bad = 0;
  for (long i = 0; i < streams; i++) {
    const uint64_t seed = 0x5eed0000ull + (uint64_t)i;
    Script sr(seed), sl(seed), sb(seed);
    Outcome ref, loops, rounds;
    refSolve(sr, ref);
    loopSolve(sl, loops);
    roundSolve(sb, rounds);
    bad += !equal(ref, sr, loops, sl, "loops", seed);
    bad += !equal(ref, sr, rounds, sb, "rounds", seed);
  }
  const struct { const char* name; long n; } rows[] = {
      {"rejected trial, then a retry", cov.retries}, {"iteration ended by max_trials", cov.endMaxTrials}, {"iteration ended by rho == 0", cov.endRhoZero},
      {"iteration ended by a non-finite lambda", cov.endLambda}, {"trial with rho = NaN", cov.rhoNaN}, {"chi2 recomputed after a rejected last trial", cov.chi2Recomputed},
      {"failed solve", cov.failedSolves}, {"second stage left at noEdgesLeft", cov.noEdgesLeft}, {"stage with 0 iterations", cov.emptyStages},
      {"stop seen before an iteration", cov.stopBeforeIteration}, {"stop seen after a trial", cov.stopAfterTrial}, {"stop seen at the hand-over", cov.stopAtHandOver},
      {"stop seen at the start of a stage", cov.stopAtStageStart}, {"single-stage run", cov.singleStage}, {"more than 32 iterations", cov.pastLogCap}};
  printf("%ld streams, %ld trials, %ld mismatches\n", cov.streams, cov.trials, bad);
  long unreached = 0;
  for (const auto& r : rows) { printf("  %-46s %ld\n", r.name, r.n); unreached += r.n == 0; }
  if (unreached) printf("UNREACHED: %ld of the branches above\n", unreached);
  return bad || unreached ? 1 : 0;
}
