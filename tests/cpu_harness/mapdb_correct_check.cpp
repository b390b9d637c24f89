// Stand-alone check of the map correction's host side in ydorbslam_amd/csrc/mapdb_host.h (no HIP, no GPU): the validation of
// ydorb_mapdb_correct, the keyframe rank table, the claim pass and what the mirror takes from a result.
// tests/test_mapcorrect_cpu.py builds it with -fsanitize=address,undefined and runs it as its own process.  One line per case; the
// exit status is the number of failed cases.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/mapdb_host.h"

using namespace ydorb::mapdb;

static int g_failed = 0;

static void expect(const char* name, bool ok, const std::string& err, const char* needle) {
  const bool pass = needle ? (!ok && err.find(needle) != std::string::npos) : ok;
  printf("%-60s %s%s%s\n", name, pass ? "ok" : "FAILED", err.empty() ? "" : ": ", err.c_str());
  if (!pass) g_failed++;
}

// 4 keyframes, 6 point slots: 0 good (ref kf 0), 1 bad, 2 good (ref kf 3), 3 never set, 4 good with an empty span (ref kf 1), 5 good (ref kf 2,
// reference level 7)
static void fill(Host& h) {
  std::string e;
  const int32_t ks[4] = {0, 1, 2, 3};
  const float cen[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  h.setCentres(ks, 4, cen, e);
  const int32_t slots[5] = {0, 1, 2, 4, 5}, start[6] = {0, 2, 3, 5, 5, 6}, kf[6] = {0, 1, 2, 3, 0, 2}, refKf[5] = {0, 2, 3, 1, 2};
  const uint8_t level[6] = {0, 1, 2, 3, 0, 7}, bad[5] = {0, 1, 0, 0, 0}, refLevel[5] = {0, 0, 3, 0, 7};
  const float pos[15] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
  h.setPoints(slots, 5, start, kf, level, bad, refKf, refLevel, pos, e);
}

struct Call {   // a well-formed Sim3 call over keyframe slots {2, 0}, to be broken one field at a time
  std::vector<int32_t> kf{2, 0}, slots{0, 5}, corrector{1, 0};
  std::vector<double> before, after;
  std::vector<float> centreAfter, sf{1.f, 1.2f, 1.44f}, normal, minD, maxD, pos;
  std::vector<uint8_t> status;
  YdMapCorrection c;
  Call() : before(16, 0.0), after(16, 0.0), centreAfter(6, 0.5f), normal(64), minD(64), maxD(64), pos(64), status(64) {
    for (int k = 0; k < 2; k++) { before[8 * k + 3] = after[8 * k + 3] = 1.0; before[8 * k + 7] = after[8 * k + 7] = 1.0; }
    memset(&c, 0, sizeof(c));
    c.n_kf = 2; c.arithmetic = YDORB_MAPCORR_SIM3; c.kf_slots = kf.data(); c.before = before.data(); c.after = after.data();
    c.centre_after = centreAfter.data(); c.centres = YDORB_MAPCORR_INTERLEAVED; c.n = 2; c.slots = slots.data(); c.corrector = corrector.data();
    c.scale_factors = sf.data(); c.n_levels = 8; c.normal = normal.data(); c.min_distance = minD.data(); c.max_distance = maxD.data();
    c.pos_out = pos.data(); c.status = status.data();
  }
};

static bool sameState(const Host& a, const Host& b) {
  YdMapDbStats x, y;
  a.stats(x); b.stats(y);
  return memcmp(&x, &y, sizeof(x)) == 0 && a.dirty() == b.dirty() && a.mirrorPos() == b.mirrorPos() && a.mirrorCentres() == b.mirrorCentres();
}

int main() {
  std::string e;
  Host h(8, 4, 32), twin(8, 4, 32);
  fill(h); fill(twin);
  Host::CorrectionPlan P;

  { Call k; expect("well formed", h.planCorrection(&k.c, P, e), e, nullptr); }
  // ---- every validation message; h stays as staged as twin
  expect("null correction", h.planCorrection(nullptr, P, e), e, "null correction");
  { Call k; k.c.arithmetic = 2; expect("unknown arithmetic", h.planCorrection(&k.c, P, e), e, "unknown arithmetic 2"); }
  { Call k; k.c.centres = 3; expect("unknown centres", h.planCorrection(&k.c, P, e), e, "unknown centres rule 3"); }
  { Call k; k.c.n_kf = -1; expect("negative n_kf", h.planCorrection(&k.c, P, e), e, "negative number of keyframe slots: -1"); }
  { Call k; k.c.n = -2; expect("negative n", h.planCorrection(&k.c, P, e), e, "negative number of entries: -2"); }
  { Call k; k.c.centre_after = nullptr; expect("centres without centre_after", h.planCorrection(&k.c, P, e), e, "a centres rule without centre_after"); }
  { Call k; k.c.kf_slots = nullptr; expect("null kf_slots", h.planCorrection(&k.c, P, e), e, "null kf_slots"); }
  { Call k; k.c.after = nullptr; expect("null after", h.planCorrection(&k.c, P, e), e, "null before or after"); }
  { Call k; k.c.status = nullptr; expect("null status", h.planCorrection(&k.c, P, e), e, "null pos_out or status"); }
  { Call k; k.c.min_distance = nullptr; expect("two of three normal outputs", h.planCorrection(&k.c, P, e), e, "all three or none"); }
  { Call k; k.c.n_levels = 9; expect("n_levels 9", h.planCorrection(&k.c, P, e), e, "n_levels 9 outside 1..8"); }
  { Call k; k.c.n_levels = 0; expect("n_levels 0", h.planCorrection(&k.c, P, e), e, "n_levels 0 outside 1..8"); }
  { Call k; k.c.scale_factors = nullptr; expect("null scale_factors", h.planCorrection(&k.c, P, e), e, "null scale_factors"); }
  { Call k; k.c.slots = nullptr; expect("null slots, n != n_points", h.planCorrection(&k.c, P, e), e, "null slots with n = 2, not n_points = 6"); }
  { Call k; k.kf[1] = 4; expect("keyframe slot out of range", h.planCorrection(&k.c, P, e), e, "kf_slots[1]: keyframe slot 4 outside 0..3"); }
  { Call k; k.kf[0] = -1; expect("keyframe slot negative", h.planCorrection(&k.c, P, e), e, "kf_slots[0]: keyframe slot -1 outside 0..3"); }
  { Call k; k.kf[1] = 2; expect("keyframe slot repeated", h.planCorrection(&k.c, P, e), e, "kf_slots[1]: keyframe slot 2 repeats kf_slots[0]"); }
  { Call k; k.after[15] = 0.0; expect("Sim3 scale zero", h.planCorrection(&k.c, P, e), e, "after[1]: the Sim3 scale is not positive and finite"); }
  { Call k; k.before[7] = -1.0; expect("Sim3 scale negative", h.planCorrection(&k.c, P, e), e, "before[0]: the Sim3 scale is not positive and finite"); }
  { Call k; k.before[15] = std::nan(""); expect("Sim3 scale NaN", h.planCorrection(&k.c, P, e), e, "before[1]: the Sim3 scale is not positive and finite"); }
  { Call k; k.after[7] = std::numeric_limits<double>::infinity(); expect("Sim3 scale infinite", h.planCorrection(&k.c, P, e), e, "after[0]: the Sim3 scale"); }
  { Call k; k.slots[1] = 6; expect("point slot out of range", h.planCorrection(&k.c, P, e), e, "slots[1]: point slot 6 outside 0..5"); }
  { Call k; k.slots[0] = -1; expect("point slot negative", h.planCorrection(&k.c, P, e), e, "slots[0]: point slot -1 outside 0..5"); }
  { Call k; k.corrector[1] = 2; expect("corrector out of range", h.planCorrection(&k.c, P, e), e, "corrector[1]: 2 outside -1..1"); }
  { Call k; k.corrector[0] = -2; expect("corrector below -1", h.planCorrection(&k.c, P, e), e, "corrector[0]: -2 outside -1..1"); }
  { Call k; k.c.n_levels = 7; expect("ref_level >= n_levels of a corrected point", h.planCorrection(&k.c, P, e), e, "slots[1]: reference level 7 of point slot 5 >= n_levels"); }
  {   // the level is not read where no normals are computed: no outputs, a bad point, an empty span, an entry another one claimed
    Call k; k.c.n_levels = 7; k.c.normal = nullptr; k.c.min_distance = nullptr; k.c.max_distance = nullptr;
    e.clear(); expect("no normals: the level is not read", h.planCorrection(&k.c, P, e), e, nullptr);
  }
  e.clear();
  expect("a refused call changes neither mirror nor staging", sameState(h, twin) && h.dirty(), e, nullptr);

  // ---- the claim pass
  {
    Call k;   // slot 1 is bad: named 3 times around good slot 0, whose first good entry claims; 3 was never set
    k.slots = {1, 0, 1, 0, 3, 0}; k.corrector = {0, 1, 0, 0, 1, 1};
    k.c.n = 6; k.c.slots = k.slots.data(); k.c.corrector = k.corrector.data();
    bool ok = h.planCorrection(&k.c, P, e);
    ok = ok && P.status == std::vector<uint8_t>({YDORB_MAPCORR_BAD, YDORB_MAPCORR_DONE, YDORB_MAPCORR_BAD, YDORB_MAPCORR_CLAIMED, YDORB_MAPCORR_BAD, YDORB_MAPCORR_CLAIMED});
    ok = ok && P.entry == std::vector<int32_t>({1}) && P.slot == std::vector<int32_t>({0}) && P.rank == std::vector<int32_t>({1});
    expect("claim: the first entry that is not bad claims", ok, e, nullptr);
  }
  {
    Host g(8, 4, 32);   // a slot named 3 times of which the first is bad -> the second claims: make slot 0 bad between two calls
    fill(g);
    Call k;
    k.slots = {0, 0, 0}; k.corrector = {0, 1, 0}; k.c.n = 3; k.c.slots = k.slots.data(); k.c.corrector = k.corrector.data();
    bool ok = g.planCorrection(&k.c, P, e) && P.status == std::vector<uint8_t>({YDORB_MAPCORR_DONE, YDORB_MAPCORR_CLAIMED, YDORB_MAPCORR_CLAIMED}) &&
              P.rank == std::vector<int32_t>({0});
    // the list {bad 1, 0, 0}: the bad entry stamps nothing, the second entry claims with its own corrector
    k.slots = {1, 0, 0}; k.corrector = {0, 1, 0};
    ok = ok && g.planCorrection(&k.c, P, e) && P.status == std::vector<uint8_t>({YDORB_MAPCORR_BAD, YDORB_MAPCORR_DONE, YDORB_MAPCORR_CLAIMED}) &&
         P.entry == std::vector<int32_t>({1}) && P.rank == std::vector<int32_t>({1});
    expect("claim: named 3 times, the first bad, the second claims", ok, e, nullptr);
  }
  {
    Call k;   // -1 correctors: slot 0 (ref kf 0 -> rank 1) and 5 (ref kf 2 -> rank 0) are covered, 2 (ref kf 3) and 4 (ref kf 1) are not
    k.slots = {0, 2, 4, 5}; k.corrector = {-1, -1, -1, -1}; k.c.n = 4; k.c.slots = k.slots.data(); k.c.corrector = k.corrector.data();
    bool ok = h.planCorrection(&k.c, P, e);
    ok = ok && P.status == std::vector<uint8_t>({YDORB_MAPCORR_DONE, YDORB_MAPCORR_NOT_COVERED, YDORB_MAPCORR_NOT_COVERED, YDORB_MAPCORR_DONE});
    ok = ok && P.rank == std::vector<int32_t>({1, 0}) && P.rankOf == std::vector<int32_t>({1, -1, 0, -1});
    k.c.corrector = nullptr;   // null corrector: all -1
    Host::CorrectionPlan Q;
    ok = ok && h.planCorrection(&k.c, Q, e) && Q.status == P.status && Q.rank == P.rank;
    expect("claim: -1 correctors, covered and not covered", ok, e, nullptr);
  }
  {
    Call k;   // null slots: every slot in order; 4 has an empty span
    k.corrector = {0, 0, 0, 0, 1, 1}; k.c.n = 6; k.c.slots = nullptr; k.c.corrector = k.corrector.data();
    bool ok = h.planCorrection(&k.c, P, e);
    ok = ok && P.status == std::vector<uint8_t>({YDORB_MAPCORR_DONE, YDORB_MAPCORR_BAD, YDORB_MAPCORR_DONE, YDORB_MAPCORR_BAD, YDORB_MAPCORR_DONE_NO_OBSERVATIONS, YDORB_MAPCORR_DONE});
    ok = ok && P.slot == std::vector<int32_t>({0, 2, 4, 5}) && P.entry == P.slot && P.rank == std::vector<int32_t>({0, 0, 1, 1});
    expect("claim: null slots", ok, e, nullptr);
    // ---- the mirror after applying a result: the claimed positions and the centres, nothing staged by it
    std::vector<uint8_t> delta;
    const Plan plan = h.plan();
    delta.resize(plan.bytes);
    h.pack(plan, delta.data());   // what the query's sync does first
    const std::vector<float> posBefore = h.mirrorPos(), cenBefore = h.mirrorCentres();
    const float got[12] = {101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112};
    h.correctionApplied(&k.c, P, got);
    std::vector<float> wantPos = posBefore, wantCen = cenBefore;
    for (size_t j = 0; j < 4; j++) memcpy(&wantPos[3 * (size_t)P.slot[j]], got + 3 * j, 12);
    for (int j = 0; j < 2; j++) for (int a = 0; a < 3; a++) wantCen[3 * (size_t)k.kf[(size_t)j] + a] = 0.5f;
    ok = h.mirrorPos() == wantPos && h.mirrorCentres() == wantCen && !h.dirty() && wantPos[3] == 4.f && wantCen[3] == 1.f && wantCen[0] == 0.5f;
    expect("the mirror after applying a result", ok, e, nullptr);
  }
  {
    Call k;   // n == 0 with centres is well formed; so is a call with no keyframes, where every good entry is NOT_COVERED
    k.c.n = 0; k.c.slots = nullptr; k.c.corrector = nullptr; k.c.pos_out = nullptr; k.c.status = nullptr;
    bool ok = h.planCorrection(&k.c, P, e) && P.status.empty() && P.slot.empty();
    Call z;
    z.c.n_kf = 0; z.c.kf_slots = nullptr; z.c.before = nullptr; z.c.after = nullptr; z.c.centre_after = nullptr; z.c.centres = YDORB_MAPCORR_RESIDENT;
    z.corrector = {-1, -1};
    ok = ok && h.planCorrection(&z.c, P, e) && P.status == std::vector<uint8_t>({YDORB_MAPCORR_NOT_COVERED, YDORB_MAPCORR_NOT_COVERED});
    expect("n == 0 with centres; no keyframes", ok, e, nullptr);
  }
  printf("%d failed\n", g_failed);
  return g_failed;
}
