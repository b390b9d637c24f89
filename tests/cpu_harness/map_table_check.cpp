// Stand-alone check of ydorbslam_amd/csrc/map_table.h (no HIP, no GPU): the validation of the map-maintenance entries, the capacity
// bound of a covisibility query and the int32 offsets near INT32_MAX, which are formed from lengths alone (nothing that large is
// allocated).  tests/test_mapmaint_cpu.py builds it with -fsanitize=address,undefined and runs it as its own process.  Prints one line
// per case; the exit status is the number of failed cases.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/map_table.h"

using namespace ydorb::maptable;

static int g_failed = 0;

static void expect(const char* name, bool ok, const std::string& err, const char* needle) {
  const bool pass = needle ? (!ok && err.find(needle) != std::string::npos) : ok;
  printf("%-44s %s%s%s\n", name, pass ? "ok" : "FAILED", err.empty() ? "" : ": ", err.c_str());
  if (!pass) g_failed++;
}

struct Scene {   // 3 points over 4 keyframes: spans {0, 1, 2}, {}, {3, 1}
  std::vector<int32_t> start{0, 3, 3, 5}, kf{0, 1, 2, 3, 1}, refKf{0, 0, 3};
  std::vector<uint8_t> level{0, 1, 0x82, 7, 3}, bad{0, 0, 0}, refLevel{0, 0, 7}, status = std::vector<uint8_t>(3);
  std::vector<float> pos = std::vector<float>(9, 1.f), centre = std::vector<float>(12, 0.f), sf{1.f, 1.2f, 1.44f, 1.7f, 2.f, 2.4f, 2.9f, 3.5f};
  std::vector<float> normal = std::vector<float>(9), mn = std::vector<float>(3), mx = std::vector<float>(3);
  YdObservationTable T{3, 4, nullptr, nullptr, nullptr, nullptr};
  YdObservationTable& table() { T.obs_start = start.data(); T.obs_kf = kf.data(); T.obs_level = level.data(); T.bad = bad.data(); return T; }
  bool normalDepth(std::string& e, int nLevels = 8, int device = 0) {
    return checkNormalDepth(&table(), pos.data(), centre.data(), refKf.data(), refLevel.data(), sf.data(), nLevels, device, normal.data(),
                            mn.data(), mx.data(), status.data(), e);
  }
};

int main() {
  std::string e;
  { Scene s; expect("normal_depth: well formed", s.normalDepth(e), e, nullptr); }
  { Scene s; e.clear(); expect("device 16", s.normalDepth(e, 8, 16), e, "device 16"); }
  { Scene s; e.clear(); expect("device -1", s.normalDepth(e, 8, -1), e, "device -1"); }
  { Scene s; e.clear(); expect("n_levels 0", s.normalDepth(e, 0), e, "n_levels 0"); }
  { Scene s; e.clear(); expect("n_levels 9", s.normalDepth(e, 9), e, "n_levels 9"); }
  { Scene s; e.clear(); s.start[0] = 1; expect("obs_start[0] != 0", s.normalDepth(e), e, "obs_start[0] is 1"); }
  { Scene s; e.clear(); s.start[2] = 2; expect("obs_start decreases", s.normalDepth(e), e, "obs_start decreases at 2"); }
  { Scene s; e.clear(); s.kf[3] = 4; expect("observer slot out of range", s.normalDepth(e), e, "observation 3: keyframe slot 4"); }
  { Scene s; e.clear(); s.kf[0] = -1; expect("observer slot negative", s.normalDepth(e), e, "observation 0: keyframe slot -1"); }
  { Scene s; e.clear(); s.refKf[2] = 4; expect("reference slot out of range", s.normalDepth(e), e, "point 2: reference keyframe slot 4"); }
  { Scene s; e.clear(); expect("reference level >= n_levels", s.normalDepth(e, 7), e, "point 2: reference level 7 >= n_levels 7"); }
  { Scene s; e.clear(); s.refKf[1] = 99; s.refLevel[1] = 99; expect("unread reference of an empty point", s.normalDepth(e), e, nullptr); }
  { Scene s; e.clear(); s.bad[2] = 1; s.refKf[2] = 99; expect("unread reference of a bad point", s.normalDepth(e), e, nullptr); }
  {
    Scene s; e.clear();
    const bool ok = checkNormalDepth(&s.table(), nullptr, s.centre.data(), s.refKf.data(), s.refLevel.data(), s.sf.data(), 8, 0, s.normal.data(),
                                     s.mn.data(), s.mx.data(), s.status.data(), e);
    expect("null pos", ok, e, "null pos");
  }
  { e.clear(); expect("null table", checkTable(nullptr, e), e, "null table"); }
  { Scene s; e.clear(); s.table(); s.T.obs_kf = nullptr; expect("null obs_kf", checkTable(&s.T, e), e, "null obs_kf"); }
  { Scene s; e.clear(); s.table(); s.T.bad = nullptr; expect("null bad", checkTable(&s.T, e), e, "null bad"); }

  // lists: two queries over the scene
  std::vector<int32_t> slot{1, 3}, ls{0, 2, 3}, idx{0, 2, 0}, os{0, 3, 6}, conn(6), w(6), cnt(2);
  std::vector<uint8_t> st(2), own{0, 1, 2}, cull(2);
  auto covis = [&](Scene& s, std::string& err) {
    return checkCovisibility(&s.table(), slot.data(), 2, ls.data(), idx.data(), os.data(), 0, conn.data(), w.data(), cnt.data(), st.data(), err);
  };
  { Scene s; e.clear(); expect("covisibility: well formed", covis(s, e), e, nullptr); }
  { Scene s; e.clear(); slot[1] = 4; expect("query slot out of range", covis(s, e), e, "query_kf[1]: keyframe slot 4"); slot[1] = 3; }
  { Scene s; e.clear(); idx[2] = 3; expect("point index out of range", covis(s, e), e, "list entry 2: point index 3"); idx[2] = 0; }
  { Scene s; e.clear(); ls[1] = 4; expect("list_start decreases", covis(s, e), e, "list_start decreases at 2"); ls[1] = 2; }
  { Scene s; e.clear(); os[0] = 2; expect("out_start[0] != 0", covis(s, e), e, "out_start[0] is 2"); os[0] = 0; }
  {
    Scene s; e.clear();
    const bool ok = checkCovisibility(&s.table(), slot.data(), 2, ls.data(), idx.data(), os.data(), 0, nullptr, w.data(), cnt.data(), st.data(), e);
    expect("null conn_kf", ok, e, "null conn_kf");
  }
  {
    Scene s; e.clear();
    bool ok = checkRedundancy(&s.table(), slot.data(), 2, ls.data(), idx.data(), own.data(), 0, cnt.data(), cnt.data(), cull.data(), e);
    expect("redundancy: well formed", ok, e, nullptr);
    e.clear();
    ok = checkRedundancy(&s.table(), slot.data(), 2, ls.data(), idx.data(), nullptr, 0, cnt.data(), cnt.data(), cull.data(), e);
    expect("null own_level", ok, e, "null own_level");
    e.clear();
    ok = checkRedundancy(&s.table(), nullptr, 2, ls.data(), idx.data(), own.data(), 0, cnt.data(), cnt.data(), cull.data(), e);
    expect("null cand_kf", ok, e, "null cand_kf");
  }

  // the capacity bound: min(n_keyframes - 1, sum of spans), never negative
  {
    bool ok = capacityBound(4, 8) == 3 && capacityBound(4, 2) == 2 && capacityBound(1, 5) == 0 && capacityBound(0, 5) == 0 && capacityBound(4, 0) == 0 &&
              capacityBound(INT32_MAX, (int64_t)INT32_MAX * 4) == INT32_MAX - 1;
    Scene s;
    int32_t out[3];
    e.clear();
    ok = ok && layoutCapacities(&s.table(), 2, ls.data(), idx.data(), out, e) && out[0] == 0 && out[1] == 3 && out[2] == 6;   // spans 3 + 2 -> min(3, 5); 3
    expect("capacity bound and layout", ok, e, nullptr);
  }
  // offsets near INT32_MAX, from lengths alone
  {
    int32_t start[4];
    const int64_t fits[3] = {INT32_MAX - 2, 1, 1}, over[3] = {INT32_MAX - 2, 1, 2}, big[1] = {(int64_t)1 << 40}, neg[2] = {5, -1};
    e.clear();
    bool ok = accumulateStarts(fits, 3, start, e) && start[3] == INT32_MAX && start[1] == INT32_MAX - 2;
    expect("offsets reach INT32_MAX exactly", ok, e, nullptr);
    e.clear(); expect("offset one past INT32_MAX", accumulateStarts(over, 3, start, e), e, "offset 2147483648 after entry 2 passes INT32_MAX");
    e.clear(); expect("one length past 32 bits", accumulateStarts(big, 1, start, e), e, "passes INT32_MAX");
    e.clear(); expect("negative length", accumulateStarts(neg, 2, start, e), e, "length -1 of entry 1 is negative");
  }
  // the verdict's double compare
  {
    const bool ok = cullVerdict(9, 10) == 0 && cullVerdict(10, 10) == 1 && cullVerdict(0, 0) == 0 && cullVerdict(1, 1) == 1 && cullVerdict(91, 100) == 1 &&
                    cullVerdict(90, 100) == 0;
    expect("cull verdict", ok, "", nullptr);
  }
  printf("%d failed\n", g_failed);
  return g_failed;
}
