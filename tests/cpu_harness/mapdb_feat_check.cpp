// Stand-alone check of ydorbslam_amd/csrc/mapdb_feat_host.h (no HIP, no GPU): the validation of the resident table's keyframe
// features, coalescing, erase, delta packing and the pool policy, with every packed delta executed on host arrays in the layout the
// kernels keep (executeFeatures: one span over a keypoint array and a right_x array).
// tests/test_mapdb_fuse_cpu.py builds it with -fsanitize=address,undefined and runs it as its own process.
//   mapdb_feat_check [ops.txt]
// Part 1 prints one line per case: the case names are the rules.  Part 2 drives a seeded sequence of feature changes against a naive
// model (a vector of feature lists): after every sync the host-applied arrays, exported flat, must equal the model's.  It prints one
// "trace" line of counters per round.  With ops.txt given it also writes every operation there:
//   F n r / n lines "kf len hex[len * 64]"    set_keyframe_features; r = 0: right_x was NULL; an element is keypoint (28 bytes) + right_x
//   S / the trace line                        sync, then the counters that follow it
// tests/test_mapdb_fuse_gpu.py replays that file through the real handle and holds ydorb_mapdb_feat_stats to the same trace.
// The exit status is the number of failed cases.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/mapdb_feat_host.h"

constexpr int kNameWidth = 72;
#include "check_common.h"

using namespace ydorb::mapdb;

static FILE* g_ops = nullptr;

constexpr int32_t kKeyframes = 16;   // tests/test_mapdb_fuse_gpu.py makes its handle with this keyframe capacity

namespace ydorb { namespace mapdb {
static bool operator==(const FeatRec& a, const FeatRec& b) { return memcmp(&a, &b, sizeof(FeatRec)) == 0; }
} }

struct Db {   // the handle's relation without a device
  FeatHost feat;
  FeatTables T;
  std::vector<uint8_t> delta;
  RowPlan last;
  int32_t nKf = kKeyframes;
  explicit Db(int32_t kc, bool enable = true) : feat(kc) { if (enable) feat.enable(); }
  void sync() {
    syncOnHost(feat.feats, last, delta, [this](const RowPlan& P, const uint8_t* d) { executeFeatures(P, d, T); });
  }
  YdMapDbFeatStats stats() const { YdMapDbFeatStats s; feat.stats(s); return s; }
  std::vector<std::vector<FeatRec>> features() const {
    const int32_t held = feat.feats.nKeyframes();
    std::vector<int32_t> start((size_t)nKf + 1);
    std::vector<YdKeyPoint> kps((size_t)feat.feats.liveAfterSync() + 1);
    std::vector<float> rx(kps.size());
    flattenFeatures(nKf, held, T.start.data(), T.len.data(), T.kps.data(), T.rightX.data(), start.data(), kps.data(), rx.data());
    std::vector<std::vector<FeatRec>> out((size_t)nKf);
    for (int32_t k = 0; k < nKf; k++)
      for (int32_t q = start[(size_t)k]; q < start[(size_t)k + 1]; q++) out[(size_t)k].push_back(FeatRec{kps[(size_t)q], rx[(size_t)q]});
    return out;
  }
};

struct FeatsIn {   // the arguments of one set_keyframe_features call
  std::vector<int32_t> kf, start{0};
  std::vector<YdKeyPoint> kps;
  std::vector<float> rx;
  bool stereo = true;
  void add(int32_t k, const std::vector<FeatRec>& f) {
    kf.push_back(k);
    for (const FeatRec& r : f) { kps.push_back(r.kp); rx.push_back(r.rightX); }
    start.push_back((int32_t)kps.size());
  }
  bool set(Db& d, std::string& e) const {
    static const YdKeyPoint none{};
    const bool ok = d.feat.set(kf.data(), (int32_t)kf.size(), start.data(), kps.empty() ? &none : kps.data(), stereo ? (rx.empty() ? (const float*)&none : rx.data()) : nullptr, e);
    if (ok) d.nKf = std::max(d.nKf, d.feat.feats.nKeyframes());   // the driver's growKeyframes
    return ok;
  }
};

static std::vector<FeatRec> featsOf(uint32_t seed, int n, bool stereo = true) {
  std::mt19937 g(seed);
  std::vector<FeatRec> out((size_t)n);
  for (FeatRec& r : out) {
    r.kp.x = (float)(g() % 64000) / 100.0f; r.kp.y = (float)(g() % 48000) / 100.0f; r.kp.size = 31.0f; r.kp.angle = (float)(g() % 36000) / 100.0f;
    r.kp.response = (float)(g() % 255); r.kp.octave = (int32_t)(g() % 8); r.kp.class_id = -1;
    r.rightX = stereo ? (g() % 3 == 0 ? -1.0f : r.kp.x - (float)(g() % 4000) / 100.0f) : -1.0f;
  }
  return out;
}

// --------------------------------------------------------------------------------------------------------------------- part 1
static void cases() {
  std::string e;
  {
    Db off(4, false);
    FeatsIn a; a.add(0, featsOf(1, 3));
    expect("set before enable", a.set(off, e), e, "keyframe features are not enabled: call ydorb_mapdb_enable_features first");
    YdMapDbFeatStats s = off.stats();
    expect("a handle that never enables counts nothing", s.enabled == 0 && s.n_features == 0 && s.pool_used == 0 && s.last_feat_sync_bytes == 0 && !off.feat.dirty(), "", nullptr);
  }
  {
    Db d(4);
    FeatsIn b;
    b.add(0, featsOf(1, 3));
    b.add(2, featsOf(2, 2));
    e.clear(); expect("set_keyframe_features: well formed", b.set(d, e), e, nullptr);
    expect("stats count what is staged", d.stats().enabled == 1 && d.stats().n_features == 5 && d.stats().pool_used == 0, "", nullptr);
    d.sync();
    const YdMapDbFeatStats s = d.stats();
    expect("a slot never set has no features", s.n_features == 5 && s.pool_used == 5 && s.last_feat_sync_records == 2 && d.features()[1].empty() &&
           d.features()[0] == featsOf(1, 3) && d.features()[2] == featsOf(2, 2), "", nullptr);
    expect("delta payload offsets are 16-byte aligned", d.last.oPayload % 16 == 0 && d.last.oHeader % 16 == 0, "", nullptr);
    expect("one span indexes both arrays", d.T.kps.size() == d.T.rightX.size() && d.T.start[2] == 3 && d.T.len[2] == 2 && d.T.rightX[3] == featsOf(2, 2)[0].rightX &&
           d.T.kps[4].x == featsOf(2, 2)[1].kp.x, "", nullptr);
    d.sync();
    expect("nothing staged: last_feat_sync_bytes == 0", d.stats().last_feat_sync_bytes == 0 && d.stats().last_feat_sync_records == 0, "", nullptr);
    {
      FeatsIn m; m.stereo = false; m.add(3, featsOf(5, 4));
      e.clear(); expect("null right_x is accepted", m.set(d, e), e, nullptr);
      d.sync();
      const std::vector<FeatRec> got = d.features()[3];
      bool all = got.size() == 4;
      for (const FeatRec& r : got) all = all && r.rightX == -1.0f;
      expect("null right_x stores -1 for every feature", all && got[2].kp.x == featsOf(5, 4)[2].kp.x, "", nullptr);
      FeatsIn z; z.add(3, {}); z.set(d, e); d.sync();
    }

    // every validation message
    const int32_t one[2] = {0, 1}, k0 = 0;
    const YdKeyPoint kp{};
    const float rx = 0.f;
    e.clear(); { FeatsIn x = b; x.start[0] = 1; expect("feat_start[0] != 0", x.set(d, e), e, "feat_start[0] is 1, not 0"); }
    e.clear(); { FeatsIn x = b; x.start[1] = 6; expect("feat_start decreases", x.set(d, e), e, "feat_start decreases at 2"); }
    e.clear(); { FeatsIn x = b; x.kf[1] = -3; expect("negative keyframe slot", x.set(d, e), e, "kf_slots[1]: negative keyframe slot -3"); }
    e.clear(); expect("null feat_start", d.feat.set(&k0, 1, nullptr, &kp, &rx, e), e, "null feat_start");
    e.clear(); expect("null kf_slots", d.feat.set(nullptr, 1, one, &kp, &rx, e), e, "null kf_slots");
    e.clear(); expect("null kps", d.feat.set(&k0, 1, one, nullptr, &rx, e), e, "null kps");
    e.clear(); expect("negative n", d.feat.set(&k0, -1, one, &kp, &rx, e), e, "negative number of keyframe slots: -1");
    e.clear(); { FeatsIn x = b; x.kps[4].octave = 8; expect("octave 8", x.set(d, e), e, "feature 4: octave 8 outside 0..7"); }
    e.clear(); { FeatsIn x = b; x.kps[1].octave = -1; expect("octave -1", x.set(d, e), e, "feature 1: octave -1 outside 0..7"); }
    e.clear(); {
      FeatsIn x; x.add(1, std::vector<FeatRec>(65536, featsOf(3, 1)[0]));
      expect("a span longer than 65 535", x.set(d, e), e, "kf_slots[0]: a span of 65536 features, more than 65535");
      FeatsIn y; y.add(1, std::vector<FeatRec>(65535, featsOf(3, 1)[0]));
      e.clear(); expect("a span of 65 535", y.set(d, e), e, nullptr);
      FeatsIn z; z.add(1, {}); z.set(d, e);
    }
    e.clear(); expect("a pool past INT32_MAX features", checkFeatPoolTotal((int64_t)INT32_MAX + 1, e), e, "the feature pool would hold 2147483648 features, past INT32_MAX");
    e.clear(); expect("a pool of INT32_MAX features", checkFeatPoolTotal(INT32_MAX, e), e, nullptr);
    d.sync();
    expect("the rejected calls staged nothing", d.stats().n_features == 5 && d.features()[0] == featsOf(1, 3) && d.features()[2] == featsOf(2, 2) && d.features()[1].empty(), "", nullptr);
    // a call whose second span is malformed stages nothing of its first either
    e.clear(); { FeatsIn x; x.add(0, featsOf(9, 1)); x.add(-1, featsOf(9, 1)); expect("a rejected set_keyframe_features stages nothing", x.set(d, e), e, "kf_slots[1]"); }
    e.clear(); { FeatsIn x; x.add(0, featsOf(9, 1)); x.add(1, featsOf(9, 2)); x.kps[2].octave = 9; expect("... nor when a later feature is malformed", x.set(d, e), e, "feature 2: octave 9"); }
    expect("... and nothing is dirty", !d.feat.dirty(), "", nullptr);
    d.sync();
    expect("... and the relation is what it was", d.stats().last_feat_sync_bytes == 0 && d.features()[0] == featsOf(1, 3), "", nullptr);
  }
  {   // coalescing, erase, clear
    Db d(8);
    FeatsIn a; a.add(3, featsOf(3, 4)); a.set(d, e); d.sync();
    FeatsIn b; b.add(3, featsOf(4, 2)); b.set(d, e);
    FeatsIn c; c.add(3, featsOf(5, 9)); c.set(d, e);
    FeatsIn f; f.add(3, featsOf(6, 5)); f.set(d, e);
    d.sync();
    expect("coalescing: features set three times cost the last span only", d.stats().n_features == 5 && d.last.nHeaderRec == 1 && d.last.nPayload == 5 &&
           d.stats().last_feat_sync_records == 1 && d.features()[3] == featsOf(6, 5), "", nullptr);
    FeatsIn v; v.add(2, featsOf(7, 3)); v.add(2, featsOf(8, 2)); v.set(d, e);
    d.sync();
    expect("coalescing: a slot named twice in one call keeps its last span", d.last.nHeaderRec == 1 && d.last.nPayload == 2 && d.features()[2] == featsOf(8, 2), "", nullptr);
    FeatsIn z; z.add(3, {}); z.set(d, e);
    d.sync();
    expect("a span of length 0 erases the features", d.features()[3].empty() && d.stats().n_features == 2 && d.T.len[3] == 0, "", nullptr);
    const YdMapDbFeatStats before = d.stats();
    d.feat.clear(); d.T = FeatTables();
    const YdMapDbFeatStats after = d.stats();
    expect("clear empties the relation and keeps capacities and counters", after.enabled == 1 && after.n_features == 0 && after.pool_used == 0 &&
           after.pool_capacity == before.pool_capacity && after.repacks_grown == before.repacks_grown && !d.feat.dirty(), "", nullptr);
    FeatsIn r; r.add(1, featsOf(7, 2)); r.set(d, e);
    d.sync();
    expect("clear, then reuse", d.features()[1] == featsOf(7, 2) && d.stats().pool_used == 2, "", nullptr);
  }
}

// --------------------------------------------------------------------------------------------------------------------- part 2
static void writeOps(const FeatsIn& f) {
  if (!g_ops || f.kf.empty()) return;
  fprintf(g_ops, "F %zu %d\n", f.kf.size(), f.stereo ? 1 : 0);
  for (size_t i = 0; i < f.kf.size(); i++) {
    fprintf(g_ops, "%d %d ", f.kf[i], f.start[i + 1] - f.start[i]);
    for (int32_t q = f.start[i]; q < f.start[i + 1]; q++) {
      const FeatRec r{f.kps[(size_t)q], f.stereo ? f.rx[(size_t)q] : -1.0f};
      const uint8_t* b = reinterpret_cast<const uint8_t*>(&r);
      for (size_t j = 0; j < sizeof(FeatRec); j++) fprintf(g_ops, "%02x", b[j]);
    }
    fprintf(g_ops, "\n");
  }
}

static void sequence() {
  std::mt19937 rng(20241105);
  auto uni = [&rng](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
  Db d(kKeyframes);
  std::string e;
  std::vector<std::vector<FeatRec>> model((size_t)kKeyframes);
  int32_t liveKf = 12;
  uint32_t seed = 100;
  bool allEqual = true;
  for (int round = 0; round < 40; round++) {
    FeatsIn f;
    f.stereo = round % 7 != 3;   // now and then a monocular call: right_x NULL
    auto setFeats = [&](int32_t k, int n) {
      std::vector<FeatRec> v = featsOf(seed++, n, f.stereo);
      f.add(k, v);
      if ((size_t)k >= model.size()) model.resize((size_t)k + 1);
      model[(size_t)k] = v;
    };
    if (round == 0) {
      for (int32_t k = 0; k < liveKf; k++) setFeats(k, uni(30, 60));
    } else {
      for (int j = 0; j < 2; j++) setFeats(uni(0, liveKf - 1), uni(20, 60));   // the same keyframe may be drawn twice: the last wins
      if (round % 6 == 4) setFeats(uni(0, liveKf - 1), 0);                      // a keyframe culled
      if (round == 10)                                                          // most keyframes culled at once: the pool is mostly garbage
        for (int32_t k = 0; k < liveKf; k++) if (k % 4 != 0) setFeats(k, 0);
      if (round == 24)                                                          // ... and re-added
        for (int32_t k = 0; k < liveKf; k++) if (k % 4 != 0) setFeats(k, uni(30, 60));
      if (round % 5 == 2) setFeats(liveKf++, uni(30, 60));                      // a new keyframe: past the initial header capacity in time
    }
    if (!f.set(d, e)) { printf("sequence: set_keyframe_features refused: %s FAILED\n", e.c_str()); g_failed++; return; }
    writeOps(f);
    d.sync();
    auto got = d.features();
    got.resize(std::max(got.size(), model.size()));
    model.resize(got.size());
    if (got != model) { allEqual = false; printf("sequence: round %d MISMATCH\n", round); }
    const YdMapDbFeatStats s = d.stats();
    char line[320];
    snprintf(line, sizeof(line), "trace %d %lld %lld %lld %d %d %lld %lld", round, (long long)s.n_features, (long long)s.pool_used, (long long)s.pool_capacity,
             s.repacks_kept, s.repacks_grown, (long long)s.last_feat_sync_bytes, (long long)s.last_feat_sync_records);
    printf("%s\n", line);
    if (g_ops) fprintf(g_ops, "S\n%s\n", line);
  }
  const YdMapDbFeatStats s = d.stats();
  expect("sequence: every sync equals the model", allEqual, "", nullptr);
  expect("sequence: a repack that kept the capacity", s.repacks_kept >= 1, "", nullptr);
  expect("sequence: a repack that grew the capacity", s.repacks_grown >= 1, "", nullptr);
  expect("sequence: the headers grew past the initial keyframe capacity", d.feat.feats.hdrCap() > kKeyframes && d.feat.feats.headerGrowths() >= 1, "", nullptr);
}

int main(int argc, char** argv) {
  if (argc > 1) g_ops = fopen(argv[1], "w");
  cases();
  sequence();
  if (g_ops) fclose(g_ops);
  printf("%d failed\n", g_failed);
  return g_failed;
}
