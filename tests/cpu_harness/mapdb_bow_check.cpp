// Stand-alone check of ydorbslam_amd/csrc/mapdb_bow_host.h (no HIP, no GPU): the validation of the resident table's BoW feature
// vectors, coalescing, erase, clear, delta packing and the pool policy, with every packed delta executed on host arrays as the plain
// span kernels execute it (executeRows over the two-int element).
// tests/test_mapdb_tri_cpu.py builds it with -fsanitize=address,undefined and runs it as its own process.
//   mapdb_bow_check [ops.txt]
// Part 1 prints one line per case: the case names are the rules.  Part 2 drives a seeded sequence of set / erase / clear against a
// naive model (a vector of pair lists): after every sync the host-applied arrays, exported flat, must equal the model's.  It prints
// one "trace" line of counters per round.  With ops.txt given it also writes every operation there:
//   B n / n lines "kf len node feat node feat ..."   set_keyframe_bow
//   C                                                clear
//   S / the trace line                               sync, then the counters that follow it
// tests/test_mapdb_tri_gpu.py replays that file through the real handle and holds ydorb_mapdb_bow_stats to the same trace.
// The exit status is the number of failed cases.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/mapdb_bow_host.h"

constexpr int kNameWidth = 72;
#include "check_common.h"

using namespace ydorb::mapdb;

static FILE* g_ops = nullptr;

constexpr int32_t kKeyframes = 16;   // tests/test_mapdb_tri_gpu.py makes its handle with this keyframe capacity

namespace ydorb { namespace mapdb {
static bool operator==(const BowRec& a, const BowRec& b) { return a.node == b.node && a.feat == b.feat; }
} }

struct Db {   // the handle's relation without a device
  BowHost bow;
  BowTables T;
  std::vector<uint8_t> delta;
  RowPlan last;
  int32_t nKf = kKeyframes;
  explicit Db(int32_t kc, bool enable = true) : bow(kc) { if (enable) bow.enable(); }
  void sync() {
    syncOnHost(bow.spans, last, delta, [this](const RowPlan& P, const uint8_t* d) { executeRows(P, d, T); });
  }
  void clear() { bow.clear(); T = BowTables(); }
  YdMapDbBowStats stats() const { YdMapDbBowStats s; bow.stats(s); return s; }
  std::vector<std::vector<BowRec>> vectors() const {
    const int32_t held = bow.spans.nKeyframes();
    std::vector<int32_t> start((size_t)nKf + 1), feat((size_t)bow.spans.liveAfterSync() + 1);
    std::vector<uint32_t> node(feat.size());
    flattenBow(nKf, held, T.rowStart.data(), T.rowLen.data(), T.pool.data(), start.data(), node.data(), feat.data());
    std::vector<std::vector<BowRec>> out((size_t)nKf);
    for (int32_t k = 0; k < nKf; k++)
      for (int32_t q = start[(size_t)k]; q < start[(size_t)k + 1]; q++) out[(size_t)k].push_back(BowRec{(int32_t)node[(size_t)q], feat[(size_t)q]});
    return out;
  }
};

struct BowIn {   // the arguments of one set_keyframe_bow call
  std::vector<int32_t> kf, start{0}, feat;
  std::vector<uint32_t> node;
  void add(int32_t k, const std::vector<BowRec>& v) {
    kf.push_back(k);
    for (const BowRec& r : v) { node.push_back((uint32_t)r.node); feat.push_back(r.feat); }
    start.push_back((int32_t)feat.size());
  }
  bool set(Db& d, std::string& e) const {
    static const uint32_t noNode = 0;
    static const int32_t noFeat = 0;
    const bool ok = d.bow.set(kf.data(), (int32_t)kf.size(), start.data(), node.empty() ? &noNode : node.data(), feat.empty() ? &noFeat : feat.data(), e);
    if (ok) d.nKf = std::max(d.nKf, d.bow.spans.nKeyframes());   // the driver's growKeyframes
    return ok;
  }
};

// a feature vector of n features over about n / 8 nodes: nodes ascending, each feature index once, in a seeded order
static std::vector<BowRec> bowOf(uint32_t seed, int n) {
  std::mt19937 g(seed);
  std::vector<int32_t> feat((size_t)n);
  for (int i = 0; i < n; i++) feat[(size_t)i] = i;
  std::shuffle(feat.begin(), feat.end(), g);
  std::vector<BowRec> out((size_t)n);
  int32_t node = (int32_t)(g() % 50);
  for (int i = 0; i < n; i++) {
    if (g() % 8 == 0) node += 1 + (int32_t)(g() % 1000);
    out[(size_t)i] = BowRec{node, feat[(size_t)i]};
  }
  return out;
}

// --------------------------------------------------------------------------------------------------------------------- part 1
static void cases() {
  std::string e;
  {
    Db off(4, false);
    BowIn a; a.add(0, bowOf(1, 3));
    expect("set before enable", a.set(off, e), e, "keyframe BoW feature vectors are not enabled: call ydorb_mapdb_enable_bow first");
    YdMapDbBowStats s = off.stats();
    expect("a handle that never enables counts nothing", s.enabled == 0 && s.n_entries == 0 && s.pool_used == 0 && s.last_bow_sync_bytes == 0 && !off.bow.dirty(), "", nullptr);
  }
  {
    Db d(4);
    BowIn b;
    b.add(0, bowOf(1, 3));
    b.add(2, bowOf(2, 2));
    e.clear(); expect("set_keyframe_bow: well formed", b.set(d, e), e, nullptr);
    expect("stats count what is staged", d.stats().enabled == 1 && d.stats().n_entries == 5 && d.stats().pool_used == 0, "", nullptr);
    d.sync();
    const YdMapDbBowStats s = d.stats();
    expect("a slot never set has no feature vector", s.n_entries == 5 && s.pool_used == 5 && s.last_bow_sync_records == 2 && d.vectors()[1].empty() &&
           d.vectors()[0] == bowOf(1, 3) && d.vectors()[2] == bowOf(2, 2), "", nullptr);
    expect("delta payload offsets are 16-byte aligned", d.last.oPayload % 16 == 0 && d.last.oHeader % 16 == 0, "", nullptr);
    expect("the delta carries no entry records", d.last.nEntryRec == 0, "", nullptr);
    d.sync();
    expect("nothing staged: last_bow_sync_bytes == 0", d.stats().last_bow_sync_bytes == 0 && d.stats().last_bow_sync_records == 0, "", nullptr);

    // every refusal
    const int32_t one[2] = {0, 1}, k0 = 0, f0 = 0;
    const uint32_t n0 = 0;
    e.clear(); { BowIn x = b; x.start[0] = 1; expect("bow_start[0] != 0", x.set(d, e), e, "bow_start[0] is 1, not 0"); }
    e.clear(); { BowIn x = b; x.start[1] = 6; expect("bow_start decreases", x.set(d, e), e, "bow_start decreases at 2"); }
    e.clear(); { BowIn x = b; x.kf[1] = -3; expect("negative keyframe slot", x.set(d, e), e, "kf_slots[1]: negative keyframe slot -3"); }
    e.clear(); expect("null bow_start", d.bow.set(&k0, 1, nullptr, &n0, &f0, e), e, "null bow_start");
    e.clear(); expect("null kf_slots", d.bow.set(nullptr, 1, one, &n0, &f0, e), e, "null kf_slots");
    e.clear(); expect("null node_id", d.bow.set(&k0, 1, one, nullptr, &f0, e), e, "null node_id or feat");
    e.clear(); expect("null feat", d.bow.set(&k0, 1, one, &n0, nullptr, e), e, "null node_id or feat");
    e.clear(); expect("negative n", d.bow.set(&k0, -1, one, &n0, &f0, e), e, "negative number of keyframe slots: -1");
    e.clear(); { BowIn x; x.add(1, {{5, 0}, {9, 1}, {7, 2}}); expect("node ids that decrease inside a span", x.set(d, e), e, "entry 2: node id 7 after 9, the nodes of a span ascend"); }
    e.clear(); { BowIn x; x.add(0, {{9, 0}}); x.add(1, {{5, 0}}); expect("node ids may fall from one span to the next", x.set(d, e), e, nullptr); BowIn r; r.add(0, bowOf(1, 3)); r.add(1, {}); r.set(d, e); }
    e.clear(); { BowIn x = b; x.node[3] = 0x80000000u; x.node[4] = 0x80000001u; expect("a node id of 2^31", x.set(d, e), e, "entry 3: node id 2147483648 outside 0..2147483647"); }
    e.clear(); { BowIn x; x.add(1, {{0x7fffffff, 0}}); expect("the largest node id, 2^31 - 1", x.set(d, e), e, nullptr); BowIn r; r.add(1, {}); r.set(d, e); }
    e.clear(); { BowIn x = b; x.feat[1] = 65535; expect("a feature index of 65535", x.set(d, e), e, "entry 1: feature index 65535 outside 0..65534"); }
    e.clear(); { BowIn x = b; x.feat[4] = -1; expect("a feature index of -1", x.set(d, e), e, "entry 4: feature index -1 outside 0..65534"); }
    e.clear(); { BowIn x; x.add(1, {{3, 4}, {3, 7}, {8, 4}}); expect("a feature index that repeats inside one span", x.set(d, e), e, "entry 2: feature index 4 repeats inside its span"); }
    e.clear(); { BowIn x; x.add(1, {{3, 4}}); x.add(3, {{3, 4}}); expect("a feature index may repeat across spans", x.set(d, e), e, nullptr); BowIn r; r.add(1, {}); r.add(3, {}); r.set(d, e); }
    e.clear(); {
      std::vector<BowRec> big(65536);
      for (int i = 0; i < 65536; i++) big[(size_t)i] = BowRec{i / 9, i % 65535};
      BowIn x; x.add(1, big);
      expect("a span longer than 65 535", x.set(d, e), e, "kf_slots[0]: a span of 65536 entries, more than 65535");
      big.pop_back();
      BowIn y; y.add(1, big);
      e.clear(); expect("a span of 65 535", y.set(d, e), e, nullptr);
      BowIn z; z.add(1, {}); z.set(d, e);
    }
    e.clear(); expect("a pool past INT32_MAX entries", checkBowPoolTotal((int64_t)INT32_MAX + 1, e), e, "the BoW pool would hold 2147483648 entries, past INT32_MAX");
    e.clear(); expect("a pool of INT32_MAX entries", checkBowPoolTotal(INT32_MAX, e), e, nullptr);
    d.sync();
    expect("the refused calls staged nothing", d.stats().n_entries == 5 && d.vectors()[0] == bowOf(1, 3) && d.vectors()[2] == bowOf(2, 2) && d.vectors()[1].empty(), "", nullptr);
    // a call whose second span is malformed stages nothing of its first either
    e.clear(); { BowIn x; x.add(0, bowOf(9, 1)); x.add(-1, bowOf(9, 1)); expect("a refused set_keyframe_bow stages nothing", x.set(d, e), e, "kf_slots[1]"); }
    e.clear(); { BowIn x; x.add(0, bowOf(9, 1)); x.add(1, bowOf(9, 2)); x.feat[2] = 70000; expect("... nor when a later entry is malformed", x.set(d, e), e, "entry 2: feature index 70000"); }
    expect("... and nothing is dirty", !d.bow.dirty(), "", nullptr);
    d.sync();
    expect("... and the relation is what it was", d.stats().last_bow_sync_bytes == 0 && d.vectors()[0] == bowOf(1, 3), "", nullptr);
  }
  {   // coalescing, erase, clear
    Db d(8);
    BowIn a; a.add(3, bowOf(3, 4)); a.set(d, e); d.sync();
    BowIn b; b.add(3, bowOf(4, 2)); b.set(d, e);
    BowIn c; c.add(3, bowOf(5, 9)); c.set(d, e);
    BowIn f; f.add(3, bowOf(6, 5)); f.set(d, e);
    d.sync();
    expect("coalescing: a vector set three times costs the last span only", d.stats().n_entries == 5 && d.last.nHeaderRec == 1 && d.last.nPayload == 5 &&
           d.stats().last_bow_sync_records == 1 && d.vectors()[3] == bowOf(6, 5), "", nullptr);
    BowIn v; v.add(2, bowOf(7, 3)); v.add(2, bowOf(8, 2)); v.set(d, e);
    d.sync();
    expect("coalescing: a slot named twice in one call keeps its last span", d.last.nHeaderRec == 1 && d.last.nPayload == 2 && d.vectors()[2] == bowOf(8, 2), "", nullptr);
    BowIn z; z.add(3, {}); z.set(d, e);
    d.sync();
    expect("a span of length 0 erases the feature vector", d.vectors()[3].empty() && d.stats().n_entries == 2 && d.T.rowLen[3] == 0, "", nullptr);
    const YdMapDbBowStats before = d.stats();
    d.clear();
    const YdMapDbBowStats after = d.stats();
    expect("clear empties the relation and keeps capacities and counters", after.enabled == 1 && after.n_entries == 0 && after.pool_used == 0 &&
           after.pool_capacity == before.pool_capacity && after.repacks_grown == before.repacks_grown && !d.bow.dirty(), "", nullptr);
    BowIn r; r.add(1, bowOf(7, 2)); r.set(d, e);
    d.sync();
    expect("clear, then reuse", d.vectors()[1] == bowOf(7, 2) && d.stats().pool_used == 2, "", nullptr);
  }
}

// --------------------------------------------------------------------------------------------------------------------- part 2
static void writeOps(const BowIn& f) {
  if (!g_ops || f.kf.empty()) return;
  fprintf(g_ops, "B %zu\n", f.kf.size());
  for (size_t i = 0; i < f.kf.size(); i++) {
    fprintf(g_ops, "%d %d", f.kf[i], f.start[i + 1] - f.start[i]);
    for (int32_t q = f.start[i]; q < f.start[i + 1]; q++) fprintf(g_ops, " %u %d", f.node[(size_t)q], f.feat[(size_t)q]);
    fprintf(g_ops, "\n");
  }
}

static void sequence() {
  std::mt19937 rng(20250212);
  auto uni = [&rng](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
  Db d(kKeyframes);
  std::string e;
  std::vector<std::vector<BowRec>> model((size_t)kKeyframes);
  int32_t liveKf = 12;
  uint32_t seed = 100;
  bool allEqual = true;
  for (int round = 0; round < 44; round++) {
    if (round == 30) {   // the map is reset: everything goes, capacities and counters stay, and the keyframes come back below
      d.clear();
      for (auto& v : model) v.clear();
      if (g_ops) fprintf(g_ops, "C\n");
    }
    BowIn f;
    auto setBow = [&](int32_t k, int n) {
      std::vector<BowRec> v = bowOf(seed++, n);
      f.add(k, v);
      if ((size_t)k >= model.size()) model.resize((size_t)k + 1);
      model[(size_t)k] = v;
    };
    if (round == 0 || round == 30) {
      for (int32_t k = 0; k < liveKf; k++) setBow(k, uni(30, 60));
    } else {
      for (int j = 0; j < 2; j++) setBow(uni(0, liveKf - 1), uni(20, 60));   // the same keyframe may be drawn twice: the last wins
      if (round % 6 == 4) setBow(uni(0, liveKf - 1), 0);                      // a keyframe culled
      if (round == 10)                                                        // most keyframes culled at once: the pool is mostly garbage
        for (int32_t k = 0; k < liveKf; k++) if (k % 4 != 0) setBow(k, 0);
      if (round == 24)                                                        // ... and re-added
        for (int32_t k = 0; k < liveKf; k++) if (k % 4 != 0) setBow(k, uni(30, 60));
      if (round % 5 == 2) setBow(liveKf++, uni(30, 60));                      // a new keyframe: past the initial header capacity in time
    }
    if (!f.set(d, e)) { printf("sequence: set_keyframe_bow refused: %s FAILED\n", e.c_str()); g_failed++; return; }
    writeOps(f);
    d.sync();
    auto got = d.vectors();
    got.resize(std::max(got.size(), model.size()));
    model.resize(got.size());
    if (got != model) { allEqual = false; printf("sequence: round %d MISMATCH\n", round); }
    const YdMapDbBowStats s = d.stats();
    char line[320];
    snprintf(line, sizeof(line), "trace %d %lld %lld %lld %d %d %lld %lld", round, (long long)s.n_entries, (long long)s.pool_used, (long long)s.pool_capacity,
             s.repacks_kept, s.repacks_grown, (long long)s.last_bow_sync_bytes, (long long)s.last_bow_sync_records);
    printf("%s\n", line);
    if (g_ops) fprintf(g_ops, "S\n%s\n", line);
  }
  const YdMapDbBowStats s = d.stats();
  expect("sequence: every sync equals the model", allEqual, "", nullptr);
  expect("sequence: a repack that kept the capacity", s.repacks_kept >= 1, "", nullptr);
  expect("sequence: a repack that grew the capacity", s.repacks_grown >= 1, "", nullptr);
  expect("sequence: the headers grew past the initial keyframe capacity", d.bow.spans.hdrCap() > kKeyframes && d.bow.spans.headerGrowths() >= 1, "", nullptr);
}

int main(int argc, char** argv) {
  if (argc > 1) g_ops = fopen(argv[1], "w");
  cases();
  sequence();
  if (g_ops) fclose(g_ops);
  printf("%d failed\n", g_failed);
  return g_failed;
}
