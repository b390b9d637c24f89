// Stand-alone check of ydorbslam_amd/csrc/mapdb_desc_host.h (no HIP, no GPU): the validation of the resident table's descriptor blocks
// and point views, coalescing, delta packing and the pool policy of both, with every packed delta executed on host arrays by
// mapdb_rows_host.h's executeRows, and the host execution of the distinctive-descriptor query against a direct restatement.
// tests/test_mapdb_desc_cpu.py builds it with -fsanitize=address,undefined and runs it as its own process.
//   mapdb_desc_check [ops.txt]
// Part 1 prints one line per case: the case names are the rules.  Part 2 drives a seeded sequence of block and view changes against a
// naive model (a vector of blocks, a vector of view lists): after every sync the host-applied tables, exported flat, must equal the
// model's, and the host query of every point must equal the restatement on rows gathered from the model.  It prints one "trace" line
// of counters per round.  With ops.txt given it also writes every operation there:
//   P n                                     the point table now holds n slots (the new ones not bad, without observations)
//   B n / n lines "kf len hex[len * 64]"    set_keyframe_descriptors
//   V n / n lines "slot m kf idx ..."       set_point_views
//   S / the trace line                      sync, then the counters that follow it
// tests/test_mapdb_desc_gpu.py replays that file through the real handle and holds ydorb_mapdb_desc_stats to the same trace.
// The exit status is the number of failed cases.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../ydorbslam_amd/csrc/mapdb_desc_host.h"

constexpr int kNameWidth = 72;
#include "check_common.h"

using namespace ydorb::mapdb;

static FILE* g_ops = nullptr;

constexpr int32_t kPoints = 200, kKeyframes = 64;   // tests/test_mapdb_desc_gpu.py sets these points and keyframes before the replay

namespace ydorb { namespace mapdb {
static bool operator==(const DescRow& a, const DescRow& b) { return memcmp(a.b, b.b, 32) == 0; }
} }

struct Db {   // the handle's two relations without a device
  DescHost desc;
  ViewTables V;
  BlockTables B;
  std::vector<uint8_t> delta;
  RowPlan lastViews, lastBlocks;
  int32_t nPoints = kPoints, nKf = kKeyframes;
  Db(int32_t pc, int32_t kc) : desc(pc, kc) {}
  void sync() {
    syncOnHost(desc.views, lastViews, delta, [this](const RowPlan& P, const uint8_t* d) { executeRows(P, d, V); });
    syncOnHost(desc.blocks, lastBlocks, delta, [this](const RowPlan& P, const uint8_t* d) { executeRows(P, d, B); });
  }
  YdMapDbDescStats stats() const { YdMapDbDescStats s; desc.stats(s); return s; }
  std::vector<std::vector<std::pair<int32_t, int32_t>>> views() const {
    const int32_t held = desc.views.nKeyframes();
    std::vector<int32_t> start((size_t)nPoints + 1), kf((size_t)desc.views.liveAfterSync() + 1), idx(kf.size());
    flattenViews(nPoints, held, V.rowStart.data(), V.rowLen.data(), V.pool.data(), start.data(), kf.data(), idx.data());
    std::vector<std::vector<std::pair<int32_t, int32_t>>> out((size_t)nPoints);
    for (int32_t p = 0; p < nPoints; p++)
      for (int32_t q = start[(size_t)p]; q < start[(size_t)p + 1]; q++) out[(size_t)p].push_back({kf[(size_t)q], idx[(size_t)q]});
    return out;
  }
  std::vector<std::vector<DescRow>> blocks() const {
    const int32_t held = desc.blocks.nKeyframes();
    std::vector<int32_t> start((size_t)nKf + 1);
    std::vector<DescRow> rows((size_t)desc.blocks.liveAfterSync() + 1);
    flattenRows(nKf, held, B.rowStart.data(), B.rowLen.data(), B.pool.data(), start.data(), rows.data());
    std::vector<std::vector<DescRow>> out((size_t)nKf);
    for (int32_t k = 0; k < nKf; k++) out[(size_t)k].assign(rows.begin() + start[(size_t)k], rows.begin() + start[(size_t)k + 1]);
    return out;
  }
};

struct BlocksIn {   // the arguments of one set_keyframe_descriptors call
  std::vector<int32_t> kf, start{0};
  std::vector<uint8_t> desc;
  void add(int32_t k, const std::vector<DescRow>& rows) {
    kf.push_back(k);
    for (const DescRow& r : rows) desc.insert(desc.end(), r.b, r.b + 32);
    start.push_back((int32_t)(desc.size() / 32));
  }
  bool set(Db& d, std::string& e) const {
    const bool ok = d.desc.setBlocks(kf.data(), (int32_t)kf.size(), start.data(), desc.empty() ? (const uint8_t*)"" : desc.data(), e);
    if (ok) d.nKf = std::max(d.nKf, d.desc.blocks.nKeyframes());   // the driver's growKeyframes
    return ok;
  }
};

struct ViewsIn {   // the arguments of one set_point_views call
  std::vector<int32_t> slot, start{0}, kf, idx;
  void add(int32_t p, const std::vector<std::pair<int32_t, int32_t>>& v) {
    slot.push_back(p);
    for (const auto& kv : v) { kf.push_back(kv.first); idx.push_back(kv.second); }
    start.push_back((int32_t)kf.size());
  }
  bool set(Db& d, std::string& e) const {
    static const int32_t none = 0;
    return d.desc.setViews(slot.data(), (int32_t)slot.size(), start.data(), kf.empty() ? &none : kf.data(), idx.empty() ? &none : idx.data(), d.nPoints, d.nKf, e);
  }
};

static DescRow rowOf(uint32_t seed) {
  DescRow r;
  std::mt19937 g(seed);
  for (int b = 0; b < 32; b++) r.b[b] = (uint8_t)g();
  return r;
}
static std::vector<DescRow> rowsOf(uint32_t seed, int n) {
  std::vector<DescRow> out;
  for (int i = 0; i < n; i++) out.push_back(rowOf(seed * 1000u + (uint32_t)i));
  return out;
}

// The query restated directly, as one would in numpy: D = popcount(rows[:, None] ^ rows[None]), med = sort(D, axis 1)[:, m // 2],
// the first argmin.  Gathers from the model, not from the host tables.
struct Answer { int32_t best = -1, kf = 0, idx = 0; uint8_t status = 0; DescRow row{}; };
static Answer restated(const std::vector<std::pair<int32_t, int32_t>>& views, const std::vector<std::vector<DescRow>>& blocks, bool bad) {
  Answer a;
  if (bad) { a.status = YDORB_MAPDESC_BAD; return a; }
  std::vector<DescRow> rows;
  std::vector<int32_t> at;
  for (size_t v = 0; v < views.size(); v++) {
    const int32_t kf = views[v].first, idx = views[v].second;
    if ((size_t)kf >= blocks.size() || blocks[(size_t)kf].empty()) continue;
    if ((size_t)idx >= blocks[(size_t)kf].size()) { a.status = YDORB_MAPDESC_VIEW_OUT_OF_RANGE; return a; }
    rows.push_back(blocks[(size_t)kf][(size_t)idx]);
    at.push_back((int32_t)v);
  }
  const size_t m = rows.size();
  if (m == 0) { a.status = YDORB_MAPDESC_NO_DESCRIPTORS; return a; }
  std::vector<int> med(m);
  for (size_t i = 0; i < m; i++) {
    std::vector<int> d(m);
    for (size_t j = 0; j < m; j++) {
      int s = 0;
      for (int w = 0; w < 8; w++) { uint32_t x, y; memcpy(&x, rows[i].b + 4 * w, 4); memcpy(&y, rows[j].b + 4 * w, 4); s += __builtin_popcount(x ^ y); }
      d[j] = s;
    }
    std::nth_element(d.begin(), d.begin() + (ptrdiff_t)(m / 2), d.end());
    med[i] = d[m / 2];
  }
  const size_t w = (size_t)(std::min_element(med.begin(), med.end()) - med.begin());   // the first of equal medians
  a.best = at[w]; a.kf = views[(size_t)at[w]].first; a.idx = views[(size_t)at[w]].second; a.row = rows[w]; a.status = YDORB_MAPDESC_UPDATED;
  return a;
}

// the host query of `slots` against the restatement on the model
static bool queryEqualsRestatement(const Db& d, const std::vector<int32_t>& slots, const std::vector<uint8_t>& bad,
                                   const std::vector<std::vector<std::pair<int32_t, int32_t>>>& views, const std::vector<std::vector<DescRow>>& blocks,
                                   int counts[4]) {
  const size_t n = slots.size();
  std::vector<int32_t> best(n), view(2 * n);
  std::vector<uint8_t> desc(32 * n), status(n);
  distinctiveOnHost(d.V, d.B, bad.data(), slots.data(), (int32_t)n, best.data(), view.data(), desc.data(), status.data());
  bool same = true;
  for (size_t q = 0; q < n; q++) {
    const Answer a = restated(views[(size_t)slots[q]], blocks, bad[(size_t)slots[q]] != 0);
    counts[a.status]++;
    same = same && a.status == status[q] && a.best == best[q] && a.kf == view[2 * q] && a.idx == view[2 * q + 1] && memcmp(a.row.b, &desc[32 * q], 32) == 0;
  }
  return same;
}

// --------------------------------------------------------------------------------------------------------------------- part 1
static void cases() {
  std::string e;
  {
    Db d(8, 4);
    BlocksIn b;
    b.add(0, rowsOf(1, 3));
    b.add(2, rowsOf(2, 2));
    expect("set_keyframe_descriptors: well formed", b.set(d, e), e, nullptr);
    ViewsIn v;
    v.add(1, {{0, 2}, {2, 0}});
    v.add(4, {{2, 1}});
    expect("set_point_views: well formed", v.set(d, e), e, nullptr);
    expect("stats count what is staged", d.stats().n_views == 3 && d.stats().n_descriptors == 5 && d.stats().view_pool_used == 0 && d.stats().desc_pool_used == 0, "", nullptr);
    d.sync();
    const YdMapDbDescStats s = d.stats();
    expect("a slot never set has no views and no block", s.n_views == 3 && s.n_descriptors == 5 && s.last_desc_sync_records == 4 && d.views()[0].empty() &&
           d.views()[1] == std::vector<std::pair<int32_t, int32_t>>({{0, 2}, {2, 0}}) && d.blocks()[1].empty() && d.blocks()[2] == rowsOf(2, 2), "", nullptr);
    expect("delta payload offsets are 16-byte aligned", d.lastBlocks.oPayload % 16 == 0 && d.lastViews.oPayload % 16 == 0 && d.lastBlocks.oHeader % 16 == 0, "", nullptr);
    d.sync();
    expect("nothing staged: last_desc_sync_bytes == 0", d.stats().last_desc_sync_bytes == 0 && d.stats().last_desc_sync_records == 0, "", nullptr);

    // every validation message
    const int32_t one[2] = {0, 1}, k0 = 0;
    const uint8_t row[32] = {0};
    e.clear(); { BlocksIn x = b; x.start[0] = 1; expect("desc_start[0] != 0", x.set(d, e), e, "desc_start[0] is 1, not 0"); }
    e.clear(); { BlocksIn x = b; x.start[1] = 6; expect("desc_start decreases", x.set(d, e), e, "desc_start decreases at 2"); }
    e.clear(); { BlocksIn x = b; x.kf[1] = -3; expect("negative keyframe slot", x.set(d, e), e, "kf_slots[1]: negative keyframe slot -3"); }
    e.clear(); expect("null desc_start", d.desc.setBlocks(&k0, 1, nullptr, row, e), e, "null desc_start");
    e.clear(); expect("null kf_slots", d.desc.setBlocks(nullptr, 1, one, row, e), e, "null kf_slots");
    e.clear(); expect("null desc", d.desc.setBlocks(&k0, 1, one, nullptr, e), e, "null desc");
    e.clear(); expect("blocks: negative n", d.desc.setBlocks(&k0, -1, one, row, e), e, "negative number of keyframe slots: -1");
    e.clear(); { ViewsIn x = v; x.start[0] = 2; expect("view_start[0] != 0", x.set(d, e), e, "view_start[0] is 2, not 0"); }
    e.clear(); { ViewsIn x = v; x.start[1] = 4; expect("view_start decreases", x.set(d, e), e, "view_start decreases at 2"); }
    e.clear(); { ViewsIn x = v; x.slot[1] = -2; expect("negative point slot", x.set(d, e), e, "slots[1]: negative point slot -2"); }
    e.clear(); { ViewsIn x = v; x.slot[0] = kPoints; expect("point slot past n_points", x.set(d, e), e, "slots[0]: point slot 200 outside 0..199; set the point before its views"); }
    e.clear(); { ViewsIn x = v; x.kf[2] = kKeyframes; expect("view_kf past n_keyframes", x.set(d, e), e, "view 2: keyframe slot 64 outside 0..63"); }
    e.clear(); { ViewsIn x = v; x.kf[0] = -1; expect("view_kf negative", x.set(d, e), e, "view 0: keyframe slot -1 outside 0..63"); }
    e.clear(); { ViewsIn x = v; x.idx[1] = -1; expect("view_idx negative", x.set(d, e), e, "view 1: negative keypoint index -1"); }
    e.clear(); {
      ViewsIn x;
      x.add(3, std::vector<std::pair<int32_t, int32_t>>(65536, {0, 0}));
      expect("a view span longer than 65 535", x.set(d, e), e, "slots[0]: a span of 65536 views, more than 65535");
      ViewsIn y;
      y.add(3, std::vector<std::pair<int32_t, int32_t>>(65535, {0, 0}));
      e.clear(); expect("a view span of 65 535", y.set(d, e), e, nullptr);
      ViewsIn z; z.add(3, {}); z.set(d, e);
    }
    e.clear(); expect("null view_start", d.desc.setViews(&k0, 1, nullptr, &k0, &k0, kPoints, kKeyframes, e), e, "null view_start");
    e.clear(); expect("null slots", d.desc.setViews(nullptr, 1, one, &k0, &k0, kPoints, kKeyframes, e), e, "null slots");
    e.clear(); expect("null view_kf", d.desc.setViews(&k0, 1, one, nullptr, &k0, kPoints, kKeyframes, e), e, "null view_kf or view_idx");
    e.clear(); expect("null view_idx", d.desc.setViews(&k0, 1, one, &k0, nullptr, kPoints, kKeyframes, e), e, "null view_kf or view_idx");
    e.clear(); expect("views: negative n", d.desc.setViews(&k0, -2, one, &k0, &k0, kPoints, kKeyframes, e), e, "negative number of point slots: -2");
    e.clear(); expect("a view pool past INT32_MAX entries", checkViewPoolTotal((int64_t)INT32_MAX + 1, e), e, "the view pool would hold 2147483648 entries, past INT32_MAX");
    e.clear(); expect("a descriptor pool past INT32_MAX entries", checkDescPoolTotal((int64_t)INT32_MAX + 1, e), e, "the descriptor pool would hold 2147483648 descriptors, past INT32_MAX");
    e.clear(); expect("a descriptor pool of INT32_MAX entries", checkDescPoolTotal(INT32_MAX, e), e, nullptr);
    int32_t bo[2]; uint8_t so[2], dd[64];
    const int32_t q2[2] = {1, kPoints}, qn[1] = {-1};
    e.clear(); expect("query slot past n_points", DescHost::checkQuery(q2, 2, kPoints, bo, bo, dd, so, e), e, "slots[1]: point slot 200 outside 0..199");
    e.clear(); expect("query slot negative", DescHost::checkQuery(qn, 1, kPoints, bo, bo, dd, so, e), e, "slots[0]: point slot -1 outside 0..199");
    e.clear(); expect("query null slots", DescHost::checkQuery(nullptr, 1, kPoints, bo, bo, dd, so, e), e, "null slots");
    e.clear(); expect("query null outputs with n > 0", DescHost::checkQuery(q2, 1, kPoints, bo, nullptr, dd, so, e), e, "null output arrays");
    e.clear(); expect("query null outputs with n == 0", DescHost::checkQuery(nullptr, 0, kPoints, nullptr, nullptr, nullptr, nullptr, e), e, nullptr);
    e.clear(); expect("query negative n", DescHost::checkQuery(q2, -1, kPoints, bo, bo, dd, so, e), e, "negative number of point slots: -1");
    e.clear(); expect("reserve with a pool in use", d.desc.reserve(64, 64, e), e, "the pools are not empty");
    e.clear(); expect("reserve a negative capacity", d.desc.reserve(-1, 64, e), e, "negative capacity");
    e.clear(); expect("reserve past INT32_MAX", d.desc.reserve((int64_t)1 << 30, 64, e), e, "past INT32_MAX");
    d.sync();
    expect("the rejected calls staged nothing", d.stats().n_views == 3 && d.stats().n_descriptors == 5 && d.views()[4] == std::vector<std::pair<int32_t, int32_t>>({{2, 1}}), "", nullptr);
    // a call whose second span is malformed stages nothing of its first either
    e.clear(); { ViewsIn x; x.add(1, {{0, 0}}); x.add(2, {{kKeyframes + 1, 0}}); expect("a rejected set_point_views stages nothing", x.set(d, e), e, "view 1: keyframe slot 65"); }
    e.clear(); { BlocksIn x; x.add(0, rowsOf(9, 1)); x.add(-1, rowsOf(9, 1)); expect("a rejected set_keyframe_descriptors stages nothing", x.set(d, e), e, "kf_slots[1]"); }
    expect("... and nothing is dirty", !d.desc.dirty(), "", nullptr);
    d.sync();
    expect("... and the relations are what they were", d.stats().last_desc_sync_bytes == 0 && d.views()[1].size() == 2 && d.blocks()[0] == rowsOf(1, 3), "", nullptr);
  }
  {   // coalescing
    Db d(8, 8);
    std::string err;
    expect("reserve on empty pools", d.desc.reserve(64, 64, err), err, nullptr);
    expect("reserve sets the capacities", d.stats().view_pool_capacity == 64 && d.stats().desc_pool_capacity == 64, "", nullptr);
    BlocksIn a; a.add(3, rowsOf(3, 4)); a.set(d, e); d.sync();
    const int64_t used = d.stats().desc_pool_used;
    BlocksIn b; b.add(3, rowsOf(4, 2)); b.set(d, e);
    BlocksIn c; c.add(3, rowsOf(5, 9)); c.set(d, e);
    BlocksIn f; f.add(3, rowsOf(6, 5)); f.set(d, e);
    d.sync();
    expect("coalescing: a block set three times costs the last block only", d.stats().desc_pool_used == used + 5 && d.lastBlocks.nHeaderRec == 1 &&
           d.lastBlocks.nPayload == 5 && d.stats().last_desc_sync_records == 1 && d.blocks()[3] == rowsOf(6, 5), "", nullptr);
    ViewsIn v1; v1.add(2, {{3, 0}, {3, 1}, {3, 2}}); v1.set(d, e);
    ViewsIn v2; v2.add(2, {{3, 4}}); v2.add(2, {{3, 1}, {3, 3}}); v2.set(d, e);
    d.sync();
    expect("coalescing: a slot named twice in one call keeps its last views", d.lastViews.nHeaderRec == 1 && d.lastViews.nPayload == 4 && d.stats().view_pool_used == 2 &&
           d.views()[2] == std::vector<std::pair<int32_t, int32_t>>({{3, 1}, {3, 3}}), "", nullptr);
    BlocksIn z; z.add(3, {}); z.set(d, e);
    ViewsIn y; y.add(2, {}); y.set(d, e);
    d.sync();
    expect("a block of length 0 erases the block", d.blocks()[3].empty() && d.stats().n_descriptors == 0, "", nullptr);
    expect("an empty span erases the views", d.views()[2].empty() && d.stats().n_views == 0, "", nullptr);
    const YdMapDbDescStats before = d.stats();
    d.desc.clear(); d.V = ViewTables(); d.B = BlockTables();
    const YdMapDbDescStats after = d.stats();
    expect("clear empties both and keeps capacities and counters", after.n_views == 0 && after.n_descriptors == 0 && after.view_pool_used == 0 && after.desc_pool_used == 0 &&
           after.view_pool_capacity == before.view_pool_capacity && after.desc_pool_capacity == before.desc_pool_capacity && !d.desc.dirty(), "", nullptr);
    expect("reserve after clear", d.desc.reserve(16, 32, err), err, nullptr);
    BlocksIn r; r.add(1, rowsOf(7, 2)); r.set(d, e);
    ViewsIn w; w.add(0, {{1, 1}}); w.set(d, e);
    d.sync();
    expect("clear, then reuse", d.blocks()[1] == rowsOf(7, 2) && d.views()[0] == std::vector<std::pair<int32_t, int32_t>>({{1, 1}}) && d.stats().desc_pool_used == 2, "", nullptr);
  }
  {   // the host query on cases whose answers are written out here
    Db d(8, 8);
    const DescRow A = rowOf(11), Bv = rowOf(12);
    DescRow A1 = A; A1.b[0] ^= 1;   // one bit from A
    BlocksIn b;
    b.add(0, {A, A1, Bv});
    b.add(1, {Bv, A});
    b.add(3, {A1});
    b.set(d, e);
    ViewsIn v;
    v.add(0, {{2, 0}, {0, 2}, {2, 5}, {0, 0}, {1, 1}, {2, 1}});   // keyframe 2 holds no block: rows Bv A A, the medians 256-ish, 0, 0
    v.add(1, {{2, 0}, {2, 1}});                                   // all skipped
    v.add(2, {{0, 1}, {0, 3}});                                   // idx == len
    v.add(3, {{3, 0}});                                           // one row
    v.add(5, {{0, 0}, {1, 0}});                                   // two rows: kth = 1, both medians d(A, Bv): the first wins
    v.set(d, e);
    d.sync();
    std::vector<uint8_t> bad(kPoints, 0);
    bad[4] = 1;
    const int32_t slots[8] = {0, 1, 2, 3, 4, 5, 6, 0};
    int32_t best[8], view[16];
    uint8_t desc[256], st[8];
    distinctiveOnHost(d.V, d.B, bad.data(), slots, 8, best, view, desc, st);
    expect("host query: best is the span position, skipped views counted", st[0] == 0 && best[0] == 3 && view[0] == 0 && view[1] == 0 && !memcmp(desc, A.b, 32), "", nullptr);
    expect("host query: every view skipped is status 2", st[1] == YDORB_MAPDESC_NO_DESCRIPTORS && best[1] == -1, "", nullptr);
    expect("host query: idx == len is status 3 with zero rows", st[2] == YDORB_MAPDESC_VIEW_OUT_OF_RANGE && best[2] == -1 && desc[64] == 0 && desc[95] == 0, "", nullptr);
    expect("host query: one row wins", st[3] == 0 && best[3] == 0 && view[6] == 3 && !memcmp(desc + 96, A1.b, 32), "", nullptr);
    expect("host query: a bad point is status 1", st[4] == YDORB_MAPDESC_BAD && best[4] == -1, "", nullptr);
    expect("host query: two rows, the first wins", st[5] == 0 && best[5] == 0 && !memcmp(desc + 160, A.b, 32), "", nullptr);
    expect("host query: a point without views is status 2", st[6] == YDORB_MAPDESC_NO_DESCRIPTORS, "", nullptr);
    expect("host query: a repeated slot repeats its answer", st[7] == st[0] && best[7] == best[0] && !memcmp(desc + 224, desc, 32), "", nullptr);
  }
}

// --------------------------------------------------------------------------------------------------------------------- part 2
static void writeOps(const BlocksIn& b, const ViewsIn& v) {
  if (!g_ops) return;
  if (!b.kf.empty()) {
    fprintf(g_ops, "B %zu\n", b.kf.size());
    for (size_t i = 0; i < b.kf.size(); i++) {
      fprintf(g_ops, "%d %d ", b.kf[i], b.start[i + 1] - b.start[i]);
      for (size_t q = 32 * (size_t)b.start[i]; q < 32 * (size_t)b.start[i + 1]; q++) fprintf(g_ops, "%02x", b.desc[q]);
      fprintf(g_ops, "\n");
    }
  }
  if (!v.slot.empty()) {
    fprintf(g_ops, "V %zu\n", v.slot.size());
    for (size_t i = 0; i < v.slot.size(); i++) {
      fprintf(g_ops, "%d %d", v.slot[i], v.start[i + 1] - v.start[i]);
      for (int32_t q = v.start[i]; q < v.start[i + 1]; q++) fprintf(g_ops, " %d %d", v.kf[(size_t)q], v.idx[(size_t)q]);
      fprintf(g_ops, "\n");
    }
  }
}

static void sequence() {
  std::mt19937 rng(20240917);
  auto uni = [&rng](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
  // descriptors from four base rows with a few flipped bits: medians collide often
  DescRow base[4];
  for (int i = 0; i < 4; i++) base[i] = rowOf(77u + (uint32_t)i);
  auto randomBlock = [&](int len) {
    std::vector<DescRow> r((size_t)len);
    for (auto& row : r) {
      row = base[uni(0, 3)];
      for (int f = uni(0, 2); f > 0; f--) row.b[uni(0, 31)] ^= (uint8_t)(1 << uni(0, 7));
    }
    return r;
  };
  Db d(kPoints, kKeyframes);   // tests/test_mapdb_desc_gpu.py: the same capacities
  std::string e;
  if (!d.desc.reserve(256, 512, e)) { printf("sequence: reserve refused: %s FAILED\n", e.c_str()); g_failed++; return; }
  std::vector<std::vector<DescRow>> blocks((size_t)kKeyframes);
  std::vector<std::vector<std::pair<int32_t, int32_t>>> views((size_t)kPoints);
  std::vector<uint8_t> bad;
  auto isBad = [](int32_t p) { return (uint8_t)(p % 11 == 5 ? 1 : 0); };
  for (int32_t p = 0; p < kPoints; p++) bad.push_back(isBad(p));
  if (g_ops) fprintf(g_ops, "P %d\n", kPoints);
  int32_t liveKf = 24;
  auto randomViews = [&](int m) {
    std::vector<std::pair<int32_t, int32_t>> v;
    for (int i = 0; i < m; i++) {
      const int32_t k = uni(0, liveKf + 1);   // now and then a keyframe without a block
      const int32_t len = (size_t)k < blocks.size() ? (int32_t)blocks[(size_t)k].size() : 0;
      v.push_back({k, uni(0, 19) == 0 ? len : uni(0, std::max(len, 1) - 1)});   // now and then idx == len
    }
    return v;
  };
  bool allEqual = true, queriesEqual = true;
  int counts[4] = {0, 0, 0, 0};
  for (int round = 0; round < 40; round++) {
    BlocksIn b;
    ViewsIn v;
    auto setBlock = [&](int32_t k, const std::vector<DescRow>& rows) {
      b.add(k, rows);
      if ((size_t)k >= blocks.size()) blocks.resize((size_t)k + 1);
      blocks[(size_t)k] = rows;
    };
    auto setViews = [&](int32_t p, const std::vector<std::pair<int32_t, int32_t>>& pv) { v.add(p, pv); views[(size_t)p] = pv; };
    if (round == 0) {
      for (int32_t k = 0; k < liveKf; k++) setBlock(k, randomBlock(uni(8, 16)));
      for (int32_t p = 0; p < 120; p++) setViews(p, randomViews(uni(2, 6)));
    } else {
      for (int j = 0; j < 3; j++) setBlock(uni(0, liveKf - 1), randomBlock(uni(6, 18)));   // replaced: views of it may now lie past its length
      if (round % 6 == 4) setBlock(uni(0, liveKf - 1), {});                               // a keyframe culled
      if (round == 10)                                                                    // most keyframes culled at once
        for (int32_t k = 0; k < liveKf; k++) if (k % 4 != 0) setBlock(k, {});
      if (round == 22)                                                                    // ... and re-added
        for (int32_t k = 0; k < liveKf; k++) if (k % 4 != 0) setBlock(k, randomBlock(uni(8, 16)));
      if (round % 5 == 2) {   // a keyframe and points that see it, staged in one interval; the point table grows
        const int32_t k = liveKf++;
        setBlock(k, randomBlock(uni(8, 16)));
        const int32_t first = d.nPoints;
        d.nPoints += 3; views.resize((size_t)d.nPoints);
        for (int32_t p = first; p < d.nPoints; p++) bad.push_back(isBad(p));
        if (g_ops) fprintf(g_ops, "P %d\n", d.nPoints);
        for (int32_t p = first; p < d.nPoints; p++) {
          auto pv = randomViews(uni(1, 4));
          pv.push_back({k, uni(0, (int)blocks[(size_t)k].size() - 1)});
          setViews(p, pv);
        }
      }
      for (int j = 0; j < 20; j++) {   // views replaced; the same point may be drawn twice: the last wins
        const int32_t p = uni(0, d.nPoints - 1);
        setViews(p, j % 7 == 6 ? std::vector<std::pair<int32_t, int32_t>>() : randomViews(uni(1, 7)));
      }
      if (round == 8)                  // most views erased at once: the pool is mostly garbage afterwards
        for (int32_t p = 0; p < d.nPoints; p++) if (p % 4 != 0) setViews(p, {});
      if (round == 30) {               // one point seen very often: past the 64-lane round
        std::vector<std::pair<int32_t, int32_t>> many;
        for (int i = 0; i < 150; i++) { const int32_t k = 4 * uni(0, 5); many.push_back({k, uni(0, std::max((int)blocks[(size_t)k].size(), 1) - 1)}); }
        setViews(8, many);
      }
    }
    if (!b.set(d, e)) { printf("sequence: set_keyframe_descriptors refused: %s FAILED\n", e.c_str()); g_failed++; return; }
    if (!v.set(d, e)) { printf("sequence: set_point_views refused: %s FAILED\n", e.c_str()); g_failed++; return; }
    writeOps(b, v);
    d.sync();
    auto gotBlocks = d.blocks();
    gotBlocks.resize(std::max(gotBlocks.size(), blocks.size()));
    blocks.resize(gotBlocks.size());
    if (d.views() != views || gotBlocks != blocks) { allEqual = false; printf("sequence: round %d MISMATCH\n", round); }
    std::vector<int32_t> all((size_t)d.nPoints);
    for (int32_t p = 0; p < d.nPoints; p++) all[(size_t)p] = p;
    if (!queryEqualsRestatement(d, all, bad, views, blocks, counts)) { queriesEqual = false; printf("sequence: round %d QUERY MISMATCH\n", round); }
    const YdMapDbDescStats s = d.stats();
    char line[320];
    snprintf(line, sizeof(line), "trace %d %lld %lld %lld %lld %lld %lld %d %d %d %d %lld %lld", round, (long long)s.n_views, (long long)s.n_descriptors,
             (long long)s.view_pool_used, (long long)s.view_pool_capacity, (long long)s.desc_pool_used, (long long)s.desc_pool_capacity, s.view_repacks_kept,
             s.view_repacks_grown, s.desc_repacks_kept, s.desc_repacks_grown, (long long)s.last_desc_sync_bytes, (long long)s.last_desc_sync_records);
    printf("%s\n", line);
    if (g_ops) fprintf(g_ops, "S\n%s\n", line);
  }
  const YdMapDbDescStats s = d.stats();
  expect("sequence: every sync equals the model", allEqual, "", nullptr);
  expect("sequence: the host query equals the restatement after every sync", queriesEqual, "", nullptr);
  expect("sequence: the queries met every status", counts[0] > 100 && counts[1] > 100 && counts[2] > 100 && counts[3] > 20,
         std::to_string(counts[0]) + " " + std::to_string(counts[1]) + " " + std::to_string(counts[2]) + " " + std::to_string(counts[3]), nullptr);
  expect("sequence: a view repack that kept the capacity", s.view_repacks_kept >= 1, "", nullptr);
  expect("sequence: a view repack that grew the capacity", s.view_repacks_grown >= 1, "", nullptr);
  expect("sequence: a descriptor repack that kept the capacity", s.desc_repacks_kept >= 1, "", nullptr);
  expect("sequence: a descriptor repack that grew the capacity", s.desc_repacks_grown >= 1, "", nullptr);
}

int main(int argc, char** argv) {
  if (argc > 1) g_ops = fopen(argv[1], "w");
  cases();
  sequence();
  if (g_ops) fclose(g_ops);
  printf("%d failed\n", g_failed);
  return g_failed;
}
