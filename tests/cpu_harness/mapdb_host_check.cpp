// Stand-alone check of ydorbslam_amd/csrc/mapdb_host.h (no HIP, no GPU): the resident map table's validation, coalescing, delta
// packing and pool policy, with every packed delta executed on host arrays by the header's own apply / repack.
// tests/test_mapdb_cpu.py builds it with -fsanitize=address,undefined and runs it as its own process.
//   mapdb_host_check [ops.txt]
// Part 1 prints one line per case.  Part 2 drives a seeded sequence of operations against a naive model (a vector of per-slot records,
// re-flattened from scratch): after every sync the host-applied table, exported flat, must equal the model's.  It prints one "trace"
// line of counters per round and asserts that the sequence met a repack that kept the capacity, one that grew it, a point-table growth
// and a keyframe-table growth.  With ops.txt given it also writes every operation there, floats as their bit patterns:
//   C n / n lines "slot x y z"          set_centres
//   P n / n lines "slot bad ref_kf ref_level x y z len kf[len] level[len]"   set_points
//   X n / n lines "slot x y z"          set_positions
//   S / the trace line                  sync, then the counters that follow it
// tests/test_mapdb_gpu.py replays that file through the real handle and holds ydorb_mapdb_stats to the same trace.
// The exit status is the number of failed cases.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/mapdb_host.h"

constexpr int kNameWidth = 52;
#include "check_common.h"

using namespace ydorb::mapdb;

static FILE* g_ops = nullptr;

static int32_t bits(float f) { int32_t b; memcpy(&b, &f, 4); return b; }

struct Db {   // the handle without a device: the Host and the arrays the kernels would hold
  Host host;
  HostTables T;
  std::vector<uint8_t> delta;
  Plan last;
  Db(int32_t pc, int32_t kc, int64_t oc) : host(pc, kc, oc) {}
  void sync() { syncOnHost(host, last, delta, [this](const Plan& P, const uint8_t* d) { execute(P, d, T); }); }
  YdMapDbStats stats() const { YdMapDbStats s; host.stats(s); return s; }
};

struct PointIn {   // the arguments of one set_points call, built point by point
  std::vector<int32_t> slots, start{0}, kf, refKf;
  std::vector<uint8_t> level, bad, refLevel;
  std::vector<float> pos;
  void add(int32_t slot, const std::vector<int32_t>& k, const std::vector<uint8_t>& l, int b, int32_t rk, int rl, float x, float y, float z) {
    slots.push_back(slot); kf.insert(kf.end(), k.begin(), k.end()); level.insert(level.end(), l.begin(), l.end());
    start.push_back((int32_t)kf.size()); bad.push_back((uint8_t)b); refKf.push_back(rk); refLevel.push_back((uint8_t)rl);
    pos.push_back(x); pos.push_back(y); pos.push_back(z);
  }
  bool set(Host& h, std::string& e) const {
    return h.setPoints(slots.data(), (int32_t)slots.size(), start.data(), kf.data(), level.data(), bad.data(), refKf.data(), refLevel.data(), pos.data(), e);
  }
};

static void centres(Host& h, int32_t n) {
  std::vector<int32_t> s((size_t)n);
  std::vector<float> c(3 * (size_t)n, 0.5f);
  for (int32_t i = 0; i < n; i++) s[(size_t)i] = i;
  std::string e;
  h.setCentres(s.data(), n, c.data(), e);
}

// --------------------------------------------------------------------------------------------------------------------- part 1
static void cases() {
  std::string e;
  {
    Db d(4, 4, 16);
    centres(d.host, 4);
    PointIn in;
    in.add(0, {0, 1, 2}, {0, 1, 0x82}, 0, 2, 1, 1.f, 2.f, 3.f);
    in.add(2, {3}, {7}, 0, 3, 7, 4.f, 5.f, 6.f);
    expect("set_points: well formed", in.set(d.host, e), e, nullptr);
    d.sync();
    const YdMapDbStats s = d.stats();
    bool ok = s.n_points == 3 && s.n_keyframes == 4 && s.n_observations == 4 && s.pool_used == 4 && s.last_sync_records == 2 + 4;
    ok = ok && d.T.bad[1] == 1 && d.T.start[1] == d.T.end[1];          // slot 1 was never set: bad, no observations
    ok = ok && d.T.end[0] - d.T.start[0] == 3 && d.T.poolLevel[(size_t)d.T.start[0] + 2] == 0x82 && d.T.pos[8] == 6.f;
    expect("a slot never set reads as bad and empty", ok, "", nullptr);
    d.sync();
    expect("nothing dirty: last_sync_bytes == 0", d.stats().last_sync_bytes == 0 && d.stats().last_sync_records == 0, "", nullptr);

    // every validation message
    e.clear(); { PointIn b = in; b.start[0] = 1; expect("obs_start[0] != 0", b.set(d.host, e), e, "obs_start[0] is 1"); }
    e.clear(); { PointIn b = in; b.start[1] = 5; expect("obs_start decreases", b.set(d.host, e), e, "obs_start decreases at 2"); }
    e.clear(); { PointIn b = in; b.kf[1] = 4; expect("obs_kf out of range", b.set(d.host, e), e, "observation 1: keyframe slot 4 outside 0..3"); }
    e.clear(); { PointIn b = in; b.kf[3] = -1; expect("obs_kf negative", b.set(d.host, e), e, "observation 3: keyframe slot -1"); }
    e.clear(); { PointIn b = in; b.refKf[1] = 4; expect("ref_kf out of range", b.set(d.host, e), e, "point 1: reference keyframe slot 4 outside 0..3"); }
    e.clear(); { PointIn b = in; b.slots[1] = -2; expect("negative point slot", b.set(d.host, e), e, "slots[1]: negative point slot -2"); }
    e.clear();
    expect("null obs_kf", d.host.setPoints(in.slots.data(), 2, in.start.data(), nullptr, in.level.data(), in.bad.data(), in.refKf.data(),
                                           in.refLevel.data(), in.pos.data(), e), e, "null obs_kf");
    e.clear();
    expect("null pos", d.host.setPoints(in.slots.data(), 2, in.start.data(), in.kf.data(), in.level.data(), in.bad.data(), in.refKf.data(),
                                        in.refLevel.data(), nullptr, e), e, "null slots, bad, ref_kf, ref_level or pos");
    e.clear();
    expect("null obs_start", d.host.setPoints(in.slots.data(), 2, nullptr, in.kf.data(), in.level.data(), in.bad.data(), in.refKf.data(),
                                              in.refLevel.data(), in.pos.data(), e), e, "null obs_start");
    e.clear();
    expect("negative n", d.host.setPoints(in.slots.data(), -1, in.start.data(), in.kf.data(), in.level.data(), in.bad.data(), in.refKf.data(),
                                          in.refLevel.data(), in.pos.data(), e), e, "negative number of point slots");
    const int32_t s3[2] = {0, 3}, neg[1] = {-1};
    const float p6[6] = {9, 9, 9, 9, 9, 9};
    e.clear(); expect("set_positions past n_points", d.host.setPositions(s3, 2, p6, e), e, "slots[1]: point slot 3 outside 0..2");
    e.clear(); expect("set_positions null pos", d.host.setPositions(s3, 1, nullptr, e), e, "null slots or pos");
    e.clear(); expect("set_centres negative slot", d.host.setCentres(neg, 1, p6, e), e, "kf_slots[0]: negative keyframe slot -1");
    e.clear(); expect("set_centres null centre", d.host.setCentres(s3, 1, nullptr, e), e, "null kf_slots or centre");
    expect("the rejected calls staged nothing", !d.host.dirty() && d.T.pos[0] == 1.f, "", nullptr);
    // a rejected set_points stages nothing, also when its first points were fine
    {
      PointIn b;
      b.add(1, {0, 1}, {0, 0}, 0, 0, 0, 7.f, 7.f, 7.f);
      b.add(5, {9}, {0}, 0, 0, 0, 7.f, 7.f, 7.f);
      e.clear();
      const bool ok2 = b.set(d.host, e);
      const YdMapDbStats t = d.stats();
      expect("a rejected set_points stages nothing", ok2 || d.host.dirty() || t.n_points != 3 || t.n_observations != 4, e, "observation 2: keyframe slot 9");
    }
    // queries
    float out[16]; uint8_t st[4];
    const float sf[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    const int32_t q[3] = {0, 1, 0};
    e.clear(); expect("query: a slot may repeat, a never-set slot is allowed", d.host.checkNormalDepth(q, 3, sf, 8, out, out, out, st, e), e, nullptr);
    e.clear(); expect("query slot past n_points", d.host.checkNormalDepth(s3, 2, sf, 8, out, out, out, st, e), e, "slots[1]: point slot 3 outside 0..2");
    e.clear(); expect("query n_levels 9", d.host.checkNormalDepth(q, 3, sf, 9, out, out, out, st, e), e, "n_levels 9 outside 1..8");
    e.clear(); expect("query null scale_factors", d.host.checkNormalDepth(q, 3, nullptr, 8, out, out, out, st, e), e, "null scale_factors");
    e.clear(); expect("query null outputs", d.host.checkNormalDepth(q, 3, sf, 8, nullptr, out, out, st, e), e, "null output arrays");
    const int32_t q2[2] = {1, 2};
    e.clear(); expect("ref_level >= n_levels of an updated point", d.host.checkNormalDepth(q2, 2, sf, 7, out, out, out, st, e), e, "slots[1]: reference level 7 of point slot 2 >= n_levels");
    e.clear(); expect("ref_level of a point that is not asked for", d.host.checkNormalDepth(q, 3, sf, 2, out, out, out, st, e), e, nullptr);
    // the lists of the other two queries: map_table.h's checks over the handle's counts
    const YdObservationTable hdr = d.host.counts();
    const int32_t kfq[1] = {4}, ls[2] = {0, 1}, idx[1] = {3}, kf0[1] = {0};
    e.clear(); expect("query_kf out of range", ydorb::maptable::checkLists(&hdr, "query_kf", kfq, 1, ls, idx, e), e, "query_kf[0]: keyframe slot 4 outside 0..3");
    e.clear(); expect("list entry out of range", ydorb::maptable::checkLists(&hdr, "cand_kf", kf0, 1, ls, idx, e), e, "list entry 0: point index 3 outside the table of 3");
    e.clear(); expect("a pool past INT32_MAX entries", checkPoolTotal((int64_t)INT32_MAX + 1, e), e, "2147483648 observations, past INT32_MAX");
    e.clear(); expect("a pool of INT32_MAX entries", checkPoolTotal(INT32_MAX, e), e, nullptr);
  }
  {   // coalescing: one slot set three times, a position before and after: one record, and the pool grows by the last span only
    Db d(8, 4, 64);
    centres(d.host, 4);
    PointIn a; a.add(3, {0, 1, 2, 3}, {0, 0, 0, 0}, 0, 0, 0, 1.f, 1.f, 1.f);
    a.set(d.host, e);
    d.sync();
    const int64_t used = d.stats().pool_used;
    const int32_t s[1] = {3};
    const float early[3] = {2.f, 2.f, 2.f}, late[3] = {5.f, 6.f, 7.f};
    d.host.setPositions(s, 1, early, e);
    PointIn b; b.add(3, {0, 1, 2, 3, 0, 1, 2}, {1, 1, 1, 1, 1, 1, 1}, 0, 1, 1, 3.f, 3.f, 3.f); b.set(d.host, e);
    PointIn c; c.add(3, {}, {}, 1, 0, 0, 3.f, 3.f, 3.f); c.set(d.host, e);
    PointIn f; f.add(3, {2, 1}, {0x83, 4}, 0, 2, 3, 4.f, 4.f, 4.f); f.set(d.host, e);
    d.host.setPositions(s, 1, late, e);
    expect("stats count the staged span", d.stats().n_observations == 2, "", nullptr);
    d.sync();
    const YdMapDbStats t = d.stats();
    bool ok = t.pool_used == used + 2 && t.n_observations == 2 && t.last_sync_records == 1 && d.last.nPointRec == 1 && d.last.nPosRec == 0 && d.last.nPayload == 2;
    ok = ok && d.T.end[3] - d.T.start[3] == 2 && d.T.poolKf[(size_t)d.T.start[3]] == 2 && d.T.poolLevel[(size_t)d.T.start[3]] == 0x83 && d.T.refKf[3] == 2 &&
         d.T.pos[9] == 5.f && d.T.pos[11] == 7.f && d.T.bad[3] == 0;
    expect("coalescing: three sets, the pool grows by the last span", ok, "", nullptr);
    // clear: no points, no keyframes, an empty pool; the capacities stay and a slot of before reads as never set
    const int64_t cap = t.pool_capacity;
    d.host.clear(); d.T.resetPoints();
    const YdMapDbStats z = d.stats();
    ok = z.n_points == 0 && z.n_keyframes == 0 && z.n_observations == 0 && z.pool_used == 0 && z.pool_capacity == cap && !d.host.dirty();
    e.clear();
    ok = ok && !a.set(d.host, e) && e.find("keyframe slot 0 outside 0..-1") != std::string::npos;   // no keyframe is known any more
    centres(d.host, 4);
    PointIn g; g.add(5, {1}, {2}, 0, 1, 2, 8.f, 8.f, 8.f);
    ok = ok && g.set(d.host, e);
    d.sync();
    ok = ok && d.stats().n_points == 6 && d.stats().pool_used == 1 && d.T.bad[3] == 1 && d.T.start[3] == d.T.end[3] && d.T.bad[5] == 0 && d.T.start[5] == 0;
    expect("clear, then reuse", ok, e, nullptr);
  }
  {   // the same three touched spans cost the same bytes in a 100-point and a 10 000-point table
    int64_t bytes[2] = {0, 0};
    for (int t = 0; t < 2; t++) {
      const int32_t n = t ? 10000 : 100;
      Db d(n, 8, (int64_t)n * 8);
      centres(d.host, 8);
      PointIn all;
      for (int32_t p = 0; p < n; p++) all.add(p, {p % 8, (p + 1) % 8, (p + 3) % 8}, {0, 1, 2}, 0, p % 8, 0, 1.f, 2.f, 3.f);
      all.set(d.host, e);
      d.sync();
      PointIn three;
      three.add(7, {0, 1}, {0, 0}, 0, 0, 0, 1.f, 1.f, 1.f); three.add(50, {2, 3, 4, 5, 6}, {0, 0, 0, 0, 0}, 0, 2, 0, 1.f, 1.f, 1.f); three.add(99, {}, {}, 1, 0, 0, 0.f, 0.f, 0.f);
      three.set(d.host, e);
      d.sync();
      bytes[t] = d.stats().last_sync_bytes;
    }
    expect("three touched spans: the same bytes at 100 and 10 000 points", bytes[0] == bytes[1] && bytes[0] > 0 && bytes[0] < 512, "", nullptr);
  }
}

// --------------------------------------------------------------------------------------------------------------------- part 2
struct ModelPoint {
  bool set = false;
  int bad = 1, refLevel = 0;
  int32_t refKf = 0;
  float pos[3] = {0, 0, 0};
  std::vector<int32_t> kf;
  std::vector<uint8_t> level;
};

struct Sequence {
  std::mt19937 rng{20261020u};
  Db d{640, 48, 4096};
  std::vector<ModelPoint> pts;
  std::vector<float> centre;
  int32_t nKf = 0;
  int mismatches = 0;

  uint32_t below(uint32_t n) { return (uint32_t)(rng() % n); }
  float coord() { return (float)((int)below(20001) - 10000) / 1024.f; }

  void setCentres(const std::vector<int32_t>& slots) {
    std::vector<float> c;
    for (const int32_t s : slots) {
      if (s >= nKf) { nKf = s + 1; centre.resize(3 * (size_t)nKf, 0.f); }
      for (int r = 0; r < 3; r++) { centre[3 * (size_t)s + (size_t)r] = coord(); c.push_back(centre[3 * (size_t)s + (size_t)r]); }
    }
    std::string e;
    if (!d.host.setCentres(slots.data(), (int32_t)slots.size(), c.data(), e)) { printf("set_centres refused: %s FAILED\n", e.c_str()); g_failed++; }
    if (g_ops) {
      fprintf(g_ops, "C %zu\n", slots.size());
      for (size_t i = 0; i < slots.size(); i++) fprintf(g_ops, "%d %d %d %d\n", slots[i], bits(c[3 * i]), bits(c[3 * i + 1]), bits(c[3 * i + 2]));
    }
  }
  // a fresh record for `slot` with `len` observers (distinct keyframes, shuffled)
  void redraw(int32_t slot, int len, int bad) {
    if ((size_t)slot >= pts.size()) pts.resize((size_t)slot + 1);
    ModelPoint& m = pts[(size_t)slot];
    m.set = true; m.bad = bad; m.kf.clear(); m.level.clear();
    len = std::min(len, (int)nKf);
    std::vector<int32_t> pool((size_t)nKf);
    for (int32_t k = 0; k < nKf; k++) pool[(size_t)k] = k;
    for (int i = 0; i < len; i++) {
      const size_t j = (size_t)i + below((uint32_t)(nKf - i));
      std::swap(pool[(size_t)i], pool[j]);
      m.kf.push_back(pool[(size_t)i]);
      m.level.push_back((uint8_t)(below(8) | (below(2) ? 0x80u : 0u)));
    }
    const size_t at = len ? below((uint32_t)len) : 0;
    m.refKf = len ? m.kf[at] : 0; m.refLevel = len ? (m.level[at] & 0x7f) : 0;
    for (float& v : m.pos) v = coord();
  }
  // set_points: mention() adds the model's record of `slot` as it is now, sendPoints() makes the one call.  A slot mentioned again after
  // a redraw travels twice with different records: the table must end with the last.
  PointIn pend;
  std::string pendOps;
  void mention(int32_t s) {
    const ModelPoint& m = pts[(size_t)s];
    pend.add(s, m.kf, m.level, m.bad, m.refKf, m.refLevel, m.pos[0], m.pos[1], m.pos[2]);
    char head[160];
    snprintf(head, sizeof(head), "%d %d %d %d %d %d %d %zu", s, m.bad, m.refKf, m.refLevel, bits(m.pos[0]), bits(m.pos[1]), bits(m.pos[2]), m.kf.size());
    pendOps += head;
    for (const int32_t k : m.kf) pendOps += " " + std::to_string(k);
    for (const uint8_t l : m.level) pendOps += " " + std::to_string((int)l);
    pendOps += "\n";
  }
  void sendPoints() {
    std::string e;
    if (!pend.set(d.host, e)) { printf("set_points refused: %s FAILED\n", e.c_str()); g_failed++; }
    if (g_ops) fprintf(g_ops, "P %zu\n%s", pend.slots.size(), pendOps.c_str());
    pend = PointIn();
    pendOps.clear();
  }
  void setPositions(const std::vector<int32_t>& slots) {
    std::vector<float> p;
    for (const int32_t s : slots) for (float& v : pts[(size_t)s].pos) { v = coord(); p.push_back(v); }
    std::string e;
    if (!d.host.setPositions(slots.data(), (int32_t)slots.size(), p.data(), e)) { printf("set_positions refused: %s FAILED\n", e.c_str()); g_failed++; }
    if (g_ops) {
      fprintf(g_ops, "X %zu\n", slots.size());
      for (size_t i = 0; i < slots.size(); i++) fprintf(g_ops, "%d %d %d %d\n", slots[i], bits(p[3 * i]), bits(p[3 * i + 1]), bits(p[3 * i + 2]));
    }
  }
  // sync, then: the host-applied table exported flat == the model re-flattened from scratch
  void syncAndCompare(int round) {
    d.sync();
    const int32_t n = (int32_t)pts.size();
    std::vector<int32_t> wantStart{0}, wantKf, gotStart((size_t)n + 1), gotKf;
    std::vector<uint8_t> wantLevel, gotLevel;
    for (const ModelPoint& m : pts) {
      wantKf.insert(wantKf.end(), m.kf.begin(), m.kf.end()); wantLevel.insert(wantLevel.end(), m.level.begin(), m.level.end());
      wantStart.push_back((int32_t)wantKf.size());
    }
    const YdMapDbStats s = d.stats();
    bool same = s.n_points == n && s.n_keyframes == nKf && s.n_observations == (int64_t)wantKf.size();
    if (same) {
      gotKf.resize(wantKf.size() + 1); gotLevel.resize(wantKf.size() + 1);
      flatten(n, d.T.start.data(), d.T.end.data(), d.T.poolKf.data(), d.T.poolLevel.data(), gotStart.data(), gotKf.data(), gotLevel.data());
      gotKf.pop_back(); gotLevel.pop_back();
      same = gotStart == wantStart && gotKf == wantKf && gotLevel == wantLevel;
      for (int32_t p = 0; same && p < n; p++) {
        const ModelPoint& m = pts[(size_t)p];
        same = d.T.bad[(size_t)p] == m.bad && d.T.refKf[(size_t)p] == m.refKf && d.T.refLevel[(size_t)p] == m.refLevel &&
               memcmp(&d.T.pos[3 * (size_t)p], m.pos, 12) == 0;
      }
      same = same && memcmp(d.T.centre.data(), centre.data(), 12 * (size_t)nKf) == 0;
      same = same && s.n_observations <= s.pool_used && s.pool_used <= s.pool_capacity;
    }
    if (!same) mismatches++;
    char line[256];
    snprintf(line, sizeof(line), "trace %d %d %d %lld %lld %lld %d %d %d %d %d %d %lld %lld", round, s.n_points, s.n_keyframes, (long long)s.n_observations,
             (long long)s.pool_used, (long long)s.pool_capacity, s.repacks_kept, s.repacks_grown, s.point_table_growths, s.keyframe_table_growths,
             s.point_capacity, s.keyframe_capacity, (long long)s.last_sync_bytes, (long long)s.last_sync_records);
    printf("%s%s\n", line, same ? "" : " MISMATCH");
    if (g_ops) fprintf(g_ops, "S\n%s\n", line);
  }

  void run() {
    std::vector<int32_t> slots;
    for (int32_t k = 0; k < 40; k++) slots.push_back(k);
    setCentres(slots);
    slots.clear();
    for (int32_t p = 0; p < 600; p++) { redraw(p, 1 + (int)below(12), below(50) == 0); mention(p); }
    sendPoints();
    syncAndCompare(0);
    for (int round = 1; round <= 48; round++) {
      const int32_t n = (int32_t)pts.size();
      const int m = 1 + (int)below(50);
      for (int i = 0; i < m; i++) {   // grow, shrink, to empty, flip bad; a slot may come twice: its last record counts
        const int32_t s = (int32_t)below((uint32_t)n);
        const uint32_t how = below(10);
        redraw(s, how == 0 ? 0 : how < 4 ? 1 + (int)below(3) : 1 + (int)below(14), how == 0 || below(12) == 0);
        mention(s);
      }
      if (round == 20) {   // once: about half of all spans go empty (erased points)
        for (int32_t s = 0; s < n; s++) if (below(2)) { redraw(s, 0, 1); mention(s); }
      }
      sendPoints();
      slots.clear();
      for (int i = (int)below(30); i > 0; i--) slots.push_back((int32_t)below((uint32_t)n));
      if (!slots.empty()) setPositions(slots);
      slots.clear();
      for (int i = (int)below(4); i > 0; i--) slots.push_back((int32_t)below((uint32_t)nKf));
      if (round % 5 == 0) for (int i = 1 + (int)below(3); i > 0; i--) slots.push_back(nKf + i - 1);   // past the high-water mark, descending
      if (!slots.empty()) setCentres(slots);
      if (round % 4 == 0) {   // new point slots past the high-water mark, one of them skipped (it stays never set)
        const int32_t first = (int32_t)pts.size() + 1;
        for (int i = 0; i < 30; i++) { redraw(first + i, 1 + (int)below(10), 0); mention(first + i); }
        sendPoints();
      }
      syncAndCompare(round);
    }
    const YdMapDbStats s = d.stats();
    expect("sequence: every sync equals the model", mismatches == 0, "", nullptr);
    expect("sequence: a repack that kept the capacity", s.repacks_kept >= 1, "", nullptr);
    expect("sequence: a repack that grew the capacity", s.repacks_grown >= 1, "", nullptr);
    expect("sequence: a point-table growth", s.point_table_growths >= 1, "", nullptr);
    expect("sequence: a keyframe-table growth", s.keyframe_table_growths >= 1, "", nullptr);
  }
};

int main(int argc, char** argv) {
  if (argc > 1 && !(g_ops = fopen(argv[1], "w"))) { fprintf(stderr, "cannot write %s\n", argv[1]); return 2; }
  cases();
  Sequence().run();
  if (g_ops) fclose(g_ops);
  printf("%d failed\n", g_failed);
  return g_failed;
}
