// Stand-alone check of ydorbslam_amd/csrc/mapdb_rows_host.h (no HIP, no GPU): the keyframe rows' validation, coalescing, delta
// packing and pool policy, with every packed delta executed on host arrays by the header's own executeRows, and of the CPU restatement
// tests/localmap_ref/localmap_ref.cpp on hand-made cases.  tests/test_mapdb_rows_cpu.py builds it with -fsanitize=address,undefined and
// runs it as its own process.
//   mapdb_rows_check [ops.txt]
// Part 1 prints one line per case.  Part 2 drives a seeded sequence of operations from 40 keyframes against a naive model (a vector of
// rows): after every sync the host-applied rows, exported flat, must equal the model's.  It prints one "trace" line of counters per
// round.  With ops.txt given it also writes every operation there:
//   R n / n lines "kf len slot[len]"    set_keyframe_rows
//   E n / n lines "kf idx slot"         set_row_entries
//   S / the trace line                  sync, then the counters that follow it
// tests/test_mapdb_rows_gpu.py replays that file through the real handle and holds ydorb_mapdb_row_stats to the same trace.
// The exit status is the number of failed cases.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/mapdb_rows_host.h"
#include "../localmap_ref/localmap_ref.cpp"

constexpr int kNameWidth = 60;
#include "check_common.h"

using namespace ydorb::mapdb;

static FILE* g_ops = nullptr;

constexpr int32_t kPoints = 500;   // the point table the rows name: slots 0 .. 499 (the GPU replay sets them first)

struct Db {   // the handle's rows without a device
  RowsHost rows;
  RowTables T;
  std::vector<uint8_t> delta;
  RowPlan last;
  Db(int32_t kc, int64_t oc) : rows(kc, oc) {}
  void sync() { syncOnHost(rows, last, delta, [this](const RowPlan& P, const uint8_t* d) { executeRows(P, d, T); }); }
  YdMapDbRowStats stats() const { YdMapDbRowStats s; rows.stats(s); return s; }
  std::vector<std::vector<int32_t>> exported() const {
    const int32_t n = rows.nKeyframes();
    std::vector<int32_t> start((size_t)n + 1), slot((size_t)rows.liveAfterSync() + 1);
    flattenRows(n, n, T.rowStart.data(), T.rowLen.data(), T.pool.data(), start.data(), slot.data());
    std::vector<std::vector<int32_t>> out((size_t)n);
    for (int32_t k = 0; k < n; k++) out[(size_t)k].assign(slot.begin() + start[(size_t)k], slot.begin() + start[(size_t)k + 1]);
    return out;
  }
};

struct RowsIn {   // the arguments of one set_keyframe_rows call
  std::vector<int32_t> kf, start{0}, slot;
  void add(int32_t k, const std::vector<int32_t>& r) { kf.push_back(k); slot.insert(slot.end(), r.begin(), r.end()); start.push_back((int32_t)slot.size()); }
  bool set(RowsHost& h, std::string& e, int32_t nPoints = kPoints) const {
    return h.setRows(kf.data(), (int32_t)kf.size(), start.data(), slot.data(), nPoints, e);
  }
};

static bool entry(RowsHost& h, int32_t k, int32_t i, int32_t v, std::string& e) { return h.setEntries(&k, &i, &v, 1, kPoints, e); }

// --------------------------------------------------------------------------------------------------------------------- part 1
static void cases() {
  std::string e;
  {
    Db d(4, 16);
    RowsIn in;
    in.add(0, {5, -1, 7});
    in.add(2, {1});
    expect("set_keyframe_rows: well formed", in.set(d.rows, e), e, nullptr);
    d.sync();
    const YdMapDbRowStats s = d.stats();
    const auto x = d.exported();
    expect("a keyframe slot never set has length 0", d.rows.nKeyframes() == 3 && s.n_entries == 4 && s.pool_used == 4 && s.last_row_sync_records == 2 &&
           x[0] == std::vector<int32_t>({5, -1, 7}) && x[1].empty() && x[2] == std::vector<int32_t>({1}), "", nullptr);
    d.sync();
    expect("nothing dirty: last_row_sync_bytes == 0", d.stats().last_row_sync_bytes == 0 && d.stats().last_row_sync_records == 0, "", nullptr);

    // every validation message
    e.clear(); { RowsIn b = in; b.start[0] = 1; expect("row_start[0] != 0", b.set(d.rows, e), e, "row_start[0] is 1, not 0"); }
    e.clear(); { RowsIn b = in; b.start[1] = 5; expect("row_start decreases", b.set(d.rows, e), e, "row_start decreases at 2"); }
    e.clear(); { RowsIn b = in; b.kf[1] = -3; expect("negative keyframe slot", b.set(d.rows, e), e, "kf_slots[1]: negative keyframe slot -3"); }
    e.clear(); { RowsIn b = in; b.slot[2] = kPoints; expect("point slot past n_points", b.set(d.rows, e), e, "row entry 2: point slot 500 outside -1..499; set the point before a row names it"); }
    e.clear(); { RowsIn b = in; b.slot[0] = -2; expect("point slot below -1", b.set(d.rows, e), e, "row entry 0: point slot -2 outside -1..499"); }
    e.clear(); expect("null row_start", d.rows.setRows(in.kf.data(), 2, nullptr, in.slot.data(), kPoints, e), e, "null row_start");
    e.clear(); expect("null kf_slots", d.rows.setRows(nullptr, 2, in.start.data(), in.slot.data(), kPoints, e), e, "null kf_slots");
    e.clear(); expect("null point_slot", d.rows.setRows(in.kf.data(), 2, in.start.data(), nullptr, kPoints, e), e, "null point_slot");
    e.clear(); expect("negative n", d.rows.setRows(in.kf.data(), -1, in.start.data(), in.slot.data(), kPoints, e), e, "negative number of keyframe slots: -1");
    e.clear(); expect("idx past the row", entry(d.rows, 0, 3, 1, e), e, "idx[0]: index 3 outside the row of 3 entries");
    e.clear(); expect("idx negative", entry(d.rows, 0, -1, 1, e), e, "idx[0]: index -1 outside the row of 3 entries");
    e.clear(); expect("idx of a keyframe with no row", entry(d.rows, 1, 0, 1, e), e, "idx[0]: index 0 outside the row of 0 entries");
    e.clear(); expect("idx of a keyframe slot past the table", entry(d.rows, 9, 0, 1, e), e, "idx[0]: index 0 outside the row of 0 entries");
    e.clear(); expect("entry: negative keyframe slot", entry(d.rows, -1, 0, 1, e), e, "kf_slot[0]: negative keyframe slot -1");
    e.clear(); expect("entry: point slot past n_points", entry(d.rows, 0, 0, kPoints, e), e, "point_slot[0]: point slot 500 outside -1..499; set the point before a row names it");
    { const int32_t k = 0; e.clear(); expect("entry: null arrays", d.rows.setEntries(&k, nullptr, &k, 1, kPoints, e), e, "null kf_slot, idx or point_slot"); }
    e.clear(); expect("entry: negative n", d.rows.setEntries(nullptr, nullptr, nullptr, -2, kPoints, e), e, "negative number of row entries: -2");
    e.clear(); expect("a row pool past INT32_MAX entries", checkRowPoolTotal((int64_t)INT32_MAX + 1, e), e, "2147483648 entries, past INT32_MAX");
    e.clear(); expect("a row pool of INT32_MAX entries", checkRowPoolTotal(INT32_MAX, e), e, nullptr);
    const int32_t kq[2] = {0, 3}, sq[3] = {-1, 4, kPoints};
    e.clear(); expect("query keyframe slot out of range", RowsHost::checkKfSlots(kq, 2, 3, e), e, "kf_slots[1]: keyframe slot 3 outside 0..2");
    e.clear(); expect("query null kf_slots", RowsHost::checkKfSlots(nullptr, 2, 3, e), e, "null kf_slots");
    e.clear(); expect("query negative n_kf", RowsHost::checkKfSlots(kq, -1, 3, e), e, "negative number of keyframe slots: -1");
    e.clear(); expect("seen slot out of range", RowsHost::checkSeen(sq, 3, kPoints, e), e, "seen_points[2]: point slot 500 outside -1..499");
    e.clear(); expect("seen -1 is accepted", RowsHost::checkSeen(sq, 2, kPoints, e), e, nullptr);
    e.clear(); expect("null seen_points", RowsHost::checkSeen(nullptr, 1, kPoints, e), e, "null seen_points");
    expect("the rejected calls staged nothing", !d.rows.dirty() && d.stats().n_entries == 4 && d.exported()[0][1] == -1, "", nullptr);
    // a call whose second row is malformed stages nothing of its first row either
    e.clear(); { RowsIn b; b.add(0, {9, 9}); b.add(1, {kPoints + 3}); expect("a refused call stages nothing", b.set(d.rows, e), e, "row entry 2"); }
    { const int32_t k2[2] = {0, 0}, i2[2] = {0, 7}, v2[2] = {3, 3}; e.clear(); expect("a refused entry call stages nothing", d.rows.setEntries(k2, i2, v2, 2, kPoints, e), e, "idx[1]"); }
    d.sync();
    expect("... and the rows are what they were", d.stats().last_row_sync_bytes == 0 && d.exported()[0] == std::vector<int32_t>({5, -1, 7}), "", nullptr);
  }
  {   // coalescing
    Db d(8, 64);
    RowsIn a; a.add(3, {1, 2, 3, 4}); a.set(d.rows, e); d.sync();
    const int64_t used = d.stats().pool_used;
    RowsIn b; b.add(3, {1, 2}); b.set(d.rows, e);
    RowsIn c; c.add(3, {9, 9, 9, 9, 9, 9, 9, 9, 9}); c.set(d.rows, e);
    RowsIn f; f.add(3, {6, 7, 8, 9, 10}); f.set(d.rows, e);
    expect("stats count the staged row", d.stats().n_entries == 5 && d.stats().pool_used == used, "", nullptr);
    d.sync();
    expect("coalescing: a row set three times costs the last row only", d.stats().pool_used == used + 5 && d.last.nHeaderRec == 1 && d.last.nPayload == 5 &&
           d.stats().last_row_sync_records == 1 && d.exported()[3] == std::vector<int32_t>({6, 7, 8, 9, 10}), "", nullptr);
    RowsIn g; g.add(3, {20, 21, 22}); g.set(d.rows, e);
    entry(d.rows, 3, 1, -1, e);
    d.sync();
    expect("coalescing: an entry change after a staged row lands in it", d.last.nHeaderRec == 1 && d.last.nEntryRec == 0 && d.last.nPayload == 3 &&
           d.exported()[3] == std::vector<int32_t>({20, -1, 22}), "", nullptr);
    entry(d.rows, 3, 2, 40, e); entry(d.rows, 3, 0, 41, e); entry(d.rows, 3, 2, 42, e);
    d.sync();
    expect("coalescing: one (keyframe, index) changed twice gives one record", d.last.nHeaderRec == 0 && d.last.nEntryRec == 2 && d.last.nPayload == 0 &&
           d.stats().last_row_sync_records == 2 && d.exported()[3] == std::vector<int32_t>({41, -1, 42}), "", nullptr);
    entry(d.rows, 3, 0, 50, e);
    RowsIn h; h.add(3, {60, 61}); h.set(d.rows, e);
    d.sync();
    expect("coalescing: a row staged after an entry change supersedes it", d.last.nHeaderRec == 1 && d.last.nEntryRec == 0 &&
           d.exported()[3] == std::vector<int32_t>({60, 61}), "", nullptr);
    RowsIn z; z.add(3, {}); z.set(d.rows, e);
    d.sync();
    expect("a row of length 0 erases", d.exported()[3].empty() && d.stats().n_entries == 0, "", nullptr);
    d.rows.clear(); d.T = RowTables();
    expect("clear", d.rows.nKeyframes() == 0 && d.stats().n_entries == 0 && d.stats().pool_used == 0 && !d.rows.dirty(), "", nullptr);
    RowsIn r; r.add(1, {3, 4}); r.set(d.rows, e); d.sync();
    expect("clear, then reuse", d.rows.nKeyframes() == 2 && d.exported()[1] == std::vector<int32_t>({3, 4}) && d.stats().pool_used == 2, "", nullptr);
  }
  {   // what a sync moves depends on what was touched, not on the table
    int64_t bytes[2];
    const int32_t sizes[2] = {10, 1000};
    for (int t = 0; t < 2; t++) {
      Db d(sizes[t], 1 << 20);
      RowsIn all;
      for (int32_t k = 0; k < sizes[t]; k++) all.add(k, std::vector<int32_t>(100, k % kPoints));
      all.set(d.rows, e); d.sync();
      RowsIn three; three.add(1, std::vector<int32_t>(90, 2)); three.add(5, std::vector<int32_t>(110, 3)); three.add(8, {});
      three.set(d.rows, e);
      entry(d.rows, 2, 7, -1, e);
      d.sync();
      bytes[t] = d.stats().last_row_sync_bytes;
    }
    expect("three touched rows: the same bytes at 10 and 1 000 keyframes", bytes[0] == bytes[1] && bytes[0] > 800 && bytes[0] < 1000, std::to_string(bytes[0]), nullptr);
  }
  {   // the restatement of the two queries, on cases whose answers are written out here
    //            kf 0: 3 -1 5 3     kf 1: (no row)     kf 2: 5 6 2 -1 0     kf 3: 4 4
    const int32_t rs[5] = {0, 4, 4, 9, 11}, slot[11] = {3, -1, 5, 3, 5, 6, 2, -1, 0, 4, 4};
    const uint8_t bad[7] = {0, 0, 1, 0, 0, 0, 0};   // point 2 is bad
    int32_t out[16]; uint8_t seen[16];
    const int32_t kfs[5] = {2, 0, 1, 3, 2}, sp[4] = {6, -1, 1, 3};
    int n = localmapref_points_of_keyframes(7, bad, rs, slot, kfs, 5, sp, 4, out, seen);
    const int32_t want[5] = {5, 6, 0, 3, 4}; const uint8_t wseen[5] = {0, 1, 0, 1, 0};
    expect("restatement: the points of a keyframe set", n == 5 && !memcmp(out, want, sizeof(want)) && !memcmp(seen, wseen, 5), "", nullptr);
    n = localmapref_points_of_keyframes(7, bad, rs, slot, kfs + 1, 1, nullptr, 0, out, seen);
    expect("restatement: a point twice within one row", n == 2 && out[0] == 3 && out[1] == 5 && seen[0] == 0, "", nullptr);
    n = localmapref_points_of_keyframes(7, bad, rs, slot, kfs + 2, 1, nullptr, 0, out, seen);
    expect("restatement: a keyframe slot with no row", n == 0, "", nullptr);
    // observations: point 0: kf 1 3   point 1: kf 3   point 2 (bad): kf 0   point 3: kf 0 1 3   point 4: none
    const int32_t os[6] = {0, 2, 3, 4, 7, 7}, okf[7] = {1, 3, 3, 0, 0, 1, 3};
    const int32_t list[7] = {0, -1, 3, 2, 3, 4, 1};
    int32_t ck[4], cw[4]; uint8_t pb[7];
    n = localmapref_observer_counter(os, okf, bad, list, 7, ck, cw, pb);
    const int32_t wk[3] = {0, 1, 3}, ww[3] = {2, 3, 4}; const uint8_t wb[7] = {0, 0, 0, 1, 0, 0, 0};
    expect("restatement: the observer counter of a frame", n == 3 && !memcmp(ck, wk, 12) && !memcmp(cw, ww, 12) && !memcmp(pb, wb, 7), "", nullptr);
  }
}

// --------------------------------------------------------------------------------------------------------------------- part 2
static void writeRows(const RowsIn& in) {
  if (!g_ops) return;
  fprintf(g_ops, "R %zu\n", in.kf.size());
  for (size_t i = 0; i < in.kf.size(); i++) {
    fprintf(g_ops, "%d %d", in.kf[i], in.start[i + 1] - in.start[i]);
    for (int32_t q = in.start[i]; q < in.start[i + 1]; q++) fprintf(g_ops, " %d", in.slot[(size_t)q]);
    fprintf(g_ops, "\n");
  }
}

static void sequence() {
  std::mt19937 rng(20240611);
  auto uni = [&rng](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
  auto randomRow = [&](int len) {
    std::vector<int32_t> r((size_t)len);
    for (auto& v : r) v = uni(0, 3) == 0 ? -1 : uni(0, kPoints - 1);
    return r;
  };
  Db d(48, 4096);   // tests/mapdb_rows_support.py: SEQUENCE_CAPACITIES
  std::vector<std::vector<int32_t>> model;
  std::string e;
  bool allEqual = true;
  int32_t hdrGrowths = 0;
  for (int round = 0; round < 40; round++) {
    RowsIn in;
    std::vector<int32_t> ek, ei, ev;
    if (round == 0) {
      for (int32_t k = 0; k < 40; k++) in.add(k, randomRow(uni(20, 120)));
    } else {
      const int nk = (int)model.size();
      for (int j = 0; j < 6; j++) {   // rows replaced with equal and different lengths; the same row may be drawn twice: the last wins
        const int k = uni(0, nk - 1);
        in.add(k, randomRow(j % 2 == 0 ? (int)model[(size_t)k].size() : uni(10, 120)));
      }
      if (round == 12)                // most keyframes culled at once: the pool is mostly garbage afterwards
        for (int k = 0; k < nk; k++) if (k % 4 != 0) in.add(k, {});
      if (round % 7 == 3) in.add(uni(0, nk - 1), {});
      if (round % 3 == 1) in.add(nk + (round % 2), randomRow(uni(30, 90)));   // slots added past the high-water mark, one skipped sometimes
    }
    if (!in.set(d.rows, e)) { printf("sequence: set_keyframe_rows refused: %s FAILED\n", e.c_str()); g_failed++; return; }
    writeRows(in);
    for (size_t i = 0; i < in.kf.size(); i++) {
      if ((size_t)in.kf[i] >= model.size()) model.resize((size_t)in.kf[i] + 1);
      model[(size_t)in.kf[i]].assign(in.slot.begin() + in.start[i], in.slot.begin() + in.start[i + 1]);
    }
    if (round > 0) {                  // single entries flipped: some in rows staged this round, some resident, some twice
      for (int j = 0; j < 12; j++) {
        const int k = uni(0, (int)model.size() - 1);
        if (model[(size_t)k].empty()) continue;
        const int i = j >= 10 && !ei.empty() && model[(size_t)ek.back()].size() > 0 ? ei.back() : uni(0, (int)model[(size_t)k].size() - 1);
        const int kk = j >= 10 && !ek.empty() ? ek.back() : k;
        ek.push_back(kk); ei.push_back(i); ev.push_back(uni(0, 4) == 0 ? -1 : uni(0, kPoints - 1));
        model[(size_t)kk][(size_t)i] = ev.back();
      }
      if (!d.rows.setEntries(ek.data(), ei.data(), ev.data(), (int32_t)ek.size(), kPoints, e)) { printf("sequence: set_row_entries refused: %s FAILED\n", e.c_str()); g_failed++; return; }
      if (g_ops) {
        fprintf(g_ops, "E %zu\n", ek.size());
        for (size_t i = 0; i < ek.size(); i++) fprintf(g_ops, "%d %d %d\n", ek[i], ei[i], ev[i]);
      }
    }
    d.sync();
    if (d.exported() != model) { allEqual = false; printf("sequence: round %d MISMATCH\n", round); }
    const YdMapDbRowStats s = d.stats();
    hdrGrowths = s.header_growths;
    char line[256];
    snprintf(line, sizeof(line), "trace %d %d %lld %lld %lld %d %d %d %d %lld %lld", round, d.rows.nKeyframes(), (long long)s.n_entries, (long long)s.pool_used,
             (long long)s.pool_capacity, s.repacks_kept, s.repacks_grown, s.header_growths, s.header_capacity, (long long)s.last_row_sync_bytes,
             (long long)s.last_row_sync_records);
    printf("%s\n", line);
    if (g_ops) fprintf(g_ops, "S\n%s\n", line);
  }
  const YdMapDbRowStats s = d.stats();
  expect("sequence: every sync equals the model", allEqual, "", nullptr);
  expect("sequence: a repack that kept the capacity", s.repacks_kept >= 1, "", nullptr);
  expect("sequence: a repack that grew the capacity", s.repacks_grown >= 1, "", nullptr);
  expect("sequence: a keyframe-table growth", hdrGrowths >= 1, "", nullptr);
}

int main(int argc, char** argv) {
  if (argc > 1) g_ops = fopen(argv[1], "w");
  cases();
  sequence();
  if (g_ops) fclose(g_ops);
  printf("%d failed\n", g_failed);
  return g_failed;
}
