// Stand-alone check of ydorbslam_amd/csrc/mapdb_attr_host.h (no HIP, no GPU): the validation of the resident table's point attributes,
// coalescing per slot and per group, the clear record of an erased point and its order against a set of the same interval, delta
// packing, and every packed delta executed on host arrays by executeAttr.  tests/test_mapdb_attr_cpu.py builds it with
// -fsanitize=address,undefined and runs it as its own process.
//   mapdb_attr_check [ops.txt]
// Part 1 prints one line per case: the case names are the rules.  Part 2 drives a seeded sequence of point and attribute changes against
// a naive model (one record per slot, changed at once by every operation) across two growths of the point table: after every sync the
// host-applied arrays must equal the model's.  It prints one "trace" line of counters per round.  With ops.txt given it also writes
// every operation there:
//   P n / n lines "slot bad"                                  set_points: a point that is not bad has one observation (keyframe 0, level 0)
//   A n groups / n lines "slot nx ny nz min max hex[64]"      set_point_attributes; groups: 1 geometry, 2 descriptor, 3 both; floats as
//                                                             the hex of their bits; the line ends after the groups given
//   S / the trace line                                        sync, then the counters that follow it
// tests/test_mapdb_attr_gpu.py replays that file through the real handle and holds ydorb_mapdb_attr_stats to the same trace.
// The exit status is the number of failed cases.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/mapdb_attr_host.h"
#include "../../ydorbslam_amd/csrc/mapdb_host.h"

constexpr int kNameWidth = 78;
#include "check_common.h"

using namespace ydorb::mapdb;

static FILE* g_ops = nullptr;

constexpr int32_t kPointCap = 64, kStartPoints = 40;   // tests/test_mapdb_attr_gpu.py creates its handle with this point capacity

struct Db {   // the handle's point table and attribute relation without a device
  Host host;
  AttrHost attr;
  HostTables T;
  AttrTables A;
  std::vector<uint8_t> delta;
  Plan lastPoints;
  AttrPlan lastAttr;
  Db() : host(kPointCap, 4, 1024) {
    const int32_t k = 0;
    const float c[3] = {0.f, 0.f, 0.f};
    std::string e;
    host.setCentres(&k, 1, c, e);
  }
  bool setPoints(const std::vector<int32_t>& slots, const std::vector<uint8_t>& bad, std::string& e) {
    const int32_t n = (int32_t)slots.size();
    std::vector<int32_t> start(1, 0), kf, ref((size_t)n, 0);
    std::vector<uint8_t> level, lv((size_t)n, 0);
    std::vector<float> pos(3 * (size_t)n + 1, 0.f);
    for (int32_t i = 0; i < n; i++) {
      if (!bad[(size_t)i]) { kf.push_back(0); level.push_back(0); }
      start.push_back((int32_t)kf.size());
      pos[3 * (size_t)i] = (float)slots[(size_t)i];
    }
    kf.push_back(0); level.push_back(0);   // never null
    if (!host.setPoints(slots.data(), n, start.data(), kf.data(), level.data(), bad.data(), ref.data(), lv.data(), pos.data(), e)) return false;
    attr.pointsSet(slots.data(), n, start.data(), bad.data());   // the driver's set_points
    if (g_ops) {
      fprintf(g_ops, "P %d\n", n);
      for (int32_t i = 0; i < n; i++) fprintf(g_ops, "%d %d\n", slots[(size_t)i], bad[(size_t)i]);
    }
    return true;
  }
  void sync() {   // the driver's sync: the points, then the attributes (which follow the point table's capacity)
    syncOnHost(host, lastPoints, delta, [this](const Plan& P, const uint8_t* d) { execute(P, d, T); });
    if (!attr.needsSync(host.pointCap())) { attr.nothingToSync(); return; }
    lastAttr = attr.plan(host.pointCap());
    delta.assign(lastAttr.bytes + 1, 0xee);
    attr.pack(lastAttr, delta.data());
    if (delta[lastAttr.bytes] != 0xee) { printf("pack wrote past the delta FAILED\n"); g_failed++; }
    executeAttr(lastAttr, delta.data(), A);
  }
  YdMapDbAttrStats stats() const { YdMapDbAttrStats s; attr.stats(s); return s; }
};

struct Value {   // what one slot holds, and the naive model's record
  float normal[3] = {0.f, 0.f, 0.f}, mn = 0.f, mx = 0.f;
  uint8_t desc[32] = {0};
  uint8_t flags = 0;
};
static Value valueOf(uint32_t seed) {
  std::mt19937 g(seed);
  Value v;
  for (float& x : v.normal) x = (float)(int32_t)(g() % 2001u) / 1000.f - 1.f;
  v.mn = (float)(g() % 9000u) / 1000.f + 0.25f; v.mx = v.mn * 3.583181f;
  for (uint8_t& b : v.desc) b = (uint8_t)g();
  return v;
}

struct AttrIn {   // the arguments of one set_point_attributes call
  std::vector<int32_t> slot;
  std::vector<float> normal, mn, mx;
  std::vector<uint8_t> desc;
  int groups = 3;
  void add(int32_t s, const Value& v) {
    slot.push_back(s);
    normal.insert(normal.end(), v.normal, v.normal + 3); mn.push_back(v.mn); mx.push_back(v.mx);
    desc.insert(desc.end(), v.desc, v.desc + 32);
  }
  bool set(Db& d, std::string& e) const {
    const bool g = groups & 1, ds = groups & 2;
    const bool ok = d.attr.set(slot.data(), (int32_t)slot.size(), g ? normal.data() : nullptr, g ? mn.data() : nullptr, g ? mx.data() : nullptr,
                               ds ? desc.data() : nullptr, d.host.nPoints(), e);
    if (ok && g_ops) {
      fprintf(g_ops, "A %d %d\n", (int)slot.size(), groups);
      for (size_t i = 0; i < slot.size(); i++) {
        fprintf(g_ops, "%d", slot[i]);
        if (g) {
          uint32_t w[5];
          memcpy(w, &normal[3 * i], 12); memcpy(w + 3, &mn[i], 4); memcpy(w + 4, &mx[i], 4);
          for (uint32_t x : w) fprintf(g_ops, " %08x", x);
        }
        if (ds) {
          fprintf(g_ops, " ");
          for (int b = 0; b < 32; b++) fprintf(g_ops, "%02x", desc[32 * i + (size_t)b]);
        }
        fprintf(g_ops, "\n");
      }
    }
    return ok;
  }
};

static bool holds(const AttrTables& A, int32_t s, const Value& v) {
  const size_t p = (size_t)s;
  return p < A.flags.size() && A.flags[p] == v.flags && memcmp(&A.normal[3 * p], v.normal, 12) == 0 && memcmp(&A.minDistance[p], &v.mn, 4) == 0 &&
         memcmp(&A.maxDistance[p], &v.mx, 4) == 0 && memcmp(&A.desc[32 * p], v.desc, 32) == 0;
}
static Value with(Value v, uint8_t flags) {   // the groups not flagged read as zero
  if (!(flags & kAttrGeometry)) { v.normal[0] = v.normal[1] = v.normal[2] = v.mn = v.mx = 0.f; }
  if (!(flags & kAttrDescriptor)) memset(v.desc, 0, 32);
  v.flags = flags;
  return v;
}
static void check(const char* name, bool ok) { expect(name, ok, "", nullptr); }

static void rules() {
  std::string e;
  const float f3[6] = {0, 0, 1, 0, 0, 1}, f1[2] = {1.f, 2.f};
  const uint8_t d64[64] = {0};
  const int32_t s01[2] = {0, 1};
  {
    Db d;
    expect("not enabled: set_point_attributes is refused", d.attr.set(s01, 1, f3, f1, f1, d64, 10, e), e, "point attributes are not enabled");
    YdMapDbAttrStats s = d.stats();
    check("not enabled: the stats are all zero", s.enabled == 0 && s.capacity == 0 && s.growths == 0 && s.last_attr_sync_bytes == 0 && s.last_attr_sync_records == 0);
    d.setPoints({0, 1, 2}, {1, 0, 1}, e);
    check("not enabled: an erased point stages nothing", !d.attr.dirty() && !d.attr.needsSync(d.host.pointCap()));
    d.attr.enable(d.host.pointCap()); d.attr.enable(d.host.pointCap());
    check("enable twice is fine", d.stats().enabled == 1 && d.stats().capacity == kPointCap && d.stats().growths == 0);
  }
  Db d;
  d.attr.enable(d.host.pointCap());
  std::vector<int32_t> all;
  for (int32_t s = 0; s < kStartPoints; s++) all.push_back(s);
  d.setPoints(all, std::vector<uint8_t>(all.size(), 0), e);
  const int32_t np = d.host.nPoints();
  e.clear();
  expect("negative n", d.attr.set(s01, -1, f3, f1, f1, d64, np, e), e, "negative number of point slots: -1");
  expect("null slots with n > 0", d.attr.set(nullptr, 2, f3, f1, f1, d64, np, e), e, "null slots");
  expect("both groups null", d.attr.set(s01, 2, nullptr, nullptr, nullptr, nullptr, np, e), e, "null geometry group and null desc: nothing to set");
  expect("a partial geometry group: normal missing", d.attr.set(s01, 2, nullptr, f1, f1, d64, np, e), e, "all three or none");
  expect("a partial geometry group: min_distance missing", d.attr.set(s01, 2, f3, nullptr, f1, nullptr, np, e), e, "all three or none");
  expect("a partial geometry group: max_distance missing", d.attr.set(s01, 2, f3, f1, nullptr, d64, np, e), e, "all three or none");
  { const int32_t s[2] = {3, kStartPoints}; expect("slot past n_points", d.attr.set(s, 2, f3, f1, f1, d64, np, e), e, "slots[1]: point slot 40 outside 0..39"); }
  { const int32_t s[2] = {-1, 3}; expect("negative slot", d.attr.set(s, 2, f3, f1, f1, d64, np, e), e, "slots[0]: point slot -1 outside 0..39"); }
  { const int32_t s[2] = {39, 40}; expect("query slot past n_points", AttrHost::checkSlots(s, 2, np, e), e, "point_slots[1]: point slot 40 outside 0..39"); }
  check("a rejected call stages nothing", !d.attr.dirty());
  e.clear();
  expect("n == 0 with a group given", d.attr.set(nullptr, 0, nullptr, nullptr, nullptr, d64, np, e), e, nullptr);
  expect("staged points count: a slot staged and not yet synced", d.attr.set(s01, 2, f3, f1, f1, nullptr, np, e), e, nullptr);
  d.sync();
  check("the first sync carries two records of 64 bytes", d.lastAttr.nRec == 2 && d.lastAttr.bytes == 128 && d.stats().last_attr_sync_bytes == 128 && d.stats().last_attr_sync_records == 2);
  d.sync();
  check("nothing staged: last_attr_sync_bytes == 0", d.stats().last_attr_sync_bytes == 0 && d.stats().last_attr_sync_records == 0);
  check("a slot never set reads as flags 0 and zero values", holds(d.A, 5, Value()));

  // coalescing per slot and per group
  const Value a = valueOf(1), b = valueOf(2), c = valueOf(3);
  { AttrIn in; in.add(7, a); in.add(7, b); in.set(d, e); }
  { AttrIn in; in.groups = 1; in.add(7, c); in.set(d, e); }
  d.sync();
  Value want = b;
  memcpy(want.normal, c.normal, 12); want.mn = c.mn; want.mx = c.mx; want.flags = 3;
  check("coalescing: a slot set three times yields one record", d.lastAttr.nRec == 1 && d.lastAttr.bytes == 64);
  check("coalescing: each group keeps its last value", holds(d.A, 7, want));
  { AttrIn in; in.groups = 2; in.add(8, a); in.set(d, e); }
  d.sync();
  check("a null geometry group leaves it and its flag alone", holds(d.A, 8, with(a, kAttrDescriptor)));
  { AttrIn in; in.groups = 1; in.add(8, b); in.set(d, e); }
  d.sync();
  want = a; memcpy(want.normal, b.normal, 12); want.mn = b.mn; want.mx = b.mx; want.flags = 3;
  check("a null desc leaves the descriptor and its flag alone", holds(d.A, 8, want));
  {
    const AttrRec* r = reinterpret_cast<const AttrRec*>(d.delta.data());
    check("the record names its groups and lies in the 64-byte format", r->slot == 8 && r->set == kAttrGeometry && r->clear == 0 && memcmp(r->normal, b.normal, 12) == 0);
  }

  // the clear record of an erased point
  d.setPoints({7}, {1}, e);
  d.sync();
  check("an erased point stages one clear record", d.lastAttr.nRec == 1 && reinterpret_cast<const AttrRec*>(d.delta.data())->clear == 1 &&
                                                      reinterpret_cast<const AttrRec*>(d.delta.data())->set == 0);
  check("an erased point reads as no attributes", holds(d.A, 7, Value()));
  d.setPoints({7}, {0}, e);
  d.sync();
  check("the slot reused for a new point still reads as no attributes", holds(d.A, 7, Value()) && d.stats().last_attr_sync_records == 0);
  { AttrIn in; in.add(8, c); in.set(d, e); }
  d.setPoints({8}, {1}, e);
  d.sync();
  check("a set staged before the erase of the same interval is dropped", d.lastAttr.nRec == 1 && holds(d.A, 8, Value()));
  d.setPoints({9}, {1}, e);
  { AttrIn in; in.groups = 1; in.add(9, c); in.set(d, e); }
  d.sync();
  check("a set staged after the erase of the same interval stays", d.lastAttr.nRec == 1 && holds(d.A, 9, with(c, kAttrGeometry)));
  { AttrIn in; in.add(9, a); in.set(d, e); }
  d.sync();
  d.setPoints({9}, {1}, e);
  { AttrIn in; in.groups = 2; in.add(9, b); in.set(d, e); }
  d.sync();
  check("... and the clear still zeroes the group the set does not name", holds(d.A, 9, with(b, kAttrDescriptor)));
  d.setPoints({10}, {0}, e);
  d.sync();
  check("set_points of a live point clears nothing", d.stats().last_attr_sync_records == 0);
  { AttrIn in; in.add(3, a); in.set(d, e); }
  d.attr.clear();
  check("clear drops what is staged and keeps capacity and counters", !d.attr.dirty() && d.stats().capacity == kPointCap && d.stats().enabled == 1);
}

static void sequence() {
  Db d;
  d.attr.enable(d.host.pointCap());
  std::vector<Value> model;
  std::vector<uint8_t> live;
  std::mt19937 g(20240611);
  std::string e;
  bool equal = true, grewOnce = false, grewEmpty = false;
  int erasedWithAttr = 0, bothOrders = 0;
  auto setPoints = [&](const std::vector<int32_t>& slots, const std::vector<uint8_t>& bad) {
    if (!d.setPoints(slots, bad, e)) { equal = false; return; }
    for (size_t i = 0; i < slots.size(); i++) {
      const size_t s = (size_t)slots[i];
      if (s >= model.size()) { model.resize(s + 1); live.resize(s + 1, 0); }
      live[s] = !bad[i];
      if (bad[i]) { erasedWithAttr += model[s].flags != 0; model[s] = Value(); }
    }
  };
  auto setAttr = [&](int groups, int count) {
    AttrIn in;
    in.groups = groups;
    for (int i = 0; i < count; i++) {
      const int32_t s = (int32_t)(g() % model.size());
      const Value v = valueOf(g());
      in.add(s, v);
      if (groups & 1) { memcpy(model[(size_t)s].normal, v.normal, 12); model[(size_t)s].mn = v.mn; model[(size_t)s].mx = v.mx; }
      if (groups & 2) memcpy(model[(size_t)s].desc, v.desc, 32);
      model[(size_t)s].flags |= (uint8_t)groups;
    }
    if (!in.set(d, e)) equal = false;
  };
  {
    std::vector<int32_t> all;
    for (int32_t s = 0; s < kStartPoints; s++) all.push_back(s);
    setPoints(all, std::vector<uint8_t>(all.size(), 0));
  }
  for (int round = 0; round < 40; round++) {
    const int32_t capBefore = d.stats().capacity > 0 ? (int32_t)d.stats().capacity : 0;
    if (round == 6 || round == 23 || round % 9 == 4) {   // new points: rounds 6 and 23 take the table past its capacity
      std::vector<int32_t> fresh;
      const int32_t n = round == 6 ? 50 : round == 23 ? 120 : 3;
      for (int32_t i = 0; i < n; i++) fresh.push_back((int32_t)model.size() + i);
      setPoints(fresh, std::vector<uint8_t>(fresh.size(), 0));
    }
    if (round != 23) {   // round 23 grows the table with no attribute staged
      setAttr(1 + (int)(g() % 3u), 1 + (int)(g() % 12u));
      if (g() % 2u) setAttr(1 + (int)(g() % 3u), 1 + (int)(g() % 6u));
      std::vector<int32_t> gone;
      for (int i = 0, n = (int)(g() % 4u); i < n; i++) gone.push_back((int32_t)(g() % model.size()));
      if (!gone.empty()) setPoints(gone, std::vector<uint8_t>(gone.size(), 1));
      if (g() % 2u) { setAttr(1 + (int)(g() % 3u), 1 + (int)(g() % 8u)); bothOrders++; }   // may name a slot erased just above
      if (round % 5 == 2) {   // erased slots come back as new points
        std::vector<int32_t> back;
        for (size_t s = 0; s < live.size(); s++) if (!live[s]) back.push_back((int32_t)s);
        if (!back.empty()) setPoints(back, std::vector<uint8_t>(back.size(), 0));
      }
    }
    d.sync();
    const YdMapDbAttrStats s = d.stats();
    if (s.capacity != capBefore) { grewOnce = true; grewEmpty = grewEmpty || s.last_attr_sync_records == 0; }
    if (d.A.flags.size() != (size_t)s.capacity || s.capacity != d.host.pointCap()) equal = false;
    for (size_t p = 0; p < model.size(); p++)
      if (!holds(d.A, (int32_t)p, model[p])) { if (equal) printf("MISMATCH round %d slot %zu\n", round, p); equal = false; }
    for (size_t p = model.size(); p < d.A.flags.size(); p++) if (!holds(d.A, (int32_t)p, Value())) equal = false;
    char line[256];
    snprintf(line, sizeof(line), "trace %d %d %d %lld %lld %lld %d", round, s.enabled, s.growths, (long long)s.capacity, (long long)s.last_attr_sync_bytes,
             (long long)s.last_attr_sync_records, d.host.nPoints());
    printf("%s\n", line);
    if (g_ops) fprintf(g_ops, "S\n%s\n", line);
  }
  check("sequence: every sync equals the model", equal);
  check("sequence: the arena grew with the point table, twice", grewOnce && d.stats().growths == 2 && d.stats().capacity > 2 * kPointCap);
  check("sequence: one growth came with no attribute staged", grewEmpty);
  check("sequence: points with attributes were erased, and sets followed erases", erasedWithAttr >= 5 && bothOrders >= 5);
}

int main(int argc, char** argv) {
  rules();
  if (argc > 1) g_ops = fopen(argv[1], "w");   // the sequence's operations only
  sequence();
  if (g_ops) fclose(g_ops);
  printf("%d failed\n", g_failed);
  return g_failed;
}
