// Stand-alone check of ydorbslam_amd/csrc/span_pool.h and layout.h (no HIP, no GPU): the pool policy that mapdb_host.h and
// mapdb_rows_host.h share, at the smallest numbers at which each rule can go wrong.  Only counts are involved: nothing of a pool's size
// is allocated.  tests/test_mapdb_cpu.py builds it with -fsanitize=address,undefined and runs it as its own process.
// It prints one line per case; the exit status is the number of failed cases.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/span_pool.h"

constexpr int kNameWidth = 64;
#include "check_common.h"

using namespace ydorb::mapdb;

static void check(const char* name, bool ok) { expect(name, ok, "", nullptr); }

static SpanPool pool(int64_t cap, int64_t used, int64_t live) {
  SpanPool p(cap);
  p.used = used; p.live = p.pending = live;
  return p;
}

static void decisions() {
  check("capacity is at least 1", SpanPool(0).cap == 1 && SpanPool(-5).cap == 1 && SpanPool(8).cap == 8);
  {   // the trigger: used + incoming against the capacity
    const SpanPool p = pool(8, 5, 5);
    const PoolPlan at = p.plan(0, 3), past = p.plan(0, 4);
    check("used + incoming == capacity: no repack, tail = used", at.repack == kNoRepack && at.tail == 5 && at.poolCap == 8 && at.survivors == 5 && at.nPayload == 3);
    check("used + incoming == capacity + 1: repack, tail = survivors", past.repack != kNoRepack && past.tail == 5 && past.survivors == 5 && past.usedBefore == 5 && past.poolCapBefore == 8);
    const PoolPlan replaced = pool(8, 6, 5).plan(2, 1);   // 6 used + 1: fits, though only 3 of the 5 live entries survive
    const PoolPlan garbage = pool(8, 7, 5).plan(3, 2);    // 7 used + 2: does not fit, though only 2 + 2 entries are needed
    check("garbage counts towards the trigger, not towards the need", replaced.repack == kNoRepack && replaced.tail == 6 && replaced.survivors == 3 &&
          garbage.repack == kRepackKept && garbage.tail == 2 && garbage.survivors == 2 && garbage.usedBefore == 7);
  }
  for (const int64_t cap : {(int64_t)8, (int64_t)9}) {   // kept or grown: need against capacity / 2, rounded down
    const PoolPlan four = pool(cap, cap, 2).plan(0, 2), five = pool(cap, cap, 2).plan(0, 3);
    const std::string c = "capacity " + std::to_string(cap);
    check((c + ": need 4 keeps the capacity").c_str(), four.repack == kRepackKept && four.poolCap == cap && four.poolCapBefore == cap && four.tail == 2);
    check((c + ": need 5 grows it to 10").c_str(), five.repack == kRepackGrown && five.poolCap == 10 && five.poolCapBefore == cap && five.tail == 2);
  }
  {
    const int64_t big = (int64_t)1 << 30;
    const PoolPlan P = pool(big, big, big).plan(0, 1);
    check("need 2^30 + 1: the capacity is INT32_MAX", P.repack == kRepackGrown && P.poolCap == INT32_MAX && P.tail == big);
    const PoolPlan Q = pool(big, big, big).plan(big, big);   // need 2^30: 2 x need is one past INT32_MAX
    check("need 2^30: the capacity is INT32_MAX", Q.repack == kRepackGrown && Q.poolCap == INT32_MAX && Q.tail == 0);
  }
  {
    const PoolPlan P = pool(8, 8, 6).plan(6, 3);
    check("all live entries replaced: survivors 0, tail 0 on repack", P.repack == kRepackKept && P.survivors == 0 && P.tail == 0);
    const PoolPlan N = pool(8, 8, 6).plan(0, 0), E = pool(8, 8, 6).plan(3, 0);
    check("nothing incoming with a full pool: no repack", N.repack == kNoRepack && N.tail == 8 && N.survivors == 6 && E.repack == kNoRepack && E.survivors == 3);
  }
  {   // commit: none, kept, grown
    SpanPool p = pool(8, 5, 5);
    PoolPlan P = p.plan(1, 3);
    p.commit(P);
    check("commit without a repack: no counter moves", p.live == 7 && p.used == 8 && p.cap == 8 && p.repacksKept == 0 && p.repacksGrown == 0);
    P = p.plan(5, 2);   // 8 + 2 > 8: survivors 2, need 4
    p.commit(P);
    check("commit of a kept repack: live, used, one counter", P.repack == kRepackKept && p.live == 4 && p.used == 4 && p.cap == 8 && p.repacksKept == 1 && p.repacksGrown == 0);
    P = p.plan(0, 5);   // 4 + 5 > 8: need 9
    p.commit(P);
    check("commit of a grown repack: live, used, the other counter", P.repack == kRepackGrown && p.live == 9 && p.used == 9 && p.cap == 18 && p.repacksKept == 1 && p.repacksGrown == 1);
    p.pending = p.live;
    p.clear();
    check("clear: empty, the capacity and the counters stay", p.used == 0 && p.live == 0 && p.pending == 0 && p.cap == 18 && p.repacksKept == 1 && p.repacksGrown == 1);
  }
}

static void offsets() {
  const std::vector<int32_t> len = {3, 0, 2, 5, 0, 4, 7};
  std::vector<int32_t> off(7, 77), newOff(7, 99);
  const int64_t end = survivorOffsets(6, len.data(), off.data(), newOff.data(), [](int32_t s) { return s == 3; });
  check("survivors in ascending slot order", newOff[0] == 0 && newOff[2] == 3 && newOff[5] == 5 && off[0] == 0 && off[2] == 3 && off[5] == 5);
  check("a replaced slot gets -1, adds nothing and keeps its offset", newOff[3] == -1 && off[3] == 77);
  check("a zero-length survivor shares the next slot's offset", newOff[1] == newOff[2] && newOff[4] == newOff[5] && off[1] == 3 && off[4] == 5);
  check("the last offset plus its length equals the survivors", newOff[5] + len[5] == 9 && end == 9);
  check("a slot at or past nBefore is not touched", newOff[6] == 99 && off[6] == 77);
  check("no slots: nothing", survivorOffsets(0, len.data(), off.data(), newOff.data(), [](int32_t) { return false; }) == 0 && newOff[0] == 0);
}

static void growth() {
  check("table growth: needed <= capacity is unchanged", grownCap(48, 48) == 48 && grownCap(0, 48) == 48 && grownCap(1, 1) == 1);
  check("table growth: capacity + 1 gives 2 x capacity", grownCap(49, 48) == 96 && grownCap(2, 1) == 2);
  check("table growth: 3 x capacity gives 3 x capacity", grownCap(144, 48) == 144);
  check("table growth: capacity 2^30 + 1 gives INT32_MAX", grownCap((1 << 30) + 2, (1 << 30) + 1) == INT32_MAX && grownCap(INT32_MAX, (1 << 30) + 1) == INT32_MAX);
}

static void guard() {
  std::string e;
  expect("a total of INT32_MAX passes", checkPoolTotal(INT32_MAX, e) && checkRowPoolTotal(INT32_MAX, e), e, nullptr);
  e.clear(); expect("INT32_MAX + 1 observations", checkPoolTotal((int64_t)INT32_MAX + 1, e), e, "the pool would hold 2147483648 observations, past INT32_MAX");
  e.clear(); expect("INT32_MAX + 1 row entries", checkRowPoolTotal((int64_t)INT32_MAX + 1, e), e, "the row pool would hold 2147483648 entries, past INT32_MAX");
  // 10 below INT32_MAX pending, 4 of them in slot 1; slot 0 is named twice in one call
  SpanPool p = pool(8, 0, (int64_t)INT32_MAX - 10);
  int asked = 0;
  const auto lenNow = [&asked](int32_t s) { asked++; return s == 1 ? 4 : 0; };
  const int32_t twice[2] = {0, 0}, fits[3] = {0, 30, 40}, over[3] = {0, 30, 41}, both[2] = {0, 1}, swap[3] = {0, 10, 14}, swapOver[3] = {0, 11, 15};
  e.clear(); expect("one slot named twice counts its last length only", p.admits(twice, 2, fits, lenNow, checkRowPoolTotal, e), e, nullptr);
  e.clear(); expect("... and one entry more is refused", p.admits(twice, 2, over, lenNow, checkRowPoolTotal, e), e, "the row pool would hold 2147483648 entries, past INT32_MAX");
  e.clear(); expect("what a named slot holds now leaves", p.admits(both, 2, swap, lenNow, checkPoolTotal, e), e, nullptr);
  e.clear(); expect("... one entry more", p.admits(both, 2, swapOver, lenNow, checkPoolTotal, e), e, "the pool would hold 2147483648 observations, past INT32_MAX");
  asked = 0;
  const int32_t ten[2] = {0, 10};
  e.clear(); expect("the cheap test passes without the exact figure", p.admits(twice, 1, ten, lenNow, checkRowPoolTotal, e) && asked == 0, e, nullptr);
  p.restaged(4, 0);
  check("restaged moves the live-after-sync count only", p.pending == (int64_t)INT32_MAX - 14 && p.live == (int64_t)INT32_MAX - 10 && p.used == 0);
}

static void layout() {   // 16-byte sections: what both plan() functions lay their deltas out with
  ydorb::Layout L;
  const size_t a = L.add(1), b = L.add(0), c = L.add(32), d = L.add(17);
  check("delta sections: 16-byte aligned, an empty one takes no room", a == 0 && b == 16 && c == 16 && d == 48 && L.bytes == 80);
}

int main() {
  decisions();
  offsets();
  growth();
  guard();
  layout();
  printf("%d failed\n", g_failed);
  return g_failed;
}
