// The span pool of the resident map table, once (DESIGN.md section 6m states the policy): mapdb_host.h keeps a point's observations in
// one, mapdb_rows_host.h a keyframe's map-point row.  Accounting and the repack decision, the survivors' offsets, the INT32_MAX guard
// and the growth rule of the slot tables.  No HIP here: a plain host compiler builds it (tests/cpu_harness/span_pool_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <unordered_map>

#include "layout.h"
#include "map_table.h"

namespace ydorb {
namespace mapdb {

using maptable::fail;

enum { kNoRepack = 0, kRepackKept = 1, kRepackGrown = 2 };

// The pool part of what one sync does; Plan and RowPlan derive from it.  The payload goes to [tail, tail + nPayload).
struct PoolPlan {
  int repack = kNoRepack;
  int64_t poolCapBefore = 0, poolCap = 0, usedBefore = 0, survivors = 0, tail = 0, nPayload = 0;
};

// A slot table of `cap` that must hold `needed`: unchanged while it does, else max(needed, 2 x cap), INT32_MAX at the most
inline int32_t grownCap(int32_t needed, int32_t cap) { return needed <= cap ? cap : (int32_t)std::min<int64_t>(std::max<int64_t>(needed, 2 * (int64_t)cap), INT32_MAX); }

inline bool checkTotal(int64_t total, const char* past, std::string& err) { return total <= INT32_MAX ? true : fail(err, past, total); }
inline bool checkPoolTotal(int64_t total, std::string& err) { return checkTotal(total, "the pool would hold %lld observations, past INT32_MAX", err); }
inline bool checkRowPoolTotal(int64_t total, std::string& err) { return checkTotal(total, "the row pool would hold %lld entries, past INT32_MAX", err); }

// A repack's survivors in ascending slot order over the slots below nBefore: newOff[] gets their offsets and off[] moves with it.  A
// slot the delta replaces gets -1 and adds nothing: apply gives it its new span.  Returns where the survivors end.
template <class Replaced> int64_t survivorOffsets(int32_t nBefore, const int32_t* len, int32_t* off, int32_t* newOff, Replaced replaced) {
  int64_t at = 0;
  for (int32_t s = 0; s < nBefore; s++) {
    if (replaced(s)) { newOff[s] = -1; continue; }
    newOff[s] = off[s] = (int32_t)at; at += len[s];
  }
  return at;
}

struct SpanPool {
  int64_t cap, used = 0, live = 0, pending = 0;   // as of the last sync, but pending: the live entries once what is staged is applied
  int32_t repacksKept = 0, repacksGrown = 0;
  explicit SpanPool(int64_t c) : cap(std::max<int64_t>(c, 1)) {}
  void clear() { used = live = pending = 0; }
  void restaged(int64_t was, int64_t now) { pending += now - was; }   // one slot's span, staged changes included

  // May a call stage start[i + 1] - start[i] entries for every slots[i]?  The cheap test, and only then the exact figure: what the named
  // slots hold now (lenNow(slot), staged changes included) leaves, each slot's last span enters.  check: the pool's of the two above.
  template <class LenNow, class Check> bool admits(const int32_t* slots, int32_t n, const int32_t* start, LenNow lenNow, Check check, std::string& err) const {
    if (pending + (int64_t)start[n] <= INT32_MAX) return true;
    std::unordered_map<int32_t, int32_t> last;
    for (int32_t i = 0; i < n; i++) last[slots[i]] = start[i + 1] - start[i];
    int64_t total = pending;
    for (const auto& kv : last) total += (int64_t)kv.second - lenNow(kv.first);
    return check(total, err);
  }

  // replaced: the entries the device holds of the spans this sync replaces; incoming: the entries it appends
  PoolPlan plan(int64_t replaced, int64_t incoming) const {
    PoolPlan P;
    P.poolCapBefore = P.poolCap = cap; P.usedBefore = P.tail = used; P.nPayload = incoming; P.survivors = live - replaced;
    if (used + incoming > cap) {
      const int64_t need = P.survivors + incoming;   // <= INT32_MAX: admits() refused what would pass it
      P.repack = need <= cap / 2 ? kRepackKept : kRepackGrown;
      if (P.repack == kRepackGrown) P.poolCap = std::min<int64_t>(2 * need, INT32_MAX);
      P.tail = P.survivors;
    }
    return P;
  }
  void commit(const PoolPlan& P) {
    live = P.survivors + P.nPayload; used = P.tail + P.nPayload; cap = P.poolCap;
    if (P.repack == kRepackKept) repacksKept++;
    if (P.repack == kRepackGrown) repacksGrown++;
  }
};

}  // namespace mapdb
}  // namespace ydorb
