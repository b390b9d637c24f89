// Host side of the resident table's point attributes (include/ydorb/c_api.h, "Resident point attributes"): per
// point slot the normal, the two raw distances of updateNormalAndDepth, the 32-byte descriptor and a flag byte (bit 0: the geometry
// group is set, bit 1: the descriptor is set).  The relation is opt-in: a handle that never enables it never builds an AttrHost's state.
//   staging   set_point_attributes validates, then writes the staged value of each named group and marks the slot: one slot yields one
//             record whatever was staged for it (the last value of a group wins), so the apply kernel never has two lanes storing to
//             one address.  An erased point (set_points with bad = 1 and an empty span, pointsSet below) stages a clear: what was staged
//             for the slot before it goes, what is staged after it stays, and the record says "clear first".
//   delta     [attribute records], 64 bytes each, in the order their slots were first dirtied; the descriptor lies at byte 32 of a
//             record, so it moves as two uint4.
//   cleared   a cleared slot reads as flags 0 and all-zero values, which is also what a slot never set reads as.
// This file holds validation, staging, coalescing, delta packing, a plain-C++ execution of a packed delta on host arrays (the record
// format k_mapdb_attr_apply reads) and the stats.  No HIP here: a plain host compiler builds it (tests/cpu_harness/mapdb_attr_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "layout.h"
#include "map_table.h"
#include "span_pool.h"

namespace ydorb {
namespace mapdb {

constexpr uint8_t kAttrGeometry = 1, kAttrDescriptor = 2;   // the flag byte, and AttrRec::set
constexpr uint8_t kAttrClear = 4;                           // staging only: clear the slot first

struct AttrRec {
  int32_t slot;
  uint8_t set;        // kAttrGeometry | kAttrDescriptor: the groups this record carries
  uint8_t clear;      // 1: flags and values of the slot are zeroed before the groups are written
  uint8_t pad0[2];
  float normal[3], minDistance, maxDistance;
  uint8_t pad1[4];
  uint8_t desc[32];
};
static_assert(sizeof(AttrRec) == 64 && offsetof(AttrRec, desc) == 32, "the kernel reads this layout, the descriptor as two uint4");

struct AttrPlan {
  int32_t nRec = 0;
  size_t bytes = 0;
  int32_t capBefore = 0, cap = 0;   // the arena covers the point table's capacity and grows with it
};

// The arrays the kernels read, on the host: the state-machine check executes deltas on them
struct AttrTables {
  std::vector<float> normal, minDistance, maxDistance;
  std::vector<uint8_t> desc, flags;
  void size(size_t cap) { normal.resize(3 * cap, 0.f); minDistance.resize(cap, 0.f); maxDistance.resize(cap, 0.f); desc.resize(32 * cap, 0); flags.resize(cap, 0); }
};

class AttrHost {
 public:
  bool enabled() const { return enabled_; }
  // pointCap: the point table's capacity now; the arena starts there
  void enable(int32_t pointCap) { if (!enabled_) { enabled_ = true; cap_ = pointCap; } }
  bool dirty() const { return !dirty_.empty(); }
  bool needsSync(int32_t pointCap) const { return enabled_ && (dirty() || pointCap != cap_); }

  void clear() {   // capacity and counters stay
    state_.clear(); normal_.clear(); min_.clear(); max_.clear(); desc_.clear(); dirty_.clear();
    lastSyncBytes_ = lastSyncRecords_ = lastWriteThrough_ = 0;
  }

  static bool checkEnabled(bool enabled, std::string& err) { return enabled ? true : fail(err, "point attributes are not enabled: call ydorb_mapdb_enable_attributes first"); }

  // nPoints: the table's count with its staged slots in it
  bool set(const int32_t* slots, int32_t n, const float* normal, const float* minDistance, const float* maxDistance, const uint8_t* desc,
           int32_t nPoints, std::string& err) {
    if (!checkEnabled(enabled_, err)) return false;
    if (n < 0) return fail(err, "negative number of point slots: %lld", n);
    const int g = (normal ? 1 : 0) + (minDistance ? 1 : 0) + (maxDistance ? 1 : 0);
    if (g != 0 && g != 3) return fail(err, "normal, min_distance and max_distance: all three or none");
    if (g == 0 && !desc) return fail(err, "null geometry group and null desc: nothing to set");
    if (n > 0 && !slots) return fail(err, "null slots");
    for (int32_t i = 0; i < n; i++)
      if (slots[i] < 0 || slots[i] >= nPoints) return fail(err, "slots[%lld]: point slot %lld outside 0..%lld", i, slots[i], (long long)nPoints - 1);
    for (int32_t i = 0; i < n; i++) {
      const int32_t s = slots[i];
      touch(s);
      if (g) {
        state_[s] |= kAttrGeometry;
        memcpy(&normal_[3 * (size_t)s], normal + 3 * (size_t)i, 12);
        min_[s] = minDistance[i]; max_[s] = maxDistance[i];
      }
      if (desc) {
        state_[s] |= kAttrDescriptor;
        memcpy(&desc_[32 * (size_t)s], desc + 32 * (size_t)i, 32);
      }
    }
    return true;
  }

  // After an accepted set_points with the same arguments: every point given as bad with an empty span is an erased point
  void pointsSet(const int32_t* slots, int32_t n, const int32_t* obsStart, const uint8_t* bad) {
    if (!enabled_) return;
    for (int32_t i = 0; i < n; i++)
      if (bad[i] && obsStart[i + 1] == obsStart[i]) erased(slots[i]);
  }
  void erased(int32_t s) {
    touch(s);
    state_[s] = kAttrClear;   // what was staged before the clear is gone
  }

  // The query slots of the searches (ydorb_mapdb_frustum_cull, ydorb_mapdb_search_local_points)
  static bool checkSlots(const int32_t* slots, int64_t n, int32_t nPoints, std::string& err) {
    for (int64_t i = 0; i < n; i++)
      if (slots[i] < 0 || slots[i] >= nPoints) return fail(err, "point_slots[%lld]: point slot %lld outside 0..%lld", i, slots[i], (long long)nPoints - 1);
    return true;
  }

  void nothingToSync() { lastSyncBytes_ = lastSyncRecords_ = 0; }
  void wroteThrough(int64_t records) { lastWriteThrough_ = records; }

  AttrPlan plan(int32_t pointCap) const {
    AttrPlan P;
    P.nRec = (int32_t)dirty_.size();
    Layout L;
    L.add(sizeof(AttrRec) * (size_t)P.nRec);
    P.bytes = L.bytes;
    P.capBefore = cap_; P.cap = pointCap;
    return P;
  }

  // Writes the delta of `P` (made by plan() with nothing staged since) into dst [P.bytes] and takes it as applied: the dirty list goes
  // and capacity and counters advance here, before the device work.  The driver therefore calls it only once nothing that follows can
  // be refused for a reason of the caller's (buffers and the grown arena are allocated first); what can still fail after it is a HIP
  // error, after which the handle's device state is not to be trusted anyway.  The older relations' pack() follow the same rule.
  void pack(const AttrPlan& P, uint8_t* dst) {
    memset(dst, 0, P.bytes);
    AttrRec* out = reinterpret_cast<AttrRec*>(dst);
    for (const int32_t s : dirty_) {
      AttrRec r;
      memset(&r, 0, sizeof(r));
      r.slot = s; r.set = state_[s] & (kAttrGeometry | kAttrDescriptor); r.clear = state_[s] & kAttrClear ? 1 : 0;
      if (r.set & kAttrGeometry) { memcpy(r.normal, &normal_[3 * (size_t)s], 12); r.minDistance = min_[s]; r.maxDistance = max_[s]; }
      if (r.set & kAttrDescriptor) memcpy(r.desc, &desc_[32 * (size_t)s], 32);
      *out++ = r;
      state_[s] = 0;
    }
    dirty_.clear();
    if (P.cap != cap_) { cap_ = P.cap; growths_++; }
    lastSyncBytes_ = (int64_t)P.bytes; lastSyncRecords_ = P.nRec;
  }

  void stats(YdMapDbAttrStats& s) const {
    s.enabled = enabled_ ? 1 : 0; s.growths = growths_; s.capacity = enabled_ ? cap_ : 0;
    s.last_attr_sync_bytes = lastSyncBytes_; s.last_attr_sync_records = lastSyncRecords_; s.last_write_through_records = lastWriteThrough_;
  }

 private:
  void touch(int32_t s) {
    if ((size_t)s >= state_.size()) {
      const size_t n = (size_t)s + 1;
      state_.resize(n, 0); normal_.resize(3 * n, 0.f); min_.resize(n, 0.f); max_.resize(n, 0.f); desc_.resize(32 * n, 0);
    }
    if (!state_[s]) dirty_.push_back(s);
  }

  bool enabled_ = false;
  int32_t cap_ = 0, growths_ = 0;
  // staged: per slot the groups named since the last sync (kAttrClear: cleared first) and their last values
  std::vector<uint8_t> state_, desc_;
  std::vector<float> normal_, min_, max_;
  std::vector<int32_t> dirty_;
  int64_t lastSyncBytes_ = 0, lastSyncRecords_ = 0, lastWriteThrough_ = 0;
};

// The packed delta executed on host arrays, step for step what the driver does on the device: grow the arena (contents kept, new slots
// zero), then k_mapdb_attr_apply.
inline void executeAttr(const AttrPlan& P, const uint8_t* delta, AttrTables& T) {
  if (T.flags.size() != (size_t)P.cap) T.size((size_t)P.cap);
  const AttrRec* rec = reinterpret_cast<const AttrRec*>(delta);
  for (int32_t i = 0; i < P.nRec; i++) {
    const AttrRec& r = rec[i];
    const size_t s = (size_t)r.slot;
    if (r.clear) {
      T.flags.at(s) = 0; T.minDistance.at(s) = 0.f; T.maxDistance.at(s) = 0.f;
      memset(&T.normal.at(3 * s), 0, 12); memset(&T.desc.at(32 * s), 0, 32);
    }
    if (r.set & kAttrGeometry) { memcpy(&T.normal.at(3 * s), r.normal, 12); T.minDistance.at(s) = r.minDistance; T.maxDistance.at(s) = r.maxDistance; }
    if (r.set & kAttrDescriptor) memcpy(&T.desc.at(32 * s), r.desc, 32);
    T.flags.at(s) |= r.set;
  }
}

}  // namespace mapdb
}  // namespace ydorb
