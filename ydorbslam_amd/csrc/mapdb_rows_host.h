// Host side of the resident table's keyframe rows (include/ydorb/c_api.h, "Keyframe rows"): a keyframe's
// map-point vector as point slots in keypoint order, -1 = a null entry.  Beside mapdb_host.h's Host, a class and a delta of its own:
// validation, the host mirror of every row, coalescing, the packing of one row delta and a plain-C++ execution of a
// packed delta on host arrays in the record format the kernels read (mapdb_span_kernels.hip.h), so that the state machine runs without
// a device (tests/cpu_harness/mapdb_rows_check.cpp).  No HIP here: a plain host compiler builds it.
//   staging   setRows / setEntries validate, then write the mirror.  A row is clean, entry-dirty or fully dirty.  A fully dirty row is
//             packed once from the mirror, so only its last value travels and a later entry change lands inside it.  Entry changes to a
//             resident row are kept per (keyframe, index) and packed with the mirror's value: one record per address, last value wins,
//             and the apply kernel never has two lanes storing to one address.
//   delta     [header records][entry records][payload point slots][repack offsets], every section 16-byte aligned.  Records are in the
//             order their rows / entries were first dirtied.  An entry record carries the pool position itself: the host knows where
//             every row lies once the delta's own repack has run.
//   pool      the rows lie in a SpanPool of their own, a replaced or erased row being its garbage: span_pool.h has the policy, and the
//             growth rule of the headers (rowStart / rowLen per keyframe slot), which is the keyframe table's.
// The state machine is a template over the span's element, SpanHost<T>; RowsHost is SpanHost<int32_t>.  mapdb_desc_host.h keeps two more
// relations in it: a point's views (int32 spans keyed by point slot, staged through stage() after a validation of their own) and a
// keyframe's descriptor block (spans of 32-byte rows).  setRows / setEntries and the two query checks belong to the keyframe rows.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "map_table.h"
#include "span_pool.h"

namespace ydorb {
namespace mapdb {

struct RowHeaderRec { int32_t kf, start, len, pad; };
struct RowEntryRec { int32_t at, value; };   // at: the pool position
static_assert(sizeof(RowHeaderRec) == 16 && sizeof(RowEntryRec) == 8, "the kernels read these layouts");

struct RowPlan : PoolPlan {
  int32_t nHeaderRec = 0, nEntryRec = 0;
  size_t oHeader = 0, oEntry = 0, oPayload = 0, oNewOff = 0, bytes = 0;
  int32_t nKfBefore = 0, hdrCapBefore = 0, hdrCap = 0;   // the device headers hold rows below nKfBefore: the repack covers those
};

// the arrays the kernels keep, on the host
template <class T> struct SpanTables {
  std::vector<int32_t> rowStart, rowLen;
  std::vector<T> pool;
};
using RowTables = SpanTables<int32_t>;

// row_start [nKf + 1] / point_slot from per-slot headers; a slot at or past `nHeld` has no row
template <class T> void flattenRows(int32_t nKf, int32_t nHeld, const int32_t* rowStart, const int32_t* rowLen, const T* pool, int32_t* outStart,
                                    T* outSlot) {
  int32_t at = 0;
  outStart[0] = 0;
  for (int32_t k = 0; k < nKf; k++) {
    const int32_t len = k < nHeld ? rowLen[k] : 0;
    if (len > 0) memcpy(outSlot + at, pool + rowStart[k], sizeof(T) * (size_t)len);
    at += len;
    outStart[k + 1] = at;
  }
}

template <class T> class SpanHost {
 public:
  SpanHost(int32_t hdrCap, int64_t poolCap) : hdrCap_(std::max(hdrCap, 1)), pool_(poolCap) {}

  int32_t nKeyframes() const { return (int32_t)row_.size(); }   // 1 + the highest slot a row call named
  int32_t hdrCap() const { return hdrCap_; }
  int64_t poolCap() const { return pool_.cap; }
  int64_t poolUsed() const { return pool_.used; }
  int64_t liveAfterSync() const { return pool_.pending; }
  int32_t headerGrowths() const { return hdrGrowths_; }
  bool dirty() const { return !dirtyRows_.empty() || !dirtyEntries_.empty(); }
  int32_t lenOf(int32_t kf) const { return kf < nKeyframes() ? (int32_t)row_[(size_t)kf].size() : 0; }   // staged changes included
  const std::vector<T>& rowOf(int32_t kf) const { return row_[(size_t)kf]; }
  int32_t offOf(int32_t kf) const { return kf < nKeyframes() ? off_[(size_t)kf] : 0; }   // where the device holds the span; with nothing staged

  void clear() {
    row_.clear(); off_.clear(); len_.clear(); state_.clear();
    dropStaged();
    pool_.clear();
    nKfSynced_ = 0;
    lastSyncBytes_ = lastSyncRecords_ = 0;
  }

  // nPoints: the point table's count with its staged points in it
  bool setRows(const int32_t* kfSlots, int32_t n, const int32_t* rowStart, const int32_t* pointSlot, int32_t nPoints, std::string& err) {
    if (n < 0) return fail(err, "negative number of keyframe slots: %lld", n);
    if (!maptable::checkStarts("row_start", rowStart, n, err)) return false;
    if (n == 0) return true;
    if (!kfSlots) return fail(err, "null kf_slots");
    const int32_t N = rowStart[n];
    if (N > 0 && !pointSlot) return fail(err, "null point_slot");
    for (int32_t i = 0; i < n; i++)
      if (kfSlots[i] < 0) return fail(err, "kf_slots[%lld]: negative keyframe slot %lld", i, kfSlots[i]);
    for (int32_t q = 0; q < N; q++)
      if (pointSlot[q] < -1 || pointSlot[q] >= nPoints)
        return fail(err, "row entry %lld: point slot %lld outside -1..%lld; set the point before a row names it", q, pointSlot[q], (long long)nPoints - 1);
    return stage(kfSlots, n, rowStart, pointSlot, checkRowPoolTotal, err);
  }

  // Stages whole spans the caller has validated (n > 0, starts well formed, no negative slot): value [start[n]].  check: the pool's
  // INT32_MAX guard, as in SpanPool::admits.
  template <class Check> bool stage(const int32_t* slots, int32_t n, const int32_t* start, const T* value, Check check, std::string& err) {
    if (!pool_.admits(slots, n, start, [this](int32_t k) { return lenOf(k); }, check, err)) return false;
    for (int32_t i = 0; i < n; i++) {
      const int32_t k = slots[i];
      growTo(k);
      if (state_[k] != kFull) { state_[k] = kFull; dirtyRows_.push_back(k); }
      pool_.restaged(lenOf(k), start[i + 1] - start[i]);
      if (start[i + 1] > start[i]) row_[k].assign(value + start[i], value + start[i + 1]);
      else row_[k].clear();
    }
    return true;
  }

  // An empty pool takes the capacity it is told: before anything was staged or synced, or after clear().
  bool reserve(int64_t poolCap) {
    if (pool_.used != 0 || pool_.pending != 0 || dirty()) return false;
    pool_.cap = std::max<int64_t>(poolCap, 1);
    return true;
  }

  bool setEntries(const int32_t* kfSlot, const int32_t* idx, const int32_t* pointSlot, int32_t n, int32_t nPoints, std::string& err) {
    if (n < 0) return fail(err, "negative number of row entries: %lld", n);
    if (n == 0) return true;
    if (!kfSlot || !idx || !pointSlot) return fail(err, "null kf_slot, idx or point_slot");
    for (int32_t i = 0; i < n; i++) {
      if (kfSlot[i] < 0) return fail(err, "kf_slot[%lld]: negative keyframe slot %lld", i, kfSlot[i]);
      if (idx[i] < 0 || idx[i] >= lenOf(kfSlot[i]))
        return fail(err, "idx[%lld]: index %lld outside the row of %lld entries", i, idx[i], lenOf(kfSlot[i]));
      if (pointSlot[i] < -1 || pointSlot[i] >= nPoints)
        return fail(err, "point_slot[%lld]: point slot %lld outside -1..%lld; set the point before a row names it", i, pointSlot[i], (long long)nPoints - 1);
    }
    for (int32_t i = 0; i < n; i++) {
      const int32_t k = kfSlot[i];
      row_[k][(size_t)idx[i]] = pointSlot[i];
      if (state_[k] == kFull) continue;   // lands inside the staged row
      const uint64_t key = ((uint64_t)(uint32_t)k << 32) | (uint32_t)idx[i];
      if (entryAt_.emplace(key, dirtyEntries_.size()).second) dirtyEntries_.push_back(key);
    }
    return true;
  }

  // the keyframe slots of a query: below nKfAll, the table's n_keyframes
  static bool checkKfSlots(const int32_t* kfSlots, int32_t n, int32_t nKfAll, std::string& err) {
    if (n < 0) return fail(err, "negative number of keyframe slots: %lld", n);
    if (n > 0 && !kfSlots) return fail(err, "null kf_slots");
    for (int32_t i = 0; i < n; i++)
      if (kfSlots[i] < 0 || kfSlots[i] >= nKfAll) return fail(err, "kf_slots[%lld]: keyframe slot %lld outside 0..%lld", i, kfSlots[i], (long long)nKfAll - 1);
    return true;
  }
  static bool checkSeen(const int32_t* seen, int32_t n, int32_t nPoints, std::string& err) {
    if (n < 0) return fail(err, "negative number of seen points: %lld", n);
    if (n > 0 && !seen) return fail(err, "null seen_points");
    for (int32_t i = 0; i < n; i++)
      if (seen[i] < -1 || seen[i] >= nPoints) return fail(err, "seen_points[%lld]: point slot %lld outside -1..%lld", i, seen[i], (long long)nPoints - 1);
    return true;
  }

  void stats(YdMapDbRowStats& s) const {
    s.n_entries = pool_.pending; s.pool_used = pool_.used; s.pool_capacity = pool_.cap;
    s.repacks_kept = pool_.repacksKept; s.repacks_grown = pool_.repacksGrown;
    s.header_growths = hdrGrowths_; s.header_capacity = hdrCap_;
    s.last_row_sync_bytes = lastSyncBytes_; s.last_row_sync_records = lastSyncRecords_;
  }
  void nothingToSync() { lastSyncBytes_ = lastSyncRecords_ = 0; }

  RowPlan plan() const {
    RowPlan P;
    int64_t replaced = 0, incoming = 0;
    for (const int32_t k : dirtyRows_) { P.nHeaderRec++; incoming += (int64_t)row_[k].size(); replaced += len_[k]; }
    for (const uint64_t key : dirtyEntries_)
      if (state_[(size_t)(key >> 32)] != kFull) P.nEntryRec++;   // a row staged after its entry change carries the entry itself
    static_cast<PoolPlan&>(P) = pool_.plan(replaced, incoming);
    P.nKfBefore = nKfSynced_; P.hdrCapBefore = hdrCap_; P.hdrCap = grownCap(nKeyframes(), hdrCap_);
    Layout L;
    P.oHeader = L.add(sizeof(RowHeaderRec) * (size_t)P.nHeaderRec); P.oEntry = L.add(sizeof(RowEntryRec) * (size_t)P.nEntryRec);
    P.oPayload = L.add(sizeof(T) * (size_t)P.nPayload);
    P.oNewOff = L.add(P.repack ? 4 * (size_t)P.nKfBefore : 0); P.bytes = L.bytes;
    return P;
  }

  // Writes the delta of `P` (made by plan() with nothing staged since) into dst [P.bytes] and takes it as applied.
  void pack(const RowPlan& P, uint8_t* dst) {
    memset(dst, 0, P.bytes);
    if (P.repack)
      survivorOffsets(P.nKfBefore, len_.data(), off_.data(), reinterpret_cast<int32_t*>(dst + P.oNewOff), [this](int32_t k) { return state_[k] == kFull; });
    RowHeaderRec* hr = reinterpret_cast<RowHeaderRec*>(dst + P.oHeader);
    T* pay = reinterpret_cast<T*>(dst + P.oPayload);
    int64_t cursor = 0;
    for (const int32_t k : dirtyRows_) {
      const int32_t len = (int32_t)row_[k].size();
      off_[k] = (int32_t)(P.tail + cursor); len_[k] = len;
      *hr++ = RowHeaderRec{k, off_[k], len, 0};
      if (len) memcpy(pay + cursor, row_[k].data(), sizeof(T) * (size_t)len);
      cursor += len;
    }
    RowEntryRec* er = reinterpret_cast<RowEntryRec*>(dst + P.oEntry);
    for (const uint64_t key : dirtyEntries_) {
      const int32_t k = (int32_t)(key >> 32), i = (int32_t)(uint32_t)key;
      if (state_[k] == kFull) continue;
      *er++ = RowEntryRec{off_[k] + i, entryValue(row_[k][(size_t)i])};   // off_: after this delta's repack
    }
    for (const int32_t k : dirtyRows_) state_[k] = kClean;
    dropStaged();
    pool_.commit(P);
    if (P.hdrCap != hdrCap_) { hdrCap_ = P.hdrCap; hdrGrowths_++; }
    nKfSynced_ = nKeyframes();
    lastSyncBytes_ = (int64_t)P.bytes; lastSyncRecords_ = (int64_t)P.nHeaderRec + P.nEntryRec;
  }

 private:
  enum : uint8_t { kClean = 0, kFull = 1 };
  void growTo(int32_t k) {
    if (k < nKeyframes()) return;
    const size_t n = (size_t)k + 1;
    row_.resize(n); off_.resize(n, 0); len_.resize(n, 0); state_.resize(n, kClean);
  }
  void dropStaged() { dirtyRows_.clear(); dirtyEntries_.clear(); entryAt_.clear(); }
  static int32_t entryValue(int32_t v) { return v; }
  template <class U> static int32_t entryValue(const U&) { return 0; }   // only int32 spans have single-entry records

  std::vector<std::vector<T>> row_;   // the mirror: what the device holds once the staged changes are applied
  std::vector<int32_t> off_, len_;          // where the device holds each row now
  std::vector<uint8_t> state_;
  std::vector<int32_t> dirtyRows_;
  std::vector<uint64_t> dirtyEntries_;      // (keyframe << 32) | index, in the order first changed
  std::unordered_map<uint64_t, size_t> entryAt_;
  int32_t hdrCap_, nKfSynced_ = 0, hdrGrowths_ = 0;
  SpanPool pool_;
  int64_t lastSyncBytes_ = 0, lastSyncRecords_ = 0;
};
using RowsHost = SpanHost<int32_t>;

// ---------------------------------------------------------------------------------------------------------------------------------
// The packed delta executed on host arrays, step for step what the driver does on the device: grow the headers (contents kept, new
// slots empty), repack (k_mapdb_span_repack), apply (k_mapdb_span_apply).
template <class E> void executeRows(const RowPlan& P, const uint8_t* delta, SpanTables<E>& T) {
  if (T.rowStart.size() != (size_t)P.hdrCap) { T.rowStart.resize((size_t)P.hdrCap, 0); T.rowLen.resize((size_t)P.hdrCap, 0); }
  if (T.pool.size() != (size_t)P.poolCapBefore) T.pool.resize((size_t)P.poolCapBefore);
  if (P.repack) {
    const int32_t* newOff = reinterpret_cast<const int32_t*>(delta + P.oNewOff);
    std::vector<E> fresh((size_t)P.poolCap);
    for (int32_t k = 0; k < P.nKfBefore; k++) {
      if (newOff[k] < 0) continue;
      for (int32_t q = 0; q < T.rowLen[k]; q++) fresh.at((size_t)(newOff[k] + q)) = T.pool.at((size_t)(T.rowStart[k] + q));
      T.rowStart[k] = newOff[k];
    }
    T.pool.swap(fresh);
  }
  const RowHeaderRec* hr = reinterpret_cast<const RowHeaderRec*>(delta + P.oHeader);
  for (int32_t i = 0; i < P.nHeaderRec; i++) { T.rowStart.at((size_t)hr[i].kf) = hr[i].start; T.rowLen.at((size_t)hr[i].kf) = hr[i].len; }
  const RowEntryRec* er = reinterpret_cast<const RowEntryRec*>(delta + P.oEntry);
  for (int32_t i = 0; i < P.nEntryRec; i++) memcpy(&T.pool.at((size_t)er[i].at), &er[i].value, 4);   // int32 spans only
  const E* pay = reinterpret_cast<const E*>(delta + P.oPayload);
  for (int64_t i = 0; i < P.nPayload; i++) T.pool.at((size_t)(P.tail + i)) = pay[i];
}

}  // namespace mapdb
}  // namespace ydorb
