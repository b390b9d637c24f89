// Host side of the resident table's keyframe BoW feature vectors (include/ydorb/c_api.h, "Resident BoW feature vectors"; DESIGN.md
// section 6t): keyframe slot -> the keyframe's DBoW3::FeatureVector flattened in map order, nodes ascending and within a node the
// features in the vector's order.  The element is the pair (node id, feature index).  One more SpanHost of mapdb_rows_host.h under the
// pool policy of span_pool.h; the relation is opt-in, like the keyframe features: a handle that never enables it keeps an empty
// BowHost and nothing is allocated, launched or counted for it.
//   staging   set_keyframe_bow validates, then stages whole spans: a keyframe's feature vector never changes, so it goes up once; a
//             span of length 0 erases it; a slot named several times between two syncs travels once with its last value.
//   delta     the span relation's: [header records][payload][repack offsets].  A payload element is a BowRec of two ints, which the
//             plain span kernels (mapdb_span_kernels.hip.h) move as two int units: no kernel of its own.
// This file holds the validation, the stats, the export's flattening and a plain-C++ execution of a packed delta on host arrays
// (executeRows of mapdb_rows_host.h over BowRec).  No HIP here: a plain host compiler builds it (tests/cpu_harness/mapdb_bow_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "map_table.h"
#include "mapdb_rows_host.h"
#include "span_pool.h"

namespace ydorb {
namespace mapdb {

struct BowRec { int32_t node, feat; };
static_assert(sizeof(BowRec) == 8, "the span kernels move a record as two ints");

constexpr int32_t kMaxBowEntries = 65535;   // a keyframe has at most 65535 features and each lies under one node
constexpr int32_t kMaxBowFeature = 65534;   // the highest index of a span of 65535 features

inline bool checkBowPoolTotal(int64_t total, std::string& err) { return checkTotal(total, "the BoW pool would hold %lld entries, past INT32_MAX", err); }

using BowTables = SpanTables<BowRec>;

class BowHost {
 public:
  explicit BowHost(int32_t kfCap) : spans(kfCap, 1) {}

  SpanHost<BowRec> spans;

  bool enabled() const { return enabled_; }
  void enable() { enabled_ = true; }
  bool dirty() const { return spans.dirty(); }
  void clear() { spans.clear(); }   // capacities and counters stay

  static bool checkEnabled(bool enabled, std::string& err) {
    return enabled ? true : fail(err, "keyframe BoW feature vectors are not enabled: call ydorb_mapdb_enable_bow first");
  }

  // node_id is DBoW3's NodeId, an unsigned int: an id of 2^31 or more is refused, the device compares ids as ints
  bool set(const int32_t* kfSlots, int32_t n, const int32_t* bowStart, const uint32_t* nodeId, const int32_t* feat, std::string& err) {
    if (!checkEnabled(enabled_, err)) return false;
    if (n < 0) return fail(err, "negative number of keyframe slots: %lld", n);
    if (!maptable::checkStarts("bow_start", bowStart, n, err)) return false;
    if (n == 0) return true;
    if (!kfSlots) return fail(err, "null kf_slots");
    const int32_t N = bowStart[n];
    if (N > 0 && (!nodeId || !feat)) return fail(err, "null node_id or feat");
    for (int32_t i = 0; i < n; i++) {
      if (kfSlots[i] < 0) return fail(err, "kf_slots[%lld]: negative keyframe slot %lld", i, kfSlots[i]);
      if (bowStart[i + 1] - bowStart[i] > kMaxBowEntries)
        return fail(err, "kf_slots[%lld]: a span of %lld entries, more than 65535", i, bowStart[i + 1] - bowStart[i]);
    }
    seen_.assign((size_t)kMaxBowFeature + 1, -1);   // the span that named a feature index last
    for (int32_t i = 0; i < n; i++)
      for (int32_t q = bowStart[i]; q < bowStart[i + 1]; q++) {
        if (nodeId[q] > (uint32_t)INT32_MAX) return fail(err, "entry %lld: node id %lld outside 0..2147483647", q, (long long)nodeId[q]);
        if (q > bowStart[i] && nodeId[q] < nodeId[q - 1])
          return fail(err, "entry %lld: node id %lld after %lld, the nodes of a span ascend", q, (long long)nodeId[q], (long long)nodeId[q - 1]);
        if (feat[q] < 0 || feat[q] > kMaxBowFeature) return fail(err, "entry %lld: feature index %lld outside 0..65534", q, feat[q]);
        if (seen_[(size_t)feat[q]] == i) return fail(err, "entry %lld: feature index %lld repeats inside its span", q, feat[q]);
        seen_[(size_t)feat[q]] = i;
      }
    rec_.resize((size_t)N);
    for (int32_t q = 0; q < N; q++) rec_[(size_t)q] = BowRec{(int32_t)nodeId[q], feat[q]};
    return spans.stage(kfSlots, n, bowStart, rec_.data(), checkBowPoolTotal, err);
  }

  void stats(YdMapDbBowStats& s) const {
    YdMapDbRowStats r;
    spans.stats(r);
    s.enabled = enabled_ ? 1 : 0;
    s.n_entries = r.n_entries; s.pool_used = r.pool_used; s.pool_capacity = r.pool_capacity;
    s.repacks_kept = r.repacks_kept; s.repacks_grown = r.repacks_grown;
    s.last_bow_sync_bytes = r.last_row_sync_bytes; s.last_bow_sync_records = r.last_row_sync_records;
  }

 private:
  bool enabled_ = false;
  std::vector<BowRec> rec_;      // scratch of set
  std::vector<int32_t> seen_;
};

// bow_start [nKf + 1] / node_id / feat from the per-slot headers; a slot at or past nHeld has no span
inline void flattenBow(int32_t nKf, int32_t nHeld, const int32_t* start, const int32_t* len, const BowRec* pool, int32_t* bowStart, uint32_t* nodeId,
                       int32_t* feat) {
  int32_t at = 0;
  bowStart[0] = 0;
  for (int32_t k = 0; k < nKf; k++) {
    const int32_t m = k < nHeld ? len[k] : 0;
    for (int32_t q = 0; q < m; q++) { nodeId[at + q] = (uint32_t)pool[start[k] + q].node; feat[at + q] = pool[start[k] + q].feat; }
    at += m;
    bowStart[k + 1] = at;
  }
}

}  // namespace mapdb
}  // namespace ydorb
