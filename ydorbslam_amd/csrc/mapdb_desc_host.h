// Host side of the resident table's keyframe descriptor blocks and point views (include/ydorb/c_api.h, "Resident descriptors";
// DESIGN.md section 6p).  Two relations, each a SpanHost of mapdb_rows_host.h under the pool policy of span_pool.h:
//   blocks   keyframe slot -> its descriptor matrix [n_k][32] in keypoint order; the pool is counted in descriptors (DescRow, 32 bytes),
//            every payload offset of a delta is a multiple of 16 bytes (the sections are 16-byte aligned, a row is 32 bytes).
//   views    point slot -> where the point is seen: (keyframe slot, keypoint index) pairs interleaved in one int32 span of length 2m, in
//            the order computeDistinctiveDescriptors iterates the observation container in.  The span format is the keyframe rows', and
//            so are the delta, the kernels and the host execution (k_mapdb_span_apply / k_mapdb_span_repack, executeRows).  The blocks
//            use the same two kernels, moving a row as two uint4 (mapdb_span_kernels.hip.h).
// This file adds what the two do not share with the rows: the validation of the two setters and of the query, the stats, and the
// query executed on host tables as the reference's sequential loop (distinctiveOnHost).  No HIP here: a plain host compiler builds it
// (tests/cpu_harness/mapdb_desc_check.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "map_table.h"
#include "mapdb_rows_host.h"
#include "span_pool.h"

namespace ydorb {
namespace mapdb {

struct DescRow { uint8_t b[32]; };
static_assert(sizeof(DescRow) == 32, "the kernels move a row as two uint4");

constexpr int32_t kMaxViews = 65535;   // the winner's key is (median << 16 | collected row)

using ViewTables = SpanTables<int32_t>;
using BlockTables = SpanTables<DescRow>;

inline bool checkViewPoolTotal(int64_t total, std::string& err) { return checkTotal(total, "the view pool would hold %lld entries, past INT32_MAX", err); }
inline bool checkDescPoolTotal(int64_t total, std::string& err) { return checkTotal(total, "the descriptor pool would hold %lld descriptors, past INT32_MAX", err); }

class DescHost {
 public:
  // the headers start at the point and keyframe tables' capacities; the pools start empty-handed and grow on demand (reserve())
  DescHost(int32_t pointCap, int32_t kfCap) : views(pointCap, 2), blocks(kfCap, 1) {}

  SpanHost<int32_t> views;
  SpanHost<DescRow> blocks;

  bool dirty() const { return views.dirty() || blocks.dirty(); }
  void clear() { views.clear(); blocks.clear(); }

  bool reserve(int64_t viewCap, int64_t descCap, std::string& err) {
    if (viewCap < 0 || descCap < 0) return fail(err, "negative capacity");
    if (2 * viewCap > INT32_MAX) return checkViewPoolTotal(2 * viewCap, err);
    if (descCap > INT32_MAX) return checkDescPoolTotal(descCap, err);
    if (views.poolUsed() != 0 || views.liveAfterSync() != 0 || views.dirty() || blocks.poolUsed() != 0 || blocks.liveAfterSync() != 0 || blocks.dirty())
      return fail(err, "reserve_descriptors: the pools are not empty; reserve before the first setter or after clear");
    views.reserve(2 * viewCap); blocks.reserve(descCap);
    return true;
  }

  bool setBlocks(const int32_t* kfSlots, int32_t n, const int32_t* descStart, const uint8_t* desc, std::string& err) {
    if (n < 0) return fail(err, "negative number of keyframe slots: %lld", n);
    if (!maptable::checkStarts("desc_start", descStart, n, err)) return false;
    if (n == 0) return true;
    if (!kfSlots) return fail(err, "null kf_slots");
    if (descStart[n] > 0 && !desc) return fail(err, "null desc");
    for (int32_t i = 0; i < n; i++)
      if (kfSlots[i] < 0) return fail(err, "kf_slots[%lld]: negative keyframe slot %lld", i, kfSlots[i]);
    return blocks.stage(kfSlots, n, descStart, reinterpret_cast<const DescRow*>(desc), checkDescPoolTotal, err);
  }

  // nPoints, nKeyframes: the table's counts with their staged slots in them
  bool setViews(const int32_t* slots, int32_t n, const int32_t* viewStart, const int32_t* viewKf, const int32_t* viewIdx, int32_t nPoints,
                int32_t nKeyframes, std::string& err) {
    if (n < 0) return fail(err, "negative number of point slots: %lld", n);
    if (!maptable::checkStarts("view_start", viewStart, n, err)) return false;
    if (n == 0) return true;
    if (!slots) return fail(err, "null slots");
    const int32_t N = viewStart[n];
    if (N > 0 && (!viewKf || !viewIdx)) return fail(err, "null view_kf or view_idx");
    for (int32_t i = 0; i < n; i++) {
      if (slots[i] < 0) return fail(err, "slots[%lld]: negative point slot %lld", i, slots[i]);
      if (slots[i] >= nPoints) return fail(err, "slots[%lld]: point slot %lld outside 0..%lld; set the point before its views", i, slots[i], (long long)nPoints - 1);
      if (viewStart[i + 1] - viewStart[i] > kMaxViews) return fail(err, "slots[%lld]: a span of %lld views, more than 65535", i, viewStart[i + 1] - viewStart[i]);
    }
    for (int32_t q = 0; q < N; q++) {
      if (viewKf[q] < 0 || viewKf[q] >= nKeyframes)
        return fail(err, "view %lld: keyframe slot %lld outside 0..%lld", q, viewKf[q], (long long)nKeyframes - 1);
      if (viewIdx[q] < 0) return fail(err, "view %lld: negative keypoint index %lld", q, viewIdx[q]);
    }
    if ((int64_t)N * 2 > INT32_MAX) return checkViewPoolTotal((int64_t)N * 2, err);
    pairStart_.resize((size_t)n + 1);
    pair_.resize(2 * (size_t)N);
    for (int32_t i = 0; i <= n; i++) pairStart_[(size_t)i] = 2 * viewStart[i];
    for (int32_t q = 0; q < N; q++) { pair_[2 * (size_t)q] = viewKf[q]; pair_[2 * (size_t)q + 1] = viewIdx[q]; }
    return views.stage(slots, n, pairStart_.data(), pair_.data(), checkViewPoolTotal, err);
  }

  // nPoints < 0: the nulls and the sign of n only (no handle to ask)
  static bool checkQuery(const int32_t* slots, int32_t n, int32_t nPoints, const int32_t* best, const int32_t* bestView, const uint8_t* descOut,
                         const uint8_t* status, std::string& err) {
    if (n < 0) return fail(err, "negative number of point slots: %lld", n);
    if (n > 0 && !slots) return fail(err, "null slots");
    if (n > 0 && (!best || !bestView || !descOut || !status)) return fail(err, "null output arrays");
    for (int32_t i = 0; i < n && nPoints >= 0; i++)
      if (slots[i] < 0 || slots[i] >= nPoints) return fail(err, "slots[%lld]: point slot %lld outside 0..%lld", i, slots[i], (long long)nPoints - 1);
    return true;
  }

  void stats(YdMapDbDescStats& s) const {
    YdMapDbRowStats v, b;
    views.stats(v); blocks.stats(b);
    s.n_views = v.n_entries / 2; s.n_descriptors = b.n_entries;
    s.view_pool_used = v.pool_used / 2; s.view_pool_capacity = v.pool_capacity / 2;
    s.desc_pool_used = b.pool_used; s.desc_pool_capacity = b.pool_capacity;
    s.view_repacks_kept = v.repacks_kept; s.view_repacks_grown = v.repacks_grown;
    s.desc_repacks_kept = b.repacks_kept; s.desc_repacks_grown = b.repacks_grown;
    s.last_desc_sync_bytes = v.last_row_sync_bytes + b.last_row_sync_bytes;
    s.last_desc_sync_records = v.last_row_sync_records + b.last_row_sync_records;
  }

 private:
  std::vector<int32_t> pairStart_, pair_;   // scratch of setViews
};

// view_start [nPoints + 1] / view_kf / view_idx from the view headers; a slot at or past nHeld has no views
inline void flattenViews(int32_t nPoints, int32_t nHeld, const int32_t* start, const int32_t* len, const int32_t* pool, int32_t* viewStart, int32_t* viewKf,
                         int32_t* viewIdx) {
  int32_t at = 0;
  viewStart[0] = 0;
  for (int32_t p = 0; p < nPoints; p++) {
    const int32_t m = p < nHeld ? len[p] / 2 : 0;
    for (int32_t v = 0; v < m; v++) { viewKf[at + v] = pool[start[p] + 2 * v]; viewIdx[at + v] = pool[start[p] + 2 * v + 1]; }
    at += m;
    viewStart[p + 1] = at;
  }
}

// MapPoint::computeDistinctiveDescriptors on gathered rows, the rule of ydorb_distinctive_descriptors (c_api.h): the first row whose
// sorted distance row has the least entry at (int)(0.5 m).  rows [m] point at 32 bytes each; m > 0.
inline int32_t distinctiveOfRows(const std::vector<const uint8_t*>& rows) {
  const size_t m = rows.size();
  std::vector<int> dist(m * m, 0);
  for (size_t i = 0; i < m; i++)
    for (size_t j = i + 1; j < m; j++) {
      int d = 0;
      for (int b = 0; b < 32; b++) d += __builtin_popcount((unsigned)(rows[i][b] ^ rows[j][b]));
      dist[i * m + j] = dist[j * m + i] = d;
    }
  int bestMedian = INT32_MAX;
  int32_t bestIdx = 0;
  std::vector<int> v(m);
  for (size_t i = 0; i < m; i++) {
    std::copy(dist.begin() + (ptrdiff_t)(i * m), dist.begin() + (ptrdiff_t)((i + 1) * m), v.begin());
    std::sort(v.begin(), v.end());
    const int median = v[(size_t)(0.5 * (double)m)];
    if (median < bestMedian) { bestMedian = median; bestIdx = (int32_t)i; }
  }
  return bestIdx;
}

// ydorb_mapdb_distinctive_descriptors on host tables, written as the reference's loop: a bad point returns first; the observations are
// walked in order and those of a bad keyframe (no block) skipped; nothing collected returns; then the rule above.  A view past its
// block's length is what the reference cannot hold: status 3, as on the device.  bad [nPoints]: the point table's flags.
inline void distinctiveOnHost(const ViewTables& V, const BlockTables& B, const uint8_t* bad, const int32_t* slots, int32_t n, int32_t* best,
                              int32_t* bestView, uint8_t* descOut, uint8_t* status) {
  for (int32_t q = 0; q < n; q++) {
    const int32_t s = slots[q];
    best[q] = -1; bestView[2 * q] = bestView[2 * q + 1] = 0;
    memset(descOut + 32 * (size_t)q, 0, 32);
    if (bad[s]) { status[q] = YDORB_MAPDESC_BAD; continue; }
    const int32_t m = (size_t)s < V.rowLen.size() ? V.rowLen[(size_t)s] / 2 : 0;
    std::vector<const uint8_t*> rows;
    std::vector<int32_t> at;   // the span position of each collected row
    bool outOfRange = false;
    for (int32_t v = 0; v < m && !outOfRange; v++) {
      const int32_t kf = V.pool.at((size_t)(V.rowStart[(size_t)s] + 2 * v)), idx = V.pool.at((size_t)(V.rowStart[(size_t)s] + 2 * v + 1));
      const int32_t len = (size_t)kf < B.rowLen.size() ? B.rowLen[(size_t)kf] : 0;
      if (len == 0) continue;
      if (idx >= len) { outOfRange = true; break; }
      rows.push_back(B.pool.at((size_t)(B.rowStart[(size_t)kf] + idx)).b);
      at.push_back(v);
    }
    if (outOfRange) { status[q] = YDORB_MAPDESC_VIEW_OUT_OF_RANGE; continue; }
    if (rows.empty()) { status[q] = YDORB_MAPDESC_NO_DESCRIPTORS; continue; }
    const int32_t w = distinctiveOfRows(rows), v = at[(size_t)w];
    status[q] = YDORB_MAPDESC_UPDATED;
    best[q] = v;
    bestView[2 * q] = V.pool[(size_t)(V.rowStart[(size_t)s] + 2 * v)]; bestView[2 * q + 1] = V.pool[(size_t)(V.rowStart[(size_t)s] + 2 * v + 1)];
    memcpy(descOut + 32 * (size_t)q, rows[(size_t)w], 32);
  }
}

}  // namespace mapdb
}  // namespace ydorb
