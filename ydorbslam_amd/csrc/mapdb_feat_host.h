// Host side of the resident table's keyframe features (include/ydorb/c_api.h, "Resident keyframe features"):
// keyframe slot -> the keyframe's undistorted keypoints [n_k] and right_x [n_k], in keypoint order: the order and the n_k of its
// descriptor block.  One more SpanHost of mapdb_rows_host.h under the pool policy of span_pool.h; the relation is opt-in, like the
// point attributes: a handle that never enables it keeps an empty FeatHost and nothing is allocated, launched or counted for it.
//   staging   set_keyframe_features validates, then stages whole spans: a keyframe's features go up once, a span of length 0 erases
//             them, a slot named several times between two syncs travels once with its last value.
//   delta     the span relation's: [header records][payload][repack offsets].  A payload element is a FeatRec of 32 bytes, the
//             keypoint and its right_x side by side, so it moves as two 16-byte loads.
//   device    ONE span (start, length) per keyframe indexes TWO arrays of one arena of 32 bytes per pool entry: KeyPoint [cap] at its
//             base and float [cap] behind it at byte 28 * cap.  Both are contiguous per keyframe, so a FrameDev (grid_build.hip.h)
//             points straight into them.  The apply kernel splits a payload element into the two, which is why the relation keeps
//             kernels of its own (mapdb_feat_kernels.hip.h) beside the span kernels the other three relations share; its driver
//             side is the same SpanDev<T> (map_resident.hip).
// This file holds the validation, the stats, the export's flattening and a plain-C++ execution of a packed delta on host arrays in the
// layout the kernels keep (mapdb_feat_kernels.hip.h).  No HIP here: a plain host compiler builds it (tests/cpu_harness/mapdb_feat_check.cpp).
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

struct FeatRec { YdKeyPoint kp; float rightX; };
static_assert(sizeof(YdKeyPoint) == 28 && sizeof(FeatRec) == 32 && offsetof(FeatRec, rightX) == 28, "the kernels move a record as two uint4");

constexpr int32_t kMaxFeatures = 65535;   // the matcher's records carry a 16-bit keypoint index
constexpr int32_t kMaxOctave = 7;         // the fuse search indexes an 8-entry sigma table with it

inline bool checkFeatPoolTotal(int64_t total, std::string& err) { return checkTotal(total, "the feature pool would hold %lld features, past INT32_MAX", err); }

// The arrays the kernels keep, on the host: kps and rightX are the two halves of one arena of `cap` pool entries
struct FeatTables {
  std::vector<int32_t> start, len;
  std::vector<YdKeyPoint> kps;
  std::vector<float> rightX;
};

class FeatHost {
 public:
  explicit FeatHost(int32_t kfCap) : feats(kfCap, 1) {}

  SpanHost<FeatRec> feats;

  bool enabled() const { return enabled_; }
  void enable() { enabled_ = true; }
  bool dirty() const { return feats.dirty(); }
  void clear() { feats.clear(); }   // capacities and counters stay

  static bool checkEnabled(bool enabled, std::string& err) {
    return enabled ? true : fail(err, "keyframe features are not enabled: call ydorb_mapdb_enable_features first");
  }

  // right_x may be null: every entry is stored as -1.0f
  bool set(const int32_t* kfSlots, int32_t n, const int32_t* featStart, const YdKeyPoint* kps, const float* rightX, std::string& err) {
    if (!checkEnabled(enabled_, err)) return false;
    if (n < 0) return fail(err, "negative number of keyframe slots: %lld", n);
    if (!maptable::checkStarts("feat_start", featStart, n, err)) return false;
    if (n == 0) return true;
    if (!kfSlots) return fail(err, "null kf_slots");
    const int32_t N = featStart[n];
    if (N > 0 && !kps) return fail(err, "null kps");
    for (int32_t i = 0; i < n; i++) {
      if (kfSlots[i] < 0) return fail(err, "kf_slots[%lld]: negative keyframe slot %lld", i, kfSlots[i]);
      if (featStart[i + 1] - featStart[i] > kMaxFeatures)
        return fail(err, "kf_slots[%lld]: a span of %lld features, more than 65535", i, featStart[i + 1] - featStart[i]);
    }
    for (int32_t q = 0; q < N; q++)
      if (kps[q].octave < 0 || kps[q].octave > kMaxOctave) return fail(err, "feature %lld: octave %lld outside 0..7", q, kps[q].octave);
    rec_.resize((size_t)N);
    for (int32_t q = 0; q < N; q++) { rec_[(size_t)q].kp = kps[q]; rec_[(size_t)q].rightX = rightX ? rightX[q] : -1.0f; }
    return feats.stage(kfSlots, n, featStart, rec_.data(), checkFeatPoolTotal, err);
  }

  void stats(YdMapDbFeatStats& s) const {
    YdMapDbRowStats r;
    feats.stats(r);
    s.enabled = enabled_ ? 1 : 0;
    s.n_features = r.n_entries; s.pool_used = r.pool_used; s.pool_capacity = r.pool_capacity;
    s.repacks_kept = r.repacks_kept; s.repacks_grown = r.repacks_grown;
    s.last_feat_sync_bytes = r.last_row_sync_bytes; s.last_feat_sync_records = r.last_row_sync_records;
  }

 private:
  bool enabled_ = false;
  std::vector<FeatRec> rec_;   // scratch of set
};

// feat_start [nKf + 1] / kps / right_x from the per-slot headers; a slot at or past nHeld has no features
inline void flattenFeatures(int32_t nKf, int32_t nHeld, const int32_t* start, const int32_t* len, const YdKeyPoint* kps, const float* rightX,
                            int32_t* featStart, YdKeyPoint* outKps, float* outRightX) {
  int32_t at = 0;
  featStart[0] = 0;
  for (int32_t k = 0; k < nKf; k++) {
    const int32_t m = k < nHeld ? len[k] : 0;
    if (m > 0) { memcpy(outKps + at, kps + start[k], sizeof(YdKeyPoint) * (size_t)m); memcpy(outRightX + at, rightX + start[k], 4 * (size_t)m); }
    at += m;
    featStart[k + 1] = at;
  }
}

// The packed delta executed on host arrays, step for step what the driver does on the device: grow the headers (contents kept, new
// slots empty), repack (k_mapdb_feat_repack: one span, both arrays), apply (k_mapdb_feat_apply: header record r owns the payload
// elements [r.start - tail, r.start - tail + r.len) and splits each into the two arrays).
inline void executeFeatures(const RowPlan& P, const uint8_t* delta, FeatTables& T) {
  if (T.start.size() != (size_t)P.hdrCap) { T.start.resize((size_t)P.hdrCap, 0); T.len.resize((size_t)P.hdrCap, 0); }
  if (T.kps.size() != (size_t)P.poolCapBefore) { T.kps.resize((size_t)P.poolCapBefore); T.rightX.resize((size_t)P.poolCapBefore); }
  if (P.repack) {
    const int32_t* newOff = reinterpret_cast<const int32_t*>(delta + P.oNewOff);
    std::vector<YdKeyPoint> kps((size_t)P.poolCap);
    std::vector<float> rightX((size_t)P.poolCap);
    for (int32_t k = 0; k < P.nKfBefore; k++) {
      if (newOff[k] < 0) continue;
      for (int32_t q = 0; q < T.len[(size_t)k]; q++) {
        kps.at((size_t)(newOff[k] + q)) = T.kps.at((size_t)(T.start[(size_t)k] + q));
        rightX.at((size_t)(newOff[k] + q)) = T.rightX.at((size_t)(T.start[(size_t)k] + q));
      }
      T.start[(size_t)k] = newOff[k];
    }
    T.kps.swap(kps); T.rightX.swap(rightX);
  }
  const RowHeaderRec* hr = reinterpret_cast<const RowHeaderRec*>(delta + P.oHeader);
  const FeatRec* pay = reinterpret_cast<const FeatRec*>(delta + P.oPayload);
  for (int32_t i = 0; i < P.nHeaderRec; i++) {
    T.start.at((size_t)hr[i].kf) = hr[i].start; T.len.at((size_t)hr[i].kf) = hr[i].len;
    for (int32_t q = 0; q < hr[i].len; q++) {
      const FeatRec& r = pay[(size_t)(hr[i].start - P.tail) + (size_t)q];
      T.kps.at((size_t)(hr[i].start + q)) = r.kp; T.rightX.at((size_t)(hr[i].start + q)) = r.rightX;
    }
  }
}

}  // namespace mapdb
}  // namespace ydorb
