// Host side of the resident map table (include/ydorb/c_api.h, "Resident map table"): the validation of its
// entries, the host mirror of the per-slot fixed records, the coalescing of staged changes, the packing of one delta
// and a plain-C++ execution of a packed delta on host arrays in the record format the kernels read (mapdb_kernels.hip.h), so that the
// whole state machine runs without a device (tests/cpu_harness/mapdb_host_check.cpp).  No HIP here: a plain host compiler builds it.
//   staging   set_points / set_positions / set_centres validate, then write the mirror and mark the slot dirty.  A point slot is clean,
//             position-dirty or fully dirty; a full record supersedes a position record and a later position lands in the full record,
//             so one slot yields one record and the apply kernel never has two lanes writing one address.  Staged spans wait in a host
//             arena; of a slot staged several times only the last span is packed.
//   delta     [point records][position records][centre records][payload keyframe slots][payload level bytes][repack offsets], every
//             section 16-byte aligned.  Records are in the order their slots were first dirtied.
//   pool      the observation spans lie in a span_pool.h SpanPool: the policy, its accounting and the table growth rule are there.
//   correct   ydorb_mapdb_correct's validation, keyframe rank table and claim pass (planCorrection), and what the mirror takes from the
//             read-back (correctionApplied): DESIGN.md section 6n.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "map_table.h"
#include "span_pool.h"

namespace ydorb {
namespace mapdb {

struct PointRec {   // one fully dirty point
  int32_t slot, off, len, refKf;
  float pos[3];
  uint8_t bad, refLevel, pad[2];
};
struct Vec3Rec {    // a position or a camera centre
  int32_t slot;
  float v[3];
};
static_assert(sizeof(PointRec) == 32 && sizeof(Vec3Rec) == 16, "the kernels read these layouts");

// What one sync does, decided before anything is written: the driver sizes its buffers from it, the kernels get their counts from it.
struct Plan : PoolPlan {
  int32_t nPointRec = 0, nPosRec = 0, nCentreRec = 0;
  size_t oPoint = 0, oPos = 0, oCentre = 0, oPayKf = 0, oPayLevel = 0, oNewOff = 0, bytes = 0;
  int32_t nPointsBefore = 0, nKeyframesBefore = 0;   // what the device tables hold: the repack covers the point slots below nPointsBefore
  int32_t pointCapBefore = 0, pointCap = 0, kfCapBefore = 0, kfCap = 0;
};

// The arrays the kernels read, on the host: the state-machine check executes deltas on them, the driver flattens its read-back with
// the same flatten().
struct HostTables {
  std::vector<int32_t> start, end, refKf, poolKf;
  std::vector<uint8_t> bad, refLevel, poolLevel;
  std::vector<float> pos, centre;
  void sizePoints(size_t cap) {   // a slot never set reads as bad with no observations
    start.resize(cap, 0); end.resize(cap, 0); refKf.resize(cap, 0); bad.resize(cap, 1); refLevel.resize(cap, 0); pos.resize(3 * cap, 0.f);
  }
  void resetPoints() { const size_t cap = start.size(); start.clear(); end.clear(); refKf.clear(); bad.clear(); refLevel.clear(); pos.clear(); sizePoints(cap); }
};

// One flat table from per-slot spans: obsStart [nPoints + 1], obsKf / obsLevel [sum of the spans]
inline void flatten(int32_t nPoints, const int32_t* start, const int32_t* end, const int32_t* poolKf, const uint8_t* poolLevel,
                    int32_t* obsStart, int32_t* obsKf, uint8_t* obsLevel) {
  int32_t at = 0;
  obsStart[0] = 0;
  for (int32_t p = 0; p < nPoints; p++) {
    const int32_t len = end[p] - start[p];
    if (len > 0) {
      memcpy(obsKf + at, poolKf + start[p], 4 * (size_t)len);
      memcpy(obsLevel + at, poolLevel + start[p], (size_t)len);
    }
    at += len;
    obsStart[p + 1] = at;
  }
}

class Host {
 public:
  Host(int32_t pointCap, int32_t kfCap, int64_t poolCap) : pointCap_(std::max(pointCap, 1)), kfCap_(std::max(kfCap, 1)), pool_(poolCap) {}

  int32_t nPoints() const { return (int32_t)len_.size(); }
  int32_t nKeyframes() const { return (int32_t)(centre_.size() / 3); }
  int32_t pointCap() const { return pointCap_; }
  int32_t kfCap() const { return kfCap_; }
  int64_t poolCap() const { return pool_.cap; }
  int64_t poolUsed() const { return pool_.used; }
  int64_t liveAfterSync() const { return pool_.pending; }
  bool dirty() const { return !dirtyPoints_.empty() || !dirtyKf_.empty() || nKeyframes() != nKfSynced_; }
  bool isBad(int32_t slot) const { return bad_[slot] != 0; }   // staged changes included
  // keyframe rows (mapdb_rows_host.h) named slots up to n - 1: the new slots' centres are zero, as the device's are, and no record travels
  void growKeyframes(int32_t n) {
    if (n > nKeyframes()) { centre_.resize(3 * (size_t)n, 0.f); kfDirty_.resize((size_t)n, 0); }
  }
  int32_t spanOf(int32_t slot) const { return state_[slot] == kFull ? stLen_[slot] : len_[slot]; }   // staged changes included

  void clear() {
    len_.clear(); off_.clear(); refKf_.clear(); bad_.clear(); refLevel_.clear(); pos_.clear(); centre_.clear();
    state_.clear(); stOff_.clear(); stLen_.clear(); kfDirty_.clear();
    dropStaged();
    pool_.clear();
    nPointsSynced_ = nKfSynced_ = 0;
    lastSyncBytes_ = lastSyncRecords_ = 0;
  }

  bool setCentres(const int32_t* slots, int32_t n, const float* centre, std::string& err) {
    if (n < 0) return fail(err, "negative number of keyframe slots: %lld", n);
    if (n > 0 && (!slots || !centre)) return fail(err, "null kf_slots or centre");
    for (int32_t i = 0; i < n; i++)
      if (slots[i] < 0) return fail(err, "kf_slots[%lld]: negative keyframe slot %lld", i, slots[i]);
    for (int32_t i = 0; i < n; i++) {
      const int32_t s = slots[i];
      if (s >= nKeyframes()) { centre_.resize(3 * ((size_t)s + 1), 0.f); kfDirty_.resize((size_t)s + 1, 0); }
      memcpy(&centre_[3 * (size_t)s], centre + 3 * (size_t)i, 12);
      if (!kfDirty_[s]) { kfDirty_[s] = 1; dirtyKf_.push_back(s); }
    }
    return true;
  }

  bool setPoints(const int32_t* slots, int32_t n, const int32_t* obsStart, const int32_t* obsKf, const uint8_t* obsLevel, const uint8_t* bad,
                 const int32_t* refKf, const uint8_t* refLevel, const float* pos, std::string& err) {
    if (n < 0) return fail(err, "negative number of point slots: %lld", n);
    if (!maptable::checkStarts("obs_start", obsStart, n, err)) return false;
    if (n == 0) return true;
    if (!slots || !bad || !refKf || !refLevel || !pos) return fail(err, "null slots, bad, ref_kf, ref_level or pos");
    const int32_t N = obsStart[n];
    if (N > 0 && (!obsKf || !obsLevel)) return fail(err, "null obs_kf or obs_level");
    for (int32_t i = 0; i < n; i++)
      if (slots[i] < 0) return fail(err, "slots[%lld]: negative point slot %lld", i, slots[i]);
    for (int32_t q = 0; q < N; q++)
      if (obsKf[q] < 0 || obsKf[q] >= nKeyframes())
        return fail(err, "observation %lld: keyframe slot %lld outside 0..%lld", q, obsKf[q], (long long)nKeyframes() - 1);
    for (int32_t i = 0; i < n; i++)
      if (refKf[i] < 0 || refKf[i] >= nKeyframes())
        return fail(err, "point %lld: reference keyframe slot %lld outside 0..%lld", i, refKf[i], (long long)nKeyframes() - 1);
    if (!pool_.admits(slots, n, obsStart, [this](int32_t s) { return s < nPoints() ? spanOf(s) : 0; }, checkPoolTotal, err)) return false;
    for (int32_t i = 0; i < n; i++) {
      const int32_t s = slots[i], len = obsStart[i + 1] - obsStart[i];
      growPointsTo(s);
      pool_.restaged(spanOf(s), len);
      if (state_[s] == kClean) dirtyPoints_.push_back(s);
      state_[s] = kFull;
      stOff_[s] = stKf_.size(); stLen_[s] = len;
      stKf_.insert(stKf_.end(), obsKf + obsStart[i], obsKf + obsStart[i] + len);
      stLevel_.insert(stLevel_.end(), obsLevel + obsStart[i], obsLevel + obsStart[i] + len);
      bad_[s] = bad[i] ? 1 : 0; refKf_[s] = refKf[i]; refLevel_[s] = refLevel[i];
      memcpy(&pos_[3 * (size_t)s], pos + 3 * (size_t)i, 12);
    }
    return true;
  }

  bool setPositions(const int32_t* slots, int32_t n, const float* pos, std::string& err) {
    if (n < 0) return fail(err, "negative number of point slots: %lld", n);
    if (n > 0 && (!slots || !pos)) return fail(err, "null slots or pos");
    for (int32_t i = 0; i < n; i++)
      if (slots[i] < 0 || slots[i] >= nPoints()) return fail(err, "slots[%lld]: point slot %lld outside 0..%lld", i, slots[i], (long long)nPoints() - 1);
    for (int32_t i = 0; i < n; i++) {
      const int32_t s = slots[i];
      memcpy(&pos_[3 * (size_t)s], pos + 3 * (size_t)i, 12);
      if (state_[s] == kClean) { state_[s] = kPos; dirtyPoints_.push_back(s); }
    }
    return true;
  }

  // the named slots of a query
  bool checkSlots(const int32_t* slots, int32_t n, std::string& err) const {
    if (n < 0) return fail(err, "negative number of point slots: %lld", n);
    if (n > 0 && !slots) return fail(err, "null slots");
    for (int32_t i = 0; i < n; i++)
      if (slots[i] < 0 || slots[i] >= nPoints()) return fail(err, "slots[%lld]: point slot %lld outside 0..%lld", i, slots[i], (long long)nPoints() - 1);
    return true;
  }
  bool checkNormalDepth(const int32_t* slots, int32_t n, const float* scaleFactors, int32_t nLevels, const float* normal, const float* minD,
                        const float* maxD, const uint8_t* status, std::string& err) const {
    if (nLevels < 1 || nLevels > maptable::kMaxLevels) return fail(err, "n_levels %lld outside 1..8", nLevels);
    if (!scaleFactors) return fail(err, "null scale_factors");
    if (!checkSlots(slots, n, err)) return false;
    if (n > 0 && (!normal || !minD || !maxD || !status)) return fail(err, "null output arrays");
    for (int32_t i = 0; i < n; i++) {
      const int32_t s = slots[i];
      if (bad_[s] || spanOf(s) == 0) continue;   // not updated: the level is not read
      if (refLevel_[s] >= nLevels) return fail(err, "slots[%lld]: reference level %lld of point slot %lld >= n_levels", i, refLevel_[s], s);
    }
    return true;
  }
  // a table header for map_table.h's list checks: they read the two counts only
  YdObservationTable counts() const { return YdObservationTable{nPoints(), nKeyframes(), nullptr, nullptr, nullptr, nullptr}; }

  // ------------------------------------------------------------------------------------------------------------- map correction
  // ydorb_mapdb_correct.  planCorrection validates the call, builds the keyframe slot -> rank table and runs
  // the claim pass over the entries in order: the mnCorrectedByKF rule, a stamp per slot.  It reads the mirror with the staged changes
  // in it, which is what the device holds once the query's sync has run.  It writes only its plan and the stamps (scratch): a refused
  // call changes neither mirror nor staging.  No two claimed entries share a slot, so the kernel never has two lanes writing one
  // address.  Every status is final here but DONE against DONE_NO_OBSERVATIONS, which the kernel reports.
  struct CorrectionPlan {
    std::vector<int32_t> rankOf;               // [n_keyframes] rank in kf_slots, -1: not in the call
    std::vector<uint8_t> status;               // [n]
    std::vector<int32_t> entry, slot, rank;    // the claimed entries, in order
    bool normals = false;
  };
  bool planCorrection(const YdMapCorrection* c, CorrectionPlan& P, std::string& err) {
    if (!c) return fail(err, "null correction");
    if (c->arithmetic != YDORB_MAPCORR_SIM3 && c->arithmetic != YDORB_MAPCORR_SE3) return fail(err, "unknown arithmetic %lld", c->arithmetic);
    if (c->centres != YDORB_MAPCORR_RESIDENT && c->centres != YDORB_MAPCORR_INTERLEAVED && c->centres != YDORB_MAPCORR_POSES_FIRST)
      return fail(err, "unknown centres rule %lld", c->centres);
    if (c->n_kf < 0) return fail(err, "negative number of keyframe slots: %lld", c->n_kf);
    if (c->n < 0) return fail(err, "negative number of entries: %lld", c->n);
    if (c->centres != YDORB_MAPCORR_RESIDENT && !c->centre_after) return fail(err, "a centres rule without centre_after");
    if (c->n_kf > 0 && !c->kf_slots) return fail(err, "null kf_slots");
    if (c->n_kf > 0 && c->n > 0 && (!c->before || !c->after)) return fail(err, "null before or after");
    if (c->n > 0 && (!c->pos_out || !c->status)) return fail(err, "null pos_out or status");
    const int nrm = (c->normal ? 1 : 0) + (c->min_distance ? 1 : 0) + (c->max_distance ? 1 : 0);
    if (nrm != 0 && nrm != 3) return fail(err, "normal, min_distance and max_distance: all three or none");
    P.normals = nrm == 3 && c->n > 0;
    if (P.normals) {
      if (c->n_levels < 1 || c->n_levels > maptable::kMaxLevels) return fail(err, "n_levels %lld outside 1..8", c->n_levels);
      if (!c->scale_factors) return fail(err, "null scale_factors");
    }
    if (!c->slots && c->n != nPoints() && c->n > 0) return fail(err, "null slots with n = %lld, not n_points = %lld", c->n, nPoints());
    P.rankOf.assign((size_t)nKeyframes(), -1);
    for (int32_t k = 0; k < c->n_kf; k++) {
      const int32_t s = c->kf_slots[k];
      if (s < 0 || s >= nKeyframes()) return fail(err, "kf_slots[%lld]: keyframe slot %lld outside 0..%lld", k, s, (long long)nKeyframes() - 1);
      if (P.rankOf[s] >= 0) return fail(err, "kf_slots[%lld]: keyframe slot %lld repeats kf_slots[%lld]", k, s, P.rankOf[s]);
      P.rankOf[s] = k;
    }
    if (c->arithmetic == YDORB_MAPCORR_SIM3 && c->n > 0)
      for (int32_t k = 0; k < c->n_kf; k++) {
        const double sb = static_cast<const double*>(c->before)[8 * (size_t)k + 7], sa = static_cast<const double*>(c->after)[8 * (size_t)k + 7];
        // !(s > 0) also catches NaN; s - s != 0 catches infinity
        if (!(sb > 0.0) || sb - sb != 0.0) return fail(err, "before[%lld]: the Sim3 scale is not positive and finite", k);
        if (!(sa > 0.0) || sa - sa != 0.0) return fail(err, "after[%lld]: the Sim3 scale is not positive and finite", k);
      }
    for (int32_t i = 0; i < c->n; i++) {
      if (c->slots && (c->slots[i] < 0 || c->slots[i] >= nPoints()))
        return fail(err, "slots[%lld]: point slot %lld outside 0..%lld", i, c->slots[i], (long long)nPoints() - 1);
      if (c->corrector && (c->corrector[i] < -1 || c->corrector[i] >= c->n_kf))
        return fail(err, "corrector[%lld]: %lld outside -1..%lld", i, c->corrector[i], (long long)c->n_kf - 1);
    }
    // the claim pass
    P.status.assign((size_t)c->n, 0);
    P.entry.clear(); P.slot.clear(); P.rank.clear();
    if (stamp_.size() < (size_t)nPoints()) stamp_.resize((size_t)nPoints(), 0);
    if (++stampNow_ == 0) { std::fill(stamp_.begin(), stamp_.end(), 0u); stampNow_ = 1; }
    for (int32_t i = 0; i < c->n; i++) {
      const int32_t s = c->slots ? c->slots[i] : i;
      if (bad_[s]) { P.status[i] = YDORB_MAPCORR_BAD; continue; }
      if (stamp_[s] == stampNow_) { P.status[i] = YDORB_MAPCORR_CLAIMED; continue; }
      stamp_[s] = stampNow_;
      const int32_t r = c->corrector && c->corrector[i] >= 0 ? c->corrector[i] : P.rankOf[refKf_[s]];
      if (r < 0) { P.status[i] = YDORB_MAPCORR_NOT_COVERED; continue; }
      P.status[i] = spanOf(s) == 0 ? YDORB_MAPCORR_DONE_NO_OBSERVATIONS : YDORB_MAPCORR_DONE;   // the kernel's word replaces it
      if (P.normals && spanOf(s) > 0 && refLevel_[s] >= c->n_levels)
        return fail(err, "slots[%lld]: reference level %lld of point slot %lld >= n_levels", i, refLevel_[s], s);
      P.entry.push_back(i); P.slot.push_back(s); P.rank.push_back(r);
    }
    return true;
  }
  // After the read-back: the mirror takes the corrected positions (pos [claimed][3]) and the new centres, with no staged record left
  // behind - the device holds the same floats already.
  void correctionApplied(const YdMapCorrection* c, const CorrectionPlan& P, const float* pos) {
    for (size_t j = 0; j < P.slot.size(); j++) memcpy(&pos_[3 * (size_t)P.slot[j]], pos + 3 * j, 12);
    if (c->centre_after)
      for (int32_t k = 0; k < c->n_kf; k++) memcpy(&centre_[3 * (size_t)c->kf_slots[k]], c->centre_after + 3 * (size_t)k, 12);
  }
  const std::vector<float>& mirrorPos() const { return pos_; }
  const std::vector<float>& mirrorCentres() const { return centre_; }

  void stats(YdMapDbStats& s) const {
    s.n_points = nPoints(); s.n_keyframes = nKeyframes();
    s.n_observations = pool_.pending; s.pool_used = pool_.used; s.pool_capacity = pool_.cap;
    s.repacks_kept = pool_.repacksKept; s.repacks_grown = pool_.repacksGrown;
    s.point_table_growths = pointGrowths_; s.keyframe_table_growths = kfGrowths_;
    s.point_capacity = pointCap_; s.keyframe_capacity = kfCap_;
    s.last_sync_bytes = lastSyncBytes_; s.last_sync_records = lastSyncRecords_;
  }
  void nothingToSync() { lastSyncBytes_ = lastSyncRecords_ = 0; }

  Plan plan() const {
    Plan P;
    int64_t replaced = 0, incoming = 0;
    for (const int32_t s : dirtyPoints_) {
      if (state_[s] == kFull) { P.nPointRec++; incoming += stLen_[s]; replaced += len_[s]; }
      else P.nPosRec++;
    }
    static_cast<PoolPlan&>(P) = pool_.plan(replaced, incoming);
    P.nCentreRec = (int32_t)dirtyKf_.size(); P.nPointsBefore = nPointsSynced_; P.nKeyframesBefore = nKfSynced_;
    P.pointCapBefore = pointCap_; P.pointCap = grownCap(nPoints(), pointCap_); P.kfCapBefore = kfCap_; P.kfCap = grownCap(nKeyframes(), kfCap_);
    Layout L;
    P.oPoint = L.add(sizeof(PointRec) * (size_t)P.nPointRec); P.oPos = L.add(sizeof(Vec3Rec) * (size_t)P.nPosRec);
    P.oCentre = L.add(sizeof(Vec3Rec) * (size_t)P.nCentreRec);
    P.oPayKf = L.add(4 * (size_t)P.nPayload); P.oPayLevel = L.add((size_t)P.nPayload);
    P.oNewOff = L.add(P.repack ? 4 * (size_t)P.nPointsBefore : 0); P.bytes = L.bytes;
    return P;
  }

  // Writes the delta of `P` (made by plan() with nothing staged since) into dst [P.bytes] and takes it as applied: the mirror's offsets
  // move, the dirty marks go, the counters advance.
  void pack(const Plan& P, uint8_t* dst) {
    memset(dst, 0, P.bytes);
    if (P.repack)
      survivorOffsets(P.nPointsBefore, len_.data(), off_.data(), reinterpret_cast<int32_t*>(dst + P.oNewOff), [this](int32_t s) { return state_[s] == kFull; });
    PointRec* pr = reinterpret_cast<PointRec*>(dst + P.oPoint);
    Vec3Rec* qr = reinterpret_cast<Vec3Rec*>(dst + P.oPos);
    int32_t* payKf = reinterpret_cast<int32_t*>(dst + P.oPayKf);
    uint8_t* payLevel = dst + P.oPayLevel;
    int64_t cursor = 0;
    for (const int32_t s : dirtyPoints_) {
      if (state_[s] == kFull) {
        const int32_t len = stLen_[s];
        off_[s] = (int32_t)(P.tail + cursor); len_[s] = len;
        PointRec r;
        memset(&r, 0, sizeof(r));
        r.slot = s; r.off = off_[s]; r.len = len; r.refKf = refKf_[s];
        memcpy(r.pos, &pos_[3 * (size_t)s], 12);
        r.bad = bad_[s]; r.refLevel = refLevel_[s];
        *pr++ = r;
        if (len) { memcpy(payKf + cursor, &stKf_[stOff_[s]], 4 * (size_t)len); memcpy(payLevel + cursor, &stLevel_[stOff_[s]], (size_t)len); }
        cursor += len;
      } else {
        Vec3Rec r;
        r.slot = s;
        memcpy(r.v, &pos_[3 * (size_t)s], 12);
        *qr++ = r;
      }
      state_[s] = kClean;
    }
    Vec3Rec* cr = reinterpret_cast<Vec3Rec*>(dst + P.oCentre);
    for (const int32_t k : dirtyKf_) {
      Vec3Rec r;
      r.slot = k;
      memcpy(r.v, &centre_[3 * (size_t)k], 12);
      *cr++ = r;
      kfDirty_[k] = 0;
    }
    dropStaged();
    pool_.commit(P);
    if (P.pointCap != pointCap_) { pointCap_ = P.pointCap; pointGrowths_++; }
    if (P.kfCap != kfCap_) { kfCap_ = P.kfCap; kfGrowths_++; }
    nPointsSynced_ = nPoints(); nKfSynced_ = nKeyframes();
    lastSyncBytes_ = (int64_t)P.bytes; lastSyncRecords_ = (int64_t)P.nPointRec + P.nPosRec + P.nCentreRec;
  }

 private:
  enum : uint8_t { kClean = 0, kPos = 1, kFull = 2 };
  void growPointsTo(int32_t s) {
    if (s < nPoints()) return;
    const size_t n = (size_t)s + 1;
    len_.resize(n, 0); off_.resize(n, 0); refKf_.resize(n, 0); bad_.resize(n, 1); refLevel_.resize(n, 0); pos_.resize(3 * n, 0.f);
    state_.resize(n, kClean); stOff_.resize(n, 0); stLen_.resize(n, 0);
  }
  void dropStaged() { dirtyPoints_.clear(); dirtyKf_.clear(); stKf_.clear(); stLevel_.clear(); }

  // the mirror: what the device holds once the staged changes are applied (off_ / len_: what it holds now)
  std::vector<int32_t> len_, off_, refKf_;
  std::vector<uint8_t> bad_, refLevel_;
  std::vector<float> pos_, centre_;
  // staged
  std::vector<uint8_t> state_, kfDirty_;
  std::vector<size_t> stOff_;
  std::vector<int32_t> stLen_, dirtyPoints_, dirtyKf_, stKf_;
  std::vector<uint8_t> stLevel_;
  // device capacities and pool use as of the last sync
  int32_t pointCap_, kfCap_, nPointsSynced_ = 0, nKfSynced_ = 0, pointGrowths_ = 0, kfGrowths_ = 0;
  SpanPool pool_;
  int64_t lastSyncBytes_ = 0, lastSyncRecords_ = 0;
  // the claim pass of planCorrection: a slot is claimed in this call when its stamp is the call's
  std::vector<uint32_t> stamp_;
  uint32_t stampNow_ = 0;
};

// ---------------------------------------------------------------------------------------------------------------------------------
// The packed delta executed on host arrays, step for step what the driver does on the device: grow the tables (contents kept, new
// slots bad and empty), repack (k_mapdb_repack), apply (k_mapdb_apply).
inline void repack(const Plan& P, const uint8_t* delta, HostTables& T) {
  const int32_t* newOff = reinterpret_cast<const int32_t*>(delta + P.oNewOff);
  std::vector<int32_t> kf((size_t)P.poolCap);
  std::vector<uint8_t> level((size_t)P.poolCap);
  for (int32_t p = 0; p < P.nPointsBefore; p++) {
    if (newOff[p] < 0) continue;
    const int32_t b = T.start[p], e = T.end[p];
    for (int32_t q = b; q < e; q++) { kf.at((size_t)(newOff[p] + q - b)) = T.poolKf.at((size_t)q); level.at((size_t)(newOff[p] + q - b)) = T.poolLevel.at((size_t)q); }
    T.start[p] = newOff[p]; T.end[p] = newOff[p] + (e - b);
  }
  T.poolKf.swap(kf); T.poolLevel.swap(level);
}

inline void apply(const Plan& P, const uint8_t* delta, HostTables& T) {
  const PointRec* pr = reinterpret_cast<const PointRec*>(delta + P.oPoint);
  for (int32_t i = 0; i < P.nPointRec; i++) {
    const PointRec& r = pr[i];
    T.start.at((size_t)r.slot) = r.off; T.end.at((size_t)r.slot) = r.off + r.len; T.refKf.at((size_t)r.slot) = r.refKf;
    T.bad.at((size_t)r.slot) = r.bad; T.refLevel.at((size_t)r.slot) = r.refLevel;
    memcpy(&T.pos.at(3 * (size_t)r.slot), r.pos, 12);
  }
  const Vec3Rec* qr = reinterpret_cast<const Vec3Rec*>(delta + P.oPos);
  for (int32_t i = 0; i < P.nPosRec; i++) memcpy(&T.pos.at(3 * (size_t)qr[i].slot), qr[i].v, 12);
  const Vec3Rec* cr = reinterpret_cast<const Vec3Rec*>(delta + P.oCentre);
  for (int32_t i = 0; i < P.nCentreRec; i++) memcpy(&T.centre.at(3 * (size_t)cr[i].slot), cr[i].v, 12);
  const int32_t* payKf = reinterpret_cast<const int32_t*>(delta + P.oPayKf);
  const uint8_t* payLevel = delta + P.oPayLevel;
  for (int64_t i = 0; i < P.nPayload; i++) { T.poolKf.at((size_t)(P.tail + i)) = payKf[i]; T.poolLevel.at((size_t)(P.tail + i)) = payLevel[i]; }
}

inline void execute(const Plan& P, const uint8_t* delta, HostTables& T) {
  if (T.start.size() != (size_t)P.pointCap) T.sizePoints((size_t)P.pointCap);
  if (T.centre.size() != 3 * (size_t)P.kfCap) T.centre.resize(3 * (size_t)P.kfCap, 0.f);
  if (T.poolKf.size() != (size_t)P.poolCapBefore) { T.poolKf.resize((size_t)P.poolCapBefore); T.poolLevel.resize((size_t)P.poolCapBefore); }
  if (P.repack) repack(P, delta, T);
  apply(P, delta, T);
}

}  // namespace mapdb
}  // namespace ydorb
