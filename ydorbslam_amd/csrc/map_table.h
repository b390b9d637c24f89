// Host checks of the map-maintenance entries (include/ydorb/c_api.h, "Map maintenance"): the validation of the
// flattened observation table and of the lists laid over it, and the capacity a caller may give a covisibility query.  Every check
// returns false with the first offender named in `err`, before the driver touches a device.  Offsets into the observation and list
// arrays are int32 in the ABI; sums of them are formed in 64 bits here and refused past INT32_MAX.  No HIP here: a plain host
// compiler builds it (tests/cpu_harness/map_table_check.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ydorb/c_api.h"

namespace ydorb {
namespace maptable {

constexpr int kCovisWindow = 8192;   // W: keyframe slots one LDS histogram covers (map_kernels.hip.h); the Python mirror's COVIS_WINDOW
constexpr int kMaxLevels = 8;

inline bool fail(std::string& err, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
  char text[256];
  snprintf(text, sizeof(text), fmt, a, b, c);
  err = text;
  return false;
}

// start[0] == 0 and start[i + 1] >= start[i] for i < n
inline bool checkStarts(const char* name, const int32_t* start, int64_t n, std::string& err) {
  char fmt[128];
  if (!start) { snprintf(fmt, sizeof(fmt), "null %s", name); return fail(err, fmt); }
  if (start[0] != 0) { snprintf(fmt, sizeof(fmt), "%s[0] is %%lld, not 0", name); return fail(err, fmt, start[0]); }
  for (int64_t i = 0; i < n; i++)
    if (start[i + 1] < start[i]) {
      snprintf(fmt, sizeof(fmt), "%s decreases at %%lld: %%lld after %%lld", name);
      return fail(err, fmt, i + 1, start[i + 1], start[i]);
    }
  return true;
}

inline bool checkDevice(int32_t device, std::string& err) {
  return device >= 0 && device < 16 ? true : fail(err, "device %lld outside 0..15", device);
}

// starts from lengths: start[0] = 0, start[i + 1] = start[i] + len[i]; refused when a length is negative or an offset passes INT32_MAX
inline bool accumulateStarts(const int64_t* len, int64_t n, int32_t* start, std::string& err) {
  int64_t at = 0;
  start[0] = 0;
  for (int64_t i = 0; i < n; i++) {
    if (len[i] < 0) return fail(err, "length %lld of entry %lld is negative", len[i], i);
    at += len[i];
    if (at > INT32_MAX) return fail(err, "offset %lld after entry %lld passes INT32_MAX", at, i);
    start[i + 1] = (int32_t)at;
  }
  return true;
}

inline bool checkTable(const YdObservationTable* T, std::string& err) {
  if (!T) return fail(err, "null table");
  if (T->n_points < 0 || T->n_keyframes < 0) return fail(err, "negative table size: %lld points, %lld keyframes", T->n_points, T->n_keyframes);
  if (!checkStarts("obs_start", T->obs_start, T->n_points, err)) return false;
  if (T->n_points > 0 && !T->bad) return fail(err, "null bad");
  const int32_t N = T->obs_start[T->n_points];
  if (N > 0 && (!T->obs_kf || !T->obs_level)) return fail(err, "null obs_kf or obs_level");
  for (int32_t q = 0; q < N; q++)
    if (T->obs_kf[q] < 0 || T->obs_kf[q] >= T->n_keyframes)
      return fail(err, "observation %lld: keyframe slot %lld outside 0..%lld", q, T->obs_kf[q], (long long)T->n_keyframes - 1);
  return true;
}

// n slots (queries or candidates), each with a list of point indices: `what` names the slot array in messages
inline bool checkLists(const YdObservationTable* T, const char* what, const int32_t* slot, int32_t n, const int32_t* listStart,
                       const int32_t* pointIdx, std::string& err) {
  char fmt[128];
  if (n < 0) { snprintf(fmt, sizeof(fmt), "negative number of %s entries: %%lld", what); return fail(err, fmt, n); }
  if (n > 0 && !slot) { snprintf(fmt, sizeof(fmt), "null %s", what); return fail(err, fmt); }
  if (!checkStarts("list_start", listStart, n, err)) return false;
  for (int32_t i = 0; i < n; i++)
    if (slot[i] < 0 || slot[i] >= T->n_keyframes) {
      snprintf(fmt, sizeof(fmt), "%s[%%lld]: keyframe slot %%lld outside 0..%%lld", what);
      return fail(err, fmt, i, slot[i], (long long)T->n_keyframes - 1);
    }
  const int32_t L = listStart[n];
  if (L > 0 && !pointIdx) return fail(err, "null point_idx");
  for (int32_t e = 0; e < L; e++)
    if (pointIdx[e] < 0 || pointIdx[e] >= T->n_points)
      return fail(err, "list entry %lld: point index %lld outside the table of %lld", e, pointIdx[e], T->n_points);
  return true;
}

inline bool checkNormalDepth(const YdObservationTable* T, const float* pos, const float* centre, const int32_t* refKf, const uint8_t* refLevel,
                             const float* scaleFactors, int32_t nLevels, int32_t device, const float* normal, const float* minD,
                             const float* maxD, const uint8_t* status, std::string& err) {
  if (!checkDevice(device, err) || !checkTable(T, err)) return false;
  if (nLevels < 1 || nLevels > kMaxLevels) return fail(err, "n_levels %lld outside 1..8", nLevels);
  if (!scaleFactors) return fail(err, "null scale_factors");
  if (T->n_points == 0) return true;
  if (!pos || !refKf || !refLevel) return fail(err, "null pos, ref_kf or ref_level");
  if (!normal || !minD || !maxD || !status) return fail(err, "null output arrays");
  if (T->n_keyframes > 0 && !centre) return fail(err, "null centre");
  for (int32_t p = 0; p < T->n_points; p++) {
    if (T->bad[p] || T->obs_start[p + 1] == T->obs_start[p]) continue;   // returns early: nothing of the reference keyframe is read
    if (refKf[p] < 0 || refKf[p] >= T->n_keyframes)
      return fail(err, "point %lld: reference keyframe slot %lld outside 0..%lld", p, refKf[p], (long long)T->n_keyframes - 1);
    if (refLevel[p] >= nLevels) return fail(err, "point %lld: reference level %lld >= n_levels %lld", p, refLevel[p], nLevels);
  }
  return true;
}

// What a covisibility call's own arrays must satisfy.  Of T only the header (n_points, n_keyframes) is read: the resident table
// passes its counts, the flat entry its table after checkTable.
inline bool checkCovisibilityArgs(const YdObservationTable* T, const int32_t* queryKf, int32_t nQueries, const int32_t* listStart,
                                  const int32_t* pointIdx, const int32_t* outStart, const int32_t* connKf, const int32_t* connWeight,
                                  const int32_t* counts, const uint8_t* status, std::string& err) {
  if (!checkLists(T, "query_kf", queryKf, nQueries, listStart, pointIdx, err)) return false;
  if (!checkStarts("out_start", outStart, nQueries, err)) return false;
  if (nQueries > 0 && (!counts || !status)) return fail(err, "null counts or status");
  if (outStart[nQueries] > 0 && (!connKf || !connWeight)) return fail(err, "null conn_kf or conn_weight");
  return true;
}

inline bool checkCovisibility(const YdObservationTable* T, const int32_t* queryKf, int32_t nQueries, const int32_t* listStart,
                              const int32_t* pointIdx, const int32_t* outStart, int32_t device, const int32_t* connKf,
                              const int32_t* connWeight, const int32_t* counts, const uint8_t* status, std::string& err) {
  return checkDevice(device, err) && checkTable(T, err) &&
         checkCovisibilityArgs(T, queryKf, nQueries, listStart, pointIdx, outStart, connKf, connWeight, counts, status, err);
}

// The same for a redundancy call: again only T's header is read.
inline bool checkRedundancyArgs(const YdObservationTable* T, const int32_t* candKf, int32_t nCand, const int32_t* listStart,
                                const int32_t* pointIdx, const uint8_t* ownLevel, const int32_t* nCounted, const int32_t* nRedundant,
                                const uint8_t* cull, std::string& err) {
  if (!checkLists(T, "cand_kf", candKf, nCand, listStart, pointIdx, err)) return false;
  if (listStart[nCand] > 0 && !ownLevel) return fail(err, "null own_level");
  if (nCand > 0 && (!nCounted || !nRedundant || !cull)) return fail(err, "null output arrays");
  return true;
}

inline bool checkRedundancy(const YdObservationTable* T, const int32_t* candKf, int32_t nCand, const int32_t* listStart, const int32_t* pointIdx,
                            const uint8_t* ownLevel, int32_t device, const int32_t* nCounted, const int32_t* nRedundant,
                            const uint8_t* cull, std::string& err) {
  return checkDevice(device, err) && checkTable(T, err) &&
         checkRedundancyArgs(T, candKf, nCand, listStart, pointIdx, ownLevel, nCounted, nRedundant, cull, err);
}

// What always fits one covisibility query: it can name no keyframe but the others, and no more than it walks observations.
inline int64_t capacityBound(int32_t nKeyframes, int64_t spanSum) {
  return std::max<int64_t>(0, std::min<int64_t>((int64_t)nKeyframes - 1, spanSum));
}

// out_start [nQueries + 1] with capacityBound per query; false when the total passes INT32_MAX.  The lists must have passed checkLists.
inline bool layoutCapacities(const YdObservationTable* T, int32_t nQueries, const int32_t* listStart, const int32_t* pointIdx,
                             int32_t* outStart, std::string& err) {
  std::vector<int64_t> bound((size_t)nQueries);
  for (int32_t q = 0; q < nQueries; q++) {
    int64_t sum = 0;
    for (int32_t e = listStart[q]; e < listStart[q + 1]; e++) sum += T->obs_start[pointIdx[e] + 1] - T->obs_start[pointIdx[e]];
    bound[q] = capacityBound(T->n_keyframes, sum);
  }
  return accumulateStarts(bound.data(), nQueries, outStart, err);
}

// the culling verdict, on the host side of the driver: the reference compares in double
inline uint8_t cullVerdict(int32_t nRedundant, int32_t nCounted) { return (double)nRedundant > 0.9 * (double)nCounted ? 1 : 0; }

}  // namespace maptable
}  // namespace ydorb
