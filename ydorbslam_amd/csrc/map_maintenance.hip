// Host driver of map maintenance + its C ABI (include/ydorb/c_api.h, "Map maintenance"): ydorb_map_update_normal_depth,
// ydorb_map_covisibility, ydorb_map_keyframe_redundancy, ydorb_map_release.  A call checks everything on the host (map_table.h) and
// hands the table to the query's body in map_queries.h, which copies it and the call's own arrays into one pinned staging area,
// uploads it in one copy, runs one kernel and reads the results back in one copy.  The culling verdict is the reference's double
// compare, made there on the host.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>

#include "../../include/ydorb/c_api.h"
#include "host_buffers.h"
#include "map_queries.h"
#include "map_table.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::mapmaint;

namespace {

StagedCtx g_ctx[16];   // this solver's own: nothing is shared with the other staged solvers

int invalid(const std::string& what) { set_error("map maintenance: %s", what.c_str()); return YDORB_ERR_INVALID_ARG; }

}  // namespace

extern "C" int ydorb_map_update_normal_depth(const YdObservationTable* T, const float* pos, const float* centre, const int32_t* ref_kf,
                                             const uint8_t* ref_level, const float* scale_factors, int32_t n_levels, int32_t device,
                                             float* normal, float* min_distance, float* max_distance, uint8_t* status) {
  std::string err;
  if (!maptable::checkNormalDepth(T, pos, centre, ref_kf, ref_level, scale_factors, n_levels, device, normal, min_distance, max_distance,
                                  status, err))
    return invalid(err);
  int rc = require_device(device);
  if (rc) return rc;
  if (T->n_points == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  MapSource src;
  src.flat = T; src.pos = pos; src.centre = centre; src.refKf = ref_kf; src.refLevel = ref_level;
  return runNormalDepth(c, src, T->n_points, scale_factors, n_levels, normal, min_distance, max_distance, status);
}

extern "C" int ydorb_map_covisibility(const YdObservationTable* T, const int32_t* query_kf, int32_t n_queries, const int32_t* list_start,
                                      const int32_t* point_idx, const int32_t* out_start, int32_t device, int32_t* conn_kf,
                                      int32_t* conn_weight, int32_t* counts, uint8_t* status) {
  std::string err;
  if (!maptable::checkCovisibility(T, query_kf, n_queries, list_start, point_idx, out_start, device, conn_kf, conn_weight, counts, status, err))
    return invalid(err);
  int rc = require_device(device);
  if (rc) return rc;
  if (n_queries == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  MapSource src;
  src.flat = T;
  return runCovisibility(c, src, query_kf, n_queries, list_start, point_idx, out_start, conn_kf, conn_weight, counts, status);
}

extern "C" int ydorb_map_keyframe_redundancy(const YdObservationTable* T, const int32_t* cand_kf, int32_t n_candidates,
                                             const int32_t* list_start, const int32_t* point_idx, const uint8_t* own_level,
                                             const uint8_t* removed, int32_t th_obs, int32_t device, int32_t* n_counted,
                                             int32_t* n_redundant, uint8_t* cull) {
  std::string err;
  if (!maptable::checkRedundancy(T, cand_kf, n_candidates, list_start, point_idx, own_level, device, n_counted, n_redundant, cull, err))
    return invalid(err);
  int rc = require_device(device);
  if (rc) return rc;
  const size_t nc = (size_t)n_candidates;
  if (nc == 0) return YDORB_OK;
  std::memset(n_counted, 0, 4 * nc);
  std::memset(n_redundant, 0, 4 * nc);
  std::memset(cull, 0, nc);               // an empty list: 0 > 0.9 * 0 is false
  if (list_start[nc] == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  MapSource src;
  src.flat = T;
  return runRedundancy(c, src, cand_kf, n_candidates, list_start, point_idx, own_level, removed, th_obs, n_counted, n_redundant, cull);
}

extern "C" int ydorb_map_release(int32_t device) { return release_staged(g_ctx, device); }
