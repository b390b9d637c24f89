// CPU restatement of pass 1 of OrbMatcher::fuseByProjection / fuseBySim3 over a map held by slot: test infrastructure, the checker of
// ydorb_mapdb_fuse_search's query kernel.  Written the adapter's way (include/ydorb/orbMatcher.hpp, fuseByProjection and
// SimProjection::query) - one target after the other, one map point after the other, small matrices in loops, the predicted level by the
// FORMULA with std::log, not by the threshold table the device uses - under the arithmetic contract of DESIGN.md section 2 ("Fuse search
// on the resident table"): float inputs, the products of the small float gemm / Mat::dot / cv::norm exact in double and summed in
// ascending index, every other operation one float operation in the order the adapter writes it.  Built with oracle/Makefile's flags
// (-ffp-contract=off) by tests/mapdb_fuse_support.py.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/ydorb/c_api.h"

namespace {

// MapPoint::predictScaleLevel(dist, keyframe): ratio = m_flt_maxDistance / dist; ceil(log(ratio) / m_flt_logScaleFactor), clamped.  Where the
// reference's conversion to int is undefined (NaN, infinite) the contract's table form rules: NaN -> 0, +inf -> nLevels - 1.
int predictScaleLevel(float maxDistance, float dist, float logScaleFactor, int nLevels) {
  const float ratio = maxDistance / dist;
  if (ratio != ratio) return 0;
  const float q = std::ceil(std::log(ratio) / logScaleFactor);
  if (q != q || q < 0) return 0;
  if (q >= (float)nLevels) return nLevels - 1;
  int nScale = (int)q;
  if (nScale < 0) nScale = 0;
  else if (nScale >= nLevels) nScale = nLevels - 1;
  return nScale;
}

}  // namespace

// The map by slot, as the resident table exports it
struct FuseRefMap {
  int32_t n_points;
  const float* pos;            // [n][3]
  const uint8_t* bad;          // [n]
  const int32_t* obs_start;    // [n + 1]
  const int32_t* obs_kf;       // [obs_start[n]]
  const float* normal;         // [n][3]
  const float *min_distance, *max_distance;   // [n] raw
  const uint8_t* desc;         // [n][32]
  const uint8_t* flags;        // [n] bit 0 geometry, bit 1 descriptor
};

// queries / qdesc / status [list_start[n_targets]]; log_scale_factor [n_targets]: each target keyframe's m_flt_logScaleFactor
extern "C" void fuseref_queries(const YdFuseTarget* targets, int32_t n_targets, const float* log_scale_factor, const int32_t* list_start,
                                const int32_t* point_slots, const uint8_t* skip, const FuseRefMap* M, YdQuery* queries, uint8_t* qdesc,
                                uint8_t* status) {
  for (int32_t t = 0; t < n_targets; t++) {
    const YdFuseTarget& G = targets[t];
    const YdFrustumView& V = G.view;
    for (int32_t e = list_start[t]; e < list_start[t + 1]; e++) {
      YdQuery& Q = queries[e];
      std::memset(&Q, 0, sizeof Q);
      std::memset(qdesc + 32 * (size_t)e, 0, 32);
      const int32_t p = point_slots[e];
      if (skip[e]) { status[e] = YDORB_FUSE_SKIPPED; continue; }                 // !mp, or the caller's found-set
      if (M->bad[p]) { status[e] = YDORB_FUSE_BAD; continue; }                   // mp->isBad()
      bool inKeyFrame = false;
      if (G.flags & YDORB_FUSE_SKIP_OBSERVED)
        for (int32_t o = M->obs_start[p]; o < M->obs_start[p + 1]; o++) inKeyFrame = inKeyFrame || M->obs_kf[o] == G.kf_slot;
      if (inKeyFrame) { status[e] = YDORB_FUSE_OBSERVED; continue; }             // mp->isInKeyFrame(kf)
      if ((M->flags[p] & 3) != 3) { status[e] = YDORB_FUSE_NO_ATTRIBUTES; continue; }
      const float* Pw = M->pos + 3 * (size_t)p;
      float Pc[3];
      for (int r = 0; r < 3; r++) {   // Rcw * Pw + tcw: gemm with its addend
        double s = 0;
        for (int k = 0; k < 3; k++) s = k == 0 ? (double)V.Rcw[3 * r] * (double)Pw[0] : s + (double)V.Rcw[3 * r + k] * (double)Pw[k];
        Pc[r] = (float)(s + (double)V.tcw[r]);
      }
      const float xc = Pc[0], yc = Pc[1], zc = Pc[2];
      const float u = V.fx * xc / zc + V.cx, v = V.fy * yc / zc + V.cy;
      const float ur = u - V.bf / zc;
      float PO[3];
      for (int k = 0; k < 3; k++) PO[k] = Pw[k] - V.Ow[k];
      double s2 = 0;
      for (int k = 0; k < 3; k++) s2 = k == 0 ? (double)PO[0] * (double)PO[0] : s2 + (double)PO[k] * (double)PO[k];
      const float dist3D = (float)std::sqrt(s2);   // cv::norm returns double; the adapter stores it in a float
      const int level = predictScaleLevel(M->max_distance[p], dist3D, log_scale_factor[t], V.n_levels);
      const float* Pn = M->normal + 3 * (size_t)p;
      double dot = 0;
      for (int k = 0; k < 3; k++) dot = k == 0 ? (double)PO[0] * (double)Pn[0] : dot + (double)PO[k] * (double)Pn[k];
      const bool isInImage = u >= V.min_x && u < V.max_x && v >= V.min_y && v < V.max_y;
      const float minInv = 0.8f * M->min_distance[p], maxInv = 1.2f * M->max_distance[p];   // getMin / getMaxDistanceInvariance
      const bool ok = zc >= 0.0f && isInImage && dist3D >= minInv && dist3D <= maxInv && dot >= 0.5 * dist3D;
      if (!ok) { status[e] = YDORB_FUSE_REJECTED; continue; }
      Q.u = u; Q.v = v; Q.ur = ur; Q.level = level; Q.min_level = -1; Q.max_level = -1;
      Q.r = G.th * V.scale_factors[level];
      Q.flags = 1;
      std::memcpy(qdesc + 32 * (size_t)e, M->desc + 32 * (size_t)p, 32);
      status[e] = YDORB_FUSE_SEARCHED;
    }
  }
}

extern "C" float fuseref_logf(float x) { return std::log(x); }
