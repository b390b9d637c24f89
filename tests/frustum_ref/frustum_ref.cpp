// CPU restatement of Frame::isInCameraFrustum with MapPoint::predictScaleLevel (ORB-SLAM2 Frame::isInFrustum / MapPoint::PredictScale,
// which YDORBSLAM renames): test infrastructure, the checker of ydorb_frustum_cull and ydorb_search_local_points.  Written the
// reference's way - one map point after the other, small matrices in loops, the predicted level by the FORMULA with std::log, not by the
// threshold table the device uses - under the arithmetic contract of DESIGN.md section 2 ("isInCameraFrustum"): float inputs, the
// products of the small float gemm / Mat::dot / cv::norm exact in double and summed in ascending index.  Built with oracle/Makefile's
// flags (-ffp-contract=off) by tests/frustum_support.py.  Also exports the adapter's table builder (include/ydorb/tracking.hpp).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/ydorb/tracking.hpp"

namespace {

// MapPoint::predictScaleLevel(dist, frame): ratio = m_flt_maxDistance / dist; ceil(log(ratio) / m_flt_logScaleFactor), clamped.  Where the
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

int isInCameraFrustum(const YdFrustumView& V, float logScaleFactor, const float* posMin, const float* normalMax, float maxDistance, bool skip,
                      YdTrackView& T) {
  std::memset(&T, 0, sizeof T);
  if (skip) return YDORB_FRUSTUM_SKIPPED;
  const float* P = posMin;
  float Pc[3];
  for (int r = 0; r < 3; r++) {   // Rcw * P + tcw: gemm with its addend, GEMMSingleMul<float, double>
    double s = 0;
    for (int k = 0; k < 3; k++) s = k == 0 ? (double)V.Rcw[3 * r] * (double)P[0] : s + (double)V.Rcw[3 * r + k] * (double)P[k];
    Pc[r] = (float)(s + (double)V.tcw[r]);
  }
  const float PcX = Pc[0], PcY = Pc[1], PcZ = Pc[2];
  if (PcZ < 0.0f) return YDORB_FRUSTUM_BEHIND;
  const float invz = 1.0f / PcZ;
  const float u = V.fx * PcX * invz + V.cx;
  const float v = V.fy * PcY * invz + V.cy;
  if (u < V.min_x || u > V.max_x) return YDORB_FRUSTUM_OUT_U;
  if (v < V.min_y || v > V.max_y) return YDORB_FRUSTUM_OUT_V;
  const float maxDist = normalMax[3], minDist = posMin[3];   // the invariance getters' values
  float PO[3];
  for (int k = 0; k < 3; k++) PO[k] = P[k] - V.Ow[k];
  double s2 = 0;
  for (int k = 0; k < 3; k++) s2 = k == 0 ? (double)PO[0] * (double)PO[0] : s2 + (double)PO[k] * (double)PO[k];
  const float dist = (float)std::sqrt(s2);   // cv::norm returns double; the reference stores it in a float
  if (dist < minDist || dist > maxDist) return YDORB_FRUSTUM_DISTANCE;
  double dot = 0;
  for (int k = 0; k < 3; k++) dot = k == 0 ? (double)PO[0] * (double)normalMax[0] : dot + (double)PO[k] * (double)normalMax[k];
  const float viewCos = (float)(dot / (double)dist);
  if (viewCos < V.viewing_cos_limit) return YDORB_FRUSTUM_VIEW_ANGLE;
  T.level = predictScaleLevel(maxDistance, dist, logScaleFactor, V.n_levels);
  T.u = u; T.v = v; T.ur = u - V.bf * invz; T.view_cos = viewCos;
  return YDORB_FRUSTUM_IN_VIEW;
}

}  // namespace

extern "C" {

// The batch of ydorb_frustum_cull; log_scale_factor [n_views] = each frame's m_flt_logScaleFactor (the views' level_ratio is not read).
int frustumref_cull(const YdFrustumBatch* B, const float* log_scale_factor, YdTrackView* rows, uint8_t* status, int32_t* n_in_view) {
  for (int f = 0; f < B->n_views; f++) {
    int inView = 0;
    for (int e = B->list_start[f]; e < B->list_start[f + 1]; e++) {
      const int p = B->point_idx[e];
      status[e] = (uint8_t)isInCameraFrustum(B->views[f], log_scale_factor[f], B->table.pos_min + 4 * p, B->table.normal_max + 4 * p,
                                             B->table.max_distance[p], B->skip[e] != 0, rows[e]);
      inView += status[e] == YDORB_FRUSTUM_IN_VIEW;
    }
    if (n_in_view) n_in_view[f] = inView;
  }
  return 0;
}

int frustumref_predict_level(float ratio, float log_scale_factor, int n_levels) { return predictScaleLevel(ratio, 1.0f, log_scale_factor, n_levels); }

// n ratios at once (the table-against-formula sweep)
void frustumref_predict_levels(const float* ratio, int n, float log_scale_factor, int n_levels, int32_t* out) {
  for (int i = 0; i < n; i++) out[i] = predictScaleLevel(ratio[i], 1.0f, log_scale_factor, n_levels);
}

// the adapter's own table builder and the float log of this machine's C library (m_flt_logScaleFactor = log(m_flt_scaleFactor))
void frustumref_level_ratio_table(float log_scale_factor, int n_levels, float* out) { ydorb::adapter::levelRatioTable(log_scale_factor, n_levels, out); }
float frustumref_logf(float x) { return std::log(x); }

}
