// CPU restatement of the two local-map queries of the resident table (include/ydorb/c_api.h, "Keyframe rows"), written the way
// ORB-SLAM2 writes Tracking::UpdateLocalPoints and the counting loop of Tracking::UpdateLocalKeyFrames: sequential loops over the
// keyframes' map-point vectors with a per-point mark, and a std::map of counters.  It shares nothing with the product: it reads the
// exported flat tables.  Built as a shared object by tests/localmap_support.py and included by tests/cpu_harness/mapdb_rows_check.cpp.
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

extern "C" {

// rows: row_start [n_keyframes + 1] / row_slot, -1 = a null entry; bad [n_points].  Returns the number of local points;
// out_slots / out_seen need room for min(entries walked, n_points).
int localmapref_points_of_keyframes(int32_t n_points, const uint8_t* bad, const int32_t* row_start, const int32_t* row_slot,
                                    const int32_t* kf_slots, int32_t n_kf, const int32_t* seen_points, int32_t n_seen, int32_t* out_slots,
                                    uint8_t* out_seen) {
  std::vector<char> trackReferenceForFrame((size_t)n_points, 0), lastFrameSeen((size_t)n_points, 0);
  for (int32_t i = 0; i < n_seen; i++)                       // SearchLocalPoints: pMP->mnLastFrameSeen = mCurrentFrame.mnId
    if (seen_points[i] >= 0) lastFrameSeen[(size_t)seen_points[i]] = 1;
  int32_t n = 0;                                             // mvpLocalMapPoints.clear();
  for (int32_t r = 0; r < n_kf; r++) {                       // for(KeyFrame* pKF : mvpLocalKeyFrames)
    const int32_t k = kf_slots[r];
    for (int32_t q = row_start[k]; q < row_start[k + 1]; q++) {   // for(MapPoint* pMP : pKF->GetMapPointMatches())
      const int32_t p = row_slot[q];
      if (p < 0) continue;                                   // if(!pMP) continue;
      if (trackReferenceForFrame[(size_t)p]) continue;       // if(pMP->mnTrackReferenceForFrame==mCurrentFrame.mnId) continue;
      if (!bad[p]) {                                         // if(!pMP->isBad())
        out_slots[n] = p;                                    //   mvpLocalMapPoints.push_back(pMP);
        out_seen[n] = (uint8_t)lastFrameSeen[(size_t)p];
        n++;
        trackReferenceForFrame[(size_t)p] = 1;               //   pMP->mnTrackReferenceForFrame=mCurrentFrame.mnId;
      }
    }
  }
  return n;
}

// One frame's list: point_slots [n], -1 = no map point.  Observations: obs_start [n_points + 1] / obs_kf.  Returns the number of
// keyframes with a non-zero count, ascending by slot in out_kf / out_weight (room for n_keyframes); point_bad [n] = the entries the
// reference nulls.
int localmapref_observer_counter(const int32_t* obs_start, const int32_t* obs_kf, const uint8_t* bad, const int32_t* point_slots, int32_t n,
                                 int32_t* out_kf, int32_t* out_weight, uint8_t* point_bad) {
  std::map<int32_t, int32_t> keyframeCounter;
  for (int32_t i = 0; i < n; i++) {
    point_bad[i] = 0;
    const int32_t p = point_slots[i];
    if (p < 0) continue;                                     // if(mCurrentFrame.mvpMapPoints[i])
    if (bad[p]) { point_bad[i] = 1; continue; }              // else mCurrentFrame.mvpMapPoints[i]=NULL;
    for (int32_t q = obs_start[p]; q < obs_start[p + 1]; q++) keyframeCounter[obs_kf[q]]++;
  }
  int32_t m = 0;
  for (const auto& kv : keyframeCounter) { out_kf[m] = kv.first; out_weight[m] = kv.second; m++; }
  return m;
}

}  // extern "C"
