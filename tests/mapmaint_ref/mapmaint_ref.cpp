// CPU restatement of the map-maintenance entries (include/ydorb/c_api.h, "Map maintenance"), written the way ORB-SLAM2 writes
// MapPoint::UpdateNormalAndDepth, the counting loop of KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling: a running cv::Mat
// style sum, a std::map of counters, the observer loop with its early break.  It shares nothing with the product but the ABI structs
// and the entries' signatures (so the Python wrappers can call either), and is built by tests/mapmaint_support.py with oracle/Makefile's
// flags (-ffp-contract=off).  The arithmetic is DESIGN.md section 2, "Map maintenance".  mapref_sequential_culling is the yardstick of
// the `removed` mask: it really erases a culled keyframe's observations before it judges the next candidate.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/ydorb/c_api.h"

namespace {

// cv::norm of a 3x1 CV_32F matrix: the squares accumulated in double, the root in double
double norm3(const float d[3]) {
  double s = 0.0;
  for (int i = 0; i < 3; i++) s += (double)d[i] * (double)d[i];
  return std::sqrt(s);
}

struct Obs { int kf, level; bool stereo; };

}  // namespace

extern "C" {

int mapref_update_normal_depth(const YdObservationTable* T, const float* pos, const float* centre, const int32_t* ref_kf,
                               const uint8_t* ref_level, const float* scale_factors, int32_t n_levels, int32_t, float* normal,
                               float* min_distance, float* max_distance, uint8_t* status) {
  for (int p = 0; p < T->n_points; p++) {
    normal[3 * p] = normal[3 * p + 1] = normal[3 * p + 2] = 0.f;
    min_distance[p] = max_distance[p] = 0.f;
    if (T->bad[p]) { status[p] = YDORB_MAP_BAD; continue; }                      // if(mbBad) return;
    const int b = T->obs_start[p], e = T->obs_start[p + 1];
    if (b == e) { status[p] = YDORB_MAP_NO_OBSERVATIONS; continue; }             // if(observations.empty()) return;
    const float* P = pos + 3 * p;
    float nrm[3] = {0.f, 0.f, 0.f};                                              // cv::Mat normal = cv::Mat::zeros(3,1,CV_32F);
    int n = 0;
    for (int q = b; q < e; q++) {
      const float* Owi = centre + 3 * T->obs_kf[q];
      float normali[3];
      for (int i = 0; i < 3; i++) normali[i] = P[i] - Owi[i];                    // normali = mWorldPos - Owi;
      const float inv = (float)(1.0 / norm3(normali));                           // normali / cv::norm(normali): scale by 1./s
      for (int i = 0; i < 3; i++) { const float t = normali[i] * inv; nrm[i] = nrm[i] + t; }
      n++;
    }
    float PC[3];
    const float* Owr = centre + 3 * ref_kf[p];
    for (int i = 0; i < 3; i++) PC[i] = P[i] - Owr[i];                           // PC = Pos - pRefKF->GetCameraCenter();
    const float dist = (float)norm3(PC);                                         // const float dist = cv::norm(PC);
    const float levelScaleFactor = scale_factors[ref_level[p]];
    max_distance[p] = dist * levelScaleFactor;                                   // mfMaxDistance = dist*levelScaleFactor;
    min_distance[p] = max_distance[p] / scale_factors[n_levels - 1];             // mfMinDistance = mfMaxDistance/mvScaleFactors[nLevels-1];
    const float invn = (float)(1.0 / (double)n);                                 // mNormalVector = normal/n;
    for (int i = 0; i < 3; i++) normal[3 * p + i] = nrm[i] * invn;
    status[p] = YDORB_MAP_UPDATED;
  }
  return 0;
}

int mapref_covisibility(const YdObservationTable* T, const int32_t* query_kf, int32_t n_queries, const int32_t* list_start,
                        const int32_t* point_idx, const int32_t* out_start, int32_t, int32_t* conn_kf, int32_t* conn_weight,
                        int32_t* counts, uint8_t* status) {
  for (int qi = 0; qi < n_queries; qi++) {
    std::map<int, int> KFcounter;                                                // map<KeyFrame*,int> KFcounter;
    for (int e = list_start[qi]; e < list_start[qi + 1]; e++) {
      const int p = point_idx[e];
      if (T->bad[p]) continue;                                                   // if(pMP->isBad()) continue;
      for (int q = T->obs_start[p]; q < T->obs_start[p + 1]; q++) {
        if (T->obs_kf[q] == query_kf[qi]) continue;                              // if(mit->first->mnId==mnId) continue;
        KFcounter[T->obs_kf[q]]++;
      }
    }
    counts[qi] = (int32_t)KFcounter.size();
    status[qi] = counts[qi] > out_start[qi + 1] - out_start[qi] ? 1 : 0;
    if (status[qi]) continue;
    int o = out_start[qi];
    for (const auto& kv : KFcounter) { conn_kf[o] = kv.first; conn_weight[o] = kv.second; o++; }
  }
  return 0;
}

// The masked form, stated over the table as the ABI words it: w(p) over the observers that are not removed.
int mapref_keyframe_redundancy(const YdObservationTable* T, const int32_t* cand_kf, int32_t n_candidates, const int32_t* list_start,
                               const int32_t* point_idx, const uint8_t* own_level, const uint8_t* removed, int32_t th_obs, int32_t,
                               int32_t* n_counted, int32_t* n_redundant, uint8_t* cull) {
  for (int c = 0; c < n_candidates; c++) {
    int nRedundantObservations = 0, nMPs = 0;
    for (int e = list_start[c]; e < list_start[c + 1]; e++) {
      const int p = point_idx[e];
      if (T->bad[p]) continue;                                                   // if(!pMP->isBad())
      int w = 0;
      bool lost = false;
      for (int q = T->obs_start[p]; q < T->obs_start[p + 1]; q++) {
        if (removed && removed[T->obs_kf[q]]) { lost = true; continue; }
        w += (T->obs_level[q] & 0x80) ? 2 : 1;
      }
      if (lost && w <= 2) continue;                                              // eraseObservation left it bad
      nMPs++;
      if (w > th_obs) {                                                          // if(pMP->Observations()>thObs)
        const int scaleLevel = own_level[e];
        int nObs = 0;
        for (int q = T->obs_start[p]; q < T->obs_start[p + 1]; q++) {
          const int kfi = T->obs_kf[q];
          if (removed && removed[kfi]) continue;
          if (kfi == cand_kf[c]) continue;                                       // if(pKFi==pKF) continue;
          const int scaleLeveli = T->obs_level[q] & 0x7f;
          if (scaleLeveli <= scaleLevel + 1) {
            nObs++;
            if (nObs >= th_obs) break;
          }
        }
        if (nObs >= th_obs) nRedundantObservations++;
      }
    }
    n_counted[c] = nMPs;
    n_redundant[c] = nRedundantObservations;
    cull[c] = (double)nRedundantObservations > 0.9 * (double)nMPs ? 1 : 0;       // if(nRedundantObservations>0.9*nMPs)
  }
  return 0;
}

// LocalMapping::KeyFrameCulling over the candidates in order, on containers that are really changed: a culled candidate (unless
// not_erase[k]: SetBadFlag then only marks it) has its observation erased from every map point, as KeyFrame::SetBadFlag does through
// MapPoint::EraseObservation, which lowers nObs by 2 for a stereo observation and by 1 otherwise and sets the point bad at nObs <= 2.
// verdict [K] = the culling test fired, erased [K] = the keyframe is now bad, n_counted / n_redundant [K] = the counts each candidate
// was judged by, bad_out [n_points] = isBad() of every point afterwards.
int mapref_sequential_culling(const YdObservationTable* T, const int32_t* cand_kf, int32_t n_candidates, const int32_t* list_start,
                              const int32_t* point_idx, const uint8_t* own_level, int32_t th_obs, const uint8_t* not_erase,
                              uint8_t* verdict, uint8_t* erased, int32_t* n_counted, int32_t* n_redundant, uint8_t* bad_out) {
  std::vector<std::vector<Obs>> observations((size_t)T->n_points);
  std::vector<int> nObsOf((size_t)T->n_points, 0);
  std::vector<uint8_t> bad(T->bad, T->bad + T->n_points);
  for (int p = 0; p < T->n_points; p++)
    for (int q = T->obs_start[p]; q < T->obs_start[p + 1]; q++) {
      const bool stereo = (T->obs_level[q] & 0x80) != 0;
      observations[p].push_back(Obs{T->obs_kf[q], T->obs_level[q] & 0x7f, stereo});
      nObsOf[p] += stereo ? 2 : 1;
    }
  for (int c = 0; c < n_candidates; c++) {
    const int pKF = cand_kf[c];
    int nRedundantObservations = 0, nMPs = 0;
    for (int e = list_start[c]; e < list_start[c + 1]; e++) {
      const int p = point_idx[e];
      if (bad[p]) continue;
      nMPs++;
      if (nObsOf[p] > th_obs) {
        const int scaleLevel = own_level[e];
        int nObs = 0;
        for (const Obs& o : observations[p]) {
          if (o.kf == pKF) continue;
          if (o.level <= scaleLevel + 1) {
            nObs++;
            if (nObs >= th_obs) break;
          }
        }
        if (nObs >= th_obs) nRedundantObservations++;
      }
    }
    n_counted[c] = nMPs;
    n_redundant[c] = nRedundantObservations;
    verdict[c] = (double)nRedundantObservations > 0.9 * (double)nMPs ? 1 : 0;
    erased[c] = 0;
    if (!verdict[c] || (not_erase && not_erase[c])) continue;
    erased[c] = 1;
    for (int p = 0; p < T->n_points; p++) {                                      // SetBadFlag: every map point loses this observation
      if (bad[p]) continue;
      std::vector<Obs>& obs = observations[p];
      for (size_t i = 0; i < obs.size(); i++)
        if (obs[i].kf == pKF) {
          nObsOf[p] -= obs[i].stereo ? 2 : 1;
          obs.erase(obs.begin() + (long)i);
          if (nObsOf[p] <= 2) bad[p] = 1;
          break;
        }
    }
  }
  std::memcpy(bad_out, bad.data(), (size_t)T->n_points);
  return 0;
}

}  // extern "C"
