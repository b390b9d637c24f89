// The counting loop of KeyFrame::updateConnections (ORB-SLAM2 KeyFrame::UpdateConnections) on top of the ydorb C
// ABI.  A function template over the reference's own KeyFrame / MapPoint types.  In the member function, the loop that fills
// `map<KeyFrame, int> KFcounter` from the keyframe's map points becomes
//   std::map<std::shared_ptr<KeyFrame>, int> KFcounter =
//       ydorb::adapter::covisibilityCounter<std::shared_ptr<KeyFrame>, std::shared_ptr<MapPoint>>(shared_from_this());
// and everything after it (the empty check, the threshold of 15, the keep-the-best rule, the sort, addConnection, the spanning-tree
// parent) stays the reference's.  One flatten, one ydorb_map_covisibility call.
// Assumed spellings: KeyFrame getMapPointMatches() -> std::vector<MapPointPtr> with null entries, and those of mapPoint.hpp.
#ifndef YDORB_ADAPTER_KEYFRAME_HPP
#define YDORB_ADAPTER_KEYFRAME_HPP

#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

#include "c_api.h"
#include "mapPoint.hpp"

namespace ydorb {
namespace adapter {

// The inputs of ydorb_map_covisibility for one keyframe: slot 0 is the keyframe itself
template <class KeyFramePtr, class MapPointPtr>
struct CovisibilityFlat {
  ObservationFlat<KeyFramePtr, MapPointPtr> obs;
  std::vector<int32_t> pointIdx;
  int32_t capacity = 0;
};

template <class KeyFramePtr, class MapPointPtr>
inline void flattenCovisibility(const KeyFramePtr& keyFrame, CovisibilityFlat<KeyFramePtr, MapPointPtr>& F) {
  F.obs.slot(keyFrame);
  int64_t spans = 0;
  for (const MapPointPtr& mp : keyFrame->getMapPointMatches()) {
    if (!mp) continue;                           // if(!pMP) continue;  (isBad() travels in the table)
    const int32_t p = F.obs.point(mp);
    F.pointIdx.push_back(p);                     // per entry of the vector: a point listed twice counts twice
    spans += F.obs.span(p);
  }
  F.capacity = (int32_t)std::max<int64_t>(0, std::min<int64_t>((int64_t)F.obs.keyFrames.size() - 1, spans));   // what always fits
}

template <class KeyFramePtr, class MapPointPtr>
inline std::map<KeyFramePtr, int> covisibilityCounter(const KeyFramePtr& keyFrame, int device = 0) {
  CovisibilityFlat<KeyFramePtr, MapPointPtr> F;
  flattenCovisibility(keyFrame, F);
  std::map<KeyFramePtr, int> counter;
  if (F.pointIdx.empty()) return counter;
  const YdObservationTable T = F.obs.table();
  const int32_t query = 0, listStart[2] = {0, (int32_t)F.pointIdx.size()}, outStart[2] = {0, F.capacity};
  std::vector<int32_t> kf((size_t)F.capacity + 1), weight((size_t)F.capacity + 1);
  int32_t count = 0;
  uint8_t status = 0;
  mapCheck(ydorb_map_covisibility(&T, &query, 1, listStart, F.pointIdx.data(), outStart, device, kf.data(), weight.data(), &count, &status));
  if (status != 0) throw std::runtime_error("ydorb: covisibility capacity bound violated");
  for (int32_t i = 0; i < count; i++) counter[F.obs.keyFrames[kf[i]]] = weight[i];
  return counter;
}

}  // namespace adapter
}  // namespace ydorb
#endif
