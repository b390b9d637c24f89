// TEST-ONLY: type-checks the resident overloads searchByBowInTwoKeyFrames(mirror, ...) / searchByBowInKeyFrameAndFrame(mirror, ...) of
// include/ydorb/orbMatcher.hpp, trackReferenceKeyFrameSearchImpl of include/ydorb/tracking.hpp and MapMirror::searchByBowKeyFrames /
// searchByBowFrame (include/ydorb/mapMirror.hpp) against mock declarations of the reference's KeyFrame / MapPoint / Frame members they
// touch (names as in adapter_syntax_check.cpp and mapmirror_syntax_check.cpp).  Built with the declaration-only OpenCV mock.
#include <map>
#include <memory>
#include <vector>
#include <opencv2/core.hpp>
#include "../../include/ydorb/mapMirror.hpp"
#include "../../include/ydorb/orbMatcher.hpp"
#include "../../include/ydorb/tracking.hpp"

struct KeyFrame;
typedef std::map<unsigned, std::vector<unsigned>> FeatureVector;
struct MapPoint {
  bool isBad(); std::map<std::shared_ptr<KeyFrame>, size_t> getObservations(); cv::Mat getPosInWorld();
  std::shared_ptr<KeyFrame> getReferenceKeyFrame();
};
struct Frame {
  int m_int_keyPointsNum; std::vector<cv::KeyPoint> m_v_keyPoints; cv::Mat m_cvMat_descriptors; FeatureVector m_bow_keyPointsVec;
};
struct KeyFrame {
  long int m_int_keyFrameID;
  std::vector<cv::KeyPoint> m_v_keyPoints; std::vector<float> m_v_rightXcords; cv::Mat m_cvMat_descriptors; FeatureVector m_bow_keyPointsVec;
  cv::Mat getCameraOriginInWorld(); std::vector<std::shared_ptr<MapPoint>> getMapPointMatches(); bool isBad();
};

namespace ya = ydorb::adapter;
typedef std::shared_ptr<KeyFrame> KF;
typedef std::shared_ptr<MapPoint> MP;
int check(KF current, const std::vector<KF>& candidates, Frame& frame) {
  ya::MapMirror<KF, MP> mirror(0);
  mirror.enableDescriptors(); mirror.enableFeatures(); mirror.enableBow();
  std::vector<std::vector<MP>> loop, reloc;
  std::vector<MP> reference;
  const std::vector<int> nLoop = ya::searchByBowInTwoKeyFrames(mirror, ya::matcher(), current, candidates, loop, 0.75f, true);
  const std::vector<int> nReloc = ya::searchByBowInKeyFrameAndFrame(mirror, ya::matcher(), candidates, frame, reloc, 0.75f, true);
  const int nRef = ya::trackReferenceKeyFrameSearchImpl(mirror, ya::matcher(), frame, current, reference);
  const ya::MapMirror<KF, MP>::BowSearchResult r = mirror.searchByBowKeyFrames(ya::matcher(), current, candidates, 0.6f, false);
  return (int)nLoop.size() + (int)nReloc.size() + nRef + (int)loop.size() + (int)reloc.size() + (int)reference.size() + (int)r.pairStatus.size();
}
