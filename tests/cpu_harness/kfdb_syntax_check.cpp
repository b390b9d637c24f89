// TEST-ONLY: type-checks include/ydorb/keyFrameDatabase.hpp against declarations of the KeyFrame / Frame members it touches (names as
// DESIGN.md section 6e assumes them).  Built with -fsyntax-only against tests/cpu_harness/mock (DBoW3 / OpenCV declarations).
#include <memory>
#include <set>
#include <vector>
#include "DBoW3/DBoW3.h"
#include "../../include/ydorb/keyFrameDatabase.hpp"

struct KeyFrame {
  DBoW3::BowVector m_bow_wordVec;
  std::vector<std::shared_ptr<KeyFrame>> getBestCovisibilityKeyFrames(const int& N);
  std::set<std::shared_ptr<KeyFrame>> getConnectedKeyFrames();
};
struct Frame {
  DBoW3::BowVector m_bow_wordVec;
};

typedef std::shared_ptr<KeyFrame> KFP;
typedef ydorb::adapter::KeyFrameDatabase<KFP, Frame> KeyFrameDatabase;

// LoopClosing::detectLoop's use, then Tracking::relocalize's
size_t sketch(KeyFrameDatabase& db, KFP cur, Frame& F) {
  db.add(cur);
  db.touch(cur);
  float minScore = 1;
  std::vector<KFP> kept;
  for (double s : db.scoreAgainst(cur, cur->getConnectedKeyFrames(), &kept)) if (s < minScore) minScore = (float)s;
  std::vector<KFP> loop = db.detectLoopCandidates(cur, minScore);
  std::vector<KFP> reloc = db.detectRelocalizationCandidates(&F);
  std::vector<const Frame*> two(2, &F);
  size_t n = db.detectRelocalizationCandidatesBatch(two).size() + db.lastStatus() + db.slotOf(cur);
  db.erase(cur);
  db.clear();
  return loop.size() + reloc.size() + kept.size() + n;
}
