// TEST-ONLY CPU restatement of ORB-SLAM2's KeyFrameDatabase (src/KeyFrameDatabase.cc) and DBoW's scoring classes
// (ScoringObject.cpp), written the reference's way: an inverted file of std::list<KeyFrame*> per word, the per-key-frame scratch members
// mnRelocQuery / mnRelocWords / mRelocScore / mnLoopQuery / mnLoopWords / mLoopScore, std::map BowVectors walked with two iterators and
// lower_bound, std::list / std::set for the intermediate lists.  Nothing of the product's dense form is shared.  Built with
// oracle/Makefile's flags (-ffp-contract=off).  DESIGN.md section 6e lists what is assumed about the reference.
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace {

typedef std::map<unsigned, double> BowVector;
enum ScoringType { L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT };

// DBoW3 ScoringObject.cpp: the two-iterator walk shared by every scoring class
struct Scoring {
  int type;
  double score(const BowVector& v1, const BowVector& v2) const {
    BowVector::const_iterator v1_it = v1.begin(), v2_it = v2.begin();
    const BowVector::const_iterator v1_end = v1.end(), v2_end = v2.end();
    double score = 0;
    while (v1_it != v1_end && v2_it != v2_end) {
      const double& vi = v1_it->second;
      const double& wi = v2_it->second;
      if (v1_it->first == v2_it->first) {
        if (type == L1_NORM) score += fabs(vi - wi) - fabs(vi) - fabs(wi);
        else if (type == CHI_SQUARE) { if (vi + wi != 0.0) score += vi * wi / (vi + wi); }
        else score += vi * wi;   // L2, dot product
        ++v1_it;
        ++v2_it;
      } else if (v1_it->first < v2_it->first) {
        v1_it = v1.lower_bound(v2_it->first);
      } else {
        v2_it = v2.lower_bound(v1_it->first);
      }
    }
    if (type == L1_NORM) score = -score / 2.0;
    else if (type == L2_NORM) { if (score >= 1) score = 1.0; else score = 1.0 - sqrt(1.0 - score); }
    else if (type == CHI_SQUARE) score = 2. * score;
    return score;
  }
};

struct KeyFrame {
  long id;
  BowVector mBowVec;
  std::vector<KeyFrame*> covis;   // GetBestCovisibilityKeyFrames(10)
  long mnRelocQuery = -1, mnLoopQuery = -1;
  int mnRelocWords = 0, mnLoopWords = 0;
  float mRelocScore = 0.0f, mLoopScore = 0.0f;   // mRelocScore: uninitialised in the reference, defined as 0.0f
  bool relocWritten = false;
};

struct Stats {   // what tests/test_kfdb_cpu.py asserts about the scenarios
  int nSharing, nScored, nRetained, nCandidates, maxCommon, minCommon, status, staleReads;
};

struct Database {
  Scoring voc;
  std::map<unsigned, std::list<KeyFrame*>> mvInvertedFile;   // the reference's vector indexed by word id, sparse here
  std::map<long, KeyFrame*> kfs;
  long nextId = 0, nextQuery = 0;

  void add(KeyFrame* pKF) {
    for (BowVector::const_iterator vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++) mvInvertedFile[vit->first].push_back(pKF);
  }
  void erase(KeyFrame* pKF) {
    for (BowVector::const_iterator vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++) {
      std::list<KeyFrame*>& lKFs = mvInvertedFile[vit->first];
      for (std::list<KeyFrame*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++)
        if (pKF == *lit) { lKFs.erase(lit); break; }
    }
  }

  std::vector<KeyFrame*> DetectRelocalizationCandidates(const BowVector& bow, Stats& S) {
    const long queryId = nextQuery++;
    std::list<KeyFrame*> lKFsSharingWords;
    for (BowVector::const_iterator vit = bow.begin(), vend = bow.end(); vit != vend; vit++) {
      std::map<unsigned, std::list<KeyFrame*>>::iterator f = mvInvertedFile.find(vit->first);
      if (f == mvInvertedFile.end()) continue;
      std::list<KeyFrame*>& lKFs = f->second;
      for (std::list<KeyFrame*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
        KeyFrame* pKFi = *lit;
        if (pKFi->mnRelocQuery != queryId) {
          pKFi->mnRelocWords = 0;
          pKFi->mnRelocQuery = queryId;
          lKFsSharingWords.push_back(pKFi);
        }
        pKFi->mnRelocWords++;
      }
    }
    S.nSharing = (int)lKFsSharingWords.size();
    if (lKFsSharingWords.empty()) return std::vector<KeyFrame*>();
    int maxCommonWords = 0;
    for (std::list<KeyFrame*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++)
      if ((*lit)->mnRelocWords > maxCommonWords) maxCommonWords = (*lit)->mnRelocWords;
    int minCommonWords = maxCommonWords * 0.8f;
    S.maxCommon = maxCommonWords; S.minCommon = minCommonWords;
    std::list<std::pair<float, KeyFrame*>> lScoreAndMatch;
    int nscores = 0;
    for (std::list<KeyFrame*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      KeyFrame* pKFi = *lit;
      if (pKFi->mnRelocWords > minCommonWords) {
        nscores++;
        float si = voc.score(bow, pKFi->mBowVec);
        pKFi->mRelocScore = si;
        pKFi->relocWritten = true;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    S.nScored = nscores;
    if (lScoreAndMatch.empty()) return std::vector<KeyFrame*>();
    std::list<std::pair<float, KeyFrame*>> lAccScoreAndMatch;
    float bestAccScore = 0;
    for (std::list<std::pair<float, KeyFrame*>>::iterator it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
      KeyFrame* pKFi = it->second;
      std::vector<KeyFrame*>& vpNeighs = pKFi->covis;
      float bestScore = it->first;
      float accScore = bestScore;
      KeyFrame* pBestKF = pKFi;
      for (std::vector<KeyFrame*>::iterator vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
        KeyFrame* pKF2 = *vit;
        if (pKF2->mnRelocQuery != queryId) continue;
        if (!pKF2->relocWritten) S.status |= 2;
        else if (!(pKF2->mnRelocWords > minCommonWords)) { S.status |= 1; S.staleReads++; }
        accScore += pKF2->mRelocScore;
        if (pKF2->mRelocScore > bestScore) {
          pBestKF = pKF2;
          bestScore = pKF2->mRelocScore;
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    float minScoreToRetain = 0.75f * bestAccScore;
    std::set<KeyFrame*> spAlreadyAddedKF;
    std::vector<KeyFrame*> vpRelocCandidates;
    vpRelocCandidates.reserve(lAccScoreAndMatch.size());
    for (std::list<std::pair<float, KeyFrame*>>::iterator it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
      const float& si = it->first;
      if (si > minScoreToRetain) {
        S.nRetained++;
        KeyFrame* pKFi = it->second;
        if (!spAlreadyAddedKF.count(pKFi)) {
          vpRelocCandidates.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        }
      }
    }
    S.nCandidates = (int)vpRelocCandidates.size();
    return vpRelocCandidates;
  }

  std::vector<KeyFrame*> DetectLoopCandidates(const BowVector& bow, const std::set<KeyFrame*>& spConnectedKeyFrames, float minScore, Stats& S) {
    const long queryId = nextQuery++;
    std::list<KeyFrame*> lKFsSharingWords;
    for (BowVector::const_iterator vit = bow.begin(), vend = bow.end(); vit != vend; vit++) {
      std::map<unsigned, std::list<KeyFrame*>>::iterator f = mvInvertedFile.find(vit->first);
      if (f == mvInvertedFile.end()) continue;
      std::list<KeyFrame*>& lKFs = f->second;
      for (std::list<KeyFrame*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
        KeyFrame* pKFi = *lit;
        if (pKFi->mnLoopQuery != queryId) {
          pKFi->mnLoopWords = 0;
          if (!spConnectedKeyFrames.count(pKFi)) {
            pKFi->mnLoopQuery = queryId;
            lKFsSharingWords.push_back(pKFi);
          }
        }
        pKFi->mnLoopWords++;
      }
    }
    S.nSharing = (int)lKFsSharingWords.size();
    if (lKFsSharingWords.empty()) return std::vector<KeyFrame*>();
    std::list<std::pair<float, KeyFrame*>> lScoreAndMatch;
    int maxCommonWords = 0;
    for (std::list<KeyFrame*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++)
      if ((*lit)->mnLoopWords > maxCommonWords) maxCommonWords = (*lit)->mnLoopWords;
    int minCommonWords = maxCommonWords * 0.8f;
    S.maxCommon = maxCommonWords; S.minCommon = minCommonWords;
    int nscores = 0;
    for (std::list<KeyFrame*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      KeyFrame* pKFi = *lit;
      if (pKFi->mnLoopWords > minCommonWords) {
        nscores++;
        float si = voc.score(bow, pKFi->mBowVec);
        pKFi->mLoopScore = si;
        if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    S.nScored = nscores;
    if (lScoreAndMatch.empty()) return std::vector<KeyFrame*>();
    std::list<std::pair<float, KeyFrame*>> lAccScoreAndMatch;
    float bestAccScore = minScore;
    for (std::list<std::pair<float, KeyFrame*>>::iterator it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
      KeyFrame* pKFi = it->second;
      std::vector<KeyFrame*>& vpNeighs = pKFi->covis;
      float bestScore = it->first;
      float accScore = it->first;
      KeyFrame* pBestKF = pKFi;
      for (std::vector<KeyFrame*>::iterator vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
        KeyFrame* pKF2 = *vit;
        if (pKF2->mnLoopQuery == queryId && pKF2->mnLoopWords > minCommonWords) {
          accScore += pKF2->mLoopScore;
          if (pKF2->mLoopScore > bestScore) {
            pBestKF = pKF2;
            bestScore = pKF2->mLoopScore;
          }
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    float minScoreToRetain = 0.75f * bestAccScore;
    std::set<KeyFrame*> spAlreadyAddedKF;
    std::vector<KeyFrame*> vpLoopCandidates;
    vpLoopCandidates.reserve(lAccScoreAndMatch.size());
    for (std::list<std::pair<float, KeyFrame*>>::iterator it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
      if (it->first > minScoreToRetain) {
        S.nRetained++;
        KeyFrame* pKFi = it->second;
        if (!spAlreadyAddedKF.count(pKFi)) {
          vpLoopCandidates.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        }
      }
    }
    S.nCandidates = (int)vpLoopCandidates.size();
    return vpLoopCandidates;
  }
};

BowVector makeBow(const int32_t* word, const double* value, int n) {
  BowVector v;
  for (int i = 0; i < n; i++) v.insert(v.end(), std::make_pair((unsigned)word[i], value[i]));
  return v;
}

}  // namespace

extern "C" {

void* kfdbref_create(int scoring) {
  Database* d = new Database;
  d->voc.type = scoring;
  return d;
}

void kfdbref_destroy(void* h) {
  Database* d = static_cast<Database*>(h);
  for (auto& kv : d->kfs) delete kv.second;
  delete d;
}

// a new key frame with this BowVector, added to the database; returns its id
long kfdbref_add(void* h, const int32_t* word, const double* value, int n) {
  Database* d = static_cast<Database*>(h);
  KeyFrame* kf = new KeyFrame;
  kf->id = d->nextId++;
  kf->mBowVec = makeBow(word, value, n);
  d->kfs[kf->id] = kf;
  d->add(kf);
  return kf->id;
}

// erase + the part of setBadFlag the queries see: the key frame leaves every covisibility list
int kfdbref_erase(void* h, long id) {
  Database* d = static_cast<Database*>(h);
  auto it = d->kfs.find(id);
  if (it == d->kfs.end()) return -1;
  KeyFrame* kf = it->second;
  d->erase(kf);
  for (auto& kv : d->kfs) {
    std::vector<KeyFrame*>& c = kv.second->covis;
    for (size_t i = 0; i < c.size();) { if (c[i] == kf) c.erase(c.begin() + i); else i++; }
  }
  d->kfs.erase(it);
  delete kf;
  return 0;
}

void kfdbref_clear(void* h) {
  Database* d = static_cast<Database*>(h);
  d->mvInvertedFile.clear();
  for (auto& kv : d->kfs) delete kv.second;
  d->kfs.clear();
}

int kfdbref_set_covisibility(void* h, long id, const long* neigh, int n) {
  Database* d = static_cast<Database*>(h);
  auto it = d->kfs.find(id);
  if (it == d->kfs.end()) return -1;
  it->second->covis.clear();
  for (int i = 0; i < n && i < 10; i++) {
    auto nb = d->kfs.find(neigh[i]);
    if (nb != d->kfs.end()) it->second->covis.push_back(nb->second);
  }
  return 0;
}

double kfdbref_score(void* h, const int32_t* word, const double* value, int n, long id) {
  Database* d = static_cast<Database*>(h);
  return d->voc.score(makeBow(word, value, n), d->kfs.at(id)->mBowVec);
}

// out ids [capacity of the database]; stats [8]; diag: per key frame in ascending id (ids[], words[], score[]), nDiag entries:
// the key frames that share a word with the query, their common-word count and (float)score
int kfdbref_detect(void* h, int loop, const int32_t* word, const double* value, int n, const long* connected, int nConnected, float minScore,
                   long* out, int* stats, long* diagId, int* diagWords, float* diagScore, int* nDiag) {
  Database* d = static_cast<Database*>(h);
  const BowVector bow = makeBow(word, value, n);
  Stats S = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<KeyFrame*> r;
  if (loop) {
    std::set<KeyFrame*> conn;
    for (int i = 0; i < nConnected; i++) { auto it = d->kfs.find(connected[i]); if (it != d->kfs.end()) conn.insert(it->second); }
    r = d->DetectLoopCandidates(bow, conn, minScore, S);
  } else {
    r = d->DetectRelocalizationCandidates(bow, S);
  }
  for (size_t i = 0; i < r.size(); i++) out[i] = r[i]->id;
  const int st[8] = {S.nSharing, S.nScored, S.nRetained, S.nCandidates, S.maxCommon, S.minCommon, S.status, S.staleReads};
  for (int i = 0; i < 8; i++) stats[i] = st[i];
  if (diagId) {
    // a tally of its own over the inverted file: a connected key frame shares words too, although it never enters the list
    std::map<long, int> tally;
    for (BowVector::const_iterator vit = bow.begin(); vit != bow.end(); vit++) {
      auto f = d->mvInvertedFile.find(vit->first);
      if (f == d->mvInvertedFile.end()) continue;
      for (KeyFrame* kf : f->second) tally[kf->id]++;
    }
    int k = 0;
    for (auto& t : tally) {
      diagId[k] = t.first; diagWords[k] = t.second; diagScore[k] = (float)d->voc.score(bow, d->kfs.at(t.first)->mBowVec);
      k++;
    }
    *nDiag = k;
  }
  return (int)r.size();
}

}  // extern "C"
