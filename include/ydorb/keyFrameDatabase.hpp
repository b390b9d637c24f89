// Drop-in KeyFrameDatabase whose place-recognition queries run on the MI355X: add / erase / clear / detectLoopCandidates(pKF, minScore) /
// detectRelocalizationCandidates(pFrame) with the reference's signatures (ORB-SLAM2 src/KeyFrameDatabase.cc; YDORBSLAM
// keyFrameDatabase.*), over the C ABI's ydorb_kfdb_*.  The adapter maps key-frame pointers to database slots and pushes the
// covisibility lists the queries read.  INTEGRATION.md has the forwarding bodies; DESIGN.md section 6e the assumed member names:
//   key frame / frame : m_bow_wordVec (DBoW3::BowVector, filled by computeBoW)
//   key frame         : getBestCovisibilityKeyFrames(10) -> std::vector<KeyFramePtr>, getConnectedKeyFrames() -> std::set<KeyFramePtr>
// Covisibility: the device keeps getBestCovisibilityKeyFrames(10) of every key frame.  A key frame's list is pushed when it is added and
// again before the next query after touch(pKF) named it; LocalMapping / LoopClosing call touch() where they call updateConnections().
#ifndef YDORB_ADAPTER_KEYFRAMEDATABASE_HPP
#define YDORB_ADAPTER_KEYFRAMEDATABASE_HPP

#include <cstdint>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "c_api.h"

namespace ydorb {
namespace adapter {

// a BowVector (std::map<WordId, WordValue>) appended to CSR arrays
template <class BowT>
inline void appendBow(const BowT& bow, std::vector<int32_t>& start, std::vector<int32_t>& word, std::vector<double>& value) {
  if (start.empty()) start.push_back(0);
  for (const auto& e : bow) { word.push_back((int32_t)e.first); value.push_back((double)e.second); }
  start.push_back((int32_t)word.size());
}

template <class KeyFramePtr, class FrameT>
class KeyFrameDatabase {
 public:
  // scoring: the vocabulary's DBoW3::ScoringType (L1_NORM for the ORB vocabulary)
  explicit KeyFrameDatabase(int scoring = YDORB_KFDB_L1_NORM, int device = 0) {
    if (ydorb_kfdb_create(device, scoring, 1024, 1 << 20, &m_handle) != YDORB_OK) fail();
  }
  ~KeyFrameDatabase() { ydorb_kfdb_destroy(m_handle); }
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

  void add(KeyFramePtr pKF) {
    std::unique_lock<std::mutex> lock(m_mutex);
    if (m_slotOf.count(pKF)) return;
    std::vector<int32_t> start, word;
    std::vector<double> value;
    appendBow(pKF->m_bow_wordVec, start, word, value);
    int32_t slot = -1;
    if (ydorb_kfdb_add(m_handle, start.data(), word.data(), value.data(), 1, &slot) != YDORB_OK) fail();
    m_slotOf[pKF] = slot;
    if ((int)m_kfOf.size() <= slot) m_kfOf.resize(slot + 1);
    m_kfOf[slot] = pKF;
    m_touched.insert(pKF);
  }

  void erase(KeyFramePtr pKF) {
    std::unique_lock<std::mutex> lock(m_mutex);
    auto it = m_slotOf.find(pKF);
    if (it == m_slotOf.end()) return;
    const int32_t slot = it->second;
    if (ydorb_kfdb_erase(m_handle, &slot, 1) != YDORB_OK) fail();
    m_kfOf[slot] = KeyFramePtr();
    m_slotOf.erase(it);
    m_touched.erase(pKF);
  }

  void clear() {
    std::unique_lock<std::mutex> lock(m_mutex);
    if (ydorb_kfdb_clear(m_handle) != YDORB_OK) fail();
    m_slotOf.clear(); m_kfOf.clear(); m_touched.clear();
  }

  // pKF's connections changed (updateConnections, addConnection, eraseConnection): its covisibility list is pushed before the next query
  void touch(KeyFramePtr pKF) {
    std::unique_lock<std::mutex> lock(m_mutex);
    if (m_slotOf.count(pKF)) m_touched.insert(pKF);
  }

  // Vocabulary::score(pKF->m_bow_wordVec, k->m_bow_wordVec) for every k of `connected` that is in the database, in iteration order:
  // LoopClosing::detectLoop's minimum-score loop.  kept (optional) receives those key frames.
  template <class Container>
  std::vector<double> scoreAgainst(KeyFramePtr pKF, const Container& connected, std::vector<KeyFramePtr>* kept = nullptr) {
    std::unique_lock<std::mutex> lock(m_mutex);
    std::vector<int32_t> slots;
    if (kept) kept->clear();
    for (const KeyFramePtr& k : connected) {
      auto it = m_slotOf.find(k);
      if (it == m_slotOf.end()) continue;
      slots.push_back(it->second);
      if (kept) kept->push_back(k);
    }
    std::vector<int32_t> start, word;
    std::vector<double> value, scores(slots.size());
    appendBow(pKF->m_bow_wordVec, start, word, value);
    if (!slots.empty() &&
        ydorb_kfdb_score(m_handle, word.data(), value.data(), (int32_t)word.size(), slots.data(), (int32_t)slots.size(), scores.data()) != YDORB_OK)
      fail();
    return scores;
  }

  std::vector<KeyFramePtr> detectLoopCandidates(KeyFramePtr pKF, float minScore) {
    std::unique_lock<std::mutex> lock(m_mutex);
    pushCovisibility();
    std::vector<int32_t> start, word, conn, connStart(2, 0);
    std::vector<double> value;
    appendBow(pKF->m_bow_wordVec, start, word, value);
    const std::set<KeyFramePtr> spConnected = pKF->getConnectedKeyFrames();
    for (const KeyFramePtr& k : spConnected) {
      auto it = m_slotOf.find(k);
      if (it != m_slotOf.end()) conn.push_back(it->second);
    }
    connStart[1] = (int32_t)conn.size();
    const int cap = (int)m_slotOf.size();
    std::vector<int32_t> cand(cap > 0 ? cap : 1);
    int32_t count = 0;
    if (ydorb_kfdb_detect_loop(m_handle, start.data(), word.data(), value.data(), 1, connStart.data(), conn.data(), &minScore, cand.data(), cap, &count,
                               &m_lastStatus, nullptr, nullptr) != YDORB_OK)
      fail();
    return toKeyFrames(cand, count);
  }

  std::vector<KeyFramePtr> detectRelocalizationCandidates(FrameT* pFrame) {
    std::vector<const FrameT*> one(1, pFrame);
    return detectRelocalizationCandidatesBatch(one)[0];
  }

  // Several frames in one call, equal to calling detectRelocalizationCandidates on each in order.
  std::vector<std::vector<KeyFramePtr>> detectRelocalizationCandidatesBatch(const std::vector<const FrameT*>& frames) {
    std::unique_lock<std::mutex> lock(m_mutex);
    std::vector<std::vector<KeyFramePtr>> out(frames.size());
    if (frames.empty()) return out;
    pushCovisibility();
    std::vector<int32_t> start, word;
    std::vector<double> value;
    for (const FrameT* f : frames) appendBow(f->m_bow_wordVec, start, word, value);
    const int cap = (int)m_slotOf.size(), Q = (int)frames.size();
    std::vector<int32_t> cand((size_t)Q * (cap > 0 ? cap : 1)), counts(Q), status(Q);
    if (ydorb_kfdb_detect_reloc(m_handle, start.data(), word.data(), value.data(), Q, cand.data(), cap, counts.data(), status.data(), nullptr, nullptr) !=
        YDORB_OK)
      fail();
    for (int q = 0; q < Q; q++) {
      std::vector<int32_t> row(cand.begin() + (size_t)q * cap, cand.begin() + (size_t)q * cap + counts[q]);
      out[q] = toKeyFrames(row, counts[q]);
    }
    m_lastStatus = status[Q - 1];
    return out;
  }

  // YDORB_KFDB_* bits of the last query (a relocalisation that read a stale or never-written mRelocScore)
  int lastStatus() const { return m_lastStatus; }
  int slotOf(KeyFramePtr pKF) const { auto it = m_slotOf.find(pKF); return it == m_slotOf.end() ? -1 : it->second; }
  ydorb_kfdb_t* handle() const { return m_handle; }

 private:
  [[noreturn]] static void fail() { throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error()); }

  void pushCovisibility() {
    if (m_touched.empty()) return;
    std::vector<int32_t> slots, neigh;
    for (const KeyFramePtr& kf : m_touched) {
      slots.push_back(m_slotOf[kf]);
      const std::vector<KeyFramePtr> nb = kf->getBestCovisibilityKeyFrames(10);
      for (int k = 0; k < 10; k++) {
        int32_t s = -1;
        if (k < (int)nb.size()) { auto it = m_slotOf.find(nb[k]); if (it != m_slotOf.end()) s = it->second; }
        neigh.push_back(s);
      }
    }
    if (ydorb_kfdb_set_covisibility(m_handle, slots.data(), neigh.data(), (int32_t)slots.size()) != YDORB_OK) fail();
    m_touched.clear();
  }

  std::vector<KeyFramePtr> toKeyFrames(const std::vector<int32_t>& slots, int count) const {
    std::vector<KeyFramePtr> v;
    v.reserve(count);
    for (int i = 0; i < count; i++) v.push_back(m_kfOf[slots[i]]);
    return v;
  }

  ydorb_kfdb_t* m_handle = nullptr;
  std::mutex m_mutex;
  std::map<KeyFramePtr, int32_t> m_slotOf;
  std::vector<KeyFramePtr> m_kfOf;
  std::set<KeyFramePtr> m_touched;
  int32_t m_lastStatus = 0;
};

}  // namespace adapter
}  // namespace ydorb
#endif
