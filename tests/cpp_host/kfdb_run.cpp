// TEST-ONLY: EXECUTES include/ydorb/keyFrameDatabase.hpp on the GPU against stand-ins of the reference's KeyFrame / Frame that carry
// real BowVectors and covisibility lists, and dumps what every query returned; tests/test_kfdb_adapter_gpu.py writes the scenario
// (the operation list of tests/kfdb_support.py) and replays it through the ctypes path.
//
//   kfdb_run scenario.bin out.bin
// scenario: records of int32 op, then  0 add: n, n x vector | 1 erase: n, ids | 2 covis: n, n x (id, m, m ids) | 3 score: vector, n, ids
//           | 4 reloc: Q, Q x vector | 5 loop: Q, Q x (vector, nConn, ids, float minScore) | -1 end;  vector = len, int32 words, double values
// out: score: n, doubles | reloc / loop: per query count, key-frame ids, status
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "../../include/ydorb/keyFrameDatabase.hpp"

namespace {

struct Reader {
  FILE* f;
  explicit Reader(const char* path) : f(fopen(path, "rb")) { if (!f) { perror(path); exit(2); } }
  ~Reader() { fclose(f); }
  template <class T> T get() { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "scenario truncated\n"); exit(2); } return v; }
};
struct Writer {
  FILE* f;
  explicit Writer(const char* path) : f(fopen(path, "wb")) { if (!f) { perror(path); exit(2); } }
  ~Writer() { fclose(f); }
  template <class T> void put(const T& v) { fwrite(&v, sizeof(T), 1, f); }
};

typedef std::map<unsigned, double> BowVector;   // DBoW3::BowVector

struct KeyFrame {
  int id = -1;
  BowVector m_bow_wordVec;
  std::vector<std::shared_ptr<KeyFrame>> covis;
  std::set<std::shared_ptr<KeyFrame>> connected;
  std::vector<std::shared_ptr<KeyFrame>> getBestCovisibilityKeyFrames(const int& N) {
    return (int)covis.size() > N ? std::vector<std::shared_ptr<KeyFrame>>(covis.begin(), covis.begin() + N) : covis;
  }
  std::set<std::shared_ptr<KeyFrame>> getConnectedKeyFrames() { return connected; }
};
struct Frame {
  BowVector m_bow_wordVec;
};
typedef std::shared_ptr<KeyFrame> KFP;
typedef ydorb::adapter::KeyFrameDatabase<KFP, Frame> Database;

BowVector readVector(Reader& R) {
  const int n = R.get<int32_t>();
  std::vector<int32_t> w(n);
  for (int i = 0; i < n; i++) w[i] = R.get<int32_t>();
  BowVector v;
  for (int i = 0; i < n; i++) v[(unsigned)w[i]] = R.get<double>();
  return v;
}

void putResult(Writer& W, const std::vector<KFP>& r, int status) {
  W.put<int32_t>((int32_t)r.size());
  for (const KFP& k : r) W.put<int32_t>(k->id);
  W.put<int32_t>(status);
}

int run(Reader& R, Writer& W) {
  Database db(YDORB_KFDB_L1_NORM);
  std::vector<KFP> kfs;   // by creation index
  for (;;) {
    const int op = R.get<int32_t>();
    if (op < 0) break;
    if (op == 0) {
      const int n = R.get<int32_t>();
      for (int i = 0; i < n; i++) {
        KFP k = std::make_shared<KeyFrame>();
        k->id = (int)kfs.size();
        k->m_bow_wordVec = readVector(R);
        kfs.push_back(k);
        db.add(k);
      }
    } else if (op == 1) {
      const int n = R.get<int32_t>();
      for (int i = 0; i < n; i++) {
        KFP k = kfs[R.get<int32_t>()];
        for (KFP& o : kfs)   // setBadFlag: the key frame leaves its neighbours' lists
          if (o) for (size_t j = 0; j < o->covis.size();) { if (o->covis[j] == k) o->covis.erase(o->covis.begin() + j); else j++; }
        db.erase(k);
      }
    } else if (op == 2) {
      const int n = R.get<int32_t>();
      for (int i = 0; i < n; i++) {
        KFP k = kfs[R.get<int32_t>()];
        const int m = R.get<int32_t>();
        k->covis.clear();
        for (int j = 0; j < m; j++) k->covis.push_back(kfs[R.get<int32_t>()]);
        db.touch(k);
      }
    } else if (op == 3) {
      KFP q = std::make_shared<KeyFrame>();
      q->m_bow_wordVec = readVector(R);
      const int n = R.get<int32_t>();
      std::vector<KFP> against;
      for (int i = 0; i < n; i++) against.push_back(kfs[R.get<int32_t>()]);
      const std::vector<double> s = db.scoreAgainst(q, against);
      W.put<int32_t>((int32_t)s.size());
      for (double v : s) W.put<double>(v);
    } else if (op == 4) {
      const int Q = R.get<int32_t>();
      std::vector<Frame> frames(Q);
      for (Frame& f : frames) f.m_bow_wordVec = readVector(R);
      if (Q == 1) {
        const std::vector<KFP> r = db.detectRelocalizationCandidates(&frames[0]);   // before lastStatus() is read
        putResult(W, r, db.lastStatus());
      } else {
        std::vector<const Frame*> ptrs;
        for (Frame& f : frames) ptrs.push_back(&f);
        // the batch reports the last query's status only: -1 marks "not reported"
        const std::vector<std::vector<KFP>> r = db.detectRelocalizationCandidatesBatch(ptrs);
        for (int q = 0; q < Q; q++) putResult(W, r[q], q == Q - 1 ? db.lastStatus() : -1);
      }
    } else if (op == 5) {
      const int Q = R.get<int32_t>();
      for (int q = 0; q < Q; q++) {
        KFP cur = std::make_shared<KeyFrame>();
        cur->m_bow_wordVec = readVector(R);
        const int n = R.get<int32_t>();
        for (int i = 0; i < n; i++) cur->connected.insert(kfs[R.get<int32_t>()]);
        const float minScore = R.get<float>();
        const std::vector<KFP> r = db.detectLoopCandidates(cur, minScore);
        putResult(W, r, db.lastStatus());
      }
    } else {
      fprintf(stderr, "unknown op %d\n", op);
      return 2;
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: kfdb_run scenario.bin out.bin\n"); return 2; }
  try {
    Reader R(argv[1]);
    Writer W(argv[2]);
    return run(R, W);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
