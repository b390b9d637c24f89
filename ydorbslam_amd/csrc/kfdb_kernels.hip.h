// Kernels of the key-frame database on the MI355X: KeyFrameDatabase::detectRelocalizationCandidates /
// detectLoopCandidates (ORB-SLAM2 src/KeyFrameDatabase.cc) and DBoW's scoring classes (ScoringObject.cpp) in a dense form: one
// sparse query BowVector against every stored one, instead of the reference's inverted file and per-key-frame scratch members.
//
//   k_kfdb_intersect : one wave per (query, slot).  The query's word ids are staged in LDS; every lane takes one word of the row and
//                      looks it up by binary search.  Gives the number of common words (mnRelocWords / mnLoopWords), the first
//                      common word (where the reference's walk over the query's words pushes the key frame into lKFsSharingWords)
//                      and the score.  The score's sum runs over the matching lanes in lane order, chunk after chunk: the common
//                      words in ascending id, one IEEE add each, exactly DBoW's loop.  Non-matching lanes add nothing at all.
//   k_kfdb_select    : one workgroup per query (loop form) or one workgroup for all queries in order (relocalisation form, whose
//                      mRelocScore carries over from query to query): max / min common words, the scored set, the neighbour
//                      accumulation, the 0.75 rule, first-occurrence de-duplication and the list order (first common word, add sequence).
//   k_kfdb_compact   : moves the live rows into a new pool.
// Every store is an ordinary vector store; nothing is read back by the host between the kernels of a call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ydorb {
namespace kfdb {

constexpr int kMaxQueryWords = 8192;   // word ids of one query in LDS (32 KB); ydorb_vocabulary_transform emits at most as many
constexpr int kNeigh = 10;             // getBestCovisibilityKeyFrames(10)
constexpr int kSlotsPerBlock = 16;     // rows one workgroup of k_kfdb_intersect takes: the staged query serves four rows per wave
constexpr int kSelectThreads = 1024;
constexpr unsigned long long kNoKey = ~0ull;

enum Scoring { kL1 = 0, kL2 = 1, kChiSquare = 2, kKL = 3, kBhattacharyya = 4, kDot = 5 };
enum Form { kReloc = 0, kLoop = 1 };
enum Status { kStaleScore = 1, kUnwrittenScore = 2 };

struct DbView {
  const int* rowWord;          // pool: word ids, ascending within a row
  const double* rowVal;        // pool: values
  const long long* rowOff;     // [slots]
  const int* rowLen;           // [slots]
  const int* live;             // [slots]
  const unsigned* seq;         // [slots] add sequence number (> 0)
  const int* neigh;            // [slots][10] neighbour slots, -1 = none
  const unsigned* neighSeq;    // [slots][10] the neighbour's sequence number when the list was set: a reused slot is another key frame
  float* relocScore;           // [slots] KeyFrame::mRelocScore, kept between queries
  unsigned* relocSeq;          // [slots] sequence number of the key frame that mRelocScore was written for (0: never)
  int nSlots;
};

struct QueryView {
  const int* start;            // [Q + 1]
  const int* word;
  const double* val;
};

// grid (ceil(n / kSlotsPerBlock), Q), 256 threads.  slotList == nullptr: item i is slot i.  Outputs at [q * n + i].
__global__ __launch_bounds__(256) void k_kfdb_intersect(DbView D, QueryView Qv, const int* __restrict__ slotList, int n, int scoring,
                                                        int* __restrict__ common, int* __restrict__ first, double* __restrict__ score) {
  __shared__ int sq[kMaxQueryWords];
  const int q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = Qv.start[q], Lq = min(Qv.start[q + 1] - q0, kMaxQueryWords);
  for (int i = threadIdx.x; i < Lq; i += 256) sq[i] = Qv.word[q0 + i];
  __syncthreads();
  const int qLo = Lq > 0 ? sq[0] : 0, qHi = Lq > 0 ? sq[Lq - 1] : -1;
  for (int r = wave; r < kSlotsPerBlock; r += 4) {
    const int item = blockIdx.x * kSlotsPerBlock + r;
    if (item >= n) break;
    const int slot = slotList ? slotList[item] : item;
    int cnt = 0, fw = -1;
    double s = 0.0;
    const bool ok = slot >= 0 && slot < D.nSlots && D.live[slot] != 0;
    if (ok) {
      const long long off = D.rowOff[slot];
      const int len = D.rowLen[slot];
      for (int c = 0; c < len; c += 64) {
        const int e = c + lane;
        int w = -1, pos = -1;
        if (e < len) w = D.rowWord[off + e];
        if (e < len && w >= qLo && w <= qHi) {
          int lo = 0, hi = Lq;   // lower_bound
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sq[mid] < w) lo = mid + 1; else hi = mid;
          }
          if (lo < Lq && sq[lo] == w) pos = lo;
        }
        const bool match = pos >= 0;
        const unsigned long long m = __ballot(match);
        if (m == 0) continue;   // wave-uniform
        if (fw < 0) fw = __shfl(w, __ffsll((long long)m) - 1, 64);
        cnt += __popcll(m);
        double term = 0.0;
        bool add = match;
        if (match) {
          const double vi = Qv.val[q0 + pos], wi = D.rowVal[off + e];   // score(query, key frame): v1 = query
          if (scoring == kL1) {
            term = fabs(vi - wi) - fabs(vi) - fabs(wi);
          } else if (scoring == kChiSquare) {
            const double d = vi + wi;
            add = d != 0.0;
            if (add) term = vi * wi / d;
          } else {   // L2, dot product
            term = vi * wi;
          }
        }
        unsigned long long ma = __ballot(add);
        while (ma) {   // the common words in ascending id: `score += term`, one add each
          const int j = __ffsll((long long)ma) - 1;
          s += __shfl(term, j, 64);
          ma &= ma - 1;
        }
      }
    }
    if (lane == 0) {
      double sc;
      if (scoring == kL1) sc = -s / 2.0;
      else if (scoring == kL2) sc = s >= 1 ? 1.0 : 1.0 - sqrt(1.0 - s);
      else if (scoring == kChiSquare) sc = 2. * s;
      else sc = s;
      const size_t at = (size_t)q * n + item;
      common[at] = cnt;
      first[at] = fw;
      score[at] = ok ? sc : 0.0;
    }
  }
}

struct SelectArgs {
  DbView D;
  int form, nQueries, candCap;
  const int* common;            // [Q][nSlots]
  const int* first;             // [Q][nSlots]
  const double* score;          // [Q][nSlots]
  const int* connStart;         // loop form: [Q + 1]
  const int* connSlots;
  const float* minScore;        // loop form: [Q]
  // scratch: one set per concurrently running query (loop: Q sets, relocalisation: 1)
  uint8_t* conn;                // [sets][nSlots]
  float* acc;                   // [sets][nSlots]
  int* bestKF;                  // [sets][nSlots]
  unsigned long long* firstKey; // [sets][nSlots]
  unsigned long long* sortKey;  // [sets][n2]
  int* sortVal;                 // [sets][n2]
  int n2;                       // nSlots rounded up to a power of two
  // results
  int* cand;                    // [Q][candCap]
  int* counts;                  // [Q]
  int* status;                  // [Q]
  int* diagWords;               // [nSlots] of the last query
  float* diagScore;             // [nSlots]
};

// Block reductions: a wave-shuffle stage, then the 16 wave results through LDS (two barriers each).  Maxima and integer sums do not
// depend on the order.
__device__ inline int block_max_int(int v, int* red) {
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
  for (int w = 1; w < kSelectThreads / 64; w++) r = max(r, red[w]);
  __syncthreads();
  return r;
}

// `if (accScore > bestAccScore) bestAccScore = accScore` over a list: the maximum, whatever the order (NaN scores are out of scope)
__device__ inline float block_max_float(float v, float* red) {
  for (int d = 32; d > 0; d >>= 1) { const float o = __shfl_xor(v, d, 64); if (o > v) v = o; }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < kSelectThreads / 64; w++) if (red[w] > r) r = red[w];
  __syncthreads();
  return r;
}

__device__ inline int block_sum_int(int v, int* red) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
  for (int w = 0; w < kSelectThreads / 64; w++) r += red[w];
  __syncthreads();
  return r;
}

// ascending bitonic sort of n2 (power of two) unique keys with a payload, in HBM scratch, by one workgroup
__device__ inline void block_sort_pairs(unsigned long long* key, int* val, int n2) {
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n2 >> 1); t += kSelectThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const unsigned long long a = key[lo], b = key[hi];
        if ((a > b) == up) {
          key[lo] = b; key[hi] = a;
          const int va = val[lo]; val[lo] = val[hi]; val[hi] = va;
        }
      }
      __syncthreads();
    }
  }
}

// One query, by the whole workgroup.  `set` selects the scratch.
__device__ void select_one(const SelectArgs& A, int q, int set, int* red) {
  __shared__ int sCount;
  const DbView& D = A.D;
  const int H = D.nSlots, tid = threadIdx.x;
  const bool loop = A.form == kLoop;
  const int* common = A.common + (size_t)q * H;
  const int* first = A.first + (size_t)q * H;
  const double* score = A.score + (size_t)q * H;
  uint8_t* conn = A.conn + (size_t)set * H;
  float* acc = A.acc + (size_t)set * H;
  int* bestKF = A.bestKF + (size_t)set * H;
  unsigned long long* firstKey = A.firstKey + (size_t)set * H;
  unsigned long long* sortKey = A.sortKey + (size_t)set * A.n2;
  int* sortVal = A.sortVal + (size_t)set * A.n2;
  float* redf = reinterpret_cast<float*>(red);

  // spConnectedKeyFrames: these never enter lKFsSharingWords
  for (int i = tid; i < H; i += kSelectThreads) { conn[i] = 0; firstKey[i] = kNoKey; }
  __syncthreads();
  if (loop) {
    for (int k = A.connStart[q] + tid; k < A.connStart[q + 1]; k += kSelectThreads) {
      const int c = A.connSlots[k];
      if (c >= 0 && c < H) conn[c] = 1;
    }
    __syncthreads();
  }
  // lKFsSharingWords = live slots with a common word (and not connected); maxCommonWords over it
  int m = 0;
  for (int i = tid; i < H; i += kSelectThreads)
    if (D.live[i] && !conn[i]) m = max(m, common[i]);
  const int maxCommon = block_max_int(m, red);
  if (q == A.nQueries - 1 && A.diagWords) {
    for (int i = tid; i < H; i += kSelectThreads) {
      const bool sh = D.live[i] && common[i] > 0;
      A.diagWords[i] = sh ? common[i] : 0;
      A.diagScore[i] = sh ? (float)score[i] : 0.0f;
    }
  }
  if (maxCommon == 0) {   // `if (lKFsSharingWords.empty()) return`
    if (tid == 0) { A.counts[q] = 0; A.status[q] = 0; }
    __syncthreads();
    return;
  }
  const int minCommon = (int)((float)maxCommon * 0.8f);   // int minCommonWords = maxCommonWords * 0.8f
  const float minScore = loop ? A.minScore[q] : 0.0f;
  // scores: mRelocScore = si (kept); mLoopScore = si is score[] itself
  if (!loop) {
    for (int i = tid; i < H; i += kSelectThreads)
      if (D.live[i] && common[i] > minCommon) { D.relocScore[i] = (float)score[i]; D.relocSeq[i] = D.seq[i]; }
    __syncthreads();
  }
  // lScoreAndMatch -> lAccScoreAndMatch: entry i is slot i
  float bestAcc = minScore;   // float bestAccScore = 0 (relocalisation) / minScore (loop)
  int st = 0, nEntries = 0;
  for (int i = tid; i < H; i += kSelectThreads) {
    bool entry = D.live[i] && !conn[i] && common[i] > minCommon;
    const float si = (float)score[i];
    if (loop && !(si >= minScore)) entry = false;
    float a = 0.0f;
    int best = -1;
    if (entry) {
      float bestScore = si;
      a = si;
      best = i;
      for (int k = 0; k < kNeigh; k++) {
        const int nb = D.neigh[(size_t)i * kNeigh + k];
        if (nb < 0 || nb >= H || !D.live[nb] || D.seq[nb] != D.neighSeq[(size_t)i * kNeigh + k]) continue;
        if (common[nb] == 0 || conn[nb]) continue;   // mnRelocQuery / mnLoopQuery != this query
        float ns;
        if (loop) {
          if (!(common[nb] > minCommon)) continue;
          ns = (float)score[nb];                     // mLoopScore, stored before the minScore filter
        } else if (D.relocSeq[nb] == D.seq[nb]) {
          ns = D.relocScore[nb];
          if (!(common[nb] > minCommon)) st |= kStaleScore;   // not scored by this query: an earlier query's value
        } else {
          ns = 0.0f;                                 // never written: defined as 0.0f
          st |= kUnwrittenScore;
        }
        a += ns;
        if (ns > bestScore) { best = nb; bestScore = ns; }
      }
      nEntries++;
      if (a > bestAcc) bestAcc = a;
    }
    acc[i] = a;
    bestKF[i] = best;
  }
  bestAcc = block_max_float(bestAcc, redf);
  nEntries = block_sum_int(nEntries, red);
  if (st) atomicOr(&A.status[q], st);
  if (nEntries == 0) {   // `if (lScoreAndMatch.empty()) return`
    if (tid == 0) A.counts[q] = 0;
    __syncthreads();
    return;
  }
  const float minRetain = 0.75f * bestAcc;
  // the place of a candidate in the result is the place of its first retained entry: key (first common word, add sequence)
  for (int i = tid; i < H; i += kSelectThreads)
    if (bestKF[i] >= 0 && acc[i] > minRetain)
      atomicMin(&firstKey[bestKF[i]], ((unsigned long long)(unsigned)first[i] << 32) | D.seq[i]);
  if (tid == 0) sCount = 0;
  __syncthreads();
  for (int i = tid; i < H; i += kSelectThreads)
    if (firstKey[i] != kNoKey) {
      const int at = atomicAdd(&sCount, 1);
      sortKey[at] = firstKey[i];
      sortVal[at] = i;
    }
  __syncthreads();
  const int R = sCount;
  int n2 = 1;
  while (n2 < R) n2 <<= 1;
  for (int i = R + tid; i < n2; i += kSelectThreads) { sortKey[i] = kNoKey; sortVal[i] = -1; }
  __syncthreads();
  block_sort_pairs(sortKey, sortVal, n2);
  for (int i = tid; i < R && i < A.candCap; i += kSelectThreads) A.cand[(size_t)q * A.candCap + i] = sortVal[i];
  if (tid == 0) A.counts[q] = R;
  __syncthreads();
}

// loop form: grid (Q); relocalisation form: grid (1), the queries one after the other.  status[] is zeroed by the host.
__global__ __launch_bounds__(kSelectThreads) void k_kfdb_select(SelectArgs A) {
  __shared__ int red[kSelectThreads / 64];
  if (A.form == kLoop) {
    select_one(A, blockIdx.x, blockIdx.x, red);
  } else {
    for (int q = 0; q < A.nQueries; q++) {
      select_one(A, q, 0, red);
      __threadfence();
      __syncthreads();
    }
  }
}

// grid (slots), 256 threads: row of slot b from the old pool to the new one
__global__ __launch_bounds__(256) void k_kfdb_compact(const int* __restrict__ oldWord, const double* __restrict__ oldVal, const long long* __restrict__ oldOff,
                                                      const long long* __restrict__ newOff, const int* __restrict__ len, const int* __restrict__ live,
                                                      int* __restrict__ newWord, double* __restrict__ newVal) {
  const int b = blockIdx.x;
  if (!live[b]) return;
  const long long o = oldOff[b], n = newOff[b];
  for (int i = threadIdx.x; i < len[b]; i += 256) { newWord[n + i] = oldWord[o + i]; newVal[n + i] = oldVal[o + i]; }
}

}  // namespace kfdb
}  // namespace ydorb
