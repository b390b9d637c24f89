// Key-frame database on the MI355X + its C ABI (include/ydorb/c_api.h, "KeyFrameDatabase"): ydorb_kfdb_*.  Replaces
// KeyFrameDatabase::add / erase / clear / detectLoopCandidates / detectRelocalizationCandidates (ORB-SLAM2 src/KeyFrameDatabase.cc) and
// the DBoW3::Vocabulary::score calls in them and in LoopClosing::detectLoop.  The BowVectors live in HBM as rows of a pool
// (word ids ascending + double values, 12 bytes per word); the host keeps the slot table (offsets, live flags, add sequence numbers,
// neighbour lists) and uploads what changed before a query.  A query runs the kernels of kfdb_kernels.hip.h back to back and reads
// back the candidates at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "host_buffers.h"
#include "kfdb_kernels.hip.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::kfdb;

namespace {

// Grows a device buffer to twice `bytes`, zero-filled, keeping its first `keep` bytes; done when it returns.
int grow(Mem& m, size_t bytes, size_t keep, hipStream_t s) {
  if (bytes <= m.cap) return YDORB_OK;
  ScopedMem n;
  int rc = n.alloc(std::max<size_t>(bytes * 2, 4096));
  if (rc) return rc;
  if (hipMemsetAsync(n.p, 0, n.cap, s) != hipSuccess || (m.p && keep && hipMemcpyAsync(n.p, m.p, keep, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
      hipStreamSynchronize(s) != hipSuccess) {
    set_error("growing a device buffer failed");
    return YDORB_ERR_HIP;
  }
  m.take(n);
  return YDORB_OK;
}

constexpr int kQueryChunk = 64;   // queries per kernel sequence: bounds the scratch (about 60 bytes per query and slot)

}  // namespace

struct ydorb_kfdb {
  int device = 0, scoring = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;   // tracking (relocalisation), local mapping (add / erase) and loop closing reach one database
  // slot table (host mirror)
  std::vector<long long> off;
  std::vector<int> len, live;
  std::vector<unsigned> seq;
  std::vector<int> neigh;
  std::vector<unsigned> neighSeq;
  std::vector<int> freeSlots;
  unsigned nextSeq = 1;
  int nLive = 0;
  long long poolUsed = 0, poolLiveWords = 0, poolCap = 0;
  int dirtyLo = 0, dirtyHi = 0;   // slots whose table entries the device copy lacks
  // device
  Mem dWord, dVal, dOff, dLen, dLive, dSeq, dNeigh, dNeighSeq, dRelocScore, dRelocSeq, dTmp;
  Mem up, work, down;
  int slotCap = 0;
  int nSlots() const { return (int)off.size(); }
  DbView view() {
    DbView D;
    D.rowWord = dWord.as<int>(); D.rowVal = dVal.as<double>(); D.rowOff = dOff.as<long long>(); D.rowLen = dLen.as<int>();
    D.live = dLive.as<int>(); D.seq = dSeq.as<unsigned>(); D.neigh = dNeigh.as<int>(); D.neighSeq = dNeighSeq.as<unsigned>();
    D.relocScore = dRelocScore.as<float>(); D.relocSeq = dRelocSeq.as<unsigned>(); D.nSlots = nSlots();
    return D;
  }
  void touch(int s) {
    if (dirtyHi <= dirtyLo) { dirtyLo = s; dirtyHi = s + 1; }
    else { dirtyLo = std::min(dirtyLo, s); dirtyHi = std::max(dirtyHi, s + 1); }
  }
};

namespace {

int growSlots(ydorb_kfdb* h, int want) {
  if (want <= h->slotCap) return YDORB_OK;
  const int cap = std::max(want * 2, 64), keep = h->slotCap;
  hipStream_t s = h->stream;
  int rc;
  if ((rc = grow(h->dOff, sizeof(long long) * cap, sizeof(long long) * keep, s)) || (rc = grow(h->dLen, sizeof(int) * cap, sizeof(int) * keep, s)) ||
      (rc = grow(h->dLive, sizeof(int) * cap, sizeof(int) * keep, s)) || (rc = grow(h->dSeq, sizeof(unsigned) * cap, sizeof(unsigned) * keep, s)) ||
      (rc = grow(h->dNeigh, sizeof(int) * kNeigh * cap, sizeof(int) * kNeigh * keep, s)) ||
      (rc = grow(h->dNeighSeq, sizeof(unsigned) * kNeigh * cap, sizeof(unsigned) * kNeigh * keep, s)) ||
      (rc = grow(h->dRelocScore, sizeof(float) * cap, sizeof(float) * keep, s)) || (rc = grow(h->dRelocSeq, sizeof(unsigned) * cap, sizeof(unsigned) * keep, s)))
    return rc;
  h->slotCap = cap;
  return YDORB_OK;
}

// makes room for `extra` more words: a new pool of twice the need, the live rows moved to its front
int growPool(ydorb_kfdb* h, long long extra) {
  if (h->poolUsed + extra <= h->poolCap) return YDORB_OK;
  const long long cap = std::max<long long>(2 * (h->poolLiveWords + extra), 1024);
  hipStream_t s = h->stream;
  const int H = h->nSlots();
  ScopedMem nw, nv;   // freed on every early return; handed over to dWord / dVal at the end
  if (nw.alloc(sizeof(int) * cap) != YDORB_OK || nv.alloc(sizeof(double) * cap) != YDORB_OK) {
    set_error("hipMalloc of a pool of %lld words failed", cap);
    return YDORB_ERR_HIP;
  }
  std::vector<long long> newOff(std::max(H, 1), 0);
  long long used = 0;
  for (int i = 0; i < H; i++) if (h->live[i]) { newOff[i] = used; used += h->len[i]; }
  int rc = YDORB_OK;
  if (H > 0 && used > 0) {
    // the device's table may lag behind the host's: bring it up to date first (old offsets), then move
    if ((rc = h->dTmp.ensure(sizeof(long long) * H))) return rc;
    if (hipMemcpyAsync(h->dOff.p, h->off.data(), sizeof(long long) * H, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(h->dLen.p, h->len.data(), sizeof(int) * H, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(h->dLive.p, h->live.data(), sizeof(int) * H, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(h->dTmp.p, newOff.data(), sizeof(long long) * H, hipMemcpyHostToDevice, s) != hipSuccess) {
      set_error("uploading the slot table failed");
      return YDORB_ERR_HIP;
    }
    hipLaunchKernelGGL(k_kfdb_compact, dim3(H), dim3(256), 0, s, h->dWord.as<int>(), h->dVal.as<double>(), h->dOff.as<long long>(),
                       h->dTmp.as<long long>(), h->dLen.as<int>(), h->dLive.as<int>(), nw.as<int>(), nv.as<double>());
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
      set_error("moving the rows to a larger pool failed");
      return YDORB_ERR_HIP;
    }
  }
  h->dWord.take(nw); h->dVal.take(nv);
  for (int i = 0; i < H; i++) if (h->live[i]) h->off[i] = newOff[i];
  h->poolUsed = used; h->poolCap = cap;
  if (H > 0) { h->dirtyLo = 0; h->dirtyHi = H; }
  return YDORB_OK;
}

int syncTable(ydorb_kfdb* h) {
  const int lo = h->dirtyLo, n = h->dirtyHi - h->dirtyLo;
  if (n <= 0) return YDORB_OK;
  hipStream_t s = h->stream;
  HIPCHK(hipMemcpyAsync(h->dOff.as<long long>() + lo, h->off.data() + lo, sizeof(long long) * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dLen.as<int>() + lo, h->len.data() + lo, sizeof(int) * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dLive.as<int>() + lo, h->live.data() + lo, sizeof(int) * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dSeq.as<unsigned>() + lo, h->seq.data() + lo, sizeof(unsigned) * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dNeigh.as<int>() + (size_t)lo * kNeigh, h->neigh.data() + (size_t)lo * kNeigh, sizeof(int) * kNeigh * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dNeighSeq.as<unsigned>() + (size_t)lo * kNeigh, h->neighSeq.data() + (size_t)lo * kNeigh, sizeof(unsigned) * kNeigh * n,
                        hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));   // the host vectors may change after the return
  h->dirtyLo = h->dirtyHi = 0;
  return YDORB_OK;
}

int checkCsr(const int32_t* start, const int32_t* word, const double* value, int n, const char* what, int maxLen) {
  if (!start || start[0] != 0) { set_error("%s: start must begin with 0", what); return YDORB_ERR_INVALID_ARG; }
  for (int i = 0; i < n; i++) {
    const int a = start[i], b = start[i + 1];
    if (b < a) { set_error("%s %d: start is not ascending", what, i); return YDORB_ERR_INVALID_ARG; }
    if (b > a && (!word || !value)) { set_error("%s %d: null word or value array", what, i); return YDORB_ERR_INVALID_ARG; }
    if (maxLen > 0 && b - a > maxLen) { set_error("%s %d: %d words, at most %d are supported", what, i, b - a, maxLen); return YDORB_ERR_UNSUPPORTED; }
    for (int k = a; k < b; k++)
      if (word[k] < 0 || (k > a && word[k] <= word[k - 1])) {   // a BowVector is a std::map: ids ascending and unique
        set_error("%s %d: word ids must be ascending, unique and >= 0", what, i);
        return YDORB_ERR_INVALID_ARG;
      }
  }
  return YDORB_OK;
}

// Shared body of the two detect calls.
int detect(ydorb_kfdb* h, int form, const int32_t* qStart, const int32_t* qWord, const double* qVal, int Q, const int32_t* connStart,
           const int32_t* connSlots, const float* minScore, int32_t* cand, int candCap, int32_t* counts, int32_t* status, int32_t* diagWords,
           float* diagScore) {
  if (!h || Q < 0 || candCap < 0 || (Q > 0 && (!counts || (candCap > 0 && !cand))) || (!diagWords != !diagScore)) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  if (Q == 0) return YDORB_OK;
  int rc = checkCsr(qStart, qWord, qVal, Q, "query", kMaxQueryWords);
  if (rc) return rc;
  if (form == kLoop) {
    if (!connStart || !minScore || connStart[0] != 0) { set_error("loop form: connected lists and minScore are required"); return YDORB_ERR_INVALID_ARG; }
    for (int q = 0; q < Q; q++)
      if (connStart[q + 1] < connStart[q] || (connStart[q + 1] > 0 && !connSlots)) { set_error("query %d: bad connected list", q); return YDORB_ERR_INVALID_ARG; }
  }
  std::lock_guard<std::mutex> lock(h->mu);
  HIPCHK(hipSetDevice(h->device));
  const int H = h->nSlots();
  for (int q = 0; q < Q; q++) { counts[q] = 0; if (status) status[q] = 0; }
  if (H == 0) return YDORB_OK;   // an empty database: every list is empty
  if (form == kLoop)
    for (int k = 0; k < connStart[Q]; k++)
      if (connSlots[k] < 0 || connSlots[k] >= H) { set_error("connected slot %d out of range", connSlots[k]); return YDORB_ERR_INVALID_ARG; }
  if ((rc = syncTable(h))) return rc;
  hipStream_t s = h->stream;
  int n2 = 1;
  while (n2 < H) n2 <<= 1;
  for (int c0 = 0; c0 < Q; c0 += kQueryChunk) {
    const int Qc = std::min(kQueryChunk, Q - c0), sets = form == kLoop ? Qc : 1;
    const int w0 = qStart[c0], nW = qStart[c0 + Qc] - w0;
    const int k0 = form == kLoop ? connStart[c0] : 0, nK = form == kLoop ? connStart[c0 + Qc] - k0 : 0;
    const bool last = c0 + Qc == Q;
    const int cw = std::min(candCap, H);   // a query returns at most H candidates
    Layout U;
    const size_t uStart = U.add(sizeof(int) * (Qc + 1)), uWord = U.add(sizeof(int) * nW), uVal = U.add(sizeof(double) * nW),
                 uCs = U.add(sizeof(int) * (Qc + 1)), uCk = U.add(sizeof(int) * nK), uMs = U.add(sizeof(float) * Qc);
    Layout W;
    const size_t QH = (size_t)Qc * H, SH = (size_t)sets * H;
    const size_t wCommon = W.add(sizeof(int) * QH), wFirst = W.add(sizeof(int) * QH), wScore = W.add(sizeof(double) * QH), wConn = W.add(SH),
                 wAcc = W.add(sizeof(float) * SH), wBest = W.add(sizeof(int) * SH), wKey = W.add(sizeof(unsigned long long) * SH),
                 wSk = W.add(sizeof(unsigned long long) * sets * n2), wSv = W.add(sizeof(int) * (size_t)sets * n2);
    Layout D;
    const size_t dCounts = D.add(sizeof(int) * Qc), dStatus = D.add(sizeof(int) * Qc), dCand = D.add(sizeof(int) * (size_t)Qc * std::max(cw, 1)),
                 dDw = D.add(sizeof(int) * H), dDs = D.add(sizeof(float) * H);
    if ((rc = h->up.ensure(U.bytes)) || (rc = h->work.ensure(W.bytes)) || (rc = h->down.ensure(D.bytes))) return rc;
    std::vector<int> st(Qc + 1), cs(Qc + 1, 0);
    for (int q = 0; q <= Qc; q++) { st[q] = qStart[c0 + q] - w0; if (form == kLoop) cs[q] = connStart[c0 + q] - k0; }
    HIPCHK(hipMemcpyAsync(at<int>(h->up, uStart), st.data(), sizeof(int) * (Qc + 1), hipMemcpyHostToDevice, s));
    if (nW) {
      HIPCHK(hipMemcpyAsync(at<int>(h->up, uWord), qWord + w0, sizeof(int) * nW, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(at<double>(h->up, uVal), qVal + w0, sizeof(double) * nW, hipMemcpyHostToDevice, s));
    }
    if (form == kLoop) {
      HIPCHK(hipMemcpyAsync(at<int>(h->up, uCs), cs.data(), sizeof(int) * (Qc + 1), hipMemcpyHostToDevice, s));
      if (nK) HIPCHK(hipMemcpyAsync(at<int>(h->up, uCk), connSlots + k0, sizeof(int) * nK, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(at<float>(h->up, uMs), minScore + c0, sizeof(float) * Qc, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemsetAsync(at<int>(h->down, dStatus), 0, sizeof(int) * Qc, s));
    const DbView V = h->view();
    QueryView Qv{at<int>(h->up, uStart), at<int>(h->up, uWord), at<double>(h->up, uVal)};
    hipLaunchKernelGGL(k_kfdb_intersect, dim3((H + kSlotsPerBlock - 1) / kSlotsPerBlock, Qc), dim3(256), 0, s, V, Qv, (const int*)nullptr, H, h->scoring,
                       at<int>(h->work, wCommon), at<int>(h->work, wFirst), at<double>(h->work, wScore));
    HIPCHK(hipGetLastError());
    SelectArgs A;
    A.D = V; A.form = form; A.nQueries = Qc; A.candCap = cw;
    A.common = at<int>(h->work, wCommon); A.first = at<int>(h->work, wFirst); A.score = at<double>(h->work, wScore);
    A.connStart = at<int>(h->up, uCs); A.connSlots = at<int>(h->up, uCk); A.minScore = at<float>(h->up, uMs);
    A.conn = at<uint8_t>(h->work, wConn); A.acc = at<float>(h->work, wAcc); A.bestKF = at<int>(h->work, wBest);
    A.firstKey = at<unsigned long long>(h->work, wKey); A.sortKey = at<unsigned long long>(h->work, wSk); A.sortVal = at<int>(h->work, wSv);
    A.n2 = n2;
    A.cand = at<int>(h->down, dCand); A.counts = at<int>(h->down, dCounts); A.status = at<int>(h->down, dStatus);
    const bool diag = last && diagWords;
    A.diagWords = diag ? at<int>(h->down, dDw) : nullptr; A.diagScore = diag ? at<float>(h->down, dDs) : nullptr;
    hipLaunchKernelGGL(k_kfdb_select, dim3(sets), dim3(kSelectThreads), 0, s, A);
    HIPCHK(hipGetLastError());
    // every phase has run; what follows only fetches the result
    HIPCHK(hipMemcpyAsync(counts + c0, A.counts, sizeof(int) * Qc, hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(hipMemcpyAsync(status + c0, A.status, sizeof(int) * Qc, hipMemcpyDeviceToHost, s));
    if (diag) {
      HIPCHK(hipMemcpyAsync(diagWords, A.diagWords, sizeof(int) * H, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(diagScore, A.diagScore, sizeof(float) * H, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    int widest = 0;
    for (int q = 0; q < Qc; q++) widest = std::max(widest, std::min(counts[c0 + q], cw));
    if (widest > 0) {
      HIPCHK(hipMemcpy2DAsync(cand + (size_t)c0 * candCap, sizeof(int) * candCap, A.cand, sizeof(int) * cw, sizeof(int) * widest, Qc,
                              hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
    }
  }
  return YDORB_OK;
}

}  // namespace

extern "C" {

int ydorb_kfdb_create(int32_t device, int32_t scoring, int32_t slot_capacity, int64_t word_capacity, ydorb_kfdb_t** out) {
  if (!out || slot_capacity < 0 || word_capacity < 0 || scoring < 0 || scoring > kDot) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  if (scoring == kKL || scoring == kBhattacharyya) {
    // both take log() of the values; the host's libm and the device's do not round alike, so the result could not be pinned bit for bit
    set_error("unsupported scoring: KL and Bhattacharyya need log(), which is not bit-reproducible between host libm and the device");
    return YDORB_ERR_UNSUPPORTED;
  }
  int rc = require_device(device);
  if (rc) return rc;
  ydorb_kfdb* h = new ydorb_kfdb;
  h->device = device; h->scoring = scoring;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    set_error("hipStreamCreate failed");
    delete h;
    return YDORB_ERR_HIP;
  }
  if ((rc = growSlots(h, std::max(slot_capacity, 1))) || (rc = growPool(h, std::max<long long>(word_capacity, 1)))) { ydorb_kfdb_destroy(h); return rc; }
  *out = h;
  return YDORB_OK;
}

void ydorb_kfdb_destroy(ydorb_kfdb_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  for (Mem* m : {&h->dWord, &h->dVal, &h->dOff, &h->dLen, &h->dLive, &h->dSeq, &h->dNeigh, &h->dNeighSeq, &h->dRelocScore, &h->dRelocSeq, &h->dTmp,
                 &h->up, &h->work, &h->down})
    m->release();
  delete h;
}

int ydorb_kfdb_add(ydorb_kfdb_t* h, const int32_t* start, const int32_t* word, const double* value, int32_t n, int32_t* slots) {
  if (!h || n < 0 || (n > 0 && !slots)) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  if (n == 0) return YDORB_OK;
  int rc = checkCsr(start, word, value, n, "key frame", 0);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPCHK(hipSetDevice(h->device));
  const long long total = start[n];
  const int fresh = std::max(0, n - (int)h->freeSlots.size());
  if ((rc = growSlots(h, h->nSlots() + fresh)) || (rc = growPool(h, total))) return rc;
  hipStream_t s = h->stream;
  if (total) {
    HIPCHK(hipMemcpyAsync(h->dWord.as<int>() + h->poolUsed, word, sizeof(int) * total, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->dVal.as<double>() + h->poolUsed, value, sizeof(double) * total, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  for (int i = 0; i < n; i++) {
    int slot;
    if (!h->freeSlots.empty()) { slot = h->freeSlots.back(); h->freeSlots.pop_back(); }
    else {
      slot = h->nSlots();
      h->off.push_back(0); h->len.push_back(0); h->live.push_back(0); h->seq.push_back(0);
      h->neigh.resize(h->neigh.size() + kNeigh, -1); h->neighSeq.resize(h->neighSeq.size() + kNeigh, 0);
    }
    h->off[slot] = h->poolUsed + start[i];
    h->len[slot] = start[i + 1] - start[i];
    h->live[slot] = 1;
    h->seq[slot] = h->nextSeq++;   // a new key frame: its mRelocScore counts as never written (relocSeq differs)
    for (int k = 0; k < kNeigh; k++) { h->neigh[(size_t)slot * kNeigh + k] = -1; h->neighSeq[(size_t)slot * kNeigh + k] = 0; }
    h->touch(slot);
    slots[i] = slot;
  }
  h->poolUsed += total; h->poolLiveWords += total; h->nLive += n;
  return YDORB_OK;
}

int ydorb_kfdb_erase(ydorb_kfdb_t* h, const int32_t* slots, int32_t n) {
  if (!h || n < 0 || (n > 0 && !slots)) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lock(h->mu);
  for (int i = 0; i < n; i++) {
    if (slots[i] < 0 || slots[i] >= h->nSlots() || !h->live[slots[i]]) { set_error("erase: slot %d is not in the database", slots[i]); return YDORB_ERR_INVALID_ARG; }
    for (int j = 0; j < i; j++) if (slots[j] == slots[i]) { set_error("erase: slot %d given twice", slots[i]); return YDORB_ERR_INVALID_ARG; }
  }
  for (int i = 0; i < n; i++) {
    const int slot = slots[i];
    h->live[slot] = 0;
    h->poolLiveWords -= h->len[slot];
    h->freeSlots.push_back(slot);
    h->touch(slot);
  }
  h->nLive -= n;
  return YDORB_OK;
}

int ydorb_kfdb_clear(ydorb_kfdb_t* h) {
  if (!h) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lock(h->mu);
  h->off.clear(); h->len.clear(); h->live.clear(); h->seq.clear(); h->neigh.clear(); h->neighSeq.clear(); h->freeSlots.clear();
  h->nLive = 0; h->poolUsed = 0; h->poolLiveWords = 0; h->dirtyLo = h->dirtyHi = 0;
  return YDORB_OK;
}

int ydorb_kfdb_size(ydorb_kfdb_t* h, int32_t* n_live, int32_t* n_slots) {
  if (!h) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lock(h->mu);
  if (n_live) *n_live = h->nLive;
  if (n_slots) *n_slots = h->nSlots();
  return YDORB_OK;
}

int ydorb_kfdb_set_covisibility(ydorb_kfdb_t* h, const int32_t* slots, const int32_t* neigh, int32_t n) {
  if (!h || n < 0 || (n > 0 && (!slots || !neigh))) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lock(h->mu);
  const int H = h->nSlots();
  for (int i = 0; i < n; i++) {
    if (slots[i] < 0 || slots[i] >= H || !h->live[slots[i]]) { set_error("set_covisibility: slot %d is not in the database", slots[i]); return YDORB_ERR_INVALID_ARG; }
    for (int k = 0; k < kNeigh; k++) {
      const int nb = neigh[(size_t)i * kNeigh + k];
      if (nb < -1 || nb >= H) { set_error("set_covisibility: neighbour slot %d out of range", nb); return YDORB_ERR_INVALID_ARG; }
    }
  }
  for (int i = 0; i < n; i++) {
    const int slot = slots[i];
    for (int k = 0; k < kNeigh; k++) {
      const int nb = neigh[(size_t)i * kNeigh + k];
      const bool ok = nb >= 0 && h->live[nb];   // a key frame that left the database (setBadFlag) is in nobody's covisibility list
      h->neigh[(size_t)slot * kNeigh + k] = ok ? nb : -1;
      h->neighSeq[(size_t)slot * kNeigh + k] = ok ? h->seq[nb] : 0;
    }
    h->touch(slot);
  }
  return YDORB_OK;
}

int ydorb_kfdb_score(ydorb_kfdb_t* h, const int32_t* q_word, const double* q_value, int32_t n_words, const int32_t* slots, int32_t n, double* scores) {
  if (!h || n_words < 0 || n < 0 || (n > 0 && (!slots || !scores))) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  if (n == 0) return YDORB_OK;
  const int32_t st[2] = {0, n_words};
  int rc = checkCsr(st, q_word, q_value, 1, "query", kMaxQueryWords);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(h->mu);
  HIPCHK(hipSetDevice(h->device));
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= h->nSlots() || !h->live[slots[i]]) { set_error("score: slot %d is not in the database", slots[i]); return YDORB_ERR_INVALID_ARG; }
  if ((rc = syncTable(h))) return rc;
  Layout U;
  const size_t uStart = U.add(sizeof(int) * 2), uWord = U.add(sizeof(int) * n_words), uVal = U.add(sizeof(double) * n_words), uSlots = U.add(sizeof(int) * n);
  Layout W;
  const size_t wCommon = W.add(sizeof(int) * n), wFirst = W.add(sizeof(int) * n), wScore = W.add(sizeof(double) * n);
  if ((rc = h->up.ensure(U.bytes)) || (rc = h->work.ensure(W.bytes))) return rc;
  hipStream_t s = h->stream;
  HIPCHK(hipMemcpyAsync(at<int>(h->up, uStart), st, sizeof st, hipMemcpyHostToDevice, s));
  if (n_words) {
    HIPCHK(hipMemcpyAsync(at<int>(h->up, uWord), q_word, sizeof(int) * n_words, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(at<double>(h->up, uVal), q_value, sizeof(double) * n_words, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemcpyAsync(at<int>(h->up, uSlots), slots, sizeof(int) * n, hipMemcpyHostToDevice, s));
  QueryView Qv{at<int>(h->up, uStart), at<int>(h->up, uWord), at<double>(h->up, uVal)};
  hipLaunchKernelGGL(k_kfdb_intersect, dim3((n + kSlotsPerBlock - 1) / kSlotsPerBlock, 1), dim3(256), 0, s, h->view(), Qv, at<const int>(h->up, uSlots), n,
                     h->scoring, at<int>(h->work, wCommon), at<int>(h->work, wFirst), at<double>(h->work, wScore));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(scores, at<double>(h->work, wScore), sizeof(double) * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return YDORB_OK;
}

int ydorb_kfdb_detect_reloc(ydorb_kfdb_t* h, const int32_t* q_start, const int32_t* q_word, const double* q_value, int32_t n_queries, int32_t* cand,
                            int32_t cand_cap, int32_t* counts, int32_t* status, int32_t* diag_words, float* diag_score) {
  return detect(h, kReloc, q_start, q_word, q_value, n_queries, nullptr, nullptr, nullptr, cand, cand_cap, counts, status, diag_words, diag_score);
}

int ydorb_kfdb_detect_loop(ydorb_kfdb_t* h, const int32_t* q_start, const int32_t* q_word, const double* q_value, int32_t n_queries,
                           const int32_t* conn_start, const int32_t* conn_slots, const float* min_score, int32_t* cand, int32_t cand_cap,
                           int32_t* counts, int32_t* status, int32_t* diag_words, float* diag_score) {
  return detect(h, kLoop, q_start, q_word, q_value, n_queries, conn_start, conn_slots, min_score, cand, cand_cap, counts, status, diag_words, diag_score);
}

}  // extern "C"
