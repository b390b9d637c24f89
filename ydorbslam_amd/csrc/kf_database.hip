// Key-frame database on the MI355X + its C ABI (include/ydorb/c_api.h, "KeyFrameDatabase"): ydorb_kfdb_*.  Replaces
// KeyFrameDatabase::add / erase / clear / detectLoopCandidates / detectRelocalizationCandidates (ORB-SLAM2 src/KeyFrameDatabase.cc) and
// the DBoW3::Vocabulary::score calls in them and in LoopClosing::detectLoop.  The BowVectors live in HBM as rows of a pool
// (word ids ascending + double values, 12 bytes per word); the host keeps the slot table (offsets, live flags, add sequence numbers,
// neighbour lists) and uploads what changed before a query.  A query runs the kernels of kfdb_kernels.hip.h back to back and reads
// back the candidates at the end.
//
// Device memory ("Memory"): two arenas that live as long as the database, the slot table (layTable) and the
// pool (layPool), and the three per-call areas of a StagedCtx: what a call uploads (layQuery, packed in pinned memory and sent in one
// copy), its scratch (layWork) and its results (layResults, the head of which comes back in one copy).
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

constexpr int kQueryChunk = 64;   // queries per kernel sequence: bounds the scratch (about 60 bytes per query and slot)

// The slot table on the device, [cap] each.  The host writes the first six from its mirror (syncTable); the last two are
// k_kfdb_select's alone.
struct Table { long long* off; int* len; int* live; unsigned* seq; int* neigh; unsigned* neighSeq; float* relocScore; unsigned* relocSeq; };

Table layTable(Carve& a, size_t cap) {
  Table t;
  a.take(t.off, cap); a.take(t.len, cap); a.take(t.live, cap); a.take(t.seq, cap); a.take(t.neigh, kNeigh * cap); a.take(t.neighSeq, kNeigh * cap);
  a.take(t.relocScore, cap); a.take(t.relocSeq, cap);
  return t;
}

struct Pool { int* word; double* val; };

Pool layPool(Carve& a, size_t cap) { Pool p; a.take(p.word, cap); a.take(p.val, cap); return p; }

// What a call uploads: Q queries as a CSR whose `start` begins at 0; for the loop form their connected lists (a CSR again) and
// minScore; for ydorb_kfdb_score the slots to score.
struct QueryUp { int* start; int* word; double* val; int* connStart; int* connSlots; float* minScore; int* list; };

QueryUp layQuery(Carve& a, size_t Q, size_t nWords, size_t nConn, size_t nList) {
  QueryUp u;
  a.take(u.start, Q + 1); a.take(u.word, nWords); a.take(u.val, nWords);
  a.take(u.connStart, Q + 1); a.take(u.connSlots, nConn); a.take(u.minScore, Q); a.take(u.list, nList);
  return u;
}

// Scratch of a call: k_kfdb_intersect's output per item, then k_kfdb_select's sets (kfdb_kernels.hip.h, SelectArgs).
struct Work { int* common; int* first; double* score; uint8_t* conn; float* acc; int* bestKF; unsigned long long *firstKey, *sortKey; int* sortVal; };

Work layWork(Carve& a, size_t items, size_t sets, size_t H, size_t n2) {
  Work w;
  a.take(w.common, items); a.take(w.first, items); a.take(w.score, items);
  a.take(w.conn, sets * H); a.take(w.acc, sets * H); a.take(w.bestKF, sets * H); a.take(w.firstKey, sets * H);
  a.take(w.sortKey, sets * n2); a.take(w.sortVal, sets * n2);
  return w;
}

// Results of a chunk.  Everything before `cand` comes back in one copy of `head` bytes; the candidate rows follow in a second one,
// once the counts say how wide it has to be.
struct Results { int* counts; int* status; int* diagWords; float* diagScore; int* cand; size_t head; };

Results layResults(Carve& a, size_t Q, size_t nDiag, size_t nCand) {
  Results r;
  a.take(r.counts, Q); a.take(r.status, Q); a.take(r.diagWords, nDiag); a.take(r.diagScore, nDiag);
  r.head = a.L.bytes;
  a.take(r.cand, nCand);
  return r;
}

}  // namespace

struct ydorb_kfdb {
  int device = 0, scoring = 0;
  // c.mu: tracking (relocalisation), local mapping (add / erase) and loop closing reach one database.  c.scratch is the work area.
  StagedCtx c;
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
  Mem table, pool;   // arenas: T and P point into them
  Table T{};
  Pool P{};
  int slotCap = 0;
  int nSlots() const { return (int)off.size(); }
  DbView view() const { return DbView{P.word, P.val, T.off, T.len, T.live, T.seq, T.neigh, T.neighSeq, T.relocScore, T.relocSeq, nSlots()}; }
  void touch(int s) {
    if (dirtyHi <= dirtyLo) { dirtyLo = s; dirtyHi = s + 1; }
    else { dirtyLo = std::min(dirtyLo, s); dirtyHi = std::max(dirtyHi, s + 1); }
  }
};

namespace {

// Makes room for `want` slots: a new table of twice the need, at least 64, all zero but for the two arrays that only the device
// holds.  The six mirrored arrays are not copied: the whole table turns dirty and the next syncTable uploads them.
int growSlots(ydorb_kfdb* h, int want) {
  if (want <= h->slotCap) return YDORB_OK;
  const int cap = std::max(want * 2, 64);
  hipStream_t s = h->c.stream;
  Carve size(nullptr);
  layTable(size, cap);
  ScopedMem n;
  int rc = n.alloc(size.L.bytes);
  if (rc) return rc;
  Carve a(n.p);
  const Table t = layTable(a, cap);
  HIPCHK(hipMemsetAsync(n.p, 0, n.cap, s));
  if (h->slotCap) {
    HIPCHK(hipMemcpyAsync(t.relocScore, h->T.relocScore, sizeof(float) * h->slotCap, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(t.relocSeq, h->T.relocSeq, sizeof(unsigned) * h->slotCap, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  h->table.take(n);
  h->T = t; h->slotCap = cap;
  h->dirtyLo = 0; h->dirtyHi = h->nSlots();
  return YDORB_OK;
}

int syncTable(ydorb_kfdb* h) {
  const int lo = h->dirtyLo, n = h->dirtyHi - h->dirtyLo;
  if (n <= 0) return YDORB_OK;
  hipStream_t s = h->c.stream;
  const Table& T = h->T;
  HIPCHK(hipMemcpyAsync(T.off + lo, h->off.data() + lo, sizeof(long long) * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(T.len + lo, h->len.data() + lo, sizeof(int) * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(T.live + lo, h->live.data() + lo, sizeof(int) * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(T.seq + lo, h->seq.data() + lo, sizeof(unsigned) * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(T.neigh + (size_t)lo * kNeigh, h->neigh.data() + (size_t)lo * kNeigh, sizeof(int) * kNeigh * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(T.neighSeq + (size_t)lo * kNeigh, h->neighSeq.data() + (size_t)lo * kNeigh, sizeof(unsigned) * kNeigh * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));   // the host vectors may change after the return
  h->dirtyLo = h->dirtyHi = 0;
  return YDORB_OK;
}

// makes room for `extra` more words: a new pool of twice the need, the live rows moved to its front
int growPool(ydorb_kfdb* h, long long extra) {
  if (h->poolUsed + extra <= h->poolCap) return YDORB_OK;
  const long long cap = std::max<long long>(2 * (h->poolLiveWords + extra), 1024);
  StagedCtx& c = h->c;
  const int H = h->nSlots();
  Carve size(nullptr);
  layPool(size, cap);
  ScopedMem n;   // freed on every early return; handed over to the handle at the end
  int rc = n.alloc(size.L.bytes);
  if (rc) return rc;
  Carve a(n.p);
  const Pool p = layPool(a, cap);
  if (h->poolLiveWords > 0) {
    // the device's table may lag behind the host's: bring it up to date first (old offsets), then move
    if ((rc = syncTable(h)) || (rc = c.hUp.ensure(sizeof(long long) * H)) || (rc = c.up.ensure(sizeof(long long) * H))) return rc;
    long long* newOff = c.hUp.as<long long>();
    long long at = 0;
    for (int i = 0; i < H; i++) { newOff[i] = at; if (h->live[i]) at += h->len[i]; }
    HIPCHK(hipMemcpyAsync(c.up.p, newOff, sizeof(long long) * H, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(k_kfdb_compact, dim3(H), dim3(256), 0, c.stream, h->P.word, h->P.val, h->T.off, c.up.as<long long>(), h->T.len, h->T.live, p.word,
                       p.val);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c.stream));
  }
  h->pool.take(n);
  h->P = p;
  long long used = 0;
  for (int i = 0; i < H; i++) if (h->live[i]) { h->off[i] = used; used += h->len[i]; }
  h->poolUsed = used; h->poolCap = cap;
  if (H > 0) { h->dirtyLo = 0; h->dirtyHi = H; }
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

// Queries [c0, c0 + Q) of the caller's CSR with the loop form's connected lists and minScore (connStart given) and
// ydorb_kfdb_score's slot list (nList > 0): laid out by layQuery, packed into hUp with both `start` arrays rebased to 0 and uploaded
// in one copy.  *dev gets the arrays on the device.  hUp is free again once the stream has been synchronised, which every call does.
int stageQuery(StagedCtx& c, const int32_t* start, const int32_t* word, const double* val, int c0, int Q, const int32_t* connStart,
               const int32_t* connSlots, const float* minScore, const int32_t* list, int nList, QueryUp* dev) {
  const int w0 = start[c0], nW = start[c0 + Q] - w0;
  const int k0 = connStart ? connStart[c0] : 0, nK = connStart ? connStart[c0 + Q] - k0 : 0;
  Carve size(nullptr);
  layQuery(size, Q, nW, nK, nList);
  int rc;
  if ((rc = c.hUp.ensure(size.L.bytes)) || (rc = c.up.ensure(size.L.bytes))) return rc;
  Carve host(c.hUp.p), device(c.up.p);
  const QueryUp u = layQuery(host, Q, nW, nK, nList);
  *dev = layQuery(device, Q, nW, nK, nList);
  for (int q = 0; q <= Q; q++) u.start[q] = start[c0 + q] - w0;
  if (nW) { std::memcpy(u.word, word + w0, sizeof(int) * nW); std::memcpy(u.val, val + w0, sizeof(double) * nW); }
  if (connStart) {
    for (int q = 0; q <= Q; q++) u.connStart[q] = connStart[c0 + q] - k0;
    if (nK) std::memcpy(u.connSlots, connSlots + k0, sizeof(int) * nK);
    std::memcpy(u.minScore, minScore + c0, sizeof(float) * Q);
  }
  if (nList) std::memcpy(u.list, list, sizeof(int) * nList);
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, size.L.bytes, hipMemcpyHostToDevice, c.stream));
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
  StagedCtx& c = h->c;
  std::lock_guard<std::mutex> lock(c.mu);
  HIPCHK(hipSetDevice(h->device));
  const int H = h->nSlots();
  for (int q = 0; q < Q; q++) { counts[q] = 0; if (status) status[q] = 0; }
  if (H == 0) return YDORB_OK;   // an empty database: every list is empty
  if (form == kLoop)
    for (int k = 0; k < connStart[Q]; k++)
      if (connSlots[k] < 0 || connSlots[k] >= H) { set_error("connected slot %d out of range", connSlots[k]); return YDORB_ERR_INVALID_ARG; }
  if ((rc = syncTable(h))) return rc;
  hipStream_t s = c.stream;
  int n2 = 1;
  while (n2 < H) n2 <<= 1;
  const int cw = std::min(candCap, H);   // a query returns at most H candidates
  for (int c0 = 0; c0 < Q; c0 += kQueryChunk) {
    const int Qc = std::min(kQueryChunk, Q - c0), sets = form == kLoop ? Qc : 1;
    const bool diag = c0 + Qc == Q && diagWords;
    const size_t nDiag = diag ? H : 0, nCand = (size_t)Qc * std::max(cw, 1);
    Carve workSize(nullptr), downSize(nullptr);
    layWork(workSize, (size_t)Qc * H, sets, H, n2);
    const size_t head = layResults(downSize, Qc, nDiag, nCand).head;
    if ((rc = c.scratch.ensure(workSize.L.bytes)) || (rc = c.down.ensure(downSize.L.bytes)) || (rc = c.hDown.ensure(head))) return rc;
    Carve work(c.scratch.p), down(c.down.p), hDown(c.hDown.p);
    const Work w = layWork(work, (size_t)Qc * H, sets, H, n2);
    const Results r = layResults(down, Qc, nDiag, nCand), hr = layResults(hDown, Qc, nDiag, 0);
    QueryUp u;
    if ((rc = stageQuery(c, qStart, qWord, qVal, c0, Qc, form == kLoop ? connStart : nullptr, connSlots, minScore, nullptr, 0, &u))) return rc;
    HIPCHK(hipMemsetAsync(r.status, 0, sizeof(int) * Qc, s));
    const DbView V = h->view();
    hipLaunchKernelGGL(k_kfdb_intersect, dim3((H + kSlotsPerBlock - 1) / kSlotsPerBlock, Qc), dim3(256), 0, s, V, QueryView{u.start, u.word, u.val},
                       (const int*)nullptr, H, h->scoring, w.common, w.first, w.score);
    HIPCHK(hipGetLastError());
    SelectArgs A;
    A.D = V; A.form = form; A.nQueries = Qc; A.candCap = cw;
    A.common = w.common; A.first = w.first; A.score = w.score;
    A.connStart = u.connStart; A.connSlots = u.connSlots; A.minScore = u.minScore;
    A.conn = w.conn; A.acc = w.acc; A.bestKF = w.bestKF; A.firstKey = w.firstKey; A.sortKey = w.sortKey; A.sortVal = w.sortVal;
    A.n2 = n2;
    A.cand = r.cand; A.counts = r.counts; A.status = r.status;
    A.diagWords = diag ? r.diagWords : nullptr; A.diagScore = diag ? r.diagScore : nullptr;
    hipLaunchKernelGGL(k_kfdb_select, dim3(sets), dim3(kSelectThreads), 0, s, A);
    HIPCHK(hipGetLastError());
    // every phase has run; what follows only fetches the result
    HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, head, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(counts + c0, hr.counts, sizeof(int) * Qc);
    if (status) std::memcpy(status + c0, hr.status, sizeof(int) * Qc);
    if (diag) { std::memcpy(diagWords, hr.diagWords, sizeof(int) * H); std::memcpy(diagScore, hr.diagScore, sizeof(float) * H); }
    int widest = 0;
    for (int q = 0; q < Qc; q++) widest = std::max(widest, std::min(counts[c0 + q], cw));
    if (widest > 0) {
      HIPCHK(hipMemcpy2DAsync(cand + (size_t)c0 * candCap, sizeof(int) * candCap, r.cand, sizeof(int) * cw, sizeof(int) * widest, Qc,
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
  if ((rc = h->c.init(device)) || (rc = growSlots(h, std::max(slot_capacity, 1))) || (rc = growPool(h, std::max<long long>(word_capacity, 1)))) {
    ydorb_kfdb_destroy(h);   // whatever was built so far
    return rc;
  }
  *out = h;
  return YDORB_OK;
}

void ydorb_kfdb_destroy(ydorb_kfdb_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->c.stream) { (void)hipStreamSynchronize(h->c.stream); (void)hipStreamDestroy(h->c.stream); }
  h->c.releaseBuffers();
  h->table.release(); h->pool.release();
  delete h;
}

int ydorb_kfdb_add(ydorb_kfdb_t* h, const int32_t* start, const int32_t* word, const double* value, int32_t n, int32_t* slots) {
  if (!h || n < 0 || (n > 0 && !slots)) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  if (n == 0) return YDORB_OK;
  int rc = checkCsr(start, word, value, n, "key frame", 0);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(h->c.mu);
  HIPCHK(hipSetDevice(h->device));
  const long long total = start[n];
  const int fresh = std::max(0, n - (int)h->freeSlots.size());
  if ((rc = growSlots(h, h->nSlots() + fresh)) || (rc = growPool(h, total))) return rc;
  hipStream_t s = h->c.stream;
  if (total) {
    HIPCHK(hipMemcpyAsync(h->P.word + h->poolUsed, word, sizeof(int) * total, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->P.val + h->poolUsed, value, sizeof(double) * total, hipMemcpyHostToDevice, s));
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
  std::lock_guard<std::mutex> lock(h->c.mu);
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
  std::lock_guard<std::mutex> lock(h->c.mu);
  h->off.clear(); h->len.clear(); h->live.clear(); h->seq.clear(); h->neigh.clear(); h->neighSeq.clear(); h->freeSlots.clear();
  h->nLive = 0; h->poolUsed = 0; h->poolLiveWords = 0; h->dirtyLo = h->dirtyHi = 0;
  return YDORB_OK;
}

int ydorb_kfdb_size(ydorb_kfdb_t* h, int32_t* n_live, int32_t* n_slots) {
  if (!h) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (n_live) *n_live = h->nLive;
  if (n_slots) *n_slots = h->nSlots();
  return YDORB_OK;
}

int ydorb_kfdb_set_covisibility(ydorb_kfdb_t* h, const int32_t* slots, const int32_t* neigh, int32_t n) {
  if (!h || n < 0 || (n > 0 && (!slots || !neigh))) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lock(h->c.mu);
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
  StagedCtx& c = h->c;
  std::lock_guard<std::mutex> lock(c.mu);
  HIPCHK(hipSetDevice(h->device));
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= h->nSlots() || !h->live[slots[i]]) { set_error("score: slot %d is not in the database", slots[i]); return YDORB_ERR_INVALID_ARG; }
  if ((rc = syncTable(h))) return rc;
  Carve workSize(nullptr);
  layWork(workSize, n, 0, 0, 0);
  if ((rc = c.scratch.ensure(workSize.L.bytes)) || (rc = c.hDown.ensure(sizeof(double) * n))) return rc;
  Carve work(c.scratch.p);
  const Work w = layWork(work, n, 0, 0, 0);
  QueryUp u;
  if ((rc = stageQuery(c, st, q_word, q_value, 0, 1, nullptr, nullptr, nullptr, slots, n, &u))) return rc;
  hipStream_t s = c.stream;
  hipLaunchKernelGGL(k_kfdb_intersect, dim3((n + kSlotsPerBlock - 1) / kSlotsPerBlock, 1), dim3(256), 0, s, h->view(), QueryView{u.start, u.word, u.val},
                     (const int*)u.list, n, h->scoring, w.common, w.first, w.score);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, w.score, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(scores, c.hDown.p, sizeof(double) * n);
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
