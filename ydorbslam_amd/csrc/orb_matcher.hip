// Host side of the MI355X descriptor matcher + its C ABI (include/ydorb/c_api.h, "Descriptor matcher").
// Mirrors YDORBSLAM::OrbMatcher's search-by-projection / search-by-BoW entry points
// (reference src/orbMatcher.cpp:24-239, 303-462) on POD views; all searching runs in the HIP kernels of
// match_kernels.hip.h.  No CPU fallback: the only host arithmetic is the one-pair popcount that the
// reference exposes as a static helper (orbMatcher.cpp:11-23) and the vocabulary-node merge-join that
// decides which buckets meet (a walk over two sorted id lists, orbMatcher.cpp:317-361).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "frustum_kernels.hip.h"
#include "host_buffers.h"
#include "map_table.h"
#include "mapdb_bow_kernels.hip.h"
#include "mapdb_bowsearch_host.h"
#include "mapdb_frustum_kernels.hip.h"
#include "mapdb_fuse_kernels.hip.h"
#include "mapdb_resident_points.h"
#include "mapdb_tri_kernels.hip.h"
#include "match_kernels.hip.h"
#include "stereo_kernels.hip.h"
#include "ydorb_host.h"

using namespace ydorb;

namespace {

// k_grid_build keeps one 16-bit cell id per keypoint in dynamic LDS beside ~12 KiB of static tables: frames with more than
// ~26 k keypoints need the kernel's dynamic-LDS limit raised (the 16-bit index format allows up to 65 535).
int launchGridBuild(int nFrames, int cap, hipStream_t s, const FrameDev* frames) {
  const size_t dyn = sizeof(int16_t) * (size_t)std::max(cap, 0);
  if (dyn > 48 * 1024)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_grid_build), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  hipLaunchKernelGGL(k_grid_build, dim3(nFrames), dim3(256), dyn, s, frames, cap);
  HIPCHK(hipGetLastError());
  return YDORB_OK;
}

__global__ void k_hamming_rows(const uint8_t* a, const uint8_t* b, int n, int* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = hamming256(a + (size_t)i * 32, b + (size_t)i * 32);
}

enum { MS_GRID = 0, MS_GATHER, MS_RESOLVE, MS_COUNT };
const char* kMatchStageNames[MS_COUNT] = {"grid_build", "gather_distances", "resolve"};

// Device memory: one arena per path, laid out afresh by every call (Carve, host_buffers.h).
// k_resolve writes the taken flags back in whole 32-bit words of its LDS copy, up to 31 bytes past the last keypoint's
constexpr size_t kTakenPad = 31;

// Sizes a layout over a null base, grows the arena if need be and lays it out for real.
template <class Lay> int layOut(Mem& arena, Lay lay) {
  const int rc = arena.ensure(lay(nullptr));
  if (rc == YDORB_OK) lay(arena.p);
  return rc;
}

// `batch`: ydorb_match_pairs_device.  The descriptors come first: they are uploaded only when they change, and where they lie depends on
// the frame and call counts alone.  The record pool, by far the largest, comes last.
struct BatchPtrs {
  FrameDev* frames; CallDev* calls; float *sf, *ident;   // descriptors; ident = one identity affine per call
  QueryDev* queries; uint8_t* taken; int* matchQ; int2* qInfo; uint2* qPre; unsigned* heads;
  int *cellStart, *cellIdx; float4* sortedKp; uint8_t* sortedDesc;
  uint32_t* pool;
};
size_t layBatch(size_t cap, size_t nCalls, size_t nFrames, size_t poolPerCall, void* base, BatchPtrs& p) {
  Carve a(base);
  a.take(p.frames, nFrames); a.take(p.calls, nCalls); a.take(p.sf, 8); a.take(p.ident, 6 * nCalls);
  a.take(p.queries, cap * nCalls); a.take(p.taken, cap * nCalls + kTakenPad); a.take(p.matchQ, cap * nCalls); a.take(p.qInfo, cap * nCalls);
  a.take(p.qPre, cap * nCalls); a.take(p.heads, nCalls); a.take(p.cellStart, (kGridCells + 1) * nFrames); a.take(p.cellIdx, cap * nFrames);
  a.take(p.sortedKp, cap * nFrames); a.take(p.sortedDesc, 32 * cap * nFrames);
  a.take(p.pool, poolPerCall * nCalls);
  return a.L.bytes;
}

// `call`, projection family: a frame of n keypoints and its grid, nq queries.  status = [0] pool head (unsigned), [1] overflow status, [2] match
// count, cleared per attempt.  table / track (ydorb_search_local_points only): the map-point table as the pinned area holds it, track rows + status.
struct ProjPtrs {
  int* status; FrameDev* frame; CallDev* call;
  KeyPointDev* kps; uint8_t* desc; float* rightX; int *cellStart, *cellIdx; float4* sortedKp; uint8_t* sortedDesc;
  QueryDev* queries; uint8_t *qdesc, *taken; int *assigned, *matchQ; int2* qInfo; uint2* qPre;
  uint8_t *table, *track;
};
size_t layProjection(size_t n, bool stereo, size_t nq, size_t tableBytes, size_t trackBytes, void* base, ProjPtrs& p) {
  Carve a(base);
  a.take(p.status, 16); a.take(p.frame, 1); a.take(p.call, 1);
  a.take(p.kps, n); a.take(p.desc, 32 * n); a.take(p.rightX, stereo ? n : 0); a.take(p.cellStart, kGridCells + 1); a.take(p.cellIdx, n);
  a.take(p.sortedKp, n); a.take(p.sortedDesc, 32 * n);
  a.take(p.queries, nq); a.take(p.qdesc, 32 * nq); a.take(p.taken, n + kTakenPad); a.take(p.assigned, n); a.take(p.matchQ, nq); a.take(p.qInfo, nq);
  a.take(p.qPre, nq); a.take(p.table, tableBytes); a.take(p.track, trackBytes);
  return a.L.bytes;
}

// `call`, BoW family: nq (feature of A, bucket of B) queries; kpsA / goodA / goodB for searchForTriangulation only.  status as above.
struct BowPtrs {
  int* status; CallDev* call;
  uint8_t *descA, *descB, *valid, *goodA, *goodB; KeyPointDev *kpsA, *kpsB; int *feat, *qFeat, *assigned, *matchQ; int2 *qRange, *qInfo; float* qAngle;
};
size_t layBow(size_t nA, size_t nB, size_t nFeatB, size_t nq, bool tri, void* base, BowPtrs& p) {
  Carve a(base);
  a.take(p.status, 16); a.take(p.call, 1);
  a.take(p.descA, 32 * nA); a.take(p.descB, 32 * nB); a.take(p.kpsB, nB); a.take(p.feat, nFeatB); a.take(p.valid, nB);
  a.take(p.qFeat, nq); a.take(p.qRange, nq); a.take(p.qAngle, nq); a.take(p.qInfo, nq); a.take(p.matchQ, nq); a.take(p.assigned, std::max(nq, nB));
  a.take(p.kpsA, tri ? nA : 0); a.take(p.goodA, tri ? nA : 0); a.take(p.goodB, tri ? nB : 0);
  return a.L.bytes;
}

// `call`, descriptor rows (Hamming rows, distinctive descriptors, top-2): two descriptor sets, a CSR over them, one int or TopkOut per row
struct RowsPtrs { uint8_t *a, *b; int *offsets, *idx, *out; TopkOut* top; };
size_t layRows(size_t nA, size_t nB, size_t nOffsets, size_t nIdx, size_t nOut, size_t nTop, void* base, RowsPtrs& r) {
  Carve a(base);
  a.take(r.a, 32 * nA); a.take(r.b, 32 * nB); a.take(r.offsets, nOffsets); a.take(r.idx, nIdx); a.take(r.out, nOut); a.take(r.top, nTop);
  return a.L.bytes;
}

// `stereo`: counters and per-pair outputs first (the device-pointer form needs no more, so they lie where they lay whichever form the
// last call had); then, for the host-pointer form (nl / nr keypoint rows), what is uploaded and the results on their way down.
struct StereoPtrs { int *counters, *kept, *status, *nL, *nR; KeyPointDev *kpsL, *kpsR; uint8_t *descL, *descR; float *rightX, *depth; };
size_t layStereo(size_t nPairs, size_t nl, size_t nr, void* base, StereoPtrs& p) {
  Carve a(base);
  a.take(p.counters, 4 * nPairs); a.take(p.kept, nPairs); a.take(p.status, nPairs);
  a.take(p.kpsL, nl); a.take(p.descL, 32 * nl); a.take(p.kpsR, nr); a.take(p.descR, 32 * nr); a.take(p.nL, nl ? nPairs : 0); a.take(p.nR, nl ? nPairs : 0);
  a.take(p.rightX, nl); a.take(p.depth, nl);
  return a.L.bytes;
}

// `call`, ydorb_mapdb_fuse_search: nt targets over nf distinct target frames with sumN features in all, L list entries.  `up` is what one
// upload brings (targets, list starts, slots, skip bytes, frame and call records), `down` what one read-back takes (matches, status
// bytes, counts, pool heads, the overflow word).  The rows of all calls lie in list order; call t points at row list_start[t].
struct FusePtrs {
  uint8_t *up, *down;
  QueryDev* queries; uint8_t* qdesc; int2* qInfo; uint2* qPre;
  uint8_t* taken; int* assigned;
  int *cellStart, *cellIdx; float4* sortedKp; uint8_t* sortedDesc;
};
size_t layFuse(size_t upBytes, size_t downBytes, size_t nt, size_t nf, size_t sumN, size_t maxN, size_t L, void* base, FusePtrs& p) {
  Carve a(base);
  a.take(p.up, upBytes); a.take(p.down, downBytes);
  a.take(p.queries, L); a.take(p.qdesc, 32 * L); a.take(p.qInfo, L); a.take(p.qPre, L);
  a.take(p.taken, (maxN + kTakenPad + 1) * nt); a.take(p.assigned, maxN * nt);
  a.take(p.cellStart, (kGridCells + 1) * nf); a.take(p.cellIdx, sumN); a.take(p.sortedKp, sumN); a.take(p.sortedDesc, 32 * sumN);
  return a.L.bytes;
}

// `call`, ydorb_mapdb_create_new_points: nNb neighbours, nq queries each (the first keyframe's BoW span), n features of the first
// keyframe.  `up` is what one upload brings (the first keyframe's record, the neighbour and call records, the depths), `down` what one
// read-back takes (the three dense outputs, match counts, pool heads, the overflow word).
struct TriPtrs {
  uint8_t *up, *down;
  int2 *qRange, *qInfo; int *qFeat, *matchQ, *assigned; float* qAngle;
};
size_t layTri(size_t upBytes, size_t downBytes, size_t nNb, size_t nq, void* base, TriPtrs& p) {
  Carve a(base);
  a.take(p.up, upBytes); a.take(p.down, downBytes);
  a.take(p.qRange, nNb * nq); a.take(p.qInfo, nNb * nq); a.take(p.qFeat, nq); a.take(p.qAngle, nq); a.take(p.matchQ, nNb * nq); a.take(p.assigned, nNb * nq);
  return a.L.bytes;
}

enum { TS_SEARCH = 0, TS_RESOLVE, TS_GEOMETRY, TS_COUNT };   // ydorb_matcher_create_points_times

// `call`, ydorb_mapdb_search_by_bow_keyframes / _frame: nqAll query slots over all pairs, nShared entries of the A-side arrays (the first
// keyframe's span once, or one per query slot), nAssigned entries of k_resolve's result.  `up` is what one upload brings (the pair and
// call records, the frame's feature vector, keypoints, descriptors and valid bytes), `down` what one read-back takes (the two dense
// outputs, match counts, pool heads, the overflow word).
struct BowBatchPtrs {
  uint8_t *up, *down;
  int2 *qRange, *qInfo; int *qFeat, *matchQ, *assigned; float* qAngle;
};
size_t layBowBatch(size_t upBytes, size_t downBytes, size_t nqAll, size_t nShared, size_t nAssigned, void* base, BowBatchPtrs& p) {
  Carve a(base);
  a.take(p.up, upBytes); a.take(p.down, downBytes);
  a.take(p.qRange, nqAll); a.take(p.qInfo, nqAll); a.take(p.qFeat, nShared); a.take(p.qAngle, nShared); a.take(p.matchQ, nqAll); a.take(p.assigned, nAssigned);
  return a.L.bytes;
}

enum { BS_SEARCH = 0, BS_RESOLVE, BS_EMIT, BS_COUNT };   // YdBowSearchStats::ms (ydorb_matcher_bow_search_stats)

}  // namespace

// Host-call and batched paths share no device state on a handle: a batched call may still be running on its caller's stream, and its
// sticky status still be unread, while a host call runs on the handle's own stream.
struct ydorb_matcher {
  int device = 0;
  hipStream_t stream = nullptr;
  Mem call;              // every synchronous host-call entry point: each ends in a stream synchronise, so the next one lays it out afresh
  Mem pool;              // the host calls' record pool: grows by poolRecords, not by a call's shape, and a replay after an overflow
  size_t poolRecords = 1u << 20;   // ... finds everything else where it was
  size_t fuseOvfPerCall = 1u << 14;   // ydorb_mapdb_fuse_search: the overflow region of each target's pool part, grown by a replay
  size_t triPoolPerNb = 1u << 14;     // ydorb_mapdb_create_new_points and ydorb_mapdb_search_by_bow_*: each neighbour's or pair's part of the pool, grown by a replay
  std::vector<hipEvent_t> triEv;      // ... its per-launch events, made when a profiled call first needs them
  double triMs[TS_COUNT]{};
  int triCalls = 0;
  hipEvent_t bowEv[BS_COUNT + 1]{};   // ydorb_mapdb_search_by_bow_*: made when a profiled call first needs them
  double bowMs[BS_COUNT]{};
  YdBowSearchStats bowStats{};
  Mem stereo;            // ydorb_stereo_matches (layStereo)
  PinnedMem hUp, hDown;  // ydorb_search_local_points: pinned staging of the map-point table, read-back of track rows + status bytes
  // What ydorb_match_pairs_device / ydorb_match_consecutive_device keep; nothing but them, synchronize and destroy touches it.
  struct Batch {
    Mem arena;           // layBatch
    Mem status;          // 64 bytes; word [1] is the overflow status, sticky until synchronize reads it
    // the descriptors the arena holds, re-uploaded only when they change.  Emptied when the arena is regrown: the new one holds none,
    // wherever it lies.  `at`: where they went; an upload stays valid only while a call's layout puts them there again.
    std::vector<FrameDev> hFrames;
    std::vector<CallDev> hCalls;
    float hSf[8] = {0};
    bool hIdentAffine = false;
    BatchPtrs at{};
    int ovfPerKeypoint = 16;
  } batch;
  bool profiling = false;
  hipEvent_t ev[MS_COUNT + 1]{};
  double stageMs[MS_COUNT]{};
  int stageCalls = 0;
  bool evPending = false;
  std::vector<Mem*> buffers() { return {&call, &pool, &stereo, &hUp, &hDown, &batch.arena, &batch.status}; }
  ydorb_matcher() { for (Mem* b : buffers()) b->slackDiv = 2; }   // 50 % slack instead of the default 25 %
};

static void collect(ydorb_matcher* m) {
  if (!m->profiling || !m->evPending) return;
  m->evPending = false;
  if (hipEventQuery(m->ev[MS_COUNT]) != hipSuccess) return;   // a pipelined caller launched again before the events completed: sample dropped, never waited for
  for (int i = 0; i < MS_COUNT; i++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, m->ev[i], m->ev[i + 1]) == hipSuccess) m->stageMs[i] += ms;
  }
  m->stageCalls++;
}

static bool validFrameView(const YdFrameView* fv) {
  return fv && fv->n >= 0 && (fv->n == 0 || (fv->kps && fv->desc)) && fv->max_x > fv->min_x && fv->max_y > fv->min_y;
}

extern "C" {

void ydorb_matcher_destroy(ydorb_matcher_t* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)hipStreamSynchronize(m->stream);
  for (Mem* b : m->buffers()) b->release();
  for (auto& e : m->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : m->triEv) (void)hipEventDestroy(e);
  for (auto& e : m->bowEv) if (e) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(m->stream);
  delete m;
}

int ydorb_matcher_create(int32_t device, ydorb_matcher_t** out) {
  if (!out) { set_error("null argument"); return YDORB_ERR_INVALID_ARG; }
  *out = nullptr;
  int rc = require_device(device);
  if (rc) return rc;
  ydorb_matcher* m = new ydorb_matcher();
  m->device = device;
  if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) {
    set_error("hipStreamCreate failed");
    delete m;
    return YDORB_ERR_HIP;
  }
  for (auto& e : m->ev) (void)hipEventCreate(&e);
  if (m->batch.status.ensure(64) != YDORB_OK || hipMemset(m->batch.status.p, 0, 64) != hipSuccess) {
    set_error("matcher scratch allocation failed");
    ydorb_matcher_destroy(m);
    return YDORB_ERR_HIP;
  }
  *out = m;
  return YDORB_OK;
}

int ydorb_descriptor_distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i += 8) {
    uint64_t x, y;
    memcpy(&x, a + i, 8);
    memcpy(&y, b + i, 8);
    d += __builtin_popcountll(x ^ y);
  }
  return d;
}

int ydorb_descriptor_distance_rows(ydorb_matcher_t* m, const uint8_t* a, const uint8_t* b, int32_t n, int32_t* out) {
  if (!m || !a || !b || !out || n < 0) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  if (n == 0) return YDORB_OK;
  HIPCHK(hipSetDevice(m->device));
  RowsPtrs r;
  if (const int rc = layOut(m->call, [&](void* base) { return layRows(n, n, 0, 0, n, 0, base, r); })) return rc;
  HIPCHK(hipMemcpyAsync(r.a, a, (size_t)32 * n, hipMemcpyHostToDevice, m->stream));
  HIPCHK(hipMemcpyAsync(r.b, b, (size_t)32 * n, hipMemcpyHostToDevice, m->stream));
  hipLaunchKernelGGL(k_hamming_rows, dim3((n + 255) / 256), dim3(256), 0, m->stream, r.a, r.b, n, r.out);
  HIPCHK(hipMemcpyAsync(out, r.out, sizeof(int) * n, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return YDORB_OK;
}

int ydorb_distinctive_descriptors(ydorb_matcher_t* m, const uint8_t* desc, const int32_t* offsets, int32_t nPoints, int32_t* best) {
  if (!m || !offsets || !best || nPoints < 0) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  if (nPoints == 0) return YDORB_OK;
  const int total = offsets[nPoints];
  if (offsets[0] != 0 || total < 0 || (total > 0 && !desc)) { set_error("invalid offsets"); return YDORB_ERR_INVALID_ARG; }
  for (int p = 0; p < nPoints; p++) {
    const int cnt = offsets[p + 1] - offsets[p];
    if (cnt < 0 || cnt > 65535) { set_error("map point %d holds %d descriptors (0..65535 supported)", p, cnt); return YDORB_ERR_INVALID_ARG; }
  }
  HIPCHK(hipSetDevice(m->device));
  RowsPtrs r;
  if (const int rc = layOut(m->call, [&](void* base) { return layRows(std::max(total, 1), 0, nPoints + 1, 0, nPoints, 0, base, r); })) return rc;
  if (total) HIPCHK(hipMemcpyAsync(r.a, desc, (size_t)32 * total, hipMemcpyHostToDevice, m->stream));
  HIPCHK(hipMemcpyAsync(r.offsets, offsets, sizeof(int) * (nPoints + 1), hipMemcpyHostToDevice, m->stream));
  hipLaunchKernelGGL(k_distinctive, dim3((nPoints + 3) / 4), dim3(256), 0, m->stream, r.a, r.offsets, nPoints, r.out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(best, r.out, sizeof(int) * nPoints, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return YDORB_OK;
}

// laid != nullptr: the caller has laid the call arena out (layProjection) and the nq query rows are in laid->queries already
// (ydorb_search_local_points builds them there with a kernel queued on m->stream; nothing below writes them or regrows the arena, so a
// record-pool replay finds them unchanged).  With laid given and qdesc == nullptr the query descriptors are in laid->qdesc already too
// (ydorb_mapdb_search_local_points copies them there on the device) and their upload is skipped.
static int searchProjectionImpl(ydorb_matcher_t* m, int32_t mode, const YdFrameView* fv, const YdQuery* queries, const uint8_t* qdesc,
                                int32_t nq, float ratio, int32_t orbDist, int32_t checkOri, uint8_t* taken, int32_t* assigned,
                                int32_t* nMatches, std::vector<uint32_t>* recordsOut, const float* invSigma2 = nullptr, int nLevels = 0,
                                int32_t* bestOut = nullptr, const ProjPtrs* laid = nullptr) {
  HIPCHK(hipSetDevice(m->device));
  const int n = fv->n;
  if (n > 65535) { set_error("frames with more than 65535 keypoints are not supported"); return YDORB_ERR_UNSUPPORTED; }
  if (nq == 0 || n == 0) { *nMatches = 0; return YDORB_OK; }
  int rc;
  ProjPtrs p;
  if (laid) p = *laid;
  else if ((rc = layOut(m->call, [&](void* base) { return layProjection(n, fv->right_x, nq, 0, 0, base, p); }))) return rc;
  for (int attempt = 0; attempt < 6; attempt++) {
    const size_t poolCap = (size_t)nq * kSlot + m->poolRecords;
    if ((rc = m->pool.ensure(sizeof(uint32_t) * poolCap))) return rc;
    HIPCHK(hipMemcpyAsync(p.kps, fv->kps, sizeof(YdKeyPoint) * n, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(p.desc, fv->desc, (size_t)32 * n, hipMemcpyHostToDevice, m->stream));
    if (fv->right_x) HIPCHK(hipMemcpyAsync(p.rightX, fv->right_x, sizeof(float) * n, hipMemcpyHostToDevice, m->stream));
    FrameDev F{};
    F.kps = p.kps; F.desc = p.desc; F.rightX = fv->right_x ? p.rightX : nullptr; F.nPtr = nullptr; F.n = n;
    F.minX = fv->min_x; F.minY = fv->min_y;
    F.gridWInv = static_cast<float>(kGridCols) / (fv->max_x - fv->min_x);  // frame.cpp:99-100
    F.gridHInv = static_cast<float>(kGridRows) / (fv->max_y - fv->min_y);
    F.cellStart = p.cellStart; F.cellIdx = p.cellIdx; F.sortedKp = p.sortedKp; F.sortedDesc = p.sortedDesc;
    HIPCHK(hipMemcpyAsync(p.frame, &F, sizeof(FrameDev), hipMemcpyHostToDevice, m->stream));
    if ((rc = launchGridBuild(1, n, m->stream, p.frame))) return rc;
    HIPCHK(hipMemsetAsync(p.status, 0, 64, m->stream));
    if (queries) HIPCHK(hipMemcpyAsync(p.queries, queries, sizeof(YdQuery) * nq, hipMemcpyHostToDevice, m->stream));
    if (qdesc || !laid) HIPCHK(hipMemcpyAsync(p.qdesc, qdesc, (size_t)32 * nq, hipMemcpyHostToDevice, m->stream));
    if (taken) HIPCHK(hipMemcpyAsync(p.taken, taken, n, hipMemcpyHostToDevice, m->stream));
    else HIPCHK(hipMemsetAsync(p.taken, 0, n, m->stream));
    if (assigned) HIPCHK(hipMemcpyAsync(p.assigned, assigned, sizeof(int) * n, hipMemcpyHostToDevice, m->stream));
    CallDev C{};
    C.tkps = p.kps; C.queries = p.queries; C.qdesc = p.qdesc; C.nq = nq; C.qInfo = p.qInfo; C.qPre = p.qPre;   // frame 0, counts from the host
    C.taken = p.taken; C.takenClear = taken ? 0 : 1; C.assigned = p.assigned; C.matchQ = p.matchQ;
    C.count = p.status + 2; C.mode = mode; C.ratio = ratio; C.orbDist = orbDist; C.checkOri = checkOri;
    for (int i = 0; i < 8; i++) C.invSigma2[i] = (invSigma2 && i < nLevels) ? invSigma2[i] : 0.f;
    HIPCHK(hipMemcpyAsync(p.call, &C, sizeof(CallDev), hipMemcpyHostToDevice, m->stream));
    hipLaunchKernelGGL(k_gather_projection, dim3((nq + 4 * kGatherQpw - 1) / (4 * kGatherQpw), 1), dim3(256), 0, m->stream, p.call, p.frame, nq,
                       m->pool.as<uint32_t>(), reinterpret_cast<unsigned*>(p.status), (unsigned)poolCap, p.status + 1);
    int hmisc[3];
    if (!recordsOut) {
      const int takenWords = (n + 31) / 32;
      hipLaunchKernelGGL(k_resolve, dim3(1), dim3(64), 2 * sizeof(unsigned) * takenWords, m->stream, p.call, p.frame, m->pool.as<uint32_t>(), takenWords);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hmisc, p.status, sizeof(hmisc), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (hmisc[1] != 0) {  // record pool too small: grow and replay (the kernels wrote nothing past the pool)
      m->poolRecords = std::max<size_t>(m->poolRecords * 4, (size_t)(unsigned)hmisc[0] + 1024);
      continue;
    }
    if (recordsOut) {
      std::vector<int2> info(nq);
      HIPCHK(hipMemcpy(info.data(), p.qInfo, sizeof(int2) * nq, hipMemcpyDeviceToHost));
      recordsOut->resize(info[0].y);
      if (info[0].y) HIPCHK(hipMemcpy(recordsOut->data(), m->pool.as<uint32_t>() + info[0].x, sizeof(uint32_t) * info[0].y, hipMemcpyDeviceToHost));
      return YDORB_OK;
    }
    if (taken) HIPCHK(hipMemcpy(taken, p.taken, n, hipMemcpyDeviceToHost));
    if (assigned) HIPCHK(hipMemcpy(assigned, p.assigned, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (bestOut) HIPCHK(hipMemcpy(bestOut, p.matchQ, sizeof(int) * nq, hipMemcpyDeviceToHost));
    *nMatches = hmisc[2];
    return YDORB_OK;
  }
  set_error("candidate record pool kept overflowing");
  return YDORB_ERR_CAPACITY;
}

// One search of the BoW family (orbMatcher.cpp:303-462, :463-565): the features of A marked eligible are matched against the features of B
// that share their vocabulary node.
struct BowJob {
  struct Side {
    const YdKeyPoint* kps; const uint8_t* desc; int n; const YdFeatureVector* fv;
    const uint8_t* ok;     // [n] A: may be a query; B: may be a candidate, null = every feature
    const uint8_t* good;   // [n] searchForTriangulation: has a stereo coordinate
  } A, B;
  int mode;                // CallDev::mode: 3, 4 or 5
  float ratio;
  int checkOri;
  BowCallDev geom;         // searchForTriangulation (geom.tri != 0): F, epipole, level tables; bowSearch fills the pointers in
};

// Join, layout, uploads, gather + resolve, read-back.  qFeat[q] = the feature of A behind query q (empty: nothing to match, res is not
// written); res = the resolved assignment: per feature of B the query it went to (mode 3), else per query its feature of B, or -1.
static int bowSearch(ydorb_matcher_t* m, const BowJob& J, std::vector<int>& qFeat, std::vector<int>& res, int32_t* nMatches) {
  // which vocabulary nodes meet: merge-join of the two ascending id lists (orbMatcher.cpp:317-361, :484-541)
  std::vector<int2> qRange;
  std::vector<float> qAngle;
  size_t records = 0;
  const YdFeatureVector &fa = *J.A.fv, &fb = *J.B.fv;
  for (int a = 0, b = 0; a < fa.n_nodes && b < fb.n_nodes;) {
    if (fa.node_ids[a] == fb.node_ids[b]) {
      for (int ia = fa.node_start[a]; ia < fa.node_start[a + 1]; ia++) {
        const int idxA = fa.feat[ia];
        if (!J.A.ok[idxA]) continue;
        qFeat.push_back(idxA);
        qRange.push_back(make_int2(fb.node_start[b], fb.node_start[b + 1]));
        qAngle.push_back(J.A.kps[idxA].angle);
        records += (size_t)(fb.node_start[b + 1] - fb.node_start[b]);
      }
      a++; b++;
    } else if (fa.node_ids[a] < fb.node_ids[b]) {
      a = (int)(std::lower_bound(fa.node_ids, fa.node_ids + fa.n_nodes, fb.node_ids[b]) - fa.node_ids);
    } else {
      b = (int)(std::lower_bound(fb.node_ids, fb.node_ids + fb.n_nodes, fa.node_ids[a]) - fb.node_ids);
    }
  }
  const int nq = (int)qFeat.size();
  if (nq == 0) return YDORB_OK;
  const int nFeatB = fb.node_start[fb.n_nodes], nA = J.A.n, nB = J.B.n;
  m->poolRecords = std::max<size_t>(m->poolRecords, records + 1024);
  int rc;
  BowPtrs p;
  if ((rc = layOut(m->call, [&](void* base) { return layBow(nA, nB, std::max(nFeatB, 1), nq, J.geom.tri, base, p); })) ||
      (rc = m->pool.ensure(sizeof(uint32_t) * m->poolRecords)))
    return rc;
  hipStream_t s = m->stream;
  HIPCHK(hipMemsetAsync(p.status, 0, 64, s));
  HIPCHK(hipMemcpyAsync(p.descA, J.A.desc, (size_t)32 * nA, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p.descB, J.B.desc, (size_t)32 * nB, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p.kpsB, J.B.kps, sizeof(YdKeyPoint) * nB, hipMemcpyHostToDevice, s));
  if (nFeatB) HIPCHK(hipMemcpyAsync(p.feat, fb.feat, sizeof(int) * nFeatB, hipMemcpyHostToDevice, s));
  if (J.B.ok) HIPCHK(hipMemcpyAsync(p.valid, J.B.ok, nB, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p.qFeat, qFeat.data(), sizeof(int) * nq, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p.qRange, qRange.data(), sizeof(int2) * nq, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p.qAngle, qAngle.data(), sizeof(float) * nq, hipMemcpyHostToDevice, s));
  res.resize(std::max(nq, nB));
  HIPCHK(hipMemsetAsync(p.assigned, 0xFF, sizeof(int) * res.size(), s));
  BowCallDev BC = J.geom;
  BC.descA = p.descA; BC.descB = p.descB; BC.qFeat = p.qFeat; BC.qRange = p.qRange;
  BC.featB = p.feat; BC.validB = J.B.ok ? p.valid : nullptr; BC.nq = nq; BC.qInfo = p.qInfo;
  if (BC.tri) {
    HIPCHK(hipMemcpyAsync(p.kpsA, J.A.kps, sizeof(YdKeyPoint) * nA, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p.goodA, J.A.good, nA, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p.goodB, J.B.good, nB, hipMemcpyHostToDevice, s));
    BC.kpsA = p.kpsA; BC.kpsB = p.kpsB; BC.goodA = p.goodA; BC.goodB = p.goodB;
  }
  hipLaunchKernelGGL(k_gather_bow, dim3((nq + 3) / 4), dim3(256), 0, s, BC, m->pool.as<uint32_t>(), reinterpret_cast<unsigned*>(p.status),
                     (unsigned)m->poolRecords, p.status + 1);
  CallDev C{};
  C.tkps = p.kpsB; C.qAngle = p.qAngle; C.nq = nq; C.qInfo = p.qInfo; C.assigned = p.assigned; C.matchQ = p.matchQ;   // no frame, query rows or taken flags
  C.count = p.status + 2; C.mode = J.mode; C.ratio = J.ratio; C.checkOri = J.checkOri;
  HIPCHK(hipMemcpyAsync(p.call, &C, sizeof(CallDev), hipMemcpyHostToDevice, s));
  const int takenWords = (nB + 31) / 32;
  hipLaunchKernelGGL(k_resolve, dim3(1), dim3(64), 2 * sizeof(unsigned) * takenWords, s, p.call, (const FrameDev*)nullptr, m->pool.as<uint32_t>(), takenWords);
  HIPCHK(hipGetLastError());
  int hmisc[3];
  HIPCHK(hipMemcpyAsync(hmisc, p.status, sizeof(hmisc), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(res.data(), p.assigned, sizeof(int) * res.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (hmisc[1] != 0) { set_error("bow record pool overflow"); return YDORB_ERR_CAPACITY; }
  *nMatches = hmisc[2];
  return YDORB_OK;
}

int ydorb_search_by_projection(ydorb_matcher_t* m, int32_t mode, const YdFrameView* fv, const YdQuery* queries, const uint8_t* qdesc,
                               int32_t nq, float ratio, int32_t orbDist, int32_t checkOri, uint8_t* taken, int32_t* assigned,
                               int32_t* nMatches) {
  if (!m || !validFrameView(fv) || !nMatches || mode < 0 || (mode > 2 && mode != 7) || nq < 0 || (nq > 0 && (!queries || !qdesc)) ||
      (fv->n > 0 && !assigned)) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  if (mode == 7) checkOri = 0;   // searchByProjectionInSim has no rotation-consistency step
  return searchProjectionImpl(m, mode, fv, queries, qdesc, nq, ratio, orbDist, checkOri, taken, assigned, nMatches, nullptr);
}

int ydorb_search_local_points(ydorb_matcher_t* m, const YdFrameView* fv, const YdFrustumView* view, const YdMapPointTable* table,
                              const uint8_t* skip, const uint8_t* hasObs, float th, float ratio, uint8_t* taken, int32_t* assigned,
                              YdTrackView* rows, uint8_t* status, int32_t* nToMatch, int32_t* nMatches) {
  if (!m || !fv || !view || !table || !nToMatch || !nMatches) { set_error("search_local_points: null argument"); return YDORB_ERR_INVALID_ARG; }
  if (view->n_levels < 1 || view->n_levels > 8) { set_error("search_local_points: n_levels %d outside 1..8", view->n_levels); return YDORB_ERR_INVALID_ARG; }
  const int np = table->n, n = fv->n;
  if (np < 0 || n < 0) { set_error("search_local_points: negative size"); return YDORB_ERR_INVALID_ARG; }
  if (np > 0 && (!table->pos_min || !table->normal_max || !table->max_distance || !table->desc || !skip || !hasObs || !rows || !status)) {
    set_error("search_local_points: null map-point table, flag or output arrays");
    return YDORB_ERR_INVALID_ARG;
  }
  if (!validFrameView(fv) || (n > 0 && !assigned)) {
    set_error("search_local_points: invalid frame view");
    return YDORB_ERR_INVALID_ARG;
  }
  *nToMatch = 0; *nMatches = 0;
  if (np == 0) return YDORB_OK;
  HIPCHK(hipSetDevice(m->device));
  const size_t p = np;
  Layout U;
  const size_t oPos = U.add(16 * p), oNrm = U.add(16 * p), oMax = U.add(4 * p), oSkip = U.add(p), oObs = U.add(p);
  Layout D;
  const size_t dRows = D.add(sizeof(YdTrackView) * p), dSt = D.add(p);
  // table, track rows and status lie in the call arena with the search's arrays: it is grown, if at all, before k_frustum_queries
  // writes the query rows into it
  int rc;
  ProjPtrs q;
  if ((rc = m->hUp.ensure(U.bytes)) || (rc = m->hDown.ensure(D.bytes))) return rc;
  if ((rc = layOut(m->call, [&](void* base) { return layProjection(std::max(n, 1), fv->right_x, np, U.bytes, D.bytes, base, q); }))) return rc;
  std::memcpy(at<void>(m->hUp, oPos), table->pos_min, 16 * p);
  std::memcpy(at<void>(m->hUp, oNrm), table->normal_max, 16 * p);
  std::memcpy(at<void>(m->hUp, oMax), table->max_distance, 4 * p);
  std::memcpy(at<void>(m->hUp, oSkip), skip, p);
  std::memcpy(at<void>(m->hUp, oObs), hasObs, p);
  HIPCHK(hipMemcpyAsync(q.table, m->hUp.p, U.bytes, hipMemcpyHostToDevice, m->stream));
  hipLaunchKernelGGL(frustum::k_frustum_queries<QueryDev>, dim3((np + frustum::kThreads - 1) / frustum::kThreads), dim3(frustum::kThreads), 0, m->stream, *view,
                     np, (const float4*)(q.table + oPos), (const float4*)(q.table + oNrm), (const float*)(q.table + oMax), q.table + oSkip, q.table + oObs, th,
                     q.queries, (YdTrackView*)(q.track + dRows), q.track + dSt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(m->hDown.p, q.track, D.bytes, hipMemcpyDeviceToHost, m->stream));
  // the search follows on the same stream without a host round trip: with no point in view every query has flags 0, nothing matches and
  // assigned / taken come back as they went up, which is the reference's skipped search
  if ((rc = searchProjectionImpl(m, YDORB_SEARCH_FRAME_MAPPOINT, fv, nullptr, table->desc, np, ratio, 0, 0, taken, assigned, nMatches, nullptr, nullptr, 0,
                                 nullptr, &q)))
    return rc;
  HIPCHK(hipStreamSynchronize(m->stream));   // the search returns early, without one, for a frame without keypoints
  std::memcpy(rows, at<void>(m->hDown, dRows), sizeof(YdTrackView) * p);
  std::memcpy(status, at<void>(m->hDown, dSt), p);
  for (int i = 0; i < np; i++) *nToMatch += status[i] == YDORB_FRUSTUM_IN_VIEW;
  return YDORB_OK;
}

// ydorb_search_local_points over a resident map table (map_resident.hip, mapdb_resident_points.h): what goes up is the slot list and
// the skip bytes; k_mapdb_local_queries reads the points by slot and leaves query rows and query descriptors in the call arena.  The
// table's mutex is held from its sync to the end of the call.  The matcher's stream is ordered behind that sync by a synchronise of
// the table's stream inside lockResident (DESIGN.md section 6q says why not an event).  Every return after the first launch, an error
// included, synchronises the matcher's stream before the mutex goes.
int ydorb_mapdb_search_local_points(ydorb_mapdb_t* db, ydorb_matcher_t* m, const YdFrameView* fv, const YdFrustumView* view, const int32_t* slots,
                                    int32_t np, const uint8_t* skip, float th, float ratio, uint8_t* taken, int32_t* assigned, YdTrackView* rows,
                                    uint8_t* status, int32_t* nToMatch, int32_t* nMatches) {
  if (!db || !m || !fv || !view || !nToMatch || !nMatches) { set_error("mapdb_search_local_points: null argument"); return YDORB_ERR_INVALID_ARG; }
  if (view->n_levels < 1 || view->n_levels > 8) { set_error("mapdb_search_local_points: n_levels %d outside 1..8", view->n_levels); return YDORB_ERR_INVALID_ARG; }
  if (np < 0) { set_error("mapdb_search_local_points: negative number of point slots: %d", np); return YDORB_ERR_INVALID_ARG; }
  if (np > 0 && (!slots || !skip || !rows || !status)) {
    set_error("mapdb_search_local_points: null point_slots, skip, rows or status");
    return YDORB_ERR_INVALID_ARG;
  }
  const int n = fv->n;
  if (!validFrameView(fv) || (n > 0 && !assigned)) {
    set_error("mapdb_search_local_points: invalid frame view");
    return YDORB_ERR_INVALID_ARG;
  }
  *nToMatch = 0; *nMatches = 0;
  mapdb::ResidentPoints R;
  mapdb::ResidentLock lock;
  int rc;
  if ((rc = mapdb::lockResident(db, m->device, slots, np, R))) return rc;   // also refuses a table without attributes
  lock.db = db;
  if (np == 0) return YDORB_OK;
  if (n > 65535) { set_error("frames with more than 65535 keypoints are not supported"); return YDORB_ERR_UNSUPPORTED; }   // before anything is queued
  HIPCHK(hipSetDevice(m->device));
  // From the first launch on, no way out of this function gives the table's mutex back while the matcher's stream may still read the
  // resident arenas: declared after `lock`, so it drains the stream before the mutex is released, on the error returns too.
  struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{m->stream};
  const size_t p = np;
  Layout U;
  const size_t oSlots = U.add(4 * p), oSkip = U.add(p);
  Layout D;
  const size_t dRows = D.add(sizeof(YdTrackView) * p), dSt = D.add(p);
  ProjPtrs q;
  if ((rc = m->hUp.ensure(U.bytes)) || (rc = m->hDown.ensure(D.bytes))) return rc;
  if ((rc = layOut(m->call, [&](void* base) { return layProjection(std::max(n, 1), fv->right_x, np, U.bytes, D.bytes, base, q); }))) return rc;
  std::memcpy(at<void>(m->hUp, oSlots), slots, 4 * p);
  std::memcpy(at<void>(m->hUp, oSkip), skip, p);
  HIPCHK(hipMemcpyAsync(q.table, m->hUp.p, U.bytes, hipMemcpyHostToDevice, m->stream));
  hipLaunchKernelGGL(frustum::k_mapdb_local_queries<QueryDev>, dim3((np + frustum::kThreads - 1) / frustum::kThreads), dim3(frustum::kThreads), 0, m->stream,
                     *view, np, (const int*)(q.table + oSlots), q.table + oSkip, R, th, q.queries, (uint4*)q.qdesc, (YdTrackView*)(q.track + dRows),
                     q.track + dSt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(m->hDown.p, q.track, D.bytes, hipMemcpyDeviceToHost, m->stream));
  if ((rc = searchProjectionImpl(m, YDORB_SEARCH_FRAME_MAPPOINT, fv, nullptr, nullptr, np, ratio, 0, 0, taken, assigned, nMatches, nullptr, nullptr, 0,
                                 nullptr, &q)))
    return rc;
  HIPCHK(hipStreamSynchronize(m->stream));   // the search returns early, without one, for a frame without keypoints
  std::memcpy(rows, at<void>(m->hDown, dRows), sizeof(YdTrackView) * p);
  std::memcpy(status, at<void>(m->hDown, dSt), p);
  for (int i = 0; i < np; i++) *nToMatch += status[i] == YDORB_FRUSTUM_IN_VIEW;
  return YDORB_OK;
}

// OrbMatcher::fuseByProjection / fuseBySim3 for several target keyframes over a resident map table (map_resident.hip,
// mapdb_resident_points.h): k_mapdb_fuse_queries builds every target's query rows and query descriptors from the resident points, the
// target frames point into the resident feature and descriptor pools, and the batch kernels of ydorb_match_pairs_device run once over
// all targets (mode 6).  One upload, one read-back.  The table's mutex is held from its sync to the end of the call, as in
// ydorb_mapdb_search_local_points; every return after the first launch, an error included, synchronises the matcher's stream first.
// The pool follows the batch layout, max_list fixed slots of kSlot records plus an overflow region per call; the overflow word is
// read here, and a set one grows the region to what the heads asked for and replays (the kernels wrote nothing past the pool).
int ydorb_mapdb_fuse_search(ydorb_mapdb_t* db, ydorb_matcher_t* m, const YdFuseTarget* targets, int32_t nTargets, const int32_t* listStart,
                            const int32_t* pointSlots, const uint8_t* skip, int32_t* bestIdx, uint8_t* status, int32_t* nFound, uint8_t* targetStatus) {
  if (!db || !m) { set_error("mapdb_fuse_search: null handle"); return YDORB_ERR_INVALID_ARG; }
  if (nTargets < 0) { set_error("mapdb_fuse_search: negative number of targets: %d", nTargets); return YDORB_ERR_INVALID_ARG; }
  std::string err;
  if (!maptable::checkStarts("list_start", listStart, nTargets, err)) { set_error("mapdb_fuse_search: %s", err.c_str()); return YDORB_ERR_INVALID_ARG; }
  const int32_t L = listStart[nTargets];
  if ((nTargets > 0 && (!targets || !nFound || !targetStatus)) || (L > 0 && (!pointSlots || !skip || !bestIdx || !status))) {
    set_error("mapdb_fuse_search: null targets, n_found, target_status, point_slots, skip, best_idx or status");
    return YDORB_ERR_INVALID_ARG;
  }
  for (int t = 0; t < nTargets; t++) {
    const YdFuseTarget& G = targets[t];
    if (G.view.n_levels < 1 || G.view.n_levels > 8) { set_error("mapdb_fuse_search: target %d: n_levels %d outside 1..8", t, G.view.n_levels); return YDORB_ERR_INVALID_ARG; }
    if (G.max_dist < 0 || G.max_dist > 256) { set_error("mapdb_fuse_search: target %d: max_dist %d outside 0..256", t, G.max_dist); return YDORB_ERR_INVALID_ARG; }
    if (!(G.view.max_x > G.view.min_x && G.view.max_y > G.view.min_y)) { set_error("mapdb_fuse_search: target %d: empty image bounds", t); return YDORB_ERR_INVALID_ARG; }
  }
  const size_t nt = (size_t)nTargets, nl = (size_t)L;
  std::vector<int32_t> kfSlots(nt), featStart(nt, 0), featLen(nt, 0), blockStart(nt, 0), blockLen(nt, 0);
  for (size_t t = 0; t < nt; t++) kfSlots[t] = targets[t].kf_slot;
  mapdb::ResidentPoints R;
  mapdb::ResidentKeyframes K;
  mapdb::ResidentLock lock;
  int rc;
  if ((rc = mapdb::lockResidentFuse(db, m->device, pointSlots, L, kfSlots.data(), nTargets, R, K, featStart.data(), featLen.data(), blockStart.data(),
                                    blockLen.data())))
    return rc;   // also refuses a table without attributes or features
  lock.db = db;
  for (size_t t = 0; t < nt; t++) { nFound[t] = 0; targetStatus[t] = YDORB_FUSE_TARGET_OK; }
  if (L == 0) {   // nothing was synced: the mirrors' lengths were not read
    return YDORB_OK;
  }
  // one FrameDev per distinct (keyframe, stereo or not, bounds); a target without a usable frame searches nothing
  struct FrameKey { int32_t kf, mono; float b[4]; };
  std::vector<FrameKey> keys;
  std::vector<int> frameOf(nt, -1);
  std::vector<size_t> frameAt;   // where each frame's grid arrays begin, in features
  size_t sumN = 0, maxN = 0, maxList = 0;
  for (size_t t = 0; t < nt; t++) {
    const YdFuseTarget& G = targets[t];
    if (featLen[t] == 0) targetStatus[t] = YDORB_FUSE_TARGET_NO_FEATURES;
    else if (blockLen[t] == 0) targetStatus[t] = YDORB_FUSE_TARGET_NO_BLOCK;
    else if (blockLen[t] != featLen[t]) targetStatus[t] = YDORB_FUSE_TARGET_LENGTH_MISMATCH;
    if (targetStatus[t] != YDORB_FUSE_TARGET_OK) continue;
    maxList = std::max(maxList, (size_t)(listStart[t + 1] - listStart[t]));
    const FrameKey key{G.kf_slot, (G.flags & YDORB_FUSE_MONOCULAR) ? 1 : 0, {G.view.min_x, G.view.max_x, G.view.min_y, G.view.max_y}};
    for (size_t f = 0; f < keys.size() && frameOf[t] < 0; f++)
      if (!memcmp(&keys[f], &key, sizeof(FrameKey))) frameOf[t] = (int)f;
    if (frameOf[t] >= 0) continue;
    frameOf[t] = (int)keys.size();
    keys.push_back(key);
    frameAt.push_back(sumN);
    sumN += (size_t)featLen[t];
    maxN = std::max(maxN, (size_t)featLen[t]);
  }
  const size_t nf = keys.size();
  HIPCHK(hipSetDevice(m->device));
  struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{m->stream};   // before the mutex goes: see above
  Layout U;
  const size_t oTargets = U.add(sizeof(YdFuseTarget) * nt), oStart = U.add(4 * (nt + 1)), oSlots = U.add(4 * nl), oSkip = U.add(nl),
               oFrames = U.add(sizeof(FrameDev) * nf), oCalls = U.add(sizeof(CallDev) * nt);
  Layout D;
  const size_t dMatch = D.add(4 * nl), dSt = D.add(nl), dCount = D.add(4 * nt), dHeads = D.add(4 * nt), dOvf = D.add(16);
  FusePtrs p;
  if ((rc = m->hUp.ensure(U.bytes)) || (rc = m->hDown.ensure(D.bytes))) return rc;
  if ((rc = layOut(m->call, [&](void* base) { return layFuse(U.bytes, D.bytes, nt, nf, sumN, maxN, nl, base, p); }))) return rc;
  const size_t takenStride = maxN + kTakenPad + 1;
  std::memcpy(at<void>(m->hUp, oTargets), targets, sizeof(YdFuseTarget) * nt);
  std::memcpy(at<void>(m->hUp, oStart), listStart, 4 * (nt + 1));
  std::memcpy(at<void>(m->hUp, oSlots), pointSlots, 4 * nl);
  std::memcpy(at<void>(m->hUp, oSkip), skip, nl);
  FrameDev* hf = at<FrameDev>(m->hUp, oFrames);
  CallDev* hc = at<CallDev>(m->hUp, oCalls);
  std::memset(hf, 0, sizeof(FrameDev) * nf);
  std::memset(hc, 0, sizeof(CallDev) * nt);
  for (size_t t = 0; t < nt; t++) {
    const int f = frameOf[t];
    const YdFuseTarget& G = targets[t];
    CallDev& C = hc[t];
    C.frame = std::max(f, 0); C.qAngle = nullptr; C.nqPtr = nullptr; C.qkps = nullptr;
    C.queries = p.queries + listStart[t]; C.qdesc = p.qdesc + 32 * (size_t)listStart[t];
    C.nq = f < 0 ? 0 : listStart[t + 1] - listStart[t];
    C.qInfo = p.qInfo + listStart[t]; C.qPre = p.qPre + listStart[t];
    C.taken = p.taken + t * takenStride; C.takenClear = 1; C.assigned = p.assigned + t * maxN;
    C.matchQ = reinterpret_cast<int*>(p.down + dMatch) + listStart[t]; C.count = reinterpret_cast<int*>(p.down + dCount) + t;
    C.mode = 6; C.ratio = 0.f; C.orbDist = G.max_dist; C.checkOri = 0;
    for (int i = 0; i < 8; i++) C.invSigma2[i] = G.inv_sigma2[i];
    if (f < 0) continue;
    FrameDev& F = hf[f];
    if (F.kps) { C.tkps = F.kps; continue; }
    F.kps = reinterpret_cast<const KeyPointDev*>(K.kps) + featStart[t];
    F.desc = K.blockPool + 32 * (size_t)blockStart[t];
    F.rightX = (G.flags & YDORB_FUSE_MONOCULAR) ? nullptr : K.rightX + featStart[t];
    F.nPtr = nullptr; F.n = featLen[t];
    F.minX = G.view.min_x; F.minY = G.view.min_y;
    F.gridWInv = static_cast<float>(kGridCols) / (G.view.max_x - G.view.min_x);
    F.gridHInv = static_cast<float>(kGridRows) / (G.view.max_y - G.view.min_y);
    F.cellStart = p.cellStart + (size_t)f * (kGridCells + 1); F.cellIdx = p.cellIdx + frameAt[f];
    F.sortedKp = p.sortedKp + frameAt[f]; F.sortedDesc = p.sortedDesc + 32 * frameAt[f];
    C.tkps = F.kps;
  }
  hipStream_t s = m->stream;
  HIPCHK(hipMemcpyAsync(p.up, m->hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(p.down, 0xFF, 4 * nl, s));   // best_idx -1 wherever no call writes it
  fuse::QueryArgs qa;
  qa.nTargets = nTargets; qa.nEntries = L;
  qa.start = reinterpret_cast<const int*>(p.up + oStart); qa.targets = reinterpret_cast<const fuse::TargetDev*>(p.up + oTargets);
  qa.slots = reinterpret_cast<const int*>(p.up + oSlots); qa.skip = p.up + oSkip;
  qa.R = R; qa.obsKf = K.obsKf; qa.qdesc = reinterpret_cast<uint4*>(p.qdesc); qa.status = p.down + dSt;
  hipLaunchKernelGGL(fuse::k_mapdb_fuse_queries<QueryDev>, dim3((unsigned)((nl + fuse::kThreads - 1) / fuse::kThreads)), dim3(fuse::kThreads), 0, s, qa, p.queries);
  HIPCHK(hipGetLastError());
  const FrameDev* dFrames = reinterpret_cast<const FrameDev*>(p.up + oFrames);
  const CallDev* dCalls = reinterpret_cast<const CallDev*>(p.up + oCalls);
  if (nf > 0 && (rc = launchGridBuild((int)nf, (int)maxN, s, dFrames))) return rc;   // once: a replay finds the grids where they are
  const int takenWords = (int)((maxN + 31) / 32);
  for (int attempt = 0; attempt < 6; attempt++) {
    const size_t poolPerCall = maxList * kSlot + m->fuseOvfPerCall;
    if (poolPerCall * nt > (size_t)INT32_MAX) { set_error("mapdb_fuse_search: a record pool of %zu entries, past INT32_MAX", poolPerCall * nt); return YDORB_ERR_CAPACITY; }
    if ((rc = m->pool.ensure(sizeof(uint32_t) * poolPerCall * nt))) return rc;
    HIPCHK(hipMemsetAsync(p.down + dCount, 0, D.bytes - dCount, s));   // counts, heads, overflow word
    if (nf > 0 && maxList > 0) {
      HIPCHK(hipMemsetAsync(p.taken, 0, takenStride * nt, s));
      hipLaunchKernelGGL(k_gather_projection, dim3((unsigned)((maxList + 4 * kGatherQpw - 1) / (4 * kGatherQpw)), nTargets), dim3(256), 0, s, dCalls, dFrames,
                         (int)maxList, m->pool.as<uint32_t>(), reinterpret_cast<unsigned*>(p.down + dHeads), (unsigned)poolPerCall,
                         reinterpret_cast<int*>(p.down + dOvf));
      hipLaunchKernelGGL(k_resolve, dim3(nTargets), dim3(64), 2 * sizeof(unsigned) * takenWords, s, dCalls, dFrames, m->pool.as<uint32_t>(), takenWords);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(m->hDown.p, p.down, D.bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (*at<int>(m->hDown, dOvf) != 0) {
      const unsigned* heads = at<unsigned>(m->hDown, dHeads);
      size_t asked = 0;
      for (size_t t = 0; t < nt; t++) asked = std::max(asked, (size_t)heads[t]);
      m->fuseOvfPerCall = std::max(m->fuseOvfPerCall * 2, asked + 1024);
      continue;
    }
    std::memcpy(bestIdx, at<void>(m->hDown, dMatch), 4 * nl);
    std::memcpy(status, at<void>(m->hDown, dSt), nl);
    std::memcpy(nFound, at<void>(m->hDown, dCount), 4 * nt);
    return YDORB_OK;
  }
  set_error("mapdb_fuse_search: candidate record pool kept overflowing");
  return YDORB_ERR_CAPACITY;
}

// LocalMapping::createNewMapPoints for all neighbours over a resident map table (mapdb_tri_kernels.hip.h has the kernels and what each
// does).  The join and the gather run once over all neighbours; then, per usable neighbour in order and with nothing crossing the host,
// the unchanged k_resolve (mode 5) and the geometry kernel, whose accepted matches empty their queries for the neighbours still to
// come.  One upload, one read-back.  The table's mutex is held from its sync to the end of the call, as in ydorb_mapdb_fuse_search;
// every return after the first launch, an error included, synchronises the matcher's stream first.  The geometry reads k_resolve's
// `assigned` row, not matchQ: with check_orientation the histogram cull clears the former only.  A set overflow word grows every
// neighbour's part of the pool to what the heads asked for and replays the whole call: the gather rewrites every qInfo, so the claims
// of the abandoned attempt are gone.
int ydorb_mapdb_create_new_points(ydorb_mapdb_t* db, ydorb_matcher_t* m, const YdCreateView* first, const YdCreateNeighbour* nbs, int32_t nNb,
                                  int32_t stereoOnly, int32_t checkOri, int32_t* matched, float* x3d, uint8_t* status, int32_t* nMatches,
                                  int32_t* nAccepted, uint8_t* nbStatus) {
  if (!db || !m) { set_error("mapdb_create_new_points: null handle"); return YDORB_ERR_INVALID_ARG; }
  if (!first) { set_error("mapdb_create_new_points: null first keyframe"); return YDORB_ERR_INVALID_ARG; }
  if (nNb < 0) { set_error("mapdb_create_new_points: negative number of neighbours: %d", nNb); return YDORB_ERR_INVALID_ARG; }
  if (first->n < 0 || (first->n > 0 && !first->depth)) { set_error("mapdb_create_new_points: first keyframe: negative n or null depth"); return YDORB_ERR_INVALID_ARG; }
  if (first->n_levels < 1 || first->n_levels > 8) { set_error("mapdb_create_new_points: first keyframe: n_levels %d outside 1..8", first->n_levels); return YDORB_ERR_INVALID_ARG; }
  if (nNb > 0 && (!nbs || !nMatches || !nAccepted || !nbStatus || (first->n > 0 && (!matched || !x3d || !status)))) {
    set_error("mapdb_create_new_points: null neighbours, matched_second, x3d, status, n_matches, n_accepted or neighbour_status");
    return YDORB_ERR_INVALID_ARG;
  }
  const size_t nn = (size_t)nNb, n1 = (size_t)first->n;
  std::vector<int32_t> kfSlots(nn + 1), nDepth(nn + 1);
  kfSlots[0] = first->kf_slot; nDepth[0] = first->n;
  size_t nDepthAll = n1;
  for (size_t i = 0; i < nn; i++) {
    const YdCreateView& V = nbs[i].view;
    if (V.n < 0 || (V.n > 0 && !V.depth)) { set_error("mapdb_create_new_points: neighbour %zu: negative n or null depth", i); return YDORB_ERR_INVALID_ARG; }
    if (V.n_levels < 1 || V.n_levels > 8) { set_error("mapdb_create_new_points: neighbour %zu: n_levels %d outside 1..8", i, V.n_levels); return YDORB_ERR_INVALID_ARG; }
    kfSlots[i + 1] = V.kf_slot; nDepth[i + 1] = V.n;
    nDepthAll += (size_t)V.n;
  }
  mapdb::ResidentTriPools P;
  std::vector<mapdb::ResidentTriSpans> spans(nn + 1);
  std::vector<uint8_t> kfStatus(nn + 1, 0);
  mapdb::ResidentLock lock;
  int rc;
  if ((rc = mapdb::lockResidentTri(db, m->device, kfSlots.data(), nDepth.data(), nNb, P, spans.data(), kfStatus.data()))) return rc;
  lock.db = db;
  if (nNb == 0) return YDORB_OK;
  bool any = false;
  for (size_t i = 0; i < nn; i++) {
    nbStatus[i] = kfStatus[0] ? kfStatus[0] : kfStatus[i + 1];
    nMatches[i] = 0; nAccepted[i] = 0;
    any = any || !nbStatus[i];
  }
  for (size_t o = 0; o < nn * n1; o++) { matched[o] = -1; status[o] = YDORB_TRI_UNMATCHED; }
  if (nn * n1) std::memset(x3d, 0, 12 * nn * n1);
  if (!any) return YDORB_OK;
  static_assert(sizeof(mapdbtri::Spans) == sizeof(mapdb::ResidentTriSpans), "one layout");
  const size_t nq = (size_t)spans[0].bowLen;
  HIPCHK(hipSetDevice(m->device));
  struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{m->stream};   // before the mutex goes: see ydorb_mapdb_search_local_points
  Layout U;
  const size_t oFirst = U.add(sizeof(mapdbtri::FirstDev)), oNb = U.add(sizeof(mapdbtri::NbDev) * nn), oCalls = U.add(sizeof(CallDev) * nn),
               oDepth = U.add(4 * nDepthAll);
  Layout D;
  const size_t dMatched = D.add(4 * nn * n1), dX = D.add(12 * nn * n1), dSt = D.add(nn * n1), dCount = D.add(4 * nn), dHeads = D.add(4 * nn), dOvf = D.add(16);
  TriPtrs p;
  if ((rc = m->hUp.ensure(U.bytes)) || (rc = m->hDown.ensure(D.bytes))) return rc;
  if ((rc = layOut(m->call, [&](void* base) { return layTri(U.bytes, D.bytes, nn, nq, base, p); }))) return rc;
  auto viewOf = [](const YdCreateView& V, tri::ViewDev& d) {
    std::memcpy(d.Tcw, V.Tcw, sizeof d.Tcw); std::memcpy(d.Rwc, V.Rwc, sizeof d.Rwc); std::memcpy(d.Ow, V.Ow, sizeof d.Ow);
    d.fx = V.fx; d.fy = V.fy; d.cx = V.cx; d.cy = V.cy; d.invfx = V.invfx; d.invfy = V.invfy; d.b = V.b; d.bf = V.bf;
  };
  mapdbtri::FirstDev* hFirst = at<mapdbtri::FirstDev>(m->hUp, oFirst);
  mapdbtri::NbDev* hNb = at<mapdbtri::NbDev>(m->hUp, oNb);
  CallDev* hc = at<CallDev>(m->hUp, oCalls);
  float* hDepth = at<float>(m->hUp, oDepth);
  std::memset(hFirst, 0, sizeof(mapdbtri::FirstDev));
  std::memset(hNb, 0, sizeof(mapdbtri::NbDev) * nn);
  std::memset(hc, 0, sizeof(CallDev) * nn);
  std::memcpy(&hFirst->k1, &spans[0], sizeof(mapdbtri::Spans));
  viewOf(*first, hFirst->view);
  for (int l = 0; l < first->n_levels; l++) { hFirst->sigma2[l] = first->level_sigma2[l]; hFirst->sf[l] = first->scale_factors[l]; }
  if (n1) std::memcpy(hDepth, first->depth, 4 * n1);
  const KeyPointDev* kps = reinterpret_cast<const KeyPointDev*>(P.kps);
  size_t depthAt = n1;
  for (size_t i = 0; i < nn; i++) {
    const YdCreateNeighbour& G = nbs[i];
    mapdbtri::NbDev& N = hNb[i];
    std::memcpy(&N.k2, &spans[i + 1], sizeof(mapdbtri::Spans));
    N.usable = nbStatus[i] == YDORB_CREATE_NB_OK; N.depthAt = (int)depthAt; N.ratioFactor = G.ratio_factor;
    N.geom.tri = 1;
    for (int k = 0; k < 9; k++) N.geom.F[k] = G.F[k];
    N.geom.ex = G.ex; N.geom.ey = G.ey;
    for (int l = 0; l < G.view.n_levels; l++) { N.geom.sfB[l] = G.view.scale_factors[l]; N.geom.sf2B[l] = G.view.level_sigma2[l]; }
    viewOf(G.view, N.view);
    if (G.view.n) std::memcpy(hDepth + depthAt, G.view.depth, 4 * (size_t)G.view.n);
    depthAt += (size_t)G.view.n;
    CallDev& C = hc[i];   // no frame, query rows or taken flags, as in the flat search
    C.tkps = kps + N.k2.featStart; C.qAngle = p.qAngle; C.nq = N.usable ? (int)nq : 0; C.qInfo = p.qInfo + i * nq;
    C.assigned = p.assigned + i * nq; C.matchQ = p.matchQ + i * nq; C.count = reinterpret_cast<int*>(p.down + dCount) + i;
    C.mode = 5; C.ratio = 0.f; C.checkOri = checkOri;
  }
  hipStream_t s = m->stream;
  HIPCHK(hipMemcpyAsync(p.up, m->hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  const mapdbtri::NbDev* dNb = reinterpret_cast<const mapdbtri::NbDev*>(p.up + oNb);
  const CallDev* dCalls = reinterpret_cast<const CallDev*>(p.up + oCalls);
  mapdbtri::SearchArgs sa;
  sa.R.rowPool = P.rowPool; sa.R.bowPool = reinterpret_cast<const int2*>(P.bowPool); sa.R.kps = kps; sa.R.rightX = P.rightX; sa.R.blockPool = P.blockPool;
  sa.k1 = hFirst->k1; sa.nq = (int)nq; sa.stereoOnly = stereoOnly ? 1 : 0; sa.nb = dNb;
  sa.qRange = p.qRange; sa.qFeat = p.qFeat; sa.qAngle = p.qAngle; sa.qInfo = p.qInfo;
  sa.heads = reinterpret_cast<unsigned*>(p.down + dHeads); sa.overflow = reinterpret_cast<int*>(p.down + dOvf);
  mapdbtri::GeometryArgs ga;
  ga.R = sa.R; ga.first = reinterpret_cast<const mapdbtri::FirstDev*>(p.up + oFirst); ga.nNb = nNb; ga.nq = (int)nq; ga.nbs = dNb;
  ga.depth = reinterpret_cast<const float*>(p.up + oDepth); ga.qFeat = p.qFeat; ga.assigned = p.assigned; ga.qInfo = p.qInfo;
  ga.matched = reinterpret_cast<int*>(p.down + dMatched); ga.x3d = reinterpret_cast<float*>(p.down + dX); ga.status = p.down + dSt;
  const bool prof = m->profiling;
  const size_t nEv = 3 + 2 * nn;
  if (prof)
    while (m->triEv.size() < nEv) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      m->triEv.push_back(e);
    }
  const unsigned qBlocks = (unsigned)((nq + mapdbtri::kThreads - 1) / mapdbtri::kThreads);
  for (int attempt = 0; attempt < 6; attempt++) {
    if (m->triPoolPerNb * nn > (size_t)INT32_MAX) { set_error("mapdb_create_new_points: a record pool of %zu entries, past INT32_MAX", m->triPoolPerNb * nn); return YDORB_ERR_CAPACITY; }
    if ((rc = m->pool.ensure(sizeof(uint32_t) * m->triPoolPerNb * nn))) return rc;
    sa.pool = m->pool.as<uint32_t>(); sa.poolPerNb = (unsigned)m->triPoolPerNb;
    HIPCHK(hipMemsetAsync(p.down + dMatched, 0xFF, 4 * nn * n1, s));
    HIPCHK(hipMemsetAsync(p.down + dX, 0, 12 * nn * n1, s));
    HIPCHK(hipMemsetAsync(p.down + dSt, YDORB_TRI_UNMATCHED, nn * n1, s));
    HIPCHK(hipMemsetAsync(p.down + dCount, 0, D.bytes - dCount, s));   // counts, heads, overflow word
    size_t ev = 0;
    if (nq > 0) {
      HIPCHK(hipMemsetAsync(p.assigned, 0xFF, 4 * nn * nq, s));
      if (prof) HIPCHK(hipEventRecord(m->triEv[ev++], s));
      hipLaunchKernelGGL(mapdbtri::k_mapdb_tri_join, dim3(qBlocks, nNb), dim3(mapdbtri::kThreads), 0, s, sa);
      hipLaunchKernelGGL(mapdbtri::k_mapdb_tri_gather, dim3((unsigned)((nq + 3) / 4), nNb), dim3(256), 0, s, sa);
      HIPCHK(hipGetLastError());
      if (prof) HIPCHK(hipEventRecord(m->triEv[ev++], s));
      for (int i = 0; i < nNb; i++) {
        if (!hNb[i].usable) continue;
        const int takenWords = (hNb[i].k2.n + 31) / 32;
        hipLaunchKernelGGL(k_resolve, dim3(1), dim3(64), 2 * sizeof(unsigned) * takenWords, s, dCalls + i, (const FrameDev*)nullptr, m->pool.as<uint32_t>(), takenWords);
        if (prof) HIPCHK(hipEventRecord(m->triEv[ev++], s));
        ga.nb = i;
        hipLaunchKernelGGL(mapdbtri::k_mapdb_tri_geometry, dim3(qBlocks), dim3(mapdbtri::kThreads), 0, s, ga);
        if (prof) HIPCHK(hipEventRecord(m->triEv[ev++], s));
      }
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(m->hDown.p, p.down, D.bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (*at<int>(m->hDown, dOvf) != 0) {
      const unsigned* heads = at<unsigned>(m->hDown, dHeads);
      size_t asked = 0;
      for (size_t i = 0; i < nn; i++) asked = std::max(asked, (size_t)heads[i]);
      m->triPoolPerNb = std::max(m->triPoolPerNb * 2, asked + 1024);
      continue;
    }
    if (prof && ev >= 2) {   // the chain's events alternate: after a resolve, after a geometry
      float ms = 0;
      if (hipEventElapsedTime(&ms, m->triEv[0], m->triEv[1]) == hipSuccess) m->triMs[TS_SEARCH] += ms;
      for (size_t e = 2; e < ev; e++)
        if (hipEventElapsedTime(&ms, m->triEv[e - 1], m->triEv[e]) == hipSuccess) m->triMs[e % 2 == 0 ? TS_RESOLVE : TS_GEOMETRY] += ms;
      m->triCalls++;
    }
    if (nn * n1) {
      std::memcpy(matched, at<void>(m->hDown, dMatched), 4 * nn * n1);
      std::memcpy(x3d, at<void>(m->hDown, dX), 12 * nn * n1);
      std::memcpy(status, at<void>(m->hDown, dSt), nn * n1);
    }
    std::memcpy(nMatches, at<void>(m->hDown, dCount), 4 * nn);
    for (size_t i = 0; i < nn; i++)
      for (size_t k = 0; k < n1; k++) nAccepted[i] += (status[i * n1 + k] & 15) == YDORB_TRI_ACCEPTED;
    return YDORB_OK;
  }
  set_error("mapdb_create_new_points: candidate record pool kept overflowing");
  return YDORB_ERR_CAPACITY;
}

int ydorb_matcher_create_points_times(ydorb_matcher_t* m, float* ms, int32_t* nCalls) {
  if (!m || !ms || !nCalls) return YDORB_ERR_INVALID_ARG;
  for (int i = 0; i < TS_COUNT; i++) ms[i] = m->triCalls ? (float)(m->triMs[i] / m->triCalls) : 0.f;
  *nCalls = m->triCalls;
  return YDORB_OK;
}

}  // extern "C"

// The one body of ydorb_mapdb_search_by_bow_keyframes (mode 4) and ydorb_mapdb_search_by_bow_frame (mode 3) over a resident map table
// (mapdb_bow_kernels.hip.h has the kernels and what each does).  The pairs are independent, so the join, the gather, the unchanged
// k_resolve (one workgroup per pair) and the emit each run once over all of them: four launches, one upload, one read-back and one
// synchronisation of the matcher's stream per attempt.  kfSlots: mode 4 the first keyframe at 0, then the nPairs second keyframes;
// mode 3 the nPairs keyframes.  The arguments have passed the entries' own checks.  The table's mutex is held from its sync to the end
// of the call, as in ydorb_mapdb_create_new_points; every return after the first launch, an error included, synchronises the
// matcher's stream first.  A set overflow word grows every pair's part of the pool to what the heads asked for and replays the call.
static int bowSearchResident(const char* who, ydorb_mapdb_t* db, ydorb_matcher_t* m, int mode, const int32_t* kfSlots, int32_t nPairs, int32_t nFirst,
                             const YdBowSide* frame, float ratio, int32_t checkOri, int32_t* matched, int32_t* point, int32_t* nMatches, uint8_t* pairStatus) {
  const size_t np = (size_t)nPairs, nKf = np + (mode == 4 ? 1 : 0), lead = mode == 4 ? 1 : 0;
  mapdb::ResidentBowPools P;
  std::vector<mapdb::ResidentTriSpans> spans(nKf);
  std::vector<uint8_t> kfStatus(nKf, 0);
  mapdb::ResidentLock lock;
  int rc;
  if ((rc = mapdb::lockResidentBow(db, m->device, kfSlots, (int32_t)nKf, nPairs, nFirst, P, spans.data(), kfStatus.data()))) return rc;
  lock.db = db;
  if (nPairs == 0) return YDORB_OK;
  const size_t nOut = (size_t)(mode == 4 ? nFirst : frame->n);
  int writer = -1;
  for (size_t i = 0; i < np; i++) {
    pairStatus[i] = (mode == 4 && kfStatus[0]) ? kfStatus[0] : kfStatus[i + lead];
    nMatches[i] = 0;
    if (!pairStatus[i] && writer < 0) writer = (int)i;
  }
  for (size_t o = 0; o < np * nOut; o++) { matched[o] = -1; point[o] = -1; }
  if (writer < 0 || nOut == 0) return YDORB_OK;
  static_assert(sizeof(mapdbbow::Spans) == sizeof(mapdb::ResidentTriSpans), "one layout");
  static_assert(sizeof(mapdb::BowRec) == sizeof(int2), "the frame's feature vector goes up as the resident ones lie");
  // where each pair's queries begin, the grid's extents and the largest B side
  std::vector<int32_t> qStart(np + 1, 0);
  size_t nq = 0, maxQ = 0, maxB = 0;
  if (mode == 4) {
    nq = (size_t)spans[0].bowLen;
    if (nq * np > (size_t)INT32_MAX) { set_error("%s: %zu queries, past INT32_MAX", who, nq * np); return YDORB_ERR_CAPACITY; }
    for (size_t i = 0; i <= np; i++) qStart[i] = (int32_t)(i * nq);
    maxQ = nq;
    for (size_t i = 0; i < np; i++) if (!pairStatus[i]) maxB = std::max(maxB, (size_t)spans[i + 1].n);
  } else {
    std::vector<int32_t> len(np);
    for (size_t i = 0; i < np; i++) { len[i] = spans[i].bowLen; if (!pairStatus[i]) maxQ = std::max(maxQ, (size_t)len[i]); }
    if (!mapdb::bowQueryStarts(len.data(), pairStatus, nPairs, qStart)) { set_error("%s: the keyframes' BoW spans hold more than INT32_MAX entries", who); return YDORB_ERR_CAPACITY; }
    maxB = nOut;
    if (np * nOut > (size_t)INT32_MAX) { set_error("%s: %zu output elements, past INT32_MAX", who, np * nOut); return YDORB_ERR_CAPACITY; }
  }
  const size_t nqAll = (size_t)qStart[np], nShared = mode == 4 ? nq : nqAll, nAssigned = mode == 4 ? nqAll : np * nOut;
  maxB = std::min<size_t>(maxB, 65535);   // a feature index of a BoW span lies below 65535 (mapdb_bow_host.h, checkBowFrame)
  std::vector<mapdb::BowRec> frameBow;
  if (mode == 3) mapdb::flattenFrameBow(frame->fv, frameBow);
  const size_t nfb = frameBow.size(), nf = mode == 3 ? (size_t)frame->n : 0;
  HIPCHK(hipSetDevice(m->device));
  struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{m->stream};   // before the mutex goes: see ydorb_mapdb_search_local_points
  Layout U;
  const size_t oPairs = U.add(sizeof(mapdbbow::PairDev) * np), oCalls = U.add(sizeof(CallDev) * np), oBow = U.add(sizeof(int2) * nfb),
               oKps = U.add(sizeof(YdKeyPoint) * nf), oDesc = U.add(32 * nf), oValid = U.add(mode == 3 && frame->valid ? nf : 0);
  Layout D;
  const size_t dMatched = D.add(4 * np * nOut), dPoint = D.add(4 * np * nOut), dCount = D.add(4 * np), dHeads = D.add(4 * np), dOvf = D.add(16);
  BowBatchPtrs p;
  if ((rc = m->hUp.ensure(U.bytes)) || (rc = m->hDown.ensure(D.bytes))) return rc;
  if ((rc = layOut(m->call, [&](void* base) { return layBowBatch(U.bytes, D.bytes, nqAll, nShared, nAssigned, base, p); }))) return rc;
  mapdbbow::PairDev* hp = at<mapdbbow::PairDev>(m->hUp, oPairs);
  CallDev* hc = at<CallDev>(m->hUp, oCalls);
  std::memset(hp, 0, sizeof(mapdbbow::PairDev) * np);
  std::memset(hc, 0, sizeof(CallDev) * np);
  if (mode == 3) {
    if (nfb) std::memcpy(at<void>(m->hUp, oBow), frameBow.data(), sizeof(int2) * nfb);
    std::memcpy(at<void>(m->hUp, oKps), frame->kps, sizeof(YdKeyPoint) * nf);
    std::memcpy(at<void>(m->hUp, oDesc), frame->desc, 32 * nf);
    if (frame->valid) std::memcpy(at<void>(m->hUp, oValid), frame->valid, nf);
  }
  const KeyPointDev* kps = reinterpret_cast<const KeyPointDev*>(P.tri.kps);
  for (size_t i = 0; i < np; i++) {
    mapdbbow::PairDev& N = hp[i];
    std::memcpy(&N.kf, &spans[i + lead], sizeof(mapdbbow::Spans));
    N.usable = pairStatus[i] == YDORB_BOW_PAIR_OK; N.qStart = qStart[i];
    CallDev& C = hc[i];   // no frame, query rows or taken flags, as in the flat search
    C.tkps = mode == 4 ? kps + N.kf.featStart : reinterpret_cast<const KeyPointDev*>(p.up + oKps);
    C.qAngle = p.qAngle + (mode == 4 ? 0 : qStart[i]);
    C.nq = !N.usable ? 0 : mode == 4 ? (int)nq : N.kf.bowLen;
    C.qInfo = p.qInfo + qStart[i]; C.matchQ = p.matchQ + qStart[i];
    C.assigned = p.assigned + (mode == 4 ? (size_t)qStart[i] : i * nOut);
    C.count = reinterpret_cast<int*>(p.down + dCount) + i;
    C.mode = mode; C.ratio = ratio; C.checkOri = checkOri;
  }
  hipStream_t s = m->stream;
  HIPCHK(hipMemcpyAsync(p.up, m->hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  mapdbbow::SearchArgs sa{};
  sa.R.rowPool = P.tri.rowPool; sa.R.bowPool = reinterpret_cast<const int2*>(P.tri.bowPool); sa.R.kps = kps; sa.R.blockPool = P.tri.blockPool;
  sa.R.bad = P.bad; sa.R.pointCap = P.pointCap;
  sa.mode = mode; sa.nq = (int)maxQ; sa.nOut = (int)nOut; sa.writer = writer;
  if (mode == 4) std::memcpy(&sa.first, &spans[0], sizeof(mapdbbow::Spans));
  sa.pairs = reinterpret_cast<const mapdbbow::PairDev*>(p.up + oPairs);
  if (mode == 3) {
    sa.frameBow = reinterpret_cast<const int2*>(p.up + oBow); sa.frameBowLen = (int)nfb;
    sa.frameDesc = p.up + oDesc; sa.frameValid = frame->valid ? p.up + oValid : nullptr;
  }
  sa.qRange = p.qRange; sa.qFeat = p.qFeat; sa.qAngle = p.qAngle; sa.qInfo = p.qInfo; sa.assigned = p.assigned;
  sa.matched = reinterpret_cast<int*>(p.down + dMatched); sa.point = reinterpret_cast<int*>(p.down + dPoint);
  sa.heads = reinterpret_cast<unsigned*>(p.down + dHeads); sa.overflow = reinterpret_cast<int*>(p.down + dOvf);
  const CallDev* dCalls = reinterpret_cast<const CallDev*>(p.up + oCalls);
  const bool prof = m->profiling;
  if (prof)
    for (auto& e : m->bowEv)
      if (!e) HIPCHK(hipEventCreate(&e));
  const int takenWords = (int)((maxB + 31) / 32);
  const size_t emitN = mode == 4 ? nq : nOut;
  YdBowSearchStats& st = m->bowStats;
  st.calls++;
  st.launches = 0; st.synchronisations = 0; st.bytes_up = (int64_t)U.bytes; st.bytes_down = 0;
  for (int attempt = 0; attempt < 6; attempt++) {
    st.attempts++;
    if (m->triPoolPerNb * np > (size_t)INT32_MAX) { set_error("%s: a record pool of %zu entries, past INT32_MAX", who, m->triPoolPerNb * np); return YDORB_ERR_CAPACITY; }
    if ((rc = m->pool.ensure(sizeof(uint32_t) * m->triPoolPerNb * np))) return rc;
    sa.pool = m->pool.as<uint32_t>(); sa.poolPerPair = (unsigned)m->triPoolPerNb;
    HIPCHK(hipMemsetAsync(p.down + dMatched, 0xFF, dCount - dMatched, s));     // both dense outputs
    HIPCHK(hipMemsetAsync(p.down + dCount, 0, D.bytes - dCount, s));           // counts, heads, overflow word
    HIPCHK(hipMemsetAsync(p.assigned, 0xFF, 4 * nAssigned, s));
    if (prof) HIPCHK(hipEventRecord(m->bowEv[0], s));
    hipLaunchKernelGGL(mapdbbow::k_mapdb_bow_join, dim3((unsigned)((maxQ + mapdbbow::kThreads - 1) / mapdbbow::kThreads), nPairs), dim3(mapdbbow::kThreads), 0, s, sa);
    hipLaunchKernelGGL(mapdbbow::k_mapdb_bow_gather, dim3((unsigned)((maxQ + 3) / 4), nPairs), dim3(256), 0, s, sa);
    if (prof) HIPCHK(hipEventRecord(m->bowEv[1], s));
    hipLaunchKernelGGL(k_resolve, dim3(nPairs), dim3(64), 2 * sizeof(unsigned) * takenWords, s, dCalls, (const FrameDev*)nullptr, m->pool.as<uint32_t>(), takenWords);
    if (prof) HIPCHK(hipEventRecord(m->bowEv[2], s));
    hipLaunchKernelGGL(mapdbbow::k_mapdb_bow_emit, dim3((unsigned)((emitN + mapdbbow::kThreads - 1) / mapdbbow::kThreads), nPairs), dim3(mapdbbow::kThreads), 0, s, sa);
    HIPCHK(hipGetLastError());
    if (prof) HIPCHK(hipEventRecord(m->bowEv[3], s));
    HIPCHK(hipMemcpyAsync(m->hDown.p, p.down, D.bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    st.launches += 4; st.synchronisations += 1; st.bytes_down += (int64_t)D.bytes;
    if (*at<int>(m->hDown, dOvf) != 0) {
      const unsigned* heads = at<unsigned>(m->hDown, dHeads);
      size_t asked = 0;
      for (size_t i = 0; i < np; i++) asked = std::max(asked, (size_t)heads[i]);
      m->triPoolPerNb = std::max(m->triPoolPerNb * 2, asked + 1024);
      continue;
    }
    if (prof) {
      float ms = 0;
      for (int e = 0; e < BS_COUNT; e++)
        if (hipEventElapsedTime(&ms, m->bowEv[e], m->bowEv[e + 1]) == hipSuccess) m->bowMs[e] += ms;
      st.profiled_calls++;
    }
    std::memcpy(matched, at<void>(m->hDown, dMatched), 4 * np * nOut);
    std::memcpy(point, at<void>(m->hDown, dPoint), 4 * np * nOut);
    std::memcpy(nMatches, at<void>(m->hDown, dCount), 4 * np);
    return YDORB_OK;
  }
  set_error("%s: candidate record pool kept overflowing", who);
  return YDORB_ERR_CAPACITY;
}

extern "C" {

int ydorb_mapdb_search_by_bow_keyframes(ydorb_mapdb_t* db, ydorb_matcher_t* m, int32_t firstKfSlot, const int32_t* secondKfSlots, int32_t nSecond, float ratio,
                                        int32_t checkOri, int32_t nFirst, int32_t* matchedSecond, int32_t* matchedPoint, int32_t* nMatches, uint8_t* pairStatus) {
  const char* who = "mapdb_search_by_bow_keyframes";
  if (!db || !m) { set_error("%s: null handle", who); return YDORB_ERR_INVALID_ARG; }
  if (nSecond < 0) { set_error("%s: negative number of second keyframes: %d", who, nSecond); return YDORB_ERR_INVALID_ARG; }
  if (nFirst < 0) { set_error("%s: negative n_first: %d", who, nFirst); return YDORB_ERR_INVALID_ARG; }
  if (nSecond > 65535) { set_error("%s: %d second keyframes, more than 65535", who, nSecond); return YDORB_ERR_UNSUPPORTED; }
  if (nSecond > 0 && (!secondKfSlots || !nMatches || !pairStatus || (nFirst > 0 && (!matchedSecond || !matchedPoint)))) {
    set_error("%s: null second_kf_slots, matched_second, matched_point, n_matches or pair_status", who);
    return YDORB_ERR_INVALID_ARG;
  }
  if (!std::isfinite(ratio)) { set_error("%s: ratio is not finite", who); return YDORB_ERR_INVALID_ARG; }
  std::vector<int32_t> kfSlots((size_t)nSecond + 1);
  kfSlots[0] = firstKfSlot;
  for (int32_t i = 0; i < nSecond; i++) kfSlots[(size_t)i + 1] = secondKfSlots[i];
  return bowSearchResident(who, db, m, 4, kfSlots.data(), nSecond, nFirst, nullptr, ratio, checkOri ? 1 : 0, matchedSecond, matchedPoint, nMatches, pairStatus);
}

int ydorb_mapdb_search_by_bow_frame(ydorb_mapdb_t* db, ydorb_matcher_t* m, const int32_t* kfSlots, int32_t nKf, const YdBowSide* frame, float ratio,
                                    int32_t checkOri, int32_t* matchedKfFeature, int32_t* matchedPoint, int32_t* nMatches, uint8_t* pairStatus) {
  const char* who = "mapdb_search_by_bow_frame";
  if (!db || !m) { set_error("%s: null handle", who); return YDORB_ERR_INVALID_ARG; }
  if (nKf < 0) { set_error("%s: negative number of keyframes: %d", who, nKf); return YDORB_ERR_INVALID_ARG; }
  if (nKf > 65535) { set_error("%s: %d keyframes, more than 65535", who, nKf); return YDORB_ERR_UNSUPPORTED; }
  std::string err;
  if (!mapdb::checkBowFrame(frame, err)) { set_error("%s: %s", who, err.c_str()); return YDORB_ERR_INVALID_ARG; }
  if (nKf > 0 && (!kfSlots || !nMatches || !pairStatus || (frame->n > 0 && (!matchedKfFeature || !matchedPoint)))) {
    set_error("%s: null kf_slots, matched_kf_feature, matched_point, n_matches or pair_status", who);
    return YDORB_ERR_INVALID_ARG;
  }
  if (!std::isfinite(ratio)) { set_error("%s: ratio is not finite", who); return YDORB_ERR_INVALID_ARG; }
  return bowSearchResident(who, db, m, 3, kfSlots, nKf, -1, frame, ratio, checkOri ? 1 : 0, matchedKfFeature, matchedPoint, nMatches, pairStatus);
}

int ydorb_matcher_bow_search_stats(ydorb_matcher_t* m, YdBowSearchStats* stats) {
  if (!m || !stats) { set_error("matcher_bow_search_stats: null handle or stats"); return YDORB_ERR_INVALID_ARG; }
  *stats = m->bowStats;
  stats->pool_per_pair = (int64_t)m->triPoolPerNb;
  for (int i = 0; i < BS_COUNT; i++) stats->ms[i] = stats->profiled_calls ? (float)(m->bowMs[i] / stats->profiled_calls) : 0.f;
  return YDORB_OK;
}

int ydorb_fuse_search(ydorb_matcher_t* m, const YdFrameView* fv, const YdQuery* queries, const uint8_t* qdesc, int32_t nq,
                      const float* invSigma2, int32_t nLevels, int32_t* best, int32_t* nFound) {
  return ydorb_window_search(m, fv, queries, qdesc, nq, invSigma2, nLevels, 50, best, nFound);
}

int ydorb_window_search(ydorb_matcher_t* m, const YdFrameView* fv, const YdQuery* queries, const uint8_t* qdesc, int32_t nq,
                        const float* invSigma2, int32_t nLevels, int32_t maxDist, int32_t* best, int32_t* nFound) {
  if (!m || !validFrameView(fv) || !nFound || nq < 0 || maxDist < 0 || maxDist > 256 || (nq > 0 && (!queries || !qdesc || !best)) || !invSigma2 || nLevels < 1 ||
      nLevels > 8) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  for (int q = 0; q < nq; q++) best[q] = -1;
  *nFound = 0;
  for (int i = 0; i < fv->n; i++)
    if (fv->kps[i].octave < 0 || fv->kps[i].octave >= nLevels) { set_error("keyframe feature %d: octave %d outside the %d-level table", i, fv->kps[i].octave, nLevels); return YDORB_ERR_INVALID_ARG; }
  return searchProjectionImpl(m, 6, fv, queries, qdesc, nq, 0.f, maxDist, 0, nullptr, nullptr, nFound, nullptr, invSigma2, nLevels, best);
}

int ydorb_frame_keypoints_in_area(ydorb_matcher_t* m, const YdFrameView* fv, float x, float y, float r, int32_t minLevel, int32_t maxLevel,
                                  int32_t* outIdx, int32_t cap, int32_t* nOut) {
  if (!m || !validFrameView(fv) || !nOut || (cap > 0 && !outIdx)) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  *nOut = 0;
  if (fv->n == 0) return YDORB_OK;
  YdQuery q{};
  q.u = x; q.v = y; q.r = r; q.min_level = minLevel; q.max_level = maxLevel; q.flags = 1;
  uint8_t zero[32] = {0};
  std::vector<uint32_t> rec;
  int dummy = 0;
  int rc = searchProjectionImpl(m, 2, fv, &q, zero, 1, 0.f, 0, 0, nullptr, nullptr, &dummy, &rec);
  if (rc) return rc;
  if ((int)rec.size() > cap) { set_error("%zu candidates, capacity %d", rec.size(), cap); return YDORB_ERR_CAPACITY; }
  for (size_t i = 0; i < rec.size(); i++) outIdx[i] = (int)(rec[i] & 0xFFFFu);
  *nOut = (int)rec.size();
  return YDORB_OK;
}

int ydorb_search_by_bow(ydorb_matcher_t* m, int32_t mode, const YdBowSide* A, const YdBowSide* B, float ratio, int32_t checkOri, int32_t* out,
                        int32_t* nMatches) {
  if (!m || !A || !B || !out || !nMatches || (mode != 3 && mode != 4) || A->n < 0 || B->n < 0 || (A->n > 0 && (!A->kps || !A->desc || !A->valid)) ||
      (B->n > 0 && (!B->kps || !B->desc)) || (mode == 4 && B->n > 0 && !B->valid)) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(m->device));
  const int nOutLen = mode == 3 ? B->n : A->n;
  for (int i = 0; i < nOutLen; i++) out[i] = -1;
  *nMatches = 0;
  if (A->n == 0 || B->n == 0) return YDORB_OK;
  if (B->n > 65535) { set_error("more than 65535 features per frame are not supported"); return YDORB_ERR_UNSUPPORTED; }
  const BowJob J{{A->kps, A->desc, A->n, &A->fv, A->valid, nullptr}, {B->kps, B->desc, B->n, &B->fv, mode == 4 ? B->valid : nullptr, nullptr}, mode, ratio, checkOri, {}};
  std::vector<int> qFeat, res;
  const int rc = bowSearch(m, J, qFeat, res, nMatches);
  if (rc || qFeat.empty()) return rc;
  if (mode == 3) {
    for (int i = 0; i < B->n; i++) out[i] = res[i] >= 0 ? qFeat[res[i]] : -1;
  } else {
    for (size_t q = 0; q < qFeat.size(); q++) out[qFeat[q]] = res[q];
  }
  return YDORB_OK;
}

int ydorb_search_for_triangulation(ydorb_matcher_t* m, const YdTriSide* A, const YdTriSide* B, const float* F, float ex, float ey,
                                   const float* sfB, const float* sf2B, int32_t nLevels, int32_t stereoOnly, int32_t checkOri, int32_t* out,
                                   int32_t* nMatches) {
  if (!m || !A || !B || !F || !sfB || !sf2B || !out || !nMatches || nLevels < 1 || nLevels > 8 || A->n < 0 || B->n < 0 ||
      (A->n > 0 && (!A->kps || !A->desc || !A->right_x || !A->has_map_point)) || (B->n > 0 && (!B->kps || !B->desc || !B->right_x || !B->has_map_point))) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(m->device));
  for (int i = 0; i < A->n; i++) out[i] = -1;
  *nMatches = 0;
  if (A->n == 0 || B->n == 0) return YDORB_OK;
  if (B->n > 65535) { set_error("more than 65535 features per frame are not supported"); return YDORB_ERR_UNSUPPORTED; }
  for (int i = 0; i < B->n; i++)
    if (B->kps[i].octave < 0 || B->kps[i].octave >= nLevels) { set_error("second keyframe: octave %d outside the %d-level tables", B->kps[i].octave, nLevels); return YDORB_ERR_INVALID_ARG; }
  // eligibility (:491-492, :497-500) is static: no map point yet, and a good stereo coordinate when only stereo points are wanted
  std::vector<uint8_t> goodA(A->n), goodB(B->n), eligibleA(A->n), validB(B->n);
  for (int i = 0; i < A->n; i++) { goodA[i] = A->right_x[i] >= 0; eligibleA[i] = !A->has_map_point[i] && (!stereoOnly || goodA[i]); }
  for (int i = 0; i < B->n; i++) { goodB[i] = B->right_x[i] >= 0; validB[i] = !B->has_map_point[i] && (!stereoOnly || goodB[i]); }
  BowJob J{{A->kps, A->desc, A->n, &A->fv, eligibleA.data(), goodA.data()}, {B->kps, B->desc, B->n, &B->fv, validB.data(), goodB.data()}, 5, 0.f, checkOri, {}};
  J.geom.tri = 1;
  for (int i = 0; i < 9; i++) J.geom.F[i] = F[i];
  J.geom.ex = ex; J.geom.ey = ey;
  for (int i = 0; i < 8; i++) { J.geom.sfB[i] = i < nLevels ? sfB[i] : 0.f; J.geom.sf2B[i] = i < nLevels ? sf2B[i] : 0.f; }
  std::vector<int> qFeat, res;
  const int rc = bowSearch(m, J, qFeat, res, nMatches);
  if (rc) return rc;
  for (size_t q = 0; q < qFeat.size(); q++) out[qFeat[q]] = res[q];
  return YDORB_OK;
}

int ydorb_stereo_matches(ydorb_matcher_t* m, const YdStereoSide* L, const YdStereoSide* R, int32_t nPairs, float bf, float b, int32_t flags,
                         float* rightX, float* depth, int32_t* nKept, int32_t* status, void* stream) {
  if (!m || !L || !R || !L->extractor || !R->extractor || !L->kps || !L->desc || !L->n || !R->kps || !R->desc || !R->n || !rightX || !depth ||
      nPairs < 1 || L->cap < 1 || R->cap < 1 || !(bf > 0.f) || !(b > 0.f)) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  if (R->cap > kStereoMaxRight) { set_error("right cap %d > %d", R->cap, kStereoMaxRight); return YDORB_ERR_CAPACITY; }
  PyramidView vl, vr;
  int rc;
  if ((rc = extractor_pyramid_view(L->extractor, &vl)) || (rc = extractor_pyramid_view(R->extractor, &vr))) return rc;
  if (vl.device != m->device || vr.device != m->device) { set_error("extractors and matcher live on different devices"); return YDORB_ERR_INVALID_ARG; }
  if (vl.nLevels != vr.nLevels) { set_error("left and right pyramids differ in depth"); return YDORB_ERR_INVALID_ARG; }
  for (int l = 0; l < vl.nLevels; l++)
    if (vl.w[l] != vr.w[l] || vl.h[l] != vr.h[l] || vl.scale[l] != vr.scale[l]) { set_error("left and right pyramids differ at level %d", l); return YDORB_ERR_INVALID_ARG; }
  const int lastL = L->first_frame + (nPairs - 1) * L->frame_step, lastR = R->first_frame + (nPairs - 1) * R->frame_step;
  if (L->first_frame < 0 || lastL < 0 || L->first_frame >= vl.frames || lastL >= vl.frames || R->first_frame < 0 || lastR < 0 ||
      R->first_frame >= vr.frames || lastR >= vr.frames) {
    set_error("pair frames outside the extractors' last call (%d / %d frames)", vl.frames, vr.frames);
    return YDORB_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(m->device));
  const bool dev = flags & YDORB_STEREO_DEVICE_POINTERS;
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  const size_t nl = (size_t)nPairs * L->cap, nr = (size_t)nPairs * R->cap;
  StereoPtrs sp;
  if ((rc = layOut(m->stereo, [&](void* base) { return layStereo(nPairs, dev ? 0 : nl, dev ? 0 : nr, base, sp); }))) return rc;
  StereoDev P{};
  if (dev) {
    P.kpsL = reinterpret_cast<const KeyPointDev*>(L->kps); P.descL = L->desc; P.nL = L->n;
    P.kpsR = reinterpret_cast<const KeyPointDev*>(R->kps); P.descR = R->desc; P.nR = R->n;
    P.rightX = rightX; P.depth = depth;
  } else {
    // the pyramids must be complete before the kernels read them from another stream
    HIPCHK(hipStreamSynchronize((hipStream_t)vl.stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)vr.stream));
    HIPCHK(hipMemcpyAsync(sp.kpsL, L->kps, sizeof(YdKeyPoint) * nl, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sp.descL, L->desc, 32 * nl, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sp.kpsR, R->kps, sizeof(YdKeyPoint) * nr, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sp.descR, R->desc, 32 * nr, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sp.nL, L->n, sizeof(int) * nPairs, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sp.nR, R->n, sizeof(int) * nPairs, hipMemcpyHostToDevice, s));
    P.kpsL = sp.kpsL; P.descL = sp.descL; P.nL = sp.nL;
    P.kpsR = sp.kpsR; P.descR = sp.descR; P.nR = sp.nR;
    P.rightX = sp.rightX; P.depth = sp.depth;
  }
  for (int l = 0; l < vl.nLevels; l++) {
    P.pyrL[l] = vl.roi[l]; P.pyrR[l] = vr.roi[l];
    P.w[l] = vl.w[l]; P.h[l] = vl.h[l]; P.pitchL[l] = vl.pitch[l]; P.pitchR[l] = vr.pitch[l];
    P.scale[l] = vl.scale[l]; P.invScale[l] = vl.invScale[l];
  }
  P.frameStrideL = vl.frameStride; P.frameStrideR = vr.frameStride;
  P.capL = L->cap; P.capR = R->cap; P.frameL0 = L->first_frame; P.frameLStep = L->frame_step; P.frameR0 = R->first_frame; P.frameRStep = R->frame_step;
  P.nLevels = vl.nLevels; P.flags = flags; P.bf = bf; P.maxD = bf / b;   // :382
  P.counters = sp.counters; P.keptOut = sp.kept; P.statusOut = sp.status;
  // replay form: the right-keypoint table (8 bytes each) + the index sorted by first band row (row starts, fill cursors, 2 bytes per keypoint)
  size_t ldsReplay = (size_t)R->cap * 8;
  {
    const size_t bytes = (size_t)R->cap * 8 + sizeof(int) * (2 * (size_t)vl.h[0] + 1) + 2 * (size_t)R->cap + 16;
    const bool noLists = getenv("YDORB_STEREO_NO_ROW_LISTS") != nullptr;   // diagnostic: force the scan form (tests compare the two)
    if (!noLists && !(flags & YDORB_STEREO_INDEX_BY_KEYPOINT) && bytes <= 120 * 1024 && vl.h[0] < 4095) { P.rowLists = 1; ldsReplay = bytes; }
  }
  // P travels as a kernel argument: an asynchronous copy out of pageable host memory makes the host wait for everything queued on
  // the stream before it - here the extraction the association waits for - and a caller that pipelines steps would run in lock step
  HIPCHK(hipMemsetAsync(sp.counters, 0, sizeof(int) * 4 * nPairs, s));
  HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(P.rightX), 0xBF800000u, nl, s));   // -1.0f, :363-364
  HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(P.depth), 0xBF800000u, nl, s));
  const size_t lds = (size_t)R->cap * 8;
  const StereoDev& dP = P;
  if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_stereo<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (ldsReplay > 48 * 1024) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_stereo<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsReplay));
  if (flags & YDORB_STEREO_INDEX_BY_KEYPOINT)
    hipLaunchKernelGGL(k_stereo<false>, dim3((L->cap + kStereoChunk - 1) / kStereoChunk, nPairs), dim3(256), lds, s, dP, 0, 0);
  else {
    // slices of the serial walk (see k_stereo): a batch keeps every launch below ~2 ms; a single pair (the adapter's call) is one launch.
    // YDORB_STEREO_SLICE: a per-call diagnostic like YDORB_STEREO_NO_ROW_LISTS (tests walk the same pairs in slices of their choosing)
    const char* sliceStr = getenv("YDORB_STEREO_SLICE");
    const int sliceEnv = sliceStr ? atoi(sliceStr) : 0;
    const int slice = sliceEnv > 0 ? sliceEnv : (nPairs >= 8 ? 1024 : L->cap);
    for (int k0 = 0; k0 < L->cap; k0 += slice)
      hipLaunchKernelGGL(k_stereo<true>, dim3(1, nPairs), dim3(256), ldsReplay, s, dP, k0, std::min(k0 + slice, L->cap));
  }
  hipLaunchKernelGGL(k_stereo_outliers, dim3(nPairs), dim3(256), 0, s, P);
  HIPCHK(hipGetLastError());
  if (dev) {
    if (nKept) HIPCHK(hipMemcpyAsync(nKept, P.keptOut, sizeof(int) * nPairs, hipMemcpyDeviceToDevice, s));
    if (status) HIPCHK(hipMemcpyAsync(status, P.statusOut, sizeof(int) * nPairs, hipMemcpyDeviceToDevice, s));
    return YDORB_OK;
  }
  HIPCHK(hipMemcpyAsync(rightX, P.rightX, sizeof(float) * nl, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(depth, P.depth, sizeof(float) * nl, hipMemcpyDeviceToHost, s));
  if (nKept) HIPCHK(hipMemcpyAsync(nKept, P.keptOut, sizeof(int) * nPairs, hipMemcpyDeviceToHost, s));
  if (status) HIPCHK(hipMemcpyAsync(status, P.statusOut, sizeof(int) * nPairs, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return YDORB_OK;
}

int ydorb_match_pairs_device(ydorb_matcher_t* m, const YdFrameSetDev* Q, const YdFrameSetDev* T, const int32_t* pairs, int32_t nCalls,
                             int32_t width, int32_t height, float th, const float* scaleFactors, int32_t nLevels, const float* d_affine,
                             int32_t checkOri, int32_t* d_assigned, int32_t* d_counts, void* stream) {
  if (!m || !Q || !T || !pairs || !Q->d_kps || !Q->d_desc || !Q->d_n || !T->d_kps || !T->d_desc || !T->d_n || !d_assigned || !d_counts || !scaleFactors ||
      Q->cap < 1 || Q->cap > 65535 || T->cap != Q->cap || Q->n_frames < 1 || T->n_frames < 1 || nCalls < 1 || nLevels < 1 || nLevels > 8 || width < 1 ||
      height < 1) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  for (int c = 0; c < nCalls; c++)
    if (pairs[2 * c] < 0 || pairs[2 * c] >= Q->n_frames || pairs[2 * c + 1] < 0 || pairs[2 * c + 1] >= T->n_frames) {
      set_error("pair %d references a frame out of range", c);
      return YDORB_ERR_INVALID_ARG;
    }
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  // grids are built only for the frames that appear as a pair's TARGET: on the multi-GPU path T is the all-gathered set (world x F
  // frames) of which this rank searches its own F
  std::vector<int> tmap(T->n_frames, -1);
  std::vector<int> tused;
  for (int c = 0; c < nCalls; c++) {
    const int tf = pairs[2 * c + 1];
    if (tmap[tf] < 0) { tmap[tf] = (int)tused.size(); tused.push_back(tf); }
  }
  auto& B = m->batch;
  const int cap = Q->cap, nFrames = (int)tused.size();
  const size_t poolPerCall = (size_t)cap * kSlot + (size_t)cap * B.ovfPerKeypoint;  // fixed slots + overflow region (records of queries with > kSlot candidates)
  BatchPtrs p;
  const size_t had = B.arena.cap;
  const int rc = layOut(B.arena, [&](void* base) { return layBatch(cap, nCalls, nFrames, poolPerCall, base, p); });
  if (B.arena.cap != had) B.hFrames.clear();
  if (rc) return rc;
  std::vector<FrameDev> hf(nFrames);
  std::vector<CallDev> hc(nCalls);
  const float minX = 0.f, minY = 0.f, maxX = (float)width, maxY = (float)height;  // Frame::computeImageBounds without distortion
  for (int f = 0; f < nFrames; f++) {
    const int tf = tused[f];
    FrameDev& F = hf[f];
    F.kps = reinterpret_cast<const KeyPointDev*>(T->d_kps) + (size_t)tf * cap; F.desc = T->d_desc + (size_t)tf * cap * 32; F.rightX = nullptr;
    F.nPtr = T->d_n + tf; F.n = 0; F.minX = minX; F.minY = minY;
    F.gridWInv = static_cast<float>(kGridCols) / (maxX - minX); F.gridHInv = static_cast<float>(kGridRows) / (maxY - minY);
    F.cellStart = p.cellStart + (size_t)f * (kGridCells + 1); F.cellIdx = p.cellIdx + (size_t)f * cap;
    F.sortedKp = p.sortedKp + (size_t)f * cap; F.sortedDesc = p.sortedDesc + (size_t)f * cap * 32;
  }
  for (int c = 0; c < nCalls; c++) {
    const int qf = pairs[2 * c], tf = tmap[pairs[2 * c + 1]];
    CallDev& C = hc[c];
    C.frame = tf; C.tkps = hf[tf].kps; C.qAngle = nullptr; C.queries = p.queries + (size_t)c * cap;
    C.qkps = reinterpret_cast<const KeyPointDev*>(Q->d_kps) + (size_t)qf * cap;
    C.qdesc = Q->d_desc + (size_t)qf * cap * 32; C.nqPtr = Q->d_n + qf; C.nq = 0; C.qInfo = p.qInfo + (size_t)c * cap;
    C.qPre = p.qPre + (size_t)c * cap; C.takenClear = 1;
    C.taken = p.taken + (size_t)c * cap; C.assigned = d_assigned + (size_t)c * cap; C.matchQ = p.matchQ + (size_t)c * cap;
    C.count = d_counts + c; C.mode = 1; C.ratio = 0.9f; C.orbDist = 0; C.checkOri = checkOri;
  }
  float hsf[8] = {0};
  for (int l = 0; l < nLevels; l++) hsf[l] = scaleFactors[l];
  const bool same = p.frames == B.at.frames && p.calls == B.at.calls && p.sf == B.at.sf && p.ident == B.at.ident &&
                    B.hFrames.size() == hf.size() && B.hCalls.size() == hc.size() && !memcmp(B.hFrames.data(), hf.data(), sizeof(FrameDev) * hf.size()) &&
                    !memcmp(B.hCalls.data(), hc.data(), sizeof(CallDev) * hc.size()) && !memcmp(B.hSf, hsf, sizeof(hsf)) && B.hIdentAffine == !d_affine;
  if (!same) {
    HIPCHK(hipStreamSynchronize(s));
    B.hFrames.clear();   // nothing is cached until all four copies are through
    HIPCHK(hipMemcpy(p.frames, hf.data(), sizeof(FrameDev) * nFrames, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p.calls, hc.data(), sizeof(CallDev) * nCalls, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p.sf, hsf, sizeof(hsf), hipMemcpyHostToDevice));
    if (!d_affine) {
      std::vector<float> ident((size_t)6 * nCalls, 0.f);
      for (int c = 0; c < nCalls; c++) { ident[6 * c] = 1.f; ident[6 * c + 4] = 1.f; }
      HIPCHK(hipMemcpy(p.ident, ident.data(), sizeof(float) * ident.size(), hipMemcpyHostToDevice));
    }
    B.hFrames.swap(hf);
    B.hCalls.swap(hc);
    memcpy(B.hSf, hsf, sizeof(hsf));
    B.hIdentAffine = !d_affine;
    B.at = p;
  }
  const float* aff = d_affine ? d_affine : p.ident;
  const bool prof = m->profiling;
  collect(m);
  // per-call pool heads, taken flags and the all -1 assignment are written by k_queries_from_keypoints (the overflow status, word [1] of
  // the batch status, is sticky until synchronize reads it)
  int* const ovf = B.status.as<int>() + 1;
  if (prof) HIPCHK(hipEventRecord(m->ev[0], s));
  hipLaunchKernelGGL(k_queries_from_keypoints, dim3((cap + 255) / 256, nCalls), dim3(256), 0, s, p.calls, cap, aff, th, p.sf, nLevels, minX, maxX, minY, maxY,
                     p.heads);
  { const int rcg = launchGridBuild(nFrames, cap, s, p.frames); if (rcg) return rcg; }
  if (prof) HIPCHK(hipEventRecord(m->ev[1], s));
  hipLaunchKernelGGL(k_gather_projection, dim3((cap + 4 * kGatherQpw - 1) / (4 * kGatherQpw), nCalls), dim3(256), 0, s, p.calls, p.frames, cap, p.pool, p.heads,
                     (unsigned)poolPerCall, ovf);
  if (prof) HIPCHK(hipEventRecord(m->ev[2], s));
  const int takenWords = (cap + 31) / 32;
  hipLaunchKernelGGL(k_resolve, dim3(nCalls), dim3(64), 2 * sizeof(unsigned) * takenWords, s, p.calls, p.frames, p.pool, takenWords);
  if (prof) { HIPCHK(hipEventRecord(m->ev[3], s)); m->evPending = true; }
  HIPCHK(hipGetLastError());
  return YDORB_OK;
}

int ydorb_match_consecutive_device(ydorb_matcher_t* m, const YdKeyPoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int32_t cap,
                                   int32_t nFrames, int32_t width, int32_t height, float th, const float* scaleFactors, int32_t nLevels,
                                   const float* d_affine, int32_t checkOri, int32_t* d_assigned, int32_t* d_counts, void* stream) {
  if (!m || nFrames < 2) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  const YdFrameSetDev S{d_kps, d_desc, d_n, nFrames, cap};
  std::vector<int32_t> pairs((size_t)2 * (nFrames - 1));
  for (int c = 0; c < nFrames - 1; c++) { pairs[2 * c] = c; pairs[2 * c + 1] = c + 1; }
  return ydorb_match_pairs_device(m, &S, &S, pairs.data(), nFrames - 1, width, height, th, scaleFactors, nLevels, d_affine, checkOri, d_assigned,
                                  d_counts, stream);
}

int ydorb_hamming_topk(ydorb_matcher_t* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, const int32_t* candOffsets,
                       const int32_t* candIdx, YdMatch2* out) {
  static_assert(sizeof(YdMatch2) == sizeof(TopkOut), "YdMatch2 layout");
  if (!m || nq < 0 || nt < 0 || nt > 65535 || (nq && (!q || !out)) || (nt && !t) || ((candOffsets == nullptr) != (candIdx == nullptr))) {
    set_error("invalid argument");
    return YDORB_ERR_INVALID_ARG;
  }
  if (nq == 0) return YDORB_OK;
  int rc = require_device(m->device);
  if (rc) return rc;
  HIPCHK(hipSetDevice(m->device));
  size_t nCand = 0;
  if (candOffsets) {
    if (candOffsets[0] != 0) { set_error("cand_offsets[0] must be 0"); return YDORB_ERR_INVALID_ARG; }
    for (int i = 0; i < nq; i++) {
      const int n = candOffsets[i + 1] - candOffsets[i];
      if (n < 0 || n > 65535) { set_error("candidate list %d has %d entries (0..65535 supported)", i, n); return YDORB_ERR_INVALID_ARG; }
    }
    nCand = (size_t)candOffsets[nq];
  }
  hipStream_t s = m->stream;
  RowsPtrs r;
  if ((rc = layOut(m->call, [&](void* base) { return layRows(nq, std::max(nt, 1), (size_t)nq + 1, std::max<size_t>(nCand, 1), 0, nq, base, r); }))) return rc;
  HIPCHK(hipMemcpyAsync(r.a, q, (size_t)32 * nq, hipMemcpyHostToDevice, s));
  if (nt) HIPCHK(hipMemcpyAsync(r.b, t, (size_t)32 * nt, hipMemcpyHostToDevice, s));
  if (candOffsets) {
    HIPCHK(hipMemcpyAsync(r.offsets, candOffsets, sizeof(int) * ((size_t)nq + 1), hipMemcpyHostToDevice, s));
    if (nCand) HIPCHK(hipMemcpyAsync(r.idx, candIdx, sizeof(int) * nCand, hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(k_topk_csr, dim3((nq + 3) / 4), dim3(256), 0, s, r.a, nq, r.b, nt, candOffsets ? r.offsets : nullptr, candOffsets ? r.idx : nullptr, r.top);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, r.top, sizeof(TopkOut) * (size_t)nq, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return YDORB_OK;
}

int ydorb_hamming_topk_device(ydorb_matcher_t* m, const uint8_t* d_qdesc, const int32_t* d_nq, const uint8_t* d_tdesc, const int32_t* d_nt, int32_t cap,
                              int32_t nPairs, YdMatch2* d_out, void* stream) {
  if (!m || !d_qdesc || !d_nq || !d_tdesc || !d_nt || !d_out || cap < 1 || cap > 65535 || nPairs < 1) { set_error("invalid argument"); return YDORB_ERR_INVALID_ARG; }
  int rc = require_device(m->device);
  if (rc) return rc;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  hipLaunchKernelGGL(k_topk_allpairs, dim3((cap + 255) / 256, nPairs), dim3(256), 0, s, d_qdesc, d_nq, (size_t)cap * 32, d_tdesc, d_nt, (size_t)cap * 32, cap,
                     reinterpret_cast<TopkOut*>(d_out));
  HIPCHK(hipGetLastError());
  return YDORB_OK;
}

int ydorb_matcher_synchronize(ydorb_matcher_t* m) {
  if (!m) { set_error("null handle"); return YDORB_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipDeviceSynchronize());
  collect(m);
  if (Mem& st = m->batch.status; st.p) {
    int hmisc[2];
    HIPCHK(hipMemcpy(hmisc, st.p, sizeof(hmisc), hipMemcpyDeviceToHost));
    if (hmisc[1] != 0) {
      (void)hipMemset(st.p, 0, 8);
      m->batch.ovfPerKeypoint *= 4;   // the next batched call gets a larger overflow region
      set_error("candidate record pool overflow in the batched search: results of that call are incomplete; the overflow region is now %d records per keypoint, call again",
                m->batch.ovfPerKeypoint);
      return YDORB_ERR_CAPACITY;
    }
  }
  return YDORB_OK;
}

int ydorb_matcher_set_profiling(ydorb_matcher_t* m, int32_t on) {
  if (!m) return YDORB_ERR_INVALID_ARG;
  m->profiling = on != 0;
  for (double& v : m->stageMs) v = 0;
  m->stageCalls = 0;
  m->evPending = false;
  for (double& v : m->triMs) v = 0;
  m->triCalls = 0;
  for (double& v : m->bowMs) v = 0;
  m->bowStats.profiled_calls = 0;
  return YDORB_OK;
}

int ydorb_matcher_stage_times(ydorb_matcher_t* m, int32_t maxStages, const char** names, float* ms, int32_t* nStages) {
  if (!m || !nStages) return YDORB_ERR_INVALID_ARG;
  const int n = std::min<int>(maxStages, MS_COUNT);
  for (int i = 0; i < n; i++) {
    if (names) names[i] = kMatchStageNames[i];
    if (ms) ms[i] = m->stageCalls ? (float)(m->stageMs[i] / m->stageCalls) : 0.f;
  }
  *nStages = n;
  return YDORB_OK;
}

}  // extern "C"
