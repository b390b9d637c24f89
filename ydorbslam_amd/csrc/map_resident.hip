// Host driver of the resident map table + its C ABI (include/ydorb/c_api.h, "Resident map table").  One handle,
// one mutex, one stream.  Every part has a host half that validates, stages and plans without HIP (the pool policy: span_pool.h) and a
// device half here that owns the arenas and executes the packed delta:
//   the point table       mapdb_host.h's Host over an SoA arena per point slot (PointColumns below), the camera centres per keyframe
//                         slot and the observation pool; k_mapdb_repack / k_mapdb_apply (mapdb_kernels.hip.h).
//   the attribute table   opt-in; mapdb_attr_host.h's AttrHost over an SoA arena per point slot (AttrColumns below) that follows the
//                         point table's capacity; k_mapdb_attr_apply (mapdb_attr_kernels.hip.h).  Three queries
//                         write their results through to it.
//   five span relations   each a SpanHost<T> (mapdb_rows_host.h) and a SpanDev<T> below: the keyframe rows (section 6o), the point
//                         views and the keyframe descriptor blocks (mapdb_desc_host.h, section 6p) and the opt-in BoW feature vectors
//                         (mapdb_bow_host.h, section 6t), which share the two kernels of mapdb_span_kernels.hip.h, and the opt-in
//                         keyframe features (mapdb_feat_host.h, section 6r), whose one pool arena holds two arrays and has kernels
//                         of its own (mapdb_feat_kernels.hip.h).
//   the local-BA graph    no relation of its own: ydorb_mapdb_local_ba_graph reads rows, views, features, positions and bad flags and
//                         keeps two per-keyframe tables that are clean between calls and a pinned result (mapdb_lba_host.h,
//                         mapdb_lba_kernels.hip.h, section 6u).
// The set_* entries only stage.  A query calls sync() first, which applies what is staged in a fixed order: points, rows, views, blocks,
// features if enabled, BoW feature vectors if enabled, attributes if enabled.  A later part may name what an earlier one introduced
// in the same interval: a row a new point, a view a new keyframe, the attribute arena the point capacity just grown.  Each part: one upload of its packed delta, the
// growths (device-to-device copies), the repack if its pool needs it, the apply; an arena that was replaced is freed only after the
// stream has drained (handOver).  With nothing staged no table byte moves.  Then the query's own arrays in one upload, its pass, one
// read-back and one synchronise.  ydorb_mapdb_correct (mapcorrect_kernels.hip.h, section 6n) is the one query that writes the point
// table: positions in place, then centres.  lockResident / lockResidentFuse at the end hand device pointers to the matcher
// (orb_matcher.hip), which reads them on another stream: they synchronise first.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ydorb/c_api.h"
#include "host_buffers.h"
#include "map_queries.h"
#include "map_table.h"
#include "mapcorrect_kernels.hip.h"
#include "mapdb_attr_host.h"
#include "mapdb_attr_kernels.hip.h"
#include "mapdb_bow_host.h"
#include "mapdb_desc_host.h"
#include "mapdb_desc_kernels.hip.h"
#include "mapdb_feat_host.h"
#include "mapdb_feat_kernels.hip.h"
#include "mapdb_frustum_kernels.hip.h"
#include "mapdb_host.h"
#include "mapdb_kernels.hip.h"
#include "mapdb_lba_host.h"
#include "mapdb_lba_kernels.hip.h"
#include "mapdb_resident_points.h"
#include "mapdb_rows_host.h"
#include "mapdb_rows_kernels.hip.h"
#include "mapdb_span_kernels.hip.h"
#include "ydorb_host.h"

using namespace ydorb;

namespace {

int invalid(const std::string& what) { set_error("resident map table: %s", what.c_str()); return YDORB_ERR_INVALID_ARG; }

int copyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {   // an empty run enqueues nothing
  if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, kind, s));
  return YDORB_OK;
}

struct DeltaPair {   // a packed delta on the device and its pinned staging; never empty: rows may grow the keyframe count alone
  Mem dev;
  PinnedMem host;
  int ensure(size_t bytes) { const int rc = dev.ensure(bytes + 16); return rc ? rc : host.ensure(bytes + 16); }
  int upload(hipStream_t s, size_t bytes) { return copyAsync(dev.p, host.p, bytes, hipMemcpyHostToDevice, s); }
  void release() { dev.release(); host.release(); }
};

int allocSpanHeaders(hipStream_t s, Mem& m, int*& start, int*& len, size_t cap) {   // every slot: no span
  int rc = m.alloc(8 * cap);
  if (rc) return rc;
  start = m.as<int>(); len = start + cap;
  HIPCHK(hipMemsetAsync(m.p, 0, m.cap, s));
  return YDORB_OK;
}

// The end of a sync: what was enqueued still reads the old arenas, so the stream drains before the handle takes each new one made
struct NewArena { Mem* mine; ScopedMem* fresh; };
int handOver(hipStream_t s, std::initializer_list<NewArena> arenas) {
  bool any = false;
  for (const NewArena& a : arenas) any = any || a.fresh->p;
  if (any) HIPCHK(hipStreamSynchronize(s));
  for (const NewArena& a : arenas) if (a.fresh->p) a.mine->take(*a.fresh);
  return YDORB_OK;
}

struct PoolPart { const void* src; size_t bytes, at; };   // a run of pool bytes for download(); at: where it lands in c.hDown

// The device half of one SpanHost<T> (mapdb_rows_host.h): the header arena (start / len per slot), the pool arena and the delta.
template <class T> struct SpanDev {
  Mem hdr, poolMem;
  DeltaPair delta;
  int *start = nullptr, *len = nullptr;
  T* pool = nullptr;

  int allocPool(const mapdb::SpanHost<T>& host) {   // at first, and after a reserve: nothing in flight may read the old one
    const int rc = poolMem.alloc(sizeof(T) * (size_t)host.poolCap());
    pool = poolMem.as<T>();
    return rc;
  }
  int alloc(hipStream_t s, const mapdb::SpanHost<T>& host) {
    const int rc = allocSpanHeaders(s, hdr, start, len, (size_t)host.hdrCap());
    return rc ? rc : allocPool(host);
  }
  int zeroHeaders(hipStream_t s) {   // every slot reads as never set again; a relation never enabled has none
    if (hdr.p) HIPCHK(hipMemsetAsync(hdr.p, 0, hdr.cap, s));
    return YDORB_OK;
  }
  void release() { hdr.release(); poolMem.release(); delta.release(); }

  // Brings the relation up to date, everything on stream s: one upload of the packed delta, the header growth, the repack if the pool
  // needs it, the apply.  repack(P, start, len, oldPool, newPool) and apply(P, start, len, pool) launch the relation's two kernels.
  template <class Repack, class Apply> int sync(hipStream_t s, mapdb::SpanHost<T>& host, Repack repack, Apply apply) {
    if (!host.dirty()) { host.nothingToSync(); return YDORB_OK; }
    const mapdb::RowPlan P = host.plan();
    int rc;
    if ((rc = delta.ensure(P.bytes))) return rc;
    ScopedMem newHdr, newPool;   // become this relation's arenas below; freed here on an early return
    int *st = start, *ln = len;
    T* pl = pool;
    if (P.hdrCap != P.hdrCapBefore && (rc = allocSpanHeaders(s, newHdr, st, ln, (size_t)P.hdrCap))) return rc;
    if (P.repack && (rc = newPool.alloc(sizeof(T) * (size_t)P.poolCap))) return rc;
    if (newPool.p) pl = newPool.as<T>();
    host.pack(P, delta.host.as<uint8_t>());   // every allocation is made: only a HIP error can fail below, and the delta counts as applied
    if ((rc = delta.upload(s, P.bytes))) return rc;
    if (newHdr.p && ((rc = copyAsync(st, start, 4 * (size_t)P.nKfBefore, hipMemcpyDeviceToDevice, s)) ||
                     (rc = copyAsync(ln, len, 4 * (size_t)P.nKfBefore, hipMemcpyDeviceToDevice, s))))
      return rc;
    if (P.repack && P.nKfBefore > 0) {
      repack(P, st, ln, pool, pl);
      HIPCHK(hipGetLastError());
    }
    apply(P, st, ln, pl);
    HIPCHK(hipGetLastError());
    if ((rc = handOver(s, {{&hdr, &newHdr}, {&poolMem, &newPool}}))) return rc;
    start = st; len = ln; pool = pl;
    return YDORB_OK;
  }

  // The first `held` headers and the given runs of the pool read back into c.hDown, with one synchronise
  template <size_t N> int download(StagedCtx& c, size_t held, size_t& dStart, size_t& dLen, PoolPart (&parts)[N]) {
    Layout D;
    dStart = D.add(4 * held); dLen = D.add(4 * held);
    for (PoolPart& p : parts) p.at = D.add(p.bytes);
    D.add(16);
    int rc = c.hDown.ensure(D.bytes);
    if (rc) return rc;
    hipStream_t s = c.stream;
    if ((rc = copyAsync(at<void>(c.hDown, dStart), start, 4 * held, hipMemcpyDeviceToHost, s)) ||
        (rc = copyAsync(at<void>(c.hDown, dLen), len, 4 * held, hipMemcpyDeviceToHost, s)))
      return rc;
    for (const PoolPart& p : parts)
      if ((rc = copyAsync(at<void>(c.hDown, p.at), p.src, p.bytes, hipMemcpyDeviceToHost, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return YDORB_OK;
  }
  int download(StagedCtx& c, size_t held, size_t used, size_t& dStart, size_t& dLen, size_t& dPool) {   // the used part of a plain pool
    PoolPart part[1] = {{pool, sizeof(T) * used, 0}};
    const int rc = download(c, held, dStart, dLen, part);
    dPool = part[0].at;
    return rc;
  }
};

}  // namespace

struct ydorb_mapdb {
  int device = 0;
  StagedCtx c;                 // c.mu: LocalMapping stages while LoopClosing queries.  c.up / c.down: a query's arrays and results
  mapdb::Host host;
  Mem points, centres, pool;   // arenas: T and the pool pointers point into them
  DeltaPair delta;
  mapdb::SlotTables T{};
  int* poolKf = nullptr;
  uint8_t* poolLevel = nullptr;
  // keyframe rows
  mapdb::RowsHost rows;
  SpanDev<int32_t> dRows;
  Mem rowset;   // first / seenStamp of the points-of-keyframes query, one entry per point slot
  int *first = nullptr, *seenStamp = nullptr;
  size_t rowsetCap = 0;
  int stamp = 0;
  // point views and keyframe descriptor blocks
  mapdb::DescHost desc;
  SpanDev<int32_t> dViews;
  SpanDev<mapdb::DescRow> dBlocks;
  // point attributes: nothing of this is allocated or launched until ydorb_mapdb_enable_attributes
  mapdb::AttrHost attr;
  Mem attrMem;
  DeltaPair attrDelta;
  mapdb::AttrArrays A{};
  // keyframe features: nothing of this is allocated or launched until ydorb_mapdb_enable_features.  The pool
  // arena has 32 bytes per entry and holds two arrays: KeyPoint [cap] at its base (featKps), right_x [cap] behind it (featRightX)
  mapdb::FeatHost feat;
  SpanDev<mapdb::FeatRec> dFeats;
  // keyframe BoW feature vectors: nothing of this is allocated or launched until ydorb_mapdb_enable_bow
  mapdb::BowHost bow;
  SpanDev<mapdb::BowRec> dBow;
  // local-BA graph: nothing of this is allocated or launched until ydorb_mapdb_local_ba_graph.  lbaFirst / lbaPoseOf
  // have one entry per keyframe slot and are UINT64_MAX / -1 everywhere between calls (mapdb_lba_kernels.hip.h); lbaDirty: a call failed
  // between its first launch and its last synchronise, the next one fills both before it starts.  The result lives in lbaHost.
  Mem lbaTables, lbaDev;
  PinnedMem lbaHost;
  unsigned long long* lbaFirst = nullptr;
  int* lbaPoseOf = nullptr;
  size_t lbaCap = 0;
  bool lbaDirty = false;
  std::vector<uint8_t> lbaMark;   // scratch of the repeat test
  YdMapDbLbaStats lbaStats{};
  bool lbaProfiling = false;
  hipEvent_t lbaEvent[6] = {};    // created by the first ydorb_mapdb_lba_set_profiling(db, 1)
  ydorb_mapdb(int32_t pc, int32_t kc, int64_t oc) : host(pc, kc, oc), rows(kc, oc), desc(pc, kc), feat(kc), bow(kc) {}
};

namespace {

// The columns of the two SoA tables, each named here and nowhere else in this file as a list: each(f) calls f(pointer-to-member,
// elements per slot).  An arena's layout, its growth copy and its export walk the list; the byte strides come from the element types.
struct PointColumns {
  using Table = mapdb::SlotTables;   // its centre is no column: the centres arena is per keyframe slot
  template <class F> static void each(F f) {
    f(&Table::start, 1); f(&Table::end, 1); f(&Table::refKf, 1); f(&Table::pos, 3); f(&Table::bad, 1); f(&Table::refLevel, 1);
  }
};
struct AttrColumns {
  using Table = mapdb::AttrArrays;
  template <class F> static void each(F f) {
    f(&Table::normal, 3); f(&Table::minDistance, 1); f(&Table::maxDistance, 1); f(&Table::desc, 2); f(&Table::flags, 1);
  }
};

template <class Cols> size_t layColumns(Carve& C, typename Cols::Table& t, size_t slots) {
  Cols::each([&](auto col, size_t per) { C.take(t.*col, per * slots); });
  return C.L.bytes;
}
// A fresh arena of `cap` slots, all zero
template <class Cols> int allocColumns(hipStream_t s, Mem& m, typename Cols::Table& t, size_t cap) {
  typename Cols::Table sizing{};
  Carve sz(nullptr);
  int rc = m.alloc(layColumns<Cols>(sz, sizing, cap));
  if (rc) return rc;
  Carve cv(m.p);
  layColumns<Cols>(cv, t, cap);
  HIPCHK(hipMemsetAsync(m.p, 0, m.cap, s));
  return YDORB_OK;
}
// The first n slots of every column, from -> to: device to device for a growth, device to host for an export's read-back, host to
// host (a plain memcpy) for its copy-out, where a column the caller does not take has a null pointer in `to`
template <class Cols> int copyColumns(hipStream_t s, hipMemcpyKind kind, const typename Cols::Table& to, const typename Cols::Table& from, size_t n) {
  int rc = YDORB_OK;
  Cols::each([&](auto col, size_t per) {
    const size_t bytes = sizeof(*(to.*col)) * per * n;
    if (rc || !(to.*col)) return;
    if (kind != hipMemcpyHostToHost) rc = copyAsync(to.*col, from.*col, bytes, kind, s);
    else if (bytes) std::memcpy(to.*col, from.*col, bytes);
  });
  return rc;
}

size_t layPool(Carve& C, int*& kf, uint8_t*& level, size_t cap) {
  C.take(kf, cap); C.take(level, cap);
  return C.L.bytes;
}

// A fresh point arena of `cap` slots: all zero, every slot bad (a slot never set reads as bad with no observations)
int allocPoints(hipStream_t s, Mem& m, mapdb::SlotTables& T, size_t cap) {
  const int rc = allocColumns<PointColumns>(s, m, T, cap);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(T.bad, 1, cap, s));
  return YDORB_OK;
}
int allocCentres(hipStream_t s, Mem& m, float*& centre, size_t cap) {
  int rc = m.alloc(12 * cap);
  if (rc) return rc;
  centre = m.as<float>();
  HIPCHK(hipMemsetAsync(m.p, 0, m.cap, s));
  return YDORB_OK;
}
int allocPool(Mem& m, int*& kf, uint8_t*& level, size_t cap) {
  int* k0 = nullptr; uint8_t* l0 = nullptr;
  Carve sz(nullptr);
  int rc = m.alloc(layPool(sz, k0, l0, cap));
  if (rc) return rc;
  Carve cv(m.p);
  layPool(cv, kf, level, cap);
  return YDORB_OK;
}

// The blocks of an apply kernel: a lane per fixed record; over the payload 2048 blocks at the most, lanes stride past that
unsigned applyBlocks(size_t nFixed, int64_t nPayload, size_t threads) {
  const size_t forFixed = (nFixed + threads - 1) / threads, forPayload = std::min<size_t>(((size_t)nPayload + threads - 1) / threads, 2048);
  return (unsigned)std::max<size_t>(std::max(forFixed, forPayload), 1);
}

// Applies what is staged.  Called with the mutex held and the device set; everything it enqueues goes to the handle's stream, and the
// arenas it replaces are freed only after that stream has drained.
int syncPoints(ydorb_mapdb* h) {
  if (!h->host.dirty()) { h->host.nothingToSync(); return YDORB_OK; }
  hipStream_t s = h->c.stream;
  const mapdb::Plan P = h->host.plan();
  int rc;
  if ((rc = h->delta.ensure(P.bytes))) return rc;
  ScopedMem newPoints, newCentres, newPool;   // become the handle's arenas below; freed here on an early return
  mapdb::SlotTables T = h->T;
  int* poolKf = h->poolKf;
  uint8_t* poolLevel = h->poolLevel;
  if (P.pointCap != P.pointCapBefore && (rc = allocPoints(s, newPoints, T, (size_t)P.pointCap))) return rc;
  if (P.kfCap != P.kfCapBefore && (rc = allocCentres(s, newCentres, T.centre, (size_t)P.kfCap))) return rc;
  if (P.repack && (rc = allocPool(newPool, poolKf, poolLevel, (size_t)P.poolCap))) return rc;
  h->host.pack(P, h->delta.host.as<uint8_t>());   // nothing below can be refused for a reason of the caller's: the delta counts as applied
  if ((rc = h->delta.upload(s, P.bytes))) return rc;
  if (newPoints.p && (rc = copyColumns<PointColumns>(s, hipMemcpyDeviceToDevice, T, h->T, (size_t)P.nPointsBefore))) return rc;
  if (newCentres.p && (rc = copyAsync(T.centre, h->T.centre, 12 * (size_t)P.nKeyframesBefore, hipMemcpyDeviceToDevice, s))) return rc;
  if (P.repack && P.nPointsBefore > 0) {
    mapdb::RepackArgs a;
    a.nPoints = P.nPointsBefore; a.start = T.start; a.end = T.end; a.newOff = at<int>(h->delta.dev, P.oNewOff);
    a.oldKf = h->poolKf; a.oldLevel = h->poolLevel; a.newKf = poolKf; a.newLevel = poolLevel;
    hipLaunchKernelGGL(mapdb::k_mapdb_repack, dim3((unsigned)((P.nPointsBefore + mapdb::kThreads - 1) / mapdb::kThreads)), dim3(mapdb::kThreads), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  {
    mapdb::ApplyArgs a;
    a.t = T;
    a.nPointRec = P.nPointRec; a.nPosRec = P.nPosRec; a.nCentreRec = P.nCentreRec; a.nPayload = (int)P.nPayload; a.tail = (int)P.tail;
    a.point = at<mapdb::PointRec>(h->delta.dev, P.oPoint); a.position = at<mapdb::Vec3Rec>(h->delta.dev, P.oPos); a.centre = at<mapdb::Vec3Rec>(h->delta.dev, P.oCentre);
    a.payKf = at<int>(h->delta.dev, P.oPayKf); a.payLevel = at<uint8_t>(h->delta.dev, P.oPayLevel);
    a.poolKf = poolKf; a.poolLevel = poolLevel;
    const unsigned blocks = applyBlocks((size_t)P.nPointRec + P.nPosRec + P.nCentreRec, P.nPayload, mapdb::kThreads);
    hipLaunchKernelGGL(mapdb::k_mapdb_apply, dim3(blocks), dim3(mapdb::kThreads), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  if ((rc = handOver(s, {{&h->points, &newPoints}, {&h->centres, &newCentres}, {&h->pool, &newPool}}))) return rc;
  h->T = T; h->poolKf = poolKf; h->poolLevel = poolLevel;
  return YDORB_OK;
}

// The plain span relations (the keyframe rows, the point views, the descriptor blocks, the BoW feature vectors) share the two kernels
// of mapdb_span_kernels.hip.h: an element moves as sizeof(T) / sizeof(unit) units, an int for the int32 spans and the two-int BoW
// pairs, a uint4 where it can.
template <class T> int syncPlainSpans(hipStream_t s, SpanDev<T>& d, mapdb::SpanHost<T>& host) {
  using U = std::conditional_t<sizeof(T) % sizeof(uint4) == 0, uint4, int>;
  constexpr int kPer = sizeof(T) / sizeof(U);
  return d.sync(s, host,
    [&](const mapdb::RowPlan& P, int* st, int* ln, T* oldPool, T* newPool) {
      mapdb::SpanRepackArgs<U> a;
      a.nSlots = P.nKfBefore; a.start = st; a.len = ln; a.newOff = at<int>(d.delta.dev, P.oNewOff);
      a.oldPool = reinterpret_cast<const U*>(oldPool); a.newPool = reinterpret_cast<U*>(newPool);
      hipLaunchKernelGGL((mapdb::k_mapdb_span_repack<U, kPer>), dim3((unsigned)((P.nKfBefore + mapdb::kSpanWaves - 1) / mapdb::kSpanWaves)),
                         dim3(mapdb::kSpanThreads), 0, s, a);
    },
    [&](const mapdb::RowPlan& P, int* st, int* ln, T* pl) {
      mapdb::SpanApplyArgs<U> a;
      a.nHeaderRec = P.nHeaderRec; a.nEntryRec = P.nEntryRec; a.tail = (int)P.tail; a.nPayload = kPer * P.nPayload;
      a.header = at<mapdb::RowHeaderRec>(d.delta.dev, P.oHeader); a.entry = at<mapdb::RowEntryRec>(d.delta.dev, P.oEntry);
      a.payload = at<U>(d.delta.dev, P.oPayload);
      a.start = st; a.len = ln; a.pool = reinterpret_cast<U*>(pl);
      const unsigned blocks = applyBlocks((size_t)P.nHeaderRec + P.nEntryRec, kPer * P.nPayload, mapdb::kSpanThreads);
      hipLaunchKernelGGL((mapdb::k_mapdb_span_apply<U, kPer>), dim3(blocks), dim3(mapdb::kSpanThreads), 0, s, a);
    });
}

// The two arrays of a feature arena of `cap` pool entries (mapdb_feat_host.h)
uint32_t* featKps(mapdb::FeatRec* pool) { return reinterpret_cast<uint32_t*>(pool); }
uint32_t* featRightX(mapdb::FeatRec* pool, int64_t cap) { return reinterpret_cast<uint32_t*>(pool) + 7 * (size_t)cap; }

// The staged features, after the blocks: a query reads a keyframe's features and its block together.
int syncFeatures(ydorb_mapdb* h) {
  hipStream_t s = h->c.stream;
  DeltaPair& delta = h->dFeats.delta;
  return h->dFeats.sync(s, h->feat.feats,
    [&](const mapdb::RowPlan& P, int* st, int* ln, mapdb::FeatRec* oldPool, mapdb::FeatRec* newPool) {
      mapdb::FeatRepackArgs a;
      a.nKf = P.nKfBefore; a.featStart = st; a.featLen = ln; a.newOff = at<int>(delta.dev, P.oNewOff);
      a.oldKps = featKps(oldPool); a.oldRightX = featRightX(oldPool, P.poolCapBefore);
      a.newKps = featKps(newPool); a.newRightX = featRightX(newPool, P.poolCap);
      hipLaunchKernelGGL(mapdb::k_mapdb_feat_repack, dim3((unsigned)((P.nKfBefore + mapdb::kFeatWaves - 1) / mapdb::kFeatWaves)), dim3(mapdb::kFeatThreads), 0, s, a);
    },
    [&](const mapdb::RowPlan& P, int* st, int* ln, mapdb::FeatRec* pl) {
      mapdb::FeatApplyArgs a;
      a.nHeaderRec = P.nHeaderRec; a.tail = (int)P.tail;
      a.header = at<mapdb::RowHeaderRec>(delta.dev, P.oHeader); a.payload = at<uint4>(delta.dev, P.oPayload);
      a.featStart = st; a.featLen = ln; a.kps = featKps(pl); a.rightX = featRightX(pl, P.poolCap);
      hipLaunchKernelGGL(mapdb::k_mapdb_feat_apply, dim3((unsigned)std::max((P.nHeaderRec + mapdb::kFeatWaves - 1) / mapdb::kFeatWaves, 1)), dim3(mapdb::kFeatThreads), 0, s, a);
    });
}

// The staged attributes, after everything else: the arena follows the point table's capacity (syncPoints may just have grown it), then
// one upload of the records and k_mapdb_attr_apply.  A fresh arena is all zero, what a slot never set reads as.
int syncAttributes(ydorb_mapdb* h) {
  mapdb::AttrHost& host = h->attr;
  if (!host.needsSync(h->host.pointCap())) { host.nothingToSync(); return YDORB_OK; }
  hipStream_t s = h->c.stream;
  const mapdb::AttrPlan P = host.plan(h->host.pointCap());
  int rc;
  if ((rc = h->attrDelta.ensure(P.bytes))) return rc;
  ScopedMem fresh;
  mapdb::AttrArrays A = h->A;
  if (P.cap != P.capBefore && (rc = allocColumns<AttrColumns>(s, fresh, A, (size_t)P.cap))) return rc;
  host.pack(P, h->attrDelta.host.as<uint8_t>());   // every allocation is made: only a HIP error can fail below, and the delta counts as applied
  if ((rc = h->attrDelta.upload(s, P.bytes))) return rc;
  if (fresh.p && (rc = copyColumns<AttrColumns>(s, hipMemcpyDeviceToDevice, A, h->A, (size_t)P.capBefore))) return rc;
  if (P.nRec) {
    hipLaunchKernelGGL(mapdb::k_mapdb_attr_apply, dim3((unsigned)((P.nRec + mapdb::kAttrThreads - 1) / mapdb::kAttrThreads)), dim3(mapdb::kAttrThreads), 0, s,
                       P.nRec, h->attrDelta.dev.as<mapdb::AttrRec>(), A);
    HIPCHK(hipGetLastError());
  }
  if ((rc = handOver(s, {{&h->attrMem, &fresh}}))) return rc;
  h->A = A;
  return YDORB_OK;
}

// Everything staged, in the one order: a row may name a point, a view a keyframe and a query a point that got its slot in the same
// interval, and a query reads a keyframe's features and its block together.
int sync(ydorb_mapdb* h) {
  hipStream_t s = h->c.stream;
  int rc = syncPoints(h);
  if (!rc) rc = syncPlainSpans(s, h->dRows, h->rows);
  if (!rc) rc = syncPlainSpans(s, h->dViews, h->desc.views);
  if (!rc) rc = syncPlainSpans(s, h->dBlocks, h->desc.blocks);
  if (!rc && h->feat.enabled()) rc = syncFeatures(h);
  if (!rc && h->bow.enabled()) rc = syncPlainSpans(s, h->dBow, h->bow.spans);
  return rc || !h->attr.enabled() ? rc : syncAttributes(h);
}

unsigned attrBlocks(size_t n) { return (unsigned)((n + mapdb::kAttrThreads - 1) / mapdb::kAttrThreads); }

// Write-through of a query that has just run and synchronised: its device result buffer still holds normal, distances and status,
// and `slots` [n] is where it uploaded them.  Queued behind it on the handle's stream and not waited for: whatever reads the arrays
// next is either on that stream or synchronises it first (lockResident).  hStatus: the statuses as read back, for the count.
int writeThroughGeometry(ydorb_mapdb* h, int n, const int* slots, const float* normal, const float* minDistance, const float* maxDistance,
                         const uint8_t* status, const uint8_t* hStatus, int want) {
  int64_t wrote = 0;
  for (int i = 0; i < n; i++) wrote += hStatus[i] == want;
  h->attr.wroteThrough(wrote);
  if (!wrote) return YDORB_OK;
  hipLaunchKernelGGL(mapdb::k_attr_scatter_geometry, dim3(attrBlocks((size_t)n)), dim3(mapdb::kAttrThreads), 0, h->c.stream, n, slots, normal, minDistance,
                     maxDistance, status, want, h->A);
  HIPCHK(hipGetLastError());
  return YDORB_OK;
}

mapdb::ResidentPoints residentOf(const ydorb_mapdb* h) {   // call after sync(), which may move the arenas
  mapdb::ResidentPoints R;
  R.pos = h->T.pos; R.bad = h->T.bad; R.obsStart = h->T.start; R.obsEnd = h->T.end;
  R.normal = h->A.normal; R.minDistance = h->A.minDistance; R.maxDistance = h->A.maxDistance;
  R.desc = reinterpret_cast<const mapdb::Desc16*>(h->A.desc); R.flags = h->A.flags;
  return R;
}

// first / seenStamp cover the point table's capacity: a fresh pair when it grew.  first is INT32_MAX everywhere between calls.
int ensureRowset(ydorb_mapdb* h) {
  const size_t cap = (size_t)h->host.pointCap();
  if (h->rowsetCap == cap) return YDORB_OK;
  h->rowsetCap = 0;
  int rc = h->rowset.alloc(8 * cap);
  if (rc) return rc;
  h->first = h->rowset.as<int>(); h->seenStamp = h->first + cap;
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)h->first, INT32_MAX, cap, h->c.stream));
  HIPCHK(hipMemsetAsync(h->seenStamp, 0, 4 * cap, h->c.stream));
  h->stamp = 0;
  h->rowsetCap = cap;
  return YDORB_OK;
}

// mark, count, emit with no host round trip between them (mapdb_rows_kernels.hip.h)
int launchRowset(hipStream_t s, const mapdb::RowsetArgs& a) {
  const size_t forMark = ((size_t)std::max(a.nE, a.nSeen) + mapdb::kRowThreads - 1) / mapdb::kRowThreads;
  hipLaunchKernelGGL(mapdb::k_rowset_mark, dim3((unsigned)forMark), dim3(mapdb::kRowThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(mapdb::k_rowset_count, dim3((unsigned)a.nBlocks), dim3(mapdb::kRowThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(mapdb::k_rowset_emit, dim3((unsigned)a.nBlocks), dim3(mapdb::kRowThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  return YDORB_OK;
}

// the call's stamp for seenStamp: a later call has a later stamp
int nextRowsetStamp(ydorb_mapdb* h) {
  if (h->stamp == INT32_MAX) { HIPCHK(hipMemsetAsync(h->seenStamp, 0, 4 * h->rowsetCap, h->c.stream)); h->stamp = 0; }
  h->stamp++;
  return YDORB_OK;
}

// lbaFirst / lbaPoseOf cover the table's keyframe slots: a fresh pair when they outgrew it, every byte 0xff (UINT64_MAX and -1)
int ensureLbaTables(ydorb_mapdb* h) {
  const size_t need = (size_t)h->host.nKeyframes();
  hipStream_t s = h->c.stream;
  if (need > h->lbaCap) {
    const size_t cap = std::max<size_t>(2 * need, 64);
    h->lbaCap = 0;
    int rc = h->lbaTables.alloc(12 * cap);
    if (rc) return rc;
    h->lbaFirst = h->lbaTables.as<unsigned long long>(); h->lbaPoseOf = reinterpret_cast<int*>(h->lbaFirst + cap);
    h->lbaCap = cap;
    h->lbaDirty = true;
  }
  if (h->lbaDirty) {
    HIPCHK(hipMemsetAsync(h->lbaTables.p, 0xff, 12 * h->lbaCap, s));
    h->lbaDirty = false;
  }
  return YDORB_OK;
}

// the table and the point attributes as the queries of map_queries.h read them: call after sync(), which may move the arenas
mapmaint::MapSource sourceOf(const ydorb_mapdb* h) {
  mapmaint::MapSource src;
  mapmaint::Table& t = src.resident;
  t.nPoints = h->host.nPoints(); t.nKeyframes = h->host.nKeyframes();
  t.obsStart = h->T.start; t.obsEnd = h->T.end; t.obsKf = h->poolKf; t.obsLevel = h->poolLevel; t.bad = h->T.bad;
  src.pos = h->T.pos; src.centre = h->T.centre; src.refKf = h->T.refKf; src.refLevel = h->T.refLevel;
  return src;
}

// Everything a new handle owns but the two opt-in parts, at the capacities its host halves start with
int allocHandle(ydorb_mapdb* h) {
  int rc = h->c.init(h->device);
  if (rc) return rc;
  hipStream_t s = h->c.stream;
  if ((rc = allocPoints(s, h->points, h->T, (size_t)h->host.pointCap())) || (rc = allocCentres(s, h->centres, h->T.centre, (size_t)h->host.kfCap())) ||
      (rc = allocPool(h->pool, h->poolKf, h->poolLevel, (size_t)h->host.poolCap())) || (rc = h->dRows.alloc(s, h->rows)) ||
      (rc = h->dViews.alloc(s, h->desc.views)) || (rc = h->dBlocks.alloc(s, h->desc.blocks)))
    return rc;
  HIPCHK(hipStreamSynchronize(s));
  return YDORB_OK;
}

}  // namespace

extern "C" int ydorb_mapdb_create(int32_t device, int32_t point_capacity, int32_t keyframe_capacity, int64_t observation_capacity,
                                  ydorb_mapdb_t** out) {
  if (!out) return invalid("null out");
  if (device < 0 || device >= 16) return invalid("device " + std::to_string(device) + " outside 0..15");
  if (point_capacity < 0 || keyframe_capacity < 0 || observation_capacity < 0) return invalid("negative capacity");
  if (observation_capacity > INT32_MAX) return invalid("a pool past INT32_MAX entries");
  int rc = require_device(device);
  if (rc) return rc;
  ydorb_mapdb* h = new ydorb_mapdb(point_capacity, keyframe_capacity, observation_capacity);
  h->device = device;
  if ((rc = allocHandle(h))) { ydorb_mapdb_destroy(h); return rc; }
  *out = h;
  return YDORB_OK;
}

extern "C" void ydorb_mapdb_destroy(ydorb_mapdb_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->c.stream) { (void)hipStreamSynchronize(h->c.stream); (void)hipStreamDestroy(h->c.stream); }
  h->c.releaseBuffers();
  h->points.release(); h->centres.release(); h->pool.release(); h->delta.release(); h->rowset.release();
  h->attrMem.release(); h->attrDelta.release();
  h->dRows.release(); h->dViews.release(); h->dBlocks.release(); h->dFeats.release(); h->dBow.release();
  h->lbaTables.release(); h->lbaDev.release(); h->lbaHost.release();
  for (hipEvent_t e : h->lbaEvent) if (e) (void)hipEventDestroy(e);
  delete h;
}

extern "C" int ydorb_mapdb_clear(ydorb_mapdb_t* h) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  HIPCHK(hipSetDevice(h->device));
  h->host.clear();
  h->rows.clear();
  h->desc.clear();
  h->attr.clear();
  h->feat.clear();
  h->bow.clear();
  hipStream_t s = h->c.stream;   // every slot reads as never set again
  int rc;
  if ((rc = h->dRows.zeroHeaders(s)) || (rc = h->dViews.zeroHeaders(s)) || (rc = h->dBlocks.zeroHeaders(s)) || (rc = h->dFeats.zeroHeaders(s)) ||
      (rc = h->dBow.zeroHeaders(s)))
    return rc;
  if (h->attrMem.p) HIPCHK(hipMemsetAsync(h->attrMem.p, 0, h->attrMem.cap, s));
  if (h->rowsetCap) {
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)h->first, INT32_MAX, h->rowsetCap, s));
    HIPCHK(hipMemsetAsync(h->seenStamp, 0, 4 * h->rowsetCap, s));
    h->stamp = 0;
  }
  HIPCHK(hipMemsetAsync(h->points.p, 0, h->points.cap, s));
  HIPCHK(hipMemsetAsync(h->T.bad, 1, (size_t)h->host.pointCap(), s));
  HIPCHK(hipMemsetAsync(h->centres.p, 0, h->centres.cap, s));
  HIPCHK(hipStreamSynchronize(s));
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_set_centres(ydorb_mapdb_t* h, const int32_t* kf_slots, int32_t n, const float* centre) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  return h->host.setCentres(kf_slots, n, centre, err) ? YDORB_OK : invalid(err);
}

extern "C" int ydorb_mapdb_set_points(ydorb_mapdb_t* h, const int32_t* slots, int32_t n, const int32_t* obs_start, const int32_t* obs_kf,
                                      const uint8_t* obs_level, const uint8_t* bad, const int32_t* ref_kf, const uint8_t* ref_level,
                                      const float* pos) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!h->host.setPoints(slots, n, obs_start, obs_kf, obs_level, bad, ref_kf, ref_level, pos, err)) return invalid(err);
  h->attr.pointsSet(slots, n, obs_start, bad);   // an erased point clears its attributes
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_set_positions(ydorb_mapdb_t* h, const int32_t* slots, int32_t n, const float* pos) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  return h->host.setPositions(slots, n, pos, err) ? YDORB_OK : invalid(err);
}

extern "C" int ydorb_mapdb_stats(ydorb_mapdb_t* h, YdMapDbStats* stats) {
  if (!h || !stats) return invalid("null handle or stats");
  std::lock_guard<std::mutex> lock(h->c.mu);
  h->host.stats(*stats);
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_update_normal_depth(ydorb_mapdb_t* h, const int32_t* slots, int32_t n, const float* scale_factors, int32_t n_levels,
                                               float* normal, float* min_distance, float* max_distance, uint8_t* status) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!h->host.checkNormalDepth(slots, n, scale_factors, n_levels, normal, min_distance, max_distance, status, err)) return invalid(err);
  if (n == 0) return YDORB_OK;
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  mapmaint::MapSource src = sourceOf(h);
  src.slots = slots;
  mapmaint::NormalDepthOnDevice dev;
  if ((rc = mapmaint::runNormalDepth(h->c, src, n, scale_factors, n_levels, normal, min_distance, max_distance, status, &dev)) || !h->attr.enabled()) return rc;
  return writeThroughGeometry(h, n, dev.slots, dev.normal, dev.minDistance, dev.maxDistance, dev.status, status, YDORB_MAP_UPDATED);
}

extern "C" int ydorb_mapdb_covisibility(ydorb_mapdb_t* h, const int32_t* query_kf, int32_t n_queries, const int32_t* list_start,
                                        const int32_t* point_idx, const int32_t* out_start, int32_t* conn_kf, int32_t* conn_weight,
                                        int32_t* counts, uint8_t* status) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  const YdObservationTable hdr = h->host.counts();
  if (!maptable::checkCovisibilityArgs(&hdr, query_kf, n_queries, list_start, point_idx, out_start, conn_kf, conn_weight, counts, status, err))
    return invalid(err);
  if (n_queries == 0) return YDORB_OK;
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  mapmaint::MapSource src = sourceOf(h);
  return mapmaint::runCovisibility(h->c, src, query_kf, n_queries, list_start, point_idx, out_start, conn_kf, conn_weight, counts, status);
}

extern "C" int ydorb_mapdb_keyframe_redundancy(ydorb_mapdb_t* h, const int32_t* cand_kf, int32_t n_candidates, const int32_t* list_start,
                                               const int32_t* point_idx, const uint8_t* own_level, const uint8_t* removed, int32_t th_obs,
                                               int32_t* n_counted, int32_t* n_redundant, uint8_t* cull) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  const YdObservationTable hdr = h->host.counts();
  if (!maptable::checkRedundancyArgs(&hdr, cand_kf, n_candidates, list_start, point_idx, own_level, n_counted, n_redundant, cull, err))
    return invalid(err);
  const size_t nc = (size_t)n_candidates;
  if (nc == 0) return YDORB_OK;
  std::memset(n_counted, 0, 4 * nc);
  std::memset(n_redundant, 0, 4 * nc);
  std::memset(cull, 0, nc);               // an empty list: 0 > 0.9 * 0 is false
  if (list_start[nc] == 0) return YDORB_OK;
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  mapmaint::MapSource src = sourceOf(h);
  return mapmaint::runRedundancy(h->c, src, cand_kf, n_candidates, list_start, point_idx, own_level, removed, th_obs, n_counted, n_redundant, cull);
}

// sync; one upload of the keyframe tables, the rank table, the claimed list and the centres; the pass; the centre write; one read-back;
// one synchronise; the scatter to entry order.  Point positions travel only as results.
extern "C" int ydorb_mapdb_correct(ydorb_mapdb_t* h, const YdMapCorrection* c) {
  if (!h) {   // without a device no handle exists: say that first, there is no CPU path to fall back to
    const int rc = require_device(0);
    return rc ? rc : invalid("null handle");
  }
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  mapdb::Host::CorrectionPlan P;
  if (!h->host.planCorrection(c, P, err)) return invalid(err);
  const size_t n = (size_t)c->n, nKf = (size_t)c->n_kf, nc = P.slot.size(), nk = (size_t)h->host.nKeyframes();
  const bool writeCentres = c->centre_after && nKf > 0;
  if (n == 0 && !writeCentres) return YDORB_OK;
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  StagedCtx& ctx = h->c;
  const size_t perKf = c->arithmetic == YDORB_MAPCORR_SIM3 ? 8 * sizeof(double) : 12 * sizeof(float);
  const size_t pairBytes = nc ? perKf * nKf : 0;
  Layout U;
  const size_t oBefore = U.add(pairBytes), oAfter = U.add(pairBytes), oRankOf = U.add(4 * nk), oKf = U.add(4 * nKf),
               oCen = U.add(c->centre_after ? 12 * nKf : 0), oSlot = U.add(4 * nc), oRank = U.add(4 * nc);
  Layout D;
  const size_t dPos = D.add(12 * nc), dNrm = D.add(P.normals ? 12 * nc : 0), dMin = D.add(P.normals ? 4 * nc : 0), dMax = D.add(P.normals ? 4 * nc : 0),
               dSt = D.add(nc);
  U.add(16); D.add(16);   // never an empty buffer
  if ((rc = ctx.ensure(U.bytes, D.bytes))) return rc;
  if (pairBytes) { std::memcpy(at<void>(ctx.hUp, oBefore), c->before, pairBytes); std::memcpy(at<void>(ctx.hUp, oAfter), c->after, pairBytes); }
  if (nk) std::memcpy(at<void>(ctx.hUp, oRankOf), P.rankOf.data(), 4 * nk);
  if (nKf) std::memcpy(at<void>(ctx.hUp, oKf), c->kf_slots, 4 * nKf);
  if (writeCentres) std::memcpy(at<void>(ctx.hUp, oCen), c->centre_after, 12 * nKf);
  if (nc) { std::memcpy(at<void>(ctx.hUp, oSlot), P.slot.data(), 4 * nc); std::memcpy(at<void>(ctx.hUp, oRank), P.rank.data(), 4 * nc); }
  hipStream_t s = ctx.stream;
  HIPCHK(hipMemcpyAsync(ctx.up.p, ctx.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  if (nc) {
    mapcorrect::CorrectArgs a;
    a.nClaimed = (int)nc; a.nKf = c->n_kf; a.arithmetic = c->arithmetic; a.centres = c->centres; a.normals = P.normals ? 1 : 0;
    a.slot = at<int>(ctx.up, oSlot); a.rank = at<int>(ctx.up, oRank); a.rankOf = at<int>(ctx.up, oRankOf);
    a.before = at<void>(ctx.up, oBefore); a.after = at<void>(ctx.up, oAfter); a.centreAfter = at<float>(ctx.up, oCen);
    a.pos = h->T.pos; a.centre = h->T.centre; a.obsStart = h->T.start; a.obsEnd = h->T.end; a.obsKf = h->poolKf;
    a.refKf = h->T.refKf; a.refLevel = h->T.refLevel;
    for (int i = 0; i < 8; i++) a.scaleFactors[i] = P.normals && i < c->n_levels ? c->scale_factors[i] : 0.f;
    a.nLevels = P.normals ? c->n_levels : 1;
    a.posOut = at<float>(ctx.down, dPos); a.normal = at<float>(ctx.down, dNrm); a.minDistance = at<float>(ctx.down, dMin);
    a.maxDistance = at<float>(ctx.down, dMax); a.status = at<uint8_t>(ctx.down, dSt);
    hipLaunchKernelGGL(mapcorrect::k_mapdb_correct, dim3((unsigned)((nc + mapcorrect::kThreads - 1) / mapcorrect::kThreads)), dim3(mapcorrect::kThreads), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  if (writeCentres) {   // after the pass: its lanes read the old centres
    mapcorrect::CentreArgs a;
    a.nKf = c->n_kf; a.kfSlots = at<int>(ctx.up, oKf); a.centreAfter = at<float>(ctx.up, oCen); a.centre = h->T.centre;
    hipLaunchKernelGGL(mapcorrect::k_mapdb_correct_centres, dim3((unsigned)((nKf + mapcorrect::kThreads - 1) / mapcorrect::kThreads)), dim3(mapcorrect::kThreads), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  if (nc) HIPCHK(hipMemcpyAsync(ctx.hDown.p, ctx.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  h->host.correctionApplied(c, P, at<float>(ctx.hDown, dPos));
  if (h->attr.enabled()) {   // a call without a normals pass computed none: it writes nothing
    h->attr.wroteThrough(0);
    if (P.normals && nc && (rc = writeThroughGeometry(h, (int)nc, at<int>(ctx.up, oSlot), at<float>(ctx.down, dNrm), at<float>(ctx.down, dMin),
                                                      at<float>(ctx.down, dMax), at<uint8_t>(ctx.down, dSt), at<uint8_t>(ctx.hDown, dSt), YDORB_MAPCORR_DONE)))
      return rc;
  }
  if (n == 0) return YDORB_OK;
  std::memset(c->pos_out, 0, 12 * n);
  if (P.normals) { std::memset(c->normal, 0, 12 * n); std::memset(c->min_distance, 0, 4 * n); std::memset(c->max_distance, 0, 4 * n); }
  std::memcpy(c->status, P.status.data(), n);
  const float* hPos = at<float>(ctx.hDown, dPos);
  const float* hNrm = at<float>(ctx.hDown, dNrm);
  const float* hMin = at<float>(ctx.hDown, dMin);
  const float* hMax = at<float>(ctx.hDown, dMax);
  const uint8_t* hSt = at<uint8_t>(ctx.hDown, dSt);
  for (size_t j = 0; j < nc; j++) {
    const size_t i = (size_t)P.entry[j];
    std::memcpy(c->pos_out + 3 * i, hPos + 3 * j, 12);
    c->status[i] = hSt[j];
    if (P.normals) { std::memcpy(c->normal + 3 * i, hNrm + 3 * j, 12); c->min_distance[i] = hMin[j]; c->max_distance[i] = hMax[j]; }
  }
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_export(ydorb_mapdb_t* h, int32_t* obs_start, int32_t* obs_kf, uint8_t* obs_level, uint8_t* bad, int32_t* ref_kf,
                                  uint8_t* ref_level, float* pos, float* centre) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  const size_t np = (size_t)h->host.nPoints(), nk = (size_t)h->host.nKeyframes();
  const size_t live = (size_t)h->host.liveAfterSync();
  if (!obs_start) return invalid("null obs_start");
  if (np > 0 && (!bad || !ref_kf || !ref_level || !pos)) return invalid("null bad, ref_kf, ref_level or pos");
  if (live > 0 && (!obs_kf || !obs_level)) return invalid("null obs_kf or obs_level");
  if (nk > 0 && !centre) return invalid("null centre");
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  StagedCtx& c = h->c;
  const size_t used = (size_t)h->host.poolUsed();
  mapdb::SlotTables H{};   // the read-back area in c.hDown: the table's columns, the centres, the used part of the pool
  int* hKf = nullptr;
  uint8_t* hLevel = nullptr;
  const auto lay = [&](void* base) {
    Carve C(base);
    layColumns<PointColumns>(C, H, np);
    C.take(H.centre, 3 * nk);
    return layPool(C, hKf, hLevel, used);
  };
  if ((rc = c.hDown.ensure(lay(nullptr)))) return rc;
  lay(c.hDown.p);
  hipStream_t s = c.stream;
  if ((rc = copyColumns<PointColumns>(s, hipMemcpyDeviceToHost, H, h->T, np)) ||
      (rc = copyAsync(H.centre, h->T.centre, 12 * nk, hipMemcpyDeviceToHost, s)) ||
      (rc = copyAsync(hKf, h->poolKf, 4 * used, hipMemcpyDeviceToHost, s)) || (rc = copyAsync(hLevel, h->poolLevel, used, hipMemcpyDeviceToHost, s)))
    return rc;
  HIPCHK(hipStreamSynchronize(s));
  mapdb::flatten((int32_t)np, H.start, H.end, hKf, hLevel, obs_start, obs_kf, obs_level);
  mapdb::SlotTables out{};   // start / end stay null: they went out through flatten
  out.refKf = ref_kf; out.pos = pos; out.bad = bad; out.refLevel = ref_level;
  copyColumns<PointColumns>(s, hipMemcpyHostToHost, out, H, np);
  if (nk) std::memcpy(centre, H.centre, 12 * nk);
  return YDORB_OK;
}

// ------------------------------------------------------------------------------------------------------------------ keyframe rows
extern "C" int ydorb_mapdb_set_keyframe_rows(ydorb_mapdb_t* h, const int32_t* kf_slots, int32_t n, const int32_t* row_start,
                                             const int32_t* point_slot) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!h->rows.setRows(kf_slots, n, row_start, point_slot, h->host.nPoints(), err)) return invalid(err);
  h->host.growKeyframes(h->rows.nKeyframes());
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_set_row_entries(ydorb_mapdb_t* h, const int32_t* kf_slot, const int32_t* idx, const int32_t* point_slot, int32_t n) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  return h->rows.setEntries(kf_slot, idx, point_slot, n, h->host.nPoints(), err) ? YDORB_OK : invalid(err);
}

extern "C" int ydorb_mapdb_row_stats(ydorb_mapdb_t* h, YdMapDbRowStats* stats) {
  if (!h || !stats) return invalid("null handle or stats");
  std::lock_guard<std::mutex> lock(h->c.mu);
  h->rows.stats(*stats);
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_export_rows(ydorb_mapdb_t* h, int32_t* row_start, int32_t* point_slot) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (!row_start) return invalid("null row_start");
  if (h->rows.liveAfterSync() > 0 && !point_slot) return invalid("null point_slot");
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  StagedCtx& c = h->c;
  const size_t held = (size_t)h->rows.nKeyframes();
  size_t dStart, dLen, dPool;
  if ((rc = h->dRows.download(c, held, (size_t)h->rows.poolUsed(), dStart, dLen, dPool))) return rc;
  mapdb::flattenRows(h->host.nKeyframes(), (int32_t)held, at<int32_t>(c.hDown, dStart), at<int32_t>(c.hDown, dLen), at<int32_t>(c.hDown, dPool),
                     row_start, point_slot);
  return YDORB_OK;
}

// sync; one upload of the keyframe slots, their starts in E and the seen list; mark, count, emit with no host round trip between
// them; one read-back; one synchronise.
extern "C" int ydorb_mapdb_points_of_keyframes(ydorb_mapdb_t* h, const int32_t* kf_slots, int32_t n_kf, const int32_t* seen_points,
                                               int32_t n_seen, int32_t capacity, int32_t* out_slots, uint8_t* out_seen, int32_t* count,
                                               uint8_t* status) {
  if (n_kf < 0 || n_seen < 0 || capacity < 0) return invalid("negative n_kf, n_seen or capacity");
  if (!count || !status) return invalid("null count or status");
  if ((n_kf > 0 && !kf_slots) || (n_seen > 0 && !seen_points)) return invalid("null kf_slots or seen_points");
  if (capacity > 0 && (!out_slots || !out_seen)) return invalid("null out_slots or out_seen");
  if (!h) {   // without a device no handle exists: say that, there is no CPU path to fall back to
    const int rc = require_device(0);
    return rc ? rc : invalid("null handle");
  }
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!mapdb::RowsHost::checkKfSlots(kf_slots, n_kf, h->host.nKeyframes(), err) ||
      !mapdb::RowsHost::checkSeen(seen_points, n_seen, h->host.nPoints(), err))
    return invalid(err);
  *count = 0; *status = 0;
  if (n_kf == 0) return YDORB_OK;
  const size_t nk = (size_t)n_kf, ns = (size_t)n_seen;
  std::vector<int32_t> eStart(nk + 1, 0);
  int64_t total = 0;
  for (size_t r = 0; r < nk; r++) {   // the mirror with its staged rows: what the device holds after the sync below
    total += h->rows.lenOf(kf_slots[r]);
    if (total > INT32_MAX) return invalid("the rows of kf_slots hold more than INT32_MAX entries");
    eStart[r + 1] = (int32_t)total;
  }
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  if (total == 0) return YDORB_OK;
  if ((rc = ensureRowset(h))) return rc;
  StagedCtx& c = h->c;
  hipStream_t s = c.stream;
  if ((rc = nextRowsetStamp(h))) return rc;
  const size_t nE = (size_t)total, nB = (nE + mapdb::kRowThreads - 1) / mapdb::kRowThreads, capOut = std::min<size_t>((size_t)capacity, nE);
  Layout U;
  const size_t oKf = U.add(4 * nk), oEs = U.add(4 * (nk + 1)), oSeen = U.add(4 * ns);
  Layout D;
  const size_t dSlots = D.add(4 * capOut), dSeen = D.add(capOut), dTotal = D.add(4);
  Layout W;
  const size_t wEnt = W.add(4 * nE), wBlock = W.add(4 * nB);
  U.add(16);
  if ((rc = c.ensure(U.bytes, D.bytes, W.bytes))) return rc;
  std::memcpy(at<void>(c.hUp, oKf), kf_slots, 4 * nk);
  std::memcpy(at<void>(c.hUp, oEs), eStart.data(), 4 * (nk + 1));
  if (ns) std::memcpy(at<void>(c.hUp, oSeen), seen_points, 4 * ns);
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  mapdb::RowsetArgs a;
  a.nKf = n_kf; a.nE = (int)nE; a.nSeen = n_seen; a.stamp = h->stamp; a.capacity = (int)capOut; a.nBlocks = (int)nB;
  a.kfSlots = at<int>(c.up, oKf); a.eStart = at<int>(c.up, oEs); a.seen = at<int>(c.up, oSeen);
  a.rowStart = h->dRows.start; a.rowLen = h->dRows.len; a.pool = h->dRows.pool; a.bad = h->T.bad;
  a.first = h->first; a.seenStamp = h->seenStamp;
  a.ent = at<int>(c.scratch, wEnt); a.blockTotal = at<int>(c.scratch, wBlock);
  a.outSlots = at<int>(c.down, dSlots); a.outSeen = at<uint8_t>(c.down, dSeen); a.total = at<int>(c.down, dTotal);
  if ((rc = launchRowset(s, a))) return rc;
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int32_t kept = *at<int32_t>(c.hDown, dTotal);
  *count = kept;
  if (kept > capacity) { *status = 1; return YDORB_OK; }
  if (kept) { std::memcpy(out_slots, at<void>(c.hDown, dSlots), 4 * (size_t)kept); std::memcpy(out_seen, at<void>(c.hDown, dSeen), (size_t)kept); }
  return YDORB_OK;
}

// k_covisibility with a self slot of -1 (no keyframe is excluded: a Frame is not in the table), over the lists without their -1 entries
extern "C" int ydorb_mapdb_observer_counter(ydorb_mapdb_t* h, int32_t n_lists, const int32_t* list_start, const int32_t* point_slots,
                                            const int32_t* out_start, int32_t* conn_kf, int32_t* conn_weight, int32_t* counts,
                                            uint8_t* status, uint8_t* point_bad) {
  std::string err;
  if (n_lists < 0) return invalid("negative number of lists: " + std::to_string(n_lists));
  if (!maptable::checkStarts("list_start", list_start, n_lists, err) || !maptable::checkStarts("out_start", out_start, n_lists, err)) return invalid(err);
  const int32_t L = list_start[n_lists];
  if (L > 0 && (!point_slots || !point_bad)) return invalid("null point_slots or point_bad");
  if (n_lists > 0 && (!counts || !status)) return invalid("null counts or status");
  if (out_start[n_lists] > 0 && (!conn_kf || !conn_weight)) return invalid("null conn_kf or conn_weight");
  if (!h) {
    const int rc = require_device(0);
    return rc ? rc : invalid("null handle");
  }
  std::lock_guard<std::mutex> lock(h->c.mu);
  for (int32_t e = 0; e < L; e++)
    if (point_slots[e] < -1 || point_slots[e] >= h->host.nPoints())
      return invalid("list entry " + std::to_string(e) + ": point slot " + std::to_string(point_slots[e]) + " outside -1.." + std::to_string(h->host.nPoints() - 1));
  if (n_lists == 0) return YDORB_OK;
  const size_t nl = (size_t)n_lists;
  std::vector<int32_t> self(nl, -1), ls(nl + 1, 0), idx;
  idx.reserve((size_t)L);
  for (size_t q = 0; q < nl; q++) {
    for (int32_t e = list_start[q]; e < list_start[q + 1]; e++) {
      const int32_t p = point_slots[e];
      point_bad[e] = p >= 0 && h->host.isBad(p) ? 1 : 0;   // the mirror with its staged points: what the device holds after the sync
      if (p >= 0) idx.push_back(p);
    }
    ls[q + 1] = (int32_t)idx.size();
  }
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  mapmaint::MapSource src = sourceOf(h);
  return mapmaint::runCovisibility(h->c, src, self.data(), n_lists, ls.data(), idx.data(), out_start, conn_kf, conn_weight, counts, status);
}

// ---------------------------------------------------------------------------------------------------------------- local BA graph
// sync; one upload of the keyframe slots, their starts in E and the sigma table; the rowset kernels, rank, mark, count, scan; a 16-byte
// read-back of the three counts and the first synchronise; the result area laid out for them; fixed, edges, reset; one read-back of
// what the device wrote into the pinned result and the second synchronise.  The point count is not read back on its own: mark, count
// and scan are launched over its bound min(|E|, n_points) and the lanes past the device-side count return.
extern "C" int ydorb_mapdb_local_ba_graph(ydorb_mapdb_t* h, const int32_t* kf_slots, int32_t n_kf, const float* inv_level_sigma2, YdLocalBaGraph* out) {
  if (!h) {   // without a device no handle exists: say that, there is no CPU path to fall back to
    const int rc = require_device(0);
    return rc ? rc : invalid("null handle");
  }
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!mapdb::checkLbaArgs(kf_slots, n_kf, inv_level_sigma2, out, h->host.nKeyframes(), h->feat.enabled(), h->lbaMark, err)) return invalid(err);
  HIPCHK(hipSetDevice(h->device));
  StagedCtx& c = h->c;
  hipStream_t s = c.stream;
  YdMapDbLbaStats st{};
  st.n_calls = h->lbaStats.n_calls + 1;
  st.last_n_local = n_kf;
  const size_t nk = (size_t)n_kf;
  int rc;
  std::vector<int32_t> eStart(nk + 1, 0);
  int64_t total = 0;
  for (size_t r = 0; r < nk; r++) {   // the mirror with its staged rows: what the device holds after the sync below
    total += h->rows.lenOf(kf_slots[r]);
    if (total > INT32_MAX) return invalid("the rows of kf_slots hold more than INT32_MAX entries");
    eStart[r + 1] = (int32_t)total;
  }
  if (n_kf > 0 && (rc = sync(h))) return rc;
  const size_t nE = (size_t)total, bound = std::min<size_t>(nE, (size_t)h->host.nPoints());
  if (bound == 0) {   // no keyframe (nothing synced: what is staged stays staged), or none with a row: the poses alone, nothing launched
    const mapdb::LbaLayout L(nk, 0, 0);
    if ((rc = h->lbaHost.ensure(L.bytes))) return rc;
    uint8_t* base = h->lbaHost.as<uint8_t>();
    std::memset(base, 0, L.bytes);
    if (nk) std::memcpy(base + L.oPoseKf, kf_slots, 4 * nk);
    mapdb::lbaPointResult(L, base, n_kf, 0, 0, 0, out);
    h->lbaStats = st;
    return YDORB_OK;
  }
  if ((rc = ensureRowset(h)) || (rc = nextRowsetStamp(h)) || (rc = ensureLbaTables(h))) return rc;
  const size_t nBr = (nE + mapdb::kRowThreads - 1) / mapdb::kRowThreads, nBp = (bound + mapdb::kLbaThreads - 1) / mapdb::kLbaThreads;
  Layout U;
  const size_t oKf = U.add(4 * nk), oEs = U.add(4 * (nk + 1)), oSigma = U.add(32);
  Layout W;
  const size_t wEnt = W.add(4 * nE), wBlock = W.add(4 * nBr), wSlots = W.add(4 * bound), wSeen = W.add(bound), wTotal = W.add(4), wStatus = W.add(bound),
               wEdgeCount = W.add(4 * bound), wWinCount = W.add(4 * bound), wEdgeOff = W.add(4 * bound), wWinOff = W.add(4 * bound),
               wBlockEdge = W.add(4 * nBp), wBlockWin = W.add(4 * nBp);
  if ((rc = c.ensure(U.bytes, 16, W.bytes))) return rc;
  std::memcpy(at<void>(c.hUp, oKf), kf_slots, 4 * nk);
  std::memcpy(at<void>(c.hUp, oEs), eStart.data(), 4 * (nk + 1));
  std::memcpy(at<void>(c.hUp, oSigma), inv_level_sigma2, 32);
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  st.last_upload_bytes = (int64_t)U.bytes;
  const bool timed = h->lbaProfiling;
  const auto stampEvent = [&](int i) { return timed ? hipEventRecord(h->lbaEvent[i], s) : hipSuccess; };
  HIPCHK(stampEvent(0));
  mapdb::RowsetArgs r;
  r.nKf = n_kf; r.nE = (int)nE; r.nSeen = 0; r.stamp = h->stamp; r.capacity = (int)bound; r.nBlocks = (int)nBr;
  r.kfSlots = at<int>(c.up, oKf); r.eStart = at<int>(c.up, oEs); r.seen = nullptr;
  r.rowStart = h->dRows.start; r.rowLen = h->dRows.len; r.pool = h->dRows.pool; r.bad = h->T.bad;
  r.first = h->first; r.seenStamp = h->seenStamp;
  r.ent = at<int>(c.scratch, wEnt); r.blockTotal = at<int>(c.scratch, wBlock);
  r.outSlots = at<int>(c.scratch, wSlots); r.outSeen = at<uint8_t>(c.scratch, wSeen); r.total = at<int>(c.scratch, wTotal);
  if ((rc = launchRowset(s, r))) return rc;
  HIPCHK(stampEvent(1));
  mapdb::LbaArgs a{};
  a.nLocal = n_kf; a.nKfAll = h->host.nKeyframes(); a.bound = (int)bound; a.nBlocks = (int)nBp;
  a.nViewHdr = h->desc.views.hdrCap(); a.nFeatHdr = h->feat.feats.hdrCap();
  a.invLevelSigma2 = at<float>(c.up, oSigma); a.kfSlots = at<int>(c.up, oKf);
  a.nPoints = r.total; a.pointSlot = r.outSlots;
  a.viewStart = h->dViews.start; a.viewLen = h->dViews.len; a.viewPool = h->dViews.pool;
  a.featStart = h->dFeats.start; a.featLen = h->dFeats.len;
  a.kps = reinterpret_cast<const YdKeyPoint*>(featKps(h->dFeats.pool));
  a.rightX = reinterpret_cast<const float*>(featRightX(h->dFeats.pool, h->feat.feats.poolCap()));
  a.pos = h->T.pos; a.poseOf = h->lbaPoseOf; a.first = h->lbaFirst;
  a.status = at<uint8_t>(c.scratch, wStatus); a.edgeCount = at<int>(c.scratch, wEdgeCount); a.winCount = at<int>(c.scratch, wWinCount);
  a.edgeOff = at<int>(c.scratch, wEdgeOff); a.winOff = at<int>(c.scratch, wWinOff);
  a.blockEdge = at<int>(c.scratch, wBlockEdge); a.blockWin = at<int>(c.scratch, wBlockWin); a.counts = c.down.as<int>();
  const auto blocks = [](size_t n) { return dim3((unsigned)std::max<size_t>((n + mapdb::kLbaThreads - 1) / mapdb::kLbaThreads, 1)); };
  const dim3 threads(mapdb::kLbaThreads);
  h->lbaDirty = true;   // until the reset below has run
  hipLaunchKernelGGL(mapdb::k_lba_rank, blocks(nk), threads, 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(mapdb::k_lba_mark, dim3((unsigned)nBp), threads, 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(mapdb::k_lba_count, dim3((unsigned)nBp), threads, 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(mapdb::k_lba_scan, dim3((unsigned)nBp), threads, 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(stampEvent(2));
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int32_t nP = c.hDown.as<int32_t>()[0], nEdges = c.hDown.as<int32_t>()[1], nFixed = c.hDown.as<int32_t>()[2];
  if (nP < 0 || (size_t)nP > bound || nEdges < 0 || nFixed < 0 || nFixed > a.nKfAll) {
    set_error("resident map table: local BA graph: counts %d points, %d edges, %d fixed keyframes are out of range", nP, nEdges, nFixed);
    return YDORB_ERR_HIP;
  }
  const mapdb::LbaLayout L(nk + (size_t)nFixed, (size_t)nP, (size_t)nEdges);
  if ((rc = h->lbaDev.ensure(L.devBytes)) || (rc = h->lbaHost.ensure(L.bytes))) return rc;
  Mem& d = h->lbaDev;
  a.outPoseFixed = at<uint8_t>(d, L.oPoseFixed); a.outPoseKf = at<int>(d, L.oPoseKf); a.outPointSlot = at<int>(d, L.oPointSlot);
  a.outStatus = at<uint8_t>(d, L.oStatus); a.outPoints = at<double>(d, L.oPoints);
  a.outEdgePose = at<int>(d, L.oEdgePose); a.outEdgePoint = at<int>(d, L.oEdgePoint); a.outEdgeKf = at<int>(d, L.oEdgeKf); a.outEdgeIdx = at<int>(d, L.oEdgeIdx);
  a.outMeas = at<double>(d, L.oMeas); a.outInfo = at<double>(d, L.oInfo);
  HIPCHK(stampEvent(3));
  hipLaunchKernelGGL(mapdb::k_lba_fixed, blocks(std::max((size_t)nP, nk)), threads, 0, s, a);
  HIPCHK(hipGetLastError());
  st.last_launches = 8;
  if (nP > 0) {
    hipLaunchKernelGGL(mapdb::k_lba_edges, blocks((size_t)nP), threads, 0, s, a);
    HIPCHK(hipGetLastError());
    st.last_launches++;
  }
  hipLaunchKernelGGL(mapdb::k_lba_reset, blocks((size_t)a.nKfAll), threads, 0, s, a.nKfAll, h->lbaPoseOf, h->lbaFirst);
  HIPCHK(hipGetLastError());
  st.last_launches++;
  HIPCHK(stampEvent(4));
  HIPCHK(hipMemcpyAsync(h->lbaHost.p, d.p, L.devBytes, hipMemcpyDeviceToHost, s));
  HIPCHK(stampEvent(5));
  HIPCHK(hipStreamSynchronize(s));
  h->lbaDirty = false;
  if (timed) {
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    HIPCHK(hipEventElapsedTime(&ms[0], h->lbaEvent[0], h->lbaEvent[1]));
    HIPCHK(hipEventElapsedTime(&ms[1], h->lbaEvent[1], h->lbaEvent[2]));
    HIPCHK(hipEventElapsedTime(&ms[2], h->lbaEvent[3], h->lbaEvent[4]));
    HIPCHK(hipEventElapsedTime(&ms[3], h->lbaEvent[4], h->lbaEvent[5]));
    st.last_ms_points = ms[0]; st.last_ms_walk = ms[1]; st.last_ms_emit = ms[2]; st.last_ms_copy = ms[3];
  }
  std::memset(h->lbaHost.as<uint8_t>() + L.oPoses, 0, L.bytes - L.oPoses);
  mapdb::lbaPointResult(L, h->lbaHost.as<uint8_t>(), n_kf, nFixed, nP, nEdges, out);
  st.last_syncs = 2; st.last_download_bytes = 16 + (int64_t)L.devBytes;
  st.last_n_fixed = nFixed; st.last_n_points = nP; st.last_n_edges = nEdges;
  h->lbaStats = st;
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_lba_stats(ydorb_mapdb_t* h, YdMapDbLbaStats* stats) {
  if (!h || !stats) return invalid("null handle or stats");
  std::lock_guard<std::mutex> lock(h->c.mu);
  *stats = h->lbaStats;
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_lba_set_profiling(ydorb_mapdb_t* h, int32_t on) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (on) {
    HIPCHK(hipSetDevice(h->device));
    for (hipEvent_t& e : h->lbaEvent) if (!e) HIPCHK(hipEventCreate(&e));
  }
  h->lbaProfiling = on != 0;
  return YDORB_OK;
}

// ------------------------------------------------------------------------------------------- point views and descriptor blocks
extern "C" int ydorb_mapdb_reserve_descriptors(ydorb_mapdb_t* h, int64_t view_capacity, int64_t descriptor_capacity) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!h->desc.reserve(view_capacity, descriptor_capacity, err)) return invalid(err);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->c.stream));   // nothing in flight reads the arenas given back below
  const int rc = h->dViews.allocPool(h->desc.views);
  return rc ? rc : h->dBlocks.allocPool(h->desc.blocks);
}

extern "C" int ydorb_mapdb_set_keyframe_descriptors(ydorb_mapdb_t* h, const int32_t* kf_slots, int32_t n, const int32_t* desc_start,
                                                    const uint8_t* desc) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!h->desc.setBlocks(kf_slots, n, desc_start, desc, err)) return invalid(err);
  h->host.growKeyframes(h->desc.blocks.nKeyframes());
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_set_point_views(ydorb_mapdb_t* h, const int32_t* slots, int32_t n, const int32_t* view_start, const int32_t* view_kf,
                                           const int32_t* view_idx) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  return h->desc.setViews(slots, n, view_start, view_kf, view_idx, h->host.nPoints(), h->host.nKeyframes(), err) ? YDORB_OK : invalid(err);
}

extern "C" int ydorb_mapdb_desc_stats(ydorb_mapdb_t* h, YdMapDbDescStats* stats) {
  if (!h || !stats) return invalid("null handle or stats");
  std::lock_guard<std::mutex> lock(h->c.mu);
  h->desc.stats(*stats);
  return YDORB_OK;
}

// sync; one upload of the slots; one wave per named point; one read-back; one synchronise.  No descriptor travels up.
extern "C" int ydorb_mapdb_distinctive_descriptors(ydorb_mapdb_t* h, const int32_t* slots, int32_t n, int32_t* best, int32_t* best_view,
                                                   uint8_t* desc_out, uint8_t* status) {
  std::string err;
  if (!mapdb::DescHost::checkQuery(slots, n, -1, best, best_view, desc_out, status, err)) return invalid(err);   // nulls and signs first
  if (!h) {   // without a device no handle exists: say that, there is no CPU path to fall back to
    const int rc = require_device(0);
    return rc ? rc : invalid("null handle");
  }
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (!mapdb::DescHost::checkQuery(slots, n, h->host.nPoints(), best, best_view, desc_out, status, err)) return invalid(err);
  if (n == 0) return YDORB_OK;
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  StagedCtx& c = h->c;
  const size_t nq = (size_t)n;
  Layout D;
  const size_t dDesc = D.add(32 * nq), dBest = D.add(4 * nq), dView = D.add(8 * nq), dSt = D.add(nq);
  if ((rc = c.ensure(4 * nq + 16, D.bytes))) return rc;
  std::memcpy(c.hUp.p, slots, 4 * nq);
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, 4 * nq, hipMemcpyHostToDevice, s));
  mapdb::DistinctiveArgs a;
  a.n = n; a.nViewHdr = h->desc.views.hdrCap(); a.nBlockHdr = h->desc.blocks.hdrCap();
  a.slots = c.up.as<int>(); a.bad = h->T.bad;
  a.viewStart = h->dViews.start; a.viewLen = h->dViews.len; a.viewPool = h->dViews.pool;
  a.blockStart = h->dBlocks.start; a.blockLen = h->dBlocks.len; a.blockPool = reinterpret_cast<const uint4*>(h->dBlocks.pool);
  a.best = at<int>(c.down, dBest); a.bestView = at<int>(c.down, dView); a.descOut = at<uint4>(c.down, dDesc); a.status = at<uint8_t>(c.down, dSt);
  hipLaunchKernelGGL(mapdb::k_mapdb_distinctive, dim3((unsigned)((nq + mapdb::kDescWaves - 1) / mapdb::kDescWaves)), dim3(mapdb::kDescThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(desc_out, at<void>(c.hDown, dDesc), 32 * nq); std::memcpy(best, at<void>(c.hDown, dBest), 4 * nq);
  std::memcpy(best_view, at<void>(c.hDown, dView), 8 * nq); std::memcpy(status, at<void>(c.hDown, dSt), nq);
  if (h->attr.enabled()) {   // the winning rows stay: see writeThroughGeometry for the ordering
    int64_t wrote = 0;
    for (size_t i = 0; i < nq; i++) wrote += status[i] == YDORB_MAPDESC_UPDATED;
    h->attr.wroteThrough(wrote);
    if (wrote) {
      hipLaunchKernelGGL(mapdb::k_attr_scatter_descriptor, dim3(attrBlocks(nq)), dim3(mapdb::kAttrThreads), 0, s, n, c.up.as<int>(), at<uint4>(c.down, dDesc),
                         at<uint8_t>(c.down, dSt), YDORB_MAPDESC_UPDATED, h->A);
      HIPCHK(hipGetLastError());
    }
  }
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_export_views(ydorb_mapdb_t* h, int32_t* view_start, int32_t* view_kf, int32_t* view_idx) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (!view_start) return invalid("null view_start");
  if (h->desc.views.liveAfterSync() > 0 && (!view_kf || !view_idx)) return invalid("null view_kf or view_idx");
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  size_t dStart, dLen, dPool;
  const size_t held = (size_t)h->desc.views.nKeyframes();
  if ((rc = h->dViews.download(h->c, held, (size_t)h->desc.views.poolUsed(), dStart, dLen, dPool))) return rc;
  mapdb::flattenViews(h->host.nPoints(), (int32_t)held, at<int32_t>(h->c.hDown, dStart), at<int32_t>(h->c.hDown, dLen), at<int32_t>(h->c.hDown, dPool),
                      view_start, view_kf, view_idx);
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_export_descriptors(ydorb_mapdb_t* h, int32_t* desc_start, uint8_t* desc) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (!desc_start) return invalid("null desc_start");
  if (h->desc.blocks.liveAfterSync() > 0 && !desc) return invalid("null desc");
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  size_t dStart, dLen, dPool;
  const size_t held = (size_t)h->desc.blocks.nKeyframes();
  if ((rc = h->dBlocks.download(h->c, held, (size_t)h->desc.blocks.poolUsed(), dStart, dLen, dPool))) return rc;
  mapdb::flattenRows(h->host.nKeyframes(), (int32_t)held, at<int32_t>(h->c.hDown, dStart), at<int32_t>(h->c.hDown, dLen),
                     at<mapdb::DescRow>(h->c.hDown, dPool), desc_start, reinterpret_cast<mapdb::DescRow*>(desc));
  return YDORB_OK;
}

// --------------------------------------------------------------------------------------------------------------- point attributes
extern "C" int ydorb_mapdb_enable_attributes(ydorb_mapdb_t* h) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (h->attr.enabled()) return YDORB_OK;
  HIPCHK(hipSetDevice(h->device));
  int rc = allocColumns<AttrColumns>(h->c.stream, h->attrMem, h->A, (size_t)h->host.pointCap());
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->c.stream));
  h->attr.enable(h->host.pointCap());
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_set_point_attributes(ydorb_mapdb_t* h, const int32_t* slots, int32_t n, const float* normal, const float* min_distance,
                                                const float* max_distance, const uint8_t* desc) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  return h->attr.set(slots, n, normal, min_distance, max_distance, desc, h->host.nPoints(), err) ? YDORB_OK : invalid(err);
}

extern "C" int ydorb_mapdb_attr_stats(ydorb_mapdb_t* h, YdMapDbAttrStats* stats) {
  if (!h || !stats) return invalid("null handle or stats");
  std::lock_guard<std::mutex> lock(h->c.mu);
  h->attr.stats(*stats);
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_export_attributes(ydorb_mapdb_t* h, float* normal, float* min_distance, float* max_distance, uint8_t* desc, uint8_t* flags) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!mapdb::AttrHost::checkEnabled(h->attr.enabled(), err)) return invalid(err);
  const size_t np = (size_t)h->host.nPoints();
  if (np > 0 && (!normal || !min_distance || !max_distance || !desc || !flags)) return invalid("null normal, min_distance, max_distance, desc or flags");
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  if (np == 0) return YDORB_OK;
  StagedCtx& c = h->c;
  mapdb::AttrArrays H{}, out{};   // the read-back area in c.hDown, and the caller's arrays
  out.normal = normal; out.minDistance = min_distance; out.maxDistance = max_distance; out.desc = reinterpret_cast<uint4*>(desc); out.flags = flags;
  Carve sz(nullptr);
  if ((rc = c.hDown.ensure(layColumns<AttrColumns>(sz, H, np)))) return rc;
  Carve cv(c.hDown.p);
  layColumns<AttrColumns>(cv, H, np);
  hipStream_t s = c.stream;
  if ((rc = copyColumns<AttrColumns>(s, hipMemcpyDeviceToHost, H, h->A, np))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  return copyColumns<AttrColumns>(s, hipMemcpyHostToHost, out, H, np);
}

// sync; one upload of views, list starts, slots and skip bytes; one lane per list entry; one read-back; one synchronise
extern "C" int ydorb_mapdb_frustum_cull(ydorb_mapdb_t* h, const YdFrustumView* views, int32_t n_views, const int32_t* list_start,
                                        const int32_t* point_slots, const uint8_t* skip, YdTrackView* rows, uint8_t* status, int32_t* n_in_view) {
  std::string err;
  if (n_views < 0) return invalid("negative number of views: " + std::to_string(n_views));
  if (!maptable::checkStarts("list_start", list_start, n_views, err)) return invalid(err);
  if (n_views > 0 && !views) return invalid("null views");
  const int32_t L = list_start[n_views];
  if (L > 0 && (!point_slots || !skip || !rows || !status)) return invalid("null point_slots, skip, rows or status");
  for (int32_t f = 0; f < n_views; f++)
    if (views[f].n_levels < 1 || views[f].n_levels > 8) return invalid("view " + std::to_string(f) + ": n_levels " + std::to_string(views[f].n_levels) + " outside 1..8");
  if (!h) {   // without a device no handle exists: say that, there is no CPU path to fall back to
    const int rc = require_device(0);
    return rc ? rc : invalid("null handle");
  }
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (!mapdb::AttrHost::checkEnabled(h->attr.enabled(), err) || !mapdb::AttrHost::checkSlots(point_slots, L, h->host.nPoints(), err)) return invalid(err);
  if (n_in_view) std::memset(n_in_view, 0, 4 * (size_t)n_views);
  if (L == 0) return YDORB_OK;
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  StagedCtx& c = h->c;
  const size_t nv = (size_t)n_views, nl = (size_t)L;
  Layout U;
  const size_t oViews = U.add(sizeof(YdFrustumView) * nv), oStart = U.add(4 * (nv + 1)), oSlots = U.add(4 * nl), oSkip = U.add(nl);
  Layout D;
  const size_t dRows = D.add(sizeof(YdTrackView) * nl), dSt = D.add(nl);
  if ((rc = c.ensure(U.bytes, D.bytes))) return rc;
  std::memcpy(at<void>(c.hUp, oViews), views, sizeof(YdFrustumView) * nv);
  std::memcpy(at<void>(c.hUp, oStart), list_start, 4 * (nv + 1));
  std::memcpy(at<void>(c.hUp, oSlots), point_slots, 4 * nl);
  std::memcpy(at<void>(c.hUp, oSkip), skip, nl);
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  frustum::ResidentCullArgs a;
  a.nViews = n_views; a.nEntries = L;
  a.start = at<int>(c.up, oStart); a.views = at<frustum::ViewDev>(c.up, oViews); a.slots = at<int>(c.up, oSlots); a.skip = at<uint8_t>(c.up, oSkip);
  a.rows = at<YdTrackView>(c.down, dRows); a.status = at<uint8_t>(c.down, dSt);
  a.R = residentOf(h);
  hipLaunchKernelGGL(frustum::k_mapdb_frustum_cull, dim3((unsigned)((nl + frustum::kThreads - 1) / frustum::kThreads)), dim3(frustum::kThreads), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(rows, at<void>(c.hDown, dRows), sizeof(YdTrackView) * nl);
  std::memcpy(status, at<void>(c.hDown, dSt), nl);
  if (n_in_view)
    for (int32_t f = 0; f < n_views; f++)
      for (int32_t e = list_start[f]; e < list_start[f + 1]; e++) n_in_view[f] += status[e] == YDORB_FRUSTUM_IN_VIEW;
  return YDORB_OK;
}

// ------------------------------------------------------------------------------------------------------------- keyframe features
extern "C" int ydorb_mapdb_enable_features(ydorb_mapdb_t* h) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (h->feat.enabled()) return YDORB_OK;
  HIPCHK(hipSetDevice(h->device));
  const int rc = h->dFeats.alloc(h->c.stream, h->feat.feats);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->c.stream));
  h->feat.enable();
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_set_keyframe_features(ydorb_mapdb_t* h, const int32_t* kf_slots, int32_t n, const int32_t* feat_start,
                                                 const YdKeyPoint* kps, const float* right_x) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!h->feat.set(kf_slots, n, feat_start, kps, right_x, err)) return invalid(err);
  h->host.growKeyframes(h->feat.feats.nKeyframes());
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_feat_stats(ydorb_mapdb_t* h, YdMapDbFeatStats* stats) {
  if (!h || !stats) return invalid("null handle or stats");
  std::lock_guard<std::mutex> lock(h->c.mu);
  h->feat.stats(*stats);
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_export_features(ydorb_mapdb_t* h, int32_t* feat_start, YdKeyPoint* kps, float* right_x) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!mapdb::FeatHost::checkEnabled(h->feat.enabled(), err)) return invalid(err);
  if (!feat_start) return invalid("null feat_start");
  if (h->feat.feats.liveAfterSync() > 0 && (!kps || !right_x)) return invalid("null kps or right_x");
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  StagedCtx& c = h->c;
  const size_t held = (size_t)h->feat.feats.nKeyframes(), used = (size_t)h->feat.feats.poolUsed();
  mapdb::FeatRec* pool = h->dFeats.pool;
  PoolPart part[2] = {{featKps(pool), sizeof(YdKeyPoint) * used, 0}, {featRightX(pool, h->feat.feats.poolCap()), 4 * used, 0}};   // the arena's two arrays
  size_t dStart, dLen;
  if ((rc = h->dFeats.download(c, held, dStart, dLen, part))) return rc;
  mapdb::flattenFeatures(h->host.nKeyframes(), (int32_t)held, at<int32_t>(c.hDown, dStart), at<int32_t>(c.hDown, dLen), at<YdKeyPoint>(c.hDown, part[0].at),
                         at<float>(c.hDown, part[1].at), feat_start, kps, right_x);
  return YDORB_OK;
}

// ------------------------------------------------------------------------------------------------------- BoW feature vectors
extern "C" int ydorb_mapdb_enable_bow(ydorb_mapdb_t* h) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  if (h->bow.enabled()) return YDORB_OK;
  HIPCHK(hipSetDevice(h->device));
  const int rc = h->dBow.alloc(h->c.stream, h->bow.spans);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->c.stream));
  h->bow.enable();
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_set_keyframe_bow(ydorb_mapdb_t* h, const int32_t* kf_slots, int32_t n, const int32_t* bow_start,
                                            const uint32_t* node_id, const int32_t* feat) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!h->bow.set(kf_slots, n, bow_start, node_id, feat, err)) return invalid(err);
  h->host.growKeyframes(h->bow.spans.nKeyframes());
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_bow_stats(ydorb_mapdb_t* h, YdMapDbBowStats* stats) {
  if (!h || !stats) return invalid("null handle or stats");
  std::lock_guard<std::mutex> lock(h->c.mu);
  h->bow.stats(*stats);
  return YDORB_OK;
}

extern "C" int ydorb_mapdb_export_bow(ydorb_mapdb_t* h, int32_t* bow_start, uint32_t* node_id, int32_t* feat) {
  if (!h) return invalid("null handle");
  std::lock_guard<std::mutex> lock(h->c.mu);
  std::string err;
  if (!mapdb::BowHost::checkEnabled(h->bow.enabled(), err)) return invalid(err);
  if (!bow_start) return invalid("null bow_start");
  if (h->bow.spans.liveAfterSync() > 0 && (!node_id || !feat)) return invalid("null node_id or feat");
  HIPCHK(hipSetDevice(h->device));
  int rc = sync(h);
  if (rc) return rc;
  size_t dStart, dLen, dPool;
  const size_t held = (size_t)h->bow.spans.nKeyframes();
  if ((rc = h->dBow.download(h->c, held, (size_t)h->bow.spans.poolUsed(), dStart, dLen, dPool))) return rc;
  mapdb::flattenBow(h->host.nKeyframes(), (int32_t)held, at<int32_t>(h->c.hDown, dStart), at<int32_t>(h->c.hDown, dLen),
                    at<mapdb::BowRec>(h->c.hDown, dPool), bow_start, node_id, feat);
  return YDORB_OK;
}

// What ydorb_mapdb_search_local_points (orb_matcher.hip) reads: mapdb_resident_points.h
int ydorb::mapdb::lockResident(ydorb_mapdb_t* h, int32_t device, const int32_t* slots, int32_t n, ResidentPoints& out) {
  std::unique_lock<std::mutex> lock(h->c.mu);
  std::string err;
  if (!AttrHost::checkEnabled(h->attr.enabled(), err) || !AttrHost::checkSlots(slots, n, h->host.nPoints(), err)) return invalid(err);
  if (device != h->device) return invalid("the map table lives on device " + std::to_string(h->device) + ", the matcher on device " + std::to_string(device));
  if (n > 0) {   // an empty list reads nothing: nothing is applied or launched for it
    HIPCHK(hipSetDevice(h->device));
    int rc = sync(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->c.stream));   // the delta and any write-through still queued: the reader runs on another stream
  }
  out = residentOf(h);
  lock.release();   // held until unlockResident
  return YDORB_OK;
}
void ydorb::mapdb::unlockResident(ydorb_mapdb_t* h) { h->c.mu.unlock(); }

// What ydorb_mapdb_fuse_search (orb_matcher.hip) reads
int ydorb::mapdb::lockResidentFuse(ydorb_mapdb_t* h, int32_t device, const int32_t* slots, int32_t n, const int32_t* kfSlots, int32_t nKf,
                                   ResidentPoints& out, ResidentKeyframes& kf, int32_t* featStart, int32_t* featLen, int32_t* blockStart,
                                   int32_t* blockLen) {
  std::unique_lock<std::mutex> lock(h->c.mu);
  std::string err;
  if (!AttrHost::checkEnabled(h->attr.enabled(), err) || !FeatHost::checkEnabled(h->feat.enabled(), err) ||
      !AttrHost::checkSlots(slots, n, h->host.nPoints(), err) || !RowsHost::checkKfSlots(kfSlots, nKf, h->host.nKeyframes(), err))
    return invalid(err);
  if (device != h->device) return invalid("the map table lives on device " + std::to_string(h->device) + ", the matcher on device " + std::to_string(device));
  if (n > 0) {   // an empty list reads nothing: nothing is applied or launched for it
    HIPCHK(hipSetDevice(h->device));
    int rc = sync(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->c.stream));   // the deltas and any write-through still queued: the reader runs on another stream
    for (int32_t t = 0; t < nKf; t++) {          // nothing is staged now: the mirrors say where the device holds each span
      featStart[t] = h->feat.feats.offOf(kfSlots[t]); featLen[t] = h->feat.feats.lenOf(kfSlots[t]);
      blockStart[t] = h->desc.blocks.offOf(kfSlots[t]); blockLen[t] = h->desc.blocks.lenOf(kfSlots[t]);
    }
  }
  out = residentOf(h);
  kf.obsKf = h->poolKf;
  kf.nFeatHdr = h->feat.feats.hdrCap(); kf.nBlockHdr = h->desc.blocks.hdrCap();
  kf.featStart = h->dFeats.start; kf.featLen = h->dFeats.len;
  kf.kps = h->dFeats.pool; kf.rightX = reinterpret_cast<const float*>(featRightX(h->dFeats.pool, h->feat.feats.poolCap()));
  kf.blockStart = h->dBlocks.start; kf.blockLen = h->dBlocks.len; kf.blockPool = reinterpret_cast<const uint8_t*>(h->dBlocks.pool);
  lock.release();   // held until unlockResident
  return YDORB_OK;
}

// Where the device holds the four spans of keyframe k after a sync, from the host mirrors, and whether a BoW-guided search can use the
// keyframe on its own: a YDORB_CREATE_NB_* / YDORB_BOW_PAIR_* value (0 = usable).  nExtra >= 0: one more length that must equal the
// feature count (createNewPoints' depth array).  Both locks below apply this rule and no other.
static uint8_t residentKeyframeSpans(const ydorb_mapdb* h, int32_t k, int32_t nExtra, ydorb::mapdb::ResidentTriSpans& S) {
  S.featStart = h->feat.feats.offOf(k); S.n = h->feat.feats.lenOf(k);
  S.blockStart = h->desc.blocks.offOf(k); S.rowStart = h->rows.offOf(k);
  S.bowStart = h->bow.spans.offOf(k); S.bowLen = h->bow.spans.lenOf(k);
  if (S.n == 0) return YDORB_CREATE_NB_NO_FEATURES;
  if (h->desc.blocks.lenOf(k) == 0) return YDORB_CREATE_NB_NO_BLOCK;
  if (S.bowLen == 0) return YDORB_CREATE_NB_NO_BOW;
  if (h->desc.blocks.lenOf(k) != S.n || h->rows.lenOf(k) != S.n || (nExtra >= 0 && nExtra != S.n)) return YDORB_CREATE_NB_LENGTH_MISMATCH;
  for (const ydorb::mapdb::BowRec& r : h->bow.spans.rowOf(k))
    if (r.feat >= S.n) return YDORB_CREATE_NB_BOW_INDEX;
  return YDORB_CREATE_NB_OK;
}
static_assert(YDORB_BOW_PAIR_OK == YDORB_CREATE_NB_OK && YDORB_BOW_PAIR_NO_FEATURES == YDORB_CREATE_NB_NO_FEATURES && YDORB_BOW_PAIR_NO_BLOCK == YDORB_CREATE_NB_NO_BLOCK &&
                  YDORB_BOW_PAIR_NO_BOW == YDORB_CREATE_NB_NO_BOW && YDORB_BOW_PAIR_LENGTH_MISMATCH == YDORB_CREATE_NB_LENGTH_MISMATCH &&
                  YDORB_BOW_PAIR_BOW_INDEX == YDORB_CREATE_NB_BOW_INDEX,
              "one usability rule, one set of values");

static void residentTriPoolsOf(const ydorb_mapdb* h, ydorb::mapdb::ResidentTriPools& pools) {
  pools.rowPool = h->dRows.pool; pools.bowPool = reinterpret_cast<const int32_t*>(h->dBow.pool);
  pools.kps = h->dFeats.pool; pools.rightX = reinterpret_cast<const float*>(featRightX(h->dFeats.pool, h->feat.feats.poolCap()));
  pools.blockPool = reinterpret_cast<const uint8_t*>(h->dBlocks.pool);
}

// What ydorb_mapdb_create_new_points (orb_matcher.hip) reads
int ydorb::mapdb::lockResidentTri(ydorb_mapdb_t* h, int32_t device, const int32_t* kfSlots, const int32_t* nDepth, int32_t nNb, ResidentTriPools& pools,
                                  ResidentTriSpans* spans, uint8_t* status) {
  std::unique_lock<std::mutex> lock(h->c.mu);
  std::string err;
  if (!FeatHost::checkEnabled(h->feat.enabled(), err) || !BowHost::checkEnabled(h->bow.enabled(), err) ||
      !RowsHost::checkKfSlots(kfSlots, nNb + 1, h->host.nKeyframes(), err))
    return invalid(err);
  if (device != h->device) return invalid("the map table lives on device " + std::to_string(h->device) + ", the matcher on device " + std::to_string(device));
  if (nDepth[0] != h->feat.feats.lenOf(kfSlots[0]))
    return invalid("the first keyframe has " + std::to_string(h->feat.feats.lenOf(kfSlots[0])) + " resident features, n is " + std::to_string(nDepth[0]));
  for (int32_t i = 1; i <= nNb; i++) {
    if (kfSlots[i] == kfSlots[0]) return invalid("neighbour " + std::to_string(i - 1) + " is the first keyframe");
    for (int32_t j = 1; j < i; j++)
      if (kfSlots[j] == kfSlots[i]) return invalid("neighbours " + std::to_string(j - 1) + " and " + std::to_string(i - 1) + " name keyframe slot " + std::to_string(kfSlots[i]) + " twice");
  }
  if (nNb > 0) {   // no neighbour reads nothing: nothing is applied or launched for it
    HIPCHK(hipSetDevice(h->device));
    int rc = sync(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->c.stream));   // the deltas and any write-through still queued: the reader runs on another stream
    for (int32_t i = 0; i <= nNb; i++)           // nothing is staged now: the mirrors say where the device holds each span
      status[i] = residentKeyframeSpans(h, kfSlots[i], nDepth[i], spans[i]);
  }
  residentTriPoolsOf(h, pools);
  lock.release();   // held until unlockResident
  return YDORB_OK;
}

// What ydorb_mapdb_search_by_bow_keyframes / _frame (orb_matcher.hip) read.  Descriptor blocks and rows are not opt-in, so only features
// and BoW feature vectors can be "not enabled".
int ydorb::mapdb::lockResidentBow(ydorb_mapdb_t* h, int32_t device, const int32_t* kfSlots, int32_t nKf, int32_t nSearched, int32_t nFirst, ResidentBowPools& pools,
                                  ResidentTriSpans* spans, uint8_t* status) {
  std::unique_lock<std::mutex> lock(h->c.mu);
  std::string err;
  if (!FeatHost::checkEnabled(h->feat.enabled(), err) || !BowHost::checkEnabled(h->bow.enabled(), err)) return invalid(err);
  for (int32_t i = 0; i < nKf; i++)
    if (kfSlots[i] < 0 || kfSlots[i] >= h->host.nKeyframes())
      return invalid((nFirst < 0 ? "kf_slots[" + std::to_string(i) + "]" : i == 0 ? std::string("first_kf_slot") : "second_kf_slots[" + std::to_string(i - 1) + "]") +
                     ": keyframe slot " + std::to_string(kfSlots[i]) + " outside 0.." + std::to_string((long long)h->host.nKeyframes() - 1));
  if (device != h->device) return invalid("the map table lives on device " + std::to_string(h->device) + ", the matcher on device " + std::to_string(device));
  if (nFirst >= 0 && nFirst != h->feat.feats.lenOf(kfSlots[0]))
    return invalid("the first keyframe has " + std::to_string(h->feat.feats.lenOf(kfSlots[0])) + " resident features, n_first is " + std::to_string(nFirst));
  if (nSearched > 0) {   // no candidate reads nothing: nothing is applied or launched for it
    HIPCHK(hipSetDevice(h->device));
    int rc = sync(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->c.stream));   // the deltas and any write-through still queued: the reader runs on another stream
    for (int32_t i = 0; i < nKf; i++) status[i] = residentKeyframeSpans(h, kfSlots[i], -1, spans[i]);
  }
  residentTriPoolsOf(h, pools.tri);
  pools.bad = h->T.bad; pools.pointCap = h->host.pointCap();
  lock.release();   // held until unlockResident
  return YDORB_OK;
}
