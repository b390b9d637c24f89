// gfx950 HIP kernels that keep the plain span relations of the resident map table on the device: the keyframe rows (DESIGN.md section
// 6o), the point views and the keyframe descriptor blocks (section 6p).  A relation is a header pair (start / length per slot) over one
// pool of elements (mapdb_rows_host.h's SpanHost<T>); the two kernels are templates over the unit U a lane moves and the units per
// element: <int, 1> for the int32 spans (rows, views), <uint4, 2> for the 32-byte descriptor rows.
//   k_mapdb_span_apply    executes one packed delta: lane i below the record count scatters header record i (start / length of its
//                         slot) or, in the int instantiation only, single entry i (one pool position; block deltas have no entry
//                         records), then all lanes stride over the payload, one unit each, into the pool's tail.  The host coalesced
//                         the delta: no two lanes store to one address.  Plain vector stores, no atomics.
//   k_mapdb_span_repack   one wave per header slot, lanes striding over the span's units, from the old arena to the offset the host
//                         computed in the new one.  A span the delta replaces carries -1 and is left to the apply.
// The keyframe features (mapdb_feat_kernels.hip.h) keep kernels of their own: one span indexes two arrays there, so their apply is one
// wave per header record, which splits each 32-byte payload element into the two.  That is another parallel shape, not another unit.
// Every index is bounded by the host: a header record's slot is below the header capacity, tail + payload and a survivor's new offset
// + length are at most the pool capacity (SpanPool::plan).  Integers only, no LDS, no inline assembly, no device-side assert / printf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mapdb_rows_host.h"

namespace ydorb {
namespace mapdb {

constexpr int kSpanThreads = 256;
constexpr int kSpanWaves = kSpanThreads / 64;

template <class U> struct SpanApplyArgs {
  int nHeaderRec, nEntryRec, tail;   // tail: in elements
  long long nPayload;                // in units
  const RowHeaderRec* header;
  const RowEntryRec* entry;          // int spans only
  const U* payload;
  int* start;   // [hdrCap]
  int* len;     // [hdrCap]
  U* pool;      // [kPer * poolCap]
};

template <class U, int kPer> static __global__ __launch_bounds__(kSpanThreads) void k_mapdb_span_apply(SpanApplyArgs<U> g) {
  const int gid = blockIdx.x * kSpanThreads + threadIdx.x, stride = gridDim.x * kSpanThreads;
  if (gid < g.nHeaderRec) {
    const RowHeaderRec r = g.header[gid];
    g.start[r.kf] = r.start; g.len[r.kf] = r.len;
  } else if constexpr (std::is_same<U, int>::value) {
    if (gid < g.nHeaderRec + g.nEntryRec) {
      const RowEntryRec r = g.entry[gid - g.nHeaderRec];
      g.pool[r.at] = r.value;
    }
  }
  U* to = g.pool + kPer * (size_t)g.tail;
  for (long long i = gid; i < g.nPayload; i += stride) to[i] = g.payload[i];
}

template <class U> struct SpanRepackArgs {
  int nSlots;
  int* start;          // [nSlots] rewritten
  const int* len;      // [nSlots]
  const int* newOff;   // [nSlots] -1: the span does not survive
  const U* oldPool;
  U* newPool;
};

template <class U, int kPer> static __global__ __launch_bounds__(kSpanThreads) void k_mapdb_span_repack(SpanRepackArgs<U> g) {
  const int k = blockIdx.x * kSpanWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= g.nSlots) return;   // uniform over the wave
  const int to = g.newOff[k];
  if (to < 0) return;
  const U* src = g.oldPool + kPer * (size_t)g.start[k];
  U* dst = g.newPool + kPer * (size_t)to;
  const long long n = kPer * (long long)g.len[k];
  for (long long q = lane; q < n; q += 64) dst[q] = src[q];
  if (lane == 0) g.start[k] = to;
}

}  // namespace mapdb
}  // namespace ydorb
