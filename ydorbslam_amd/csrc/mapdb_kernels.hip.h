// gfx950 HIP kernels of the resident map table (include/ydorb/c_api.h, "Resident map table").  The three passes
// over the table are map_kernels.hip.h's; these two keep the table.
//   k_mapdb_apply   executes one packed delta (mapdb_host.h): lane i < nFixed scatters fixed record i (point, position or centre) into
//                   the slot tables, then all lanes stride over the payload and copy it to the pool's tail.  The host coalesced the
//                   delta, so no two records name one slot and no two lanes write one address: plain vector stores, no atomics.
//   k_mapdb_repack  one lane per point slot copies its live span from the old arena to the offset the host computed in the new one
//                   and rewrites the slot's start / end; a span of kLongSpan entries or more is copied by the slot's whole wave
//                   instead, lanes striding over it, one such span after the other.  Spans are a handful of entries for most points
//                   (4-8 at the sizes of DESIGN.md 6m), where a wave per span would idle most of its lanes; a long span copied by one
//                   lane is 64 times the serial work and uncoalesced.  A slot the delta replaces carries -1 and is left to
//                   k_mapdb_apply.
// Every index is bounded by the host before the launch: slots below the table capacities, tail + nPayload and every new offset + length
// within the pool's capacity.  No inline assembly, no device-side assert / printf, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapdb_host.h"

namespace ydorb {
namespace mapdb {

constexpr int kThreads = 256;
constexpr int kLongSpan = 64;   // k_mapdb_repack: from this length on a span is copied by its wave, not by its lane

struct SlotTables {
  int* start;          // [pointCap]
  int* end;            // [pointCap]
  int* refKf;          // [pointCap]
  float* pos;          // [pointCap][3]
  uint8_t* bad;        // [pointCap]
  uint8_t* refLevel;   // [pointCap]
  float* centre;       // [kfCap][3]
};

struct ApplyArgs {
  SlotTables t;
  int nPointRec, nPosRec, nCentreRec, nPayload, tail;
  const PointRec* point;
  const Vec3Rec* position;
  const Vec3Rec* centre;
  const int* payKf;
  const uint8_t* payLevel;
  int* poolKf;
  uint8_t* poolLevel;
};

static __global__ __launch_bounds__(kThreads) void k_mapdb_apply(ApplyArgs g) {
  const int gid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  if (gid < g.nPointRec) {
    const PointRec r = g.point[gid];
    g.t.start[r.slot] = r.off; g.t.end[r.slot] = r.off + r.len; g.t.refKf[r.slot] = r.refKf;
    g.t.pos[3 * r.slot] = r.pos[0]; g.t.pos[3 * r.slot + 1] = r.pos[1]; g.t.pos[3 * r.slot + 2] = r.pos[2];
    g.t.bad[r.slot] = r.bad; g.t.refLevel[r.slot] = r.refLevel;
  } else if (gid < g.nPointRec + g.nPosRec) {
    const Vec3Rec r = g.position[gid - g.nPointRec];
    g.t.pos[3 * r.slot] = r.v[0]; g.t.pos[3 * r.slot + 1] = r.v[1]; g.t.pos[3 * r.slot + 2] = r.v[2];
  } else if (gid < g.nPointRec + g.nPosRec + g.nCentreRec) {
    const Vec3Rec r = g.centre[gid - g.nPointRec - g.nPosRec];
    g.t.centre[3 * r.slot] = r.v[0]; g.t.centre[3 * r.slot + 1] = r.v[1]; g.t.centre[3 * r.slot + 2] = r.v[2];
  }
  for (int i = gid; i < g.nPayload; i += stride) {
    g.poolKf[g.tail + i] = g.payKf[i];
    g.poolLevel[g.tail + i] = g.payLevel[i];
  }
}

struct RepackArgs {
  int nPoints;
  int* start;                 // [nPoints] rewritten
  int* end;                   // [nPoints] rewritten
  const int* newOff;          // [nPoints] -1: the slot's span does not survive
  const int* oldKf;
  const uint8_t* oldLevel;
  int* newKf;
  uint8_t* newLevel;
};

static __global__ __launch_bounds__(kThreads) void k_mapdb_repack(RepackArgs g) {
  const int p = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63;
  int to = -1, b = 0, len = 0;
  if (p < g.nPoints) {
    to = g.newOff[p];
    if (to >= 0) { b = g.start[p]; len = g.end[p] - b; }
  }
  const bool isLong = len >= kLongSpan;
  if (!isLong)
    for (int q = 0; q < len; q++) {
      g.newKf[to + q] = g.oldKf[b + q];
      g.newLevel[to + q] = g.oldLevel[b + q];
    }
  // the wave's long spans, one after the other, all lanes striding over each (no lane has left: the ballot and shuffles are wave-wide)
  for (unsigned long long m = __ballot(isLong); m; m &= m - 1) {
    const int src = __ffsll((long long)m) - 1;
    const int b0 = __shfl(b, src), len0 = __shfl(len, src), to0 = __shfl(to, src);
    for (int q = lane; q < len0; q += 64) {
      g.newKf[to0 + q] = g.oldKf[b0 + q];
      g.newLevel[to0 + q] = g.oldLevel[b0 + q];
    }
  }
  if (to >= 0) { g.start[p] = to; g.end[p] = to + len; }
}

}  // namespace mapdb
}  // namespace ydorb
