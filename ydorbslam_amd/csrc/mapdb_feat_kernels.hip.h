// gfx950 HIP kernels of the resident table's keyframe features (include/ydorb/c_api.h, "Resident keyframe features"; DESIGN.md section
// 6r; mapdb_feat_host.h has the layout).  One span per keyframe indexes two arrays of one arena: KeyPoint [cap] and right_x [cap].
//   k_mapdb_feat_apply    executes one packed delta, one wave per header record: lane 0 scatters the record (start / length of its
//                         keyframe slot), then the wave's lanes stride over the record's own payload elements, which the host packed
//                         at [start - tail, start - tail + len): a lane loads one 32-byte element as two uint4 and stores the seven
//                         words of the keypoint to the first array and right_x to the second.  The host coalesced the delta: one
//                         record per keyframe slot, spans disjoint, so no two lanes store to one address.
//   k_mapdb_feat_repack   one wave per keyframe slot, lanes striding over the span's keypoint words and right_x entries, from the old
//                         arena to the offset the host computed in the new one.  A span the delta replaces carries -1 and is left
//                         to the apply.
// Every index is bounded by the host: a header record's slot is below the header capacity, start + len is at most the pool capacity
// (SpanPool::plan), a survivor's new offset + len is at most the new capacity.  Plain vector stores, integers only, no LDS, no inline
// assembly, no device-side assert / printf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapdb_feat_host.h"

namespace ydorb {
namespace mapdb {

constexpr int kFeatThreads = 256;
constexpr int kFeatWaves = kFeatThreads / 64;

struct FeatApplyArgs {
  int nHeaderRec, tail;          // tail: in pool entries
  const RowHeaderRec* header;
  const uint4* payload;          // [nPayload][2]
  int* featStart;                // [hdrCap]
  int* featLen;                  // [hdrCap]
  uint32_t* kps;                 // [poolCap][7]
  uint32_t* rightX;              // [poolCap]
};

static __global__ __launch_bounds__(kFeatThreads) void k_mapdb_feat_apply(FeatApplyArgs g) {
  const int r = blockIdx.x * kFeatWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= g.nHeaderRec) return;   // uniform over the wave
  const RowHeaderRec h = g.header[r];
  if (lane == 0) { g.featStart[h.kf] = h.start; g.featLen[h.kf] = h.len; }
  const uint4* from = g.payload + 2 * (size_t)(h.start - g.tail);
  for (int q = lane; q < h.len; q += 64) {
    const uint4 a = from[2 * (size_t)q], b = from[2 * (size_t)q + 1];
    uint32_t* k = g.kps + 7 * ((size_t)h.start + (size_t)q);
    k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w; k[4] = b.x; k[5] = b.y; k[6] = b.z;
    g.rightX[(size_t)h.start + (size_t)q] = b.w;
  }
}

struct FeatRepackArgs {
  int nKf;
  int* featStart;          // [nKf] rewritten
  const int* featLen;      // [nKf]
  const int* newOff;       // [nKf] -1: the span does not survive
  const uint32_t *oldKps, *oldRightX;
  uint32_t *newKps, *newRightX;
};

static __global__ __launch_bounds__(kFeatThreads) void k_mapdb_feat_repack(FeatRepackArgs g) {
  const int k = blockIdx.x * kFeatWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= g.nKf) return;   // uniform over the wave
  const int to = g.newOff[k];
  if (to < 0) return;
  const int b = g.featStart[k], len = g.featLen[k];
  const uint32_t* src = g.oldKps + 7 * (size_t)b;
  uint32_t* dst = g.newKps + 7 * (size_t)to;
  for (long long w = lane; w < 7 * (long long)len; w += 64) dst[w] = src[w];
  for (int q = lane; q < len; q += 64) g.newRightX[(size_t)to + (size_t)q] = g.oldRightX[(size_t)b + (size_t)q];
  if (lane == 0) g.featStart[k] = to;
}

}  // namespace mapdb
}  // namespace ydorb
