// gfx950 HIP kernels of the resident table's point attributes (mapdb_attr_host.h): the apply of a packed delta
// and the three write-through scatters that follow ydorb_mapdb_update_normal_depth, ydorb_mapdb_correct and
// ydorb_mapdb_distinctive_descriptors on the handle's stream.  One lane per record or per query entry, plain vector stores, no LDS, no
// atomics.  All four are bound by launch latency at the sizes they run at: a record is 64 bytes, an entry at most 36.
//   k_mapdb_attr_apply       the host coalesces: no two records name one slot, so no two lanes store to one address.
//   k_attr_scatter_*         a slot repeated within one query stores the same value twice: every entry of a slot is computed from the
//                            same table by the same code, so the lanes that race write equal bytes (and ydorb_mapdb_correct's claim
//                            pass leaves one entry per slot anyway).
// Slots were validated on the host against n_points, and the arena covers the point table's capacity.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapdb_attr_host.h"

namespace ydorb {
namespace mapdb {

constexpr int kAttrThreads = 256;

struct AttrArrays {   // the arena, [capacity] each
  float *normal, *minDistance, *maxDistance;
  uint4* desc;        // [2] per slot
  uint8_t* flags;
};

static __global__ __launch_bounds__(kAttrThreads) void k_mapdb_attr_apply(int n, const AttrRec* __restrict__ rec, AttrArrays A) {
  const int i = blockIdx.x * kAttrThreads + threadIdx.x;
  if (i >= n) return;
  const uint4* r = reinterpret_cast<const uint4*>(rec + i);   // a record is four uint4
  const uint4 head = r[0], geo = r[1];
  const int slot = (int)head.x;
  const unsigned set = head.y & 0xffu, clear = (head.y >> 8) & 0xffu;
  const bool g = (set & kAttrGeometry) != 0, d = (set & kAttrDescriptor) != 0;
  if (g || clear) {   // a clear stores the zeros the host packed
    A.normal[3 * slot] = __uint_as_float(head.z); A.normal[3 * slot + 1] = __uint_as_float(head.w); A.normal[3 * slot + 2] = __uint_as_float(geo.x);
    A.minDistance[slot] = __uint_as_float(geo.y); A.maxDistance[slot] = __uint_as_float(geo.z);
  }
  if (d || clear) { A.desc[2 * slot] = r[2]; A.desc[2 * slot + 1] = r[3]; }
  A.flags[slot] = (uint8_t)((clear ? 0u : A.flags[slot]) | set);
}

// normal [n][3], minDistance / maxDistance [n], status [n]: a query's device result buffer; entries with status == want are copied
static __global__ __launch_bounds__(kAttrThreads) void k_attr_scatter_geometry(int n, const int* __restrict__ slots, const float* __restrict__ normal,
                                                                               const float* __restrict__ minDistance, const float* __restrict__ maxDistance,
                                                                               const uint8_t* __restrict__ status, int want, AttrArrays A) {
  const int i = blockIdx.x * kAttrThreads + threadIdx.x;
  if (i >= n || status[i] != want) return;
  const int slot = slots[i];
  A.normal[3 * slot] = normal[3 * i]; A.normal[3 * slot + 1] = normal[3 * i + 1]; A.normal[3 * slot + 2] = normal[3 * i + 2];
  A.minDistance[slot] = minDistance[i]; A.maxDistance[slot] = maxDistance[i];
  A.flags[slot] = (uint8_t)(A.flags[slot] | kAttrGeometry);
}

// desc [n][2]: the winning rows of k_mapdb_distinctive
static __global__ __launch_bounds__(kAttrThreads) void k_attr_scatter_descriptor(int n, const int* __restrict__ slots, const uint4* __restrict__ desc,
                                                                                 const uint8_t* __restrict__ status, int want, AttrArrays A) {
  const int i = blockIdx.x * kAttrThreads + threadIdx.x;
  if (i >= n || status[i] != want) return;
  const int slot = slots[i];
  A.desc[2 * slot] = desc[2 * i]; A.desc[2 * slot + 1] = desc[2 * i + 1];
  A.flags[slot] = (uint8_t)(A.flags[slot] | kAttrDescriptor);
}

}  // namespace mapdb
}  // namespace ydorb
