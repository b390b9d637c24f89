// gfx950 HIP kernels of the points-of-keyframes query on the resident table's keyframe rows (include/ydorb/c_api.h, "Keyframe rows";
// DESIGN.md section 6o).  The rows themselves are kept by the span kernels of mapdb_span_kernels.hip.h.
//   k_rowset_mark        the points of a keyframe set, pass 1: one lane per position e of E (the rows of the call's keyframes
//                        concatenated).  The keyframe's rank comes from a search in the start table, as in k_redundancy.  The lane
//                        stores its entry to ent[e] (-1 for a null or bad one) and does an integer atomicMin(&first[slot], e) for the
//                        others: an integer min does not depend on the order the atomics land in.  Lanes below nSeen stamp
//                        seenStamp[slot] with the call's stamp (equal values to one address: the order is immaterial).
//   k_rowset_count       per workgroup the number of positions with first[slot] == e: ballot and popcount per wave.
//   k_rowset_emit        each workgroup takes its base from the totals before it and writes its kept entries in position order,
//                        at base + the waves before + popcount(ballot below the lane), never by an arrival-order cursor.  The
//                        winning lane puts first[slot] back to INT32_MAX, also when the result overflows `capacity` and nothing is
//                        written.  first is INT32_MAX everywhere between calls; seenStamp needs no clearing, a later call has a
//                        later stamp.  A lane that reads first[slot] while another workgroup's winner resets it sees that winner's
//                        position or INT32_MAX, neither its own.
// Every index is bounded by the host before the launch or checked here: a row entry is below n_points (validated when staged), a
// position inside a row is checked against the device's rowLen.  No float anywhere.  No inline assembly, no device-side assert / printf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapdb_rows_host.h"

namespace ydorb {
namespace mapdb {

constexpr int kRowThreads = 256;
constexpr int kRowWaves = kRowThreads / 64;

struct RowsetArgs {
  int nKf, nE, nSeen, stamp, capacity, nBlocks;
  const int* kfSlots;      // [nKf]
  const int* eStart;       // [nKf + 1] where each keyframe's row begins in E
  const int* seen;         // [nSeen]
  const int* rowStart;     // the handle's tables
  const int* rowLen;
  const int* pool;
  const uint8_t* bad;      // [pointCap]
  int* first;              // [pointCap] INT32_MAX between calls
  int* seenStamp;          // [pointCap]
  int* ent;                // [nE] scratch: the entry of each position, -1 when it cannot be kept
  int* blockTotal;         // [nBlocks] scratch
  int* outSlots;           // [min(capacity, nE)]
  uint8_t* outSeen;        // [min(capacity, nE)]
  int* total;              // [1]
};

static __global__ __launch_bounds__(kRowThreads) void k_rowset_mark(RowsetArgs g) {
  const int e = blockIdx.x * kRowThreads + threadIdx.x;
  if (e < g.nSeen) {
    const int s = g.seen[e];
    if (s >= 0) g.seenStamp[s] = g.stamp;
  }
  if (e >= g.nE) return;
  // the keyframe whose row holds e: the last r with eStart[r] <= e (empty rows share a start and are skipped by "last")
  int lo = 0, hi = g.nKf - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (g.eStart[mid] <= e) lo = mid; else hi = mid - 1;
  }
  const int k = g.kfSlots[lo], i = e - g.eStart[lo];
  int slot = i < g.rowLen[k] ? g.pool[g.rowStart[k] + i] : -1;
  if (slot >= 0 && g.bad[slot]) slot = -1;
  g.ent[e] = slot;
  if (slot >= 0) atomicMin(&g.first[slot], e);
}

static __global__ __launch_bounds__(kRowThreads) void k_rowset_count(RowsetArgs g) {
  __shared__ int waveTotal[kRowWaves];
  const int e = blockIdx.x * kRowThreads + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool kept = false;
  if (e < g.nE) {
    const int slot = g.ent[e];
    kept = slot >= 0 && g.first[slot] == e;
  }
  const int n = __popcll(__ballot(kept));
  if (lane == 0) waveTotal[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int v = 0; v < kRowWaves; v++) sum += waveTotal[v];
    g.blockTotal[blockIdx.x] = sum;
  }
}

static __global__ __launch_bounds__(kRowThreads) void k_rowset_emit(RowsetArgs g) {
  __shared__ int partBefore[kRowWaves], partAll[kRowWaves], waveTotal[kRowWaves];
  const int tid = threadIdx.x, e = blockIdx.x * kRowThreads + tid, lane = tid & 63, wave = tid >> 6;
  int before = 0, all = 0;
  for (int b = tid; b < g.nBlocks; b += kRowThreads) {
    const int t = g.blockTotal[b];
    all += t;
    before += b < (int)blockIdx.x ? t : 0;
  }
  for (int d = 32; d > 0; d >>= 1) { before += __shfl_xor(before, d); all += __shfl_xor(all, d); }
  int slot = -1;
  bool kept = false;
  if (e < g.nE) {
    slot = g.ent[e];
    kept = slot >= 0 && g.first[slot] == e;
  }
  const unsigned long long m = __ballot(kept);
  if (lane == 0) { partBefore[wave] = before; partAll[wave] = all; waveTotal[wave] = __popcll(m); }
  __syncthreads();
  int base = 0, total = 0;
  for (int v = 0; v < kRowWaves; v++) { base += partBefore[v]; total += partAll[v]; base += v < wave ? waveTotal[v] : 0; }
  if (blockIdx.x == 0 && tid == 0) *g.total = total;
  if (!kept) return;
  if (total <= g.capacity) {
    const int o = base + __popcll(m & ((1ull << lane) - 1ull));
    g.outSlots[o] = slot;
    g.outSeen[o] = g.seenStamp[slot] == g.stamp ? 1 : 0;
  }
  g.first[slot] = INT32_MAX;
}

}  // namespace mapdb
}  // namespace ydorb
