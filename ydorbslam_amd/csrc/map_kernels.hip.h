// gfx950 HIP kernels of map maintenance (include/ydorb/c_api.h, "Map maintenance"): the three passes over the
// flattened observation table (map point -> observing keyframes) that restate ORB-SLAM2's MapPoint::UpdateNormalAndDepth, the counting
// loop of KeyFrame::UpdateConnections and the counting of LocalMapping::KeyFrameCulling.
//   k_normal_depth  one lane per map point walks its span in order: the float sum over the observers is ordered, so the lane mapping
//                   cannot change a bit.  fp32 under the written-order contract of DESIGN.md section 2 ("Map maintenance"): + - * / sqrt
//                   only, every op a single IEEE operation (-ffp-contract=off), equal to tests/mapmaint_ref/mapmaint_ref.cpp bit for bit.
//   k_covisibility  one workgroup per query keyframe and a histogram of kWindow int32 counters in LDS (32 KB, static), updated with LDS
//                   integer atomics (integer adds commute: the counts are reproducible).  Lanes stride over the list entries and walk
//                   each point's observers.  The non-zero counters are compacted in ascending slot order by ballots and a prefix over
//                   the waves, never by an arrival-order cursor.  Past kWindow keyframes the slots are processed in windows; a first
//                   sweep over all windows sizes the result and decides the overflow status before a second one writes.
//   k_redundancy    one lane per list entry; a wave whose lanes all belong to one candidate adds its two sums with one integer atomic
//                   each, a wave that straddles candidates adds per lane.
// The passes serve the flat entries and the resident table (map_resident.hip) alike: a point's span is obsStart[p] .. obsEnd[p], and
// k_normal_depth takes an optional list of the points asked for.
// No float atomics, no inline assembly, no device-side assert / printf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_table.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace mapmaint {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWindow = maptable::kCovisWindow;
static_assert(kWindow % kThreads == 0, "every wave compacts a whole number of 64-slot rows");

struct Table {
  int nPoints, nKeyframes;
  const int* obsStart;        // [nPoints] where point p's span begins ...
  const int* obsEnd;          // [nPoints] ... and ends: obsStart + 1 for a flat table, an array of its own for the resident one
  const int* obsKf;           // [N]
  const uint8_t* obsLevel;    // [N]
  const uint8_t* bad;         // [nPoints]
};

struct NormalArgs {
  Table t;
  const float* pos;           // [nPoints][3]
  const float* centre;        // [nKeyframes][3]
  const int* refKf;           // [nPoints]
  const uint8_t* refLevel;    // [nPoints]
  float scaleFactors[8];
  int nLevels;
  const int* slots;           // [n] the points asked for (a slot may repeat), or null: all nPoints in order
  int n;                      // lanes: results i = 0 .. n-1
  float* normal;              // [n][3]
  float* minDistance;         // [n]
  float* maxDistance;         // [n]
  uint8_t* status;            // [n]
};

// sqrt of the squared length: the squares exact in double, summed in ascending index (cv::norm returns a double)
__device__ __forceinline__ double norm3(float x, float y, float z) {
  return sqrt(((double)x * (double)x + (double)y * (double)y) + (double)z * (double)z);
}

struct NormalDepth { float nx, ny, nz, mn, mx; };

// MapPoint::updateNormalAndDepth of one point with a non-empty span [b, e): position P, reference keyframe slot r at level lr.
// centreOf(k) returns a pointer to the three floats of keyframe slot k's camera centre: the table's for k_normal_depth, the rule of
// the map correction for k_mapdb_correct (mapcorrect_kernels.hip.h).  The one copy of the ordered sum.
template <class CentreOf>
__device__ __forceinline__ NormalDepth normalDepthOf(const int* obsKf, int b, int e, float Px, float Py, float Pz, int r, int lr,
                                                     const float (&scaleFactors)[8], int nLevels, CentreOf centreOf) {
  float nx = 0.f, ny = 0.f, nz = 0.f;
  for (int q = b; q < e; q++) {
    const float* c = centreOf(obsKf[q]);
    const float dx = Px - c[0], dy = Py - c[1], dz = Pz - c[2];
    const float inv = (float)(1.0 / norm3(dx, dy, dz));
    nx = nx + dx * inv; ny = ny + dy * inv; nz = nz + dz * inv;
  }
  const float f = (float)(1.0 / (double)(e - b));
  nx = nx * f; ny = ny * f; nz = nz * f;
  const float* cr = centreOf(r);
  const float dist = (float)norm3(Px - cr[0], Py - cr[1], Pz - cr[2]);
  float sfRef = scaleFactors[0], sfTop = scaleFactors[0];
#pragma unroll
  for (int i = 1; i < 8; i++) { sfRef = lr == i ? scaleFactors[i] : sfRef; sfTop = nLevels - 1 == i ? scaleFactors[i] : sfTop; }
  const float mx = dist * sfRef;
  return {nx, ny, nz, mx / sfTop, mx};
}

static __global__ __launch_bounds__(kThreads) void k_normal_depth(NormalArgs g) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= g.n) return;
  const int p = g.slots ? g.slots[i] : i;
  const int b = g.t.obsStart[p], e = g.t.obsEnd[p];
  float nx = 0.f, ny = 0.f, nz = 0.f, mn = 0.f, mx = 0.f;
  int code = YDORB_MAP_UPDATED;
  if (g.t.bad[p]) code = YDORB_MAP_BAD;
  else if (b == e) code = YDORB_MAP_NO_OBSERVATIONS;
  else {
    const float* centre = g.centre;
    const NormalDepth nd = normalDepthOf(g.t.obsKf, b, e, g.pos[3 * p], g.pos[3 * p + 1], g.pos[3 * p + 2], g.refKf[p], g.refLevel[p], g.scaleFactors,
                                         g.nLevels, [centre](int k) { return centre + 3 * k; });
    nx = nd.nx; ny = nd.ny; nz = nd.nz; mn = nd.mn; mx = nd.mx;
  }
  g.normal[3 * i] = nx; g.normal[3 * i + 1] = ny; g.normal[3 * i + 2] = nz;
  g.minDistance[i] = mn; g.maxDistance[i] = mx;
  g.status[i] = (uint8_t)code;
}

struct CovisArgs {
  Table t;
  int nQueries;
  const int* queryKf;         // [nQueries]
  const int* listStart;       // [nQueries + 1]
  const int* pointIdx;        // [L]
  const int* outStart;        // [nQueries + 1]
  int* connKf;                // [outStart[nQueries]]
  int* connWeight;            // [outStart[nQueries]]
  int* counts;                // [nQueries]
  uint8_t* status;            // [nQueries]
};

static __global__ __launch_bounds__(kThreads) void k_covisibility(CovisArgs g) {
  __shared__ int hist[kWindow];
  __shared__ int waveTotal[kWaves];
  const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int self = g.queryKf[qi];
  const int lb = g.listStart[qi], le = g.listStart[qi + 1];
  const int outBase = g.outStart[qi], cap = g.outStart[qi + 1] - outBase;
  const int nWin = (g.t.nKeyframes + kWindow - 1) / kWindow;
  constexpr int kRows = kWindow / kThreads;   // 64-slot rows per wave: wave w owns the slots w * kRows * 64 .. of a window
  for (int pass = 0; pass < 2; pass++) {      // 0 sizes the result over all windows, 1 writes it
    int written = 0;
    for (int w = 0; w < nWin; w++) {
      const int w0 = w * kWindow;
      if (pass == 0 || nWin > 1) {            // one window: the histogram of the sizing sweep is still there
        __syncthreads();                      // the previous window's readers are done
        for (int i = tid; i < kWindow; i += kThreads) hist[i] = 0;
        __syncthreads();
        for (int e = lb + tid; e < le; e += kThreads) {
          const int p = g.pointIdx[e];
          if (g.t.bad[p]) continue;
          const int ob = g.t.obsStart[p], oe = g.t.obsEnd[p];
          for (int q = ob; q < oe; q++) {
            const int k = g.t.obsKf[q];
            if (k != self && k >= w0 && k - w0 < kWindow) atomicAdd(&hist[k - w0], 1);
          }
        }
        __syncthreads();
      }
      const int rowBase = wave * kRows * 64;
      int mine = 0;
      for (int r = 0; r < kRows; r++) mine += __popcll(__ballot(hist[rowBase + r * 64 + lane] != 0));
      if (lane == 0) waveTotal[wave] = mine;
      __syncthreads();
      int before = 0, all = 0;
      for (int v = 0; v < kWaves; v++) { before += v < wave ? waveTotal[v] : 0; all += waveTotal[v]; }
      if (pass == 1) {
        int at = outBase + written + before;
        for (int r = 0; r < kRows; r++) {
          const int slot = rowBase + r * 64 + lane;
          const int c = hist[slot];
          const unsigned long long m = __ballot(c != 0);
          if (c != 0) {
            const int o = at + __popcll(m & ((1ull << lane) - 1ull));
            g.connKf[o] = w0 + slot;
            g.connWeight[o] = c;
          }
          at += __popcll(m);
        }
      }
      written += all;
      __syncthreads();                        // waveTotal is read before the next window rewrites it
    }
    if (pass == 0) {
      if (tid == 0) { g.counts[qi] = written; g.status[qi] = written > cap ? 1 : 0; }
      if (written > cap) return;              // uniform over the workgroup: nothing of an overflowing query is written
    }
  }
}

struct RedundancyArgs {
  Table t;
  int nCand, nEntries, thObs;
  const int* candKf;          // [nCand]
  const int* listStart;       // [nCand + 1]
  const int* pointIdx;        // [nEntries]
  const uint8_t* ownLevel;    // [nEntries]
  const uint8_t* removed;     // [nKeyframes] (all zero when the caller passed NULL)
  int* nCounted;              // [nCand], zeroed before the launch
  int* nRedundant;            // [nCand], zeroed before the launch
};

static __global__ __launch_bounds__(kThreads) void k_redundancy(RedundancyArgs g) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  const bool live = e < g.nEntries;
  int c = 0, counted = 0, redundant = 0;
  if (live) {
    // the candidate whose range holds e: the last c with listStart[c] <= e (empty candidates share a start and are skipped by "last")
    int lo = 0, hi = g.nCand - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (g.listStart[mid] <= e) lo = mid; else hi = mid - 1;
    }
    c = lo;
    const int p = g.pointIdx[e];
    if (!g.t.bad[p]) {
      const int self = g.candKf[c], limit = (int)g.ownLevel[e] + 1;
      const int ob = g.t.obsStart[p], oe = g.t.obsEnd[p];
      int weight = 0, near = 0;
      bool lost = false;
      for (int q = ob; q < oe; q++) {
        const int k = g.t.obsKf[q];
        const int lv = g.t.obsLevel[q];
        if (g.removed[k]) { lost = true; continue; }
        weight += (lv & 0x80) ? 2 : 1;
        near += (k != self && (lv & 0x7f) <= limit) ? 1 : 0;
      }
      if (!(lost && weight <= 2)) {
        counted = 1;
        redundant = (weight > g.thObs && near >= g.thObs) ? 1 : 0;
      }
    }
  }
  // one candidate in the whole wave (the usual case: lists are far longer than 64): one atomic per sum and wave
  // (entries ascend with the lane, so a wave with a live lane has lane 0 live; a wave without one has nothing to add)
  if (__ballot(live) == 0) return;
  const int first = __shfl(c, 0);
  const bool uniform = __ballot(live && c != first) == 0;
  if (uniform) {
    const int nc = __popcll(__ballot(counted != 0)), nr = __popcll(__ballot(redundant != 0));
    if ((threadIdx.x & 63) == 0) {
      if (nc) atomicAdd(&g.nCounted[c], nc);
      if (nr) atomicAdd(&g.nRedundant[c], nr);
    }
  } else if (live) {
    if (counted) atomicAdd(&g.nCounted[c], 1);
    if (redundant) atomicAdd(&g.nRedundant[c], 1);
  }
}

}  // namespace mapmaint
}  // namespace ydorb
