// The 64x48 candidate grid of a frame (reference src/frame.cpp:249-264,327-336), shared by the matcher's k_grid_build and the frame tail's
// k_frame_grid: the records a grid is built from, the cell rule and the body of the one-workgroup CSR build.  Holds no kernel, so
// every translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace ydorb {

constexpr int kGridCols = 64, kGridRows = 48, kGridCells = kGridCols * kGridRows;  // frame.hpp:137-138

struct KeyPointDev { float x, y, size, angle, response; int octave, class_id; };
struct FrameDev {  // one target frame of a batched call
  const KeyPointDev* kps;
  const uint8_t* desc;
  const float* rightX;  // may be null (monocular: every entry <= 0)
  const int* nPtr;      // device count (batched pipeline) or null
  int n;                // used when nPtr is null
  float minX, minY, gridWInv, gridHInv;
  int* cellStart;       // [kGridCells + 1]
  int* cellIdx;         // [cap]
  float4* sortedKp;     // [cap] (x, y, octave bits, index bits) in grid (CSR) order: a window column is one contiguous run
  uint8_t* sortedDesc;  // [cap][32] descriptors in the same order
};
__device__ __forceinline__ int frame_n(const FrameDev& F) { return F.nPtr ? *F.nPtr : F.n; }

// The cell rule, in one place for every kernel that builds the grid: the cell ix * 48 + iy of a keypoint, or -1 when it lies outside.
__device__ __forceinline__ int grid_cell_of(float x, float y, float minX, float gridWInv, float gridHInv) {
  const int lx = (int)roundf(__fmul_rn(__fsub_rn(x, minX), gridWInv));
  const int ly = (int)roundf(__fmul_rn(__fsub_rn(y, minX), gridHInv));
  return (lx < 0 || lx >= kGridCols || ly < 0 || ly >= kGridRows) ? -1 : lx * kGridRows + ly;
}

// One workgroup of 256 lanes builds the CSR of frame F: cellStart [kGridCells + 1], cellIdx in push_back order; kSorted adds the
// matcher's keypoints and descriptors in CSR order.  hist [kGridCells], wsum [4] and cellOf [cap] are the caller's LDS.
template <bool kSorted>
__device__ __forceinline__ void grid_build(const FrameDev& F, int cap, int* hist, int* wsum, int16_t* cellOf) {
  const int n = min(frame_n(F), cap);
  for (int c = threadIdx.x; c < kGridCells; c += 256) hist[c] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) {
    const KeyPointDev kp = F.kps[i];
    const int cell = grid_cell_of(kp.x, kp.y, F.minX, F.gridWInv, F.gridHInv);
    if (cell >= 0) atomicAdd(&hist[cell], 1);
    cellOf[i] = (int16_t)cell;
  }
  __syncthreads();
  // exclusive scan of 3072 counts: 12 per thread
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int local[12], s = 0;
#pragma unroll
  for (int k = 0; k < 12; k++) { local[k] = s; s += hist[threadIdx.x * 12 + k]; }
  int x = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  int off = x - s;
  for (int j = 0; j < wv; j++) off += wsum[j];
#pragma unroll
  for (int k = 0; k < 12; k++) F.cellStart[threadIdx.x * 12 + k] = off + local[k];
  if (threadIdx.x == 255) F.cellStart[kGridCells] = off + s;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 12; k++) hist[threadIdx.x * 12 + k] = off + local[k];  // now: start offsets
  __syncthreads();
  // stable fill: rank inside the cell = number of earlier keypoints with the same cell
  for (int i = threadIdx.x; i < n; i += 256) {
    const int cell = cellOf[i];
    if (cell < 0) continue;
    int rank = 0;
    for (int j = 0; j < i; j++) rank += cellOf[j] == cell;
    const int pos = hist[cell] + rank;
    F.cellIdx[pos] = i;
    if constexpr (kSorted) {
      const KeyPointDev kp = F.kps[i];
      F.sortedKp[pos] = make_float4(kp.x, kp.y, __int_as_float(kp.octave), __int_as_float(i));
      const uint4* d = reinterpret_cast<const uint4*>(F.desc + (size_t)i * 32);
      uint4* o = reinterpret_cast<uint4*>(F.sortedDesc + (size_t)pos * 32);
      o[0] = d[0]; o[1] = d[1];
    }
  }
}

}  // namespace ydorb
