// gfx950 HIP kernels of the map correction on the resident table (include/ydorb/c_api.h, "Map correction"; DESIGN.md section 2 "Map
// correction" and section 6n): the point loops of LoopClosing::correctLoop, of optimizeEssentialGraph's tail and of the map update after
// a global BA, in place on the table's positions.
//   k_mapdb_correct          one lane per claimed entry (mapdb_host.h's claim pass: no two share a slot).  It reads pos[slot], applies the
//                            pair of its correcting keyframe, stores the float result to pos[slot] and to its output row and, when
//                            normals are asked for, walks the point's span with the new position through map_kernels.hip.h's
//                            normalDepthOf.  An observer (and the reference keyframe in `dist`) whose rank in the call is below
//                            `limit` shows its centre_after, every other the resident centre: limit = the lane's own rank
//                            (interleaved: the keyframes before it have had their setPose), n_kf (poses first) or 0 (resident).
//                              Sim3  sim3Map(inverse(after), sim3Map(before, X)) of sim3_math.hip.h: float in, the chain in double,
//                                    rounded once.
//                              SE3   two row products of frustum_kernels.hip.h's kind: each product exact in double, the three products
//                                    and the float addend summed in double in ascending index, rounded once to float - twice.
//                            Bound by the gathers over the spans, like k_normal_depth; the per-keyframe tables (128 B a keyframe for
//                            Sim3) sit in cache.  No LDS.
//   k_mapdb_correct_centres  one lane per keyframe of the call writes its centre_after into the table.  A launch of its own after the
//                            pass, on the same stream: lanes of the pass still read the old centres.
// The pass reads the centres and every lane only its own position, so the in-place store races with nothing.  Every index is bounded
// by the host before the launch (slots below n_points, ranks below n_kf, observer and reference slots below n_keyframes).  Plain
// vector stores, no atomics, no inline assembly, no device-side assert / printf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ydorb/c_api.h"
#include "map_kernels.hip.h"
#include "sim3_math.hip.h"

#pragma clang fp contract(off)

namespace ydorb {
namespace mapcorrect {

constexpr int kThreads = 256;

struct CorrectArgs {
  int nClaimed, nKf, arithmetic, centres, normals;
  const int* slot;            // [nClaimed] point slot of the claimed entry
  const int* rank;            // [nClaimed] rank in the call of the keyframe that corrects it
  const int* rankOf;          // [nKeyframes] keyframe slot -> rank in the call, -1: not in it
  const void* before;         // [nKf][8] double or [nKf][12] float
  const void* after;
  const float* centreAfter;   // [nKf][3], read only where limit > 0
  // the table
  float* pos;                 // [nPoints][3] corrected in place
  const float* centre;        // [nKeyframes][3]
  const int* obsStart;
  const int* obsEnd;
  const int* obsKf;
  const int* refKf;
  const uint8_t* refLevel;
  float scaleFactors[8];
  int nLevels;
  // results, compact: row j of claimed entry j
  float* posOut;              // [nClaimed][3]
  float* normal;              // [nClaimed][3]
  float* minDistance;         // [nClaimed]
  float* maxDistance;         // [nClaimed]
  uint8_t* status;            // [nClaimed]
};

// row r of a row-major 3x3 times (x, y, z) plus the addend: products exact in double, summed in ascending index, rounded once
__device__ __forceinline__ float rowMap(const float* M, const float* t, int r, float x, float y, float z) {
  return (float)((((double)M[3 * r] * (double)x + (double)M[3 * r + 1] * (double)y) + (double)M[3 * r + 2] * (double)z) + (double)t[r]);
}

__device__ __forceinline__ sim3::S3 loadSim3(const double* s) { return {{s[0], s[1], s[2], s[3]}, {s[4], s[5], s[6]}, s[7]}; }

static __global__ __launch_bounds__(kThreads) void k_mapdb_correct(CorrectArgs g) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= g.nClaimed) return;
  const int p = g.slot[j], r = g.rank[j];
  const float X = g.pos[3 * p], Y = g.pos[3 * p + 1], Z = g.pos[3 * p + 2];
  float Px, Py, Pz;
  if (g.arithmetic == YDORB_MAPCORR_SIM3) {
    const sim3::S3 Siw = loadSim3(static_cast<const double*>(g.before) + 8 * r);
    const sim3::S3 correctedSwi = sim3::inverse(loadSim3(static_cast<const double*>(g.after) + 8 * r));
    const sim3::V3 P = sim3::sim3Map(correctedSwi, sim3::sim3Map(Siw, {(double)X, (double)Y, (double)Z}));
    Px = (float)P.x; Py = (float)P.y; Pz = (float)P.z;
  } else {
    const float* B = static_cast<const float*>(g.before) + 12 * r;
    const float* A = static_cast<const float*>(g.after) + 12 * r;
    const float cx = rowMap(B, B + 9, 0, X, Y, Z), cy = rowMap(B, B + 9, 1, X, Y, Z), cz = rowMap(B, B + 9, 2, X, Y, Z);
    Px = rowMap(A, A + 9, 0, cx, cy, cz); Py = rowMap(A, A + 9, 1, cx, cy, cz); Pz = rowMap(A, A + 9, 2, cx, cy, cz);
  }
  g.pos[3 * p] = Px; g.pos[3 * p + 1] = Py; g.pos[3 * p + 2] = Pz;
  g.posOut[3 * j] = Px; g.posOut[3 * j + 1] = Py; g.posOut[3 * j + 2] = Pz;
  const int b = g.obsStart[p], e = g.obsEnd[p];
  g.status[j] = (uint8_t)(b == e ? YDORB_MAPCORR_DONE_NO_OBSERVATIONS : YDORB_MAPCORR_DONE);
  if (!g.normals) return;
  mapmaint::NormalDepth nd{0.f, 0.f, 0.f, 0.f, 0.f};
  if (b != e) {
    const int limit = g.centres == YDORB_MAPCORR_INTERLEAVED ? r : g.centres == YDORB_MAPCORR_POSES_FIRST ? g.nKf : 0;
    const int* rankOf = g.rankOf;
    const float* centre = g.centre;
    const float* centreAfter = g.centreAfter;
    nd = mapmaint::normalDepthOf(g.obsKf, b, e, Px, Py, Pz, g.refKf[p], g.refLevel[p], g.scaleFactors, g.nLevels,
                                 [rankOf, centre, centreAfter, limit](int k) {
                                   const int rk = rankOf[k];   // -1 < 0 <= limit: a keyframe outside the call never passes
                                   return rk >= 0 && rk < limit ? centreAfter + 3 * rk : centre + 3 * k;
                                 });
  }
  g.normal[3 * j] = nd.nx; g.normal[3 * j + 1] = nd.ny; g.normal[3 * j + 2] = nd.nz;
  g.minDistance[j] = nd.mn; g.maxDistance[j] = nd.mx;
}

struct CentreArgs {
  int nKf;
  const int* kfSlots;         // [nKf] distinct
  const float* centreAfter;   // [nKf][3]
  float* centre;              // [nKeyframes][3]
};

static __global__ __launch_bounds__(kThreads) void k_mapdb_correct_centres(CentreArgs g) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= g.nKf) return;
  const int s = g.kfSlots[k];
  g.centre[3 * s] = g.centreAfter[3 * k]; g.centre[3 * s + 1] = g.centreAfter[3 * k + 1]; g.centre[3 * s + 2] = g.centreAfter[3 * k + 2];
}

}  // namespace mapcorrect
}  // namespace ydorb
