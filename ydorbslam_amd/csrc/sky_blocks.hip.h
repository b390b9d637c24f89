// Device primitives that the two block-skyline solvers (essential_skyline.hip.h, 7x7 blocks; ba_skyline.hip.h, 6x6 blocks) and the
// dense BA kernels share: the packed lower triangle, the Cholesky of one diagonal block held in registers and the substitutions against
// it, all in fp64 with every sum in a fixed order.  Plain HIP, no driver types.  The walks over the block columns are not here: each
// solve kernel keeps its own schedule (DESIGN.md sections 6j and 6k).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace ydorb {
namespace sky {

__device__ __forceinline__ constexpr int tri(int r, int c) { return r * (r + 1) / 2 + c; }   // entry (r, c), c <= r, of packed rows

// Row of entry t of a packed lower triangle (its column is t - tri(row, 0)), in the width of T.  The two loops make the rounded root exact.
template <class T> __device__ __forceinline__ int triRow(T t) {
  int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((T)r * (r + 1) / 2 > t) r--;
  while ((T)(r + 1) * (r + 2) / 2 <= t) r++;
  return r;
}

// L L^T of the lower triangle of D ([B][B]) into l (packed rows) and the reciprocals of its diagonal into inv; false when a pivot was
// not positive (it is then taken as 1).  Every division by a pivot in the column, here, in the panel and in the back substitution, is
// a product with inv: one division per pivot instead of B and more on the column's chain of dependent fp64 operations.
template <int B> __device__ __forceinline__ bool factorBlock(const double* D, double* l, double* inv) {
  bool ok = true;
#pragma unroll
  for (int r = 0; r < B; r++)
#pragma unroll
    for (int c = 0; c <= r; c++) {
      double s = D[B * r + c];
#pragma unroll
      for (int q = 0; q < c; q++) s -= l[tri(r, q)] * l[tri(c, q)];
      if (c == r) {
        if (!(s > 0)) { ok = false; s = 1.0; }
        l[tri(r, r)] = sqrt(s);
        inv[r] = 1.0 / l[tri(r, r)];
      } else {
        l[tri(r, c)] = s * inv[c];
      }
    }
  return ok;
}

// One row of a panel (or b_j) against the factor of the diagonal block: v L^T = row, in place
template <int B> __device__ __forceinline__ void solveRow(double* v, const double* l, const double* inv) {
#pragma unroll
  for (int c = 0; c < B; c++) {
    double s = v[c];
#pragma unroll
    for (int q = 0; q < c; q++) s -= v[q] * l[tri(c, q)];
    v[c] = s * inv[c];
  }
}

// The factor over the lower triangle of its block and the reciprocal pivots into row j of dinv: one thread, after every thread read D
template <int B> __device__ __forceinline__ void storeFactor(double* D, double* dinv, size_t j, const double* l, const double* inv) {
#pragma unroll
  for (int r = 0; r < B; r++)
#pragma unroll
    for (int c = 0; c <= r; c++) D[B * r + c] = l[tri(r, c)];
#pragma unroll
  for (int c = 0; c < B; c++) dinv[B * j + c] = inv[c];
}

// L^T x_i = y_i against the stored factor of diagonal block i (rows i of y and of dinv), the entries downwards
template <int B> __device__ __forceinline__ void solveDiagBack(const double* D, const double* dinv, const double* y, size_t i, double* xv) {
#pragma unroll
  for (int c = B - 1; c >= 0; c--) {
    double s = y[B * i + c];
#pragma unroll
    for (int q = c + 1; q < B; q++) s -= D[B * q + c] * xv[q];
    xv[c] = s * dinv[B * i + c];
  }
}

}  // namespace sky
}  // namespace ydorb
