// The arrays of a sky::Plan (skyline_plan.h) as the skyline kernels read them: one view into a driver's upload arena, or into the
// staging area laid out like it.  Included by .hip files only.
#pragma once
#include "host_buffers.h"
#include "skyline_plan.h"

namespace ydorb {
namespace sky {

static_assert(sizeof(long long) == sizeof(int64_t), "the plan's offsets go to the device as they are");

struct PlanArrays {
  int *inv = nullptr, *perm = nullptr, *first = nullptr, *colRows = nullptr;
  long long *rowOff = nullptr, *colStart = nullptr, *colBlk = nullptr;
  // In the arena's order: inv (for the driver whose kernels look positions up), perm, first, rowOff, colStart, colRows, colBlk; the two
  // column arrays take room for at least minCols entries.
  void take(Carve& a, const Plan& P, bool withInv, size_t minCols = 0) {
    const size_t nF = P.nF, nCol = std::max(P.colRows.size(), minCols);
    if (withInv) a.take(inv, nF);
    a.take(perm, nF); a.take(first, nF); a.take(rowOff, nF + 1); a.take(colStart, nF + 1); a.take(colRows, nCol); a.take(colBlk, nCol);
  }
  // The plan into this view: put(dst, src, bytes) copies one array, or none of it when it is empty
  template <class Put> void fill(const Plan& P, Put put) const {
    auto one = [&](auto* dst, const auto& vec) { put(dst, vec.data(), sizeof(vec[0]) * vec.size()); };
    if (inv) one(inv, P.inv);
    one(perm, P.perm); one(first, P.first); one(rowOff, P.rowOff); one(colStart, P.colStart); one(colRows, P.colRows); one(colBlk, P.colBlk);
  }
};

}  // namespace sky
}  // namespace ydorb
