// What ydorb_mapdb_search_local_points (orb_matcher.hip) reads of a resident map table (map_resident.hip): the device pointers of the
// per-slot arrays the frustum test and the fused search load, and the one function that hands them out.  Each handle struct stays
// private to its translation unit.  No HIP types here beyond plain pointers.
#pragma once
#include <stdint.h>

#include "../../include/ydorb/c_api.h"

namespace ydorb {
namespace mapdb {

struct alignas(16) Desc16 { uint32_t w[4]; };   // half a descriptor: the kernels move it as one 16-byte load and store

struct ResidentPoints {
  // the point table, [point capacity] each
  const float* pos = nullptr;           // [3] per slot
  const uint8_t* bad = nullptr;
  const int32_t *obsStart = nullptr, *obsEnd = nullptr;
  // the attributes (section 6q)
  const float *normal = nullptr, *minDistance = nullptr, *maxDistance = nullptr;
  const Desc16* desc = nullptr;         // [2] per slot
  const uint8_t* flags = nullptr;
};

// Takes the handle's mutex, checks that attributes are enabled, that `device` is the handle's and that every slot lies in
// 0..n_points-1, applies what is staged and synchronises the handle's stream, so that work queued on another stream afterwards sees
// the table as of this call.  On YDORB_OK the mutex stays held until unlockResident: no stager can repack or grow an arena under the
// reader.  On any other return it has been released.
int lockResident(ydorb_mapdb_t* db, int32_t device, const int32_t* slots, int32_t n, ResidentPoints& out);
void unlockResident(ydorb_mapdb_t* db);

struct ResidentLock {   // unlocks on every way out of the reader
  ydorb_mapdb_t* db = nullptr;
  ~ResidentLock() { if (db) unlockResident(db); }
};

}  // namespace mapdb
}  // namespace ydorb
