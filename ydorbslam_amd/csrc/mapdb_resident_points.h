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

// What ydorb_mapdb_fuse_search reads besides: the observation pool (isInKeyFrame), and per keyframe slot the feature span (DESIGN.md
// section 6r; one span over two arrays) and the descriptor block (section 6p).
struct ResidentKeyframes {
  const int32_t* obsKf = nullptr;                                   // the observation pool: [obsStart[p], obsEnd[p]) of a point
  int32_t nFeatHdr = 0, nBlockHdr = 0;                              // the header capacities: a slot at or past one has no span
  const int32_t *featStart = nullptr, *featLen = nullptr;           // [nFeatHdr] in features
  const void* kps = nullptr;                                        // KeyPoint [pool]: 28 bytes each
  const float* rightX = nullptr;                                    // [pool]
  const int32_t *blockStart = nullptr, *blockLen = nullptr;         // [nBlockHdr] in descriptors
  const uint8_t* blockPool = nullptr;                               // [pool][32]
};

// lockResident for the fuse search: also checks that features are enabled and every kfSlots[i] lies in 0..n_keyframes-1, and hands out where the
// device holds the two spans of each named keyframe after the sync, from the host mirrors: featStart / featLen / blockStart / blockLen
// [nKf], so that the caller builds its FrameDev records without a read-back.
int lockResidentFuse(ydorb_mapdb_t* db, int32_t device, const int32_t* slots, int32_t n, const int32_t* kfSlots, int32_t nKf, ResidentPoints& out,
                     ResidentKeyframes& kf, int32_t* featStart, int32_t* featLen, int32_t* blockStart, int32_t* blockLen);

// What ydorb_mapdb_create_new_points reads: the pools of four keyframe relations (rows section 6o, blocks 6p, features 6r, BoW feature
// vectors 6t) and, per named keyframe, where the device holds its four spans after the sync, from the host mirrors.
struct ResidentTriPools {
  const int32_t* rowPool = nullptr;       // point slot per keypoint, -1 = none
  const int32_t* bowPool = nullptr;       // (node id, feature index) pairs
  const void* kps = nullptr;              // KeyPoint [pool]: 28 bytes each
  const float* rightX = nullptr;          // [pool]
  const uint8_t* blockPool = nullptr;     // [pool][32]
};
struct ResidentTriSpans { int32_t featStart, n, blockStart, rowStart, bowStart, bowLen; };   // n: the keyframe's feature count

// lockResident for createNewPoints: refuses features or BoW not enabled, another device, a keyframe slot outside 0..n_keyframes-1, a
// second keyframe equal to the first or named twice and nFirst != the first keyframe's resident feature count.  kfSlots [1 + nNb], the
// first keyframe at 0; nDepth [1 + nNb] = the caller's depth lengths; spans / status [1 + nNb] out.  status[i] is a
// YDORB_CREATE_NB_* of keyframe i on its own (0 = usable); with nNb == 0 nothing is synced and nothing is written.
int lockResidentTri(ydorb_mapdb_t* db, int32_t device, const int32_t* kfSlots, const int32_t* nDepth, int32_t nNb, ResidentTriPools& pools,
                    ResidentTriSpans* spans, uint8_t* status);

// What the batched BoW searches read: createNewPoints' pools and, for "has a good map point", the point table's bad flags
// [pointCap] (1 for a slot never set).
struct ResidentBowPools {
  ResidentTriPools tri;
  const uint8_t* bad = nullptr;
  int32_t pointCap = 0;
};

// lockResident for the BoW searches: refuses features or BoW not enabled, another device, a keyframe slot outside 0..n_keyframes-1 and,
// with nFirst >= 0, nFirst != the resident feature count of kfSlots[0].  kfSlots / spans / status [nKf]; status[i] is a
// YDORB_BOW_PAIR_* of keyframe i on its own, by the rule lockResidentTri applies (0 = usable).  A slot may repeat.  nSearched = the
// number of candidates: with 0 nothing is synced and nothing is written.
int lockResidentBow(ydorb_mapdb_t* db, int32_t device, const int32_t* kfSlots, int32_t nKf, int32_t nSearched, int32_t nFirst, ResidentBowPools& pools,
                    ResidentTriSpans* spans, uint8_t* status);

struct ResidentLock {   // unlocks on every way out of the reader
  ydorb_mapdb_t* db = nullptr;
  ~ResidentLock() { if (db) unlockResident(db); }
};

}  // namespace mapdb
}  // namespace ydorb
