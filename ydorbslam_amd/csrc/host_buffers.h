// Host-side scaffolding the HIP drivers share: the error-check macro, grow-only device / pinned buffers, the aligned layout of a
// staging area and the per-device context of the staged solvers.  Included by .hip files only (ydorb_host.h stays free of HIP types).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <mutex>

#include "../../include/ydorb/c_api.h"
#include "layout.h"
#include "ydorb_host.h"

// A macro, so that __FILE__ / __LINE__ name the call site.
#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      ydorb::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return YDORB_ERR_HIP;                                                                   \
    }                                                                                         \
  } while (0)

namespace ydorb {

// Grow-only device buffer, or pinned host buffer when `host` is set; growing does not keep the contents.
// A Mem always owns the allocation `p` points at.  A slice of a buffer is a typed pointer computed from a Layout offset, never a
// second Mem: release / alloc / take on a Mem that pointed into another one would free an interior pointer.
// No destructor, on purpose: the solvers keep their contexts in static arrays, and freeing during static destruction would call
// into a HIP runtime that may already be gone.  Owners release() explicitly in their destroy / release entry points; a buffer
// that lives in one function is a ScopedMem.
struct Mem {
  void* p = nullptr;
  size_t cap = 0;
  bool host = false;
  size_t slackDiv = 4, floor = 4096;   // growth policy, set once by the owner: request bytes + bytes / slackDiv, at least floor
  size_t want(size_t bytes) const { return std::max(bytes + bytes / slackDiv, floor); }
  int ensure(size_t bytes) { return bytes <= cap ? YDORB_OK : alloc(want(bytes)); }
  int alloc(size_t bytes) {   // drops what it holds and requests exactly `bytes`
    release();
    if ((host ? hipHostMalloc(&p, bytes) : hipMalloc(&p, bytes)) != hipSuccess) {
      p = nullptr;
      set_error("%s(%zu) failed", host ? "hipHostMalloc" : "hipMalloc", bytes);
      return YDORB_ERR_HIP;
    }
    cap = bytes;
    return YDORB_OK;
  }
  void release() {
    if (p) (void)(host ? hipHostFree(p) : hipFree(p));
    p = nullptr; cap = 0;
  }
  void take(Mem& o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }   // o's allocation becomes this buffer's
  template <class T> T* as() { return reinterpret_cast<T*>(p); }
  template <class T> T* at(size_t off) { return reinterpret_cast<T*>(static_cast<uint8_t*>(p) + off); }
};

struct PinnedMem : Mem {   // pinned host memory: staging and read-back areas
  PinnedMem() { host = true; }
};

struct ScopedMem : Mem {   // for function-local buffers only (see Mem)
  ScopedMem() = default;
  ScopedMem(const ScopedMem&) = delete;
  ScopedMem& operator=(const ScopedMem&) = delete;
  ~ScopedMem() { release(); }
};

template <class T> T* at(Mem& m, size_t off) { return m.at<T>(off); }

// Hands out the arrays of an arena in order, every one 256-byte aligned.  A driver's lay*() functions run twice per (re)layout: over a
// null base for the size the arena needs, then over the arena for the pointers.
struct Carve {
  uintptr_t base;
  Layout L{0, 256};
  explicit Carve(void* p) : base(reinterpret_cast<uintptr_t>(p)) {}
  template <class T> void take(T*& ptr, size_t count) { ptr = reinterpret_cast<T*>(base + L.add(sizeof(T) * count)); }
};

// Per-device scratch of a solver that stages a batch up and its results down, reused between calls.  Every solver keeps its own
// array of these: solvers run concurrently from different host threads and share neither stream, mutex nor buffers.
struct StagedCtx {
  std::mutex mu;
  hipStream_t stream = nullptr;
  Mem up, down, scratch;
  PinnedMem hUp, hDown;
  int init(int device) {
    HIPCHK(hipSetDevice(device));
    if (!stream) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return YDORB_OK;
  }
  // Grows the upload area and its staging to upBytes, the read-back area and its staging to downBytes, scratch when asked for.  A
  // buffer that grows moves: take device pointers only afterwards.
  int ensure(size_t upBytes, size_t downBytes, size_t scratchBytes = 0) {
    int rc;
    if ((rc = up.ensure(upBytes)) || (rc = hUp.ensure(upBytes)) || (rc = down.ensure(downBytes)) || (rc = hDown.ensure(downBytes))) return rc;
    return scratchBytes ? scratch.ensure(scratchBytes) : YDORB_OK;
  }
  void releaseBuffers() { up.release(); down.release(); scratch.release(); hUp.release(); hDown.release(); }
};

// Body of a solver's ydorb_*_release(device) over its array of contexts (StagedCtx or a context derived from it): checks the
// ordinal, waits for the context's stream and gives its buffers back (the stream stays).
template <class Ctx> int release_staged(Ctx (&ctx)[16], int device) {
  if (device < 0 || device >= 16) { set_error("invalid device"); return YDORB_ERR_INVALID_ARG; }
  int rc = require_device(device);
  if (rc) return rc;
  StagedCtx& c = ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  HIPCHK(hipSetDevice(device));
  if (c.stream) (void)hipStreamSynchronize(c.stream);
  c.releaseBuffers();
  return YDORB_OK;
}

}  // namespace ydorb
