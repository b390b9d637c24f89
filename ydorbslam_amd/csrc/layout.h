// Lays arrays out at aligned offsets of one area: the same offsets address the pinned staging and the device copy.  `align` is a
// power of two, set before the first add(): 16 bytes serve any element type; the arenas (host_buffers.h's Carve) ask for 256 so that
// every array of one starts on the boundary a buffer of its own had (hipMalloc returns at least that).  No HIP here: host_buffers.h
// and the host-only headers share it.
#pragma once
#include <stddef.h>

namespace ydorb {
struct Layout {
  size_t bytes = 0, align = 16;
  size_t add(size_t n) { const size_t at = bytes; bytes += (n + align - 1) & ~(align - 1); return at; }
};
}  // namespace ydorb
