// Host-only: the layout of one allocation carved into 256-byte-aligned
// segments (the planning and greedy arenas of ops/hip/wva_ctx.inc). Checked by
// the stand-alone driver ops/native/stage_driver.cpp.
#ifndef WVA_ARENA_H
#define WVA_ARENA_H

#include <stddef.h>

static inline size_t wva_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Segment i holds sizes[i] bytes (0 is fine: it then shares its offset with
// the next one) and starts at offsets[i], a multiple of 256; segments follow
// each other in table order. Returns the bytes to allocate: the sum of the
// sizes, each padded to 256.
static inline size_t wva_arena_layout(const size_t *sizes, int n, size_t *offsets) {
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    offsets[i] = total;
    total += wva_align256(sizes[i]);
  }
  return total;
}

#endif  // WVA_ARENA_H
