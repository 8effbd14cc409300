// ah_arena.h — the growth policy of the context's grow-only device arenas (scratch, temp, pack: ah_ctx.hip), in ONE place: the
// reserve functions of libarrowhip.so and the sibling libraries on the same ah_ctx (libarrowhip_strings.so,
// libarrowhip_string_transform.so — they cannot call libarrowhip.so's internal functions) all grow an arena through this.
#pragma once
#include "ah_common.h"

// Make *block hold at least nbytes (its size in *bytes, rounded up to 1 MiB); contents are undefined after the call.  The old
// block may still be in use by enqueued kernels, so growing synchronises the stream first.  `what` names the arena in the
// out-of-memory error ("out of device memory (N bytes of <what>)"; nullptr: the plain hipMalloc error); *out_of_memory (nullable)
// tells a failed hipMalloc from a failed synchronisation or hipFree.
static inline int ah_arena_reserve(ah_ctx* c, void** block, size_t* bytes, size_t nbytes, const char* what, void** out, bool* out_of_memory = nullptr) {
  if (out_of_memory) *out_of_memory = false;
  if (nbytes > *bytes) {
    AH_HIP(c, hipStreamSynchronize(c->stream));
    if (*block) AH_HIP(c, hipFree(*block));
    *block = nullptr;
    *bytes = 0;
    const size_t want = (nbytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    if (what) {
      if (hipMalloc(block, want) != hipSuccess) {
        (void)hipGetLastError();
        if (out_of_memory) *out_of_memory = true;
        return ah_fail(c, AH_EHIP, "out of device memory (%zu bytes of %s)", want, what);
      }
    } else {
      AH_HIP(c, hipMalloc(block, want));
    }
    *bytes = want;
  }
  *out = *block;
  return AH_OK;
}
