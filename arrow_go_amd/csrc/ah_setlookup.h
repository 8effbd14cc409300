// ah_setlookup.h — pieces shared by ah_setlookup.hip (is_in of 1/2/4/8-byte keys) and ah_setlookup_binary.hip (is_in of
// byte-string and wider fixed-width keys): the null-behaviour truth table, the bit-range writer of the result, and the
// internal entry of the fixed-width kernels over a value set in pieces.
#pragma once
#include "ah_common.h"

namespace {

enum { kFlagSetHasNull = 1u, kFlagAllOnesKey = 2u };

// isInKernelExec (kernels/scalar_set_lookup.go:374-413), per row:
//   valid: found → (true, valid) · else Inconclusive ∧ set-has-null → (false, NULL) · else (false, valid)
//   null:  Match ∧ set-has-null → (true, valid) · Skip ∨ (Match ∧ ¬set-has-null) → (false, valid) · else (false, NULL)
//   set-has-null is forced false under Skip (NullIndex stays −1, :239-242).
// Folded into three wave-uniform flags: valid row → (found, found ∨ vmiss) · null row → (dnull, vnull).
struct NullRule { bool vmiss, dnull, vnull; };
__device__ __forceinline__ NullRule null_rule(unsigned flags, int null_behavior) {
  const bool set_has_null = (flags & kFlagSetHasNull) && null_behavior != AH_NULL_SKIP;
  NullRule r;
  r.vmiss = !(null_behavior == AH_NULL_INCONCLUSIVE && set_has_null);
  r.dnull = null_behavior == AH_NULL_MATCH && set_has_null;
  r.vnull = r.dnull || null_behavior == AH_NULL_SKIP || (!set_has_null && null_behavior == AH_NULL_MATCH);
  return r;
}

// ---- output: bits [pos, pos + cnt) := low cnt bits of `word`, every other bit preserved -----
__device__ __forceinline__ void put_bits(uint8_t* __restrict__ bm, int64_t pos, unsigned long long word, int cnt) {
  const uintptr_t addr = (uintptr_t)bm + (uintptr_t)(pos >> 3);
  const int sub = (int)(pos & 7);
  if (cnt == 64 && sub == 0 && (addr & 7) == 0) {
    *(unsigned long long*)addr = word;
    return;
  }
  // general position: up to three aligned 32-bit words, atomics because a neighbouring chunk may
  // own the other bits of the same word
  const uintptr_t base = addr & ~(uintptr_t)3;
  int shift = (int)((addr - base) * 8) + sub;  // 0..31
  const unsigned long long m = cnt >= 64 ? ~0ull : ((1ull << cnt) - 1);
  word &= m;
  unsigned* w = (unsigned*)base;
  // 96-bit window
  const unsigned long long mlo = m << shift, vlo = word << shift;
  const unsigned long long mhi = shift ? (m >> (64 - shift)) : 0ull, vhi = shift ? (word >> (64 - shift)) : 0ull;
  const unsigned m0 = (unsigned)mlo, m1 = (unsigned)(mlo >> 32), m2 = (unsigned)mhi;
  const unsigned v0 = (unsigned)vlo, v1 = (unsigned)(vlo >> 32), v2 = (unsigned)vhi;
  if (m0) { atomicAnd(&w[0], ~m0); if (v0) atomicOr(&w[0], v0); }
  if (m1) { atomicAnd(&w[1], ~m1); if (v1) atomicOr(&w[1], v1); }
  if (m2) { atomicAnd(&w[2], ~m2); if (v2) atomicOr(&w[2], v2); }
}

}  // namespace

// one piece of a fixed-width value set: `values` = its row 0, validity bit valid_off + i
struct SetPart {
  const void* values;
  const uint8_t* valid;
  int64_t valid_off, n;
};
// ah_is_in over a value set in pieces (byte_width 1, 2, 4 or 8; `values` = row 0 of the call, validity bit off + i).  No AH_ENTER.
int ah_is_in_parts(ah_ctx* c, int byte_width, const void* values, const uint8_t* valid, int64_t off, int64_t n, int nparts, const SetPart* parts,
                   int null_behavior, uint8_t* out_data, uint8_t* out_valid, int64_t out_bit_offset);
