// ah_setlookup.h — pieces shared by ah_setlookup.hip (is_in of 1/2/4/8-byte keys) and ah_setlookup_binary.hip (is_in of
// byte-string and wider fixed-width keys): the null-behaviour truth table and the internal entry of the fixed-width kernels
// over a value set in pieces.  The result words are written with put_bits / put_word (ah_common.h).
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
