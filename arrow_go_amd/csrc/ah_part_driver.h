// ah_part_driver.h — what the host drivers of the partition-first paths (ah_groupby.hip, ah_hash_part.hip) have in common: a run-time
// switch as a compile-time constant (one launch per kernel), the temporaries described once, the three words a call brings home.
#pragma once
#include <type_traits>
#include "ah_partition.h"

namespace {

// f(std::true_type{}) or f(std::false_type{}): the launch inside f is written once, with b.value among its template arguments
template <class F>
inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// How a driver's attempt ended (an error code travels beside it).
enum class PartOutcome {
  Done,       // out_* hold the result
  Declined,   // not this path's call, or the attempt is void (kPartOverflow, kPartWide): the caller's other path answers
  Retry,      // a reserving attempt whose regions were too small (kPartRegionSmall alone) or whose larger temporaries did not fit
};

// The temporaries of one call: `carve` lists them (TempCarver::take) and is run twice — without a base to measure, then on the
// reserved block.  Out of device memory → *fits = false and, with may_decline, AH_OK and no error text (a path with smaller
// temporaries answers); any other failure of the reservation is returned as it is.
template <class Carve>
inline int part_reserve(ah_ctx* c, bool may_decline, Carve&& carve, bool* fits) {
  TempCarver measure, tc;
  carve(measure);
  bool oom = false;
  const int rc = ah_temp_reserve(c, measure.used, (void**)&tc.base, &oom);
  *fits = rc == AH_OK;
  if (rc != AH_OK && !(oom && may_decline)) return rc;
  if (rc != AH_OK) { c->err[0] = 0; return AH_OK; }
  carve(tc);
  return tc.used == measure.used ? AH_OK : ah_fail(c, AH_EHIP, "temporaries: %zu bytes carved, %zu reserved", tc.used, measure.used);
}

// {flags, total, null id} as a call's last kernel left them → the outcome; Done fills the two host outputs (nullable)
inline PartOutcome part_outcome(const unsigned long long w[3], bool reserving, int64_t* out_total, int32_t* out_null_id) {
  const unsigned flags = (unsigned)w[0];
  if (flags) return reserving && (flags & kPartRegionSmall) && !(flags & (kPartOverflow | kPartWide)) ? PartOutcome::Retry : PartOutcome::Declined;
  if (out_total) *out_total = (int64_t)w[1];
  if (out_null_id) *out_null_id = (int32_t)(long long)w[2];
  return PartOutcome::Done;
}
// … brought home from dscalars[ds_flags … + 2] through the mailbox (everything enqueued before has completed when this returns)
inline int part_finish(ah_ctx* c, int ds_flags, bool reserving, int64_t* out_total, int32_t* out_null_id, PartOutcome* outcome) {
  unsigned long long w[3];
  const int rc = ah_mailbox_read(c, (const unsigned long long*)&c->dscalars[ds_flags], 3, w);
  if (rc == AH_OK) *outcome = part_outcome(w, reserving, out_total, out_null_id);
  return rc;
}

// attempt(reserving, &outcome): first reserving, and once more behind a histogram when that says Retry — the one place a call is run again
template <class Attempt>
inline int part_with_retry(Attempt&& attempt, PartOutcome* outcome) {
  const int rc = attempt(true, outcome);
  return rc == AH_OK && *outcome == PartOutcome::Retry ? attempt(false, outcome) : rc;
}

}  // namespace
