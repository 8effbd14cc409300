// ah_index.h — the index layer of the selection kernels: ah_take.hip (primitive, clustered, boolean, arbitrary-width Take),
// ah_take_binned.hip (binned Take), ah_varlen.hip (var-length Take) and, for the value carriers only, ah_filter.hip.  The unsigned
// carrier of a value width (UIntOf), the index rule (index_ref), the lane of a row-per-lane Take (lane_index), the
// idx_byte_width × idx_signed → IdxT and value-width dispatchers, the entry checks every Take starts with, and the one turn from
// "first offending position" into the reference's error.
#pragma once
#include <type_traits>
#include "ah_common.h"

namespace {

// values of W bytes move as unsigned integers of that width …
template <int W> struct UIntOf;
template <> struct UIntOf<1> { using type = uint8_t; };
template <> struct UIntOf<2> { using type = uint16_t; };
template <> struct UIntOf<4> { using type = uint32_t; };
template <> struct UIntOf<8> { using type = uint64_t; };
// … and 16- and 32-byte values — Decimal128 / Decimal256 and FixedSizeBinary of those widths (FSBImpl, vector_selection.go:1997, takes any
// width byte by byte; here the widths that are whole 16-byte accesses) — as 2 / 4 × 64-bit vectors, in the plain gather kernel only
template <> struct UIntOf<16> { using type = unsigned long long __attribute__((ext_vector_type(2))); };
template <> struct UIntOf<32> { using type = unsigned long long __attribute__((ext_vector_type(4))); };

// The index rule (checkIndexBounds, kernels/helpers.go:937-939; takeIdxDispatch, vector_selection.go:1147-1158): an index is
// reinterpreted as unsigned of its own width, and a VALID index slot that is negative or ≥ nvalues is out of bounds.  Whether the slot
// is valid, and how the smallest offending position is reduced and published, is each kernel's own business.
struct IndexRef {
  uint64_t u;   // the unsigned value
  bool oob;     // negative or past the column
};
template <typename IdxT>
__device__ __forceinline__ IndexRef index_ref(IdxT s, uint64_t nvalues) {
  const uint64_t u = (uint64_t)(typename std::make_unsigned<IdxT>::type)s;
  return IndexRef{u, (std::is_signed<IdxT>::value && s < 0) || u >= nvalues};
}

// The row-per-lane Takes (boolean values, slots of any width, var-length lengths): f(c, i) for this lane's row i of every 64-row
// chunk c the wave owns — chunks are dealt to the grid's waves round-robin, all 64 lanes call f (rows past n included: ballots).
template <int BLOCK, typename F>
__device__ __forceinline__ void for_wave_chunks(int64_t n, F f) {
  const int64_t nchunks = (n + 63) >> 6, wave_stride = (int64_t)gridDim.x * (BLOCK / 64);
  for (int64_t c = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); c < nchunks; c += wave_stride) f(c, c * 64 + ah_lane());
}
// … and row i's index there: ok = the row exists, its index slot is valid and in bounds (else the position goes to *first_bad) and
// the value it names is valid; u = the index (0 for a row past the end or a null slot).
struct LaneIndex {
  bool ok;
  uint64_t u;
};
template <typename IdxT>
__device__ __forceinline__ LaneIndex lane_index(const IdxT* __restrict__ idx, const uint8_t* __restrict__ ivalid, int64_t ioff, int64_t i, int64_t n,
                                                const uint8_t* __restrict__ vvalid, int64_t voff, uint64_t nvalues,
                                                unsigned long long* __restrict__ first_bad) {
  LaneIndex r{false, 0};
  if (i < n && ah_bit(ivalid, ioff + i)) {
    const IndexRef x = index_ref(idx[i], nvalues);
    r.u = x.u;
    if (x.oob) atomicMin(first_bad, (unsigned long long)i);
    else r.ok = ah_bit(vvalid, voff + (int64_t)x.u);
  }
  return r;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// idx_byte_width × idx_signed → f(TypeTag<IdxT>{}); false (and no call) for a width no index type has — what that means is the call
// site's decision ("invalid indices byte width", vector_selection.go:1157, or "this path is not used")
template <class F>
inline bool with_index_type(int iw, int is_signed, F&& f) {
  switch (iw) {
    case 1: if (is_signed) f(TypeTag<int8_t>{}); else f(TypeTag<uint8_t>{}); return true;
    case 2: if (is_signed) f(TypeTag<int16_t>{}); else f(TypeTag<uint16_t>{}); return true;
    case 4: if (is_signed) f(TypeTag<int32_t>{}); else f(TypeTag<uint32_t>{}); return true;
    case 8: if (is_signed) f(TypeTag<int64_t>{}); else f(TypeTag<uint64_t>{}); return true;
  }
  return false;
}
// byte width of a value → f(std::integral_constant<int, W>{}) for the W among Ws...; false (and no call) for any other width
template <int... Ws, class F>
inline bool with_value_width(int w, F&& f) {
  return ((w == Ws ? (f(std::integral_constant<int, Ws>{}), true) : false) || ...);
}

// What every Take entry point starts with: lengths and offsets, the buffers the call cannot do without (`have_buffers`, the caller's
// own list), a zeroed null count, and: a caller that passes no out_valid has decided there are no nulls (PrimitiveTake :1176 uses the
// null COUNTS) — both validity inputs are then ignored exactly like the reference's no-null path.
inline int take_enter(ah_ctx* c, int64_t nidx, int64_t nvalues, int64_t voff, int64_t ioff, bool have_buffers, const uint8_t* out_valid,
                      const uint8_t** vvalid, const uint8_t** ivalid, int64_t* out_null_count_host) {
  if (nidx < 0 || nvalues < 0 || voff < 0 || ioff < 0) return ah_fail(c, AH_EINVALID, "take: negative length/offset");
  if (out_null_count_host) *out_null_count_host = 0;
  if (!have_buffers) return ah_fail(c, AH_EINVALID, "take: null buffer");
  if (!out_valid) *vvalid = *ivalid = nullptr;
  return AH_OK;
}

// bad_pos = the smallest position of an out-of-bounds index, home from the device: fetch that index for the message ("%d out of
// bounds", helpers.go:950) — an unsigned 64-bit index prints as unsigned
inline int take_fail_bad_index(ah_ctx* c, const void* idx, int iw, int is_signed, uint64_t bad_pos, int64_t* bad_index_host) {
  uint64_t raw = 0;
  AH_HIP(c, hipMemcpy(&raw, (const uint8_t*)idx + bad_pos * (uint64_t)iw, (size_t)iw, hipMemcpyDeviceToHost));
  int64_t val;
  switch (iw) {
    case 1: val = is_signed ? (int64_t)(int8_t)raw : (int64_t)(uint8_t)raw; break;
    case 2: val = is_signed ? (int64_t)(int16_t)raw : (int64_t)(uint16_t)raw; break;
    case 4: val = is_signed ? (int64_t)(int32_t)raw : (int64_t)(uint32_t)raw; break;
    default: val = (int64_t)raw; break;
  }
  if (bad_index_host) *bad_index_host = val;
  if (is_signed || iw < 8) return ah_fail(c, AH_EINDEX, "%lld out of bounds", (long long)val);
  return ah_fail(c, AH_EINDEX, "%llu out of bounds", (unsigned long long)raw);
}

}  // namespace
