// ah_minmax.hip — min and max of an integer column in one pass (row §8(f)-2).
//
// Replaces utils.GetMinMax{Int8…Uint64} (internal/utils/min_max.go:161-215; AVX2 leaves
// _int64_max_min_avx2 …, internal/utils/_lib/min_max.c:23-126; pure Go :30-148): min starts at the
// type's maximum and max at its minimum, so an EMPTY slice returns (MaxOf, MinOf).  The reference
// uses it for Parquet statistics and dictionary-index validation; validity is not consulted.
// On the streaming-reduction layer (ah_reduce.h, DESIGN.md §3 "Streaming reductions"), 2 workgroups per CU.  w bytes per row.
#include <limits>
#include "ah_common.h"
#include "ah_reduce.h"

namespace {

constexpr int kBlock = kReduceBlock;
constexpr int kUnroll = kReduceUnroll;

template <typename T>
struct MM {   // the part
  T lo, hi;
  __device__ __forceinline__ void init() { lo = std::numeric_limits<T>::max(); hi = std::numeric_limits<T>::min(); }
  __device__ __forceinline__ void add(T v) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
  __device__ __forceinline__ void merge(const MM& o) { lo = o.lo < lo ? o.lo : lo; hi = o.hi > hi ? o.hi : hi; }
};

template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) void minmax_partials_kernel(const T* __restrict__ values, int64_t n, MM<T>* __restrict__ partials) {
  constexpr int V = 16 / sizeof(T);
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  MM<T> a;
  a.init();
  const ah_split sp = ah_reduce_split(values, n);   // 16-byte aligned body + element head / tail
  // Rows out of the loaded words by shifts: a __builtin_bit_cast to a carrier struct costs the load its hint (ah_common.h).
  // The scheduling group (four VMEM reads first) keeps an iteration's loads together: the compares are so cheap that the
  // scheduler otherwise waits for the first vector in front of the third load — two loads in flight instead of four.  It
  // relies on ah_reduce_walk calling f kReduceUnroll = 4 times, unrolled, behind the iteration's four loads (in the ragged
  // steps, behind one plain load, it orders nothing); tests/test_isa_hints.py counts the hinted loads, not their grouping.
  ah_reduce_walk<u32x4, NT>((const u32x4*)(values + sp.head), sp.nvec, [&](int64_t, const u32x4& v) {
    __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
#pragma unroll
    for (int j = 0; j < V; j++) {
      if constexpr (sizeof(T) == 8) a.add((T)(((uint64_t)v[2 * j + 1] << 32) | v[2 * j]));
      else a.add((T)(v[j * (int)sizeof(T) / 4] >> (8 * ((j * (int)sizeof(T)) & 3))));
    }
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t k = 0; k < sp.head; k++) a.add(values[k]);
    for (int64_t k = n - sp.tail; k < n; k++) a.add(values[k]);
  }
  a = ah_block_reduce<kBlock>(a);
  if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

template <typename T>
struct EmitMinMax {
  T* out;   // [min, max]
  __device__ __forceinline__ void operator()(const MM<T>& a) const { out[0] = a.lo; out[1] = a.hi; }
};

template <typename T>
int run_minmax(ah_ctx* c, const void* values, int64_t n, void* out_min_host, void* out_max_host) {
  T* res = (T*)&c->dscalars[kDsMinMax];
  int rc = ah_reduce_two_launch<MM<T>>(c, ah_ceil_div(ah_ceil_div(n, 16 / sizeof(T)), (int64_t)kBlock * kUnroll), /*default_bpc=*/2,
      [&](unsigned grid, MM<T>* partials) {
        if (c->tune_nt) minmax_partials_kernel<T, true><<<grid, kBlock, 0, c->stream>>>((const T*)values, n, partials);
        else minmax_partials_kernel<T, false><<<grid, kBlock, 0, c->stream>>>((const T*)values, n, partials);
      },
      EmitMinMax<T>{res});
  if (rc != AH_OK) return rc;
  AH_HIP(c, hipMemcpyAsync(c->pinned, res, 2 * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  memcpy(out_min_host, (const void*)c->pinned, sizeof(T));
  memcpy(out_max_host, (const uint8_t*)c->pinned + sizeof(T), sizeof(T));
  return AH_OK;
}

}  // namespace

AH_EXPORT int ah_min_max(ah_ctx* c, int type, const void* values, int64_t n, void* out_min_host, void* out_max_host) {
  AH_ENTER(c);
  if (n < 0) return ah_fail(c, AH_EINVALID, "min_max: negative length");
  if (!out_min_host || !out_max_host) return ah_fail(c, AH_EINVALID, "min_max: null result pointer");
  const int w = ah_type_width(type);
  if (!w || type == AH_FLOAT32 || type == AH_FLOAT64) return ah_fail(c, AH_ENOTIMPL, "min_max: integer types only (got %d)", type);
  if (n > 0 && (!values || ((uintptr_t)values & (uintptr_t)(w - 1)))) return ah_fail(c, AH_EINVALID, "min_max: null or misaligned buffer");
  switch (type) {
#define AH_MM(ID, T)                                                                                              \
  case ID: {                                                                                                      \
    if (n == 0) { T lo = std::numeric_limits<T>::max(), hi = std::numeric_limits<T>::min();                     \
                  memcpy(out_min_host, &lo, sizeof(T)); memcpy(out_max_host, &hi, sizeof(T)); return AH_OK; }     \
    return run_minmax<T>(c, values, n, out_min_host, out_max_host);                                               \
  }
    AH_MM(AH_UINT8, uint8_t) AH_MM(AH_INT8, int8_t) AH_MM(AH_UINT16, uint16_t) AH_MM(AH_INT16, int16_t)
    AH_MM(AH_UINT32, uint32_t) AH_MM(AH_INT32, int32_t) AH_MM(AH_UINT64, uint64_t) AH_MM(AH_INT64, int64_t)
#undef AH_MM
  }
  return ah_fail(c, AH_ENOTIMPL, "min_max: integer types only (got %d)", type);
}
