// ah_lz4_enc.hip — independent LZ4 blocks compressed in HBM, one wavefront per block (ah_lz4_compress_blocks), and the IPC writer's
// messages put together from the compressed blocks (ah_ipc_pack_body).  DESIGN.md §3.8.
//
// No reference analogue: the reference compresses IPC bodies on the host (arrow/ipc/writer.go:425-470, compression.go:66-72).  The
// mirror image of ah_lz4.hip: every ≤ 64 KiB piece of a body buffer is compressed by one workgroup of one wavefront — the piece
// staged in LDS (64 KiB), a table of 4096 16-bit positions (8 KiB), a 4 KiB output window and 256 bytes of lane state: 78 080 bytes,
// two blocks per CU — by the algorithm of ah_lz4_enc.h, which the tests' host harness runs lane by lane to the same bytes.
// ah_ipc_pack_body then moves the blocks, whose sizes the host now knows, to their final places between the length prefixes, frame
// headers, block size words and end marks the host has laid out (host/ipc_writer.cc).
#include "ah_common.h"
#include "ah_lz4_enc.h"

#include <vector>

namespace {

struct WavePar {
  template <class F>
  __device__ __forceinline__ void lanes(F&& f) {
    f((int)threadIdx.x, AH_WAVE);
    __syncthreads();
  }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
  template <class F>
  __device__ __forceinline__ uint32_t first(F&& f) {
    const unsigned long long hit = __ballot(f((int)threadIdx.x, AH_WAVE));
    return hit ? (uint32_t)__ffsll((long long)hit) - 1u : (uint32_t)AH_WAVE;
  }
};

constexpr uint32_t kEncStoredBit = 1u << 31;

__global__ __launch_bounds__(AH_WAVE) void lz4_compress_blocks_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                      const int64_t* __restrict__ blocks, uint32_t* __restrict__ result) {
  __shared__ alignas(16) uint8_t image[kLz4MaxBlock];
  __shared__ alignas(16) uint16_t table[kLz4EncTable];
  __shared__ alignas(16) uint8_t win[kLz4EncOutWindow];
  __shared__ uint32_t state[kLz4EncMaxLanes];
  static_assert(kLz4EncMaxLanes == AH_WAVE, "one lane state word per lane of the wavefront");
  const int64_t* b = blocks + 3 * (int64_t)blockIdx.x;
  const int64_t src_off = b[0], src_len = b[1], dst_off = b[2];
  WavePar par;
  uint32_t size = 0, lz4_size = 0;
  if (src_len > 0 && src_len <= (int64_t)kLz4MaxBlock)   // (the table was checked on the host)
    size = ah_lz4_encode_block(par, src + src_off, (uint32_t)src_len, dst + dst_off, image, table, state, win, &lz4_size);
  if (threadIdx.x == 0) result[blockIdx.x] = size | (lz4_size >= (uint32_t)src_len ? kEncStoredBit : 0u);
}

// ---- the body of an IPC message from its pieces --------------------------------------------------------------------------------
// One workgroup per row {src_off, len, dst_off, word}: len bytes of source (word & 3: 0 compressed blocks, 1 plain bytes, 2 the
// host's literal bytes) → dst + dst_off; word bit 8: the 32 bits above bit 32 are written, little-endian, in the 4 bytes before
// dst_off (the size word of a frame's block).  16 bytes per lane to aligned addresses of dst; the source of such a line is read as
// one 16-byte load where it is aligned too, else as the aligned 4-byte words that hold it, shifted — only where all of those words
// lie inside the source buffer, so no load leaves it.
constexpr int kPackThreads = 256;
struct PackSources {
  const uint8_t* base[3];
  int64_t bytes[3];
};

__global__ __launch_bounds__(kPackThreads) void ipc_pack_body_kernel(PackSources srcs, uint8_t* __restrict__ dst, const int64_t* __restrict__ rows) {
  const int64_t* r = rows + 4 * (int64_t)blockIdx.x;
  const int64_t src_off = r[0], len = r[1], dst_off = r[2], word = r[3];
  const int kind = (int)(word & 3);
  const uint8_t* __restrict__ base = srcs.base[kind];
  const int64_t base_bytes = srcs.bytes[kind];
  uint8_t* out = dst + dst_off;
  const int t = (int)threadIdx.x;
  if ((word & 0x100) && t < 4) out[t - 4] = (uint8_t)((uint64_t)word >> (32 + 8 * t));
  if (len <= 0) return;
  const uint8_t* in = base + src_off;
  int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15);
  if (head > len) head = len;
  if (t < head) out[t] = in[t];
  const int64_t nvec = (len - head) / 16;
  for (int64_t j = t; j < nvec; j += kPackThreads) {
    const uint8_t* s = in + head + 16 * j;
    uint8_t* d = out + head + 16 * j;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(s);
    if ((sa & 15) == 0) {
      *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
      continue;
    }
    const uint32_t sh = (uint32_t)(sa & 3) * 8;
    const int64_t first_word = (int64_t)((sa & ~(uintptr_t)3) - reinterpret_cast<uintptr_t>(base));   // ≥ −3
    if (first_word >= 0 && first_word + 20 <= base_bytes) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(base + first_word);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
      uint4 v;
      if (sh == 0) {
        v = make_uint4(w0, w1, w2, w3);
      } else {
        const uint32_t w4 = w[4];
        v = make_uint4((w0 >> sh) | (w1 << (32 - sh)), (w1 >> sh) | (w2 << (32 - sh)), (w2 >> sh) | (w3 << (32 - sh)), (w3 >> sh) | (w4 << (32 - sh)));
      }
      *reinterpret_cast<uint4*>(d) = v;
    } else {
      for (int k = 0; k < 16; k++) d[k] = s[k];
    }
  }
  const int64_t done = head + 16 * nvec;
  if (done + t < len) out[done + t] = in[done + t];   // (fewer than 16 bytes)
}

}  // namespace

AH_EXPORT int ah_lz4_compress_blocks(ah_ctx* c, const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, const int64_t* blocks_host,
                                     int64_t nblocks, int32_t* out_sizes_host, uint8_t* out_stored_host) {
  AH_ENTER(c);
  if (nblocks < 0 || src_bytes < 0 || dst_bytes < 0) return ah_fail(c, AH_EINVALID, "lz4_compress_blocks: negative length");
  if (nblocks == 0) return AH_OK;
  if (nblocks > 0x7fffffff) return ah_fail(c, AH_EINVALID, "lz4_compress_blocks: more than 2^31 - 1 blocks");
  if (!blocks_host || !out_sizes_host || !out_stored_host || (!src && src_bytes > 0) || (!dst && dst_bytes > 0))
    return ah_fail(c, AH_EINVALID, "lz4_compress_blocks: null buffer");
  int64_t dst_end = 0;
  for (int64_t i = 0; i < nblocks; i++) {
    const int64_t so = blocks_host[3 * i], sl = blocks_host[3 * i + 1], d0 = blocks_host[3 * i + 2];
    if (sl < 0 || sl > (int64_t)kLz4MaxBlock) return ah_fail(c, AH_EINVALID, "lz4_compress_blocks: block %lld: src_len %lld outside 0 … 65536", (long long)i, (long long)sl);
    if (so < 0 || so > src_bytes || sl > src_bytes - so)
      return ah_fail(c, AH_EINVALID, "lz4_compress_blocks: block %lld: source range outside the %lld source bytes", (long long)i, (long long)src_bytes);
    if (d0 < 0 || d0 > dst_bytes || sl > dst_bytes - d0)
      return ah_fail(c, AH_EINVALID, "lz4_compress_blocks: block %lld: its slot of src_len bytes lies outside the %lld output bytes", (long long)i, (long long)dst_bytes);
    if (d0 < dst_end) return ah_fail(c, AH_EINVALID, "lz4_compress_blocks: block %lld: slots of src_len bytes must ascend without overlap", (long long)i);
    dst_end = d0 + sl;
  }
  if (ah_fcache_overlaps(c, dst, (size_t)dst_bytes)) c->fcache.valid = false;
  void* tmp = nullptr;
  const size_t table_bytes = (size_t)nblocks * 24;
  if (int rc = ah_scratch_reserve(c, ah_pad(table_bytes) + ah_pad((size_t)nblocks * 4), &tmp)) return rc;
  int64_t* table = (int64_t*)tmp;
  uint32_t* result = (uint32_t*)((uint8_t*)tmp + ah_pad(table_bytes));
  AH_HIP(c, hipMemcpyAsync(table, blocks_host, table_bytes, hipMemcpyHostToDevice, c->stream));
  lz4_compress_blocks_kernel<<<(unsigned)nblocks, AH_WAVE, 0, c->stream>>>(src, dst, table, result);
  AH_LAUNCH_CHECK(c);
  static_assert(sizeof(int32_t) == sizeof(uint32_t), "");
  AH_HIP(c, hipMemcpyAsync(out_sizes_host, result, (size_t)nblocks * 4, hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < nblocks; i++) {
    const uint32_t w = (uint32_t)out_sizes_host[i];
    out_stored_host[i] = (uint8_t)(w >> 31);
    out_sizes_host[i] = (int32_t)(w & ~kEncStoredBit);
  }
  return AH_OK;
}

AH_EXPORT int ah_ipc_pack_body(ah_ctx* c, const uint8_t* comp, int64_t comp_bytes, const uint8_t* plain, int64_t plain_bytes, const uint8_t* lits_host,
                               int64_t lits_bytes, const int64_t* rows_host, int64_t nrows, uint8_t* dst, int64_t dst_bytes) {
  AH_ENTER(c);
  if (nrows < 0 || comp_bytes < 0 || plain_bytes < 0 || lits_bytes < 0 || dst_bytes < 0) return ah_fail(c, AH_EINVALID, "ipc_pack_body: negative length");
  if (nrows > 0x7fffffff) return ah_fail(c, AH_EINVALID, "ipc_pack_body: more than 2^31 - 1 rows");
  if ((nrows > 0 && !rows_host) || (!comp && comp_bytes > 0) || (!plain && plain_bytes > 0) || (!lits_host && lits_bytes > 0) || (!dst && dst_bytes > 0))
    return ah_fail(c, AH_EINVALID, "ipc_pack_body: null buffer");
  const int64_t src_bytes[3] = {comp_bytes, plain_bytes, lits_bytes};
  int64_t at = 0;   // the rows tile [0, dst_bytes): every byte of the body is written, and written once
  for (int64_t i = 0; i < nrows; i++) {
    const int64_t so = rows_host[4 * i], len = rows_host[4 * i + 1], d0 = rows_host[4 * i + 2], word = rows_host[4 * i + 3];
    const int kind = (int)(word & 3);
    if (kind > 2 || (word & 0xFFFFFEFCll) != 0) return ah_fail(c, AH_EINVALID, "ipc_pack_body: row %lld: unknown source or flag", (long long)i);
    if (len < 0 || so < 0 || so > src_bytes[kind] || len > src_bytes[kind] - so)
      return ah_fail(c, AH_EINVALID, "ipc_pack_body: row %lld: source range outside the %lld bytes of source %d", (long long)i, (long long)src_bytes[kind], kind);
    const int64_t lead = (word & 0x100) ? 4 : 0;
    if (d0 - lead != at) return ah_fail(c, AH_EINVALID, "ipc_pack_body: row %lld starts at %lld, the row before it ended at %lld", (long long)i, (long long)(d0 - lead), (long long)at);
    if (d0 > dst_bytes || len > dst_bytes - d0) return ah_fail(c, AH_EINVALID, "ipc_pack_body: row %lld: output range outside the %lld output bytes", (long long)i, (long long)dst_bytes);
    at = d0 + len;
  }
  if (at != dst_bytes) return ah_fail(c, AH_EINVALID, "ipc_pack_body: the rows end at %lld of %lld output bytes", (long long)at, (long long)dst_bytes);
  if (nrows == 0) return AH_OK;
  if (ah_fcache_overlaps(c, dst, (size_t)dst_bytes)) c->fcache.valid = false;
  void* tmp = nullptr;
  const size_t table_bytes = (size_t)nrows * 32;
  if (int rc = ah_scratch_reserve(c, ah_pad(table_bytes) + ah_pad((size_t)lits_bytes), &tmp)) return rc;
  int64_t* table = (int64_t*)tmp;
  uint8_t* lits = (uint8_t*)tmp + ah_pad(table_bytes);
  AH_HIP(c, hipMemcpyAsync(table, rows_host, table_bytes, hipMemcpyHostToDevice, c->stream));
  if (lits_bytes > 0) AH_HIP(c, hipMemcpyAsync(lits, lits_host, (size_t)lits_bytes, hipMemcpyHostToDevice, c->stream));
  PackSources srcs{{comp, plain, lits}, {comp_bytes, plain_bytes, lits_bytes}};
  ipc_pack_body_kernel<<<(unsigned)nrows, kPackThreads, 0, c->stream>>>(srcs, dst, table);
  AH_LAUNCH_CHECK(c);
  AH_HIP(c, hipStreamSynchronize(c->stream));   // the host's rows and literal bytes are the caller's again
  return AH_OK;
}
