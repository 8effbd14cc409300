// ah_lz4.hip — independent LZ4 blocks inflated in HBM, one wavefront per block (ah_lz4_decompress_blocks).
//
// No reference analogue: the reference inflates IPC bodies on the host (arrow/ipc/compression.go:66-72, pierrec/lz4).  The frames its
// writer produces — 64 KiB blocks that do not refer to each other — are taken apart by the host (host/lz4_frame.h) into a table of
// {source range, output range} and decoded here, every block by one workgroup of one wavefront:
//   * the block's output image (≤ 64 KiB) is built in LDS, so a match reads LDS and never an HBM byte another lane has just written;
//   * the compressed bytes pass through a 4 KiB LDS window the 64 lanes refill together with 16-byte loads;
//   * the finished image goes to HBM once, 16 bytes per lane.
// 68 KiB of LDS per workgroup: two blocks per CU.  The decoder itself — parsing, bounds, copy loops — is ah_lz4.h, shared with the
// host harness of the tests.  No block waits for another one and no loop is unbounded: a corrupt block ends as a status byte.
#include "ah_common.h"
#include "ah_lz4.h"

#include <vector>

namespace {

constexpr int64_t kStoredBit = (int64_t)1 << 62;

struct WavePar {
  template <class F>
  __device__ __forceinline__ void lanes(F&& f) {
    f((int)threadIdx.x, AH_WAVE);
    __syncthreads();
  }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
};

__global__ __launch_bounds__(AH_WAVE) void lz4_blocks_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                             const int64_t* __restrict__ blocks, uint8_t* __restrict__ status) {
  __shared__ alignas(16) uint8_t image[kLz4MaxBlock];
  __shared__ alignas(16) uint8_t win[kLz4Window];
  const int64_t* b = blocks + 4 * (int64_t)blockIdx.x;
  const int64_t src_off = b[0], src_len = b[1] & ~kStoredBit, dst_off = b[2], dst_len = b[3];
  const bool stored = (b[1] & kStoredBit) != 0;
  WavePar par;
  int st = AH_LZ4_CORRUPT;   // the table was checked on the host; a length outside the decoder's range is still only a status
  if (src_len >= 0 && src_len <= (int64_t)kLz4MaxSrc && dst_len >= 0 && dst_len <= (int64_t)kLz4MaxBlock)
    st = ah_lz4_decode_block(par, src + src_off, (uint32_t)src_len, stored, dst + dst_off, (uint32_t)dst_len, image, win);
  if (threadIdx.x == 0) status[blockIdx.x] = (uint8_t)st;
}

}  // namespace

AH_EXPORT int ah_lz4_decompress_blocks(ah_ctx* c, const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes,
                                       const int64_t* blocks_host, int64_t nblocks, uint8_t* out_status_host, int64_t* out_nbad_host) {
  AH_ENTER(c);
  if (out_nbad_host) *out_nbad_host = 0;
  if (nblocks < 0 || src_bytes < 0 || dst_bytes < 0) return ah_fail(c, AH_EINVALID, "lz4_decompress_blocks: negative length");
  if (nblocks == 0) return AH_OK;
  if (nblocks > 0x7fffffff) return ah_fail(c, AH_EINVALID, "lz4_decompress_blocks: more than 2^31 - 1 blocks");
  if (!blocks_host || (!src && src_bytes > 0) || (!dst && dst_bytes > 0)) return ah_fail(c, AH_EINVALID, "lz4_decompress_blocks: null buffer");
  int64_t dst_end = 0;
  for (int64_t i = 0; i < nblocks; i++) {
    const int64_t* b = blocks_host + 4 * i;
    const int64_t so = b[0], sl = b[1] & ~kStoredBit, d0 = b[2], dl = b[3];
    if (b[1] < 0 || so < 0 || so > src_bytes || sl > src_bytes - so || sl > (int64_t)kLz4MaxSrc)
      return ah_fail(c, AH_EINVALID, "lz4_decompress_blocks: block %lld: source range outside the %lld source bytes", (long long)i, (long long)src_bytes);
    if (dl < 0 || dl > (int64_t)kLz4MaxBlock) return ah_fail(c, AH_EINVALID, "lz4_decompress_blocks: block %lld: dst_len %lld beyond 65536", (long long)i, (long long)dl);
    if (d0 < 0 || d0 > dst_bytes || dl > dst_bytes - d0)
      return ah_fail(c, AH_EINVALID, "lz4_decompress_blocks: block %lld: output range outside the %lld output bytes", (long long)i, (long long)dst_bytes);
    if (d0 < dst_end) return ah_fail(c, AH_EINVALID, "lz4_decompress_blocks: block %lld: output ranges must ascend without overlap", (long long)i);
    dst_end = d0 + dl;
  }
  void* tmp = nullptr;
  const size_t table_bytes = (size_t)nblocks * 32;
  if (int rc = ah_scratch_reserve(c, ah_pad(table_bytes) + ah_pad((size_t)nblocks), &tmp)) return rc;
  int64_t* table = (int64_t*)tmp;
  uint8_t* status = (uint8_t*)tmp + ah_pad(table_bytes);
  AH_HIP(c, hipMemcpyAsync(table, blocks_host, table_bytes, hipMemcpyHostToDevice, c->stream));
  lz4_blocks_kernel<<<(unsigned)nblocks, AH_WAVE, 0, c->stream>>>(src, dst, table, status);
  AH_LAUNCH_CHECK(c);
  std::vector<uint8_t> own;
  if (!out_status_host) {
    own.resize((size_t)nblocks);
    out_status_host = own.data();
  }
  AH_HIP(c, hipMemcpyAsync(out_status_host, status, (size_t)nblocks, hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  int64_t nbad = 0;
  for (int64_t i = 0; i < nblocks; i++) nbad += out_status_host[i] != 0;
  if (out_nbad_host) *out_nbad_host = nbad;
  return AH_OK;
}
