// ah_bytes.h — byte-string pieces shared by ah_hash.hip (unique / dictionary_encode of binary and fixed-width binary keys) and
// ah_setlookup_binary.hip (is_in of the same keys): unaligned 8-byte loads, the 64-bit hash of a byte string, byte equality.
#pragma once
#include "ah_common.h"

namespace {

struct U64u { unsigned long long v; } __attribute__((packed, aligned(1)));
__device__ __forceinline__ unsigned long long load8(const uint8_t* p) { return reinterpret_cast<const U64u*>(p)->v; }
__device__ __forceinline__ unsigned long long load_tail(const uint8_t* p, int nb) {  // 1..7 bytes, little-endian
  unsigned long long w = 0;
  for (int t = 0; t < nb; t++) w |= (unsigned long long)p[t] << (8 * t);
  return w;
}
// Any 64-bit hash will do: ids and dictionary order depend only on which rows are EQUAL and on row order,
// never on hash values (the reference's xxh3 / custom short-string hash, hash_funcs.go:86-124, decides
// only where its own memo table stores an entry).  Multiply-xorshift over 8-byte words.
__device__ __forceinline__ uint64_t hash_bytes(const uint8_t* p, int64_t len) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)len * 0xC2B2AE3D27D4EB4Full);
  int64_t j = 0;
  for (; j + 8 <= len; j += 8) {
    h = (h ^ load8(p + j)) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  if (j < len) {
    h = (h ^ load_tail(p + j, (int)(len - j))) * 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 29;
  }
  h *= 0x9FB21C651E98DF25ull;
  return h ^ (h >> 32);
}
__device__ __forceinline__ bool equal_bytes(const uint8_t* a, const uint8_t* b, int64_t len) {
  int64_t j = 0;
  for (; j + 8 <= len; j += 8)
    if (load8(a + j) != load8(b + j)) return false;
  return j == len || load_tail(a + j, (int)(len - j)) == load_tail(b + j, (int)(len - j));
}

}  // namespace
