// Pieces of the PNG encoder's second token route, match = ATTWARP_PNG_MATCH_LZ (png.hip), shared by its
// kernel, the host planner and the host test: the candidate hash, deflate's distance symbols and the per-position token
// word.  Restated by tests/pnglz_ref.py.
#pragma once
#include "png_blocks.hpp"

namespace attwarp {

constexpr int PNG_LZ_HASH_BITS = 12;                     // one head per hash value: 4096 words, kept where the output goes later
constexpr uint32_t PNG_LZ_HASH_MUL = 0x9E3779B1u;
constexpr int PNG_LZ_BLOCK = PNG_NT;                     // positions that look up their candidate together, then publish themselves
constexpr uint32_t PNG_LZ_FAR_MIN = 4;                   // a far match counts from the key's four bytes
constexpr uint32_t PNG_LZ_MAX_LEN = 258;
constexpr int PNG_DSYMS = 30;
constexpr uint32_t PNG_LZ_HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + (PNG_SYMS + PNG_DSYMS) * 4;
constexpr size_t PNG_LZ_TOKEN_BYTES = (size_t)(PNG_SEG + PNG_NT) * 4;   // dynamic LDS of the kernel: one token word per position, one pad word per chunk
constexpr size_t PNG_LZ_STATIC_LDS = 63464;              // the kernel's own __shared__ variables (kernel-resource-usage)
enum { PNG_ROUTE_RLE = 0, PNG_ROUTE_LZ = 1, PNG_ROUTE_STORED = 2 };
static_assert((1 << PNG_LZ_HASH_BITS) <= PNG_OUT_WORDS, "the heads must fit the output words");
static_assert(PNG_SEG < (1 << 15), "a distance must fit 15 bits");

// the four bytes at a position, little endian -> hash
__host__ __device__ inline uint32_t png_lz_hash(uint32_t key) { return (key * PNG_LZ_HASH_MUL) >> (32 - PNG_LZ_HASH_BITS); }

// ---- deflate: distance 1 .. 32768 -> symbol 0 .. 29, extra bits and their value -----------------------------------------------
__host__ __device__ inline void png_dist_symbol(uint32_t D, uint32_t& sym, uint32_t& eb, uint32_t& ev) {
  const uint32_t m = D - 1;
  if (m < 4) { sym = m; eb = 0; ev = 0; }
  else {
    const uint32_t e = 30u - (uint32_t)__builtin_clz(m);       // floor(log2 m) - 1
    sym = 2 * e + 2 + ((m >> e) & 1u);
    eb = e;
    ev = m & ((1u << e) - 1u);
  }
}
__host__ __device__ inline uint32_t png_dist_extra(uint32_t sym) { return sym < 4 ? 0u : (sym - 2u) / 2u; }
__host__ __device__ inline uint32_t png_length_extra(uint32_t ls) {      // ls = symbol - 257
  return (ls < 8u || ls == 28u) ? 0u : (ls - 4u) / 4u;
}

// ---- the token that starts at a position: distance (15 bits, 0: a literal), length - 3 (8 bits), and where the greedy chain
// that passes through this position first lands at or behind the end of the position's chunk, relative to that end (9 bits)
__host__ __device__ inline uint32_t png_lz_token(uint32_t dist, uint32_t len, uint32_t exit_rel) {
  return dist | (dist ? len - 3u : 0u) << 15 | exit_rel << 23;
}
__host__ __device__ inline uint32_t png_lz_token_dist(uint32_t t) { return t & 0x7fffu; }
__host__ __device__ inline uint32_t png_lz_token_len(uint32_t t) { return ((t >> 15) & 255u) + 3u; }
__host__ __device__ inline uint32_t png_lz_token_exit(uint32_t t) { return t >> 23; }

// far (length, distance) against the distance-1 run: the far match only when it is longer
__host__ __device__ inline bool png_lz_takes_far(uint32_t far, uint32_t run) { return far >= PNG_LZ_FAR_MIN && far > run; }

}  // namespace attwarp
