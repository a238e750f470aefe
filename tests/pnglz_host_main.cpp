// Host-only check of the host / device pieces of the PNG encoder's match = LZ route (attwarp_amd/csrc/png_lz_blocks.hpp) for
// tests/test_pnglz_host_cpu.py: the same text the kernel runs, compiled for the CPU with -fsanitize=address,undefined.
//   png_dist_symbol       every distance 1 .. 32768 against RFC 1951's table of bases and extra bits, written out here;
//   png_dist_extra / png_length_extra   the extra bits of every symbol against the two tables;
//   png_lz_hash           12 bits, and the value the restatement computes for a known key;
//   png_lz_token          every (distance, length, exit) round trip at the fields' limits;
//   png_lz_takes_far      the tie rule: a far match only when it is longer than the distance-1 run and at least 4 bytes.
// Prints one line and returns 0.
#include <cstdio>

#include "png_lz_blocks.hpp"

using namespace attwarp;

static int bad(const char* what, long a, long b, long c) {
  fprintf(stderr, "pnglz_host: %s at %ld %ld %ld\n", what, a, b, c);
  return 3;
}

// RFC 1951 3.2.5: distance codes 0 .. 29 and length codes 257 .. 285
static const int DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                  4097, 6145, 8193, 12289, 16385, 24577};
static const int DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const int LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};

int main() {
  long checked = 0;
  for (int d = 1; d <= 32768; ++d) {
    int k = 29;
    while (d < DIST_BASE[k]) --k;
    uint32_t sym, eb, ev;
    png_dist_symbol((uint32_t)d, sym, eb, ev);
    if ((int)sym != k || (int)eb != DIST_EXTRA[k] || (int)ev != d - DIST_BASE[k]) return bad("png_dist_symbol", d, sym, ev);
    if (ev >> eb) return bad("png_dist_symbol: value wider than its bits", d, eb, ev);
    ++checked;
  }
  for (int s = 0; s < 30; ++s)
    if ((int)png_dist_extra((uint32_t)s) != DIST_EXTRA[s]) return bad("png_dist_extra", s, 0, 0);
  for (int s = 0; s < 29; ++s) {
    if ((int)png_length_extra((uint32_t)s) != LEN_EXTRA[s]) return bad("png_length_extra", s, 0, 0);
    checked += 2;
  }
  // the hash: 12 bits; key 0x04030201 (bytes 1 2 3 4) gives (0x04030201 * 0x9E3779B1 mod 2^32) >> 20
  if (png_lz_hash(0x04030201u) != (uint32_t)((0x04030201ull * 0x9E3779B1ull & 0xffffffffull) >> 20)) return bad("png_lz_hash", 0, 0, 0);
  for (uint32_t k = 0; k < (1u << 20); ++k) {
    const uint32_t key = k * 2654435761u + 12345u;
    if (png_lz_hash(key) >> PNG_LZ_HASH_BITS) return bad("png_lz_hash: more than 12 bits", key, 0, 0);
    ++checked;
  }
  const uint32_t dists[] = {0, 1, 2, 255, 256, 24572, 24575, 32767}, lens[] = {3, 4, 130, 257, 258}, exits[] = {0, 1, 95, 256, 257, 511};
  for (uint32_t d : dists)
    for (uint32_t l : lens)
      for (uint32_t e : exits) {
        const uint32_t t = png_lz_token(d, d ? l : 1u, e);
        if (png_lz_token_dist(t) != d || png_lz_token_exit(t) != e || (d && png_lz_token_len(t) != l)) return bad("png_lz_token", d, l, e);
        ++checked;
      }
  for (uint32_t far = 0; far <= 258; ++far)
    for (uint32_t run = 0; run <= 258; ++run) {
      if (png_lz_takes_far(far, run) != (far >= 4 && far > run)) return bad("png_lz_takes_far", far, run, 0);
      ++checked;
    }
  static_assert(PNG_LZ_HEADER_BITS == 1338, "the LZ block's header");
  static_assert(PNG_LZ_TOKEN_BYTES + PNG_LZ_STATIC_LDS <= LDS_CU_BYTES, "the kernel's LDS fits a CU");
  printf("pnglz_host ok %ld\n", checked);
  return 0;
}
