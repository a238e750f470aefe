// Pieces of the PNG encoder (png.hip) shared by its kernels and its host planner: the table layouts, CRC-32 arithmetic
// in the reflected representation, the PNG filters and deflate's length symbols.  Restated by tests/png_ref.py.
#pragma once
#include "common.hpp"

namespace attwarp {

constexpr int PNG_NT = 256;                              // threads per workgroup of every kernel
constexpr int PNG_SEG = ATTWARP_PNG_SEG_BYTES;           // filtered bytes per segment at most
constexpr int PNG_CH = PNG_SEG / PNG_NT;                 // bytes of a segment one thread tokenises (96)
constexpr int PNG_CHW = PNG_CH / 4;                      // ... in dwords (24)
constexpr int PNG_FILT_WORDS = PNG_NT * (PNG_CHW + 1);   // the segment in LDS: one pad dword per chunk, so the 64 lanes of
                                                         //   a wave walking their chunks hit 64 different banks (stride 25)
constexpr int PNG_OUT_WORDS = PNG_SEG / 4 + 8;           // the segment's deflate bytes (<= PNG_SEG + 5) and one spill word
constexpr int PNG_SYMS = 286, PNG_SYMS_PAD = 288;
constexpr uint32_t PNG_HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 287 * 4;
constexpr uint32_t PNG_POLY = 0xEDB88320u;
constexpr uint32_t PNG_ADLER = 65521u;
constexpr int PNG_FILE_HEAD = 8 + 25 + 8 + 2;            // signature, IHDR, IDAT length + type, zlib header
constexpr int PNG_FILE_TAIL = 5 + 4 + 4 + 12;            // final stored block, Adler-32, IDAT CRC, IEND
static_assert(PNG_FILE_HEAD + PNG_FILE_TAIL == ATTWARP_PNG_FILE_OVERHEAD, "file overhead");
static_assert(PNG_CH * PNG_NT == PNG_SEG && PNG_CH % 4 == 0 && (PNG_CHW + 1) % 2 == 1, "chunk layout");
static_assert(ATTWARP_PNG_MAX_ROW_BYTES <= PNG_SEG, "a row must fit a segment");

struct PngImage {                      // == attwarp_png_image
  const uint8_t* src;
  int32_t H, W, C, pitch, order, filter;
};
static_assert(sizeof(PngImage) == sizeof(attwarp_png_image), "descriptor layout");

struct PngImageDev {                   // the per-image record of a planned table
  const uint8_t* src;
  int32_t H, W, C, pitch, swap, filter;
  int32_t seg0, nseg, rows_per_seg, row_bytes;
  uint8_t ihdr[25];                    // the whole IHDR chunk: length, type, 13 bytes, CRC
  uint8_t pad[7];
};
static_assert(sizeof(PngImageDev) == 80, "record layout");

struct PngSeg {                        // one work item of the encode kernel
  int32_t image, row0, nrows, n;       // n: filtered bytes (nrows * row_bytes)
  uint64_t scratch_off;                // where its deflate bytes go in the scratch buffer (16-byte aligned)
  uint64_t after;                      // filtered bytes of the image behind this segment
};
static_assert(sizeof(PngSeg) == 32, "record layout");

struct PngSegOut {                     // what the encode kernel leaves per segment at the start of the scratch buffer
  uint32_t len, crc, s1, s2;           // deflate bytes, their CRC-32, the Adler partial sums of the filtered bytes
  uint32_t pre, pad;                   // (assemble kernel) deflate bytes of the image's earlier segments
};

// ---- CRC-32, reflected: bit 31 is x^0 ------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 4
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? PNG_POLY : 0u);
  }
  return p;
}
// x^(8 n) from the table pow8[k] = x^(8 * 2^k)
template <typename P>
__host__ __device__ inline uint32_t crc_xpow8(uint32_t n, const P* pow8) {
  uint32_t p = 0x80000000u;
  for (int k = 0; k < 32; ++k)
    if ((n >> k) & 1u) p = crc_mulmod(p, pow8[k]);
  return p;
}
__host__ __device__ inline uint32_t crc_table_entry(uint32_t n) {
  for (int k = 0; k < 8; ++k) n = (n >> 1) ^ ((n & 1u) ? PNG_POLY : 0u);
  return n;
}
// plain bitwise CRC-32 (host planner, and the nine trailer bytes on the device)
__host__ __device__ inline uint32_t crc_bytes(const uint8_t* p, int n, uint32_t crc = 0) {
  uint32_t c = ~crc;
  for (int i = 0; i < n; ++i) c = crc_table_entry((c ^ p[i]) & 255u) ^ (c >> 8);
  return ~c;
}

// ---- PNG filters ---------------------------------------------------------------------------------------------------------
// cur - predictor(a = left, b = up, c = upper left), modulo 256
__host__ __device__ inline uint32_t png_filter(int ft, int cur, int a, int b, int c) {
  int pred = 0;
  if (ft == 1) pred = a;
  else if (ft == 2) pred = b;
  else if (ft == 3) pred = (a + b) >> 1;
  else if (ft == 4) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return (uint32_t)(cur - pred) & 255u;
}

// ---- deflate: match length 3 .. 258 -> symbol 257 .. 285, extra bits and their value ------------------------------------------
__host__ __device__ inline void png_length_symbol(uint32_t L, uint32_t& sym, uint32_t& eb, uint32_t& ev) {
  const uint32_t m = L - 3;
  if (L == 258) { sym = 285; eb = 0; ev = 0; }
  else if (m < 8) { sym = 257 + m; eb = 0; ev = 0; }
  else {
    const uint32_t e = 29u - (uint32_t)__builtin_clz(m);       // floor(log2 m) - 2
    sym = 261 + 4 * e + ((m >> e) & 3u);
    eb = e;
    ev = m & ((1u << e) - 1u);
  }
}

__host__ __device__ inline int png_rows_per_segment(int row_bytes) {
  const int r = PNG_SEG / row_bytes;
  return r < 1 ? 1 : (r > ATTWARP_PNG_SEG_MAX_ROWS ? ATTWARP_PNG_SEG_MAX_ROWS : r);
}

}  // namespace attwarp
