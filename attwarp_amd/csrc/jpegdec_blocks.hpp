// Pieces of the JPEG decoder (jpegdec.hip) as __host__ __device__ code: the table layouts, the canonical
// Huffman tables, the bit reader that un-stuffs FF 00, the decode of one block with its statuses, and the integer IDCT,
// chroma up-sampling and colour arithmetic of libjpeg as Pillow runs it.  The same text runs inside the kernels and, under
// a sanitizer, in tests/jpegdec_host_main.cpp; tests/jpegdec_ref.py restates it.
//
// Bounds by construction: every read of the stream goes through JdBits (checked against the unit's end), every
// coefficient index is checked against 63 before the store, every table index is masked, and every loop is bounded by a
// constant: 16 bits per code, 64 coefficients per block.
//
// Hostile values are defined, not trusted: the DC predictor is a 32-bit two's-complement sum that wraps, the coefficient
// stored is its low 16 bits, all IDCT arithmetic is 32-bit with wrap-around (unsigned in the text, so that nothing here
// is undefined behaviour), and the final clamp saturates.
#pragma once
#include "common.hpp"

namespace attwarp {

#if defined(__HIP_DEVICE_COMPILE__)
#define JD_FN __host__ __device__ __forceinline__
#else
#define JD_FN __host__ __device__ inline
#endif

constexpr int JD_LOOK_BITS = 8;

struct JdImage {                       // the per-image record of a planned table
  uint64_t stream_off;                 // entropy data (everything behind the SOS header) in the packed stream buffer
  uint64_t coef_off;                   // int16 coefficients in the scratch buffer (256-byte aligned)
  uint64_t plane_off;                  // uint8 component planes in the scratch buffer (256-byte aligned)
  uint64_t out_off;                    // pixels in the output buffer
  uint32_t stream_len;                 // below 2^31
  int32_t H, W, ncomp;
  int32_t hs, vs;                      // luma sampling factors (chroma is 1 x 1; grey: 1 x 1)
  int32_t oc, to_luma, swap;           // output channels; colour file to "L"; BGR
  int32_t mcux, mcuy, ri;              // MCUs per row / rows, MCUs per unit (never 0 here: no restart interval = all of them)
  int32_t nunits, unit0;               // planned units, and the first of them among the call's units
  int32_t idct_tile0, color_tile0;     // first workgroup of the IDCT / colour launch that belongs to this image
  int32_t bw[3], bh[3];                // blocks per row / block rows of each component's padded plane
  uint32_t block0[3];                  // first block of each component among the image's blocks
  uint32_t nblocks;
  uint16_t qt[3][64];                  // natural order
  uint8_t dc_counts[3][16], ac_counts[3][16];
  uint8_t dc_symbols[3][256], ac_symbols[3][256];
};
static_assert(sizeof(JdImage) % 8 == 0, "record layout");

struct JdState {                       // per image (scratch)
  uint32_t st_scan;                    // ATTWARP_JPEGDEC_E_RESTART or 0
  uint32_t eoi;                        // the first marker behind the data is EOI
  uint32_t fail;                       // min over failing units of (unit << 8 | status); 0xffffffff: none
  uint32_t nrst;                       // restart markers found in front of the data's end
};

struct JdHuff {                        // one canonical code, ready to decode
  uint16_t look[1 << JD_LOOK_BITS];    // by the next 8 bits: length << 8 | symbol; 0: a longer code or none
  int32_t maxcode[17];                 // largest code of each length, -1: none
  int32_t valoff[17];                  // index of a length's first symbol minus its first code
  uint8_t symbols[256];
};

// zigzag position -> natural position (the kernels decode through a copy in LDS)
constexpr uint8_t JD_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- tables: three steps, a barrier between them inside a kernel ------------------------------------------------------------------
// counts[16] is never over-subscribed and sums to nsym <= 256 (the planner checked it).
JD_FN void jd_huff_ranges(JdHuff& h, const uint8_t* counts) {              // one lane
  int32_t code = 0, k = 0;
  h.maxcode[0] = -1; h.valoff[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const int32_t c = counts[l - 1];
    h.valoff[l] = k - code;
    h.maxcode[l] = c ? code + c - 1 : -1;
    k += c;
    code = (code + c) << 1;
  }
}
JD_FN void jd_huff_clear(JdHuff& h, const uint8_t* symbols, int nsym, int lane, int nlanes) {
  for (int i = lane; i < (1 << JD_LOOK_BITS); i += nlanes) h.look[i] = 0;
  for (int i = lane; i < 256; i += nlanes) h.symbols[i] = i < nsym ? symbols[i] : (uint8_t)0;
}
JD_FN void jd_huff_fill(JdHuff& h, const uint8_t* counts, int lane, int nlanes) {
  // symbol k of length l <= 8 owns the 2^(8 - l) entries that start with its code
  for (int k = lane; k < 256; k += nlanes) {
    int first = 0, l = 0;
    for (int j = 1; j <= JD_LOOK_BITS; ++j) {
      const int c = counts[j - 1];
      if (l == 0 && k < first + c) l = j;
      if (l == 0) first += c;
    }
    if (l == 0) continue;
    const int32_t code = k - h.valoff[l];
    const int span = 1 << (JD_LOOK_BITS - l);
    const int at = (code << (JD_LOOK_BITS - l)) & ((1 << JD_LOOK_BITS) - 1);
    for (int e = 0; e < span; ++e) h.look[(at + e) & ((1 << JD_LOOK_BITS) - 1)] = (uint16_t)(l << 8 | h.symbols[k]);
  }
}
JD_FN int jd_nsym(const uint8_t* counts) {
  int n = 0;
  for (int l = 0; l < 16; ++l) n += counts[l];
  return n < 256 ? n : 256;
}

// ---- the bit reader: MSB first, FF 00 -> FF, never loads at or past `end` ------------------------------------------------------
// Byte `pos` of the unit's stream is p[pos & mask]: the host reads the stream itself (mask = all ones), a kernel reads a ring
// in LDS that the whole wave keeps filled ahead of the reader (mask = ring size - 1, ring aligned to pos).
struct JdBits {
  const uint8_t* p;
  uint32_t mask;
  uint32_t end, pos;                   // the unit is bytes pos .. end
  uint32_t cnt;                        // real bits in acc (the low cnt bits; the bits above are zero)
  uint64_t acc;
  uint32_t word, nword;                // up to four bytes loaded at once, lowest byte next
  JD_FN void init(const uint8_t* s, uint32_t m, uint32_t from, uint32_t to) {
    p = s; mask = m; pos = from < to ? from : to; end = to; cnt = 0; acc = 0; word = 0; nword = 0;
  }
  JD_FN bool next(uint32_t& b) {
    if (nword == 0) {
      if (pos >= end) return false;
      if ((pos & 3u) == 0 && end - pos >= 4u) {
#if defined(__HIP_DEVICE_COMPILE__)
        word = *reinterpret_cast<const uint32_t*>(p + (pos & mask));     // (the ring is dword aligned)
#else
        word = *reinterpret_cast<const u32_una*>(p + (pos & mask));
#endif
        nword = 4;
      } else {
        word = p[pos & mask];
        nword = 1;
      }
    }
    b = word & 255u;
    word >>= 8;
    --nword;
    ++pos;
    return true;
  }
  JD_FN void refill() {
    while (cnt <= 48) {
      uint32_t b, z;
      if (!next(b)) return;
      if (b == 0xffu) next(z);           // the stuffed 00 (inside a unit nothing else follows an FF: the scan ended it there)
      acc = acc << 8 | b;
      cnt += 8;
    }
  }
  // the next 16 bits, zeros behind the end
  JD_FN uint32_t peek16() const { return (uint32_t)(cnt >= 16 ? acc >> (cnt - 16) : acc << (16 - cnt)) & 0xffffu; }
  JD_FN void skip(uint32_t n) { cnt -= n; acc &= ((uint64_t)1 << cnt) - 1u; }      // n <= cnt <= 56
  JD_FN bool bits(uint32_t n, uint32_t& v) {                                         // n <= 16
    refill();
    if (n > cnt) return false;
    v = (uint32_t)(acc >> (cnt - n)) & ((1u << n) - 1u);
    skip(n);
    return true;
  }
};

// one symbol -> status
JD_FN uint32_t jd_symbol(JdBits& br, const JdHuff& h, uint32_t& sym) {
  br.refill();
  const uint32_t c = br.peek16();
  const uint32_t e = h.look[c >> (16 - JD_LOOK_BITS)];
  uint32_t len = e >> 8;
  sym = e & 255u;
  if (len == 0) {
    for (uint32_t l = JD_LOOK_BITS + 1; l <= 16; ++l) {
      const int32_t code = (int32_t)(c >> (16 - l));
      if (code <= h.maxcode[l]) {
        len = l;
        sym = h.symbols[(uint32_t)(h.valoff[l] + code) & 255u];
        break;
      }
    }
    if (len == 0) return br.cnt < 16 ? (uint32_t)ATTWARP_JPEGDEC_E_TRUNCATED : (uint32_t)ATTWARP_JPEGDEC_E_HUFFMAN;
  }
  if (len > br.cnt) return ATTWARP_JPEGDEC_E_TRUNCATED;
  br.skip(len);
  return 0;
}

JD_FN int32_t jd_extend(uint32_t v, uint32_t s) {
  return s == 0 || v >= (1u << (s - 1)) ? (int32_t)v : (int32_t)v - (int32_t)(1u << s) + 1;
}

// One block into blk[64] (natural order, zero on entry) -> status.  pred: the component's DC predictor; zz: JD_ZIGZAG or a copy.
JD_FN uint32_t jd_decode_block(JdBits& br, const JdHuff& dc, const JdHuff& ac, int32_t& pred, int16_t* blk, const uint8_t* zz) {
  uint32_t s, v, rs;
  if (const uint32_t st = jd_symbol(br, dc, s)) return st;
  s &= 15u;
  if (!br.bits(s, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
  pred = (int32_t)((uint32_t)pred + (uint32_t)jd_extend(v, s));
  blk[0] = (int16_t)(uint16_t)((uint32_t)pred & 0xffffu);
  uint32_t k = 1;
  for (int it = 0; it < 63 && k < 64; ++it) {
    if (const uint32_t st = jd_symbol(br, ac, rs)) return st;
    const uint32_t r = rs >> 4;
    s = rs & 15u;
    if (s == 0) {
      if (r != 15) break;
      if (k + 16 > 64) return ATTWARP_JPEGDEC_E_COEFF;
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return ATTWARP_JPEGDEC_E_COEFF;
    if (!br.bits(s, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
    blk[zz[k] & 63u] = (int16_t)jd_extend(v, s);
    ++k;
  }
  return 0;
}

// block (yy, xx) of a component (first block block0, bw blocks per row, h x v blocks per MCU) inside MCU (mx, my)
JD_FN uint32_t jd_block_at(uint32_t block0, uint32_t bw, int h, int v, uint32_t mx, uint32_t my, int yy, int xx) {
  return block0 + (my * (uint32_t)v + (uint32_t)yy) * bw + mx * (uint32_t)h + (uint32_t)xx;
}
// the same by component and MCU number -> its index among the image's blocks
JD_FN uint32_t jd_block_index(const JdImage& im, int c, uint32_t m, int yy, int xx) {
  const uint32_t mx = m % (uint32_t)im.mcux, my = m / (uint32_t)im.mcux;
  return jd_block_at(im.block0[c], (uint32_t)im.bw[c], c == 0 ? im.hs : 1, c == 0 ? im.vs : 1, mx, my, yy, xx);
}

// ---- the integer IDCT of jidctint.c (CONST_BITS 13, PASS1_BITS 2), 32-bit wrap-around arithmetic ---------------------------------
JD_FN int32_t jd_sra(uint32_t x, int n) { return (int32_t)x >> n; }
JD_FN void jd_idct_1d(const uint32_t i[8], int shift, int32_t o[8]) {
  uint32_t z1 = (i[2] + i[6]) * 4433u;
  const uint32_t t2 = z1 - i[6] * 15137u, t3 = z1 + i[2] * 6270u;
  const uint32_t t0 = (i[0] + i[4]) * 8192u, t1 = (i[0] - i[4]) * 8192u;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a = i[7], b = i[5], c = i[3], d = i[1];
  const uint32_t z5 = (a + c + b + d) * 9633u;
  z1 = (a + d) * (uint32_t)-7373;
  const uint32_t z2 = (b + c) * (uint32_t)-20995;
  const uint32_t z3 = (a + c) * (uint32_t)-16069 + z5, z4 = (b + d) * (uint32_t)-3196 + z5;
  a = a * 2446u + z1 + z3;
  b = b * 16819u + z2 + z4;
  c = c * 25172u + z2 + z3;
  d = d * 12299u + z1 + z4;
  const uint32_t rnd = 1u << (shift - 1);
  o[0] = jd_sra(t10 + d + rnd, shift); o[7] = jd_sra(t10 - d + rnd, shift);
  o[1] = jd_sra(t11 + c + rnd, shift); o[6] = jd_sra(t11 - c + rnd, shift);
  o[2] = jd_sra(t12 + b + rnd, shift); o[5] = jd_sra(t12 - b + rnd, shift);
  o[3] = jd_sra(t13 + a + rnd, shift); o[4] = jd_sra(t13 - a + rnd, shift);
}
JD_FN uint32_t jd_clamp8(int32_t v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// ---- chroma up-sampling ("fancy", jdsample.c) and colour (jdcolor.c) -----------------------------------------------------------
// p: the plane (pitch bytes per row), dw x dh its true size; (x, y) an output pixel.
JD_FN int32_t jd_chroma(const uint8_t* p, int pitch, int dw, int dh, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(size_t)y * pitch + x];
  const int i = x >> 1;
  const int in = (x & 1) ? (i + 1 < dw ? i + 1 : i) : (i > 0 ? i - 1 : 0);
  if (vs == 1) {
    const uint8_t* row = p + (size_t)y * pitch;
    if (x == 0 || x == 2 * dw - 1) return row[i];
    return (3 * row[i] + row[in] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int r = y >> 1;
  const int rn = (y & 1) ? (r + 1 < dh ? r + 1 : r) : (r > 0 ? r - 1 : 0);
  const uint8_t *r0 = p + (size_t)r * pitch, *r1 = p + (size_t)rn * pitch;
  const int32_t s = 3 * r0[i] + r1[i], sn = 3 * r0[in] + r1[in];
  return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;            // (at an edge sn = s: 4 s + 8 / 4 s + 7)
}
JD_FN void jd_ycc_to_rgb(int32_t y, int32_t cb, int32_t cr, uint32_t& r, uint32_t& g, uint32_t& b) {
  cb -= 128; cr -= 128;
  r = jd_clamp8(y + ((91881 * cr + 32768) >> 16));
  g = jd_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  b = jd_clamp8(y + ((116130 * cb + 32768) >> 16));
}
JD_FN uint32_t jd_luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

}  // namespace attwarp
