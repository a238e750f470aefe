// The progressive JPEG decoder's block routines (jpegdec.hip) as __host__ __device__ code, on top of the
// bit reader, tables and symbol decode of jpegdec_blocks.hpp: the scan record of a planned table and the four routines of
// T.81 G.1.2 / G.2 as libjpeg's jdphuff.c runs them.  The same text runs inside jpegprog_entropy_kernel and, under a
// sanitizer, in tests/jpegprog_host_main.cpp; tests/jpegprog_ref.py restates it.
//
// Bounds by construction: every stream read goes through JdBits with the unit's end, every coefficient index is a zigzag
// position checked against the scan's Se <= 63 before the store, and every loop is bounded by the band: at most 64
// symbols and 64 correction bits per block.  An EOB run (<= 32767) is only ever counted down by the caller, block by block.
//
// Hostile values are defined: DC is the low 16 bits of the wrapping 32-bit (predictor << Al); an AC value is the low 16
// bits of extend(v, s) << Al; a correction moves a coefficient by 1 << Al in 16-bit wrap-around arithmetic.
#pragma once
#include "jpegdec_blocks.hpp"

namespace attwarp {

enum { JP_DC_FIRST = 0, JP_DC_REFINE = 1, JP_AC_FIRST = 2, JP_AC_REFINE = 3 };

struct JpScan {                        // one scan of one image, in the table behind the sub-stream records
  uint32_t image;                      // its image among the call's
  uint32_t index;                      // its position among the image's scans, in file order (< ATTWARP_JPEGDEC_MAX_SCANS)
  uint32_t off;                        // its entropy data, relative to the image's packed data
  uint32_t kind;                       // JP_DC_FIRST .. JP_AC_REFINE
  uint32_t ss, se, al;                 // the band in zigzag positions (0, 0 for a DC scan), the point transform
  uint32_t nslot;                      // blocks per MCU; 1: not interleaved, the MCUs are the component's covered blocks
  uint32_t mcux, nmcu;                 // MCUs per row, MCUs
  uint32_t ri;                         // MCUs per unit (never 0: no restart interval = all of them)
  uint32_t nunits, unit0;              // planned units, the first of them among the call's scan units
  uint32_t level;                      // dependency level
  uint32_t wave0;                      // the first wave of its level's launch that belongs to it
  uint32_t last;                       // 1: the image's last scan (the marker behind it decides E_NO_EOI)
  uint8_t slot_c[8], slot_y[8], slot_x[8], slot_t[8];   // per block of an MCU: component, place inside the MCU, table
  uint8_t counts[3][16];               // the tables the scan names: one per component of a DC scan, [0] of an AC scan
  uint8_t symbols[3][256];
};
static_assert(sizeof(JpScan) % 8 == 0, "record layout");

JD_FN int16_t jp_low16(uint32_t v) { return (int16_t)(uint16_t)(v & 0xffffu); }

// DC, first pass: symbol, value, pred += diff -> the coefficient
JD_FN uint32_t jp_dc_first(JdBits& br, const JdHuff& dc, int32_t& pred, uint32_t al, int16_t& coef0) {
  uint32_t s, v;
  if (const uint32_t st = jd_symbol(br, dc, s)) return st;
  s &= 15u;
  if (!br.bits(s, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
  pred = (int32_t)((uint32_t)pred + (uint32_t)jd_extend(v, s));
  coef0 = jp_low16((uint32_t)pred << al);
  return 0;
}

// DC, refinement: one bit
JD_FN uint32_t jp_dc_refine(JdBits& br, uint32_t al, int16_t& coef0) {
  uint32_t v;
  if (!br.bits(1, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
  if (v) coef0 = jp_low16((uint32_t)(uint16_t)coef0 | (1u << al));
  return 0;
}

// AC, first pass, of a block whose EOB run is 0 on entry (the caller skips the blocks of a run without calling).  blk:
// natural order; only positions zz[ss..se] are written.  eobrun: on return, the blocks BEHIND this one that the run covers.
JD_FN uint32_t jp_ac_first(JdBits& br, const JdHuff& ac, uint32_t ss, uint32_t se, uint32_t al, uint32_t& eobrun, int16_t* blk,
                           const uint8_t* zz) {
  uint32_t k = ss, rs, v;
  for (int it = 0; it < 64 && k <= se; ++it) {
    if (const uint32_t st = jd_symbol(br, ac, rs)) return st;
    const uint32_t r = rs >> 4, s = rs & 15u;
    if (s == 0) {
      if (r == 15u) {
        if (k + 16u > se + 1u) return ATTWARP_JPEGDEC_E_COEFF;
        k += 16u;
        continue;
      }
      if (!br.bits(r, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
      eobrun = (1u << r) + v - 1u;
      return 0;
    }
    k += r;
    if (k > se) return ATTWARP_JPEGDEC_E_COEFF;
    if (!br.bits(s, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
    blk[zz[k] & 63u] = jp_low16((uint32_t)jd_extend(v, s) << al);
    ++k;
  }
  return 0;
}

// one correction bit for a coefficient with history
JD_FN uint32_t jp_correct(JdBits& br, uint32_t al, int16_t& c) {
  uint32_t v;
  if (!br.bits(1, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
  const uint32_t u = (uint16_t)c, p1 = 1u << al;
  if (v && !(u & p1)) c = jp_low16(c >= 0 ? u + p1 : u - p1);
  return 0;
}

// AC, refinement (decode_mcu_AC_refine).  eobrun: on entry the blocks the run still covers, this one included; on return
// the blocks behind this one.  A block inside a run still takes one correction bit per non-zero coefficient of the band.
JD_FN uint32_t jp_ac_refine(JdBits& br, const JdHuff& ac, uint32_t ss, uint32_t se, uint32_t al, uint32_t& eobrun, int16_t* blk,
                            const uint8_t* zz) {
  uint32_t k = ss, rs, v;
  if (eobrun == 0) {
    for (int it = 0; it < 64 && k <= se; ++it) {
      if (const uint32_t st = jd_symbol(br, ac, rs)) return st;
      int32_t r = (int32_t)(rs >> 4);
      const uint32_t s = rs & 15u;
      int16_t place = 0;
      if (s != 0) {
        if (s != 1u) return ATTWARP_JPEGDEC_E_COEFF;
        if (!br.bits(1, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
        place = jp_low16(v ? (1u << al) : 0u - (1u << al));
      } else if (r != 15) {
        if (!br.bits((uint32_t)r, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
        eobrun = (1u << r) + v;
        break;
      }
      // pass r zero-history coefficients, one correction bit for every coefficient with history on the way
      bool found = false;
      for (; k <= se; ++k) {
        int16_t& c = blk[zz[k] & 63u];
        if (c != 0) {
          if (const uint32_t st = jp_correct(br, al, c)) return st;
        } else if (--r < 0) {
          found = true;
          break;
        }
      }
      if (!found) return ATTWARP_JPEGDEC_E_COEFF;            // the run leaves the band
      if (s != 0) blk[zz[k] & 63u] = place;
      ++k;
    }
  }
  if (eobrun > 0) {
    for (; k <= se; ++k) {
      int16_t& c = blk[zz[k] & 63u];
      if (c != 0)
        if (const uint32_t st = jp_correct(br, al, c)) return st;
    }
    --eobrun;
  }
  return 0;
}

// The block of MCU m, slot j of a scan -> its index among the image's blocks.  An interleaved scan walks the frame's
// MCUs; a scan of one component walks the blocks that cover the component's TRUE size (mcux of them per row), which is
// not the padded row of bw blocks the coefficient memory is laid out in.
JD_FN uint32_t jp_block_index(const JdImage& im, const JpScan& sc, uint32_t m, uint32_t j) {
  const uint32_t mx = m % sc.mcux, my = m / sc.mcux;
  const int c = sc.slot_c[j & 7u] % 3;
  if (sc.nslot == 1u) return im.block0[c] + my * (uint32_t)im.bw[c] + mx;
  return jd_block_at(im.block0[c], (uint32_t)im.bw[c], c == 0 ? im.hs : 1, c == 0 ? im.vs : 1, mx, my, sc.slot_y[j & 7u], sc.slot_x[j & 7u]);
}

}  // namespace attwarp
