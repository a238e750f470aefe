// The JPEG decoder's SCANS-OF-ANY-LAYOUT family (jpegdec.hip, attwarp_jpegdec_plan_layout_scans) as __host__
// __device__ code: the scan record of a planned table over JfImage frames (jpegfmt_blocks.hpp: up to four components of any
// sampling), where a block of a scan lies in its component's padded plane, and the serial walk of one unit of one scan
// with the five block routines: the four of jpegprog_blocks.hpp and the sequential block of jpegdec_blocks.hpp.  The same
// text runs inside jpegscan_entropy_kernel and, under a sanitizer, in tests/jpegscan_host_main.cpp; tests/jpegscan_ref.py
// restates it.
//
// Bounds by construction: a slot index is clamped below JF_MAX_SLOTS, a component and a table index masked to 0..3 (the kernel
// also holds the table index below the tables its launch built), every
// block index is held against the image's nblocks before a load or store, every stream read goes through JdBits with
// the unit's end, and the band is clamped to 0..63.
#pragma once
#include "jpegfmt_blocks.hpp"
#include "jpegprog_blocks.hpp"

namespace attwarp {

constexpr uint32_t JS_SEQUENTIAL = 4;  // the fifth kind of a scan, behind JP_DC_FIRST .. JP_AC_REFINE: band 0..63, DC and AC in one pass

struct JsScan {                        // one scan of one image, in the table behind the layout family's records
  uint32_t image;                      // its image among the call's
  uint32_t index;                      // its position among the image's scans, in file order (< ATTWARP_JPEGDEC_MAX_SCANS)
  uint32_t off;                        // its entropy data, relative to the image's packed data
  uint32_t kind;                       // JP_DC_FIRST .. JP_AC_REFINE, JS_SEQUENTIAL
  uint32_t ss, se, al;                 // the band in zigzag positions, the point transform
  uint32_t nslot;                      // blocks per MCU of THIS scan; 1 with ncomp 1: not interleaved
  uint32_t mcux, nmcu;                 // MCUs per row, MCUs: the frame's, or the blocks that cover the one component's true size
  uint32_t ri;                         // MCUs per unit (never 0)
  uint32_t nunits, unit0;              // planned units, the first of them among the call's scan units
  uint32_t level, wave0;               // dependency level, the first wave of its level's launch that belongs to it
  uint32_t last;                       // 1: the image's last scan (the marker behind it decides E_NO_EOI)
  uint32_t ncomp, reserved;            // components of the scan
  uint8_t slot_c[12], slot_y[12], slot_x[12], slot_t[12];   // per block of an MCU: component, place inside the MCU, table
  uint8_t dc_counts[JF_MAX_COMP][16], ac_counts[JF_MAX_COMP][16];       // by the component's place in the scan; [0] of an AC scan
  uint8_t dc_symbols[JF_MAX_COMP][256], ac_symbols[JF_MAX_COMP][256];
};
static_assert(sizeof(JsScan) % 8 == 0, "record layout");

JD_FN uint32_t js_nslot(const JsScan& sc) { return sc.nslot >= 1u && sc.nslot <= (uint32_t)JF_MAX_SLOTS ? sc.nslot : 1u; }

// The block of MCU m, slot j of a scan -> its index among the image's blocks.  An interleaved scan walks the FRAME's MCUs,
// also when it holds a subset of the components; a scan of one component walks the blocks that cover the component's true
// size (sc.mcux of them per row), at the pitch of its padded plane.
JD_FN uint32_t js_block_index(const JfImage& im, const JsScan& sc, uint32_t m, uint32_t j) {
  const uint32_t mcux = sc.mcux ? sc.mcux : 1u, mx = m % mcux, my = m / mcux;
  const uint32_t s = j < (uint32_t)JF_MAX_SLOTS ? j : 0u;
  const JfComp& k = im.comp[sc.slot_c[s] & 3u];
  if (sc.ncomp <= 1u) return k.block0 + my * (uint32_t)k.bw + mx;
  return jd_block_at(k.block0, (uint32_t)k.bw, k.h, k.v, mx, my, sc.slot_y[s], sc.slot_x[s]);
}

// One block of a scan of `kind` decoded into blk[64] (natural order; its history on entry for a refinement, zero for a
// first pass) -> status.  dc / ac: the scan's tables by the component's place t in it; pred: the scan's predictors; eobrun as
// the routines of jpegprog_blocks.hpp define it.
JD_FN uint32_t js_decode_block(JdBits& br, uint32_t kind, const JdHuff* dc, const JdHuff* ac, uint32_t t, int32_t* pred, uint32_t ss,
                               uint32_t se, uint32_t al, uint32_t& eobrun, int16_t* blk, const uint8_t* zz) {
  t &= 3u;
  if (kind == JS_SEQUENTIAL) return jd_decode_block(br, dc[t], ac[t], pred[t], blk, zz);
  if (kind == JP_DC_FIRST) return jp_dc_first(br, dc[t], pred[t], al, blk[0]);
  if (kind == JP_DC_REFINE) return jp_dc_refine(br, al, blk[0]);
  if (kind == JP_AC_FIRST) return jp_ac_first(br, ac[0], ss, se, al, eobrun, blk, zz);
  return jp_ac_refine(br, ac[0], ss, se, al, eobrun, blk, zz);
}

// Unit k of a scan decoded serially from br into coef (the image's blocks, 64 int16 each): the walk of the entropy kernel
// as host code, the band rule included -> status.
JD_FN uint32_t js_decode_unit(JdBits& br, const JfImage& im, const JsScan& sc, const JdHuff* dc, const JdHuff* ac, uint32_t k, int16_t* coef) {
  const uint32_t nslot = js_nslot(sc), kind = sc.kind, ss = sc.ss < 63u ? sc.ss : 63u, se = sc.se < 63u ? sc.se : 63u, al = sc.al < 15u ? sc.al : 15u;
  const uint32_t m0 = k * sc.ri, m1 = m0 + sc.ri < sc.nmcu ? m0 + sc.ri : sc.nmcu, iend = m1 * nslot;
  int32_t pred[JF_MAX_COMP] = {0, 0, 0, 0};
  uint32_t eobrun = 0;
  for (uint32_t i = m0 * nslot; i < iend;) {
    const uint32_t m = i / nslot, j = i - m * nslot;
    const uint32_t bi = js_block_index(im, sc, m, j);
    int16_t blk[64];
    __builtin_memset(blk, 0, sizeof blk);
    if (bi < im.nblocks && (kind == JP_AC_REFINE || kind == JP_DC_REFINE)) __builtin_memcpy(blk, coef + (size_t)bi * 64u, sizeof blk);
    if (const uint32_t st = js_decode_block(br, kind, dc, ac, sc.slot_t[j < 12u ? j : 0u], pred, ss, se, al, eobrun, blk, JD_ZIGZAG)) return st;
    if (bi < im.nblocks) {
      const uint32_t lo = kind == JS_SEQUENTIAL ? 0u : kind <= JP_DC_REFINE ? 0u : ss, hi = kind == JS_SEQUENTIAL ? 63u : kind <= JP_DC_REFINE ? 0u : se;
      for (uint32_t z = lo; z <= hi; ++z) coef[(size_t)bi * 64u + JD_ZIGZAG[z]] = blk[JD_ZIGZAG[z]];
    }
    uint32_t adv = 1;
    if (kind == JP_AC_FIRST && eobrun > 0) {                 // the blocks of the run are skipped without touching memory
      const uint32_t skip = eobrun < iend - i - 1u ? eobrun : iend - i - 1u;
      adv += skip;
      eobrun -= skip;
    }
    i += adv;
  }
  return 0;
}

}  // namespace attwarp
