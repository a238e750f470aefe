// Pieces of the JPEG decoder's LAYOUT family (jpegdec.hip, attwarp_jpegdec_plan_layouts) as __host__
// __device__ code: the record of an image with up to four components of any sampling, the check of its factors and the
// block-slot map of its MCU, the general entropy walk, the up-sampler libjpeg picks per component, and the four colour
// rules with Pillow's mode conversions.  The block decode, the bit reader, the sub-stream walk and the IDCT are those of
// jpegdec_blocks.hpp.  The same text runs inside the kernels and, under a sanitizer, in tests/jpegfmt_host_main.cpp;
// tests/jpegfmt_ref.py restates it.
//
// Bounds by construction: jf_layout admits only factors 1..4 that divide the frame's largest and at most JF_MAX_SLOTS
// blocks per MCU, so every slot index is below JF_MAX_SLOTS, every component index below JF_MAX_COMP and every block of
// every slot lies inside its component's padded plane; a sample is read at (x / rx, y / ry) or a neighbour clamped to the
// component's true size.
#pragma once
#include "jpegdec_blocks.hpp"

namespace attwarp {

constexpr int JF_MAX_COMP = 4, JF_MAX_SLOTS = 10;
enum { JF_UP_COPY = 0, JF_UP_H2V1 = 1, JF_UP_H2V2 = 2, JF_UP_H1V2 = 3, JF_UP_BOX = 4 };   // the up-sampler of a component
enum { JF_CONV_KEEP = 0, JF_CONV_RGB = 1, JF_CONV_L = 2 };                               // Pillow's conversion behind the colour rule
enum { JF_OK = 0, JF_E_COMPONENTS, JF_E_FACTOR, JF_E_SLOTS, JF_E_FRACTION, JF_E_COLOR };

struct JfComp {
  int32_t h, v;                        // sampling factors
  int32_t bw, bh;                      // blocks per row / block rows of the padded plane
  uint32_t block0;                     // its first block among the image's blocks
  int32_t dw, dh;                      // true size: ceil(W h / hmax) x ceil(H v / vmax)
  int32_t up, rx, ry;                  // JF_UP_*, and hmax / h, vmax / v
};

struct JfImage {                       // the per-image record of a table of attwarp_jpegdec_plan_layouts
  uint64_t stream_off, coef_off, plane_off, out_off;     // as in JdImage
  uint32_t stream_len;
  int32_t H, W, ncomp;
  int32_t hmax, vmax;
  int32_t color;                       // ATTWARP_JPEGDEC_COLOR_*
  int32_t oc, conv, swap;              // output channels; JF_CONV_*; BGR
  int32_t mcux, mcuy, ri;
  int32_t nunits, unit0;
  int32_t idct_tile0, color_tile0;
  int32_t nslot;                       // blocks per MCU, 1..JF_MAX_SLOTS
  uint32_t nblocks;
  int32_t period, reserved;            // the slots a decoder's state can tell apart by their tables (jf_period), a divisor of nslot
  uint8_t slot_c[12], slot_x[12], slot_y[12];            // block slot of the MCU -> component, block column and row inside the MCU
  JfComp comp[JF_MAX_COMP];
  uint16_t qt[JF_MAX_COMP][64];        // natural order
  uint8_t dc_counts[JF_MAX_COMP][16], ac_counts[JF_MAX_COMP][16];
  uint8_t dc_symbols[JF_MAX_COMP][256], ac_symbols[JF_MAX_COMP][256];
};
static_assert(sizeof(JfImage) == 3000, "record layout (JPEGDEC_LAYOUT_RECORD_BYTES of _lib.py)");

struct JfSegState {                    // per segment (scratch): JdSegState with four predictors
  JdSync entry;
  uint32_t dirty, before;
  uint32_t pred[JF_MAX_COMP];
};
static_assert(sizeof(JfSegState) == 32, "segment layout");
struct JfSegment {                     // JdSegment with the DC sums by the owned block's place in the segment, mod the MCU's blocks
  JdSync exit;
  uint32_t owned, nend, eclean, pad;
  uint32_t dc[JF_MAX_SLOTS];
};
static_assert(sizeof(JfSegment) == 64, "segment layout");

// The geometry of an image from its size and factors -> JF_OK or what is refused; nothing is written on a refusal.  A
// one-component image is not interleaved: its factors do not count (libjpeg ignores them) and become 1 x 1.
JD_FN int jf_layout(JfImage& im, int W, int H, int ncomp, const int32_t* h, const int32_t* v, int color) {
  if (ncomp != 1 && ncomp != 3 && ncomp != 4) return JF_E_COMPONENTS;
  if (color < ATTWARP_JPEGDEC_COLOR_GREY || color > ATTWARP_JPEGDEC_COLOR_YCCK) return JF_E_COLOR;
  if ((color == ATTWARP_JPEGDEC_COLOR_GREY) != (ncomp == 1) || (color >= ATTWARP_JPEGDEC_COLOR_CMYK) != (ncomp == 4)) return JF_E_COLOR;
  int hh[JF_MAX_COMP], vv[JF_MAX_COMP], hmax = 1, vmax = 1, slots = 0;
  for (int c = 0; c < ncomp; ++c) {
    if (h[c] < 1 || h[c] > 4 || v[c] < 1 || v[c] > 4) return JF_E_FACTOR;
    hh[c] = ncomp == 1 ? 1 : h[c];
    vv[c] = ncomp == 1 ? 1 : v[c];
    hmax = hh[c] > hmax ? hh[c] : hmax;
    vmax = vv[c] > vmax ? vv[c] : vmax;
    slots += hh[c] * vv[c];
  }
  if (slots > JF_MAX_SLOTS) return JF_E_SLOTS;
  for (int c = 0; c < ncomp; ++c)
    if (hmax % hh[c] != 0 || vmax % vv[c] != 0) return JF_E_FRACTION;
  im.W = W; im.H = H; im.ncomp = ncomp; im.hmax = hmax; im.vmax = vmax; im.color = color;
  im.mcux = (W + 8 * hmax - 1) / (8 * hmax);
  im.mcuy = (H + 8 * vmax - 1) / (8 * vmax);
  im.nslot = 0;
  uint32_t blocks = 0;
  for (int c = 0; c < JF_MAX_COMP; ++c) {
    JfComp& k = im.comp[c];
    if (c >= ncomp) { k = JfComp{1, 1, 0, 0, blocks, 0, 0, JF_UP_COPY, 1, 1}; continue; }
    k.h = hh[c]; k.v = vv[c];
    k.bw = im.mcux * k.h; k.bh = im.mcuy * k.v;
    k.block0 = blocks;
    blocks += (uint32_t)k.bw * (uint32_t)k.bh;             // (the caller bounds mcux x mcuy: jf_blocks)
    k.dw = (W * k.h + hmax - 1) / hmax;
    k.dh = (H * k.v + vmax - 1) / vmax;
    k.rx = hmax / k.h; k.ry = vmax / k.v;
    // jinit_upsampler of jdsample.c with fancy up-sampling on: the triangle filters of 2 x 1 and 2 x 2 only for a
    // component wider than two samples, the vertical one of 1 x 2 always, box replication for every other ratio
    k.up = k.rx == 1 && k.ry == 1 ? JF_UP_COPY
         : k.rx == 2 && k.ry == 1 && k.dw > 2 ? JF_UP_H2V1
         : k.rx == 2 && k.ry == 2 && k.dw > 2 ? JF_UP_H2V2
         : k.rx == 1 && k.ry == 2 ? JF_UP_H1V2 : JF_UP_BOX;
    for (int y = 0; y < k.v; ++y)
      for (int x = 0; x < k.h; ++x) {
        im.slot_c[im.nslot] = (uint8_t)c; im.slot_x[im.nslot] = (uint8_t)x; im.slot_y[im.nslot] = (uint8_t)y;
        ++im.nslot;
      }
  }
  im.nblocks = blocks;
  return JF_OK;
}
// blocks of an image of these factors, in 64 bits: what the planner holds against ATTWARP_JPEGDEC_MAX_BLOCKS BEFORE jf_layout
JD_FN uint64_t jf_blocks(int W, int H, int ncomp, const int32_t* h, const int32_t* v) {
  int hmax = 1, vmax = 1, slots = 0;
  for (int c = 0; c < ncomp && c < JF_MAX_COMP; ++c) {
    const int hc = ncomp == 1 ? 1 : h[c], vc = ncomp == 1 ? 1 : v[c];
    hmax = hc > hmax ? hc : hmax; vmax = vc > vmax ? vc : vmax;
    slots += hc * vc;
  }
  return (uint64_t)((W + 8 * hmax - 1) / (8 * hmax)) * (uint64_t)((H + 8 * vmax - 1) / (8 * vmax)) * (uint64_t)slots;
}

// the index among the image's blocks of block slot `slot` of MCU (mx, my)
JD_FN uint32_t jf_slot_block(const JfImage& im, uint32_t slot, uint32_t mx, uint32_t my) {
  const uint32_t s = slot < (uint32_t)JF_MAX_SLOTS ? slot : 0u;
  const JfComp& k = im.comp[im.slot_c[s] & 3u];
  return jd_block_at(k.block0, (uint32_t)k.bw, k.h, k.v, mx, my, im.slot_y[s], im.slot_x[s]);
}

// The general MCU as a layout of jd_decode_segment_of / jd_write_segment_of.  Components that share their Huffman tables
// (all four of a CMYK file libjpeg wrote) make slots no decoder can tell apart: a decoder in step with the bits but off by
// some slots would never fall in step with the truth, and the true state would travel one segment per round.  So a state
// carries the slot only modulo the PERIOD of the slots' table sequence, a segment sums its DC differences by the owned
// block's place in the segment, and both the true slot of every block and its component follow from the count of blocks in
// front of the segment, as the block's index already does.
struct JfLayout {
  static constexpr int NC = JF_MAX_COMP, NDC = JF_MAX_SLOTS;
  const JfImage& im;
  JD_FN uint32_t period(uint32_t nblk) const { return im.period >= 1 && (uint32_t)im.period <= nblk ? (uint32_t)im.period : nblk; }
  JD_FN uint32_t dc_slot(uint32_t, uint32_t owned, uint32_t nblk) const { return owned % nblk; }
  JD_FN uint32_t comp(uint32_t slot) const { return im.slot_c[slot < (uint32_t)JF_MAX_SLOTS ? slot : 0u] & 3u; }
  JD_FN uint32_t block(uint32_t m, uint32_t slot) const { return jf_slot_block(im, slot, m % (uint32_t)im.mcux, m / (uint32_t)im.mcux); }
  JD_FN uint32_t nblocks() const { return im.nblocks; }
};

// The period of the MCU's table sequence: the smallest divisor P of nslot with equal Huffman tables (counts, and symbols as
// far as the counts go) in slots j and j + P for every j.  Needs the record's slot map and tables.
JD_FN bool jf_same_tables(const JfImage& im, uint32_t a, uint32_t b) {
  if (a == b) return true;
  for (int l = 0; l < 16; ++l)
    if (im.dc_counts[a][l] != im.dc_counts[b][l] || im.ac_counts[a][l] != im.ac_counts[b][l]) return false;
  const int nd = jd_nsym(im.dc_counts[a]), na = jd_nsym(im.ac_counts[a]);
  for (int k = 0; k < nd; ++k)
    if (im.dc_symbols[a][k] != im.dc_symbols[b][k]) return false;
  for (int k = 0; k < na; ++k)
    if (im.ac_symbols[a][k] != im.ac_symbols[b][k]) return false;
  return true;
}
JD_FN int jf_period(const JfImage& im) {
  const int n = im.nslot >= 1 && im.nslot <= JF_MAX_SLOTS ? im.nslot : 1;
  for (int P = 1; P < n; ++P) {
    if (n % P) continue;
    bool same = true;
    for (int j = 0; j + P < n && same; ++j) same = jf_same_tables(im, im.slot_c[j] & 3u, im.slot_c[j + P] & 3u);
    if (same) return P;
  }
  return n;
}

// One unit (MCUs m0 .. m1) decoded serially from br into coef: the walk of the entropy kernel as host code -> status.
JD_FN uint32_t jf_decode_unit(JdBits& br, const JfImage& im, const JdHuff* dc, const JdHuff* ac, uint32_t m0, uint32_t m1, int16_t* coef) {
  int32_t pred[JF_MAX_COMP] = {0, 0, 0, 0};
  for (uint32_t m = m0; m < m1; ++m) {
    const uint32_t mx = m % (uint32_t)im.mcux, my = m / (uint32_t)im.mcux;
    for (uint32_t j = 0; j < (uint32_t)im.nslot && j < (uint32_t)JF_MAX_SLOTS; ++j) {
      const uint32_t c = im.slot_c[j] & 3u;
      int16_t blk[64];
      __builtin_memset(blk, 0, sizeof blk);
      if (const uint32_t st = jd_decode_block(br, dc[c], ac[c], pred[c], blk, JD_ZIGZAG)) return st;
      const uint32_t bi = jf_slot_block(im, j, mx, my);
      if (bi < im.nblocks) __builtin_memcpy(coef + (size_t)bi * 64u, blk, sizeof blk);
    }
  }
  return 0;
}

// ---- up-sampling: the sample of component k at output pixel (x, y).  p: its plane, pitch bytes per row ----------------------------
JD_FN int32_t jf_sample(const uint8_t* p, int pitch, const JfComp& k, int x, int y) {
  if (k.up == JF_UP_COPY) return p[(size_t)y * pitch + x];
  if (k.up == JF_UP_H2V1 || k.up == JF_UP_H2V2) return jd_chroma(p, pitch, k.dw, k.dh, 2, k.ry, x, y);
  if (k.up == JF_UP_H1V2) {            // h1v2_fancy_upsample: 3/4 of the nearer row, 1/4 of the further, the edge rows repeated
    const int r = y >> 1;
    const int rn = (y & 1) ? (r + 1 < k.dh ? r + 1 : r) : (r > 0 ? r - 1 : 0);
    return (3 * p[(size_t)r * pitch + x] + p[(size_t)rn * pitch + x] + ((y & 1) ? 2 : 1)) >> 2;
  }
  return p[(size_t)(y / k.ry) * pitch + x / k.rx];
}

// ---- colour: the components' samples at one pixel -> the oc bytes of the output (o[4]) ------------------------------------------
JD_FN uint32_t jf_muldiv255(uint32_t a, uint32_t b) {
  const uint32_t t = a * b + 128u;
  return ((t >> 8) + t) >> 8;
}
JD_FN void jf_pixel(int color, int conv, bool swap, const int32_t* s, uint8_t* o) {
  if (color == ATTWARP_JPEGDEC_COLOR_GREY) {
    o[0] = o[1] = o[2] = (uint8_t)s[0];
    return;
  }
  uint32_t r, g, b;
  if (color == ATTWARP_JPEGDEC_COLOR_YCC || color == ATTWARP_JPEGDEC_COLOR_YCCK) jd_ycc_to_rgb(s[0], s[1], s[2], r, g, b);
  else { r = (uint32_t)s[0]; g = (uint32_t)s[1]; b = (uint32_t)s[2]; }
  if (color >= ATTWARP_JPEGDEC_COLOR_CMYK) {
    // Pillow's CMYK bytes ("CMYK;I": every stored sample inverted).  libjpeg hands a YCCK file out as 255 - RGB and K as
    // stored, so inverted that is RGB and 255 - K; a CMYK file is 255 - sample in all four.
    if (color == ATTWARP_JPEGDEC_COLOR_CMYK) { r = 255u - r; g = 255u - g; b = 255u - b; }
    const uint32_t k = 255u - (uint32_t)s[3];
    if (conv == JF_CONV_KEEP) { o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b; o[3] = (uint8_t)k; return; }
    const uint32_t nk = 255u - k;      // Pillow's cmyk2rgb
    r = jd_clamp8((int32_t)(nk - jf_muldiv255(r, nk)));
    g = jd_clamp8((int32_t)(nk - jf_muldiv255(g, nk)));
    b = jd_clamp8((int32_t)(nk - jf_muldiv255(b, nk)));
  }
  if (conv == JF_CONV_L) { o[0] = (uint8_t)jd_luma(r, g, b); return; }
  o[0] = (uint8_t)(swap ? b : r); o[1] = (uint8_t)g; o[2] = (uint8_t)(swap ? r : b);
}

}  // namespace attwarp
