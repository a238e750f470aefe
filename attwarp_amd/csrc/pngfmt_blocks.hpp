// What lies behind the filters of a PNG file that is not 8-bit, non-interlaced grey / RGB (pngdec.hip) as
// __host__ __device__ code: which depth / colour-type pairs exist, the seven Adam7 passes and their sizes, the filter
// unit, bit unpacking, the palette and the conversion to 8 bits.  The same text runs inside pngdec_unfilter_formats_kernel,
// in the host planner and, under a sanitizer, in tests/pngfmt_host_main.cpp; tests/pngfmt_ref.py restates it.
#pragma once
#include "pngdec_blocks.hpp"

namespace attwarp {

constexpr int PF_PASSES = 7;
constexpr int PF_PALETTE_LDS = 1024;                     // 256 converted palette entries, one uint32 each

struct PfImage {                       // the per-image format record of a planned table (behind the chunks)
  int32_t depth, ctype, interlace;
  uint32_t pal_off;                    // 768 palette bytes (zero padded) in the table, 0: no palette
};
static_assert(sizeof(PfImage) == 16, "record layout");

// channels of a colour type, alpha included (palette: one index)
__host__ __device__ inline int pf_channels(int ctype) { return ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 1; }

// the depth / colour-type pairs of the PNG specification
__host__ __device__ inline bool pf_valid(int depth, int ctype) {
  if (ctype == 0) return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
  if (ctype == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
  if (ctype == 2 || ctype == 4 || ctype == 6) return depth == 8 || depth == 16;
  return false;
}

// true: the parent's kernel decodes it (8 bits, no interlace, no palette)
__host__ __device__ inline bool pf_plain(int depth, int ctype, int interlace) { return depth == 8 && interlace == 0 && ctype != 3; }

// bytes of one filter unit, the filters' "pixel": 1, 2, 3, 4, 6 or 8
__host__ __device__ inline int pf_unit(int ch, int depth) { return ch * depth >= 8 ? ch * depth / 8 : 1; }

// 1 + ceil(w * ch * depth / 8): one filtered row of w pixels
__host__ __device__ inline int64_t pf_row_bytes(int64_t w, int ch, int depth) { return 1 + (w * ch * depth + 7) / 8; }

// output channels: L 1, RGB 3, keep the file's without alpha (a palette file: its palette's three)
__host__ __device__ inline int pf_out_channels(int ctype, int mode) {
  return mode == ATTWARP_PNGDEC_L ? 1 : mode == ATTWARP_PNGDEC_RGB ? 3 : (ctype == 0 || ctype == 4 ? 1 : 3);
}

struct PfPass {
  int x0, y0, dx, dy;                  // first column / row of the pass in the image and its steps
  int w, h;                            // its size; w == 0 or h == 0: the pass has no bytes
};

// Pass p (0 .. 6) of a W x H image.  Adam7's (x0, y0, dx, dy) are (0,0,8,8) (4,0,8,8) (0,4,4,8) (2,0,4,4) (0,2,2,4) (1,0,2,2)
// (0,1,1,2), one hexadecimal digit each; a non-interlaced image is its pass 0 alone.
__host__ __device__ inline PfPass pf_pass(int interlace, int p, int W, int H) {
  PfPass g;
  if (!interlace) {
    g.x0 = 0; g.y0 = 0; g.dx = 1; g.dy = 1;
    g.w = p == 0 ? W : 0;
    g.h = p == 0 ? H : 0;
    return g;
  }
  const int sh = 4 * p;
  g.x0 = (0x0102040 >> sh) & 15;
  g.y0 = (0x1020400 >> sh) & 15;
  g.dx = (0x1224488 >> sh) & 15;
  g.dy = (0x2244888 >> sh) & 15;
  g.w = W > g.x0 ? (W - g.x0 + g.dx - 1) / g.dx : 0;
  g.h = H > g.y0 ? (H - g.y0 + g.dy - 1) / g.dy : 0;
  return g;
}

__host__ __device__ inline int64_t pf_pass_bytes(const PfPass& g, int ch, int depth) {
  return g.w > 0 && g.h > 0 ? (int64_t)g.h * pf_row_bytes(g.w, ch, depth) : 0;
}

// where pass p starts in the image's filtered bytes; p == PF_PASSES: their sum, the image's filtered size
__host__ __device__ inline int64_t pf_pass_offset(int interlace, int p, int W, int H, int ch, int depth) {
  int64_t off = 0;
  for (int q = 0; q < p; ++q) off += pf_pass_bytes(pf_pass(interlace, q, W, H), ch, depth);
  return off;
}

// pixels one filter unit holds: 8 / 4 / 2 below 8 bits, else 1
__host__ __device__ inline int pf_unit_pixels(int depth) { return depth < 8 ? 8 / depth : 1; }

// Pixel j of a reconstructed unit (its bytes in file order from bit 0) -> the file's channels at 8 bits without alpha:
// grey or the palette index in the low byte, or R | G << 8 | B << 16.
//   below 8 bits   samples MSB first in the byte; grey scaled by 255 / 85 / 17;
//   16-bit grey    saturates, min(v, 255), as Pillow's I;16 -> L does;
//   other 16 bits  the high byte of each sample.
__host__ __device__ inline uint32_t pf_pixel(int ctype, int depth, uint64_t unit, int j) {
  if (depth < 8) {
    const uint32_t mask = (1u << depth) - 1u;
    const uint32_t s = ((uint32_t)unit >> (8 - depth * (j + 1))) & mask;
    return ctype == 0 ? s * (255u / mask) : s;
  }
  if (depth == 8) return ctype == 2 || ctype == 6 ? (uint32_t)unit & 0xffffffu : (uint32_t)unit & 255u;
  if (ctype == 0) {
    const uint32_t v = ((uint32_t)unit & 255u) << 8 | ((uint32_t)(unit >> 8) & 255u);
    return v < 255u ? v : 255u;
  }
  if (ctype == 4) return (uint32_t)unit & 255u;
  return ((uint32_t)unit & 255u) | ((uint32_t)(unit >> 16) & 255u) << 8 | ((uint32_t)(unit >> 32) & 255u) << 16;
}

// entry i of the palette (768 bytes, zero padded: an index at or past the entries is black) as the output's packed bytes
__host__ __device__ inline uint32_t pf_palette_entry(const uint8_t* pal, int i, int oc, bool swap) {
  const uint32_t r = pal[3 * i], g = pal[3 * i + 1], b = pal[3 * i + 2];
  if (oc == 1) return pd_luma(r, g, b);
  return swap ? b | g << 8 | r << 16 : r | g << 8 | b << 16;
}

// what pf_pixel gave -> the output pixel's oc bytes, packed from bit 0; ptab: the 256 pf_palette_entry values
template <typename Table>
__host__ __device__ inline uint32_t pf_output(int ctype, uint32_t px, int oc, bool swap, const Table& ptab) {
  if (ctype == 3) return ptab[px & 255u];
  if (ctype == 0 || ctype == 4) return oc == 1 ? px : px * 0x010101u;
  const uint32_t r = px & 255u, g = (px >> 8) & 255u, b = (px >> 16) & 255u;
  if (oc == 1) return pd_luma(r, g, b);
  return swap ? b | g << 8 | r << 16 : px;
}

}  // namespace attwarp
