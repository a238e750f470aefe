// Host-only check of the JPEG encoder's shared host / device pieces (attwarp_amd/csrc/jpegenc_blocks.hpp) for
// tests/test_jpegenc_host_cpu.py: the same text the kernels run, compiled for the CPU with -fsanitize=address,undefined.
//   je_y / je_cb / je_cr  all 2^24 triples against the formulas in 64-bit arithmetic;
//   je_quantize           every divisor 8 * (1 .. 255) and every coefficient -DCT_RANGE .. DCT_RANGE against plain division;
//   je_fdct               the recorded blocks of the input file (all 0, all 255, checkerboards, noise) against the restatement's
//                         coefficients; UBSan guards the claim that int32 suffices;
//   JeSrc::block / je_slot / je_fdct / je_quantize
//                         the transform kernel's body, block by block in scan order, over the recorded images (every layout,
//                         odd sizes, dummy blocks, both channel orders, a pitch) against the restatement's zigzag coefficients;
//                         every pixel buffer is exactly H * pitch bytes, so the sanitizer sees a read outside the image;
//   je_build_huffman      prints the four DHT payloads (class / id, BITS, VALS) and the code of every symbol for the Python side.
// File: int32 words.  nblk, nblk x (64 samples, 64 coefficients); nimg, nimg x (H, W, C, hmax, vmax, swap, pitch, quality,
// nblocks, H * pitch pixel bytes one per word, nblocks x 64 coefficients).  Prints the tables, one line "jpegenc_host ok N".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpegenc_blocks.hpp"

using namespace attwarp;

constexpr int DCT_RANGE = 1 << 16;     // the DCT's output (scaled by 8) stays below 8 * 1026; checked far beyond

static int bad(const char* what, long a, long b, long c) {
  fprintf(stderr, "jpegenc_host: %s at %ld %ld %ld\n", what, a, b, c);
  return 3;
}

int main(int argc, char** argv) {
  long checks = 0;
  // ---- colour ---------------------------------------------------------------------------------------------------------------
  for (int r = 0; r < 256; ++r)
    for (int g = 0; g < 256; ++g)
      for (int b = 0; b < 256; ++b) {
        const long long y = (19595LL * r + 38470LL * g + 7471LL * b + 32768LL) >> 16;
        const long long cb = (-11059LL * r - 21709LL * g + 32768LL * b + (128LL << 16) + 32767LL) >> 16;
        const long long cr = (32768LL * r - 27439LL * g - 5329LL * b + (128LL << 16) + 32767LL) >> 16;
        if (je_y(r, g, b) != y || je_cb(r, g, b) != cb || je_cr(r, g, b) != cr) return bad("colour", r, g, b);
        if (y < 0 || y > 255 || cb < 0 || cb > 255 || cr < 0 || cr > 255) return bad("colour range", r, g, b);
        ++checks;
      }
  // ---- quantiser ------------------------------------------------------------------------------------------------------------
  for (int q = 1; q <= 255; ++q) {
    const uint32_t d = (uint32_t)q << 3, rc = je_recip(d);
    for (int c = -DCT_RANGE; c <= DCT_RANGE; ++c) {
      const int mag = ((c < 0 ? -c : c) + (int)(d >> 1)) / (int)d;
      if (je_quantize(c, d, rc) != (c < 0 ? -mag : mag)) return bad("quantise", q, c, je_quantize(c, d, rc));
    }
    checks += 2 * DCT_RANGE + 1;
  }
  // ---- Huffman tables ---------------------------------------------------------------------------------------------------------
  for (int t = 0; t < 4; ++t) {
    printf("dht %d", (t & 1) << 4 | t >> 1);
    for (int k = 0; k < 16; ++k) printf(" %d", JE_BITS[t][k]);
    for (int k = 0; k < je_nvals(t); ++k) printf(" %d", je_vals(t)[k]);
    printf("\n");
    uint32_t code[256];
    je_build_huffman(t, code);
    printf("codes %d", t);
    for (int s = 0; s < 256; ++s) printf(" %u", code[s]);
    printf("\n");
  }
  for (int quality : {1, 30, 75, 95, 100}) {
    printf("quant %d", quality);
    for (int t = 0; t < 2; ++t)
      for (int k = 0; k < 64; ++k) printf(" %d", je_quant_value(quality, t, k));
    printf(" bound %d %d\n", je_block_bound_bits(quality, 1), je_block_bound_bits(quality, 3));
    if (je_block_bound_bits(quality, 3) > JE_BLOCK_MAX_BITS) return bad("block bound", quality, 0, 0);
  }
  if (argc < 2) return bad("no input file", 0, 0, 0);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return bad("cannot open the input file", 0, 0, 0);
  auto word = [&]() {
    int32_t v = 0;
    if (fread(&v, 4, 1, f) != 1) { fprintf(stderr, "jpegenc_host: short file\n"); exit(4); }
    return (int)v;
  };
  // ---- the DCT on recorded blocks -----------------------------------------------------------------------------------------------
  const int nblk = word();
  for (int i = 0; i < nblk; ++i) {
    int d[64], want[64];
    for (int& v : d) v = word();
    for (int& v : want) v = word();
    je_fdct(d);
    for (int k = 0; k < 64; ++k)
      if (d[k] != want[k]) return bad("fdct", i, k, d[k]);
    ++checks;
  }
  // ---- the transform over recorded images -----------------------------------------------------------------------------------------
  const int nimg = word();
  for (int n = 0; n < nimg; ++n) {
    JeSrc src;
    src.H = word(); src.W = word(); src.C = word(); src.hmax = word(); src.vmax = word();
    src.swap = word() != 0;
    src.pitch = word();
    const int quality = word(), nblocks = word();
    std::vector<uint8_t> pix((size_t)src.H * (size_t)src.pitch);
    for (auto& v : pix) v = (uint8_t)word();
    src.p = pix.data();
    const int bpm = src.C == 3 ? src.hmax * src.vmax + 2 : 1;
    const int mcus_x = (src.W + 8 * src.hmax - 1) / (8 * src.hmax), mcus_y = (src.H + 8 * src.vmax - 1) / (8 * src.vmax);
    const int wb = (src.W + 7) >> 3, hb = (src.H + 7) >> 3;
    if (nblocks != mcus_x * mcus_y * bpm) return bad("block count", n, nblocks, mcus_x * mcus_y * bpm);
    for (int blk = 0; blk < nblocks; ++blk) {
      const int mcu = blk / bpm, s = blk % bpm, my = mcu / mcus_x, mx = mcu % mcus_x;
      JeSlot sl = je_slot(s, src.hmax, src.vmax, src.C, mx, my, wb, hb);
      const bool dummy = sl.src >= 0;
      if (dummy) sl = je_slot(sl.src, src.hmax, src.vmax, src.C, mx, my, wb, hb);
      if (sl.src >= 0) return bad("a dummy block's source is a dummy", n, blk, sl.src);
      const int col = sl.comp ? mx : mx * src.hmax + sl.bx, row = sl.comp ? my : my * src.vmax + sl.by;
      int d[64];
      src.block(sl.comp, col, row, d);
      je_fdct(d);
      const int t = sl.comp ? 1 : 0;
      for (int k = 0; k < 64; ++k) {
        const int nat = je_zigzag(k);
        const uint32_t div = (uint32_t)je_quant_value(quality, t, nat) << 3;
        int v = je_quantize(d[nat], div, je_recip(div));
        if (dummy && k) v = 0;
        const int want = word();
        if (v != want) return bad("transform", n, blk, k);
      }
      ++checks;
    }
  }
  fclose(f);
  printf("jpegenc_host ok %ld\n", checks);
  return 0;
}
