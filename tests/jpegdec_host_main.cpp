// Host-only driver of the JPEG decoder's shared core (attwarp_amd/csrc/jpegdec_blocks.hpp) for
// tests/test_jpegdec_host_cpu.py: the same text the kernels run, compiled for the CPU with -fsanitize=address,undefined.
// Reads a corpus file
//   u32 nfiles, then per file: u32 W, H, ncomp, hs, vs, ri, per component (dc counts[16], dc symbols[256], ac counts[16],
//   ac symbols[256]), u32 stream length, the bytes behind the SOS header
// and prints per file: status, CRC-32 of the coefficients as the device lays them out (0 unless the status is OK), planned
// units.  The IDCT, up-sampling and colour arithmetic run once over hostile values at the end.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpegdec_blocks.hpp"
#include "png_blocks.hpp"

using namespace attwarp;

static uint32_t rd32(FILE* f) {
  uint8_t b[4];
  if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short corpus\n"); exit(2); }
  return b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}
static void rdn(FILE* f, uint8_t* d, size_t n) {
  if (n && fread(d, 1, n, f) != n) { fprintf(stderr, "short corpus\n"); exit(2); }
}

static void build(JdHuff& h, const uint8_t* counts, const uint8_t* symbols) {
  jd_huff_ranges(h, counts);
  jd_huff_clear(h, symbols, jd_nsym(counts), 0, 1);
  jd_huff_fill(h, counts, 0, 1);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t nfiles = rd32(f);
  for (uint32_t i = 0; i < nfiles; ++i) {
    JdImage* im = new JdImage();
    im->W = (int32_t)rd32(f); im->H = (int32_t)rd32(f); im->ncomp = (int32_t)rd32(f);
    im->hs = (int32_t)rd32(f); im->vs = (int32_t)rd32(f);
    const uint32_t ri_file = rd32(f);
    for (int c = 0; c < im->ncomp; ++c) {
      rdn(f, im->dc_counts[c], 16); rdn(f, im->dc_symbols[c], 256);
      rdn(f, im->ac_counts[c], 16); rdn(f, im->ac_symbols[c], 256);
    }
    const uint32_t n = rd32(f);
    std::vector<uint8_t> s(n);                     // exactly as long as the data: the sanitizer sees any byte read outside it
    rdn(f, s.data(), n);
    im->mcux = (im->W + 8 * im->hs - 1) / (8 * im->hs);
    im->mcuy = (im->H + 8 * im->vs - 1) / (8 * im->vs);
    const uint32_t nmcu = (uint32_t)im->mcux * (uint32_t)im->mcuy;
    im->ri = ri_file ? (int32_t)ri_file : (int32_t)nmcu;
    const uint32_t nunits = (nmcu + (uint32_t)im->ri - 1) / (uint32_t)im->ri;
    uint32_t blocks = 0;
    for (int c = 0; c < im->ncomp; ++c) {
      im->bw[c] = im->mcux * (c == 0 ? im->hs : 1);
      im->bh[c] = im->mcuy * (c == 0 ? im->vs : 1);
      im->block0[c] = blocks;
      blocks += (uint32_t)(im->bw[c] * im->bh[c]);
    }
    im->nblocks = blocks;
    // the scan, serially
    std::vector<uint32_t> starts(1, 0u), ends;
    uint32_t term = n, bad = 0;
    for (uint32_t q = 0; q < n; ++q) {
      if (s[q] != 0xff) continue;
      if (q + 1 < n && s[q + 1] == 0) { ++q; continue; }
      if (q + 1 < n && s[q + 1] >= 0xd0 && s[q + 1] <= 0xd7) {
        if ((s[q + 1] & 7u) != (ends.size() & 7u)) bad = 1;
        ends.push_back(q);
        starts.push_back(q + 2);
        ++q;
        continue;
      }
      term = q;
      break;
    }
    ends.push_back(term);
    uint32_t q = term;
    while (q < n && s[q] == 0xff) ++q;
    const bool eoi = q > term && q < n && s[q] == 0xd9;
    uint32_t status = (starts.size() != nunits || bad) ? (uint32_t)ATTWARP_JPEGDEC_E_RESTART : 0u;
    std::vector<int16_t> coef((size_t)blocks * 64, 0);
    if (!status) {
      JdHuff* dc = new JdHuff[3];
      JdHuff* ac = new JdHuff[3];
      for (int c = 0; c < im->ncomp; ++c) { build(dc[c], im->dc_counts[c], im->dc_symbols[c]); build(ac[c], im->ac_counts[c], im->ac_symbols[c]); }
      for (uint32_t k = 0; k < nunits; ++k) {
        JdBits br;
        br.init(s.data(), 0xffffffffu, starts[k], ends[k]);
        int32_t pred[3] = {0, 0, 0};
        uint32_t err = 0;
        const uint32_t m0 = k * (uint32_t)im->ri, m1 = m0 + (uint32_t)im->ri < nmcu ? m0 + (uint32_t)im->ri : nmcu;
        for (uint32_t m = m0; m < m1 && !err; ++m)
          for (int c = 0; c < im->ncomp && !err; ++c) {
            const int nb = c == 0 ? im->hs * im->vs : 1, hh = c == 0 ? im->hs : 1;
            for (int j = 0; j < nb && !err; ++j) {
              int16_t blk[64] = {0};
              err = jd_decode_block(br, dc[c], ac[c], pred[c], blk, JD_ZIGZAG);
              if (err) break;
              const uint32_t bi = jd_block_index(*im, c, m, j / hh, j % hh);
              if (bi >= blocks) { fprintf(stderr, "block index %u outside %u\n", bi, blocks); return 3; }
              for (int e = 0; e < 64; ++e) coef[(size_t)bi * 64 + e] = blk[e];
            }
          }
        if (err && !status) status = err;             // the lowest failing unit
      }
      delete[] dc;
      delete[] ac;
      if (!status && !eoi) status = ATTWARP_JPEGDEC_E_NO_EOI;
    }
    uint32_t crc = 0;
    if (!status) crc = crc_bytes(reinterpret_cast<const uint8_t*>(coef.data()), (int)(coef.size() * 2));
    printf("%u %u %u\n", status, crc, nunits);
    delete im;
  }
  fclose(f);
  // the pixel arithmetic over extreme values: nothing here may be undefined behaviour
  uint32_t acc = 0;
  for (int32_t a : {-32768, -1, 0, 1, 32767})
    for (uint32_t qv : {0u, 1u, 255u}) {
      uint32_t in[8];
      int32_t o[8], o2[8];
      for (int e = 0; e < 8; ++e) in[e] = (uint32_t)(a * (e & 1 ? -1 : 1)) * qv;
      jd_idct_1d(in, 11, o);
      for (int e = 0; e < 8; ++e) in[e] = (uint32_t)o[e];
      jd_idct_1d(in, 18, o2);
      for (int e = 0; e < 8; ++e) acc += jd_clamp8(o2[e] + 128);
    }
  const uint8_t plane[6] = {0, 255, 7, 200, 255, 0};
  for (int y = 0; y < 4; ++y)
    for (int x = 0; x < 6; ++x) {
      uint32_t r, g, b;
      jd_ycc_to_rgb(255, jd_chroma(plane, 3, 3, 2, 2, 2, x, y), jd_chroma(plane, 3, 3, 2, 2, 1, x, y >> 1), r, g, b);
      acc += jd_luma(r, g, b);
    }
  printf("arith %u\n", acc);
  return 0;
}
