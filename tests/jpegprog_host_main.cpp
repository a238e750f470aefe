// Host-only driver of the progressive JPEG decoder's shared core (attwarp_amd/csrc/jpegprog_blocks.hpp) for
// tests/test_jpegprog_host_cpu.py: the same text the kernels run, compiled for the CPU with -fsanitize=address,undefined.
// Reads a corpus file
//   u32 nfiles, then per file: u32 W, H, ncomp, hs, vs, nscans, data length, the bytes behind the first SOS header, then per
//   scan: u32 ncomp, comp[3], ss, se, ah, al, ri, offset of its data, ntables, per table counts[16] and symbols[256]
// and prints per file: status, CRC-32 of the coefficients as the device lays them out (0 unless the status is OK), units.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpegprog_blocks.hpp"
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

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t nfiles = rd32(f);
  for (uint32_t i = 0; i < nfiles; ++i) {
    JdImage* im = new JdImage();
    im->W = (int32_t)rd32(f); im->H = (int32_t)rd32(f); im->ncomp = (int32_t)rd32(f);
    im->hs = (int32_t)rd32(f); im->vs = (int32_t)rd32(f);
    const uint32_t nscans = rd32(f), n = rd32(f);
    std::vector<uint8_t> data(n);                   // exactly as long as the data: the sanitizer sees any byte read outside it
    rdn(f, data.data(), n);
    im->mcux = (im->W + 8 * im->hs - 1) / (8 * im->hs);
    im->mcuy = (im->H + 8 * im->vs - 1) / (8 * im->vs);
    uint32_t blocks = 0;
    for (int c = 0; c < im->ncomp; ++c) {
      im->bw[c] = im->mcux * (c == 0 ? im->hs : 1);
      im->bh[c] = im->mcuy * (c == 0 ? im->vs : 1);
      im->block0[c] = blocks;
      blocks += (uint32_t)(im->bw[c] * im->bh[c]);
    }
    im->nblocks = blocks;
    std::vector<int16_t> coef((size_t)blocks * 64, 0);
    std::vector<JpScan> scans(nscans);
    std::vector<std::vector<uint32_t>> starts(nscans), ends(nscans);
    uint32_t restart = 0, units = 0;
    bool eoi = false;
    for (uint32_t q = 0; q < nscans; ++q) {
      JpScan& sc = scans[q];
      sc = JpScan();
      const uint32_t nc = rd32(f);
      uint32_t comp[3];
      for (int c = 0; c < 3; ++c) comp[c] = rd32(f);
      sc.ss = rd32(f); sc.se = rd32(f);
      const uint32_t ah = rd32(f);
      sc.al = rd32(f);
      const uint32_t ri = rd32(f);
      sc.off = rd32(f);
      const uint32_t ntab = rd32(f);
      for (uint32_t t = 0; t < ntab && t < 3; ++t) { rdn(f, sc.counts[t], 16); rdn(f, sc.symbols[t], 256); }
      sc.index = q;
      sc.kind = (sc.ss ? 2u : 0u) + (ah ? 1u : 0u);
      if (nc == 1) {
        const int c = (int)comp[0], h = c == 0 ? im->hs : 1, v = c == 0 ? im->vs : 1;
        const int cw = (im->W * h + im->hs - 1) / im->hs, ch = (im->H * v + im->vs - 1) / im->vs;
        sc.nslot = 1; sc.mcux = (uint32_t)((cw + 7) / 8); sc.nmcu = sc.mcux * (uint32_t)((ch + 7) / 8);
        sc.slot_c[0] = (uint8_t)c;
      } else {
        sc.mcux = (uint32_t)im->mcux; sc.nmcu = (uint32_t)(im->mcux * im->mcuy);
        for (uint32_t t = 0; t < nc; ++t) {
          const int c = (int)comp[t], h = c == 0 ? im->hs : 1, v = c == 0 ? im->vs : 1;
          for (int y = 0; y < v; ++y)
            for (int x = 0; x < h; ++x) {
              sc.slot_c[sc.nslot] = (uint8_t)c; sc.slot_y[sc.nslot] = (uint8_t)y; sc.slot_x[sc.nslot] = (uint8_t)x; sc.slot_t[sc.nslot] = (uint8_t)t;
              ++sc.nslot;
            }
        }
      }
      sc.ri = ri ? ri : sc.nmcu;
      sc.nunits = (sc.nmcu + sc.ri - 1) / sc.ri;
      units += sc.nunits;
      // the scan's restart markers, serially
      const uint8_t* s = data.data() + sc.off;
      const uint32_t len = n - sc.off;
      uint32_t term = len, bad = 0;
      starts[q].push_back(0);
      for (uint32_t p = 0; p < len; ++p) {
        if (s[p] != 0xff) continue;
        if (p + 1 < len && s[p + 1] == 0) { ++p; continue; }
        if (p + 1 < len && s[p + 1] >= 0xd0 && s[p + 1] <= 0xd7) {
          if ((s[p + 1] & 7u) != (ends[q].size() & 7u)) bad = 1;
          ends[q].push_back(p);
          starts[q].push_back(p + 2);
          ++p;
          continue;
        }
        term = p;
        break;
      }
      ends[q].push_back(term);
      if (starts[q].size() != sc.nunits || bad) restart = 1;
      uint32_t p = term;
      while (p < len && s[p] == 0xff) ++p;
      eoi = p > term && p < len && s[p] == 0xd9;
    }
    uint32_t status = restart ? (uint32_t)ATTWARP_JPEGDEC_E_RESTART : 0u;
    JdHuff* h = new JdHuff[3];
    for (uint32_t q = 0; q < nscans && !status; ++q) {
      const JpScan& sc = scans[q];
      const int ntab = sc.kind == JP_DC_FIRST ? 3 : sc.kind == JP_DC_REFINE ? 0 : 1;
      for (int t = 0; t < ntab; ++t) {
        jd_huff_ranges(h[t], sc.counts[t]);
        jd_huff_clear(h[t], sc.symbols[t], jd_nsym(sc.counts[t]), 0, 1);
        jd_huff_fill(h[t], sc.counts[t], 0, 1);
      }
      for (uint32_t k = 0; k < sc.nunits; ++k) {
        JdBits br;
        br.init(data.data() + sc.off, 0xffffffffu, starts[q][k], ends[q][k]);
        int32_t pred[3] = {0, 0, 0};
        uint32_t err = 0, eobrun = 0;
        const uint32_t m0 = k * sc.ri, m1 = m0 + sc.ri < sc.nmcu ? m0 + sc.ri : sc.nmcu;
        for (uint32_t b = m0 * sc.nslot; b < m1 * sc.nslot && !err; ++b) {
          const uint32_t m = b / sc.nslot, j = b - m * sc.nslot;
          const uint32_t bi = jp_block_index(*im, sc, m, j);
          if (bi >= blocks) { fprintf(stderr, "block index %u outside %u\n", bi, blocks); return 3; }
          int16_t* blk = coef.data() + (size_t)bi * 64;
          if (sc.kind == JP_DC_FIRST) err = jp_dc_first(br, h[sc.slot_t[j]], pred[sc.slot_t[j]], sc.al, blk[0]);
          else if (sc.kind == JP_DC_REFINE) err = jp_dc_refine(br, sc.al, blk[0]);
          else if (sc.kind == JP_AC_FIRST) {
            if (eobrun > 0) --eobrun;
            else err = jp_ac_first(br, h[0], sc.ss, sc.se, sc.al, eobrun, blk, JD_ZIGZAG);
          } else err = jp_ac_refine(br, h[0], sc.ss, sc.se, sc.al, eobrun, blk, JD_ZIGZAG);
        }
        if (err && !status) status = err;             // the lowest failing (scan, unit)
      }
    }
    delete[] h;
    if (!status && !eoi) status = ATTWARP_JPEGDEC_E_NO_EOI;
    uint32_t crc = 0;
    if (!status) crc = crc_bytes(reinterpret_cast<const uint8_t*>(coef.data()), (int)(coef.size() * 2));
    printf("%u %u %u\n", status, crc, units);
    delete im;
  }
  fclose(f);
  return 0;
}
