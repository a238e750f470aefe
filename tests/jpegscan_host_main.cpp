// Host-only driver of the shared core of the JPEG decoder's scans-of-any-layout family (attwarp_amd/csrc/jpegscan_blocks.hpp,
// over jpegfmt_blocks.hpp and jpegprog_blocks.hpp) for tests/test_jpegscan_host_cpu.py: the same text the kernels run,
// compiled for the CPU with -fsanitize=address,undefined.  Reads a corpus file
//   u32 nfiles, then per file: u32 W, H, ncomp, h[4], v[4], colour rule, nscans, data length, the bytes behind the first SOS
//   header, then per scan: u32 ncomp, comp[4], ss, se, ah, al, sequential, ri, offset of its data, DC tables, AC tables, and
//   per table counts[16] and symbols[256] (the DC tables first)
// and prints per file: status, CRC-32 of the coefficients as the device lays them out (0 unless the status is OK), units.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpegscan_blocks.hpp"
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
    JfImage* im = new JfImage();
    const int W = (int)rd32(f), H = (int)rd32(f), ncomp = (int)rd32(f);
    int32_t h[4], v[4];
    for (int c = 0; c < 4; ++c) h[c] = (int32_t)rd32(f);
    for (int c = 0; c < 4; ++c) v[c] = (int32_t)rd32(f);
    const int color = (int)rd32(f);
    const uint32_t nscans = rd32(f), n = rd32(f);
    std::vector<uint8_t> data(n);                   // exactly as long as the data: the sanitizer sees any byte read outside it
    rdn(f, data.data(), n);
    if (jf_layout(*im, W, H, ncomp, h, v, color) != JF_OK) { fprintf(stderr, "file %u: layout refused\n", i); return 3; }
    const uint32_t blocks = im->nblocks;
    std::vector<int16_t> coef((size_t)blocks * 64, 0);
    std::vector<JsScan> scans(nscans);
    std::vector<std::vector<uint32_t>> starts(nscans), ends(nscans);
    uint32_t restart = 0, units = 0;
    bool eoi = false;
    for (uint32_t q = 0; q < nscans; ++q) {
      JsScan& sc = scans[q];
      sc = JsScan();
      sc.ncomp = rd32(f);
      uint32_t comp[4];
      for (int c = 0; c < 4; ++c) comp[c] = rd32(f);
      sc.ss = rd32(f); sc.se = rd32(f);
      const uint32_t ah = rd32(f);
      sc.al = rd32(f);
      const uint32_t seq = rd32(f), ri = rd32(f);
      sc.off = rd32(f);
      const uint32_t ndc = rd32(f), nac = rd32(f);
      for (uint32_t t = 0; t < ndc && t < 4; ++t) { rdn(f, sc.dc_counts[t], 16); rdn(f, sc.dc_symbols[t], 256); }
      for (uint32_t t = 0; t < nac && t < 4; ++t) { rdn(f, sc.ac_counts[t], 16); rdn(f, sc.ac_symbols[t], 256); }
      sc.index = q;
      sc.kind = seq ? JS_SEQUENTIAL : (sc.ss ? 2u : 0u) + (ah ? 1u : 0u);
      if (sc.ncomp == 1) {
        const JfComp& k = im->comp[comp[0] & 3u];
        sc.nslot = 1; sc.mcux = (uint32_t)((k.dw + 7) / 8); sc.nmcu = sc.mcux * (uint32_t)((k.dh + 7) / 8);
        sc.slot_c[0] = (uint8_t)comp[0];
      } else {
        sc.mcux = (uint32_t)im->mcux; sc.nmcu = (uint32_t)(im->mcux * im->mcuy);
        for (uint32_t t = 0; t < sc.ncomp && t < 4; ++t) {
          const JfComp& k = im->comp[comp[t] & 3u];
          for (int y = 0; y < k.v; ++y)
            for (int x = 0; x < k.h && sc.nslot < (uint32_t)JF_MAX_SLOTS; ++x) {
              sc.slot_c[sc.nslot] = (uint8_t)comp[t]; sc.slot_y[sc.nslot] = (uint8_t)y; sc.slot_x[sc.nslot] = (uint8_t)x; sc.slot_t[sc.nslot] = (uint8_t)t;
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
    JdHuff* dc = new JdHuff[4];
    JdHuff* ac = new JdHuff[4];
    for (uint32_t q = 0; q < nscans && !status; ++q) {
      const JsScan& sc = scans[q];
      for (int t = 0; t < 4; ++t) { build(dc[t], sc.dc_counts[t], sc.dc_symbols[t]); build(ac[t], sc.ac_counts[t], sc.ac_symbols[t]); }
      for (uint32_t k = 0; k < sc.nunits; ++k) {
        for (uint32_t m = k * sc.ri; m < sc.nmcu && m < (k + 1) * sc.ri; ++m)
          for (uint32_t j = 0; j < sc.nslot; ++j)
            if (js_block_index(*im, sc, m, j) >= blocks) { fprintf(stderr, "block index outside %u\n", blocks); return 3; }
        JdBits br;
        br.init(data.data() + sc.off, 0xffffffffu, starts[q][k], ends[q][k]);
        const uint32_t err = js_decode_unit(br, *im, sc, dc, ac, k, coef.data());
        if (err && !status) status = err;             // the lowest failing (scan, unit)
      }
    }
    delete[] dc;
    delete[] ac;
    if (!status && !eoi) status = ATTWARP_JPEGDEC_E_NO_EOI;
    uint32_t crc = 0;
    if (!status) crc = crc_bytes(reinterpret_cast<const uint8_t*>(coef.data()), (int)(coef.size() * 2));
    printf("%u %u %u\n", status, crc, units);
    delete im;
  }
  fclose(f);
  return 0;
}
