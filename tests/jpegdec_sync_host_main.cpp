// Host-only driver of the JPEG decoder's sub-stream core (attwarp_amd/csrc/jpegdec_blocks.hpp: jd_segment_guess,
// jd_decode_segment, jd_segment_check, jd_write_segment) for tests/test_jpegdec_sync_host_cpu.py: the same text the kernel
// runs, compiled for the CPU with -fsanitize=address,undefined, with a host loop standing in for the workgroup.
//   jpegdec_sync_host <corpus> <segment_bytes> <max_rounds>
// reads the corpus format of tests/jpegdec_host_main.cpp and prints per file: accepted, rounds, CRC-32 of the coefficients as
// the device lays them out (0 unless accepted).  File i's data lies i % 4 bytes behind a dword boundary, as a packed batch
// leaves it.
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
  if (argc != 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t S = (uint32_t)atoi(argv[2]), max_rounds = (uint32_t)atoi(argv[3]);
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
    const uint32_t n = rd32(f), lo = i & 3u;
    std::vector<uint8_t> buf(lo + n);              // exactly as long as the data: the sanitizer sees any byte read behind it
    rdn(f, buf.data() + lo, n);
    const uint8_t* s = buf.data() + lo;
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
    const uint32_t nseg = (n + S - 1) / S;
    // the scan of a one-unit file, serially: the data's end, and whether a restart marker lies in front of it
    uint32_t term = n, bad = 0;
    for (uint32_t q = 0; q < n; ++q) {
      if (s[q] != 0xff) continue;
      if (q + 1 < n && s[q + 1] == 0) { ++q; continue; }
      if (q + 1 < n && s[q + 1] >= 0xd0 && s[q + 1] <= 0xd7) { bad = 1; ++q; continue; }
      term = q;
      break;
    }
    uint32_t accepted = 0, rounds = 0, crc = 0;
    if (nunits == 1 && n >= 2 * S && nseg <= 16384 && !bad) {
      JdHuff* dc = new JdHuff[3];
      JdHuff* ac = new JdHuff[3];
      for (int c = 0; c < im->ncomp; ++c) { build(dc[c], im->dc_counts[c], im->dc_symbols[c]); build(ac[c], im->ac_counts[c], im->ac_symbols[c]); }
      const uint32_t nb0 = (uint32_t)(im->hs * im->vs), nblk = nb0 + (uint32_t)im->ncomp - 1u, expected = nmcu * nblk;
      std::vector<JdSync> entry(nseg);
      std::vector<JdSegment> res(nseg);
      std::vector<uint8_t> dirty(nseg, 1);
      for (uint32_t k = 0; k < nseg; ++k) entry[k] = jd_segment_guess(s, k, S, term);
      bool converged = false;
      while (rounds < max_rounds && !converged) {
        ++rounds;
        for (uint32_t k = 0; k < nseg; ++k)
          if (dirty[k]) jd_decode_segment(buf.data(), lo, entry[k], jd_segment_end(k, S, term), term, dc, ac, nb0, nblk, res[k]);
        bool changed = false;
        dirty[0] = 0;
        for (uint32_t k = 1; k < nseg; ++k) {
          dirty[k] = !jd_sync_equal(res[k - 1].exit, entry[k]);
          if (dirty[k]) { entry[k] = res[k - 1].exit; changed = true; }
        }
        converged = !changed;
      }
      if (converged) {
        std::vector<uint32_t> before(nseg), pred(3 * (size_t)nseg);
        uint32_t b = 0, sum[3] = {0, 0, 0}, flags = 0;
        for (uint32_t k = 0; k < nseg; ++k) {
          before[k] = b;
          for (int c = 0; c < 3; ++c) { pred[3 * (size_t)k + c] = sum[c]; sum[c] += res[k].dc[c]; }
          flags |= jd_segment_check(entry[k], res[k], b, expected, nblk);
          b += res[k].owned;
        }
        if (flags == 2u) {
          std::vector<int16_t> coef((size_t)blocks * 64, 0);
          alignas(4) int16_t blk[64];
          uint32_t werr = 0;
          for (uint32_t k = 0; k < nseg; ++k)
            werr |= jd_write_segment(buf.data(), lo, entry[k], term, dc, ac, *im, nb0, nblk, before[k], &pred[3 * (size_t)k], res[k].owned,
                                     expected, blk, JD_ZIGZAG, coef.data());
          if (werr) { fprintf(stderr, "file %u: the write pass failed with %u after the check passed\n", i, werr); return 3; }
          accepted = 1;
          crc = crc_bytes(reinterpret_cast<const uint8_t*>(coef.data()), (int)(coef.size() * 2));
        }
      }
      delete[] dc;
      delete[] ac;
    }
    printf("%u %u %u\n", accepted, rounds, crc);
    delete im;
  }
  fclose(f);
  return 0;
}
