// Host-only driver of the JPEG decoder's layout family (attwarp_amd/csrc/jpegfmt_blocks.hpp on jpegdec_blocks.hpp) for
// tests/test_jpegfmt_host_cpu.py: the same text the kernels run, compiled for the CPU with -fsanitize=address,undefined.
// Reads a corpus file
//   u32 nfiles, segment bytes, max rounds, then per file: u32 W, H, ncomp, h[4], v[4], colour rule, ri, per component
//   (dc counts[16], dc symbols[256], ac counts[16], ac symbols[256]), u32 stream length, the bytes behind the SOS header
// and prints per file: the planner's check (jf_layout; a refused file ends its line there), status, CRC-32 of the
// coefficients as the device lays them out (0 unless the status is OK), planned units, then what the sub-streams make of
// a marker-less file: accepted, whether the coefficients they wrote equal the sequential walk's, the rounds they took and the
// period of the MCU's table sequence.  The up-sampling and colour arithmetic run once over extreme values at the end.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpegfmt_blocks.hpp"
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
  const uint32_t nfiles = rd32(f), S = rd32(f), max_rounds = rd32(f);
  for (uint32_t i = 0; i < nfiles; ++i) {
    JfImage* im = new JfImage();
    const int W = (int)rd32(f), H = (int)rd32(f), ncomp = (int)rd32(f);
    int32_t h[4], v[4];
    for (int c = 0; c < 4; ++c) h[c] = (int32_t)rd32(f);
    for (int c = 0; c < 4; ++c) v[c] = (int32_t)rd32(f);
    const int color = (int)rd32(f);
    const uint32_t ri_file = rd32(f);
    for (int c = 0; c < ncomp && c < 4; ++c) {
      rdn(f, im->dc_counts[c], 16); rdn(f, im->dc_symbols[c], 256);
      rdn(f, im->ac_counts[c], 16); rdn(f, im->ac_symbols[c], 256);
    }
    const uint32_t n = rd32(f), lo = i & 3u;
    std::vector<uint8_t> buf(lo + n);              // exactly as long as the data: the sanitizer sees any byte read outside it
    rdn(f, buf.data() + lo, n);
    const uint8_t* s = buf.data() + lo;
    const int rc = jf_layout(*im, W, H, ncomp, h, v, color);
    if (rc != JF_OK) { printf("%d\n", rc); delete im; continue; }
    if (jf_blocks(W, H, ncomp, h, v) != im->nblocks) { fprintf(stderr, "file %u: jf_blocks disagrees with jf_layout\n", i); return 3; }
    const uint32_t nmcu = (uint32_t)im->mcux * (uint32_t)im->mcuy, blocks = im->nblocks;
    im->ri = ri_file ? (int32_t)ri_file : (int32_t)nmcu;
    const uint32_t nunits = (nmcu + (uint32_t)im->ri - 1) / (uint32_t)im->ri;
    for (uint32_t m = 0; m < nmcu; ++m)            // every slot of every MCU lies inside its component's blocks
      for (uint32_t j = 0; j < (uint32_t)im->nslot; ++j) {
        const JfComp& k = im->comp[im->slot_c[j]];
        const uint32_t bi = jf_slot_block(*im, j, m % (uint32_t)im->mcux, m / (uint32_t)im->mcux);
        if (bi < k.block0 || bi >= k.block0 + (uint32_t)(k.bw * k.bh)) { fprintf(stderr, "file %u: block %u outside its plane\n", i, bi); return 3; }
      }
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
    JdHuff* dc = new JdHuff[JF_MAX_COMP];
    JdHuff* ac = new JdHuff[JF_MAX_COMP];
    for (int c = 0; c < ncomp; ++c) { build(dc[c], im->dc_counts[c], im->dc_symbols[c]); build(ac[c], im->ac_counts[c], im->ac_symbols[c]); }
    if (!status) {
      for (uint32_t k = 0; k < nunits; ++k) {
        JdBits br;
        br.init(s, 0xffffffffu, starts[k], ends[k]);
        const uint32_t m0 = k * (uint32_t)im->ri, m1 = m0 + (uint32_t)im->ri < nmcu ? m0 + (uint32_t)im->ri : nmcu;
        const uint32_t err = jf_decode_unit(br, *im, dc, ac, m0, m1, coef.data());
        if (err && !status) status = err;             // the lowest failing unit
      }
      if (!status && !eoi) status = ATTWARP_JPEGDEC_E_NO_EOI;
    }
    const bool decoded = status == 0 || status == (uint32_t)ATTWARP_JPEGDEC_E_NO_EOI;
    uint32_t crc = 0;
    if (!status) crc = crc_bytes(reinterpret_cast<const uint8_t*>(coef.data()), (int)(coef.size() * 2));
    // the sub-streams of a marker-less file (jpegfmt_substream_kernel, serially): accepted only where the sequential walk
    // reaches the last block, and then with its coefficients
    const uint32_t nseg = (n + S - 1) / S;
    uint32_t accepted = 0, same = 0, rounds = 0;
    im->period = jf_period(*im);
    if (im->period < 1 || im->nslot % im->period) { fprintf(stderr, "file %u: period %d of %d slots\n", i, im->period, im->nslot); return 3; }
    if (nunits == 1 && n >= 2 * S && nseg <= 16384 && starts.size() == 1) {
      const JfLayout lay{*im};
      const uint32_t nblk = (uint32_t)im->nslot, expected = nmcu * nblk;
      std::vector<JdSync> entry(nseg);
      std::vector<JfSegment> res(nseg);
      std::vector<uint8_t> dirty(nseg, 1);
      for (uint32_t k = 0; k < nseg; ++k) entry[k] = jd_segment_guess(s, k, S, term);
      bool converged = false;
      while (rounds < max_rounds && !converged) {
        ++rounds;
        for (uint32_t k = 0; k < nseg; ++k)
          if (dirty[k]) jd_decode_segment_of(lay, buf.data(), lo, entry[k], jd_segment_end(k, S, term), term, dc, ac, nblk, res[k]);
        bool changed = false;
        dirty[0] = 0;
        for (uint32_t k = 1; k < nseg; ++k) {
          dirty[k] = !jd_sync_equal(res[k - 1].exit, entry[k]);
          if (dirty[k]) { entry[k] = res[k - 1].exit; changed = true; }
        }
        converged = !changed;
      }
      if (converged) {
        std::vector<uint32_t> before(nseg), pred(4 * (size_t)nseg);
        uint32_t b = 0, sum[4] = {0, 0, 0, 0}, flags = 0;
        for (uint32_t k = 0; k < nseg; ++k) {
          before[k] = b;
          for (int c = 0; c < 4; ++c) pred[4 * (size_t)k + c] = sum[c];
          for (uint32_t e = 0; e < nblk; ++e) sum[lay.comp((b + e) % nblk)] += res[k].dc[e];     // the e-th owned block is block b + e
          flags |= jd_segment_check(entry[k], res[k], b, expected, nblk, lay.period(nblk));
          b += res[k].owned;
        }
        if (flags == 2u) {
          std::vector<int16_t> coef2((size_t)blocks * 64, 0);
          alignas(4) int16_t blk[64];
          uint32_t werr = 0;
          for (uint32_t k = 0; k < nseg; ++k)
            werr |= jd_write_segment_of(lay, buf.data(), lo, entry[k], term, dc, ac, nblk, before[k], &pred[4 * (size_t)k], res[k].owned, expected, blk,
                                        JD_ZIGZAG, coef2.data());
          if (werr) { fprintf(stderr, "file %u: the write pass failed with %u after the check passed\n", i, werr); return 3; }
          accepted = 1;
          same = coef2 == coef;
        }
      }
      if (accepted && !decoded) { fprintf(stderr, "file %u: sub-streams accepted what the sequential walk rejects (%u)\n", i, status); return 3; }
    }
    delete[] dc;
    delete[] ac;
    printf("0 %u %u %u %u %u %u %d\n", status, crc, nunits, accepted, same, rounds, im->period);
    delete im;
  }
  fclose(f);
  // the pixel arithmetic over extreme values and every up-sampler at the planes' edges: nothing here may be undefined
  // behaviour or read outside the plane (3 x 2 samples, exactly as long as that)
  uint32_t acc = 0;
  std::vector<uint8_t> plane = {0, 255, 7, 200, 255, 0};
  for (int up = JF_UP_COPY; up <= JF_UP_BOX; ++up) {
    const int rx = up == JF_UP_COPY || up == JF_UP_H1V2 ? 1 : up == JF_UP_BOX ? 4 : 2, ry = up == JF_UP_COPY || up == JF_UP_H2V1 ? 1 : up == JF_UP_BOX ? 3 : 2;
    const JfComp k = {1, 1, 1, 1, 0, 3, 2, up, rx, ry};
    for (int y = 0; y < 2 * ry; ++y)
      for (int x = 0; x < 3 * rx; ++x) acc += (uint32_t)jf_sample(plane.data(), 3, k, x, y);
  }
  for (int color = ATTWARP_JPEGDEC_COLOR_GREY; color <= ATTWARP_JPEGDEC_COLOR_YCCK; ++color)
    for (int conv = JF_CONV_KEEP; conv <= JF_CONV_L; ++conv)
      for (int32_t a : {0, 1, 127, 128, 254, 255})
        for (int32_t b : {0, 255}) {
          const int32_t smp[4] = {a, b, 255 - a, b ^ a};
          uint8_t o[4] = {0, 0, 0, 0};
          jf_pixel(color, conv, (a & 1) != 0, smp, o);
          acc += o[0] + 3u * o[1] + 5u * o[2] + 7u * o[3];
        }
  printf("arith %u\n", acc);
  return 0;
}
