// Host-only driver of the progressive scans' sub-stream core (attwarp_amd/csrc/jpegprog_sync_blocks.hpp) for
// tests/test_jpegprog_sync_host_cpu.py: the same text jpegprog_substream_kernel runs, compiled for the CPU with
// -fsanitize=address,undefined, with a host loop standing for the workgroup (rounds over all segments, then the sums).
// Usage: program corpus segment_bytes max_rounds.  The corpus is that of tests/jpegprog_host_main.cpp.
// Every file is decoded twice, scan by scan in file order: by the sequential walk of jpegprog_blocks.hpp, and by the
// sub-stream routes with the sequential walk where a scan is not cut or not accepted.  After every scan both coefficient
// memories must be equal, and a scan the sequential walk fails must not have been accepted: otherwise exit status 4.
// Prints per file: status, CRC-32 of the coefficients (0 unless the status is OK), then per scan
// "route segments rounds accepted crc": the record, and the CRC-32 of the coefficients behind the scan (0: the scan was not run).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegprog_sync_blocks.hpp"
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

// one unit of one scan by the sequential walk -> status
static uint32_t walk(const JdImage& im, const JpScan& sc, const uint8_t* s, uint32_t start, uint32_t end, uint32_t k, const JdHuff* h,
                     int16_t* coef) {
  JdBits br;
  br.init(s, 0xffffffffu, start, end);
  int32_t pred[3] = {0, 0, 0};
  uint32_t err = 0, eobrun = 0;
  const uint32_t m0 = k * sc.ri, m1 = m0 + sc.ri < sc.nmcu ? m0 + sc.ri : sc.nmcu;
  for (uint32_t b = m0 * sc.nslot; b < m1 * sc.nslot && !err; ++b) {
    const uint32_t m = b / sc.nslot, j = b - m * sc.nslot;
    const uint32_t bi = jp_block_index(im, sc, m, j);
    if (bi >= im.nblocks) { fprintf(stderr, "block index %u outside %u\n", bi, im.nblocks); exit(3); }
    int16_t* blk = coef + (size_t)bi * 64;
    if (sc.kind == JP_DC_FIRST) err = jp_dc_first(br, h[sc.slot_t[j]], pred[sc.slot_t[j]], sc.al, blk[0]);
    else if (sc.kind == JP_DC_REFINE) err = jp_dc_refine(br, sc.al, blk[0]);
    else if (sc.kind == JP_AC_FIRST) {
      if (eobrun > 0) --eobrun;
      else err = jp_ac_first(br, h[0], sc.ss, sc.se, sc.al, eobrun, blk, JD_ZIGZAG);
    } else err = jp_ac_refine(br, h[0], sc.ss, sc.se, sc.al, eobrun, blk, JD_ZIGZAG);
  }
  return err;
}

// the workgroup of jpegprog_substream_kernel for one cut scan -> accepted; rounds: those it ran
static bool substreams(const JdImage& im, const JpScan& sc, const uint8_t* data, uint32_t uend, uint32_t S, uint32_t max_rounds,
                       const JdHuff* h, int16_t* coef, uint32_t& rounds) {
  const uint32_t nseg = (uend + S - 1) / S, expected = sc.nmcu * sc.nslot;
  const uint32_t se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se);
  std::vector<JpSeg> seg(nseg);
  std::memset(seg.data(), 0, nseg * sizeof(JpSeg));
  rounds = 0;
  if (sc.kind == JP_DC_FIRST || sc.kind == JP_AC_FIRST) {
    for (uint32_t s = 0; s < nseg; ++s) {
      seg[s].entry = jd_segment_guess(data, s, S, uend);
      if (sc.kind == JP_AC_FIRST) seg[s].entry.bsk = ss;
      seg[s].dirty = 1;
    }
    bool converged = false;
    while (rounds < max_rounds) {
      ++rounds;
      for (uint32_t s = 0; s < nseg; ++s)
        if (seg[s].dirty) {
          JpSeg r;
          jp_first_segment(sc, data, 0, seg[s].entry, jd_segment_end(s, S, uend), uend, h, r);
          seg[s].exit = r.exit; seg[s].nbeg = r.nbeg; seg[s].nend = r.nend; seg[s].eclean = r.eclean;
          for (int c = 0; c < 3; ++c) seg[s].dc[c] = r.dc[c];
        }
      bool changed = false;
      for (uint32_t s = nseg; s-- > 0;) {                      // (downwards: every entry takes the exit of THIS round's decode)
        uint32_t d = 0;
        if (s > 0 && !jd_sync_equal(seg[s - 1].exit, seg[s].entry)) { seg[s].entry = seg[s - 1].exit; d = 1; changed = true; }
        seg[s].dirty = d;
      }
      if (!changed) { converged = true; break; }
    }
    uint32_t sum[4] = {0, 0, 0, 0}, flags = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
      seg[s].before = sum[0];
      for (int c = 0; c < 3; ++c) seg[s].pred[c] = sum[1 + c];
      flags |= jp_first_check(sc, seg[s].entry, seg[s], sum[0], expected);
      sum[0] = jp_sat_add(sum[0], seg[s].nend);
      for (int c = 0; c < 3; ++c) sum[1 + c] += seg[s].dc[c];
    }
    if (!converged || !(flags & 2u) || (flags & 1u)) return false;
    for (uint32_t s = 0; s < nseg; ++s)
      jp_first_write(sc, im, data, 0, seg[s].entry, jd_segment_end(s, S, uend), uend, h, seg[s].before, seg[s].pred, expected, JD_ZIGZAG, coef);
    return true;
  }
  uint32_t bytes = 0;
  for (uint32_t s = 0; s < nseg; ++s) {
    const uint64_t b = (uint64_t)s * S;
    seg[s].nbeg = jp_data_bytes(data, b < uend ? (uint32_t)b : uend, jd_segment_end(s, S, uend));
    seg[s].pred[1] = bytes;
    bytes += seg[s].nbeg;
  }
  if (sc.kind == JP_DC_REFINE) {
    if ((uint64_t)bytes * 8u < expected) return false;
    for (uint32_t s = 0; s < nseg; ++s) {
      const uint64_t b = (uint64_t)s * S;
      jp_dc_refine_write(sc, im, data, b < uend ? (uint32_t)b : uend, jd_segment_end(s, S, uend), seg[s].pred[1], expected, coef);
    }
    return true;
  }
  std::vector<uint64_t> mask(expected);                        // exactly as long as the scan's blocks
  std::vector<uint32_t> P(expected + 1);
  uint32_t bits = 0;
  for (uint32_t n = 0; n < expected; ++n) {
    const uint32_t bi = jp_ac_block_index(im, sc, n);
    mask[n] = bi < im.nblocks ? jp_refine_mask(coef + (size_t)bi * 64, ss, se, JD_ZIGZAG) : 0;
    P[n] = bits;
    bits += jp_popc64(mask[n]);
  }
  P[expected] = bits;
  if (!jp_refine_skim(sc, data, 0, uend, h[0], mask.data(), P.data(), expected, seg.data(), nseg)) return false;
  for (uint32_t s = nseg; s-- > 0;) {                          // (any order: the lanes of a workgroup run side by side)
    const uint32_t n1 = s + 1 < nseg ? seg[s + 1].before : expected, k1 = s + 1 < nseg ? seg[s + 1].entry.bsk & 63u : ss;
    jp_refine_write(sc, im, data, 0, jd_segment_guess(data, s, S, uend).byte, uend, h[0], seg[s], n1, k1, mask.data(), expected, JD_ZIGZAG,
                    coef);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t S = (uint32_t)atoi(argv[2]), max_rounds = (uint32_t)atoi(argv[3]);
  if (S < 32 || S > 512 || (S & (S - 1)) || max_rounds < 1) return 2;
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
    std::vector<int16_t> coef((size_t)blocks * 64, 0), coef2((size_t)blocks * 64, 0);
    std::vector<JpScan> scans(nscans);
    std::vector<std::vector<uint32_t>> starts(nscans), ends(nscans);
    uint32_t restart = 0;
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
    std::vector<uint32_t> info((size_t)nscans * 5, 0);
    JdHuff* h = new JdHuff[3];
    for (uint32_t q = 0; q < nscans && !status; ++q) {
      const JpScan& sc = scans[q];
      const int ntab = sc.kind == JP_DC_FIRST ? 3 : sc.kind == JP_DC_REFINE ? 0 : 1;
      for (int t = 0; t < ntab; ++t) {
        jd_huff_ranges(h[t], sc.counts[t]);
        jd_huff_clear(h[t], sc.symbols[t], jd_nsym(sc.counts[t]), 0, 1);
        jd_huff_fill(h[t], sc.counts[t], 0, 1);
      }
      const uint8_t* s = data.data() + sc.off;
      uint32_t err = 0;
      for (uint32_t k = 0; k < sc.nunits; ++k)
        if (const uint32_t e = walk(*im, sc, s, starts[q][k], ends[q][k], k, h, coef.data()))
          if (!err) err = e;
      const uint32_t uend = ends[q][0], nseg = (uend + S - 1) / S;
      bool accepted = false;
      if (sc.nunits == 1 && uend >= 2 * S && nseg <= JP_SYNC_MAX_SEGS) {
        uint32_t rounds = 0;
        accepted = substreams(*im, sc, s, uend, S, max_rounds, h, coef2.data(), rounds);
        info[q * 5] = 1 + sc.kind; info[q * 5 + 1] = nseg; info[q * 5 + 2] = rounds; info[q * 5 + 3] = accepted;
      }
      if (accepted && err) { fprintf(stderr, "file %u scan %u: accepted, but the sequential walk reports %u\n", i, q, err); return 4; }
      if (!accepted)
        for (uint32_t k = 0; k < sc.nunits; ++k) walk(*im, sc, s, starts[q][k], ends[q][k], k, h, coef2.data());
      if (!err && std::memcmp(coef.data(), coef2.data(), coef.size() * 2) != 0) {
        fprintf(stderr, "file %u scan %u (kind %u, %u segments, accepted %d): coefficients differ\n", i, q, sc.kind, nseg, (int)accepted);
        return 4;
      }
      if (err) status = err;
      else info[q * 5 + 4] = crc_bytes(reinterpret_cast<const uint8_t*>(coef2.data()), (int)(coef2.size() * 2));
    }
    delete[] h;
    if (!status && !eoi) status = ATTWARP_JPEGDEC_E_NO_EOI;
    uint32_t crc = 0;
    if (!status) crc = crc_bytes(reinterpret_cast<const uint8_t*>(coef2.data()), (int)(coef2.size() * 2));
    printf("%u %u", status, crc);
    for (uint32_t q = 0; q < nscans; ++q) printf(" %u %u %u %u %u", info[q * 5], info[q * 5 + 1], info[q * 5 + 2], info[q * 5 + 3], info[q * 5 + 4]);
    printf("\n");
    delete im;
  }
  fclose(f);
  return 0;
}
