// Host-only driver of the layout scans' sub-stream core (attwarp_amd/csrc/jpegscan_sync_blocks.hpp) for
// tests/test_jpegscan_sync_host_cpu.py: the same text jpegscan_substream_kernel runs, compiled for the CPU with
// -fsanitize=address,undefined, with a host loop standing for the workgroup (rounds over all segments, then the sums).
// Usage: program corpus segment_bytes max_rounds.  The corpus is that of tests/jpegscan_host_main.cpp.
// Every file is decoded twice, scan by scan in file order: by js_decode_unit's sequential walk, and by the sub-stream routes
// with that walk where a scan is not cut or not accepted.  After every scan both coefficient memories must be equal, and a
// scan the sequential walk fails must not have been accepted: otherwise exit status 4.
// Prints per file: status, CRC-32 of the coefficients (0 unless the status is OK), then per scan
// "route segments rounds accepted crc": the record, and the CRC-32 of the coefficients behind the scan (0: the scan was not run).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegscan_sync_blocks.hpp"
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

// the workgroup of jpegscan_substream_kernel for one cut scan -> accepted; rounds: those it ran.  h: the scan's nh tables.
static bool substreams(const JfImage& im, const JsScan& sc, const uint8_t* data, uint32_t uend, uint32_t S, uint32_t max_rounds,
                       const JdHuff* h, uint32_t nh, int16_t* coef, uint32_t& rounds) {
  const uint32_t nslot = js_nslot(sc), nseg = (uend + S - 1) / S, expected = sc.nmcu * nslot;
  const uint32_t se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se), period = js_period(sc);
  std::vector<JsSeg> seg(nseg);
  std::memset(seg.data(), 0, nseg * sizeof(JsSeg));
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
          JsSegOut r;
          std::vector<uint32_t> acc(nslot);                    // exactly the sums the segment may write
          js_first_segment(sc, period, data, 0, seg[s].entry, jd_segment_end(s, S, uend), uend, h, nh, r, acc.data(), 1);
          seg[s].exit = r.exit; seg[s].nbeg = r.nbeg; seg[s].nend = r.nend; seg[s].eclean = r.eclean;
          for (uint32_t i = 0; i < nslot; ++i) seg[s].dc[i] = acc[i];
        }
      bool changed = false;
      for (uint32_t s = nseg; s-- > 0;) {                      // (downwards: every entry takes the exit of THIS round's decode)
        uint32_t d = 0;
        if (s > 0 && !jd_sync_equal(seg[s - 1].exit, seg[s].entry)) { seg[s].entry = seg[s - 1].exit; d = 1; changed = true; }
        seg[s].dirty = d;
      }
      if (!changed) { converged = true; break; }
    }
    uint32_t nb = 0, sum[JF_MAX_COMP] = {0, 0, 0, 0}, flags = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
      seg[s].before = nb;
      for (int c = 0; c < JF_MAX_COMP; ++c) seg[s].pred[c] = sum[c];
      flags |= js_first_check(sc, period, seg[s].entry, seg[s].nend, seg[s].eclean, nb, expected);
      if (sc.kind == JP_DC_FIRST) js_component_sums(sc, seg[s].dc, nb, sum);
      nb = jp_sat_add(nb, seg[s].nend);
    }
    if (!converged || !(flags & 2u) || (flags & 1u)) return false;
    for (uint32_t s = nseg; s-- > 0;) {                        // (any order: the lanes of a workgroup run side by side)
      uint32_t pred[JF_MAX_COMP];
      for (int c = 0; c < JF_MAX_COMP; ++c) pred[c] = seg[s].pred[c];
      js_first_write(sc, im, data, 0, seg[s].entry, jd_segment_end(s, S, uend), uend, h, nh, seg[s].before, pred, 1, expected, JD_ZIGZAG, coef);
    }
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
    for (uint32_t s = nseg; s-- > 0;) {
      const uint64_t b = (uint64_t)s * S;
      js_dc_refine_write(sc, im, data, b < uend ? (uint32_t)b : uend, jd_segment_end(s, S, uend), seg[s].pred[1], expected, coef);
    }
    return true;
  }
  if (nslot != 1u) return false;
  std::vector<uint64_t> mask(expected);                        // exactly as long as the scan's blocks
  std::vector<uint32_t> P(expected + 1);
  uint32_t bits = 0;
  for (uint32_t n = 0; n < expected; ++n) {
    const uint32_t bi = js_block_index(im, sc, n, 0);
    mask[n] = bi < im.nblocks ? jp_refine_mask(coef + (size_t)bi * 64, ss, se, JD_ZIGZAG) : 0;
    P[n] = bits;
    bits += jp_popc64(mask[n]);
  }
  P[expected] = bits;
  if (!js_refine_skim(sc, data, 0, uend, h[0], mask.data(), P.data(), expected, seg.data(), nseg)) return false;
  for (uint32_t s = nseg; s-- > 0;) {
    const uint32_t n1 = s + 1 < nseg ? seg[s + 1].before : expected, k1 = s + 1 < nseg ? seg[s + 1].entry.bsk & 63u : ss;
    js_refine_write(sc, im, data, 0, jd_segment_guess(data, s, S, uend).byte, uend, h[0], seg[s].before, seg[s].entry.bsk, seg[s].pred[0],
                    seg[s].entry.byte, n1, k1, mask.data(), expected, JD_ZIGZAG, coef);
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
    JfImage* im = new JfImage();
    const int W = (int)rd32(f), H = (int)rd32(f), ncomp = (int)rd32(f);
    int32_t hh[4], vv[4];
    for (int c = 0; c < 4; ++c) hh[c] = (int32_t)rd32(f);
    for (int c = 0; c < 4; ++c) vv[c] = (int32_t)rd32(f);
    const int color = (int)rd32(f);
    const uint32_t nscans = rd32(f), n = rd32(f);
    std::vector<uint8_t> data(n);                   // exactly as long as the data: the sanitizer sees any byte read outside it
    rdn(f, data.data(), n);
    if (jf_layout(*im, W, H, ncomp, hh, vv, color) != JF_OK) { fprintf(stderr, "file %u: layout refused\n", i); return 3; }
    const uint32_t blocks = im->nblocks;
    std::vector<int16_t> coef((size_t)blocks * 64, 0), coef2((size_t)blocks * 64, 0);
    std::vector<JsScan> scans(nscans);
    std::vector<std::vector<uint32_t>> starts(nscans), ends(nscans);
    uint32_t restart = 0;
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
    JdHuff* dc = new JdHuff[4];
    JdHuff* ac = new JdHuff[4];
    for (uint32_t q = 0; q < nscans && !status; ++q) {
      const JsScan& sc = scans[q];
      for (int t = 0; t < 4; ++t) { build(dc[t], sc.dc_counts[t], sc.dc_symbols[t]); build(ac[t], sc.ac_counts[t], sc.ac_symbols[t]); }
      const uint8_t* s = data.data() + sc.off;
      uint32_t err = 0;
      for (uint32_t k = 0; k < sc.nunits; ++k) {
        JdBits br;
        br.init(s, 0xffffffffu, starts[q][k], ends[q][k]);
        if (const uint32_t e = js_decode_unit(br, *im, sc, dc, ac, k, coef.data()))
          if (!err) err = e;
      }
      const uint32_t uend = ends[q][0], nseg = (uend + S - 1) / S;
      bool accepted = false;
      if (sc.kind <= JP_AC_REFINE && sc.nunits == 1 && uend >= 2 * S && nseg <= JP_SYNC_MAX_SEGS && (uint64_t)sc.nmcu * sc.nslot < JP_SYNC_CAP) {
        uint32_t rounds = 0;
        // exactly the tables the kernel builds for the scan: its DC tables for a DC first pass, one AC table for an AC scan
        const uint32_t nh = sc.kind == JP_DC_FIRST ? sc.ncomp : sc.kind == JP_DC_REFINE ? 0u : 1u;
        std::vector<JdHuff> h(nh);
        for (uint32_t t = 0; t < nh; ++t) h[t] = sc.kind == JP_DC_FIRST ? dc[t] : ac[t];
        accepted = substreams(*im, sc, s, uend, S, max_rounds, h.data(), nh, coef2.data(), rounds);
        info[q * 5] = 1 + sc.kind; info[q * 5 + 1] = nseg; info[q * 5 + 2] = rounds; info[q * 5 + 3] = accepted;
      }
      if (accepted && err) { fprintf(stderr, "file %u scan %u: accepted, but the sequential walk reports %u\n", i, q, err); return 4; }
      if (!accepted)
        for (uint32_t k = 0; k < sc.nunits; ++k) {
          JdBits br;
          br.init(s, 0xffffffffu, starts[q][k], ends[q][k]);
          js_decode_unit(br, *im, sc, dc, ac, k, coef2.data());
        }
      if (!err && std::memcmp(coef.data(), coef2.data(), coef.size() * 2) != 0) {
        fprintf(stderr, "file %u scan %u (kind %u, %u segments, accepted %d): coefficients differ\n", i, q, sc.kind, nseg, (int)accepted);
        return 4;
      }
      if (err) status = err;
      else info[q * 5 + 4] = crc_bytes(reinterpret_cast<const uint8_t*>(coef2.data()), (int)(coef2.size() * 2));
    }
    delete[] dc;
    delete[] ac;
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
