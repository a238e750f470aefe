// Marker-less progressive scans of EVERY layout in parallel segments (jpegdec.hip's jpegscan_substream_kernel)
// as __host__ __device__ code: the four routes of jpegprog_sync_blocks.hpp moved onto the general MCU of jpegscan_blocks.hpp
// (JsScan records over JfImage frames: up to ten blocks per MCU, four components, four DC tables).  The same text runs
// inside the kernel and, under a sanitizer, in tests/jpegscan_sync_host_main.cpp; tests/jpegscan_sync_ref.py restates it.
//
// Geometry: block ordinal n of a scan is MCU n / nslot, slot n % nslot, and lies at js_block_index(im, sc, m, j): an
// interleaved scan walks the frame's MCUs, a scan of one component the blocks that cover its true size at its plane's pitch.
//
// The DC first pass and the period.  Several components may name one Huffman table (libjpeg gives all four of a CMYK file
// one), so a decoder entered at a guessed place can tell the slots of the MCU apart only by the tables they take: two
// decoders at the same bit whose slots differ by a multiple of the PERIOD P of the scan's table sequence (js_period) read the
// same bits for ever.  The state therefore carries the slot modulo P, a segment sums its DC differences by the block's place
// in the segment modulo nslot (ten sums), and the true slot, component and predictor of every block follow from the count
// of blocks in front of the segment, as its index does.  A scan is accepted only if every entry's slot is the count in front
// modulo P, which makes every table the segment took the true one.
//
// Nothing here sets a status or stores a coefficient before the scan is accepted.  Bounds by construction: every stream read
// goes through JdBits with the unit's end (the byte counts read data[i] below the unit's end only), every turn of a segment
// loop consumes a bit or ends a block, a slot is clamped below JF_MAX_SLOTS, a component or table index masked to 0..3 and
// held below `ntab`, every block index is checked against the image's blocks before a load or store and every mask / prefix
// index against the scan's block count.
#pragma once
#include <cstddef>
#include "jpegprog_sync_blocks.hpp"
#include "jpegscan_blocks.hpp"

namespace attwarp {

constexpr uint32_t JS_SYNC_MAGIC = 0x4745504fu;

struct JsSyncHeader {                  // behind the JsScan records of a table planned with sub-streams
  uint32_t magic, ncut;                // scans that are cut
  uint64_t info_off;                   // JpSyncInfo[nscans] in the scratch buffer, in the order the caller passed the scans
  uint32_t level_cut0[ATTWARP_JPEGDEC_MAX_SCANS + 2];     // the first workgroup of each level among all sub-stream workgroups
  uint32_t level_tables[ATTWARP_JPEGDEC_MAX_SCANS + 2];   // code tables the CUT scans of each level hold in LDS at most (1 .. 4)
};
static_assert(sizeof(JsSyncHeader) % 8 == 0, "record layout");

struct JsSync {                        // behind the header, one per scan record, in the records' order: JpSync and the period
  uint64_t seg_off;                    // JsSeg[nseg] in the scratch buffer
  uint64_t mask_off;                   // AC refinement: uint64 masks[nmcu], then uint32 prefix[nmcu + 1]
  uint32_t nseg;                       // planned segments; 0: the scan stays on one lane
  uint32_t segment_bytes, max_rounds;
  uint32_t slot;                       // its JpSyncInfo: the scan's position in the caller's array
  uint32_t cut;                        // record w: the scan record that sub-stream workgroup w decodes
  uint32_t period;                     // js_period of a cut DC first pass, else 1 (the JsScan record's bytes do not change)
  uint32_t pad[6];
};
static_assert(sizeof(JsSync) == 64, "record layout");

struct JsSeg {                         // per segment (scratch, 96 bytes): JpSeg with ten DC sums and four predictors
  JdSync entry;                        // first passes: the state at the segment's start (DC: the slot modulo the period).  AC
                                       // refinement: byte = data bits between the segment's first byte and the entry, bsk = the index
  JdSync exit;                         // the state at the first symbol that starts at or behind the segment's end
  uint32_t dirty;                      // the entry changed in the last round
  uint32_t nbeg;                       // DC first pass: blocks decoded.  Refinements: data bytes of the segment
  uint32_t nend;                       // blocks that end in the segment's decode, the blocks of EOB runs included (saturating)
  uint32_t eclean;                     // blocks that ended before its first error; JD_NO_ERROR: none
  uint32_t dc[JF_MAX_SLOTS];           // the wrapping sums of its DC differences by the block's place in the segment mod nslot
  uint32_t before;                     // blocks in front of the segment; AC refinement: the entry's block
  uint32_t pred[JF_MAX_COMP];          // the DC predictors at its start by the component's place in the scan; refinements: [0] the
                                       // entry's EOB run, [1] data bytes in front
  uint32_t pad;
};
static_assert(sizeof(JsSeg) == 96 && offsetof(JsSeg, dc) == 32 && offsetof(JsSeg, before) == 72, "segment layout");

struct JsSegOut {                      // what a first-pass decode of one segment leaves beside its DC sums
  JdSync exit;
  uint32_t nbeg, nend, eclean;
};

// Equal DC tables (counts, and symbols as far as the counts go) of the components at places a and b of a scan
JD_FN bool js_same_dc(const JsScan& sc, uint32_t a, uint32_t b) {
  a &= 3u; b &= 3u;
  if (a == b) return true;
  for (int l = 0; l < 16; ++l)
    if (sc.dc_counts[a][l] != sc.dc_counts[b][l]) return false;
  const int nd = jd_nsym(sc.dc_counts[a]);
  for (int k = 0; k < nd; ++k)
    if (sc.dc_symbols[a][k] != sc.dc_symbols[b][k]) return false;
  return true;
}
// The period of a DC first pass's table sequence: the smallest divisor P of nslot with equal tables in slots j and j + P
// for every j (jf_period's rule for a scan); 1 for every other kind, whose state carries no slot.
JD_FN uint32_t js_period(const JsScan& sc) {
  const uint32_t n = js_nslot(sc);
  if (sc.kind != JP_DC_FIRST) return 1u;
  for (uint32_t P = 1; P < n; ++P) {
    if (n % P) continue;
    bool same = true;
    for (uint32_t j = 0; j + P < n && same; ++j) same = js_same_dc(sc, sc.slot_t[j], sc.slot_t[j + P]);
    if (same) return P;
  }
  return n;
}
JD_FN uint32_t js_clamp_period(const JsScan& sc, uint32_t P) {
  const uint32_t n = js_nslot(sc);
  return P >= 1u && P <= n && n % P == 0u ? P : n;
}
// the table of slot j (< nslot) of a DC first pass, below the ntab tables the caller built
JD_FN uint32_t js_slot_table(const JsScan& sc, uint32_t j, uint32_t ntab) {
  const uint32_t t = sc.slot_t[j < (uint32_t)JF_MAX_SLOTS ? j : 0u] & 3u;
  return t < ntab ? t : 0u;
}

// ---- first passes: one segment from `entry` until the position reaches seg_end.  h: the scan's tables, ntab of them (an AC
// scan: h[0]); P: the period (DC).  dcsum[i * stride], i < nslot: zeroed here, then the DC sums by place.  An invalid code or a
// run past Se marks the decode, skips a bit and starts a new block.
JD_FN void js_first_segment(const JsScan& sc, uint32_t P, const uint8_t* p, uint32_t lo, const JdSync& entry, uint32_t seg_end, uint32_t uend,
                            const JdHuff* h, uint32_t ntab, JsSegOut& r, uint32_t* dcsum, uint32_t stride) {
  const bool dc = sc.kind == JP_DC_FIRST;
  const uint32_t nslot = js_nslot(sc), se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se);
  P = js_clamp_period(sc, P);
  JdBits br;
  jd_sync_open(br, p, lo, entry, uend);
  uint32_t q = (entry.bsk >> 8) & 255u, k = entry.bsk & 63u, place = 0;
  if (q >= P || !dc) q = 0;
  if (dc) k = 0;
  else if (k < ss || k > se) k = ss;
  r.nbeg = 0; r.nend = 0; r.eclean = JD_NO_ERROR;
  for (uint32_t i = 0; i < nslot; ++i) dcsum[i * stride] = 0;
  const uint32_t from = entry.byte < seg_end ? entry.byte : seg_end;
  const uint32_t limit = (seg_end - from) * 8u + 8u;
  bool at_end = false;
  for (uint32_t it = 0; it < limit; ++it) {
    br.refill();
    if (jp_reached(br, lo, seg_end)) break;
    uint32_t st, s = 0, v = 0, ended = 0;
    if (dc) {
      st = jd_symbol(br, h[js_slot_table(sc, q, ntab)], s);
      s &= 15u;
      if (!st && !br.bits(s, v)) st = ATTWARP_JPEGDEC_E_TRUNCATED;
      if (!st) {
        dcsum[place * stride] += (uint32_t)jd_extend(v, s);
        ++r.nbeg;
        ended = 1;
      }
    } else {
      uint32_t rs = 0;
      st = jd_symbol(br, h[0], rs);
      if (!st) {
        const uint32_t run = rs >> 4;
        s = rs & 15u;
        if (s == 0) {
          if (run == 15u) {
            if (k + 16u > se + 1u) st = ATTWARP_JPEGDEC_E_COEFF;
            else k += 16u;
          } else if (!br.bits(run, v)) st = ATTWARP_JPEGDEC_E_TRUNCATED;
          else ended = (1u << run) + v;                        // this block and the run's further blocks
        } else if (k + run > se) st = ATTWARP_JPEGDEC_E_COEFF;
        else if (!br.bits(s, v)) st = ATTWARP_JPEGDEC_E_TRUNCATED;
        else k += run + 1u;
      }
      if (!st && !ended && k > se) ended = 1;
    }
    if (st) {
      if (r.eclean == JD_NO_ERROR) r.eclean = r.nend;
      br.refill();
      if (st == (uint32_t)ATTWARP_JPEGDEC_E_TRUNCATED || br.cnt == 0) { at_end = true; break; }
      br.skip(1);
    } else if (ended) r.nend = jp_sat_add(r.nend, ended);
    if (st || ended) {
      q = q + 1u >= P ? 0u : q + 1u;
      place = place + 1u >= nslot ? 0u : place + 1u;
      k = dc ? 0u : ss;
    }
  }
  uint32_t byte = lo + uend, bit = 0;
  if (!at_end) jd_sync_position(br, lo, byte, bit);
  r.exit.byte = byte - lo;
  r.exit.bsk = bit << 16 | q << 8 | k;
}

// What the converged states must satisfy: `before` blocks end in front of the segment.  Bit 0: the segment contradicts a
// sequential decode of `expected` blocks; bit 1: block expected - 1 ends in this segment, cleanly (a run may overshoot it).
JD_FN uint32_t js_first_check(const JsScan& sc, uint32_t P, const JdSync& entry, uint32_t nend, uint32_t eclean, uint32_t before, uint32_t expected) {
  if (before >= expected) return 0u;                             // behind the last block: whatever follows it is tolerated
  P = js_clamp_period(sc, P);
  if (sc.kind == JP_DC_FIRST && ((entry.bsk >> 8) & 255u) != before % P) return 1u;
  const uint32_t last = expected - 1u - before;
  if (last < nend) return eclean > last ? 2u : 1u;
  return eclean == JD_NO_ERROR ? 0u : 1u;
}

// The DC sums of a segment by place -> by the component's place in the scan, `before` blocks in front: sums[0..3] += .
JD_FN void js_component_sums(const JsScan& sc, const uint32_t* dcsum, uint32_t before, uint32_t* sums) {
  const uint32_t nslot = js_nslot(sc);
  uint32_t j = before % nslot;
  for (uint32_t i = 0; i < nslot; ++i) {
    const uint32_t t = sc.slot_t[j] & 3u, d = dcsum[i];
    sums[0] += t == 0u ? d : 0u; sums[1] += t == 1u ? d : 0u; sums[2] += t == 2u ? d : 0u; sums[3] += t == 3u ? d : 0u;
    j = j + 1u >= nslot ? 0u : j + 1u;
  }
}

// The write pass of one segment from its TRUE entry: every symbol that starts in the segment.  before: blocks in front;
// pred[t * stride]: the predictors at its start (updated in place).  Blocks with ordinal >= expected are dropped.
JD_FN void js_first_write(const JsScan& sc, const JfImage& im, const uint8_t* p, uint32_t lo, const JdSync& entry, uint32_t seg_end,
                          uint32_t uend, const JdHuff* h, uint32_t ntab, uint32_t before, uint32_t* pred, uint32_t stride, uint32_t expected,
                          const uint8_t* zz, int16_t* coef) {
  if (before >= expected) return;
  const bool dc = sc.kind == JP_DC_FIRST;
  const uint32_t nslot = js_nslot(sc), se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se);
  const uint32_t al = jp_min(sc.al, 15u);
  JdBits br;
  jd_sync_open(br, p, lo, entry, uend);
  uint32_t k = entry.bsk & 63u, n = before;
  if (k < ss || k > se) k = ss;
  const uint32_t from = entry.byte < seg_end ? entry.byte : seg_end;
  const uint32_t limit = (seg_end - from) * 8u + 8u;
  for (uint32_t it = 0; it < limit && n < expected; ++it) {
    br.refill();
    if (jp_reached(br, lo, seg_end)) break;
    const uint32_t m = n / nslot, j = n - m * nslot;
    const uint32_t bi = js_block_index(im, sc, m, j);
    uint32_t s = 0, v = 0;
    if (dc) {
      const uint32_t t = js_slot_table(sc, j, ntab);
      if (jd_symbol(br, h[t], s)) return;
      s &= 15u;
      if (!br.bits(s, v)) return;
      const uint32_t pr = pred[t * stride] + (uint32_t)jd_extend(v, s);
      pred[t * stride] = pr;
      if (bi < im.nblocks) coef[(size_t)bi * 64u] = jp_low16(pr << al);
      ++n;
      continue;
    }
    uint32_t rs = 0;
    if (jd_symbol(br, h[0], rs)) return;
    const uint32_t run = rs >> 4;
    s = rs & 15u;
    if (s == 0) {
      if (run == 15u) {
        if (k + 16u > se + 1u) return;
        k += 16u;
      } else {
        if (!br.bits(run, v)) return;
        n = jp_sat_add(n, jp_min((1u << run) + v, JP_SYNC_CAP));
        k = ss;
        continue;
      }
    } else {
      if (k + run > se) return;
      if (!br.bits(s, v)) return;
      k += run;
      if (bi < im.nblocks) coef[(size_t)bi * 64u + (zz[k] & 63u)] = jp_low16((uint32_t)jd_extend(v, s) << al);
      ++k;
    }
    if (k > se) { ++n; k = ss; }
  }
}

// DC refinement, the write of one segment: data bit n is block n's; before: data bytes in front of the segment.
JD_FN void js_dc_refine_write(const JsScan& sc, const JfImage& im, const uint8_t* data, uint32_t from, uint32_t to, uint32_t before,
                              uint32_t expected, int16_t* coef) {
  const uint32_t nslot = js_nslot(sc), al = jp_min(sc.al, 15u);
  uint64_t n0 = (uint64_t)before * 8u;
  for (uint32_t i = from; i < to && n0 < expected; ++i) {
    const uint32_t b = data[i];
    if (b == 0u && i > 0u && data[i - 1u] == 0xffu) continue;
    for (uint32_t e = 0; e < 8u; ++e) {
      const uint64_t n = n0 + e;
      if (n >= expected || !((b >> (7u - e)) & 1u)) continue;
      const uint32_t m = (uint32_t)n / nslot, j = (uint32_t)n - m * nslot;
      const uint32_t bi = js_block_index(im, sc, m, j);
      if (bi < im.nblocks) coef[(size_t)bi * 64u] = jp_low16((uint32_t)(uint16_t)coef[(size_t)bi * 64u] | (1u << al));
    }
    n0 += 8u;
  }
}

// ---- AC refinement (a scan of one component: block n is js_block_index(im, sc, n, 0)) ----
// The exact skim by ONE lane: jp_refine_skim over this family's segment records.  mask[n] / P[n]: block n's in-band history
// and the bits set in front of block n (P[expected]: all), seg[s].pred[1]: data bytes in front of segment s.  Writes every
// segment's true entry: bits to skip, block, zigzag index, remaining run.  -> false: the one-lane route would report an error.
JD_FN bool js_refine_skim(const JsScan& sc, const uint8_t* p, uint32_t lo, uint32_t uend, const JdHuff& h, const uint64_t* mask,
                          const uint32_t* P, uint32_t expected, JsSeg* seg, uint32_t nseg) {
  const uint32_t se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se);
  JdBits br;
  br.init(p, 0xffffffffu, lo, lo + uend);
  uint64_t dbit = 0;
  uint32_t n = 0, k = ss, run = 0, snext = 0;
  for (;;) {                                                     // every turn consumes a bit or ends a block
    for (; snext < nseg && dbit >= (uint64_t)seg[snext].pred[1] * 8u; ++snext) {
      JsSeg& e = seg[snext];
      e.entry.byte = (uint32_t)(dbit - (uint64_t)e.pred[1] * 8u);
      e.entry.bsk = k;
      e.before = n;
      e.pred[0] = run;
    }
    if (n >= expected) break;
    if (run > 0u) {                                              // the blocks of a run: up to the next segment's first block
      const uint32_t rem = jp_min(run, expected - n);
      uint32_t j = rem;
      if (snext < nseg) {
        const uint64_t target = (uint64_t)seg[snext].pred[1] * 8u - dbit;      // > 0
        if ((uint64_t)(P[n + rem] - P[n]) >= target) {
          uint32_t a = 1, b = rem;                               // the smallest j with P[n + j] - P[n] >= target
          for (int it = 0; it < 32 && a < b; ++it) {
            const uint32_t mid = (a + b) >> 1;
            if ((uint64_t)(P[n + mid] - P[n]) >= target) b = mid;
            else a = mid + 1u;
          }
          j = a;
        }
      }
      const uint32_t nb = P[n + j] - P[n];
      if (!jp_skip_bits(br, nb)) return false;
      dbit += nb;
      n += j;
      run -= j;
      continue;
    }
    br.refill();
    const uint32_t c0 = br.cnt;
    uint32_t rs, v;
    if (jd_symbol(br, h, rs)) return false;
    dbit += c0 - br.cnt;
    uint32_t r = rs >> 4;
    const uint32_t s = rs & 15u;
    const uint64_t m = mask[n];
    if (s == 0u && r != 15u) {
      if (!br.bits(r, v)) return false;
      run = (1u << r) + v;
      const uint32_t nb = jp_popc64(m >> k);
      if (!jp_skip_bits(br, nb)) return false;
      dbit += r + nb;
      ++n; --run; k = ss;
      continue;
    }
    if (s != 0u) {
      if (s != 1u || !br.bits(1, v)) return false;
      dbit += 1u;
    }
    uint32_t nb = 0, kk = k;
    bool found = false;
    for (; kk <= se; ++kk) {
      if ((m >> kk) & 1u) ++nb;
      else if (r-- == 0u) { found = true; break; }
    }
    if (!found || !jp_skip_bits(br, nb)) return false;
    dbit += nb;
    k = kk + 1u;
    if (k > se) { ++n; k = ss; }
  }
  for (; snext < nseg; ++snext) {                                // segments behind the last block
    JsSeg& e = seg[snext];
    e.entry.byte = 0; e.entry.bsk = ss; e.before = expected; e.pred[0] = 0;
  }
  return true;
}

// The write of one segment from its true entry (block n0, index k0, run0 blocks of a run left, skip bits behind `start`, the
// segment's first raw byte) up to the next segment's entry (block n1, index k1).  A lane loads and stores only the in-band
// positions it visits; a block of a run without history costs nothing.
JD_FN void js_refine_write(const JsScan& sc, const JfImage& im, const uint8_t* p, uint32_t lo, uint32_t start, uint32_t uend, const JdHuff& h,
                           uint32_t n0, uint32_t k0, uint32_t run0, uint32_t skip, uint32_t n1, uint32_t k1, const uint64_t* mask,
                           uint32_t expected, const uint8_t* zz, int16_t* coef) {
  const uint32_t se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se), al = jp_min(sc.al, 15u);
  uint32_t n = n0, k = k0 & 63u, run = run0;
  if (n1 > expected) n1 = expected;
  if (k < ss || k > se) k = ss;
  if (!(n < n1 || (n == n1 && n < expected && k < k1))) return;
  JdBits br;
  br.init(p, 0xffffffffu, lo + jp_min(start, uend), lo + uend);
  if (!jp_skip_bits(br, skip)) return;
  while (n < n1 || (n == n1 && n < expected && k < k1)) {         // every turn consumes a bit or ends a block
    const uint64_t m = mask[n];
    const uint32_t bi = js_block_index(im, sc, n, 0);
    if (bi >= im.nblocks) return;
    int16_t* blk = coef + (size_t)bi * 64u;
    uint32_t rs = 0, v = 0, r = 0, s = 0;
    bool tail = run > 0u;                                        // the rest of the block takes correction bits only
    if (!tail) {
      if (jd_symbol(br, h, rs)) return;
      r = rs >> 4;
      s = rs & 15u;
      if (s == 0u && r != 15u) {
        if (!br.bits(r, v)) return;
        run = (1u << r) + v;
        tail = true;
      }
    }
    if (tail) {
      for (uint64_t left = m >> k << k; left; left &= left - 1u) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t kk = (uint32_t)__ffsll((unsigned long long)left) - 1u;
#else
        const uint32_t kk = (uint32_t)__builtin_ctzll(left);
#endif
        if (jp_correct(br, al, blk[zz[kk] & 63u])) return;
      }
      ++n; --run; k = ss;
      continue;
    }
    int16_t place = 0;
    if (s != 0u) {
      if (s != 1u || !br.bits(1, v)) return;
      place = jp_low16(v ? (1u << al) : 0u - (1u << al));
    }
    uint32_t kk = k;
    bool found = false;
    for (; kk <= se; ++kk) {
      if ((m >> kk) & 1u) {
        if (jp_correct(br, al, blk[zz[kk] & 63u])) return;
      } else if (r-- == 0u) { found = true; break; }
    }
    if (!found) return;
    if (s != 0u) blk[zz[kk] & 63u] = place;
    k = kk + 1u;
    if (k > se) { ++n; k = ss; }
  }
}

}  // namespace attwarp
