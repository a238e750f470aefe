// Marker-less progressive scans in parallel segments (jpegdec.hip's jpegprog_substream_kernel) as
// __host__ __device__ code, on top of the block routines of jpegprog_blocks.hpp and the JdSync machinery of
// jpegdec_blocks.hpp.  The same text runs inside the kernel and, under a sanitizer, in tests/jpegprog_sync_host_main.cpp.
//
// A scan of ONE unit is cut into byte segments, one lane each.  Four routes, by the scan's kind:
//   DC first pass   3.16's scheme with blocks of one DC symbol and its value: Jacobi rounds over guessed states (position,
//                   slot of the MCU), sums of blocks and DC differences, then 2-byte stores of low16(pred << Al);
//   AC first pass   the same with the state (position, zigzag index); an EOBn symbol ends its block and the run's further
//                   blocks at once, so the state carries no run; the write pass stores the non-zero coefficients only;
//   DC refinement   no code at all: block n's bit is data bit n; the segments' data bytes are counted and summed;
//   AC refinement   cannot self-synchronise (how many correction bits a block takes depends on which block it is), so one
//                   lane SKIMS the scan exactly, symbol by symbol, over bit masks of the coefficients with history and
//                   their prefix sums, without touching a coefficient, and notes every segment's true entry; then all
//                   lanes decode their segments from those entries with jp_ac_refine's arithmetic.
// Nothing here sets a status or stores a coefficient before the scan is accepted.
//
// Bounds by construction: every stream read goes through JdBits with the unit's end (the byte counts read data[i] for i
// below the unit's end only), every turn of a segment loop consumes a bit or ends a block, every block index is checked
// against the image's blocks before a store and every mask / prefix index against the scan's block count.
#pragma once
#include "jpegprog_blocks.hpp"

namespace attwarp {

constexpr uint32_t JP_SYNC_MAGIC = 0x4745504eu;
constexpr uint32_t JP_SYNC_MAX_SEGS = 1u << 14;
constexpr uint32_t JP_SYNC_CAP = 1u << 24;     // block counts saturate here (an image has fewer blocks): sums never wrap

struct JpSyncHeader {                  // behind the scan records of a table planned with sub-streams
  uint32_t magic, ncut;                // scans that are cut
  uint64_t info_off;                   // JpSyncInfo[nscans] in the scratch buffer, in the order the caller passed the scans
  uint32_t level_cut0[ATTWARP_JPEGDEC_MAX_SCANS + 2];   // the first workgroup of each level among all sub-stream workgroups
};
static_assert(sizeof(JpSyncHeader) % 8 == 0, "record layout");

struct JpSync {                        // behind the header, one per scan record, in the records' order
  uint64_t seg_off;                    // JpSeg[nseg] in the scratch buffer
  uint64_t mask_off;                   // AC refinement: uint64 masks[nmcu], then uint32 prefix[nmcu + 1]
  uint32_t nseg;                       // planned segments; 0: the scan stays on one lane
  uint32_t segment_bytes, max_rounds;
  uint32_t slot;                       // its JpSyncInfo: the scan's position in the caller's array
  uint32_t cut;                        // record w: the scan record that sub-stream workgroup w decodes
  uint32_t pad[7];
};
static_assert(sizeof(JpSync) == 64, "record layout");

struct JpSyncInfo {                    // per scan (scratch), written on every run
  uint32_t route;                      // 0: one lane; 1 + JP_DC_FIRST .. 1 + JP_AC_REFINE
  uint32_t nseg, rounds, accepted;
  uint32_t ticks[3];                   // 100 MHz ticks of the workgroup's three parts: first passes rounds / sums and checks / write,
                                       // refinements counts and masks / skim (a DC refinement: none) / write
  uint32_t pad;
};
static_assert(sizeof(JpSyncInfo) == 32, "record layout");

struct JpSeg {                         // per segment (scratch, 64 bytes)
  JdSync entry;                        // first passes: the state at the segment's start.  AC refinement: byte = data bits between
                                       // the segment's first byte and the entry, bsk = the zigzag index
  JdSync exit;                         // the state at the first symbol that starts at or behind the segment's end
  uint32_t dirty;                      // the entry changed in the last round
  uint32_t nbeg;                       // DC first pass: blocks decoded.  Refinements: data bytes of the segment
  uint32_t nend;                       // blocks that end in the segment's decode, the blocks of EOB runs included (saturating)
  uint32_t eclean;                     // blocks that ended before its first error; JD_NO_ERROR: none
  uint32_t dc[3];                      // per table of the scan, the wrapping sum of the segment's DC differences
  uint32_t before;                     // blocks in front of the segment; AC refinement: the entry's block
  uint32_t pred[3];                    // the DC predictors at its start; refinements: [0] the entry's EOB run, [1] data bytes in front
  uint32_t pad;
};
static_assert(sizeof(JpSeg) == 64, "segment layout");

JD_FN uint32_t jp_sat_add(uint32_t a, uint32_t b) { return a + b < JP_SYNC_CAP ? a + b : JP_SYNC_CAP; }   // (a, b <= JP_SYNC_CAP)
JD_FN uint32_t jp_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// the reader stands at or behind raw byte seg_end of the scan's data
JD_FN bool jp_reached(const JdBits& br, uint32_t lo, uint32_t seg_end) {
  if (br.pos - ((br.cnt + 7u) >> 3) < lo + seg_end) return false;          // (an upper bound of the position)
  uint32_t byte, bit;
  jd_sync_position(br, lo, byte, bit);
  return byte >= lo + seg_end;
}

// ---- first passes: one segment from `entry` until the position reaches seg_end (jd_decode_segment for blocks of one DC
// symbol, or of AC symbols of the band).  h: the scan's tables.  An invalid code or a run past Se marks the decode, skips a
// bit and starts a new block.
JD_FN void jp_first_segment(const JpScan& sc, const uint8_t* p, uint32_t lo, const JdSync& entry, uint32_t seg_end, uint32_t uend,
                            const JdHuff* h, JpSeg& r) {
  const bool dc = sc.kind == JP_DC_FIRST;
  const uint32_t nslot = sc.nslot >= 1u && sc.nslot <= 6u ? sc.nslot : 1u, se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se);
  JdBits br;
  jd_sync_open(br, p, lo, entry, uend);
  uint32_t slot = (entry.bsk >> 8) & 255u, k = entry.bsk & 63u;
  if (slot >= nslot || !dc) slot = 0;
  if (dc) k = 0;
  else if (k < ss || k > se) k = ss;
  r.nbeg = 0; r.nend = 0; r.eclean = JD_NO_ERROR;
  r.dc[0] = r.dc[1] = r.dc[2] = 0;
  const uint32_t from = entry.byte < seg_end ? entry.byte : seg_end;
  const uint32_t limit = (seg_end - from) * 8u + 8u;
  bool at_end = false;
  for (uint32_t it = 0; it < limit; ++it) {
    br.refill();
    if (jp_reached(br, lo, seg_end)) break;
    uint32_t st, s = 0, v = 0, ended = 0;
    if (dc) {
      const uint32_t t = sc.slot_t[slot & 7u] % 3u;
      st = jd_symbol(br, h[t], s);
      s &= 15u;
      if (!st && !br.bits(s, v)) st = ATTWARP_JPEGDEC_E_TRUNCATED;
      if (!st) {
        r.dc[t] += (uint32_t)jd_extend(v, s);
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
      slot = slot + 1u >= nslot ? 0u : slot + 1u;
      k = dc ? 0u : ss;
    }
  }
  uint32_t byte = lo + uend, bit = 0;
  if (!at_end) jd_sync_position(br, lo, byte, bit);
  r.exit.byte = byte - lo;
  r.exit.bsk = bit << 16 | slot << 8 | k;
}

// What the converged states must satisfy: `before` blocks end in front of the segment.  Bit 0: the segment contradicts a
// sequential decode of `expected` blocks; bit 1: block expected - 1 ends in this segment, cleanly (a run may overshoot it).
JD_FN uint32_t jp_first_check(const JpScan& sc, const JdSync& entry, const JpSeg& r, uint32_t before, uint32_t expected) {
  if (before >= expected) return 0u;                             // behind the last block: whatever follows it is tolerated
  const uint32_t nslot = sc.nslot >= 1u && sc.nslot <= 6u ? sc.nslot : 1u;
  if (sc.kind == JP_DC_FIRST && ((entry.bsk >> 8) & 255u) != before % nslot) return 1u;
  const uint32_t last = expected - 1u - before;
  if (last < r.nend) return r.eclean > last ? 2u : 1u;
  return r.eclean == JD_NO_ERROR ? 0u : 1u;
}

// The write pass of one segment from its TRUE entry: every symbol that starts in the segment.  before: blocks in front;
// pred0: the predictors at its start.  Blocks with ordinal >= expected are dropped.  Stores 2 bytes per coefficient.
JD_FN void jp_first_write(const JpScan& sc, const JdImage& im, const uint8_t* p, uint32_t lo, const JdSync& entry, uint32_t seg_end,
                          uint32_t uend, const JdHuff* h, uint32_t before, const uint32_t* pred0, uint32_t expected, const uint8_t* zz,
                          int16_t* coef) {
  if (before >= expected) return;
  const bool dc = sc.kind == JP_DC_FIRST;
  const uint32_t nslot = sc.nslot >= 1u && sc.nslot <= 6u ? sc.nslot : 1u, se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se);
  const uint32_t al = jp_min(sc.al, 15u);
  JdBits br;
  jd_sync_open(br, p, lo, entry, uend);
  uint32_t k = entry.bsk & 63u, n = before;
  if (k < ss || k > se) k = ss;
  uint32_t pred[3] = {pred0[0], pred0[1], pred0[2]};
  const uint32_t from = entry.byte < seg_end ? entry.byte : seg_end;
  const uint32_t limit = (seg_end - from) * 8u + 8u;
  for (uint32_t it = 0; it < limit && n < expected; ++it) {
    br.refill();
    if (jp_reached(br, lo, seg_end)) break;
    const uint32_t m = n / nslot, j = n - m * nslot;
    const uint32_t bi = jp_block_index(im, sc, m, j);
    uint32_t s = 0, v = 0;
    if (dc) {
      const uint32_t t = sc.slot_t[j & 7u] % 3u;
      if (jd_symbol(br, h[t], s)) return;
      s &= 15u;
      if (!br.bits(s, v)) return;
      pred[t] += (uint32_t)jd_extend(v, s);
      if (bi < im.nblocks) coef[(size_t)bi * 64u] = jp_low16(pred[t] << al);
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

// ---- refinements: the data bytes among raw bytes from .. to of the scan's data (to <= the unit's end): every byte but the
// 00 behind an FF, an FF 00 pair across `from` counted once ----
JD_FN uint32_t jp_data_bytes(const uint8_t* data, uint32_t from, uint32_t to) {
  uint32_t n = 0;
  for (uint32_t i = from; i < to; ++i) n += !(data[i] == 0u && i > 0u && data[i - 1u] == 0xffu);
  return n;
}

// DC refinement, the write of one segment: data bit n is block n's; before: data bytes in front of the segment.
JD_FN void jp_dc_refine_write(const JpScan& sc, const JdImage& im, const uint8_t* data, uint32_t from, uint32_t to, uint32_t before,
                              uint32_t expected, int16_t* coef) {
  const uint32_t nslot = sc.nslot >= 1u && sc.nslot <= 6u ? sc.nslot : 1u, al = jp_min(sc.al, 15u);
  uint64_t n0 = (uint64_t)before * 8u;
  for (uint32_t i = from; i < to && n0 < expected; ++i) {
    const uint32_t b = data[i];
    if (b == 0u && i > 0u && data[i - 1u] == 0xffu) continue;
    for (uint32_t e = 0; e < 8u; ++e) {
      const uint64_t n = n0 + e;
      if (n >= expected || !((b >> (7u - e)) & 1u)) continue;
      const uint32_t m = (uint32_t)n / nslot, j = (uint32_t)n - m * nslot;
      const uint32_t bi = jp_block_index(im, sc, m, j);
      if (bi < im.nblocks) coef[(size_t)bi * 64u] = jp_low16((uint32_t)(uint16_t)coef[(size_t)bi * 64u] | (1u << al));
    }
    n0 += 8u;
  }
}

// AC refinement: the coefficients of a block (natural order) that are not zero, by zigzag position, inside the band
JD_FN uint64_t jp_refine_mask(const int16_t* blk, uint32_t ss, uint32_t se, const uint8_t* zz) {
  uint64_t m = 0;
  for (uint32_t k = ss; k <= se && k < 64u; ++k)
    if (blk[zz[k] & 63u] != 0) m |= (uint64_t)1 << k;
  return m;
}
JD_FN uint32_t jp_popc64(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(m);
#else
  return (uint32_t)__builtin_popcountll(m);
#endif
}
JD_FN bool jp_skip_bits(JdBits& br, uint32_t n) {                // every turn consumes a bit
  while (n > 0u) {
    br.refill();
    if (br.cnt == 0u) return false;
    const uint32_t t = n < br.cnt ? n : br.cnt;
    br.skip(t);
    n -= t;
  }
  return true;
}
JD_FN uint32_t jp_ac_block_index(const JdImage& im, const JpScan& sc, uint32_t n) { return jp_block_index(im, sc, n, 0); }

// The exact skim by ONE lane: the scan's symbols from its first bit, no coefficient touched.  mask[n] / P[n]: block n's
// in-band history and the bits set in front of block n (P[expected]: all), seg[s].pred[1]: data bytes in front of segment
// s.  Writes every segment's true entry (the first symbol, or block of an EOB run, that starts at or behind the segment's
// first data bit): bits to skip, block, zigzag index, remaining run.  -> false: the one-lane route would report an error.
JD_FN bool jp_refine_skim(const JpScan& sc, const uint8_t* p, uint32_t lo, uint32_t uend, const JdHuff& h, const uint64_t* mask,
                          const uint32_t* P, uint32_t expected, JpSeg* seg, uint32_t nseg) {
  const uint32_t se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se);
  JdBits br;
  br.init(p, 0xffffffffu, lo, lo + uend);
  uint64_t dbit = 0;
  uint32_t n = 0, k = ss, run = 0, snext = 0;
  for (;;) {                                                     // every turn consumes a bit or ends a block
    for (; snext < nseg && dbit >= (uint64_t)seg[snext].pred[1] * 8u; ++snext) {
      JpSeg& e = seg[snext];
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
    JpSeg& e = seg[snext];
    e.entry.byte = 0; e.entry.bsk = ss; e.before = expected; e.pred[0] = 0;
  }
  return true;
}

// The write of one segment from its true entry `e` up to the next segment's entry (block n1, index k1); start: the segment's
// first raw byte.  A lane loads and stores only the in-band positions it visits; a block of a run without history costs nothing.
JD_FN void jp_refine_write(const JpScan& sc, const JdImage& im, const uint8_t* p, uint32_t lo, uint32_t start, uint32_t uend, const JdHuff& h,
                           const JpSeg& e, uint32_t n1, uint32_t k1, const uint64_t* mask, uint32_t expected, const uint8_t* zz,
                           int16_t* coef) {
  const uint32_t se = jp_min(sc.se, 63u), ss = jp_min(sc.ss, se), al = jp_min(sc.al, 15u);
  uint32_t n = e.before, k = e.entry.bsk & 63u, run = e.pred[0];
  if (n1 > expected) n1 = expected;
  if (k < ss || k > se) k = ss;
  if (!(n < n1 || (n == n1 && n < expected && k < k1))) return;
  JdBits br;
  br.init(p, 0xffffffffu, lo + jp_min(start, uend), lo + uend);
  if (!jp_skip_bits(br, e.entry.byte)) return;
  while (n < n1 || (n == n1 && n < expected && k < k1)) {         // every turn consumes a bit or ends a block
    const uint64_t m = mask[n];
    const uint32_t bi = jp_ac_block_index(im, sc, n);
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
