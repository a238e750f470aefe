// The wave route of the PNG decoder (pngdec.hip) as __host__ __device__ code: one wave inflates one zlib
// stream with all 64 lanes.  The same text runs in pngdec_wave_kernel and, with a host loop in place of the wave and under
// a sanitizer, in tests/pngwave_host_main.cpp; tests/pngwave_ref.py restates it in the bit domain.
//
// Inside a Huffman block a WINDOW of 64 segments of seg_bytes stream bytes is decoded by 64 lanes at once.  The state at a
// segment's entry is one number, the bit position of the next literal / length code; segment 0 enters at the true
// position, every other one guesses its own first bit, and in Jacobi rounds every lane whose entry changed decodes from
// its entry to its exit (the first token that STARTS behind its segment) and hands the exit to the next lane.  After round
// r the entries of segments 0 .. r are the serial decoder's, so a fixed point IS the serial decode and 64 rounds suffice.
// A second pass over the true chain writes literals into a staging buffer and records the matches, which are resolved in
// rounds out of the staging buffer and a 32 KiB ring that always holds the last 32768 output bytes; the ring is flushed to
// the image's filtered bytes in 16-byte stores, and what enters it is summed for the stream's Adler-32.  Anything that does
// not check out leaves accepted = 0, and the lane route (pd_inflate from the stream's start) decodes the image and states
// its status.
//
// Bounds: every stream read goes through PdBits, every table index is masked as in pd_decode, every staged byte and match
// record is checked against the buffer's capacity, every flushed byte against filt_bytes, every distance against the bytes
// produced.  Every loop consumes a bit, produces a byte or retires a match; rounds are at most max_rounds.
#pragma once
#include "pngdec_blocks.hpp"

namespace attwarp {

constexpr int PW_WAVE = 64;
constexpr uint32_t PW_RING = 32768, PW_STAGE = 8192, PW_MATCHES = 1024, PW_STORED_CHUNK = 16384;
constexpr uint32_t PW_NONE = 0xffffffffu;
constexpr uint32_t PW_MAX_STREAM = 1u << 28;             // bit positions are uint32: longer streams stay on the lane route

struct PwMatch { uint32_t dst; uint16_t len, dist; };    // dst: offset in the staging buffer; dist <= 32768
struct PwRecord { uint32_t windows, rounds, accepted, resolution_rounds; };   // per image, behind the filtered bytes (scratch)
struct PwCode { uint32_t first[16], start[16], nsym; };  // per code length: the first canonical code, the first sorted symbol

struct alignas(16) PwShared {
  uint8_t ring[PW_RING];                                 // output byte q stands at ring[q & (PW_RING - 1)]
  uint8_t stage[PW_STAGE];                               // the bytes of one run, before they enter the ring
  PwMatch match[PW_MATCHES];
  PdTables tb, fx;                                       // the dynamic block's tables / the fixed block's, built once
  PwCode cl, cd;
  // per lane: the round state ...
  uint32_t entry[PW_WAVE], exit_[PW_WAVE], nbytes[PW_WAVE], nmatch[PW_WAVE], eob0[PW_WAVE], eob1[PW_WAVE], err[PW_WAVE], dirty[PW_WAVE];
  // ... and the write pass: cursor and stop bit, what is left, the run's offsets and budgets, what the run emitted
  uint32_t cur[PW_WAVE], stop[PW_WAVE], roff[PW_WAVE], moff[PW_WAVE], bbud[PW_WAVE], mbud[PW_WAVE], emb[PW_WAVE], emm[PW_WAVE];
  uint32_t mdone[PW_WAVE], pend[PW_WAVE];
  unsigned long long ad_a[PW_WAVE], ad_w[PW_WAVE];        // Adler-32 of what entered the ring: sums of bytes / of byte * weight
  // what lane 0 decides for the wave
  uint32_t bit, produced, flushed, fail, bad, bfinal, btype, have_fixed;
  uint32_t st_at, st_len, nlen, ndist, changed, nl, blockend, run_a, run_b, run_bytes, low;
  uint32_t windows, rounds, res_rounds;
};
static_assert(sizeof(PwShared) < 64 * 1024, "the wave route's LDS stays below the 64 KiB that need no grant");

// "every lane does this, then the wave meets": the kernel's lane is threadIdx.x and the meeting a barrier of its one wave;
// the host program runs the lanes one after the other.  The code between two such loops is uniform.
#if defined(__HIP_DEVICE_COMPILE__)
#define PW_EACH(lane) for (int lane = (int)threadIdx.x, pw_once = 1; pw_once; pw_once = 0, __syncthreads())
#else
#define PW_EACH(lane) for (int lane = 0; lane < PW_WAVE; ++lane)
#endif

// output byte x at position q enters the ring: the lane's share of S1 and S2 (pd_adler_finish has the weights)
PD_FN void pw_ring_put(PwShared& S, int lane, uint32_t q, uint32_t x, uint32_t filt_bytes) {
  S.ring[q & (PW_RING - 1u)] = (uint8_t)x;
  S.ad_a[lane] += x;
  S.ad_w[lane] += (unsigned long long)x * (filt_bytes - q);  // (q < filt_bytes: the callers checked the sizes)
}

PD_FN uint32_t pw_bitpos(const PdBits& br) { return 8u * br.pos - br.cnt; }
PD_FN void pw_seek(PdBits& br, const uint8_t* s, uint32_t n, uint32_t bit) {   // bit < 8 n
  br.init(s, n, bit >> 3);
  uint32_t v;
  if (bit & 7u) br.bits(bit & 7u, v);
}

// One token.  0: literal a; 1: a match of a bytes at distance b; 2: the end-of-block code; 16 + status: an error.
PD_FN uint32_t pw_token(PdBits& br, const PdTables& T, uint32_t& a, uint32_t& b) {
  uint32_t sym, v = 0, base, eb;
  if (const uint32_t rc = pd_decode(br, T.lit, PD_LBITS, T.hl, sym)) return 16u + rc;
  if (sym < 256) { a = sym; return 0; }
  if (sym == 256) return 2;
  sym -= 257;
  if (sym >= 29) return 16u + ATTWARP_PNGDEC_E_SYMBOL;
  pd_length_base(sym, base, eb);
  if (!br.bits(eb, v)) return 16u + ATTWARP_PNGDEC_E_TRUNCATED;
  a = base + v;
  if (const uint32_t rc = pd_decode(br, T.dist, PD_DBITS, T.hd, sym)) return 16u + rc;
  if (sym >= 30) return 16u + ATTWARP_PNGDEC_E_SYMBOL;
  pd_dist_base(sym, base, eb);
  if (!br.bits(eb, v)) return 16u + ATTWARP_PNGDEC_E_TRUNCATED;
  b = base + v;
  return 1;
}

// ---- tables by the whole wave -------------------------------------------------------------------------------------------------
// pd_build's first half on one lane: counts, the acceptance rules, the sorted symbols; and per length the first code and
// the first sorted index, from which every lane finds the code of any sorted symbol on its own.
PD_FN uint32_t pw_count(const uint8_t* lens, int n, PdHuff& h, PwCode& c, bool allow_single) {
  for (int l = 0; l < 16; ++l) h.count[l] = 0;
  for (int i = 0; i < n; ++i) ++h.count[lens[i] & 15];
  int left = 1, maxl = 0;
  for (int l = 1; l < 16; ++l) {
    left = 2 * left - (int)h.count[l];
    if (left < 0) return ATTWARP_PNGDEC_E_CODE_LENGTHS;
    if (h.count[l]) maxl = l;
  }
  if (left > 0 && !(allow_single && maxl <= 1)) return ATTWARP_PNGDEC_E_CODE_LENGTHS;
  uint16_t offs[16];
  offs[0] = 0; offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
  for (int i = 0; i < n; ++i) {
    const int l = lens[i] & 15;
    if (l) h.symbol[offs[l]++] = (uint16_t)i;
  }
  uint32_t code = 0, idx = 0;
  c.first[0] = 0; c.start[0] = 0;
  for (int l = 1; l < 16; ++l) {
    c.first[l] = code;
    c.start[l] = idx;
    code = (code + h.count[l]) << 1;
    idx += h.count[l];
  }
  c.nsym = idx;                                            // <= n <= 288
  return ATTWARP_PNGDEC_OK;
}
// pd_build's second half, one sorted symbol per lane and step: a short code fills its 2^(pbits - l) entries, a long one marks
// its index.  No two codes write one entry with different values (the code is prefix-free), so the order does not matter.
PD_FN void pw_fill(int lane, const uint8_t* lens, const PdHuff& h, const PwCode& c, uint16_t* primary, int pbits) {
  const uint32_t size = 1u << pbits;
  for (uint32_t idx = (uint32_t)lane; idx < c.nsym; idx += PW_WAVE) {
    const uint32_t sym = h.symbol[idx] % 288u, l = lens[sym] & 15u;
    const uint32_t r = pd_rev(c.first[l] + (idx - c.start[l]), (int)l);
    if (l == 0) continue;                                  // (never: sorted symbols have a length)
    if ((int)l <= pbits) {
      const uint16_t e = (uint16_t)((sym << 4) | l);
      for (uint32_t j = r & (size - 1u); j < size; j += 1u << l) primary[j] = e;
    } else {
      primary[r & (size - 1u)] = (uint16_t)PD_LONG;
    }
  }
}

// A dynamic block's header behind its three bits, as pd_inflate reads it: lengths into tb.lens.  0, or the status.
PD_FN uint32_t pw_read_lengths(PdBits& br, PdTables& tb, uint32_t& nlen, uint32_t& ndist) {
  uint32_t v = 0;
  if (!br.bits(14, v)) return ATTWARP_PNGDEC_E_TRUNCATED;
  nlen = 257u + (v & 31u);
  ndist = 1u + ((v >> 5) & 31u);
  const uint32_t ncode = 4u + (v >> 10);
  if (nlen > 286u || ndist > 30u) return ATTWARP_PNGDEC_E_CODE_LENGTHS;
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (int i = 0; i < 19; ++i) tb.lens[i] = 0;
  for (uint32_t i = 0; i < ncode; ++i) {
    if (!br.bits(3, v)) return ATTWARP_PNGDEC_E_TRUNCATED;
    tb.lens[order[i]] = (uint8_t)v;
  }
  if (pd_build(tb.lens, 19, tb.hl, tb.lit, PD_CBITS, false)) return ATTWARP_PNGDEC_E_CODE_LENGTHS;
  const uint32_t total = nlen + ndist;                     // <= 316
  uint32_t i = 0;
  while (i < total) {                                      // every pass adds at least one length
    uint32_t sym;
    if (const uint32_t rc = pd_decode(br, tb.lit, PD_CBITS, tb.hl, sym)) return rc == ATTWARP_PNGDEC_E_SYMBOL ? (uint32_t)ATTWARP_PNGDEC_E_CODE_LENGTHS : rc;
    if (sym < 16) { tb.lens[i++] = (uint8_t)sym; continue; }
    uint32_t rep, val = 0;
    if (sym == 16) {
      if (i == 0) return ATTWARP_PNGDEC_E_CODE_LENGTHS;
      val = tb.lens[i - 1];
      if (!br.bits(2, v)) return ATTWARP_PNGDEC_E_TRUNCATED;
      rep = 3 + v;
    } else if (sym == 17) {
      if (!br.bits(3, v)) return ATTWARP_PNGDEC_E_TRUNCATED;
      rep = 3 + v;
    } else {
      if (!br.bits(7, v)) return ATTWARP_PNGDEC_E_TRUNCATED;
      rep = 11 + v;
    }
    if (i + rep > total) return ATTWARP_PNGDEC_E_CODE_LENGTHS;
    for (uint32_t k = 0; k < rep; ++k) tb.lens[i++] = (uint8_t)val;
  }
  if (tb.lens[256] == 0) return ATTWARP_PNGDEC_E_CODE_LENGTHS;
  return ATTWARP_PNGDEC_OK;
}

// Lane 0 at a block's start: the three header bits, a stored block's LEN / NLEN and bounds as pd_inflate checks them, a
// dynamic block's lengths and the serial halves of its two tables.  Leaves S.bit on the first symbol (a stored block's first
// byte is S.st_at); any status is S.fail: the lane route will state it.
PD_FN void pw_header(PwShared& S, const uint8_t* s, uint32_t n, uint32_t filt_bytes) {
  if (S.bit >= 8u * n) { S.fail = 1; return; }
  PdBits br;
  pw_seek(br, s, n, S.bit);
  uint32_t hdr = 0;
  if (!br.bits(3, hdr)) { S.fail = 1; return; }
  S.bfinal = hdr & 1u;
  S.btype = hdr >> 1;
  if (S.btype == 3) { S.fail = 1; return; }
  if (S.btype == 0) {
    uint32_t at = (pw_bitpos(br) + 7u) >> 3;
    if (at + 4u > n) { S.fail = 1; return; }
    const uint32_t len = s[at] | (uint32_t)s[at + 1] << 8, nlen = s[at + 2] | (uint32_t)s[at + 3] << 8;
    at += 4;
    if ((len ^ nlen) != 0xffffu || len > n - at || len > filt_bytes - S.produced) { S.fail = 1; return; }
    S.st_at = at;
    S.st_len = len;
    S.bit = 8u * (at + len);
    return;
  }
  if (S.btype == 2) {
    if (pw_read_lengths(br, S.tb, S.nlen, S.ndist)) { S.fail = 1; return; }
    if (pw_count(S.tb.lens + S.nlen, (int)S.ndist, S.tb.hd, S.cd, true) || pw_count(S.tb.lens, (int)S.nlen, S.tb.hl, S.cl, true)) { S.fail = 1; return; }
  } else if (!S.have_fixed) {
    for (int i = 0; i < 288; ++i) S.fx.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = 0; i < 32; ++i) S.fx.lens[288 + i] = 5;
    pw_count(S.fx.lens + 288, 32, S.fx.hd, S.cd, false);
    pw_count(S.fx.lens, 288, S.fx.hl, S.cl, false);
  }
  S.bit = pw_bitpos(br);
}

// ---- a segment ----------------------------------------------------------------------------------------------------------------
// Round work of one lane: from its entry over every token that starts in front of segend.  Counts bytes and matches, notes the
// first end-of-block code (where it starts and ends; the counts are those in front of it) or the first error, and stops there.
PD_FN void pw_scan(PwShared& S, int lane, const uint8_t* s, uint32_t n, const PdTables& T, uint32_t segend) {
  const uint32_t e = S.entry[lane];
  uint32_t nb = 0, nm = 0, ex = PW_NONE, e0 = PW_NONE, e1 = PW_NONE, er = 0;
  if (e != PW_NONE) {
    if (e >= 8u * n) {
      er = 1;
    } else {
      PdBits br;
      pw_seek(br, s, n, e);
      for (;;) {                                           // every token consumes at least one bit
        const uint32_t at = pw_bitpos(br);
        if (at >= segend) { ex = at; break; }
        uint32_t a = 0, b = 0;
        const uint32_t k = pw_token(br, T, a, b);
        if (k == 0) { ++nb; }
        else if (k == 1) { nb += a; ++nm; }
        else if (k == 2) { e0 = at; e1 = pw_bitpos(br); break; }
        else { er = 1; break; }
      }
    }
  }
  S.exit_[lane] = ex; S.nbytes[lane] = nb; S.nmatch[lane] = nm; S.eob0[lane] = e0; S.eob1[lane] = e1; S.err[lane] = er;
}

// Write pass of one lane of a run: from its cursor to its stop bit, or until the next token would pass a budget.  Literals go
// to the staging buffer, matches are recorded; a match that starts before the image's first byte raises S.bad.
PD_FN void pw_emit(PwShared& S, int lane, const uint8_t* s, uint32_t n, const PdTables& T) {
  const uint32_t stop = S.stop[lane], ro = S.roff[lane], mo = S.moff[lane], bb = S.bbud[lane], mb = S.mbud[lane];
  uint32_t cursor = S.cur[lane], ob = 0, om = 0;
  if (cursor < stop && cursor < 8u * n) {
    PdBits br;
    pw_seek(br, s, n, cursor);
    for (;;) {
      cursor = pw_bitpos(br);
      if (cursor >= stop) break;
      uint32_t a = 0, b = 0;
      const uint32_t k = pw_token(br, T, a, b);
      if (k == 0) {
        if (ob + 1u > bb || ro + ob >= PW_STAGE) break;
        S.stage[ro + ob] = (uint8_t)a;
        ++ob;
      } else if (k == 1) {
        if (ob + a > bb || om + 1u > mb || ro + ob + a > PW_STAGE || mo + om >= PW_MATCHES) break;
        if (b > S.produced + ro + ob) S.bad = 1;
        PwMatch m;
        m.dst = ro + ob; m.len = (uint16_t)a; m.dist = (uint16_t)b;
        S.match[mo + om] = m;
        ob += a;
        ++om;
      } else {                                             // (never: the rounds saw this chain clean)
        S.bad = 1;
        break;
      }
    }
  }
  S.cur[lane] = cursor; S.emb[lane] = ob; S.emm[lane] = om; S.mdone[lane] = 0;
}

// One resolution round of one lane: its pending matches in stream order, as long as their source bytes are final -- below
// the lowest pending match of the run (S.low), or in the lane's own range, whose earlier matches are done.  Byte by byte, so
// an overlapping match (dist < len) gives what pd_inflate's copy gives.
PD_FN void pw_resolve(PwShared& S, int lane) {
  const uint32_t mo = S.moff[lane], nm = S.emm[lane], ro = S.roff[lane], low = S.low;
  uint32_t done = S.mdone[lane];
  while (done < nm) {
    const PwMatch m = S.match[(mo + done) % PW_MATCHES];
    const int32_t src = (int32_t)m.dst - (int32_t)m.dist, last = src + (int32_t)m.len < (int32_t)m.dst ? src + (int32_t)m.len : (int32_t)m.dst;
    if (!(last <= (int32_t)low || src >= (int32_t)ro || low >= ro)) break;
    for (uint32_t k = 0; k < m.len && m.dst + k < PW_STAGE; ++k) {
      const int32_t q = src + (int32_t)k;
      S.stage[m.dst + k] = q < 0 ? S.ring[(S.produced + (uint32_t)q) & (PW_RING - 1u)] : S.stage[q];
    }
    ++done;
  }
  S.mdone[lane] = done;
}

// Ring -> filtered bytes: the whole 16-byte groups in front of S.produced (all of it when `all`), each lane a group per step.
PD_FN void pw_flush(PwShared& S, int lane, uint8_t* filt, uint32_t filt_bytes, bool all) {
  const uint32_t upto = (S.produced < filt_bytes ? S.produced : filt_bytes) & ~15u;
  for (uint32_t q = S.flushed + 16u * (uint32_t)lane; q < upto; q += 16u * PW_WAVE)      // (S.flushed is a multiple of 16)
    __builtin_memcpy(__builtin_assume_aligned(filt + q, 16), __builtin_assume_aligned(S.ring + (q & (PW_RING - 1u)), 16), 16);
  if (all)
    for (uint32_t q = upto + (uint32_t)lane; q < S.produced && q < filt_bytes; q += PW_WAVE) filt[q] = S.ring[q & (PW_RING - 1u)];
}

// ---- one image ----------------------------------------------------------------------------------------------------------------
// filt: the image's filtered bytes (16-byte aligned, filt_bytes long).  seg_bytes: 16 .. 256, a power of two; max_rounds 1 .. 64.
// Writes *rec; on acceptance also *adler_pos.
PD_FN void pw_image(PwShared& S, const uint8_t* s, uint32_t n, uint8_t* filt, uint32_t filt_bytes, uint32_t seg_bytes, uint32_t max_rounds,
                    PwRecord* rec, uint32_t* adler_pos) {
  const uint32_t segbits = 8u * seg_bytes;
  PW_EACH(lane) {
    S.ad_a[lane] = 0;
    S.ad_w[lane] = 0;
  }
  PW_EACH(lane) if (lane == 0) {
    S.bit = 16; S.produced = 0; S.flushed = 0; S.fail = n >= PW_MAX_STREAM || n < 2u; S.bad = 0; S.bfinal = 0; S.btype = 0; S.have_fixed = 0;
    S.windows = 0; S.rounds = 0; S.res_rounds = 0;
  }
  while (!S.fail) {                                        // every block consumes at least three bits
    PW_EACH(lane) if (lane == 0) pw_header(S, s, n, filt_bytes);
    if (S.fail) break;
    if (S.btype == 0) {                                    // stored: stream -> ring -> filtered bytes, a chunk at a time
      for (uint32_t done = 0; done < S.st_len; done += PW_STORED_CHUNK) {
        const uint32_t m = S.st_len - done < PW_STORED_CHUNK ? S.st_len - done : PW_STORED_CHUNK;
        PW_EACH(lane)
          for (uint32_t i = (uint32_t)lane; i < m; i += PW_WAVE) pw_ring_put(S, lane, S.produced + i, s[S.st_at + done + i], filt_bytes);
        PW_EACH(lane) if (lane == 0) S.produced += m;
        PW_EACH(lane) pw_flush(S, lane, filt, filt_bytes, false);
        PW_EACH(lane) if (lane == 0) S.flushed = S.produced & ~15u;
      }
    } else {
      const bool fixed = S.btype == 1;
      PdTables& T = fixed ? S.fx : S.tb;
      if (!fixed || !S.have_fixed) {
        const uint8_t* dl = fixed ? S.fx.lens + 288 : S.tb.lens + S.nlen;
        PW_EACH(lane) {
          for (uint32_t j = (uint32_t)lane; j < (1u << PD_LBITS); j += PW_WAVE) T.lit[j] = 0;
          for (uint32_t j = (uint32_t)lane; j < (1u << PD_DBITS); j += PW_WAVE) T.dist[j] = 0;
        }
        PW_EACH(lane) {
          pw_fill(lane, T.lens, T.hl, S.cl, T.lit, PD_LBITS);
          pw_fill(lane, dl, T.hd, S.cd, T.dist, PD_DBITS);
          if (lane == 0 && fixed) S.have_fixed = 1;
        }
      }
      uint32_t wbase = S.bit;
      for (;;) {                                           // windows: each ends the block or moves 64 segments on
        PW_EACH(lane) {
          S.entry[lane] = lane == 0 ? S.bit : wbase + (uint32_t)lane * segbits;
          S.dirty[lane] = 1;
        }
        uint32_t round = 0;
        bool converged = false;
        while (round < max_rounds) {
          ++round;
          PW_EACH(lane) {
            if (lane == 0) S.changed = 0;
            if (S.dirty[lane]) pw_scan(S, lane, s, n, T, wbase + (uint32_t)(lane + 1) * segbits);
            S.dirty[lane] = 0;
          }
          // (a lane behind an end-of-block code or an error keeps its guess: such ends are common on garbage, and the chain
          // is read from lane 0 up to its first end, so what stands behind one is never looked at)
          PW_EACH(lane) if (lane > 0 && S.exit_[lane - 1] != PW_NONE && S.exit_[lane - 1] != S.entry[lane]) {
            S.entry[lane] = S.exit_[lane - 1];
            S.dirty[lane] = 1;
            S.changed = 1;
          }
          if (!S.changed) { converged = true; break; }
        }
        PW_EACH(lane) if (lane == 0) {                       // the true chain: up to the first end of block
          ++S.windows;
          S.rounds += round;
          uint32_t nl = PW_WAVE, end = 0, total = 0, bad = !converged;
          for (uint32_t j = 0; j < (uint32_t)PW_WAVE && !bad; ++j) {
            if (S.err[j] || S.nbytes[j] > filt_bytes - S.produced - total) { bad = 1; break; }
            total += S.nbytes[j];
            if (S.eob0[j] != PW_NONE) { nl = j + 1; end = 1; break; }
          }
          S.nl = nl; S.blockend = end; S.run_a = 0;
          if (bad) S.fail = 1;
        }
        if (S.fail) break;
        PW_EACH(lane) {
          S.cur[lane] = S.entry[lane];
          S.stop[lane] = S.eob0[lane] != PW_NONE ? S.eob0[lane] : S.exit_[lane];
        }
        for (;;) {                                         // runs of consecutive lanes whose bytes and matches fit the buffers
          PW_EACH(lane) if (lane == 0) {
            uint32_t a = S.run_a;
            while (a < S.nl && (S.cur[a] >= S.stop[a] || S.nbytes[a] == 0)) ++a;
            uint32_t b = a;
            if (a < S.nl) {
              if (S.nbytes[a] <= PW_STAGE && S.nmatch[a] <= PW_MATCHES) {
                uint32_t ob = 0, om = 0;
                while (b < S.nl && ob + S.nbytes[b] <= PW_STAGE && om + S.nmatch[b] <= PW_MATCHES) {
                  S.roff[b] = ob; S.moff[b] = om; S.bbud[b] = S.nbytes[b]; S.mbud[b] = S.nmatch[b];
                  ob += S.nbytes[b]; om += S.nmatch[b];
                  ++b;
                }
              } else {                                     // one lane alone does not fit: as many of its tokens as do
                S.roff[a] = 0; S.moff[a] = 0; S.bbud[a] = PW_STAGE; S.mbud[a] = PW_MATCHES;
                b = a + 1;
              }
            }
            S.run_a = a; S.run_b = b;
          }
          if (S.run_a >= S.run_b) break;
          PW_EACH(lane) if ((uint32_t)lane >= S.run_a && (uint32_t)lane < S.run_b) pw_emit(S, lane, s, n, T);
          PW_EACH(lane) {
            if ((uint32_t)lane >= S.run_a && (uint32_t)lane < S.run_b) {
              S.nbytes[lane] -= S.emb[lane];               // (emitted <= the budget <= what was left)
              S.nmatch[lane] -= S.emm[lane];
              if (S.run_b - S.run_a > 1u && S.emb[lane] != S.bbud[lane]) S.bad = 1;   // (never: whole lanes emit what they counted)
            }
            if (lane == 0) {
              const uint32_t last = S.run_b - 1u;
              S.run_bytes = S.roff[last] + S.emb[last];
              if (S.run_bytes > PW_STAGE || S.run_bytes > filt_bytes - S.produced || S.run_bytes == 0) S.bad = 1;
            }
          }
          if (S.bad) break;
          for (;;) {                                       // resolution rounds: each retires the lowest pending match at least
            PW_EACH(lane) S.pend[lane] = (uint32_t)lane >= S.run_a && (uint32_t)lane < S.run_b && S.mdone[lane] < S.emm[lane]
                                             ? S.match[(S.moff[lane] + S.mdone[lane]) % PW_MATCHES].dst : PW_NONE;
            PW_EACH(lane) if (lane == 0) {
              uint32_t low = PW_NONE;
              for (uint32_t j = S.run_a; j < S.run_b && low == PW_NONE; ++j) low = S.pend[j];
              S.low = low;
              if (low != PW_NONE) ++S.res_rounds;
            }
            if (S.low == PW_NONE) break;
            PW_EACH(lane) if ((uint32_t)lane >= S.run_a && (uint32_t)lane < S.run_b) pw_resolve(S, lane);
          }
          PW_EACH(lane)
            for (uint32_t i = (uint32_t)lane; i < S.run_bytes; i += PW_WAVE) pw_ring_put(S, lane, S.produced + i, S.stage[i], filt_bytes);
          PW_EACH(lane) if (lane == 0) S.produced += S.run_bytes;
          PW_EACH(lane) pw_flush(S, lane, filt, filt_bytes, false);
          PW_EACH(lane) if (lane == 0) S.flushed = S.produced & ~15u;
        }
        if (S.bad) break;
        if (S.blockend) {
          PW_EACH(lane) if (lane == 0) S.bit = S.eob1[S.nl - 1u];
          break;
        }
        PW_EACH(lane) if (lane == 0) S.bit = S.exit_[PW_WAVE - 1];
        wbase += (uint32_t)PW_WAVE * segbits;
      }
      if (S.fail || S.bad) break;
    }
    if (S.bfinal) break;
  }
  PW_EACH(lane) pw_flush(S, lane, filt, filt_bytes, true);
  PW_EACH(lane) if (lane == 0) {
    const uint32_t end = (S.bit + 7u) >> 3;
    bool ok = !S.fail && !S.bad && S.bfinal && S.produced == filt_bytes && end <= n && n - end >= 4u;
    if (ok) {                                              // a stream whose Adler-32 is wrong is left to the lane route as well
      unsigned long long a = 0, w = 0;
      for (int j = 0; j < PW_WAVE; ++j) { a += S.ad_a[j] % PNG_ADLER; w += S.ad_w[j] % PNG_ADLER; }
      ok = pd_be32(s + end) == pd_adler_finish(a, w, filt_bytes);
    }
    PwRecord r;
    r.windows = S.windows; r.rounds = S.rounds; r.accepted = ok ? 1u : 0u; r.resolution_rounds = S.res_rounds;
    *rec = r;
    if (ok) *adler_pos = end;
  }
}

}  // namespace attwarp
