// Pieces of the JPEG decoder (jpegdec.hip) as __host__ __device__ code: the table layouts, the canonical
// Huffman tables, the bit reader that un-stuffs FF 00, the decode of one block with its statuses, and the integer IDCT,
// chroma up-sampling and colour arithmetic of libjpeg as Pillow runs it.  The same text runs inside the kernels and, under
// a sanitizer, in tests/jpegdec_host_main.cpp; tests/jpegdec_ref.py restates it.
//
// Bounds by construction: every read of the stream goes through JdBits (checked against the unit's end), every
// coefficient index is checked against 63 before the store, every table index is masked, and every loop is bounded by a
// constant: 16 bits per code, 64 coefficients per block.
//
// Hostile values are defined, not trusted: the DC predictor is a 32-bit two's-complement sum that wraps, the coefficient
// stored is its low 16 bits, all IDCT arithmetic is 32-bit with wrap-around (unsigned in the text, so that nothing here
// is undefined behaviour), and the final clamp saturates.
#pragma once
#include "common.hpp"

namespace attwarp {

#if defined(__HIP_DEVICE_COMPILE__)
#define JD_FN __host__ __device__ __forceinline__
#else
#define JD_FN __host__ __device__ inline
#endif

constexpr int JD_LOOK_BITS = 8;

struct JdImage {                       // the per-image record of a planned table
  uint64_t stream_off;                 // entropy data (everything behind the SOS header) in the packed stream buffer
  uint64_t coef_off;                   // int16 coefficients in the scratch buffer (256-byte aligned)
  uint64_t plane_off;                  // uint8 component planes in the scratch buffer (256-byte aligned)
  uint64_t out_off;                    // pixels in the output buffer
  uint32_t stream_len;                 // below 2^31
  int32_t H, W, ncomp;
  int32_t hs, vs;                      // luma sampling factors (chroma is 1 x 1; grey: 1 x 1)
  int32_t oc, to_luma, swap;           // output channels; colour file to "L"; BGR
  int32_t mcux, mcuy, ri;              // MCUs per row / rows, MCUs per unit (never 0 here: no restart interval = all of them)
  int32_t nunits, unit0;               // planned units, and the first of them among the call's units
  int32_t idct_tile0, color_tile0;     // first workgroup of the IDCT / colour launch that belongs to this image
  int32_t bw[3], bh[3];                // blocks per row / block rows of each component's padded plane
  uint32_t block0[3];                  // first block of each component among the image's blocks
  uint32_t nblocks;
  uint16_t qt[3][64];                  // natural order
  uint8_t dc_counts[3][16], ac_counts[3][16];
  uint8_t dc_symbols[3][256], ac_symbols[3][256];
};
static_assert(sizeof(JdImage) % 8 == 0, "record layout");

struct JdState {                       // per image (scratch)
  uint32_t st_scan;                    // ATTWARP_JPEGDEC_E_RESTART or 0
  uint32_t eoi;                        // the first marker behind the data is EOI
  uint32_t fail;                       // min over failing units of (unit << 8 | status); 0xffffffff: none
  uint32_t nrst;                       // restart markers found in front of the data's end
};

struct JdHuff {                        // one canonical code, ready to decode
  uint16_t look[1 << JD_LOOK_BITS];    // by the next 8 bits: length << 8 | symbol; 0: a longer code or none
  int32_t maxcode[17];                 // largest code of each length, -1: none
  int32_t valoff[17];                  // index of a length's first symbol minus its first code
  uint8_t symbols[256];
};

// zigzag position -> natural position (the kernels decode through a copy in LDS)
constexpr uint8_t JD_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- tables: three steps, a barrier between them inside a kernel ------------------------------------------------------------------
// counts[16] is never over-subscribed and sums to nsym <= 256 (the planner checked it).
JD_FN void jd_huff_ranges(JdHuff& h, const uint8_t* counts) {              // one lane
  int32_t code = 0, k = 0;
  h.maxcode[0] = -1; h.valoff[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const int32_t c = counts[l - 1];
    h.valoff[l] = k - code;
    h.maxcode[l] = c ? code + c - 1 : -1;
    k += c;
    code = (code + c) << 1;
  }
}
JD_FN void jd_huff_clear(JdHuff& h, const uint8_t* symbols, int nsym, int lane, int nlanes) {
  for (int i = lane; i < (1 << JD_LOOK_BITS); i += nlanes) h.look[i] = 0;
  for (int i = lane; i < 256; i += nlanes) h.symbols[i] = i < nsym ? symbols[i] : (uint8_t)0;
}
JD_FN void jd_huff_fill(JdHuff& h, const uint8_t* counts, int lane, int nlanes) {
  // symbol k of length l <= 8 owns the 2^(8 - l) entries that start with its code
  for (int k = lane; k < 256; k += nlanes) {
    int first = 0, l = 0;
    for (int j = 1; j <= JD_LOOK_BITS; ++j) {
      const int c = counts[j - 1];
      if (l == 0 && k < first + c) l = j;
      if (l == 0) first += c;
    }
    if (l == 0) continue;
    const int32_t code = k - h.valoff[l];
    const int span = 1 << (JD_LOOK_BITS - l);
    const int at = (code << (JD_LOOK_BITS - l)) & ((1 << JD_LOOK_BITS) - 1);
    for (int e = 0; e < span; ++e) h.look[(at + e) & ((1 << JD_LOOK_BITS) - 1)] = (uint16_t)(l << 8 | h.symbols[k]);
  }
}
JD_FN int jd_nsym(const uint8_t* counts) {
  int n = 0;
  for (int l = 0; l < 16; ++l) n += counts[l];
  return n < 256 ? n : 256;
}

// ---- the bit reader: MSB first, FF 00 -> FF, never loads at or past `end` ------------------------------------------------------
// Byte `pos` of the unit's stream is p[pos & mask]: the host reads the stream itself (mask = all ones), a kernel reads a ring
// in LDS that the whole wave keeps filled ahead of the reader (mask = ring size - 1, ring aligned to pos).
struct JdBits {
  const uint8_t* p;
  uint32_t mask;
  uint32_t end, pos;                   // the unit is bytes pos .. end
  uint32_t cnt;                        // real bits in acc (the low cnt bits; the bits above are zero)
  uint64_t acc;
  uint32_t word, nword;                // up to four bytes loaded at once, lowest byte next
  JD_FN void init(const uint8_t* s, uint32_t m, uint32_t from, uint32_t to) {
    p = s; mask = m; pos = from < to ? from : to; end = to; cnt = 0; acc = 0; word = 0; nword = 0;
  }
  JD_FN bool next(uint32_t& b) {
    if (nword == 0) {
      if (pos >= end) return false;
      if ((pos & 3u) == 0 && end - pos >= 4u) {
#if defined(__HIP_DEVICE_COMPILE__)
        word = *reinterpret_cast<const uint32_t*>(p + (pos & mask));     // (the ring is dword aligned)
#else
        word = *reinterpret_cast<const u32_una*>(p + (pos & mask));
#endif
        nword = 4;
      } else {
        word = p[pos & mask];
        nword = 1;
      }
    }
    b = word & 255u;
    word >>= 8;
    --nword;
    ++pos;
    return true;
  }
  JD_FN void refill() {
    while (cnt <= 48) {
      uint32_t b, z;
      if (!next(b)) return;
      if (b == 0xffu) next(z);           // the stuffed 00 (inside a unit nothing else follows an FF: the scan ended it there)
      acc = acc << 8 | b;
      cnt += 8;
    }
  }
  // the next 16 bits, zeros behind the end
  JD_FN uint32_t peek16() const { return (uint32_t)(cnt >= 16 ? acc >> (cnt - 16) : acc << (16 - cnt)) & 0xffffu; }
  JD_FN void skip(uint32_t n) { cnt -= n; acc &= ((uint64_t)1 << cnt) - 1u; }      // n <= cnt <= 56
  JD_FN bool bits(uint32_t n, uint32_t& v) {                                         // n <= 16
    refill();
    if (n > cnt) return false;
    v = (uint32_t)(acc >> (cnt - n)) & ((1u << n) - 1u);
    skip(n);
    return true;
  }
};

// one symbol -> status
JD_FN uint32_t jd_symbol(JdBits& br, const JdHuff& h, uint32_t& sym) {
  br.refill();
  const uint32_t c = br.peek16();
  const uint32_t e = h.look[c >> (16 - JD_LOOK_BITS)];
  uint32_t len = e >> 8;
  sym = e & 255u;
  if (len == 0) {
    for (uint32_t l = JD_LOOK_BITS + 1; l <= 16; ++l) {
      const int32_t code = (int32_t)(c >> (16 - l));
      if (code <= h.maxcode[l]) {
        len = l;
        sym = h.symbols[(uint32_t)(h.valoff[l] + code) & 255u];
        break;
      }
    }
    if (len == 0) return br.cnt < 16 ? (uint32_t)ATTWARP_JPEGDEC_E_TRUNCATED : (uint32_t)ATTWARP_JPEGDEC_E_HUFFMAN;
  }
  if (len > br.cnt) return ATTWARP_JPEGDEC_E_TRUNCATED;
  br.skip(len);
  return 0;
}

JD_FN int32_t jd_extend(uint32_t v, uint32_t s) {
  return s == 0 || v >= (1u << (s - 1)) ? (int32_t)v : (int32_t)v - (int32_t)(1u << s) + 1;
}

// One block into blk[64] (natural order, zero on entry) -> status.  pred: the component's DC predictor; zz: JD_ZIGZAG or a copy.
JD_FN uint32_t jd_decode_block(JdBits& br, const JdHuff& dc, const JdHuff& ac, int32_t& pred, int16_t* blk, const uint8_t* zz) {
  uint32_t s, v, rs;
  if (const uint32_t st = jd_symbol(br, dc, s)) return st;
  s &= 15u;
  if (!br.bits(s, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
  pred = (int32_t)((uint32_t)pred + (uint32_t)jd_extend(v, s));
  blk[0] = (int16_t)(uint16_t)((uint32_t)pred & 0xffffu);
  uint32_t k = 1;
  for (int it = 0; it < 63 && k < 64; ++it) {
    if (const uint32_t st = jd_symbol(br, ac, rs)) return st;
    const uint32_t r = rs >> 4;
    s = rs & 15u;
    if (s == 0) {
      if (r != 15) break;
      if (k + 16 > 64) return ATTWARP_JPEGDEC_E_COEFF;
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return ATTWARP_JPEGDEC_E_COEFF;
    if (!br.bits(s, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
    blk[zz[k] & 63u] = (int16_t)jd_extend(v, s);
    ++k;
  }
  return 0;
}

// block (yy, xx) of a component (first block block0, bw blocks per row, h x v blocks per MCU) inside MCU (mx, my)
JD_FN uint32_t jd_block_at(uint32_t block0, uint32_t bw, int h, int v, uint32_t mx, uint32_t my, int yy, int xx) {
  return block0 + (my * (uint32_t)v + (uint32_t)yy) * bw + mx * (uint32_t)h + (uint32_t)xx;
}
// the same by component and MCU number -> its index among the image's blocks
JD_FN uint32_t jd_block_index(const JdImage& im, int c, uint32_t m, int yy, int xx) {
  const uint32_t mx = m % (uint32_t)im.mcux, my = m / (uint32_t)im.mcux;
  return jd_block_at(im.block0[c], (uint32_t)im.bw[c], c == 0 ? im.hs : 1, c == 0 ? im.vs : 1, mx, my, yy, xx);
}

// ---- self-synchronising sub-streams: a marker-less unit cut into byte segments, one decoder each ----------------
// A decoder's state between two symbols: where the next bit lies in the raw (stuffed) stream, which block of the MCU it
// belongs to and the zigzag index of the next coefficient (0: a DC symbol is next).  The position is canonical: the offset
// of the byte that holds the next bit, never a stuffed 00, and the bit's index in it (0: the top bit); at the unit's end
// it is (end, 0).  Two decoders that consumed the same bits report the same state.
struct JdSync {
  uint32_t byte;                       // relative to the image's data
  uint32_t bsk;                        // bit << 16 | slot << 8 | k
};
JD_FN bool jd_sync_equal(const JdSync& a, const JdSync& b) { return a.byte == b.byte && a.bsk == b.bsk; }

constexpr uint32_t JD_NO_ERROR = 0xffffffffu;
struct JdSegment {                     // what one segment's decode found (scratch, 32 bytes)
  JdSync exit;                         // the state at the first symbol that starts at or behind the segment's end
  uint32_t owned;                      // blocks whose DC symbol starts in the segment
  uint32_t nend;                       // blocks that end in its decode
  uint32_t eclean;                     // blocks that ended before its first error; JD_NO_ERROR: no error
  uint32_t dc[3];                      // per component, the wrapping sum of the owned blocks' DC differences
};
static_assert(sizeof(JdSegment) == 32, "segment layout");

// The reader's canonical position, in the reader's own coordinates (>= lo, the first byte of the image's data).  The bits
// still in acc came from the cnt / 8 (rounded up) data bytes in front of the next raw byte; each step back over a data
// byte also steps over the stuffed 00 behind an FF.
JD_FN void jd_sync_position(const JdBits& br, uint32_t lo, uint32_t& byte, uint32_t& bit) {
  uint32_t q = br.pos;                                        // (the next raw byte: pos counts bytes handed out, not loaded)
  const uint32_t nb = (br.cnt + 7u) >> 3;                     // <= 7
  for (uint32_t i = 0; i < nb && q > lo; ++i) {
    --q;
    if (q > lo && br.p[q & br.mask] == 0u && br.p[(q - 1u) & br.mask] == 0xffu) --q;
  }
  byte = q;
  bit = (8u - (br.cnt & 7u)) & 7u;
}

// Where segment `seg` starts before anything is known: its first byte, one later if that is the 00 behind an FF; a block
// is assumed to start there.  s: the image's data.
JD_FN JdSync jd_segment_guess(const uint8_t* s, uint32_t seg, uint32_t segment_bytes, uint32_t uend) {
  uint64_t b = (uint64_t)seg * segment_bytes;
  if (b >= uend) b = uend;
  else if (b > 0 && s[b] == 0u && s[b - 1] == 0xffu) ++b;     // (b + 1 <= uend)
  JdSync e;
  e.byte = (uint32_t)b;
  e.bsk = 0;
  return e;
}
JD_FN uint32_t jd_segment_end(uint32_t seg, uint32_t segment_bytes, uint32_t uend) {
  const uint64_t e = ((uint64_t)seg + 1u) * segment_bytes;
  return e < uend ? (uint32_t)e : uend;
}

JD_FN void jd_sync_open(JdBits& br, const uint8_t* p, uint32_t lo, const JdSync& entry, uint32_t uend) {
  br.init(p, 0xffffffffu, lo + (entry.byte < uend ? entry.byte : uend), lo + uend);
  br.refill();
  const uint32_t bit = (entry.bsk >> 16) & 7u;
  br.skip(bit < br.cnt ? bit : br.cnt);                       // (an entry in front of the end has a whole byte behind it)
}

// One segment, symbol by symbol, from `entry` until the position reaches seg_end.  p + lo: the image's data, p dword
// aligned; uend: the unit's end, nothing at or behind it is read.  nb0 / nblk: luma blocks / all blocks of an MCU.  An
// invalid code or a run past 63 marks the decode, skips one bit and starts a new block in the next slot, so a decoder that
// began in the wrong place goes on until it falls in step; a code or value that needs bits behind the unit's end marks it
// and ends at the unit's end.  Every turn of the loop consumes at least one bit.
// (The walk is written once over a LAYOUT: comp(slot) the component of a block slot of the MCU, block(m, slot) the index of
// that slot's block of MCU m among the image's blocks, nblocks their number, NC the components it may name; period(nblk)
// the slots a decoder's state tells apart and dc_slot(c, i, nblk) where a segment sums the DC difference of its i-th owned
// block, of component c, NDC such sums.  JdLayout is the one of the records above: every slot is told apart and the sums
// are per component; jpegfmt_blocks.hpp has the general one.)
struct JdLayout {
  static constexpr int NC = 3, NDC = 3;
  JD_FN uint32_t period(uint32_t nblk) const { return nblk; }
  JD_FN uint32_t dc_slot(uint32_t c, uint32_t, uint32_t) const { return c; }
  const JdImage* im;                   // (nullptr where only comp() is asked)
  uint32_t nb0;                        // luma blocks of an MCU
  JD_FN uint32_t comp(uint32_t slot) const { return slot < nb0 ? 0u : slot - nb0 + 1u; }
  JD_FN uint32_t block(uint32_t m, uint32_t slot) const {
    const uint32_t c = comp(slot), hs = (uint32_t)im->hs;
    return jd_block_index(*im, (int)c, m, c == 0 ? (int)(slot / hs) : 0, c == 0 ? (int)(slot % hs) : 0);
  }
  JD_FN uint32_t nblocks() const { return im->nblocks; }
};
template <class Layout, class Segment>
JD_FN void jd_decode_segment_of(const Layout& lay, const uint8_t* p, uint32_t lo, const JdSync& entry, uint32_t seg_end, uint32_t uend,
                                const JdHuff* dc, const JdHuff* ac, uint32_t nblk, Segment& r) {
  JdBits br;
  jd_sync_open(br, p, lo, entry, uend);
  const uint32_t nslot = lay.period(nblk);
  uint32_t slot = (entry.bsk >> 8) & 255u, k = entry.bsk & 63u;
  if (slot >= nslot) slot = 0;
  r.owned = 0; r.nend = 0; r.eclean = JD_NO_ERROR;
  for (int c = 0; c < Layout::NDC; ++c) r.dc[c] = 0;
  const uint32_t from = entry.byte < seg_end ? entry.byte : seg_end;
  const uint32_t limit = (seg_end - from) * 8u + 8u;
  uint32_t byte = 0, bit = 0;
  bool at_end = false;
  for (uint32_t it = 0; it < limit; ++it) {
    br.refill();
    if (br.pos - ((br.cnt + 7u) >> 3) >= lo + seg_end) {          // (an upper bound of the position)
      jd_sync_position(br, lo, byte, bit);
      if (byte >= lo + seg_end) break;
    }
    const uint32_t c = lay.comp(slot);
    uint32_t st, s = 0, v = 0;
    bool endblk = false;
    if (k == 0) {
      st = jd_symbol(br, dc[c], s);
      s &= 15u;
      if (!st && !br.bits(s, v)) st = ATTWARP_JPEGDEC_E_TRUNCATED;
      if (!st) {
        r.dc[lay.dc_slot(c, r.owned, nblk)] += (uint32_t)jd_extend(v, s);
        ++r.owned;
        k = 1;
      }
    } else {
      uint32_t rs = 0;
      st = jd_symbol(br, ac[c], rs);
      if (!st) {
        const uint32_t run = rs >> 4;
        s = rs & 15u;
        if (s == 0) {
          if (run != 15u) endblk = true;
          else if (k + 16u > 64u) st = ATTWARP_JPEGDEC_E_COEFF;
          else k += 16u;
        } else if (k + run > 63u) st = ATTWARP_JPEGDEC_E_COEFF;
        else if (!br.bits(s, v)) st = ATTWARP_JPEGDEC_E_TRUNCATED;
        else k += run + 1u;
      }
      if (!st && k >= 64u) endblk = true;
    }
    if (st) {
      if (r.eclean == JD_NO_ERROR) r.eclean = r.nend;
      br.refill();
      if (st == (uint32_t)ATTWARP_JPEGDEC_E_TRUNCATED || br.cnt == 0) { at_end = true; break; }
      br.skip(1);
      slot = slot + 1u == nslot ? 0u : slot + 1u;
      k = 0;
    } else if (endblk) {
      ++r.nend;
      slot = slot + 1u == nslot ? 0u : slot + 1u;
      k = 0;
    }
  }
  if (at_end) { byte = lo + uend; bit = 0; }
  else jd_sync_position(br, lo, byte, bit);
  r.exit.byte = byte - lo;
  r.exit.bsk = bit << 16 | slot << 8 | k;
}
JD_FN void jd_decode_segment(const uint8_t* p, uint32_t lo, const JdSync& entry, uint32_t seg_end, uint32_t uend, const JdHuff* dc,
                             const JdHuff* ac, uint32_t nb0, uint32_t nblk, JdSegment& r) {
  jd_decode_segment_of(JdLayout{nullptr, nb0}, p, lo, entry, seg_end, uend, dc, ac, nblk, r);
}

// What the converged states must satisfy, segment by segment: `before` blocks start in front of the segment.  Bit 0: the
// segment contradicts a sequential decode of `expected` blocks (an error in front of the end of block expected - 1, or an
// entry slot that does not follow from the count); bit 1: block expected - 1 ends in this segment, cleanly.  period: the
// slots the states tell apart (0: all nblk of them).
template <class Segment>                // (JdSegment, or JfSegment of jpegfmt_blocks.hpp: the counts alone are read)
JD_FN uint32_t jd_segment_check(const JdSync& entry, const Segment& r, uint32_t before, uint32_t expected, uint32_t nblk,
                                uint32_t period = 0) {
  const uint32_t inprog = (entry.bsk & 63u) != 0u;
  if (before < inprog) return 1u;
  const uint32_t done = before - inprog;                     // blocks that ended in front of the segment
  if (done >= expected) return 0u;                           // behind the last block: whatever follows it is tolerated
  if (((entry.bsk >> 8) & 255u) != done % (period ? period : nblk)) return 1u;
  const uint32_t last = expected - 1u - done;
  if (last < r.nend) return r.eclean > last ? 2u : 1u;
  return r.eclean == JD_NO_ERROR ? 0u : 1u;
}

// The write pass of one segment from its TRUE entry: the rest of a block begun earlier is skipped, then every owned block
// is decoded in full (reading past the segment's end until it ends) and stored whole at its true index.  pred: the
// predictors at the segment's start (the sums of all DC differences in front of it), before: the owned blocks in front of
// it; blocks with ordinal >= expected are dropped.  blk: 64 int16 of the caller's (dword aligned).  -> status
template <class Layout>
JD_FN uint32_t jd_write_segment_of(const Layout& lay, const uint8_t* p, uint32_t lo, const JdSync& entry, uint32_t uend, const JdHuff* dc,
                                   const JdHuff* ac, uint32_t nblk, uint32_t before, const uint32_t* pred0, uint32_t owned,
                                   uint32_t expected, int16_t* blk, const uint8_t* zz, int16_t* coef) {
  if (before >= expected || owned == 0) return 0;
  JdBits br;
  jd_sync_open(br, p, lo, entry, uend);
  uint32_t slot = (entry.bsk >> 8) & 255u, k = entry.bsk & 63u;
  if (slot >= nblk) slot = 0;
  if (k != 0) {
    const uint32_t c = lay.comp(slot);
    for (int it = 0; it < 63 && k < 64u; ++it) {
      uint32_t rs, v;
      if (const uint32_t st = jd_symbol(br, ac[c], rs)) return st;
      const uint32_t run = rs >> 4, s = rs & 15u;
      if (s == 0) {
        if (run != 15u) break;
        if (k + 16u > 64u) return ATTWARP_JPEGDEC_E_COEFF;
        k += 16u;
        continue;
      }
      if (k + run > 63u) return ATTWARP_JPEGDEC_E_COEFF;
      if (!br.bits(s, v)) return ATTWARP_JPEGDEC_E_TRUNCATED;
      k += run + 1u;
    }
    slot = slot + 1u == nblk ? 0u : slot + 1u;
  }
  int32_t pred[Layout::NC];
  for (int c = 0; c < Layout::NC; ++c) pred[c] = (int32_t)pred0[c];
  const uint32_t n = owned < expected - before ? owned : expected - before;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t o = before + i, m = o / nblk, j = o - m * nblk;
    const uint32_t c = lay.comp(j);
    __builtin_memset(blk, 0, 128);
    if (const uint32_t st = jd_decode_block(br, dc[c], ac[c], pred[c], blk, zz)) return st;
    const uint32_t bi = lay.block(m, j);
    if (bi < lay.nblocks()) __builtin_memcpy(coef + (size_t)bi * 64u, blk, 128);
  }
  return 0;
}
JD_FN uint32_t jd_write_segment(const uint8_t* p, uint32_t lo, const JdSync& entry, uint32_t uend, const JdHuff* dc, const JdHuff* ac,
                                const JdImage& im, uint32_t nb0, uint32_t nblk, uint32_t before, const uint32_t* pred0, uint32_t owned,
                                uint32_t expected, int16_t* blk, const uint8_t* zz, int16_t* coef) {
  return jd_write_segment_of(JdLayout{&im, nb0}, p, lo, entry, uend, dc, ac, nblk, before, pred0, owned, expected, blk, zz, coef);
}

// ---- the integer IDCT of jidctint.c (CONST_BITS 13, PASS1_BITS 2), 32-bit wrap-around arithmetic ---------------------------------
JD_FN int32_t jd_sra(uint32_t x, int n) { return (int32_t)x >> n; }
JD_FN void jd_idct_1d(const uint32_t i[8], int shift, int32_t o[8]) {
  uint32_t z1 = (i[2] + i[6]) * 4433u;
  const uint32_t t2 = z1 - i[6] * 15137u, t3 = z1 + i[2] * 6270u;
  const uint32_t t0 = (i[0] + i[4]) * 8192u, t1 = (i[0] - i[4]) * 8192u;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a = i[7], b = i[5], c = i[3], d = i[1];
  const uint32_t z5 = (a + c + b + d) * 9633u;
  z1 = (a + d) * (uint32_t)-7373;
  const uint32_t z2 = (b + c) * (uint32_t)-20995;
  const uint32_t z3 = (a + c) * (uint32_t)-16069 + z5, z4 = (b + d) * (uint32_t)-3196 + z5;
  a = a * 2446u + z1 + z3;
  b = b * 16819u + z2 + z4;
  c = c * 25172u + z2 + z3;
  d = d * 12299u + z1 + z4;
  const uint32_t rnd = 1u << (shift - 1);
  o[0] = jd_sra(t10 + d + rnd, shift); o[7] = jd_sra(t10 - d + rnd, shift);
  o[1] = jd_sra(t11 + c + rnd, shift); o[6] = jd_sra(t11 - c + rnd, shift);
  o[2] = jd_sra(t12 + b + rnd, shift); o[5] = jd_sra(t12 - b + rnd, shift);
  o[3] = jd_sra(t13 + a + rnd, shift); o[4] = jd_sra(t13 - a + rnd, shift);
}
JD_FN uint32_t jd_clamp8(int32_t v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// ---- chroma up-sampling ("fancy", jdsample.c) and colour (jdcolor.c) -----------------------------------------------------------
// p: the plane (pitch bytes per row), dw x dh its true size; (x, y) an output pixel.  libjpeg picks the triangle filter
// only for a component with `downsampled_width > 2` (jinit_upsampler in jdsample.c); a plane of one or two columns is
// replicated instead, in both directions: sample (x >> 1, y >> 1) at 2 x 2, (x >> 1, y) at 2 x 1.
JD_FN int32_t jd_chroma(const uint8_t* p, int pitch, int dw, int dh, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(size_t)y * pitch + x];
  if (dw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * pitch + (x >> 1)];
  const int i = x >> 1;
  const int in = (x & 1) ? (i + 1 < dw ? i + 1 : i) : (i > 0 ? i - 1 : 0);
  if (vs == 1) {
    const uint8_t* row = p + (size_t)y * pitch;
    if (x == 0 || x == 2 * dw - 1) return row[i];
    return (3 * row[i] + row[in] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int r = y >> 1;
  const int rn = (y & 1) ? (r + 1 < dh ? r + 1 : r) : (r > 0 ? r - 1 : 0);
  const uint8_t *r0 = p + (size_t)r * pitch, *r1 = p + (size_t)rn * pitch;
  const int32_t s = 3 * r0[i] + r1[i], sn = 3 * r0[in] + r1[in];
  return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;            // (at an edge sn = s: 4 s + 8 / 4 s + 7)
}
JD_FN void jd_ycc_to_rgb(int32_t y, int32_t cb, int32_t cr, uint32_t& r, uint32_t& g, uint32_t& b) {
  cb -= 128; cr -= 128;
  r = jd_clamp8(y + ((91881 * cr + 32768) >> 16));
  g = jd_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  b = jd_clamp8(y + ((116130 * cb + 32768) >> 16));
}
JD_FN uint32_t jd_luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

}  // namespace attwarp
