// Pieces of the PNG decoder (pngdec.hip) as __host__ __device__ code: the table layouts, the inflate core
// (all of RFC 1951), the chain of decoding units, Adler-32, filter reconstruction and the pixel conversions.  The same
// text runs inside the kernels and, under a sanitizer, in tests/pngdec_host_main.cpp; tests/pngdec_ref.py restates it.
//
// Bounds by construction: every read of the stream goes through PdBits (checked against the stream's length), every write
// and every match goes through pd_inflate's `cap` / `produced` checks, every table index is a masked or range-checked
// value, and every loop consumes stream bits or produces output, both of which are finite and planner-checked.
#pragma once
#include "png_blocks.hpp"

namespace attwarp {

// Inside a kernel the core is inlined into its single call site: the compiler then sees which pointers are global memory and
// which are LDS (no flat instructions, whose LDS half would make every table look-up wait for the stores in flight).
#if defined(__HIP_DEVICE_COMPILE__)
#define PD_FN __host__ __device__ __forceinline__
#else
#define PD_FN __host__ __device__ inline
#endif

constexpr int PD_MAX_UNITS = ATTWARP_PNGDEC_MAX_UNITS;
constexpr int PD_LBITS = 10, PD_DBITS = 8, PD_CBITS = 7;  // index bits of the primary tables: literal / length, distance, code lengths
constexpr uint32_t PD_LONG = 15;                         // length field of a primary entry whose code is longer than the index

struct PdImage {                       // the per-image record of a planned table
  uint64_t stream_off;                 // zlib stream in the packed stream buffer
  uint64_t filt_off;                   // filtered bytes in the scratch buffer (16-byte aligned)
  uint64_t out_off;                    // pixels in the output buffer
  uint32_t stream_len, filt_bytes;     // both below 2^31
  int32_t H, W, ch, oc;                // channels of the file / of the output
  int32_t swap, row_bytes;             // row_bytes = 1 + W * ch
};
static_assert(sizeof(PdImage) == 56, "record layout");

struct PdUnit {                        // one decoding unit of an image (scratch)
  uint32_t start, end;                 // byte positions in the image's stream: first block header / behind the last block
  uint32_t out_len, out_off;           // bytes it produces / where they go in the image's filtered bytes
  uint32_t status;                     // ATTWARP_PNGDEC_*
  uint32_t final, dependent, on_chain; // saw BFINAL / a match reached back before its first byte / the chain arrives here
};

struct PdState {                       // per image (scratch)
  uint32_t nunits, route;              // route 1: decoded by the serial kernel
  uint32_t st_crc, st_inflate, st_adler, st_filter;
  uint32_t adler_pos;                  // where the stream's Adler-32 stands
  uint32_t chain_len;                  // units on the chain (route 0)
};

struct PdHuff {                        // a canonical code: symbols sorted by (length, symbol)
  uint16_t count[16];
  uint16_t symbol[288];
};
struct PdTables {
  uint16_t lit[1 << PD_LBITS];         // symbol << 4 | length; length 0: no code, PD_LONG: a longer code
  uint16_t dist[1 << PD_DBITS];
  PdHuff hl, hd;
  uint8_t lens[320];
};

struct PdResult {
  uint32_t status, end, out_len, final, dependent;
};

PD_FN uint32_t pd_load32(const uint8_t* p) { return *reinterpret_cast<const u32_una*>(p); }

// ---- the bit reader: LSB first, never reads at or past p + n ---------------------------------------------------------------
struct PdBits {
  const uint8_t* p;
  uint32_t n, pos, cnt;                // stream length, next byte to go into acc, valid bits in acc (the bits above are zero)
  uint32_t ahead, has_ahead;           // bytes pos .. pos + 3, loaded one refill early so that their latency hides behind decoding
  uint64_t acc;
  PD_FN void init(const uint8_t* s, uint32_t len, uint32_t at) { p = s; n = len; to_byte(at < len ? at : len); }
  PD_FN void refill() {
    if (cnt > 32) return;
    if (!has_ahead && pos + 4u <= n) { ahead = pd_load32(p + pos); has_ahead = 1; }
    if (has_ahead) {
      acc |= (uint64_t)ahead << cnt;
      pos += 4;
      cnt += 32;
      has_ahead = pos + 4u <= n;
      if (has_ahead) ahead = pd_load32(p + pos);
    } else {
      while (cnt <= 56 && pos < n) { acc |= (uint64_t)p[pos++] << cnt; cnt += 8; }
    }
  }
  // nb <= 16 bits; false: the stream ended
  PD_FN bool bits(uint32_t nb, uint32_t& v) {
    refill();
    if (nb > cnt) return false;
    v = (uint32_t)acc & ((1u << nb) - 1u);
    acc >>= nb;
    cnt -= nb;
    return true;
  }
  PD_FN uint32_t byte_pos() const { return pos - cnt / 8u; }   // partial byte counts as consumed
  PD_FN void to_byte(uint32_t at) { pos = at; cnt = 0; acc = 0; ahead = 0; has_ahead = 0; }
};

// ---- tables ----------------------------------------------------------------------------------------------------------------------
PD_FN uint32_t pd_rev(uint32_t c, int l) {
  uint32_t r = 0;
  for (int i = 0; i < l; ++i) r |= ((c >> i) & 1u) << (l - 1 - i);
  return r;
}

// Code lengths lens[0 .. n) (n <= 288, each <= 15) -> canonical code h and its primary table of 2^pbits entries.
// Over-subscribed sets are refused; incomplete ones too, except (allow_single) no code at all or one code of length 1,
// which zlib accepts and this project's encoder writes for its distance tree.
PD_FN uint32_t pd_build(const uint8_t* lens, int n, PdHuff& h, uint16_t* primary, int pbits, bool allow_single) {
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
    if (l) h.symbol[offs[l]++] = (uint16_t)i;             // (sum of the counts <= n <= 288)
  }
  const uint32_t size = 1u << pbits;
  for (uint32_t j = 0; j < size; ++j) primary[j] = 0;
  uint32_t code = 0, idx = 0;
  for (int l = 1; l < 16; ++l) {
    for (uint32_t k = 0; k < h.count[l]; ++k, ++code, ++idx) {
      const uint32_t r = pd_rev(code, l);                  // (code < 2^l: the set is not over-subscribed)
      if (l <= pbits) {
        const uint16_t e = (uint16_t)(((uint32_t)h.symbol[idx] << 4) | (uint32_t)l);
        for (uint32_t j = r; j < size; j += 1u << l) primary[j] = e;
      } else {
        primary[r & (size - 1u)] = (uint16_t)PD_LONG;
      }
    }
    code <<= 1;
  }
  return ATTWARP_PNGDEC_OK;
}

// One symbol.  The bits behind the stream's end read as zeros; a code that needs them is a truncation.
PD_FN uint32_t pd_decode(PdBits& br, const uint16_t* primary, int pbits, const PdHuff& h, uint32_t& sym) {
  br.refill();
  const uint32_t v = (uint32_t)br.acc;
  const uint32_t e = primary[v & ((1u << pbits) - 1u)];
  uint32_t l = e & 15u;
  if (l == 0) return ATTWARP_PNGDEC_E_SYMBOL;
  sym = e >> 4;
  if (l == PD_LONG) {                                      // bit by bit over the canonical code
    int code = 0, first = 0, index = 0;
    l = 0;
    for (int k = 1; k < 16; ++k) {
      code |= (int)((v >> (k - 1)) & 1u);
      const int c = h.count[k];
      if (code - c < first) { sym = h.symbol[index + (code - first)]; l = (uint32_t)k; break; }
      index += c;
      first = (first + c) << 1;
      code <<= 1;
    }
    if (l == 0) return ATTWARP_PNGDEC_E_SYMBOL;
  }
  if (l > br.cnt) return ATTWARP_PNGDEC_E_TRUNCATED;
  br.acc >>= l;
  br.cnt -= l;
  return ATTWARP_PNGDEC_OK;
}

// length symbol 257 + s -> base and extra bits; distance symbol d likewise (the inverse of png_length_symbol)
PD_FN void pd_length_base(uint32_t s, uint32_t& base, uint32_t& eb) {
  if (s < 8) { base = 3 + s; eb = 0; }
  else if (s == 28) { base = 258; eb = 0; }
  else { eb = (s >> 2) - 1u; base = 3u + ((4u + (s & 3u)) << eb); }
}
PD_FN void pd_dist_base(uint32_t d, uint32_t& base, uint32_t& eb) {
  if (d < 4) { base = 1 + d; eb = 0; }
  else { eb = (d >> 1) - 1u; base = 1u + ((2u + (d & 1u)) << eb); }
}

__host__ __device__ inline uint32_t pd_zlib_header(const uint8_t* s, uint32_t n) {
  if (n < 2) return ATTWARP_PNGDEC_E_TRUNCATED;
  const uint32_t cmf = s[0], flg = s[1];
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (cmf * 256u + flg) % 31u != 0u || (flg & 32u)) return ATTWARP_PNGDEC_E_ZLIB_HEADER;
  return ATTWARP_PNGDEC_OK;
}

// ---- the inflate core --------------------------------------------------------------------------------------------------------
// Decodes whole blocks of the stream s[0 .. n) from byte position `start` until the final block, or (kept != nullptr)
// until it stands byte-aligned behind an EMPTY non-final stored block exactly on one of the sorted positions
// kept[0 .. nkept) that lie behind `start`.
//   out == nullptr  counting: nothing is written; a match that reaches back before the first produced byte sets
//                   `dependent` and counting goes on (the bits do not depend on the bytes);
//   out != nullptr  bytes go to out[0 .. cap); such a match is ATTWARP_PNGDEC_E_DISTANCE.
// More than `cap` bytes is ATTWARP_PNGDEC_E_OVERFLOW.  On an error `end` / `out_len` say how far it came.
PD_FN PdResult pd_inflate(const uint8_t* s, uint32_t n, uint32_t start, uint8_t* out, uint32_t cap,
                                               const uint32_t* kept, uint32_t nkept, PdTables& tb) {
  PdResult R = {ATTWARP_PNGDEC_OK, start, 0, 0, 0};
  PdBits br;
  br.init(s, n, start);
  uint32_t produced = 0, v = 0;
#define PD_FAIL(code) do { R.status = (code); R.end = br.byte_pos(); R.out_len = produced; return R; } while (0)
  for (;;) {                                               // every block consumes at least 3 bits of a finite stream
    uint32_t hdr;
    if (!br.bits(3, hdr)) PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED);
    const uint32_t bfinal = hdr & 1u, btype = hdr >> 1;
    if (btype == 3) PD_FAIL(ATTWARP_PNGDEC_E_BLOCK_TYPE);
    if (btype == 0) {
      uint32_t at = br.byte_pos();
      if (at + 4u > n) { br.to_byte(n); PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED); }
      const uint32_t len = s[at] | (uint32_t)s[at + 1] << 8, nlen = s[at + 2] | (uint32_t)s[at + 3] << 8;
      at += 4;
      br.to_byte(at);
      if ((len ^ nlen) != 0xffffu) PD_FAIL(ATTWARP_PNGDEC_E_STORED_LEN);
      if (len > n - at) { br.to_byte(n); PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED); }
      if (len > cap - produced) PD_FAIL(ATTWARP_PNGDEC_E_OVERFLOW);
      if (out)
        for (uint32_t i = 0; i < len; ++i) out[produced + i] = s[at + i];
      produced += len;
      at += len;
      br.to_byte(at);
      if (!bfinal && len == 0 && kept) {                   // a sync point: does a later unit start here?
        uint32_t lo = 0, hi = nkept;
        while (lo < hi) {                                  // (first kept position >= at)
          const uint32_t mid = (lo + hi) / 2;
          if (kept[mid] < at) lo = mid + 1; else hi = mid;
        }
        if (lo < nkept && kept[lo] == at && at > start) { R.end = at; R.out_len = produced; return R; }
      }
    } else {
      if (btype == 1) {
        for (int i = 0; i < 288; ++i) tb.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 32; ++i) tb.lens[288 + i] = 5;
        pd_build(tb.lens, 288, tb.hl, tb.lit, PD_LBITS, false);
        pd_build(tb.lens + 288, 32, tb.hd, tb.dist, PD_DBITS, false);
      } else {
        if (!br.bits(14, v)) PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED);
        const uint32_t nlen = 257u + (v & 31u), ndist = 1u + ((v >> 5) & 31u), ncode = 4u + (v >> 10);
        if (nlen > 286u || ndist > 30u) PD_FAIL(ATTWARP_PNGDEC_E_CODE_LENGTHS);
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (int i = 0; i < 19; ++i) tb.lens[i] = 0;
        for (uint32_t i = 0; i < ncode; ++i) {
          if (!br.bits(3, v)) PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED);
          tb.lens[order[i]] = (uint8_t)v;
        }
        if (pd_build(tb.lens, 19, tb.hl, tb.lit, PD_CBITS, false)) PD_FAIL(ATTWARP_PNGDEC_E_CODE_LENGTHS);
        const uint32_t total = nlen + ndist;                // <= 316
        uint32_t i = 0;
        while (i < total) {                                // every pass adds at least one length
          uint32_t sym;
          if (const uint32_t rc = pd_decode(br, tb.lit, PD_CBITS, tb.hl, sym)) PD_FAIL(rc == ATTWARP_PNGDEC_E_SYMBOL ? (uint32_t)ATTWARP_PNGDEC_E_CODE_LENGTHS : rc);
          if (sym < 16) { tb.lens[i++] = (uint8_t)sym; continue; }
          uint32_t rep, val = 0;
          if (sym == 16) {
            if (i == 0) PD_FAIL(ATTWARP_PNGDEC_E_CODE_LENGTHS);
            val = tb.lens[i - 1];
            if (!br.bits(2, v)) PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED);
            rep = 3 + v;
          } else if (sym == 17) {
            if (!br.bits(3, v)) PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED);
            rep = 3 + v;
          } else {
            if (!br.bits(7, v)) PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED);
            rep = 11 + v;
          }
          if (i + rep > total) PD_FAIL(ATTWARP_PNGDEC_E_CODE_LENGTHS);
          for (uint32_t k = 0; k < rep; ++k) tb.lens[i++] = (uint8_t)val;
        }
        if (tb.lens[256] == 0) PD_FAIL(ATTWARP_PNGDEC_E_CODE_LENGTHS);
        // (the distance lengths first: building the literal table reuses nothing of tb.lens, but keep the order explicit)
        if (pd_build(tb.lens + nlen, (int)ndist, tb.hd, tb.dist, PD_DBITS, true)) PD_FAIL(ATTWARP_PNGDEC_E_CODE_LENGTHS);
        if (pd_build(tb.lens, (int)nlen, tb.hl, tb.lit, PD_LBITS, true)) PD_FAIL(ATTWARP_PNGDEC_E_CODE_LENGTHS);
      }
      for (;;) {                                           // every symbol consumes at least one bit
        uint32_t sym;
        if (const uint32_t rc = pd_decode(br, tb.lit, PD_LBITS, tb.hl, sym)) PD_FAIL(rc);
        if (sym < 256) {
          if (produced >= cap) PD_FAIL(ATTWARP_PNGDEC_E_OVERFLOW);
          if (out) out[produced] = (uint8_t)sym;
          ++produced;
          continue;
        }
        if (sym == 256) break;
        sym -= 257;
        if (sym >= 29) PD_FAIL(ATTWARP_PNGDEC_E_SYMBOL);
        uint32_t base, eb, len, dist;
        pd_length_base(sym, base, eb);
        if (!br.bits(eb, v)) PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED);
        len = base + v;
        if (const uint32_t rc = pd_decode(br, tb.dist, PD_DBITS, tb.hd, sym)) PD_FAIL(rc);
        if (sym >= 30) PD_FAIL(ATTWARP_PNGDEC_E_SYMBOL);
        pd_dist_base(sym, base, eb);
        if (!br.bits(eb, v)) PD_FAIL(ATTWARP_PNGDEC_E_TRUNCATED);
        dist = base + v;
        if (dist > produced) {
          if (out) PD_FAIL(ATTWARP_PNGDEC_E_DISTANCE);
          R.dependent = 1;
        }
        if (len > cap - produced) PD_FAIL(ATTWARP_PNGDEC_E_OVERFLOW);
        if (out) {
          uint8_t* o = out + produced;
          if (dist == 1) {                                 // a run: no read-back of the bytes just stored
            const uint8_t b = o[-1];
            for (uint32_t k = 0; k < len; ++k) o[k] = b;
          } else {
            for (uint32_t k = 0; k < len; ++k) o[k] = o[(int32_t)k - (int32_t)dist];   // may overlap: byte by byte
          }
        }
        produced += len;
      }
    }
    if (bfinal) {
      R.final = 1;
      R.end = br.byte_pos();
      R.out_len = produced;
      return R;
    }
  }
#undef PD_FAIL
}

// ---- the chain of units -------------------------------------------------------------------------------------------------------
// Walks the units from the stream's start: unit u hands over to the unit that starts where u ended.  Marks the units on the
// chain and gives them their output offsets.  Returns true (the unit route) when the chain reaches the final block with
// every unit clean and independent, exactly filt_bytes produced and the Adler-32's four bytes inside the stream; anything
// else is left to the serial route, which then finds the status.
__host__ __device__ inline bool pd_chain(PdUnit* units, uint32_t nunits, uint32_t filt_bytes, uint32_t stream_len, uint32_t& adler_pos,
                                         uint32_t& chain_len) {
  uint32_t u = 0, total = 0;
  chain_len = 0;
  for (uint32_t step = 0; step < nunits; ++step) {          // u grows with every step
    PdUnit& U = units[u];
    if (U.status != ATTWARP_PNGDEC_OK || U.dependent) return false;
    if (U.out_len > filt_bytes - total) return false;
    U.out_off = total;
    U.on_chain = 1;
    total += U.out_len;
    ++chain_len;
    if (U.final) {
      adler_pos = U.end;
      return total == filt_bytes && U.end <= stream_len && stream_len - U.end >= 4u;
    }
    uint32_t v = u + 1;
    while (v < nunits && units[v].start != U.end) ++v;     // (sorted; the unit stopped only on a kept position)
    if (v >= nunits) return false;
    u = v;
  }
  return false;
}

// the serial route's whole job after pd_inflate from the start: sizes and the Adler's place
__host__ __device__ inline uint32_t pd_serial_status(const PdResult& r, uint32_t filt_bytes, uint32_t stream_len) {
  if (r.status) return r.status;
  if (r.out_len < filt_bytes) return ATTWARP_PNGDEC_E_UNDERFLOW;
  if (r.end > stream_len || stream_len - r.end < 4u) return ATTWARP_PNGDEC_E_TRUNCATED;
  return ATTWARP_PNGDEC_OK;
}

// ---- Adler-32 of a slice: S1 = sum d_i, S2 = sum (weight of d_i), weight = bytes from d_i to the END of the data -------------
__host__ __device__ inline uint32_t pd_adler_finish(unsigned long long s1, unsigned long long s2, uint32_t nbytes) {
  const uint32_t a = (uint32_t)((1ull + s1) % PNG_ADLER), b = (uint32_t)(((unsigned long long)nbytes + s2) % PNG_ADLER);
  return b << 16 | a;
}
__host__ __device__ inline uint32_t pd_be32(const uint8_t* p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

// ---- filters and pixels -----------------------------------------------------------------------------------------------------------
// filtered byte f, a = left, b = up, c = upper left (all reconstructed) -> the reconstructed byte
__host__ __device__ inline uint32_t pd_recon(int ft, uint32_t f, int a, int b, int c) { return (f - png_filter(ft, 0, a, b, c)) & 255u; }
__host__ __device__ inline uint32_t pd_luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

}  // namespace attwarp
