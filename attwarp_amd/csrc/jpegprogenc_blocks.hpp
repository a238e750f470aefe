// Progressive files of the JPEG encoder (jpegenc.hip), shared by the jpegprogenc_* kernels, the host planner and
// the host test (tests/jpegprogenc_host_main.cpp): jpeg_simple_progression's script, where a scan's blocks lie among the
// coefficients the transform kernel left, the four block coders of libjpeg's jcphuff.c with the end-of-band run and its pending
// correction bits, the byte writer, the bit bounds, and the records the planner and the kernels exchange.  A coder writes into
// a SINK: sym(slot, symbol) is a Huffman symbol of table slot `slot`, bits(value, n) are n <= 16 raw bits.  The statistics pass
// counts the symbols, the second pass codes them: both run the same text, so both see the same symbols, those of a forced flush
// of the run included.  Restated by tests/jpegprogenc_ref.py.
#pragma once
#include "jpegopt_blocks.hpp"

namespace attwarp {

constexpr int PE_MAX_SCANS = 10;                         // colour: ten scans, grey: six
constexpr int PE_SLOTS = 11;                             // table slots per image: slot i is scan i's table (scan 0: DC table 0) ...
constexpr int PE_DC1_SLOT = 10;                          // ... and slot 10 the DC table of Cb and Cr
constexpr uint32_t PE_EOBRUN_MAX = 0x7fff;               // the run is written out when it gets here ...
constexpr int PE_MAX_CORR_BITS = 1000;                   // ... and when more than 1000 - 64 + 1 correction bits wait behind it
constexpr uint32_t PE_BE_LIMIT = PE_MAX_CORR_BITS - 64 + 1;
constexpr int PE_CORR_WORDS = (PE_MAX_CORR_BITS + 31) / 32;
static_assert(PE_BE_LIMIT + 63 <= PE_MAX_CORR_BITS, "the pending bits and a block's own fit the buffer");
// Bits a block adds to a scan at most.  An optimised code has at most 16 bits.  DC first pass: a difference of shifted values
// below 2^11 has at most 12 bits.  AC first pass: per coefficient a symbol and a value that, shifted by one at least, has at
// most 10 bits (sixteen zeros cost one symbol, less than sixteen coefficients); in front of them at most one run symbol with 14
// bits.  AC refinement: per coefficient a symbol and a sign, or one correction bit (its own, written by this block or by the
// run symbol of a later one: either way one bit per coefficient of the scan), and one run symbol.
constexpr int PE_EOBRUN_BITS = 16 + 14;
constexpr int PE_DC_FIRST_BITS = 16 + 12;
constexpr int PE_AC_FIRST_COEF_BITS = 16 + 10;
constexpr int PE_AC_REFINE_BLOCK_BITS = PE_EOBRUN_BITS + 63 * 17;
constexpr int PE_DHT_MAX = 277;                          // marker, length, class / id, 16 counts, 256 symbols

struct PeScan {
  int comp;                            // the scan's component; -1: all of them, interleaved
  int ss, se, ah, al;
};
__host__ __device__ inline PeScan pe_scan(int ncomp, int i) {
  // Cr (2) before Cb (1)
  constexpr int COLOUR[PE_MAX_SCANS][5] = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {2, 1, 63, 0, 1}, {1, 1, 63, 0, 1}, {0, 6, 63, 0, 2},
                                           {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {2, 1, 63, 1, 0}, {1, 1, 63, 1, 0}, {0, 1, 63, 1, 0}};
  constexpr int GREY[6][5] = {{0, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {0, 6, 63, 0, 2}, {0, 1, 63, 2, 1}, {0, 0, 0, 1, 0}, {0, 1, 63, 1, 0}};
  const int* r = ncomp == 3 ? COLOUR[i] : GREY[i];
  PeScan s = {r[0], r[1], r[2], r[3], r[4]};
  return s;
}
__host__ __device__ inline int pe_nscans(int ncomp) { return ncomp == 3 ? 10 : 6; }
// whether slot `slot` holds a table of an image with ncomp components; class << 4 | id of its DHT
__host__ __device__ inline bool pe_slot_used(int ncomp, int slot) {
  if (slot == PE_DC1_SLOT) return ncomp == 3;
  if (slot >= pe_nscans(ncomp)) return false;
  const PeScan s = pe_scan(ncomp, slot);
  return !(s.ss == 0 && s.ah != 0);                         // a DC refinement has no table
}
__host__ __device__ inline int pe_slot_class(int ncomp, int slot) {
  if (slot == PE_DC1_SLOT) return 0x01;
  const PeScan s = pe_scan(ncomp, slot);
  return s.ss == 0 ? 0x00 : (s.comp > 0 ? 0x11 : 0x10);
}
__host__ __device__ inline int pe_block_bits(const PeScan& s) {
  if (s.ss == 0) return s.ah ? 1 : PE_DC_FIRST_BITS;
  return s.ah ? PE_AC_REFINE_BLOCK_BITS : PE_EOBRUN_BITS + (s.se - s.ss + 1) * PE_AC_FIRST_COEF_BITS;
}
// bytes an interval of n blocks takes at most: every block at its bound, one more run symbol at its end, every byte stuffed
__host__ __device__ inline uint64_t pe_interval_bytes(uint64_t n, int block_bits) {
  return 2u * ((n * (uint64_t)block_bits + PE_EOBRUN_BITS + 7u) / 8u);
}

// Where block j of a scan's walk lies among the image's coefficients, which the transform kernel left MCU by MCU ([MCU][block
// of the MCU][64 zigzag int16], dummy blocks included).  An interleaved scan walks exactly that order; a scan of one
// component walks the component's own wc x hc blocks in raster order, which skips the dummy blocks.
struct PeWalk {
  const int16_t* coef;
  int bpm, ny, hmax, vmax, mcus_x;
  int comp, wc;                        // comp < 0: interleaved
  __host__ __device__ const int16_t* block(int64_t j, int& ci) const {
    if (comp < 0) {
      const int s = (int)(j % bpm);
      ci = s < ny ? 0 : s - ny + 1;
      return coef + j * 64;
    }
    ci = comp;
    const int64_t row = j / wc, col = j - row * wc;
    int64_t mcu;
    int s;
    if (comp == 0) {
      mcu = (row / vmax) * mcus_x + col / hmax;
      s = (int)(row % vmax) * hmax + (int)(col % hmax);
    } else {
      mcu = row * mcus_x + col;
      s = ny + comp - 1;
    }
    return coef + (mcu * bpm + s) * 64;
  }
};

__host__ __device__ inline int pe_nbits(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

// EOBRUN, and the correction bits that wait behind it (jcphuff.c: EOBRUN, BE, bit_buffer); the DC predictors
struct PeState {
  int last_dc[3];
  uint32_t eobrun, be;
  uint32_t corr[PE_CORR_WORDS];
  __host__ __device__ void reset() {
    last_dc[0] = last_dc[1] = last_dc[2] = 0;
    eobrun = be = 0;
    for (int i = 0; i < PE_CORR_WORDS; ++i) corr[i] = 0u;
  }
  __host__ __device__ void set(uint32_t i, uint32_t bit) {
    if (i >= (uint32_t)PE_MAX_CORR_BITS) return;             // (never: the run is flushed above PE_BE_LIMIT pending bits)
    const uint32_t m = 1u << (i & 31u);
    corr[i >> 5] = bit ? (corr[i >> 5] | m) : (corr[i >> 5] & ~m);
  }
  __host__ __device__ uint32_t get(uint32_t i) const { return (corr[i >> 5] >> (i & 31u)) & 1u; }
};

template <class Sink>
__host__ __device__ inline void pe_emit_corr(const PeState& st, uint32_t from, uint32_t n, Sink& sink) {
  for (uint32_t i = 0; i < n && from + i < (uint32_t)PE_MAX_CORR_BITS; ++i) sink.bits(st.get(from + i), 1);
}
template <class Sink>
__host__ __device__ inline void pe_emit_eobrun(PeState& st, int slot, Sink& sink) {
  if (st.eobrun == 0) return;
  const int nb = pe_nbits(st.eobrun) - 1;
  sink.sym(slot, nb << 4);
  if (nb) sink.bits(st.eobrun & ((1u << nb) - 1u), nb);
  st.eobrun = 0;
  pe_emit_corr(st, 0, st.be, sink);
  st.be = 0;
}
// the block ended in zeros (or in correction bits, own of them): the run grows and is written out at its limits
template <class Sink>
__host__ __device__ inline void pe_end_block(PeState& st, uint32_t own, int slot, Sink& sink) {
  ++st.eobrun;
  st.be += own;
  if (st.eobrun == PE_EOBRUN_MAX || st.be > PE_BE_LIMIT) pe_emit_eobrun(st, slot, sink);
}

template <class Sink>
__host__ __device__ inline void pe_dc_first(const int16_t* z, int ci, int al, int slot, PeState& st, Sink& sink) {
  const int t = (int)z[0] >> al;                            // arithmetic: -3 >> 1 is -2
  const int d = t - st.last_dc[ci];
  st.last_dc[ci] = t;
  const int n = pe_nbits((uint32_t)(d < 0 ? -d : d));
  sink.sym(slot, n);
  if (n) sink.bits((uint32_t)(d < 0 ? d - 1 : d) & ((1u << n) - 1u), n);
}
template <class Sink>
__host__ __device__ inline void pe_dc_refine(const int16_t* z, int al, Sink& sink) {
  sink.bits(((uint32_t)(int)z[0] >> al) & 1u, 1);
}
template <class Sink>
__host__ __device__ inline void pe_ac_first(const int16_t* z, const PeScan& sc, int slot, PeState& st, Sink& sink) {
  int r = 0;
  for (int k = sc.ss; k <= sc.se; ++k) {
    const int v = z[k];
    const uint32_t t = (uint32_t)(v < 0 ? -v : v) >> sc.al;
    if (t == 0) { ++r; continue; }
    pe_emit_eobrun(st, slot, sink);
    for (; r > 15; r -= 16) sink.sym(slot, 0xf0);
    const int n = pe_nbits(t);
    sink.sym(slot, r << 4 | n);
    sink.bits((v < 0 ? ~t : t) & ((1u << n) - 1u), n);
    r = 0;
  }
  if (r > 0) pe_end_block(st, 0, slot, sink);
}
template <class Sink>
__host__ __device__ inline void pe_ac_refine(const int16_t* z, const PeScan& sc, int slot, PeState& st, Sink& sink) {
  int eob = 0;
  for (int k = sc.ss; k <= sc.se; ++k) {
    const int v = z[k];
    if (((uint32_t)(v < 0 ? -v : v) >> sc.al) == 1u) eob = k;
  }
  int r = 0;
  uint32_t base = st.be, br = 0;                            // the block's own correction bits: corr[base .. base + br)
  for (int k = sc.ss; k <= sc.se; ++k) {
    const int v = z[k];
    const uint32_t t = (uint32_t)(v < 0 ? -v : v) >> sc.al;
    if (t == 0) { ++r; continue; }
    while (r > 15 && k <= eob) {                            // (at most three times per block)
      pe_emit_eobrun(st, slot, sink);
      sink.sym(slot, 0xf0);
      r -= 16;
      pe_emit_corr(st, base, br, sink);
      base = 0;
      br = 0;
    }
    if (t > 1) {                                            // already non-zero: one more bit of it, buffered
      st.set(base + br, t & 1u);
      ++br;
      continue;
    }
    pe_emit_eobrun(st, slot, sink);
    sink.sym(slot, r << 4 | 1);
    sink.bits(v < 0 ? 0u : 1u, 1);
    pe_emit_corr(st, base, br, sink);
    base = 0;
    br = 0;
    r = 0;
  }
  if (r > 0 || br > 0) pe_end_block(st, br, slot, sink);     // (base is st.be: either never reset, or both are zero)
}

// One restart interval of a scan (the whole scan without restarts): blocks [j0, j0 + n) of the walk.
template <class Sink>
__host__ __device__ inline void pe_code_interval(const PeWalk& w, const PeScan& sc, int scan, int64_t j0, int64_t n, PeState& st, Sink& sink) {
  st.reset();
  for (int64_t j = j0; j < j0 + n; ++j) {
    int ci;
    const int16_t* z = w.block(j, ci);
    if (sc.ss == 0) {
      if (sc.ah == 0) pe_dc_first(z, ci, sc.al, ci ? PE_DC1_SLOT : scan, st, sink);
      else pe_dc_refine(z, sc.al, sink);
    } else if (sc.ah == 0) {
      pe_ac_first(z, sc, scan, st, sink);
    } else {
      pe_ac_refine(z, sc, scan, st, sink);
    }
  }
  pe_emit_eobrun(st, scan, sink);
}

// ---- block by block: what the kernels run ----------------------------------------------------------------------
// pe_code_interval above is the reference order: one walk with the run carried from block to block.  The device cuts that
// dependency in two steps.  A SUMMARY of every block of an AC scan says what the run needs to know of it; one walk over the
// summaries of an interval (pe_resolve_step, no coefficient read) gives the run's state IN FRONT of every block; with that
// state a block is coded on its own (pe_code_block), the blocks of an interval in any order.
constexpr uint32_t PE_SUM_SYM = 0x80;                    // the block codes a symbol of its own (which writes a pending run out first)
constexpr uint32_t PE_SUM_RUN = 0x40;                    // it ends in zeros or correction bits: the run grows by it
constexpr uint32_t PE_SUM_TAIL = 0x3f;                   // correction bits behind its last symbol: they wait behind the run
__host__ __device__ inline uint32_t pe_summary_of(unsigned long long newly, unsigned long long nonzero, const PeScan& sc) {
  // newly / nonzero: per zigzag position of the band, |coefficient| >> Al is 1 / is not 0
  const unsigned long long last = 1ull << sc.se;
  if (sc.ah == 0) return (nonzero ? PE_SUM_SYM : 0u) | ((nonzero & last) ? 0u : PE_SUM_RUN);
  const unsigned long long big = nonzero & ~newly;
  const unsigned long long behind = newly ? ~((2ull << (63 - __builtin_clzll(newly))) - 1ull) : ~0ull;
  return (newly ? PE_SUM_SYM : 0u) | ((newly & last) ? 0u : PE_SUM_RUN) | (uint32_t)__builtin_popcountll(big & behind);
}
__host__ __device__ inline uint32_t pe_summary(const int16_t* z, const PeScan& sc) {
  unsigned long long newly = 0, nonzero = 0;
  for (int k = sc.ss; k <= sc.se; ++k) {
    const int v = z[k];
    const uint32_t t = (uint32_t)(v < 0 ? -v : v) >> sc.al;
    if (t) nonzero |= 1ull << k;
    if (t == 1u && sc.ah) newly |= 1ull << k;
  }
  return pe_summary_of(newly, nonzero, sc);
}
struct PeRun {
  uint32_t e, be;                      // EOBRUN and the number of correction bits behind it
};
// the run in front of a block -> the run behind it: jcphuff.c's counters without the bits
__host__ __device__ inline void pe_resolve_step(uint32_t sum, PeRun& r) {
  const uint32_t tail = sum & PE_SUM_TAIL;
  if (sum & PE_SUM_SYM) {
    r.e = (sum & PE_SUM_RUN) ? 1u : 0u;
    r.be = (sum & PE_SUM_RUN) ? tail : 0u;
  } else {
    ++r.e;
    r.be += tail;
    if (r.e == PE_EOBRUN_MAX || r.be > PE_BE_LIMIT) r.e = r.be = 0u;
  }
}
// whether the block writes the run in front of it out: with a symbol, at the limits, or at the interval's end
__host__ __device__ inline bool pe_will_emit(uint32_t sum, const PeRun& pre, bool last) {
  return (sum & PE_SUM_SYM) || last || pre.e + 1u == PE_EOBRUN_MAX || pre.be + (sum & PE_SUM_TAIL) > PE_BE_LIMIT;
}
// The correction bits that wait in front of block j: the tails of the run's blocks, oldest first, taken from the coefficients
// again.  summary: of the interval's blocks, [0] is block j0.  At most PE_MAX_CORR_BITS bits, so at most that many blocks.
__host__ __device__ inline void pe_pending(const PeWalk& w, const PeScan& sc, const uint8_t* summary, int64_t j0, int64_t j, uint32_t be, PeState& st) {
  int64_t s = j;
  for (uint32_t have = 0; have < be && s > j0;) have += summary[--s - j0] & PE_SUM_TAIL;
  uint32_t n = 0;
  for (; s < j; ++s) {
    if (!(summary[s - j0] & PE_SUM_TAIL)) continue;
    int ci;
    const int16_t* z = w.block(s, ci);
    int eob = 0;
    for (int k = sc.ss; k <= sc.se; ++k) {
      const int v = z[k];
      if (((uint32_t)(v < 0 ? -v : v) >> sc.al) == 1u) eob = k;
    }
    for (int k = eob + 1 > sc.ss ? eob + 1 : sc.ss; k <= sc.se; ++k) {
      const int v = z[k];
      const uint32_t t = (uint32_t)(v < 0 ? -v : v) >> sc.al;
      if (t > 1u) st.set(n++, t & 1u);
    }
  }
}
// the block whose DC value block j's difference is taken to; -1: none (the interval starts at j0)
__host__ __device__ inline int64_t pe_dc_previous(const PeWalk& w, int64_t j0, int64_t j) {
  if (w.comp >= 0) return j > j0 ? j - 1 : -1;
  const int s = (int)(j % w.bpm);
  const int64_t p = (s > 0 && s < w.ny) ? j - 1 : (s == 0 ? j - w.bpm + w.ny - 1 : j - w.bpm);
  return j - s - w.bpm >= j0 || (s > 0 && s < w.ny) ? p : -1;
}
// Block j of the interval [j0, j0 + n) on its own; pre: the run in front of it (pe_resolve_step over the blocks before it).
template <class Sink>
__host__ __device__ inline void pe_code_block(const PeWalk& w, const PeScan& sc, int scan, int64_t j0, int64_t n, int64_t j, const uint8_t* summary,
                                              const PeRun& pre, PeState& st, Sink& sink) {
  st.reset();
  int ci;
  const int16_t* z = w.block(j, ci);
  if (sc.ss == 0) {
    if (sc.ah) { pe_dc_refine(z, sc.al, sink); return; }
    const int64_t p = pe_dc_previous(w, j0, j);
    int pc;
    if (p >= 0) st.last_dc[ci] = (int)w.block(p, pc)[0] >> sc.al;
    pe_dc_first(z, ci, sc.al, ci ? PE_DC1_SLOT : scan, st, sink);
    return;
  }
  const bool last = j == j0 + n - 1;
  const uint32_t sum = summary[j - j0];
  st.eobrun = pre.e;
  st.be = pre.be;
  if (pre.be && pe_will_emit(sum, pre, last)) pe_pending(w, sc, summary, j0, j, pre.be, st);
  if (sc.ah == 0) pe_ac_first(z, sc, scan, st, sink);
  else pe_ac_refine(z, sc, scan, st, sink);
  if (last) pe_emit_eobrun(st, scan, sink);
}

// The byte writer of the one walk (the host program's reference; the kernels OR every block's bits to their place and stuff in
// the write launch): code words from the image's tables, bytes stuffed as they leave, 1-bits behind the interval's end.
// Nothing is written at or behind `cap`: pe_interval_bytes keeps the count below it, the check guards the memory.
struct PeByteSink {
  const JoTable* tables;               // [PE_SLOTS]
  uint8_t* out;
  uint32_t cap, n;
  uint64_t acc;
  int nacc;
  __host__ __device__ void byte(uint32_t b) {
    if (n < cap) out[n] = (uint8_t)b;
    ++n;
  }
  __host__ __device__ void bits(uint32_t v, int nb) {
    acc = acc << nb | v;
    nacc += nb;
    while (nacc >= 8) {
      const uint32_t b = (uint32_t)(acc >> (nacc - 8)) & 255u;
      nacc -= 8;
      byte(b);
      if (b == 255u) byte(0);
    }
  }
  __host__ __device__ void sym(int slot, int s) {
    const uint32_t c = tables[slot].code[s & 255];
    bits(c & 0xffffu, (int)(c >> 16));
  }
  __host__ __device__ void finish() {
    if (nacc) bits((1u << (8 - nacc)) - 1u, 8 - nacc);
  }
};

// ---- what the planner leaves in the table (attwarp_jpegenc_header::reserved is the record's offset / 16) -----------------------
struct PePlan {                        // then PeImage[nimages], PeSeg[nsegs]; the transform units of the images lie behind the
  int32_t nimages, nsegs;              // call's other units (attwarp_jpegenc_header::nunits counts only those)
  int32_t ntunits, pad;
  uint64_t off_images, off_segs;       // in the table
  uint64_t off_hist, off_tables, off_seg_out;   // scratch: uint32 [nimages][PE_SLOTS][256], JoTable [nimages][PE_SLOTS], PeSegOut[nsegs]
};
static_assert(sizeof(PePlan) == 56, "record layout");

struct PeScanPlan {
  int32_t seg0, nsegs;                 // the scan's intervals among the image's segments
  int32_t wc, dri;                     // blocks per row of its walk (interleaved: unused); the DRI value in front of it, 0: none
};
struct PeImage {
  int32_t image, nscans;
  int32_t seg0, nsegs;                 // its segments among the plan's, scan by scan
  int32_t header_len, pad;             // JeImageDev::header holds SOI .. SOF2
  PeScanPlan scan[PE_MAX_SCANS];
};
static_assert(sizeof(PeImage) == 24 + 16 * PE_MAX_SCANS, "record layout");

struct PeSeg {                         // one restart interval of one scan
  int32_t pimage, scan;                // index among the progressive images
  int32_t block0, nblocks;             // of the scan's walk
  int32_t index, cap;                  // interval in its scan; bytes its bits take at most before stuffing (pe_interval_bytes / 2)
  uint64_t slot_off;                   // scratch: its bits, big-endian words (cap + 8 bytes, 16-byte aligned)
  uint64_t aux_off;                    // scratch, per block of the interval: uint64 bit position [n], uint32 run in front [n], uint8 summary [n]
};
static_assert(sizeof(PeSeg) == 40, "record layout");
static_assert(PE_DHT_MAX <= JO_DHT_BYTES && PE_DHT_MAX == 21 + 256, "a DHT of 256 symbols fits JoTable::dht and is what the bound counts");
static_assert(PE_SUM_TAIL >= 63, "a block buffers at most 63 correction bits");
static_assert(PE_EOBRUN_MAX < (1u << 16) && PE_MAX_CORR_BITS < (1 << 16), "the run in front of a block packs into one word");
__host__ __device__ inline uint64_t pe_aux_bytes(uint64_t n) { return (13u * n + 15u) / 16u * 16u; }

struct PeSegOut {
  uint32_t nbytes, nff;                // (code) bytes of the interval before stuffing, padding included; the FF among them
  uint64_t fpos;                       // (place) where the interval's part of the file starts: what precedes its bytes included
};

}  // namespace attwarp
