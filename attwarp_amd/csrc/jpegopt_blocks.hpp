// Per-image optimised Huffman tables of the JPEG encoder (jpegenc.hip), shared by the table kernel, the host
// planner and the host test (tests/jpegopt_host_main.cpp): the records the planner and the kernels exchange, and libjpeg's
// jpeg_gen_optimal_table, written once for a wave of NL lanes (the device: 64) and for one lane (the host: the same text).
// Restated by tests/jpegopt_ref.py.
#pragma once
#include "jpegenc_blocks.hpp"

namespace attwarp {

constexpr int JO_LEAVES = 257;                           // 256 symbols and the reserved leaf, which keeps the all-ones code free
constexpr int JO_MAX_DEPTH = JO_LEAVES - 1;              // the deepest code a tree of 257 leaves can hold
constexpr uint32_t JO_SENTINEL = 1000000000u;            // libjpeg's search starts here: a larger frequency is never selected
constexpr int JO_DHT_BYTES = 280;                        // marker, length, class / id, 16 counts, at most 256 symbols: 277
constexpr int JO_SYMBOLS_PER_BLOCK = 64;                 // one DC symbol; every AC symbol (F0 and EOB too) spends a position
// An optimised DC table codes 12 categories and the reserved leaf, so its longest code has 12 bits where Annex K's has 11 (and
// a depth of 12 needs no limiting); an AC code stays within 16.  The LDS of the entropy kernel holds the longer block too.
constexpr int JO_EXTRA_BLOCK_BITS = 1;
static_assert((JE_BLOCK_MAX_BITS + JO_EXTRA_BLOCK_BITS + 31) / 32 == JE_BLOCK_WORDS, "an optimised block fits the words of a standard one");
// At most 12 and 162 symbols per DHT, the numbers of Annex K's tables: an optimised header is never longer than the standard one.
static_assert(JE_HEADER_MAX >= 629, "the header of an optimised file fits JeImageDev::header");

struct JoPlan {                        // in the table at attwarp_jpegenc_header::off_optimize; then JoImage[nimages], int32 unit[nunits]
  int32_t nimages, nunits;             // optimised images; their units (indices into the table's units), in order
  uint64_t off_hist, off_out;          // scratch: uint32 [nimages][4][256] histograms (DHT order), JoImageOut[nimages]
};
static_assert(sizeof(JoPlan) == 24, "record layout");

struct JoImage {
  int32_t image;                       // index into the images of the call
  int32_t pre_len, suf_len;            // JeImageDev::header holds SOI .. SOF0 (pre_len bytes), then DRI / SOS (suf_len bytes)
  int32_t ntables;                     // 2: grey, 4: colour
};
static_assert(sizeof(JoImage) == 16, "record layout");

struct JoTable {                       // what the table kernel leaves per (image, table)
  uint32_t code[256];                  // length << 16 | code, 0 for a symbol without one: je_build_huffman's packing
  uint8_t dht[JO_DHT_BYTES];           // the DHT segment, marker included
  int32_t dht_len, depth, nsym, pad;   // depth: the longest code BEFORE limiting
};
struct JoImageOut {
  JoTable table[4];
  uint8_t header[JE_HEADER_MAX];       // SOI .. SOS with this image's DHTs spliced in
  int32_t header_len, pad;
};
static_assert(sizeof(JoTable) % 8 == 0 && sizeof(JoImageOut) % 8 == 0, "record layout");

// What one lane of the search needs besides its frequencies: arrays only lane 0 touches (the device: LDS of its wave).
struct JoWork {
  int16_t others[JO_LEAVES];
  uint16_t codesize[JO_LEAVES];
  int32_t bits[JO_MAX_DEPTH + 2];      // codes per length, sized for the deepest tree (libjpeg: 33 entries, and an overflow behind them)
  int32_t first[JO_MAX_DEPTH + 2];
};

// jpeg_gen_optimal_table (jchuff.c) for the histogram hist[256] -> out.  Lane `lane` of NL holds the frequencies of the leaves
// lane, lane + NL, ...; wave_min(key) gives every lane the smallest key of all lanes (NL = 1: the key itself).  The two
// smallest non-zero frequencies, ties to the LARGER index, are merged until one tree is left; the chain walks that bump the
// code sizes, the limiter and the listing run on lane 0.  Every loop is bounded by a constant.
template <int NL, class WaveMin>
__host__ __device__ inline void jo_optimal_table(const uint32_t* hist, int class_id, int lane, WaveMin wave_min, JoWork& w, JoTable& out) {
  constexpr int PER = (JO_LEAVES + NL - 1) / NL;
  constexpr uint64_t NONE = ~(uint64_t)0;
  uint32_t f[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = lane + NL * k;
    f[k] = i < 256 ? hist[i] : (i == 256 ? 1u : 0u);        // the reserved leaf: frequency 1
  }
  if (lane == 0)
    for (int i = 0; i < JO_LEAVES; ++i) { w.others[i] = -1; w.codesize[i] = 0; }
  for (int round = 0; round < JO_LEAVES - 1; ++round) {     // 257 leaves: at most 256 merges
    // key: frequency, then 511 - index, so that the smallest key is the smallest frequency at the largest index
    uint64_t best = NONE;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = lane + NL * k;
      const uint64_t key = (uint64_t)f[k] << 16 | (uint32_t)(511 - i);
      if (i < JO_LEAVES && f[k] && f[k] <= JO_SENTINEL && key < best) best = key;
    }
    const uint64_t k1 = wave_min(best);
    best = NONE;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = lane + NL * k;
      const uint64_t key = (uint64_t)f[k] << 16 | (uint32_t)(511 - i);
      if (i < JO_LEAVES && f[k] && f[k] <= JO_SENTINEL && key != k1 && key < best) best = key;
    }
    const uint64_t k2 = wave_min(best);
    if (k2 == NONE) break;                                  // (the same on every lane)
    const int c1 = 511 - (int)(k1 & 0xffffu), c2 = 511 - (int)(k2 & 0xffffu);
    const uint32_t sum = (uint32_t)(k1 >> 16) + (uint32_t)(k2 >> 16);     // (below 2^32: the planner bounds an image's symbols)
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = lane + NL * k;
      if (i == c1) f[k] = sum;
      if (i == c2) f[k] = 0;
    }
    if (lane == 0) {
      int c = c1;
      ++w.codesize[c];
      for (int g = 0; g < JO_LEAVES && w.others[c] >= 0; ++g) { c = w.others[c]; ++w.codesize[c]; }
      w.others[c] = (int16_t)c2;
      c = c2;
      ++w.codesize[c];
      for (int g = 0; g < JO_LEAVES && w.others[c] >= 0; ++g) { c = w.others[c]; ++w.codesize[c]; }
    }
  }
  if (lane != 0) return;
  for (int i = 0; i < JO_MAX_DEPTH + 2; ++i) { w.bits[i] = 0; w.first[i] = 0; }
  int depth = 0;
  for (int i = 0; i < JO_LEAVES; ++i) {
    const int n = w.codesize[i] <= JO_MAX_DEPTH ? w.codesize[i] : JO_MAX_DEPTH;   // (a leaf is merged at most 256 times)
    if (!n) continue;
    ++w.bits[n];
    if (i < 256) ++w.first[n];
    depth = n > depth ? n : depth;
  }
  // libjpeg's limiter from the deepest length down: two codes of length i lose their last bit and share the prefix (one code of
  // length i - 1); the other goes below a code of the longest shorter length j, which becomes two of length j + 1.  The code
  // stays complete, so the deepest length always holds an even number of codes.
  for (int i = JO_MAX_DEPTH; i > 16; --i)
    for (int g = 0; g < JO_LEAVES && w.bits[i] > 0; ++g) {
      int j = i - 2;
      while (j > 0 && w.bits[j] == 0) --j;
      if (j == 0) break;                                    // (never: 257 leaves cannot all be 16 bits deep or deeper)
      w.bits[i] -= 2;
      ++w.bits[i - 1];
      w.bits[j + 1] += 2;
      --w.bits[j];
    }
  int last = 16;
  while (last > 1 && w.bits[last] == 0) --last;
  if (w.bits[last] > 0) --w.bits[last];                     // the reserved leaf leaves the longest used length
  // symbols by code size, then by value: a counting sort over the sizes before limiting
  int nsym = 0;
  for (int i = 1; i <= JO_MAX_DEPTH; ++i) {
    const int n = w.first[i];
    w.first[i] = nsym;
    nsym += n;
  }
  uint8_t* vals = out.dht + 21;
  for (int s = 0; s < 256; ++s)
    if (w.codesize[s]) vals[w.first[w.codesize[s] <= JO_MAX_DEPTH ? w.codesize[s] : JO_MAX_DEPTH]++] = (uint8_t)s;
  out.dht[0] = 0xff;
  out.dht[1] = 0xc4;
  out.dht[2] = (uint8_t)((19 + nsym) >> 8);
  out.dht[3] = (uint8_t)((19 + nsym) & 255);
  out.dht[4] = (uint8_t)class_id;
  for (int k = 1; k <= 16; ++k) out.dht[4 + k] = (uint8_t)w.bits[k];
  for (int s = 0; s < 256; ++s) out.code[s] = 0;
  uint32_t c = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < w.bits[len] && k < nsym; ++i) out.code[vals[k++]] = (uint32_t)len << 16 | c++;
    c <<= 1;
  }
  out.dht_len = 21 + nsym;
  out.depth = depth;
  out.nsym = nsym;
  out.pad = 0;
}

struct JoOneLane {
  __host__ __device__ uint64_t operator()(uint64_t v) const { return v; }
};

}  // namespace attwarp
