// Pieces of the JPEG encoder (jpegenc.hip) shared by its kernels, its host planner and the host test
// (tests/jpegenc_host_main.cpp): the table layouts, libjpeg's colour conversion, the islow forward DCT, the exact
// quantiser, the Annex K Huffman tables and one block's sample fetch with the edge rule.  Restated by tests/jpegenc_ref.py.
#pragma once
#include "common.hpp"

namespace attwarp {

constexpr int JE_NT = 256;                               // threads per workgroup of every kernel but the transform
constexpr int JE_TNT = 128;                              // threads of the transform kernel: one per block of a unit
constexpr int JE_UNIT_MCUS = ATTWARP_JPEGENC_UNIT_MCUS;  // MCUs per entropy unit at most
constexpr int JE_UNIT_BLOCKS = JE_UNIT_MCUS * 6;         // blocks per unit at most (4:2:0)
constexpr int JE_BLOCK_MAX_BITS = 22 + 63 * 27;          // DC 11 + 11, every AC a 16-bit symbol and category 11 at most
constexpr int JE_BLOCK_WORDS = (JE_BLOCK_MAX_BITS + 31) / 32;
constexpr int JE_UNIT_WORDS = JE_UNIT_BLOCKS * JE_BLOCK_WORDS + 2;   // a unit's bits in LDS and two spill words
constexpr int JE_HEADER_MAX = 640;                       // SOI .. SOS of a three-component file with DRI: 629 bytes
constexpr int JE_MAX_DIM = ATTWARP_JPEGENC_MAX_DIM;
static_assert(JE_UNIT_BLOCKS <= JE_TNT, "one transform thread per block");
static_assert(JE_UNIT_WORDS * 4 < 48 * 1024, "the unit's bits stay well inside the static LDS");

struct JeImageDev {                    // the per-image record of a planned table
  const uint8_t* src;
  int32_t H, W, C, pitch, swap;
  int32_t hmax, vmax, bpm;             // sampling factors of the luma component, blocks per MCU
  int32_t mcus_x, nmcu;
  int32_t interval, nint, upi;         // MCUs per restart interval (nmcu without restarts), intervals, units per full interval
  int32_t unit0, nunits;
  int32_t header_len, block_bits;      // bytes of SOI .. SOS; bits one block takes at most at this image's quality
  int32_t opt;                         // 0, or 1 + the image's index among the optimised ones (jpegopt_blocks.hpp)
  uint64_t coef_off, ustream_off;     // scratch: zigzag int16 coefficients of every block; the unstuffed stream
  uint16_t divisor[2][64];             // q << 3, natural order, luma and chroma
  uint32_t recip[2][64];               // ceil(2^32 / divisor)
  uint8_t header[JE_HEADER_MAX];
};
static_assert(sizeof(JeImageDev) % 8 == 0, "record layout");

struct JeUnit {                        // one work item of the transform, entropy, gather and write kernels
  int32_t image, mcu0, nmcu, interval; // interval: index of the restart interval the unit lies in
  int32_t last, index;                 // last: the last unit of its interval; index in the image
  uint64_t slot_off;                   // scratch: where the unit's bits go (16-byte aligned)
};
static_assert(sizeof(JeUnit) == 32, "record layout");

struct JeUnitOut {                     // what the kernels leave per unit at the start of the scratch buffer
  uint32_t bits;                       // (entropy) length of the unit's bit string
  uint32_t nbytes, nff, upos;          // (gather) bytes of the unstuffed stream the unit owns, the FF among them, and where
                                       // they start in the image's unstuffed stream (read by the write kernel)
  uint64_t pre;                        // (scan A) bits of the image's earlier units
  uint64_t fpos;                       // (scan B) where the unit's stuffed bytes start, behind the file's header
};
static_assert(sizeof(JeUnitOut) == 32, "record layout");

// The parts of a planned table: its header, image i, unit i.
__host__ __device__ inline const attwarp_jpegenc_header* je_header(const uint8_t* table) {
  return reinterpret_cast<const attwarp_jpegenc_header*>(table);
}
__host__ __device__ inline const JeImageDev* je_image(const uint8_t* table, int i) {
  return reinterpret_cast<const JeImageDev*>(table + je_header(table)->off_images) + i;
}
__host__ __device__ inline const JeUnit& je_unit(const uint8_t* table, int i) {
  return reinterpret_cast<const JeUnit*>(table + je_header(table)->off_units)[i];
}

__host__ __device__ inline int je_min(int a, int b) { return a < b ? a : b; }

// ---- Annex K ---------------------------------------------------------------------------------------------------------------
// natural index of zigzag position k
__host__ __device__ inline int je_zigzag(int k) {
  constexpr uint8_t Z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return Z[k];
}
static const uint8_t JE_STD_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// BITS and VALS in the order of the DHT segments: DC 0, AC 0, DC 1, AC 1
static const uint8_t JE_BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                       {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                       {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                       {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t JE_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t JE_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
     0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
     0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
     0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
     0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
     0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
     0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
     0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
     0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
     0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
     0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
     0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
inline const uint8_t* je_vals(int t) { return (t & 1) ? JE_AC_VALS[t >> 1] : JE_DC_VALS; }
inline int je_nvals(int t) { return (t & 1) ? 162 : 12; }

// T.81 Annex C: table t (DHT order) -> code[symbol] = length << 16 | code, 0 for a symbol without a code
inline void je_build_huffman(int t, uint32_t (&code)[256]) {
  for (int s = 0; s < 256; ++s) code[s] = 0;
  uint32_t c = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < JE_BITS[t][len - 1]; ++i) code[je_vals(t)[k++]] = (uint32_t)len << 16 | c++;
    c <<= 1;
  }
}

// jpeg_quality_scaling and jpeg_add_quant_table with force_baseline: table 0 / 1, natural order
inline int je_quant_value(int quality, int table, int k) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = (JE_STD_Q[table][k] * scale + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}
inline uint32_t je_recip(uint32_t divisor) { return (uint32_t)((((uint64_t)1 << 32) + divisor - 1) / divisor); }

inline int je_bit_length(uint32_t v) {
  int n = 0;
  while (v) { ++n; v >>= 1; }
  return n;
}
// Bits one block takes at most at a quality (the derivation is DESIGN.md 3.20's): DC code and low bits 11 + 11; per AC
// position a symbol of at most 16 bits and the largest category its quantiser leaves of a coefficient below 1024 + 2.
inline int je_block_bound_bits(int quality, int ncomp) {
  int worst = 0;
  for (int t = 0; t < (ncomp == 3 ? 2 : 1); ++t) {
    int bits = 22;
    for (int k = 1; k < 64; ++k) {
      const uint32_t q = (uint32_t)je_quant_value(quality, t, k);
      bits += 16 + je_bit_length((1026u + (q >> 1)) / q);
    }
    worst = bits > worst ? bits : worst;
  }
  return worst;
}

// ---- colour: libjpeg's 16-bit fixed point --------------------------------------------------------------------------------------
__host__ __device__ inline int je_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__host__ __device__ inline int je_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__host__ __device__ inline int je_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// ---- quantisation: sign(c) * ((|c| + (d >> 1)) / d), the division by a multiplication with ceil(2^32 / d) ---------------------
// Exact while (|c| + d / 2) * (d - 1) < 2^32: the host test runs every divisor 8 .. 2040 against every coefficient the DCT gives.
__host__ __device__ inline int je_quantize(int c, uint32_t divisor, uint32_t recip) {
  const uint32_t mag = (uint32_t)(c < 0 ? -c : c) + (divisor >> 1);
  const int q = (int)(uint32_t)(((uint64_t)mag * recip) >> 32);
  return c < 0 ? -q : q;
}

// ---- jfdctint.c (islow): 64 samples with 128 subtracted, in place, row pass then column pass; output scaled by 8 ---------------
template <bool FIRST>
__host__ __device__ inline void je_fdct_1d(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
  int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d0 = FIRST ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;
  d4 = FIRST ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;
  int z1 = (t12 + t13) * 4433;
  d2 = (z1 + t13 * 6270 + R) >> N;
  d6 = (z1 - t12 * 15137 + R) >> N;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d7 = (t4 + z1 + z3 + R) >> N;
  d5 = (t5 + z2 + z4 + R) >> N;
  d3 = (t6 + z2 + z3 + R) >> N;
  d1 = (t7 + z1 + z4 + R) >> N;
}
__host__ __device__ inline void je_fdct(int (&d)[64]) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    je_fdct_1d<true>(d[8 * r], d[8 * r + 1], d[8 * r + 2], d[8 * r + 3], d[8 * r + 4], d[8 * r + 5], d[8 * r + 6], d[8 * r + 7]);
#pragma unroll
  for (int c = 0; c < 8; ++c)
    je_fdct_1d<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
}

// ---- one block's samples (minus 128) with the edge rule --------------------------------------------------------------------------
// comp 0: block (col, row) of the luma (or grey) plane, pixels clamped to the image.  comp 1 / 2: block (col, row) of Cb / Cr:
// a down-sampled row below the last real one (ceil(H / vmax) - 1) repeats THAT row; inside it, the input rows and columns are
// clamped to the image.  h2v1: (a + b + bias) >> 1 with bias 0, 1, 0, 1 ...; h2v2: (a + b + c + d + bias) >> 2 with 1, 2, 1, 2 ....
struct JeSrc {
  const uint8_t* p;
  int64_t pitch;
  int H, W, C, hmax, vmax;
  bool swap;
  __host__ __device__ inline int chroma(int comp, int y, int x) const {
    const uint8_t* q = p + (int64_t)y * pitch + 3 * (int64_t)x;
    const int r = q[swap ? 2 : 0], g = q[1], b = q[swap ? 0 : 2];
    return comp == 1 ? je_cb(r, g, b) : je_cr(r, g, b);
  }
  __host__ __device__ inline void block(int comp, int col, int row, int (&d)[64]) const {
    if (comp == 0) {
      for (int y = 0; y < 8; ++y) {
        const int yy = je_min(row * 8 + y, H - 1);
        const uint8_t* line = p + (int64_t)yy * pitch;
        for (int x = 0; x < 8; ++x) {
          const int xx = je_min(col * 8 + x, W - 1);
          int v;
          if (C == 1) v = line[xx];
          else v = je_y(line[3 * xx + (swap ? 2 : 0)], line[3 * xx + 1], line[3 * xx + (swap ? 0 : 2)]);
          d[8 * y + x] = v - 128;
        }
      }
      return;
    }
    const int last = (H + vmax - 1) / vmax - 1;
    for (int y = 0; y < 8; ++y) {
      const int rc = je_min(row * 8 + y, last);
      const int y0 = je_min(rc * vmax, H - 1), y1 = je_min(rc * vmax + vmax - 1, H - 1);
      for (int x = 0; x < 8; ++x) {
        const int c = col * 8 + x;
        const int x0 = je_min(c * hmax, W - 1), x1 = je_min(c * hmax + hmax - 1, W - 1);
        int v;
        if (hmax == 1) v = chroma(comp, y0, x0);
        else if (vmax == 1) v = (chroma(comp, y0, x0) + chroma(comp, y0, x1) + (x & 1)) >> 1;
        else v = (chroma(comp, y0, x0) + chroma(comp, y0, x1) + chroma(comp, y1, x0) + chroma(comp, y1, x1) + 1 + (x & 1)) >> 2;
        d[8 * y + x] = v - 128;
      }
    }
  }
};

// Slot s of an MCU -> component, and for luma the block's place in the MCU.  A luma block outside the component's real blocks
// (wb x hb) is a dummy: no AC and the DC of slot `src` (resolved to a real block: the block before it in the MCU, and for a
// whole dummy row the last block of the row above, itself a dummy when the MCU is in the last column too).
struct JeSlot {
  int comp, bx, by, src;               // src < 0: a real block
};
__host__ __device__ inline JeSlot je_slot(int s, int hmax, int vmax, int ncomp, int mcu_x, int mcu_y, int wb, int hb) {
  JeSlot o;
  const int ny = ncomp == 3 ? hmax * vmax : 1;
  o.src = -1;
  if (s >= ny) { o.comp = s - ny + 1; o.bx = 0; o.by = 0; return o; }
  o.comp = 0;
  o.bx = s % hmax;
  o.by = s / hmax;
  const bool right = mcu_x * hmax + o.bx >= wb, below = mcu_y * vmax + o.by >= hb;
  if (below) o.src = (mcu_x * hmax + hmax - 1 < wb) ? o.by * hmax - 1 : (o.by - 1) * hmax;   // (by >= 1: the MCU's first row is real)
  else if (right) o.src = s - 1;                                                            // (bx >= 1 likewise)
  return o;
}

}  // namespace attwarp
