// JPEG files of a whole ragged batch of uint8 images, written on the device (include/attwarp.h): the bytes of
// Pillow's Image.save(f, "JPEG", quality, subsampling, restart_marker_rows).  Seven launches, none with a host-dependent argument:
//   jpegenc_transform_kernel  one workgroup per UNIT (at most 16 MCUs of one restart interval, planned on the host), one thread
//                             per block: colour, edge replication, down-sampling, islow DCT, quantisation -> zigzag int16
//                             coefficients in the scratch buffer (a dummy block: the DC of the block it repeats, no AC);
//   jpegenc_entropy_kernel    one workgroup per unit, one wave per block, one lane per coefficient: a ballot gives the non-zero
//                             mask, a bit scan the zero run, a wave prefix sum the place of every lane's bits, which are ORed
//                             into zeroed LDS words -> the unit's bit string and its length;
//   jpegenc_scan_bits_kernel  one workgroup per image: prefix sums of the units' bit lengths;
//   jpegenc_gather_kernel     one workgroup per unit: the bytes of its interval's stream that START in the unit, shifted out of
//                             the unit's (and, for the last one, its successors') bit strings, 1-bits behind the interval's end
//                             -> the unstuffed stream; counts the FF bytes among them;
//   jpegenc_scan_bytes_kernel one workgroup per image: prefix sums of bytes + FF bytes + markers, the file's length;
//   jpegenc_scan_files_kernel one workgroup: prefix sums of the files' lengths -> offsets[B + 1];
//   jpegenc_write_kernel      one workgroup per unit: stuffed bytes to their place, RSTn behind an interval, the header before
//                             the first unit, EOI behind the last.
// A file with restart markers takes the same route: an interval is a stretch at whose start the bit offset returns to zero.
// Every loop is bounded by a constant or by a size the planner checked; tests/jpegenc_ref.py restates the byte stream.
// A call with optimised images (attwarp_jpegenc_plan_ex) puts three launches between the first two, which
// work on those images alone and whose results the later launches read from the scratch buffer:
//   jpegopt_clear_kernel      one workgroup per optimised image: its four symbol histograms to zero;
//   jpegopt_histogram_kernel  one workgroup per unit of an optimised image: the symbols the entropy kernel would code (the same
//                             derivation, je_lane_symbol), counted in LDS, the non-zero counts added to the image's histograms;
//   jpegopt_tables_kernel     one workgroup per optimised image, one wave per table: libjpeg's optimal table (jpegopt_blocks.hpp),
//                             its code words and DHT segment; then the header with the DHTs spliced in.
// tests/jpegopt_ref.py restates the tables.
// A call with progressive images (attwarp_jpegenc_plan_prog) transforms them with the others; none of the six
// launches above touches them further (they own no entropy unit).  Eight launches of their own write their files, all scans of
// all images at once, per SEGMENT = (scan, restart interval) and inside it per block (jpegprogenc_blocks.hpp):
//   jpegprogenc_clear_kernel     one workgroup per progressive image: its eleven symbol histograms to zero;
//   jpegprogenc_summary_kernel   one workgroup per segment of an AC scan, one wave per block, one lane per coefficient: two
//                                ballots say whether the block codes a symbol, whether it ends in the run, and how many
//                                correction bits it leaves behind the run;
//   jpegprogenc_resolve_kernel   one lane per segment: the walk over the summaries (no coefficient) that splits the end-of-band
//                                runs at 0x7FFF blocks and above 937 pending bits -> the run in front of every block;
//   jpegprogenc_count_kernel     one workgroup per segment, one lane per block: jcphuff.c's coder on the block alone, its
//                                symbols counted in LDS, the counts added to the image's histograms;
//   jpegprogenc_tables_kernel    one workgroup per image, its waves over the up to ten tables (jo_optimal_table, unchanged);
//   jpegprogenc_code_kernel      one workgroup per segment, one lane per block: bit lengths and their prefix sums, then every
//                                block's bits ORed to their place in the segment's zeroed words; counts the FF bytes;
//   jpegprogenc_place_kernel     one workgroup per image: prefix sums of DHT + DRI + SOS + bytes + FF + marker, the file's length;
//   jpegprogenc_write_kernel     one workgroup per segment: what precedes the scan, the stuffed bytes, RSTn (numbered per scan) or EOI.
// tests/jpegprogenc_ref.py restates the files.
// The host side plans all three kinds at once: je_image_plan derives one image's geometry, bound and refusal (the bound entries,
// jpegenc_count and the planner call it), attwarp_jpegenc_plan_prog is je_fill_image + je_plan_units / je_plan_progressive per
// image and je_close_plans behind the last, with scratch offsets from one JeCursor; attwarp_jpegenc_encode reads the table's
// header and optional records once (je_read_table) and launches through JE_LAUNCH.  tests/test_jpegenc_recording_cpu.py
// holds the tables, bounds and refusals to a recording.
#include <algorithm>
#include <cstring>

#include "jpegprogenc_blocks.hpp"

namespace attwarp {

#define JE_G __attribute__((address_space(1)))
constexpr uint32_t JE_MAGIC = 0x474a5041u;
constexpr int JE_MAX_UNITS = 1 << 24;

struct JeImageOut {
  uint64_t bits;                       // (scan A) bits of all units of the image
  uint64_t file_bytes;                 // (scan B)
};

// exclusive prefix sum over the JE_NT threads (tmp: JE_NT values)
template <typename T>
__device__ __forceinline__ T je_excl_sum(T v, T* tmp, T& total) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  for (int o = 1; o < JE_NT; o <<= 1) {
    const T a = t >= o ? tmp[t - o] : (T)0;
    __syncthreads();
    tmp[t] += a;
    __syncthreads();
  }
  const T incl = tmp[t];
  total = tmp[JE_NT - 1];
  __syncthreads();
  return incl - v;
}

// Exclusive prefix sums over n elements, JE_NT of them at a time with a carry: value(s) is element s, put(s, sum) receives the
// sum of the elements in front of it; the total comes back on every thread (tmp: JE_NT values).
template <typename Value, typename Put>
__device__ __forceinline__ unsigned long long je_chunked_excl_sum(int n, unsigned long long* tmp, Value value, Put put) {
  unsigned long long carry = 0;
  for (int base = 0; base < n; base += JE_NT) {
    const int s = base + threadIdx.x;
    const unsigned long long v = s < n ? (unsigned long long)value(s) : 0ull;
    unsigned long long tot;
    const unsigned long long pre = carry + je_excl_sum(v, tmp, tot);
    if (s < n) put(s, pre);
    carry += tot;
  }
  return carry;
}

// The stuffing of both write kernels: the n bytes byte(i) of an unstuffed stretch go to dst with a zero behind every FF.  Every
// lane takes one run of them; the prefix sums of the runs' FF counts say where each lands (tmp: JE_NT values).
template <typename Byte>
__device__ __forceinline__ void je_stuff(Byte byte, uint32_t n, JE_G uint8_t* dst, uint32_t* tmp) {
  const uint32_t per = (n + JE_NT - 1) / JE_NT;
  const uint32_t lo = min(n, (uint32_t)threadIdx.x * per), hi = min(n, lo + per);
  uint32_t ff = 0;
  for (uint32_t i = lo; i < hi; ++i) ff += byte(i) == 255u;
  uint32_t tot;
  uint32_t at = lo + je_excl_sum(ff, tmp, tot);
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t b = byte(i);
    dst[at++] = (uint8_t)b;
    if (b == 255u) dst[at++] = 0;
  }
}

// n histogram words to zero (the clear kernels of the optimised and the progressive images)
__device__ __forceinline__ void je_clear_words(uint32_t* hist, int n) {
  for (int i = threadIdx.x; i < n; i += JE_NT) hist[i] = 0u;
}

__device__ __forceinline__ JeImageOut* je_image_out(const uint8_t* table, uint8_t* scratch) {
  return reinterpret_cast<JeImageOut*>(scratch + je_header(table)->off_image_out);
}
__device__ __forceinline__ const JeImageOut* je_image_out(const uint8_t* table, const uint8_t* scratch) {
  return reinterpret_cast<const JeImageOut*>(scratch + je_header(table)->off_image_out);
}

__device__ __forceinline__ uint32_t je_wave_incl_sum(uint32_t v) {
  const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const uint32_t a = __shfl_up(v, o, WAVE);
    if (lane >= o) v += a;
  }
  return v;
}

__device__ __forceinline__ JeSrc je_source(const JeImageDev* im) {
  JeSrc s;
  s.p = im->src;
  s.pitch = im->pitch;
  s.H = im->H; s.W = im->W; s.C = im->C; s.hmax = im->hmax; s.vmax = im->vmax;
  s.swap = im->swap != 0;
  return s;
}

// ---- 1. pixels -> quantised coefficients ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(JE_TNT) void jpegenc_transform_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  const JeUnit u = je_unit(table, blockIdx.x);
  const JeImageDev* im = je_image(table, u.image);
  const int bpm = im->bpm, i = threadIdx.x;
  if (i >= u.nmcu * bpm) return;
  const int mcu = u.mcu0 + i / bpm, s = i - (i / bpm) * bpm;
  const int my = mcu / im->mcus_x, mx = mcu - my * im->mcus_x;
  const int wb = (im->W + 7) >> 3, hb = (im->H + 7) >> 3;
  JeSlot sl = je_slot(s, im->hmax, im->vmax, im->C, mx, my, wb, hb);
  const bool dummy = sl.src >= 0;
  if (dummy) sl = je_slot(sl.src, im->hmax, im->vmax, im->C, mx, my, wb, hb);
  const int col = sl.comp ? mx : mx * im->hmax + sl.bx, row = sl.comp ? my : my * im->vmax + sl.by;
  int d[64];
  je_source(im).block(sl.comp, col, row, d);
  je_fdct(d);
  const int t = sl.comp ? 1 : 0;
  uint32_t* dst = reinterpret_cast<uint32_t*>(scratch + im->coef_off) + ((size_t)mcu * bpm + s) * 32;
#pragma unroll
  for (int k = 0; k < 64; k += 2) {
    const int n0 = je_zigzag(k), n1 = je_zigzag(k + 1);
    int a = je_quantize(d[n0], im->divisor[t][n0], im->recip[t][n0]);
    int b = je_quantize(d[n1], im->divisor[t][n1], im->recip[t][n1]);
    if (dummy) { a = k ? 0 : a; b = 0; }
    dst[k >> 1] = ((uint32_t)a & 0xffffu) | ((uint32_t)b << 16);
  }
}

// ---- 2. coefficients -> one bit string per unit ----------------------------------------------------------------------------------
// What lane k of a wave contributes to its block: nf0 codes of sixteen zeros, then `len` bits of `code` (the symbol's code and
// the value's low bits; lane 0: the DC difference; lane 63 when its coefficient is zero: the end-of-block code).
struct JeLane {
  uint32_t nf0, code, len;
};
// The symbol behind it, shared with the histogram of the optimised tables: nf0 symbols F0, then `sym` (lane 0: of the DC table,
// the difference's category; the others: run << 4 | size of the AC table, 0 = end of block) with n low bits; sym < 0: nothing.
struct JeSymbol {
  uint32_t nf0, n;
  int sym;
};
__device__ __forceinline__ JeSymbol je_lane_symbol(int lane, int v) {
  JeSymbol o = {0u, 0u, -1};
  const unsigned long long mask = __ballot(lane > 0 && v != 0);
  if (lane == 0 || v != 0) {
    const uint32_t mag = (uint32_t)(v < 0 ? -v : v);
    o.n = 32u - (uint32_t)__clz(mag);                       // (mag = 0: 32 - 32)
    if (lane == 0) o.sym = (int)o.n;
    else {
      const unsigned long long below = mask & ((1ull << lane) - 1ull);
      const int prev = below ? 63 - __clzll((long long)below) : 0;
      const uint32_t run = (uint32_t)(lane - 1 - prev);
      o.nf0 = run >> 4;
      o.sym = (int)((run & 15u) << 4 | o.n);
    }
  } else if (lane == 63) {
    o.sym = 0;
  }
  return o;
}
__device__ __forceinline__ JeLane je_lane_code(int lane, int v, const uint32_t* dc, const uint32_t* ac) {
  JeLane o = {0u, 0u, 0u};
  const JeSymbol s = je_lane_symbol(lane, v);
  if (s.sym < 0) return o;
  const uint32_t h = (lane == 0 ? dc : ac)[s.sym];
  const uint32_t low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s.n) - 1u);       // (the end of block: n = 0, no low bits)
  o.nf0 = s.nf0;
  o.code = (h & 0xffffu) << s.n | low;
  o.len = (h >> 16) + s.n;
  return o;
}
// What lane `lane` sees of block i of unit u: its zigzag coefficient; lane 0: the difference to the DC of the component's
// previous block, to zero at the start of a restart interval.  comp: the block's component.
__device__ __forceinline__ int je_block_lane_value(const int16_t* coef, const JeUnit& u, const JeImageDev* im, int i, int lane, int& comp) {
  const int bpm = im->bpm, ny = im->C == 3 ? im->hmax * im->vmax : 1;
  const int m = i / bpm, s = i - m * bpm;
  const int64_t blk = (int64_t)u.mcu0 * bpm + i;
  int v = coef[blk * 64 + lane];
  comp = s < ny ? 0 : s - ny + 1;
  const int first = comp ? s : 0, last = comp ? s : ny - 1;
  if (lane == 0) {
    int pred = 0;
    if (s > first) pred = coef[(blk - 1) * 64];
    else if ((u.mcu0 + m) % im->interval != 0) pred = coef[(blk - s - bpm + last) * 64];
    v -= pred;
  }
  return v;
}
// The optimised image's record in the scratch buffer; nullptr: the image takes the Annex K tables.
__device__ __forceinline__ const JoPlan* jo_plan(const uint8_t* table) {
  return reinterpret_cast<const JoPlan*>(table + je_header(table)->off_optimize);
}
__device__ __forceinline__ const JoImageOut* je_optimized(const uint8_t* table, const JeImageDev* im, const uint8_t* scratch) {
  if (!im->opt) return nullptr;
  return reinterpret_cast<const JoImageOut*>(scratch + jo_plan(table)->off_out) + (im->opt - 1);
}
// nbits <= 27 of `value` at bit `pos` of the big-endian words w
__device__ __forceinline__ void je_put(uint32_t* w, uint32_t pos, uint32_t value, uint32_t nbits) {
  const uint64_t x = (uint64_t)value << (64u - nbits - (pos & 31u));
  atomicOr(&w[pos >> 5], (uint32_t)(x >> 32));
  if ((uint32_t)x) atomicOr(&w[(pos >> 5) + 1], (uint32_t)x);
}

__global__ __launch_bounds__(JE_NT) void jpegenc_entropy_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_bits[JE_UNIT_WORDS];
  __shared__ uint32_t s_huff[4 * 256];
  __shared__ uint32_t s_blen[2 * WAVE], s_bstart[2 * WAVE];
  __shared__ uint32_t s_total;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const JeUnit u = je_unit(table, blockIdx.x);
  const JeImageDev* im = je_image(table, u.image);
  const uint32_t* huff = reinterpret_cast<const uint32_t*>(table + je_header(table)->off_huffman);
  const JoImageOut* opt = je_optimized(table, im, scratch);
  const int bpm = im->bpm, nblk = u.nmcu * bpm, ny = im->C == 3 ? im->hmax * im->vmax : 1;
  const int nwords = min(JE_UNIT_WORDS, (nblk * im->block_bits + 31) / 32 + 2);
  for (int i = tid; i < nwords; i += JE_NT) s_bits[i] = 0;
  if (opt) {                                                // the image's own code words (a grey image: two tables)
    const int nt = im->C == 3 ? 4 : 2;
    for (int t = 0; t < 4; ++t) s_huff[256 * t + tid] = t < nt ? opt->table[t].code[tid] : 0u;
  } else {
    for (int i = tid; i < 4 * 256; i += JE_NT) s_huff[i] = huff[i];
  }
  if (tid < 2 * WAVE) s_blen[tid] = 0;
  __syncthreads();
  const int16_t* coef = reinterpret_cast<const int16_t*>(scratch + im->coef_off);
  // the coefficient of this lane in block i of the unit; lane 0: the difference to the component's previous block
  auto lane_code = [&](int i) {
    int comp;
    const int v = je_block_lane_value(coef, u, im, i, lane, comp);
    const int t = comp ? 2 : 0;
    return je_lane_code(lane, v, s_huff + 256 * t, s_huff + 256 * (t + 1));
  };
  const uint32_t f0[2] = {s_huff[256 + 0xf0], s_huff[768 + 0xf0]};
  for (int i = wave; i < nblk; i += JE_NT / WAVE) {
    const JeLane c = lane_code(i);
    const int t = (i % bpm) < ny ? 0 : 1;
    uint32_t n = c.nf0 * (f0[t] >> 16) + c.len;
    n = je_wave_incl_sum(n);
    if (lane == WAVE - 1) s_blen[i] = n;
  }
  __syncthreads();
  if (wave == 0) {                                          // 2 x 64 >= JE_UNIT_BLOCKS block lengths -> block starts
    const uint32_t a = s_blen[2 * lane], b = s_blen[2 * lane + 1];
    const uint32_t incl = je_wave_incl_sum(a + b);
    s_bstart[2 * lane] = incl - a - b;
    s_bstart[2 * lane + 1] = incl - b;
    if (lane == WAVE - 1) s_total = incl;
  }
  __syncthreads();
  for (int i = wave; i < nblk; i += JE_NT / WAVE) {
    const JeLane c = lane_code(i);
    const int t = (i % bpm) < ny ? 0 : 1;
    const uint32_t fl = f0[t] >> 16, n = c.nf0 * fl + c.len;
    uint32_t pos = s_bstart[i] + je_wave_incl_sum(n) - n;
    for (uint32_t k = 0; k < c.nf0; ++k, pos += fl) je_put(s_bits, pos, f0[t] & 0xffffu, fl);     // (nf0 <= 3)
    if (c.len) je_put(s_bits, pos, c.code, c.len);
  }
  __syncthreads();
  // The bits above were ORed into s_bits without a check: the LDS writes rely on the planner's bound, which holds for every
  // block (coefficients stay below 1024).  The clamp guards the copy to the unit's slot in global memory only.
  const uint32_t total = min(s_total, (uint32_t)(nblk * im->block_bits));
  uint32_t* dst = reinterpret_cast<uint32_t*>(scratch + u.slot_off);
  for (uint32_t i = tid; i < (total + 31u) / 32u; i += JE_NT) dst[i] = __builtin_bswap32(s_bits[i]);
  if (tid == 0) reinterpret_cast<JeUnitOut*>(scratch)[blockIdx.x].bits = total;
}

// ---- 1a - 1c. optimised images: histograms, tables, header (launched in front of 2.) -----------------------------------------------
static_assert(JE_NT == 256 && JE_NT == 4 * WAVE, "a thread per symbol of a table, a wave per table");
__global__ __launch_bounds__(JE_NT) void jpegopt_clear_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  je_clear_words(reinterpret_cast<uint32_t*>(scratch + jo_plan(table)->off_hist) + (size_t)blockIdx.x * 4 * 256, 4 * 256);
}

__global__ __launch_bounds__(JE_NT) void jpegopt_histogram_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_hist[4 * 256];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const JoPlan* plan = jo_plan(table);
  const int32_t* list = reinterpret_cast<const int32_t*>(reinterpret_cast<const JoImage*>(plan + 1) + plan->nimages);
  const JeUnit u = je_unit(table, list[blockIdx.x]);
  const JeImageDev* im = je_image(table, u.image);
  for (int i = tid; i < 4 * 256; i += JE_NT) s_hist[i] = 0u;
  __syncthreads();
  const int16_t* coef = reinterpret_cast<const int16_t*>(scratch + im->coef_off);
  const int nblk = u.nmcu * im->bpm;
  for (int i = wave; i < nblk; i += JE_NT / WAVE) {
    int comp;
    const int v = je_block_lane_value(coef, u, im, i, lane, comp);
    const JeSymbol s = je_lane_symbol(lane, v);
    uint32_t* h = s_hist + (comp ? 512 : 0);                // DHT order: DC 0, AC 0, DC 1, AC 1
    if (s.sym >= 0) atomicAdd(&h[(lane ? 256 : 0) + (s.sym & 255)], 1u);
    if (s.nf0) atomicAdd(&h[256 + 0xf0], s.nf0);
  }
  __syncthreads();
  uint32_t* hist = reinterpret_cast<uint32_t*>(scratch + plan->off_hist) + (size_t)(im->opt - 1) * 1024;
  for (int i = tid; i < 4 * 256; i += JE_NT)
    if (s_hist[i]) atomicAdd(&hist[i], s_hist[i]);
}

struct JoWaveMin {                     // the smallest key of the wave's 64 lanes, on every lane
  __device__ __forceinline__ uint64_t operator()(uint64_t v) const {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)v, o, WAVE), hi = __shfl_xor((uint32_t)(v >> 32), o, WAVE);
      const uint64_t other = (uint64_t)hi << 32 | lo;
      v = other < v ? other : v;
    }
    return v;
  }
};

__global__ __launch_bounds__(JE_NT) void jpegopt_tables_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ JoWork s_work[JE_NT / WAVE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const JoPlan* plan = jo_plan(table);
  const JoImage oi = reinterpret_cast<const JoImage*>(plan + 1)[blockIdx.x];
  const JeImageDev* im = je_image(table, oi.image);
  const uint32_t* hist = reinterpret_cast<const uint32_t*>(scratch + plan->off_hist) + (size_t)blockIdx.x * 1024;
  JoImageOut* out = reinterpret_cast<JoImageOut*>(scratch + plan->off_out) + blockIdx.x;
  if (wave < oi.ntables) jo_optimal_table<WAVE>(hist + 256 * wave, (wave & 1) << 4 | wave >> 1, lane, JoWaveMin(), s_work[wave], out->table[wave]);
  __syncthreads();
  // SOI .. SOF0, the image's DHTs, DRI / SOS; the clamp guards the record, the symbol counts keep the header within the standard one's
  int at = oi.pre_len;
  for (int i = tid; i < oi.pre_len; i += JE_NT) out->header[i] = im->header[i];
  for (int t = 0; t < oi.ntables; ++t) {
    const int n = min(out->table[t].dht_len, JE_HEADER_MAX - oi.suf_len - at);
    for (int i = tid; i < n; i += JE_NT) out->header[at + i] = out->table[t].dht[i];
    at += max(n, 0);
  }
  for (int i = tid; i < oi.suf_len; i += JE_NT) out->header[at + i] = im->header[oi.pre_len + i];
  if (tid == 0) out->header_len = at + oi.suf_len;
}

// ---- 3. bits of the image's earlier units -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(JE_NT) void jpegenc_scan_bits_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ unsigned long long s_tmp[JE_NT];
  const JeImageDev* im = je_image(table, blockIdx.x);
  JeUnitOut* uo = reinterpret_cast<JeUnitOut*>(scratch) + im->unit0;
  const unsigned long long bits = je_chunked_excl_sum(im->nunits, s_tmp, [&](int s) { return uo[s].bits; },
                                                      [&](int s, unsigned long long pre) { uo[s].pre = pre; });
  if (threadIdx.x == 0) je_image_out(table, scratch)[blockIdx.x].bits = bits;
}

// Where the unit's bytes lie in its interval's stream: bits [off, off + bits) of `ibits`; it owns bytes [j0, j1), the bytes
// whose first bit is its own (the last unit: up to the interval's padded end).  The interval's stream starts at `upos0` of the
// image's unstuffed buffer: floor(bits before it / 8) + its index leaves room for every earlier interval's padding.
struct JePlace {
  uint64_t off, end, ibits, upos0;
  uint32_t j0, j1;
  int unit_end;                        // index (in the image) behind the interval's last unit
};
__device__ __forceinline__ JePlace je_place(const JeUnit& u, const JeImageDev* im, const JeUnitOut* uo, const JeImageOut* io) {
  JePlace p;
  const int f = u.interval * im->upi;
  p.unit_end = min(f + im->upi, im->nunits);
  const uint64_t base = uo[f].pre;
  p.off = uo[u.index].pre - base;
  p.end = p.off + uo[u.index].bits;
  p.ibits = (p.unit_end < im->nunits ? uo[p.unit_end].pre : io[u.image].bits) - base;
  p.upos0 = base / 8u + (uint64_t)u.interval;
  p.j0 = (uint32_t)((p.off + 7u) / 8u);
  p.j1 = (uint32_t)(((u.last ? p.ibits : p.end) + 7u) / 8u);
  return p;
}

// ---- 4. the unstuffed stream: shifted gather, FF count ------------------------------------------------------------------------------
__global__ __launch_bounds__(JE_NT) void jpegenc_gather_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_ff;
  const int tid = threadIdx.x;
  const JeUnit u = je_unit(table, blockIdx.x);
  const JeImageDev* im = je_image(table, u.image);
  JeUnitOut* uo = reinterpret_cast<JeUnitOut*>(scratch) + im->unit0;
  const JePlace p = je_place(u, im, uo, je_image_out(table, scratch));
  if (tid == 0) s_ff = 0;
  __syncthreads();
  const JE_G uint8_t* slot = (const JE_G uint8_t*)scratch + u.slot_off;
  JE_G uint8_t* ust = (JE_G uint8_t*)scratch + im->ustream_off + p.upos0;
  // whole bytes of this unit's own bits: 8 j + 8 <= end
  const uint32_t full = (uint32_t)(p.end / 8u), nfull = full > p.j0 ? full - p.j0 : 0u;
  uint32_t ff = 0;
  for (uint32_t k = tid; k < nfull; k += JE_NT) {
    const uint32_t j = p.j0 + k, q = (uint32_t)(8ull * j - p.off);
    const uint32_t two = (uint32_t)slot[q >> 3] << 8 | slot[(q >> 3) + 1];
    const uint32_t byte = (two >> (8u - (q & 7u))) & 255u;
    ust[j] = (uint8_t)byte;
    ff += byte == 255u;
  }
  // the byte that straddles the unit's end (at most one): bit by bit out of this and the following units, 1-bits behind the interval
  if (tid == 0 && p.j1 > p.j0 + nfull) {
    const uint32_t j = p.j1 - 1u;
    int v = u.index;
    uint64_t voff = p.off, vend = p.end;
    uint32_t byte = 0;
    for (int t = 0; t < 8; ++t) {
      const uint64_t pos = 8ull * j + (uint64_t)t;
      while (pos >= vend && v + 1 < p.unit_end) {           // (a unit holds at least one block's four bits)
        ++v;
        voff = vend;
        vend = voff + uo[v].bits;
      }
      uint32_t bit = 1;
      if (pos < p.ibits) {
        const uint32_t q = (uint32_t)(pos - voff);
        const JE_G uint8_t* sv = (const JE_G uint8_t*)scratch + je_unit(table, im->unit0 + v).slot_off;
        bit = (sv[q >> 3] >> (7u - (q & 7u))) & 1u;
      }
      byte = byte << 1 | bit;
    }
    ust[j] = (uint8_t)byte;
    ff += byte == 255u;
  }
  for (int o = WAVE / 2; o > 0; o >>= 1) ff += __shfl_xor(ff, o, WAVE);
  if ((tid & (WAVE - 1)) == 0 && ff) atomicAdd(&s_ff, ff);
  __syncthreads();
  if (tid == 0) {
    JeUnitOut& o = uo[u.index];
    o.nbytes = p.j1 - p.j0;
    o.nff = s_ff;
    o.upos = (uint32_t)(p.upos0 + p.j0);
  }
}

// ---- 5. where every unit's stuffed bytes go; the file's length ----------------------------------------------------------------------
__global__ __launch_bounds__(JE_NT) void jpegenc_scan_bytes_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ unsigned long long s_tmp[JE_NT];
  const JeImageDev* im = je_image(table, blockIdx.x);
  JeUnitOut* uo = reinterpret_cast<JeUnitOut*>(scratch) + im->unit0;
  const unsigned long long bytes = je_chunked_excl_sum(
      im->nunits, s_tmp, [&](int s) { return (unsigned long long)uo[s].nbytes + uo[s].nff; },
      [&](int s, unsigned long long pre) { uo[s].fpos = pre + 2ull * (unsigned long long)(s / im->upi); });   // an RSTn behind every earlier interval
  if (threadIdx.x == 0) {
    const JoImageOut* opt = je_optimized(table, im, scratch);
    je_image_out(table, scratch)[blockIdx.x].file_bytes =
        (unsigned long long)(opt ? opt->header_len : im->header_len) + bytes + 2ull * (unsigned long long)(im->nint - 1) + 2ull;
  }
}

// ---- 6. where every file starts: offsets[B + 1] ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JE_NT) void jpegenc_scan_files_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ scratch,
                                                                   int64_t* __restrict__ offsets) {
  __shared__ unsigned long long s_tmp[JE_NT];
  const int B = je_header(table)->B;
  const JeImageOut* io = je_image_out(table, scratch);
  const unsigned long long all = je_chunked_excl_sum(B, s_tmp, [&](int b) { return io[b].file_bytes; },
                                                     [&](int b, unsigned long long pre) { offsets[b] = (int64_t)pre; });
  if (threadIdx.x == 0) offsets[B] = (int64_t)all;
}

// ---- 7. the files -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JE_NT) void jpegenc_write_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ scratch,
                                                              uint8_t* __restrict__ out, const int64_t* __restrict__ offsets) {
  __shared__ uint32_t s_tmp[JE_NT];
  const int tid = threadIdx.x;
  const JeUnit u = je_unit(table, blockIdx.x);
  const JeImageDev* im = je_image(table, u.image);
  const JeUnitOut o = reinterpret_cast<const JeUnitOut*>(scratch)[blockIdx.x];
  const int64_t off = offsets[u.image];                      // (jpegenc_scan_files_kernel)
  JE_G uint8_t* file = (JE_G uint8_t*)out + off;
  const JoImageOut* opt = je_optimized(table, im, scratch);          // its header: where jpegopt_tables_kernel left it
  const uint8_t* header = opt ? opt->header : im->header;
  const int header_len = opt ? opt->header_len : im->header_len;
  JE_G uint8_t* dst = file + header_len + o.fpos;
  const JE_G uint8_t* ust = (const JE_G uint8_t*)scratch + im->ustream_off + o.upos;
  je_stuff([&](uint32_t i) { return (uint32_t)ust[i]; }, o.nbytes, dst, s_tmp);
  if (u.index == 0)
    for (int i = tid; i < header_len; i += JE_NT) file[i] = header[i];
  if (tid == 0 && u.last) {
    JE_G uint8_t* m = dst + o.nbytes + o.nff;
    m[0] = 0xff;
    m[1] = u.index == im->nunits - 1 ? 0xd9 : (uint8_t)(0xd0 + (u.interval & 7));
  }
}

// ---- progressive images -------------------------------------------------------------------------------------------
__device__ __forceinline__ const PePlan* pe_plan(const uint8_t* table) {
  return reinterpret_cast<const PePlan*>(table + (uint64_t)je_header(table)->reserved * 16u);
}
__device__ __forceinline__ PeWalk pe_walk(const JeImageDev* im, const PeScan& sc, const PeScanPlan& sp, const uint8_t* scratch) {
  PeWalk w;
  w.coef = reinterpret_cast<const int16_t*>(scratch + im->coef_off);
  w.bpm = im->bpm;
  w.ny = im->C == 3 ? im->hmax * im->vmax : 1;
  w.hmax = im->hmax; w.vmax = im->vmax; w.mcus_x = im->mcus_x;
  w.comp = sc.comp;
  w.wc = sp.wc;
  return w;
}
constexpr int PE_LANES = 64;           // intervals per workgroup of the resolve kernel

// What a workgroup of the per-interval kernels works on: its segment, the walk of the segment's scan, the per-block arrays.
struct PeWork {
  PeSeg sg;
  PeScan sc;
  PeWalk w;
  uint64_t* pos;                       // bit position of every block in the interval's string
  uint32_t* pre;                       // the run in front of every block: EOBRUN | correction bits << 16
  uint8_t* summary;
};
__device__ __forceinline__ PeWork pe_work(const uint8_t* table, uint8_t* scratch, int sidx) {
  const PePlan* plan = pe_plan(table);
  PeWork k;
  k.sg = reinterpret_cast<const PeSeg*>(table + plan->off_segs)[sidx];
  const PeImage* pi = reinterpret_cast<const PeImage*>(table + plan->off_images) + k.sg.pimage;
  const JeImageDev* im = je_image(table, pi->image);
  k.sc = pe_scan(im->C, k.sg.scan);
  k.w = pe_walk(im, k.sc, pi->scan[k.sg.scan], scratch);
  k.pos = reinterpret_cast<uint64_t*>(scratch + k.sg.aux_off);
  k.pre = reinterpret_cast<uint32_t*>(k.pos + k.sg.nblocks);
  k.summary = reinterpret_cast<uint8_t*>(k.pre + k.sg.nblocks);
  return k;
}

__global__ __launch_bounds__(JE_NT) void jpegprogenc_clear_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  je_clear_words(reinterpret_cast<uint32_t*>(scratch + pe_plan(table)->off_hist) + (size_t)blockIdx.x * PE_SLOTS * 256, PE_SLOTS * 256);
}

// one workgroup per segment of an AC scan, one wave per block, one lane per coefficient: two ballots are the block's summary
__global__ __launch_bounds__(JE_NT) void jpegprogenc_summary_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  const PeWork k = pe_work(table, scratch, blockIdx.x);
  if (k.sc.ss == 0) return;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const bool band = lane >= k.sc.ss && lane <= k.sc.se;
  for (int i = wave; i < k.sg.nblocks; i += JE_NT / WAVE) {
    int ci;
    const int v = k.w.block((int64_t)k.sg.block0 + i, ci)[lane];
    const uint32_t t = (uint32_t)(v < 0 ? -v : v) >> k.sc.al;
    const unsigned long long nonzero = __ballot(band && t != 0u), newly = __ballot(band && k.sc.ah && t == 1u);
    if (lane == 0) k.summary[i] = (uint8_t)pe_summary_of(newly, nonzero, k.sc);
  }
}

// one lane per segment of an AC scan: the walk over the summaries, four blocks per load
__global__ __launch_bounds__(PE_LANES) void jpegprogenc_resolve_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  const int sidx = blockIdx.x * PE_LANES + threadIdx.x;
  if (sidx >= pe_plan(table)->nsegs) return;
  const PeWork k = pe_work(table, scratch, sidx);
  if (k.sc.ss == 0) return;
  PeRun r = {0u, 0u};
  for (int i = 0; i < k.sg.nblocks; ++i) {
    k.pre[i] = r.e | r.be << 16;
    pe_resolve_step(k.summary[i], r);
  }
}

struct PeCountSink {                   // the statistics pass: integer counts in LDS, so a file does not depend on the order of the lanes
  uint32_t* hist;                      // [2][256]: the scan's slot, the DC table of Cb / Cr
  __device__ void sym(int slot, int s) { atomicAdd(&hist[(slot == PE_DC1_SLOT ? 256 : 0) + (s & 255)], 1u); }
  __device__ void bits(uint32_t, int) {}
};
struct PeLengthSink {
  const uint32_t* code;                // [2][256] in LDS
  uint32_t n;
  __device__ void sym(int slot, int s) { n += code[(slot == PE_DC1_SLOT ? 256 : 0) + (s & 255)] >> 16; }
  __device__ void bits(uint32_t, int nb) { n += (uint32_t)nb; }
};
struct PeBitSink {                     // bits ORed into zeroed big-endian words; nothing at or behind word `nwords`
  const uint32_t* code;
  uint32_t* words;
  uint64_t pos, nwords;
  __device__ void bits(uint32_t v, int nb) {
    if (nb == 0) return;
    const uint64_t x = (uint64_t)v << (64u - (uint32_t)nb - (uint32_t)(pos & 31u));
    const uint64_t wi = pos >> 5;
    if (wi < nwords) atomicOr(&words[wi], (uint32_t)(x >> 32));
    if ((uint32_t)x && wi + 1 < nwords) atomicOr(&words[wi + 1], (uint32_t)x);
    pos += (uint32_t)nb;
  }
  __device__ void sym(int slot, int s) {
    const uint32_t c = code[(slot == PE_DC1_SLOT ? 256 : 0) + (s & 255)];
    bits(c & 0xffffu, (int)(c >> 16));
  }
};
__device__ __forceinline__ PeRun pe_run_in_front(const PeWork& k, int i) {
  PeRun r = {0u, 0u};
  if (k.sc.ss) { const uint32_t p = k.pre[i]; r.e = p & 0xffffu; r.be = p >> 16; }
  return r;
}

// one workgroup per segment, one lane per block: the block's symbols counted in LDS, the counts added to the image's histograms
__global__ __launch_bounds__(JE_NT) void jpegprogenc_count_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_hist[2 * 256];
  const int tid = threadIdx.x;
  const PeWork k = pe_work(table, scratch, blockIdx.x);
  for (int i = tid; i < 2 * 256; i += JE_NT) s_hist[i] = 0u;
  __syncthreads();
  PeState st;
  PeCountSink sink = {s_hist};
  for (int i = tid; i < k.sg.nblocks; i += JE_NT)
    pe_code_block(k.w, k.sc, k.sg.scan, k.sg.block0, k.sg.nblocks, (int64_t)k.sg.block0 + i, k.summary, pe_run_in_front(k, i), st, sink);
  __syncthreads();
  uint32_t* hist = reinterpret_cast<uint32_t*>(scratch + pe_plan(table)->off_hist) + (size_t)k.sg.pimage * PE_SLOTS * 256;
  for (int i = tid; i < 2 * 256; i += JE_NT)
    if (s_hist[i]) atomicAdd(&hist[(i < 256 ? k.sg.scan : PE_DC1_SLOT) * 256 + (i & 255)], s_hist[i]);
}

// One workgroup per segment, one lane per block, three passes: every block's bit length and from the prefix sums its place;
// the words of the interval's string to zero; every block's bits ORed to their place, 1-bits up to the byte's end.  Then the FF
// bytes are counted for the stuffing, which the write kernel does.
__global__ __launch_bounds__(JE_NT) void jpegprogenc_code_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_code[2 * 256];
  __shared__ unsigned long long s_tmp[JE_NT];
  __shared__ uint32_t s_ff;
  const int tid = threadIdx.x;
  const PeWork k = pe_work(table, scratch, blockIdx.x);
  const JoTable* tables = reinterpret_cast<const JoTable*>(scratch + pe_plan(table)->off_tables) + (size_t)k.sg.pimage * PE_SLOTS;
  for (int i = tid; i < 2 * 256; i += JE_NT) s_code[i] = tables[i < 256 ? k.sg.scan : PE_DC1_SLOT].code[i & 255];
  if (tid == 0) s_ff = 0;
  __syncthreads();
  PeState st;
  const unsigned long long carry = je_chunked_excl_sum(
      k.sg.nblocks, s_tmp,
      [&](int i) {
        PeLengthSink ls = {s_code, 0u};
        pe_code_block(k.w, k.sc, k.sg.scan, k.sg.block0, k.sg.nblocks, (int64_t)k.sg.block0 + i, k.summary, pe_run_in_front(k, i), st, ls);
        return ls.n;
      },
      [&](int i, unsigned long long at) { k.pos[i] = at; });
  // the clamp guards the slot; the planner's bound (pe_interval_bytes) keeps the string within it
  const uint64_t nwords = ((uint64_t)k.sg.cap + 7u) / 4u;
  const uint64_t bits = carry < 8ull * (uint64_t)k.sg.cap ? carry : 8ull * (uint64_t)k.sg.cap;
  const uint32_t nbytes = (uint32_t)((bits + 7u) / 8u);
  uint32_t* words = reinterpret_cast<uint32_t*>(scratch + k.sg.slot_off);
  for (uint64_t i = tid; i < ((uint64_t)nbytes + 3u) / 4u + 1u && i < nwords; i += JE_NT) words[i] = 0u;
  __syncthreads();
  for (int i = tid; i < k.sg.nblocks; i += JE_NT) {
    PeBitSink bs = {s_code, words, k.pos[i], nwords};
    pe_code_block(k.w, k.sc, k.sg.scan, k.sg.block0, k.sg.nblocks, (int64_t)k.sg.block0 + i, k.summary, pe_run_in_front(k, i), st, bs);
  }
  if (tid == 0 && (bits & 7u)) {
    PeBitSink bs = {s_code, words, bits, nwords};
    bs.bits((1u << (8u - (uint32_t)(bits & 7u))) - 1u, (int)(8u - (uint32_t)(bits & 7u)));
  }
  __syncthreads();
  uint32_t ff = 0;
  for (uint32_t i = tid; i < nbytes; i += JE_NT) ff += ((words[i >> 2] >> (24u - 8u * (i & 3u))) & 255u) == 255u;
  for (int o = WAVE / 2; o > 0; o >>= 1) ff += __shfl_xor(ff, o, WAVE);
  if ((tid & (WAVE - 1)) == 0 && ff) atomicAdd(&s_ff, ff);
  __syncthreads();
  if (tid == 0) {
    PeSegOut& o = reinterpret_cast<PeSegOut*>(scratch + pe_plan(table)->off_seg_out)[blockIdx.x];
    o.nbytes = nbytes;
    o.nff = s_ff;
  }
}

__global__ __launch_bounds__(JE_NT) void jpegprogenc_tables_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ JoWork s_work[JE_NT / WAVE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const PePlan* plan = pe_plan(table);
  const PeImage* pi = reinterpret_cast<const PeImage*>(table + plan->off_images) + blockIdx.x;
  const int ncomp = je_image(table, pi->image)->C;
  const uint32_t* hist = reinterpret_cast<const uint32_t*>(scratch + plan->off_hist) + (size_t)blockIdx.x * PE_SLOTS * 256;
  JoTable* out = reinterpret_cast<JoTable*>(scratch + plan->off_tables) + (size_t)blockIdx.x * PE_SLOTS;
  for (int slot = wave; slot < PE_SLOTS; slot += JE_NT / WAVE)
    if (pe_slot_used(ncomp, slot)) jo_optimal_table<WAVE>(hist + 256 * slot, pe_slot_class(ncomp, slot), lane, JoWaveMin(), s_work[wave], out[slot]);
}

// What precedes a segment's bytes in the file: nothing, or (the first of a scan) the file's header in front of the first scan,
// the scan's DHTs, a DRI where the interval changes, the SOS.  What follows them: RSTn, nothing (a scan's end) or EOI.
struct PePieces {
  int header, dht[2], ndht, dri, sos, tail;
  __device__ int before() const { return header + dht[0] + dht[1] + (dri ? 6 : 0) + sos; }
};
__device__ __forceinline__ PePieces pe_pieces(const PeImage* pi, int ncomp, const PeSeg& sg, const JoTable* tables) {
  PePieces p = {0, {0, 0}, 0, 0, 0, 2};
  const PeScanPlan& sp = pi->scan[sg.scan];
  if (sg.index == sp.nsegs - 1 && sg.scan != pi->nscans - 1) p.tail = 0;
  if (sg.index != 0) return p;
  const PeScan sc = pe_scan(ncomp, sg.scan);
  p.header = sg.scan == 0 ? pi->header_len : 0;
  if (pe_slot_used(ncomp, sg.scan)) {
    p.dht[p.ndht++] = min(tables[sg.scan].dht_len, PE_DHT_MAX);
    if (sc.comp < 0) p.dht[p.ndht++] = min(tables[PE_DC1_SLOT].dht_len, PE_DHT_MAX);
  }
  p.dri = sp.dri;
  p.sos = 6 + 2 * (sc.comp < 0 ? ncomp : 1) + 2;
  return p;
}

__global__ __launch_bounds__(JE_NT) void jpegprogenc_place_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ unsigned long long s_tmp[JE_NT];
  const PePlan* plan = pe_plan(table);
  const PeImage* pi = reinterpret_cast<const PeImage*>(table + plan->off_images) + blockIdx.x;
  const int ncomp = je_image(table, pi->image)->C;
  const PeSeg* segs = reinterpret_cast<const PeSeg*>(table + plan->off_segs) + pi->seg0;
  PeSegOut* so = reinterpret_cast<PeSegOut*>(scratch + plan->off_seg_out) + pi->seg0;
  const JoTable* tables = reinterpret_cast<const JoTable*>(scratch + plan->off_tables) + (size_t)blockIdx.x * PE_SLOTS;
  const unsigned long long bytes = je_chunked_excl_sum(
      pi->nsegs, s_tmp,
      [&](int s) {
        const PePieces p = pe_pieces(pi, ncomp, segs[s], tables);
        return (unsigned long long)p.before() + so[s].nbytes + so[s].nff + (unsigned long long)p.tail;
      },
      [&](int s, unsigned long long pre) { so[s].fpos = pre; });
  if (threadIdx.x == 0) je_image_out(table, scratch)[pi->image].file_bytes = bytes;
}

__global__ __launch_bounds__(JE_NT) void jpegprogenc_write_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ scratch,
                                                               uint8_t* __restrict__ out, const int64_t* __restrict__ offsets) {
  __shared__ uint32_t s_tmp[JE_NT];
  const int tid = threadIdx.x;
  const PePlan* plan = pe_plan(table);
  const PeSeg sg = reinterpret_cast<const PeSeg*>(table + plan->off_segs)[blockIdx.x];
  const PeImage* pi = reinterpret_cast<const PeImage*>(table + plan->off_images) + sg.pimage;
  const JeImageDev* im = je_image(table, pi->image);
  const PeSegOut o = reinterpret_cast<const PeSegOut*>(scratch + plan->off_seg_out)[blockIdx.x];
  const JoTable* tables = reinterpret_cast<const JoTable*>(scratch + plan->off_tables) + (size_t)sg.pimage * PE_SLOTS;
  const PePieces p = pe_pieces(pi, im->C, sg, tables);
  JE_G uint8_t* dst = (JE_G uint8_t*)out + offsets[pi->image] + o.fpos;
  if (sg.index == 0) {
    for (int i = tid; i < p.header; i += JE_NT) dst[i] = im->header[i];
    dst += p.header;
    for (int t = 0; t < p.ndht; ++t) {
      const uint8_t* dht = tables[t ? PE_DC1_SLOT : sg.scan].dht;
      for (int i = tid; i < p.dht[t]; i += JE_NT) dst[i] = dht[i];
      dst += p.dht[t];
    }
    if (tid == 0) {
      const PeScan sc = pe_scan(im->C, sg.scan);
      int n = 0;
      if (p.dri) {
        const uint8_t dri[6] = {0xff, 0xdd, 0x00, 0x04, (uint8_t)(p.dri >> 8), (uint8_t)(p.dri & 255)};
        for (int i = 0; i < 6; ++i) dst[n++] = dri[i];
      }
      const int nc = sc.comp < 0 ? im->C : 1;
      dst[n++] = 0xff; dst[n++] = 0xda; dst[n++] = 0x00; dst[n++] = (uint8_t)(6 + 2 * nc); dst[n++] = (uint8_t)nc;
      for (int c = 0; c < nc; ++c) {
        const int ci = sc.comp < 0 ? c : sc.comp;
        const int id = ci ? 1 : 0;                          // the table a component names: DC in a DC first pass, AC in an AC scan
        dst[n++] = (uint8_t)(ci + 1);
        dst[n++] = (uint8_t)(sc.ss ? id : (sc.ah ? 0 : id << 4));
      }
      dst[n++] = (uint8_t)sc.ss; dst[n++] = (uint8_t)sc.se; dst[n++] = (uint8_t)(sc.ah << 4 | sc.al);
    }
    dst += (p.dri ? 6 : 0) + p.sos;
  }
  // the interval's bytes out of its big-endian words, a zero behind every FF (the stuffing of launch 7)
  const uint32_t* words = reinterpret_cast<const uint32_t*>(scratch + sg.slot_off);
  je_stuff([&](uint32_t i) { return (words[i >> 2] >> (24u - 8u * (i & 3u))) & 255u; }, o.nbytes, dst, s_tmp);
  if (tid == 0 && p.tail) {
    dst[o.nbytes + o.nff] = 0xff;
    dst[o.nbytes + o.nff + 1] = sg.index == pi->scan[sg.scan].nsegs - 1 ? 0xd9 : (uint8_t)(0xd0 + (sg.index & 7));
  }
}

// ---- host: limits, header, bound, plan -----------------------------------------------------------------------------------------------------
static uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

struct JeGeometry {
  int hmax, vmax, bpm, mcus_x, interval, nint, upi, nunits;
  int64_t nmcu;
};
// false: outside the limits (what: the reason)
static bool je_geometry(int H, int W, int C, int quality, int subsampling, int restart_rows, JeGeometry& g, const char*& what) {
  what = nullptr;
  if (H < 1 || W < 1) what = "non-positive size";
  else if (C != 1 && C != 3) what = "channels (1 or 3)";
  else if (quality < 1 || quality > 100) what = "quality (1 .. 100)";
  else if (C == 3 && (subsampling < ATTWARP_JPEGENC_444 || subsampling > ATTWARP_JPEGENC_420)) what = "unknown subsampling";
  else if (restart_rows < 0) what = "negative restart_rows";
  if (what) return false;
  if (H > JE_MAX_DIM || W > JE_MAX_DIM) { what = "size above 65500"; return false; }
  g.hmax = (C == 3 && subsampling != ATTWARP_JPEGENC_444) ? 2 : 1;
  g.vmax = (C == 3 && subsampling == ATTWARP_JPEGENC_420) ? 2 : 1;
  g.bpm = C == 3 ? g.hmax * g.vmax + 2 : 1;
  g.mcus_x = (W + 8 * g.hmax - 1) / (8 * g.hmax);
  g.nmcu = (int64_t)g.mcus_x * ((H + 8 * g.vmax - 1) / (8 * g.vmax));
  const int64_t interval = restart_rows ? (int64_t)restart_rows * g.mcus_x : g.nmcu;
  if (restart_rows && interval > 65535) { what = "restart interval above 65535"; return false; }
  g.interval = (int)interval;
  g.nint = (int)((g.nmcu + interval - 1) / interval);
  g.upi = (int)((interval + JE_UNIT_MCUS - 1) / JE_UNIT_MCUS);
  const int64_t last = g.nmcu - (int64_t)(g.nint - 1) * interval;
  g.nunits = (int)((int64_t)(g.nint - 1) * g.upi + (last + JE_UNIT_MCUS - 1) / JE_UNIT_MCUS);
  return true;
}
static int je_header_len(int C, int restart_rows) { return 2 + 18 + (C == 3 ? 2 : 1) * 69 + (10 + 3 * C) + (C == 3 ? 432 : 216) + (restart_rows ? 6 : 0) + (8 + 2 * C); }
// optimize: the header is never longer than the standard one (at most 12 and 162 symbols per DHT); a DC code may take 12 bits
static uint64_t je_bound64(int C, int quality, int restart_rows, const JeGeometry& g, bool optimize = false) {
  const uint64_t bits = (uint64_t)g.nmcu * g.bpm * (uint64_t)(je_block_bound_bits(quality, C) + (optimize ? JO_EXTRA_BLOCK_BITS : 0));
  return (uint64_t)je_header_len(C, restart_rows) + 2u * ((bits + 7u) / 8u + (uint64_t)g.nint) + 2u * (uint64_t)g.nint + 2u;
}

// The scans of a progressive image: blocks, blocks per restart interval, intervals, blocks per row of a one-component walk.
struct PeScanGeometry {
  int64_t nblk, step;
  int nseg, block_bits, ndht, ncomp, wc, interval;          // interval: the DRI value, in MCUs of the scan (0: none)
};
struct PeGeometry {
  int nscans;
  int64_t nsegs;
  PeScanGeometry scan[PE_MAX_SCANS];
};
// false: a scan's restart interval is above 65535 MCUs (libjpeg would clamp it there, silently, and cut the rows elsewhere)
static bool pe_geometry(int H, int W, int C, int restart_rows, const JeGeometry& g, PeGeometry& p) {
  p.nscans = pe_nscans(C);
  p.nsegs = 0;
  for (int i = 0; i < p.nscans; ++i) {
    const PeScan sc = pe_scan(C, i);
    PeScanGeometry& q = p.scan[i];
    int64_t per_row, per_mcu = 1;
    if (sc.comp < 0) {
      per_row = g.mcus_x;
      per_mcu = g.bpm;
      q.nblk = g.nmcu * g.bpm;
      q.wc = 0;
    } else {
      const int fh = sc.comp > 0 ? g.hmax : 1, fv = sc.comp > 0 ? g.vmax : 1;
      q.wc = ((W + fh - 1) / fh + 7) / 8;
      per_row = q.wc;
      q.nblk = (int64_t)q.wc * (((H + fv - 1) / fv + 7) / 8);
    }
    const int64_t interval = (int64_t)restart_rows * per_row;
    if (interval > 65535) return false;
    q.interval = (int)interval;
    q.step = restart_rows ? interval * per_mcu : q.nblk;
    q.nseg = (int)((q.nblk + q.step - 1) / q.step);
    q.block_bits = pe_block_bits(sc);
    q.ndht = (sc.ss == 0 && sc.ah) ? 0 : (sc.comp < 0 ? 2 : 1);
    q.ncomp = sc.comp < 0 ? C : 1;
    p.nsegs += q.nseg;
  }
  return true;
}
static int pe_frame_header_len(int C) { return 2 + 18 + (C == 3 ? 2 : 1) * 69 + (10 + 3 * C); }
// SOI .. SOF2; per scan its DHTs at their longest, a DRI, the SOS, every interval at its bound and a marker behind it; EOI
static uint64_t pe_bound64(int C, const PeGeometry& p) {
  uint64_t n = (uint64_t)pe_frame_header_len(C) + 2u;
  for (int i = 0; i < p.nscans; ++i) {
    const PeScanGeometry& q = p.scan[i];
    n += (uint64_t)PE_DHT_MAX * q.ndht + 6u + 6u + 2u * q.ncomp;
    const uint64_t full = (uint64_t)(q.nblk / q.step), rest = (uint64_t)(q.nblk % q.step);
    n += full * (pe_interval_bytes((uint64_t)q.step, q.block_bits) + 2u);
    if (rest) n += pe_interval_bytes(rest, q.block_bits) + 2u;
  }
  return n;
}

// pre_len: the file's DHTs are left out (the device splices the image's own in) and *pre_len receives where they belong
static int je_write_header(uint8_t* h, const attwarp_jpegenc_image& d, const JeGeometry& g, int* pre_len = nullptr) {
  int n = 0;
  auto put = [&](std::initializer_list<int> b) { for (int v : b) h[n++] = (uint8_t)v; };
  put({0xff, 0xd8, 0xff, 0xe0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00});
  const int nc = d.C;
  for (int t = 0; t < (nc == 3 ? 2 : 1); ++t) {
    put({0xff, 0xdb, 0x00, 0x43, t});
    for (int k = 0; k < 64; ++k) h[n++] = (uint8_t)je_quant_value(d.quality, t, je_zigzag(k));
  }
  put({0xff, 0xc0, 0x00, 8 + 3 * nc, 0x08, d.H >> 8, d.H & 255, d.W >> 8, d.W & 255, nc});
  for (int c = 0; c < nc; ++c) put({c + 1, c == 0 ? (g.hmax << 4 | g.vmax) : 0x11, c ? 1 : 0});
  if (pre_len) *pre_len = n;
  for (int t = 0; t < (nc == 3 ? 4 : 2) && !pre_len; ++t) {
    const int nv = je_nvals(t);
    put({0xff, 0xc4, (19 + nv) >> 8, (19 + nv) & 255, (t & 1) << 4 | t >> 1});
    for (int k = 0; k < 16; ++k) h[n++] = JE_BITS[t][k];
    for (int k = 0; k < nv; ++k) h[n++] = je_vals(t)[k];
  }
  if (d.restart_rows) put({0xff, 0xdd, 0x00, 0x04, g.interval >> 8, g.interval & 255});
  put({0xff, 0xda, 0x00, 6 + 2 * nc, nc});
  for (int c = 0; c < nc; ++c) put({c + 1, c ? 0x11 : 0x00});
  put({0x00, 0x3f, 0x00});
  return n;
}

// Everything the callers need of one image, derived once: its geometry, the scans' when it is progressive, and its file's
// bound.  optimize is ignored for a progressive image (such a file always has tables of its own).
struct JeImagePlan {
  bool prog, opt;
  JeGeometry g;
  PeGeometry p;                        // (prog)
  uint64_t bound;                      // the file's length at most, below 2 GiB
  bool geometry;                       // false: the refusal is je_geometry's (the later checks were not reached)
  char why[256];                       // the reason of a refusal: what follows "jpegenc: image <b>" in the error
};
// false: refused, and pl.why says why
static bool je_image_plan(const attwarp_jpegenc_image& d, bool optimize, bool progressive, JeImagePlan& pl) {
  pl.prog = progressive;
  pl.opt = optimize && !progressive;
  pl.bound = 0;
  const char* what;
  pl.geometry = je_geometry(d.H, d.W, d.C, d.quality, d.subsampling, d.restart_rows, pl.g, what);
  if (!pl.geometry) {
    std::snprintf(pl.why, sizeof pl.why, " (%d x %d x %d, quality %d, subsampling %d, restart_rows %d): %s", d.H, d.W, d.C, d.quality, d.subsampling,
                  d.restart_rows, what);
    return false;
  }
  if (pl.prog && !pe_geometry(d.H, d.W, d.C, d.restart_rows, pl.g, pl.p)) {
    std::snprintf(pl.why, sizeof pl.why, " (%d x %d x %d, restart_rows %d): a progressive scan's restart interval above 65535 "
                  "(libjpeg clamps it to 65535 and no longer restarts at the rows)", d.H, d.W, d.C, d.restart_rows);
    return false;
  }
  const uint64_t bound = pl.prog ? pe_bound64(d.C, pl.p) : je_bound64(d.C, d.quality, d.restart_rows, pl.g, pl.opt);
  if (bound >= ((uint64_t)1 << 31)) {
    std::snprintf(pl.why, sizeof pl.why, ": the %sbound of %d x %d x %d is 2 GiB or more", pl.prog ? "progressive " : "", d.H, d.W, d.C);
    return false;
  }
  pl.bound = bound;
  return true;
}
static size_t je_bound_of(int H, int W, int C, int quality, int subsampling, int restart_rows, bool optimize, bool progressive) {
  attwarp_jpegenc_image d;
  std::memset(&d, 0, sizeof d);
  d.H = H; d.W = W; d.C = C; d.quality = quality; d.subsampling = subsampling; d.restart_rows = restart_rows;
  JeImagePlan pl;
  return je_image_plan(d, optimize, progressive, pl) ? (size_t)pl.bound : 0;
}

// What a call holds.  A progressive image owns no entropy unit: its transform units and its segments are counted apart.
struct JeCounts {
  int64_t nunits = 0;                  // units of the plain and the optimised images
  int nopt = 0;                        // optimised images
  int64_t nopt_units = 0;              // and their units
  int nprog = 0;                       // progressive images
  int64_t nprog_units = 0, nsegs = 0;  // their transform units; their segments (scans x restart intervals)
};
// optimize, progressive: NULL, or one flag per image
static int jpegenc_count(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, const int32_t* progressive, JeCounts& n) {
  ATTWARP_REQUIRE(images, "jpegenc: null image array");
  ATTWARP_REQUIRE(B > 0, "jpegenc: non-positive batch size");
  if (B > (1 << 20)) return fail(ATTWARP_E_UNSUPPORTED, "jpegenc: B=%d > 2^20", B);
  n = JeCounts();
  for (int b = 0; b < B; ++b) {
    const attwarp_jpegenc_image& d = images[b];
    ATTWARP_REQUIRE(!progressive || progressive[b] == 0 || progressive[b] == 1, "jpegenc: image %d: progressive must be 0 or 1", b);
    ATTWARP_REQUIRE(!optimize || optimize[b] == 0 || optimize[b] == 1, "jpegenc: image %d: optimize must be 0 or 1", b);
    ATTWARP_REQUIRE(d.src, "jpegenc: image %d: null pointer", b);
    ATTWARP_REQUIRE(d.order == ATTWARP_RGB || d.order == ATTWARP_BGR, "jpegenc: image %d: channel order must be ATTWARP_RGB or ATTWARP_BGR", b);
    JeImagePlan pl;
    const bool ok = je_image_plan(d, optimize && optimize[b], progressive && progressive[b], pl);
    if (!pl.geometry) return fail(ATTWARP_E_UNSUPPORTED, "jpegenc: image %d%s", b, pl.why);
    ATTWARP_REQUIRE((int64_t)d.pitch >= (int64_t)d.W * d.C, "jpegenc: image %d: pitch %d below the row's %lld bytes", b, d.pitch, (long long)d.W * d.C);
    if (!ok) return fail(ATTWARP_E_UNSUPPORTED, "jpegenc: image %d%s", b, pl.why);
    // A table's frequencies add up to at most 64 symbols per block.  A block's bound is above 1024 bits (22 + 63 x 17) and the
    // file's bound, twice its bytes, is below 2^31: fewer than 2^23 blocks and 2^29 symbols, below libjpeg's sentinel (a larger
    // frequency would never be merged) and far below the 2^32 of the counters (a progressive image's too).  This refusal can never trigger.
    if (pl.opt && (uint64_t)pl.g.nmcu * pl.g.bpm * JO_SYMBOLS_PER_BLOCK >= JO_SENTINEL)
      return fail(ATTWARP_E_UNSUPPORTED, "jpegenc: image %d: %lld blocks could hold 10^9 symbols or more", b, (long long)pl.g.nmcu * pl.g.bpm);
    if (pl.prog) { n.nprog += 1; n.nprog_units += pl.g.nunits; n.nsegs += pl.p.nsegs; }
    else n.nunits += pl.g.nunits;
    if (pl.opt) { n.nopt += 1; n.nopt_units += pl.g.nunits; }
  }
  if (n.nunits + n.nprog_units > JE_MAX_UNITS)
    return fail(ATTWARP_E_UNSUPPORTED, "jpegenc: %lld units in one call (> %d)", (long long)(n.nunits + n.nprog_units), JE_MAX_UNITS);
  if (n.nsegs > JE_MAX_UNITS)
    return fail(ATTWARP_E_UNSUPPORTED, "jpegenc: %lld progressive segments (scans x restart intervals) in one call (> %d)", (long long)n.nsegs, JE_MAX_UNITS);
  return ATTWARP_OK;
}

// Where the parts of a table lie.  Without an optimised image the table ends behind the units, as it always did; with one, the
// JoPlan follows them; the PePlan, its images and segments follow that, 16-byte aligned.
struct JeLayout {
  uint64_t off_huffman, off_images, off_units, off_optimize, off_progressive, bytes;       // (off_optimize, off_progressive 0: none)
};
static JeLayout jpegenc_table_layout(int B, const JeCounts& n) {
  static_assert(sizeof(attwarp_jpegenc_header) == 80, "the header ends where the Annex K code words start");
  JeLayout at;
  at.off_huffman = align_up(sizeof(attwarp_jpegenc_header), 16);
  at.off_images = at.off_huffman + 4 * 256 * sizeof(uint32_t);
  at.off_units = at.off_images + align_up((uint64_t)B * sizeof(JeImageDev), 16);
  uint64_t end = at.off_units + (uint64_t)(n.nunits + n.nprog_units) * sizeof(JeUnit);     // the progressive images' transform units last
  at.off_optimize = n.nopt ? end : 0;
  if (n.nopt) end += sizeof(JoPlan) + (uint64_t)n.nopt * sizeof(JoImage) + (uint64_t)n.nopt_units * sizeof(int32_t);
  at.off_progressive = n.nprog ? align_up(end, 16) : 0;
  if (n.nprog) end = at.off_progressive + align_up(sizeof(PePlan), 16) + (uint64_t)n.nprog * sizeof(PeImage) + (uint64_t)n.nsegs * sizeof(PeSeg);
  at.bytes = end;
  return at;
}

struct JeCursor {                      // the next free byte of the scratch buffer
  uint64_t at = 0;
  uint64_t take(uint64_t bytes, uint64_t align = 1) {        // where `bytes` go; the cursor moves on by them, rounded up to `align`
    const uint64_t off = at;
    at += align_up(bytes, align);
    return off;
  }
  void align(uint64_t a) { at = align_up(at, a); }
};

// The planner's state: the records it fills in the table and how far it got in each of them.
struct JePlanner {
  const JeCounts n;
  const JeLayout at;
  JeCursor scratch;
  JeUnit* units;
  int32_t unit = 0, tunit;             // the next entropy unit; the next transform unit of a progressive image (behind every other unit)
  JoPlan* jo;                          // nullptr: no optimised image; then its JoImage[nopt], int32 unit[nopt_units]
  JoImage* jo_image;
  int32_t* jo_unit;
  PePlan* pe;                          // nullptr: no progressive image; then (16-byte aligned) PeImage[nprog], PeSeg[nsegs]
  PeImage* pe_image;
  PeSeg* pe_seg;
  int k_opt = 0, k_prog = 0;           // the next optimised image and its next unit, the next progressive image and its next segment
  int64_t k_opt_unit = 0;
  int32_t k_seg = 0;

  JePlanner(uint8_t* t, const JeCounts& n, const JeLayout& at)
      : n(n), at(at), units(reinterpret_cast<JeUnit*>(t + at.off_units)), tunit((int32_t)n.nunits),
        jo(n.nopt ? reinterpret_cast<JoPlan*>(t + at.off_optimize) : nullptr), jo_image(jo ? reinterpret_cast<JoImage*>(jo + 1) : nullptr),
        jo_unit(jo ? reinterpret_cast<int32_t*>(jo_image + n.nopt) : nullptr),
        pe(n.nprog ? reinterpret_cast<PePlan*>(t + at.off_progressive) : nullptr),
        pe_image(pe ? reinterpret_cast<PeImage*>(t + at.off_progressive + align_up(sizeof(PePlan), 16)) : nullptr),
        pe_seg(pe ? reinterpret_cast<PeSeg*>(pe_image + n.nprog) : nullptr) {}
};

// The part of its record every image shares: source, swap, factors, quantisation divisors and reciprocals, header.
// own_tables: the header's DHTs are left out; returns where they belong (else 0).
static int je_fill_image(JeImageDev& r, const attwarp_jpegenc_image& d, const JeGeometry& g, bool own_tables) {
  r.src = d.src; r.H = d.H; r.W = d.W; r.C = d.C; r.pitch = d.pitch;
  r.swap = d.C == 3 && d.order == ATTWARP_BGR;
  r.hmax = g.hmax; r.vmax = g.vmax; r.bpm = g.bpm;
  r.mcus_x = g.mcus_x; r.nmcu = (int32_t)g.nmcu;
  for (int tb = 0; tb < 2; ++tb)
    for (int k = 0; k < 64; ++k) {
      r.divisor[tb][k] = (uint16_t)(je_quant_value(d.quality, tb, k) << 3);
      r.recip[tb][k] = je_recip(r.divisor[tb][k]);
    }
  int pre = 0;
  r.header_len = je_write_header(r.header, d, g, own_tables ? &pre : nullptr);
  return pre;
}

// A plain or optimised image: its intervals, cut into units; pre: je_fill_image's answer.
static void je_plan_units(JePlanner& P, int b, JeImageDev& r, const JeImagePlan& pl, int quality, int pre) {
  const JeGeometry& g = pl.g;
  r.interval = g.interval; r.nint = g.nint; r.upi = g.upi;
  r.nunits = g.nunits;
  r.block_bits = je_block_bound_bits(quality, r.C) + (pl.opt ? JO_EXTRA_BLOCK_BITS : 0);
  if (pl.opt) {
    JoImage& o = P.jo_image[P.k_opt];
    o.image = b;
    o.pre_len = pre;
    o.suf_len = r.header_len - pre;
    o.ntables = r.C == 3 ? 4 : 2;
    r.opt = ++P.k_opt;
  }
  const uint64_t nblocks = (uint64_t)g.nmcu * g.bpm;
  r.coef_off = P.scratch.take(nblocks * 128, 256);
  r.ustream_off = P.scratch.take((nblocks * r.block_bits + 7) / 8 + (uint64_t)g.nint + 8, 256);
  for (int i = 0; i < g.nint; ++i) {
    const int m0 = i * g.interval, m1 = (int)std::min<int64_t>(g.nmcu, (int64_t)m0 + g.interval);
    for (int m = m0; m < m1; m += JE_UNIT_MCUS, ++P.unit) {
      JeUnit& q = P.units[P.unit];
      q.image = b;
      q.mcu0 = m;
      q.nmcu = std::min(JE_UNIT_MCUS, m1 - m);
      q.interval = i;
      q.last = m + JE_UNIT_MCUS >= m1;
      q.index = P.unit - r.unit0;
      q.slot_off = P.scratch.take(((uint64_t)q.nmcu * g.bpm * r.block_bits + 7) / 8 + 8, 16);
      if (pl.opt) P.jo_unit[P.k_opt_unit++] = P.unit;
    }
  }
}

// A progressive image.  Its record serves the transform kernel and the jpegprogenc_* kernels; with no unit of its own the scans
// of launches 3 and 5 pass over it, and jpegprogenc_place_kernel sets its file's length behind them.  pre: SOI .. SOF0.
static void je_plan_progressive(JePlanner& P, int b, JeImageDev& r, const JeImagePlan& pl, int pre) {
  const JeGeometry& g = pl.g;
  r.interval = (int32_t)g.nmcu; r.nint = 1; r.upi = 1;
  r.nunits = 0;
  r.header[pre - (10 + 3 * r.C) + 1] = 0xc2;                  // the frame becomes SOF2
  r.header_len = pre;
  r.coef_off = P.scratch.take((uint64_t)g.nmcu * g.bpm * 128, 256);
  for (int64_t m = 0; m < g.nmcu; m += JE_UNIT_MCUS) {
    JeUnit& q = P.units[P.tunit++];
    q.image = b;
    q.mcu0 = (int32_t)m;
    q.nmcu = (int32_t)std::min<int64_t>(JE_UNIT_MCUS, g.nmcu - m);
  }
  PeImage& pi = P.pe_image[P.k_prog];
  pi.image = b;
  pi.nscans = pl.p.nscans;
  pi.seg0 = P.k_seg;
  pi.nsegs = (int32_t)pl.p.nsegs;
  pi.header_len = pre;
  int last_dri = 0;
  for (int i = 0; i < pl.p.nscans; ++i) {
    const PeScanGeometry& q = pl.p.scan[i];
    PeScanPlan& sp = pi.scan[i];
    sp.seg0 = P.k_seg - pi.seg0;
    sp.nsegs = q.nseg;
    sp.wc = q.wc;
    sp.dri = q.interval != last_dri ? q.interval : 0;        // libjpeg writes a DRI when the interval differs from the last one written
    last_dri = q.interval;
    for (int k = 0; k < q.nseg; ++k, ++P.k_seg) {
      PeSeg& sg = P.pe_seg[P.k_seg];
      sg.pimage = P.k_prog;
      sg.scan = i;
      sg.block0 = (int32_t)(k * q.step);
      sg.nblocks = (int32_t)std::min<int64_t>(q.step, q.nblk - k * q.step);
      sg.index = k;
      sg.cap = (int32_t)(pe_interval_bytes((uint64_t)sg.nblocks, q.block_bits) / 2u);   // (the file's bound counts every byte twice)
      sg.slot_off = P.scratch.take((uint64_t)sg.cap + 8, 16);
      sg.aux_off = P.scratch.take(pe_aux_bytes((uint64_t)sg.nblocks));
    }
  }
  ++P.k_prog;
}

// Behind the last image: what the kernels of the optimised and of the progressive images keep in the scratch buffer.
static void je_close_plans(JePlanner& P) {
  if (P.jo) {
    P.jo->nimages = P.n.nopt;
    P.jo->nunits = (int32_t)P.n.nopt_units;
    P.scratch.align(256);
    P.jo->off_hist = P.scratch.take((uint64_t)P.n.nopt * 4 * 256 * sizeof(uint32_t));
    P.jo->off_out = P.scratch.take((uint64_t)P.n.nopt * sizeof(JoImageOut));
  }
  if (P.pe) {
    P.pe->nimages = P.n.nprog;
    P.pe->nsegs = (int32_t)P.n.nsegs;
    P.pe->ntunits = (int32_t)P.n.nprog_units;
    P.pe->off_images = P.at.off_progressive + align_up(sizeof(PePlan), 16);
    P.pe->off_segs = P.pe->off_images + (uint64_t)P.n.nprog * sizeof(PeImage);
    P.scratch.align(256);
    P.pe->off_hist = P.scratch.take((uint64_t)P.n.nprog * PE_SLOTS * 256 * sizeof(uint32_t));
    P.pe->off_tables = P.scratch.take((uint64_t)P.n.nprog * PE_SLOTS * sizeof(JoTable));
    P.pe->off_seg_out = P.scratch.take((uint64_t)P.n.nsegs * sizeof(PeSegOut));
  }
}

// The header of a planned table and its two optional records, read once and checked (jo.nimages, pe.nimages 0: no such record).
struct JeTableHead {
  attwarp_jpegenc_header h;
  JoPlan jo;
  PePlan pe;
};
static int je_read_table(const void* table_host, const void* table_dev, const void* scratch, const uint8_t* out, size_t out_bytes,
                         const int64_t* offsets, JeTableHead& T) {
  ATTWARP_REQUIRE(table_host && table_dev && scratch && out && offsets, "jpegenc_encode: null pointer");
  std::memset(&T, 0, sizeof T);
  attwarp_jpegenc_header& h = T.h;
  std::memcpy(&h, table_host, sizeof h);
  if (h.magic == JE_MAGIC && h.reserved) {                   // reserved: where the PePlan lies, in 16-byte steps
    const uint64_t at = (uint64_t)(uint32_t)h.reserved * 16u;
    ATTWARP_REQUIRE(h.reserved > 0 && at + sizeof(PePlan) <= h.table_bytes, "jpegenc_encode: not a table of attwarp_jpegenc_plan_prog");
    std::memcpy(&T.pe, static_cast<const uint8_t*>(table_host) + at, sizeof T.pe);
    ATTWARP_REQUIRE(T.pe.nimages > 0 && T.pe.nimages <= h.B && T.pe.ntunits >= T.pe.nimages && T.pe.nsegs >= T.pe.nimages && T.pe.nsegs <= JE_MAX_UNITS &&
                        T.pe.ntunits <= JE_MAX_UNITS, "jpegenc_encode: not a table of attwarp_jpegenc_plan_prog");
  }
  ATTWARP_REQUIRE(h.magic == JE_MAGIC && h.B > 0 && h.nunits >= h.B - T.pe.nimages && h.nunits <= JE_MAX_UNITS, "jpegenc_encode: not a table of attwarp_jpegenc_plan");
  ATTWARP_REQUIRE(out_bytes >= h.out_bytes, "jpegenc_encode: out of %zu bytes, %llu needed", out_bytes, (unsigned long long)h.out_bytes);
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(table_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(scratch) % 16 == 0 &&
                      reinterpret_cast<uintptr_t>(offsets) % 8 == 0,
                  "jpegenc_encode: table_dev / offsets must be 8-byte, scratch 16-byte aligned");
  if (h.off_optimize) {                                      // (attwarp_jpegenc_plan_ex: some image takes tables of its own)
    ATTWARP_REQUIRE(h.off_optimize % 8 == 0 && h.off_optimize + sizeof(JoPlan) <= h.table_bytes, "jpegenc_encode: not a table of attwarp_jpegenc_plan_ex");
    std::memcpy(&T.jo, static_cast<const uint8_t*>(table_host) + h.off_optimize, sizeof T.jo);
    ATTWARP_REQUIRE(T.jo.nimages > 0 && T.jo.nimages <= h.B && T.jo.nunits >= T.jo.nimages && T.jo.nunits <= h.nunits,
                    "jpegenc_encode: not a table of attwarp_jpegenc_plan_ex");
  }
  return ATTWARP_OK;
}

}  // namespace attwarp

using namespace attwarp;

extern "C" size_t attwarp_jpegenc_bound(int H, int W, int C, int quality, int subsampling, int restart_rows) {
  return je_bound_of(H, W, C, quality, subsampling, restart_rows, false, false);
}

extern "C" size_t attwarp_jpegenc_bound_ex(int H, int W, int C, int quality, int subsampling, int restart_rows, int optimize) {
  return je_bound_of(H, W, C, quality, subsampling, restart_rows, optimize != 0, false);
}

extern "C" size_t attwarp_jpegenc_bound_prog(int H, int W, int C, int quality, int subsampling, int restart_rows, int optimize, int progressive) {
  return je_bound_of(H, W, C, quality, subsampling, restart_rows, optimize != 0, progressive != 0);
}

extern "C" size_t attwarp_jpegenc_table_bytes_prog(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, const int32_t* progressive) {
  JeCounts n;
  if (jpegenc_count(images, B, optimize, progressive, n) != ATTWARP_OK) return 0;
  return (size_t)jpegenc_table_layout(B, n).bytes;
}

extern "C" size_t attwarp_jpegenc_table_bytes_ex(const attwarp_jpegenc_image* images, int B, const int32_t* optimize) {
  return attwarp_jpegenc_table_bytes_prog(images, B, optimize, nullptr);
}

extern "C" size_t attwarp_jpegenc_table_bytes(const attwarp_jpegenc_image* images, int B) {
  return attwarp_jpegenc_table_bytes_ex(images, B, nullptr);
}

extern "C" int attwarp_jpegenc_plan_prog(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, const int32_t* progressive,
                                         void* table, size_t table_bytes) {
  JeCounts n;
  if (const int rc = jpegenc_count(images, B, optimize, progressive, n)) return rc;
  ATTWARP_REQUIRE(table, "jpegenc_plan: null table");
  const JeLayout at = jpegenc_table_layout(B, n);
  const size_t need = (size_t)at.bytes;
  ATTWARP_REQUIRE(table_bytes >= need, "jpegenc_plan: table of %zu bytes, %zu needed", table_bytes, need);
  if (at.off_progressive / 16 > 0x7fffffffull) return fail(ATTWARP_E_UNSUPPORTED, "jpegenc: a table of %zu bytes", need);
  uint8_t* t = static_cast<uint8_t*>(table);
  std::memset(t, 0, need);
  attwarp_jpegenc_header h;
  std::memset(&h, 0, sizeof h);
  h.magic = JE_MAGIC;
  h.B = B;
  h.nunits = (int32_t)n.nunits;
  h.reserved = (int32_t)(at.off_progressive / 16);           // where the PePlan lies, in 16-byte steps (0: no progressive image)
  h.table_bytes = need;
  h.off_images = at.off_images; h.off_units = at.off_units; h.off_huffman = at.off_huffman; h.off_optimize = at.off_optimize;
  for (int k = 0; k < 4; ++k) {
    uint32_t code[256];
    je_build_huffman(k, code);
    std::memcpy(t + h.off_huffman + (size_t)k * 1024, code, sizeof code);
  }
  JePlanner P(t, n, at);
  P.scratch.take((uint64_t)n.nunits * sizeof(JeUnitOut), 256);                 // the units' JeUnitOut lead the scratch buffer
  h.off_image_out = P.scratch.take((uint64_t)B * sizeof(JeImageOut), 256);
  JeImageDev* im = reinterpret_cast<JeImageDev*>(t + h.off_images);
  for (int b = 0; b < B; ++b) {
    JeImagePlan pl;
    je_image_plan(images[b], optimize && optimize[b], progressive && progressive[b], pl);     // (jpegenc_count accepted it)
    const int pre = je_fill_image(im[b], images[b], pl.g, pl.opt || pl.prog);
    im[b].unit0 = P.unit;
    if (pl.prog) je_plan_progressive(P, b, im[b], pl, pre);
    else je_plan_units(P, b, im[b], pl, images[b].quality, pre);
    h.out_bytes += pl.bound;
  }
  je_close_plans(P);
  h.scratch_bytes = P.scratch.at;
  std::memcpy(t, &h, sizeof h);
  return ATTWARP_OK;
}

extern "C" int attwarp_jpegenc_plan_ex(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, void* table, size_t table_bytes) {
  return attwarp_jpegenc_plan_prog(images, B, optimize, nullptr, table, table_bytes);
}

extern "C" int attwarp_jpegenc_plan(const attwarp_jpegenc_image* images, int B, void* table, size_t table_bytes) {
  return attwarp_jpegenc_plan_ex(images, B, nullptr, table, table_bytes);
}

// One launch: the kernel over `grid` workgroups of `block` threads on st; its own name goes into the error text.
#define JE_LAUNCH(kernel, grid, block, ...)                                          \
  do {                                                                               \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);         \
    if (const int rc = check_launch(#kernel)) return rc;                             \
  } while (0)

extern "C" int attwarp_jpegenc_encode(const void* table_host, const void* table_dev, void* scratch, uint8_t* out, size_t out_bytes,
                                      int64_t* offsets, void* stream) {
  JeTableHead T;
  if (const int rc = je_read_table(table_host, table_dev, scratch, out, out_bytes, offsets, T)) return rc;
  const attwarp_jpegenc_header& h = T.h;
  hipStream_t st = as_stream(stream);
  const uint8_t* td = static_cast<const uint8_t*>(table_dev);
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  const uint8_t* csc = sc;
  const int64_t* coffsets = offsets;
  const bool plain = h.nunits > 0;                           // (false: every image of the call is progressive)
  JE_LAUNCH(jpegenc_transform_kernel, h.nunits + T.pe.ntunits, JE_TNT, td, sc);
  if (T.jo.nimages) {                                        // optimised images: histograms, tables, header
    if (tune(TUNE_JPEGOPT_GIVEN_HIST) != 1) {                // (tuning flavour, 1: the caller filled the histograms)
      JE_LAUNCH(jpegopt_clear_kernel, T.jo.nimages, JE_NT, td, sc);
      JE_LAUNCH(jpegopt_histogram_kernel, T.jo.nunits, JE_NT, td, sc);
    }
    JE_LAUNCH(jpegopt_tables_kernel, T.jo.nimages, JE_NT, td, sc);
  }
  if (T.pe.nimages) {                                        // progressive images: statistics, tables, bytes
    JE_LAUNCH(jpegprogenc_clear_kernel, T.pe.nimages, JE_NT, td, sc);
    JE_LAUNCH(jpegprogenc_summary_kernel, T.pe.nsegs, JE_NT, td, sc);
    JE_LAUNCH(jpegprogenc_resolve_kernel, (T.pe.nsegs + PE_LANES - 1) / PE_LANES, PE_LANES, td, sc);
    JE_LAUNCH(jpegprogenc_count_kernel, T.pe.nsegs, JE_NT, td, sc);
    JE_LAUNCH(jpegprogenc_tables_kernel, T.pe.nimages, JE_NT, td, sc);
    JE_LAUNCH(jpegprogenc_code_kernel, T.pe.nsegs, JE_NT, td, sc);
  }
  if (plain) JE_LAUNCH(jpegenc_entropy_kernel, h.nunits, JE_NT, td, sc);
  JE_LAUNCH(jpegenc_scan_bits_kernel, h.B, JE_NT, td, sc);
  if (plain) JE_LAUNCH(jpegenc_gather_kernel, h.nunits, JE_NT, td, sc);
  JE_LAUNCH(jpegenc_scan_bytes_kernel, h.B, JE_NT, td, sc);
  if (T.pe.nimages) JE_LAUNCH(jpegprogenc_place_kernel, T.pe.nimages, JE_NT, td, sc);   // behind the scan above, which leaves no length for an image without units
  JE_LAUNCH(jpegenc_scan_files_kernel, 1, JE_NT, td, csc, offsets);
  if (plain) JE_LAUNCH(jpegenc_write_kernel, h.nunits, JE_NT, td, csc, out, coffsets);
  if (T.pe.nimages) JE_LAUNCH(jpegprogenc_write_kernel, T.pe.nsegs, JE_NT, td, csc, out, coffsets);
  return ATTWARP_OK;
}
