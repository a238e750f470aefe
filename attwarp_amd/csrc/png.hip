// PNG files of a whole ragged batch of uint8 images, written on the device (include/attwarp.h): what the
// reference's drivers do per sample with cv2.imwrite (main_batched.py:243-303; OpenCV's PNG writer defaults to the SUB
// filter and Z_RLE, i.e. matches at distance 1 only).  Three launches, none with a host-dependent argument:
//   png_encode_kernel    one workgroup per SEGMENT (whole rows, <= 24 KiB of filtered bytes, planned on the host from the
//                        image sizes): filter into LDS, find the runs, 286-bin histogram, length-limited Huffman code,
//                        one dynamic block + an empty stored block (byte aligned) or one stored block, built in LDS and
//                        copied to the segment's slot of the scratch buffer with its length, CRC-32 and Adler partial sums;
//   png_assemble_kernel  one workgroup per IMAGE: prefix sums of the segment lengths (file offset, segment offsets),
//                        Adler-32 and IDAT CRC-32 combined from the partials, signature / IHDR / IDAT head and the trailer;
//   png_gather_kernel    one workgroup per segment: scratch slot -> its place in the file.
// Every loop is bounded by a constant or by a size the planner checked; tests/png_ref.py restates the byte stream.
#include <algorithm>
#include <cstring>

#include "png_lz_blocks.hpp"

namespace attwarp {

#define PNG_G __attribute__((address_space(1)))
constexpr uint32_t PNG_MAGIC = 0x474e5041u;
constexpr int PNG_MAX_SEGS = 1 << 24;

// ---- workgroup scans over PNG_NT values (tmp: PNG_NT words) -----------------------------------------------------------------
__device__ __forceinline__ uint32_t png_excl_sum(uint32_t v, uint32_t* tmp, uint32_t& total) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  for (int o = 1; o < PNG_NT; o <<= 1) {
    const uint32_t a = t >= o ? tmp[t - o] : 0u;
    __syncthreads();
    tmp[t] += a;
    __syncthreads();
  }
  const uint32_t incl = tmp[t];
  total = tmp[PNG_NT - 1];
  __syncthreads();
  return incl - v;
}
// min over the threads AFTER this one (`none` when there is none)
__device__ __forceinline__ uint32_t png_suffix_min_excl(uint32_t v, uint32_t* tmp, uint32_t none) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  for (int o = 1; o < PNG_NT; o <<= 1) {
    const uint32_t a = t + o < PNG_NT ? tmp[t + o] : none;
    __syncthreads();
    tmp[t] = min(tmp[t], a);
    __syncthreads();
  }
  const uint32_t r = t + 1 < PNG_NT ? tmp[t + 1] : none;
  __syncthreads();
  return r;
}

// ---- source bytes ------------------------------------------------------------------------------------------------------------
struct PngSrc {
  const PNG_G uint8_t* p;
  int64_t pitch;
  int C;
  bool swap;
  // byte x of row r in the FILE's channel order; 0 outside the image (the specification's rule for the first row / pixel)
  __device__ __forceinline__ int at(int r, int x) const {
    if (r < 0 || x < 0) return 0;
    const int xs = swap ? x + 2 - 2 * (x % 3) : x;
    return p[(int64_t)r * pitch + xs];
  }
  __device__ __forceinline__ uint32_t filtered(int ft, int r, int x) const {
    const int a = (ft == 1 || ft >= 3) ? at(r, x - C) : 0, b = ft >= 2 ? at(r - 1, x) : 0;
    const int c = (ft == 4 && x >= C) ? at(r - 1, x - C) : 0;
    return png_filter(ft, at(r, x), a, b, c);
  }
};

// Twelve consecutive bytes of a row (four RGB pixels or twelve grey ones, x0 a multiple of 12, x0 + 12 <= W * C) from at
// most four dwords of the row and four of the row above, at any byte address -> their filtered bytes f[0 .. 11].
template <int C, bool SWAP>
__device__ __forceinline__ void png_filter_group(const PngSrc& src, int ft, int r, int x0, uint32_t (&f)[12]) {
  const PNG_G uint8_t* row = src.p + (int64_t)r * src.pitch + x0;
  uint32_t cw[4] = {0, 0, 0, 0}, uw[4] = {0, 0, 0, 0};       // [0]: bytes x0 - 4 .. x0 - 1, [1 .. 3]: the group
#pragma unroll
  for (int k = 0; k < 3; ++k) cw[1 + k] = *(const PNG_G u32_una*)(row + 4 * k);
  if (x0 > 0 && (ft == 1 || ft >= 3)) cw[0] = *(const PNG_G u32_una*)(row - 4);
  if (ft >= 2 && r > 0) {
    const PNG_G uint8_t* up = row - src.pitch;
#pragma unroll
    for (int k = 0; k < 3; ++k) uw[1 + k] = *(const PNG_G u32_una*)(up + 4 * k);
    if (x0 > 0 && ft == 4) uw[0] = *(const PNG_G u32_una*)(up - 4);
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    // byte k (and its left neighbour k - C) of the FILE's order sits at source byte k + 2 - 2 * channel when swapped
    const int kc = SWAP ? k + 2 - 2 * (k % 3) : k, ka = SWAP ? (k - 3) + 2 - 2 * (k % 3) : k - C;
    const int qc = kc + 4, qa = ka + 4;                       // 1 <= qa < qc <= 15
    const int cur = (cw[qc >> 2] >> (8 * (qc & 3))) & 255u, a = (cw[qa >> 2] >> (8 * (qa & 3))) & 255u;
    const int b = (uw[qc >> 2] >> (8 * (qc & 3))) & 255u, c = (uw[qa >> 2] >> (8 * (qa & 3))) & 255u;
    f[k] = png_filter(ft, cur, a, b, c);
  }
}

// ---- the bit writer: LSB first into zeroed LDS words; the first and last word of a thread are shared with its neighbours ----
struct PngBits {
  uint32_t* out;
  uint32_t word, n;
  uint64_t acc;
  __device__ __forceinline__ PngBits(uint32_t* o, uint32_t pos) : out(o), word(pos >> 5), n(pos & 31u), acc(0) {}
  __device__ __forceinline__ void put(uint32_t v, uint32_t nb) {      // nb <= 32
    acc |= (uint64_t)v << n;
    n += nb;
    if (n >= 32) {
      atomicOr(&out[word], (uint32_t)acc);
      acc >>= 32;
      n -= 32;
      ++word;
    }
  }
  __device__ __forceinline__ void flush() {
    if (acc) atomicOr(&out[word], (uint32_t)acc);
    acc = 0;
  }
  __device__ __forceinline__ uint32_t pos() const { return word * 32u + n; }
};

// The runs of equal bytes that START in this thread's chunk [lo, hi) of the segment, in order: f(value, length).  The last one
// ends at e_next, the first run start in a later chunk (the segment's end when there is none).
template <class F>
__device__ __forceinline__ void png_walk(const uint32_t* myw, int lo, int hi, uint32_t prevb, int e_next, F&& f) {
  int start = -1;
  uint32_t val = 0, prev = prevb, w = 0;
  for (int i = lo; i < hi; ++i) {
    const int k = i - lo;
    if ((k & 3) == 0) w = myw[k >> 2];
    const uint32_t b = (w >> (8 * (k & 3))) & 255u;
    if (b != prev) {
      if (start >= 0) f(val, (uint32_t)(i - start));
      start = i;
      val = b;
    }
    prev = b;
  }
  if (start >= 0) f(val, (uint32_t)(e_next - start));
}

// A run of n equal bytes: one literal, (n - 1) / 258 matches of 258, then the rest as one match (3 .. 257) or 1 - 2 literals.
struct PngRun {
  uint32_t lits, full, rem;            // rem >= 3: one more match of rem
  __device__ __forceinline__ explicit PngRun(uint32_t n) {
    const uint32_t r = n - 1;
    full = r / 258u;
    rem = r - full * 258u;
    lits = 1u + (rem < 3u ? rem : 0u);
    if (rem < 3u) rem = 0;
  }
};

// The segment a workgroup of an encode launch takes.  A table without LZ images (header.reserved == 0) has no order list:
// workgroup k takes segment k.  Otherwise the list behind the segments names the RLE segments first, then the LZ ones;
// `base` is where the launch's part starts.
__device__ __forceinline__ int png_segment_of(const uint8_t* table, const attwarp_png_header* hdr, int k, int base = 0) {
  if (hdr->reserved == 0) return k;
  return reinterpret_cast<const int32_t*>(table + hdr->off_segs + (uint64_t)hdr->nseg * sizeof(PngSeg))[base + k];
}

// Stage 4 of both encode kernels: code lengths of at most 15 bits for nsym <= PNG_SYMS symbols, at least two of them used:
// Huffman over (frequency, symbol) order; too deep -> halve the frequencies and rebuild.  Thread t owns symbols t and t + PNG_NT.
// At most 17 rounds: frequencies are below 2^16, after 16 halvings all are 1 and a tree of 286 equal leaves is 9 deep.  Ends on a
// barrier.
struct PngTree {
  uint32_t *freq, *lf, *nf;
  uint16_t* parent;
  uint32_t *n, *maxd;
};
__device__ __forceinline__ void png_code_lengths(const uint32_t* hist, int nsym, uint8_t* lens, const PngTree& w) {
  const int tid = threadIdx.x;
  const int sy[2] = {tid, tid + PNG_NT};
  for (int k = 0; k < 2; ++k)
    if (sy[k] < nsym) w.freq[sy[k]] = hist[sy[k]];
  __syncthreads();
  for (int round = 0; round < 17; ++round) {
    if (tid == 0) { *w.n = 0; *w.maxd = 0; }
    __syncthreads();
    int rank[2] = {-1, -1};
    for (int k = 0; k < 2; ++k) {
      const int s = sy[k];
      const uint32_t f = s < nsym ? w.freq[s] : 0u;
      if (f) {
        int r = 0;
        for (int o = 0; o < nsym; ++o) {
          const uint32_t fo = w.freq[o];
          r += (fo != 0u) && (fo < f || (fo == f && o < s));
        }
        rank[k] = r;
        w.lf[r] = f;
        atomicAdd(w.n, 1u);
      }
    }
    __syncthreads();
    const int n = (int)*w.n;
    if (tid == 0) {
      int li = 0, nj = 0, nn = 0;
      uint32_t lf = w.lf[0], nf = 0;
      for (int k = 0; k < n - 1; ++k) {
        uint32_t fsum = 0;
        for (int pick = 0; pick < 2; ++pick) {
          int id;
          if (li < n && (nj >= nn || lf <= nf)) {
            id = li; fsum += lf; ++li;
            lf = li < n ? w.lf[li] : 0u;
          } else {
            id = n + nj; fsum += nf; ++nj;
            nf = nj < nn ? w.nf[nj] : 0u;
          }
          w.parent[id] = (uint16_t)(n + k);
        }
        w.nf[k] = fsum;
        if (nj == nn) nf = fsum;
        nn = k + 1;
      }
    }
    __syncthreads();
    const int root = 2 * n - 2;
    for (int k = 0; k < 2; ++k) {
      if (sy[k] >= nsym) continue;
      int d = 0;
      if (rank[k] >= 0) {
        int id = rank[k];
        for (int step = 0; step < PNG_SYMS && id != root; ++step) { id = w.parent[id]; ++d; }
        atomicMax(w.maxd, (uint32_t)d);
      }
      lens[sy[k]] = (uint8_t)d;
    }
    __syncthreads();
    if (*w.maxd <= 15u) break;
    for (int k = 0; k < 2; ++k)
      if (sy[k] < nsym) { const uint32_t f = w.freq[sy[k]]; w.freq[sy[k]] = f ? (f + 1u) >> 1 : 0u; }
    __syncthreads();
  }
  __syncthreads();
}

// Canonical codes of nsym <= PNG_SYMS lengths, reversed for the LSB-first writer, packed as code | length << 16.  blc: 16 words.
__device__ __forceinline__ void png_canonical_codes(const uint8_t* lens, int nsym, uint32_t* codes, uint32_t* blc) {
  const int tid = threadIdx.x;
  const int sy[2] = {tid, tid + PNG_NT};
  if (tid < 16) blc[tid] = 0;
  __syncthreads();
  for (int k = 0; k < 2; ++k)
    if (sy[k] < nsym && lens[sy[k]]) atomicAdd(&blc[lens[sy[k]]], 1u);
  __syncthreads();
  uint32_t next[16];
  {
    uint32_t code = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) { code = (code + (b > 1 ? blc[b - 1] : 0u)) << 1; next[b] = code; }
  }
  for (int k = 0; k < 2; ++k) {
    const int s = sy[k];
    if (s >= nsym) continue;
    const uint32_t l = lens[s];
    uint32_t packed = 0;
    if (l) {
      uint32_t c = 0;
      for (int b = 1; b < 16; ++b) c = (l == (uint32_t)b) ? next[b] : c;
      for (int o = 0; o < s; ++o) c += lens[o] == l;
      packed = (__brev(c) >> (32u - l)) | (l << 16);
    }
    codes[s] = packed;
  }
  __syncthreads();
}

// Stage 1 of both encode kernels: the segment's rows, filtered, into LDS (one pad dword per chunk of PNG_CH bytes).
__device__ __forceinline__ void png_filter_segment(const PngSrc& src, const PngSeg& sg, int ftype, int RB, int WC, uint32_t* s_filt,
                                                   uint8_t* s_rowf) {
  const int tid = threadIdx.x;
  if (ftype == ATTWARP_PNG_ADAPTIVE) {                     // per row: the filter with the smallest sum of |int8|, one wave per row
    const int lane = tid & (WAVE - 1);
    for (int lr = tid / WAVE; lr < sg.nrows; lr += PNG_NT / WAVE) {
      const int r = sg.row0 + lr;
      uint32_t sum[5] = {0, 0, 0, 0, 0};
      for (int x = lane; x < WC; x += WAVE) {
        const int cur = src.at(r, x), a = src.at(r, x - src.C), b = src.at(r - 1, x), c = (x >= src.C) ? src.at(r - 1, x - src.C) : 0;
#pragma unroll
        for (int ft = 0; ft < 5; ++ft) {
          const uint32_t f = png_filter(ft, cur, a, b, c);
          sum[ft] += f < 128u ? f : 256u - f;
        }
      }
      int best = 0;
#pragma unroll
      for (int ft = 0; ft < 5; ++ft) {
        for (int o = WAVE / 2; o > 0; o >>= 1) sum[ft] += __shfl_xor(sum[ft], o, WAVE);
        if (sum[ft] < sum[best]) best = ft;
      }
      if (lane == 0) s_rowf[lr] = (uint8_t)best;
    }
  }
  __syncthreads();
  {
    // work items: (row, group of 12 source bytes); whole groups from dword loads, a row's last partial group byte by byte
    uint8_t* filt8 = reinterpret_cast<uint8_t*>(s_filt);
    auto put = [&](int i, uint32_t b) { filt8[i + (i / PNG_CH) * 4] = (uint8_t)b; };
    const int G = (WC + 11) / 12, items = sg.nrows * G;
    for (int item = tid; item < items; item += PNG_NT) {
      const int lr = item / G, g = item - lr * G, x0 = 12 * g, r = sg.row0 + lr;
      const int ft = ftype == ATTWARP_PNG_ADAPTIVE ? (int)s_rowf[lr] : ftype;
      const int i0 = lr * RB + 1 + x0;
      if (g == 0) put(i0 - 1, (uint32_t)ft);
      if (x0 + 12 <= WC) {
        uint32_t f[12];
        if (src.C == 1) png_filter_group<1, false>(src, ft, r, x0, f);
        else if (src.swap) png_filter_group<3, true>(src, ft, r, x0, f);
        else png_filter_group<3, false>(src, ft, r, x0, f);
#pragma unroll
        for (int k = 0; k < 12; ++k) put(i0 + k, f[k]);
      } else {
        for (int k = 0; k < WC - x0; ++k) put(i0 + k, src.filtered(ft, r, x0 + k));
      }
    }
  }
  __syncthreads();
}

// Last stage of both encode kernels: CRC-32 of the segment's deflate bytes (one table CRC per lane over equal slices, shifted to
// the end, XORed), the bytes to the segment's scratch slot, the segment's record (pad: the route, for PngBatch.routes()).
__device__ __forceinline__ void png_finish_segment(uint32_t out_len, uint32_t route, int seg, const PngSeg& sg, uint8_t* scratch,
                                                   const uint32_t* s_out, const uint32_t* s_crc, const uint32_t* s_pow, uint32_t* s_x,
                                                   const unsigned long long& s_a1, const unsigned long long& s_a2) {
  const int tid = threadIdx.x;
  const uint8_t* out8 = reinterpret_cast<const uint8_t*>(s_out);
  {
    const uint32_t L = (out_len + PNG_NT - 1) / PNG_NT;
    const uint32_t b0 = min(out_len, (uint32_t)tid * L), b1 = min(out_len, b0 + L);
    uint32_t c = 0xffffffffu;
    for (uint32_t i = b0; i < b1; ++i) c = s_crc[(c ^ out8[i]) & 255u] ^ (c >> 8);
    c = ~c;
    if (b0 == b1) c = 0;
    c = crc_mulmod(c, crc_xpow8(out_len - b1, s_pow));
    for (int o = WAVE / 2; o > 0; o >>= 1) c ^= __shfl_xor(c, o, WAVE);
    if ((tid & (WAVE - 1)) == 0) atomicXor(s_x, c);
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(scratch + sg.scratch_off);
  for (uint32_t i = tid; i < (out_len + 3u) / 4u; i += PNG_NT) dst[i] = s_out[i];
  __syncthreads();
  if (tid == 0) {
    PngSegOut o;
    o.len = out_len;
    o.crc = *s_x;
    o.s1 = (uint32_t)(s_a1 % PNG_ADLER);
    o.s2 = (uint32_t)(s_a2 % PNG_ADLER);
    o.pre = 0; o.pad = route;
    reinterpret_cast<PngSegOut*>(scratch)[seg] = o;
  }
}

__global__ __launch_bounds__(PNG_NT) void png_encode_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_filt[PNG_FILT_WORDS];
  __shared__ uint32_t s_out[PNG_OUT_WORDS];
  __shared__ uint32_t s_hist[PNG_SYMS_PAD], s_freq[PNG_SYMS_PAD], s_lf[PNG_SYMS_PAD], s_nf[PNG_SYMS_PAD], s_code[PNG_SYMS_PAD];
  __shared__ uint16_t s_parent[2 * PNG_SYMS_PAD];
  __shared__ uint8_t s_len[PNG_SYMS_PAD];
  __shared__ uint32_t s_crc[256], s_tmp[PNG_NT], s_pow[32], s_blc[16];
  __shared__ uint8_t s_rowf[ATTWARP_PNG_SEG_MAX_ROWS];
  __shared__ uint32_t s_n, s_maxd, s_bits, s_x;
  __shared__ unsigned long long s_a1, s_a2;

  const int tid = threadIdx.x;
  const attwarp_png_header* hdr = reinterpret_cast<const attwarp_png_header*>(table);
  const int seg = png_segment_of(table, hdr, (int)blockIdx.x);
  const PngSeg sg = reinterpret_cast<const PngSeg*>(table + hdr->off_segs)[seg];
  const PngImageDev* imp = reinterpret_cast<const PngImageDev*>(table + hdr->off_images) + sg.image;
  const int N = sg.n, RB = imp->row_bytes, WC = RB - 1, ftype = imp->filter;
  PngSrc src;
  src.p = (const PNG_G uint8_t*)imp->src;
  src.pitch = imp->pitch;
  src.C = imp->C;
  src.swap = imp->swap != 0;

  for (int i = tid; i < PNG_OUT_WORDS; i += PNG_NT) s_out[i] = 0;
  for (int i = tid; i < PNG_SYMS_PAD; i += PNG_NT) { s_hist[i] = 0; s_len[i] = 0; s_code[i] = 0; }
  s_crc[tid] = crc_table_entry((uint32_t)tid);
  if (tid < 32) s_pow[tid] = hdr->crc_pow8[tid];
  if (tid == 0) { s_bits = 0; s_x = 0; s_a1 = 0; s_a2 = 0; }

  // ---- 1. filter the segment's rows into LDS ------------------------------------------------------------------------------
  png_filter_segment(src, sg, ftype, RB, WC, s_filt, s_rowf);

  // ---- 2. run starts, Adler partial sums -----------------------------------------------------------------------------------
  const int lo = min(N, tid * PNG_CH), hi = min(N, lo + PNG_CH);
  const uint32_t* myw = s_filt + tid * (PNG_CHW + 1);
  uint32_t prevb = 0x100u;                                 // (no byte: position 0 starts a run)
  if (lo > 0 && lo < N) {
    const int q = (lo - 1) >> 2;
    prevb = (s_filt[q + q / PNG_CHW] >> (8 * ((lo - 1) & 3))) & 255u;
  }
  uint32_t first = (uint32_t)N;
  {
    uint32_t prev = prevb, w = 0;
    unsigned long long a1 = 0, a2 = 0;
    for (int i = lo; i < hi; ++i) {
      const int k = i - lo;
      if ((k & 3) == 0) w = myw[k >> 2];
      const uint32_t b = (w >> (8 * (k & 3))) & 255u;
      if (b != prev && first == (uint32_t)N) first = (uint32_t)i;
      prev = b;
      a1 += b;
      a2 += (unsigned long long)(N - i) * b;
    }
    if (lo < hi) { atomicAdd(&s_a1, a1); atomicAdd(&s_a2, a2); }
  }
  const int e_next = (int)png_suffix_min_excl(first, s_tmp, (uint32_t)N);

  // ---- 3. histogram ----------------------------------------------------------------------------------------------------------
  png_walk(myw, lo, hi, prevb, e_next, [&](uint32_t v, uint32_t n) {
    const PngRun run(n);
    atomicAdd(&s_hist[v], run.lits);
    if (run.full) atomicAdd(&s_hist[285], run.full);
    if (run.rem) {
      uint32_t sym, eb, ev;
      png_length_symbol(run.rem, sym, eb, ev);
      atomicAdd(&s_hist[sym], 1u);
    }
  });
  if (tid == 0) atomicAdd(&s_hist[256], 1u);               // end of block
  __syncthreads();

  // ---- 4. code lengths of at most 15 bits ----------------------------------------------------------------------------------------
  const int sy[2] = {tid, tid + PNG_NT};
  png_code_lengths(s_hist, PNG_SYMS, s_len, PngTree{s_freq, s_lf, s_nf, s_parent, &s_n, &s_maxd});

  // ---- 5. size of the dynamic block; canonical codes ------------------------------------------------------------------------------
  {
    uint32_t bits = 0;
    for (int k = 0; k < 2; ++k) {
      const int s = sy[k];
      if (s < PNG_SYMS) {
        uint32_t per = s_len[s];
        if (s > 256) {                                     // a match: extra bits (0 x 8, 1 x 4, .. 5 x 4, 0) and the 1-bit distance code
          const uint32_t ls = (uint32_t)s - 257u;
          per += ((ls < 8u || ls == 28u) ? 0u : (ls - 4u) / 4u) + 1u;
        }
        bits += s_hist[s] * per;
      }
    }
    atomicAdd(&s_bits, bits);
  }
  __syncthreads();
  const uint32_t dyn_bits = PNG_HEADER_BITS + s_bits;
  const uint32_t dyn_bytes = (dyn_bits + 3u + 7u) / 8u + 4u;
  const bool stored = dyn_bytes > (uint32_t)N + 5u;
  uint32_t out_len;
  uint8_t* out8 = reinterpret_cast<uint8_t*>(s_out);
  if (stored) {
    if (tid == 0) {
      out8[0] = 0;                                         // BFINAL = 0, BTYPE = 00
      out8[1] = (uint8_t)N; out8[2] = (uint8_t)(N >> 8);
      out8[3] = (uint8_t)~N; out8[4] = (uint8_t)(~N >> 8);
    }
    for (int i = tid; i < N; i += PNG_NT) {
      const int q = i >> 2;
      out8[5 + i] = (uint8_t)(s_filt[q + q / PNG_CHW] >> (8 * (i & 3)));
    }
    out_len = (uint32_t)N + 5u;
  } else {
    png_canonical_codes(s_len, PNG_SYMS, s_code, s_blc);
    // block header: BFINAL 0, BTYPE 10, HLIT 286, HDIST 1, HCLEN 19; a flat 4-bit code-length code for 0 .. 15 (16, 17, 18
    // unused come first in the transmission order); 286 + 1 lengths of 4 bits each, the distance code's being 1
    if (tid == 0) {
      PngBits w(s_out, 0);
      w.put(4u | 29u << 3 | 0u << 8 | 15u << 13, 17);
      w.put(0, 9);
      for (int k = 0; k < 16; ++k) w.put(4, 3);
      w.flush();
    }
    for (int k = 0; k < 2; ++k) {
      const int s = sy[k];
      if (s > PNG_SYMS) continue;
      const uint32_t l = s == PNG_SYMS ? 1u : s_len[s];
      PngBits w(s_out, 74u + 4u * (uint32_t)s);
      w.put(((l & 1u) << 3) | ((l & 2u) << 1) | ((l & 4u) >> 1) | ((l & 8u) >> 3), 4);
      w.flush();
    }
    // the tokens: bits per thread, their prefix sum, emission
    uint32_t mybits = 0;
    const uint32_t c285 = s_code[285];
    png_walk(myw, lo, hi, prevb, e_next, [&](uint32_t v, uint32_t n) {
      const PngRun run(n);
      mybits += run.lits * (s_code[v] >> 16) + run.full * ((c285 >> 16) + 1u);
      if (run.rem) {
        uint32_t sym, eb, ev;
        png_length_symbol(run.rem, sym, eb, ev);
        mybits += (s_code[sym] >> 16) + eb + 1u;
      }
    });
    uint32_t total;
    const uint32_t at = png_excl_sum(mybits, s_tmp, total);
    PngBits w(s_out, PNG_HEADER_BITS + at);
    png_walk(myw, lo, hi, prevb, e_next, [&](uint32_t v, uint32_t n) {
      const PngRun run(n);
      const uint32_t lit = s_code[v];
      w.put(lit & 0xffffu, lit >> 16);
      for (uint32_t k = 0; k < run.full; ++k) {            // (<= PNG_SEG / 258)
        w.put(c285 & 0xffffu, c285 >> 16);
        w.put(0, 1);
      }
      if (run.rem) {
        uint32_t sym, eb, ev;
        png_length_symbol(run.rem, sym, eb, ev);
        const uint32_t c = s_code[sym];
        w.put(c & 0xffffu, c >> 16);
        w.put(ev, eb + 1u);                                // extra bits, then the distance code 0
      } else {
        for (uint32_t k = 1; k < run.lits; ++k) w.put(lit & 0xffffu, lit >> 16);
      }
    });
    w.flush();
    if (tid == PNG_NT - 1) {                               // end of block, then the empty stored block 000 / pad / 00 00 FF FF
      PngBits e(s_out, PNG_HEADER_BITS + total);
      const uint32_t c = s_code[256];
      e.put(c & 0xffffu, c >> 16);
      e.flush();
      const uint32_t byte = (e.pos() + 3u + 7u) / 8u;
      PngBits t(s_out, byte * 8u);
      t.put(0xffff0000u, 32);
      t.flush();
    }
    out_len = dyn_bytes;
  }
  __syncthreads();

  // ---- 6. CRC-32 of the segment's bytes; write out -------------------------------------------------------------------------------
  png_finish_segment(out_len, stored ? PNG_ROUTE_STORED : PNG_ROUTE_RLE, seg, sg, scratch, s_out, s_crc, s_pow, &s_x, s_a1, s_a2);
}

// ---- the second token route: matches at any distance inside the segment (tests/pnglz_ref.py restates it) ---------
// The segment's bytes in LDS (the chunk layout above): aligned dword q, byte i, the four bytes at i (i + 4 <= N).
__device__ __forceinline__ uint32_t png_seg_word(const uint32_t* f, int q) { return f[q + q / PNG_CHW]; }
__device__ __forceinline__ uint32_t png_seg_byte(const uint32_t* f, int i) { return (png_seg_word(f, i >> 2) >> (8 * (i & 3))) & 255u; }
__device__ __forceinline__ uint32_t png_seg_ld32(const uint32_t* f, int i) {
  const int q = i >> 2, sh = 8 * (i & 3);
  const uint32_t a = png_seg_word(f, q);
  return sh ? (a >> sh) | (png_seg_word(f, q + 1) << (32 - sh)) : a;
}
// common prefix of the bytes at i and at c < i, at most cap <= min(258, N - i): at most 64 dword rounds and 3 bytes
__device__ __forceinline__ uint32_t png_match_len(const uint32_t* f, int i, int c, uint32_t cap) {
  uint32_t k = 0;
  for (; k + 4u <= cap; k += 4u) {
    const uint32_t x = png_seg_ld32(f, i + (int)k) ^ png_seg_ld32(f, c + (int)k);
    if (x) return k + ((uint32_t)__builtin_ctz(x) >> 3);
  }
  for (; k < cap; ++k)
    if (png_seg_byte(f, i + (int)k) != png_seg_byte(f, c + (int)k)) break;
  return k;
}

// Where position i's token word lives: one pad word per chunk, as the filtered bytes (a wave walking its chunks hits 64 banks).
__device__ __forceinline__ int png_tok_at(int i) { return i + i / PNG_CH; }

// The LZ tokens that START in [e, hi), e being where the greedy chain enters the chunk (>= hi: none): fl(value) for a
// literal, fm(length, distance) for a match.  At most hi - e <= PNG_CH rounds.
template <class FL, class FM>
__device__ __forceinline__ void png_lz_walk(const uint32_t* tok, const uint32_t* f, int e, int hi, FL&& fl, FM&& fm) {
  for (int i = e; i < hi;) {
    const uint32_t t = tok[png_tok_at(i)], dist = png_lz_token_dist(t);
    if (dist == 0) { fl(png_seg_byte(f, i)); ++i; }
    else { const uint32_t len = png_lz_token_len(t); fm(len, dist); i += (int)len; }
  }
}

// One workgroup per segment of a match = LZ image.  It sizes png_encode_kernel's block, the LZ block and the stored block and
// writes the shortest (ties: in that order), so a segment where RLE wins carries png_encode_kernel's bytes.
__global__ __launch_bounds__(PNG_NT) void png_encode_lz_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  // The __shared__ variables below sum to PNG_LZ_STATIC_LDS (png_lz_blocks.hpp), which the launcher's static_assert holds against the
  // CU's 160 KiB beside the token words: change that constant with them ("LDS Size" of -Rpass-analysis=kernel-resource-usage).
  extern __shared__ uint32_t s_tok[];                      // PNG_LZ_TOKEN_BYTES: candidate + 1, then the token, of every position
  __shared__ uint32_t s_filt[PNG_FILT_WORDS];
  __shared__ uint32_t s_out[PNG_OUT_WORDS];
  __shared__ uint32_t s_hist[PNG_SYMS_PAD], s_histz[PNG_SYMS_PAD], s_freq[PNG_SYMS_PAD], s_lf[PNG_SYMS_PAD], s_nf[PNG_SYMS_PAD];
  __shared__ uint32_t s_code[PNG_SYMS_PAD], s_dhist[32], s_dcode[32];
  __shared__ uint16_t s_parent[2 * PNG_SYMS_PAD];
  __shared__ uint8_t s_len[PNG_SYMS_PAD], s_lenz[PNG_SYMS_PAD], s_dlen[32];
  __shared__ uint32_t s_crc[256], s_tmp[PNG_NT], s_entry[PNG_NT], s_pow[32], s_blc[16];
  __shared__ uint8_t s_rowf[ATTWARP_PNG_SEG_MAX_ROWS];
  __shared__ uint32_t s_n, s_maxd, s_bits[2], s_x;
  __shared__ unsigned long long s_a1, s_a2;

  const int tid = threadIdx.x;
  const attwarp_png_header* hdr = reinterpret_cast<const attwarp_png_header*>(table);
  const int seg = png_segment_of(table, hdr, (int)blockIdx.x, hdr->nseg - hdr->reserved);
  const PngSeg sg = reinterpret_cast<const PngSeg*>(table + hdr->off_segs)[seg];
  const PngImageDev* imp = reinterpret_cast<const PngImageDev*>(table + hdr->off_images) + sg.image;
  const int N = sg.n, RB = imp->row_bytes, WC = RB - 1, ftype = imp->filter;
  PngSrc src;
  src.p = (const PNG_G uint8_t*)imp->src;
  src.pitch = imp->pitch;
  src.C = imp->C;
  src.swap = imp->swap != 0;
  const PngTree tree = {s_freq, s_lf, s_nf, s_parent, &s_n, &s_maxd};

  for (int i = tid; i < PNG_OUT_WORDS; i += PNG_NT) s_out[i] = 0;
  for (int i = tid; i < PNG_SYMS_PAD; i += PNG_NT) { s_hist[i] = 0; s_histz[i] = 0; s_len[i] = 0; s_lenz[i] = 0; s_code[i] = 0; }
  if (tid < 32) { s_dhist[tid] = 0; s_dcode[tid] = 0; s_dlen[tid] = 0; }
  s_crc[tid] = crc_table_entry((uint32_t)tid);
  if (tid < 32) s_pow[tid] = hdr->crc_pow8[tid];
  if (tid == 0) { s_bits[0] = 0; s_bits[1] = 0; s_x = 0; s_a1 = 0; s_a2 = 0; }

  // ---- 1. filter the segment's rows into LDS ------------------------------------------------------------------------------
  png_filter_segment(src, sg, ftype, RB, WC, s_filt, s_rowf);

  // ---- 2. run starts, Adler partial sums (png_encode_kernel's stage 2) ----------------------------------------------------------
  const int lo = min(N, tid * PNG_CH), hi = min(N, lo + PNG_CH);
  const uint32_t* myw = s_filt + tid * (PNG_CHW + 1);
  uint32_t prevb = 0x100u;
  if (lo > 0 && lo < N) prevb = png_seg_byte(s_filt, lo - 1);
  uint32_t first = (uint32_t)N;
  {
    uint32_t prev = prevb, w = 0;
    unsigned long long a1 = 0, a2 = 0;
    for (int i = lo; i < hi; ++i) {
      const int k = i - lo;
      if ((k & 3) == 0) w = myw[k >> 2];
      const uint32_t b = (w >> (8 * (k & 3))) & 255u;
      if (b != prev && first == (uint32_t)N) first = (uint32_t)i;
      prev = b;
      a1 += b;
      a2 += (unsigned long long)(N - i) * b;
    }
    if (lo < hi) { atomicAdd(&s_a1, a1); atomicAdd(&s_a2, a2); }
  }
  const int e_next = (int)png_suffix_min_excl(first, s_tmp, (uint32_t)N);

  // ---- 3. candidates: block after block of PNG_LZ_BLOCK positions looks its hash up, then publishes itself.  atomicMax of
  // positions: the head of a hash is the largest position of the earlier blocks whatever the order of arrival.  The heads live
  // in the (still unused, zero) output words as position + 1. ----------------------------------------------------------------------
  {
    uint32_t* head = s_out;
    const int nh = N >= 4 ? N - 3 : 0;                     // positions that have a key
    for (int b0 = 0; b0 < N; b0 += PNG_LZ_BLOCK) {         // (<= PNG_SEG / PNG_LZ_BLOCK rounds, uniform)
      const int i = b0 + tid;
      const bool keyed = i < nh;
      uint32_t h = 0;
      if (keyed) h = png_lz_hash(png_seg_ld32(s_filt, i));
      if (i < N) s_tok[png_tok_at(i)] = keyed ? head[h] : 0u;
      __syncthreads();
      if (keyed) atomicMax(&head[h], (uint32_t)i + 1u);
      __syncthreads();
    }
    for (int i = tid; i < (1 << PNG_LZ_HASH_BITS); i += PNG_NT) head[i] = 0;
    s_entry[tid] = (uint32_t)N;
  }
  __syncthreads();

  // ---- 4. the token of every position of this thread's chunk, last position first: the distance-1 run from the run ends, the
  // far match by comparing dwords, and where the chain through the position leaves the chunk -----------------------------------------
  {
    int re = e_next;                                       // the first run start behind position i
    uint32_t b = hi > lo ? png_seg_byte(s_filt, hi - 1) : 0u;
    for (int i = hi - 1; i >= lo; --i) {
      const uint32_t pb = i > 0 ? png_seg_byte(s_filt, i - 1) : 0x100u;
      const uint32_t cap = min(PNG_LZ_MAX_LEN, (uint32_t)(N - i));
      uint32_t run = 0;
      if (b == pb) run = min(cap, (uint32_t)(re - i));
      else re = i;
      const uint32_t c1 = s_tok[png_tok_at(i)];                        // candidate + 1 <= i
      uint32_t far = 0;
      if (c1 && run < cap) far = png_match_len(s_filt, i, (int)c1 - 1, cap);
      uint32_t len = 1, dist = 0;
      if (png_lz_takes_far(far, run)) { len = far; dist = (uint32_t)i + 1u - c1; }
      else if (run >= 3u) { len = run; dist = 1; }
      const int nx = i + (int)len;                         // <= N
      const uint32_t ex = nx >= hi ? (uint32_t)(nx - hi) : png_lz_token_exit(s_tok[png_tok_at(nx)]);
      s_tok[png_tok_at(i)] = png_lz_token(dist, len, ex);
      b = pb;
    }
  }
  __syncthreads();
  // the greedy chain from position 0, chunk by chunk: where it enters each chunk (N: it jumps over the chunk)
  if (tid == 0) {
    int p = 0;
    for (int k = 0; k < PNG_NT && p < N; ++k) {
      const int t = p / PNG_CH;
      s_entry[t] = (uint32_t)p;
      p = min(N, (t + 1) * PNG_CH) + (int)png_lz_token_exit(s_tok[png_tok_at(p)]);
    }
  }
  __syncthreads();
  const int entry = (int)s_entry[tid];

  // ---- 5. both histograms, both pairs of codes, the three sizes ------------------------------------------------------------------------
  png_walk(myw, lo, hi, prevb, e_next, [&](uint32_t v, uint32_t n) {
    const PngRun run(n);
    atomicAdd(&s_hist[v], run.lits);
    if (run.full) atomicAdd(&s_hist[285], run.full);
    if (run.rem) {
      uint32_t sym, eb, ev;
      png_length_symbol(run.rem, sym, eb, ev);
      atomicAdd(&s_hist[sym], 1u);
    }
  });
  png_lz_walk(s_tok, s_filt, entry, hi, [&](uint32_t v) { atomicAdd(&s_histz[v], 1u); },
              [&](uint32_t len, uint32_t dist) {
                uint32_t sym, eb, ev;
                png_length_symbol(len, sym, eb, ev);
                atomicAdd(&s_histz[sym], 1u);
                png_dist_symbol(dist, sym, eb, ev);
                atomicAdd(&s_dhist[sym], 1u);
              });
  if (tid == 0) { atomicAdd(&s_hist[256], 1u); atomicAdd(&s_histz[256], 1u); }
  __syncthreads();
  png_code_lengths(s_hist, PNG_SYMS, s_len, tree);
  png_code_lengths(s_histz, PNG_SYMS, s_lenz, tree);
  int dused = 0, dfirst = 0;                               // (uniform: every thread reads the same 30 words)
  for (int s = PNG_DSYMS - 1; s >= 0; --s)
    if (s_dhist[s]) { ++dused; dfirst = s; }
  if (dused >= 2) png_code_lengths(s_dhist, PNG_DSYMS, s_dlen, tree);
  else if (tid < 32) s_dlen[tid] = tid == dfirst;          // no distance or one: a single 1-bit code
  __syncthreads();
  {
    const int sy[2] = {tid, tid + PNG_NT};
    uint32_t br = 0, bz = 0;
    for (int k = 0; k < 2; ++k) {
      const int s = sy[k];
      if (s >= PNG_SYMS) continue;
      const uint32_t ex = s > 256 ? png_length_extra((uint32_t)s - 257u) : 0u;
      br += s_hist[s] * (s_len[s] + ex + (s > 256 ? 1u : 0u));      // (+ the 1-bit distance code)
      bz += s_histz[s] * (s_lenz[s] + ex);
    }
    if (tid < PNG_DSYMS) bz += s_dhist[tid] * (s_dlen[tid] + png_dist_extra((uint32_t)tid));
    atomicAdd(&s_bits[0], br);
    atomicAdd(&s_bits[1], bz);
  }
  __syncthreads();
  const uint32_t rle_bytes = (PNG_HEADER_BITS + s_bits[0] + 3u + 7u) / 8u + 4u;
  const uint32_t lz_bytes = (PNG_LZ_HEADER_BITS + s_bits[1] + 3u + 7u) / 8u + 4u;
  const uint32_t st_bytes = (uint32_t)N + 5u;
  const uint32_t route = (rle_bytes <= lz_bytes && rle_bytes <= st_bytes) ? PNG_ROUTE_RLE : lz_bytes <= st_bytes ? PNG_ROUTE_LZ : PNG_ROUTE_STORED;

  // ---- 6. the chosen form into the output words ---------------------------------------------------------------------------------------
  uint32_t out_len;
  uint8_t* out8 = reinterpret_cast<uint8_t*>(s_out);
  if (route == PNG_ROUTE_STORED) {
    if (tid == 0) {
      out8[0] = 0;
      out8[1] = (uint8_t)N; out8[2] = (uint8_t)(N >> 8);
      out8[3] = (uint8_t)~N; out8[4] = (uint8_t)(~N >> 8);
    }
    for (int i = tid; i < N; i += PNG_NT) out8[5 + i] = (uint8_t)png_seg_byte(s_filt, i);
    out_len = st_bytes;
  } else {
    const bool lz = route == PNG_ROUTE_LZ;
    const uint8_t* lens = lz ? s_lenz : s_len;
    const int nd = lz ? PNG_DSYMS : 1;
    const uint32_t header_bits = lz ? PNG_LZ_HEADER_BITS : PNG_HEADER_BITS;
    if (!lz && tid < 32) s_dlen[tid] = tid == 0;           // the RLE block's one distance code
    png_canonical_codes(lens, PNG_SYMS, s_code, s_blc);    // (its first barrier covers s_dlen)
    png_canonical_codes(s_dlen, PNG_DSYMS, s_dcode, s_blc);
    // block header: BFINAL 0, BTYPE 10, HLIT 286, HDIST nd, HCLEN 19; the flat 4-bit code-length code; 286 + nd lengths
    if (tid == 0) {
      PngBits w(s_out, 0);
      w.put(4u | 29u << 3 | (uint32_t)(nd - 1) << 8 | 15u << 13, 17);
      w.put(0, 9);
      for (int k = 0; k < 16; ++k) w.put(4, 3);
      w.flush();
    }
    for (int s = tid; s < PNG_SYMS + nd; s += PNG_NT) {
      const uint32_t l = s < PNG_SYMS ? lens[s] : s_dlen[s - PNG_SYMS];
      PngBits w(s_out, 74u + 4u * (uint32_t)s);
      w.put(((l & 1u) << 3) | ((l & 2u) << 1) | ((l & 4u) >> 1) | ((l & 8u) >> 3), 4);
      w.flush();
    }
    // the tokens of this thread's chunk in stream order, of either route: fl(value), fm(length, distance)
    auto walk = [&](auto&& fl, auto&& fm) {
      if (lz) png_lz_walk(s_tok, s_filt, entry, hi, fl, fm);
      else
        png_walk(myw, lo, hi, prevb, e_next, [&](uint32_t v, uint32_t n) {
          const PngRun run(n);
          fl(v);
          for (uint32_t k = 0; k < run.full; ++k) fm(258u, 1u);       // (<= PNG_SEG / 258)
          if (run.rem) fm(run.rem, 1u);
          else
            for (uint32_t k = 1; k < run.lits; ++k) fl(v);
        });
    };
    uint32_t mybits = 0;
    walk([&](uint32_t v) { mybits += s_code[v] >> 16; },
         [&](uint32_t len, uint32_t dist) {
           uint32_t sym, eb, ev, dsym, deb, dev;
           png_length_symbol(len, sym, eb, ev);
           png_dist_symbol(dist, dsym, deb, dev);
           mybits += (s_code[sym] >> 16) + eb + (s_dcode[dsym] >> 16) + deb;
         });
    uint32_t total;
    const uint32_t at = png_excl_sum(mybits, s_tmp, total);
    PngBits w(s_out, header_bits + at);
    walk([&](uint32_t v) { const uint32_t c = s_code[v]; w.put(c & 0xffffu, c >> 16); },
         [&](uint32_t len, uint32_t dist) {
           uint32_t sym, eb, ev, dsym, deb, dev;
           png_length_symbol(len, sym, eb, ev);
           png_dist_symbol(dist, dsym, deb, dev);
           const uint32_t c = s_code[sym], d = s_dcode[dsym];
           w.put(c & 0xffffu, c >> 16);
           w.put(ev, eb);
           w.put(d & 0xffffu, d >> 16);
           w.put(dev, deb);
         });
    w.flush();
    if (tid == PNG_NT - 1) {                               // end of block, then the empty stored block 000 / pad / 00 00 FF FF
      PngBits e(s_out, header_bits + total);
      const uint32_t c = s_code[256];
      e.put(c & 0xffffu, c >> 16);
      e.flush();
      const uint32_t byte = (e.pos() + 3u + 7u) / 8u;
      PngBits t(s_out, byte * 8u);
      t.put(0xffff0000u, 32);
      t.flush();
    }
    out_len = lz ? lz_bytes : rle_bytes;
  }
  __syncthreads();

  // ---- 7. CRC-32 of the segment's bytes; write out -------------------------------------------------------------------------------
  png_finish_segment(out_len, route, seg, sg, scratch, s_out, s_crc, s_pow, &s_x, s_a1, s_a2);
}

// One workgroup per image.
__global__ __launch_bounds__(PNG_NT) void png_assemble_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch,
                                                              uint8_t* __restrict__ out, int64_t* __restrict__ offsets) {
  __shared__ uint32_t s_tmp[PNG_NT], s_pow[32];
  __shared__ unsigned long long s_prev, s_a, s_b;
  __shared__ uint32_t s_x;
  const int tid = threadIdx.x, b = blockIdx.x;
  const attwarp_png_header* hdr = reinterpret_cast<const attwarp_png_header*>(table);
  const PngSeg* segs = reinterpret_cast<const PngSeg*>(table + hdr->off_segs);
  const PngImageDev* imp = reinterpret_cast<const PngImageDev*>(table + hdr->off_images) + b;
  PngSegOut* so = reinterpret_cast<PngSegOut*>(scratch);
  const int seg0 = imp->seg0, nseg = imp->nseg;
  if (tid < 32) s_pow[tid] = hdr->crc_pow8[tid];
  if (tid == 0) { s_prev = 0; s_a = 0; s_b = 0; s_x = 0; }
  __syncthreads();
  // deflate bytes of every earlier image -> this file's offset
  {
    unsigned long long v = 0;
    for (int s = tid; s < seg0; s += PNG_NT) v += so[s].len;
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    if ((tid & (WAVE - 1)) == 0) atomicAdd(&s_prev, v);
  }
  // offsets of the image's segments in its stream
  uint32_t carry = 0;
  for (int base = 0; base < nseg; base += PNG_NT) {
    const int s = base + tid;
    const uint32_t len = s < nseg ? so[seg0 + s].len : 0u;
    uint32_t tot;
    const uint32_t pre = carry + png_excl_sum(len, s_tmp, tot);
    if (s < nseg) so[seg0 + s].pre = pre;
    carry += tot;
  }
  const uint32_t total = carry;                            // (after a barrier of png_excl_sum: s_prev is complete too)
  // Adler-32: a = 1 + sum S1, b = N + sum S2 + sum S1 * (filtered bytes behind the segment); CRC-32 of the segments, each
  // shifted by the IDAT bytes behind it (the rest of the segments and the 9 trailer bytes)
  {
    unsigned long long a = 0, bb = 0;
    uint32_t x = 0;
    for (int s = tid; s < nseg; s += PNG_NT) {
      const PngSegOut o = so[seg0 + s];
      const PngSeg g = segs[seg0 + s];
      a += o.s1;
      bb += o.s2 + (unsigned long long)o.s1 * (g.after % PNG_ADLER) % PNG_ADLER;
      x ^= crc_mulmod(o.crc, crc_xpow8(total - o.pre - o.len + 9u, s_pow));
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, WAVE);
      bb += __shfl_xor(bb, o, WAVE);
      x ^= __shfl_xor(x, o, WAVE);
    }
    if ((tid & (WAVE - 1)) == 0) { atomicAdd(&s_a, a); atomicAdd(&s_b, bb); atomicXor(&s_x, x); }
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned long long nraw = (unsigned long long)imp->H * (unsigned long long)imp->row_bytes;
    const uint32_t a = (uint32_t)((1ull + s_a) % PNG_ADLER), bsum = (uint32_t)((nraw + s_b) % PNG_ADLER);
    const uint32_t adler = bsum << 16 | a;
    const int64_t off = (int64_t)s_prev + (int64_t)ATTWARP_PNG_FILE_OVERHEAD * b;
    PNG_G uint8_t* f = (PNG_G uint8_t*)out + off;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int i = 0; i < 8; ++i) f[i] = sig[i];
    for (int i = 0; i < 25; ++i) f[8 + i] = imp->ihdr[i];
    const uint32_t dlen = 2u + total + 9u;
    f[33] = (uint8_t)(dlen >> 24); f[34] = (uint8_t)(dlen >> 16); f[35] = (uint8_t)(dlen >> 8); f[36] = (uint8_t)dlen;
    f[37] = 'I'; f[38] = 'D'; f[39] = 'A'; f[40] = 'T';
    f[41] = 0x78; f[42] = 0x01;
    uint8_t tail[9] = {0x01, 0x00, 0x00, 0xff, 0xff, (uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8), (uint8_t)adler};
    uint32_t crc = crc_mulmod(hdr->idat_head_crc, crc_xpow8(total + 9u, s_pow)) ^ s_x ^ crc_bytes(tail, 9);
    PNG_G uint8_t* t = f + PNG_FILE_HEAD + total;
    for (int i = 0; i < 9; ++i) t[i] = tail[i];
    t[9] = (uint8_t)(crc >> 24); t[10] = (uint8_t)(crc >> 16); t[11] = (uint8_t)(crc >> 8); t[12] = (uint8_t)crc;
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) t[13 + i] = iend[i];
    offsets[b] = off;
    if (b == (int)gridDim.x - 1) offsets[b + 1] = off + ATTWARP_PNG_FILE_OVERHEAD + total;
  }
}

// One workgroup per segment: its bytes from the scratch slot to their place in the file (aligned dword stores).
__global__ __launch_bounds__(PNG_NT) void png_gather_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ scratch,
                                                            uint8_t* __restrict__ out, const int64_t* __restrict__ offsets) {
  const int tid = threadIdx.x;
  const attwarp_png_header* hdr = reinterpret_cast<const attwarp_png_header*>(table);
  const PngSeg sg = reinterpret_cast<const PngSeg*>(table + hdr->off_segs)[blockIdx.x];
  const PngSegOut o = reinterpret_cast<const PngSegOut*>(scratch)[blockIdx.x];
  const PNG_G uint8_t* s = (const PNG_G uint8_t*)scratch + sg.scratch_off;
  PNG_G uint8_t* d = (PNG_G uint8_t*)out + offsets[sg.image] + PNG_FILE_HEAD + o.pre;
  const uint32_t len = o.len;
  const uint32_t head = min(len, (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(d) & 3u)) & 3u));
  const uint32_t nw = (len - head) / 4u;
  if ((uint32_t)tid < head) d[tid] = s[tid];
  for (uint32_t w = tid; w < nw; w += PNG_NT)
    *(PNG_G uint32_t*)(d + head + 4u * w) = *(const PNG_G u32_una*)(s + head + 4u * w);
  const uint32_t done = head + 4u * nw;
  if ((uint32_t)tid < len - done) d[done + tid] = s[done + tid];
}

// ---- host: limits, bound, plan ---------------------------------------------------------------------------------------------
static bool png_shape_ok(int64_t H, int64_t W, int64_t C) {
  return H >= 1 && W >= 1 && (C == 1 || C == 3) && 1 + W * C <= ATTWARP_PNG_MAX_ROW_BYTES;
}
static uint64_t png_bound64(int64_t H, int64_t W, int64_t C) {
  const int64_t rb = 1 + W * C, rps = png_rows_per_segment((int)rb), nseg = (H + rps - 1) / rps;
  return (uint64_t)ATTWARP_PNG_FILE_OVERHEAD + (uint64_t)H * rb + 5u * (uint64_t)nseg;
}
static uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

}  // namespace attwarp

using namespace attwarp;

extern "C" size_t attwarp_png_bound(int H, int W, int C) {
  if (!png_shape_ok(H, W, C)) return 0;
  const uint64_t b = png_bound64(H, W, C);
  return b < ((uint64_t)1 << 31) ? (size_t)b : 0;
}

static int png_count(const attwarp_png_image* images, int B, const int32_t* match, int64_t& nseg, int64_t& nlz) {
  ATTWARP_REQUIRE(images, "png: null image array");
  ATTWARP_REQUIRE(B > 0, "png: non-positive batch size");
  if (B > (1 << 20)) return fail(ATTWARP_E_UNSUPPORTED, "png: B=%d > 2^20", B);
  nseg = nlz = 0;
  for (int b = 0; b < B; ++b) {
    const attwarp_png_image& d = images[b];
    ATTWARP_REQUIRE(d.src, "png: image %d: null pointer", b);
    ATTWARP_REQUIRE(!match || match[b] == ATTWARP_PNG_MATCH_RLE || match[b] == ATTWARP_PNG_MATCH_LZ, "png: image %d: unknown match %d", b,
                    match ? match[b] : 0);
    ATTWARP_REQUIRE(d.H >= 1 && d.W >= 1, "png: image %d: non-positive size %d x %d", b, d.H, d.W);
    ATTWARP_REQUIRE(d.C == 1 || d.C == 3, "png: image %d: %d channels (1 or 3)", b, d.C);
    ATTWARP_REQUIRE(d.order == ATTWARP_RGB || d.order == ATTWARP_BGR, "png: image %d: channel order must be ATTWARP_RGB or ATTWARP_BGR", b);
    ATTWARP_REQUIRE(d.filter >= ATTWARP_PNG_NONE && d.filter <= ATTWARP_PNG_ADAPTIVE, "png: image %d: unknown filter %d", b, d.filter);
    if (!png_shape_ok(d.H, d.W, d.C))
      return fail(ATTWARP_E_UNSUPPORTED, "png: image %d: row of %lld bytes (> %d)", b, 1 + (long long)d.W * d.C, ATTWARP_PNG_MAX_ROW_BYTES);
    ATTWARP_REQUIRE((int64_t)d.pitch >= (int64_t)d.W * d.C, "png: image %d: pitch %d below the row's %lld bytes", b, d.pitch, (long long)d.W * d.C);
    if (attwarp_png_bound(d.H, d.W, d.C) == 0) return fail(ATTWARP_E_UNSUPPORTED, "png: image %d: %d x %d x %d is 2 GiB or more", b, d.H, d.W, d.C);
    const int rps = png_rows_per_segment(1 + d.W * d.C);
    nseg += (d.H + rps - 1) / rps;
    if (match && match[b] == ATTWARP_PNG_MATCH_LZ) nlz += (d.H + rps - 1) / rps;
  }
  if (nseg > PNG_MAX_SEGS) return fail(ATTWARP_E_UNSUPPORTED, "png: %lld segments in one call (> %d)", (long long)nseg, PNG_MAX_SEGS);
  return ATTWARP_OK;
}

// A table with LZ segments ends with the order list (png_segment_of): one int32 per segment.
extern "C" size_t attwarp_png_table_bytes_ex(const attwarp_png_image* images, int B, const int32_t* match) {
  int64_t nseg, nlz;
  if (png_count(images, B, match, nseg, nlz) != ATTWARP_OK) return 0;
  return (size_t)(align_up(sizeof(attwarp_png_header), 16) + align_up((uint64_t)B * sizeof(PngImageDev), 16) + (uint64_t)nseg * sizeof(PngSeg) +
                  (nlz ? align_up((uint64_t)nseg * sizeof(int32_t), 8) : 0u));
}
extern "C" size_t attwarp_png_table_bytes(const attwarp_png_image* images, int B) { return attwarp_png_table_bytes_ex(images, B, nullptr); }

extern "C" int attwarp_png_plan_ex(const attwarp_png_image* images, int B, const int32_t* match, void* table, size_t table_bytes) {
  int64_t nseg, nlz;
  if (const int rc = png_count(images, B, match, nseg, nlz)) return rc;
  ATTWARP_REQUIRE(table, "png_plan: null table");
  const size_t need = attwarp_png_table_bytes_ex(images, B, match);
  ATTWARP_REQUIRE(table_bytes >= need, "png_plan: table of %zu bytes, %zu needed", table_bytes, need);
  uint8_t* t = static_cast<uint8_t*>(table);
  std::memset(t, 0, need);
  attwarp_png_header h;
  std::memset(&h, 0, sizeof h);
  h.magic = PNG_MAGIC;
  h.B = B;
  h.nseg = (int32_t)nseg;
  h.reserved = (int32_t)nlz;                               // LZ segments: the LZ launch's grid (0: no order list, no LZ launch)
  h.table_bytes = need;
  h.off_images = align_up(sizeof(attwarp_png_header), 16);
  h.off_segs = h.off_images + align_up((uint64_t)B * sizeof(PngImageDev), 16);
  uint32_t p = 0x40000000u;                                // x^1
  for (int k = 0; k < 3; ++k) p = crc_mulmod(p, p);        // x^8
  for (int k = 0; k < 32; ++k) { h.crc_pow8[k] = p; p = crc_mulmod(p, p); }
  const uint8_t idat[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
  h.idat_head_crc = crc_bytes(idat, 6);
  PngImageDev* im = reinterpret_cast<PngImageDev*>(t + h.off_images);
  PngSeg* sg = reinterpret_cast<PngSeg*>(t + h.off_segs);
  uint64_t soff = align_up((uint64_t)nseg * sizeof(PngSegOut), 256), out_bytes = 0;
  int32_t s = 0;
  for (int b = 0; b < B; ++b) {
    const attwarp_png_image& d = images[b];
    PngImageDev& r = im[b];
    r.src = d.src; r.H = d.H; r.W = d.W; r.C = d.C; r.pitch = d.pitch;
    r.swap = d.C == 3 && d.order == ATTWARP_BGR;
    r.filter = d.filter;
    r.pad[0] = (uint8_t)(match ? match[b] : ATTWARP_PNG_MATCH_RLE);
    r.row_bytes = 1 + d.W * d.C;
    r.rows_per_seg = png_rows_per_segment(r.row_bytes);
    r.seg0 = s;
    r.nseg = (d.H + r.rows_per_seg - 1) / r.rows_per_seg;
    const uint8_t ihdr[21] = {0, 0, 0, 13, 'I', 'H', 'D', 'R',
                              (uint8_t)(d.W >> 24), (uint8_t)(d.W >> 16), (uint8_t)(d.W >> 8), (uint8_t)d.W,
                              (uint8_t)(d.H >> 24), (uint8_t)(d.H >> 16), (uint8_t)(d.H >> 8), (uint8_t)d.H,
                              8, (uint8_t)(d.C == 1 ? 0 : 2), 0, 0, 0};
    std::memcpy(r.ihdr, ihdr, 21);
    const uint32_t c = crc_bytes(ihdr + 4, 17);
    r.ihdr[21] = (uint8_t)(c >> 24); r.ihdr[22] = (uint8_t)(c >> 16); r.ihdr[23] = (uint8_t)(c >> 8); r.ihdr[24] = (uint8_t)c;
    for (int row0 = 0; row0 < d.H; row0 += r.rows_per_seg, ++s) {
      PngSeg& g = sg[s];
      g.image = b;
      g.row0 = row0;
      g.nrows = std::min(r.rows_per_seg, d.H - row0);
      g.n = g.nrows * r.row_bytes;
      g.scratch_off = soff;
      g.after = (uint64_t)(d.H - row0 - g.nrows) * (uint64_t)r.row_bytes;
      soff += align_up((uint64_t)g.n + 5 + 3, 16);
    }
    out_bytes += png_bound64(d.H, d.W, d.C);
  }
  if (nlz) {                                               // RLE segments first, then LZ, each in segment order
    int32_t* order = reinterpret_cast<int32_t*>(t + h.off_segs + (uint64_t)nseg * sizeof(PngSeg));
    int64_t at[2] = {0, nseg - nlz};
    for (int32_t k = 0; k < (int32_t)nseg; ++k) order[at[im[sg[k].image].pad[0] == ATTWARP_PNG_MATCH_LZ]++] = k;
  }
  h.scratch_bytes = soff;
  h.out_bytes = out_bytes;
  std::memcpy(t, &h, sizeof h);
  return ATTWARP_OK;
}
extern "C" int attwarp_png_plan(const attwarp_png_image* images, int B, void* table, size_t table_bytes) {
  return attwarp_png_plan_ex(images, B, nullptr, table, table_bytes);
}

extern "C" int attwarp_png_encode(const void* table_host, const void* table_dev, void* scratch, uint8_t* out, size_t out_bytes,
                                  int64_t* offsets, void* stream) {
  ATTWARP_REQUIRE(table_host && table_dev && scratch && out && offsets, "png_encode: null pointer");
  attwarp_png_header h;
  std::memcpy(&h, table_host, sizeof h);
  ATTWARP_REQUIRE(h.magic == PNG_MAGIC && h.B > 0 && h.nseg >= h.B && h.nseg <= PNG_MAX_SEGS && h.reserved >= 0 && h.reserved <= h.nseg,
                  "png_encode: not a table of attwarp_png_plan");
  ATTWARP_REQUIRE(out_bytes >= h.out_bytes, "png_encode: out of %zu bytes, %llu needed", out_bytes, (unsigned long long)h.out_bytes);
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(table_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(scratch) % 16 == 0 &&
                      reinterpret_cast<uintptr_t>(offsets) % 8 == 0,
                  "png_encode: table_dev / offsets must be 8-byte, scratch 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const uint8_t* td = static_cast<const uint8_t*>(table_dev);
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  const int nlz = h.reserved, nrle = h.nseg - nlz;
  if (nrle) {
    hipLaunchKernelGGL(png_encode_kernel, dim3(nrle), dim3(PNG_NT), 0, st, td, sc);
    if (const int rc = check_launch("png_encode_kernel")) return rc;
  }
  if (nlz) {                                               // (the token words need more than the default 64 KB of LDS)
    // (the grant is for the dynamic part alone: the runtime adds the kernel's static LDS itself and refuses a sum above the CU's)
    static_assert(PNG_LZ_TOKEN_BYTES + PNG_LZ_STATIC_LDS <= LDS_CU_BYTES, "the LZ kernel's LDS must fit a CU");
    if (const int rc = grant_dynamic_lds(png_encode_lz_kernel, PNG_LZ_TOKEN_BYTES, "png_encode")) return rc;
    hipLaunchKernelGGL(png_encode_lz_kernel, dim3(nlz), dim3(PNG_NT), PNG_LZ_TOKEN_BYTES, st, td, sc);
    if (const int rc = check_launch("png_encode_lz_kernel")) return rc;
  }
  hipLaunchKernelGGL(png_assemble_kernel, dim3(h.B), dim3(PNG_NT), 0, st, td, sc, out, offsets);
  if (const int rc = check_launch("png_assemble_kernel")) return rc;
  hipLaunchKernelGGL(png_gather_kernel, dim3(h.nseg), dim3(PNG_NT), 0, st, td, static_cast<const uint8_t*>(sc), out, offsets);
  return check_launch("png_gather_kernel");
}
