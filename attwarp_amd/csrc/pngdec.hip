// PNG files of a whole ragged batch decoded on the device (include/attwarp.h): the reading half of png.hip.
// The host walks the chunks and packs the IDAT payloads; everything per byte happens here.  Seven launches, none with a
// host-dependent argument:
//   pngdec_scan_kernel      one workgroup per IMAGE: zlib header, the byte positions behind every 00 00 FF FF (the first
//                           ATTWARP_PNGDEC_MAX_UNITS - 1 of them, in order), per-image state zeroed;
//   pngdec_crc_kernel       one workgroup per IDAT chunk (check_crc): sliced CRC-32, combined with crc_xpow8;
//   pngdec_inflate_kernel   pass 0, one workgroup per kept position (a UNIT): lane 0 walks the blocks with pd_inflate and
//                           COUNTS -- output length, where it stopped, whether a match reached back before its first byte;
//   pngdec_chain_kernel     one thread per image: the chain of units from the stream's start, their output offsets, the route;
//   pngdec_inflate_kernel   pass 1: the units on the chain decode again and WRITE at their offsets; slot MAX_UNITS of every
//                           image is the serial route -- one wave from the start -- and exits at once unless the chain failed;
//   pngdec_adler_kernel     one workgroup per image: Adler-32 of the filtered bytes against the stream's;
//   pngdec_unfilter_kernel  one wave per image: 64 rows in flight, skewed by one pixel per lane, so that the row above is one
//                           lane away; reconstructs, converts and writes the pixels, then the image's status.
// A table of attwarp_pngdec_plan_formats with the format flag (palette, 1 / 2 / 4 / 16 bits, Adam7: DESIGN.md 3.18) takes, in
// place of the last launch, pngdec_unfilter_formats_kernel (one wave per image and PASS) and pngdec_status_formats_kernel.
// A table of attwarp_pngdec_plan_wave takes one launch more, between the chain and the write pass:
//   pngdec_wave_kernel      one wave per image of the serial route: all 64 lanes inflate the one stream (pngdec_wave_blocks.hpp);
//                           an image it accepts is skipped by the write pass's serial slot, any other decodes there as ever.
// Every loop is bounded by a constant, by a size the planner checked, or by the stream's bits (pngdec_blocks.hpp).
#include <algorithm>
#include <cstring>

#include "pngfmt_blocks.hpp"
#include "pngdec_wave_blocks.hpp"

namespace attwarp {

#define PD_G __attribute__((address_space(1)))
constexpr uint32_t PD_MAGIC = 0x44474e50u;
constexpr int PD_NT = 256;
constexpr int PD_MAX_B = 1 << 20, PD_MAX_CHUNKS = 1 << 26;

__host__ __device__ inline uint64_t pd_align(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
// the scratch buffer: states, units, kept positions, then every image's filtered bytes (PdImage::filt_off)
__host__ __device__ inline uint64_t pd_units_off(int B) { return pd_align((uint64_t)B * sizeof(PdState), 16); }
__host__ __device__ inline uint64_t pd_kept_off(int B) { return pd_units_off(B) + (uint64_t)B * PD_MAX_UNITS * sizeof(PdUnit); }
__host__ __device__ inline uint64_t pd_filt_base(int B) { return pd_align(pd_kept_off(B) + (uint64_t)B * PD_MAX_UNITS * 4u, 256); }
// a table with the format flag: the format records stand behind the chunks, the palettes behind them
__host__ __device__ inline uint64_t pf_formats_off(const attwarp_pngdec_header& h) {
  return pd_align(h.off_chunks + (uint64_t)h.nchunks * sizeof(attwarp_pngdec_chunk), 16);
}

// a table of attwarp_pngdec_plan_wave: header.reserved2 = 1 | segment_bytes << 8 | max_rounds << 20, and the per-image wave
// records are the last B * sizeof(PwRecord) bytes of the scratch buffer
__host__ __device__ inline uint32_t pw_segment_bytes(uint32_t r2) { return (r2 >> 8) & 0xfffu; }
__host__ __device__ inline uint32_t pw_max_rounds(uint32_t r2) { return (r2 >> 20) & 0xfffu; }
__host__ __device__ inline bool pw_valid(uint32_t sb, uint32_t mr) {
  return (sb == 16 || sb == 32 || sb == 64 || sb == 128 || sb == 256) && mr >= 1 && mr <= (uint32_t)PW_WAVE;
}
__host__ __device__ inline uint64_t pw_records_off(const attwarp_pngdec_header& h) { return h.scratch_bytes - (uint64_t)h.B * sizeof(PwRecord); }

struct PdView {
  const attwarp_pngdec_header* hdr;
  const PdImage* images;
  const attwarp_pngdec_chunk* chunks;
  PdState* states;
  PdUnit* units;
  uint32_t* kept;
  __device__ __forceinline__ PdView(const uint8_t* table, uint8_t* scratch) {
    hdr = reinterpret_cast<const attwarp_pngdec_header*>(table);
    images = reinterpret_cast<const PdImage*>(table + hdr->off_images);
    chunks = reinterpret_cast<const attwarp_pngdec_chunk*>(table + hdr->off_chunks);
    states = reinterpret_cast<PdState*>(scratch);
    units = reinterpret_cast<PdUnit*>(scratch + pd_units_off(hdr->B));
    kept = reinterpret_cast<uint32_t*>(scratch + pd_kept_off(hdr->B));
  }
};

__device__ __forceinline__ uint32_t pd_excl_sum(uint32_t v, uint32_t* tmp, uint32_t& total) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  for (int o = 1; o < PD_NT; o <<= 1) {
    const uint32_t a = t >= o ? tmp[t - o] : 0u;
    __syncthreads();
    tmp[t] += a;
    __syncthreads();
  }
  const uint32_t incl = tmp[t];
  total = tmp[PD_NT - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(PD_NT) void pngdec_scan_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                            uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_tmp[PD_NT];
  const int tid = threadIdx.x, b = blockIdx.x;
  const PdView v(table, scratch);
  const PdImage im = v.images[b];
  const PD_G uint8_t* s = (const PD_G uint8_t*)stream + im.stream_off;
  const uint32_t n = im.stream_len;
  uint32_t* kept = v.kept + (size_t)b * PD_MAX_UNITS;
  const uint32_t zst = pd_zlib_header(stream + im.stream_off, n);
  if (tid == 0) kept[0] = 2;
  uint32_t running = 1;
  constexpr uint32_t PER = 8, TILE = PD_NT * PER;
  // candidate i: bytes i .. i + 3 are 00 00 FF FF and the unit would start at i + 4 < n
  for (uint32_t base = 2; zst == 0 && base + 5u <= n && running < (uint32_t)PD_MAX_UNITS; base += TILE) {
    const uint32_t i0 = base + tid * PER;
    uint64_t lo = 0;
    uint32_t hi = 0;
    if (i0 + 12u <= n) {
      lo = *(const PD_G u32_una*)(s + i0) | (uint64_t)(*(const PD_G u32_una*)(s + i0 + 4)) << 32;
      hi = *(const PD_G u32_una*)(s + i0 + 8);
    } else {
      for (uint32_t k = 0; k < 8; ++k)
        if (i0 + k < n) lo |= (uint64_t)s[i0 + k] << (8 * k);
      for (uint32_t k = 0; k < 4; ++k)
        if (i0 + 8 + k < n) hi |= (uint32_t)s[i0 + 8 + k] << (8 * k);
    }
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
      const uint32_t word = k <= 4 ? (uint32_t)(lo >> (8 * k)) : ((uint32_t)(lo >> (8 * k)) | hi << (64 - 8 * k));
      if (word == 0xffff0000u && i0 + k + 5u <= n) mask |= 1u << k;
    }
    uint32_t total;
    uint32_t at = running + pd_excl_sum((uint32_t)__popc(mask), s_tmp, total);
    for (uint32_t k = 0; k < PER; ++k)
      if ((mask >> k) & 1u) {
        if (at < (uint32_t)PD_MAX_UNITS) kept[at] = i0 + k + 4u;
        ++at;
      }
    running += total;
  }
  if (tid == 0) {
    PdState st;
    st.nunits = zst ? 0u : min(running, (uint32_t)PD_MAX_UNITS);
    st.route = 1;
    st.st_crc = 0; st.st_inflate = zst; st.st_adler = 0; st.st_filter = 0;
    st.adler_pos = 0; st.chain_len = 0;
    v.states[b] = st;
  }
}

// One workgroup per IDAT chunk: one table CRC per lane over equal slices, each shifted to the chunk's end, XORed; then
// "IDAT" in front.
__global__ __launch_bounds__(PD_NT) void pngdec_crc_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                           uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_crc[256], s_pow[32], s_x;
  const int tid = threadIdx.x;
  const PdView v(table, scratch);
  const attwarp_pngdec_chunk ck = v.chunks[blockIdx.x];
  s_crc[tid] = crc_table_entry((uint32_t)tid);
  if (tid < 32) s_pow[tid] = v.hdr->crc_pow8[tid];
  if (tid == 0) s_x = 0;
  __syncthreads();
  const PD_G uint8_t* p = (const PD_G uint8_t*)stream + ck.off;
  const uint32_t len = ck.len, L = (len + PD_NT - 1) / PD_NT;
  const uint32_t b0 = min(len, (uint32_t)tid * L), b1 = min(len, b0 + L);
  uint32_t c = 0xffffffffu;
  for (uint32_t i = b0; i < b1; ++i) c = s_crc[(c ^ p[i]) & 255u] ^ (c >> 8);
  c = ~c;
  if (b0 == b1) c = 0;
  else c = crc_mulmod(c, crc_xpow8(len - b1, s_pow));
  for (int o = WAVE / 2; o > 0; o >>= 1) c ^= __shfl_xor(c, o, WAVE);
  if ((tid & (WAVE - 1)) == 0) atomicXor(&s_x, c);
  __syncthreads();
  if (tid == 0) {
    const uint32_t crc = crc_mulmod(v.hdr->idat_crc, crc_xpow8(len, s_pow)) ^ s_x;
    if (crc != ck.crc) v.states[ck.image].st_crc = ATTWARP_PNGDEC_E_CRC;
  }
}

// grid (B, PD_MAX_UNITS + 1), one wave each; lane 0 runs the inflate core with its tables in LDS.
__global__ __launch_bounds__(WAVE) void pngdec_inflate_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                              uint8_t* __restrict__ scratch, int pass) {
  __shared__ PdTables tb;
  const uint32_t u = blockIdx.y;
  const int b = blockIdx.x;
  const PdView v(table, scratch);
  PdState* st = v.states + b;
  const uint32_t nunits = st->nunits;
  if (threadIdx.x != 0 || nunits == 0) return;
  const PdImage im = v.images[b];
  const uint8_t* s = stream + im.stream_off;
  const uint32_t* kept = v.kept + (size_t)b * PD_MAX_UNITS;
  PdUnit* U = v.units + (size_t)b * PD_MAX_UNITS + u;
  uint8_t* filt = scratch + im.filt_off;
  // one call of the core, so that it is inlined once: where it starts, where it writes and how much, by pass and slot
  uint32_t start, cap, nk = nunits;
  uint8_t* out = nullptr;
  const uint32_t* kp = kept;
  if (pass == 0) {                                         // count (a stream without sync points goes serial at once)
    if (u >= nunits || nunits == 1) return;
    start = kept[u];
    cap = im.filt_bytes;
  } else if (u < (uint32_t)PD_MAX_UNITS) {                 // write
    if (st->route != 0 || u >= nunits || !U->on_chain) return;
    if (U->out_off > im.filt_bytes || U->out_len > im.filt_bytes - U->out_off) return;   // (pd_chain never leaves such a unit)
    start = U->start;
    cap = U->out_len;
    out = filt + U->out_off;
  } else {                                                 // the serial route
    if (st->route != 1) return;
    if (v.hdr->reserved2 && reinterpret_cast<const PwRecord*>(scratch + pw_records_off(*v.hdr))[b].accepted) return;   // (the wave route wrote it)
    start = 2;
    cap = im.filt_bytes;
    out = filt;
    kp = nullptr;
    nk = 0;
  }
  const PdResult r = pd_inflate(s, im.stream_len, start, out, cap, kp, nk, tb);
  if (pass == 0) {
    PdUnit o;
    o.start = start; o.end = r.end; o.out_len = r.out_len; o.out_off = 0;
    o.status = r.status; o.final = r.final; o.dependent = r.dependent; o.on_chain = 0;
    *U = o;
  } else if (u < (uint32_t)PD_MAX_UNITS) {
    if (r.status || r.out_len != U->out_len || r.end != U->end) st->st_inflate = r.status ? r.status : (uint32_t)ATTWARP_PNGDEC_E_UNDERFLOW;
  } else {
    st->st_inflate = pd_serial_status(r, im.filt_bytes, im.stream_len);
    st->adler_pos = r.end;
  }
}

__global__ __launch_bounds__(WAVE) void pngdec_chain_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch, int force_serial) {
  const PdView v(table, scratch);
  const int b = blockIdx.x * WAVE + threadIdx.x;
  if (b >= v.hdr->B) return;
  PdState* st = v.states + b;
  const uint32_t nunits = st->nunits;
  if (nunits == 0) { st->route = 2; return; }              // (the zlib header failed: nothing decodes)
  uint32_t route = 1, adler_pos = 0, chain_len = 0;
  if (nunits > 1 && !force_serial && nunits <= (uint32_t)PD_MAX_UNITS)
    route = pd_chain(v.units + (size_t)b * PD_MAX_UNITS, nunits, v.images[b].filt_bytes, v.images[b].stream_len, adler_pos, chain_len) ? 0u : 1u;
  st->route = route;
  st->adler_pos = adler_pos;
  st->chain_len = route == 0 ? chain_len : 0u;
}

// Grid B, one wave each: the wave route for every image that the chain left to the serial route.  Writes the image's wave
// record; on acceptance the filtered bytes and adler_pos too, and st_inflate stays OK as pd_serial_status would leave it.
__global__ __launch_bounds__(WAVE) void pngdec_wave_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                           uint8_t* __restrict__ scratch) {
  __shared__ PwShared S;
  static_assert(WAVE == PW_WAVE, "one wave per image");
  const int b = blockIdx.x;
  const PdView v(table, scratch);
  PdState* st = v.states + b;
  PwRecord* rec = reinterpret_cast<PwRecord*>(scratch + pw_records_off(*v.hdr)) + b;
  const uint32_t sb = pw_segment_bytes(v.hdr->reserved2), mr = pw_max_rounds(v.hdr->reserved2);
  if (st->route != 1 || st->nunits == 0 || st->st_crc != 0 || !pw_valid(sb, mr)) {   // (uniform; a file with a wrong CRC is not worth a wave)
    if (threadIdx.x == 0) *rec = PwRecord{0, 0, 0, 0};
    return;
  }
  const PdImage im = v.images[b];
  uint8_t* filt = scratch + im.filt_off;
  pw_image(S, stream + im.stream_off, im.stream_len, filt, im.filt_bytes, sb, mr, rec, &st->adler_pos);
  if (!rec->accepted) return;                              // (uniform: written in front of pw_image's last barrier)
  // a filter byte above 4 is the unfilter kernels' to state: such an image, too, takes the lane route as without the wave
  bool badf = false;
  if (v.hdr->formats) {
    const PfImage fm = reinterpret_cast<const PfImage*>(table + pf_formats_off(*v.hdr))[b];
    for (int p = 0; p < PF_PASSES; ++p) {
      const PfPass g = pf_pass(fm.interlace, p, im.W, im.H);
      if (g.w <= 0 || g.h <= 0) continue;
      const uint64_t rb = (uint64_t)pf_row_bytes(g.w, im.ch, fm.depth), off = (uint64_t)pf_pass_offset(fm.interlace, p, im.W, im.H, im.ch, fm.depth);
      for (int r = threadIdx.x; r < g.h; r += WAVE) {
        const uint64_t q = off + (uint64_t)r * rb;
        badf |= q < im.filt_bytes && filt[q] > 4;
      }
    }
  } else {
    for (int r = threadIdx.x; r < im.H; r += WAVE) {
      const uint64_t q = (uint64_t)r * (uint64_t)im.row_bytes;
      badf |= q < im.filt_bytes && filt[q] > 4;
    }
  }
  if (__ballot(badf) != 0ull && threadIdx.x == 0) rec->accepted = 0;
}

__global__ __launch_bounds__(PD_NT) void pngdec_adler_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                             uint8_t* __restrict__ scratch) {
  __shared__ unsigned long long s_a, s_b;
  const int tid = threadIdx.x, b = blockIdx.x;
  const PdView v(table, scratch);
  PdState* st = v.states + b;
  if (st->nunits == 0 || st->st_inflate != 0) return;      // (uniform)
  const PdImage im = v.images[b];
  const uint32_t N = im.filt_bytes;
  const PD_G uint8_t* f = (const PD_G uint8_t*)scratch + im.filt_off;
  if (tid == 0) { s_a = 0; s_b = 0; }
  __syncthreads();
  // a thread sums at most N / 256 + 16 bytes: S2 stays below 2^23 * 255 * 2^31 < 2^63
  unsigned long long a = 0, w = 0;
  for (uint32_t i = (uint32_t)tid * 16u; i < N; i += PD_NT * 16u) {
    if (i + 16u <= N) {
      const PD_G uint32_t* q = (const PD_G uint32_t*)(f + i);   // (filt_off is 16-byte aligned)
      const uint32_t d[4] = {q[0], q[1], q[2], q[3]};
#pragma unroll
      for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t x = (d[k >> 2] >> (8 * (k & 3))) & 255u;
        a += x;
        w += (unsigned long long)x * (N - i - k);
      }
    } else {
      for (uint32_t k = 0; i + k < N; ++k) {
        const uint32_t x = f[i + k];
        a += x;
        w += (unsigned long long)x * (N - i - k);
      }
    }
  }
  a %= PNG_ADLER;
  w %= PNG_ADLER;
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, WAVE);
    w += __shfl_xor(w, o, WAVE);
  }
  if ((tid & (WAVE - 1)) == 0) { atomicAdd(&s_a, a); atomicAdd(&s_b, w); }
  __syncthreads();
  if (tid == 0) {
    const uint32_t pos = st->adler_pos;
    uint32_t want = 0;
    const bool inside = pos <= im.stream_len && im.stream_len - pos >= 4u;   // (pd_chain / pd_serial_status checked it)
    if (inside) want = pd_be32(stream + im.stream_off + pos);
    if (!inside || want != pd_adler_finish(s_a, s_b, N)) st->st_adler = ATTWARP_PNGDEC_E_ADLER;
  }
}

// One wave per image.  Lane l reconstructs row r0 + l; at step s it stands on pixel s - l, so the pixel above it is what
// lane l - 1 reconstructed one step earlier (one shuffle of the packed pixel) and the one up-left what it received the step
// before.  Lane 0 reads the row above from LDS, where lane 63 of the previous 64 rows left it.
__global__ __launch_bounds__(WAVE) void pngdec_unfilter_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch,
                                                               uint8_t* __restrict__ out, int32_t* __restrict__ status) {
  extern __shared__ uint8_t s_carry[];
  const int lane = threadIdx.x, b = blockIdx.x;
  const PdView v(table, scratch);
  PdState* st = v.states + b;
  uint32_t stat = st->st_crc ? st->st_crc : st->st_inflate ? st->st_inflate : st->st_adler;
  if (stat == 0) {
    const PdImage im = v.images[b];
    const int H = im.H, W = im.W, ch = im.ch, oc = im.oc, RB = im.row_bytes;
    const bool swap = im.swap != 0;
    const PD_G uint8_t* filt = (const PD_G uint8_t*)scratch + im.filt_off;
    PD_G uint8_t* o = (PD_G uint8_t*)out + im.out_off;
    for (int r0 = 0; r0 < H; r0 += WAVE) {
      const int r = r0 + lane;
      const bool active = r < H;
      const PD_G uint8_t* frow = filt + (size_t)(active ? r : r0) * RB;
      const int ft = frow[0];
      if (__ballot(active && ft > 4) != 0ull) { stat = ATTWARP_PNGDEC_E_FILTER; break; }
      const int rows = min(WAVE, H - r0), steps = W + rows - 1;
      const bool keep = r0 + WAVE < H;                     // a later batch needs this one's last row
      uint32_t cur = 0, up = 0, upleft = 0;
      for (int s = 0; s < steps; ++s) {
        const int x = s - lane;
        const bool on = active && x >= 0 && x < W;
        const uint32_t above = __shfl_up(cur, 1, WAVE);
        upleft = up;
        up = above;
        if (lane == 0) {
          up = 0;
          if (r0 > 0 && on)
            for (int k = 0; k < ch; ++k) up |= (uint32_t)s_carry[x * ch + k] << (8 * k);
        }
        if (on) {
          const uint32_t left = cur;
          uint32_t px = 0;
          for (int k = 0; k < ch; ++k) {
            const uint32_t f = frow[1 + x * ch + k];
            px |= pd_recon(ft, f, (left >> (8 * k)) & 255u, (up >> (8 * k)) & 255u, (upleft >> (8 * k)) & 255u) << (8 * k);
          }
          cur = px;
          if (keep && lane == WAVE - 1)
            for (int k = 0; k < ch; ++k) s_carry[x * ch + k] = (uint8_t)(px >> (8 * k));
          const uint32_t p0 = px & 255u, p1 = (px >> 8) & 255u, p2 = (px >> 16) & 255u;
          PD_G uint8_t* d = o + ((size_t)r * W + x) * oc;
          if (oc == 1) {
            d[0] = (uint8_t)(ch <= 2 ? p0 : pd_luma(p0, p1, p2));
          } else if (ch <= 2) {
            d[0] = (uint8_t)p0; d[1] = (uint8_t)p0; d[2] = (uint8_t)p0;
          } else {
            d[0] = (uint8_t)(swap ? p2 : p0); d[1] = (uint8_t)p1; d[2] = (uint8_t)(swap ? p0 : p2);
          }
        }
      }
    }
    if (stat && lane == 0) st->st_filter = stat;
  }
  if (lane == 0) status[b] = (int32_t)stat;
}

// The same skewed scheme for every format of the specification.  Grid (B, 7), one wave per (image, pass):
// the passes of an interlaced image are filtered on their own, so they are independent once inflated; a non-interlaced
// image is its slot 0 and the other slots exit.  Lane l reconstructs row r0 + l of the PASS, one filter unit of 1 .. 8 bytes
// per step (packed into 64 bits), and scatters the converted pixels to ((y0 + r dy) W + x0 + x dx) oc; a unit below 8 bits
// holds up to 8 pixels, clipped at the pass's width.  LDS: the converted palette (1 KiB), then lane 63's row.
// A bad filter byte raises st_filter with an atomic max; pngdec_status_formats_kernel then states the image's status.
__global__ __launch_bounds__(WAVE) void pngdec_unfilter_formats_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch,
                                                                       uint8_t* __restrict__ out) {
  extern __shared__ uint8_t s_dyn[];
  uint32_t* s_pal = reinterpret_cast<uint32_t*>(s_dyn);
  uint8_t* s_carry = s_dyn + PF_PALETTE_LDS;
  const int lane = threadIdx.x, b = blockIdx.x, p = blockIdx.y;
  const PdView v(table, scratch);
  PdState* st = v.states + b;
  if (st->st_crc || st->st_inflate || st->st_adler) return;   // (uniform)
  const PdImage im = v.images[b];
  const PfImage fm = reinterpret_cast<const PfImage*>(table + pf_formats_off(*v.hdr))[b];
  const int W = im.W, ch = im.ch, oc = im.oc, depth = fm.depth, ctype = fm.ctype;
  const PfPass g = pf_pass(fm.interlace, p, W, im.H);
  if (g.w <= 0 || g.h <= 0) return;                         // (uniform)
  const bool swap = im.swap != 0;
  if (ctype == 3) {
    const uint8_t* pal = table + fm.pal_off;
    for (int i = lane; i < 256; i += WAVE) s_pal[i] = pf_palette_entry(pal, i, oc, swap);
    __syncthreads();
  }
  const int unit = pf_unit(ch, depth), ppu = pf_unit_pixels(depth);
  const int RB = (int)pf_row_bytes(g.w, ch, depth), nu = (RB - 1) / unit;
  const PD_G uint8_t* filt = (const PD_G uint8_t*)scratch + im.filt_off + pf_pass_offset(fm.interlace, p, W, im.H, ch, depth);
  PD_G uint8_t* o = (PD_G uint8_t*)out + im.out_off;
  for (int r0 = 0; r0 < g.h; r0 += WAVE) {
    const int r = r0 + lane;
    const bool active = r < g.h;
    const PD_G uint8_t* frow = filt + (size_t)(active ? r : r0) * RB;
    const int ft = frow[0];
    if (__ballot(active && ft > 4) != 0ull) {
      if (lane == 0) atomicMax(&st->st_filter, (uint32_t)ATTWARP_PNGDEC_E_FILTER);
      return;
    }
    const int rows = min(WAVE, g.h - r0), steps = nu + rows - 1;
    const bool keep = r0 + WAVE < g.h;                      // a later batch needs this one's last row
    const size_t orow = ((size_t)(g.y0 + r * g.dy) * W + g.x0) * oc;
    uint64_t cur = 0, up = 0, upleft = 0;
    for (int s = 0; s < steps; ++s) {
      const int x = s - lane;
      const bool on = active && x >= 0 && x < nu;
      const uint32_t alo = __shfl_up((uint32_t)cur, 1, WAVE), ahi = __shfl_up((uint32_t)(cur >> 32), 1, WAVE);
      upleft = up;
      up = (uint64_t)ahi << 32 | alo;
      if (lane == 0) {
        up = 0;
        if (r0 > 0 && on)
          for (int k = 0; k < unit; ++k) up |= (uint64_t)s_carry[x * unit + k] << (8 * k);
      }
      if (on) {
        const uint64_t left = cur;
        uint64_t px = 0;
        for (int k = 0; k < unit; ++k) {
          const uint32_t f = frow[1 + x * unit + k];
          px |= (uint64_t)pd_recon(ft, f, (int)((left >> (8 * k)) & 255u), (int)((up >> (8 * k)) & 255u), (int)((upleft >> (8 * k)) & 255u)) << (8 * k);
        }
        cur = px;
        if (keep && lane == WAVE - 1)
          for (int k = 0; k < unit; ++k) s_carry[x * unit + k] = (uint8_t)(px >> (8 * k));
        const int n = min(ppu, g.w - x * ppu);              // pixels of this unit inside the pass
        for (int j = 0; j < n; ++j) {
          const uint32_t q = pf_output(ctype, pf_pixel(ctype, depth, px, j), oc, swap, s_pal);
          PD_G uint8_t* d = o + orow + (size_t)(x * ppu + j) * g.dx * oc;
          d[0] = (uint8_t)q;
          if (oc == 3) { d[1] = (uint8_t)(q >> 8); d[2] = (uint8_t)(q >> 16); }
        }
      }
    }
  }
}

// One thread per image: the first failing check in the order CRC, inflate, Adler, filter, as pngdec_unfilter_kernel states it.
__global__ __launch_bounds__(WAVE) void pngdec_status_formats_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ scratch,
                                                                     int32_t* __restrict__ status) {
  const attwarp_pngdec_header* hdr = reinterpret_cast<const attwarp_pngdec_header*>(table);
  const int b = blockIdx.x * WAVE + threadIdx.x;
  if (b >= hdr->B) return;
  const PdState st = reinterpret_cast<const PdState*>(scratch)[b];
  status[b] = (int32_t)(st.st_crc ? st.st_crc : st.st_inflate ? st.st_inflate : st.st_adler ? st.st_adler : st.st_filter);
}

}  // namespace attwarp

using namespace attwarp;

// formats == nullptr: the 8-bit, non-interlaced records of attwarp_pngdec_plan
static int pngdec_check(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B, const attwarp_pngdec_chunk* chunks,
                        int nchunks) {
  ATTWARP_REQUIRE(images, "pngdec: null image array");
  ATTWARP_REQUIRE(B > 0, "pngdec: non-positive batch size");
  ATTWARP_REQUIRE(nchunks >= 0 && (nchunks == 0 || chunks), "pngdec: null chunk array");
  if (B > PD_MAX_B) return fail(ATTWARP_E_UNSUPPORTED, "pngdec: B=%d > 2^20", B);
  if (nchunks > PD_MAX_CHUNKS) return fail(ATTWARP_E_UNSUPPORTED, "pngdec: %d IDAT chunks > 2^26", nchunks);
  for (int b = 0; b < B; ++b) {
    const attwarp_pngdec_image& d = images[b];
    ATTWARP_REQUIRE(d.H >= 1 && d.W >= 1, "pngdec: image %d: non-positive size %d x %d", b, d.H, d.W);
    int depth = 8, lace = 0;
    if (formats) {
      const attwarp_pngdec_format& f = formats[b];
      depth = f.depth;
      lace = f.interlace;
      ATTWARP_REQUIRE(pf_valid(depth, d.color_type), "pngdec: image %d: bit depth %d with colour type %d", b, depth, d.color_type);
      ATTWARP_REQUIRE(lace == 0 || lace == 1, "pngdec: image %d: interlace method %d (0 or 1)", b, lace);
      ATTWARP_REQUIRE(d.color_type == 3 ? f.palette_entries >= 1 && f.palette_entries <= 256 : f.palette_entries >= 0 && f.palette_entries <= 256,
                      "pngdec: image %d: a PLTE of %d entries", b, f.palette_entries);
    } else {
      ATTWARP_REQUIRE(d.color_type == 0 || d.color_type == 2 || d.color_type == 4 || d.color_type == 6,
                      "pngdec: image %d: colour type %d (0, 2, 4 or 6)", b, d.color_type);
    }
    ATTWARP_REQUIRE(d.mode >= ATTWARP_PNGDEC_RGB && d.mode <= ATTWARP_PNGDEC_KEEP, "pngdec: image %d: unknown mode %d", b, d.mode);
    ATTWARP_REQUIRE(d.order == ATTWARP_RGB || d.order == ATTWARP_BGR, "pngdec: image %d: channel order must be ATTWARP_RGB or ATTWARP_BGR", b);
    const int ch = pf_channels(d.color_type);
    const int64_t rb = pf_row_bytes(d.W, ch, depth);
    if (rb > ATTWARP_PNGDEC_MAX_ROW_BYTES)
      return fail(ATTWARP_E_UNSUPPORTED, "pngdec: image %d: row of %lld bytes (> %d)", b, (long long)rb, ATTWARP_PNGDEC_MAX_ROW_BYTES);
    if (pf_pass_offset(lace, PF_PASSES, d.W, d.H, ch, depth) >= ((int64_t)1 << 31))
      return fail(ATTWARP_E_UNSUPPORTED, "pngdec: image %d: %d x %d x %lld is 2 GiB or more", b, d.H, d.W, (long long)ch);
    if (d.stream_len >= ((uint64_t)1 << 31) || d.stream_off >= ((uint64_t)1 << 62))
      return fail(ATTWARP_E_UNSUPPORTED, "pngdec: image %d: a zlib stream of 2 GiB or more", b);
  }
  for (int c = 0; c < nchunks; ++c) {
    const attwarp_pngdec_chunk& k = chunks[c];
    ATTWARP_REQUIRE(k.image >= 0 && k.image < B, "pngdec: chunk %d: image %d outside the batch", c, k.image);
    const attwarp_pngdec_image& d = images[k.image];
    ATTWARP_REQUIRE(k.off >= d.stream_off && k.off - d.stream_off <= d.stream_len && k.len <= d.stream_len - (k.off - d.stream_off),
                    "pngdec: chunk %d lies outside the stream of image %d", c, k.image);
  }
  return ATTWARP_OK;
}

// the format flag: at least one image that pngdec_unfilter_kernel does not decode
static bool pngdec_needs_formats(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B) {
  if (!formats) return false;
  for (int b = 0; b < B; ++b)
    if (!pf_plain(formats[b].depth, images[b].color_type, formats[b].interlace)) return true;
  return false;
}

static size_t pngdec_bytes(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B, int nchunks) {
  uint64_t n = pd_align(sizeof(attwarp_pngdec_header), 16) + pd_align((uint64_t)B * sizeof(PdImage), 16) +
               (uint64_t)nchunks * sizeof(attwarp_pngdec_chunk);
  if (pngdec_needs_formats(images, formats, B)) {
    n = pd_align(n, 16) + (uint64_t)B * sizeof(PfImage);
    for (int b = 0; b < B; ++b)
      if (images[b].color_type == 3) n += 768;
  }
  return (size_t)n;
}

static bool pngdec_bytes_args(const void* images, int B, int nchunks) {
  if (images && B > 0 && B <= PD_MAX_B && nchunks >= 0 && nchunks <= PD_MAX_CHUNKS) return true;
  fail(ATTWARP_E_ARG, "pngdec_table_bytes: B=%d, nchunks=%d outside the limits", B, nchunks);
  return false;
}

extern "C" size_t attwarp_pngdec_table_bytes(const attwarp_pngdec_image* images, int B, int nchunks) {
  return pngdec_bytes_args(images, B, nchunks) ? pngdec_bytes(images, nullptr, B, nchunks) : 0;
}

extern "C" size_t attwarp_pngdec_table_bytes_formats(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B,
                                                     const attwarp_pngdec_chunk* chunks, int nchunks) {
  (void)chunks;
  if (!pngdec_bytes_args(images, B, nchunks)) return 0;
  if (!formats) { fail(ATTWARP_E_ARG, "pngdec_table_bytes_formats: null format array"); return 0; }
  return pngdec_bytes(images, formats, B, nchunks);
}

// wave != 0: the table of attwarp_pngdec_plan_wave (segment_bytes, max_rounds checked by the caller)
static int pngdec_plan(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B, const attwarp_pngdec_chunk* chunks,
                       int nchunks, int check_crc, void* table, size_t table_bytes, uint32_t wave = 0) {
  if (const int rc = pngdec_check(images, formats, B, chunks, nchunks)) return rc;
  ATTWARP_REQUIRE(table, "pngdec_plan: null table");
  const bool fmt = pngdec_needs_formats(images, formats, B);
  const size_t need = pngdec_bytes(images, formats, B, nchunks);
  ATTWARP_REQUIRE(table_bytes >= need, "pngdec_plan: table of %zu bytes, %zu needed", table_bytes, need);
  uint8_t* t = static_cast<uint8_t*>(table);
  std::memset(t, 0, need);
  attwarp_pngdec_header h;
  std::memset(&h, 0, sizeof h);
  h.magic = PD_MAGIC;
  h.B = B;
  h.nchunks = nchunks;
  h.check_crc = check_crc != 0;
  h.formats = fmt ? 1 : 0;
  h.table_bytes = need;
  h.off_images = pd_align(sizeof(attwarp_pngdec_header), 16);
  h.off_chunks = h.off_images + pd_align((uint64_t)B * sizeof(PdImage), 16);
  uint32_t p = 0x40000000u;                                // x^1
  for (int k = 0; k < 3; ++k) p = crc_mulmod(p, p);        // x^8
  for (int k = 0; k < 32; ++k) { h.crc_pow8[k] = p; p = crc_mulmod(p, p); }
  const uint8_t idat[4] = {'I', 'D', 'A', 'T'};
  h.idat_crc = crc_bytes(idat, 4);
  PdImage* im = reinterpret_cast<PdImage*>(t + h.off_images);
  PfImage* fm = fmt ? reinterpret_cast<PfImage*>(t + pf_formats_off(h)) : nullptr;
  uint64_t soff = pd_filt_base(B), ooff = 0, stream_bytes = 0, poff = fmt ? pf_formats_off(h) + (uint64_t)B * sizeof(PfImage) : 0;
  int lds = 16;
  for (int b = 0; b < B; ++b) {
    const attwarp_pngdec_image& d = images[b];
    const int depth = formats ? formats[b].depth : 8, lace = formats ? formats[b].interlace : 0;
    PdImage& r = im[b];
    r.ch = pf_channels(d.color_type);
    r.oc = pf_out_channels(d.color_type, d.mode);
    r.H = d.H; r.W = d.W;
    r.swap = r.oc == 3 && (r.ch >= 3 || d.color_type == 3) && d.order == ATTWARP_BGR;
    r.row_bytes = (int32_t)pf_row_bytes(d.W, r.ch, depth);
    r.stream_off = d.stream_off;
    r.stream_len = (uint32_t)d.stream_len;
    r.filt_bytes = (uint32_t)pf_pass_offset(lace, PF_PASSES, d.W, d.H, r.ch, depth);
    r.filt_off = soff;
    r.out_off = ooff;
    soff += pd_align(r.filt_bytes, 16);
    ooff += (uint64_t)d.H * d.W * r.oc;
    stream_bytes = std::max(stream_bytes, d.stream_off + d.stream_len);
    lds = std::max(lds, (int)pd_align((uint64_t)r.row_bytes - 1, 16));
    if (fmt) {
      PfImage& f = fm[b];
      f.depth = depth; f.ctype = d.color_type; f.interlace = lace; f.pal_off = 0;
      if (d.color_type == 3) {                             // padded with zeros: an index past the entries is black
        f.pal_off = (uint32_t)poff;
        std::memcpy(t + poff, formats[b].palette, (size_t)formats[b].palette_entries * 3);
        poff += 768;
      }
    }
  }
  if (nchunks) std::memcpy(t + h.off_chunks, chunks, (size_t)nchunks * sizeof(attwarp_pngdec_chunk));
  h.scratch_bytes = soff + (wave ? (uint64_t)B * sizeof(PwRecord) : 0);   // (soff is a multiple of 16)
  h.reserved2 = wave;
  h.out_bytes = ooff;
  h.stream_bytes = stream_bytes;
  h.lds_bytes = lds + (fmt ? PF_PALETTE_LDS : 0);
  std::memcpy(t, &h, sizeof h);
  return ATTWARP_OK;
}

extern "C" int attwarp_pngdec_plan(const attwarp_pngdec_image* images, int B, const attwarp_pngdec_chunk* chunks, int nchunks,
                                   int check_crc, void* table, size_t table_bytes) {
  return pngdec_plan(images, nullptr, B, chunks, nchunks, check_crc, table, table_bytes);
}

extern "C" int attwarp_pngdec_plan_formats(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B,
                                           const attwarp_pngdec_chunk* chunks, int nchunks, int check_crc, void* table, size_t table_bytes) {
  ATTWARP_REQUIRE(formats, "pngdec_plan_formats: null format array");
  return pngdec_plan(images, formats, B, chunks, nchunks, check_crc, table, table_bytes);
}

extern "C" size_t attwarp_pngdec_table_bytes_wave(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B,
                                                  const attwarp_pngdec_chunk* chunks, int nchunks) {
  (void)chunks;
  return pngdec_bytes_args(images, B, nchunks) ? pngdec_bytes(images, formats, B, nchunks) : 0;
}

extern "C" int attwarp_pngdec_plan_wave(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B,
                                        const attwarp_pngdec_chunk* chunks, int nchunks, int check_crc, int segment_bytes, int max_rounds,
                                        void* table, size_t table_bytes) {
  ATTWARP_REQUIRE(segment_bytes > 0 && max_rounds > 0 && pw_valid((uint32_t)segment_bytes, (uint32_t)max_rounds),
                  "pngdec_plan_wave: segment_bytes=%d (16, 32, 64, 128 or 256), max_rounds=%d (1 .. 64)", segment_bytes, max_rounds);
  return pngdec_plan(images, formats, B, chunks, nchunks, check_crc, table, table_bytes,
                     1u | (uint32_t)segment_bytes << 8 | (uint32_t)max_rounds << 20);
}

extern "C" int attwarp_pngdec_decode(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                                     uint8_t* out, size_t out_bytes, int32_t* status, void* stream) {
  ATTWARP_REQUIRE(table_host && table_dev && stream_bytes && scratch && out && status, "pngdec_decode: null pointer");
  attwarp_pngdec_header h;
  std::memcpy(&h, table_host, sizeof h);
  ATTWARP_REQUIRE(h.magic == PD_MAGIC && h.B > 0 && h.B <= PD_MAX_B && h.nchunks >= 0 && h.nchunks <= PD_MAX_CHUNKS &&
                      (h.formats == 0 || h.formats == 1) && h.lds_bytes >= 16 + h.formats * PF_PALETTE_LDS &&
                      h.lds_bytes <= ATTWARP_PNGDEC_MAX_ROW_BYTES + h.formats * PF_PALETTE_LDS &&
                      (h.reserved2 == 0 || ((h.reserved2 & 0xffu) == 1u && pw_valid(pw_segment_bytes(h.reserved2), pw_max_rounds(h.reserved2)) &&
                                            h.scratch_bytes >= (uint64_t)h.B * sizeof(PwRecord))),
                  "pngdec_decode: not a table of attwarp_pngdec_plan");
  ATTWARP_REQUIRE(out_bytes >= h.out_bytes, "pngdec_decode: out of %zu bytes, %llu needed", out_bytes, (unsigned long long)h.out_bytes);
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(table_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(scratch) % 16 == 0 &&
                      reinterpret_cast<uintptr_t>(status) % 4 == 0,
                  "pngdec_decode: table_dev must be 8-byte, scratch 16-byte, status 4-byte aligned");
  hipStream_t st = as_stream(stream);
  const uint8_t* td = static_cast<const uint8_t*>(table_dev);
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  const int force_serial = tune(TUNE_PNGDEC_ROUTE) == 1;
  hipLaunchKernelGGL(pngdec_scan_kernel, dim3(h.B), dim3(PD_NT), 0, st, td, stream_bytes, sc);
  if (const int rc = check_launch("pngdec_scan_kernel")) return rc;
  if (h.check_crc && h.nchunks > 0) {
    hipLaunchKernelGGL(pngdec_crc_kernel, dim3(h.nchunks), dim3(PD_NT), 0, st, td, stream_bytes, sc);
    if (const int rc = check_launch("pngdec_crc_kernel")) return rc;
  }
  const dim3 ugrid(h.B, PD_MAX_UNITS + 1);
  hipLaunchKernelGGL(pngdec_inflate_kernel, ugrid, dim3(WAVE), 0, st, td, stream_bytes, sc, 0);
  if (const int rc = check_launch("pngdec_inflate_kernel (count)")) return rc;
  hipLaunchKernelGGL(pngdec_chain_kernel, dim3((h.B + WAVE - 1) / WAVE), dim3(WAVE), 0, st, td, sc, force_serial);
  if (const int rc = check_launch("pngdec_chain_kernel")) return rc;
  if (h.reserved2) {
    hipLaunchKernelGGL(pngdec_wave_kernel, dim3(h.B), dim3(WAVE), 0, st, td, stream_bytes, sc);
    if (const int rc = check_launch("pngdec_wave_kernel")) return rc;
  }
  hipLaunchKernelGGL(pngdec_inflate_kernel, ugrid, dim3(WAVE), 0, st, td, stream_bytes, sc, 1);
  if (const int rc = check_launch("pngdec_inflate_kernel (write)")) return rc;
  hipLaunchKernelGGL(pngdec_adler_kernel, dim3(h.B), dim3(PD_NT), 0, st, td, stream_bytes, sc);
  if (const int rc = check_launch("pngdec_adler_kernel")) return rc;
  if (!h.formats) {
    hipLaunchKernelGGL(pngdec_unfilter_kernel, dim3(h.B), dim3(WAVE), (size_t)h.lds_bytes, st, td, sc, out, status);
    return check_launch("pngdec_unfilter_kernel");
  }
  hipLaunchKernelGGL(pngdec_unfilter_formats_kernel, dim3(h.B, PF_PASSES), dim3(WAVE), (size_t)h.lds_bytes, st, td, sc, out);
  if (const int rc = check_launch("pngdec_unfilter_formats_kernel")) return rc;
  hipLaunchKernelGGL(pngdec_status_formats_kernel, dim3((h.B + WAVE - 1) / WAVE), dim3(WAVE), 0, st, td, sc, status);
  return check_launch("pngdec_status_formats_kernel");
}
