// Baseline JPEG files of a whole ragged batch decoded on the device (include/attwarp.h).  The host walks
// the marker segments and packs everything behind each SOS header; everything per byte happens here.  Five launches,
// none with a host-dependent argument:
//   jpegdec_scan_kernel     one workgroup per IMAGE: the FF D0..D7 positions in order (the k-th starts unit k + 1), the
//                           data's end (the first other marker), whether that marker is EOI; E_RESTART unless the markers
//                           number units - 1 with indices cycling 0..7;
//   jpegdec_substream_kernel one workgroup per marker-less IMAGE planned for it: the unit is cut into byte segments, every lane
//                           decodes segments from guessed states until every segment enters where the one before it
//                           leaves (jd_decode_segment, Jacobi rounds under a cap), then the blocks are written with their
//                           true indices and DC predictors; an image it accepts is flagged and skipped by the next kernel;
//   jpegdec_entropy_kernel  one wave per UNIT (restart interval): the wave builds the image's decode tables in LDS and
//                           keeps a ring of the unit's bytes filled; lane 0 decodes block after block with the shared core
//                           (jpegdec_blocks.hpp); the wave stores each block as one 128-byte row of int16[64];
//   jpegdec_idct_kernel     one THREAD per 8x8 block: dequantise, both IDCT passes in registers, eight 8-byte stores into the
//                           component's padded uint8 plane;
//   jpegdec_color_kernel    one thread per output pixel (eight pixels, a workgroup apart): chroma up-sampling, YCbCr -> RGB,
//                           mode and order, the store; the first thread of every image writes its status.
// Every loop is bounded by a header-derived count (units, MCUs per unit, blocks per MCU), by 64 coefficients or 16 bits,
// by the stream's length, or by the plan's cap on rounds.
#include <algorithm>
#include <cstring>

#include "jpegdec_blocks.hpp"

namespace attwarp {

#define JD_G __attribute__((address_space(1)))
constexpr uint32_t JD_MAGIC = 0x4745504au;
constexpr int JD_NT = 256;
constexpr int JD_MAX_B = 1 << 20, JD_MAX_TOTAL_UNITS = 1 << 30;
constexpr int JD_RING = 2048, JD_CHUNK = WAVE * 4;        // bytes of the entropy kernel's ring / loaded per step
constexpr int JD_IDCT_TILE = JD_NT;                       // blocks per workgroup
constexpr int JD_CPX = 8, JD_COLOR_TILE = JD_NT * JD_CPX;  // pixels per thread / workgroup
constexpr int JD_SUB_MAX_SEGS = 1 << 14, JD_SUB_MAX_ROUNDS = 1 << 16;
constexpr int JD_SUB_BLK = 66;                            // int16 per lane's block in LDS: 33 dwords, so lanes spread over the banks

struct JdSub {                         // behind the image records of a table, one per image
  uint64_t seg_off;                    // the image's JdSegState[nseg], then JdSegment[nseg], in the scratch buffer
  uint64_t info_off;                   // JdSubInfo[B] in the scratch buffer (the same in every record)
  uint32_t nseg;                       // planned segments; 0: the image is decoded sequentially
  uint32_t segment_bytes, max_rounds;
  int32_t image;                       // record w: the image that workgroup w of the sub-stream launch decodes
};
static_assert(sizeof(JdSub) == 32, "record layout");
struct JdSubInfo {                     // per image (scratch), written on every run
  uint32_t nseg, rounds, accepted, pad;
};
struct JdSegState {                    // per segment (scratch)
  JdSync entry;
  uint32_t dirty;                      // the entry changed in the last round
  uint32_t before;                     // blocks that start in front of the segment
  uint32_t pred[3];                    // the DC predictors at its start
  uint32_t pad;
};
static_assert(sizeof(JdSegState) == 32, "segment layout");

__host__ __device__ inline uint64_t jd_align(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
// the scratch buffer: states, unit starts, unit ends, then every image's coefficients and planes (JdImage::coef_off, plane_off)
__host__ __device__ inline uint64_t jd_starts_off(int B) { return jd_align((uint64_t)B * sizeof(JdState), 16); }
__host__ __device__ inline uint64_t jd_ends_off(int B, int units) { return jd_starts_off(B) + (uint64_t)units * 4u; }
__host__ __device__ inline uint64_t jd_data_base(int B, int units) { return jd_align(jd_ends_off(B, units) + (uint64_t)units * 4u, 256); }

struct JdView {
  const attwarp_jpegdec_header* hdr;
  const JdImage* images;
  const JdSub* subs;
  JdSubInfo* infos;
  JdState* states;
  uint32_t *starts, *ends;
  __device__ __forceinline__ JdView(const uint8_t* table, uint8_t* scratch) {
    hdr = reinterpret_cast<const attwarp_jpegdec_header*>(table);
    images = reinterpret_cast<const JdImage*>(table + hdr->off_images);
    subs = reinterpret_cast<const JdSub*>(table + hdr->off_images + (uint64_t)hdr->B * sizeof(JdImage));
    infos = reinterpret_cast<JdSubInfo*>(scratch + subs[0].info_off);
    states = reinterpret_cast<JdState*>(scratch);
    starts = reinterpret_cast<uint32_t*>(scratch + jd_starts_off(hdr->B));
    ends = reinterpret_cast<uint32_t*>(scratch + jd_ends_off(hdr->B, hdr->total_units));
  }
  // the image whose range of units / tiles holds t: the last one whose first is <= t (the firsts ascend strictly)
  __device__ __forceinline__ int find(int32_t JdImage::*first, int t) const {
    int lo = 0, hi = hdr->B - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const int mid = (lo + hi + 1) >> 1;
      if (images[mid].*first <= t) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  }
};

__device__ __forceinline__ uint32_t jd_excl_sum(uint32_t v, uint32_t* tmp, uint32_t& total) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  for (int o = 1; o < JD_NT; o <<= 1) {
    const uint32_t a = t >= o ? tmp[t - o] : 0u;
    __syncthreads();
    tmp[t] += a;
    __syncthreads();
  }
  const uint32_t incl = tmp[t];
  total = tmp[JD_NT - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(JD_NT) void jpegdec_scan_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                             uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_tmp[JD_NT], s_term, s_bad;
  const int tid = threadIdx.x, b = blockIdx.x;
  const JdView v(table, scratch);
  const JdImage* im = v.images + b;
  const JD_G uint8_t* s = (const JD_G uint8_t*)stream + im->stream_off;
  const uint32_t n = im->stream_len, nunits = (uint32_t)im->nunits;
  uint32_t* starts = v.starts + im->unit0;
  uint32_t* ends = v.ends + im->unit0;
  if (tid == 0) { s_term = 0xffffffffu; s_bad = 0; starts[0] = 0; }
  __syncthreads();
  uint32_t running = 0, term = n;
  constexpr uint32_t PER = 8, TILE = JD_NT * PER;
  for (uint32_t base = 0; base < n; base += TILE) {
    const uint32_t i0 = base + tid * PER;
    uint32_t by[PER + 1];
#pragma unroll
    for (uint32_t k = 0; k <= PER; ++k) by[k] = i0 + k < n ? (uint32_t)s[i0 + k] : 0x100u;   // 0x100: behind the end
    uint32_t mask = 0, mine = 0xffffffffu;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
      if (by[k] != 0xffu || by[k + 1] == 0u) continue;
      if (by[k + 1] >= 0xd0u && by[k + 1] <= 0xd7u) mask |= 1u << k;
      else if (mine == 0xffffffffu) mine = i0 + k;            // another marker, a fill byte or the last byte: the data ends
    }
    if (mine != 0xffffffffu) atomicMin(&s_term, mine);
    __syncthreads();
    const uint32_t T = s_term;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k)
      if (i0 + k >= T) mask &= ~(1u << k);
    uint32_t total;
    uint32_t at = running + jd_excl_sum((uint32_t)__popc(mask), s_tmp, total);
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k)
      if ((mask >> k) & 1u) {
        if (at + 1u < nunits) {
          ends[at] = i0 + k;
          starts[at + 1u] = i0 + k + 2u;
        }
        if ((by[k + 1] & 7u) != (at & 7u)) atomicOr(&s_bad, 1u);
        ++at;
      }
    running += total;
    if (T != 0xffffffffu) { term = T; break; }                // (uniform: T comes from LDS behind a barrier)
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t q = term;
    while (q < n && s[q] == 0xffu) ++q;                        // fill bytes in front of the marker's code
    JdState st;
    st.st_scan = (running + 1u != nunits || s_bad) ? (uint32_t)ATTWARP_JPEGDEC_E_RESTART : 0u;
    st.eoi = q > term && q < n && s[q] == 0xd9u;
    st.fail = 0xffffffffu;
    st.nrst = running;
    if (!st.st_scan) ends[nunits - 1u] = term;
    v.states[b] = st;
    JdSubInfo info;
    info.nseg = v.subs[b].nseg; info.rounds = 0; info.accepted = 0; info.pad = 0;
    v.infos[b] = info;
  }
}

// grid: one workgroup per image planned for sub-streams (at least one workgroup, which then has nothing to do).
__global__ __launch_bounds__(JD_NT) void jpegdec_substream_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                                  uint8_t* scratch) {
  __shared__ JdHuff s_dc[3], s_ac[3];
  __shared__ int16_t s_blk[JD_NT][JD_SUB_BLK];
  __shared__ uint32_t s_tmp[JD_NT];
  __shared__ uint8_t s_zz[64];
  const int tid = threadIdx.x;
  const JdView v(table, scratch);
  if ((int)blockIdx.x >= v.hdr->reserved) return;
  const int b = v.subs[blockIdx.x].image;
  if (b < 0 || b >= v.hdr->B) return;
  const JdImage* im = v.images + b;
  const JdSub sub = v.subs[b];
  if (v.states[b].st_scan != 0 || sub.nseg == 0) return;      // (uniform) the info record already says "not accepted"
  const uint32_t n = im->stream_len, nseg = sub.nseg, S = sub.segment_bytes;
  uint32_t uend = v.ends[im->unit0];
  if (uend > n) uend = n;
  const int ncomp = im->ncomp;
  for (int c = 0; c < ncomp; ++c) {
    if (tid == 0) { jd_huff_ranges(s_dc[c], im->dc_counts[c]); jd_huff_ranges(s_ac[c], im->ac_counts[c]); }
    jd_huff_clear(s_dc[c], im->dc_symbols[c], jd_nsym(im->dc_counts[c]), tid, JD_NT);
    jd_huff_clear(s_ac[c], im->ac_symbols[c], jd_nsym(im->ac_counts[c]), tid, JD_NT);
  }
  if (tid < 64) s_zz[tid] = JD_ZIGZAG[tid];
  __syncthreads();
  for (int c = 0; c < ncomp; ++c) {
    jd_huff_fill(s_dc[c], im->dc_counts[c], tid, JD_NT);
    jd_huff_fill(s_ac[c], im->ac_counts[c], tid, JD_NT);
  }
  __syncthreads();
  // the stream is read in place: p is the dword in front of the image's first byte, lo that byte's offset in it
  const uint8_t* data = stream + im->stream_off;
  const uint32_t lo = (uint32_t)(reinterpret_cast<uintptr_t>(data) & 3u);
  const uint8_t* p = data - lo;
  JdSegState* seg = reinterpret_cast<JdSegState*>(scratch + sub.seg_off);
  JdSegment* res = reinterpret_cast<JdSegment*>(scratch + sub.seg_off + (uint64_t)nseg * sizeof(JdSegState));
  const uint32_t nb0 = (uint32_t)(im->hs * im->vs), nblk = nb0 + (uint32_t)ncomp - 1u;
  const uint32_t expected = (uint32_t)im->mcux * (uint32_t)im->mcuy * nblk;
  // every loop over segments below gives segment s to lane s % JD_NT, so a lane reads back its own entry and dirty flag
  for (uint32_t s = tid; s < nseg; s += JD_NT) {
    seg[s].entry = jd_segment_guess(data, s, S, uend);
    seg[s].dirty = 1u;
  }
  uint32_t rounds = 0;
  bool converged = false;
  while (rounds < sub.max_rounds) {                          // (uniform)
    ++rounds;
    for (uint32_t s = tid; s < nseg; s += JD_NT)
      if (seg[s].dirty) {
        JdSegment r;
        jd_decode_segment(p, lo, seg[s].entry, jd_segment_end(s, S, uend), uend, s_dc, s_ac, nb0, nblk, r);
        res[s] = r;
      }
    __syncthreads();                                         // every exit of this round is written
    int changed = 0;
    for (uint32_t s = tid; s < nseg; s += JD_NT) {
      uint32_t d = 0;
      if (s > 0) {
        const JdSync e = res[s - 1].exit;
        if (!jd_sync_equal(e, seg[s].entry)) { seg[s].entry = e; d = 1u; changed = 1; }
      }
      seg[s].dirty = d;
    }
    if (!__syncthreads_or(changed)) { converged = true; break; }
  }
  // exclusive sums of (owned blocks, DC differences) over the segments: lane t sums segments t * chunk .. in order
  const uint32_t chunk = (nseg + JD_NT - 1) / JD_NT;
  const uint32_t s0 = min((uint32_t)tid * chunk, nseg), s1 = min(s0 + chunk, nseg);
  uint32_t sum[4] = {0, 0, 0, 0};
  for (uint32_t s = s0; s < s1; ++s) {
    const JdSegment r = res[s];
    sum[0] += r.owned; sum[1] += r.dc[0]; sum[2] += r.dc[1]; sum[3] += r.dc[2];
  }
  uint32_t total;
  for (int e = 0; e < 4; ++e) sum[e] = jd_excl_sum(sum[e], s_tmp, total);
  uint32_t flags = 0;
  for (uint32_t s = s0; s < s1; ++s) {
    const JdSegment r = res[s];
    seg[s].before = sum[0];
    seg[s].pred[0] = sum[1]; seg[s].pred[1] = sum[2]; seg[s].pred[2] = sum[3];
    flags |= jd_segment_check(seg[s].entry, r, sum[0], expected, nblk);
    sum[0] += r.owned; sum[1] += r.dc[0]; sum[2] += r.dc[1]; sum[3] += r.dc[2];
  }
  const int bad = __syncthreads_or((int)(flags & 1u));
  const int found = __syncthreads_or((int)(flags & 2u));       // (and every `before` and predictor is written)
  bool accepted = converged && found && !bad;
  if (accepted) {                                            // (uniform)
    int16_t* coef = reinterpret_cast<int16_t*>(scratch + im->coef_off);
    uint32_t werr = 0;
    for (uint32_t s = tid; s < nseg; s += JD_NT) {
      const JdSegState e = seg[s];
      werr |= jd_write_segment(p, lo, e.entry, uend, s_dc, s_ac, *im, nb0, nblk, e.before, e.pred, res[s].owned, expected, s_blk[tid], s_zz,
                               coef);
    }
    if (__syncthreads_or((int)werr)) accepted = false;       // (never, after the checks: the sequential decode then redoes it)
  }
  if (tid == 0) {
    JdSubInfo info;
    info.nseg = nseg; info.rounds = rounds; info.accepted = accepted ? 1u : 0u; info.pad = 0;
    v.infos[b] = info;
  }
}

// grid: one wave per planned unit of the call.
__global__ __launch_bounds__(WAVE) void jpegdec_entropy_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                               uint8_t* __restrict__ scratch) {
  __shared__ JdHuff s_dc[3], s_ac[3];
  __shared__ uint32_t s_ring[JD_RING / 4];
  __shared__ int16_t s_blk[64];
  __shared__ int32_t s_pred[4];
  __shared__ uint8_t s_zz[64];
  __shared__ uint32_t s_pos, s_err;
  const int lane = threadIdx.x, u = blockIdx.x;
  const JdView v(table, scratch);
  const int b = v.find(&JdImage::unit0, u);
  const JdImage* im = v.images + b;
  JdState* state = v.states + b;
  if (state->st_scan != 0) return;                           // (uniform) the units' limits were never written
  if (v.infos[b].accepted != 0) return;                      // (uniform) the sub-stream kernel decoded this image's only unit
  const uint32_t k = (uint32_t)(u - im->unit0), n = im->stream_len;
  const int ncomp = im->ncomp;
  uint32_t start = v.starts[u], end = v.ends[u];
  if (end > n) end = n;                                      // (the scan never writes such limits)
  if (start > end) start = end;
  for (int c = 0; c < ncomp; ++c) {
    if (lane == 0) { jd_huff_ranges(s_dc[c], im->dc_counts[c]); jd_huff_ranges(s_ac[c], im->ac_counts[c]); }
    jd_huff_clear(s_dc[c], im->dc_symbols[c], jd_nsym(im->dc_counts[c]), lane, WAVE);
    jd_huff_clear(s_ac[c], im->ac_symbols[c], jd_nsym(im->ac_counts[c]), lane, WAVE);
  }
  s_zz[lane] = JD_ZIGZAG[lane];
  if (lane == 0) { s_pos = start; s_err = 0; }
  if (lane < 4) s_pred[lane] = 0;
  __syncthreads();
  for (int c = 0; c < ncomp; ++c) {
    jd_huff_fill(s_dc[c], im->dc_counts[c], lane, WAVE);
    jd_huff_fill(s_ac[c], im->ac_counts[c], lane, WAVE);
  }
  const JD_G uint8_t* s = (const JD_G uint8_t*)stream + im->stream_off;
  JD_G int16_t* coef = (JD_G int16_t*)(scratch + im->coef_off);
  // the geometry in registers: nothing in the loop below goes back to the table
  const int hs = im->hs, vs = im->vs, nb0 = hs * vs, nblk = min(nb0 + ncomp - 1, 6);   // blocks per MCU
  const uint32_t mcux = (uint32_t)im->mcux, nblocks = im->nblocks;
  const uint32_t bw0 = (uint32_t)im->bw[0], bw1 = (uint32_t)im->bw[1], b1 = im->block0[1], b2 = im->block0[2];
  const uint32_t nmcu = mcux * (uint32_t)im->mcuy, ri = (uint32_t)im->ri;
  const uint32_t m0 = k * ri, m1 = m0 + ri < nmcu ? m0 + ri : nmcu;
  JdBits br;
  br.init(reinterpret_cast<const uint8_t*>(s_ring), JD_RING - 1, start, end);
  uint32_t loaded = start & ~3u, err = 0;
  uint32_t my = m0 / mcux, mx = m0 - my * mcux;
  for (uint32_t m = m0; m < m1 && !err; ++m) {
    for (int jb = 0; jb < nblk; ++jb) {
      __syncthreads();                                       // s_pos of the block before; the tables the first time
      const uint32_t base = s_pos & ~3u;
      // keep the ring filled: a block takes at most 64 x (16 + 16) bits = 256 bytes, 512 with stuffing, and the reader looks
      // 8 more bytes ahead; after this loop more than JD_RING - JD_CHUNK bytes lie ahead of it, or the whole unit.  A chunk
      // only ever lands on ring bytes behind the reader: loaded - base <= JD_RING - JD_CHUNK.
      for (int it = 0; it < JD_RING / JD_CHUNK && loaded < end && loaded - base <= (uint32_t)(JD_RING - JD_CHUNK); ++it) {
        const uint32_t q = loaded + (uint32_t)lane * 4u;
        uint32_t w = 0;
        if (q < end && end - q >= 4u) w = *(const JD_G u32_una*)(s + q);
        else
          for (uint32_t e = 0; e < 4; ++e)
            if (q + e < end) w |= (uint32_t)s[q + e] << (8 * e);
        s_ring[(q & (uint32_t)(JD_RING - 1)) >> 2] = w;
        loaded += JD_CHUNK;
      }
      s_blk[lane] = 0;
      __syncthreads();
      if (lane == 0) {
        br.end = loaded < end ? loaded : end;
        const int c = jb < nb0 ? 0 : jb - nb0 + 1;
        int32_t p = s_pred[c];
        const uint32_t st = jd_decode_block(br, s_dc[c], s_ac[c], p, s_blk, s_zz);
        s_pred[c] = p;
        s_pos = br.pos;
        if (st) s_err = st;
      }
      __syncthreads();
      err = s_err;
      if (err) break;                                        // (uniform)
      uint32_t bi;
      if (jb < nb0) bi = jd_block_at(0u, bw0, hs, vs, mx, my, hs == 2 ? jb >> 1 : jb, hs == 2 ? jb & 1 : 0);
      else bi = jd_block_at(jb == nb0 ? b1 : b2, bw1, 1, 1, mx, my, 0, 0);
      if (bi < nblocks) coef[(size_t)bi * 64u + lane] = s_blk[lane];
    }
    if (++mx == mcux) { mx = 0; ++my; }
  }
  if (err && lane == 0) atomicMin(&state->fail, k << 8 | err);
}

// One thread per 8x8 block: all 64 values stay in registers through both passes, no lane talks to another, and the eight
// stores of neighbouring blocks of a block row are contiguous.
__global__ __launch_bounds__(JD_NT) void jpegdec_idct_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ uint16_t s_qt[3][64];
  const JdView v(table, scratch);
  const int b = v.find(&JdImage::idct_tile0, (int)blockIdx.x);
  const JdImage* im = v.images + b;
  if (threadIdx.x < 192) s_qt[threadIdx.x >> 6][threadIdx.x & 63] = im->qt[threadIdx.x >> 6][threadIdx.x & 63];
  __syncthreads();
  const uint32_t bi = (uint32_t)((int)blockIdx.x - im->idct_tile0) * JD_IDCT_TILE + threadIdx.x;
  if (bi >= im->nblocks) return;
  const int c = (im->ncomp == 3 && bi >= im->block0[1]) ? (bi >= im->block0[2] ? 2 : 1) : 0;
  const uint32_t local = bi - im->block0[c];
  const uint32_t bw = (uint32_t)im->bw[c], by = local / bw, bx = local - by * bw;
  const uint4* src = reinterpret_cast<const uint4*>(scratch + im->coef_off + (size_t)bi * 128u);
  uint32_t x[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 q = src[r];
    const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int32_t cf = (int16_t)(d[e >> 1] >> (16 * (e & 1)));
      x[r * 8 + e] = (uint32_t)cf * (uint32_t)s_qt[c][r * 8 + e];
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    uint32_t in[8];
    int32_t o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = x[r * 8 + col];
    jd_idct_1d(in, 11, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r * 8 + col] = (uint32_t)o[r];
  }
  const size_t pitch = (size_t)bw * 8u;
  uint8_t* dst = scratch + im->plane_off + (size_t)im->block0[c] * 64u + (size_t)by * 8u * pitch + (size_t)bx * 8u;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int32_t o[8];
    jd_idct_1d(&x[r * 8], 18, o);
    uint2 px;
    px.x = jd_clamp8(o[0] + 128) | jd_clamp8(o[1] + 128) << 8 | jd_clamp8(o[2] + 128) << 16 | jd_clamp8(o[3] + 128) << 24;
    px.y = jd_clamp8(o[4] + 128) | jd_clamp8(o[5] + 128) << 8 | jd_clamp8(o[6] + 128) << 16 | jd_clamp8(o[7] + 128) << 24;
    *reinterpret_cast<uint2*>(dst + (size_t)r * pitch) = px;
  }
}

__global__ __launch_bounds__(JD_NT) void jpegdec_color_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ scratch,
                                                              const JdState* __restrict__ states, uint8_t* __restrict__ out,
                                                              int32_t* __restrict__ status) {
  const attwarp_jpegdec_header* hdr = reinterpret_cast<const attwarp_jpegdec_header*>(table);
  const JdImage* images = reinterpret_cast<const JdImage*>(table + hdr->off_images);
  int lo = 0, hi = hdr->B - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (images[mid].color_tile0 <= (int)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const int b = lo;
  const JdImage* im = images + b;
  const int tile = (int)blockIdx.x - im->color_tile0;
  if (tile == 0 && threadIdx.x == 0) {
    const JdState st = states[b];
    status[b] = (int32_t)(st.st_scan ? st.st_scan : st.fail != 0xffffffffu ? (st.fail & 255u) : st.eoi ? 0u : (uint32_t)ATTWARP_JPEGDEC_E_NO_EOI);
  }
  const int W = im->W, H = im->H, hs = im->hs, vs = im->vs, oc = im->oc;
  const bool colour = im->ncomp == 3, to_luma = im->to_luma != 0, swap = im->swap != 0;
  const uint32_t npx = (uint32_t)W * (uint32_t)H;
  const uint8_t* p0 = scratch + im->plane_off;
  const int pitch0 = im->bw[0] * 8;
  const uint8_t* p1 = colour ? scratch + im->plane_off + (size_t)im->block0[1] * 64u : p0;
  const uint8_t* p2 = colour ? scratch + im->plane_off + (size_t)im->block0[2] * 64u : p0;
  const int pitchc = colour ? im->bw[1] * 8 : pitch0;
  const int dw = (W + hs - 1) / hs, dh = (H + vs - 1) / vs;
  JD_G uint8_t* o = (JD_G uint8_t*)out + im->out_off;
  for (int j = 0; j < JD_CPX; ++j) {
    const uint32_t px = (uint32_t)tile * JD_COLOR_TILE + (uint32_t)j * JD_NT + threadIdx.x;
    if (px >= npx) break;
    const int y = (int)(px / (uint32_t)W), x = (int)(px - (uint32_t)y * (uint32_t)W);
    const uint32_t Y = p0[(size_t)y * pitch0 + x];
    JD_G uint8_t* d = o + (size_t)px * oc;
    if (!colour) {
      d[0] = (uint8_t)Y;
      if (oc == 3) { d[1] = (uint8_t)Y; d[2] = (uint8_t)Y; }
      continue;
    }
    uint32_t r, g, bl;
    jd_ycc_to_rgb((int32_t)Y, jd_chroma(p1, pitchc, dw, dh, hs, vs, x, y), jd_chroma(p2, pitchc, dw, dh, hs, vs, x, y), r, g, bl);
    if (to_luma) d[0] = (uint8_t)jd_luma(r, g, bl);
    else { d[0] = (uint8_t)(swap ? bl : r); d[1] = (uint8_t)g; d[2] = (uint8_t)(swap ? r : bl); }
  }
}

}  // namespace attwarp

using namespace attwarp;

struct JdGeom {
  int mcux, mcuy, nunits;
  int bw[3], bh[3];
  uint32_t block0[3], nblocks;
};

static int jpegdec_geom(const attwarp_jpegdec_image& d, int b, JdGeom& g) {
  ATTWARP_REQUIRE(d.H >= 1 && d.W >= 1 && d.H <= 65535 && d.W <= 65535, "jpegdec: image %d: size %d x %d outside 1..65535", b, d.H, d.W);
  ATTWARP_REQUIRE(d.ncomp == 1 || d.ncomp == 3, "jpegdec: image %d: %d components (1 or 3)", b, d.ncomp);
  ATTWARP_REQUIRE((d.hs == 1 && d.vs == 1) || (d.ncomp == 3 && d.hs == 2 && (d.vs == 1 || d.vs == 2)),
                  "jpegdec: image %d: luma sampling %d x %d (1x1, 2x1, 2x2; grey 1x1)", b, d.hs, d.vs);
  ATTWARP_REQUIRE(d.restart_interval >= 0 && d.restart_interval <= 65535, "jpegdec: image %d: restart interval %d", b, d.restart_interval);
  ATTWARP_REQUIRE(d.mode >= ATTWARP_JPEGDEC_RGB && d.mode <= ATTWARP_JPEGDEC_KEEP, "jpegdec: image %d: unknown mode %d", b, d.mode);
  ATTWARP_REQUIRE(d.order == ATTWARP_RGB || d.order == ATTWARP_BGR, "jpegdec: image %d: channel order must be ATTWARP_RGB or ATTWARP_BGR", b);
  for (int c = 0; c < d.ncomp; ++c) {
    for (int k = 0; k < 64; ++k) ATTWARP_REQUIRE(d.qt[c][k] <= 255, "jpegdec: image %d: a quantisation value above 255", b);
    for (int t = 0; t < 2; ++t) {
      const uint8_t* counts = t ? d.ac_counts[c] : d.dc_counts[c];
      int left = 1, n = 0;
      for (int l = 0; l < 16; ++l) {
        left = 2 * left - counts[l];
        n += counts[l];
        ATTWARP_REQUIRE(left >= 0, "jpegdec: image %d: an over-subscribed Huffman table", b);
      }
      ATTWARP_REQUIRE(n <= 256, "jpegdec: image %d: a Huffman table of %d symbols", b, n);
      if (!t)
        for (int k = 0; k < n; ++k) ATTWARP_REQUIRE(d.dc_symbols[c][k] <= 15, "jpegdec: image %d: a DC category above 15", b);
    }
  }
  g.mcux = (d.W + 8 * d.hs - 1) / (8 * d.hs);
  g.mcuy = (d.H + 8 * d.vs - 1) / (8 * d.vs);
  const int64_t nmcu = (int64_t)g.mcux * g.mcuy;
  const int64_t units = d.restart_interval ? (nmcu + d.restart_interval - 1) / d.restart_interval : 1;
  int64_t blocks = 0;
  for (int c = 0; c < 3; ++c) {
    g.bw[c] = c < d.ncomp ? g.mcux * (c == 0 ? d.hs : 1) : 0;
    g.bh[c] = c < d.ncomp ? g.mcuy * (c == 0 ? d.vs : 1) : 0;
    g.block0[c] = (uint32_t)blocks;
    blocks += (int64_t)g.bw[c] * g.bh[c];
  }
  if (units > ATTWARP_JPEGDEC_MAX_UNITS)
    return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: image %d: %lld restart intervals (> %d)", b, (long long)units, ATTWARP_JPEGDEC_MAX_UNITS);
  if (blocks >= ATTWARP_JPEGDEC_MAX_BLOCKS)
    return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: image %d: %lld blocks (>= %d)", b, (long long)blocks, ATTWARP_JPEGDEC_MAX_BLOCKS);
  if (d.stream_len >= ((uint64_t)1 << 31) || d.stream_off >= ((uint64_t)1 << 62))
    return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: image %d: entropy data of 2 GiB or more", b);
  g.nunits = (int)units;
  g.nblocks = (uint32_t)blocks;
  return ATTWARP_OK;
}

// header, image records, sub-stream records (always present, so that the size depends on B alone)
static size_t jpegdec_bytes(int B) {
  return (size_t)(jd_align(sizeof(attwarp_jpegdec_header), 16) + (uint64_t)B * sizeof(JdImage) + (uint64_t)B * sizeof(JdSub));
}

extern "C" size_t attwarp_jpegdec_table_bytes(const attwarp_jpegdec_image* images, int B) {
  if (!images || B <= 0 || B > JD_MAX_B) {
    fail(ATTWARP_E_ARG, "jpegdec_table_bytes: B=%d outside the limits", B);
    return 0;
  }
  return jpegdec_bytes(B);
}

extern "C" int attwarp_jpegdec_plan(const attwarp_jpegdec_image* images, int B, void* table, size_t table_bytes) {
  return attwarp_jpegdec_plan_ex(images, B, table, table_bytes, 0, 0);
}

extern "C" int attwarp_jpegdec_plan_ex(const attwarp_jpegdec_image* images, int B, void* table, size_t table_bytes, int segment_bytes,
                                       int max_rounds) {
  ATTWARP_REQUIRE(images, "jpegdec: null image array");
  const bool substreams = segment_bytes != 0 || max_rounds != 0;
  if (substreams) {
    ATTWARP_REQUIRE(segment_bytes >= 32 && segment_bytes <= 512 && (segment_bytes & (segment_bytes - 1)) == 0,
                    "jpegdec: segment_bytes=%d must be a power of two in 32..512", segment_bytes);
    ATTWARP_REQUIRE(max_rounds >= 1 && max_rounds <= JD_SUB_MAX_ROUNDS, "jpegdec: max_rounds=%d outside 1..%d", max_rounds, JD_SUB_MAX_ROUNDS);
  }
  ATTWARP_REQUIRE(B > 0, "jpegdec: non-positive batch size");
  if (B > JD_MAX_B) return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: B=%d > 2^20", B);
  ATTWARP_REQUIRE(table, "jpegdec_plan: null table");
  const size_t need = jpegdec_bytes(B);
  ATTWARP_REQUIRE(table_bytes >= need, "jpegdec_plan: table of %zu bytes, %zu needed", table_bytes, need);
  int64_t units = 0, itiles = 0, ctiles = 0;
  for (int b = 0; b < B; ++b) {                              // everything is checked before anything is written
    JdGeom g;
    if (const int rc = jpegdec_geom(images[b], b, g)) return rc;
    units += g.nunits;
    itiles += (g.nblocks + JD_IDCT_TILE - 1) / JD_IDCT_TILE;
    ctiles += ((int64_t)images[b].H * images[b].W + JD_COLOR_TILE - 1) / JD_COLOR_TILE;
  }
  if (units > JD_MAX_TOTAL_UNITS || itiles > JD_MAX_TOTAL_UNITS || ctiles > JD_MAX_TOTAL_UNITS)
    return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: %lld units, %lld + %lld workgroups in one call (> 2^30)", (long long)units, (long long)itiles, (long long)ctiles);
  uint8_t* t = static_cast<uint8_t*>(table);
  std::memset(t, 0, need);
  attwarp_jpegdec_header h;
  std::memset(&h, 0, sizeof h);
  h.magic = JD_MAGIC;
  h.B = B;
  h.total_units = (int32_t)units;
  h.idct_tiles = (int32_t)itiles;
  h.color_tiles = (int32_t)ctiles;
  h.table_bytes = need;
  h.off_images = jd_align(sizeof(attwarp_jpegdec_header), 16);
  JdImage* im = reinterpret_cast<JdImage*>(t + h.off_images);
  JdSub* sub = reinterpret_cast<JdSub*>(t + h.off_images + (uint64_t)B * sizeof(JdImage));
  int32_t nsub = 0;
  uint64_t soff = jd_data_base(B, (int)units), ooff = 0, stream_bytes = 0;
  int32_t u0 = 0, it0 = 0, ct0 = 0;
  for (int b = 0; b < B; ++b) {
    const attwarp_jpegdec_image& d = images[b];
    JdGeom g;
    jpegdec_geom(d, b, g);
    JdImage& r = im[b];
    r.stream_off = d.stream_off;
    r.stream_len = (uint32_t)d.stream_len;
    r.H = d.H; r.W = d.W; r.ncomp = d.ncomp; r.hs = d.hs; r.vs = d.vs;
    r.oc = d.mode == ATTWARP_JPEGDEC_L ? 1 : d.mode == ATTWARP_JPEGDEC_RGB ? 3 : d.ncomp;
    r.to_luma = d.ncomp == 3 && r.oc == 1;
    r.swap = d.ncomp == 3 && r.oc == 3 && d.order == ATTWARP_BGR;
    r.mcux = g.mcux; r.mcuy = g.mcuy;
    r.ri = d.restart_interval ? d.restart_interval : g.mcux * g.mcuy;
    r.nunits = g.nunits; r.unit0 = u0;
    r.idct_tile0 = it0; r.color_tile0 = ct0;
    for (int c = 0; c < 3; ++c) { r.bw[c] = g.bw[c]; r.bh[c] = g.bh[c]; r.block0[c] = g.block0[c]; }
    r.nblocks = g.nblocks;
    std::memcpy(r.qt, d.qt, sizeof r.qt);
    std::memcpy(r.dc_counts, d.dc_counts, sizeof r.dc_counts);
    std::memcpy(r.ac_counts, d.ac_counts, sizeof r.ac_counts);
    std::memcpy(r.dc_symbols, d.dc_symbols, sizeof r.dc_symbols);
    std::memcpy(r.ac_symbols, d.ac_symbols, sizeof r.ac_symbols);
    r.coef_off = soff;
    soff += jd_align((uint64_t)g.nblocks * 128u, 256);
    r.plane_off = soff;
    soff += jd_align((uint64_t)g.nblocks * 64u, 256);
    r.out_off = ooff;
    ooff += (uint64_t)d.H * d.W * r.oc;
    u0 += g.nunits;
    it0 += (int32_t)((g.nblocks + JD_IDCT_TILE - 1) / JD_IDCT_TILE);
    ct0 += (int32_t)(((int64_t)d.H * d.W + JD_COLOR_TILE - 1) / JD_COLOR_TILE);
    stream_bytes = std::max(stream_bytes, d.stream_off + d.stream_len);
    // sub-streams: a marker-less image (one unit) whose data is at least two segments long
    const uint64_t nseg = substreams ? (d.stream_len + (uint64_t)segment_bytes - 1) / (uint64_t)segment_bytes : 0;
    sub[b].segment_bytes = (uint32_t)segment_bytes;
    sub[b].max_rounds = (uint32_t)max_rounds;
    if (substreams && g.nunits == 1 && d.stream_len >= 2u * (uint64_t)segment_bytes && nseg <= (uint64_t)JD_SUB_MAX_SEGS) {
      sub[b].nseg = (uint32_t)nseg;
      sub[nsub++].image = b;
    }
  }
  // behind everything there was: the per-image sub-stream results, then the segments of every image planned for them
  const uint64_t info_off = soff;
  soff += jd_align((uint64_t)B * sizeof(JdSubInfo), 256);
  for (int b = 0; b < B; ++b) {
    sub[b].info_off = info_off;
    sub[b].seg_off = soff;
    soff += jd_align((uint64_t)sub[b].nseg * (sizeof(JdSegState) + sizeof(JdSegment)), 256);
  }
  h.reserved = nsub;
  h.scratch_bytes = soff;
  h.out_bytes = ooff;
  h.stream_bytes = stream_bytes;
  std::memcpy(t, &h, sizeof h);
  return ATTWARP_OK;
}

extern "C" uint64_t attwarp_jpegdec_info_offset(const void* table_host) {
  if (!table_host) return 0;
  attwarp_jpegdec_header h;
  std::memcpy(&h, table_host, sizeof h);
  if (h.magic != JD_MAGIC || h.B <= 0 || h.B > JD_MAX_B) return 0;
  JdSub s;
  std::memcpy(&s, static_cast<const uint8_t*>(table_host) + h.off_images + (uint64_t)h.B * sizeof(JdImage), sizeof s);
  return s.info_off;
}

extern "C" int attwarp_jpegdec_decode(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                                      uint8_t* out, size_t out_bytes, int32_t* status, void* stream) {
  ATTWARP_REQUIRE(table_host && table_dev && stream_bytes && scratch && out && status, "jpegdec_decode: null pointer");
  attwarp_jpegdec_header h;
  std::memcpy(&h, table_host, sizeof h);
  ATTWARP_REQUIRE(h.magic == JD_MAGIC && h.B > 0 && h.B <= JD_MAX_B && h.total_units >= h.B && h.total_units <= JD_MAX_TOTAL_UNITS &&
                      h.idct_tiles >= h.B && h.idct_tiles <= JD_MAX_TOTAL_UNITS && h.color_tiles >= h.B && h.color_tiles <= JD_MAX_TOTAL_UNITS &&
                      h.reserved >= 0 && h.reserved <= h.B,
                  "jpegdec_decode: not a table of attwarp_jpegdec_plan");
  ATTWARP_REQUIRE(out_bytes >= h.out_bytes, "jpegdec_decode: out of %zu bytes, %llu needed", out_bytes, (unsigned long long)h.out_bytes);
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(table_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(scratch) % 256 == 0 &&
                      reinterpret_cast<uintptr_t>(status) % 4 == 0,
                  "jpegdec_decode: table_dev must be 8-byte, scratch 256-byte, status 4-byte aligned");
  hipStream_t st = as_stream(stream);
  const uint8_t* td = static_cast<const uint8_t*>(table_dev);
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  hipLaunchKernelGGL(jpegdec_scan_kernel, dim3(h.B), dim3(JD_NT), 0, st, td, stream_bytes, sc);
  if (const int rc = check_launch("jpegdec_scan_kernel")) return rc;
  hipLaunchKernelGGL(jpegdec_substream_kernel, dim3(std::max(h.reserved, 1)), dim3(JD_NT), 0, st, td, stream_bytes, sc);
  if (const int rc = check_launch("jpegdec_substream_kernel")) return rc;
  hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3(h.total_units), dim3(WAVE), 0, st, td, stream_bytes, sc);
  if (const int rc = check_launch("jpegdec_entropy_kernel")) return rc;
  hipLaunchKernelGGL(jpegdec_idct_kernel, dim3(h.idct_tiles), dim3(JD_NT), 0, st, td, sc);
  if (const int rc = check_launch("jpegdec_idct_kernel")) return rc;
  hipLaunchKernelGGL(jpegdec_color_kernel, dim3(h.color_tiles), dim3(JD_NT), 0, st, td, (const uint8_t*)sc, (const JdState*)sc, out, status);
  return check_launch("jpegdec_color_kernel");
}
