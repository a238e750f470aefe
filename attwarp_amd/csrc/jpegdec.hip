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
// Files of every other layout (attwarp_jpegdec_plan_layouts / attwarp_jpegdec_decode_layouts, DESIGN.md 3.19: four components,
// any sampling, RGB-coded) take the same five launches over records of their own: the jpegfmt_* kernels behind the scan families'.
// Progressive files (attwarp_jpegdec_plan_scans / attwarp_jpegdec_decode_scans) keep the last two launches
// and put in front of them
//   jpegprog_clear_kernel   the coefficient memory of every image zeroed (the scans only refine it), the states opened;
//   jpegprog_scan_kernel    one workgroup per SCAN: the restart-marker rule above (jd_scan_units) for the scan's own data;
//   jpegprog_entropy_kernel one launch per dependency level of the scans, one wave per (scan, unit): the four block routines
//                           of jpegprog_blocks.hpp; a wave stores only the int16s of its band Ss..Se (the band rule).
// A table of attwarp_jpegdec_plan_scans_ex with sub-streams puts, in front of a level's entropy launch,
//   jpegprog_substream_kernel one workgroup per marker-less scan of the level that is cut into segments: the four routes of
//                           jpegprog_sync_blocks.hpp; a scan it accepts is flagged and skipped by the entropy launch.
// Progressive files of every other layout and sequential files of several scans (attwarp_jpegdec_plan_layout_scans /
// attwarp_jpegdec_decode_layout_scans) are the cross term: JfImage frames, JsScan records (jpegscan_blocks.hpp),
// jpegscan_clear_kernel, jpegscan_marks_kernel, one jpegscan_entropy_kernel launch per level over the general MCU with a
// fifth, sequential kind of block, then jpegfmt_idct_kernel and jpegfmt_color_kernel unchanged.
// All kernels come first, then the host side, written once over the record family: JdFrames / JfFrames (the image records:
// jd_plan_frames is both frame planners), JpScans / JsScans (the scan records: jp_plan_scans is the three scan planners), and
// jd_decode_args, jd_decode_frames and jd_launch_idct_color for the four decode entry points.  The kernels themselves stay
// one per family and launch: they share the block-level code (JdLayout / JfLayout), jd_scan_image, jp_clear_body, jp_marks_body
// and jd_status, and no more, because any further sharing tried changed their instructions (docs/experiments.md).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "jpegfmt_blocks.hpp"
#include "jpegprog_blocks.hpp"
#include "jpegprog_sync_blocks.hpp"
#include "jpegscan_blocks.hpp"
#include "jpegscan_sync_blocks.hpp"

namespace attwarp {

#define JD_G __attribute__((address_space(1)))
constexpr uint32_t JD_MAGIC = 0x4745504au, JD_MAGIC_LAYOUTS = 0x4745504cu;   // (the second: attwarp_jpegdec_plan_layouts)
constexpr uint32_t JD_MAGIC_LAYOUT_SCANS = 0x4745504du;                      // (attwarp_jpegdec_plan_layout_scans)
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

template <class Image>
struct JdViewOf {                      // a planned table and its scratch buffer: JdImage records, or JfImage of the layout family
  const attwarp_jpegdec_header* hdr;
  const Image* images;
  const JdSub* subs;
  JdSubInfo* infos;
  JdState* states;
  uint32_t *starts, *ends;
  __device__ __forceinline__ JdViewOf(const uint8_t* table, uint8_t* scratch) {
    hdr = reinterpret_cast<const attwarp_jpegdec_header*>(table);
    images = reinterpret_cast<const Image*>(table + hdr->off_images);
    subs = reinterpret_cast<const JdSub*>(table + hdr->off_images + (uint64_t)hdr->B * sizeof(Image));
    infos = reinterpret_cast<JdSubInfo*>(scratch + subs[0].info_off);
    states = reinterpret_cast<JdState*>(scratch);
    starts = reinterpret_cast<uint32_t*>(scratch + jd_starts_off(hdr->B));
    ends = reinterpret_cast<uint32_t*>(scratch + jd_ends_off(hdr->B, hdr->total_units));
  }
  // the image whose range of units / tiles holds t: the last one whose first is <= t (the firsts ascend strictly)
  __device__ __forceinline__ int find(int32_t Image::*first, int t) const {
    int lo = 0, hi = hdr->B - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const int mid = (lo + hi + 1) >> 1;
      if (images[mid].*first <= t) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  }
};
using JdView = JdViewOf<JdImage>;
using JfView = JdViewOf<JfImage>;

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

// The restart-marker scan of one run of entropy data by one workgroup: s[0 .. n), planned for nunits units.  Writes the
// units' starts and all ends but the last, -> the markers found in front of the data's end (running) and that end (term);
// s_bad: an index out of its cycle.  Ends behind a barrier.
__device__ __forceinline__ void jd_scan_units(const JD_G uint8_t* s, uint32_t n, uint32_t nunits, uint32_t* starts, uint32_t* ends,
                                              uint32_t* s_tmp, uint32_t& s_term, uint32_t& s_bad, uint32_t& running, uint32_t& term) {
  const int tid = threadIdx.x;
  if (tid == 0) { s_term = 0xffffffffu; s_bad = 0; starts[0] = 0; }
  __syncthreads();
  running = 0; term = n;
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
}

// The restart scan of image b of a view: its units' limits, its state and its (empty) sub-stream result.
template <class Image>
__device__ __forceinline__ void jd_scan_image(const JdViewOf<Image>& v, const uint8_t* stream, int b, uint32_t* s_tmp, uint32_t& s_term,
                                              uint32_t& s_bad) {
  const int tid = threadIdx.x;
  const Image* im = v.images + b;
  const JD_G uint8_t* s = (const JD_G uint8_t*)stream + im->stream_off;
  const uint32_t n = im->stream_len, nunits = (uint32_t)im->nunits;
  uint32_t* ends = v.ends + im->unit0;
  uint32_t running, term;
  jd_scan_units(s, n, nunits, v.starts + im->unit0, ends, s_tmp, s_term, s_bad, running, term);
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

__global__ __launch_bounds__(JD_NT) void jpegdec_scan_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                             uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_tmp[JD_NT], s_term, s_bad;
  const JdView v(table, scratch);
  jd_scan_image(v, stream, (int)blockIdx.x, s_tmp, s_term, s_bad);
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

// One wave keeps its ring of the unit's bytes filled: chunks of JD_CHUNK bytes from `loaded` on, while they land on ring
// bytes behind the reader (base: the reader's position, rounded down to a dword).  Nothing at or behind `end` is loaded.
__device__ __forceinline__ void jd_ring_fill(uint32_t* s_ring, const JD_G uint8_t* s, uint32_t& loaded, uint32_t base, uint32_t end, int lane) {
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
      jd_ring_fill(s_ring, s, loaded, base, end, lane);
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

// One block by one thread: src its 64 int16 coefficients, qt the component's table (LDS), dst its top-left pixel in a plane
// of `pitch` bytes per row.  All 64 values stay in registers through both passes.
__device__ __forceinline__ void jd_idct_block(const uint4* src, const uint16_t* qt, uint8_t* dst, size_t pitch) {
  uint32_t x[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 q = src[r];
    const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int32_t cf = (int16_t)(d[e >> 1] >> (16 * (e & 1)));
      x[r * 8 + e] = (uint32_t)cf * (uint32_t)qt[r * 8 + e];
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

// One thread per 8x8 block: no lane talks to another, and the eight stores of neighbouring blocks of a block row are contiguous.
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
  jd_idct_block(reinterpret_cast<const uint4*>(scratch + im->coef_off + (size_t)bi * 128u), s_qt[c],
                scratch + im->plane_off + (size_t)im->block0[c] * 64u + (size_t)by * 8u * ((size_t)bw * 8u) + (size_t)bx * 8u, (size_t)bw * 8u);
}

// The status word of an image: the restart scan's, else the first failing unit's, else whether EOI follows the data.
__device__ __forceinline__ int32_t jd_status(const JdState& st) {
  return (int32_t)(st.st_scan ? st.st_scan : st.fail != 0xffffffffu ? (st.fail & 255u) : st.eoi ? 0u : (uint32_t)ATTWARP_JPEGDEC_E_NO_EOI);
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
    status[b] = jd_status(st);
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

// ---- progressive files: a table of attwarp_jpegdec_plan_scans is a baseline table of B one-unit images (what
// the IDCT and colour kernels read) with a JpHeader and the scan records behind it, sorted by (level, image, position) ---------
constexpr uint32_t JP_MAGIC = 0x4745504bu;
struct JpHeader {
  uint32_t magic;
  int32_t nscans, nlevels, total_units;
  uint64_t off_scans;                  // JpScan[nscans] in the table
  uint64_t starts_off;                 // uint32 starts[total_units], ends[total_units] in the scratch buffer
  uint64_t clear_off, clear_bytes;     // every image's coefficients (and planes) in the scratch buffer, multiples of 16
  int32_t level_scan0[ATTWARP_JPEGDEC_MAX_SCANS + 1];   // the first record of each level
  int32_t level_waves[ATTWARP_JPEGDEC_MAX_SCANS + 1];   // waves of each level's launch
};
static_assert(sizeof(JpHeader) % 8 == 0, "record layout");
// (behind the first part of a table: header, image records of `record` bytes, sub-stream records, always present; for
// JdImage records attwarp_jpegdec_table_bytes is this sum)
__host__ __device__ inline uint64_t jp_header_off(int B, size_t record) {
  return jd_align(sizeof(attwarp_jpegdec_header), 16) + (uint64_t)B * record + (uint64_t)B * sizeof(JdSub);
}
struct JsHeader {                      // of the scans over JfImage records: a JpHeader and
  JpHeader h;
  int32_t level_tables[ATTWARP_JPEGDEC_MAX_SCANS + 1];  // code tables the scans of each level hold in LDS at most (1 .. 8)
};
static_assert(sizeof(JpHeader) == 568 && sizeof(JsHeader) == 832 && offsetof(JsHeader, level_tables) == sizeof(JpHeader), "record layout");
static_assert(offsetof(JsHeader, h.magic) == 0 && offsetof(JsHeader, h.nscans) == 4 && offsetof(JsHeader, h.nlevels) == 8 &&
                  offsetof(JsHeader, h.total_units) == 12 && offsetof(JsHeader, h.off_scans) == 16 && offsetof(JsHeader, h.starts_off) == 24 &&
                  offsetof(JsHeader, h.clear_off) == 32 && offsetof(JsHeader, h.clear_bytes) == 40 && offsetof(JsHeader, h.level_scan0) == 48 &&
                  offsetof(JsHeader, h.level_waves) == 48 + 4 * (ATTWARP_JPEGDEC_MAX_SCANS + 1), "record layout");

// The coefficient memory of every image zeroed (the scans only refine it) and the per-image states opened: the clear launch of
// both scan families (JdImage records with a JpHeader, JfImage records with a JsHeader).
template <class Image>
__device__ __forceinline__ void jp_clear_body(const JdViewOf<Image>& v, uint8_t* scratch, uint64_t clear_off, uint64_t clear_bytes) {
  uint4* d = reinterpret_cast<uint4*>(scratch + clear_off);
  const uint64_t n = clear_bytes / 16u;
  for (uint64_t i = (uint64_t)blockIdx.x * JD_NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * JD_NT) d[i] = make_uint4(0, 0, 0, 0);
  for (int b = (int)(blockIdx.x * JD_NT + threadIdx.x); b < v.hdr->B; b += (int)(gridDim.x * JD_NT)) {
    JdState st;
    st.st_scan = 0; st.eoi = 0; st.fail = 0xffffffffu; st.nrst = 0;
    v.states[b] = st;
    JdSubInfo info;
    info.nseg = 0; info.rounds = 0; info.accepted = 0; info.pad = 0;
    v.infos[b] = info;
  }
}

// The sub-stream records of a table planned with them (behind the scan records) and the per-scan results in scratch.
struct JpSyncView {
  const JpSyncHeader* sh;
  const JpSync* sy;
  JpSyncInfo* infos;
};
__device__ __forceinline__ bool jp_sync_view(const JdView& v, const JpHeader* ph, const uint8_t* table, uint8_t* scratch, JpSyncView& y) {
  const uint64_t at = ph->off_scans + (uint64_t)ph->nscans * sizeof(JpScan);
  if (v.hdr->table_bytes < at + sizeof(JpSyncHeader) + (uint64_t)ph->nscans * sizeof(JpSync)) return false;   // planned without them
  y.sh = reinterpret_cast<const JpSyncHeader*>(table + at);
  y.sy = reinterpret_cast<const JpSync*>(table + at + sizeof(JpSyncHeader));
  y.infos = reinterpret_cast<JpSyncInfo*>(scratch + y.sh->info_off);
  return y.sh->magic == JP_SYNC_MAGIC;
}

__global__ __launch_bounds__(JD_NT) void jpegprog_clear_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  const JdView v(table, scratch);
  const JpHeader* ph = reinterpret_cast<const JpHeader*>(table + jp_header_off(v.hdr->B, sizeof(JdImage)));
  jp_clear_body(v, scratch, ph->clear_off, ph->clear_bytes);
  JpSyncView y;
  if (!jp_sync_view(v, ph, table, scratch, y)) return;
  const JpScan* scans = reinterpret_cast<const JpScan*>(table + ph->off_scans);
  for (int i = (int)(blockIdx.x * JD_NT + threadIdx.x); i < ph->nscans; i += (int)(gridDim.x * JD_NT)) {
    JpSyncInfo info;
    info.route = y.sy[i].nseg ? 1u + scans[i].kind : 0u; info.nseg = y.sy[i].nseg; info.rounds = 0; info.accepted = 0;
    info.ticks[0] = info.ticks[1] = info.ticks[2] = 0; info.pad = 0;
    if (y.sy[i].slot < (uint32_t)ph->nscans) y.infos[y.sy[i].slot] = info;
  }
}

// The restart-marker rule of jpegdec_scan_kernel for one SCAN's own data and units, by one workgroup: the restart launch of
// both scan families (sc: a JpScan or a JsScan; starts: uint32 starts[total_units], ends[total_units] of the call).
template <class Image, class Scan>
__device__ __forceinline__ void jp_marks_body(const JdViewOf<Image>& v, const Scan* sc, const uint8_t* stream, uint32_t* all_starts,
                                              int32_t total_units, uint32_t* s_tmp, uint32_t& s_term, uint32_t& s_bad) {
  if (sc->image >= (uint32_t)v.hdr->B) return;
  const Image* im = v.images + sc->image;
  const uint32_t off = sc->off < im->stream_len ? sc->off : im->stream_len;
  const JD_G uint8_t* s = (const JD_G uint8_t*)stream + im->stream_off + off;
  const uint32_t n = im->stream_len - off, nunits = sc->nunits;
  uint32_t* starts = all_starts + sc->unit0;
  uint32_t* ends = starts + total_units;
  uint32_t running, term;
  jd_scan_units(s, n, nunits, starts, ends, s_tmp, s_term, s_bad, running, term);
  if (threadIdx.x == 0) {
    JdState* st = v.states + sc->image;
    if (running + 1u != nunits || s_bad) st->st_scan = (uint32_t)ATTWARP_JPEGDEC_E_RESTART;   // (every writer stores this value)
    else ends[nunits - 1u] = term;
    atomicAdd(&st->nrst, running);
    if (sc->last) {
      uint32_t q = term;
      while (q < n && s[q] == 0xffu) ++q;
      st->eoi = q > term && q < n && s[q] == 0xd9u;
    }
  }
}

// grid: one workgroup per SCAN.
__global__ __launch_bounds__(JD_NT) void jpegprog_scan_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                              uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_tmp[JD_NT], s_term, s_bad;
  const JdView v(table, scratch);
  const JpHeader* ph = reinterpret_cast<const JpHeader*>(table + jp_header_off(v.hdr->B, sizeof(JdImage)));
  jp_marks_body(v, reinterpret_cast<const JpScan*>(table + ph->off_scans) + blockIdx.x, stream,
                reinterpret_cast<uint32_t*>(scratch + ph->starts_off), ph->total_units, s_tmp, s_term, s_bad);
}

// grid: one wave per (scan, unit) of the launch's level.  The band rule: a wave may LOAD a block's whole row for its
// history, but stores only the int16s at zigzag positions Ss..Se, one 2-byte store per lane: another wave of the level may
// be refining another band of the same block.
__global__ __launch_bounds__(WAVE) void jpegprog_entropy_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                                uint8_t* scratch, int level) {
  __shared__ JdHuff s_h[3];
  __shared__ uint32_t s_ring[JD_RING / 4];
  __shared__ int16_t s_blk[64];
  __shared__ int32_t s_pred[4];
  __shared__ uint8_t s_zz[64];
  __shared__ uint32_t s_pos, s_err, s_run;
  const int lane = threadIdx.x, w = blockIdx.x;
  const JdView v(table, scratch);
  const JpHeader* ph = reinterpret_cast<const JpHeader*>(table + jp_header_off(v.hdr->B, sizeof(JdImage)));
  const JpScan* scans = reinterpret_cast<const JpScan*>(table + ph->off_scans);
  int lo = ph->level_scan0[level], hi = ph->level_scan0[level + 1] - 1;
  if (hi < lo) return;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (scans[mid].wave0 <= (uint32_t)w) lo = mid;
    else hi = mid - 1;
  }
  const JpScan* sc = scans + lo;
  if (sc->image >= (uint32_t)v.hdr->B) return;
  const JdImage* im = v.images + sc->image;
  JdState* state = v.states + sc->image;
  if (state->st_scan != 0) return;                           // (uniform) some scan's limits were never written
  JpSyncView y;
  if (jp_sync_view(v, ph, table, scratch, y) && y.sy[lo].slot < (uint32_t)ph->nscans && y.infos[y.sy[lo].slot].accepted != 0)
    return;                                                  // (uniform) the sub-stream kernel decoded this scan's only unit
  const uint32_t k = (uint32_t)w - sc->wave0;
  if (k >= sc->nunits) return;
  const uint32_t off = sc->off < im->stream_len ? sc->off : im->stream_len, n = im->stream_len - off;
  const uint32_t* pstarts = reinterpret_cast<const uint32_t*>(scratch + ph->starts_off) + sc->unit0;
  uint32_t start = pstarts[k], end = pstarts[ph->total_units + k];
  if (end > n) end = n;
  if (start > end) start = end;
  const uint32_t kind = sc->kind, ss = sc->ss, se = sc->se < 63u ? sc->se : 63u, al = sc->al < 15u ? sc->al : 15u;
  const int ntab = kind == JP_DC_FIRST ? 3 : kind == JP_DC_REFINE ? 0 : 1;
  for (int c = 0; c < ntab; ++c) {
    if (lane == 0) jd_huff_ranges(s_h[c], sc->counts[c]);
    jd_huff_clear(s_h[c], sc->symbols[c], jd_nsym(sc->counts[c]), lane, WAVE);
  }
  s_zz[lane] = JD_ZIGZAG[lane];
  if (lane == 0) { s_pos = start; s_err = 0; s_run = 0; }
  if (lane < 4) s_pred[lane] = 0;
  __syncthreads();
  for (int c = 0; c < ntab; ++c) jd_huff_fill(s_h[c], sc->counts[c], lane, WAVE);
  const JD_G uint8_t* s = (const JD_G uint8_t*)stream + im->stream_off + off;
  JD_G int16_t* coef = (JD_G int16_t*)(scratch + im->coef_off);
  const uint32_t nslot = sc->nslot >= 1u && sc->nslot <= 6u ? sc->nslot : 1u, nblocks = im->nblocks;
  const uint32_t nmcu = sc->nmcu, ri = sc->ri;
  const uint32_t m0 = k * ri, m1 = m0 + ri < nmcu ? m0 + ri : nmcu;
  const uint32_t iend = m1 * nslot;
  const bool dc = kind <= JP_DC_REFINE;
  JdBits br;
  br.init(reinterpret_cast<const uint8_t*>(s_ring), JD_RING - 1, start, end);
  uint32_t loaded = start & ~3u, err = 0, eobrun = 0;
  for (uint32_t i = m0 * nslot; i < iend;) {
    const uint32_t m = i / nslot, j = i - m * nslot;
    const uint32_t bi = jp_block_index(*im, *sc, m, j);
    __syncthreads();                                         // s_pos of the block before; the tables the first time
    jd_ring_fill(s_ring, s, loaded, s_pos & ~3u, end, lane);  // a block takes at most 64 x 16 + 64 + 14 bits: the baseline's bound holds
    int16_t have = 0;
    if (bi < nblocks && (kind == JP_AC_REFINE || (kind == JP_DC_REFINE && lane == 0))) have = coef[(size_t)bi * 64u + lane];
    s_blk[lane] = have;
    __syncthreads();
    if (lane == 0) {
      br.end = loaded < end ? loaded : end;
      uint32_t st;
      if (kind == JP_DC_FIRST) {
        const int t = sc->slot_t[j & 7u] % 3;
        int32_t p = s_pred[t];
        st = jp_dc_first(br, s_h[t], p, al, s_blk[0]);
        s_pred[t] = p;
      } else if (kind == JP_DC_REFINE) st = jp_dc_refine(br, al, s_blk[0]);
      else if (kind == JP_AC_FIRST) st = jp_ac_first(br, s_h[0], ss, se, al, eobrun, s_blk, s_zz);
      else st = jp_ac_refine(br, s_h[0], ss, se, al, eobrun, s_blk, s_zz);
      s_pos = br.pos;
      s_run = eobrun;
      if (st) s_err = st;
    }
    __syncthreads();
    err = s_err;
    if (err) break;                                          // (uniform)
    if (bi < nblocks && (dc ? lane == 0 : ((uint32_t)lane >= ss && (uint32_t)lane <= se))) {
      const uint32_t at = s_zz[lane] & 63u;
      coef[(size_t)bi * 64u + at] = s_blk[at];
    }
    eobrun = s_run;
    uint32_t adv = 1;
    if (kind == JP_AC_FIRST && eobrun > 0) {                 // the blocks of the run are skipped without touching memory
      const uint32_t skip = eobrun < iend - i - 1u ? eobrun : iend - i - 1u;
      adv += skip;
      eobrun -= skip;                                        // (what is left at the unit's end is dropped with the unit)
    }
    i += adv;
  }
  if (err && lane == 0) atomicMin(&state->fail, sc->index << 24 | k << 8 | err);
}

// jd_excl_sum over block counts that saturate at JP_SYNC_CAP (saturating addition of such counts is associative)
__device__ __forceinline__ uint32_t jp_excl_sum_sat(uint32_t v, uint32_t* tmp) {
  const int t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  for (int o = 1; o < JD_NT; o <<= 1) {
    const uint32_t a = t >= o ? tmp[t - o] : 0u;
    __syncthreads();
    tmp[t] = jp_sat_add(tmp[t], a);
    __syncthreads();
  }
  const uint32_t before = t > 0 ? tmp[t - 1] : 0u;
  __syncthreads();
  return before;
}

// grid: one workgroup per cut scan of the launch's level.  Segment s goes to lane s % JD_NT in every loop
// over segments, so a lane reads back its own entry and dirty flag; sums over the segments go by chunks of neighbours.
__global__ __launch_bounds__(JD_NT) void jpegprog_substream_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                                   uint8_t* scratch, int level) {
  __shared__ JdHuff s_h[3];
  __shared__ uint32_t s_tmp[JD_NT];
  __shared__ uint8_t s_zz[64];
  __shared__ uint32_t s_ok;
  const int tid = threadIdx.x;
  const JdView v(table, scratch);
  const JpHeader* ph = reinterpret_cast<const JpHeader*>(table + jp_header_off(v.hdr->B, sizeof(JdImage)));
  const JpScan* scans = reinterpret_cast<const JpScan*>(table + ph->off_scans);
  JpSyncView y;
  if (!jp_sync_view(v, ph, table, scratch, y) || level < 0 || level >= ph->nlevels) return;
  const uint32_t w = y.sh->level_cut0[level] + blockIdx.x;
  if (w >= y.sh->level_cut0[level + 1] || w >= (uint32_t)ph->nscans) return;
  const uint32_t si = y.sy[w].cut;
  if (si >= (uint32_t)ph->nscans) return;
  const JpScan* sc = scans + si;
  const JpSync sub = y.sy[si];
  if (sc->image >= (uint32_t)v.hdr->B || sub.nseg < 2u || sub.nseg > JP_SYNC_MAX_SEGS || sc->nunits != 1u || sub.slot >= (uint32_t)ph->nscans) return;
  const JdImage* im = v.images + sc->image;
  if (v.states[sc->image].st_scan != 0) return;               // (uniform) the info record already says "not accepted"
  const uint32_t off = sc->off < im->stream_len ? sc->off : im->stream_len, n = im->stream_len - off;
  const uint32_t* pstarts = reinterpret_cast<const uint32_t*>(scratch + ph->starts_off) + sc->unit0;
  uint32_t uend = pstarts[ph->total_units];
  if (uend > n) uend = n;
  const uint32_t nseg = sub.nseg, S = sub.segment_bytes;
  if ((uint64_t)nseg * S < uend) return;                      // (uniform) never: the plan's length is the marker walk's
  const uint32_t kind = sc->kind, se = sc->se < 63u ? sc->se : 63u, ss = sc->ss < se ? sc->ss : se;
  const int ntab = kind == JP_DC_FIRST ? 3 : kind == JP_DC_REFINE ? 0 : 1;
  for (int c = 0; c < ntab; ++c) {
    if (tid == 0) jd_huff_ranges(s_h[c], sc->counts[c]);
    jd_huff_clear(s_h[c], sc->symbols[c], jd_nsym(sc->counts[c]), tid, JD_NT);
  }
  if (tid < 64) s_zz[tid] = JD_ZIGZAG[tid];
  if (tid == 0) s_ok = 0;
  __syncthreads();
  for (int c = 0; c < ntab; ++c) jd_huff_fill(s_h[c], sc->counts[c], tid, JD_NT);
  __syncthreads();
  // the stream is read in place: p is the dword in front of the scan's first byte, lo that byte's offset in it
  const uint8_t* data = stream + im->stream_off + off;
  const uint32_t lo = (uint32_t)(reinterpret_cast<uintptr_t>(data) & 3u);
  const uint8_t* p = data - lo;
  JpSeg* seg = reinterpret_cast<JpSeg*>(scratch + sub.seg_off);
  int16_t* coef = reinterpret_cast<int16_t*>(scratch + im->coef_off);
  const uint32_t nslot = sc->nslot >= 1u && sc->nslot <= 6u ? sc->nslot : 1u;
  const uint64_t nblk = (uint64_t)sc->nmcu * nslot;
  const uint32_t expected = nblk < JP_SYNC_CAP ? (uint32_t)nblk : JP_SYNC_CAP - 1u;        // (the planner: fewer than 2^24 blocks)
  const uint32_t chunk = (nseg + JD_NT - 1) / JD_NT;
  const uint32_t s0 = min((uint32_t)tid * chunk, nseg), s1 = min(s0 + chunk, nseg);
  uint32_t rounds = 0, total;
  bool accepted = false;
  const uint64_t t0 = wall_clock64();                        // (lane 0's stamps go into the scan's record: 100 MHz)
  uint64_t t1 = t0, t2 = t0;
  if (kind == JP_DC_FIRST || kind == JP_AC_FIRST) {
    for (uint32_t s = tid; s < nseg; s += JD_NT) {
      JdSync e = jd_segment_guess(data, s, S, uend);
      if (kind == JP_AC_FIRST) e.bsk = ss;
      seg[s].entry = e;
      seg[s].dirty = 1u;
    }
    bool converged = false;
    while (rounds < sub.max_rounds) {                        // (uniform)
      ++rounds;
      for (uint32_t s = tid; s < nseg; s += JD_NT)
        if (seg[s].dirty) {
          JpSeg r;
          jp_first_segment(*sc, p, lo, seg[s].entry, jd_segment_end(s, S, uend), uend, s_h, r);
          seg[s].exit = r.exit;
          seg[s].nbeg = r.nbeg; seg[s].nend = r.nend; seg[s].eclean = r.eclean;
          seg[s].dc[0] = r.dc[0]; seg[s].dc[1] = r.dc[1]; seg[s].dc[2] = r.dc[2];
        }
      __syncthreads();                                       // every exit of this round is written
      int changed = 0;
      for (uint32_t s = tid; s < nseg; s += JD_NT) {
        uint32_t d = 0;
        if (s > 0) {
          const JdSync e = seg[s - 1].exit;
          if (!jd_sync_equal(e, seg[s].entry)) { seg[s].entry = e; d = 1u; changed = 1; }
        }
        seg[s].dirty = d;
      }
      if (!__syncthreads_or(changed)) { converged = true; break; }
    }
    t1 = wall_clock64();
    // exclusive sums of (blocks ended, DC differences) over the segments
    uint32_t sum[4] = {0, 0, 0, 0};
    for (uint32_t s = s0; s < s1; ++s) {
      sum[0] = jp_sat_add(sum[0], seg[s].nend);
      sum[1] += seg[s].dc[0]; sum[2] += seg[s].dc[1]; sum[3] += seg[s].dc[2];
    }
    sum[0] = jp_excl_sum_sat(sum[0], s_tmp);
    for (int e = 1; e < 4; ++e) sum[e] = jd_excl_sum(sum[e], s_tmp, total);
    uint32_t flags = 0;
    for (uint32_t s = s0; s < s1; ++s) {
      const JpSeg r = seg[s];
      seg[s].before = sum[0];
      seg[s].pred[0] = sum[1]; seg[s].pred[1] = sum[2]; seg[s].pred[2] = sum[3];
      flags |= jp_first_check(*sc, r.entry, r, sum[0], expected);
      sum[0] = jp_sat_add(sum[0], r.nend);
      sum[1] += r.dc[0]; sum[2] += r.dc[1]; sum[3] += r.dc[2];
    }
    const int bad = __syncthreads_or((int)(flags & 1u));
    const int found = __syncthreads_or((int)(flags & 2u));     // (and every `before` and predictor is written)
    accepted = converged && found && !bad;
    t2 = wall_clock64();
    if (accepted)                                            // (uniform)
      for (uint32_t s = tid; s < nseg; s += JD_NT) {
        const JpSeg e = seg[s];
        jp_first_write(*sc, *im, p, lo, e.entry, jd_segment_end(s, S, uend), uend, s_h, e.before, e.pred, expected, s_zz, coef);
      }
  } else {
    // the data bytes of every segment and of everything in front of it
    for (uint32_t s = tid; s < nseg; s += JD_NT) {
      const uint64_t b = (uint64_t)s * S;
      seg[s].nbeg = jp_data_bytes(data, b < uend ? (uint32_t)b : uend, jd_segment_end(s, S, uend));
    }
    __syncthreads();
    uint32_t bytes = 0;
    for (uint32_t s = s0; s < s1; ++s) bytes += seg[s].nbeg;
    bytes = jd_excl_sum(bytes, s_tmp, total);
    for (uint32_t s = s0; s < s1; ++s) {
      seg[s].pred[1] = bytes;
      bytes += seg[s].nbeg;
    }
    __syncthreads();
    if (kind == JP_DC_REFINE) {
      t1 = t2 = wall_clock64();
      accepted = (uint64_t)total * 8u >= expected;
      if (accepted)
        for (uint32_t s = tid; s < nseg; s += JD_NT) {
          const uint64_t b = (uint64_t)s * S;
          jp_dc_refine_write(*sc, *im, data, b < uend ? (uint32_t)b : uend, jd_segment_end(s, S, uend), seg[s].pred[1], expected, coef);
        }
    } else {
      // phase 1: the history masks of the scan's blocks and the bits set in front of each
      uint64_t* masks = reinterpret_cast<uint64_t*>(scratch + sub.mask_off);
      uint32_t* P = reinterpret_cast<uint32_t*>(masks + sc->nmcu);
      const uint32_t bchunk = (expected + JD_NT - 1) / JD_NT;
      const uint32_t b0 = min((uint32_t)tid * bchunk, expected), b1 = min(b0 + bchunk, expected);
      uint32_t bits = 0;
      for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t bi = jp_ac_block_index(*im, *sc, b);
        const uint64_t m = bi < im->nblocks ? jp_refine_mask(coef + (size_t)bi * 64u, ss, se, s_zz) : 0u;
        masks[b] = m;
        bits += jp_popc64(m);
      }
      bits = jd_excl_sum(bits, s_tmp, total);
      for (uint32_t b = b0; b < b1; ++b) {
        P[b] = bits;
        bits += jp_popc64(masks[b]);
      }
      if (tid == 0) P[expected] = total;
      __syncthreads();
      t1 = wall_clock64();
      // phase 2: the exact skim by one lane
      if (tid == 0) s_ok = jp_refine_skim(*sc, p, lo, uend, s_h[0], masks, P, expected, seg, nseg) ? 1u : 0u;
      __syncthreads();
      accepted = s_ok != 0;
      t2 = wall_clock64();
      // phase 3: every segment from its true entry up to the next one's
      if (accepted)                                          // (uniform)
        for (uint32_t s = tid; s < nseg; s += JD_NT) {
          const uint32_t n1 = s + 1u < nseg ? seg[s + 1u].before : expected, k1 = s + 1u < nseg ? seg[s + 1u].entry.bsk & 63u : ss;
          const JpSeg e = seg[s];
          jp_refine_write(*sc, *im, p, lo, jd_segment_guess(data, s, S, uend).byte, uend, s_h[0], e, n1, k1, masks, expected, s_zz, coef);
        }
    }
  }
  __syncthreads();                                           // every lane's write is done
  if (tid == 0) {
    const uint64_t t3 = wall_clock64();
    JpSyncInfo info;
    info.route = 1u + kind; info.nseg = nseg; info.rounds = rounds; info.accepted = accepted ? 1u : 0u;
    info.ticks[0] = (uint32_t)(t1 - t0); info.ticks[1] = (uint32_t)(t2 - t1); info.ticks[2] = (uint32_t)(t3 - t2); info.pad = 0;
    y.infos[sub.slot] = info;
  }
}

// ---- every layout of a sequential file (attwarp_jpegdec_plan_layouts / attwarp_jpegdec_decode_layouts): the five
// launches of the baseline family over JfImage records: up to four components of any sampling, a block-slot map of the MCU,
// four DC predictors, four quantisation tables, the up-sampler libjpeg picks per component and four colour rules ----------------
__global__ __launch_bounds__(JD_NT) void jpegfmt_scan_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                             uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_tmp[JD_NT], s_term, s_bad;
  const JfView v(table, scratch);
  jd_scan_image(v, stream, (int)blockIdx.x, s_tmp, s_term, s_bad);
}

// The code tables of an image's components in LDS, by all lanes of the workgroup; ends behind a barrier.
__device__ __forceinline__ void jf_build_tables(JdHuff* s_dc, JdHuff* s_ac, const JfImage* im, int ncomp, int tid, int nt) {
  for (int c = 0; c < ncomp; ++c) {
    if (tid == 0) { jd_huff_ranges(s_dc[c], im->dc_counts[c]); jd_huff_ranges(s_ac[c], im->ac_counts[c]); }
    jd_huff_clear(s_dc[c], im->dc_symbols[c], jd_nsym(im->dc_counts[c]), tid, nt);
    jd_huff_clear(s_ac[c], im->ac_symbols[c], jd_nsym(im->ac_counts[c]), tid, nt);
  }
  __syncthreads();
  for (int c = 0; c < ncomp; ++c) {
    jd_huff_fill(s_dc[c], im->dc_counts[c], tid, nt);
    jd_huff_fill(s_ac[c], im->ac_counts[c], tid, nt);
  }
  __syncthreads();
}

// grid: one workgroup per image planned for sub-streams (at least one).  jpegdec_substream_kernel over the general MCU: the
// slot of a JdSync runs to the period of the image's MCU (up to 10 blocks; JfLayout), a segment carries the DC sums of its
// owned blocks by their place and four predictors.
__global__ __launch_bounds__(JD_NT) void jpegfmt_substream_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                                  uint8_t* scratch) {
  __shared__ JdHuff s_dc[JF_MAX_COMP], s_ac[JF_MAX_COMP];
  __shared__ int16_t s_blk[JD_NT][JD_SUB_BLK];
  __shared__ uint32_t s_tmp[JD_NT];
  __shared__ uint8_t s_zz[64];
  const int tid = threadIdx.x;
  const JfView v(table, scratch);
  if ((int)blockIdx.x >= v.hdr->reserved) return;
  const int b = v.subs[blockIdx.x].image;
  if (b < 0 || b >= v.hdr->B) return;
  const JfImage* im = v.images + b;
  const JdSub sub = v.subs[b];
  if (v.states[b].st_scan != 0 || sub.nseg == 0) return;      // (uniform) the info record already says "not accepted"
  const uint32_t n = im->stream_len, nseg = sub.nseg, S = sub.segment_bytes;
  uint32_t uend = v.ends[im->unit0];
  if (uend > n) uend = n;
  const int ncomp = min(max(im->ncomp, 1), JF_MAX_COMP);
  if (tid < 64) s_zz[tid] = JD_ZIGZAG[tid];
  jf_build_tables(s_dc, s_ac, im, ncomp, tid, JD_NT);
  const uint8_t* data = stream + im->stream_off;
  const uint32_t lo = (uint32_t)(reinterpret_cast<uintptr_t>(data) & 3u);
  const uint8_t* p = data - lo;
  JfSegState* seg = reinterpret_cast<JfSegState*>(scratch + sub.seg_off);
  JfSegment* res = reinterpret_cast<JfSegment*>(scratch + sub.seg_off + (uint64_t)nseg * sizeof(JfSegState));
  const uint32_t nblk = (uint32_t)min(max(im->nslot, 1), JF_MAX_SLOTS);
  const uint32_t expected = (uint32_t)im->mcux * (uint32_t)im->mcuy * nblk;
  const JfLayout lay{*im};
  for (uint32_t s = tid; s < nseg; s += JD_NT) {               // (segment s belongs to lane s % JD_NT in every loop below)
    seg[s].entry = jd_segment_guess(data, s, S, uend);
    seg[s].dirty = 1u;
  }
  uint32_t rounds = 0;
  bool converged = false;
  while (rounds < sub.max_rounds) {                          // (uniform)
    ++rounds;
    for (uint32_t s = tid; s < nseg; s += JD_NT)
      if (seg[s].dirty) {
        JfSegment r;
        r.pad = 0;
        jd_decode_segment_of(lay, p, lo, seg[s].entry, jd_segment_end(s, S, uend), uend, s_dc, s_ac, nblk, r);
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
  // exclusive sums over the segments, lane t over its chunk in order: first the owned blocks, which give every segment the
  // blocks in front of it and with them the component of each of its owned blocks; then the DC differences per component
  const uint32_t chunk = (nseg + JD_NT - 1) / JD_NT;
  const uint32_t s0 = min((uint32_t)tid * chunk, nseg), s1 = min(s0 + chunk, nseg);
  uint32_t own = 0, total;
  for (uint32_t s = s0; s < s1; ++s) own += res[s].owned;
  const uint32_t own0 = jd_excl_sum(own, s_tmp, total);
  uint32_t sum[JF_MAX_COMP] = {0, 0, 0, 0}, before = own0;
  for (uint32_t s = s0; s < s1; ++s) {
    const JfSegment r = res[s];
    for (uint32_t i = 0; i < nblk; ++i) sum[lay.comp((before + i) % nblk)] += r.dc[i];
    before += r.owned;
  }
  for (int e = 0; e < JF_MAX_COMP; ++e) sum[e] = jd_excl_sum(sum[e], s_tmp, total);
  uint32_t flags = 0;
  before = own0;
  for (uint32_t s = s0; s < s1; ++s) {
    const JfSegment r = res[s];
    seg[s].before = before;
    for (int c = 0; c < JF_MAX_COMP; ++c) seg[s].pred[c] = sum[c];
    flags |= jd_segment_check(seg[s].entry, r, before, expected, nblk, lay.period(nblk));
    for (uint32_t i = 0; i < nblk; ++i) sum[lay.comp((before + i) % nblk)] += r.dc[i];
    before += r.owned;
  }
  const int bad = __syncthreads_or((int)(flags & 1u));
  const int found = __syncthreads_or((int)(flags & 2u));       // (and every `before` and predictor is written)
  bool accepted = converged && found && !bad;
  if (accepted) {                                            // (uniform)
    int16_t* coef = reinterpret_cast<int16_t*>(scratch + im->coef_off);
    uint32_t werr = 0;
    for (uint32_t s = tid; s < nseg; s += JD_NT) {
      const JfSegState e = seg[s];
      werr |= jd_write_segment_of(lay, p, lo, e.entry, uend, s_dc, s_ac, nblk, e.before, e.pred, res[s].owned, expected, s_blk[tid], s_zz, coef);
    }
    if (__syncthreads_or((int)werr)) accepted = false;       // (never, after the checks: the sequential decode then redoes it)
  }
  if (tid == 0) {
    JdSubInfo info;
    info.nseg = nseg; info.rounds = rounds; info.accepted = accepted ? 1u : 0u; info.pad = 0;
    v.infos[b] = info;
  }
}

// grid: one wave per planned unit of the call: jpegdec_entropy_kernel over the general MCU.
__global__ __launch_bounds__(WAVE) void jpegfmt_entropy_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                               uint8_t* __restrict__ scratch) {
  __shared__ JdHuff s_dc[JF_MAX_COMP], s_ac[JF_MAX_COMP];
  __shared__ uint32_t s_ring[JD_RING / 4];
  __shared__ int16_t s_blk[64];
  __shared__ int32_t s_pred[JF_MAX_COMP];
  __shared__ uint8_t s_zz[64], s_slot_c[16];
  __shared__ uint32_t s_pos, s_err;
  const int lane = threadIdx.x, u = blockIdx.x;
  const JfView v(table, scratch);
  const int b = v.find(&JfImage::unit0, u);
  const JfImage* im = v.images + b;
  JdState* state = v.states + b;
  if (state->st_scan != 0) return;                           // (uniform) the units' limits were never written
  if (v.infos[b].accepted != 0) return;                      // (uniform) the sub-stream kernel decoded this image's only unit
  const uint32_t k = (uint32_t)(u - im->unit0), n = im->stream_len;
  const int ncomp = min(max(im->ncomp, 1), JF_MAX_COMP);
  uint32_t start = v.starts[u], end = v.ends[u];
  if (end > n) end = n;
  if (start > end) start = end;
  s_zz[lane] = JD_ZIGZAG[lane];
  if (lane < 16) s_slot_c[lane] = lane < 12 ? (im->slot_c[lane] & 3u) : 0u;
  if (lane == 0) { s_pos = start; s_err = 0; }
  if (lane < JF_MAX_COMP) s_pred[lane] = 0;
  jf_build_tables(s_dc, s_ac, im, ncomp, lane, WAVE);
  const JD_G uint8_t* s = (const JD_G uint8_t*)stream + im->stream_off;
  JD_G int16_t* coef = (JD_G int16_t*)(scratch + im->coef_off);
  const int nslot = min(max(im->nslot, 1), JF_MAX_SLOTS);
  const uint32_t mcux = (uint32_t)im->mcux, nblocks = im->nblocks;
  const uint32_t nmcu = mcux * (uint32_t)im->mcuy, ri = (uint32_t)im->ri;
  const uint32_t m0 = k * ri, m1 = m0 + ri < nmcu ? m0 + ri : nmcu;
  JdBits br;
  br.init(reinterpret_cast<const uint8_t*>(s_ring), JD_RING - 1, start, end);
  uint32_t loaded = start & ~3u, err = 0;
  uint32_t my = m0 / mcux, mx = m0 - my * mcux;
  for (uint32_t m = m0; m < m1 && !err; ++m) {
    for (int jb = 0; jb < nslot; ++jb) {
      __syncthreads();                                       // s_pos of the block before
      jd_ring_fill(s_ring, s, loaded, s_pos & ~3u, end, lane);   // (the ring's bound is per block: jpegdec_entropy_kernel)
      s_blk[lane] = 0;
      __syncthreads();
      if (lane == 0) {
        br.end = loaded < end ? loaded : end;
        const int c = s_slot_c[jb];
        int32_t p = s_pred[c];
        const uint32_t st = jd_decode_block(br, s_dc[c], s_ac[c], p, s_blk, s_zz);
        s_pred[c] = p;
        s_pos = br.pos;
        if (st) s_err = st;
      }
      __syncthreads();
      err = s_err;
      if (err) break;                                        // (uniform)
      const uint32_t bi = jf_slot_block(*im, (uint32_t)jb, mx, my);
      if (bi < nblocks) coef[(size_t)bi * 64u + lane] = s_blk[lane];
    }
    if (++mx == mcux) { mx = 0; ++my; }
  }
  if (err && lane == 0) atomicMin(&state->fail, k << 8 | err);
}

// One thread per 8x8 block of up to four planes, four quantisation tables in LDS.
__global__ __launch_bounds__(JD_NT) void jpegfmt_idct_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  __shared__ uint16_t s_qt[JF_MAX_COMP][64];
  const JfView v(table, scratch);
  const int b = v.find(&JfImage::idct_tile0, (int)blockIdx.x);
  const JfImage* im = v.images + b;
  s_qt[threadIdx.x >> 6][threadIdx.x & 63] = im->qt[threadIdx.x >> 6][threadIdx.x & 63];
  __syncthreads();
  const uint32_t bi = (uint32_t)((int)blockIdx.x - im->idct_tile0) * JD_IDCT_TILE + threadIdx.x;
  if (bi >= im->nblocks) return;
  int c = 0;
  for (int e = 1; e < JF_MAX_COMP; ++e)
    if (e < im->ncomp && bi >= im->comp[e].block0) c = e;
  const JfComp& k = im->comp[c];
  const uint32_t local = bi - k.block0, bw = (uint32_t)k.bw, by = local / bw, bx = local - by * bw;
  jd_idct_block(reinterpret_cast<const uint4*>(scratch + im->coef_off + (size_t)bi * 128u), s_qt[c],
                scratch + im->plane_off + (size_t)k.block0 * 64u + (size_t)by * 8u * ((size_t)bw * 8u) + (size_t)bx * 8u, (size_t)bw * 8u);
}

// One thread per output pixel (eight pixels, a workgroup apart): every component up-sampled by its own rule (uniform per
// image), the colour rule, Pillow's conversion, the store; the first thread of every image writes its status.
__global__ __launch_bounds__(JD_NT) void jpegfmt_color_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ scratch,
                                                              const JdState* __restrict__ states, uint8_t* __restrict__ out,
                                                              int32_t* __restrict__ status) {
  __shared__ JfComp s_comp[JF_MAX_COMP];
  const attwarp_jpegdec_header* hdr = reinterpret_cast<const attwarp_jpegdec_header*>(table);
  const JfImage* images = reinterpret_cast<const JfImage*>(table + hdr->off_images);
  int lo = 0, hi = hdr->B - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (images[mid].color_tile0 <= (int)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const int b = lo;
  const JfImage* im = images + b;
  const int tile = (int)blockIdx.x - im->color_tile0;
  if (tile == 0 && threadIdx.x == 0) {
    const JdState st = states[b];
    status[b] = jd_status(st);
  }
  if (threadIdx.x < JF_MAX_COMP) s_comp[threadIdx.x] = im->comp[threadIdx.x];
  __syncthreads();
  const int W = im->W, oc = min(max(im->oc, 1), 4), ncomp = min(max(im->ncomp, 1), JF_MAX_COMP);
  const int color = im->color, conv = im->conv;
  const bool swap = im->swap != 0;
  const uint32_t npx = (uint32_t)W * (uint32_t)im->H;
  const uint8_t* planes = scratch + im->plane_off;
  JD_G uint8_t* o = (JD_G uint8_t*)out + im->out_off;
  for (int j = 0; j < JD_CPX; ++j) {
    const uint32_t px = (uint32_t)tile * JD_COLOR_TILE + (uint32_t)j * JD_NT + threadIdx.x;
    if (px >= npx) break;
    const int y = (int)(px / (uint32_t)W), x = (int)(px - (uint32_t)y * (uint32_t)W);
    int32_t smp[JF_MAX_COMP] = {0, 0, 0, 0};
    for (int c = 0; c < ncomp; ++c) smp[c] = jf_sample(planes + (size_t)s_comp[c].block0 * 64u, s_comp[c].bw * 8, s_comp[c], x, y);
    uint8_t q[4] = {0, 0, 0, 0};
    jf_pixel(color, conv, swap, smp, q);
    JD_G uint8_t* d = o + (size_t)px * oc;
    for (int e = 0; e < oc; ++e) d[e] = q[e];
  }
}

// ---- scans of every layout (attwarp_jpegdec_plan_layout_scans / attwarp_jpegdec_decode_layout_scans): a table of
// attwarp_jpegdec_plan_layouts for B one-unit images (all the IDCT and colour kernels read; its magic replaced, so that
// attwarp_jpegdec_decode_layouts refuses it) with a JsHeader and the JsScan records behind it, sorted by (level, image, position) ---
constexpr uint32_t JS_MAGIC = JD_MAGIC_LAYOUT_SCANS, JS_MAGIC_SCANS = 0x4745504eu;   // of the table's first header / of the JsHeader
// The sub-stream records of a table planned with them (behind the JsScan records) and the per-scan results in scratch.
struct JsSyncView {
  const JsSyncHeader* sh;
  const JsSync* sy;
  JpSyncInfo* infos;
};
__device__ __forceinline__ bool js_sync_view(const JfView& v, const JpHeader* ph, const uint8_t* table, uint8_t* scratch, JsSyncView& y) {
  const uint64_t at = ph->off_scans + (uint64_t)ph->nscans * sizeof(JsScan);
  if (v.hdr->table_bytes < at + sizeof(JsSyncHeader) + (uint64_t)ph->nscans * sizeof(JsSync)) return false;   // planned without them
  y.sh = reinterpret_cast<const JsSyncHeader*>(table + at);
  y.sy = reinterpret_cast<const JsSync*>(table + at + sizeof(JsSyncHeader));
  y.infos = reinterpret_cast<JpSyncInfo*>(scratch + y.sh->info_off);
  return y.sh->magic == JS_SYNC_MAGIC;
}
__global__ __launch_bounds__(JD_NT) void jpegscan_clear_kernel(const uint8_t* __restrict__ table, uint8_t* __restrict__ scratch) {
  const JfView v(table, scratch);
  const JpHeader* sh = reinterpret_cast<const JpHeader*>(table + jp_header_off(v.hdr->B, sizeof(JfImage)));
  jp_clear_body(v, scratch, sh->clear_off, sh->clear_bytes);
  JsSyncView y;
  if (!js_sync_view(v, sh, table, scratch, y)) return;
  const JsScan* scans = reinterpret_cast<const JsScan*>(table + sh->off_scans);
  for (int i = (int)(blockIdx.x * JD_NT + threadIdx.x); i < sh->nscans; i += (int)(gridDim.x * JD_NT)) {
    JpSyncInfo info;
    info.route = y.sy[i].nseg ? 1u + scans[i].kind : 0u; info.nseg = y.sy[i].nseg; info.rounds = 0; info.accepted = 0;
    info.ticks[0] = info.ticks[1] = info.ticks[2] = 0; info.pad = 0;
    if (y.sy[i].slot < (uint32_t)sh->nscans) y.infos[y.sy[i].slot] = info;
  }
}

// grid: one workgroup per SCAN.
__global__ __launch_bounds__(JD_NT) void jpegscan_marks_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                               uint8_t* __restrict__ scratch) {
  __shared__ uint32_t s_tmp[JD_NT], s_term, s_bad;
  const JfView v(table, scratch);
  const JpHeader* sh = reinterpret_cast<const JpHeader*>(table + jp_header_off(v.hdr->B, sizeof(JfImage)));
  jp_marks_body(v, reinterpret_cast<const JsScan*>(table + sh->off_scans) + blockIdx.x, stream,
                reinterpret_cast<uint32_t*>(scratch + sh->starts_off), sh->total_units, s_tmp, s_term, s_bad);
}

// grid: one wave per (scan, unit) of the launch's level: jpegprog_entropy_kernel over the general MCU (up to ten slots, four
// predictors) with a fifth kind of block, the sequential one, whose scan names a DC and an AC table per component (eight
// tables in LDS at most).  The band rule holds: only zigzag positions Ss..Se are stored (DC: position 0), which is the whole
// row for a sequential scan, and such a scan never shares a block with another scan of its level: every component of a
// sequential file is sent once.  The code tables live in dynamic LDS, ntab of them (the most a scan of this level names:
// 1 for AC scans, up to 4 for a DC first pass, up to 8 for a sequential scan), so that a level of AC scans keeps 8 waves
// per SIMD; a scan that names more than the launch holds is not decoded (the planner never writes such a level).
__global__ __launch_bounds__(WAVE) void jpegscan_entropy_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                                uint8_t* scratch, int level, int ntab) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  __shared__ uint32_t s_ring[JD_RING / 4];
  __shared__ int16_t s_blk[64];
  __shared__ int32_t s_pred[JF_MAX_COMP];
  __shared__ uint8_t s_zz[64], s_slot_t[16];
  __shared__ uint32_t s_pos, s_err, s_run;
  const int lane = threadIdx.x, w = blockIdx.x;
  const JfView v(table, scratch);
  const JpHeader* sh = reinterpret_cast<const JpHeader*>(table + jp_header_off(v.hdr->B, sizeof(JfImage)));
  const JsScan* scans = reinterpret_cast<const JsScan*>(table + sh->off_scans);
  if (level < 0 || level >= ATTWARP_JPEGDEC_MAX_SCANS) return;
  int lo = sh->level_scan0[level], hi = sh->level_scan0[level + 1] - 1;
  if (hi < lo || lo < 0 || hi >= sh->nscans) return;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (scans[mid].wave0 <= (uint32_t)w) lo = mid;
    else hi = mid - 1;
  }
  const JsScan* sc = scans + lo;
  if (sc->image >= (uint32_t)v.hdr->B) return;
  const JfImage* im = v.images + sc->image;
  JdState* state = v.states + sc->image;
  if (state->st_scan != 0) return;                           // (uniform) some scan's limits were never written
  JsSyncView y;
  if (js_sync_view(v, sh, table, scratch, y) && y.sy[lo].slot < (uint32_t)sh->nscans && y.infos[y.sy[lo].slot].accepted != 0)
    return;                                                  // (uniform) the sub-stream kernel decoded this scan's only unit
  const uint32_t k = (uint32_t)w - sc->wave0;
  if (k >= sc->nunits) return;
  const uint32_t off = sc->off < im->stream_len ? sc->off : im->stream_len, n = im->stream_len - off;
  const uint32_t* pstarts = reinterpret_cast<const uint32_t*>(scratch + sh->starts_off) + sc->unit0;
  uint32_t start = pstarts[k], end = pstarts[sh->total_units + k];
  if (end > n) end = n;
  if (start > end) start = end;
  const uint32_t kind = sc->kind <= JS_SEQUENTIAL ? sc->kind : JS_SEQUENTIAL;
  const uint32_t ss = sc->ss < 63u ? sc->ss : 63u, se = sc->se < 63u ? sc->se : 63u, al = sc->al < 15u ? sc->al : 15u;
  const int nc = (int)(sc->ncomp >= 1u && sc->ncomp <= (uint32_t)JF_MAX_COMP ? sc->ncomp : 1u);
  const int ndc = kind == JS_SEQUENTIAL || kind == JP_DC_FIRST ? nc : 0;                  // (uniform: the scan's)
  const int nac = kind == JS_SEQUENTIAL ? nc : kind >= JP_AC_FIRST ? 1 : 0;
  if (ndc + nac > ntab) return;                              // (uniform)
  JdHuff* s_dc = reinterpret_cast<JdHuff*>(s_dyn);
  JdHuff* s_ac = s_dc + ndc;
  for (int c = 0; c < ndc; ++c) {
    if (lane == 0) jd_huff_ranges(s_dc[c], sc->dc_counts[c]);
    jd_huff_clear(s_dc[c], sc->dc_symbols[c], jd_nsym(sc->dc_counts[c]), lane, WAVE);
  }
  for (int c = 0; c < nac; ++c) {
    if (lane == 0) jd_huff_ranges(s_ac[c], sc->ac_counts[c]);
    jd_huff_clear(s_ac[c], sc->ac_symbols[c], jd_nsym(sc->ac_counts[c]), lane, WAVE);
  }
  s_zz[lane] = JD_ZIGZAG[lane];
  if (lane < 16) s_slot_t[lane] = lane < 12 && (int)(sc->slot_t[lane] & 3u) < nc ? (sc->slot_t[lane] & 3u) : 0u;   // (below the tables built)
  if (lane == 0) { s_pos = start; s_err = 0; s_run = 0; }
  if (lane < JF_MAX_COMP) s_pred[lane] = 0;
  __syncthreads();
  for (int c = 0; c < ndc; ++c) jd_huff_fill(s_dc[c], sc->dc_counts[c], lane, WAVE);
  for (int c = 0; c < nac; ++c) jd_huff_fill(s_ac[c], sc->ac_counts[c], lane, WAVE);
  const JD_G uint8_t* s = (const JD_G uint8_t*)stream + im->stream_off + off;
  JD_G int16_t* coef = (JD_G int16_t*)(scratch + im->coef_off);
  const uint32_t nslot = js_nslot(*sc), nblocks = im->nblocks;
  const uint32_t nmcu = sc->nmcu, ri = sc->ri;
  const uint32_t m0 = k * ri, m1 = m0 + ri < nmcu ? m0 + ri : nmcu;
  const uint32_t iend = m1 * nslot;
  const bool dc = kind <= JP_DC_REFINE, seq = kind == JS_SEQUENTIAL;
  JdBits br;
  br.init(reinterpret_cast<const uint8_t*>(s_ring), JD_RING - 1, start, end);
  uint32_t loaded = start & ~3u, err = 0, eobrun = 0;
  for (uint32_t i = m0 * nslot; i < iend;) {
    const uint32_t m = i / nslot, j = i - m * nslot;
    const uint32_t bi = js_block_index(*im, *sc, m, j);
    __syncthreads();                                         // s_pos of the block before; the tables the first time
    jd_ring_fill(s_ring, s, loaded, s_pos & ~3u, end, lane);  // (the ring's bound is per block: jpegdec_entropy_kernel's holds for all five kinds)
    int16_t have = 0;
    if (bi < nblocks && (kind == JP_AC_REFINE || (kind == JP_DC_REFINE && lane == 0))) have = coef[(size_t)bi * 64u + lane];
    s_blk[lane] = have;
    __syncthreads();
    if (lane == 0) {
      br.end = loaded < end ? loaded : end;
      const uint32_t st = js_decode_block(br, kind, s_dc, s_ac, s_slot_t[j & 15u], s_pred, ss, se, al, eobrun, s_blk, s_zz);
      s_pos = br.pos;
      s_run = eobrun;
      if (st) s_err = st;
    }
    __syncthreads();
    err = s_err;
    if (err) break;                                          // (uniform)
    if (bi < nblocks) {
      if (seq) coef[(size_t)bi * 64u + lane] = s_blk[lane];
      else if (dc ? lane == 0 : ((uint32_t)lane >= ss && (uint32_t)lane <= se)) {
        const uint32_t at = s_zz[lane] & 63u;
        coef[(size_t)bi * 64u + at] = s_blk[at];
      }
    }
    eobrun = s_run;
    uint32_t adv = 1;
    if (kind == JP_AC_FIRST && eobrun > 0) {                 // the blocks of the run are skipped without touching memory
      const uint32_t skip = eobrun < iend - i - 1u ? eobrun : iend - i - 1u;
      adv += skip;
      eobrun -= skip;                                        // (what is left at the unit's end is dropped with the unit)
    }
    i += adv;
  }
  if (err && lane == 0) atomicMin(&state->fail, sc->index << 24 | k << 8 | err);
}

// grid: one workgroup per cut scan of the launch's level: jpegprog_substream_kernel over the general MCU.
// Segment s goes to lane s % JD_NT in every loop over segments, so a lane reads back its own entry and dirty flag; sums over
// the segments go by chunks of neighbours.  ntab code tables in dynamic LDS (the most a cut scan of the level names: up to 4
// DC tables, 1 AC table); a scan that names more is left to the one-lane route.  s_acc: a lane's ten DC sums of the segment
// it decodes (rounds), then its four predictors (write), lane-strided so that no two lanes share a bank.
__global__ __launch_bounds__(JD_NT) void jpegscan_substream_kernel(const uint8_t* __restrict__ table, const uint8_t* __restrict__ stream,
                                                                   uint8_t* scratch, int level, int ntab) {
  extern __shared__ __align__(16) uint8_t s_tables[];
  __shared__ uint32_t s_scan[JD_NT];
  __shared__ uint32_t s_acc[JF_MAX_SLOTS * JD_NT];
  __shared__ uint8_t s_zig[64];
  __shared__ uint32_t s_good;
  const int tid = threadIdx.x;
  const JfView v(table, scratch);
  const JpHeader* ph = reinterpret_cast<const JpHeader*>(table + jp_header_off(v.hdr->B, sizeof(JfImage)));
  const JsScan* scans = reinterpret_cast<const JsScan*>(table + ph->off_scans);
  JsSyncView y;
  if (!js_sync_view(v, ph, table, scratch, y) || level < 0 || level >= ph->nlevels || level >= ATTWARP_JPEGDEC_MAX_SCANS) return;
  const uint32_t w = y.sh->level_cut0[level] + blockIdx.x;
  if (w >= y.sh->level_cut0[level + 1] || w >= (uint32_t)ph->nscans) return;
  const uint32_t si = y.sy[w].cut;
  if (si >= (uint32_t)ph->nscans) return;
  const JsScan* sc = scans + si;
  const JsSync sub = y.sy[si];
  if (sc->image >= (uint32_t)v.hdr->B || sub.nseg < 2u || sub.nseg > JP_SYNC_MAX_SEGS || sc->nunits != 1u || sub.slot >= (uint32_t)ph->nscans) return;
  const JfImage* im = v.images + sc->image;
  if (v.states[sc->image].st_scan != 0) return;               // (uniform) the info record already says "not accepted"
  const uint32_t off = sc->off < im->stream_len ? sc->off : im->stream_len, n = im->stream_len - off;
  const uint32_t* pstarts = reinterpret_cast<const uint32_t*>(scratch + ph->starts_off) + sc->unit0;
  uint32_t uend = pstarts[ph->total_units];
  if (uend > n) uend = n;
  const uint32_t nseg = sub.nseg, S = sub.segment_bytes;
  if ((uint64_t)nseg * S < uend) return;                      // (uniform) never: the plan's length is the marker walk's
  const uint32_t kind = sc->kind, se = sc->se < 63u ? sc->se : 63u, ss = sc->ss < se ? sc->ss : se;
  if (kind > JP_AC_REFINE) return;                            // (uniform) a sequential scan is never cut
  const uint32_t nslot = js_nslot(*sc);
  if (kind >= JP_AC_FIRST && (nslot != 1u || sc->ncomp != 1u)) return;       // (uniform) an AC scan holds one component
  const uint32_t nc = sc->ncomp >= 1u && sc->ncomp <= (uint32_t)JF_MAX_COMP ? sc->ncomp : 1u;
  const uint32_t nh = kind == JP_DC_FIRST ? nc : kind == JP_DC_REFINE ? 0u : 1u;
  if (ntab < 0 || nh > (uint32_t)ntab) return;                // (uniform)
  JdHuff* s_h = reinterpret_cast<JdHuff*>(s_tables);
  for (uint32_t c = 0; c < nh; ++c) {
    const uint8_t* counts = kind == JP_DC_FIRST ? sc->dc_counts[c] : sc->ac_counts[c];
    if (tid == 0) jd_huff_ranges(s_h[c], counts);
    jd_huff_clear(s_h[c], kind == JP_DC_FIRST ? sc->dc_symbols[c] : sc->ac_symbols[c], jd_nsym(counts), tid, JD_NT);
  }
  if (tid < 64) s_zig[tid] = JD_ZIGZAG[tid];
  if (tid == 0) s_good = 0;
  __syncthreads();
  for (uint32_t c = 0; c < nh; ++c) jd_huff_fill(s_h[c], kind == JP_DC_FIRST ? sc->dc_counts[c] : sc->ac_counts[c], tid, JD_NT);
  __syncthreads();
  // the stream is read in place: p is the dword in front of the scan's first byte, lo that byte's offset in it
  const uint8_t* data = stream + im->stream_off + off;
  const uint32_t lo = (uint32_t)(reinterpret_cast<uintptr_t>(data) & 3u);
  const uint8_t* p = data - lo;
  JsSeg* seg = reinterpret_cast<JsSeg*>(scratch + sub.seg_off);
  int16_t* coef = reinterpret_cast<int16_t*>(scratch + im->coef_off);
  const uint64_t nblk = (uint64_t)sc->nmcu * nslot;
  const uint32_t expected = nblk < JP_SYNC_CAP ? (uint32_t)nblk : JP_SYNC_CAP - 1u;        // (the planner: fewer than 2^24 blocks)
  const uint32_t period = js_clamp_period(*sc, sub.period);
  const uint32_t chunk = (nseg + JD_NT - 1) / JD_NT;
  const uint32_t s0 = min((uint32_t)tid * chunk, nseg), s1 = min(s0 + chunk, nseg);
  uint32_t rounds = 0, total;
  bool accepted = false;
  const uint64_t t0 = wall_clock64();                        // (lane 0's stamps go into the scan's record: 100 MHz)
  uint64_t t1 = t0, t2 = t0;
  if (kind == JP_DC_FIRST || kind == JP_AC_FIRST) {
    for (uint32_t s = tid; s < nseg; s += JD_NT) {
      JdSync e = jd_segment_guess(data, s, S, uend);
      if (kind == JP_AC_FIRST) e.bsk = ss;
      seg[s].entry = e;
      seg[s].dirty = 1u;
    }
    bool converged = false;
    while (rounds < sub.max_rounds) {                        // (uniform)
      ++rounds;
      for (uint32_t s = tid; s < nseg; s += JD_NT)
        if (seg[s].dirty) {
          JsSegOut r;
          js_first_segment(*sc, period, p, lo, seg[s].entry, jd_segment_end(s, S, uend), uend, s_h, nh, r, s_acc + tid, JD_NT);
          seg[s].exit = r.exit;
          seg[s].nbeg = r.nbeg; seg[s].nend = r.nend; seg[s].eclean = r.eclean;
          for (uint32_t i = 0; i < nslot; ++i) seg[s].dc[i] = s_acc[i * JD_NT + tid];
        }
      __syncthreads();                                       // every exit of this round is written
      int changed = 0;
      for (uint32_t s = tid; s < nseg; s += JD_NT) {
        uint32_t d = 0;
        if (s > 0) {
          const JdSync e = seg[s - 1].exit;
          if (!jd_sync_equal(e, seg[s].entry)) { seg[s].entry = e; d = 1u; changed = 1; }
        }
        seg[s].dirty = d;
      }
      if (!__syncthreads_or(changed)) { converged = true; break; }
    }
    t1 = wall_clock64();
    // the blocks in front of every segment, then the DC differences in front of it by component: two exclusive sums
    uint32_t nb = 0;
    for (uint32_t s = s0; s < s1; ++s) nb = jp_sat_add(nb, seg[s].nend);
    nb = jp_excl_sum_sat(nb, s_scan);
    uint32_t sum[JF_MAX_COMP] = {0, 0, 0, 0}, flags = 0;
    for (uint32_t s = s0; s < s1; ++s) {
      seg[s].before = nb;
      flags |= js_first_check(*sc, period, seg[s].entry, seg[s].nend, seg[s].eclean, nb, expected);
      if (kind == JP_DC_FIRST) js_component_sums(*sc, seg[s].dc, nb, sum);
      nb = jp_sat_add(nb, seg[s].nend);
    }
    for (int e = 0; e < JF_MAX_COMP; ++e) sum[e] = jd_excl_sum(sum[e], s_scan, total);
    if (kind == JP_DC_FIRST)
      for (uint32_t s = s0; s < s1; ++s) {
        for (int e = 0; e < JF_MAX_COMP; ++e) seg[s].pred[e] = sum[e];
        js_component_sums(*sc, seg[s].dc, seg[s].before, sum);
      }
    const int bad = __syncthreads_or((int)(flags & 1u));
    const int found = __syncthreads_or((int)(flags & 2u));     // (and every `before` and predictor is written)
    accepted = converged && found && !bad;
    t2 = wall_clock64();
    if (accepted)                                            // (uniform)
      for (uint32_t s = tid; s < nseg; s += JD_NT) {
        for (int e = 0; e < JF_MAX_COMP; ++e) s_acc[e * JD_NT + tid] = seg[s].pred[e];
        js_first_write(*sc, *im, p, lo, seg[s].entry, jd_segment_end(s, S, uend), uend, s_h, nh, seg[s].before, s_acc + tid, JD_NT, expected,
                       s_zig, coef);
      }
  } else {
    // the data bytes of every segment and of everything in front of it
    for (uint32_t s = tid; s < nseg; s += JD_NT) {
      const uint64_t b = (uint64_t)s * S;
      seg[s].nbeg = jp_data_bytes(data, b < uend ? (uint32_t)b : uend, jd_segment_end(s, S, uend));
    }
    __syncthreads();
    uint32_t bytes = 0;
    for (uint32_t s = s0; s < s1; ++s) bytes += seg[s].nbeg;
    bytes = jd_excl_sum(bytes, s_scan, total);
    for (uint32_t s = s0; s < s1; ++s) {
      seg[s].pred[1] = bytes;
      bytes += seg[s].nbeg;
    }
    __syncthreads();
    if (kind == JP_DC_REFINE) {
      t1 = t2 = wall_clock64();
      accepted = (uint64_t)total * 8u >= expected;
      if (accepted)
        for (uint32_t s = tid; s < nseg; s += JD_NT) {
          const uint64_t b = (uint64_t)s * S;
          js_dc_refine_write(*sc, *im, data, b < uend ? (uint32_t)b : uend, jd_segment_end(s, S, uend), seg[s].pred[1], expected, coef);
        }
    } else {
      // phase 1: the history masks of the scan's blocks and the bits set in front of each
      uint64_t* masks = reinterpret_cast<uint64_t*>(scratch + sub.mask_off);
      uint32_t* P = reinterpret_cast<uint32_t*>(masks + sc->nmcu);
      const uint32_t bchunk = (expected + JD_NT - 1) / JD_NT;
      const uint32_t b0 = min((uint32_t)tid * bchunk, expected), b1 = min(b0 + bchunk, expected);
      uint32_t bits = 0;
      for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t bi = js_block_index(*im, *sc, b, 0);
        const uint64_t m = bi < im->nblocks ? jp_refine_mask(coef + (size_t)bi * 64u, ss, se, s_zig) : 0u;
        masks[b] = m;
        bits += jp_popc64(m);
      }
      bits = jd_excl_sum(bits, s_scan, total);
      for (uint32_t b = b0; b < b1; ++b) {
        P[b] = bits;
        bits += jp_popc64(masks[b]);
      }
      if (tid == 0) P[expected] = total;
      __syncthreads();
      t1 = wall_clock64();
      // phase 2: the exact skim by one lane
      if (tid == 0) s_good = js_refine_skim(*sc, p, lo, uend, s_h[0], masks, P, expected, seg, nseg) ? 1u : 0u;
      __syncthreads();
      accepted = s_good != 0;
      t2 = wall_clock64();
      // phase 3: every segment from its true entry up to the next one's
      if (accepted)                                          // (uniform)
        for (uint32_t s = tid; s < nseg; s += JD_NT) {
          const uint32_t n1 = s + 1u < nseg ? seg[s + 1u].before : expected, k1 = s + 1u < nseg ? seg[s + 1u].entry.bsk & 63u : ss;
          js_refine_write(*sc, *im, p, lo, jd_segment_guess(data, s, S, uend).byte, uend, s_h[0], seg[s].before, seg[s].entry.bsk, seg[s].pred[0],
                          seg[s].entry.byte, n1, k1, masks, expected, s_zig, coef);
        }
    }
  }
  __syncthreads();                                           // every lane's write is done
  if (tid == 0) {
    const uint64_t t3 = wall_clock64();
    JpSyncInfo info;
    info.route = 1u + kind; info.nseg = nseg; info.rounds = rounds; info.accepted = accepted ? 1u : 0u;
    info.ticks[0] = (uint32_t)(t1 - t0); info.ticks[1] = (uint32_t)(t2 - t1); info.ticks[2] = (uint32_t)(t3 - t2); info.pad = 0;
    y.infos[sub.slot] = info;
  }
}

}  // namespace attwarp

using namespace attwarp;

// ---- the host side: planners and entry points of the four families ---------------------------------------------------------------------
// What is wrong with a Huffman table (counts per length, symbols), in words for the caller's message; nullptr: nothing.
static const char* jd_huffman_fault(const uint8_t* counts, const uint8_t* symbols, bool dc, char (&what)[48]) {
  int left = 1, n = 0;
  for (int l = 0; l < 16 && left >= 0; ++l) { left = 2 * left - counts[l]; n += counts[l]; }
  if (left < 0) return "an over-subscribed Huffman table";
  std::snprintf(what, sizeof what, "a Huffman table of %d symbols", n);
  if (n > 256) return what;
  for (int k = 0; dc && k < n; ++k)
    if (symbols[k] > 15) return "a DC category above 15";
  return nullptr;
}

// What both frames check of the quantisation and Huffman tables of component c (d: an attwarp_jpegdec_image or _layout_image).
template <class Input>
static int jd_check_tables(const Input& d, int b, int c) {
  for (int k = 0; k < 64; ++k) ATTWARP_REQUIRE(d.qt[c][k] <= 255, "jpegdec: image %d: a quantisation value above 255", b);
  for (int t = 0; t < 2; ++t) {
    char what[48];
    const char* fault = t ? jd_huffman_fault(d.ac_counts[c], d.ac_symbols[c], false, what) : jd_huffman_fault(d.dc_counts[c], d.dc_symbols[c], true, what);
    ATTWARP_REQUIRE(!fault, "jpegdec: image %d: %s", b, fault);
  }
  return ATTWARP_OK;
}
// ... and of its units, blocks and data, once the geometry is known -> r.ri, r.nunits.
template <class Input, class Image>
static int jd_check_sizes(const Input& d, int b, uint64_t blocks, Image& r) {
  const int64_t nmcu = (int64_t)r.mcux * r.mcuy;
  const int64_t units = d.restart_interval ? (nmcu + d.restart_interval - 1) / d.restart_interval : 1;
  if (units > ATTWARP_JPEGDEC_MAX_UNITS)
    return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: image %d: %lld restart intervals (> %d)", b, (long long)units, ATTWARP_JPEGDEC_MAX_UNITS);
  if (blocks >= ATTWARP_JPEGDEC_MAX_BLOCKS)
    return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: image %d: %llu blocks (>= %d)", b, (unsigned long long)blocks, ATTWARP_JPEGDEC_MAX_BLOCKS);
  if (d.stream_len >= ((uint64_t)1 << 31) || d.stream_off >= ((uint64_t)1 << 62))
    return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: image %d: entropy data of 2 GiB or more", b);
  r.ri = d.restart_interval ? d.restart_interval : (int32_t)nmcu;
  r.nunits = (int32_t)units;
  return ATTWARP_OK;
}

// A record family on the host: the caller's image type, its record, segment-state and segment types with the most components
// and block slots of an MCU, the table's magic, the planner's name in messages, and two steps per image: geom() checks everything the kernels index by
// and writes the record's geometry (nothing else of r), fill() writes what else is the family's own.  jd_plan_frames does
// the rest for both.
struct JdFrames {
  using Input = attwarp_jpegdec_image;
  using Image = JdImage;
  using SegState = JdSegState;
  using Segment = JdSegment;
  static constexpr int MAX_COMP = 3, MAX_SLOTS = 6;
  static constexpr uint32_t MAGIC = JD_MAGIC;
  static constexpr const char* PLAN = "jpegdec_plan";
  static int geom(const Input& d, int b, JdImage& r) {
    ATTWARP_REQUIRE(d.H >= 1 && d.W >= 1 && d.H <= 65535 && d.W <= 65535, "jpegdec: image %d: size %d x %d outside 1..65535", b, d.H, d.W);
    ATTWARP_REQUIRE(d.ncomp == 1 || d.ncomp == 3, "jpegdec: image %d: %d components (1 or 3)", b, d.ncomp);
    ATTWARP_REQUIRE((d.hs == 1 && d.vs == 1) || (d.ncomp == 3 && d.hs == 2 && (d.vs == 1 || d.vs == 2)),
                    "jpegdec: image %d: luma sampling %d x %d (1x1, 2x1, 2x2; grey 1x1)", b, d.hs, d.vs);
    ATTWARP_REQUIRE(d.restart_interval >= 0 && d.restart_interval <= 65535, "jpegdec: image %d: restart interval %d", b, d.restart_interval);
    ATTWARP_REQUIRE(d.mode >= ATTWARP_JPEGDEC_RGB && d.mode <= ATTWARP_JPEGDEC_KEEP, "jpegdec: image %d: unknown mode %d", b, d.mode);
    ATTWARP_REQUIRE(d.order == ATTWARP_RGB || d.order == ATTWARP_BGR, "jpegdec: image %d: channel order must be ATTWARP_RGB or ATTWARP_BGR", b);
    for (int c = 0; c < d.ncomp; ++c)
      if (const int rc = jd_check_tables(d, b, c)) return rc;
    r.H = d.H; r.W = d.W; r.ncomp = d.ncomp; r.hs = d.hs; r.vs = d.vs;
    r.mcux = (d.W + 8 * d.hs - 1) / (8 * d.hs);
    r.mcuy = (d.H + 8 * d.vs - 1) / (8 * d.vs);
    int64_t blocks = 0;
    for (int c = 0; c < 3; ++c) {
      r.bw[c] = c < d.ncomp ? r.mcux * (c == 0 ? d.hs : 1) : 0;
      r.bh[c] = c < d.ncomp ? r.mcuy * (c == 0 ? d.vs : 1) : 0;
      r.block0[c] = (uint32_t)blocks;
      blocks += (int64_t)r.bw[c] * r.bh[c];
    }
    r.nblocks = (uint32_t)blocks;
    return jd_check_sizes(d, b, (uint64_t)blocks, r);
  }
  static void fill(const Input& d, JdImage& r) {
    r.to_luma = d.ncomp == 3 && r.oc == 1;
    r.swap = d.ncomp == 3 && r.oc == 3 && d.order == ATTWARP_BGR;
    std::memcpy(r.qt, d.qt, sizeof r.qt);
    std::memcpy(r.dc_counts, d.dc_counts, sizeof r.dc_counts);
    std::memcpy(r.ac_counts, d.ac_counts, sizeof r.ac_counts);
    std::memcpy(r.dc_symbols, d.dc_symbols, sizeof r.dc_symbols);
    std::memcpy(r.ac_symbols, d.ac_symbols, sizeof r.ac_symbols);
  }
};
struct JfFrames {
  using Input = attwarp_jpegdec_layout_image;
  using Image = JfImage;
  using SegState = JfSegState;
  using Segment = JfSegment;
  static constexpr int MAX_COMP = JF_MAX_COMP, MAX_SLOTS = JF_MAX_SLOTS;
  static constexpr uint32_t MAGIC = JD_MAGIC_LAYOUTS;
  static constexpr const char* PLAN = "jpegdec_plan_layouts";
  static int geom(const Input& d, int b, JfImage& r) {
    ATTWARP_REQUIRE(d.H >= 1 && d.W >= 1 && d.H <= 65535 && d.W <= 65535, "jpegdec: image %d: size %d x %d outside 1..65535", b, d.H, d.W);
    ATTWARP_REQUIRE(d.ncomp == 1 || d.ncomp == 3 || d.ncomp == 4, "jpegdec: image %d: %d components (1, 3 or 4)", b, d.ncomp);
    ATTWARP_REQUIRE(d.restart_interval >= 0 && d.restart_interval <= 65535, "jpegdec: image %d: restart interval %d", b, d.restart_interval);
    ATTWARP_REQUIRE(d.mode >= ATTWARP_JPEGDEC_RGB && d.mode <= ATTWARP_JPEGDEC_KEEP, "jpegdec: image %d: unknown mode %d", b, d.mode);
    ATTWARP_REQUIRE(d.order == ATTWARP_RGB || d.order == ATTWARP_BGR, "jpegdec: image %d: channel order must be ATTWARP_RGB or ATTWARP_BGR", b);
    for (int c = 0; c < d.ncomp; ++c) {
      ATTWARP_REQUIRE(d.h[c] >= 1 && d.h[c] <= 4 && d.v[c] >= 1 && d.v[c] <= 4, "jpegdec: image %d: component %d: sampling factors %d x %d outside 1..4",
                      b, c, d.h[c], d.v[c]);
      if (const int rc = jd_check_tables(d, b, c)) return rc;
    }
    const uint64_t blocks = jf_blocks(d.W, d.H, d.ncomp, d.h, d.v);
    const int rc = jf_layout(r, d.W, d.H, d.ncomp, d.h, d.v, d.color);
    ATTWARP_REQUIRE(rc != JF_E_SLOTS, "jpegdec: image %d: more than %d blocks per MCU", b, JF_MAX_SLOTS);
    ATTWARP_REQUIRE(rc != JF_E_FRACTION, "jpegdec: image %d: a component's sampling factors do not divide the frame's largest (fractional up-sampling)", b);
    ATTWARP_REQUIRE(rc != JF_E_COLOR, "jpegdec: image %d: colour rule %d with %d components", b, d.color, d.ncomp);
    ATTWARP_REQUIRE(rc == JF_OK, "jpegdec: image %d: bad layout", b);
    return jd_check_sizes(d, b, blocks, r);
  }
  static void fill(const Input& d, JfImage& r) {
    r.conv = d.mode == ATTWARP_JPEGDEC_L ? JF_CONV_L : d.mode == ATTWARP_JPEGDEC_RGB ? JF_CONV_RGB : JF_CONV_KEEP;
    r.swap = d.ncomp != 1 && r.oc == 3 && d.order == ATTWARP_BGR;
    for (int c = 0; c < d.ncomp; ++c) {
      std::memcpy(r.qt[c], d.qt[c], sizeof r.qt[c]);
      std::memcpy(r.dc_counts[c], d.dc_counts[c], 16);
      std::memcpy(r.ac_counts[c], d.ac_counts[c], 16);
      std::memcpy(r.dc_symbols[c], d.dc_symbols[c], 256);
      std::memcpy(r.ac_symbols[c], d.ac_symbols[c], 256);
    }
    r.period = jf_period(r);
  }
};

static int jd_substream_args(int segment_bytes, int max_rounds) {
  ATTWARP_REQUIRE(segment_bytes >= 32 && segment_bytes <= 512 && (segment_bytes & (segment_bytes - 1)) == 0,
                  "jpegdec: segment_bytes=%d must be a power of two in 32..512", segment_bytes);
  ATTWARP_REQUIRE(max_rounds >= 1 && max_rounds <= JD_SUB_MAX_ROUNDS, "jpegdec: max_rounds=%d outside 1..%d", max_rounds, JD_SUB_MAX_ROUNDS);
  return ATTWARP_OK;
}

// The table of a family's frames: header, image records, sub-stream records; segment_bytes = max_rounds = 0 plans no sub-streams.
template <class F>
static int jd_plan_frames(const typename F::Input* images, int B, void* table, size_t table_bytes, int segment_bytes, int max_rounds) {
  using Image = typename F::Image;
  ATTWARP_REQUIRE(images, "jpegdec: null image array");
  const bool substreams = segment_bytes != 0 || max_rounds != 0;
  if (substreams)
    if (const int rc = jd_substream_args(segment_bytes, max_rounds)) return rc;
  ATTWARP_REQUIRE(B > 0, "jpegdec: non-positive batch size");
  if (B > JD_MAX_B) return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: B=%d > 2^20", B);
  ATTWARP_REQUIRE(table, "%s: null table", F::PLAN);
  const size_t need = (size_t)jp_header_off(B, sizeof(Image));
  ATTWARP_REQUIRE(table_bytes >= need, "%s: table of %zu bytes, %zu needed", F::PLAN, table_bytes, need);
  const auto tiles = [](uint64_t n, uint64_t tile) { return (int64_t)((n + tile - 1) / tile); };
  int64_t units = 0, itiles = 0, ctiles = 0;
  {
    std::vector<Image> probe(1);
    for (int b = 0; b < B; ++b) {                            // everything is checked before anything is written
      if (const int rc = F::geom(images[b], b, probe[0])) return rc;
      units += probe[0].nunits;
      itiles += tiles(probe[0].nblocks, JD_IDCT_TILE);
      ctiles += tiles((uint64_t)images[b].H * images[b].W, JD_COLOR_TILE);
    }
  }
  if (units > JD_MAX_TOTAL_UNITS || itiles > JD_MAX_TOTAL_UNITS || ctiles > JD_MAX_TOTAL_UNITS)
    return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: %lld units, %lld + %lld workgroups in one call (> 2^30)", (long long)units, (long long)itiles, (long long)ctiles);
  uint8_t* t = static_cast<uint8_t*>(table);
  std::memset(t, 0, need);
  attwarp_jpegdec_header h;
  std::memset(&h, 0, sizeof h);
  h.magic = F::MAGIC;
  h.B = B;
  h.total_units = (int32_t)units;
  h.idct_tiles = (int32_t)itiles;
  h.color_tiles = (int32_t)ctiles;
  h.table_bytes = need;
  h.off_images = jd_align(sizeof(attwarp_jpegdec_header), 16);
  Image* im = reinterpret_cast<Image*>(t + h.off_images);
  JdSub* sub = reinterpret_cast<JdSub*>(t + h.off_images + (uint64_t)B * sizeof(Image));
  int32_t nsub = 0;
  uint64_t soff = jd_data_base(B, (int)units), ooff = 0, stream_bytes = 0;
  int32_t u0 = 0, it0 = 0, ct0 = 0;
  for (int b = 0; b < B; ++b) {
    const typename F::Input& d = images[b];
    Image& r = im[b];
    F::geom(d, b, r);
    r.stream_off = d.stream_off;
    r.stream_len = (uint32_t)d.stream_len;
    r.oc = d.mode == ATTWARP_JPEGDEC_L ? 1 : d.mode == ATTWARP_JPEGDEC_RGB ? 3 : d.ncomp;
    F::fill(d, r);
    r.unit0 = u0; r.idct_tile0 = it0; r.color_tile0 = ct0;
    r.coef_off = soff;
    soff += jd_align((uint64_t)r.nblocks * 128u, 256);
    r.plane_off = soff;
    soff += jd_align((uint64_t)r.nblocks * 64u, 256);
    r.out_off = ooff;
    ooff += (uint64_t)d.H * d.W * r.oc;
    u0 += r.nunits;
    it0 += (int32_t)tiles(r.nblocks, JD_IDCT_TILE);
    ct0 += (int32_t)tiles((uint64_t)d.H * d.W, JD_COLOR_TILE);
    stream_bytes = std::max(stream_bytes, d.stream_off + d.stream_len);
    // sub-streams: a marker-less image (one unit) whose data is at least two segments long
    const uint64_t nseg = substreams ? (d.stream_len + (uint64_t)segment_bytes - 1) / (uint64_t)segment_bytes : 0;
    sub[b].segment_bytes = (uint32_t)segment_bytes;
    sub[b].max_rounds = (uint32_t)max_rounds;
    if (substreams && r.nunits == 1 && d.stream_len >= 2u * (uint64_t)segment_bytes && nseg <= (uint64_t)JD_SUB_MAX_SEGS) {
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
    soff += jd_align((uint64_t)sub[b].nseg * (sizeof(typename F::SegState) + sizeof(typename F::Segment)), 256);
  }
  h.reserved = nsub;
  h.scratch_bytes = soff;
  h.out_bytes = ooff;
  h.stream_bytes = stream_bytes;
  std::memcpy(t, &h, sizeof h);
  return ATTWARP_OK;
}

extern "C" size_t attwarp_jpegdec_table_bytes(const attwarp_jpegdec_image* images, int B) {
  if (!images || B <= 0 || B > JD_MAX_B) {
    fail(ATTWARP_E_ARG, "jpegdec_table_bytes: B=%d outside the limits", B);
    return 0;
  }
  return (size_t)jp_header_off(B, sizeof(JdImage));
}
extern "C" size_t attwarp_jpegdec_layouts_table_bytes(const attwarp_jpegdec_layout_image* images, int B) {
  if (!images || B <= 0 || B > JD_MAX_B) {
    fail(ATTWARP_E_ARG, "jpegdec_layouts_table_bytes: B=%d outside the limits", B);
    return 0;
  }
  return (size_t)jp_header_off(B, sizeof(JfImage));
}

extern "C" int attwarp_jpegdec_plan(const attwarp_jpegdec_image* images, int B, void* table, size_t table_bytes) {
  return jd_plan_frames<JdFrames>(images, B, table, table_bytes, 0, 0);
}
extern "C" int attwarp_jpegdec_plan_ex(const attwarp_jpegdec_image* images, int B, void* table, size_t table_bytes, int segment_bytes,
                                       int max_rounds) {
  return jd_plan_frames<JdFrames>(images, B, table, table_bytes, segment_bytes, max_rounds);
}
extern "C" int attwarp_jpegdec_plan_layouts(const attwarp_jpegdec_layout_image* images, int B, void* table, size_t table_bytes,
                                            int segment_bytes, int max_rounds) {
  return jd_plan_frames<JfFrames>(images, B, table, table_bytes, segment_bytes, max_rounds);
}

extern "C" uint64_t attwarp_jpegdec_info_offset(const void* table_host) {
  if (!table_host) return 0;
  attwarp_jpegdec_header h;
  std::memcpy(&h, table_host, sizeof h);
  if ((h.magic != JD_MAGIC && h.magic != JD_MAGIC_LAYOUTS && h.magic != JD_MAGIC_LAYOUT_SCANS) || h.B <= 0 || h.B > JD_MAX_B) return 0;
  JdSub s;
  const size_t record = h.magic == JD_MAGIC ? sizeof(JdImage) : sizeof(JfImage);
  std::memcpy(&s, static_cast<const uint8_t*>(table_host) + h.off_images + (uint64_t)h.B * record, sizeof s);
  return s.info_off;
}

// ---- the plan over all scans of a list of files: a table of the family's frames for B one-unit images (what the IDCT and
// colour kernels read) with a scan header and the scan records behind it, sorted by (level, image, position) ------------------------
// A scan family on the host: its frames, the caller's scan type, the record and the header it writes, the magic of the table
// and of the header, the planner's name in messages, whether a frame is checked in front of its first scan's own fields or
// behind them (what the caller is told first when both are wrong), and per scan: band() checks the progression, fill()
// writes the kind and the checked Huffman tables, geometry() says how a component lies in the frame; per level: close().
struct JpScans {
  using Frames = JdFrames;
  using Input = attwarp_jpegdec_scan;
  using Scan = JpScan;
  using Header = JpHeader;
  static constexpr uint32_t TABLE_MAGIC = JD_MAGIC, MAGIC = JP_MAGIC;
  static constexpr const char* PLAN = "jpegdec_plan_scans";
  static constexpr const char* PLAN_EX = "jpegdec_plan_scans_ex";
  static size_t sync_bytes(int nscans) { return sizeof(JpSyncHeader) + (size_t)nscans * sizeof(JpSync); }
  static constexpr bool FRAME_FIRST = false;
  static JpHeader& scans(Header& h) { return h; }
  static int band(const Input& d, int index) {
    ATTWARP_REQUIRE(d.ss >= 0 && d.ss <= d.se && d.se <= 63 && (d.ss != 0 || d.se == 0) && (d.ss == 0 || d.ncomp == 1) && d.al >= 0 &&
                        d.al <= 13 && d.ah >= 0 && d.ah <= 14 && (d.ah == 0 || d.al == d.ah - 1),
                    "jpegdec: image %d scan %d: bad progression Ss=%d Se=%d Ah=%d Al=%d", d.image, index, d.ss, d.se, d.ah, d.al);
    return ATTWARP_OK;
  }
  static int fill(const Input& d, int index, JpScan& r) {
    r.kind = (uint32_t)((d.ss ? 2 : 0) + (d.ah ? 1 : 0));
    const int ntab = d.ss ? 1 : d.ncomp;
    for (int t = 0; t < ntab; ++t) {
      char what[48];
      const char* fault = jd_huffman_fault(d.counts[t], d.symbols[t], !d.ss, what);
      ATTWARP_REQUIRE(!fault, "jpegdec: image %d scan %d: %s", d.image, index, fault);
      std::memcpy(r.counts[t], d.counts[t], 16);
      std::memcpy(r.symbols[t], d.symbols[t], 256);
    }
    return ATTWARP_OK;
  }
  static void geometry(const JdImage& f, int c, int& h, int& v, int& dw, int& dh) {
    h = c == 0 ? f.hs : 1; v = c == 0 ? f.vs : 1;
    dw = (f.W * h + f.hs - 1) / f.hs; dh = (f.H * v + f.vs - 1) / f.vs;
  }
  static void close(Header&, int, const std::vector<JpScan>&) {}
};
struct JsScans {
  using Frames = JfFrames;
  using Input = attwarp_jpegdec_layout_scan;
  using Scan = JsScan;
  using Header = JsHeader;
  static constexpr uint32_t TABLE_MAGIC = JS_MAGIC, MAGIC = JS_MAGIC_SCANS;
  static constexpr const char* PLAN = "jpegdec_plan_layout_scans";
  static constexpr const char* PLAN_EX = "jpegdec_plan_layout_scans_ex";
  static size_t sync_bytes(int nscans) { return sizeof(JsSyncHeader) + (size_t)nscans * sizeof(JsSync); }
  static constexpr bool FRAME_FIRST = true;
  static JpHeader& scans(Header& h) { return h.h; }
  static int band(const Input& d, int index) {
    if (d.sequential)
      ATTWARP_REQUIRE(d.ss == 0 && d.se == 63 && d.ah == 0 && d.al == 0, "jpegdec: image %d scan %d: a sequential scan with Ss=%d Se=%d Ah=%d Al=%d",
                      d.image, index, d.ss, d.se, d.ah, d.al);
    else
      ATTWARP_REQUIRE(d.ss >= 0 && d.ss <= d.se && d.se <= 63 && (d.ss != 0 || d.se == 0) && (d.ss == 0 || d.ncomp == 1) && d.al >= 0 &&
                          d.al <= 13 && d.ah >= 0 && d.ah <= 14 && (d.ah == 0 || d.al == d.ah - 1),
                      "jpegdec: image %d scan %d: bad progression Ss=%d Se=%d Ah=%d Al=%d in a scan of %d component(s)", d.image, index, d.ss,
                      d.se, d.ah, d.al, d.ncomp);
    return ATTWARP_OK;
  }
  // the code tables a scan holds in LDS: a DC and an AC table per component of a sequential scan
  static int tables(uint32_t kind, int ncomp, bool dc) {
    return kind == JS_SEQUENTIAL ? ncomp : dc ? (kind == JP_DC_FIRST ? ncomp : 0) : (kind >= JP_AC_FIRST ? 1 : 0);
  }
  static int fill(const Input& d, int index, JsScan& r) {
    r.kind = d.sequential ? JS_SEQUENTIAL : (uint32_t)((d.ss ? 2 : 0) + (d.ah ? 1 : 0));
    r.ncomp = (uint32_t)d.ncomp;
    const int ndc = tables(r.kind, d.ncomp, true), nac = tables(r.kind, d.ncomp, false);
    for (int t = 0; t < ndc + nac; ++t) {
      const bool isdc = t < ndc;
      const int e = isdc ? t : t - ndc;
      char what[48];
      const char* fault = isdc ? jd_huffman_fault(d.dc_counts[e], d.dc_symbols[e], true, what) : jd_huffman_fault(d.ac_counts[e], d.ac_symbols[e], false, what);
      ATTWARP_REQUIRE(!fault, "jpegdec: image %d scan %d: %s", d.image, index, fault);
      std::memcpy(isdc ? r.dc_counts[e] : r.ac_counts[e], isdc ? d.dc_counts[e] : d.ac_counts[e], 16);
      std::memcpy(isdc ? r.dc_symbols[e] : r.ac_symbols[e], isdc ? d.dc_symbols[e] : d.ac_symbols[e], 256);
    }
    return ATTWARP_OK;
  }
  static void geometry(const JfImage& f, int c, int& h, int& v, int& dw, int& dh) {
    const JfComp& k = f.comp[c];
    h = k.h; v = k.v; dw = k.dw; dh = k.dh;
  }
  static void close(Header& h, int l, const std::vector<JsScan>& rec) {      // the most tables a scan of the level names, at least 1
    h.level_tables[l] = 1;
    for (const JsScan& r : rec)
      if ((int)r.level == l) h.level_tables[l] = std::max(h.level_tables[l], tables(r.kind, (int)r.ncomp, true) + tables(r.kind, (int)r.ncomp, false));
  }
};

template <class S>
static size_t jp_scans_bytes(int B, int nscans) {
  return (size_t)(jp_header_off(B, sizeof(typename S::Frames::Image)) + sizeof(typename S::Header) + (uint64_t)nscans * sizeof(typename S::Scan));
}
static size_t jpegprog_sync_bytes(int nscans) { return JpScans::sync_bytes(nscans); }

extern "C" size_t attwarp_jpegdec_scans_table_bytes(const attwarp_jpegdec_image* images, int B, int nscans) {
  if (!images || B <= 0 || B > JD_MAX_B || nscans < B || (int64_t)nscans > (int64_t)B * ATTWARP_JPEGDEC_MAX_SCANS) {
    fail(ATTWARP_E_ARG, "jpegdec_scans_table_bytes: B=%d, %d scans outside the limits", B, nscans);
    return 0;
  }
  return jp_scans_bytes<JpScans>(B, nscans);
}
extern "C" size_t attwarp_jpegdec_scans_table_bytes_ex(const attwarp_jpegdec_image* images, int B, int nscans, int segment_bytes,
                                                       int max_rounds) {
  const size_t base = attwarp_jpegdec_scans_table_bytes(images, B, nscans);
  return base && (segment_bytes != 0 || max_rounds != 0) ? base + jpegprog_sync_bytes(nscans) : base;
}
extern "C" size_t attwarp_jpegdec_layout_scans_table_bytes(const attwarp_jpegdec_layout_image* images, int B, int nscans) {
  if (!images || B <= 0 || B > JD_MAX_B || nscans < B || (int64_t)nscans > (int64_t)B * ATTWARP_JPEGDEC_MAX_SCANS) {
    fail(ATTWARP_E_ARG, "jpegdec_layout_scans_table_bytes: B=%d, %d scans outside the limits", B, nscans);
    return 0;
  }
  return jp_scans_bytes<JsScans>(B, nscans);
}

// The sub-stream trailer of attwarp_jpegdec_plan_scans_ex behind the scan records (rec in the caller's order; order: record ->
// the scan's position there) -> the scratch bytes with it.  Behind everything there was: the per-scan results, then per cut
// scan its segments and, for an AC refinement, the history masks (8 bytes per block of the scan) and their prefix sums (4
// bytes per block, one more).
static uint64_t jp_plan_sync(const std::vector<JpScan>& rec, const std::vector<int>& order, int nlevels, int segment_bytes, int max_rounds,
                             const uint64_t* data_bytes, uint64_t scratch_bytes, uint8_t* trailer) {
  const int nscans = (int)rec.size();
  JpSyncHeader sh;
  std::memset(&sh, 0, sizeof sh);
  sh.magic = JP_SYNC_MAGIC;
  uint64_t soff = jd_align(scratch_bytes, 256);
  sh.info_off = soff;
  soff += jd_align((uint64_t)nscans * sizeof(JpSyncInfo), 256);
  std::vector<JpSync> sy((size_t)nscans);
  uint32_t ncut = 0;
  int level = 0;
  for (int q = 0; q < nscans; ++q) {
    const JpScan& r = rec[(size_t)order[(size_t)q]];
    const uint64_t len = data_bytes[order[(size_t)q]];
    for (; level < (int)r.level; ++level) sh.level_cut0[level + 1] = ncut;
    JpSync& y = sy[(size_t)q];
    std::memset(&y, 0, sizeof y);
    y.segment_bytes = (uint32_t)segment_bytes;
    y.max_rounds = (uint32_t)max_rounds;
    y.slot = (uint32_t)order[(size_t)q];
    const uint64_t nseg = (len + (uint64_t)segment_bytes - 1) / (uint64_t)segment_bytes;
    // a marker-less scan (one unit) whose data is at least two segments long
    const int kinds = tune(TUNE_JPEGPROG_SYNC_KINDS);        // (the tuning flavour's per-kind timing; -1 in the product)
    if (r.nunits == 1 && len >= 2u * (uint64_t)segment_bytes && nseg <= JP_SYNC_MAX_SEGS && (kinds < 0 || ((kinds >> r.kind) & 1))) {
      y.nseg = (uint32_t)nseg;
      y.seg_off = soff;
      soff += jd_align(nseg * sizeof(JpSeg), 256);
      if (r.kind == JP_AC_REFINE) {
        y.mask_off = soff;
        soff += jd_align((uint64_t)r.nmcu * 12u + 4u, 256);
      }
      sy[ncut++].cut = (uint32_t)q;
    }
  }
  for (; level < nlevels + 1 && level <= ATTWARP_JPEGDEC_MAX_SCANS; ++level) sh.level_cut0[level + 1] = ncut;
  sh.ncut = ncut;
  std::memcpy(trailer, &sh, sizeof sh);
  std::memcpy(trailer + sizeof sh, sy.data(), (size_t)nscans * sizeof(JpSync));
  return soff;
}

// The same for attwarp_jpegdec_plan_layout_scans_ex: a JsSyncHeader and JsSync records behind the JsScan
// records, segments of 96 bytes.  A sequential scan, a scan without data_bytes and a scan of 2^24 blocks or more stay on
// one lane; a cut DC first pass gets the period of its table sequence.
static uint64_t js_plan_sync(const std::vector<JsScan>& rec, const std::vector<int>& order, int nlevels, int segment_bytes, int max_rounds,
                             const uint64_t* data_bytes, uint64_t scratch_bytes, uint8_t* trailer) {
  const int nscans = (int)rec.size();
  JsSyncHeader sh;
  std::memset(&sh, 0, sizeof sh);
  sh.magic = JS_SYNC_MAGIC;
  uint64_t soff = jd_align(scratch_bytes, 256);
  sh.info_off = soff;
  soff += jd_align((uint64_t)nscans * sizeof(JpSyncInfo), 256);
  std::vector<JsSync> sy((size_t)nscans);
  uint32_t ncut = 0;
  int level = 0;
  const int kinds = tune(TUNE_JPEGPROG_SYNC_KINDS);          // (the tuning flavour's per-kind timing; -1 in the product)
  for (int q = 0; q < nscans; ++q) {
    const JsScan& r = rec[(size_t)order[(size_t)q]];
    const uint64_t len = data_bytes[order[(size_t)q]];
    for (; level < (int)r.level; ++level) sh.level_cut0[level + 1] = ncut;
    JsSync& y = sy[(size_t)q];
    std::memset(&y, 0, sizeof y);
    y.segment_bytes = (uint32_t)segment_bytes;
    y.max_rounds = (uint32_t)max_rounds;
    y.slot = (uint32_t)order[(size_t)q];
    y.period = 1;
    const uint64_t nseg = (len + (uint64_t)segment_bytes - 1) / (uint64_t)segment_bytes;
    if (r.kind <= JP_AC_REFINE && r.nunits == 1 && len >= 2u * (uint64_t)segment_bytes && nseg <= JP_SYNC_MAX_SEGS &&
        (uint64_t)r.nmcu * r.nslot < JP_SYNC_CAP && (kinds < 0 || ((kinds >> r.kind) & 1))) {
      y.nseg = (uint32_t)nseg;
      y.period = js_period(r);
      y.seg_off = soff;
      soff += jd_align(nseg * sizeof(JsSeg), 256);
      if (r.kind == JP_AC_REFINE) {
        y.mask_off = soff;
        soff += jd_align((uint64_t)r.nmcu * 12u + 4u, 256);
      }
      const uint32_t ntab = r.kind == JP_DC_FIRST ? r.ncomp : r.kind == JP_DC_REFINE ? 0u : 1u;
      sh.level_tables[r.level] = std::max(sh.level_tables[r.level], ntab);
      sy[ncut++].cut = (uint32_t)q;
    }
  }
  for (; level < nlevels + 1 && level <= ATTWARP_JPEGDEC_MAX_SCANS; ++level) sh.level_cut0[level + 1] = ncut;
  for (int l = 0; l < nlevels; ++l) sh.level_tables[l] = std::max(sh.level_tables[l], 1u);
  sh.ncut = ncut;
  std::memcpy(trailer, &sh, sizeof sh);
  std::memcpy(trailer + sizeof sh, sy.data(), (size_t)nscans * sizeof(JsSync));
  return soff;
}

// The scan planner of both families.  segment_bytes = max_rounds = 0 plans no sub-streams and writes the table of
// attwarp_jpegdec_plan_scans / attwarp_jpegdec_plan_layout_scans.
template <class S>
static int jp_plan_scans(const typename S::Frames::Input* images, int B, const typename S::Input* scans, int nscans, void* table,
                         size_t table_bytes, int by_level, int segment_bytes, int max_rounds, const uint64_t* data_bytes) {
  using Image = typename S::Frames::Image;
  using Scan = typename S::Scan;
  ATTWARP_REQUIRE(images && scans && table, "%s: null pointer", S::PLAN);
  ATTWARP_REQUIRE(B > 0 && B <= JD_MAX_B && nscans >= B && (int64_t)nscans <= (int64_t)B * ATTWARP_JPEGDEC_MAX_SCANS,
                  "%s: B=%d, %d scans outside the limits", S::PLAN, B, nscans);
  const bool substreams = segment_bytes != 0 || max_rounds != 0;
  if (substreams) {
    if (const int rc = jd_substream_args(segment_bytes, max_rounds)) return rc;
    ATTWARP_REQUIRE(data_bytes, "%s: null data_bytes", S::PLAN_EX);
    for (int i = 0; i < nscans; ++i)
      ATTWARP_REQUIRE(scans[i].image >= 0 && scans[i].image < B && scans[i].stream_off <= images[scans[i].image].stream_len &&
                          data_bytes[i] <= images[scans[i].image].stream_len - scans[i].stream_off,
                      "%s: scan %d: data outside the image's", S::PLAN_EX, i);
  }
  const size_t need = jp_scans_bytes<S>(B, nscans) + (substreams ? S::sync_bytes(nscans) : 0);
  ATTWARP_REQUIRE(table_bytes >= need, "%s: table of %zu bytes, %zu needed", S::PLAN, table_bytes, need);
  for (int b = 0; b < B; ++b)
    ATTWARP_REQUIRE(images[b].restart_interval == 0, "%s: image %d: the restart interval belongs to the scans", S::PLAN, b);
  // everything is checked before anything is written: the scans come image by image, in file order
  std::vector<Scan> rec((size_t)nscans);
  std::vector<int> count(B, 0);
  std::vector<int64_t> per(B, 0);                              // the units of an image, over all its scans
  std::vector<Image> frame(1);
  int64_t total_units = 0;
  int nlevels = 0, prev = -1;
  for (int i = 0, first = 0; i < nscans; ++i) {
    const typename S::Input& d = scans[i];
    ATTWARP_REQUIRE(d.image >= 0 && d.image < B && d.image >= prev, "%s: scan %d: image %d out of order", S::PLAN, i, d.image);
    const typename S::Frames::Input& img = images[d.image];
    if (d.image != prev) { first = i; prev = d.image; }
    const int index = i - first;
    if (index == 0 && S::FRAME_FIRST)
      if (const int rc = S::Frames::geom(img, d.image, frame[0])) return rc;
    if (index >= ATTWARP_JPEGDEC_MAX_SCANS)
      return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: image %d: more than %d scans", d.image, ATTWARP_JPEGDEC_MAX_SCANS);
    ++count[d.image];
    ATTWARP_REQUIRE(d.ncomp >= 1 && d.ncomp <= img.ncomp && d.ncomp <= S::Frames::MAX_COMP, "jpegdec: image %d scan %d: %d components",
                    d.image, index, d.ncomp);
    for (int c = 0; c < d.ncomp; ++c)
      ATTWARP_REQUIRE(d.comp[c] >= 0 && d.comp[c] < img.ncomp && (c == 0 || d.comp[c] > d.comp[c - 1]),
                      "jpegdec: image %d scan %d: components not in frame order", d.image, index);
    if (const int rc = S::band(d, index)) return rc;
    ATTWARP_REQUIRE(d.restart_interval >= 0 && d.restart_interval <= 65535, "jpegdec: image %d scan %d: restart interval %d", d.image, index,
                    d.restart_interval);
    ATTWARP_REQUIRE(d.stream_off <= img.stream_len, "jpegdec: image %d scan %d: data outside the image's", d.image, index);
    if (index == 0 && !S::FRAME_FIRST)
      if (const int rc = S::Frames::geom(img, d.image, frame[0])) return rc;
    const Image& f = frame[0];
    Scan& r = rec[(size_t)i];
    std::memset(&r, 0, sizeof r);
    r.image = (uint32_t)d.image; r.index = (uint32_t)index; r.off = (uint32_t)d.stream_off;
    r.ss = (uint32_t)d.ss; r.se = (uint32_t)d.se; r.al = (uint32_t)d.al;
    if (const int rc = S::fill(d, index, r)) return rc;
    int h, v, dw, dh;
    if (d.ncomp == 1) {                                        // not interleaved: the blocks that cover the component's true size
      S::geometry(f, d.comp[0], h, v, dw, dh);
      r.nslot = 1;
      r.mcux = (uint32_t)((dw + 7) / 8);
      r.nmcu = r.mcux * (uint32_t)((dh + 7) / 8);
      r.slot_c[0] = (uint8_t)d.comp[0];
    } else {                                                   // the frame's MCUs, also for a subset of its components
      r.mcux = (uint32_t)f.mcux;
      r.nmcu = (uint32_t)f.mcux * (uint32_t)f.mcuy;
      for (int t = 0; t < d.ncomp; ++t) {
        S::geometry(f, d.comp[t], h, v, dw, dh);
        for (int y = 0; y < v; ++y)
          for (int x = 0; x < h; ++x) {
            ATTWARP_REQUIRE(r.nslot < (uint32_t)S::Frames::MAX_SLOTS, "jpegdec: image %d scan %d: more than %d blocks per MCU", d.image, index,
                            S::Frames::MAX_SLOTS);
            r.slot_c[r.nslot] = (uint8_t)d.comp[t]; r.slot_y[r.nslot] = (uint8_t)y; r.slot_x[r.nslot] = (uint8_t)x; r.slot_t[r.nslot] = (uint8_t)t;
            ++r.nslot;
          }
      }
    }
    r.ri = d.restart_interval ? (uint32_t)d.restart_interval : r.nmcu;
    r.nunits = (r.nmcu + r.ri - 1) / r.ri;
    // the level: behind every earlier scan of the image that shares a component and overlaps the band
    uint32_t level = by_level ? 0u : (uint32_t)index;
    if (by_level)
      for (int j = first; j < i; ++j) {
        const typename S::Input& e = scans[j];
        bool share = false;
        for (int a = 0; a < d.ncomp; ++a)
          for (int bb = 0; bb < e.ncomp; ++bb) share = share || d.comp[a] == e.comp[bb];
        if (share && e.ss <= d.se && d.ss <= e.se) level = std::max(level, rec[(size_t)j].level + 1u);
      }
    r.level = level;
    nlevels = std::max(nlevels, (int)level + 1);
    total_units += r.nunits;
    per[d.image] += r.nunits;
  }
  for (int b = 0; b < B; ++b) ATTWARP_REQUIRE(count[b] >= 1, "%s: image %d has no scan", S::PLAN, b);
  for (int b = 0; b < B; ++b)
    if (per[b] > ATTWARP_JPEGDEC_MAX_UNITS)
      return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: image %d: %lld units over its scans (> %d)", b, (long long)per[b], ATTWARP_JPEGDEC_MAX_UNITS);
  if (total_units > JD_MAX_TOTAL_UNITS) return fail(ATTWARP_E_UNSUPPORTED, "jpegdec: %lld units in one call (> 2^30)", (long long)total_units);
  if (const int rc = jd_plan_frames<typename S::Frames>(images, B, table, table_bytes, 0, 0)) return rc;
  uint8_t* t = static_cast<uint8_t*>(table);
  attwarp_jpegdec_header h;
  std::memcpy(&h, t, sizeof h);
  typename S::Header header;
  std::memset(&header, 0, sizeof header);
  JpHeader& ph = S::scans(header);
  const uint64_t header_off = jp_header_off(B, sizeof(Image));
  ph.magic = S::MAGIC;
  ph.nscans = nscans; ph.nlevels = nlevels; ph.total_units = (int32_t)total_units;
  ph.off_scans = header_off + sizeof header;
  const JdSub* sub = reinterpret_cast<const JdSub*>(t + h.off_images + (uint64_t)B * sizeof(Image));
  ph.clear_off = jd_data_base(B, h.total_units);
  ph.clear_bytes = sub[0].info_off - ph.clear_off;             // (both are multiples of 256)
  ph.starts_off = jd_align(h.scratch_bytes, 256);
  h.scratch_bytes = ph.starts_off + jd_align((uint64_t)total_units * 8u, 256);
  h.table_bytes = need;
  h.magic = S::TABLE_MAGIC;                                    // (of the layout scans: attwarp_jpegdec_decode_layouts refuses the table)
  // records sorted by (level, image, position): a stable pass per level over the input order
  Scan* out = reinterpret_cast<Scan*>(t + ph.off_scans);
  uint32_t unit0 = 0;
  for (int i = 0; i < nscans; ++i) {
    rec[(size_t)i].unit0 = unit0;
    unit0 += rec[(size_t)i].nunits;
    rec[(size_t)i].last = i + 1 == nscans || scans[i + 1].image != scans[i].image;
  }
  int at = 0;
  std::vector<int> order((size_t)nscans);                     // record -> the scan's position in the caller's array
  for (int l = 0; l < nlevels; ++l) {
    ph.level_scan0[l] = at;
    uint32_t wave = 0;
    for (int i = 0; i < nscans; ++i)
      if ((int)rec[(size_t)i].level == l) {
        rec[(size_t)i].wave0 = wave;
        wave += rec[(size_t)i].nunits;
        order[(size_t)at] = i;
        std::memcpy(out + at++, &rec[(size_t)i], sizeof(Scan));
      }
    ph.level_waves[l] = (int32_t)wave;
    S::close(header, l, rec);
  }
  ph.level_scan0[nlevels] = at;
  if (substreams) {
    uint8_t* trailer = t + ph.off_scans + (uint64_t)nscans * sizeof(Scan);
    if constexpr (std::is_same<Scan, JpScan>::value)
      h.scratch_bytes = jp_plan_sync(rec, order, nlevels, segment_bytes, max_rounds, data_bytes, h.scratch_bytes, trailer);
    else
      h.scratch_bytes = js_plan_sync(rec, order, nlevels, segment_bytes, max_rounds, data_bytes, h.scratch_bytes, trailer);
  }
  std::memcpy(t + header_off, &header, sizeof header);
  std::memcpy(t, &h, sizeof h);
  return ATTWARP_OK;
}

extern "C" int attwarp_jpegdec_plan_scans(const attwarp_jpegdec_image* images, int B, const attwarp_jpegdec_scan* scans, int nscans,
                                          void* table, size_t table_bytes, int by_level) {
  return jp_plan_scans<JpScans>(images, B, scans, nscans, table, table_bytes, by_level, 0, 0, nullptr);
}
extern "C" int attwarp_jpegdec_plan_scans_ex(const attwarp_jpegdec_image* images, int B, const attwarp_jpegdec_scan* scans, int nscans,
                                             void* table, size_t table_bytes, int by_level, int segment_bytes, int max_rounds,
                                             const uint64_t* data_bytes) {
  return jp_plan_scans<JpScans>(images, B, scans, nscans, table, table_bytes, by_level, segment_bytes, max_rounds, data_bytes);
}
extern "C" int attwarp_jpegdec_plan_layout_scans(const attwarp_jpegdec_layout_image* images, int B, const attwarp_jpegdec_layout_scan* scans,
                                                 int nscans, void* table, size_t table_bytes, int by_level) {
  return jp_plan_scans<JsScans>(images, B, scans, nscans, table, table_bytes, by_level, 0, 0, nullptr);
}

extern "C" size_t attwarp_jpegdec_layout_scans_table_bytes_ex(const attwarp_jpegdec_layout_image* images, int B, int nscans, int segment_bytes,
                                                              int max_rounds) {
  const size_t base = attwarp_jpegdec_layout_scans_table_bytes(images, B, nscans);
  return base && (segment_bytes != 0 || max_rounds != 0) ? base + JsScans::sync_bytes(nscans) : base;
}
extern "C" int attwarp_jpegdec_plan_layout_scans_ex(const attwarp_jpegdec_layout_image* images, int B, const attwarp_jpegdec_layout_scan* scans,
                                                    int nscans, void* table, size_t table_bytes, int by_level, int segment_bytes, int max_rounds,
                                                    const uint64_t* data_bytes) {
  return jp_plan_scans<JsScans>(images, B, scans, nscans, table, table_bytes, by_level, segment_bytes, max_rounds, data_bytes);
}

// (a table of either scan family)
extern "C" uint64_t attwarp_jpegdec_scan_info_offset(const void* table_host) {
  if (!table_host) return 0;
  attwarp_jpegdec_header h;
  std::memcpy(&h, table_host, sizeof h);
  if (h.magic == JS_MAGIC) {
    const uint64_t at0 = jp_header_off(h.B, sizeof(JfImage));
    if (h.B <= 0 || h.B > JD_MAX_B || h.table_bytes < at0 + sizeof(JsHeader)) return 0;
    JsHeader js;
    std::memcpy(&js, static_cast<const uint8_t*>(table_host) + at0, sizeof js);
    if (js.h.magic != JS_MAGIC_SCANS || js.h.nscans < 1) return 0;
    const uint64_t at = js.h.off_scans + (uint64_t)js.h.nscans * sizeof(JsScan);
    if (h.table_bytes < at + JsScans::sync_bytes(js.h.nscans)) return 0;
    JsSyncHeader sh;
    std::memcpy(&sh, static_cast<const uint8_t*>(table_host) + at, sizeof sh);
    return sh.magic == JS_SYNC_MAGIC ? sh.info_off : 0;
  }
  const uint64_t header_off = jp_header_off(h.B, sizeof(JdImage));
  if (h.magic != JD_MAGIC || h.B <= 0 || h.B > JD_MAX_B || h.table_bytes < header_off + sizeof(JpHeader)) return 0;
  JpHeader ph;
  std::memcpy(&ph, static_cast<const uint8_t*>(table_host) + header_off, sizeof ph);
  if (ph.magic != JP_MAGIC || ph.nscans < 1) return 0;
  const uint64_t at = ph.off_scans + (uint64_t)ph.nscans * sizeof(JpScan);
  if (h.table_bytes < at + jpegprog_sync_bytes(ph.nscans)) return 0;
  JpSyncHeader sh;
  std::memcpy(&sh, static_cast<const uint8_t*>(table_host) + at, sizeof sh);
  return sh.magic == JP_SYNC_MAGIC ? sh.info_off : 0;
}

// ---- the four decode entry points ------------------------------------------------------------------------------------------------------
// What all of them (`who`) check: pointers, the table of `planner` (its magic, image records of `record` bytes -> h; scans:
// and its scan header of scans_bytes, a JpHeader or a JsHeader, with scans_magic), sizes, alignment.
static int jd_decode_args(const char* who, const char* planner, uint32_t magic, size_t record, uint32_t scans_magic, void* scans,
                          size_t scans_bytes, const void* table_host, const void* table_dev, const uint8_t* stream_bytes, const void* scratch,
                          const uint8_t* out, size_t out_bytes, const int32_t* status, attwarp_jpegdec_header& h) {
  ATTWARP_REQUIRE(table_host && table_dev && stream_bytes && scratch && out && status, "%s: null pointer", who);
  std::memcpy(&h, table_host, sizeof h);
  bool ok = h.magic == magic && h.B > 0 && h.B <= JD_MAX_B && h.idct_tiles >= h.B && h.idct_tiles <= JD_MAX_TOTAL_UNITS &&
            h.color_tiles >= h.B && h.color_tiles <= JD_MAX_TOTAL_UNITS;
  if (!scans) ok = ok && h.total_units >= h.B && h.total_units <= JD_MAX_TOTAL_UNITS && h.reserved >= 0 && h.reserved <= h.B;
  else ok = ok && h.total_units == h.B && h.reserved == 0 && h.table_bytes >= jp_header_off(h.B, record) + scans_bytes;
  if (ok && scans) {
    std::memcpy(scans, static_cast<const uint8_t*>(table_host) + jp_header_off(h.B, record), scans_bytes);
    const JpHeader& ph = *static_cast<const JpHeader*>(scans);                 // (a JsHeader begins with one)
    ok = ph.magic == scans_magic && ph.nscans >= h.B && ph.nlevels >= 1 && ph.nlevels <= ATTWARP_JPEGDEC_MAX_SCANS &&
         ph.total_units >= ph.nscans && ph.total_units <= JD_MAX_TOTAL_UNITS;
    if (scans_bytes == sizeof(JsHeader))                                       // every level launches, with 1..8 tables in LDS
      for (int l = 0; ok && l < ph.nlevels; ++l)
        ok = ph.level_waves[l] >= 1 && static_cast<const JsHeader*>(scans)->level_tables[l] >= 1 &&
             static_cast<const JsHeader*>(scans)->level_tables[l] <= 2 * JF_MAX_COMP;
  }
  ATTWARP_REQUIRE(ok, "%s: not a table of %s", who, planner);
  ATTWARP_REQUIRE(out_bytes >= h.out_bytes, "%s: out of %zu bytes, %llu needed", who, out_bytes, (unsigned long long)h.out_bytes);
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(table_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(scratch) % 256 == 0 &&
                      reinterpret_cast<uintptr_t>(status) % 4 == 0,
                  "%s: table_dev must be 8-byte, scratch 256-byte, status 4-byte aligned", who);
  return ATTWARP_OK;
}

// The last two launches of every entry point: coefficients -> planes -> pixels and statuses, over JdImage or (layouts) JfImage records.
static int jd_launch_idct_color(bool layouts, const attwarp_jpegdec_header& h, const uint8_t* td, uint8_t* sc, uint8_t* out, int32_t* status,
                                hipStream_t st) {
  hipLaunchKernelGGL(layouts ? jpegfmt_idct_kernel : jpegdec_idct_kernel, dim3(h.idct_tiles), dim3(JD_NT), 0, st, td, sc);
  if (const int rc = check_launch(layouts ? "jpegfmt_idct_kernel" : "jpegdec_idct_kernel")) return rc;
  hipLaunchKernelGGL(layouts ? jpegfmt_color_kernel : jpegdec_color_kernel, dim3(h.color_tiles), dim3(JD_NT), 0, st, td, (const uint8_t*)sc,
                     (const JdState*)sc, out, status);
  return check_launch(layouts ? "jpegfmt_color_kernel" : "jpegdec_color_kernel");
}
// The clear launch of the scan families: enough workgroups for the bytes and the states, 4096 at most.
static unsigned jp_clear_groups(const JpHeader& ph, int B) {
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>((ph.clear_bytes / 16u + JD_NT - 1) / JD_NT, (uint64_t)(B + JD_NT - 1) / JD_NT), 4096);
}

// The sequential entry points: restart scan, sub-streams, one wave per unit, then jd_launch_idct_color.
static int jd_decode_frames(bool layouts, const attwarp_jpegdec_header& h, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                            uint8_t* out, int32_t* status, void* stream) {
  hipStream_t st = as_stream(stream);
  const uint8_t* td = static_cast<const uint8_t*>(table_dev);
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  hipLaunchKernelGGL(layouts ? jpegfmt_scan_kernel : jpegdec_scan_kernel, dim3(h.B), dim3(JD_NT), 0, st, td, stream_bytes, sc);
  if (const int rc = check_launch(layouts ? "jpegfmt_scan_kernel" : "jpegdec_scan_kernel")) return rc;
  hipLaunchKernelGGL(layouts ? jpegfmt_substream_kernel : jpegdec_substream_kernel, dim3(std::max(h.reserved, 1)), dim3(JD_NT), 0, st, td,
                     stream_bytes, sc);
  if (const int rc = check_launch(layouts ? "jpegfmt_substream_kernel" : "jpegdec_substream_kernel")) return rc;
  hipLaunchKernelGGL(layouts ? jpegfmt_entropy_kernel : jpegdec_entropy_kernel, dim3(h.total_units), dim3(WAVE), 0, st, td, stream_bytes, sc);
  if (const int rc = check_launch(layouts ? "jpegfmt_entropy_kernel" : "jpegdec_entropy_kernel")) return rc;
  return jd_launch_idct_color(layouts, h, td, sc, out, status, st);
}

extern "C" int attwarp_jpegdec_decode(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                                      uint8_t* out, size_t out_bytes, int32_t* status, void* stream) {
  attwarp_jpegdec_header h;
  if (const int rc = jd_decode_args("jpegdec_decode", "attwarp_jpegdec_plan", JD_MAGIC, sizeof(JdImage), 0, nullptr, 0, table_host, table_dev,
                                    stream_bytes, scratch, out, out_bytes, status, h))
    return rc;
  return jd_decode_frames(false, h, table_dev, stream_bytes, scratch, out, status, stream);
}
extern "C" int attwarp_jpegdec_decode_layouts(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                                              uint8_t* out, size_t out_bytes, int32_t* status, void* stream) {
  attwarp_jpegdec_header h;
  if (const int rc = jd_decode_args("jpegdec_decode_layouts", "attwarp_jpegdec_plan_layouts", JD_MAGIC_LAYOUTS, sizeof(JfImage), 0, nullptr, 0,
                                    table_host, table_dev, stream_bytes, scratch, out, out_bytes, status, h))
    return rc;
  return jd_decode_frames(true, h, table_dev, stream_bytes, scratch, out, status, stream);
}

extern "C" int attwarp_jpegdec_decode_scans(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                                            uint8_t* out, size_t out_bytes, int32_t* status, void* stream) {
  attwarp_jpegdec_header h;
  JpHeader ph;
  if (const int rc = jd_decode_args("jpegdec_decode_scans", "attwarp_jpegdec_plan_scans", JD_MAGIC, sizeof(JdImage), JP_MAGIC, &ph, sizeof ph,
                                    table_host, table_dev, stream_bytes, scratch, out, out_bytes, status, h))
    return rc;
  hipStream_t st = as_stream(stream);
  const uint8_t* td = static_cast<const uint8_t*>(table_dev);
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  hipLaunchKernelGGL(jpegprog_clear_kernel, dim3(jp_clear_groups(ph, h.B)), dim3(JD_NT), 0, st, td, sc);
  if (const int rc = check_launch("jpegprog_clear_kernel")) return rc;
  hipLaunchKernelGGL(jpegprog_scan_kernel, dim3(ph.nscans), dim3(JD_NT), 0, st, td, stream_bytes, sc);
  if (const int rc = check_launch("jpegprog_scan_kernel")) return rc;
  JpSyncHeader sh;
  std::memset(&sh, 0, sizeof sh);
  const uint64_t sync_at = ph.off_scans + (uint64_t)ph.nscans * sizeof(JpScan);
  if (h.table_bytes >= sync_at + jpegprog_sync_bytes(ph.nscans)) {       // planned with sub-streams
    std::memcpy(&sh, static_cast<const uint8_t*>(table_host) + sync_at, sizeof sh);
    bool ok = sh.magic == JP_SYNC_MAGIC && sh.ncut <= (uint32_t)ph.nscans && sh.level_cut0[0] == 0;
    for (int l = 0; ok && l < ph.nlevels; ++l) ok = sh.level_cut0[l] <= sh.level_cut0[l + 1] && sh.level_cut0[l + 1] <= sh.ncut;
    ATTWARP_REQUIRE(ok, "jpegdec_decode_scans: not a table of attwarp_jpegdec_plan_scans_ex");
  }
  for (int l = 0; l < ph.nlevels; ++l) {
    ATTWARP_REQUIRE(ph.level_waves[l] >= 1, "jpegdec_decode_scans: not a table of attwarp_jpegdec_plan_scans");
    if (const uint32_t ncut = sh.level_cut0[l + 1] - sh.level_cut0[l]) {  // the level holds a cut scan
      hipLaunchKernelGGL(jpegprog_substream_kernel, dim3(ncut), dim3(JD_NT), 0, st, td, stream_bytes, sc, l);
      if (const int rc = check_launch("jpegprog_substream_kernel")) return rc;
    }
    hipLaunchKernelGGL(jpegprog_entropy_kernel, dim3(ph.level_waves[l]), dim3(WAVE), 0, st, td, stream_bytes, sc, l);
    if (const int rc = check_launch("jpegprog_entropy_kernel")) return rc;
  }
  return jd_launch_idct_color(false, h, td, sc, out, status, st);
}

extern "C" int attwarp_jpegdec_decode_layout_scans(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                                                   uint8_t* out, size_t out_bytes, int32_t* status, void* stream) {
  attwarp_jpegdec_header h;
  JsHeader sh;
  if (const int rc = jd_decode_args("jpegdec_decode_layout_scans", "attwarp_jpegdec_plan_layout_scans", JS_MAGIC, sizeof(JfImage), JS_MAGIC_SCANS,
                                    &sh, sizeof sh, table_host, table_dev, stream_bytes, scratch, out, out_bytes, status, h))
    return rc;
  hipStream_t st = as_stream(stream);
  const uint8_t* td = static_cast<const uint8_t*>(table_dev);
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  hipLaunchKernelGGL(jpegscan_clear_kernel, dim3(jp_clear_groups(sh.h, h.B)), dim3(JD_NT), 0, st, td, sc);
  if (const int rc = check_launch("jpegscan_clear_kernel")) return rc;
  hipLaunchKernelGGL(jpegscan_marks_kernel, dim3(sh.h.nscans), dim3(JD_NT), 0, st, td, stream_bytes, sc);
  if (const int rc = check_launch("jpegscan_marks_kernel")) return rc;
  JsSyncHeader yh;
  std::memset(&yh, 0, sizeof yh);
  const uint64_t sync_at = sh.h.off_scans + (uint64_t)sh.h.nscans * sizeof(JsScan);
  if (h.table_bytes >= sync_at + JsScans::sync_bytes(sh.h.nscans)) {          // planned with sub-streams
    std::memcpy(&yh, static_cast<const uint8_t*>(table_host) + sync_at, sizeof yh);
    bool ok = yh.magic == JS_SYNC_MAGIC && yh.ncut <= (uint32_t)sh.h.nscans && yh.level_cut0[0] == 0;
    for (int l = 0; ok && l < sh.h.nlevels; ++l)
      ok = yh.level_cut0[l] <= yh.level_cut0[l + 1] && yh.level_cut0[l + 1] <= yh.ncut && yh.level_tables[l] >= 1 &&
           yh.level_tables[l] <= (uint32_t)JF_MAX_COMP;
    ATTWARP_REQUIRE(ok, "jpegdec_decode_layout_scans: not a table of attwarp_jpegdec_plan_layout_scans_ex");
  }
  for (int l = 0; l < sh.h.nlevels; ++l) {
    if (const uint32_t ncut = yh.level_cut0[l + 1] - yh.level_cut0[l]) {      // the level holds a cut scan
      hipLaunchKernelGGL(jpegscan_substream_kernel, dim3(ncut), dim3(JD_NT), (size_t)yh.level_tables[l] * sizeof(JdHuff), st, td, stream_bytes, sc,
                         l, (int)yh.level_tables[l]);
      if (const int rc = check_launch("jpegscan_substream_kernel")) return rc;
    }
    hipLaunchKernelGGL(jpegscan_entropy_kernel, dim3(sh.h.level_waves[l]), dim3(WAVE), (size_t)sh.level_tables[l] * sizeof(JdHuff), st, td,
                       stream_bytes, sc, l, sh.level_tables[l]);
    if (const int rc = check_launch("jpegscan_entropy_kernel")) return rc;
  }
  return jd_launch_idct_color(true, h, td, sc, out, status, st);
}
