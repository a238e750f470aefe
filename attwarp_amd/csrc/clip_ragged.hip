// The first visit to CLIP (AGW/attention_extraction/functions.py:262-271: process_images on the driver's batch of PIL
// images of different sizes): uint8 [H_i,W_i,C] images -> [B,C,S,S] float32 / float16, a whole ragged batch per call.
//
// Arithmetic = LLaVA-1.5's process_images + the HF CLIPImageProcessor (PIL backend), per image:
//   canvas     image_aspect_ratio == "pad": the image pasted at (pad_x, pad_y) onto a canvas_w x canvas_h canvas of the
//              background colour (expand2square).  The canvas is never stored: a tap outside the image reads the
//              background byte of its channel, and a canvas row wholly outside the image has the background as its
//              horizontal-pass result (Pillow's 22-bit coefficient rows sum to 2^22 within a few units, far below the
//              rounding half).  Without padding the canvas is the image.
//   resample   Pillow's 8-bit two-pass BICUBIC (pil8.hpp; ATTWARP_PIL_BICUBIC tables canvas_w -> nw, canvas_h -> nh,
//              identity tables on an axis that keeps its size), horizontal pass first with uint8 in between -- vertical
//              pass first for the images Image.resize treats so (the caller marks them) -- computed only for the S x S
//              centre crop at (left, top).
//   epilogue   as clip.hip: float32(float64(u8) * (1/255)), (x - mean_c) / std_c in float32, channels first; float16 is
//              that value rounded once.
//
// clip_ragged_fused_kernel follows prep_fused_kernel (dataprep.hip): a workgroup owns one (image, band of output rows)
// item, stages the canvas rows the band needs into LDS RB rows at a time (background left and right, image bytes in
// between, dword loads at any byte address), runs the horizontal pass with the byte window of pil8.hpp into uint8 rows
// that stay in LDS, then the vertical pass through a 256-entry epilogue table per channel, a lane storing four
// consecutive pixels of one plane.  Images whose horizontal taps exceed the 16-tap window, vertical-first images and
// bands that do not fit the LDS take two launches with the uint8 intermediate in the caller's tmp buffer.
#include "common.hpp"
#include "pil8.hpp"

#include <cstring>
#include <vector>

namespace attwarp {
namespace clipr {

constexpr uint32_t CLIPR_MAGIC = 0x52504c43u;      // "CLPR"
constexpr int NT = 256;                            // == entries of a channel's epilogue table: thread t writes entry t
constexpr int MAX_C = 3;
constexpr int LUT_BYTES = MAX_C * 256 * 4;
constexpr int SLACK = 128;                         // behind the staged rows: the byte window of the last pixels reads past the row
constexpr int SPLIT_H_ROWS = 16, SPLIT_V_ROWS = 8; // rows per item of the two-launch route
constexpr int MAX_CANVAS = 8192, MAX_SIZE = 4096;

struct ClipImageDev {                              // the per-image record inside a table
  attwarp_clip_image r;
  int64_t tmp_off;                                 // two-launch route: where its uint8 intermediate starts in tmp
  int32_t fused, ny, rb, nr_cap;                   // one-launch route: band height, staged rows per round, LDS rows of the band
  int32_t window, reserved;                        // one-launch route: taps of the register window (8 or 16)
};
struct ClipItem { int32_t img, y0, ny, reserved; };
struct ClipConst { float mean[MAX_C], stdv[MAX_C]; uint32_t bg; };      // bg: the background bytes, channel c in bits 8c ..

__device__ __forceinline__ uint32_t bg_byte(uint32_t bg, int c) { return (bg >> (8 * c)) & 0xffu; }
__device__ __forceinline__ float epilogue(int u8, float mean, float stdv) { return fsub(pil_u8_to_unit(u8), mean) / stdv; }

__device__ __forceinline__ void store4(float* o, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(o) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void store4(__half* o, float a, float b, float c, float d) {
  const uint32_t lo = (uint32_t)__half_as_ushort(__float2half_rn(a)) | ((uint32_t)__half_as_ushort(__float2half_rn(b)) << 16);
  const uint32_t hi = (uint32_t)__half_as_ushort(__float2half_rn(c)) | ((uint32_t)__half_as_ushort(__float2half_rn(d)) << 16);
  *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
}

// grid = items, NT threads.  LDS: lut[MAX_C][256] float | kyl[ny][ksize_y] | inter[nr_cap][ocp] | srow[rb][wcp] | SLACK
// (row bytes rounded up to 4).  Every global load the passes depend on is issued in batches: the staging loop keeps STAGE_U
// dwords per lane in flight (one dependent load per dword made the staging the longest part of a band), the horizontal
// coefficients of a lane's first pixel are read once per band, the band's vertical coefficients once into LDS.
constexpr int STAGE_U = 8;
template <typename OutT, int C, int KS>
__global__ __launch_bounds__(NT) void clip_ragged_fused_kernel(const ClipImageDev* __restrict__ images,
                                                               const ClipItem* __restrict__ items, int S, ClipConst cc,
                                                               OutT* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  const int tid = threadIdx.x;
  const ClipItem it = items[blockIdx.x];
  const ClipImageDev& im = images[it.img];
  const attwarp_clip_image& r = im.r;
  const int H = r.H, W = r.W, cw = r.canvas_w, ch = r.canvas_h, wc = W * C, cwc = cw * C, oc = S * C;
  const int wcp = (cwc + 3) & ~3, ocp = (oc + 3) & ~3, px0 = r.pad_x * C, top = r.top, left = r.left;
  const int RB = im.rb;
  float* lut = reinterpret_cast<float*>(lds_b);
  int* kyl = reinterpret_cast<int*>(lds_b + LUT_BYTES);
  uint8_t* inter = lds_b + LUT_BYTES + (size_t)im.ny * r.ksize_y * 4;
  uint8_t* srow = inter + (size_t)im.nr_cap * ocp;
#pragma unroll
  for (int c = 0; c < C; ++c) lut[c * 256 + tid] = epilogue(tid, cc.mean[c], cc.stdv[c]);
  for (int i = tid; i < it.ny * r.ksize_y; i += NT) kyl[i] = r.kk_y[(size_t)(top + it.y0) * r.ksize_y + i];

  const int32_t* __restrict__ by = r.bounds_y;
  const int y0 = it.y0, y1 = it.y0 + it.ny;
  const int r0 = clampi(by[2 * (top + y0)], 0, ch - 1);
  const int nr = clampi(by[2 * (top + y1 - 1)] + by[2 * (top + y1 - 1) + 1], r0 + 1, ch) - r0;
  OutT* oimg = out + (size_t)it.img * C * S * S;
  if (nr > im.nr_cap) {
    // The band's taps span more canvas rows than the host's bound (band_rows) reserved in LDS: tables that are not Pillow's
    // for this size, or a bound gone wrong.  Computing on would clamp taps and give plausible wrong pixels: the band's
    // output becomes NaN instead (block-uniform branch, before any barrier).
    for (int e = tid; e < C * it.ny * S; e += NT) {
      const int c = e / (it.ny * S), rem = e - c * it.ny * S;
      oimg[((size_t)c * S + y0) * S + rem] = from_f32<OutT>(__int_as_float(0x7fc00000));
    }
    return;
  }

  // ---- horizontal pass: canvas rows r0 .. r0 + nr -> inter (only the S cropped columns)
  const int ndw = wcp >> 2, ksx = r.ksize_x;
  const int32_t* __restrict__ bx = r.bounds_x;
  const int32_t* __restrict__ kx = r.kk_x;
  // the coefficients and first tap of the lane's first pixel stay in registers for the whole band
  int kreg0[KS], o0 = 0;
  {
    const int xo = left + min(tid, S - 1);
    const int xmin = clampi(bx[2 * xo], 0, cw - 1), cnt = bx[2 * xo + 1];
#pragma unroll
    for (int x = 0; x < KS; ++x) kreg0[x] = (x < cnt && x < ksx) ? kx[(size_t)xo * ksx + x] : 0;
    o0 = xmin * C;
  }
  const bool wide_rows = wc >= 4;                  // a dword load at a clamped offset stays inside the image row
  for (int rs = 0; rs < nr; rs += RB) {
    const int nrows = min(RB, nr - rs), total = nrows * ndw;
    for (int i0 = tid; i0 < total; i0 += NT * STAGE_U) {
      uint32_t v[STAGE_U];
      int ibs[STAGE_U], irs[STAGE_U];
#pragma unroll
      for (int u = 0; u < STAGE_U; ++u) {          // STAGE_U loads in flight: addresses clamped into the image, no branch
        const int i = min(i0 + u * NT, total - 1), rr = i / ndw, d = i - rr * ndw;
        irs[u] = r0 + rs + rr - r.pad_y;           // the canvas row's image row
        ibs[u] = 4 * d - px0;                      // the dword's first byte, counted from the image row's start
        v[u] = 0;
        if (wide_rows)
          v[u] = *reinterpret_cast<const u32_una*>(r.image + (size_t)clampi(irs[u], 0, H - 1) * wc + clampi(ibs[u], 0, wc - 4));
      }
#pragma unroll
      for (int u = 0; u < STAGE_U; ++u) {
        const int i = i0 + u * NT, ir = irs[u], ib = ibs[u];
        if (i >= total || ir < 0 || ir >= H) continue;       // a background row: not staged, its result is written below
        const int rr = i / ndw, d = i - rr * ndw;
        uint32_t w = v[u];
        if (!(wide_rows && ib >= 0 && ib + 4 <= wc)) {       // the row's ends and the background: never a load outside the image row
          const uint8_t* a = r.image + (size_t)ir * wc;
          w = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int jb = ib + j;
            const uint32_t b = (jb >= 0 && jb < wc) ? (uint32_t)a[jb] : bg_byte(cc.bg, (4 * d + j) % C);
            w |= b << (8 * j);
          }
        }
        reinterpret_cast<uint32_t*>(srow + (size_t)rr * wcp)[d] = w;
      }
    }
    __syncthreads();
    // the byte window of pil8.hpp; its over-read lands in the next staged row or in SLACK
    for (int xx = tid; xx < S; xx += NT) {
      int kreg[KS], o = o0;
#pragma unroll
      for (int x = 0; x < KS; ++x) kreg[x] = kreg0[x];
      if (xx != tid) {                             // sizes above NT: the further pixels' coefficients are read per round
        const int xo = left + xx;
        const int xmin = clampi(bx[2 * xo], 0, cw - 1), cnt = bx[2 * xo + 1];
#pragma unroll
        for (int x = 0; x < KS; ++x) kreg[x] = (x < cnt && x < ksx) ? kx[(size_t)xo * ksx + x] : 0;
        o = xmin * C;
      }
      const int sh = o & 3;
      const uint8_t* first = srow + (o & ~3);
      for (int rr = 0; rr < nrows; ++rr) {
        uint8_t* op = inter + (size_t)(rs + rr) * ocp + xx * C;
        const int ir = r0 + rs + rr - r.pad_y;
        if (ir < 0 || ir >= H) {                   // block-uniform
#pragma unroll
          for (int c = 0; c < C; ++c) op[c] = (uint8_t)bg_byte(cc.bg, c);
        } else {
          pil_h_window<C, KS>(reinterpret_cast<const uint32_t*>(first + (size_t)rr * wcp), sh, kreg, op);
        }
      }
    }
    __syncthreads();
  }

  // ---- vertical pass: inter -> planar rows; a lane owns four consecutive pixels of one plane (one 16- or 8-byte store)
  const int ksy = r.ksize_y;
  const bool vec = (S & 3) == 0;
  const int per = vec ? 4 : 1, groups = C * S / per;
  for (int yy = y0; yy < y1; ++yy) {
    const int yo = top + yy;
    const int rel = clampi(by[2 * yo], 0, ch - 1) - r0, cnt = min(by[2 * yo + 1], ksy);
    const int* k = kyl + (yy - y0) * ksy;
    for (int g = tid; g < groups; g += NT) {
      const int i = g * per, c = i / S, xx = i - c * S;
      const uint8_t* col = inter + xx * C + c;
      const float* lc = lut + c * 256;
      OutT* o = oimg + ((size_t)c * S + yy) * S + xx;
      if (vec) {
        int a0 = PIL_ROUND_HALF, a1 = a0, a2 = a0, a3 = a0;
        for (int t = 0; t < cnt; ++t) {
          const int kv = k[t];
          const uint8_t* row = col + (size_t)clampi(rel + t, 0, nr - 1) * ocp;
          mad24(a0, row[0], kv);
          mad24(a1, row[C], kv);
          mad24(a2, row[2 * C], kv);
          mad24(a3, row[3 * C], kv);
        }
        store4(o, lc[pil_clip8(a0)], lc[pil_clip8(a1)], lc[pil_clip8(a2)], lc[pil_clip8(a3)]);
      } else {
        int a0 = PIL_ROUND_HALF;
        for (int t = 0; t < cnt; ++t) {
          mad24(a0, col[(size_t)clampi(rel + t, 0, nr - 1) * ocp], k[t]);
        }
        *o = from_f32<OutT>(lc[pil_clip8(a0)]);
      }
    }
  }
}

// ---- the two-launch route: one thread per output element, taps from memory, the uint8 intermediate in `tmp`.
// Horizontal pass first ([canvas_h, S*C] in between), or -- vertical_first images, which have no padding -- vertical pass
// first ([S, W*C]).
struct Taps { int lo, cnt; const int32_t* k; };
__device__ __forceinline__ Taps taps_of(const int32_t* bounds, const int32_t* kk, int ksize, int o, int n_in) {
  const int lo = clampi(bounds[2 * o], 0, n_in - 1);
  return Taps{lo, min(min(bounds[2 * o + 1], ksize), n_in - lo), kk + (size_t)o * ksize};
}

__global__ __launch_bounds__(NT) void clip_ragged_first_kernel(const ClipImageDev* __restrict__ images,
                                                               const ClipItem* __restrict__ items, int C, int S, uint32_t bg,
                                                               uint8_t* __restrict__ tmp) {
  const ClipItem it = items[blockIdx.x];
  const ClipImageDev& im = images[it.img];
  const attwarp_clip_image& r = im.r;
  const int wc = r.W * C, L = r.vertical_first ? wc : S * C;              // bytes of an intermediate row
  uint8_t* t = tmp + im.tmp_off;
  for (int e = threadIdx.x; e < it.ny * L; e += NT) {
    const int row = it.y0 + e / L, j = e % L;
    uint8_t v;
    if (r.vertical_first) {
      const Taps tp = taps_of(r.bounds_y, r.kk_y, r.ksize_y, r.top + row, r.H);
      v = pil_tap_sum(r.image + (size_t)tp.lo * wc + j, (size_t)wc, tp.k, tp.cnt);
    } else {
      const int c = j % C, ir = row - r.pad_y;
      if (ir < 0 || ir >= r.H) {
        v = (uint8_t)bg_byte(bg, c);
      } else {
        const Taps tp = taps_of(r.bounds_x, r.kk_x, r.ksize_x, r.left + j / C, r.canvas_w);
        const uint8_t* a = r.image + (size_t)ir * wc + c;
        int ss = PIL_ROUND_HALF;
        for (int i = 0; i < tp.cnt; ++i) {
          const int ic = tp.lo + i - r.pad_x;
          ss += (int)((ic >= 0 && ic < r.W) ? (uint32_t)a[ic * C] : bg_byte(bg, c)) * tp.k[i];
        }
        v = pil_clip8(ss);
      }
    }
    t[(size_t)row * L + j] = v;
  }
}

template <typename OutT>
__global__ __launch_bounds__(NT) void clip_ragged_second_kernel(const ClipImageDev* __restrict__ images,
                                                                const ClipItem* __restrict__ items, int C, int S, ClipConst cc,
                                                                const uint8_t* __restrict__ tmp, OutT* __restrict__ out) {
  __shared__ float lut[MAX_C * 256];
  for (int c = 0; c < C; ++c) lut[c * 256 + threadIdx.x] = epilogue(threadIdx.x, cc.mean[c], cc.stdv[c]);
  __syncthreads();
  const ClipItem it = items[blockIdx.x];
  const ClipImageDev& im = images[it.img];
  const attwarp_clip_image& r = im.r;
  const int wc = r.W * C, oc = S * C, plane = C * S;
  const uint8_t* t = tmp + im.tmp_off;
  OutT* oimg = out + (size_t)it.img * C * S * S;
  for (int e = threadIdx.x; e < it.ny * plane; e += NT) {
    const int q = e / plane, rem = e - q * plane, c = rem / S, xx = rem - c * S, yy = it.y0 + q;
    uint8_t v;
    if (r.vertical_first) {
      const Taps tp = taps_of(r.bounds_x, r.kk_x, r.ksize_x, r.left + xx, r.W);
      v = pil_tap_sum(t + (size_t)yy * wc + tp.lo * C + c, (size_t)C, tp.k, tp.cnt);
    } else {
      const Taps tp = taps_of(r.bounds_y, r.kk_y, r.ksize_y, r.top + yy, r.canvas_h);
      v = pil_tap_sum(t + (size_t)tp.lo * oc + xx * C + c, (size_t)oc, tp.k, tp.cnt);
    }
    oimg[((size_t)c * S + yy) * S + xx] = from_f32<OutT>(lut[c * 256 + v]);
  }
}

// ---- host: the table of one batch
struct ClipLayout {
  attwarp_clip_header h;
  std::vector<ClipImageDev> images;
  std::vector<ClipItem> fused, wide, hitems, vitems;      // fused: the 8-tap window; wide: 9 .. 16 horizontal taps
};

static size_t fused_lds(long long ny, long long ksize_y, long long nr, long long ocp, long long rb, long long wcp) {
  return (size_t)(LUT_BYTES + ny * ksize_y * 4 + nr * ocp + rb * wcp + SLACK);
}

// canvas rows a band of ny output rows can touch: the first taps of two rows ny - 1 apart lie at most
// floor((ny - 1) * scale) + 1 apart, the last row adds its ksize_y taps
static long long band_rows(int ny, int n_in, int n_out, int ksize_y) {
  const long long nr = (long long)(ny - 1) * n_in / n_out + 2 + ksize_y;
  return nr < n_in ? nr : n_in;
}

static int clip_layout(const attwarp_clip_image* images, int B, int C, int S, ClipLayout& L) {
  ATTWARP_REQUIRE(images, "clip_images: null image list");
  ATTWARP_REQUIRE(B > 0 && S > 0, "clip_images: non-positive size");
  ATTWARP_REQUIRE(C == 1 || C == 3, "clip_images: C must be 1 or 3 (got %d)", C);
  if (B > (1 << 20) || S > MAX_SIZE) return fail(ATTWARP_E_UNSUPPORTED, "clip_images: B > 2^20 or size > %d", MAX_SIZE);
  const bool force_split = tune(TUNE_CLIP_RAGGED_VARIANT) == 1;
  const long long oc = (long long)S * C, ocp = (oc + 3) & ~3LL;
  attwarp_clip_header& h = L.h;
  memset(&h, 0, sizeof(h));
  h.magic = CLIPR_MAGIC; h.B = B; h.C = C; h.size = S; h.ks = 8;
  L.images.resize((size_t)B);
  size_t lds = 0;
  long long tmp = 0;
  for (int b = 0; b < B; ++b) {
    const attwarp_clip_image& r = images[b];
    ATTWARP_REQUIRE(r.image && r.bounds_x && r.kk_x && r.bounds_y && r.kk_y, "clip_images: image %d: null pointer", b);
    ATTWARP_REQUIRE(r.H > 0 && r.W > 0 && r.ksize_x > 0 && r.ksize_y > 0 && r.nw > 0 && r.nh > 0,
                    "clip_images: image %d: non-positive size", b);
    ATTWARP_REQUIRE(r.pad_x >= 0 && r.pad_y >= 0 && (long long)r.pad_x + r.W <= r.canvas_w && (long long)r.pad_y + r.H <= r.canvas_h,
                    "clip_images: image %d: %d x %d at (%d, %d) does not lie on its %d x %d canvas", b, r.H, r.W, r.pad_y,
                    r.pad_x, r.canvas_h, r.canvas_w);
    if (r.canvas_w > MAX_CANVAS || r.canvas_h > MAX_CANVAS)
      return fail(ATTWARP_E_UNSUPPORTED, "clip_images: image %d: canvas %d x %d exceeds %d", b, r.canvas_h, r.canvas_w, MAX_CANVAS);
    if (r.nw > (1 << 20) || r.nh > (1 << 20))
      return fail(ATTWARP_E_UNSUPPORTED, "clip_images: image %d: resized to %d x %d, beyond 2^20", b, r.nh, r.nw);
    ATTWARP_REQUIRE(r.left >= 0 && r.top >= 0 && (long long)r.left + S <= r.nw && (long long)r.top + S <= r.nh,
                    "clip_images: image %d: the %d x %d crop at (%d, %d) leaves the %d x %d resized image", b, S, S, r.top,
                    r.left, r.nh, r.nw);
    ATTWARP_REQUIRE(!r.vertical_first || (r.canvas_w == r.W && r.canvas_h == r.H),
                    "clip_images: image %d: a vertical-first image cannot be padded", b);
    ClipImageDev& d = L.images[(size_t)b];
    memset(&d, 0, sizeof(d));
    d.r = r;
    const long long wcp = ((long long)r.canvas_w * C + 3) & ~3LL;
    // band height from the vertical scale: neighbouring bands share about 2 * max(scale, 1) canvas rows, a band of ny
    // output rows spans ny * scale, so 14 * max(1, nh / canvas_h) output rows keep the recomputed share near an eighth
    const int ny = r.nh <= r.canvas_h ? 16 : (14LL * r.nh <= 32LL * r.canvas_h ? 32 : 64);
    bool fused = !force_split && !r.vertical_first && r.ksize_x <= 16;
    if (fused) {
      fused = false;
      for (int pass = 0; pass < 2 && !fused; ++pass)            // first a plan two workgroups of which fit a CU's LDS
        for (int n = ny; n >= 8 && !fused; n >>= 1)
          for (int rb = 8; rb >= 4 && !fused; rb >>= 1) {
            const long long nr = band_rows(n < S ? n : S, r.canvas_h, r.nh, r.ksize_y);
            if (fused_lds(n, r.ksize_y, nr, ocp, rb, wcp) <= (pass == 0 ? LDS_CU_BYTES / 2 : LDS_CU_BYTES)) {
              fused = true; d.ny = n; d.rb = rb; d.nr_cap = (int32_t)nr;
            }
          }
    }
    d.fused = fused;
    if (fused) {
      ++h.n_fused_images;
      d.window = r.ksize_x > 8 ? 16 : 8;
      if (d.window > h.ks) h.ks = d.window;
      const size_t need = fused_lds(d.ny, r.ksize_y, d.nr_cap, ocp, d.rb, wcp);
      if (need > lds) lds = need;
      std::vector<ClipItem>& list = r.ksize_x > 8 ? L.wide : L.fused;      // (a launch of its own: the others keep 8 taps)
      for (int y0 = 0; y0 < S; y0 += d.ny) list.push_back(ClipItem{b, y0, S - y0 < d.ny ? S - y0 : d.ny, 0});
    } else {
      ++h.n_split_images;
      d.tmp_off = tmp;
      const int rows1 = r.vertical_first ? S : r.canvas_h;         // rows of the intermediate
      tmp += ((long long)rows1 * (r.vertical_first ? (long long)r.W * C : oc) + 3) & ~3LL;
      for (int y0 = 0; y0 < rows1; y0 += SPLIT_H_ROWS)
        L.hitems.push_back(ClipItem{b, y0, rows1 - y0 < SPLIT_H_ROWS ? rows1 - y0 : SPLIT_H_ROWS, 0});
      for (int y0 = 0; y0 < S; y0 += SPLIT_V_ROWS)
        L.vitems.push_back(ClipItem{b, y0, S - y0 < SPLIT_V_ROWS ? S - y0 : SPLIT_V_ROWS, 0});
    }
  }
  L.fused.insert(L.fused.end(), L.wide.begin(), L.wide.end());        // 8-tap items first, then the wide ones
  const size_t nitems = L.fused.size() + L.hitems.size() + L.vitems.size();
  if (nitems > 0x7fffffffu) return fail(ATTWARP_E_UNSUPPORTED, "clip_images: too many work items");
  h.n_wide_items = (int32_t)L.wide.size();
  h.n_fused_items = (int32_t)L.fused.size(); h.n_h_items = (int32_t)L.hitems.size(); h.n_v_items = (int32_t)L.vitems.size();
  h.tmp_bytes = (uint64_t)tmp; h.lds_bytes = lds;
  h.off_images = (sizeof(attwarp_clip_header) + 15) & ~(size_t)15;
  h.off_items = h.off_images + (size_t)B * sizeof(ClipImageDev);
  h.table_bytes = (h.off_items + nitems * sizeof(ClipItem) + 15) & ~(uint64_t)15;
  return ATTWARP_OK;
}

template <typename OutT, int C, int KS>
static int launch_fused_one(const attwarp_clip_header* h, const ClipImageDev* images, const ClipItem* items, int n,
                            const ClipConst& cc, OutT* out, hipStream_t st) {
  const size_t lds = (size_t)h->lds_bytes;
  if (const int rc = grant_dynamic_lds(clip_ragged_fused_kernel<OutT, C, KS>, lds, "clip_images_u8")) return rc;
  hipLaunchKernelGGL((clip_ragged_fused_kernel<OutT, C, KS>), dim3(n), dim3(NT), lds, st, images, items, h->size, cc, out);
  return check_launch("clip_ragged_fused_kernel");
}

template <typename OutT, int C>
static int launch_fused(const attwarp_clip_header* h, const ClipImageDev* images, const ClipItem* items, const ClipConst& cc,
                        OutT* out, hipStream_t st) {
  const int n8 = h->n_fused_items - h->n_wide_items;
  if (n8 > 0)
    if (const int rc = launch_fused_one<OutT, C, 8>(h, images, items, n8, cc, out, st)) return rc;
  if (h->n_wide_items > 0)          // canvases shrunk 1.5 .. 3.5 times: the 16-tap window, a launch of their own
    if (const int rc = launch_fused_one<OutT, C, 16>(h, images, items + n8, h->n_wide_items, cc, out, st)) return rc;
  return ATTWARP_OK;
}

template <typename OutT>
static int launch_all(const attwarp_clip_header* h, const ClipImageDev* images, const ClipItem* items, const ClipConst& cc,
                      uint8_t* tmp, OutT* out, hipStream_t st) {
  if (h->n_fused_items > 0)
    if (const int rc = h->C == 1 ? launch_fused<OutT, 1>(h, images, items, cc, out, st) : launch_fused<OutT, 3>(h, images, items, cc, out, st))
      return rc;
  if (h->n_h_items > 0) {
    hipLaunchKernelGGL(clip_ragged_first_kernel, dim3(h->n_h_items), dim3(NT), 0, st, images, items + h->n_fused_items, h->C,
                       h->size, cc.bg, tmp);
    if (const int rc = check_launch("clip_ragged_first_kernel")) return rc;
    hipLaunchKernelGGL((clip_ragged_second_kernel<OutT>), dim3(h->n_v_items), dim3(NT), 0, st, images,
                       items + h->n_fused_items + h->n_h_items, h->C, h->size, cc, tmp, out);
    if (const int rc = check_launch("clip_ragged_second_kernel")) return rc;
  }
  return ATTWARP_OK;
}

}  // namespace clipr
}  // namespace attwarp

using namespace attwarp;
using namespace attwarp::clipr;

extern "C" size_t attwarp_clip_images_table_bytes(const attwarp_clip_image* images, int B, int C, int size) try {
  ClipLayout L;
  if (clip_layout(images, B, C, size, L) != ATTWARP_OK) return 0;
  return (size_t)L.h.table_bytes;
} catch (...) {
  fail(ATTWARP_E_UNSUPPORTED, "clip_images_table_bytes: out of host memory");
  return 0;
}

extern "C" int attwarp_clip_images_plan(const attwarp_clip_image* images, int B, int C, int size, void* table,
                                        size_t table_bytes) try {
  ATTWARP_REQUIRE(table, "clip_images_plan: null table");
  ClipLayout L;
  if (const int rc = clip_layout(images, B, C, size, L)) return rc;
  ATTWARP_REQUIRE(table_bytes >= L.h.table_bytes, "clip_images_plan: the table needs %llu bytes (got %zu)",
                  (unsigned long long)L.h.table_bytes, table_bytes);
  uint8_t* t = static_cast<uint8_t*>(table);
  memset(t, 0, (size_t)L.h.table_bytes);
  memcpy(t, &L.h, sizeof(L.h));
  memcpy(t + L.h.off_images, L.images.data(), L.images.size() * sizeof(ClipImageDev));
  ClipItem* items = reinterpret_cast<ClipItem*>(t + L.h.off_items);
  if (!L.fused.empty()) memcpy(items, L.fused.data(), L.fused.size() * sizeof(ClipItem));
  if (!L.hitems.empty()) memcpy(items + L.fused.size(), L.hitems.data(), L.hitems.size() * sizeof(ClipItem));
  if (!L.vitems.empty()) memcpy(items + L.fused.size() + L.hitems.size(), L.vitems.data(), L.vitems.size() * sizeof(ClipItem));
  return ATTWARP_OK;
} catch (...) {
  return fail(ATTWARP_E_UNSUPPORTED, "clip_images_plan: out of host memory");
}

extern "C" int attwarp_clip_images_u8(const void* table_host, const void* table_dev, const float* mean, const float* stdv,
                                      const uint8_t* background, uint8_t* tmp, void* out, int out_dtype, void* stream) {
  ATTWARP_REQUIRE(table_host && table_dev && mean && stdv && background && out, "clip_images_u8: null pointer");
  const attwarp_clip_header* h = static_cast<const attwarp_clip_header*>(table_host);
  ATTWARP_REQUIRE(h->magic == CLIPR_MAGIC, "clip_images_u8: the table was not written by attwarp_clip_images_plan");
  ATTWARP_REQUIRE(out_dtype == ATTWARP_F32 || out_dtype == ATTWARP_F16, "clip_images_u8: out dtype must be F32 or F16");
  ATTWARP_REQUIRE((reinterpret_cast<uintptr_t>(table_dev) & 7u) == 0, "clip_images_u8: the device table must be 8-byte aligned");
  ATTWARP_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15u) == 0, "clip_images_u8: out must be 16-byte aligned");
  ATTWARP_REQUIRE(h->tmp_bytes == 0 || tmp, "clip_images_u8: this batch needs %llu bytes of tmp", (unsigned long long)h->tmp_bytes);
  ClipConst cc;
  memset(&cc, 0, sizeof(cc));
  for (int c = 0; c < MAX_C; ++c) cc.stdv[c] = 1.0f;
  for (int c = 0; c < h->C; ++c) {
    cc.mean[c] = mean[c]; cc.stdv[c] = stdv[c];
    cc.bg |= (uint32_t)background[c] << (8 * c);
  }
  hipStream_t st = as_stream(stream);
  const uint8_t* td = static_cast<const uint8_t*>(table_dev);
  const ClipImageDev* images = reinterpret_cast<const ClipImageDev*>(td + h->off_images);
  const ClipItem* items = reinterpret_cast<const ClipItem*>(td + h->off_items);
  return out_dtype == ATTWARP_F32 ? launch_all<float>(h, images, items, cc, tmp, static_cast<float*>(out), st)
                                  : launch_all<__half>(h, images, items, cc, tmp, static_cast<__half*>(out), st);
}
