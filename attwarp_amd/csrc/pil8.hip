// Pillow's 8-bit resampler outside the kernels that fuse it into something larger: the host builder of its coefficient
// tables, which every resampling kernel consumes (clip.hip, dataprep.hip, the chains), and
//   A4  ToPILImage (x255, truncate) + PIL resize(LANCZOS) of the token-grid mask   AGW/attention_extraction/llava.py:192-196,243,253
// The arithmetic is pil8.hpp's; the column-strip body the chains share is lanczos_strip_block (mask_blocks.hpp).
#include "common.hpp"
#include "mask_blocks.hpp"

#include <cmath>
#include <vector>

namespace attwarp {

constexpr int NT = 256;

// ---- A4: the LANCZOS up-sampling of the mask, arithmetic from pil8.hpp ----
// (quantises a float source on the fly, so it keeps a tap loop of its own)
// horizontal pass: tmp[b][y][xx], one thread per output.  grid = (ceil(out_w/NT), h, B)
__global__ __launch_bounds__(NT) void lanczos_h_kernel(const float* __restrict__ mf, const uint8_t* __restrict__ mu,
                                                       int h, int w, int out_w, const int32_t* __restrict__ bounds,
                                                       const int32_t* __restrict__ kk, int ksize,
                                                       uint8_t* __restrict__ tmp) {
  const int xx = blockIdx.x * NT + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (xx >= out_w) return;
  const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
  const int32_t* k = kk + (size_t)xx * ksize;
  const size_t row = ((size_t)b * h + y) * w;
  int ss = PIL_ROUND_HALF;
  for (int x = 0; x < cnt; ++x) {
    const int px = mf ? (int)to_pil_u8(mf[row + xmin + x]) : (int)mu[row + xmin + x];
    ss += px * k[x];
  }
  tmp[((size_t)b * h + y) * out_w + xx] = pil_clip8(ss);
}

// vertical pass.  grid = (ceil(out_w/NT), out_h, B)
__global__ __launch_bounds__(NT) void lanczos_v_kernel(const uint8_t* __restrict__ tmp, int h, int out_w, int out_h,
                                                       const int32_t* __restrict__ bounds,
                                                       const int32_t* __restrict__ kk, int ksize,
                                                       uint8_t* __restrict__ out) {
  const int xx = blockIdx.x * NT + threadIdx.x, yy = blockIdx.y, b = blockIdx.z;
  if (xx >= out_w) return;
  const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
  out[((size_t)b * out_h + yy) * out_w + xx] =
      pil_tap_sum(tmp + ((size_t)b * h + ymin) * out_w + xx, (size_t)out_w, kk + (size_t)yy * ksize, cnt);
}

// vertical pass, 4 pixels per thread (out_w % 4 == 0): 4-byte loads and stores, 256 B per wave instruction.
// grid = (ceil(out_w/4/NT), out_h, B)
__global__ __launch_bounds__(NT) void lanczos_v4_kernel(const uint8_t* __restrict__ tmp, int h, int out_w, int out_h,
                                                        const int32_t* __restrict__ bounds,
                                                        const int32_t* __restrict__ kk, int ksize,
                                                        uint8_t* __restrict__ out) {
  const int x4 = blockIdx.x * NT + threadIdx.x, yy = blockIdx.y, b = blockIdx.z;
  if (x4 * 4 >= out_w) return;
  const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
  const uint8_t* col = tmp + ((size_t)b * h + ymin) * out_w + (size_t)x4 * 4;
  *reinterpret_cast<uint32_t*>(out + ((size_t)b * out_h + yy) * out_w + (size_t)x4 * 4) =
      pil_tap_sum4(col, (size_t)out_w, kk + (size_t)yy * ksize, cnt);
}

// Both passes in one launch for SMALL sources (the 24 x 24 token grid): the workgroup of (image, block of R output
// rows) quantises the source rows it needs into LDS, runs the horizontal pass for them into an LDS uint8 tile
// [h][out_w] and the vertical pass from that tile, 4 output pixels per thread (one ds_read_b32 per tap row, one
// dword store).  Same integer arithmetic as the two-kernel form; no tmp round trip, one launch instead of two.
// What reaches it: masks that shrink vertically while they grow horizontally (9 .. 32 vertical taps).  With 8 vertical
// taps the dispatcher takes the column-strip kernel unless that kernel's LDS does not fit, h * (256 + w) > 48 KiB with
// h * w <= 4096: a mask of at least 177 rows and at most 23 columns, which no token grid is (ragged_plan caps g at 32).
// So the vertical pass has one form for every tap count up to 32, not tuned for 8: up-sampling on both axes runs here
// only under the tuning knob lanczos_variant = 2.
// grid = (ceil(out_h / R), B); out_w % 4 == 0; ksize_x <= KS; ksize_y <= 32; R <= 64.  LDS: src[h*w] | tile[h*out_w]
template <int KS>
__global__ __launch_bounds__(NT) void lanczos_fused_kernel(const float* __restrict__ mf, const uint8_t* __restrict__ mu,
                                                           int h, int w, int out_h, int out_w,
                                                           const int32_t* __restrict__ bounds_x,
                                                           const int32_t* __restrict__ kk_x, int ksize_x,
                                                           const int32_t* __restrict__ bounds_y,
                                                           const int32_t* __restrict__ kk_y, int ksize_y, int R,
                                                           uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lz[];
  __shared__ int32_t s_ky[64 * 32];                  // vertical coefficients and bounds of the block's rows (R <= 64)
  __shared__ int32_t s_by[64 * 2];
  const int srcp = (h * w + 3) & ~3;
  uint8_t* src = lz;
  uint8_t* tile = lz + srcp;
  const int tid = threadIdx.x, b = blockIdx.y;
  const int yy0 = blockIdx.x * R, yy1 = min(yy0 + R, out_h), nrows = yy1 - yy0;
  const int ys = bounds_y[2 * yy0];                                          // first / one-past-last source row
  const int ye = bounds_y[2 * (yy1 - 1)] + bounds_y[2 * (yy1 - 1) + 1];
  const size_t ib = (size_t)b * h * w;
  for (int i = ys * w + tid; i < ye * w; i += NT) src[i] = mf ? to_pil_u8(mf[ib + i]) : mu[ib + i];
  for (int i = tid; i < nrows * ksize_y; i += NT) s_ky[i] = kk_y[(size_t)yy0 * ksize_y + i];
  if (tid < 2 * nrows) s_by[tid] = bounds_y[2 * yy0 + tid];
  __syncthreads();
  for (int xx = tid; xx < out_w; xx += NT) {
    const int xmin = bounds_x[2 * xx], cnt = bounds_x[2 * xx + 1];
    int kreg[KS], toff[KS];
#pragma unroll
    for (int x = 0; x < KS; ++x) {
      kreg[x] = (x < cnt) ? kk_x[(size_t)xx * ksize_x + min(x, ksize_x - 1)] : 0;
      toff[x] = xmin + min(x, cnt - 1);
    }
    for (int r = ys; r < ye; ++r) {
      const uint8_t* row = src + r * w;
      int ss = PIL_ROUND_HALF;
#pragma unroll
      for (int x = 0; x < KS; ++x) ss += __mul24((int)row[toff[x]], kreg[x]);
      tile[r * out_w + xx] = pil_clip8(ss);
    }
  }
  __syncthreads();
  // vertical pass: a thread owns dword q of an output row; rows are spread over the threads left
  const int nq = out_w >> 2;
  const int rstep = nq >= NT ? 1 : NT / nq;          // rows in flight per sweep
  const int q0 = nq >= NT ? tid : tid % nq, r0 = nq >= NT ? 0 : tid / nq;
  if (r0 < rstep) {
    for (int ry = r0; ry < nrows; ry += rstep) {
      const int yy = yy0 + ry;
      const int ymin = s_by[2 * ry], cnt = s_by[2 * ry + 1];
      for (int q = q0; q < nq; q += NT)
        reinterpret_cast<uint32_t*>(out + ((size_t)b * out_h + yy) * out_w)[q] =
            pil_tap_sum4(tile + ymin * out_w + 4 * q, (size_t)out_w, s_ky + ry * ksize_y, cnt);
    }
  }
}

// Up-sampling form of the fused kernel (<= 8 taps on both axes): body lanczos_strip_block (mask_blocks.hpp).
// grid = (nstrips * nchunks, B).  LDS: src[h*w] | tile[h][256].   kk_y rows hold exactly 8 coefficients (zero padded).
template <int KS, bool UA>
__global__ __launch_bounds__(NT) void lanczos_strip_kernel(const LanczosStripArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lz[];
  const int b = blockIdx.y;
  lanczos_strip_block<KS, UA>(a, blockIdx.x, (size_t)b * a.h * a.w, a.out + (size_t)b * a.out_h * a.out_w, lz);
}

// copy / quantise pass used when an axis keeps its size (Pillow skips that pass)
__global__ __launch_bounds__(NT) void quantise_copy_kernel(const float* __restrict__ mf, const uint8_t* __restrict__ mu,
                                                           size_t n, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i < n) out[i] = mf ? to_pil_u8(mf[i]) : mu[i];
}

// ---- host: Pillow's coefficient tables (ImagingResample precompute_coeffs + normalize_coeffs_8bpc, Resample.c) -------
static double pil_sinc(double x) {
  if (x == 0.0) return 1.0;
  x *= M_PI;
  return sin(x) / x;
}
static double pil_lanczos3(double x) { return (-3.0 <= x && x < 3.0) ? pil_sinc(x) * pil_sinc(x / 3.0) : 0.0; }
static double pil_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
static double pil_bilinear(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

}  // namespace attwarp

using namespace attwarp;

extern "C" int attwarp_pil_coeffs_8bpc(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk, int kk_cols) try {
  ATTWARP_REQUIRE(bounds && kk, "pil_coeffs_8bpc: null pointer");
  ATTWARP_REQUIRE(in_size > 0 && out_size > 0 && kk_cols > 0, "pil_coeffs_8bpc: non-positive size");
  ATTWARP_REQUIRE(filter == ATTWARP_PIL_LANCZOS || filter == ATTWARP_PIL_BICUBIC || filter == ATTWARP_PIL_BILINEAR,
                  "pil_coeffs_8bpc: unknown filter %d", filter);
  double (*fn)(double) = filter == ATTWARP_PIL_LANCZOS ? pil_lanczos3 : filter == ATTWARP_PIL_BICUBIC ? pil_bicubic : pil_bilinear;
  const double support0 = filter == ATTWARP_PIL_LANCZOS ? 3.0 : filter == ATTWARP_PIL_BICUBIC ? 2.0 : 1.0;
  if (in_size == out_size) {     // Pillow skips the pass; an identity table makes clip8((v << 22 + 2^21) >> 22) == v
    for (int o = 0; o < out_size; ++o) {
      bounds[2 * o] = o; bounds[2 * o + 1] = 1;
      for (int i = 0; i < kk_cols; ++i) kk[(size_t)o * kk_cols + i] = i == 0 ? (1 << PIL_PRECISION_BITS) : 0;
    }
    return 1;
  }
  const double scale = (double)in_size / (double)out_size;
  const double fscale = scale < 1.0 ? 1.0 : scale;
  const double support = support0 * fscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  if (ksize > kk_cols) return fail(ATTWARP_E_ARG, "pil_coeffs_8bpc: %d taps do not fit %d columns", ksize, kk_cols);
  const double ss = 1.0 / fscale;
  std::vector<double> w((size_t)ksize);
  for (int o = 0; o < out_size; ++o) {
    const double center = (o + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in_size) hi = in_size;
    const int cnt = hi - lo;
    double tot = 0.0;
    for (int i = 0; i < cnt; ++i) {
      w[i] = fn((i + lo - center + 0.5) * ss);
      tot += w[i];
    }
    for (int i = 0; i < cnt; ++i)
      if (tot != 0.0) w[i] /= tot;
    int32_t* row = kk + (size_t)o * kk_cols;
    for (int i = 0; i < kk_cols; ++i) row[i] = 0;
    for (int i = 0; i < cnt; ++i) row[i] = (int32_t)((w[i] < 0 ? -0.5 : 0.5) + w[i] * (1 << PIL_PRECISION_BITS));
    bounds[2 * o] = lo; bounds[2 * o + 1] = cnt;
  }
  return ksize;
} catch (...) {
  return fail(ATTWARP_E_UNSUPPORTED, "pil_coeffs_8bpc: out of host memory");
}

extern "C" int attwarp_mask_upsample_lanczos(const float* mask_f32, const uint8_t* mask_u8, int B, int h, int w,
                                             int out_h, int out_w, const int32_t* bounds_x, const int32_t* kk_x,
                                             int ksize_x, const int32_t* bounds_y, const int32_t* kk_y, int ksize_y,
                                             uint8_t* tmp, uint8_t* out, void* stream) {
  ATTWARP_REQUIRE((mask_f32 != nullptr) != (mask_u8 != nullptr), "mask_upsample_lanczos: pass exactly one of mask_f32 / mask_u8");
  ATTWARP_REQUIRE(out, "mask_upsample_lanczos: null output");
  ATTWARP_REQUIRE(B > 0 && h > 0 && w > 0 && out_h > 0 && out_w > 0, "mask_upsample_lanczos: non-positive size");
  if (B > 65535 || h > 65535 || out_h > 65535) return fail(ATTWARP_E_UNSUPPORTED, "mask_upsample_lanczos: dims > 65535");
  const bool need_h = out_w != w, need_v = out_h != h;
  ATTWARP_REQUIRE(!need_h || (bounds_x && kk_x && ksize_x > 0), "mask_upsample_lanczos: missing x coefficients");
  ATTWARP_REQUIRE(!need_v || (bounds_y && kk_y && ksize_y > 0), "mask_upsample_lanczos: missing y coefficients");
  ATTWARP_REQUIRE(!(need_h && need_v) || tmp, "mask_upsample_lanczos: tmp workspace required for a two-pass resize");
  hipStream_t st = as_stream(stream);
  if (!need_h && !need_v) {
    const size_t n = (size_t)B * h * w;
    hipLaunchKernelGGL(quantise_copy_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, mask_f32, mask_u8, n, out);
    return check_launch("quantise_copy_kernel");
  }
  // up-sampling of a small source with <= 8 taps per axis (the 24 x 24 token grid): column-strip kernel
  if (need_h && need_v && tune(TUNE_LANCZOS_VARIANT) <= 0 && (long long)h * w <= 4096 && ksize_x <= 8 &&
      ksize_y == 8 && (size_t)((h * w + 3) & ~3) + (size_t)h * NT <= 48 * 1024) {
    // rows that do not start on dword boundaries (out_w % 4 != 0, e.g. the mask of a 683-pixel-wide image): the UA form
    const bool ua = out_w % 4 != 0 || (reinterpret_cast<uintptr_t>(out) & 3u) != 0;
    const int nstrips = (out_w + NT - 1) / NT;
    // enough workgroups to fill the chip (~4096: measured 1024x1024 B=256, rows per chunk 512 / 256 / 128 / 64:
    // 108 / 105 / 111 / 127 us), at least 16 rows per wave
    long long nchunks = (4096 + (long long)B * nstrips - 1) / ((long long)B * nstrips);
    const int max_chunks = (out_h + 63) / 64;
    if (nchunks > max_chunks) nchunks = max_chunks;
    if (nchunks < 1) nchunks = 1;
    const int rows_per_chunk = (int)((out_h + nchunks - 1) / nchunks);
    nchunks = (out_h + rows_per_chunk - 1) / rows_per_chunk;
    const size_t lds = (size_t)((h * w + 3) & ~3) + (size_t)h * NT;
    LanczosStripArgs la{mask_f32, mask_u8, h, w, out_h, out_w, bounds_x, kk_x, ksize_x, bounds_y, kk_y, (int)nchunks, rows_per_chunk, out};
    if (ua) hipLaunchKernelGGL((lanczos_strip_kernel<8, true>), dim3((unsigned)(nstrips * nchunks), B), dim3(NT), lds, st, la);
    else hipLaunchKernelGGL((lanczos_strip_kernel<8, false>), dim3((unsigned)(nstrips * nchunks), B), dim3(NT), lds, st, la);
    return check_launch("lanczos_strip_kernel");
  }
  // small source and both passes needed, any tap count: one fused launch (row-block form)
  {
    const bool two_kernel = tune(TUNE_LANCZOS_VARIANT) == 1;      // 2: the row-block fused kernel
    const size_t lds = (size_t)((h * w + 3) & ~3) + (size_t)h * out_w;
    if (need_h && need_v && !two_kernel && (long long)h * w <= 4096 && out_w % 4 == 0 && ksize_x <= 8 &&
        ksize_y <= 32 &&
        lds <= 48 * 1024 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
      const int R = out_h >= 448 ? 64 : 32;   // measured: 24->336 R=32 27 us (two-kernel form 34), 24->1024 B=256 R=64 258 us (287)
      hipLaunchKernelGGL((lanczos_fused_kernel<8>), dim3((out_h + R - 1) / R, B), dim3(NT), lds, st, mask_f32, mask_u8,
                         h, w, out_h, out_w, bounds_x, kk_x, ksize_x, bounds_y, kk_y, ksize_y, R, out);
      return check_launch("lanczos_fused_kernel");
    }
  }
  const uint8_t* vsrc = mask_u8;
  if (need_h) {
    uint8_t* hdst = need_v ? tmp : out;
    hipLaunchKernelGGL(lanczos_h_kernel, dim3((out_w + NT - 1) / NT, h, B), dim3(NT), 0, st, mask_f32, mask_u8, h, w,
                       out_w, bounds_x, kk_x, ksize_x, hdst);
    int rc = check_launch("lanczos_h_kernel");
    if (rc) return rc;
    vsrc = hdst;
  } else if (mask_f32) {
    ATTWARP_REQUIRE(tmp, "mask_upsample_lanczos: tmp workspace required to quantise a float mask");
    const size_t n = (size_t)B * h * w;
    hipLaunchKernelGGL(quantise_copy_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, mask_f32, nullptr, n, tmp);
    int rc = check_launch("quantise_copy_kernel");
    if (rc) return rc;
    vsrc = tmp;
  }
  if (need_v) {
    const bool vec4 = (out_w % 4 == 0) && ((reinterpret_cast<uintptr_t>(vsrc) | reinterpret_cast<uintptr_t>(out)) % 4 == 0);
    if (vec4)
      hipLaunchKernelGGL(lanczos_v4_kernel, dim3((out_w / 4 + NT - 1) / NT, out_h, B), dim3(NT), 0, st, vsrc, h, out_w,
                         out_h, bounds_y, kk_y, ksize_y, out);
    else
      hipLaunchKernelGGL(lanczos_v_kernel, dim3((out_w + NT - 1) / NT, out_h, B), dim3(NT), 0, st, vsrc, h, out_w,
                         out_h, bounds_y, kk_y, ksize_y, out);
    return check_launch("lanczos_v_kernel");
  }
  return ATTWARP_OK;
}
