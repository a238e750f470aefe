// Jet heat-map overlays of the reference's drivers, for a whole batch of differently sized images per launch:
//   BLEND_MASK  : blend_mask, AGW/attention_extraction/llava.py:254-269 -- cv2.normalize(NORM_MINMAX) of the up-sampled
//                 uint8 mask, applyColorMap(COLORMAP_JET), addWeighted(image, 1 - a, heat, a, 0)
//   SAVE_WARPED : save_warped_image's overlay, AGW/new_method.py:455-475 -- numpy min-max in the map's own dtype with
//                 EPSILON = 1e-9, (x * 255).astype(uint8), applyColorMap(COLORMAP_JET), addWeighted(heat, a, image, 1 - a, 0)
// Two launches: overlay_minmax_kernel writes one (min, max) partial per block, overlay_color_kernel reduces an image's
// partials in its prologue (fixed order, NaN propagating like np.min / np.max), builds the 256-entry colour table of the
// image in LDS and streams the pixels: 1 byte (uint8 map) + 3 image bytes read, 3 bytes written, plus the map read once
// more by the first pass -- 8 bytes per pixel for a uint8 map.  Grid: (chunks, B); every image is cut into the same
// number of chunks of whole 1024-pixel units, so a block finds its image and its range with no table.
// The OpenCV arithmetic restated here (DESIGN.md "Heat-map overlay"): normalize's scale / shift in double rounded to
// float32 and one fmaf per value (convertTo's AVX2 path), addWeighted's nested fmaf with cvRound (half to even).
#include "common.hpp"
#include "overlay_jet.hpp"

namespace attwarp {

constexpr int OV_NT = 256;             // threads per block
constexpr int OV_UNIT = 4 * OV_NT;     // pixels per block iteration of the colour pass (4 per thread)
constexpr int OV_MAX_CHUNKS = 256;     // blocks per image: the colour prologue reads one partial per thread
constexpr int OV_CHUNK_PX = 8192;      // pixels per block aimed at (the mean image size sets the chunk count)

typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x3 u32x3_una __attribute__((aligned(1)));      // 12 / 16 bytes at ANY byte address (683 x 3-byte rows,
typedef u32x4 u32x4_una __attribute__((aligned(1)));      // images packed back to back): one dwordx3 / dwordx4 each
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef double f64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// The records are read from memory, so the compiler cannot tell that their pointers are global ones: without this it
// emits flat loads / stores (which also count against the LDS wait counter) for the pixel stream.
#define OV_G __attribute__((address_space(1)))

struct OvImage {                       // == attwarp_overlay_image
  const uint8_t* image;
  const void* map;
  uint8_t* out;
  int32_t H, W;
};
static_assert(sizeof(OvImage) == sizeof(attwarp_overlay_image), "descriptor layout");

struct OvParams {
  int k;                               // chunks (blocks) per image
  int style;                           // ATTWARP_OVERLAY_*
  int out_bgr;                         // channel order of the output (the image's order is out_bgr ^ SWAP)
  float w_img, w_heat;                 // addWeighted's weights of the image and of the heat map, as float32
};

// Chunk c of k of an image of n pixels: whole 1024-pixel units, the last chunks possibly empty.
__device__ __forceinline__ void ov_chunk(int64_t n, int c, int k, int64_t& lo, int64_t& hi) {
  const int64_t units = (n + OV_UNIT - 1) / OV_UNIT, per = (units + k - 1) / k;
  lo = min(n, (int64_t)c * per * OV_UNIT);
  hi = min(n, lo + per * OV_UNIT);
}

// ---- pass 1: per-block (min, max) ------------------------------------------------------------------------------------
struct MinMaxAcc {
  double mn = __builtin_inf(), mx = -__builtin_inf();
  bool nan = false;
};

template <typename T>
__device__ __forceinline__ void fold(MinMaxAcc& a, T v) {
  a.nan |= v != v;
  a.mn = fmin(a.mn, (double)v);        // fmin / fmax skip a NaN; the flag keeps it
  a.mx = fmax(a.mx, (double)v);
}

// Block reduction of (min, max, nan): exact and order independent (min / max are), the same in every thread.
__device__ __forceinline__ void block_minmax(MinMaxAcc& a, double* s_mn, double* s_mx, int* s_nan) {
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    a.mn = fmin(a.mn, __shfl_xor(a.mn, o, WAVE));
    a.mx = fmax(a.mx, __shfl_xor(a.mx, o, WAVE));
  }
  const bool wnan = __any(a.nan);
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  if (lane == 0) { s_mn[wid] = a.mn; s_mx[wid] = a.mx; s_nan[wid] = wnan; }
  __syncthreads();
  a = MinMaxAcc();
  for (int i = 0; i < OV_NT / WAVE; ++i) { a.mn = fmin(a.mn, s_mn[i]); a.mx = fmax(a.mx, s_mx[i]); a.nan |= s_nan[i] != 0; }
}

__device__ __forceinline__ void fold_u8x4(u16x2& mn, u16x2& mx, uint32_t w) {
  const uint32_t e = w & 0x00ff00ffu, o = (w >> 8) & 0x00ff00ffu;
  const u16x2 ev = __builtin_bit_cast(u16x2, e), ov = __builtin_bit_cast(u16x2, o);
  mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(ev, ov));
  mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(ev, ov));
}

template <typename T>
__global__ __launch_bounds__(OV_NT) void overlay_minmax_kernel(const OvImage* __restrict__ imgs, int k, double2* __restrict__ part) {
  __shared__ double s_mn[OV_NT / WAVE], s_mx[OV_NT / WAVE];
  __shared__ int s_nan[OV_NT / WAVE];
  const OvImage d = imgs[blockIdx.y];
  int64_t lo, hi;
  ov_chunk((int64_t)d.H * d.W, blockIdx.x, k, lo, hi);
  const OV_G T* __restrict__ m = (const OV_G T*)d.map;
  constexpr int V = 16 / sizeof(T);    // elements per 16-byte load
  MinMaxAcc a;
  if constexpr (sizeof(T) == 1) {
    u16x2 mn = {0xffff, 0xffff}, mx = {0, 0};
    for (int64_t p = lo + (int64_t)V * threadIdx.x; p < hi; p += (int64_t)V * OV_NT) {
      if (p + V <= hi) {
        const u32x4 w = *(const OV_G u32x4_una*)(m + p);
        fold_u8x4(mn, mx, w.x); fold_u8x4(mn, mx, w.y); fold_u8x4(mn, mx, w.z); fold_u8x4(mn, mx, w.w);
      } else {
        for (int64_t q = p; q < hi; ++q) fold_u8x4(mn, mx, (uint32_t)m[q] * 0x01010101u);
      }
    }
    if (lo < hi) {                     // (the 0xffff / 0 start values of an empty range are not pixel values)
      a.mn = (double)min(mn.x, mn.y);
      a.mx = (double)max(mx.x, mx.y);
    }
  } else {
    for (int64_t p = lo + (int64_t)V * threadIdx.x; p < hi; p += (int64_t)V * OV_NT) {
      if (p + V <= hi) {
        if constexpr (sizeof(T) == 4) {
          const f32x4_a4 v = *(const OV_G f32x4_a4*)(m + p);
          fold(a, v.x); fold(a, v.y); fold(a, v.z); fold(a, v.w);
        } else {
          const f64x2_a8 v = *(const OV_G f64x2_a8*)(m + p);
          fold(a, v.x); fold(a, v.y);
        }
      } else {
        for (int64_t q = p; q < hi; ++q) fold(a, m[q]);
      }
    }
  }
  block_minmax(a, s_mn, s_mx, s_nan);
  if (threadIdx.x == 0)
    part[(size_t)blockIdx.y * k + blockIdx.x] = a.nan ? make_double2(__builtin_nan(""), __builtin_nan("")) : make_double2(a.mn, a.mx);
}

// ---- the map value -> Jet index arithmetic ------------------------------------------------------------------------------
// blend_mask: cv2.normalize(m.astype(float32), None, 0, 255, NORM_MINMAX).astype(uint8) (OpenCV core/src/norm.cpp):
// scale = 255 * (smax - smin > DBL_EPSILON ? 1 / (smax - smin) : 0) in double, rounded to float32 (CV_32F result);
// shift = 0.0f - (float)(smin * scale); convertTo = fmaf(v, scale, shift); numpy's cast truncates.
__device__ __forceinline__ int index_blend_mask(int v, int smin, int smax) {
  const double r = (double)(smax - smin);
  const float a = (float)(255.0 * (r > 2.220446049250313e-16 ? 1.0 / r : 0.0));
  const float b = 0.0f - (float)((double)smin * (double)a);
  const float y = fmaf((float)v, a, b);
  return min(max((int)y, 0), 255);     // (y > -1 for v >= smin: truncation gives 0 there)
}

// save_warped_image, uint8 map: max > min + 1e-9 (float64); (m - min) / (max - min) divides the uint8 differences in
// float64, * 255 in float64, astype(uint8) truncates.  Otherwise zeros_like: index 0.
__device__ __forceinline__ int index_save_warped_u8(int v, int mn, int mx) {
  if (!((double)mx > (double)mn + 1e-9) || v < mn) return 0;
  const double q = (double)(v - mn) / (double)(mx - mn);
  return min((int)(q * 255.0), 255);
}

// save_warped_image, float32 / float64 map: the same in the map's dtype (float32 stays float32 under NEP 50; the
// EPSILON test then runs in float32 too).  A NaN product (an infinite range) is cast to 0, as numpy's cast does on x86.
template <typename T> struct FloatIndex;
template <> struct FloatIndex<float> {
  float mn, r;
  bool valid;
  __device__ FloatIndex(double dmn, double dmx) : mn((float)dmn) {
    const float mx = (float)dmx;
    valid = mx > __fadd_rn(mn, 1e-9f);
    r = __fsub_rn(mx, mn);
  }
  __device__ __forceinline__ int operator()(float v) const {
    const float s = __fmul_rn(__fdiv_rn(__fsub_rn(v, mn), r), 255.0f);
    return (valid && s == s) ? min((int)s, 255) : 0;
  }
};
template <> struct FloatIndex<double> {
  double mn, r;
  bool valid;
  __device__ FloatIndex(double dmn, double dmx) : mn(dmn) {
    valid = dmx > __dadd_rn(dmn, 1e-9);
    r = __dsub_rn(dmx, dmn);
  }
  __device__ __forceinline__ int operator()(double v) const {
    const double s = __dmul_rn(__ddiv_rn(__dsub_rn(v, mn), r), 255.0);
    return (valid && s == s) ? min((int)s, 255) : 0;
  }
};

// ---- pass 2: colour and blend ---------------------------------------------------------------------------------------
// addWeighted on 8-bit data, the AVX2 vector path: cvRound(fmaf(s1, w1, fmaf(s2, w2, 0))), saturated to [0, 255].
// BLEND_MASK: s1 = image, s2 = heat; SAVE_WARPED: s1 = heat, s2 = image.
__device__ __forceinline__ uint32_t blend_byte(uint32_t img, uint32_t heat, bool heat_first, float w_img, float w_heat) {
  const float i = (float)img, h = (float)heat;
  const float s1 = heat_first ? h : i, w1 = heat_first ? w_heat : w_img;
  const float s2 = heat_first ? i : h, w2 = heat_first ? w_img : w_heat;
  const float y = rintf(fmaf(s1, w1, fmaf(s2, w2, 0.0f)));
  return (uint32_t)fminf(fmaxf(y, 0.0f), 255.0f);           // (a NaN weight: cvRound -> INT_MIN -> 0)
}

// One pixel: image bytes (in the image's order) and the packed heat colour (output order) -> packed output pixel.
template <bool SWAP>
__device__ __forceinline__ uint32_t blend_px(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t heat, bool heat_first,
                                             float w_img, float w_heat) {
  if (SWAP) { const uint32_t t = c0; c0 = c2; c2 = t; }
  return blend_byte(c0, heat & 255u, heat_first, w_img, w_heat) | blend_byte(c1, (heat >> 8) & 255u, heat_first, w_img, w_heat) << 8 |
         blend_byte(c2, heat >> 16, heat_first, w_img, w_heat) << 16;
}

template <typename T, bool SWAP>
__global__ __launch_bounds__(OV_NT) void overlay_color_kernel(const OvImage* __restrict__ imgs, const double2* __restrict__ part,
                                                              const OvParams prm) {
  __shared__ uint32_t s_col[256];      // uint8 maps: colour of each map VALUE; float maps: colour of each Jet index
  __shared__ double s_mn[OV_NT / WAVE], s_mx[OV_NT / WAVE];
  __shared__ int s_nan[OV_NT / WAVE];
  const OvImage d = imgs[blockIdx.y];
  int64_t lo, hi;
  ov_chunk((int64_t)d.H * d.W, blockIdx.x, prm.k, lo, hi);
  if (lo >= hi) return;                // (block-uniform: before any barrier)
  // the image's min / max from the partials of pass 1 (empty chunks hold (+inf, -inf))
  MinMaxAcc a;
  if ((int)threadIdx.x < prm.k) {
    const double2 p = part[(size_t)blockIdx.y * prm.k + threadIdx.x];
    a.nan = p.x != p.x;
    a.mn = p.x; a.mx = p.y;
  }
  block_minmax(a, s_mn, s_mx, s_nan);
  // the colour table, in the output's channel order
  {
    const int t = threadIdx.x;
    int idx = t;
    if constexpr (sizeof(T) == 1) {
      const int mn = (int)a.mn, mx = (int)a.mx;               // (finite: a uint8 map has no NaN)
      idx = prm.style == ATTWARP_OVERLAY_BLEND_MASK ? index_blend_mask(t, mn, mx) : index_save_warped_u8(t, mn, mx);
    }
    const uint32_t b = kJetBGR[3 * idx], g = kJetBGR[3 * idx + 1], r = kJetBGR[3 * idx + 2];
    s_col[t] = prm.out_bgr ? (b | g << 8 | r << 16) : (r | g << 8 | b << 16);
  }
  __syncthreads();
  const bool heat_first = prm.style == ATTWARP_OVERLAY_SAVE_WARPED;
  const float w_img = prm.w_img, w_heat = prm.w_heat;
  const OV_G uint8_t* __restrict__ img = (const OV_G uint8_t*)d.image;
  const OV_G T* __restrict__ m = (const OV_G T*)d.map;
  OV_G uint8_t* __restrict__ out = (OV_G uint8_t*)d.out;
  // float maps: a NaN anywhere fails the EPSILON test (index 0 everywhere), as in numpy
  const FloatIndex<typename std::conditional<sizeof(T) == 8, double, float>::type> fidx(a.nan ? __builtin_nan("") : a.mn, a.mx);
  auto heat_of = [&](T v) -> uint32_t {
    if constexpr (sizeof(T) == 1) return s_col[v];
    else return s_col[fidx(v)];
  };
  for (int64_t p = lo + 4 * (int64_t)threadIdx.x; p < hi; p += OV_UNIT) {
    if (p + 4 <= hi) {
      uint32_t h0, h1, h2, h3;
      if constexpr (sizeof(T) == 1) {
        const uint32_t w = *(const OV_G u32_una*)(m + p);
        h0 = s_col[w & 255u]; h1 = s_col[(w >> 8) & 255u]; h2 = s_col[(w >> 16) & 255u]; h3 = s_col[w >> 24];
      } else if constexpr (sizeof(T) == 4) {
        const f32x4_a4 v = *(const OV_G f32x4_a4*)(m + p);
        h0 = heat_of(v.x); h1 = heat_of(v.y); h2 = heat_of(v.z); h3 = heat_of(v.w);
      } else {
        const f64x2_a8 v0 = *(const OV_G f64x2_a8*)(m + p), v1 = *(const OV_G f64x2_a8*)(m + p + 2);
        h0 = heat_of(v0.x); h1 = heat_of(v0.y); h2 = heat_of(v1.x); h3 = heat_of(v1.y);
      }
      const u32x3 s = *(const OV_G u32x3_una*)(img + 3 * p);      // 4 pixels: bytes 0-11
      const uint32_t o0 = blend_px<SWAP>(s.x & 255u, (s.x >> 8) & 255u, (s.x >> 16) & 255u, h0, heat_first, w_img, w_heat);
      const uint32_t o1 = blend_px<SWAP>(s.x >> 24, s.y & 255u, (s.y >> 8) & 255u, h1, heat_first, w_img, w_heat);
      const uint32_t o2 = blend_px<SWAP>((s.y >> 16) & 255u, s.y >> 24, s.z & 255u, h2, heat_first, w_img, w_heat);
      const uint32_t o3 = blend_px<SWAP>((s.z >> 8) & 255u, (s.z >> 16) & 255u, s.z >> 24, h3, heat_first, w_img, w_heat);
      u32x3 o;
      o.x = o0 | o1 << 24;
      o.y = o1 >> 8 | o2 << 16;
      o.z = o2 >> 16 | o3 << 8;
      *(OV_G u32x3_una*)(out + 3 * p) = o;
    } else {                           // the last pixels of an image whose size is not a multiple of 4
      for (int64_t q = p; q < hi; ++q) {
        const OV_G uint8_t* s = img + 3 * q;
        const uint32_t o = blend_px<SWAP>(s[0], s[1], s[2], heat_of(m[q]), heat_first, w_img, w_heat);
        out[3 * q] = (uint8_t)o; out[3 * q + 1] = (uint8_t)(o >> 8); out[3 * q + 2] = (uint8_t)(o >> 16);
      }
    }
  }
}

template <typename T>
static int launch_overlay(const OvImage* dimgs, int B, const OvParams& prm, bool swap, double2* part, hipStream_t st) {
  const dim3 grid(prm.k, B);
  hipLaunchKernelGGL(overlay_minmax_kernel<T>, grid, dim3(OV_NT), 0, st, dimgs, prm.k, part);
  if (const int rc = check_launch("overlay_minmax_kernel")) return rc;
  if (swap) hipLaunchKernelGGL((overlay_color_kernel<T, true>), grid, dim3(OV_NT), 0, st, dimgs, part, prm);
  else hipLaunchKernelGGL((overlay_color_kernel<T, false>), grid, dim3(OV_NT), 0, st, dimgs, part, prm);
  return check_launch("overlay_color_kernel");
}

}  // namespace attwarp

using namespace attwarp;

extern "C" size_t attwarp_overlay_workspace_bytes(int B) {
  if (B <= 0 || B > 65535) return 0;
  return (size_t)B * OV_MAX_CHUNKS * sizeof(double2);
}

extern "C" int attwarp_heatmap_overlay(const attwarp_overlay_image* images, const attwarp_overlay_image* images_dev, int B,
                                       int map_dtype, int style, double alpha, int in_order, int out_order, void* ws,
                                       void* stream) {
  ATTWARP_REQUIRE(images && images_dev && ws, "heatmap_overlay: null pointer");
  ATTWARP_REQUIRE(B > 0, "heatmap_overlay: non-positive batch size");
  ATTWARP_REQUIRE(map_dtype == ATTWARP_U8 || map_dtype == ATTWARP_F32 || map_dtype == ATTWARP_F64,
                  "heatmap_overlay: map_dtype must be U8, F32 or F64 (got %d)", map_dtype);
  ATTWARP_REQUIRE(style == ATTWARP_OVERLAY_BLEND_MASK || style == ATTWARP_OVERLAY_SAVE_WARPED,
                  "heatmap_overlay: unknown style %d", style);
  ATTWARP_REQUIRE(style != ATTWARP_OVERLAY_BLEND_MASK || map_dtype == ATTWARP_U8,
                  "heatmap_overlay: the blend_mask style takes uint8 masks");
  ATTWARP_REQUIRE((in_order == ATTWARP_RGB || in_order == ATTWARP_BGR) && (out_order == ATTWARP_RGB || out_order == ATTWARP_BGR),
                  "heatmap_overlay: channel orders must be ATTWARP_RGB or ATTWARP_BGR");
  ATTWARP_REQUIRE(__builtin_isfinite(alpha), "heatmap_overlay: alpha must be finite");
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0 && reinterpret_cast<uintptr_t>(images_dev) % 8 == 0,
                  "heatmap_overlay: ws must be 16-byte and images_dev 8-byte aligned");
  if (B > 65535) return fail(ATTWARP_E_UNSUPPORTED, "heatmap_overlay: B=%d > 65535", B);
  const size_t esz = map_dtype == ATTWARP_U8 ? 1 : map_dtype == ATTWARP_F32 ? 4 : 8;
  double px = 0.0;
  for (int b = 0; b < B; ++b) {
    const attwarp_overlay_image& d = images[b];
    ATTWARP_REQUIRE(d.image && d.map && d.out, "heatmap_overlay: image %d: null pointer", b);
    ATTWARP_REQUIRE(d.H > 0 && d.W > 0, "heatmap_overlay: image %d: non-positive size %d x %d", b, d.H, d.W);
    ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(d.map) % esz == 0, "heatmap_overlay: image %d: map not %zu-byte aligned", b, esz);
    if ((int64_t)d.H * d.W > (int64_t)1 << 30)
      return fail(ATTWARP_E_UNSUPPORTED, "heatmap_overlay: image %d: %d x %d pixels (> 2^30)", b, d.H, d.W);
    px += (double)d.H * d.W;
  }
  OvParams prm;
  prm.k = (int)std::min<double>(OV_MAX_CHUNKS, std::max(1.0, std::ceil(px / B / OV_CHUNK_PX)));
  prm.style = style;
  prm.out_bgr = out_order == ATTWARP_BGR;
  // addWeighted(src1, alpha, src2, beta, 0) takes double weights and runs in float32 (the caller's 1 - alpha in double)
  prm.w_heat = (float)alpha;
  prm.w_img = (float)(1.0 - alpha);
  const bool swap = in_order != out_order;
  const OvImage* dimgs = reinterpret_cast<const OvImage*>(images_dev);
  double2* part = static_cast<double2*>(ws);
  hipStream_t st = as_stream(stream);
  if (map_dtype == ATTWARP_U8) return launch_overlay<uint8_t>(dimgs, B, prm, swap, part, st);
  if (map_dtype == ATTWARP_F32) return launch_overlay<float>(dimgs, B, prm, swap, part, st);
  return launch_overlay<double>(dimgs, B, prm, swap, part, st);
}
