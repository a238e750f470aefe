// The trainer's debug and validation panels (MN/trainer.py:301-307, :484-517) in ONE launch: the first n images of every
// row source -- float32 images and warps, uint8 images, the low-resolution attention map as a normalised, bilinearly
// up-sampled heat row -- converted to bytes as (x * 255).byte() does and laid out as torchvision.utils.make_grid lays them
// out, straight into one uint8 canvas (HWC, what Pillow and the PNG encoder read, or CHW, what make_grid returns).
// Work split: the canvas is cut into one rectangle per grid slot (the cell with the padding above and left of it; the last
// column also owns the right padding and the margin, the last row the bottom padding), a rectangle into chunks of whole
// lines of about PN_BLOCK_BYTES; one workgroup per chunk.  A workgroup of a heat cell first loads the h x w map into LDS,
// reduces its maximum (NaN propagating, like amax) and normalises the tile in place: neither the normalised nor the
// up-sampled map ever reaches memory.  Lines are written as aligned dwords; the bytes before the first and after the last
// whole dword of a line (rows of 3 * Wg bytes start at any residue mod 4) are byte stores.
// Arithmetic (restated by tests/panel_ref.py): every float32 operation individually rounded.
#include "common.hpp"

namespace attwarp {

constexpr int PN_NT = 256;                 // threads per block
constexpr int PN_BLOCK_BYTES = 4096;       // canvas bytes one workgroup writes, about (four dwords per thread: the launch is
                                           // bound by the latency of its loads, so it wants many short workgroups)
#define PN_G __attribute__((address_space(1)))

struct PnSource {                          // == attwarp_panel_source
  const void* data;
  int64_t batch_stride;
  int32_t kind, C, N, h, w, clamp;
};
static_assert(sizeof(PnSource) == sizeof(attwarp_panel_source), "descriptor layout");

struct PnParams {
  PnSource src[ATTWARP_PANEL_MAX_SRC];
  uint8_t* out;
  int n, K, H, W, xmaps, ymaps, pad, margin, Hg, Wt;   // Wt = Wg + margin: pixels of a canvas row
  int lpc, nchunk;                         // lines per chunk, chunks per slot
  uint32_t pad_value;
};

// (unsigned char)(v * 255.0f) where torch defines it (-1 < t < 256); saturated outside, NaN -> 0.
__device__ __forceinline__ uint32_t pn_byte(float v) {
  const float t = fmul(v, 255.0f);
  return t >= 256.0f ? 255u : (t > -1.0f ? (uint32_t)(int)t : 0u);
}

// torch's area_pixel_compute_source_index (align_corners=False, not cubic) and the two taps of one axis.
struct PnTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ PnTap pn_tap(int dst, float scale, int in) {
  const float s = fmaxf(fsub(fmul(scale, fadd((float)dst, 0.5f)), 0.5f), 0.0f);
  PnTap t;
  t.i0 = min((int)s, in - 1);              // (src < in - 0.5 in exact arithmetic: the bound only guards the LDS tile)
  t.i1 = t.i0 + (t.i0 < in - 1);
  t.l1 = fsub(s, (float)t.i0);
  t.l0 = fsub(1.0f, t.l1);
  return t;
}

template <bool CHW>
__global__ __launch_bounds__(PN_NT) void panel_grid_kernel(const PnParams p) {
  __shared__ float s_heat[ATTWARP_PANEL_MAX_HEAT];
  __shared__ float s_mx[PN_NT / WAVE];
  __shared__ int s_nan[PN_NT / WAVE];
  const int tid = threadIdx.x;
  const int slot = blockIdx.x / p.nchunk, chunk = blockIdx.x - slot * p.nchunk;
  const int cy = slot / p.xmaps, cx = slot - cy * p.xmaps;
  const int cellh = p.H + p.pad, cellw = p.W + p.pad;
  const int y0 = cy * cellh, x0 = cx * cellw;
  const int rh = cellh + (cy == p.ymaps - 1 ? p.pad : 0);                 // the rectangle this slot owns
  const int rw = cellw + (cx == p.xmaps - 1 ? p.pad + p.margin : 0);
  const int nlines = CHW ? 3 * rh : rh, lb = CHW ? rw : 3 * rw;           // lines of lb bytes
  const int l_lo = chunk * p.lpc, l_hi = min(nlines, l_lo + p.lpc);
  if (l_lo >= l_hi) return;                                               // (block-uniform: before any barrier)
  const bool live = slot < p.K;                                           // cells missing from the last row stay pad_value
  const int r = live ? slot / p.n : 0, img = live ? slot - r * p.n : 0;
  const PnSource s = p.src[r];
  const int kind = live ? s.kind : -1;
  const size_t plane = (size_t)p.H * p.W;
  const PN_G float* __restrict__ f32 = (const PN_G float*)s.data + (int64_t)img * s.batch_stride;
  const PN_G uint8_t* __restrict__ u8 = (const PN_G uint8_t*)s.data + (int64_t)img * s.batch_stride;
  const bool clampv = s.clamp != 0, one = s.C == 1;
  float scale_y = 0.0f, scale_x = 0.0f;

  if (kind == ATTWARP_PANEL_HEAT) {
    const int hw = s.h * s.w;
    float mx = -__builtin_inff();
    bool nan = false;
    for (int t = tid; t < hw; t += PN_NT) {
      const float v = f32[t];
      s_heat[t] = v;
      nan |= v != v;
      mx = fmaxf(mx, v);                   // fmaxf skips a NaN; the flag keeps it
    }
    mx = wave_max(mx);
    const bool wnan = __any(nan);
    if ((tid & (WAVE - 1)) == 0) { s_mx[tid / WAVE] = mx; s_nan[tid / WAVE] = wnan; }
    __syncthreads();
    mx = s_mx[0];
    nan = s_nan[0] != 0;
    for (int i = 1; i < PN_NT / WAVE; ++i) { mx = fmaxf(mx, s_mx[i]); nan |= s_nan[i] != 0; }
    const float d = fadd(nan ? __builtin_nanf("") : mx, 1e-6f);
    for (int t = tid; t < hw; t += PN_NT) s_heat[t] = __fdiv_rn(s_heat[t], d);   // (each thread its own cells)
    __syncthreads();
    scale_y = __fdiv_rn((float)s.h, (float)p.H);
    scale_x = __fdiv_rn((float)s.w, (float)p.W);
  }

  PN_G uint8_t* __restrict__ out = (PN_G uint8_t*)p.out;
  const int dpl = (lb + 6) / 4;            // dwords a line spans at most: ceil((lb + 3) / 4), 3 = the largest misalignment
  const int items = (l_hi - l_lo) * dpl;
  for (int it = tid; it < items; it += PN_NT) {
    const int ll = it / dpl, j = it - ll * dpl;
    const int l = l_lo + ll;
    const int c_line = CHW ? l / rh : 0;
    const int ry = CHW ? l - c_line * rh : l;
    const int iy = ry - p.pad;
    const bool row_live = live && iy >= 0 && iy < p.H;
    const size_t line = CHW ? ((size_t)c_line * p.Hg + (y0 + ry)) * p.Wt + x0 : ((size_t)(y0 + ry) * p.Wt + x0) * 3;
    const int a = (int)((reinterpret_cast<uintptr_t>(p.out) + line) & 3);
    const int b0 = 4 * j - a;              // bytes b0 .. b0 + 3 of the line: an aligned dword of the canvas
    PnTap ty = {0, 0, 0.0f, 0.0f};
    if (kind == ATTWARP_PANEL_HEAT && row_live) ty = pn_tap(iy, scale_y, s.h);
    int last_ix = -1;
    uint32_t last = 0, word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = b0 + q;
      if (b < 0 || b >= lb) continue;
      const int rx = CHW ? b : b / 3;
      const int c = CHW ? c_line : b - 3 * rx;
      const int ix = rx - p.pad;
      uint32_t v = p.pad_value;
      if (row_live && ix >= 0 && ix < p.W) {
        if (kind == ATTWARP_PANEL_HEAT) {
          if (ix != last_ix) {
            const PnTap tx = pn_tap(ix, scale_x, s.w);
            const float q00 = s_heat[ty.i0 * s.w + tx.i0], q01 = s_heat[ty.i0 * s.w + tx.i1];
            const float q10 = s_heat[ty.i1 * s.w + tx.i0], q11 = s_heat[ty.i1 * s.w + tx.i1];
            const float top = fadd(fmul(tx.l0, q00), fmul(tx.l1, q01)), bot = fadd(fmul(tx.l0, q10), fmul(tx.l1, q11));
            last = pn_byte(fadd(fmul(ty.l0, top), fmul(ty.l1, bot)));
            last_ix = ix;
          }
          v = last;
        } else {
          const size_t e = (one ? 0 : (size_t)c * plane) + (size_t)iy * p.W + ix;
          if (kind == ATTWARP_PANEL_U8) {
            v = u8[e];
          } else {
            float x = f32[e];
            if (clampv) x = fminf(fmaxf(x, 0.0f), 1.0f);      // (a NaN becomes 0 here, as pn_byte makes it)
            v = pn_byte(x);
          }
        }
      }
      word |= v << (8 * q);
    }
    if (b0 >= 0 && b0 + 4 <= lb) {
      *(PN_G uint32_t*)(out + line + b0) = word;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (b0 + q >= 0 && b0 + q < lb) out[line + b0 + q] = (uint8_t)(word >> (8 * q));
    }
  }
}

}  // namespace attwarp

using namespace attwarp;

extern "C" int attwarp_panel_grid(const attwarp_panel_source* sources, int nsrc, int n, int H, int W, int nrow, int padding,
                                  int pad_value, int layout, int right_margin, int flags, uint8_t* out, void* stream) {
  ATTWARP_REQUIRE(sources && out, "panel_grid: null pointer");
  ATTWARP_REQUIRE(nsrc >= 1, "panel_grid: no source");
  if (nsrc > ATTWARP_PANEL_MAX_SRC)
    return fail(ATTWARP_E_UNSUPPORTED, "panel_grid: %d sources (> ATTWARP_PANEL_MAX_SRC = %d)", nsrc, ATTWARP_PANEL_MAX_SRC);
  ATTWARP_REQUIRE(n >= 1 && H >= 1 && W >= 1, "panel_grid: zero size (n=%d, H=%d, W=%d)", n, H, W);
  ATTWARP_REQUIRE(nrow >= 1, "panel_grid: nrow=%d", nrow);
  ATTWARP_REQUIRE(padding >= 0 && right_margin >= 0, "panel_grid: negative padding %d or right_margin %d", padding, right_margin);
  ATTWARP_REQUIRE(pad_value >= 0 && pad_value <= 255, "panel_grid: pad_value %d is not a byte", pad_value);
  ATTWARP_REQUIRE(layout == ATTWARP_HWC || layout == ATTWARP_CHW, "panel_grid: unknown layout %d", layout);
  ATTWARP_REQUIRE((flags & ~ATTWARP_PANEL_FOR_PNG) == 0, "panel_grid: unknown flags %d", flags);
  if (H > (1 << 24) || W > (1 << 24) || padding > (1 << 24) || right_margin > (1 << 24))
    return fail(ATTWARP_E_UNSUPPORTED, "panel_grid: H, W, padding and right_margin are at most 2^24");
  PnParams p = {};
  for (int r = 0; r < nsrc; ++r) {
    const attwarp_panel_source& s = sources[r];
    ATTWARP_REQUIRE(s.data, "panel_grid: source %d: null pointer", r);
    ATTWARP_REQUIRE(s.kind == ATTWARP_PANEL_F32 || s.kind == ATTWARP_PANEL_U8 || s.kind == ATTWARP_PANEL_HEAT,
                    "panel_grid: source %d: unknown kind %d", r, s.kind);
    ATTWARP_REQUIRE(s.N >= n, "panel_grid: source %d holds N=%d images, fewer than n=%d", r, s.N, n);
    int64_t need;
    if (s.kind == ATTWARP_PANEL_HEAT) {
      ATTWARP_REQUIRE(s.C == 1, "panel_grid: source %d: a heat source has one channel (C=%d)", r, s.C);
      ATTWARP_REQUIRE(s.h >= 1 && s.w >= 1, "panel_grid: source %d: zero size heat map %d x %d", r, s.h, s.w);
      if ((int64_t)s.h * s.w > ATTWARP_PANEL_MAX_HEAT)
        return fail(ATTWARP_E_UNSUPPORTED, "panel_grid: source %d: heat map %d x %d has more than ATTWARP_PANEL_MAX_HEAT = %d cells",
                    r, s.h, s.w, ATTWARP_PANEL_MAX_HEAT);
      need = (int64_t)s.h * s.w;
    } else {
      ATTWARP_REQUIRE(s.C == 1 || s.C == 3, "panel_grid: source %d: C=%d (3 or 1)", r, s.C);
      need = (int64_t)s.C * H * W;
    }
    ATTWARP_REQUIRE(n == 1 || s.batch_stride >= need, "panel_grid: source %d: batch stride %lld below the %lld elements of an image",
                    r, (long long)s.batch_stride, (long long)need);
    ATTWARP_REQUIRE(s.kind == ATTWARP_PANEL_U8 || reinterpret_cast<uintptr_t>(s.data) % 4 == 0,
                    "panel_grid: source %d: float32 data not 4-byte aligned", r);
    p.src[r] = PnSource{s.data, s.batch_stride, s.kind, s.C, s.N, s.h, s.w, s.clamp};
  }
  const int64_t K = (int64_t)nsrc * n;
  if (K > (1 << 20)) return fail(ATTWARP_E_UNSUPPORTED, "panel_grid: %lld cells (> 2^20)", (long long)K);
  const int pad = K == 1 ? 0 : padding;    // make_grid returns a single image as it is
  const int xmaps = (int)std::min<int64_t>(nrow, K), ymaps = (int)((K + xmaps - 1) / xmaps);
  const int64_t Hg = (int64_t)ymaps * (H + pad) + pad, Wt = (int64_t)xmaps * (W + pad) + pad + right_margin;
  if (Hg >= (1 << 30) || 3 * Wt >= (1 << 30))
    return fail(ATTWARP_E_UNSUPPORTED, "panel_grid: canvas of %lld x %lld pixels (a side of 2^30 bytes or more)", (long long)Hg, (long long)Wt);
  if ((flags & ATTWARP_PANEL_FOR_PNG) && 1 + 3 * Wt > ATTWARP_PNG_MAX_ROW_BYTES)
    return fail(ATTWARP_E_UNSUPPORTED, "panel_grid: a row of 1 + 3 x %lld bytes exceeds ATTWARP_PNG_MAX_ROW_BYTES = %d", (long long)Wt,
                ATTWARP_PNG_MAX_ROW_BYTES);
  const bool chw = layout == ATTWARP_CHW;
  // the largest rectangle: a cell of the last column and the last row
  const int64_t rw = W + 2 * (int64_t)pad + right_margin, rh = H + 2 * (int64_t)pad;
  const int64_t lb = chw ? rw : 3 * rw, nlines = chw ? 3 * rh : rh;
  const int64_t lpc = std::max<int64_t>(1, PN_BLOCK_BYTES / lb), nchunk = (nlines + lpc - 1) / lpc;
  const int64_t blocks = nchunk * xmaps * ymaps;
  if (blocks >= (int64_t)1 << 31 || lpc * ((lb + 6) / 4) >= (int64_t)1 << 31)
    return fail(ATTWARP_E_UNSUPPORTED, "panel_grid: %lld workgroups (>= 2^31)", (long long)blocks);
  p.out = out;
  p.n = n; p.K = (int)K; p.H = H; p.W = W; p.xmaps = xmaps; p.ymaps = ymaps; p.pad = pad; p.margin = right_margin;
  p.Hg = (int)Hg; p.Wt = (int)Wt; p.lpc = (int)lpc; p.nchunk = (int)nchunk; p.pad_value = (uint32_t)pad_value;
  hipStream_t st = as_stream(stream);
  if (chw) hipLaunchKernelGGL(panel_grid_kernel<true>, dim3((unsigned)blocks), dim3(PN_NT), 0, st, p);
  else hipLaunchKernelGGL(panel_grid_kernel<false>, dim3((unsigned)blocks), dim3(PN_NT), 0, st, p);
  return check_launch("panel_grid_kernel");
}
