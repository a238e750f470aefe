// The Stable-Diffusion warp ablation (Ablations/Stable_diffusion_based_warp.py): what nothing else in csrc/ computes.
//
//  * xattn_reduce: compute_token_importance (:310-360) and aggregate_attention_map_for_tokens (:365-402) read every captured
//    cross-attention tensor [B,heads,H,W,tokens] with stock ops; here every tensor crosses HBM ONCE.  A workgroup owns
//    chunk = attwarp_xattn_chunk(tokens) consecutive positions of HW (E = chunk * tokens <= 2048 consecutive elements of
//    every (b, head) slice) and streams them as aligned 16-byte loads (token = flat index mod tokens; the groups cut by the
//    chunk's unaligned head and tail are read element by element).  Summation order (restated in tests/sdwarp_ref.py):
//      per element e of the chunk, float64:  s_b(h) = ((0 + v[0,h]) + v[1,h]) + ...      over b ascending
//                                            tot(e) = ((0 + s_b(0)) + s_b(1)) + ...      over heads ascending
//                                            hw_tok(e) = round(((0 + round(s_b(0))) + round(s_b(1))) + ...)   (the reference's
//                                                        two roundings: sum(dim=0), then sum(dim=0) again)
//      per token t of the chunk, float64:    part(t) = (tot(t) + tot(tokens + t)) + ...  over the chunk's positions ascending
//      second launch:                        token_sums(t) = round((part_0(t) + part_1(t)) + ...)   over chunks ascending
//  * resize_cubic: OpenCV 4.x resizeGeneric_ with the scalar HResizeCubic / VResizeCubic, one float32 channel, any source
//    size: a thread owns an output column of a (256-column, 64-row) tile, keeps the horizontal results of the four source
//    rows of its current window in registers and moves the window as ofs_y advances (ofs_y is non-decreasing).
//  * blur5_minmax / minmax_normalize: cv2.GaussianBlur(5 x 5, sigma 1, BORDER_REFLECT_101) and numpy's in-place
//    a -= a.min(); a /= (a.max() + 1e-9) in float32.
// OpenCV's arithmetic is restated from its published source; OpenCV is absent where this is built, so parity with it is
// unpinned (tests/test_sdwarp_vs_opencv.py reports the distance where cv2 imports).  Bit-exact with tests/sdwarp_ref.py.
#include "common.hpp"
#include "pil8.hpp"          // clampi
#include "resize_axis.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

namespace attwarp {
namespace sdwarp {

constexpr int NT = 256;
constexpr int MAX_RECORDS = 65535;
constexpr int MAX_SIDE = 1 << 15;

// ---- cross-attention reduce ------------------------------------------------------------------------------------------
constexpr int XA_ELEMS = 2048;     // elements of one (b, head) slice per workgroup: 16 KB of float64 in LDS
constexpr int MAX_TOKENS = 256;
typedef attwarp_xattn_map XMap;

inline int chunk_of(int tokens) { return std::max(1, XA_ELEMS / tokens); }
inline int chunks_of(int HW, int tokens) { const int c = chunk_of(tokens); return (HW + c - 1) / c; }

// Elements k of a group of V with e0 + k inside [0, E) from an element-aligned address, one load each (the first and the
// last group of a slice, and every group of a tensor whose slices do not share one 16-byte phase); the rest are 0.
template <typename T, int V>
__device__ __forceinline__ void load_edge(const T* s, int e0, int E, float* v) {
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = (e0 + k >= 0 && e0 + k < E) ? to_f32<T>(s[k]) : 0.0f;
}
// A whole group at a 16-byte aligned address: one global dwordx4 load
template <typename T, int V>
__device__ __forceinline__ void load_vec(const T* s, float* v) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef const u32x4 __attribute__((address_space(1)))* gvec;
  const u32x4 raw = *reinterpret_cast<gvec>(reinterpret_cast<uintptr_t>(s));
  T t[V];
  __builtin_memcpy(t, &raw, sizeof(raw));
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = to_f32<T>(t[k]);
}
template <typename T, int V>
__device__ __forceinline__ void load_group(const T* s, int e0, int E, bool full, float* v) {
  if (full) load_vec<T, V>(s, v);
  else load_edge<T, V>(s, e0, E, v);
}

// The chunk's elements are cut into groups of V = 16 / sizeof(T) at the 16-byte boundaries of memory when every (b, head)
// slice of the chunk starts at the same phase m of a 16-byte block (the slice stride HW * tokens is a multiple of V: every
// SD-2.1 layer); a thread then owns groups, reads the whole ones with one aligned 16-byte load per slice and the two cut
// ones element by element.  Otherwise (m = 0, no group is "whole") every element is loaded on its own.  The sums of an
// element do not depend on which thread forms them: both forms give the same bits.
template <typename T>
__global__ __launch_bounds__(NT) void xattn_kernel(const XMap* __restrict__ maps, int tokens, int chunk, int max_chunks,
                                                   double* __restrict__ parts) {
  __shared__ double tot_e[XA_ELEMS];
  constexpr int V = 16 / (int)sizeof(T);
  const XMap d = maps[blockIdx.y];
  const int nc = (d.HW + chunk - 1) / chunk;
  if ((int)blockIdx.x >= nc) return;
  const int p0 = blockIdx.x * chunk, np = min(chunk, d.HW - p0), E = np * tokens;
  const int64_t slice = (int64_t)d.HW * tokens;
  const T* base = static_cast<const T*>(d.attn) + (int64_t)p0 * tokens;
  T* hw = d.hw_tok ? static_cast<T*>(d.hw_tok) + (int64_t)p0 * tokens : nullptr;
  const bool phased = slice % V == 0;
  const int m = phased ? (int)((reinterpret_cast<uintptr_t>(base) / sizeof(T)) % V) : 0;
  const int ngroups = (m + E + V - 1) / V;
  const int pairs = (d.B + 1) / 2, steps = d.heads * pairs;       // a step = the slices (b0, h), (b0 + 1, h): two loads in flight
  for (int g = threadIdx.x; g < ngroups; g += NT) {
    const int e0 = g * V - m;
    const bool full = phased && e0 >= 0 && e0 + V <= E;
    double tot[V], acc_h[V], acc_b[V];
#pragma unroll
    for (int k = 0; k < V; ++k) tot[k] = acc_h[k] = acc_b[k] = 0.0;
    const T* s0 = base + e0;
    // the loads of step q + 1 are issued before the sums of step q (the sums of a head end in a rounding chain)
    float v0[V], v1[V], n0[V], n1[V];
    load_group<T, V>(s0, e0, E, full, v0);
    if (d.B > 1) load_group<T, V>(s0 + (int64_t)d.heads * slice, e0, E, full, v1);
    int h = 0, b0 = 0;
    for (int q = 0; q < steps; ++q) {
      const bool two = b0 + 1 < d.B;
      int hn = h, bn = b0 + 2;
      if (bn >= d.B) { bn = 0; ++hn; }
      if (q + 1 < steps) {
        load_group<T, V>(s0 + ((int64_t)bn * d.heads + hn) * slice, e0, E, full, n0);
        if (bn + 1 < d.B) load_group<T, V>(s0 + ((int64_t)(bn + 1) * d.heads + hn) * slice, e0, E, full, n1);
      }
#pragma unroll
      for (int k = 0; k < V; ++k) acc_b[k] += (double)v0[k];
      if (two) {
#pragma unroll
        for (int k = 0; k < V; ++k) acc_b[k] += (double)v1[k];
      }
      if (hn != h) {                                  // the head is complete
#pragma unroll
        for (int k = 0; k < V; ++k) tot[k] += acc_b[k];
        if (hw) {                                     // (the roundings of hw_tok only where it is asked for)
#pragma unroll
          for (int k = 0; k < V; ++k) acc_h[k] += (double)to_f32<T>(from_f64<T>(acc_b[k]));
        }
#pragma unroll
        for (int k = 0; k < V; ++k) acc_b[k] = 0.0;
      }
#pragma unroll
      for (int k = 0; k < V; ++k) { v0[k] = n0[k]; v1[k] = n1[k]; }
      h = hn;
      b0 = bn;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (e0 + k >= 0 && e0 + k < E) {
        tot_e[e0 + k] = tot[k];
        if (hw) hw[e0 + k] = from_f64<T>(acc_h[k]);
      }
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < tokens) {
    double a = tot_e[t];
    for (int p = 1; p < np; ++p) a += tot_e[p * tokens + t];
    parts[((int64_t)blockIdx.y * max_chunks + blockIdx.x) * tokens + t] = a;
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void xattn_final_kernel(const XMap* __restrict__ maps, int tokens, int chunk, int max_chunks,
                                                         const double* __restrict__ parts) {
  const int t = threadIdx.x;
  if (t >= tokens) return;
  const XMap d = maps[blockIdx.x];
  const int nc = (d.HW + chunk - 1) / chunk;
  const double* p = parts + (int64_t)blockIdx.x * max_chunks * tokens + t;
  double a = p[0];
  for (int c = 1; c < nc; ++c) a += p[(int64_t)c * tokens];
  static_cast<T*>(d.token_sums)[t] = from_f64<T>(a);
}

template <typename T>
static int launch_xattn(const XMap* maps_dev, int M, int tokens, int mc, double* parts, hipStream_t st) {
  const int chunk = chunk_of(tokens);
  hipLaunchKernelGGL(xattn_kernel<T>, dim3((unsigned)mc, (unsigned)M), dim3(NT), 0, st, maps_dev, tokens, chunk, mc, parts);
  if (const int rc = check_launch("xattn_kernel")) return rc;
  hipLaunchKernelGGL(xattn_final_kernel<T>, dim3((unsigned)M), dim3(NT), 0, st, maps_dev, tokens, chunk, mc, parts);
  return check_launch("xattn_final_kernel");
}

// ---- INTER_CUBIC -----------------------------------------------------------------------------------------------------
constexpr int TILE = NT;          // output columns per workgroup
constexpr int BAND = 64;          // output rows per workgroup
typedef attwarp_cubic_map CMap;

inline int ctiles_of(int W) { return (W + TILE - 1) / TILE; }
inline int cbands_of(int H) { return (H + BAND - 1) / BAND; }

// OpenCV's interpolateCubic (imgproc/src/resize.cpp), float32, one rounding per operation (host code is built with
// -ffp-contract=off as well)
static void interpolate_cubic(float x, float* coeffs) {
  const float A = -0.75f;
  coeffs[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
  coeffs[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
  coeffs[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
  coeffs[3] = 1.f - coeffs[0] - coeffs[1] - coeffs[2];
}

// horizontal pass of this thread's column at source row r
__device__ __forceinline__ float hcubic(const CMap& d, int r, const int* col, const float* c) {
  const float* S = d.src + (int64_t)clampi(r, 0, d.h - 1) * d.w;
  float v = fmul(S[col[0]], c[0]);
#pragma unroll
  for (int j = 1; j < 4; ++j) v = fadd(v, fmul(S[col[j]], c[j]));
  return v;
}

__global__ __launch_bounds__(NT) void cubic_kernel(const CMap* __restrict__ maps) {
  const CMap d = maps[blockIdx.y];
  const int tx = (d.W + TILE - 1) / TILE, nb = tx * ((d.H + BAND - 1) / BAND);
  if ((int)blockIdx.x >= nb) return;
  const int x = (blockIdx.x % tx) * TILE + threadIdx.x;
  if (x >= d.W) return;
  const int y0 = (blockIdx.x / tx) * BAND, y1 = min(d.H, y0 + BAND);
  if (d.H == d.h && d.W == d.w) {
    for (int y = y0; y < y1; ++y) d.out[(int64_t)y * d.W + x] = d.src[(int64_t)y * d.W + x];
    return;
  }
  const int ox = d.ofs_x[x];
  float c[4];
  int col[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = d.coef_x[(int64_t)x * 4 + j];
    col[j] = clampi(ox - 1 + j, 0, d.w - 1);
  }
  float win[4];                     // horizontal results of source rows clamp(cur - 1 .. cur + 2)
  int cur = 0;
  bool have = false;
  for (int y = y0; y < y1; ++y) {
    const int oy = d.ofs_y[y];
    if (!have || oy < cur || oy - cur > 3) {
#pragma unroll
      for (int k = 0; k < 4; ++k) win[k] = hcubic(d, oy - 1 + k, col, c);
      cur = oy;
      have = true;
    }
    while (cur < oy) {
      ++cur;
      win[0] = win[1]; win[1] = win[2]; win[2] = win[3];
      win[3] = hcubic(d, cur + 2, col, c);
    }
    const float* cy = d.coef_y + (int64_t)y * 4;
    float v = fmul(win[0], cy[0]);
#pragma unroll
    for (int k = 1; k < 4; ++k) v = fadd(v, fmul(win[k], cy[k]));
    d.out[(int64_t)y * d.W + x] = v;
  }
}

// ---- Gaussian 5 x 5, min / max, normalise ----------------------------------------------------------------------------
constexpr int BT = 64;            // a workgroup covers BT x BT pixels: 64 columns, four waves of 16 rows each
typedef attwarp_f32_map FMap;
struct MinMax { float mn, mx; };   // both NaN: a NaN was seen

inline int btiles_of(int n) { return (n + BT - 1) / BT; }
inline int64_t bblocks_of(int H, int W) { return (int64_t)btiles_of(H) * btiles_of(W); }

// cv::borderInterpolate(p, len, BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

struct Taps { float k0, k1, k2; };

__device__ __forceinline__ float sym5(const Taps& k, float a, float b, float c, float dd, float e) {
  return fadd(fadd(fmul(k.k0, c), fmul(k.k1, fadd(b, dd))), fmul(k.k2, fadd(a, e)));
}
__device__ __forceinline__ float blur_row(const float* S, int W, int x, const Taps& k) {
  return sym5(k, S[reflect101(x - 2, W)], S[reflect101(x - 1, W)], S[x], S[reflect101(x + 1, W)], S[reflect101(x + 2, W)]);
}

__device__ __forceinline__ void mm_take(float& mn, float& mx, bool& nan, float v) {
  nan = nan || v != v;
  mn = fminf(mn, v);
  mx = fmaxf(mx, v);
}

template <bool BLUR>
__global__ __launch_bounds__(NT) void blur_kernel(const FMap* __restrict__ maps, Taps k, int max_blocks, MinMax* __restrict__ parts) {
  __shared__ float s_mn[NT / WAVE], s_mx[NT / WAVE];
  __shared__ int s_nan[NT / WAVE];
  const FMap d = maps[blockIdx.y];
  const int tx = (d.W + BT - 1) / BT, nb = tx * ((d.H + BT - 1) / BT);
  if ((int)blockIdx.x >= nb) return;
  const int x = (blockIdx.x % tx) * BT + (threadIdx.x & (BT - 1));
  const int y0 = (blockIdx.x / tx) * BT + (threadIdx.x / BT) * (BT / (NT / BT));
  const int y1 = min(d.H, y0 + BT / (NT / BT));
  float mn = INFINITY, mx = -INFINITY;
  bool nan = false;
  if (x < d.W && y0 < y1) {
    if (BLUR) {
      float win[5];                 // row-pass values of source rows reflect(y - 2 .. y + 2)
#pragma unroll
      for (int j = 0; j < 4; ++j) win[j + 1] = blur_row(d.src + (int64_t)reflect101(y0 - 2 + j, d.H) * d.W, d.W, x, k);
      for (int y = y0; y < y1; ++y) {
#pragma unroll
        for (int j = 0; j < 4; ++j) win[j] = win[j + 1];
        win[4] = blur_row(d.src + (int64_t)reflect101(y + 2, d.H) * d.W, d.W, x, k);
        const float v = sym5(k, win[0], win[1], win[2], win[3], win[4]);
        d.out[(int64_t)y * d.W + x] = v;
        mm_take(mn, mx, nan, v);
      }
    } else {
      for (int y = y0; y < y1; ++y) mm_take(mn, mx, nan, d.src[(int64_t)y * d.W + x]);
    }
  }
  if (!parts) return;
  mn = wave_min(mn);
  mx = wave_max(mx);
  const bool wnan = __any(nan);
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  if (lane == 0) { s_mn[wid] = mn; s_mx[wid] = mx; s_nan[wid] = wnan ? 1 : 0; }
  __syncthreads();
  if (threadIdx.x == 0) {
    bool anan = false;
    for (int w = 0; w < NT / WAVE; ++w) { mn = fminf(mn, s_mn[w]); mx = fmaxf(mx, s_mx[w]); anan = anan || s_nan[w]; }
    MinMax p;
    p.mn = anan ? NAN : mn;
    p.mx = anan ? NAN : mx;
    parts[(int64_t)blockIdx.y * max_blocks + blockIdx.x] = p;
  }
}

// one workgroup per map: its partials -> final[m] (min and max are order independent; a NaN partial makes both NaN)
__global__ __launch_bounds__(NT) void minmax_final_kernel(const FMap* __restrict__ maps, int max_blocks,
                                                          const MinMax* __restrict__ parts, MinMax* __restrict__ fin) {
  __shared__ float s_mn[NT / WAVE], s_mx[NT / WAVE];
  __shared__ int s_nan[NT / WAVE];
  const FMap d = maps[blockIdx.x];
  const int nb = ((d.W + BT - 1) / BT) * ((d.H + BT - 1) / BT);
  const MinMax* p = parts + (int64_t)blockIdx.x * max_blocks;
  float mn = INFINITY, mx = -INFINITY;
  bool nan = false;
  for (int i = threadIdx.x; i < nb; i += NT) {
    mm_take(mn, mx, nan, p[i].mn);
    mx = fmaxf(mx, p[i].mx);
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  const bool wnan = __any(nan);
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  if (lane == 0) { s_mn[wid] = mn; s_mx[wid] = mx; s_nan[wid] = wnan ? 1 : 0; }
  __syncthreads();
  if (threadIdx.x == 0) {
    bool anan = false;
    for (int w = 0; w < NT / WAVE; ++w) { mn = fminf(mn, s_mn[w]); mx = fmaxf(mx, s_mx[w]); anan = anan || s_nan[w]; }
    MinMax r;
    r.mn = anan ? NAN : mn;
    r.mx = anan ? NAN : mx;
    fin[blockIdx.x] = r;
  }
}

constexpr int NORM_PER_BLOCK = NT * 4;
// a -= a.min(); a /= (a.max() + 1e-9) in float32: the maximum after the subtraction is fl(max - min) (rounding is monotonic)
// except that a minimum of -inf leaves a NaN in the array (-inf - -inf), which numpy's max then returns.
__global__ __launch_bounds__(NT) void normalize_kernel(const FMap* __restrict__ maps, const MinMax* __restrict__ fin) {
  const FMap d = maps[blockIdx.y];
  const int64_t n = (int64_t)d.H * d.W, i0 = (int64_t)blockIdx.x * NORM_PER_BLOCK;
  if (i0 >= n) return;
  const MinMax r = fin[blockIdx.y];
  const float mx1 = (r.mn == -INFINITY) ? NAN : fsub(r.mx, r.mn);
  const float den = fadd(mx1, 1e-9f);
  for (int j = 0; j < 4; ++j) {
    const int64_t i = i0 + j * NT + threadIdx.x;
    if (i < n) d.out[i] = fsub(d.src[i], r.mn) / den;
  }
}

static int validate_fmaps(const char* who, const FMap* maps, const FMap* maps_dev, int M, bool need_out, int64_t* max_blocks,
                          int64_t* max_elems) {
  ATTWARP_REQUIRE(maps && maps_dev, "%s: null pointer", who);
  ATTWARP_REQUIRE(M > 0, "%s: non-positive map count", who);
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(maps_dev) % 8 == 0, "%s: maps_dev must be 8-byte aligned", who);
  if (M > MAX_RECORDS) return fail(ATTWARP_E_UNSUPPORTED, "%s: M=%d > %d", who, M, MAX_RECORDS);
  int64_t mb = 0, me = 0;
  for (int m = 0; m < M; ++m) {
    const FMap& d = maps[m];
    ATTWARP_REQUIRE(d.src, "%s: map %d: null src", who, m);
    ATTWARP_REQUIRE(!need_out || d.out, "%s: map %d: null out", who, m);
    ATTWARP_REQUIRE(d.H > 0 && d.W > 0, "%s: map %d: non-positive size %d x %d", who, m, d.H, d.W);
    if (d.H > MAX_SIDE || d.W > MAX_SIDE) return fail(ATTWARP_E_UNSUPPORTED, "%s: map %d: %d x %d (> %d)", who, m, d.H, d.W, MAX_SIDE);
    ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(d.src) % 4 == 0 && reinterpret_cast<uintptr_t>(d.out) % 4 == 0,
                    "%s: map %d: src / out not 4-byte aligned", who, m);
    mb = std::max(mb, bblocks_of(d.H, d.W));
    me = std::max(me, (int64_t)d.H * d.W);
  }
  *max_blocks = mb;
  *max_elems = me;
  return ATTWARP_OK;
}

}  // namespace sdwarp
}  // namespace attwarp

using namespace attwarp;
using namespace attwarp::sdwarp;

extern "C" int attwarp_xattn_chunk(int tokens) {
  if (tokens < 1 || tokens > MAX_TOKENS) return fail(ATTWARP_E_ARG, "xattn_chunk: tokens=%d outside 1 .. %d", tokens, MAX_TOKENS);
  return chunk_of(tokens);
}

extern "C" size_t attwarp_xattn_reduce_workspace_bytes(const attwarp_xattn_map* maps, int M, int tokens) {
  if (!maps || M <= 0 || tokens < 1 || tokens > MAX_TOKENS) return 0;
  int mc = 0;
  for (int m = 0; m < M; ++m)
    if (maps[m].HW > 0) mc = std::max(mc, chunks_of(maps[m].HW, tokens));
  return (size_t)M * mc * tokens * sizeof(double);
}

extern "C" int attwarp_xattn_reduce(const attwarp_xattn_map* maps, const attwarp_xattn_map* maps_dev, int M, int dtype,
                                    int tokens, void* ws, void* stream) {
  ATTWARP_REQUIRE(maps && maps_dev && ws, "xattn_reduce: null pointer");
  ATTWARP_REQUIRE(M > 0, "xattn_reduce: non-positive record count");
  if (M > MAX_RECORDS) return fail(ATTWARP_E_UNSUPPORTED, "xattn_reduce: M=%d > %d", M, MAX_RECORDS);
  ATTWARP_REQUIRE(tokens >= 1 && tokens <= MAX_TOKENS, "xattn_reduce: tokens=%d outside 1 .. %d", tokens, MAX_TOKENS);
  ATTWARP_REQUIRE(dtype == ATTWARP_F32 || dtype == ATTWARP_F16 || dtype == ATTWARP_BF16, "xattn_reduce: dtype %d (F32, F16 or BF16)", dtype);
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(maps_dev) % 8 == 0, "xattn_reduce: maps_dev must be 8-byte aligned");
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "xattn_reduce: ws must be 16-byte aligned");
  const uintptr_t es = dtype == ATTWARP_F32 ? 4 : 2;
  int mc = 0;
  for (int m = 0; m < M; ++m) {
    const XMap& d = maps[m];
    ATTWARP_REQUIRE(d.attn && d.token_sums, "xattn_reduce: record %d: null attn / token_sums", m);
    ATTWARP_REQUIRE(d.B > 0 && d.heads > 0 && d.HW > 0, "xattn_reduce: record %d: non-positive shape [%d,%d,%d]", m, d.B, d.heads, d.HW);
    ATTWARP_REQUIRE((int64_t)d.HW * tokens < ((int64_t)1 << 31) && (int64_t)d.B * d.heads < ((int64_t)1 << 24),
                    "xattn_reduce: record %d: [%d,%d,%d,%d] too large", m, d.B, d.heads, d.HW, tokens);
    ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(d.attn) % es == 0 && reinterpret_cast<uintptr_t>(d.token_sums) % es == 0 &&
                        reinterpret_cast<uintptr_t>(d.hw_tok) % es == 0,
                    "xattn_reduce: record %d: pointer not element aligned", m);
    mc = std::max(mc, chunks_of(d.HW, tokens));
  }
  hipStream_t st = as_stream(stream);
  double* parts = static_cast<double*>(ws);
  if (dtype == ATTWARP_F32) return launch_xattn<float>(maps_dev, M, tokens, mc, parts, st);
  if (dtype == ATTWARP_F16) return launch_xattn<__half>(maps_dev, M, tokens, mc, parts, st);
  return launch_xattn<__hip_bfloat16>(maps_dev, M, tokens, mc, parts, st);
}

extern "C" int attwarp_cubic_coeffs(int n_in, int n_out, int32_t* ofs, float* coeffs) {
  ATTWARP_REQUIRE(ofs && coeffs, "cubic_coeffs: null pointer");
  ATTWARP_REQUIRE(n_in > 0 && n_out > 0, "cubic_coeffs: non-positive size %d -> %d", n_in, n_out);
  for (int d = 0; d < n_out; ++d) {
    int s;
    const float f = resize_source_coord(n_in, n_out, d, &s);
    ofs[d] = s;
    interpolate_cubic(f, coeffs + (size_t)d * 4);
  }
  return ATTWARP_OK;
}

extern "C" int attwarp_resize_cubic(const attwarp_cubic_map* maps, const attwarp_cubic_map* maps_dev, int M, void* stream) {
  ATTWARP_REQUIRE(maps && maps_dev, "resize_cubic: null pointer");
  ATTWARP_REQUIRE(M > 0, "resize_cubic: non-positive map count");
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(maps_dev) % 8 == 0, "resize_cubic: maps_dev must be 8-byte aligned");
  if (M > MAX_RECORDS) return fail(ATTWARP_E_UNSUPPORTED, "resize_cubic: M=%d > %d", M, MAX_RECORDS);
  int mb = 0;
  for (int m = 0; m < M; ++m) {
    const CMap& d = maps[m];
    ATTWARP_REQUIRE(d.src && d.out, "resize_cubic: map %d: null src / out", m);
    ATTWARP_REQUIRE(d.h > 0 && d.w > 0 && d.H > 0 && d.W > 0, "resize_cubic: map %d: non-positive size %d x %d -> %d x %d", m, d.h, d.w, d.H, d.W);
    if (d.h > MAX_SIDE || d.w > MAX_SIDE || d.H > MAX_SIDE || d.W > MAX_SIDE)
      return fail(ATTWARP_E_UNSUPPORTED, "resize_cubic: map %d: %d x %d -> %d x %d (> %d)", m, d.h, d.w, d.H, d.W, MAX_SIDE);
    ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(d.src) % 4 == 0 && reinterpret_cast<uintptr_t>(d.out) % 4 == 0,
                    "resize_cubic: map %d: src / out not 4-byte aligned", m);
    if (!(d.H == d.h && d.W == d.w))
      ATTWARP_REQUIRE(d.ofs_x && d.coef_x && d.ofs_y && d.coef_y, "resize_cubic: map %d: null coefficient table", m);
    mb = std::max(mb, ctiles_of(d.W) * cbands_of(d.H));
  }
  hipLaunchKernelGGL(cubic_kernel, dim3((unsigned)mb, (unsigned)M), dim3(NT), 0, as_stream(stream), maps_dev);
  return check_launch("cubic_kernel");
}

extern "C" int attwarp_gaussian5_taps(double sigma, float* taps) {
  ATTWARP_REQUIRE(taps, "gaussian5_taps: null pointer");
  ATTWARP_REQUIRE(sigma > 0, "gaussian5_taps: sigma must be positive");
  const double scale2x = -0.5 / (sigma * sigma);
  double t[5], sum = 0;
  for (int i = 0; i < 5; ++i) {
    const double x = i - 2.0;
    t[i] = std::exp(scale2x * x * x);
    sum += t[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < 5; ++i) taps[i] = (float)(t[i] * sum);
  return ATTWARP_OK;
}

extern "C" size_t attwarp_blur5_minmax_workspace_bytes(const attwarp_f32_map* maps, int M) {
  if (!maps || M <= 0) return 0;
  int64_t mb = 0;
  for (int m = 0; m < M; ++m)
    if (maps[m].H > 0 && maps[m].W > 0) mb = std::max(mb, bblocks_of(maps[m].H, maps[m].W));
  return (size_t)M * (size_t)(mb + 1) * sizeof(MinMax);       // [M, mb] partials, then [M] finals
}

extern "C" int attwarp_blur5_minmax(const attwarp_f32_map* maps, const attwarp_f32_map* maps_dev, int M, int blur, void* ws,
                                    void* stream) {
  int64_t mb = 0, me = 0;
  if (const int rc = validate_fmaps("blur5_minmax", maps, maps_dev, M, blur != 0, &mb, &me)) return rc;
  ATTWARP_REQUIRE(blur != 0 || ws, "blur5_minmax: blur == 0 without a workspace has nothing to do");
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, "blur5_minmax: ws must be 8-byte aligned");
  if (blur)
    for (int m = 0; m < M; ++m) ATTWARP_REQUIRE(maps[m].out != maps[m].src, "blur5_minmax: map %d: the blur cannot run in place", m);
  float t[5];
  if (const int rc = attwarp_gaussian5_taps(1.0, t)) return rc;
  Taps k;
  k.k0 = t[2]; k.k1 = t[1]; k.k2 = t[0];
  const dim3 grid((unsigned)mb, (unsigned)M);
  MinMax* parts = static_cast<MinMax*>(ws);
  if (blur) hipLaunchKernelGGL(blur_kernel<true>, grid, dim3(NT), 0, as_stream(stream), maps_dev, k, (int)mb, parts);
  else hipLaunchKernelGGL(blur_kernel<false>, grid, dim3(NT), 0, as_stream(stream), maps_dev, k, (int)mb, parts);
  return check_launch("blur_kernel");
}

extern "C" int attwarp_minmax_normalize(const attwarp_f32_map* maps, const attwarp_f32_map* maps_dev, int M, void* ws,
                                        void* stream) {
  int64_t mb = 0, me = 0;
  if (const int rc = validate_fmaps("minmax_normalize", maps, maps_dev, M, true, &mb, &me)) return rc;
  ATTWARP_REQUIRE(ws, "minmax_normalize: null workspace");
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, "minmax_normalize: ws must be 8-byte aligned");
  MinMax* parts = static_cast<MinMax*>(ws);
  MinMax* fin = parts + (size_t)M * (size_t)mb;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(minmax_final_kernel, dim3((unsigned)M), dim3(NT), 0, st, maps_dev, (int)mb, parts, fin);
  if (const int rc = check_launch("minmax_final_kernel")) return rc;
  const unsigned gx = (unsigned)((me + NORM_PER_BLOCK - 1) / NORM_PER_BLOCK);
  hipLaunchKernelGGL(normalize_kernel, dim3(gx, (unsigned)M), dim3(NT), 0, st, maps_dev, fin);
  return check_launch("normalize_kernel");
}
