// The layer-selection study's map arithmetic (Ablations/uncertainty_attn_maps_llava.py:62-64 and
// Ablations/attention_redistribution/metrics.py:15-25): cv2.resize(float32 grid, (W, H), INTER_LANCZOS4) of a 24 x 24
// attention grid, and top1 / am_all of the up-sampled map against a box -- either on maps in memory (dense) or on the
// LANCZOS4 value of each pixel computed on the fly (fused: the full-resolution map is never written).
//
// Resize arithmetic = OpenCV 4.x resizeGeneric_ with HResizeLanczos4 / VResizeLanczos4 for one float32 channel
// (modules/imgproc/src/resize.cpp), restated in tests/grounding_ref.py:
//   * coefficient tables per axis on the HOST (attwarp_lanczos4_coeffs below: glibc sin / cos, as OpenCV on Linux);
//   * horizontal pass first, Hrow[x] = sum_j c_x[j] * S[clamp(ofs_x - 3 + j)], then the vertical pass
//     out[y][x] = sum_k c_y[k] * Hrow[clamp(ofs_y - 3 + k)][x]; float32, every product and sum rounded separately
//     (-ffp-contract=off), taps summed in ascending order starting from the first product;
//   * dsize == ssize is a plain copy (cv::resize does src.copyTo(dst)).
//
// Work decomposition (resize and both metric paths): one 256-thread workgroup per (map, 256-column tile, 256-row band).
// The workgroup computes the horizontal pass of its tile for every grid row into LDS (h x 256 floats, h <= 64), then each
// thread walks down its column: the eight Hrow values of the current source window stay in registers and are reloaded
// only when ofs_y moves (every ~H/h rows when up-sampling), so a pixel costs 8 multiplies and 7 adds.
//
// Metrics: per thread, its column's float64 sums (rows inside / outside the box's row range) and the np.argmax candidate
// (first index among equal maxima, the first NaN wins over everything); fixed-order block reductions into one partial per
// workgroup; a second launch combines each map's partials in block order.  No floating-point atomics: the same inputs give
// the same bits, and the dense and fused paths -- the same kernel body with another value source -- give identical bits on
// identical values.
#include "common.hpp"
#include "pil8.hpp"          // clampi
#include "resize_axis.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace attwarp {
namespace grounding {

constexpr int NT = 256;        // threads = output columns of a tile
constexpr int TILE = NT;
constexpr int BAND = 256;      // output rows per workgroup
constexpr int MAX_GRID = 64;   // h, w <= 64: the horizontal pass of a tile is h x TILE floats of LDS (<= 64 KB)
constexpr int MAX_SIDE = 1 << 15;

typedef attwarp_grid_map Map;

struct Part {                  // one workgroup's partial (32 bytes)
  double tot, box;             // float64 sums: all pixels / pixels of the box slice
  float best;                  // argmax candidate and its row-major index (-1: no pixel)
  int32_t pad;
  int64_t idx;
};

inline int tiles_of(int W) { return (W + TILE - 1) / TILE; }
inline int bands_of(int H) { return (H + BAND - 1) / BAND; }

// np.argmax's order: a NaN beats every number and the first NaN wins; otherwise the larger value, the first index on ties
// (-0.0 == 0.0).  (v, i) takes (v2, i2) when that is the earlier element of this order; i < 0 marks "no candidate".
__device__ __forceinline__ void amax_combine(float& v, int64_t& i, float v2, int64_t i2) {
  if (i2 < 0) return;
  bool take;
  if (i < 0) take = true;
  else {
    const bool n1 = v != v, n2 = v2 != v2;
    if (n1 || n2) take = n2 && (!n1 || i2 < i);
    else take = v2 > v || (v2 == v && i2 < i);
  }
  if (take) { v = v2; i = i2; }
}

// horizontal pass of the column x of a tile for all h grid rows -> hrow[r * TILE + threadIdx.x]
__device__ __forceinline__ void hpass(const Map& d, int h, int w, int x, float* hrow) {
  if (x >= d.W) return;
  const int ox = d.ofs_x[x];
  float c[8];
  int col[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = d.coef_x[(int64_t)x * 8 + j];
    col[j] = clampi(ox - 3 + j, 0, w - 1);
  }
  for (int r = 0; r < h; ++r) {
    const float* S = d.src + r * w;
    float v = fmul(S[col[0]], c[0]);
#pragma unroll
    for (int j = 1; j < 8; ++j) v = fadd(v, fmul(S[col[j]], c[j]));
    hrow[r * TILE + threadIdx.x] = v;
  }
}

// vertical pass at output row y for this thread's column; win holds Hrow of source rows clamp(cur-3 .. cur+4)
struct Window {
  int cur;
  float v[8];
};
__device__ __forceinline__ float vpass(const Map& d, const float* hrow, int h, int y, Window& win) {
  const int oy = d.ofs_y[y];
  if (oy != win.cur) {
#pragma unroll
    for (int k = 0; k < 8; ++k) win.v[k] = hrow[clampi(oy - 3 + k, 0, h - 1) * TILE + threadIdx.x];
    win.cur = oy;
  }
  const float* c = d.coef_y + (int64_t)y * 8;
  float v = fmul(win.v[0], c[0]);
#pragma unroll
  for (int k = 1; k < 8; ++k) v = fadd(v, fmul(win.v[k], c[k]));
  return v;
}

// the workgroup's (map, tile, band); false when this block has no work (grid.x = the largest block count of the call)
struct Block {
  int x, y0, y1;
};
__device__ __forceinline__ bool block_of(const Map& d, Block& b) {
  const int tx = (d.W + TILE - 1) / TILE, nb = tx * ((d.H + BAND - 1) / BAND);
  if ((int)blockIdx.x >= nb) return false;
  const int tile = blockIdx.x % tx, band = blockIdx.x / tx;
  b.x = tile * TILE + threadIdx.x;
  b.y0 = band * BAND;
  b.y1 = min(d.H, b.y0 + BAND);
  return true;
}

__global__ __launch_bounds__(NT) void resize_kernel(const Map* __restrict__ maps, int h, int w) {
  extern __shared__ float hrow[];
  const Map d = maps[blockIdx.y];
  Block b;
  if (!block_of(d, b)) return;
  const bool copy = d.H == h && d.W == w;
  if (!copy) hpass(d, h, w, b.x, hrow);
  __syncthreads();
  if (b.x >= d.W) return;
  if (copy) {
    for (int y = b.y0; y < b.y1; ++y) d.out[(int64_t)y * d.W + b.x] = d.src[(int64_t)y * d.W + b.x];
    return;
  }
  Window win;
  win.cur = INT_MIN;
  for (int y = b.y0; y < b.y1; ++y) d.out[(int64_t)y * d.W + b.x] = vpass(d, hrow, h, y, win);
}

// FUSED: the value of a pixel is the LANCZOS4 value of the grid src [h,w]; dense: src is the map [H,W] itself
template <bool FUSED>
__global__ __launch_bounds__(NT) void metrics_kernel(const Map* __restrict__ maps, int h, int w, int max_blocks,
                                                     Part* __restrict__ parts) {
  extern __shared__ float hrow[];
  __shared__ double red[NT / WAVE];
  __shared__ float s_v[NT / WAVE];
  __shared__ int64_t s_i[NT / WAVE];
  const Map d = maps[blockIdx.y];
  Block b;
  if (!block_of(d, b)) return;
  const bool direct = !FUSED || (d.H == h && d.W == w);
  if (!direct) hpass(d, h, w, b.x, hrow);
  __syncthreads();
  double a_in = 0.0, a_out = 0.0;          // this column's sums over the rows inside / outside [r0, r1)
  float bv = 0.0f;
  int64_t bi = -1;
  if (b.x < d.W) {
    Window win;
    win.cur = INT_MIN;
    for (int y = b.y0; y < b.y1; ++y) {
      const int64_t idx = (int64_t)y * d.W + b.x;
      const float v = direct ? d.src[idx] : vpass(d, hrow, h, y, win);
      if (y >= d.r0 && y < d.r1) a_in += (double)v;
      else a_out += (double)v;
      if (bi < 0 || (!(bv != bv) && (v != v || v > bv))) { bv = v; bi = idx; }   // rows ascend: first index on ties
    }
  }
  const bool in_cols = b.x >= d.c0 && b.x < d.c1;
  const double tot = block_sum(a_out + a_in, red);
  const double box = block_sum(in_cols ? a_in : 0.0, red);
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(bv, o, WAVE);
    const int64_t i2 = __shfl_xor(bi, o, WAVE);
    amax_combine(bv, bi, v2, i2);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) { s_v[threadIdx.x / WAVE] = bv; s_i[threadIdx.x / WAVE] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = s_v[0];
    int64_t i = s_i[0];
    for (int k = 1; k < NT / WAVE; ++k) amax_combine(v, i, s_v[k], s_i[k]);
    Part p;
    p.tot = tot; p.box = box; p.best = v; p.pad = 0; p.idx = i;
    parts[(int64_t)blockIdx.y * max_blocks + blockIdx.x] = p;
  }
}

// one thread per map: its partials in block order -> argmax, top1 (the plain inequalities of metrics.py:19 on the box as
// interpret_bbox gives it), am = box / (total + 1e-12) in float64 (metrics.py:25)
__global__ __launch_bounds__(NT) void metrics_final_kernel(const Map* __restrict__ maps, int M, int max_blocks,
                                                           const Part* __restrict__ parts, int64_t* __restrict__ argmax,
                                                           int32_t* __restrict__ top1, double* __restrict__ am) {
  const int m = blockIdx.x * NT + threadIdx.x;
  if (m >= M) return;
  const Map d = maps[m];
  const int nb = ((d.W + TILE - 1) / TILE) * ((d.H + BAND - 1) / BAND);
  const Part* p = parts + (int64_t)m * max_blocks;
  double tot = p[0].tot, box = p[0].box;
  float bv = p[0].best;
  int64_t bi = p[0].idx;
  for (int k = 1; k < nb; ++k) {
    tot += p[k].tot;
    box += p[k].box;
    amax_combine(bv, bi, p[k].best, p[k].idx);
  }
  const int64_t r = bi / d.W, c = bi - r * d.W;
  argmax[m] = bi;
  top1[m] = (d.box_x <= c && c < d.box_x + d.box_w && d.box_y <= r && r < d.box_y + d.box_h) ? 1 : 0;
  am[m] = box / (tot + 1e-12);
}

// ---- host: OpenCV's interpolateLanczos4 (imgproc/src/resize.cpp) and the per-axis tables of resizeGeneric_ ------------
static void interpolate_lanczos4(float x, float* coeffs) {
  static const double s45 = 0.70710678118654752440084436210485;
  static const double cs[][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
  const double pi = 3.1415926535897932384626433832795;   // CV_PI
  float sum = 0;
  const double y0 = -(x + 3) * pi * 0.25, s0 = std::sin(y0), c0 = std::cos(y0);
  for (int i = 0; i < 8; i++) {
    const float y0_ = (x + 3 - i);
    if (std::fabs(y0_) >= 1e-6f) {
      const double y = -y0_ * pi * 0.25;
      coeffs[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
    } else {
      coeffs[i] = 1e30f;
    }
    sum += coeffs[i];
  }
  sum = 1.f / sum;
  for (int i = 0; i < 8; i++) coeffs[i] *= sum;
}

static int validate_maps(const char* who, const Map* maps, const Map* maps_dev, int M, int h, int w, bool need_out,
                         bool dense, int* max_blocks) {
  ATTWARP_REQUIRE(maps && maps_dev, "%s: null pointer", who);
  ATTWARP_REQUIRE(M > 0, "%s: non-positive map count", who);
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(maps_dev) % 8 == 0, "%s: maps_dev must be 8-byte aligned", who);
  if (M > 65535) return fail(ATTWARP_E_UNSUPPORTED, "%s: M=%d > 65535", who, M);
  if (!dense) {
    ATTWARP_REQUIRE(h > 0 && w > 0, "%s: non-positive grid size %d x %d", who, h, w);
    if (h > MAX_GRID || w > MAX_GRID) return fail(ATTWARP_E_UNSUPPORTED, "%s: grid %d x %d (> %d)", who, h, w, MAX_GRID);
  }
  int mb = 0;
  for (int m = 0; m < M; ++m) {
    const Map& d = maps[m];
    ATTWARP_REQUIRE(d.src, "%s: map %d: null src", who, m);
    ATTWARP_REQUIRE(!need_out || d.out, "%s: map %d: null out", who, m);
    ATTWARP_REQUIRE(d.H > 0 && d.W > 0, "%s: map %d: non-positive size %d x %d", who, m, d.H, d.W);
    if (d.H > MAX_SIDE || d.W > MAX_SIDE) return fail(ATTWARP_E_UNSUPPORTED, "%s: map %d: %d x %d (> %d)", who, m, d.H, d.W, MAX_SIDE);
    ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(d.src) % 4 == 0 && reinterpret_cast<uintptr_t>(d.out) % 4 == 0,
                    "%s: map %d: src / out not 4-byte aligned", who, m);
    if (!dense && !(d.H == h && d.W == w))
      ATTWARP_REQUIRE(d.ofs_x && d.coef_x && d.ofs_y && d.coef_y, "%s: map %d: null coefficient table", who, m);
    mb = std::max(mb, tiles_of(d.W) * bands_of(d.H));
  }
  *max_blocks = mb;
  return ATTWARP_OK;
}

static size_t lds_bytes(int h) { return (size_t)h * TILE * sizeof(float); }
// metrics_kernel's own __shared__ variables (red, s_v, s_i): its "LDS Size" at zero dynamic LDS.  With them the fused
// kernel needs 65616 bytes at h = 64, past the 64 KB a launch gets by default, so its launcher asks for the grant.
constexpr size_t METRICS_STATIC_LDS = 80;

}  // namespace grounding
}  // namespace attwarp

using namespace attwarp;
using namespace attwarp::grounding;

extern "C" int attwarp_lanczos4_coeffs(int n_in, int n_out, int32_t* ofs, float* coeffs) {
  ATTWARP_REQUIRE(ofs && coeffs, "lanczos4_coeffs: null pointer");
  ATTWARP_REQUIRE(n_in > 0 && n_out > 0, "lanczos4_coeffs: non-positive size %d -> %d", n_in, n_out);
  for (int d = 0; d < n_out; ++d) {
    int s;
    const float f = resize_source_coord(n_in, n_out, d, &s);
    ofs[d] = s;
    interpolate_lanczos4(f, coeffs + (size_t)d * 8);
  }
  return ATTWARP_OK;
}

extern "C" int attwarp_resize_lanczos4(const attwarp_grid_map* maps, const attwarp_grid_map* maps_dev, int M, int h, int w,
                                       void* stream) {
  int mb = 0;
  if (const int rc = validate_maps("resize_lanczos4", maps, maps_dev, M, h, w, true, false, &mb)) return rc;
  if (const int rc = grant_dynamic_lds(resize_kernel, lds_bytes(h), "resize_lanczos4")) return rc;   // (no static LDS: 64 KB at h = 64)
  hipLaunchKernelGGL(resize_kernel, dim3((unsigned)mb, (unsigned)M), dim3(NT), lds_bytes(h), as_stream(stream), maps_dev, h, w);
  return check_launch("resize_kernel");
}

extern "C" size_t attwarp_box_metrics_workspace_bytes(const attwarp_grid_map* maps, int M) {
  if (!maps || M <= 0) return 0;
  int mb = 0;
  for (int m = 0; m < M; ++m)
    if (maps[m].H > 0 && maps[m].W > 0) mb = std::max(mb, tiles_of(maps[m].W) * bands_of(maps[m].H));
  return (size_t)M * mb * sizeof(Part);
}

extern "C" int attwarp_box_metrics(const attwarp_grid_map* maps, const attwarp_grid_map* maps_dev, int M, int fused, int h,
                                   int w, int64_t* argmax, int32_t* top1, double* am, void* ws, void* stream) {
  int mb = 0;
  const bool dense = fused == 0;
  if (const int rc = validate_maps("box_metrics", maps, maps_dev, M, h, w, false, dense, &mb)) return rc;
  ATTWARP_REQUIRE(argmax && top1 && am && ws, "box_metrics: null output or workspace");
  ATTWARP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "box_metrics: ws must be 16-byte aligned");
  for (int m = 0; m < M; ++m) {
    const Map& d = maps[m];
    ATTWARP_REQUIRE(0 <= d.r0 && d.r0 <= d.r1 && d.r1 <= d.H && 0 <= d.c0 && d.c0 <= d.c1 && d.c1 <= d.W,
                    "box_metrics: map %d: box slice [%d:%d, %d:%d] outside %d x %d (or reversed)", m, d.r0, d.r1, d.c0, d.c1,
                    d.H, d.W);
    const int64_t lim = (int64_t)1 << 40;
    ATTWARP_REQUIRE(d.box_x > -lim && d.box_x < lim && d.box_y > -lim && d.box_y < lim && d.box_w > -lim && d.box_w < lim &&
                        d.box_h > -lim && d.box_h < lim,
                    "box_metrics: map %d: box coordinates beyond +-2^40", m);
  }
  hipStream_t st = as_stream(stream);
  Part* parts = static_cast<Part*>(ws);
  const dim3 grid((unsigned)mb, (unsigned)M);
  if (dense) {
    hipLaunchKernelGGL(metrics_kernel<false>, grid, dim3(NT), 0, st, maps_dev, h, w, mb, parts);
  } else {
    if (const int rc = grant_dynamic_lds(metrics_kernel<true>, lds_bytes(h), "box_metrics", METRICS_STATIC_LDS)) return rc;
    hipLaunchKernelGGL(metrics_kernel<true>, grid, dim3(NT), lds_bytes(h), st, maps_dev, h, w, mb, parts);
  }
  if (const int rc = check_launch("metrics_kernel")) return rc;
  hipLaunchKernelGGL(metrics_final_kernel, dim3((unsigned)((M + NT - 1) / NT)), dim3(NT), 0, st, maps_dev, M, mb, parts, argmax,
                     top1, am);
  return check_launch("metrics_final_kernel");
}
