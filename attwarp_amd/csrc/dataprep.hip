// The MarginalNet trainer's batches from decoded samples (MN/dataloader.py:123-137, 160-189, 204-273; collate_str of
// MN/data.py): images of their own sizes -> T.Resize((S,S)) + T.ToTensor, attention arrays -> normalise -> x255 truncated
// to 8 bits -> NEAREST resize -> ToTensor, stacked.
//
// Arithmetic:
//   image      Pillow's 8-bit two-pass resample with the triangle filter (ATTWARP_PIL_BILINEAR tables of
//              attwarp_pil_coeffs_8bpc: 22-bit fixed point, horizontal pass first, uint8 between the passes, identity tables
//              on an axis that keeps its size; Image.resize runs the VERTICAL pass first on a source more than 100 times
//              as high as wide that it shrinks vertically: the caller marks those images vertical_first), then
//              float32(float64(u8) * (1/255)) -- equal to the IEEE float32 division u8 / 255 of ToTensor for all 256
//              values (u8 * float32(1/255) is not) -- channels first.
//   attention  see attwarp.h; the 8-bit image of the reference is never stored: x255, the truncation and /255 are applied
//              to each gathered element (NEAREST only selects).
//
// prep_fused_kernel: a workgroup owns one (image, band of output rows) item of a host-built list.  It stages the source
// rows the band's vertical taps need into LDS RB rows at a time (dword loads at any byte address), runs the horizontal
// pass from LDS with the byte window of pil8.hpp (as clip.hip does) into uint8 rows of S_w*C bytes that stay in LDS,
// then the vertical pass from those rows through the 256-entry /255 table, each lane storing four consecutive floats of
// one plane.  The band height follows the image's vertical scale: neighbouring bands recompute the 2 * support source
// rows they share, which the host keeps near an eighth of a band's rows.
#include "common.hpp"
#include "pil8.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace attwarp {
namespace prep {

constexpr uint32_t PREP_MAGIC = 0x50455250u;       // "PREP"
constexpr int NT = 256;                            // == entries of the /255 table: thread t writes entry t
constexpr int LUT_BYTES = 256 * 4;
constexpr int SLACK = 128;                         // behind the staged rows: the byte window of the last pixels reads past the row
constexpr int SPLIT_H_ROWS = 16, SPLIT_V_ROWS = 8; // rows per item of the two-launch route
constexpr int ATT_CH = 16;                         // partial maxima per attention map
constexpr int ATT_ROWS = 8;                        // output rows per workgroup of the attention gather

struct PrepImageDev {                              // the per-image record inside a table
  attwarp_prep_image r;
  int64_t tmp_off;                                 // two-launch route: where its uint8 intermediate starts in tmp
  int32_t fused, ny, rb, nr_cap;                   // one-launch route: band height, staged rows per round, LDS rows of the band
};
struct PrepItem { int32_t img, y0, ny, reserved; };

// grid = items, NT threads.  LDS: lut[256] float | inter[nr_cap][ocp] | srow[rb][wcp] | SLACK   (row bytes rounded up to 4)
template <int C, int KS>
__global__ __launch_bounds__(NT) void prep_fused_kernel(const PrepImageDev* __restrict__ images,
                                                        const PrepItem* __restrict__ items, int S_h, int S_w,
                                                        float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  const int tid = threadIdx.x;
  const PrepItem it = items[blockIdx.x];
  const PrepImageDev& im = images[it.img];
  const int H = im.r.H, W = im.r.W, wc = W * C, oc = S_w * C, wcp = (wc + 3) & ~3, ocp = (oc + 3) & ~3;
  const int RB = im.rb;
  float* lut = reinterpret_cast<float*>(lds_b);
  uint8_t* inter = lds_b + LUT_BYTES;
  uint8_t* srow = inter + (size_t)im.nr_cap * ocp;
  lut[tid] = pil_u8_to_unit(tid);

  const int32_t* __restrict__ by = im.r.bounds_y;
  const int y0 = it.y0, y1 = it.y0 + it.ny;
  const int r0 = clampi(by[2 * y0], 0, H - 1);
  const int nr = clampi(by[2 * (y1 - 1)] + by[2 * (y1 - 1) + 1], r0 + 1, H) - r0;
  if (nr > im.nr_cap) {
    // The band's taps span more source rows than the host's bound (band_rows) reserved in LDS: tables that are not Pillow's
    // for this size, or a bound gone wrong.  Computing on would clamp taps and give plausible wrong pixels: the band's
    // output becomes NaN instead (block-uniform branch, before any barrier).
    float* oimg = out + (size_t)it.img * C * S_h * S_w;
    for (int e = tid; e < C * it.ny * S_w; e += NT) {
      const int c = e / (it.ny * S_w), rem = e - c * it.ny * S_w;
      oimg[((size_t)c * S_h + y0) * S_w + rem] = __int_as_float(0x7fc00000);
    }
    return;
  }

  // ---- horizontal pass: source rows r0 .. r0 + nr -> inter
  const int ndw = wcp >> 2, full = wc >> 2, ksx = im.r.ksize_x;
  const int32_t* __restrict__ bx = im.r.bounds_x;
  const int32_t* __restrict__ kx = im.r.kk_x;
  for (int rs = 0; rs < nr; rs += RB) {
    const int nrows = min(RB, nr - rs);
    const uint8_t* sp = im.r.image + (size_t)(r0 + rs) * wc;
    for (int i = tid; i < nrows * ndw; i += NT) {
      const int r = i / ndw, d = i - r * ndw;
      const uint8_t* a = sp + (size_t)r * wc + 4 * d;
      uint32_t v;
      if (d < full) {
        v = *reinterpret_cast<const u32_una*>(a);
      } else {                                     // the row's last 1..3 bytes: never a load past the image
        v = 0;
        for (int j = 0; j < wc - 4 * full; ++j) v |= (uint32_t)a[j] << (8 * j);
      }
      reinterpret_cast<uint32_t*>(srow + (size_t)r * wcp)[d] = v;
    }
    __syncthreads();
    // the byte window of pil8.hpp; its over-read lands in the next staged row or in SLACK
    for (int xx = tid; xx < S_w; xx += NT) {
      const int xmin = clampi(bx[2 * xx], 0, W - 1), cnt = bx[2 * xx + 1];
      int kreg[KS];
#pragma unroll
      for (int x = 0; x < KS; ++x) kreg[x] = (x < cnt && x < ksx) ? kx[(size_t)xx * ksx + x] : 0;
      const int o = xmin * C, sh = o & 3;
      const uint8_t* first = srow + (o & ~3);
      for (int r = 0; r < nrows; ++r)
        pil_h_window<C, KS>(reinterpret_cast<const uint32_t*>(first + (size_t)r * wcp), sh, kreg,
                            inter + (size_t)(rs + r) * ocp + xx * C);
    }
    __syncthreads();
  }

  // ---- vertical pass: inter -> planar float32 rows; a lane owns four consecutive pixels of one plane (one dwordx4 store)
  const int32_t* __restrict__ ky = im.r.kk_y;
  const int ksy = im.r.ksize_y;
  float* oimg = out + (size_t)it.img * C * S_h * S_w;
  const bool vec = (S_w & 3) == 0;
  const int per = vec ? 4 : 1, groups = C * S_w / per;
  for (int yy = y0; yy < y1; ++yy) {
    const int rel = clampi(by[2 * yy], 0, H - 1) - r0, cnt = min(by[2 * yy + 1], ksy);
    const int32_t* k = ky + (size_t)yy * ksy;
    for (int g = tid; g < groups; g += NT) {
      const int i = g * per, c = i / S_w, xx = i - c * S_w;
      const uint8_t* col = inter + xx * C + c;
      float* o = oimg + ((size_t)c * S_h + yy) * S_w + xx;
      if (vec) {
        int a0 = PIL_ROUND_HALF, a1 = a0, a2 = a0, a3 = a0;
        for (int t = 0; t < cnt; ++t) {
          const int kv = __builtin_amdgcn_readfirstlane(k[t]);
          const uint8_t* row = col + (size_t)clampi(rel + t, 0, nr - 1) * ocp;
          mad24s(a0, row[0], kv);
          mad24s(a1, row[C], kv);
          mad24s(a2, row[2 * C], kv);
          mad24s(a3, row[3 * C], kv);
        }
        *reinterpret_cast<float4*>(o) =
            make_float4(lut[pil_clip8(a0)], lut[pil_clip8(a1)], lut[pil_clip8(a2)], lut[pil_clip8(a3)]);
      } else {
        int a0 = PIL_ROUND_HALF;
        for (int t = 0; t < cnt; ++t) {
          const int kv = __builtin_amdgcn_readfirstlane(k[t]);
          mad24s(a0, col[(size_t)clampi(rel + t, 0, nr - 1) * ocp], kv);
        }
        *o = lut[pil_clip8(a0)];
      }
    }
  }
}

// ---- the two-launch route: one thread per output element, taps from memory, the uint8 intermediate in `tmp`.
// Horizontal pass first ([H, S_w*C] in between), or -- vertical_first images -- vertical pass first ([S_h, W*C]).
struct SplitTaps { const uint8_t* p; const int32_t* k; int cnt; size_t step; };
__device__ __forceinline__ SplitTaps split_taps(const int32_t* bounds, const int32_t* kk, int ksize, int o, int n_in,
                                                const uint8_t* base, size_t step) {
  const int lo = clampi(bounds[2 * o], 0, n_in - 1);
  return SplitTaps{base + lo * step, kk + (size_t)o * ksize, min(min(bounds[2 * o + 1], ksize), n_in - lo), step};
}
__device__ __forceinline__ uint8_t split_sum(const SplitTaps& t) { return pil_tap_sum(t.p, t.step, t.k, t.cnt); }

__global__ __launch_bounds__(NT) void prep_split_first_kernel(const PrepImageDev* __restrict__ images,
                                                              const PrepItem* __restrict__ items, int C, int S_w,
                                                              uint8_t* __restrict__ tmp) {
  const PrepItem it = items[blockIdx.x];
  const PrepImageDev& im = images[it.img];
  const attwarp_prep_image& r = im.r;
  const int wc = r.W * C, L = r.vertical_first ? wc : S_w * C;            // bytes of an intermediate row
  uint8_t* t = tmp + im.tmp_off;
  for (int e = threadIdx.x; e < it.ny * L; e += NT) {
    const int row = it.y0 + e / L, j = e % L;
    const SplitTaps taps = r.vertical_first
        ? split_taps(r.bounds_y, r.kk_y, r.ksize_y, row, r.H, r.image + j, (size_t)wc)
        : split_taps(r.bounds_x, r.kk_x, r.ksize_x, j / C, r.W, r.image + (size_t)row * wc + j % C, (size_t)C);
    t[(size_t)row * L + j] = split_sum(taps);
  }
}

__global__ __launch_bounds__(NT) void prep_split_second_kernel(const PrepImageDev* __restrict__ images,
                                                               const PrepItem* __restrict__ items, int C, int S_h, int S_w,
                                                               const uint8_t* __restrict__ tmp, float* __restrict__ out) {
  __shared__ float lut[256];
  lut[threadIdx.x] = pil_u8_to_unit(threadIdx.x);
  __syncthreads();
  const PrepItem it = items[blockIdx.x];
  const PrepImageDev& im = images[it.img];
  const attwarp_prep_image& r = im.r;
  const int wc = r.W * C, oc = S_w * C, plane = C * S_w;
  const uint8_t* t = tmp + im.tmp_off;
  float* oimg = out + (size_t)it.img * C * S_h * S_w;
  for (int e = threadIdx.x; e < it.ny * plane; e += NT) {
    const int q = e / plane, rem = e - q * plane, c = rem / S_w, xx = rem - c * S_w, yy = it.y0 + q;
    const SplitTaps taps = r.vertical_first
        ? split_taps(r.bounds_x, r.kk_x, r.ksize_x, xx, r.W, t + (size_t)yy * wc + c, (size_t)C)
        : split_taps(r.bounds_y, r.kk_y, r.ksize_y, yy, r.H, t + xx * C + c, (size_t)oc);
    oimg[((size_t)c * S_h + yy) * S_w + xx] = lut[split_sum(taps)];
  }
}

// ---- attention maps
// grid = B * ATT_CH: partial maximum of one ATT_CH-th of a map; NaN if that part holds one (np.max propagates it)
__global__ __launch_bounds__(NT) void prep_att_max_kernel(const attwarp_prep_attention* __restrict__ maps, float* __restrict__ ws) {
  __shared__ float red[NT / WAVE];
  __shared__ int rnan[NT / WAVE];
  const int b = blockIdx.x / ATT_CH, ch = blockIdx.x - b * ATT_CH;
  const attwarp_prep_attention m = maps[b];
  const long long n = (long long)m.h * m.w, chunk = (n + ATT_CH - 1) / ATT_CH;
  const long long lo = ch * chunk, hi = lo + chunk < n ? lo + chunk : n;
  float mx = -INFINITY;
  int nan = 0;
  for (long long i = lo + threadIdx.x; i < hi; i += NT) {
    const float v = m.map[i];
    nan |= v != v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  nan = __any(nan);
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  if (lane == 0) { red[wid] = mx; rnan[wid] = nan; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < NT / WAVE; ++i) { mx = fmaxf(mx, red[i]); nan |= rnan[i]; }
    ws[blockIdx.x] = nan ? NAN : mx;
  }
}

// grid = B * ceil(S_h / ATT_ROWS): gather, item 4 of the arithmetic per gathered element, store
__global__ __launch_bounds__(NT) void prep_att_gather_kernel(const attwarp_prep_attention* __restrict__ maps,
                                                             const float* __restrict__ ws, int S_h, int S_w, int nblk,
                                                             float* __restrict__ out) {
  __shared__ float lut[256];
  lut[threadIdx.x] = pil_u8_to_unit(threadIdx.x);
  const int b = blockIdx.x / nblk, y0 = (blockIdx.x - b * nblk) * ATT_ROWS, rows = min(ATT_ROWS, S_h - y0);
  const attwarp_prep_attention m = maps[b];
  float mx = -INFINITY;
  bool nan = false;
  for (int i = 0; i < ATT_CH; ++i) {
    const float v = ws[(size_t)b * ATT_CH + i];
    nan |= v != v;
    mx = fmaxf(mx, v);
  }
  const bool divide = m.normalize != 0 && !nan && mx > 1.0f;
  __syncthreads();
  auto value = [&](int iy, int xx) -> float {
    const int ix = clampi(m.idx_x[xx], 0, m.w - 1);
    float v = m.map[(size_t)iy * m.w + ix];
    if (divide) v = __fdiv_rn(v, mx);
    if (v != v || fabsf(v) == INFINITY) v = 0.0f;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return lut[(int)fmul(v, 255.0f)];
  };
  float* o = out + ((size_t)b * S_h + y0) * S_w;
  if ((S_w & 3) == 0) {
    const int q = S_w >> 2;
    for (int e = threadIdx.x; e < rows * q; e += NT) {
      const int r = e / q, xx = 4 * (e - r * q), iy = clampi(m.idx_y[y0 + r], 0, m.h - 1);
      *reinterpret_cast<float4*>(o + (size_t)r * S_w + xx) =
          make_float4(value(iy, xx), value(iy, xx + 1), value(iy, xx + 2), value(iy, xx + 3));
    }
  } else {
    for (int e = threadIdx.x; e < rows * S_w; e += NT) {
      const int r = e / S_w, xx = e - r * S_w, iy = clampi(m.idx_y[y0 + r], 0, m.h - 1);
      o[(size_t)r * S_w + xx] = value(iy, xx);
    }
  }
}

// ---- host: the table of one batch
struct PrepLayout {
  attwarp_prep_header h;
  std::vector<PrepImageDev> images;
  std::vector<PrepItem> fused, wide, hitems, vitems;      // fused: the 8-tap window; wide: 9 .. 16 horizontal taps
};

static size_t fused_lds(long long nr, long long ocp, long long rb, long long wcp) {
  return (size_t)(LUT_BYTES + nr * ocp + rb * wcp + SLACK);
}

// source rows a band of ny output rows can touch: the first taps of two rows ny - 1 apart lie at most
// floor((ny - 1) * scale) + 1 apart, the last row adds its ksize_y taps
static long long band_rows(int ny, int H, int S_h, int ksize_y) {
  const long long nr = (long long)(ny - 1) * H / S_h + 2 + ksize_y;
  return nr < H ? nr : H;
}

static int prep_layout(const attwarp_prep_image* images, int B, int C, int S_h, int S_w, PrepLayout& L) {
  ATTWARP_REQUIRE(images, "prep_images: null image list");
  ATTWARP_REQUIRE(B > 0 && S_h > 0 && S_w > 0, "prep_images: non-positive size");
  ATTWARP_REQUIRE(C == 1 || C == 3, "prep_images: C must be 1 or 3 (got %d)", C);
  if (B > (1 << 20) || (long long)S_w * C > 65536 || S_h > 65535)
    return fail(ATTWARP_E_UNSUPPORTED, "prep_images: B > 2^20, S_h > 65535 or S_w * C > 65536");
  const bool force_split = tune(TUNE_PREP_VARIANT) == 1;
  const long long oc = (long long)S_w * C, ocp = (oc + 3) & ~3LL;
  attwarp_prep_header& h = L.h;
  memset(&h, 0, sizeof(h));
  h.magic = PREP_MAGIC; h.B = B; h.C = C; h.S_h = S_h; h.S_w = S_w; h.ks = 8;
  L.images.resize((size_t)B);
  size_t lds = 0;
  long long tmp = 0;
  for (int b = 0; b < B; ++b) {
    const attwarp_prep_image& r = images[b];
    ATTWARP_REQUIRE(r.image && r.bounds_x && r.kk_x && r.bounds_y && r.kk_y, "prep_images: image %d: null pointer", b);
    ATTWARP_REQUIRE(r.H > 0 && r.W > 0 && r.ksize_x > 0 && r.ksize_y > 0, "prep_images: image %d: non-positive size", b);
    if (r.H > 65535 || r.W > 65535) return fail(ATTWARP_E_UNSUPPORTED, "prep_images: image %d: %d x %d exceeds 65535", b, r.H, r.W);
    PrepImageDev& d = L.images[(size_t)b];
    memset(&d, 0, sizeof(d));
    d.r = r;
    const long long wcp = ((long long)r.W * C + 3) & ~3LL;
    // band height from the vertical scale: neighbouring bands share about 2 * max(scale, 1) source rows, a band of ny
    // output rows spans ny * scale, so 14 * max(1, S_h / H) output rows keep the recomputed share near an eighth
    int ny = S_h <= r.H ? 16 : (14LL * S_h <= 32LL * r.H ? 32 : 64);
    bool fused = !force_split && !r.vertical_first && r.ksize_x <= 16;
    if (fused) {
      fused = false;
      for (int pass = 0; pass < 2 && !fused; ++pass)            // first a plan two workgroups of which fit a CU's LDS
        for (int n = ny; n >= 8 && !fused; n >>= 1)
          for (int rb = 8; rb >= 4 && !fused; rb >>= 1) {
            const long long nr = band_rows(n < S_h ? n : S_h, r.H, S_h, r.ksize_y);
            if (fused_lds(nr, ocp, rb, wcp) <= (pass == 0 ? LDS_CU_BYTES / 2 : LDS_CU_BYTES)) {
              fused = true; d.ny = n; d.rb = rb; d.nr_cap = (int32_t)nr;
            }
          }
    }
    d.fused = fused;
    if (fused) {
      ++h.n_fused_images;
      if (r.ksize_x > 8) h.ks = 16;
      const size_t need = fused_lds(d.nr_cap, ocp, d.rb, wcp);
      if (need > lds) lds = need;
      std::vector<PrepItem>& list = r.ksize_x > 8 ? L.wide : L.fused;      // (a launch of its own: the others keep 8 taps)
      for (int y0 = 0; y0 < S_h; y0 += d.ny) list.push_back(PrepItem{b, y0, S_h - y0 < d.ny ? S_h - y0 : d.ny, 0});
    } else {
      ++h.n_split_images;
      d.tmp_off = tmp;
      const int rows1 = r.vertical_first ? S_h : r.H;              // rows of the intermediate
      tmp += ((long long)rows1 * (r.vertical_first ? (long long)r.W * C : oc) + 3) & ~3LL;
      for (int y0 = 0; y0 < rows1; y0 += SPLIT_H_ROWS)
        L.hitems.push_back(PrepItem{b, y0, rows1 - y0 < SPLIT_H_ROWS ? rows1 - y0 : SPLIT_H_ROWS, 0});
      for (int y0 = 0; y0 < S_h; y0 += SPLIT_V_ROWS)
        L.vitems.push_back(PrepItem{b, y0, S_h - y0 < SPLIT_V_ROWS ? S_h - y0 : SPLIT_V_ROWS, 0});
    }
  }
  L.fused.insert(L.fused.end(), L.wide.begin(), L.wide.end());        // 8-tap items first, then the wide ones
  const size_t nitems = L.fused.size() + L.hitems.size() + L.vitems.size();
  if (nitems > 0x7fffffffu) return fail(ATTWARP_E_UNSUPPORTED, "prep_images: too many work items");
  h.n_wide_items = (int32_t)L.wide.size();
  h.n_fused_items = (int32_t)L.fused.size(); h.n_h_items = (int32_t)L.hitems.size(); h.n_v_items = (int32_t)L.vitems.size();
  h.tmp_bytes = (uint64_t)tmp; h.lds_bytes = lds;
  h.off_images = (sizeof(attwarp_prep_header) + 15) & ~(size_t)15;
  h.off_items = h.off_images + (size_t)B * sizeof(PrepImageDev);
  h.table_bytes = (h.off_items + nitems * sizeof(PrepItem) + 15) & ~(uint64_t)15;
  return ATTWARP_OK;
}

template <int C>
static int launch_fused(const attwarp_prep_header* h, const PrepImageDev* images, const PrepItem* items, float* out,
                        hipStream_t st) {
  const size_t lds = (size_t)h->lds_bytes;
  const int n8 = h->n_fused_items - h->n_wide_items;
  if (n8 > 0) {
    if (const int rc = grant_dynamic_lds(prep_fused_kernel<C, 8>, lds, "prep_images_u8")) return rc;
    hipLaunchKernelGGL((prep_fused_kernel<C, 8>), dim3(n8), dim3(NT), lds, st, images, items, h->S_h, h->S_w, out);
    if (const int rc = check_launch("prep_fused_kernel")) return rc;
  }
  if (h->n_wide_items > 0) {        // images shrunk 3 .. 7 times horizontally: the 16-tap window, a launch of their own
    if (const int rc = grant_dynamic_lds(prep_fused_kernel<C, 16>, lds, "prep_images_u8")) return rc;
    hipLaunchKernelGGL((prep_fused_kernel<C, 16>), dim3(h->n_wide_items), dim3(NT), lds, st, images, items + n8, h->S_h, h->S_w, out);
  }
  return check_launch("prep_fused_kernel");
}

}  // namespace prep
}  // namespace attwarp

using namespace attwarp;
using namespace attwarp::prep;

extern "C" size_t attwarp_prep_images_table_bytes(const attwarp_prep_image* images, int B, int C, int S_h, int S_w) try {
  PrepLayout L;
  if (prep_layout(images, B, C, S_h, S_w, L) != ATTWARP_OK) return 0;
  return (size_t)L.h.table_bytes;
} catch (...) {
  fail(ATTWARP_E_UNSUPPORTED, "prep_images_table_bytes: out of host memory");
  return 0;
}

extern "C" int attwarp_prep_images_plan(const attwarp_prep_image* images, int B, int C, int S_h, int S_w, void* table,
                                        size_t table_bytes) try {
  ATTWARP_REQUIRE(table, "prep_images_plan: null table");
  PrepLayout L;
  if (const int rc = prep_layout(images, B, C, S_h, S_w, L)) return rc;
  ATTWARP_REQUIRE(table_bytes >= L.h.table_bytes, "prep_images_plan: the table needs %llu bytes (got %zu)",
                  (unsigned long long)L.h.table_bytes, table_bytes);
  uint8_t* t = static_cast<uint8_t*>(table);
  memset(t, 0, (size_t)L.h.table_bytes);
  memcpy(t, &L.h, sizeof(L.h));
  memcpy(t + L.h.off_images, L.images.data(), L.images.size() * sizeof(PrepImageDev));
  PrepItem* items = reinterpret_cast<PrepItem*>(t + L.h.off_items);
  if (!L.fused.empty()) memcpy(items, L.fused.data(), L.fused.size() * sizeof(PrepItem));
  if (!L.hitems.empty()) memcpy(items + L.fused.size(), L.hitems.data(), L.hitems.size() * sizeof(PrepItem));
  if (!L.vitems.empty()) memcpy(items + L.fused.size() + L.hitems.size(), L.vitems.data(), L.vitems.size() * sizeof(PrepItem));
  return ATTWARP_OK;
} catch (...) {
  return fail(ATTWARP_E_UNSUPPORTED, "prep_images_plan: out of host memory");
}

extern "C" int attwarp_prep_images_u8(const void* table_host, const void* table_dev, uint8_t* tmp, float* out, void* stream) {
  ATTWARP_REQUIRE(table_host && table_dev && out, "prep_images_u8: null pointer");
  const attwarp_prep_header* h = static_cast<const attwarp_prep_header*>(table_host);
  ATTWARP_REQUIRE(h->magic == PREP_MAGIC, "prep_images_u8: the table was not written by attwarp_prep_images_plan");
  ATTWARP_REQUIRE((reinterpret_cast<uintptr_t>(table_dev) & 7u) == 0, "prep_images_u8: the device table must be 8-byte aligned");
  ATTWARP_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15u) == 0, "prep_images_u8: out must be 16-byte aligned");
  ATTWARP_REQUIRE(h->tmp_bytes == 0 || tmp, "prep_images_u8: this batch needs %llu bytes of tmp", (unsigned long long)h->tmp_bytes);
  hipStream_t st = as_stream(stream);
  const uint8_t* td = static_cast<const uint8_t*>(table_dev);
  const PrepImageDev* images = reinterpret_cast<const PrepImageDev*>(td + h->off_images);
  const PrepItem* items = reinterpret_cast<const PrepItem*>(td + h->off_items);
  if (h->n_fused_items > 0)
    if (const int rc = h->C == 1 ? launch_fused<1>(h, images, items, out, st) : launch_fused<3>(h, images, items, out, st)) return rc;
  if (h->n_h_items > 0) {
    hipLaunchKernelGGL(prep_split_first_kernel, dim3(h->n_h_items), dim3(NT), 0, st, images, items + h->n_fused_items, h->C, h->S_w, tmp);
    if (const int rc = check_launch("prep_split_first_kernel")) return rc;
    hipLaunchKernelGGL(prep_split_second_kernel, dim3(h->n_v_items), dim3(NT), 0, st, images,
                       items + h->n_fused_items + h->n_h_items, h->C, h->S_h, h->S_w, tmp, out);
    if (const int rc = check_launch("prep_split_second_kernel")) return rc;
  }
  return ATTWARP_OK;
}

extern "C" int attwarp_pil_nearest_index(int n_in, int n_out, int32_t* idx) {
  ATTWARP_REQUIRE(idx, "pil_nearest_index: null pointer");
  ATTWARP_REQUIRE(n_in > 0 && n_out > 0, "pil_nearest_index: non-positive size");
  const double a = (double)n_in / (double)n_out;
  double xo = a * 0.5;
  for (int x = 0; x < n_out; ++x) {
    const int i = (int)floor(xo);
    idx[x] = i < n_in ? i : n_in - 1;
    xo += a;
  }
  return ATTWARP_OK;
}

extern "C" size_t attwarp_prep_attention_workspace_bytes(int B) {
  return B > 0 ? (size_t)B * ATT_CH * sizeof(float) : 0;
}

extern "C" int attwarp_prep_attention_f32(const attwarp_prep_attention* maps_dev, int B, int S_h, int S_w, void* ws, float* out,
                                          void* stream) {
  ATTWARP_REQUIRE(maps_dev && ws && out, "prep_attention_f32: null pointer");
  ATTWARP_REQUIRE(B > 0 && S_h > 0 && S_w > 0, "prep_attention_f32: non-positive size");
  ATTWARP_REQUIRE((reinterpret_cast<uintptr_t>(maps_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0 &&
                  (reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "prep_attention_f32: misaligned pointer");
  const long long nblk = (S_h + ATT_ROWS - 1) / ATT_ROWS;
  if (B > (1 << 20) || nblk * B > 0x7fffffffLL) return fail(ATTWARP_E_UNSUPPORTED, "prep_attention_f32: batch too large");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(prep_att_max_kernel, dim3((unsigned)B * ATT_CH), dim3(NT), 0, st, maps_dev, static_cast<float*>(ws));
  if (const int rc = check_launch("prep_att_max_kernel")) return rc;
  hipLaunchKernelGGL(prep_att_gather_kernel, dim3((unsigned)(nblk * B)), dim3(NT), 0, st, maps_dev, static_cast<const float*>(ws),
                     S_h, S_w, (int)nblk, out);
  return check_launch("prep_att_gather_kernel");
}
