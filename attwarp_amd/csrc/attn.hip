// Attention-side stages on the 24x24 token grid:
//   A1  BatchMaskHookLogger._process_attention   AGW/attention_extraction/llava.py:385-396
//   A2  BatchMaskHookLogger.finalize_batch       llava.py:401-411
//   A3  revise_mask (normalize -> enhance -> box) llava.py:207-238
// (A4, ToPILImage + PIL resize(LANCZOS) of the mask, llava.py:192-196,243,253, is pil8.hip.)
//
// A1 is the only bandwidth-relevant one: per generation step it reads heads*ntok elements per
// sample (T*32*576*elemsize algorithmic bytes per image over a generation) with
// coalesced row segments; the rest is 576 numbers per image.
//
// Rounding follows the reference's dtype transitions: the hook works in the MODEL dtype
// (float16 in LLaVA), so every reference op boundary rounds to that dtype; reductions are
// accumulated in double and rounded once (see oracle/warp_oracle.py, module docstring).
#include "common.hpp"
#include "attn_f32v.hpp"
#include "mask_blocks.hpp"

namespace attwarp {

constexpr int NT = 256;
constexpr int MAXPL = 16;          // tokens per lane: ntok <= 1024
constexpr int MAX_NTOK = MAXPL * WAVE;

// attention rows are read exactly once per step: nontemporal loads keep them from displacing what the resample kernel
// of the same step left in (and needs from) the L2 / Infinity Cache -- in-step time of this kernel at B=256: 0.110 ->
// 0.074 ms (1024 x 1024 step), 0.112 -> 0.084 ms (336 x 336 step), stand-alone unchanged
template <typename T> __device__ __forceinline__ T nt_load(const T* p);
template <> __device__ __forceinline__ float nt_load<float>(const float* p) { return __builtin_nontemporal_load(p); }
template <> __device__ __forceinline__ __half nt_load<__half>(const __half* p) {
  return __builtin_bit_cast(__half, __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p)));
}
template <> __device__ __forceinline__ __hip_bfloat16 nt_load<__hip_bfloat16>(const __hip_bfloat16* p) {
  return __builtin_bit_cast(__hip_bfloat16, __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p)));
}

// One workgroup per (pseudo-)sample, any dtype / kv stride / slice length.  Each wave takes heads w, w+4, ...; lane l
// owns tokens l, l+64, ... (NPL = ceil(ntok/64) values per head in registers).  Heads are processed HU at a time so
// that HU*NPL independent coalesced loads are in flight per lane before the first reduction.  The float32 sums follow
// the path's fixed order (attn_f32v.hpp): with one token per lane the four tokens of a quad sit in four neighbouring
// lanes (two xor-shuffles give every lane (x0 + x1) + (x2 + x3)), register i' belongs to 256-token block i'/4 and to
// the lane group r = i' mod 4 of the canonical 64 lanes (canonical lane = 16 r + lane/4), so a lane keeps four running
// sums s_r; the butterfly's first two steps (o = 32, 16) combine the s_r, the last four are shuffles over lane/4.
// grid = nb
template <typename T, int NPL, int HU>
__global__ __launch_bounds__(NT) void attn_reduce_step_kernel(const T* __restrict__ attn, int heads, int64_t sb,
                                                              int64_t sh, int64_t row_off, int64_t skv,
                                                              const int32_t* __restrict__ starts, int starts_mod,
                                                              int max_start, int ntok, T* __restrict__ out) {
  __shared__ float part[NT / WAVE][NPL * WAVE];
  constexpr int NW = NT / WAVE;
  const int b = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  // a slice start outside [0, kv_len - ntok] is clamped for memory safety; the host shims reject such starts
  // (the reference would raise: a truncated slice cannot be stacked, llava.py:390-395)
  const int st = min(max(starts[b % starts_mod], 0), max_start);
  const T* base = attn + (int64_t)b * sb + row_off + (int64_t)st * skv;
  float acc[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) acc[i] = 0.0f;
  for (int h0 = wid; h0 < heads; h0 += NW * HU) {
    T v[HU][NPL];
#pragma unroll
    for (int u = 0; u < HU; ++u) {
      const int h = h0 + u * NW;
      const T* rp = base + (int64_t)min(h, heads - 1) * sh;      // clamped: tail heads re-read, not used
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const int t = lane + WAVE * i;
        v[u][i] = nt_load<T>(rp + (int64_t)min(t, ntok - 1) * skv);
      }
    }
#pragma unroll
    for (int u = 0; u < HU; ++u) {
      const int h = h0 + u * NW;
      if (h < heads) {                                            // wave uniform
        float sr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
          const float x = (lane + WAVE * i < ntok) ? to_f32<T>(v[u][i]) : 0.0f;
          const float pr = fadd(x, __shfl_xor(x, 1, WAVE));       // (x0 + x1) in lanes 0,1; (x2 + x3) in lanes 2,3
          const float q = fadd(pr, __shfl_xor(pr, 2, WAVE));      // (x0 + x1) + (x2 + x3) in all four
          sr[i & 3] = fadd(sr[i & 3], q);
        }
        float s = fadd(fadd(sr[0], sr[2]), fadd(sr[1], sr[3]));   // butterfly o = 32, then o = 16
        s = fadd(s, __shfl_xor(s, 32, WAVE));                     // o = 8, 4, 2, 1 over lane / 4
        s = fadd(s, __shfl_xor(s, 16, WAVE));
        s = fadd(s, __shfl_xor(s, 8, WAVE));
        s = fadd(s, __shfl_xor(s, 4, WAVE));
        const T den = add_tiny<T>(from_f32<T>(s));      // (row sum + 1e-12) in the model dtype
#pragma unroll
        for (int i = 0; i < NPL; ++i) acc[i] = fadd(acc[i], to_f32<T>(div_t<T>(v[u][i], den)));
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NPL; ++i) part[wid][lane + WAVE * i] = acc[i];
  __syncthreads();
  const T nheads = from_f32<T>((float)heads);
  for (int t = threadIdx.x; t < ntok; t += NT) {
    float m = 0.0f;
#pragma unroll
    for (int w = 0; w < NW; ++w) m = fadd(m, part[w][t]);
    out[(int64_t)b * ntok + t] = div_t<T>(from_f32<T>(m), nheads);    // mean = sum / N in dtype T
  }
}

// rows with unit kv stride and a slice length that is a multiple of 4: four tokens per lane (body: attn_f32v.hpp)
template <typename T, int NV, int HU>
__global__ __launch_bounds__(NT) void attn_reduce_step_v4_kernel(const AttnStepArgsT<T> a) {
  extern __shared__ __attribute__((aligned(16))) float attn_part[];
  attn_reduce_v4_block<T, NV, HU>(a, blockIdx.x, attn_part);
}

// mean over steps.  steps [Tn, n] -> out [n]
template <typename T>
__global__ __launch_bounds__(NT) void attn_finalize_kernel(const T* __restrict__ steps, int Tn, int64_t n,
                                                           T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  for (int t = 0; t < Tn; ++t) acc += (double)to_f32<T>(steps[(int64_t)t * n + i]);
  out[i] = div_t<T>(from_f64<T>(acc), from_f32<T>((float)Tn));
}

// ---- A3: one workgroup per mask (body: mask_blocks.hpp) ---------------------------------------
__global__ __launch_bounds__(NT) void mask_postproc_kernel(const float* __restrict__ mask, int n, int ks, float coe,
                                                           float* __restrict__ out) {
  __shared__ float x[32 * 32];
  __shared__ double red[NT / WAVE];
  __shared__ float fred[2][NT / WAVE];
  mask_postproc_block(mask, n, ks, coe, out, blockIdx.x, x, red, &fred[0][0]);
}


template <typename T>
static int launch_step(const void* attn, int nb, int heads, int64_t sb, int64_t sh, int64_t row_off, int64_t skv,
                       const int32_t* starts, int starts_mod, int max_start, int ntok, void* out, hipStream_t st) {
  // contiguous kv, slice length a multiple of 4 and <= 768: four tokens per lane (16-byte / 8-byte loads)
  if (skv == 1 && ntok % 4 == 0 && ntok >= 4 && ntok <= 3 * 4 * WAVE) {
    AttnStepArgsT<T> a;
    a.attn = (const T*)attn; a.heads = heads; a.sb = sb; a.sh = sh; a.row_off = row_off; a.starts = starts;
    a.starts_mod = starts_mod; a.max_start = max_start; a.ntok = ntok; a.out = (T*)out;
    const int hu = tune(TUNE_ATTN_HU);
    if (hu == 2)
      hipLaunchKernelGGL((attn_reduce_step_v4_kernel<T, 3, 2>), dim3(nb), dim3(NT), attn_v4_lds_bytes<3>(), st, a);
    else if (hu == 8)
      hipLaunchKernelGGL((attn_reduce_step_v4_kernel<T, 3, 8>), dim3(nb), dim3(NT), attn_v4_lds_bytes<3>(), st, a);
    else if (hu == 1)
      hipLaunchKernelGGL((attn_reduce_step_v4_kernel<T, 3, 1>), dim3(nb), dim3(NT), attn_v4_lds_bytes<3>(), st, a);
    else
      hipLaunchKernelGGL((attn_reduce_step_v4_kernel<T, 3, 4>), dim3(nb), dim3(NT), attn_v4_lds_bytes<3>(), st, a);
    return check_launch("attn_reduce_step_v4_kernel");
  }
  if (ntok <= 9 * WAVE)      // 576 image tokens (LLaVA-1.5): 9 per lane, 4 heads in flight
    hipLaunchKernelGGL((attn_reduce_step_kernel<T, 9, 4>), dim3(nb), dim3(NT), 0, st, (const T*)attn, heads, sb, sh,
                       row_off, skv, starts, starts_mod, max_start, ntok, (T*)out);
  else
    hipLaunchKernelGGL((attn_reduce_step_kernel<T, MAXPL, 2>), dim3(nb), dim3(NT), 0, st, (const T*)attn, heads, sb,
                       sh, row_off, skv, starts, starts_mod, max_start, ntok, (T*)out);
  return check_launch("attn_reduce_step_kernel");
}
template <typename T>
static int launch_finalize(const void* steps, int Tn, int64_t n, void* out, hipStream_t st) {
  hipLaunchKernelGGL((attn_finalize_kernel<T>), dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, (const T*)steps,
                     Tn, n, (T*)out);
  return check_launch("attn_finalize_kernel");
}

// dtype-dispatched A1 launch for other translation units (probe.hip chains into it)
int launch_attn_step_dtype(int dtype, const void* attn, int nb, int heads, int64_t sb, int64_t sh, int64_t row_off,
                           int64_t skv, const int32_t* starts, int starts_mod, int max_start, int ntok, void* out,
                           hipStream_t st) {
  switch (dtype) {
    case ATTWARP_F32: return launch_step<float>(attn, nb, heads, sb, sh, row_off, skv, starts, starts_mod, max_start, ntok, out, st);
    case ATTWARP_F16: return launch_step<__half>(attn, nb, heads, sb, sh, row_off, skv, starts, starts_mod, max_start, ntok, out, st);
    default: return launch_step<__hip_bfloat16>(attn, nb, heads, sb, sh, row_off, skv, starts, starts_mod, max_start, ntok, out, st);
  }
}

static int check_attn_dtype(int dtype, const char* who) {
  if (dtype == ATTWARP_F32 || dtype == ATTWARP_F16 || dtype == ATTWARP_BF16) return 0;
  return fail(ATTWARP_E_ARG, "%s: dtype must be F32, F16 or BF16 (got %d)", who, dtype);
}

}  // namespace attwarp

using namespace attwarp;

extern "C" int attwarp_attn_reduce_step(const void* attn, int dtype, int B, int heads, int q_len, int kv_len,
                                        int64_t stride_b, int64_t stride_h, int64_t stride_q, int64_t stride_kv,
                                        const int32_t* starts, int ntok, void* out, void* stream) {
  ATTWARP_REQUIRE(attn && starts && out, "attn_reduce_step: null pointer");
  ATTWARP_REQUIRE(B > 0 && heads > 0 && q_len > 0 && kv_len > 0 && ntok > 0, "attn_reduce_step: non-positive size");
  ATTWARP_REQUIRE(ntok <= kv_len, "attn_reduce_step: ntok=%d > kv_len=%d", ntok, kv_len);
  if (check_attn_dtype(dtype, "attn_reduce_step")) return ATTWARP_E_ARG;
  if (ntok > MAX_NTOK) return fail(ATTWARP_E_UNSUPPORTED, "attn_reduce_step: ntok=%d > %d", ntok, MAX_NTOK);
  const int64_t row_off = (int64_t)(q_len - 1) * stride_q;
  hipStream_t st = as_stream(stream);
  switch (dtype) {
    case ATTWARP_F32: return launch_step<float>(attn, B, heads, stride_b, stride_h, row_off, stride_kv, starts, B, kv_len - ntok, ntok, out, st);
    case ATTWARP_F16: return launch_step<__half>(attn, B, heads, stride_b, stride_h, row_off, stride_kv, starts, B, kv_len - ntok, ntok, out, st);
    default: return launch_step<__hip_bfloat16>(attn, B, heads, stride_b, stride_h, row_off, stride_kv, starts, B, kv_len - ntok, ntok, out, st);
  }
}

extern "C" int attwarp_attn_finalize(const void* steps, int dtype, int T, int B, int ntok, void* out, void* stream) {
  ATTWARP_REQUIRE(steps && out, "attn_finalize: null pointer");
  ATTWARP_REQUIRE(T > 0 && B > 0 && ntok > 0, "attn_finalize: non-positive size");
  if (check_attn_dtype(dtype, "attn_finalize")) return ATTWARP_E_ARG;
  const int64_t n = (int64_t)B * ntok;
  hipStream_t st = as_stream(stream);
  switch (dtype) {
    case ATTWARP_F32: return launch_finalize<float>(steps, T, n, out, st);
    case ATTWARP_F16: return launch_finalize<__half>(steps, T, n, out, st);
    default: return launch_finalize<__hip_bfloat16>(steps, T, n, out, st);
  }
}

extern "C" size_t attwarp_attn_reduce_stack_workspace_bytes(int dtype, int T, int B, int ntok) {
  if (T <= 0 || B <= 0 || ntok <= 0) return 0;
  return (size_t)T * B * ntok * (dtype == ATTWARP_F32 ? 4 : 2);
}

extern "C" int attwarp_attn_reduce_stack(const void* rows, int dtype, int T, int B, int heads, int kv_len,
                                         const int32_t* starts, int ntok, void* out, void* ws, void* stream) {
  ATTWARP_REQUIRE(rows && starts && out && ws, "attn_reduce_stack: null pointer");
  ATTWARP_REQUIRE(T > 0 && B > 0 && heads > 0 && kv_len > 0 && ntok > 0, "attn_reduce_stack: non-positive size");
  ATTWARP_REQUIRE(ntok <= kv_len, "attn_reduce_stack: ntok=%d > kv_len=%d", ntok, kv_len);
  if (check_attn_dtype(dtype, "attn_reduce_stack")) return ATTWARP_E_ARG;
  if (ntok > MAX_NTOK) return fail(ATTWARP_E_UNSUPPORTED, "attn_reduce_stack: ntok=%d > %d", ntok, MAX_NTOK);
  hipStream_t st = as_stream(stream);
  const int64_t sb = (int64_t)heads * kv_len, sh = kv_len;
  int rc;
  switch (dtype) {
    case ATTWARP_F32: rc = launch_step<float>(rows, T * B, heads, sb, sh, 0, 1, starts, B, kv_len - ntok, ntok, ws, st); break;
    case ATTWARP_F16: rc = launch_step<__half>(rows, T * B, heads, sb, sh, 0, 1, starts, B, kv_len - ntok, ntok, ws, st); break;
    default: rc = launch_step<__hip_bfloat16>(rows, T * B, heads, sb, sh, 0, 1, starts, B, kv_len - ntok, ntok, ws, st); break;
  }
  if (rc) return rc;
  return attwarp_attn_finalize(ws, dtype, T, B, ntok, out, stream);
}

extern "C" int attwarp_mask_postproc(const float* mask, int B, int n, int kernel_size, float enhance_coe, float* out,
                                     void* stream) {
  ATTWARP_REQUIRE(mask && out, "mask_postproc: null pointer");
  ATTWARP_REQUIRE(B > 0 && n > 0, "mask_postproc: non-positive size");
  ATTWARP_REQUIRE(kernel_size > 0 && (kernel_size & 1), "mask_postproc: kernel_size must be odd (got %d)", kernel_size);
  if (n > 32 || kernel_size > 7) return fail(ATTWARP_E_UNSUPPORTED, "mask_postproc: n <= 32 and kernel_size <= 7");
  hipLaunchKernelGGL(mask_postproc_kernel, dim3(B), dim3(NT), 0, as_stream(stream), mask, n, kernel_size, enhance_coe,
                     out);
  return check_launch("mask_postproc_kernel");
}
