// Pillow's 8-bit two-pass resampler (ImagingResampleHorizontal/Vertical_8bpc, Resample.c) as device arithmetic: 22-bit
// fixed-point coefficients, sum = 2^21 + sum(pixel * k), >> 22, clip to a byte, uint8 between the passes.  Every kernel
// that has to be bit-identical to Image.resize takes its pieces from here: the LANCZOS mask up-sampling (pil8.hip,
// mask_blocks.hpp), the CLIP preprocess (clip.hip, clip_ragged.hip), the trainer's data preparation (dataprep.hip) and,
// through the strip block, the two chains.  The coefficient tables come from attwarp_pil_coeffs_8bpc (pil8.hip).
#pragma once
#include "common.hpp"

namespace attwarp {

constexpr int PIL_PRECISION_BITS = 32 - 8 - 2;
constexpr int PIL_ROUND_HALF = 1 << (PIL_PRECISION_BITS - 1);      // what every sum starts from

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ uint8_t pil_clip8(int v) { return (uint8_t)min(max(v >> PIL_PRECISION_BITS, 0), 255); }
// four clip8 results packed into a dword: gfx950's v_ashr_pk_u8_i32 shifts, saturates to [0,255] and packs two
// values into the low 16 bits.  Used through the builtin with an explicit 16-bit mask: when the compiler forms the
// instruction by itself from `clip8(a) | clip8(b) << 8 | clip8(c) << 16 | ...` it omits that mask (ROCm 7.2) and the
// stale upper half of the destination register corrupts bytes 2 and 3.
__device__ __forceinline__ uint32_t pil_clip8x4(int s0, int s1, int s2, int s3) {
  const uint32_t lo = (uint32_t)(uint16_t)__builtin_amdgcn_ashr_pk_u8_i32(s0, s1, PIL_PRECISION_BITS);
  const uint32_t hi = (uint32_t)(uint16_t)__builtin_amdgcn_ashr_pk_u8_i32(s2, s3, PIL_PRECISION_BITS);
  return lo | (hi << 16);
}

// ToPILImage on a float tensor: pic.mul(255).byte()  (truncating cast)
__device__ __forceinline__ uint8_t to_pil_u8(float v) {
  const float s = fmul(v, 255.0f);
  return (uint8_t)min(max((int)truncf(s), 0), 255);
}

// ToTensor / the CLIP rescale of a byte: float32(float64(u8) * (1/255)) -- equal to the IEEE float32 division u8 / 255
// for all 256 values (u8 * float32(1/255) is not)
__device__ __forceinline__ float pil_u8_to_unit(int u8) { return (float)((double)u8 * (1.0 / 255.0)); }

// acc += pixel * coefficient with ONE full-rate instruction: pixels are 8 bit, Pillow's coefficients |k| <= 2^22, so the
// 24-bit multiply-add is exact (left to itself the compiler emits the quarter-rate v_mul_lo_u32 + an add, or pairs
// v_mul_i32_i24 with v_add3_u32: 1.5 instructions per tap)
__device__ __forceinline__ void mad24(int& acc, int px, int k) { asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(acc) : "v"(px), "v"(k)); }
// the same with a wave-uniform coefficient (an SGPR operand: no v_mov per tap)
__device__ __forceinline__ void mad24s(int& acc, int px, int k) { asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(acc) : "v"(px), "s"(k)); }

// One output byte from cnt taps `stride` bytes apart (a pass over memory, one thread per output).
__device__ __forceinline__ uint8_t pil_tap_sum(const uint8_t* p, size_t stride, const int32_t* k, int cnt) {
  int ss = PIL_ROUND_HALF;
  for (int i = 0; i < cnt; ++i) ss += (int)p[i * stride] * k[i];
  return pil_clip8(ss);
}
// Four neighbouring output bytes of a vertical pass, packed: one dword load per tap row (p 4-byte aligned, stride % 4 == 0).
__device__ __forceinline__ uint32_t pil_tap_sum4(const uint8_t* p, size_t stride, const int32_t* k, int cnt) {
  int s0 = PIL_ROUND_HALF, s1 = s0, s2 = s0, s3 = s0;
  for (int i = 0; i < cnt; ++i) {
    const uint32_t wv = *reinterpret_cast<const uint32_t*>(p + i * stride);
    const int kv = k[i];
    s0 += (int)(wv & 0xffu) * kv;
    s1 += (int)((wv >> 8) & 0xffu) * kv;
    s2 += (int)((wv >> 16) & 0xffu) * kv;
    s3 += (int)(wv >> 24) * kv;
  }
  return pil_clip8x4(s0, s1, s2, s3);
}

// One pixel of the horizontal pass on interleaved C-channel rows staged in LDS.  The KS taps x C channels of a pixel are
// KS*C CONSECUTIVE bytes of the source row starting at xmin*C: they are read as NA + 1 dwords from rw (the dword that
// holds byte xmin*C), shifted into place by sh = xmin*C & 3 with v_alignbyte_b32 and consumed with a static byte extract
// + one v_mad_i32_i24 each (byte reads made the LDS the bottleneck: 24 ds_read_u8 per pixel and row for RGB, 41 % of the
// LDS cycles bank conflicts -- profiles/round2_clip_pmc.txt).  Taps past the pixel's count carry a zero coefficient in
// kreg; the bytes they multiply may lie past the row (the next row, or the caller's slack behind the last one).
template <int C, int KS>
__device__ __forceinline__ void pil_h_window(const uint32_t* rw, int sh, const int (&kreg)[KS], uint8_t* op) {
  constexpr int NA = (KS * C + 3) / 4, NW = NA + 1;
  uint32_t wv[NW], a[NA];
#pragma unroll
  for (int i = 0; i < NW; ++i) wv[i] = rw[i];
#pragma unroll
  for (int i = 0; i < NA; ++i) a[i] = __builtin_amdgcn_alignbyte(wv[i + 1], wv[i], sh);
  int ss[C];
#pragma unroll
  for (int c = 0; c < C; ++c) ss[c] = PIL_ROUND_HALF;
#pragma unroll
  for (int x = 0; x < KS; ++x)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int j = x * C + c;
      mad24(ss[c], (int)((a[j >> 2] >> (8 * (j & 3))) & 0xffu), kreg[x]);
    }
#pragma unroll
  for (int c = 0; c < C; ++c) op[c] = pil_clip8(ss[c]);
}

}  // namespace attwarp
