// Device blocks shared by the training-loss kernels (losses.hip) and the target builders of profiles.hip: value
// clamps with torch's semantics, a double block scan, the pooled-CDF finalise of MN/losses.py:50-77 and the
// deterministic in-launch reduction of a loss to one scalar.  Every function is called by ALL threads of the workgroup.
#pragma once
#include "common.hpp"

namespace attwarp {

constexpr int LOSS_NT = 256;
constexpr int LOSS_MAX_N = 4096;        // row length of the row kernels (LDS: a few doubles per element)

// x.clamp_min(0) followed by nan_to_num(nan=0, posinf=0, neginf=0): NaN and +-inf count as 0
__device__ __forceinline__ float clamp_finite0(float v) { return (v > 0.0f && v <= 3.402823466e38f) ? v : 0.0f; }
// x.clamp_min(lo): NaN propagates (fmaxf would drop it)
__device__ __forceinline__ float clamp_min_nan(float v, float lo) { return (v != v) ? v : fmaxf(v, lo); }
// d clamp_min(x, lo) / dx as torch's autograd has it: 1 where x >= lo (ties pass), 0 elsewhere and at NaN
__device__ __forceinline__ bool clamp_passes(float v, float lo) { return v >= lo; }
__device__ __forceinline__ double sgn(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }   // torch.sign: 0 at 0

// torch's adaptive_avg_pool1d window k of n inputs -> L outputs: [floor(k n / L), ceil((k+1) n / L))
__device__ __forceinline__ void pool_window(int k, int n, int L, int& s, int& e) {
  s = (int)(((long long)k * n) / L);
  e = (int)((((long long)k + 1) * n + L - 1) / L);
}

// Inclusive prefix sum of x[0, n) in place (LDS doubles).  Each thread scans a contiguous chunk; the chunk totals are
// combined by a wave shuffle scan and the wave totals in `red` (NT/64 doubles).  The order is fixed: run-to-run identical.
__device__ void block_inclusive_scan(double* x, int n, double* red) {
  const int per = (n + (int)blockDim.x - 1) / (int)blockDim.x;
  const int k0 = threadIdx.x * per, k1 = min(k0 + per, n);
  double s = 0.0;
  for (int k = k0; k < k1; ++k) s += x[k];
  double inc = s;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const double t = __shfl_up(inc, o, WAVE);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == WAVE - 1) red[wid] = inc;
  __syncthreads();
  double c = inc - s;
  for (int w = 0; w < wid; ++w) c += red[w];
  for (int k = k0; k < k1; ++k) {
    c += x[k];
    x[k] = c;
  }
  __syncthreads();
}

// MN/losses.py:50-77 after the axis sums: m[0, n) (LDS doubles, already clamped / nan_to_num'd) -> normalise with
// clamp_min(1e-6) -> adaptive_avg_pool1d to L -> cumsum -> renormalise by clamp_min(last, 1e-6) -> last entry 1.
// c: LDS double[L], red: NT/64 doubles, out: float[L] (global).  Float64 throughout, one rounding at the store.
__device__ void pooled_cdf_block(const double* m, int n, int L, double* c, double* red, float* out) {
  double acc = 0.0;
  for (int k = threadIdx.x; k < n; k += blockDim.x) acc += m[k];
  const double den = fmax(block_sum(acc, red), 1e-6);
  for (int j = threadIdx.x; j < L; j += blockDim.x) {
    int s, e;
    pool_window(j, n, L, s, e);
    double w = 0.0;
    for (int i = s; i < e; ++i) w += m[i] / den;
    c[j] = w / (double)(e - s);
  }
  __syncthreads();
  block_inclusive_scan(c, L, red);
  const double last = fmax(c[L - 1], 1e-6);
  for (int j = threadIdx.x; j < L; j += blockDim.x) out[j] = (j == L - 1) ? 1.0f : (float)(c[j] / last);
}

// The last step of every loss forward: thread 0's `part` goes to parts[block], the workgroup that draws the last ticket
// sums parts[0, nparts) in index order (fixed tree, no float atomics: bitwise repeatable), stores the float32 loss and
// resets the ticket.  Publish / acquire at agent scope: the partials cross XCDs (their L2s are not coherent).
__device__ void finish_loss(double part, double* parts, uint32_t* ticket, int nparts, float* loss) {
  __shared__ double red[LOSS_NT / WAVE];
  __shared__ int last;
  if (threadIdx.x == 0) {
    parts[blockIdx.x + (size_t)blockIdx.y * gridDim.x] = part;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (t == (uint32_t)nparts - 1u);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) acc += parts[i];
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) {
    *loss = (float)tot;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace attwarp
