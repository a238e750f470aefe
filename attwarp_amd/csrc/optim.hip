// The trainer's optimiser step (MN/trainer.py:259-264): GradScaler unscale, global gradient norm, clip and AdamW in two
// kernels (include/attwarp.h "the trainer's optimiser step").
//
//   adamw_norm_kernel   a workgroup owns one CHUNK of one tensor's gradient: x = g * inv_scale in float32, sum x^2 in
//                       float64, one partial per workgroup.  The workgroup that draws the last ticket of the STEP (over all
//                       launch groups) sums the partials in index order, stores grad_norm and the step record
//                       {inv_scale, coef, skip}, advances the step counts of the tensors present and writes their
//                       {lr / (1 - beta1^t), sqrt(1 - beta2^t)}; it resets the ticket (finish_loss's hand-off).
//   adamw_apply_kernel  reads the records (the kernel boundary is the hand-off), returns on skip, otherwise re-reads g and
//                       updates m, v, p.
//
// The tensor descriptors travel BY VALUE in the kernel arguments (gradient addresses change every step after
// zero_grad(set_to_none=True): a device table would cost an upload per step), at most GROUP per launch: 64 x 56 bytes
// (norm) and 64 x 48 bytes (apply) stay under the 4 KB of a kernarg segment.
#include "common.hpp"

namespace attwarp {
namespace {

constexpr int NT = 256;
#ifndef ATTWARP_ADAMW_CHUNK
#define ATTWARP_ADAMW_CHUNK 4096          // elements per workgroup: measured, DESIGN 3.11 (attwarp_amd/optim.py: CHUNK)
#endif
constexpr int CHUNK = ATTWARP_ADAMW_CHUNK;
constexpr int GROUP = 64;                 // descriptors per launch
constexpr int ROUNDS = CHUNK / (4 * NT);  // a thread takes 4 consecutive elements per round
static_assert(CHUNK % (4 * NT) == 0 && ROUNDS >= 1, "a chunk is a whole number of rounds of 4 elements per thread");

struct NormDesc {
  const float* g;
  int64_t numel;
  double lr, beta1, beta2;
  float decay, eps;                       // float32(1 - lr * wd), float32(eps)
  uint32_t first_chunk;                   // of this tensor inside the launch
  int32_t slot;
};
struct ApplyDesc {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t numel;
  uint32_t first_chunk;
  int32_t slot;
};
static_assert(sizeof(NormDesc) == 56 && sizeof(ApplyDesc) == 48, "descriptor blocks must fit the kernarg segment");

// workspace: [0,16) ticket, [16,32) StepRec, partials (double) upwards from 32, TensorRec of slot s at end - 64 (s + 1)
struct StepRec {
  float inv_scale, coef;
  uint32_t skip, pad;
};
struct TensorRec {
  double lr, beta1, beta2;                // written by the workgroup of the tensor's first chunk, with `present`
  float decay, eps;
  float step_size, bc2_sqrt;              // written by the finishing workgroup
  uint32_t present, pad[5];
};
static_assert(sizeof(StepRec) == 16 && sizeof(TensorRec) == 64, "workspace layout");
constexpr size_t WS_HEAD = 32;

struct NormArgs {
  NormDesc t[GROUP];
  int n;                                  // descriptors of this launch
  uint32_t part_base;                     // chunks of the launches before this one
  uint32_t total_parts;                   // chunks of the whole step
  int n_slots;                            // highest slot of the step + 1
  double max_norm, norm_eps;
};
struct ApplyArgs {
  ApplyDesc t[GROUP];
  int n;
};
// + the other arguments (at most 48 bytes) and the 256 bytes of hidden arguments the runtime appends
static_assert(sizeof(NormArgs) + 48 + 256 <= 4096 && sizeof(ApplyArgs) + 48 + 256 <= 4096, "kernarg segment");

template <typename D>
__device__ __forceinline__ int find_tensor(const D* t, int n, uint32_t c) {   // the last j with first_chunk <= c
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float inv_scale_of(const float* grad_scale) {
  return grad_scale ? (float)(1.0 / (double)*grad_scale) : 1.0f;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__global__ __launch_bounds__(NT) void adamw_norm_kernel(const NormArgs a, const float* grad_scale, const float* found_inf,
                                                        float* steps, float* grad_norm, unsigned char* ws,
                                                        unsigned char* ws_end) {
  __shared__ double red[NT / WAVE];
  __shared__ int last;
  const uint32_t c = blockIdx.x;
  const int j = find_tensor(a.t, a.n, c);
  const NormDesc d = a.t[j];
  const uint32_t k = c - d.first_chunk;
  const int64_t base = (int64_t)k * CHUNK;
  const int len = (int)min((int64_t)CHUNK, d.numel - base);
  const float* g = d.g + base;
  const float inv_scale = inv_scale_of(grad_scale);
  const bool vec = aligned16(d.g);

  // the element order of a thread and of the workgroup is the same on both routes: the partial does not depend on alignment
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int i = r * 4 * NT + 4 * (int)threadIdx.x;
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (vec && i + 3 < len) {
      const float4 q = *reinterpret_cast<const float4*>(g + i);
      x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < len) x[e] = g[i + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double s = (double)fmul(x[e], inv_scale);
      acc += s * s;
    }
  }
  const double part = block_sum(acc, red);

  double* parts = reinterpret_cast<double*>(ws + WS_HEAD);
  uint32_t* ticket = reinterpret_cast<uint32_t*>(ws);
  TensorRec* recs = reinterpret_cast<TensorRec*>(ws_end);      // record of slot s: recs[-(s + 1)]
  if (threadIdx.x == 0) {
    parts[a.part_base + c] = part;
    if (k == 0) {
      TensorRec* r = recs - (d.slot + 1);
      r->lr = d.lr; r->beta1 = d.beta1; r->beta2 = d.beta2;
      r->decay = d.decay; r->eps = d.eps;
      r->present = 1u;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (t == a.total_parts - 1u);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;

  // the finishing workgroup of the step: partials and records are read per thread (vector loads behind the acquire)
  double tot = 0.0;
  for (uint32_t i = threadIdx.x; i < a.total_parts; i += NT) tot += parts[i];
  tot = block_sum(tot, red);
  const double norm = sqrt(tot);
  double coef = 1.0;
  if (a.max_norm >= 0.0) {
    const double q = a.max_norm / (norm + a.norm_eps);
    coef = (q < 1.0 || q != q) ? q : 1.0;                      // torch.clamp(max=1): NaN stays NaN
  }
  const bool skip = found_inf && *found_inf != 0.0f;
  for (int s = threadIdx.x; s < a.n_slots; s += NT) {
    TensorRec* r = recs - (s + 1);
    if (!r->present) continue;
    r->present = 0u;
    if (skip) continue;
    const float t = fadd(steps[s], 1.0f);
    steps[s] = t;
    r->step_size = (float)(r->lr / (1.0 - pow(r->beta1, (double)t)));
    r->bc2_sqrt = (float)sqrt(1.0 - pow(r->beta2, (double)t));
  }
  if (threadIdx.x == 0) {
    *grad_norm = (float)norm;
    StepRec* sr = reinterpret_cast<StepRec*>(ws + 16);
    sr->inv_scale = inv_scale;
    sr->coef = (float)coef;
    sr->skip = skip ? 1u : 0u;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct Coefs {
  float inv_scale, coef, decay, w1, b2, w2, eps, step_size, bc2_sqrt;
};

// The moment update is torch.lerp(m, g, w1) as torch.optim.AdamW takes it: m + w1 (g - m) below a weight of 0.5 and
// g - (g - m)(1 - w1) from there on (beta1 <= 0.5), where the first form would leave a rounding of size ulp(m) in a result
// of size |g| (beta1 = 0 must give exactly g).  1 - w1 is taken in float32.
__device__ __forceinline__ void adamw_element(const Coefs& c, float graw, float& p, float& m, float& v) {
  const float g = fmul(fmul(graw, c.inv_scale), c.coef);
  p = fmul(p, c.decay);
  const float d = fsub(g, m);
  m = (c.w1 < 0.5f) ? fadd(m, fmul(c.w1, d)) : fsub(g, fmul(d, fsub(1.0f, c.w1)));
  v = fadd(fmul(v, c.b2), fmul(fmul(c.w2, g), g));
  const float denom = fadd(sqrtf(v) / c.bc2_sqrt, c.eps);
  p = fsub(p, fmul(c.step_size, m / denom));
}

__global__ __launch_bounds__(NT) void adamw_apply_kernel(const ApplyArgs a, const unsigned char* ws,
                                                         const unsigned char* ws_end) {
  const StepRec sr = *reinterpret_cast<const StepRec*>(ws + 16);
  if (sr.skip) return;
  const uint32_t c = blockIdx.x;
  const int j = find_tensor(a.t, a.n, c);
  const ApplyDesc d = a.t[j];
  const TensorRec* r = reinterpret_cast<const TensorRec*>(ws_end) - (d.slot + 1);
  Coefs cf;
  cf.inv_scale = sr.inv_scale; cf.coef = sr.coef;
  cf.decay = r->decay; cf.eps = r->eps;
  cf.w1 = (float)(1.0 - r->beta1); cf.b2 = (float)r->beta2; cf.w2 = (float)(1.0 - r->beta2);
  cf.step_size = r->step_size; cf.bc2_sqrt = r->bc2_sqrt;

  const int64_t base = (int64_t)(c - d.first_chunk) * CHUNK;
  const int len = (int)min((int64_t)CHUNK, d.numel - base);
  float* p = d.p + base;
  const float* g = d.g + base;
  float* m = d.m + base;
  float* v = d.v + base;
  const bool vec = aligned16(d.p) && aligned16(d.g) && aligned16(d.m) && aligned16(d.v);
#pragma unroll
  for (int rr = 0; rr < ROUNDS; ++rr) {
    const int i = rr * 4 * NT + 4 * (int)threadIdx.x;
    if (vec && i + 3 < len) {
      const float4 gq = *reinterpret_cast<const float4*>(g + i);
      float4 pq = *reinterpret_cast<float4*>(p + i), mq = *reinterpret_cast<float4*>(m + i),
             vq = *reinterpret_cast<float4*>(v + i);
      adamw_element(cf, gq.x, pq.x, mq.x, vq.x);
      adamw_element(cf, gq.y, pq.y, mq.y, vq.y);
      adamw_element(cf, gq.z, pq.z, mq.z, vq.z);
      adamw_element(cf, gq.w, pq.w, mq.w, vq.w);
      *reinterpret_cast<float4*>(p + i) = pq;
      *reinterpret_cast<float4*>(m + i) = mq;
      *reinterpret_cast<float4*>(v + i) = vq;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < len) {
          float pe = p[i + e], me = m[i + e], ve = v[i + e];
          adamw_element(cf, g[i + e], pe, me, ve);
          p[i + e] = pe; m[i + e] = me; v[i + e] = ve;
        }
    }
  }
}

inline int64_t chunks_of(int64_t numel) { return (numel + CHUNK - 1) / CHUNK; }

}  // namespace
}  // namespace attwarp

using namespace attwarp;

extern "C" size_t attwarp_adamw_workspace_bytes(int64_t total_numel, int n_tensors) {
  if (total_numel < 0 || n_tensors < 0) return 0;
  // a tensor's last chunk may be partial: at most total_numel / CHUNK + n_tensors chunks
  const size_t parts = (size_t)(total_numel / CHUNK) + (size_t)n_tensors;
  return WS_HEAD + parts * sizeof(double) + (size_t)n_tensors * sizeof(TensorRec);
}

extern "C" int attwarp_adamw_step(const attwarp_adamw_tensor* tensors, int n, double max_norm, double norm_eps,
                                  const float* grad_scale, const float* found_inf, float* steps, float* grad_norm,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  ATTWARP_REQUIRE(tensors && steps && grad_norm && workspace, "adamw_step: null pointer");
  ATTWARP_REQUIRE(n > 0, "adamw_step: no tensors");
  ATTWARP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0 && workspace_bytes % 8 == 0,
                  "adamw_step: the workspace must be 16-byte aligned and a multiple of 8 bytes");
  ATTWARP_REQUIRE(norm_eps == norm_eps && max_norm == max_norm, "adamw_step: NaN max_norm or norm_eps");
  int64_t total_chunks = 0;
  int n_slots = 0;
  for (int i = 0; i < n; ++i) {
    const attwarp_adamw_tensor& t = tensors[i];
    ATTWARP_REQUIRE(t.p && t.g && t.m && t.v, "adamw_step: tensor %d: null pointer", i);
    ATTWARP_REQUIRE(((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                      reinterpret_cast<uintptr_t>(t.v)) & 3u) == 0, "adamw_step: tensor %d: pointer not 4-byte aligned", i);
    ATTWARP_REQUIRE(t.numel > 0, "adamw_step: tensor %d: non-positive numel", i);
    ATTWARP_REQUIRE(t.step_slot >= 0, "adamw_step: tensor %d: negative step_slot", i);
    ATTWARP_REQUIRE(t.beta1 >= 0.0 && t.beta1 < 1.0 && t.beta2 >= 0.0 && t.beta2 < 1.0, "adamw_step: tensor %d: betas outside [0, 1)", i);
    total_chunks += chunks_of(t.numel);
    if (t.step_slot + 1 > n_slots) n_slots = t.step_slot + 1;
  }
  if (total_chunks > 0x7fffffffLL) return fail(ATTWARP_E_UNSUPPORTED, "adamw_step: %lld chunks (> 2^31 - 1)", (long long)total_chunks);
  const size_t need = WS_HEAD + (size_t)total_chunks * sizeof(double) + (size_t)n_slots * sizeof(TensorRec);
  ATTWARP_REQUIRE(workspace_bytes >= need, "adamw_step: workspace of %zu bytes, %zu needed (%lld chunks, %d step slots)",
                  workspace_bytes, need, (long long)total_chunks, n_slots);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  unsigned char* ws_end = ws + workspace_bytes;
  hipStream_t st = as_stream(stream);

  uint32_t part_base = 0;
  for (int i0 = 0; i0 < n; i0 += GROUP) {
    NormArgs a;
    a.n = (n - i0 < GROUP) ? n - i0 : GROUP;
    uint32_t chunks = 0;
    for (int i = 0; i < GROUP; ++i) {
      const attwarp_adamw_tensor& t = tensors[i0 + (i < a.n ? i : a.n - 1)];     // unused entries repeat the last one
      a.t[i] = NormDesc{t.g, t.numel, t.lr, t.beta1, t.beta2, (float)(1.0 - t.lr * t.weight_decay), (float)t.eps,
                        chunks, t.step_slot};
      if (i < a.n) chunks += (uint32_t)chunks_of(t.numel);
    }
    a.part_base = part_base;
    a.total_parts = (uint32_t)total_chunks;
    a.n_slots = n_slots;
    a.max_norm = max_norm;
    a.norm_eps = norm_eps;
    hipLaunchKernelGGL(adamw_norm_kernel, dim3(chunks), dim3(NT), 0, st, a, grad_scale, found_inf, steps, grad_norm, ws, ws_end);
    if (int rc = check_launch("adamw_norm_kernel")) return rc;
    part_base += chunks;
  }
  for (int i0 = 0; i0 < n; i0 += GROUP) {
    ApplyArgs a;
    a.n = (n - i0 < GROUP) ? n - i0 : GROUP;
    uint32_t chunks = 0;
    for (int i = 0; i < GROUP; ++i) {
      const attwarp_adamw_tensor& t = tensors[i0 + (i < a.n ? i : a.n - 1)];
      a.t[i] = ApplyDesc{t.p, t.g, t.m, t.v, t.numel, chunks, t.step_slot};
      if (i < a.n) chunks += (uint32_t)chunks_of(t.numel);
    }
    hipLaunchKernelGGL(adamw_apply_kernel, dim3(chunks), dim3(NT), 0, st, a, ws, ws_end);
    if (int rc = check_launch("adamw_apply_kernel")) return rc;
  }
  return ATTWARP_OK;
}
