// L: the MarginalNet training losses (MN/losses.py:11-77, MN/model.py:98-106) and the trainer's image-resolution PDF
// loss (MN/trainer.py:216-250), forward and backward.  One 256-thread workgroup per sample (or per (sample, axis)),
// the row in LDS, float64 sums; a forward ends in finish_loss (loss_blocks.hpp), a backward recomputes what it needs
// and writes the gradient rows.  Tie conventions (DESIGN.md "training losses"): clamp_min passes the gradient where
// the input >= the bound, |d| has gradient 0 at d == 0, nan_to_num has gradient 0 at non-finite inputs, a normaliser
// clamped to its floor is a constant, the CDF entry overwritten with 1.0 has gradient 0.
#include "axis_blocks.hpp"
#include "loss_blocks.hpp"

namespace attwarp {

namespace {

constexpr int NT = LOSS_NT;
// static LDS next to the dynamic rows (kernel-resource-usage: 32 bytes for a kernel's `red`, 80 with finish_loss's
// `red` and `last`), counted where a launcher's dynamic LDS can reach a limit
constexpr size_t RED_LDS = (NT / WAVE) * sizeof(double), FINISH_LDS = 48;

// ---- cdf_from_density_downsample (MN/losses.py:70-77).  grid = B ----------------------------------------------------
__global__ __launch_bounds__(NT) void cdf_downsample_kernel(const float* __restrict__ p, int N, int L, float* __restrict__ F) {
  extern __shared__ __attribute__((aligned(16))) double smem_d[];     // N + L doubles
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x;
  double* m = smem_d;
  for (int k = threadIdx.x; k < N; k += blockDim.x) m[k] = (double)clamp_finite0(p[(size_t)b * N + k]);
  __syncthreads();
  pooled_cdf_block(m, N, L, smem_d + N, red, F + (size_t)b * L);
}

// ---- cdf_from_density (checkpoint_utils.py:30-41) of one row in float64: F[k] = cumsum(a / max(sum a, 1e-6)),
// a = clamp_finite0(p); F[N-1] is NOT overwritten here (the callers treat it).  Returns sum a; den = the normaliser.
__device__ double row_cdf(const float* p, int N, double* F, double* red, double& den) {
  double acc = 0.0;
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    const double a = (double)clamp_finite0(p[k]);
    F[k] = a;
    acc += a;
  }
  const double s = block_sum(acc, red);
  den = fmax(s, 1e-6);
  for (int k = threadIdx.x; k < N; k += blockDim.x) F[k] = F[k] / den;
  __syncthreads();
  block_inclusive_scan(F, N, red);
  return s;
}

// ---- l1_cdf_loss (MN/losses.py:11-12): mean |cdf(p) - cdf(q)| over B x N.  grid = B -------------------------------
__global__ __launch_bounds__(NT) void l1_cdf_kernel(const float* __restrict__ p, const float* __restrict__ q, int B, int N,
                                                    double* parts, uint32_t* ticket, float* loss) {
  extern __shared__ __attribute__((aligned(16))) double smem_d[];     // 2N doubles
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x;
  double dp, dq;
  double* Fp = smem_d;
  double* Fq = smem_d + N;
  row_cdf(p + (size_t)b * N, N, Fp, red, dp);
  row_cdf(q + (size_t)b * N, N, Fq, red, dq);
  double acc = 0.0;
  for (int k = threadIdx.x; k < N - 1; k += blockDim.x) acc += fabs(Fp[k] - Fq[k]);   // the last entries are both 1.0
  const double part = block_sum(acc, red) / ((double)B * N);
  finish_loss(part, parts, ticket, B, loss);
}

// d loss / d p of one row: r = dL/dF (LDS, overwritten), the CDF was cumsum(a / den) with a = clamp_finite0(p), s = sum a.
// dL/d(a/den)_j = sum_{k >= j} r_k; the normaliser passes when s >= 1e-6; nan_to_num and clamp_min(0) pass where
// 0 <= p < inf.
__device__ void row_cdf_backward(const float* p, int N, double* r, double s, double den, double* red, float* g) {
  block_inclusive_scan(r, N, red);                                 // r[j] = sum_{k <= j} r_k
  const double tot = r[N - 1];
  __syncthreads();
  double acc = 0.0;
  for (int j = threadIdx.x; j < N; j += blockDim.x) acc += (tot - (j ? r[j - 1] : 0.0)) * (double)clamp_finite0(p[j]);
  const double dot = block_sum(acc, red);                          // sum_j dr_j a_j
  const double corr = (s >= 1e-6) ? dot / (den * den) : 0.0;
  for (int j = threadIdx.x; j < N; j += blockDim.x) {
    const float v = p[j];
    const double dr = tot - (j ? r[j - 1] : 0.0);
    g[j] = (v >= 0.0f && v <= 3.402823466e38f) ? (float)(dr / den - corr) : 0.0f;
  }
  __syncthreads();
}

__global__ __launch_bounds__(NT) void l1_cdf_backward_kernel(const float* __restrict__ p, const float* __restrict__ q, int B,
                                                             int N, const float* __restrict__ gout, float* __restrict__ gp,
                                                             float* __restrict__ gq) {
  extern __shared__ __attribute__((aligned(16))) double smem_d[];     // 3N doubles
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x;
  const float* pb = p + (size_t)b * N;
  const float* qb = q + (size_t)b * N;
  double dp, dq;
  double* Fp = smem_d;
  double* Fq = smem_d + N;
  double* r = smem_d + 2 * N;
  const double sp = row_cdf(pb, N, Fp, red, dp);
  const double sq = row_cdf(qb, N, Fq, red, dq);
  const double c = (double)gout[0] / ((double)B * N);
  for (int k = threadIdx.x; k < N; k += blockDim.x) r[k] = (k == N - 1) ? 0.0 : c * sgn(Fp[k] - Fq[k]);
  __syncthreads();
  row_cdf_backward(pb, N, r, sp, dp, red, gp + (size_t)b * N);
  for (int k = threadIdx.x; k < N; k += blockDim.x) r[k] = (k == N - 1) ? 0.0 : -c * sgn(Fp[k] - Fq[k]);
  __syncthreads();
  row_cdf_backward(qb, N, r, sq, dq, red, gq + (size_t)b * N);
}

// ---- sym_kl (MN/losses.py:15-22): 0.5 (KL(P||Q) + KL(Q||P)) = 0.5/B sum (P - Q)(log P - log Q),
// P = clamp_min(p, eps) / sum, Q likewise (the sums are not clamped).  grid = B ----------------------------------------
__device__ double row_clamped_sum(const float* p, int N, float eps, double* red) {
  double acc = 0.0;
  for (int k = threadIdx.x; k < N; k += blockDim.x) acc += (double)clamp_min_nan(p[k], eps);
  return block_sum(acc, red);
}

__global__ __launch_bounds__(NT) void sym_kl_kernel(const float* __restrict__ p, const float* __restrict__ q, int B, int N,
                                                    float eps, double* parts, uint32_t* ticket, float* loss) {
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x;
  const float* pb = p + (size_t)b * N;
  const float* qb = q + (size_t)b * N;
  const double Sp = row_clamped_sum(pb, N, eps, red), Sq = row_clamped_sum(qb, N, eps, red);
  double acc = 0.0;
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    const double P = (double)clamp_min_nan(pb[k], eps) / Sp, Q = (double)clamp_min_nan(qb[k], eps) / Sq;
    acc += (P - Q) * (log(P) - log(Q));
  }
  const double part = 0.5 * block_sum(acc, red) / (double)B;
  finish_loss(part, parts, ticket, B, loss);
}

__global__ __launch_bounds__(NT) void sym_kl_backward_kernel(const float* __restrict__ p, const float* __restrict__ q, int B,
                                                             int N, float eps, const float* __restrict__ gout,
                                                             float* __restrict__ gp, float* __restrict__ gq) {
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x;
  const float* pb = p + (size_t)b * N;
  const float* qb = q + (size_t)b * N;
  const double Sp = row_clamped_sum(pb, N, eps, red), Sq = row_clamped_sum(qb, N, eps, red);
  const double c = 0.5 * (double)gout[0] / (double)B;
  // dL/dP_i = c (log P_i - log Q_i + (P_i - Q_i) / P_i); through P = p'/Sp: dp'_j = (dP_j - sum_i dP_i P_i) / Sp
  double ap = 0.0, aq = 0.0;
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    const double P = (double)clamp_min_nan(pb[k], eps) / Sp, Q = (double)clamp_min_nan(qb[k], eps) / Sq;
    const double l = log(P) - log(Q);
    ap += c * (l + (P - Q) / P) * P;
    aq += c * (-l + (Q - P) / Q) * Q;
  }
  const double dotp = block_sum(ap, red), dotq = block_sum(aq, red);
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    const float vp = pb[k], vq = qb[k];
    const double P = (double)clamp_min_nan(vp, eps) / Sp, Q = (double)clamp_min_nan(vq, eps) / Sq;
    const double l = log(P) - log(Q);
    const double dP = c * (l + (P - Q) / P), dQ = c * (-l + (Q - P) / Q);
    gp[(size_t)b * N + k] = clamp_passes(vp, eps) ? (float)((dP - dotp) / Sp) : 0.0f;
    gq[(size_t)b * N + k] = clamp_passes(vq, eps) ? (float)((dQ - dotq) / Sq) : 0.0f;
  }
}

// ---- separable_recon_loss (MSE) and recon_l1 (MN/losses.py:25-47).  grid = B --------------------------------------
// P = py px^T / Dp, Dp = max(Sx Sy, 1e-6); Ahat = A+ / Da, A+ = clamp_min(A, 0) (NaN propagates), Da = max(sum A+, 1e-6).
// MSE: sum (P - Ahat)^2 = Qx Qy / Dp^2 - 2 py^T A+ px / (Dp Da) + sum (A+)^2 / Da^2: one pass over A.
// L1: sum A+ first, then sum |P - Ahat|: two passes.  The outer product is never stored.
struct ReconRow {
  double Sx, Sy, Qx, Qy, Dp, Da, sa;
};

__device__ ReconRow recon_row_sums(const float* px, const float* py, const float* A, int H, int W, bool mse, double* red,
                                   double& sa2, double& bil) {
  ReconRow r;
  double sx = 0.0, qx = 0.0, sy = 0.0, qy = 0.0;
  for (int k = threadIdx.x; k < W; k += blockDim.x) { const double v = px[k]; sx += v; qx += v * v; }
  for (int k = threadIdx.x; k < H; k += blockDim.x) { const double v = py[k]; sy += v; qy += v * v; }
  r.Sx = block_sum(sx, red); r.Qx = block_sum(qx, red); r.Sy = block_sum(sy, red); r.Qy = block_sum(qy, red);
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  const int HW = H * W;
  for (int i = threadIdx.x; i < HW; i += blockDim.x) {
    const double a = (double)clamp_min_nan(A[i], 0.0f);
    s1 += a;
    if (mse) {
      const int h = i / W, w = i - h * W;
      s2 += a * a;
      s3 += (double)py[h] * a * (double)px[w];
    }
  }
  r.sa = block_sum(s1, red);
  sa2 = mse ? block_sum(s2, red) : 0.0;
  bil = mse ? block_sum(s3, red) : 0.0;
  r.Dp = fmax(r.Sx * r.Sy, 1e-6);
  r.Da = fmax(r.sa, 1e-6);
  return r;
}

__global__ __launch_bounds__(NT) void recon_kernel(const float* __restrict__ px, const float* __restrict__ py,
                                                   const float* __restrict__ A, int B, int H, int W, int kind,
                                                   double* parts, uint32_t* ticket, float* loss) {
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x;
  const float* xb = px + (size_t)b * W;
  const float* yb = py + (size_t)b * H;
  const float* Ab = A + (size_t)b * H * W;
  const bool mse = (kind == ATTWARP_RECON_MSE);
  double sa2, bil;
  const ReconRow r = recon_row_sums(xb, yb, Ab, H, W, mse, red, sa2, bil);
  double tot;
  if (mse) {
    tot = r.Qx * r.Qy / (r.Dp * r.Dp) - 2.0 * bil / (r.Dp * r.Da) + sa2 / (r.Da * r.Da);
  } else {
    double acc = 0.0;
    const int HW = H * W;
    for (int i = threadIdx.x; i < HW; i += blockDim.x) {
      const int h = i / W, w = i - h * W;
      acc += fabs((double)yb[h] * (double)xb[w] / r.Dp - (double)clamp_min_nan(Ab[i], 0.0f) / r.Da);
    }
    tot = block_sum(acc, red);
  }
  finish_loss(tot / ((double)B * H * W), parts, ticket, B, loss);
}

// e(h, w): A+ (MSE) or sign(P - Ahat) (L1).  Row dots u_h = sum_w e px_w (a wave per row), column dots
// v_w = sum_h e py_h (a thread per column), then
//  MSE: dpx_w = 2c (px_w Qy / Dp^2 - m Sy Qx Qy / Dp^3 - v_w / (Dp Da) + m Sy (py.u) / (Dp^2 Da))
//  L1:  dpx_w = c (v_w / Dp - m Sy (py.u) / Dp^2)
// (py symmetric), c = gout / (B H W), m = [Sx Sy >= 1e-6].  LDS: u [H] doubles.
__global__ __launch_bounds__(NT) void recon_backward_kernel(const float* __restrict__ px, const float* __restrict__ py,
                                                            const float* __restrict__ A, int B, int H, int W, int kind,
                                                            const float* __restrict__ gout, float* __restrict__ gpx,
                                                            float* __restrict__ gpy) {
  extern __shared__ __attribute__((aligned(16))) double smem_d[];     // H doubles
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x;
  const float* xb = px + (size_t)b * W;
  const float* yb = py + (size_t)b * H;
  const float* Ab = A + (size_t)b * H * W;
  const bool mse = (kind == ATTWARP_RECON_MSE);
  double sa2, bil;
  const ReconRow r = recon_row_sums(xb, yb, Ab, H, W, false, red, sa2, bil);
  auto e = [&](int h, int w) -> double {
    const double a = (double)clamp_min_nan(Ab[(size_t)h * W + w], 0.0f);
    if (mse) return a;
    return sgn((double)yb[h] * (double)xb[w] / r.Dp - a / r.Da);
  };
  double* u = smem_d;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
  for (int h = wid; h < H; h += nw) {
    double acc = 0.0;
    for (int w = lane; w < W; w += WAVE) acc += e(h, w) * (double)xb[w];
    acc = wave_sum(acc);
    if (lane == 0) u[h] = acc;
  }
  __syncthreads();
  double a = 0.0;
  for (int h = threadIdx.x; h < H; h += blockDim.x) a += (double)yb[h] * u[h];
  const double yu = block_sum(a, red);                              // py^T E px
  const double c = (double)gout[0] / ((double)B * H * W);
  const bool m = r.Sx * r.Sy >= 1e-6;
  const double Dp = r.Dp, Da = r.Da;
  for (int w = threadIdx.x; w < W; w += blockDim.x) {
    double v = 0.0;
    for (int h = 0; h < H; ++h) v += e(h, w) * (double)yb[h];
    double g;
    if (mse)
      g = 2.0 * c * ((double)xb[w] * r.Qy / (Dp * Dp) - (m ? r.Sy * r.Qx * r.Qy / (Dp * Dp * Dp) : 0.0) - v / (Dp * Da) +
                     (m ? r.Sy * yu / (Dp * Dp * Da) : 0.0));
    else
      g = c * (v / Dp - (m ? r.Sy * yu / (Dp * Dp) : 0.0));
    gpx[(size_t)b * W + w] = (float)g;
  }
  for (int h = threadIdx.x; h < H; h += blockDim.x) {
    double g;
    if (mse)
      g = 2.0 * c * ((double)yb[h] * r.Qx / (Dp * Dp) - (m ? r.Sx * r.Qx * r.Qy / (Dp * Dp * Dp) : 0.0) - u[h] / (Dp * Da) +
                     (m ? r.Sx * yu / (Dp * Dp * Da) : 0.0));
    else
      g = c * (u[h] / Dp - (m ? r.Sx * yu / (Dp * Dp) : 0.0));
    gpy[(size_t)b * H + h] = (float)g;
  }
}

// ---- mix_with_uniform (model.py:98-101) and its backward: out = c1 * p + c2, float32, two roundings --------------
__global__ __launch_bounds__(NT) void scale_shift_kernel(const float* __restrict__ p, int64_t n, float c1, float c2,
                                                         float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = fadd(fmul(c1, p[i]), c2);
}

// ---- entropy (model.py:104-106): -(1/B) sum q log q, q = clamp_min(p, eps).  grid = B -------------------------------
__global__ __launch_bounds__(NT) void entropy_kernel(const float* __restrict__ p, int B, int N, float eps, double* parts,
                                                     uint32_t* ticket, float* loss) {
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x;
  double acc = 0.0;
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    const double q = (double)clamp_min_nan(p[(size_t)b * N + k], eps);
    acc += q * log(q);
  }
  finish_loss(-block_sum(acc, red) / (double)B, parts, ticket, B, loss);
}

__global__ __launch_bounds__(NT) void entropy_backward_kernel(const float* __restrict__ p, int B, int N, float eps,
                                                              const float* __restrict__ gout, float* __restrict__ gp) {
  const size_t n = (size_t)B * N;
  const double c = -(double)gout[0] / (double)B;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = p[i];
    gp[i] = clamp_passes(v, eps) ? (float)(c * (log((double)v) + 1.0)) : 0.0f;
  }
}

// ---- the trainer's image-resolution PDF loss (MN/trainer.py:216-250).  grid = (B, 2 axes) --------------------------
// u = right_inverse(pred) (pre-clamp, LDS), t = right_inverse(gt).clamp_min(0) (LDS), both renormalised with
// clamp_min(1e-6); the block's partial is sum |u+/Du - t/Dt| / (B L).
struct PdfL1Args {
  const float *px, *py, *gx, *gy;
  int B, Lx, Ly, W, H;
  const double *inv_x, *inv_y;
};
constexpr size_t pdf_l1_lds_bytes(int L) { return (size_t)2 * L * sizeof(float) + 64 * sizeof(float) + 64 * sizeof(double); }

struct PdfRow {
  int Lo, L;
  const double* inv;
  double su, st, Du, Dt;
};

__device__ PdfRow pdf_row(const PdfL1Args& a, int b, int axis, float* u, float* t, float* tmp, double* red) {
  PdfRow r;
  r.Lo = axis ? a.Ly : a.Lx;
  r.L = axis ? a.H : a.W;
  r.inv = axis ? a.inv_y : a.inv_x;
  const float* pred = (axis ? a.py : a.px) + (size_t)b * r.Lo;
  const float* gt = (axis ? a.gy : a.gx) + (size_t)b * r.Lo;
  right_inverse_block(pred, r.Lo, r.L, r.inv, tmp, u, false);
  right_inverse_block(gt, r.Lo, r.L, r.inv, tmp, t, true);
  double s1 = 0.0, s2 = 0.0;
  for (int l = threadIdx.x; l < r.L; l += blockDim.x) {
    s1 += (double)clamp_min_nan(u[l], 0.0f);
    s2 += (double)t[l];
  }
  r.su = block_sum(s1, red);
  r.st = block_sum(s2, red);
  r.Du = fmax(r.su, 1e-6);
  r.Dt = fmax(r.st, 1e-6);
  return r;
}

__global__ __launch_bounds__(NT) void pdf_l1_kernel(const PdfL1Args a, double* parts, uint32_t* ticket, float* loss) {
  extern __shared__ __attribute__((aligned(16))) double smem_d[];     // pdf_l1_lds_bytes(max(W, H))
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x, axis = blockIdx.y;
  const int Lmax = max(a.W, a.H);
  float* u = reinterpret_cast<float*>(smem_d + 64);
  float* t = u + Lmax;
  float* tmp = t + Lmax;
  const PdfRow r = pdf_row(a, b, axis, u, t, tmp, red);
  double acc = 0.0;
  for (int l = threadIdx.x; l < r.L; l += blockDim.x)
    acc += fabs((double)clamp_min_nan(u[l], 0.0f) / r.Du - (double)t[l] / r.Dt);
  finish_loss(block_sum(acc, red) / ((double)a.B * r.L), parts, ticket, 2 * a.B, loss);
}

// Backward: d = c sign(u+/Du - t/Dt) (c = gout / (B L)); du_l = d_l / Du - m (sum_k d_k u+_k) / Du^2 (m = [su >= 1e-6]);
// clamp_min(0) passes where u_l >= 0; then the adjoint of the right inverse (_RightInverse.backward in
// checkpoint_utils.py): adaptive_avg_pool1d to Lo, times the symmetric inverse.
__global__ __launch_bounds__(NT) void pdf_l1_backward_kernel(const PdfL1Args a, const float* __restrict__ gout,
                                                             float* __restrict__ gpx, float* __restrict__ gpy) {
  extern __shared__ __attribute__((aligned(16))) double smem_d[];
  __shared__ double red[NT / WAVE];
  const int b = blockIdx.x, axis = blockIdx.y;
  const int Lmax = max(a.W, a.H);
  double* pooled = smem_d;                                          // 64 doubles
  float* u = reinterpret_cast<float*>(smem_d + 64);
  float* t = u + Lmax;
  float* tmp = t + Lmax;
  const PdfRow r = pdf_row(a, b, axis, u, t, tmp, red);
  const double c = (double)gout[0] / ((double)a.B * r.L);
  double acc = 0.0;
  for (int l = threadIdx.x; l < r.L; l += blockDim.x) {
    const double up = (double)clamp_min_nan(u[l], 0.0f);
    acc += c * sgn(up / r.Du - (double)t[l] / r.Dt) * up;
  }
  const double dot = block_sum(acc, red);
  const double corr = (r.su >= 1e-6) ? dot / (r.Du * r.Du) : 0.0;
  // the gradient at image resolution overwrites t (u stays: its sign is the clamp mask)
  for (int l = threadIdx.x; l < r.L; l += blockDim.x) {
    const double up = (double)clamp_min_nan(u[l], 0.0f);
    const double d = c * sgn(up / r.Du - (double)t[l] / r.Dt);
    t[l] = clamp_passes(u[l], 0.0f) ? (float)(d / r.Du - corr) : 0.0f;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < r.Lo; k += blockDim.x) {           // adaptive_avg_pool1d(g, Lo) in float32
    int s, e;
    adaptive_window(k, r.L, r.Lo, s, e);
    float w = 0.0f;
    for (int l = s; l < e; ++l) w = fadd(w, t[l]);
    pooled[k] = (double)(w / (float)(e - s));
  }
  __syncthreads();
  float* g = (axis ? gpy : gpx) + (size_t)b * r.Lo;
  for (int j = threadIdx.x; j < r.Lo; j += blockDim.x) {
    double s = 0.0;
    for (int k = 0; k < r.Lo; ++k) s += pooled[k] * r.inv[(size_t)k * r.Lo + j];
    g[j] = (float)s;
  }
}

int launch_dims_ok(int B, int N, const char* what) {
  ATTWARP_REQUIRE(B > 0 && N > 0, "%s: non-positive size", what);
  if (B > 65535) return fail(ATTWARP_E_UNSUPPORTED, "%s: B=%d > 65535", what, B);
  if (N > LOSS_MAX_N) return fail(ATTWARP_E_UNSUPPORTED, "%s: row length %d > %d", what, N, LOSS_MAX_N);
  return ATTWARP_OK;
}

int pdf_l1_check(const float* px, const float* py, const float* gx, const float* gy, int B, int Lx, int Ly, int W, int H,
                 const double* inv_x, const double* inv_y, const char* what) {
  ATTWARP_REQUIRE(px && py && gx && gy && inv_x && inv_y, "%s: null pointer", what);
  ATTWARP_REQUIRE(B > 0 && Lx > 0 && Ly > 0 && W > 0 && H > 0, "%s: non-positive size", what);
  if (B > 65535) return fail(ATTWARP_E_UNSUPPORTED, "%s: B=%d > 65535", what, B);
  if (Lx > 64 || Ly > 64) return fail(ATTWARP_E_UNSUPPORTED, "%s: low-resolution length > 64", what);
  if (W > 8192 || H > 8192) return fail(ATTWARP_E_UNSUPPORTED, "%s: W, H must be <= 8192", what);
  return ATTWARP_OK;
}

}  // namespace
}  // namespace attwarp

using namespace attwarp;

extern "C" int attwarp_cdf_downsample(const float* p, int B, int N, int L, float* F, void* stream) {
  ATTWARP_REQUIRE(p && F, "cdf_downsample: null pointer");
  ATTWARP_REQUIRE(L > 0, "cdf_downsample: non-positive size");
  if (const int rc = launch_dims_ok(B, N, "cdf_downsample")) return rc;
  if (L > LOSS_MAX_N) return fail(ATTWARP_E_UNSUPPORTED, "cdf_downsample: L=%d > %d", L, LOSS_MAX_N);
  const size_t lds = (size_t)(N + L) * sizeof(double);
  if (const int rc = grant_dynamic_lds(cdf_downsample_kernel, lds, "cdf_downsample", RED_LDS)) return rc;
  hipLaunchKernelGGL(cdf_downsample_kernel, dim3(B), dim3(NT), lds, as_stream(stream), p, N, L, F);
  return check_launch("cdf_downsample_kernel");
}

extern "C" int attwarp_l1_cdf_loss(const float* p, const float* q, int B, int N, double* parts, uint32_t* ticket,
                                   float* loss, void* stream) {
  ATTWARP_REQUIRE(p && q && parts && ticket && loss, "l1_cdf_loss: null pointer");
  if (const int rc = launch_dims_ok(B, N, "l1_cdf_loss")) return rc;
  const size_t lds = (size_t)2 * N * sizeof(double);
  if (const int rc = grant_dynamic_lds(l1_cdf_kernel, lds, "l1_cdf_loss", RED_LDS + FINISH_LDS)) return rc;
  hipLaunchKernelGGL(l1_cdf_kernel, dim3(B), dim3(NT), lds, as_stream(stream), p, q, B, N, parts, ticket, loss);
  return check_launch("l1_cdf_kernel");
}

extern "C" int attwarp_l1_cdf_loss_backward(const float* p, const float* q, int B, int N, const float* gout, float* gp,
                                            float* gq, void* stream) {
  ATTWARP_REQUIRE(p && q && gout && gp && gq, "l1_cdf_loss_backward: null pointer");
  if (const int rc = launch_dims_ok(B, N, "l1_cdf_loss_backward")) return rc;
  const size_t lds = (size_t)3 * N * sizeof(double);
  if (const int rc = grant_dynamic_lds(l1_cdf_backward_kernel, lds, "l1_cdf_loss_backward", RED_LDS)) return rc;
  hipLaunchKernelGGL(l1_cdf_backward_kernel, dim3(B), dim3(NT), lds, as_stream(stream), p, q, B, N, gout, gp, gq);
  return check_launch("l1_cdf_backward_kernel");
}

extern "C" int attwarp_sym_kl(const float* p, const float* q, int B, int N, float eps, double* parts, uint32_t* ticket,
                              float* loss, void* stream) {
  ATTWARP_REQUIRE(p && q && parts && ticket && loss, "sym_kl: null pointer");
  if (const int rc = launch_dims_ok(B, N, "sym_kl")) return rc;
  hipLaunchKernelGGL(sym_kl_kernel, dim3(B), dim3(NT), 0, as_stream(stream), p, q, B, N, eps, parts, ticket, loss);
  return check_launch("sym_kl_kernel");
}

extern "C" int attwarp_sym_kl_backward(const float* p, const float* q, int B, int N, float eps, const float* gout,
                                       float* gp, float* gq, void* stream) {
  ATTWARP_REQUIRE(p && q && gout && gp && gq, "sym_kl_backward: null pointer");
  if (const int rc = launch_dims_ok(B, N, "sym_kl_backward")) return rc;
  hipLaunchKernelGGL(sym_kl_backward_kernel, dim3(B), dim3(NT), 0, as_stream(stream), p, q, B, N, eps, gout, gp, gq);
  return check_launch("sym_kl_backward_kernel");
}

extern "C" int attwarp_recon_loss(const float* px, const float* py, const float* A, int B, int H, int W, int kind,
                                  double* parts, uint32_t* ticket, float* loss, void* stream) {
  ATTWARP_REQUIRE(px && py && A && parts && ticket && loss, "recon_loss: null pointer");
  ATTWARP_REQUIRE(kind == ATTWARP_RECON_MSE || kind == ATTWARP_RECON_L1, "recon_loss: unknown kind %d", kind);
  ATTWARP_REQUIRE(H > 0 && W > 0, "recon_loss: non-positive size");
  if (const int rc = launch_dims_ok(B, W > H ? W : H, "recon_loss")) return rc;
  hipLaunchKernelGGL(recon_kernel, dim3(B), dim3(NT), 0, as_stream(stream), px, py, A, B, H, W, kind, parts, ticket, loss);
  return check_launch("recon_kernel");
}

extern "C" int attwarp_recon_loss_backward(const float* px, const float* py, const float* A, int B, int H, int W, int kind,
                                           const float* gout, float* gpx, float* gpy, void* stream) {
  ATTWARP_REQUIRE(px && py && A && gout && gpx && gpy, "recon_loss_backward: null pointer");
  ATTWARP_REQUIRE(kind == ATTWARP_RECON_MSE || kind == ATTWARP_RECON_L1, "recon_loss_backward: unknown kind %d", kind);
  ATTWARP_REQUIRE(H > 0 && W > 0, "recon_loss_backward: non-positive size");
  if (const int rc = launch_dims_ok(B, W > H ? W : H, "recon_loss_backward")) return rc;
  hipLaunchKernelGGL(recon_backward_kernel, dim3(B), dim3(NT), (size_t)H * sizeof(double), as_stream(stream), px, py, A,
                     B, H, W, kind, gout, gpx, gpy);
  return check_launch("recon_backward_kernel");
}

extern "C" int attwarp_scale_shift(const float* p, int64_t n, float c1, float c2, float* out, void* stream) {
  ATTWARP_REQUIRE(p && out, "scale_shift: null pointer");
  ATTWARP_REQUIRE(n > 0, "scale_shift: non-positive size");
  const int64_t blocks = (n + NT - 1) / NT;
  hipLaunchKernelGGL(scale_shift_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(NT), 0, as_stream(stream),
                     p, n, c1, c2, out);
  return check_launch("scale_shift_kernel");
}

extern "C" int attwarp_entropy(const float* p, int B, int N, float eps, double* parts, uint32_t* ticket, float* loss,
                               void* stream) {
  ATTWARP_REQUIRE(p && parts && ticket && loss, "entropy: null pointer");
  if (const int rc = launch_dims_ok(B, N, "entropy")) return rc;
  hipLaunchKernelGGL(entropy_kernel, dim3(B), dim3(NT), 0, as_stream(stream), p, B, N, eps, parts, ticket, loss);
  return check_launch("entropy_kernel");
}

extern "C" int attwarp_entropy_backward(const float* p, int B, int N, float eps, const float* gout, float* gp,
                                        void* stream) {
  ATTWARP_REQUIRE(p && gout && gp, "entropy_backward: null pointer");
  if (const int rc = launch_dims_ok(B, N, "entropy_backward")) return rc;
  const int64_t blocks = ((int64_t)B * N + NT - 1) / NT;
  hipLaunchKernelGGL(entropy_backward_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(NT), 0,
                     as_stream(stream), p, B, N, eps, gout, gp);
  return check_launch("entropy_backward_kernel");
}

extern "C" int attwarp_pdf_l1_loss(const float* px, const float* py, const float* gx, const float* gy, int B, int Lx,
                                   int Ly, int W, int H, const double* inv_x, const double* inv_y, double* parts,
                                   uint32_t* ticket, float* loss, void* stream) {
  if (const int rc = pdf_l1_check(px, py, gx, gy, B, Lx, Ly, W, H, inv_x, inv_y, "pdf_l1_loss")) return rc;
  ATTWARP_REQUIRE(parts && ticket && loss, "pdf_l1_loss: null pointer");
  const size_t lds = pdf_l1_lds_bytes(W > H ? W : H);
  if (const int rc = grant_dynamic_lds(pdf_l1_kernel, lds, "pdf_l1_loss")) return rc;
  const PdfL1Args a{px, py, gx, gy, B, Lx, Ly, W, H, inv_x, inv_y};
  hipLaunchKernelGGL(pdf_l1_kernel, dim3(B, 2), dim3(NT), lds, as_stream(stream), a, parts, ticket, loss);
  return check_launch("pdf_l1_kernel");
}

extern "C" int attwarp_pdf_l1_loss_backward(const float* px, const float* py, const float* gx, const float* gy, int B,
                                            int Lx, int Ly, int W, int H, const double* inv_x, const double* inv_y,
                                            const float* gout, float* gpx, float* gpy, void* stream) {
  if (const int rc = pdf_l1_check(px, py, gx, gy, B, Lx, Ly, W, H, inv_x, inv_y, "pdf_l1_loss_backward")) return rc;
  ATTWARP_REQUIRE(gout && gpx && gpy, "pdf_l1_loss_backward: null pointer");
  const size_t lds = pdf_l1_lds_bytes(W > H ? W : H);
  if (const int rc = grant_dynamic_lds(pdf_l1_backward_kernel, lds, "pdf_l1_loss_backward")) return rc;
  const PdfL1Args a{px, py, gx, gy, B, Lx, Ly, W, H, inv_x, inv_y};
  hipLaunchKernelGGL(pdf_l1_backward_kernel, dim3(B, 2), dim3(NT), lds, as_stream(stream), a, gout, gpx, gpy);
  return check_launch("pdf_l1_backward_kernel");
}
