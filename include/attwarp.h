/*
 * attwarp.h -- C ABI of libattwarp_hip.so, the MI355X (gfx950) implementation of
 * AttWarp's attention-guided image-warping hot path.
 *
 * The reference (dwipddalal/AttWarp) is pure Python: it has no FFI, custom-op or
 * plugin layer for this path, so there is no existing binding to mirror.  Each
 * entry point below replaces one reference *function* (cited as file:line,
 * AGW = "Attention Guided Warping", MN = "model/marginalnet_full_dataset"); the
 * Python package attwarp_amd re-exposes the reference's names on top of these
 * through ctypes (see INTEGRATION.md for the stub a maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter comment says "host";
 *   - all tensors are dense, row-major ("C contiguous") with the shape given in
 *     the comment, except attwarp_attn_reduce_step which takes element strides;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every
 *     call only enqueues work on that stream, never synchronises, never
 *     allocates: outputs and workspaces are owned by the caller;
 *   - return value: 0 on success, a negative ATTWARP_E_* code on failure (nothing
 *     is enqueued then); attwarp_last_error() gives a thread-local message;
 *   - the library keeps no global mutable state on the product path: transform selection etc. are
 *     arguments (the reference keeps them in module globals, AGW/new_method.py:159-163,378-403) and no
 *     environment variable is read; the only process-wide setting is the test hook attwarp_debug_set().
 */
#ifndef ATTWARP_H
#define ATTWARP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATTWARP_VERSION 100 /* 0.1.0 */

#if defined(__GNUC__)
#define ATTWARP_API __attribute__((visibility("default")))
#else
#define ATTWARP_API
#endif

/* element types */
enum { ATTWARP_F32 = 0, ATTWARP_F16 = 1, ATTWARP_BF16 = 2, ATTWARP_U8 = 3, ATTWARP_F64 = 4 };
/* image layouts: HWC = [B,H,W,C] interleaved (OpenCV / numpy), CHW = [B,C,H,W] planar (torch) */
enum { ATTWARP_HWC = 0, ATTWARP_CHW = 1 };
/* resample arithmetic: CV2 = what cv2.remap(INTER_LINEAR) computes per OpenCV's published algorithm: coordinates
 * rounded to 1/32 pixel, 4 table weights for float32, 15-bit fixed point for uint8 (the reference's arithmetic,
 * the default of the numpy / uint8 drop-ins; unpinned); EXACT = bilinear on the unquantised
 * coordinates (= F.grid_sample(bilinear, border, align_corners=True), north_star's named op).
 * Both modes run on the same staged kernels. */
enum { ATTWARP_EXACT = 0, ATTWARP_CV2 = 1 };
/* attention transforms, AGW/new_method.py:134-179 */
enum { ATTWARP_T_IDENTITY = 0, ATTWARP_T_SQUARE = 1, ATTWARP_T_SQRT = 2, ATTWARP_T_EXP = 3, ATTWARP_T_LOG = 4 };

/* error codes */
enum {
  ATTWARP_OK = 0,
  ATTWARP_E_ARG = -1,      /* bad argument (null pointer, non-positive size, unknown enum) */
  ATTWARP_E_UNSUPPORTED = -2, /* valid request this build cannot serve (size limit, dtype) */
  ATTWARP_E_LAUNCH = -3    /* HIP reported an error while enqueueing */
};

ATTWARP_API int attwarp_version(void);
ATTWARP_API const char* attwarp_last_error(void);

/* ---- test / measurement hook: exists ONLY in the tuning flavour of the library (libattwarp_hip_tuning.so, built with
 * -DATTWARP_TUNING; the product library libattwarp_hip.so does not export it and contains no override table).
 * Kernel variants are chosen automatically from the shapes; the parity tests and the A/B tools force a particular one
 * to check the variants against each other (e.g. key "remap_variant" = 1: generic gather kernel only; "remap_rows" =
 * R).  value < 0 restores "automatic", key "reset" restores every key; the previous value of the key is returned
 * through *previous when it is not NULL.  Keys: see kTuneNames in csrc/error.hip.  Process wide, single threaded,
 * test only.
 * One key is a query and sets nothing: "remap_plan:<layout>,<mode>,<B>,<C>,<H>,<W>,<H_out>,<W_out>" writes to *previous
 * what the float32 staged resample would launch for 16-byte aligned images of that shape under the overrides in force,
 * packed as rows per block | row blocks per workgroup << 8 | XCD group << 16 | streaming policy << 24, or -1 when the
 * request takes the generic gather kernel.  Nothing is launched; no GPU is needed. */
#ifdef ATTWARP_TUNING
ATTWARP_API int attwarp_debug_set(const char* key, int value, int* previous);
/* measurement yardstick (csrc/calib.hip): ONE launch that reads read_bytes from src and writes write_bytes to dst (16-byte
 * aligned device buffers) -- a plain streaming kernel for the bytes of a chain step, the ruler of bench.py's `step_over_copy` */
ATTWARP_API int attwarp_debug_stream_copy(const void* src, size_t read_bytes, void* dst, size_t write_bytes, void* stream);
#endif

/* ---- A1: BatchMaskHookLogger._process_attention, AGW/attention_extraction/llava.py:385-396
 * attn [B,heads,q,kv] with element strides; for sample b uses row q-1, columns
 * starts[b] .. starts[b]+ntok-1; per-head renormalisation (x / (sum + 1e-12)), mean over heads.
 * out [B,ntok] in the same dtype (F32/F16/BF16).  starts: device int32[B]; ntok <= kv_len is required and a start
 * outside [0, kv_len-ntok] is clamped into it on the device (no out-of-row reads).
 * F16 / BF16 rows with unit kv stride whose slice starts at an odd element are read in dword-aligned four-element words:
 * the element before the slice and up to three elements behind it are read with it -- elements of the same row (a slice
 * that ends within three elements of the row's end is read with plain element-aligned loads instead), so nothing outside
 * the allocation the tensor lives in is touched (the element before the slice of a view that starts at an odd element of
 * its buffer is the only access outside the tensor itself). */
ATTWARP_API int attwarp_attn_reduce_step(const void* attn, int dtype, int B, int heads, int q_len, int kv_len,
                             int64_t stride_b, int64_t stride_h, int64_t stride_q, int64_t stride_kv,
                             const int32_t* starts, int ntok, void* out, void* stream);

/* ---- A2: BatchMaskHookLogger.finalize_batch, llava.py:401-411
 * steps [T,B,ntok] -> out [B,ntok] = mean over T (same dtype). */
ATTWARP_API int attwarp_attn_finalize(const void* steps, int dtype, int T, int B, int ntok, void* out, void* stream);

/* ---- A1+A2 fused over a captured stack of last-query rows.
 * rows [T,B,heads,kv] -> out [B,ntok]; equals finalize(step(rows[t]) for t).
 * ws: workspace of attwarp_attn_reduce_stack_workspace_bytes(...) bytes ([T,B,ntok] step maps). */
ATTWARP_API size_t attwarp_attn_reduce_stack_workspace_bytes(int dtype, int T, int B, int ntok);
ATTWARP_API int attwarp_attn_reduce_stack(const void* rows, int dtype, int T, int B, int heads, int kv_len,
                              const int32_t* starts, int ntok, void* out, void* ws, void* stream);

/* ---- "next" row 4: hook-side capture without materialising [B,heads,q,kv] probabilities.
 * Replaces  register_hook_and_patch (llava.py:422-438: output_attentions=True on the target layer, i.e. HF's
 * eager_attention_forward producing softmax(QK^T*scaling + mask) for every query row) followed by
 * _process_attention (llava.py:385-396), which only consumes the LAST query row.
 *   q  : post-RoPE query vectors of the last token, [B,heads,head_dim], element strides q_stride_b/_h
 *   k  : post-RoPE key cache, [B,kv_heads,kv_len,head_dim], element strides k_stride_b/_h/_t
 *        (head_dim contiguous; heads % kv_heads == 0: grouped-query attention shares a key head)
 *   kv_begin : device int32[B] or NULL - first attended key position (left padding); earlier keys get p = 0
 *   starts   : device int32[B], image-token slice starts, clamped into [0, kv_len-ntok] on the device
 *   out      : [B,ntok] in `dtype` = mean over heads of p[st:st+ntok] / (sum + 1e-12), as A1
 *   ws       : attwarp_attn_probe_workspace_bytes(...) bytes, 16-byte aligned
 * Rounding mirrors the eager path's dtype transitions (matmul -> dtype, *scaling -> dtype, softmax in
 * float32 -> dtype).  q, k 16-byte aligned, strides multiples of 16 bytes, kv_len <= 15872, ntok <= 1024. */
ATTWARP_API size_t attwarp_attn_probe_workspace_bytes(int dtype, int B, int heads, int ntok);
ATTWARP_API int attwarp_attn_probe_last_query(const void* q, const void* k, int dtype, int B, int heads, int kv_heads,
                                  int head_dim, int kv_len, int64_t q_stride_b, int64_t q_stride_h,
                                  int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t,
                                  const int32_t* kv_begin, const int32_t* starts, int ntok, float scaling,
                                  void* out, void* ws, void* stream);

/* ---- the layer-selection study's raw row (Ablations/uncertainty_attn_maps_llava.py:56:
 * out.attentions[L-1][b, :, -1, span].mean(0)): same arguments, workspace and per-head probabilities as
 * attwarp_attn_probe_last_query, but out[b,t] = mean over heads of p[b,h,st+t] WITHOUT the per-head renormalisation:
 * the head probabilities (model dtype) summed in double in head order, divided by heads in double, rounded once to
 * `dtype`.  Two launches (probabilities, head mean). */
ATTWARP_API int attwarp_attn_probe_head_mean(const void* q, const void* k, int dtype, int B, int heads, int kv_heads,
                                 int head_dim, int kv_len, int64_t q_stride_b, int64_t q_stride_h,
                                 int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t,
                                 const int32_t* kv_begin, const int32_t* starts, int ntok, float scaling,
                                 void* out, void* ws, void* stream);

/* ---- A3: revise_mask = normalize("min") -> enhance -> k x k box filter, llava.py:207-238
 * mask [B,n,n] float32 -> out [B,n,n] float32 (n <= 32, odd kernel_size <= 7). */
ATTWARP_API int attwarp_mask_postproc(const float* mask, int B, int n, int kernel_size, float enhance_coe,
                          float* out, void* stream);

/* ---- A4: ToPILImage (x*255, truncating cast) + PIL Image.resize(LANCZOS), llava.py:192-196,243,253
 * mask_f32 [B,h,w] float32 in [0,1]  (or mask_u8 [B,h,w] if mask_f32 is NULL)
 * -> out [B,out_h,out_w] uint8.  Coefficients: host-computed Pillow tables uploaded by the
 * caller: bounds_* int32[out,2] = (first tap, tap count), kk_* int32[out,ksize] (22-bit fixed point; entries at
 * index >= tap count are never used: every kernel form masks them by the row's tap count; a row stride of exactly 8
 * -- pad narrower tables to 8 columns with anything -- selects the fastest vertical pass).
 * tmp: uint8 [B,h,out_w] workspace (horizontal pass output). */
ATTWARP_API int attwarp_mask_upsample_lanczos(const float* mask_f32, const uint8_t* mask_u8, int B, int h, int w,
                                  int out_h, int out_w,
                                  const int32_t* bounds_x, const int32_t* kk_x, int ksize_x,
                                  const int32_t* bounds_y, const int32_t* kk_y, int ksize_y,
                                  uint8_t* tmp, uint8_t* out, void* stream);

/* ---- "next" row 3: warped uint8 image -> CLIP-ready tensor, replacing the PNG round trip
 * AGW/new_method.py:491 (cv2.imwrite) -> AGW/evaluate_accuracy.py:157-158 (Image.open, process_images):
 * HF CLIPImageProcessor as LLaVA-1.5 configures it = PIL BICUBIC resize (shorter edge -> size), center crop,
 * float32(float64(u8)*(1/255)), (x-mean)/std in float32, channels first.
 * src [B,h,w,C] uint8 (C<=4) -> out [B,C,size,size] (F32 or F16).  The caller passes Pillow's 8-bit coefficient
 * tables for the resized width / height (identity tables when an axis keeps its size) and the crop origin
 * (top,left) in the resized image; mean/stdv are HOST arrays of C floats; tmp: uint8 [B,h,size,C]. */
ATTWARP_API int attwarp_clip_preprocess_u8(const uint8_t* src, int B, int h, int w, int C, int top, int left, int size,
                               const int32_t* bounds_x, const int32_t* kk_x, int ksize_x,
                               const int32_t* bounds_y, const int32_t* kk_y, int ksize_y,
                               const float* mean, const float* stdv, uint8_t* tmp, void* out, int out_dtype,
                               void* stream);

/* ---- "next" row 1: the memory-bound tail of MarginalNet.forward, MN/model.py:73-88.
 * masked_token_mean: tok [B,Lt,D] (F32/F16/BF16), mask [B,Lt] float32 (the reference's [B,Lt,1])
 *   -> out [B,D] float32 = sum_l(float(tok)*mask) / max(sum_l mask, 1)            (model.py:77-78)
 * film_axis_means: v [B,Ch,H,W] float32, gamma_beta [B,2*Ch] float32 (film output: gamma | beta)
 *   -> vx [B,Ch,W] = mean over H of (gamma*v + beta), vy [B,Ch,H] = mean over W   (model.py:80-88)
 *   H*(W+1) <= 4096. */
ATTWARP_API int attwarp_masked_token_mean(const void* tok, int dtype, const float* mask, int B, int Lt, int D,
                              float* out, void* stream);
ATTWARP_API int attwarp_film_axis_means(const float* v, const float* gamma_beta, int B, int Ch, int H, int W,
                            float* vx, float* vy, void* stream);
/* Training (autograd) forms of film_axis_means.  _t: v and gamma_beta in their own dtypes (v_dtype, gb_dtype: F32, F16
 * or BF16, as the trainer's autocast gives them), upcast exactly and computed as above; float32 inputs give the bits of
 * attwarp_film_axis_means.  _backward: upstream gradients gx [B,Ch,W], gy [B,Ch,H] float32 ->
 *   dv [B,Ch,H,W] (v_dtype) = gamma * (gx*(1/H) + gy*(1/W)), bit for bit torch's float32 autograd on the GPU (which
 *   divides by a scalar as a multiply by its float32 reciprocal);
 *   dgamma_beta [B,2*Ch] (gb_dtype) = (sum_yx v*gw | sum_yx gw), gw = gx*(1/H) + gy*(1/W), float64 sums rounded once.
 * One wave per (b, c) plane: deterministic, no atomics.  H*(W+1) <= 4096. */
ATTWARP_API int attwarp_film_axis_means_t(const void* v, int v_dtype, const void* gamma_beta, int gb_dtype, int B,
                              int Ch, int H, int W, float* vx, float* vy, void* stream);
ATTWARP_API int attwarp_film_axis_means_backward(const void* v, int v_dtype, const void* gamma_beta, int gb_dtype,
                                     const float* gx, const float* gy, int B, int Ch, int H, int W, void* dv,
                                     void* dgamma_beta, void* stream);

/* ---- A5: F.adaptive_avg_pool2d(A,(oh,ow)), call sites MN/trainer.py:197,433,465
 * A [B,H,W] float32 -> out [B,oh,ow] float32.  sanitize != 0 also applies the trainer's
 * torch.nan_to_num(A, nan=0, posinf=0, neginf=0).clamp_min(0) (MN/trainer.py:202) to the pooled map. */
ATTWARP_API int attwarp_adaptive_avg_pool(const float* A, int B, int H, int W, int oh, int ow, int sanitize, float* out,
                              void* stream);

/* ---- A6: gt_marginals, MN/checkpoint_utils.py:43-51
 * A [B,H,W] float32 -> px [B,W], py [B,H] float32.  ws: workspace of
 * attwarp_axis_sums_workspace_bytes(B,H,W) bytes. */
ATTWARP_API size_t attwarp_axis_sums_workspace_bytes(int B, int H, int W);
ATTWARP_API int attwarp_gt_marginals(const float* A, int B, int H, int W, float* px, float* py, void* ws, void* stream);

/* ---- A7: safe_softmax(dim=1), MN/model.py:8-14.  logits [B,N] -> out [B,N], N <= 4096. */
ATTWARP_API int attwarp_safe_softmax(const float* logits, int B, int N, float eps, float* out, void* stream);
/* Its backward: logits [B,N], upstream gradient g [B,N] -> dlogits [B,N], all float32, N <= 4096.  The forward is
 * recomputed from the logits; torch autograd's rules are applied in reverse (amax: split evenly over tied maxima;
 * nan_to_num: 0 at non-finite logits).  Elementwise float32, float64 row sums. */
ATTWARP_API int attwarp_safe_softmax_backward(const float* logits, const float* g, int B, int N, float eps,
                                  float* dlogits, void* stream);

/* ---- A8: upsample_pdf_right_inverse, MN/checkpoint_utils.py:64-131
 * y [N,Lo] float32 -> out [N,L] float32.  inv: device float64 [Lo,Lo] = (A A^T + eps I)^-1 of the
 * adaptive-avg-pool1d matrix A[Lo,L] (24x24: computed once per (Lo,L,eps) on the host). Lo <= 64. */
ATTWARP_API int attwarp_upsample_pdf_right_inverse(const float* y, int N, int Lo, int L, const double* inv,
                                       float* out, void* stream);

/* ---- A9: cdf_from_density, MN/checkpoint_utils.py:30-41.  p [B,L] -> F [B,L] float32. */
ATTWARP_API int attwarp_cdf_from_density(const float* p, int B, int L, float* F, void* stream);

/* ---- A10: _make_strictly_increasing (:17-28) and resample_cdf (:53-62). */
ATTWARP_API int attwarp_make_strictly_increasing(const float* F, int B, int N, double eps, float* out, void* stream);
ATTWARP_API int attwarp_resample_cdf(const float* F, int B, int N, int L, float* out, void* stream);

/* ---- A11: grid construction of warp_from_cdf_torch, MN/checkpoint_utils.py:167-193
 * F [B,L] float32 CDF -> map [B,n_out] float32 source coordinate per output index
 * (the reference meshgrids two such vectors into dense maps for cv2.remap). L <= 16384. */
ATTWARP_API int attwarp_axis_map_from_cdf(const float* F, int B, int L, int n_out, float* map, void* stream);

/* ---- A8+A9+A11 fused: 24-bin PDFs -> maps, the MarginalNet inference chain MN/trainer.py:285-289
 * px [B,Lo], py [B,Lo] -> map_x [B,W_out], map_y [B,H_out]; inv_x / inv_y as in A8 for L=W / L=H. */
ATTWARP_API int attwarp_axis_maps_from_pdf(const float* px, const float* py, int B, int Lo, int W, int H,
                               int W_out, int H_out, const double* inv_x, const double* inv_y,
                               float* map_x, float* map_y, void* stream);

/* ---- A2+A6+A8+A9+A11 fused: per-step attention maps (A1 output) -> inverse maps in ONE launch.
 * steps [T,B,g*g] float32 -> mean over steps -> marginals of the g x g map -> PDF up-sample -> CDF ->
 * map_x [B,W_out], map_y [B,H_out]; att_out (optional, may be NULL): the aggregated [B,g*g] map (A2 output).
 * Bit-identical to the separate stages. */
ATTWARP_API int attwarp_axis_maps_from_steps(const float* steps, int T, int B, int g, int W, int H, int W_out, int H_out,
                                 const double* inv_x, const double* inv_y, float* map_x, float* map_y,
                                 float* att_out, void* stream);

/* the same for step maps in the model dtype (F32 / F16 / BF16): the mean over steps (A2) is accumulated in double,
 * rounded ONCE to that dtype and divided by T in it, as attwarp_attn_finalize does; the rest is float32.  Equals
 * attwarp_attn_finalize -> float() -> attwarp_gt_marginals -> attwarp_axis_maps_from_pdf bit for bit. */
ATTWARP_API int attwarp_axis_maps_from_steps_t(const void* steps, int dtype, int T, int B, int g, int W, int H, int W_out,
                                   int H_out, const double* inv_x, const double* inv_y, float* map_x, float* map_y,
                                   float* att_out, void* stream);

/* ---- one step of a STREAM of equally shaped batches in ONE launch (pipeline.OverlappedWarp; replaces the three
 * launches reduce -> maps -> resample of AGW/main_batched.py's per-batch chain when batches follow each other):
 *   R  the A12 resample of batch k      src [B,...] float32 + map_x/map_y (built by the previous step)  -> dst
 *   M  the maps of batch k+1            steps_in [T,B,g*g] (previous step's reduce) -> map_x_next / map_y_next
 *   A  the A1 reduce of batch k+2       rows [n_rows = T*B, heads, kv_len], row j uses starts[j % starts_mod]
 *                                       -> steps_out [T*B, ntok]
 * rows, steps_in and steps_out share attn_dtype (F32 / F16 / BF16: the model dtype, as the hook delivers them; A2's
 * mean over steps is rounded in that dtype like llava.py:409-411);
 * as block ranges of one grid (map blocks first, then reduce and resample blocks interleaved in chunks of 8): no
 * launch boundary, no queue hand-off inside a step.  The three pieces work on different batches and must not alias
 * (steps_out != steps_in, map_*_next != map_*).  M (steps_in == NULL) and A (rows == NULL) are optional.  Same
 * arithmetic, bit for bit, as attwarp_remap_bilinear / attwarp_axis_maps_from_steps / attwarp_attn_reduce_step.
 * ATTWARP_E_UNSUPPORTED when the image shape takes the generic resample (rows wider than 4096 floats, unaligned
 * rows), ntok is not a multiple of 4 or > 768, g > 32, ntok != g*g while both steps_in and rows are given (steps_out of
 * one call is steps_in [T,B,g*g] of the next), or an axis so long that the map construction needs more than 64 KB of
 * LDS (max(W,H) > ~4800): use the three separate entry points then. */
ATTWARP_API int attwarp_warp_step_fused(const float* src, float* dst, int layout, int B, int C, int H, int W, int H_out,
                            int W_out, const float* map_x, const float* map_y, int mode,
                            int attn_dtype, const void* steps_in, int T, int g, const double* inv_x,
                            const double* inv_y, float* map_x_next, float* map_y_next,
                            const void* rows, int n_rows, int heads, int kv_len, const int32_t* starts,
                            int starts_mod, int ntok, void* steps_out, void* stream);

/* ---- the same one-launch step for TWO consecutive batches of the stream per piece ("slots"): R(k), R(k+1) | M(k+2),
 * M(k+3) | A(k+4), A(k+5) -- every dependency is on an earlier launch, and the launch's ramp and tail are paid once per two
 * batches.  `slots` is a HOST array of nslots (1 or 2) pointer sets (device pointers, meanings as the arguments of
 * attwarp_warp_step_fused; `starts` per slot); geometry, dtype and mode are shared.  nslots == 1 equals
 * attwarp_warp_step_fused.  Both slots must carry the same pieces, write different buffers, and their images must share
 * their 16-byte alignment. */
typedef struct attwarp_step_slot {
  const float* src; float* dst; const float* map_x; const float* map_y;      /* R: resample of this slot's batch       */
  const void* steps_in; float* map_x_next; float* map_y_next;                 /* M: step maps [T,B,g*g] -> its maps     */
  const void* rows; const int32_t* starts; void* steps_out;                   /* A: rows [n_rows,heads,kv] -> step maps */
} attwarp_step_slot;
ATTWARP_API int attwarp_warp_step_fused_slots(const attwarp_step_slot* slots, int nslots, int layout, int B, int C, int H, int W,
                                  int H_out, int W_out, int mode, int attn_dtype, int T, int g, const double* inv_x,
                                  const double* inv_y, int n_rows, int heads, int kv_len, int starts_mod, int ntok,
                                  void* stream);

/* ---- the attention reduce of batch k+2 and the map construction of batch k+1 of a batch stream in ONE launch (for
 * large images, where the resample keeps its own launch): rows [n_rows = T*B, heads, kv_len] -> steps_out [T*B, ntok];
 * steps_in [T,B,g*g] (the previous call's steps_out buffer of the other parity) -> map_x [B,W_out], map_y [B,H_out].
 * One dtype (F32 / F16 / BF16) for rows and both step buffers; ntok == g*g.  Equals attwarp_attn_reduce_step +
 * attwarp_axis_maps_from_steps_t bit for bit. */
ATTWARP_API int attwarp_attn_reduce_and_maps(int attn_dtype, const void* rows, int n_rows, int heads, int kv_len,
                                 const int32_t* starts, int starts_mod, int ntok, void* steps_out,
                                 const void* steps_in, int T, int B, int g, int W, int H, int W_out, int H_out,
                                 const double* inv_x, const double* inv_y, float* map_x, float* map_y, void* stream);

/* ---- one step of the main_batched chain (AGW/main_batched.py:243-287: revise_mask -> x255 uint8 -> PIL LANCZOS ->
 * float64 marginals -> CDF -> np.interp -> uint8 cv2.remap) for a STREAM of equally shaped batches, as ONE launch, with
 * save_warped_image's own keyword arguments (AGW/new_method.py:405-411: transform, exp_scale, exp_divisor, apply_inverse;
 * :134-191 the five transforms and their inverses, :219-226 the inverse on the marginals; main_batched.py:280-287 passes
 * "identity", 1.0, 1.0, False; the module default is "sqrt", :191).  The five stages run on five different batches (block
 * ranges of one grid):
 *   R(k)    images [B,H,W,C] uint8 + map_x [B,W_out], map_y [B,H_out]         -> out [B,H_out,W_out,C]   (mode cv2)
 *   F(k+1)  sums_in (axis sums of the mask of batch k+1, written by P)        -> map_x_next, map_y_next
 *   P(k+2)  mota_in [B,H,W] uint8 (up-sampled mask of batch k+2)              -> sums_out
 *   L(k+3)  rev_in [B,g,g] float32 (revised mask of batch k+3) + Pillow tables (ksize_y == 8, zero padded) -> mota_out
 *   V(k+4)  masks [B,g,g] float32 (aggregated attention of batch k+4)         -> rev_out
 * sums_*: attwarp_axis_sums_workspace_bytes(B,H,W) bytes each.  An output buffer must not alias the buffer the next
 * stage reads in the same launch (double buffer each intermediate by batch parity).  transform = ATTWARP_T_* applies in
 * P (element transform) and F (apply_inverse: the inverse on the marginals); transform_lut: for ATTWARP_T_SQRT / EXP / LOG
 * the 256 doubles attwarp_attention_transform_lut wrote for the same (transform, exp_scale, exp_divisor) -- a constant of the
 * stream, computed once -- NULL allowed for identity / square.  Every stage computes what
 * attwarp_mask_postproc / attwarp_mask_upsample_lanczos / attwarp_axis_maps_from_attention(U8, transform, ...) /
 * attwarp_remap_bilinear(U8, HWC, CV2) compute, bit for bit.  ATTWARP_E_UNSUPPORTED when one of the stages would not
 * run on its staged kernel for this shape (rows wider than 4096 bytes, W not a multiple of 4, W or H equal to g, ...):
 * use the separate entry points, or attwarp_mask_chain_ragged (below: any width), then. */
ATTWARP_API int attwarp_mask_chain_step(const uint8_t* images, uint8_t* out, int B, int C, int H, int W, int H_out, int W_out,
                            const float* map_x, const float* map_y,
                            const void* sums_in, float* map_x_next, float* map_y_next,
                            const uint8_t* mota_in, void* sums_out,
                            const float* rev_in, const int32_t* bounds_x, const int32_t* kk_x, int ksize_x,
                            const int32_t* bounds_y, const int32_t* kk_y, int ksize_y, uint8_t* mota_out,
                            const float* masks, int g, int kernel_size, float enhance_coe, float* rev_out,
                            int transform, double exp_scale, double exp_divisor, int apply_inverse,
                            const double* transform_lut, void* stream);

/* The 256-entry table of the transformed byte values of a uint8 attention map: lut[v] = transform(max(v, 0)) + 1e-9 for
 * v = 0 .. 255 (AGW/new_method.py:134-179,208-215), by the very device functions attwarp_axis_maps_from_attention(U8) uses
 * (bit-identical).  lut: 256 doubles on the device.  Needed by the one-launch chain steps for ATTWARP_T_SQRT / EXP / LOG. */
ATTWARP_API int attwarp_attention_transform_lut(int transform, double exp_scale, double exp_divisor, double* lut, void* stream);

/* ---- the same chain for batches of DIFFERENTLY sized images: what AGW/main_batched.py:243-287 actually holds (`b_images[j]`
 * are PIL images at their native sizes; blend_mask up-samples the mask to `image.size`, llava.py:253; save_warped_image warps
 * at that size to width x height = 500 x 500, new_method.py:415-422,478-488).  Output is dense: [B,H_out,W_out,C].
 *
 * A batch is described by a TABLE the host builds once per batch and copies to the device unchanged (it is position
 * independent):
 *   1. fill attwarp_ragged_image[B] (HOST array of DEVICE pointers): the image, its size, and Pillow's 8-bit LANCZOS
 *      coefficient tables for g -> W (ksize_x <= 8 columns) and g -> H (exactly 8 columns, zero padded) --
 *      attwarp_pil_coeffs_8bpc computes them on the host, callers cache them per distinct size;
 *   2. attwarp_ragged_table_bytes(...) -> size; attwarp_ragged_plan(...) writes the table into HOST memory: an
 *      attwarp_ragged_header (public, below: buffer sizes the caller must provide) followed by per-image records, numpy's
 *      pairwise-summation plans of the distinct widths / heights, the block maps of the stages whose block count
 *      depends on the image and the order in which the stages visit the images (largest first);
 *   3. copy table_bytes to the device (any 8-byte aligned address);
 *   4. attwarp_mask_chain_ragged(...) with the host AND the device copy of each stage's table.
 * Limits (ATTWARP_E_UNSUPPORTED from attwarp_ragged_plan otherwise; use the per-image entry points then): rows of 4 ..
 * 4096 bytes on both sides (W*C, W_out*C), H, W > g (the mask is up-sampled on both axes), max(H,W) <= 8192, g <= 32,
 * B <= 65535.  Any alignment: 683 x 3-byte rows are served by the same staged kernels as 684 x 3. */
#define ATTWARP_RAGGED_MAX_LEAVES 64
enum { ATTWARP_PIL_LANCZOS = 0, ATTWARP_PIL_BICUBIC = 1, ATTWARP_PIL_BILINEAR = 2 };
typedef struct attwarp_ragged_image {
  const uint8_t* image;                            /* device: [H,W,C] uint8 interleaved, any byte address */
  const int32_t* bounds_x; const int32_t* kk_x;    /* device: Pillow tables g -> W: int32 [W,2], int32 [W,ksize_x] */
  const int32_t* bounds_y; const int32_t* kk_y;    /* device: g -> H: int32 [H,2], int32 [H,8] (zero padded to 8 columns) */
  int32_t H, W, ksize_x, reserved;
} attwarp_ragged_image;
typedef struct attwarp_ragged_header {             /* first bytes of a table written by attwarp_ragged_plan */
  uint32_t magic;
  int32_t B, C, g, H_out, W_out;
  int32_t nL, nP, nR, nplans;                      /* blocks of the up-sampling, marginals and resample stages; distinct plans */
  int32_t rows_per_block, blocks_per_image, kd, max_hw;
  uint64_t table_bytes;                            /* size of the table (copy this many bytes to the device) */
  uint64_t mota_bytes;                             /* the batch's up-sampled masks, packed: uint8 buffer of this size */
  uint64_t sums_bytes;                             /* the batch's axis-sum workspace (float64) */
  uint64_t lds_bytes;
  uint64_t off_images, off_plans, off_lmap, off_pmap, off_order;
} attwarp_ragged_header;

/* HOST: Pillow's ImagingResample coefficient tables for an 8-bit image (precompute_coeffs + normalize_coeffs_8bpc,
 * libImaging/Resample.c; 22-bit fixed point) for resizing in_size -> out_size with `filter`.  bounds: int32 [out_size,2]
 * = (first tap, tap count); kk: int32 [out_size,kk_cols], zero padded.  Returns the tap-count bound ksize (<= kk_cols),
 * 1 with identity tables when in_size == out_size (Pillow skips that pass), or a negative error code. */
ATTWARP_API int attwarp_pil_coeffs_8bpc(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk, int kk_cols);

/* HOST: size of / contents of the table of one batch (see above).  0 / a negative code when the batch does not run on
 * the ragged kernel (attwarp_last_error() says which image and why). */
ATTWARP_API size_t attwarp_ragged_table_bytes(const attwarp_ragged_image* images, int B, int C, int g, int H_out, int W_out);
ATTWARP_API int attwarp_ragged_plan(const attwarp_ragged_image* images, int B, int C, int g, int H_out, int W_out, void* table,
                        size_t table_bytes);

/* One launch running up to five stages, each on ITS OWN batch (as attwarp_mask_chain_step; a stage whose host table --
 * V: whose `masks` -- is NULL is skipped, so one batch alone is five calls with one stage each):
 *   R(k)    r_*: images of the table + map_x [B,W_out], map_y [B,H_out]          -> out [B,H_out,W_out,C]   (mode cv2)
 *   F(k+1)  f_*: sums_in (sums_bytes of that table, written by P)               -> map_x_next, map_y_next
 *   P(k+2)  p_*: mota_in (mota_bytes of that table, written by L)               -> sums_out
 *   L(k+3)  l_*: rev_in [B,g,g] float32 (written by V) + the images' Pillow tables -> mota_out
 *   V(k+4)  masks [B_masks,g,g] float32                                          -> rev_out
 * transform / exp_scale / exp_divisor / apply_inverse / transform_lut: as attwarp_mask_chain_step (used by the P and F stages).
 * Every stage computes what attwarp_mask_postproc / attwarp_mask_upsample_lanczos / attwarp_axis_maps_from_attention(U8,
 * transform, ...) / attwarp_remap_bilinear(U8, HWC, CV2) compute on that image alone, bit for bit.  The batches of one
 * launch share C, g and the output size; their B and image sizes are free. */
ATTWARP_API int attwarp_mask_chain_ragged(const void* r_host, const void* r_dev, uint8_t* out, const float* map_x, const float* map_y,
                              const void* f_host, const void* f_dev, const void* sums_in, float* map_x_next, float* map_y_next,
                              const void* p_host, const void* p_dev, const uint8_t* mota_in, void* sums_out,
                              const void* l_host, const void* l_dev, const float* rev_in, uint8_t* mota_out,
                              const float* masks, int B_masks, int g, int kernel_size, float enhance_coe, float* rev_out,
                              int transform, double exp_scale, double exp_divisor, int apply_inverse,
                              const double* transform_lut, void* stream);

/* ---- A13: grid construction of warp_image_by_attention, AGW/new_method.py:206-265
 * att [B,h,w] (U8/F32/F64) -> map_x [B,new_w], map_y [B,new_h] float32.
 * ws: workspace of attwarp_axis_sums_workspace_bytes(B,h,w) bytes. */
ATTWARP_API int attwarp_axis_maps_from_attention(const void* att, int dtype, int B, int h, int w, int new_w, int new_h,
                                     int transform, double exp_scale, double exp_divisor, int apply_inverse,
                                     float* map_x, float* map_y, void* ws, void* stream);

/* ---- cv2.resize(image, (W_out, H_out), interpolation=cv2.INTER_LINEAR), AGW/new_method.py:369 (reached from :478
 * when the attention map's size differs from the image's; a no-op in both reference drivers).
 * src [B,H,W,C] interleaved, F32 or U8 -> dst [B,H_out,W_out,C].  OpenCV's published algorithm (resize.cpp): half-pixel
 * centres, uint8 with 11-bit fixed-point coefficients and its (b * (D >> 4)) >> 16 vertical pass, an exact 2 x 2
 * decimation as INTER_AREA; parity unpinned like attwarp_remap_bilinear's cv2 mode (OpenCV is absent here). */
ATTWARP_API int attwarp_resize_linear(const void* src, void* dst, int dtype, int B, int C, int H, int W, int H_out,
                          int W_out, void* stream);

/* ---- Jet heat-map overlays of the reference's drivers, a whole batch of differently sized images per call:
 *   ATTWARP_OVERLAY_BLEND_MASK  blend_mask's merged image, AGW/attention_extraction/llava.py:254-269:
 *       idx = (uint8) fmaf(m, a, b) with cv2.normalize(NORM_MINMAX)'s a = (float)(255 / (max - min)) (0 when max == min),
 *       b = -(float)(min * a) -- uint8 masks only; out = addWeighted(image, 1 - alpha, jet[idx], alpha, 0)
 *   ATTWARP_OVERLAY_SAVE_WARPED save_warped_image's masked overlay, AGW/new_method.py:455-475:
 *       idx = (uint8)((m - min) / (max - min) * 255) in the map's dtype (uint8 differences divided in float64; float32
 *       stays float32), 0 everywhere unless max > min + 1e-9 (a NaN anywhere fails that test); out = addWeighted(jet[idx],
 *       alpha, image, 1 - alpha, 0)
 * jet = cv2.COLORMAP_JET, restated from OpenCV's colormap.cpp (csrc/overlay_jet.hpp, tools/gen_jet_table.py).  addWeighted
 * on 8-bit data: cvRound(fmaf(s1, w1, fmaf(s2, w2, 0))) with the weights alpha and 1 - alpha (double) rounded to float32 --
 * OpenCV's AVX2 vector path; exact in any evaluation order at alpha = 0.5, OpenCV's scalar tail may differ by 1 elsewhere.
 * Parity with OpenCV itself is unpinned here (OpenCV is absent; tests/test_overlay_vs_opencv.py pins it where present).
 *   images     : HOST array of B records (validated here; the grid is sized from it)
 *   images_dev : a DEVICE copy of the same B records, 8-byte aligned (the kernels read it)
 *   map_dtype  : U8, F32 or F64 (one dtype for the batch); in_order / out_order: ATTWARP_RGB or ATTWARP_BGR
 *   ws         : attwarp_overlay_workspace_bytes(B) bytes, 16-byte aligned (per-block min / max partials)
 * Images: [H,W,3] uint8 interleaved at any byte address (683 x 3-byte rows, images packed back to back); maps: [H,W] dense,
 * uint8 at any byte address, float32 / float64 element aligned; out: [H,W,3] uint8 at any byte address (may equal image).
 * Two launches (per-block min / max, then colour + blend), each over the whole batch.  H * W <= 2^30, B <= 65535. */
enum { ATTWARP_OVERLAY_BLEND_MASK = 0, ATTWARP_OVERLAY_SAVE_WARPED = 1 };
enum { ATTWARP_RGB = 0, ATTWARP_BGR = 1 };
typedef struct attwarp_overlay_image {
  const uint8_t* image;                            /* device: [H,W,3] uint8 */
  const void* map;                                 /* device: [H,W] of map_dtype (e.g. a view into a ragged batch's packed masks) */
  uint8_t* out;                                    /* device: [H,W,3] uint8 */
  int32_t H, W;
} attwarp_overlay_image;
ATTWARP_API size_t attwarp_overlay_workspace_bytes(int B);
ATTWARP_API int attwarp_heatmap_overlay(const attwarp_overlay_image* images, const attwarp_overlay_image* images_dev, int B,
                            int map_dtype, int style, double alpha, int in_order, int out_order, void* ws, void* stream);

/* ---- the layer-selection study's maps and box metrics (Ablations/uncertainty_attn_maps_llava.py:62-64, 164;
 * Ablations/attention_redistribution/metrics.py:15-25), a whole batch of differently sized maps per call.
 * cv2.resize(float32 grid [h,w], (W, H), INTER_LANCZOS4) = OpenCV 4.x resizeGeneric_ (HResizeLanczos4, VResizeLanczos4)
 * for one channel: horizontal pass, then vertical pass, float32 with every product and sum rounded, taps in ascending
 * order; dsize == ssize copies.  Parity with OpenCV itself is a few ulp (its vectorised vertical pass sums in another
 * order); bit-exact with tests/grounding_ref.py.
 *
 * HOST: attwarp_lanczos4_coeffs(n_in, n_out, ofs int32 [n_out], coeffs float [n_out,8]): the per-axis tables of
 * resizeGeneric_ (source index ofs[d] = floor((float)((d + 0.5) * n_in / n_out - 0.5)), taps ofs-3 .. ofs+4 clamped into
 * the source, interpolateLanczos4 with glibc's sin / cos).  Callers upload them once per distinct size.
 *
 * A call takes M records (a HOST array, validated here and used to size the grid, plus a DEVICE copy of the same bytes,
 * 8-byte aligned): */
typedef struct attwarp_grid_map {
  const float* src;                                /* device: grid [h,w] (resize, fused metrics) or map [H,W] (dense metrics) */
  float* out;                                      /* device: [H,W] output of attwarp_resize_lanczos4 (unused by the metrics) */
  const int32_t* ofs_x; const float* coef_x;       /* device: attwarp_lanczos4_coeffs(w, W) tables (unused when dense) */
  const int32_t* ofs_y; const float* coef_y;       /* device: attwarp_lanczos4_coeffs(h, H) tables */
  int32_t H, W;                                    /* output / map size */
  int64_t box_x, box_y, box_w, box_h;              /* metrics: the box as interpret_bbox gives it (top1's inequalities) */
  int32_t r0, r1, c0, c1;                          /* metrics: the box's numpy slice a[r0:r1, c0:c1], resolved by the caller */
} attwarp_grid_map;
/* resize: every record's src is a grid [h,w] (h, w <= 64), out its own [H,W].  H, W <= 32768, M <= 65535.
 * box metrics: fused != 0 -- src is a grid [h,w] and the value of a pixel is its LANCZOS4 value, computed on the fly
 * (the full-resolution map is never written); fused == 0 -- src is a float32 map [H,W] in memory (h, w ignored).
 * Per record: argmax (int64, row-major, np.argmax: first index among equal maxima, -0.0 == 0.0, the first NaN wins),
 * top1 (int32: box_x <= c < box_x + box_w and box_y <= r < box_y + box_h at the argmax), am (float64: sum over the slice
 * / (sum over the map + 1e-12), both sums in float64).  ws: attwarp_box_metrics_workspace_bytes(maps, M) bytes, 16-byte
 * aligned.  Deterministic (fixed-order reductions, two launches); both paths give identical bits on identical values. */
ATTWARP_API int attwarp_lanczos4_coeffs(int n_in, int n_out, int32_t* ofs, float* coeffs);
ATTWARP_API int attwarp_resize_lanczos4(const attwarp_grid_map* maps, const attwarp_grid_map* maps_dev, int M, int h, int w,
                            void* stream);
ATTWARP_API size_t attwarp_box_metrics_workspace_bytes(const attwarp_grid_map* maps, int M);
ATTWARP_API int attwarp_box_metrics(const attwarp_grid_map* maps, const attwarp_grid_map* maps_dev, int M, int fused, int h,
                        int w, int64_t* argmax, int32_t* top1, double* am, void* ws, void* stream);

/* ---- the Stable-Diffusion warp ablation (Ablations/Stable_diffusion_based_warp.py:142-172, 310-413, 445-456): the
 * cross-attention reductions behind compute_token_importance / aggregate_attention_map_for_tokens, cv2.resize(float32
 * map, INTER_CUBIC), cv2.GaussianBlur(5 x 5, sigma 1) and the in-place min-max.  Every call takes a HOST array of
 * records (validated here and used to size the grid) plus a DEVICE copy of the same bytes (8-byte aligned), M <= 65535.
 * No floating-point atomics anywhere: the same inputs give the same bits (summation orders: DESIGN.md 3.9; restated in
 * tests/sdwarp_ref.py, bit for bit).
 *
 * attwarp_xattn_reduce: one pass over every captured tensor attn [B,heads,HW,tokens] (dense, element aligned only; one
 * dtype F32 / F16 / BF16 and one tokens in 1 .. 256 per call).  Per record, in the tensor's dtype:
 *   token_sums [tokens] = attn.sum(dim=(0,1,2,3)), accumulated in float64, rounded once (float16 beyond 65504 -> inf);
 *   hw_tok [HW,tokens]  = attn.sum(dim=0).sum(dim=0): float64 over B, rounded, float64 over heads, rounded (NULL: skip).
 * A workgroup owns attwarp_xattn_chunk(tokens) consecutive positions of HW for all (b, head) and leaves float64
 * partials [tokens] in ws (attwarp_xattn_reduce_workspace_bytes bytes, 16-byte aligned); a second small launch adds a
 * record's partials in chunk order. */
typedef struct attwarp_xattn_map {
  const void* attn;                                /* device: [B,heads,HW,tokens] */
  void* token_sums;                                /* device: [tokens] */
  void* hw_tok;                                    /* device: [HW,tokens] or NULL */
  int32_t B, heads, HW;
} attwarp_xattn_map;
ATTWARP_API int attwarp_xattn_chunk(int tokens);
ATTWARP_API size_t attwarp_xattn_reduce_workspace_bytes(const attwarp_xattn_map* maps, int M, int tokens);
ATTWARP_API int attwarp_xattn_reduce(const attwarp_xattn_map* maps, const attwarp_xattn_map* maps_dev, int M, int dtype,
                         int tokens, void* ws, void* stream);

/* cv2.resize(float32 map [h,w], (W, H), INTER_CUBIC) = OpenCV 4.x resizeGeneric_ with the scalar HResizeCubic /
 * VResizeCubic for one channel: horizontal pass, then vertical pass, float32 with every product and sum rounded, taps
 * ofs-1 .. ofs+2 (clamped into the source) in ascending order from the first product; dsize == ssize copies; plain cubic
 * when down-sampling (no anti-aliasing).  Published algorithm, parity with OpenCV itself unpinned (OpenCV is absent
 * where this is built; its vectorised passes may sum in another order); bit-exact with tests/sdwarp_ref.py.
 * HOST: attwarp_cubic_coeffs(n_in, n_out, ofs int32 [n_out], coeffs float [n_out,4]): source coordinate and cvFloor split
 * as attwarp_lanczos4_coeffs, interpolateCubic in float32 with A = -0.75f.
 * The source may have any size up to 32768 x 32768: each thread keeps the horizontal results of the four source rows of
 * its column's current window and moves it as ofs_y advances; nothing is held for the whole source. */
typedef struct attwarp_cubic_map {
  const float* src;                                /* device: [h,w] */
  float* out;                                      /* device: [H,W] */
  const int32_t* ofs_x; const float* coef_x;       /* device: attwarp_cubic_coeffs(w, W) (unused when H == h and W == w) */
  const int32_t* ofs_y; const float* coef_y;       /* device: attwarp_cubic_coeffs(h, H) */
  int32_t h, w, H, W;                              /* all 1 .. 32768 */
} attwarp_cubic_map;
ATTWARP_API int attwarp_cubic_coeffs(int n_in, int n_out, int32_t* ofs, float* coeffs);
ATTWARP_API int attwarp_resize_cubic(const attwarp_cubic_map* maps, const attwarp_cubic_map* maps_dev, int M, void* stream);

/* cv2.GaussianBlur(map, (5, 5), sigmaX=1.0) of float32 maps [H,W] (:410) and the min-max of :160 / :400-401 / :411-412.
 * HOST: attwarp_gaussian5_taps(sigma, taps float [5]) = getGaussianKernel(5, sigma): exp(-i*i / (2 sigma^2)) normalised
 * in double, each tap rounded to float32.  Blur: row pass then column pass, BORDER_REFLECT_101 (sides 1 and 2 included),
 * symmetric form k0*s0 + k1*(s-1 + s1) + k2*(s-2 + s2), every operation rounded.  Published algorithm, parity with OpenCV
 * unpinned.  blur != 0: out = blur(src) (not in place); blur == 0: out is not written.  With ws != NULL every workgroup
 * leaves the min / max of what it produced (blur != 0) or read (blur == 0) in ws
 * (attwarp_blur5_minmax_workspace_bytes bytes, 8-byte aligned; NaN marks "a NaN was seen", numpy's min / max).
 * attwarp_minmax_normalize (same M and sizes as the call that filled ws): out = (src - min) / (float)(max' + 1e-9f) in
 * float32, max' the maximum after the subtraction (numpy 2 scalar rules: a constant map gives 0, a NaN gives NaN
 * everywhere); may run in place (out == src).  Two launches: the partials of a map in index order, then the map. */
typedef struct attwarp_f32_map {
  const float* src;                                /* device: [H,W] */
  float* out;                                      /* device: [H,W] */
  int32_t H, W;                                    /* 1 .. 32768 */
} attwarp_f32_map;
ATTWARP_API int attwarp_gaussian5_taps(double sigma, float* taps);
ATTWARP_API size_t attwarp_blur5_minmax_workspace_bytes(const attwarp_f32_map* maps, int M);
ATTWARP_API int attwarp_blur5_minmax(const attwarp_f32_map* maps, const attwarp_f32_map* maps_dev, int M, int blur, void* ws,
                         void* stream);
ATTWARP_API int attwarp_minmax_normalize(const attwarp_f32_map* maps, const attwarp_f32_map* maps_dev, int M, void* ws,
                             void* stream);

/* ---- A12 / A13 tail: cv2.remap(INTER_LINEAR, BORDER_REPLICATE) with separable maps,
 * AGW/new_method.py:268-271, MN/checkpoint_utils.py:195-198.
 * src [B,H,W,C] (HWC) or [B,C,H,W] (CHW), dtype F32, U8 or F64 -> dst same layout with (H_out,W_out).
 * map_x [B,W_out], map_y [B,H_out] float32 source coordinates.  C <= 4.  (F64: the dtype pass-through of
 * warp_from_cdf_torch, MN/checkpoint_utils.py:152,203 -- OpenCV's CV_64F arithmetic: float32 table weights, the four
 * products accumulated in double; generic gather kernel only.)
 * Coordinates outside the image take the replicate border.  Non-finite / huge coordinates: mode CV2 follows
 * cvRound(32 * m) of OpenCV's x86 builds (NaN, +-Inf and products outside int32 -> INT_MIN -> pixel 0, zero fraction,
 * for either sign); mode EXACT clamps the coordinate to [-1, size] first (NaN counts as -1).  No output is NaN
 * unless a source pixel is. */
ATTWARP_API int attwarp_remap_bilinear(const void* src, void* dst, int dtype, int layout, int B, int C, int H, int W,
                           int H_out, int W_out, const float* map_x, const float* map_y, int mode,
                           void* stream);

/* ---- L: the MarginalNet training losses, MN/losses.py:11-77, MN/model.py:98-106, MN/trainer.py:173-257
 * Row kernels (one 256-thread workgroup per sample, or per (sample, axis)), float32 in and out, float64 sums.
 * A loss forward writes one float32 scalar `loss` through a deterministic in-launch reduction: every workgroup stores
 * its partial into `parts` (float64 [nparts] as documented per call), the last one to draw from `ticket` sums them in
 * index order and resets *ticket to 0.  `ticket` is one uint32 that is 0 before the launch; launches sharing a ticket
 * must be stream ordered.  A backward reads the incoming gradient from the device scalar `gout` (float32) and
 * follows torch autograd's conventions at ties (DESIGN.md "training losses").
 * Row lengths: N, H, W, L <= 4096 except pdf_l1 (W, H <= 8192) and the target builders (see attwarp_gt_marginals). */
enum { ATTWARP_RECON_MSE = 0, ATTWARP_RECON_L1 = 1 };
/* trainer_attention_targets transform per sample: identity, sqrt, and "none" (identity + uniform marginals) */
enum { ATTWARP_TT_IDENTITY = 0, ATTWARP_TT_SQRT = 1, ATTWARP_TT_NONE = 2 };

/* cdf_from_density_downsample (:70-77): p [B,N] -> F [B,L].  build_axis_cdf_targets (:50-67): A [B,H,W] -> Fx, Fy
 * [B,L]; ws: attwarp_axis_sums_workspace_bytes(B,H,W) bytes.  Both forward only.  build_axis_cdf_targets keeps
 * max(H,W) + L doubles in LDS: H, W <= 16384 and L <= 4096, but not the largest of both at once (ATTWARP_E_UNSUPPORTED
 * when max(H,W) + L > 20476). */
ATTWARP_API int attwarp_cdf_downsample(const float* p, int B, int N, int L, float* F, void* stream);
ATTWARP_API int attwarp_build_axis_cdf_targets(const float* A, int B, int H, int W, int L, float* Fx, float* Fy, void* ws,
                                   void* stream);
/* l1_cdf_loss (:11-12), p, q [B,N]; parts [B].  Backward -> gp, gq [B,N]. */
ATTWARP_API int attwarp_l1_cdf_loss(const float* p, const float* q, int B, int N, double* parts, uint32_t* ticket,
                        float* loss, void* stream);
ATTWARP_API int attwarp_l1_cdf_loss_backward(const float* p, const float* q, int B, int N, const float* gout, float* gp,
                                 float* gq, void* stream);
/* sym_kl (:15-22), p, q [B,N]; parts [B].  Backward -> gp, gq [B,N]. */
ATTWARP_API int attwarp_sym_kl(const float* p, const float* q, int B, int N, float eps, double* parts, uint32_t* ticket,
                   float* loss, void* stream);
ATTWARP_API int attwarp_sym_kl_backward(const float* p, const float* q, int B, int N, float eps, const float* gout,
                            float* gp, float* gq, void* stream);
/* separable_recon_loss (kind MSE, :25-34) and recon_l1 (kind L1, :37-47): px [B,W], py [B,H], A [B,H,W]; parts [B].
 * The (B,H,W) outer product is never stored.  Backward -> gpx [B,W], gpy [B,H] (A is a target). */
ATTWARP_API int attwarp_recon_loss(const float* px, const float* py, const float* A, int B, int H, int W, int kind,
                       double* parts, uint32_t* ticket, float* loss, void* stream);
ATTWARP_API int attwarp_recon_loss_backward(const float* px, const float* py, const float* A, int B, int H, int W, int kind,
                                const float* gout, float* gpx, float* gpy, void* stream);
/* mix_with_uniform (model.py:98-101): out = c1 * p + c2 elementwise over n floats, c1 = 1 - alpha, c2 = alpha / N
 * (the backward is the same call with c2 = 0).  entropy (model.py:104-106), p [B,N]; parts [B]. */
ATTWARP_API int attwarp_scale_shift(const float* p, int64_t n, float c1, float c2, float* out, void* stream);
ATTWARP_API int attwarp_entropy(const float* p, int B, int N, float eps, double* parts, uint32_t* ticket, float* loss,
                    void* stream);
ATTWARP_API int attwarp_entropy_backward(const float* p, int B, int N, float eps, const float* gout, float* gp,
                             void* stream);
/* The trainer's image-resolution PDF loss (MN/trainer.py:216-250): px, gx [B,Lx], py, gy [B,Ly] low-resolution PDFs
 * (prediction, target) -> right-inverse up-sample to W / H (inv_x: [Lx,Lx], inv_y: [Ly,Ly] as for
 * attwarp_upsample_pdf_right_inverse), clamp_min(0), renormalise, l1_loss(x) + l1_loss(y); parts [2B].
 * Lx, Ly <= 64; W and H may be shorter than Lx and Ly (the kernels walk every window that covers an output; the table
 * is the caller's).  Backward -> gpx [B,Lx], gpy [B,Ly] (the targets get none). */
ATTWARP_API int attwarp_pdf_l1_loss(const float* px, const float* py, const float* gx, const float* gy, int B, int Lx,
                        int Ly, int W, int H, const double* inv_x, const double* inv_y, double* parts,
                        uint32_t* ticket, float* loss, void* stream);
ATTWARP_API int attwarp_pdf_l1_loss_backward(const float* px, const float* py, const float* gx, const float* gy, int B,
                                 int Lx, int Ly, int W, int H, const double* inv_x, const double* inv_y,
                                 const float* gout, float* gpx, float* gpy, void* stream);
/* The trainer's attention targets (MN/trainer.py:173-202, 220-236): A [B,H,W] float32, modes [B] int32 ATTWARP_TT_*
 * -> pooled [B,oh,ow] = sanitise(adaptive_avg_pool2d(transform(A))) (bit for bit attwarp_adaptive_avg_pool with
 * sanitize = 1 of the transformed map), px [B,ow], py [B,oh] = gt_marginals(pooled), 1/L on ATTWARP_TT_NONE rows. */
ATTWARP_API int attwarp_trainer_attention_targets(const float* A, const int32_t* modes, int B, int H, int W, int oh,
                                      int ow, float* pooled, float* px, float* py, void* stream);

/* ---- the trainer's batches from decoded samples (MN/dataloader.py:123-137, 160-189, 204-273; MN/data.py collate_str):
 * images of their own sizes -> T.Resize((S_h,S_w)) (Pillow's 8-bit BILINEAR resample, ATTWARP_PIL_BILINEAR tables) ->
 * ToTensor (float32(float64(u8) * (1/255)) == u8 / 255 in IEEE float32, channels first), stacked: out [B,C,S_h,S_w].
 *
 * As for the ragged chain, a batch is described by a table the host builds once and copies to the device unchanged:
 *   1. fill attwarp_prep_image[B] (HOST array of DEVICE pointers): image, size, Pillow tables W -> S_w and H -> S_h
 *      (attwarp_pil_coeffs_8bpc; identity tables on an axis that keeps its size: Pillow skips that pass);
 *   2. attwarp_prep_images_table_bytes(...) -> size; attwarp_prep_images_plan(...) writes header, records and the work
 *      items (image, band of output rows) into HOST memory; header.tmp_bytes is the uint8 intermediate the caller provides;
 *   3. copy table_bytes to the device (8-byte aligned); 4. attwarp_prep_images_u8(host copy, device copy, tmp, out, stream).
 * An image runs on the one-launch kernel (both passes, the uint8 intermediate in LDS) when its horizontal taps fit the
 * 16-tap register window, a band of 8 output rows fits the LDS and the horizontal pass comes first; the others (and every image in the tuning library under
 * prep_variant = 1) take two more launches with the intermediate in `tmp`.  Both compute the same bytes.
 * Images with 9 .. 16 horizontal taps run as a second launch of the same kernel with the wider window (n_wide_items).
 * The LDS rows of a band are bounded on the host from H, S_h and ksize_y, which holds for the tables of
 * attwarp_pil_coeffs_8bpc; a band whose tables reach further is written as NaN, never computed from clamped taps.
 * Limits: C 1 or 3, S_w * C <= 65536, H, W <= 65535, B <= 2^20. */
typedef struct attwarp_prep_image {
  const uint8_t* image;                            /* device: [H,W,C] uint8 interleaved, any byte address */
  const int32_t* bounds_x; const int32_t* kk_x;    /* device: W -> S_w: int32 [S_w,2], int32 [S_w,ksize_x] */
  const int32_t* bounds_y; const int32_t* kk_y;    /* device: H -> S_h: int32 [S_h,2], int32 [S_h,ksize_y] */
  int32_t H, W, ksize_x, ksize_y;
  int32_t vertical_first, reserved;                /* 1: vertical pass first (what PIL.Image.resize does when H > 100 * W and
                                                      S_h < H); such an image takes the two-launch route */
} attwarp_prep_image;
typedef struct attwarp_prep_header {               /* first bytes of a table written by attwarp_prep_images_plan */
  uint32_t magic;
  int32_t B, C, S_h, S_w;
  int32_t n_fused_images, n_fused_items;           /* images / (image, band) items of the one-launch kernel */
  int32_t n_split_images, n_h_items, n_v_items;    /* the two-launch route: its images, row-block items of either pass */
  int32_t ks;                                      /* widest register window of the batch: 8 or 16 taps */
  int32_t n_wide_items;                            /* the last n_wide_items of n_fused_items belong to images with 9 .. 16
                                                      horizontal taps: they run as a launch of their own on the 16-tap window */
  uint64_t table_bytes, tmp_bytes, lds_bytes;
  uint64_t off_images, off_items;
} attwarp_prep_header;
ATTWARP_API size_t attwarp_prep_images_table_bytes(const attwarp_prep_image* images, int B, int C, int S_h, int S_w);
ATTWARP_API int attwarp_prep_images_plan(const attwarp_prep_image* images, int B, int C, int S_h, int S_w, void* table,
                             size_t table_bytes);
ATTWARP_API int attwarp_prep_images_u8(const void* table_host, const void* table_dev, uint8_t* tmp, float* out, void* stream);

/* HOST: the source index of every output position of Pillow's NEAREST resize n_in -> n_out (the affine scale path:
 * a = n_in / n_out in double, xo = a * 0.5, idx = floor(xo), xo += a -- accumulated, which the closed form does not equal). */
ATTWARP_API int attwarp_pil_nearest_index(int n_in, int n_out, int32_t* idx);

/* The attention maps of the same samples (MN/dataloader.py:178-189, 230-231): float32 maps of their own sizes -> (if
 * normalize and max > 1: / max in float32; a NaN anywhere makes the max NaN, so nothing is divided) -> NaN, +-inf -> 0 ->
 * clip(0,1) -> trunc(v * 255) -> NEAREST resize by the index tables -> / 255: out [B,1,S_h,S_w] float32.  normalize = 0
 * (the overlay branch, values gray / 255) skips only the division.  ws: attwarp_prep_attention_workspace_bytes(B) bytes. */
typedef struct attwarp_prep_attention {
  const float* map;                                /* device: [h,w] float32, dense */
  const int32_t* idx_x; const int32_t* idx_y;      /* device: int32 [S_w], int32 [S_h] (attwarp_pil_nearest_index) */
  int32_t h, w, normalize, reserved;
} attwarp_prep_attention;
ATTWARP_API size_t attwarp_prep_attention_workspace_bytes(int B);
ATTWARP_API int attwarp_prep_attention_f32(const attwarp_prep_attention* maps_dev, int B, int S_h, int S_w, void* ws, float* out,
                               void* stream);

/* ---- the first visit to CLIP (AGW/attention_extraction/functions.py:262-271: LLaVA's process_images on a batch of images
 * of their own sizes): per image expand2square (image_aspect_ratio == "pad") or nothing, the HF CLIPImageProcessor's PIL
 * BICUBIC resize, centre crop to size x size, float32(float64(u8) * (1/255)), (x - mean) / std in float32, channels first:
 * out [B,C,size,size] float32 or float16 (the float32 value rounded once), bit for bit what Pillow + the processor compute.
 *
 * The table pattern of attwarp_prep_images_*:
 *   1. fill attwarp_clip_image[B] (HOST array of DEVICE pointers).  The source Pillow resizes is a canvas_w x canvas_h
 *      canvas of the background colour with the image at (pad_x, pad_y) -- the canvas is never stored, taps outside the
 *      image read the background -- or, without padding, the image itself (canvas == image, pads 0).  Tables:
 *      attwarp_pil_coeffs_8bpc(canvas_w, nw, ATTWARP_PIL_BICUBIC, ...) and (canvas_h, nh, ...), identity tables on an axis
 *      that keeps its size (Pillow skips that pass); (left, top) is the crop's origin in the nh x nw resized image;
 *   2. attwarp_clip_images_table_bytes(...) -> size; attwarp_clip_images_plan(...) writes header, records and the work
 *      items (image, band of output rows) into HOST memory; header.tmp_bytes is the uint8 intermediate the caller provides;
 *   3. copy table_bytes to the device (8-byte aligned); 4. attwarp_clip_images_u8(host copy, device copy, ...).
 * An image runs on the one-launch kernel (both passes, the uint8 intermediate in LDS) when its horizontal taps fit the
 * 16-tap register window (canvas_w <= 3.5 nw: 1176 -> 336), a band of 8 output rows fits the LDS and the horizontal pass
 * comes first; images with 9 .. 16 taps run as a second launch of that kernel (n_wide_items).  The others (and every image
 * in the tuning library under clip_ragged_variant = 1) take two launches with the intermediate in `tmp`.  Both routes
 * compute the same bytes.  The LDS rows of a band are bounded on the host from canvas_h, nh and ksize_y, which holds for
 * the tables of attwarp_pil_coeffs_8bpc; a band whose tables reach further is written as NaN, never computed from clamped
 * taps.
 * Limits (ATTWARP_E_UNSUPPORTED from the plan, with a message): C 1 or 3, canvas_w, canvas_h <= 8192, size <= 4096,
 * nw, nh <= 2^20, B <= 2^20.  A vertical-first image cannot be padded (a padded canvas is square). */
typedef struct attwarp_clip_image {
  const uint8_t* image;                            /* device: [H,W,C] uint8 interleaved, any byte address */
  const int32_t* bounds_x; const int32_t* kk_x;    /* device: canvas_w -> nw: int32 [nw,2], int32 [nw,ksize_x] */
  const int32_t* bounds_y; const int32_t* kk_y;    /* device: canvas_h -> nh: int32 [nh,2], int32 [nh,ksize_y] */
  int32_t H, W, ksize_x, ksize_y;
  int32_t pad_x, pad_y;                            /* where the image's first pixel lies on the canvas */
  int32_t canvas_w, canvas_h;
  int32_t nw, nh;                                  /* size the canvas is resized to */
  int32_t left, top;                               /* origin of the size x size crop in the resized image */
  int32_t vertical_first, reserved;                /* 1: vertical pass first (what PIL.Image.resize does when H > 100 * W and
                                                      nh < H); such an image takes the two-launch route */
} attwarp_clip_image;
typedef struct attwarp_clip_header {               /* first bytes of a table written by attwarp_clip_images_plan */
  uint32_t magic;
  int32_t B, C, size;
  int32_t n_fused_images, n_fused_items;           /* images / (image, band) items of the one-launch kernel */
  int32_t n_wide_items;                            /* the last n_wide_items of n_fused_items: images with 9 .. 16 horizontal taps */
  int32_t n_split_images, n_h_items, n_v_items;    /* the two-launch route: its images, row-block items of either pass */
  int32_t ks, reserved;                            /* widest register window of the batch: 8 or 16 taps */
  uint64_t table_bytes, tmp_bytes, lds_bytes;
  uint64_t off_images, off_items;
} attwarp_clip_header;
ATTWARP_API size_t attwarp_clip_images_table_bytes(const attwarp_clip_image* images, int B, int C, int size);
ATTWARP_API int attwarp_clip_images_plan(const attwarp_clip_image* images, int B, int C, int size, void* table,
                             size_t table_bytes);
/* mean, stdv: HOST, C floats each; background: HOST, C bytes (read only where an image is padded); tmp: header.tmp_bytes
 * bytes (may be NULL when that is 0); out: 16-byte aligned; out_dtype ATTWARP_F32 or ATTWARP_F16. */
ATTWARP_API int attwarp_clip_images_u8(const void* table_host, const void* table_dev, const float* mean, const float* stdv,
                           const uint8_t* background, uint8_t* tmp, void* out, int out_dtype, void* stream);

/* ---- the trainer's optimiser step (MN/trainer.py:259-264): GradScaler unscale, global L2 gradient norm, clip and
 * torch.optim.AdamW (decoupled weight decay, no amsgrad, no maximize) in two kernels per group of 64 tensors.
 *   g = g_raw * inv_scale, inv_scale = float32(1 / float64(*grad_scale)) (1 when grad_scale is NULL);
 *   total_norm = sqrt(sum g^2) over every tensor of the call, x^2 accumulated in float64 in a fixed order;
 *   coef = min(max_norm / (total_norm + norm_eps), 1) (1 when max_norm < 0), g = g * coef;
 *   p = p * (1 - lr * wd);  m = lerp(m, g, w1) with w1 = 1 - beta1 as torch.lerp takes it: m + w1 * (g - m) for w1 < 0.5,
 *   g - (g - m) * (1 - w1) from 0.5 on (beta1 <= 0.5; 1 - w1 in float32);  v = beta2 * v + (1 - beta2) * g * g;
 *   p = p - lr / (1 - beta1^t) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)),  t = steps[step_slot] + 1 (stored back).
 * Every float32 operation is rounded on its own; the scalars that depend on t, lr and the betas are computed in float64
 * and rounded once.  When found_inf is not NULL and *found_inf != 0 nothing is written but grad_norm (p, m, v and steps
 * keep their bits).  Gradients are only read.  grad_norm (float32, device) receives total_norm.
 * `tensors` is a HOST array of n records of DEVICE pointers; p, g, m, v are dense float32 arrays of numel elements at
 * any 4-byte aligned address (16-byte loads and stores when all four of a tensor are 16-byte aligned).  steps: device
 * float32 array indexed by step_slot (0 <= step_slot < the n_tensors the workspace was sized for).  The workspace is
 * attwarp_adamw_workspace_bytes(total_numel, n_tensors) bytes for calls whose numel sum to at most total_numel, ZERO
 * before its first use, 16-byte aligned, and handed over with the SAME workspace_bytes every call; calls sharing it
 * must be stream ordered.  Nothing is allocated, nothing synchronises; 2 * ceil(n / 64) launches. */
typedef struct attwarp_adamw_tensor {
  float* p; const float* g; float* m; float* v;    /* device */
  int64_t numel;
  double lr, beta1, beta2, eps, weight_decay;
  int32_t step_slot, reserved;
} attwarp_adamw_tensor;
ATTWARP_API size_t attwarp_adamw_workspace_bytes(int64_t total_numel, int n_tensors);
ATTWARP_API int attwarp_adamw_step(const attwarp_adamw_tensor* tensors, int n, double max_norm, double norm_eps,
                       const float* grad_scale, const float* found_inf, float* steps, float* grad_norm,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- PNG files of a whole batch of differently sized uint8 images, encoded on the device (png.hip):
 * what the reference's drivers write per sample with cv2.imwrite (main_batched.py:243-303, new_method.py:405-506).
 * 8-bit grey (C = 1) or RGB (C = 3), non-interlaced; signature, IHDR, ONE IDAT, IEND.  The zlib stream is 78 01, then
 * per SEGMENT (whole rows: at most ATTWARP_PNG_SEG_BYTES filtered bytes and ATTWARP_PNG_SEG_MAX_ROWS rows) one
 * dynamic-Huffman block of literals and distance-1 matches followed by an empty stored block, which ends the segment on
 * a byte boundary -- or one stored block where that is shorter --, then 01 00 00 FF FF and the Adler-32.  One workgroup
 * encodes one segment; sizes, offsets, Adler-32 and the IDAT CRC-32 are combined on the device, so a call's launches
 * depend on nothing the host has to read back and can be captured in a graph.
 *   1. fill attwarp_png_image[B] (HOST array of DEVICE pointers);
 *   2. attwarp_png_table_bytes -> size; attwarp_png_plan writes header, records and segments into HOST memory;
 *   3. copy table_bytes to the device (8-byte aligned);
 *   4. attwarp_png_encode(host copy, device copy, scratch of header.scratch_bytes (16-byte aligned), out of at least
 *      header.out_bytes, offsets int64 [B+1], stream): file b is out[offsets[b] .. offsets[b+1]), files back to back.
 * header.out_bytes is the sum of attwarp_png_bound(H, W, C) over the batch: every segment stored.
 * Filters: the specification's five, and ADAPTIVE: per row the filter with the smallest sum of |filtered byte as int8|,
 * ties to the lower number.  order = ATTWARP_BGR swaps the channels of a 3-channel source while filtering (the file is RGB).
 * Limits (ATTWARP_E_UNSUPPORTED from the planner): 1 + W * C <= ATTWARP_PNG_MAX_ROW_BYTES, C 1 or 3, a file bound below
 * 2^31, at most 2^24 segments per call; pitch >= W * C is the distance between rows in bytes, any byte address.
 * The _ex planners take match[B] (or NULL: all ATTWARP_PNG_MATCH_RLE, the table of the plain planners byte for byte; any
 * other value is ATTWARP_E_INVALID).  The segments of an ATTWARP_PNG_MATCH_LZ image are encoded by a
 * second kernel, launched only when the table has such segments: it also looks for matches of 4 .. 258 bytes at distance
 * 2 .. 24,572 INSIDE the segment (one hashed candidate per position from the earlier 256-position blocks, greedy parse,
 * HDIST = 30) and writes per segment the shortest of the distance-1 block above, that block and the stored block -- so
 * the file is never longer, a segment where distance 1 wins carries the same bytes, and segments stay independent.
 * header.reserved is the number of such segments; bound, scratch size and the other two launches do not change. */
#define ATTWARP_PNG_SEG_BYTES 24576
#define ATTWARP_PNG_MAX_ROW_BYTES 24576
#define ATTWARP_PNG_SEG_MAX_ROWS 1024
#define ATTWARP_PNG_FILE_OVERHEAD 68  /* bytes of a file that belong to no segment */
enum { ATTWARP_PNG_NONE = 0, ATTWARP_PNG_SUB = 1, ATTWARP_PNG_UP = 2, ATTWARP_PNG_AVERAGE = 3, ATTWARP_PNG_PAETH = 4,
       ATTWARP_PNG_ADAPTIVE = 5 };
enum { ATTWARP_PNG_MATCH_RLE = 0, ATTWARP_PNG_MATCH_LZ = 1 };
typedef struct attwarp_png_image {
  const uint8_t* src;                              /* device: H rows of W * C bytes, pitch bytes apart */
  int32_t H, W, C;
  int32_t pitch;
  int32_t order;                                   /* ATTWARP_RGB / ATTWARP_BGR (ignored for C = 1) */
  int32_t filter;                                  /* ATTWARP_PNG_* */
} attwarp_png_image;
typedef struct attwarp_png_header {                /* first bytes of a table written by attwarp_png_plan */
  uint32_t magic;
  int32_t B, nseg, reserved;                       /* reserved: segments of ATTWARP_PNG_MATCH_LZ images */
  uint64_t table_bytes, scratch_bytes, out_bytes;
  uint64_t off_images, off_segs;
  uint32_t crc_pow8[32];                           /* x^(8 * 2^k) mod the CRC-32 polynomial, reflected */
  uint32_t idat_head_crc, reserved2;               /* CRC-32 of "IDAT" 78 01 */
} attwarp_png_header;
ATTWARP_API size_t attwarp_png_bound(int H, int W, int C);   /* 0: outside the limits */
ATTWARP_API size_t attwarp_png_table_bytes(const attwarp_png_image* images, int B);
ATTWARP_API int attwarp_png_plan(const attwarp_png_image* images, int B, void* table, size_t table_bytes);
ATTWARP_API size_t attwarp_png_table_bytes_ex(const attwarp_png_image* images, int B, const int32_t* match);
ATTWARP_API int attwarp_png_plan_ex(const attwarp_png_image* images, int B, const int32_t* match, void* table, size_t table_bytes);
ATTWARP_API int attwarp_png_encode(const void* table_host, const void* table_dev, void* scratch, uint8_t* out, size_t out_bytes,
                       int64_t* offsets, void* stream);

/* ---- The trainer's debug and validation panels (panel.hip): MN/trainer.py:301-307 and :484-517 --
 * heat = A / (A.amax + 1e-6) up-sampled with F.interpolate(bilinear, align_corners=False), torch.cat of the first n
 * samples of every row, (grid * 255).byte() and torchvision.utils.make_grid -- as ONE launch into one uint8 canvas.
 * sources: HOST array of nsrc <= ATTWARP_PANEL_MAX_SRC records; source r contributes its first n images as cells
 * r*n .. r*n + n-1.  Planes are dense ([C,H,W] per image), images are batch_stride ELEMENTS apart (a slice of a larger
 * batch needs no copy).  Kinds:
 *   ATTWARP_PANEL_F32  float32 [N,C,H,W], C 3 or 1 (one channel fills all three): byte = (unsigned char)(v * 255.0f), one
 *                      rounded float32 product truncated toward zero; clamp != 0 clamps v to [0, 1] first;
 *   ATTWARP_PANEL_U8   uint8 [N,C,H,W], C 3 or 1: copied;
 *   ATTWARP_PANEL_HEAT float32 [N,1,h,w], h * w <= ATTWARP_PANEL_MAX_HEAT, h and w independent of H and W: per image
 *                      m = max(A) (a NaN propagates), q = A / (m + 1e-6f), then torch's bilinear with align_corners=False in
 *                      individually rounded float32 operations -- scale = (float)in / (float)out,
 *                      src = max(scale * (dst + 0.5f) - 0.5f, 0), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0,
 *                      l0 = 1 - l1, v = l0y * (l0x * q00 + l1x * q01) + l1y * (l0x * q10 + l1x * q11) -- and the byte of
 *                      v * 255.0f as above, in all three channels.  q lives in LDS only.
 * Values: the byte is torch's wherever (t).byte() is defined (-1 < t < 256); t <= -1 gives 0, t >= 256 gives 255, NaN
 * gives 0 (a heat image whose maximum is NaN or +inf is all zeros).
 * Geometry (torchvision.utils.make_grid): K = nsrc * n cells, xmaps = min(nrow, K), ymaps = ceil(K / xmaps); cell k at
 * row k / xmaps, column k % xmaps of a canvas of Hg x Wg = (ymaps * (H + padding) + padding) x (xmaps * (W + padding) +
 * padding) filled with pad_value, each cell offset by padding; K == 1 gives the bare image (no padding).
 * out: layout ATTWARP_HWC [Hg, Wg + right_margin, 3] or ATTWARP_CHW [3, Hg, Wg + right_margin] uint8, any byte address;
 * the right_margin columns hold pad_value.  flags: ATTWARP_PANEL_FOR_PNG refuses a canvas whose HWC row does not fit the
 * PNG encoder (1 + 3 * (Wg + right_margin) > ATTWARP_PNG_MAX_ROW_BYTES).  Every limit is refused before anything is
 * enqueued; no argument depends on device data, so a call can be captured in a graph. */
#define ATTWARP_PANEL_MAX_SRC 8
#define ATTWARP_PANEL_MAX_HEAT 4096   /* h * w of a heat source: one float32 tile in LDS */
#define ATTWARP_PANEL_FOR_PNG 1
enum { ATTWARP_PANEL_F32 = 0, ATTWARP_PANEL_U8 = 1, ATTWARP_PANEL_HEAT = 2 };
typedef struct attwarp_panel_source {
  const void* data;                                /* device: image 0 of the source */
  int64_t batch_stride;                            /* elements between images, >= C * H * W (heat: >= h * w) */
  int32_t kind;                                    /* ATTWARP_PANEL_* */
  int32_t C;                                       /* 3 or 1 (heat: 1) */
  int32_t N;                                       /* images the source holds, >= n */
  int32_t h, w;                                    /* heat: the map's size (other kinds: ignored) */
  int32_t clamp;                                   /* ATTWARP_PANEL_F32: clamp to [0, 1] before the product */
} attwarp_panel_source;
ATTWARP_API int attwarp_panel_grid(const attwarp_panel_source* sources, int nsrc, int n, int H, int W, int nrow, int padding,
                       int pad_value, int layout, int right_margin, int flags, uint8_t* out, void* stream);

/* ---- PNG files of a whole batch DECODED on the device (pngdec.hip): the reading half of attwarp_png_*.
 * 8-bit, non-interlaced, colour types 0 (grey), 2 (RGB), 4 (grey + alpha), 6 (RGBA).  The HOST walks the chunks only and
 * packs the IDAT payloads of all files back to back into one buffer, so every image's zlib stream is contiguous; the
 * device inflates (all of RFC 1951), verifies zlib header, Adler-32, final size and, with check_crc, the CRC-32 of every
 * IDAT chunk, undoes the five filters and converts.
 *   1. fill attwarp_pngdec_image[B] and attwarp_pngdec_chunk[nchunks] (HOST arrays, offsets into the packed stream buffer);
 *   2. attwarp_pngdec_table_bytes -> size; attwarp_pngdec_plan writes header, records and chunks into HOST memory;
 *   3. copy the table (8-byte aligned) and header.stream_bytes packed stream bytes to the device;
 *   4. attwarp_pngdec_decode(host copy, device copy, the packed stream, scratch of header.scratch_bytes (16-byte
 *      aligned), out of at least header.out_bytes, status int32 [B], stream): image b is the dense [H, W, out_channels]
 *      block at out + sum of the blocks before it; status[b] is ATTWARP_PNGDEC_OK or the FIRST failing check in the order
 *      CRC, inflate (the codes from ZLIB_HEADER to UNDERFLOW), ADLER, FILTER.  A failing image touches nothing but its own
 *      scratch and output block, whose content is then unspecified; the other images are unaffected.
 * mode: ATTWARP_PNGDEC_RGB (3 channels: grey replicated, alpha dropped), ATTWARP_PNGDEC_L (1 channel: colour files give
 * (19595 R + 38470 G + 7471 B + 32768) >> 16, Pillow's), ATTWARP_PNGDEC_KEEP (the file's channels without alpha).  order =
 * ATTWARP_BGR swaps the channels of a 3-channel output.
 * Sync points: per image the stream's start and the first ATTWARP_PNGDEC_MAX_UNITS - 1 byte positions behind a
 * 00 00 FF FF start one decoding unit (one workgroup) each; a 1024 x 1024 x 3 file of attwarp_png_encode has 147 segments
 * and 149 such positions.  Later positions are ignored: the last kept unit decodes on to the end.
 * Limits (ATTWARP_E_UNSUPPORTED from the planner): 1 + W * channels <= ATTWARP_PNGDEC_MAX_ROW_BYTES (the unfilter kernel
 * keeps one row in LDS); H * (1 + W * channels) and an image's stream below 2^31 bytes (positions inside an image are
 * uint32; offsets between images are uint64); at most 2^20 images and 2^26 chunks per call.  No launch depends on
 * anything the host reads back: a call can be captured in a graph. */
#define ATTWARP_PNGDEC_MAX_UNITS 256
#define ATTWARP_PNGDEC_MAX_ROW_BYTES 49152
enum { ATTWARP_PNGDEC_RGB = 0, ATTWARP_PNGDEC_L = 1, ATTWARP_PNGDEC_KEEP = 2 };
enum { ATTWARP_PNGDEC_OK = 0,
       ATTWARP_PNGDEC_E_CRC = 1,           /* an IDAT chunk's CRC-32 */
       ATTWARP_PNGDEC_E_ZLIB_HEADER = 2,   /* CM / CINFO / FCHECK / FDICT */
       ATTWARP_PNGDEC_E_TRUNCATED = 3,     /* a read past the stream's end (the Adler-32's four bytes included) */
       ATTWARP_PNGDEC_E_BLOCK_TYPE = 4,    /* BTYPE 3 */
       ATTWARP_PNGDEC_E_STORED_LEN = 5,    /* LEN != ~NLEN */
       ATTWARP_PNGDEC_E_CODE_LENGTHS = 6,  /* over-subscribed or incomplete set, bad repeat, too many symbols, no end of block */
       ATTWARP_PNGDEC_E_SYMBOL = 7,        /* bits that are no code of the table, length symbol > 285, distance symbol > 29 */
       ATTWARP_PNGDEC_E_DISTANCE = 8,      /* a match that starts before the first byte */
       ATTWARP_PNGDEC_E_OVERFLOW = 9,      /* more than H * (1 + W * channels) bytes */
       ATTWARP_PNGDEC_E_UNDERFLOW = 10,    /* fewer */
       ATTWARP_PNGDEC_E_ADLER = 11,
       ATTWARP_PNGDEC_E_FILTER = 12 };     /* a filter byte above 4 */
typedef struct attwarp_pngdec_image {
  uint64_t stream_off;                             /* the image's zlib stream in the packed buffer */
  uint64_t stream_len;
  int32_t H, W;
  int32_t color_type;                              /* 0, 2, 4, 6 (attwarp_pngdec_plan_formats: 3 too) */
  int32_t mode;                                    /* ATTWARP_PNGDEC_RGB / L / KEEP */
  int32_t order;                                   /* ATTWARP_RGB / ATTWARP_BGR */
  int32_t reserved;
} attwarp_pngdec_image;
typedef struct attwarp_pngdec_chunk {              /* one IDAT chunk: its payload in the packed buffer, the CRC-32 the file states */
  uint64_t off;
  uint32_t len, crc;
  int32_t image, reserved;
} attwarp_pngdec_chunk;
typedef struct attwarp_pngdec_header {             /* first bytes of a table written by attwarp_pngdec_plan */
  uint32_t magic;
  int32_t B, nchunks, check_crc;
  int32_t lds_bytes, formats;                      /* formats: 1 in a table of attwarp_pngdec_plan_formats that needs the formats kernel */
  uint64_t table_bytes, scratch_bytes, out_bytes, stream_bytes;
  uint64_t off_images, off_chunks;
  uint32_t crc_pow8[32];
  uint32_t idat_crc, reserved2;                    /* CRC-32 of "IDAT" */
} attwarp_pngdec_header;
ATTWARP_API size_t attwarp_pngdec_table_bytes(const attwarp_pngdec_image* images, int B, int nchunks);
ATTWARP_API int attwarp_pngdec_plan(const attwarp_pngdec_image* images, int B, const attwarp_pngdec_chunk* chunks, int nchunks,
                       int check_crc, void* table, size_t table_bytes);
ATTWARP_API int attwarp_pngdec_decode(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                       uint8_t* out, size_t out_bytes, int32_t* status, void* stream);

/* ---- every format of the PNG specification: attwarp_pngdec_format[B] stands parallel to the image array
 * and adds what IHDR and PLTE say besides.  Accepted: grey at 1 / 2 / 4 / 8 / 16 bits, palette (color_type 3) at 1 / 2 / 4 / 8,
 * RGB, grey + alpha and RGBA at 8 / 16, each with interlace 0 or 1 (Adam7).  The two planners are host-only and depend on
 * IHDR, PLTE and the chunk lengths alone; the table goes to attwarp_pngdec_decode like any other.  When every image is 8-bit,
 * non-interlaced and no palette file, table and launches are attwarp_pngdec_plan's, byte for byte; otherwise the header's
 * `formats` is 1, EVERY image of the call is unfiltered by pngdec_unfilter_formats_kernel (one wave per image and pass) and a
 * closing launch states the statuses: nine launches, still none that depends on anything read back.
 * Pixels are Pillow's Image.open(f).convert(mode), bit for bit: samples below 8 bits are MSB first and grey ones scaled by
 * 255 / 85 / 17; 16-bit GREY (colour type 0) SATURATES, min(v, 255), as Pillow's I;16 does (256 -> 255); every other 16-bit
 * sample gives its high byte (grey + alpha included); a palette index is looked up in PLTE, one at or past palette_entries
 * is (0, 0, 0), and L is the luma of the entry; tRNS and alpha are dropped.  ATTWARP_PNGDEC_KEEP: the file's channels
 * without alpha at 8 bits by these rules, a palette file its palette's three; ATTWARP_BGR swaps any 3-channel result.
 * A filtered row is 1 + ceil(w * channels * depth / 8) bytes, the filters' unit max(1, channels * depth / 8) bytes; the
 * filtered size is the sum over the passes (w = ceil((W - x0) / dx), h = ceil((H - y0) / dy), an empty pass has no bytes),
 * and that is what E_OVERFLOW / E_UNDERFLOW compare with.  A filter byte above 4 in ANY pass is E_FILTER.
 * Limits (ATTWARP_E_UNSUPPORTED): 1 + ceil(W * channels * depth / 8) <= ATTWARP_PNGDEC_MAX_ROW_BYTES; the filtered size
 * below 2^31.  ATTWARP_E_ARG: a depth / colour-type pair outside the list, interlace above 1, a palette file without
 * 1 .. 256 entries. */
typedef struct attwarp_pngdec_format {
  int32_t depth;                                   /* IHDR's bit depth */
  int32_t interlace;                               /* 0, or 1: Adam7 */
  int32_t palette_entries;                         /* PLTE's length / 3 (colour type 3: 1 .. 256; otherwise ignored) */
  int32_t reserved;
  uint8_t palette[768];                            /* R, G, B per entry */
} attwarp_pngdec_format;
ATTWARP_API size_t attwarp_pngdec_table_bytes_formats(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B,
                       const attwarp_pngdec_chunk* chunks, int nchunks);
ATTWARP_API int attwarp_pngdec_plan_formats(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B,
                       const attwarp_pngdec_chunk* chunks, int nchunks, int check_crc, void* table, size_t table_bytes);

/* ---- the wave route: the same table as attwarp_pngdec_plan (formats == NULL) or attwarp_pngdec_plan_formats,
 * with header.reserved2 = 1 | segment_bytes << 8 | max_rounds << 20 and B records of four uint32 (windows, rounds, accepted,
 * resolution rounds) added at the END of the scratch buffer.  attwarp_pngdec_decode then launches pngdec_wave_kernel between
 * the chain and the write pass: one wave per image of the serial route (no sync point, a dependent unit, more than
 * ATTWARP_PNGDEC_MAX_UNITS units) inflates the one stream with all 64 lanes, segments of segment_bytes (16, 32, 64, 128 or
 * 256) stream bytes per lane, at most max_rounds (1 .. 64) rounds per window of 64 segments.  An image that does not check
 * out (rounds, an error on the true chain, a match before the first byte, the size, the Adler-32's place) is decoded by the
 * serial route from the stream's start as without this planner, so pixels, filtered bytes and statuses are the same; the
 * wave route never sets a status.  Streams of 2^28 bytes or more stay on the serial route. */
ATTWARP_API size_t attwarp_pngdec_table_bytes_wave(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B,
                       const attwarp_pngdec_chunk* chunks, int nchunks);
ATTWARP_API int attwarp_pngdec_plan_wave(const attwarp_pngdec_image* images, const attwarp_pngdec_format* formats, int B,
                       const attwarp_pngdec_chunk* chunks, int nchunks, int check_crc, int segment_bytes, int max_rounds,
                       void* table, size_t table_bytes);

/* ---- baseline JPEG files of a whole batch DECODED on the device (jpegdec.hip).  SOF0 / SOF1 (sequential
 * Huffman, 8 bits), one component (grey) or three (YCbCr, luma 1x1, 2x1 or 2x2 and chroma 1x1: 4:4:4, 4:2:2, 4:2:0), one
 * interleaved scan.  The HOST walks the marker segments only and packs, per file, everything behind the SOS header into
 * one buffer; the device finds the restart markers, decodes the entropy data (one wave per restart interval),
 * dequantises, runs libjpeg's integer IDCT, "fancy" chroma up-sampling and YCbCr -> RGB: the pixels of
 * Pillow's Image.open(f).convert(mode), bit for bit.
 *   1. fill attwarp_jpegdec_image[B] (a HOST array: sizes, sampling, the tables the scan names, resolved per component);
 *   2. attwarp_jpegdec_table_bytes -> size; attwarp_jpegdec_plan writes header and records into HOST memory;
 *   3. copy the table (8-byte aligned) and header.stream_bytes packed bytes to the device;
 *   4. attwarp_jpegdec_decode(host copy, device copy, the packed bytes, scratch of header.scratch_bytes (256-byte
 *      aligned), out of at least header.out_bytes, status int32 [B], stream): five launches, none with an argument that
 *      depends on anything read back, so a call can be captured in a graph.  Image b is the dense [H, W, out_channels]
 *      block at out + sum of the blocks before it.
 * Units: with a restart interval Ri an image has ceil(MCUs / Ri) units (else one), known from the headers; the k-th restart
 * marker of the data starts unit k + 1.  The data ends at the first FF that is followed by neither 00 nor D0..D7.
 * status[b], in this precedence: E_RESTART (the markers in front of the data's end do not number units - 1 with indices
 * cycling 0..7; nothing is resynchronised and no unit is decoded), then the status of the LOWEST failing unit
 * (E_TRUNCATED: a code or value needs bits behind the unit's end, which read as zero; E_HUFFMAN: 16 bits that start no
 * code; E_COEFF: a run that leaves coefficient 63), then E_NO_EOI (the marker behind the data is not EOI; fill bytes are
 * skipped).  Bytes between the last MCU and the next marker are tolerated.  A failing image touches nothing but its own
 * scratch and output block, whose content is then unspecified.
 * Hostile values: the DC predictor is a 32-bit sum that wraps; the coefficient stored is its low 16 bits; dequantisation
 * and IDCT are 32-bit with wrap-around; the final clamp to 0..255 saturates.  Every file gets the same pixels on every run.
 * mode: ATTWARP_JPEGDEC_RGB (3 channels, grey replicated), ATTWARP_JPEGDEC_L (1 channel: colour files give
 * (19595 R + 38470 G + 7471 B + 32768) >> 16 of the RGB pixel, grey files the plane), ATTWARP_JPEGDEC_KEEP (1 or 3).
 * order = ATTWARP_BGR swaps a 3-channel output.
 * Sub-streams (attwarp_jpegdec_plan_ex; attwarp_jpegdec_plan plans without them): an image of ONE unit (no restart
 * interval, or one of at least all its MCUs) whose data is at least two segments of segment_bytes long (and at most 16384
 * of them) is cut into such segments, known from the headers and the length alone.  The second of the five launches gives
 * it one workgroup (the launch always happens; header.reserved holds the workgroups that have work).  A lane decodes a
 * segment from a guessed state (a block starts at the segment's first byte), and every round hands each segment's exit
 * state (position in the raw stream, block of the MCU, coefficient index) to the next segment as its entry, until no
 * entry changes: after round r segments 0..r enter where a sequential decoder would, so a fixed point is the sequential
 * decode.  A decoder that meets an invalid code goes on one bit later, so a wrong guess falls in step instead of dying.
 * The unit is ACCEPTED only if the rounds end within max_rounds, block MCUs x blocks-per-MCU - 1 ends inside the data,
 * no segment up to that one met an error in front of it, and every entry's block slot follows from the count of blocks in
 * front of it; then the blocks are written with their true indices and DC predictors, and the one-wave-per-unit kernel
 * skips the image.  FALLBACK: any other image, a rejected one included, is decoded by that kernel exactly as without
 * sub-streams; the sub-stream path never sets a status, so status[] and the pixels do not depend on the plan.  The time
 * of a workgroup is bounded by max_rounds x ceil(segments / 256) segment decodes.  Scratch: the states stay at offset 0;
 * per image 16 bytes (uint32 segments planned, rounds run, accepted, 0), written on every run, lie at the offset held
 * in the sub-stream records, which follow the image records in the table (one per image, always present).
 * Limits (ATTWARP_E_UNSUPPORTED from the planner): at most ATTWARP_JPEGDEC_MAX_UNITS units and fewer than
 * ATTWARP_JPEGDEC_MAX_BLOCKS 8x8 blocks per image (offsets inside an image stay below 2^31: 128 bytes of coefficients
 * per block), an image's data below 2^31 bytes, at most 2^20 images and 2^30 units per call. */
#define ATTWARP_JPEGDEC_MAX_UNITS 65536
#define ATTWARP_JPEGDEC_MAX_BLOCKS 16777216
enum { ATTWARP_JPEGDEC_RGB = 0, ATTWARP_JPEGDEC_L = 1, ATTWARP_JPEGDEC_KEEP = 2 };
enum { ATTWARP_JPEGDEC_OK = 0,
       ATTWARP_JPEGDEC_E_TRUNCATED = 1,    /* a code or value needs bits behind the unit's end */
       ATTWARP_JPEGDEC_E_HUFFMAN = 2,      /* no code of <= 16 bits matches */
       ATTWARP_JPEGDEC_E_COEFF = 3,        /* a run past coefficient 63 */
       ATTWARP_JPEGDEC_E_RESTART = 4,      /* restart markers: wrong number or wrong index */
       ATTWARP_JPEGDEC_E_NO_EOI = 5 };     /* the first marker behind the data is not EOI */
typedef struct attwarp_jpegdec_image {
  uint64_t stream_off;                             /* the image's entropy data in the packed buffer */
  uint64_t stream_len;
  int32_t H, W;
  int32_t ncomp;                                   /* 1 or 3 */
  int32_t hs, vs;                                  /* luma sampling: 1x1, 2x1, 2x2 (grey: 1x1) */
  int32_t restart_interval;                        /* MCUs, 0: none */
  int32_t mode;                                    /* ATTWARP_JPEGDEC_RGB / L / KEEP */
  int32_t order;                                   /* ATTWARP_RGB / ATTWARP_BGR */
  uint16_t qt[3][64];                              /* per component, natural (de-zigzagged) order, 0..255 */
  uint8_t dc_counts[3][16], ac_counts[3][16];      /* DHT: codes of each length 1..16 */
  uint8_t dc_symbols[3][256], ac_symbols[3][256];  /* DHT: symbols by (length, code); DC symbols are categories <= 15 */
} attwarp_jpegdec_image;
typedef struct attwarp_jpegdec_header {            /* first bytes of a table written by attwarp_jpegdec_plan */
  uint32_t magic;
  int32_t B, total_units, idct_tiles, color_tiles;
  int32_t reserved;                                /* workgroups of the sub-stream launch that have an image; 0: none planned */
  uint64_t table_bytes, scratch_bytes, out_bytes, stream_bytes;
  uint64_t off_images;
} attwarp_jpegdec_header;
ATTWARP_API size_t attwarp_jpegdec_table_bytes(const attwarp_jpegdec_image* images, int B);
ATTWARP_API int attwarp_jpegdec_plan(const attwarp_jpegdec_image* images, int B, void* table, size_t table_bytes);
/* The same with sub-streams: segment_bytes a power of two in 32..512, max_rounds in 1..65536; (0, 0): attwarp_jpegdec_plan. */
ATTWARP_API int attwarp_jpegdec_plan_ex(const attwarp_jpegdec_image* images, int B, void* table, size_t table_bytes, int segment_bytes,
                       int max_rounds);
/* Where a table keeps, per image, the uint32[4] (segments planned, rounds, accepted, 0) in the scratch buffer. */
ATTWARP_API uint64_t attwarp_jpegdec_info_offset(const void* table_host);
ATTWARP_API int attwarp_jpegdec_decode(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                       uint8_t* out, size_t out_bytes, int32_t* status, void* stream);

/* ---- PROGRESSIVE files (SOF2) of a whole batch, scans by dependency level (jpegdec.hip).  The same frames
 * as above; the HOST walks every marker of the file, applies DHT / DRI in file order and describes every scan: its
 * components (indices in frame order, ascending), band Ss..Se, Ah, Al, the restart interval in force at its SOS (MCUs of
 * THAT scan, 0: none), where its entropy data starts inside the image's packed data (everything behind the first SOS
 * header, as above), and the tables it names (one DC table per component of a DC scan, [0] the AC table of an AC scan).
 * attwarp_jpegdec_image carries sizes, sampling, qt, mode and order; its tables and restart_interval stay zero.  The scans
 * are passed image by image, in file order.  The table is a table of attwarp_jpegdec_plan (what the IDCT and colour
 * launches read) followed by the scan records; it depends on the headers, the scan records and the lengths alone.
 * Geometry: a scan of several components walks the frame's MCUs; a scan of one component walks the ceil(cw / 8) x
 * ceil(ch / 8) blocks that cover the component's true size (cw = ceil(W h / hmax)), in raster order, and its restart
 * interval counts those.  Units of a scan: ceil(MCUs / Ri), one wave each; predictors and the EOB run reset per unit.
 * Level of a scan: 0 if no earlier scan of the image shares a component with it and overlaps its band, else 1 + the
 * largest level among those; by_level = 0 plans one level per scan position instead (for tests: pixels, statuses and
 * coefficients do not depend on it).  Launches: one clear (the coefficient memory is zeroed on every run), one restart scan
 * (per SCAN the rule above), one entropy launch per level of the call's deepest image, IDCT, colour: constant per plan.
 * The planner checks what the kernels' bounds rest on (Ss <= Se <= 63, Ss = 0 only with Se = 0, an AC scan of one
 * component, Al <= 13, Ah = 0 or Al + 1, at most ATTWARP_JPEGDEC_MAX_SCANS scans and ATTWARP_JPEGDEC_MAX_UNITS units per
 * image over all its scans); whether the scans form a complete, consistent progression is the caller's to check.
 * status[b]: E_RESTART from any scan first, then the status of the lowest failing (scan in file order, unit), then
 * E_NO_EOI by the marker behind the LAST scan.  E_COEFF also names a refinement symbol whose size is not 1. */
#define ATTWARP_JPEGDEC_MAX_SCANS 64
typedef struct attwarp_jpegdec_scan {
  int32_t image;                                   /* index into the images of the call; ascending over the array */
  int32_t ncomp, comp[3];                          /* components of the scan, indices in frame order */
  int32_t ss, se, ah, al;
  int32_t restart_interval;                        /* MCUs of this scan, 0: none */
  uint64_t stream_off;                             /* its entropy data, relative to the image's stream_off */
  uint8_t counts[3][16], symbols[3][256];          /* DHT of the tables it names */
} attwarp_jpegdec_scan;
ATTWARP_API size_t attwarp_jpegdec_scans_table_bytes(const attwarp_jpegdec_image* images, int B, int nscans);
ATTWARP_API int attwarp_jpegdec_plan_scans(const attwarp_jpegdec_image* images, int B, const attwarp_jpegdec_scan* scans, int nscans,
                       void* table, size_t table_bytes, int by_level);
ATTWARP_API int attwarp_jpegdec_decode_scans(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                       uint8_t* out, size_t out_bytes, int32_t* status, void* stream);
/* The same with SUB-STREAMS PER SCAN: attwarp_jpegdec_plan_scans plus segment_bytes (a power of two in
 * 32..512) and max_rounds (1..65536), as attwarp_jpegdec_plan_ex is to attwarp_jpegdec_plan, and data_bytes[nscans]: the
 * bytes of each scan's entropy data, up to the first FF that neither 00 nor D0..D7 follows (the scan record carries no
 * length).  (0, 0, NULL) is attwarp_jpegdec_plan_scans and writes the same table, byte for byte.  A scan of ONE unit whose
 * data is at least two segments long (at most 16384 of them) is cut; attwarp_jpegdec_decode_scans then launches, per level
 * that holds a cut scan and in front of that level's entropy launch, jpegprog_substream_kernel with one workgroup of 256
 * lanes per cut scan, segment s on lane s mod 256: constant launches per plan.  Routes: a DC or AC first pass runs the rounds
 * of attwarp_jpegdec_plan_ex over its own blocks (one DC symbol; the AC symbols of the band, an EOB run ending its blocks at
 * once) and is accepted under the same rule; a DC refinement counts the segments' data bytes (block n's bit is data bit n)
 * and is accepted when the bits cover the blocks; an AC refinement is skimmed exactly by one lane over bit masks of the
 * coefficients with history (no coefficient touched), which notes every segment's true entry, and is accepted unless the
 * one-lane route would report a status; then all lanes write.  The entropy launch skips an accepted scan and decodes every
 * other one exactly as without sub-streams; the sub-stream path never sets a status and stores no coefficient before its
 * scan is accepted, so status[] and the pixels do not depend on the plan.
 * Table: behind the scan records a header and one 64-byte record per scan; attwarp_jpegdec_scans_table_bytes_ex gives the
 * size.  Scratch, behind everything the other kernels use: per scan, in the order of scans[], an attwarp_jpegdec_scan_info (32 bytes)
 * at attwarp_jpegdec_scan_info_offset (0: the table has none), written on every run, first by the clear launch; per cut
 * scan 64 bytes per segment and, for an AC refinement, 12 bytes per block of the scan (masks and prefix sums). */
typedef struct attwarp_jpegdec_scan_info {
  uint32_t route;                                  /* 0: one lane; 1 DC first pass, 2 DC refinement, 3 AC first pass, 4 AC refinement */
  uint32_t segments, rounds, accepted;
  uint32_t ticks[3];                               /* FOR MEASUREMENTS ONLY (tools/jpegprogsync_bench.py; four clock reads by one lane per
                                                      workgroup): 100 MHz ticks of its workgroup's three parts: a first pass: rounds,
                                                      sums and checks, write; a refinement: counts and masks, skim (DC: none), write */
  uint32_t pad;
} attwarp_jpegdec_scan_info;
ATTWARP_API size_t attwarp_jpegdec_scans_table_bytes_ex(const attwarp_jpegdec_image* images, int B, int nscans, int segment_bytes,
                       int max_rounds);
ATTWARP_API int attwarp_jpegdec_plan_scans_ex(const attwarp_jpegdec_image* images, int B, const attwarp_jpegdec_scan* scans, int nscans,
                       void* table, size_t table_bytes, int by_level, int segment_bytes, int max_rounds, const uint64_t* data_bytes);
ATTWARP_API uint64_t attwarp_jpegdec_scan_info_offset(const void* table_host);

/* ---- every LAYOUT of a sequential file (jpegdec.hip, jpegfmt_blocks.hpp): a second family beside
 * attwarp_jpegdec_plan / attwarp_jpegdec_decode, with records of its own, for what those refuse.  SOF0 / SOF1, 8 bits, one
 * interleaved scan, any restart interval, and
 *   components: 1, 3 or 4;
 *   sampling:   per component factors h, v of 1..4 that divide the frame's largest (libjpeg has no fractional up-sampling),
 *               with sum of h v <= 10 (T.81 B.2.3); a one-component image is not interleaved and its factors do not count;
 *   colour:     the caller's decision (libjpeg's rule over the Adobe transform, JFIF and the component ids):
 *               ATTWARP_JPEGDEC_COLOR_GREY (1 component), _YCC or _RGB (3), _CMYK or _YCCK (4).
 * Everything else is the contract of attwarp_jpegdec_plan_ex / attwarp_jpegdec_decode: the same packed stream, scratch
 * layout, units, sub-streams (segment_bytes = max_rounds = 0: none), statuses and their precedence, limits, and five
 * capturable launches.  A sub-stream state carries the block slot modulo the PERIOD of the MCU's sequence of Huffman tables
 * (components that share their tables, as all four of libjpeg's CMYK files do, make slots no decoder can tell apart), a
 * segment sums the DC differences of its blocks by their place in it, and every block's slot, component and predictor
 * follow from the count of blocks in front of its segment: up to 10 slots, four predictors, the same acceptance rule.
 * Each component is up-sampled as
 * jdsample.c would: same size copied; 2 x 1 and 2 x 2 by the triangle filters when its true width ceil(W h / hmax) exceeds 2,
 * else replicated; 1 x 2 by the vertical triangle filter; every other integral ratio replicated.  Then the colour rule,
 * then Pillow's conversion: mode RGB / L give Image.open(f).convert(mode) bit for bit, for four components through
 * Pillow's CMYK bytes (every stored sample of a CMYK file inverted; a YCCK file's YCbCr -> RGB taken as C, M, Y and K
 * inverted), R = (255 - K) - muldiv255(C, 255 - K) with muldiv255(a, b) = ((t >> 8) + t) >> 8, t = a b + 128, then the luma
 * of that RGB.  KEEP gives the file's channels: 1, 3 (RGB) or 4 (Pillow's CMYK bytes).  ATTWARP_BGR swaps a 3-channel
 * output only.  The planner refuses (ATTWARP_E_ARG) factors, components and colour rules outside the above and Huffman
 * tables that are over-subscribed, longer than 256 symbols or hold a DC category above 15. */
enum { ATTWARP_JPEGDEC_COLOR_GREY = 0, ATTWARP_JPEGDEC_COLOR_YCC = 1, ATTWARP_JPEGDEC_COLOR_RGB = 2, ATTWARP_JPEGDEC_COLOR_CMYK = 3,
       ATTWARP_JPEGDEC_COLOR_YCCK = 4 };
typedef struct attwarp_jpegdec_layout_image {
  uint64_t stream_off;                             /* the image's entropy data in the packed buffer */
  uint64_t stream_len;
  int32_t H, W;
  int32_t ncomp;                                   /* 1, 3 or 4 */
  int32_t h[4], v[4];                              /* sampling factors per component */
  int32_t color;                                   /* ATTWARP_JPEGDEC_COLOR_* */
  int32_t restart_interval;                        /* MCUs, 0: none */
  int32_t mode;                                    /* ATTWARP_JPEGDEC_RGB / L / KEEP */
  int32_t order;                                   /* ATTWARP_RGB / ATTWARP_BGR */
  int32_t reserved;
  uint16_t qt[4][64];                              /* per component, natural order, 0..255 */
  uint8_t dc_counts[4][16], ac_counts[4][16];
  uint8_t dc_symbols[4][256], ac_symbols[4][256];
} attwarp_jpegdec_layout_image;
/* The table starts with an attwarp_jpegdec_header (of this family: attwarp_jpegdec_decode refuses it and the reverse). */
ATTWARP_API size_t attwarp_jpegdec_layouts_table_bytes(const attwarp_jpegdec_layout_image* images, int B);
ATTWARP_API int attwarp_jpegdec_plan_layouts(const attwarp_jpegdec_layout_image* images, int B, void* table, size_t table_bytes,
                       int segment_bytes, int max_rounds);
ATTWARP_API int attwarp_jpegdec_decode_layouts(const void* table_host, const void* table_dev, const uint8_t* stream_bytes, void* scratch,
                       uint8_t* out, size_t out_bytes, int32_t* status, void* stream);

/* ---- SCANS of every layout (jpegdec.hip, jpegscan_blocks.hpp): a fourth family, the cross term of the two
 * above, for what both refuse: a PROGRESSIVE file (SOF2) of any layout attwarp_jpegdec_plan_layouts takes (1, 3 or 4 components,
 * factors 1..4 that divide the largest, sum of h v <= 10: the slot map of an image record has ten entries, colour by the
 * caller), and a SEQUENTIAL file (SOF0 / SOF1) whose components come in several scans.  The images are
 * attwarp_jpegdec_layout_image records with the tables and restart_interval left zero; the scans are passed image by image,
 * in file order, as for attwarp_jpegdec_plan_scans, with
 *   comp[]:      the scan's components, indices in frame order, ascending, any subset of the frame's;
 *   sequential:  1: band 0..63 with Ah = Al = 0, DC and AC of every block in one pass (a scan of a sequential file);
 *                0: a progressive scan under the rules of attwarp_jpegdec_plan_scans;
 *   tables:      dc_*[t], ac_*[t] for the t-th component of a sequential scan; dc_*[t] of a DC first pass; ac_*[0] of an AC
 *                scan; none of a DC refinement.
 * Geometry: a scan of several components walks the FRAME's MCUs, ceil(W / 8 hmax) x ceil(H / 8 vmax), also when it holds a
 * subset of the components, and visits its components' h x v blocks of each; a scan of one component walks the
 * ceil(cw / 8) x ceil(ch / 8) blocks that cover the component's true size (cw = ceil(W h / hmax)) in raster order, at the
 * pitch of the component's padded plane.  Restart intervals count those.  Levels, by_level, units, launches (one clear, one
 * restart scan per SCAN, one entropy launch per level, then the IDCT and colour launches of attwarp_jpegdec_decode_layouts,
 * unchanged), statuses and their precedence are those of attwarp_jpegdec_plan_scans / attwarp_jpegdec_decode_scans; all scans
 * of a sequential file are level 0, since each of its components is sent once.  The table is a table of
 * attwarp_jpegdec_plan_layouts for B one-unit images under a magic of its own (each decode entry point refuses the tables of
 * the other families before any launch), then a header and the scan records.  The planner checks what the kernels'
 * bounds rest on: the band and Al rules, an AC or refinement scan of one component, component indices ascending and below
 * the frame's, every table named, ATTWARP_JPEGDEC_MAX_SCANS scans and ATTWARP_JPEGDEC_MAX_UNITS units per image over all
 * its scans.  Whether the scans form a complete, consistent file (every coefficient reaching Al = 0; every component of a
 * sequential file sent exactly once) is the caller's to check. */
typedef struct attwarp_jpegdec_layout_scan {
  int32_t image;                                   /* index into the images of the call; ascending over the array */
  int32_t ncomp, comp[4];                          /* components of the scan, indices in frame order */
  int32_t ss, se, ah, al;
  int32_t sequential;                              /* 1: band 0..63, DC and AC in one pass */
  int32_t restart_interval;                        /* MCUs of this scan, 0: none */
  uint64_t stream_off;                             /* its entropy data, relative to the image's stream_off */
  uint8_t dc_counts[4][16], ac_counts[4][16];      /* DHT of the tables it names */
  uint8_t dc_symbols[4][256], ac_symbols[4][256];
} attwarp_jpegdec_layout_scan;
ATTWARP_API size_t attwarp_jpegdec_layout_scans_table_bytes(const attwarp_jpegdec_layout_image* images, int B, int nscans);
ATTWARP_API int attwarp_jpegdec_plan_layout_scans(const attwarp_jpegdec_layout_image* images, int B, const attwarp_jpegdec_layout_scan* scans,
                       int nscans, void* table, size_t table_bytes, int by_level);
ATTWARP_API int attwarp_jpegdec_decode_layout_scans(const void* table_host, const void* table_dev, const uint8_t* stream_bytes,
                       void* scratch, uint8_t* out, size_t out_bytes, int32_t* status, void* stream);

/* Marker-less PROGRESSIVE scans of this family in parallel segments (jpegscan_sync_blocks.hpp):
 * attwarp_jpegdec_plan_scans_ex for layout scans.  Arguments, cut rule (one unit, data_bytes[i] >= 2 segment_bytes, at most
 * 16384 segments, fewer than 2^24 blocks; data_bytes[i] = 0 leaves scan i on one lane), routes, acceptance and the
 * attwarp_jpegdec_scan_info records at attwarp_jpegdec_scan_info_offset are those of the plain family, over the general
 * MCU: block ordinal n of a scan is MCU n / nslot, slot n % nslot.  A SEQUENTIAL scan is never cut (route 0).  A DC first
 * pass may find several components on one Huffman table, so its decoder's state carries the slot only modulo the period of
 * the scan's table sequence (the smallest divisor P of the blocks per MCU whose DC tables repeat, compared by content, kept
 * in the scan's sub-stream record), a segment sums its DC differences by the block's place in it, and the scan is accepted
 * only if every segment's entry slot is the count of blocks in front of it modulo P.  With segment_bytes = max_rounds = 0
 * and data_bytes = NULL the table is attwarp_jpegdec_plan_layout_scans' byte for byte.  Table: behind the scan records a
 * header and one 64-byte record per scan.  Scratch, behind everything there was: the records, per cut scan 96 bytes per
 * segment and, for an AC refinement, 12 bytes per block.  attwarp_jpegdec_decode_layout_scans launches
 * jpegscan_substream_kernel (one workgroup per cut scan) in front of the entropy launch of every level that holds a cut
 * scan; status[] and the pixels do not depend on the plan. */
ATTWARP_API size_t attwarp_jpegdec_layout_scans_table_bytes_ex(const attwarp_jpegdec_layout_image* images, int B, int nscans,
                       int segment_bytes, int max_rounds);
ATTWARP_API int attwarp_jpegdec_plan_layout_scans_ex(const attwarp_jpegdec_layout_image* images, int B,
                       const attwarp_jpegdec_layout_scan* scans, int nscans, void* table, size_t table_bytes, int by_level,
                       int segment_bytes, int max_rounds, const uint64_t* data_bytes);

/* ---- JPEG files of a whole batch of differently sized uint8 images, encoded on the device (jpegenc.hip):
 * the bytes of Pillow's Image.save(f, "JPEG", quality, subsampling, restart_marker_rows), whole file: baseline sequential,
 * JFIF APP0, one DQT per table, SOF0, the four Annex K Huffman tables, DRI when restarts are on, one interleaved scan.
 * C = 1 is one grey component; C = 3 is YCbCr (libjpeg's 16-bit fixed point) with 4:4:4, 4:2:2 or 4:2:0 chroma.  Edges: the
 * input is replicated to the right and down to a multiple of the vertical factor, the DOWN-SAMPLED rows below that.  The DCT
 * is jfdctint's, quantisation rounds half away from zero, quality scales the Annex K tables as jpeg_set_quality does.
 * Seven launches, none with a host-dependent argument (capturable): transform (one thread per block), entropy (one workgroup
 * per unit of at most ATTWARP_JPEGENC_UNIT_MCUS MCUs, one wave per block), a scan of the units' bit lengths per image, a
 * shifted gather into the unstuffed stream that counts the FF bytes, a second scan, a scan of the files' lengths into offsets,
 * and the pass that writes stuffed bytes, RSTn, header and EOI.  Steps 1 - 4 are those of attwarp_png_*.
 * header.out_bytes is the sum of attwarp_jpegenc_bound over the batch.
 * Limits (ATTWARP_E_UNSUPPORTED from the planner): H, W <= ATTWARP_JPEGENC_MAX_DIM, a restart interval (restart_rows x MCUs
 * per row) <= 65535, a file bound below 2^31, B <= 2^20, at most 2^24 units per call. */
#define ATTWARP_JPEGENC_UNIT_MCUS 16
#define ATTWARP_JPEGENC_MAX_DIM 65500
enum { ATTWARP_JPEGENC_444 = 0, ATTWARP_JPEGENC_422 = 1, ATTWARP_JPEGENC_420 = 2 };   /* Pillow's subsampling numbers */
typedef struct attwarp_jpegenc_image {
  const uint8_t* src;                              /* device: H rows of W * C bytes, pitch bytes apart, any byte address */
  int32_t H, W, C;
  int32_t pitch;
  int32_t order;                                   /* ATTWARP_RGB / ATTWARP_BGR (ignored for C = 1) */
  int32_t quality;                                 /* 1 .. 100 */
  int32_t subsampling;                             /* ATTWARP_JPEGENC_* (ignored for C = 1) */
  int32_t restart_rows;                            /* MCU rows per restart interval, 0: no restart markers */
} attwarp_jpegenc_image;
typedef struct attwarp_jpegenc_header {            /* first bytes of a table written by attwarp_jpegenc_plan */
  uint32_t magic;
  int32_t B, nunits, reserved;
  uint64_t table_bytes, scratch_bytes, out_bytes;
  uint64_t off_images, off_units, off_huffman;     /* in the table */
  uint64_t off_image_out;                          /* in the scratch buffer: per image the file's bytes */
  uint64_t off_optimize;                           /* in the table: 0, or the record of the optimised images (attwarp_jpegenc_plan_ex) */
} attwarp_jpegenc_header;
/* 0: outside the limits */
ATTWARP_API size_t attwarp_jpegenc_bound(int H, int W, int C, int quality, int subsampling, int restart_rows);
ATTWARP_API size_t attwarp_jpegenc_table_bytes(const attwarp_jpegenc_image* images, int B);
ATTWARP_API int attwarp_jpegenc_plan(const attwarp_jpegenc_image* images, int B, void* table, size_t table_bytes);
ATTWARP_API int attwarp_jpegenc_encode(const void* table_host, const void* table_dev, void* scratch, uint8_t* out, size_t out_bytes,
                       int64_t* offsets, void* stream);

/* Per-image optimised Huffman tables (jpegopt_blocks.hpp): optimize is NULL or one flag (0 / 1) per image.  An
 * image with optimize[i] = 1 is written as Image.save(..., optimize=True) writes it: the same pixels, its DHT segments (in the
 * order DC 0, AC 0, DC 1, AC 1, in front of DRI) holding the tables libjpeg's jpeg_gen_optimal_table builds from the image's
 * own symbol counts: the two smallest non-zero frequencies merged, ties to the larger index, a reserved leaf of frequency 1,
 * lengths limited to 16 bits, symbols listed by length and then by value.  With optimize = NULL or all zero the table is
 * attwarp_jpegenc_plan's byte for byte and attwarp_jpegenc_encode runs its seven launches.  Otherwise the table ends with a
 * record of the optimised images and their units, scratch grows by 4096 + 5928 bytes per optimised image, and
 * attwarp_jpegenc_encode (unchanged: it reads what to do from the table) puts three launches behind the transform: a clear of
 * the images' histograms, the histogram (one workgroup per unit), the tables (one workgroup per image, one wave per table,
 * which also splices the DHTs into the header).  All are capturable.  An optimised DC table holds up to 12 categories and the
 * reserved leaf, so a DC code may take 12 bits: attwarp_jpegenc_bound_ex(..., 1) is attwarp_jpegenc_bound plus one bit per
 * block (the header never grows), and header.out_bytes sums attwarp_jpegenc_bound_ex.  The limits are the plain family's. */
ATTWARP_API size_t attwarp_jpegenc_bound_ex(int H, int W, int C, int quality, int subsampling, int restart_rows, int optimize);
ATTWARP_API size_t attwarp_jpegenc_table_bytes_ex(const attwarp_jpegenc_image* images, int B, const int32_t* optimize);
ATTWARP_API int attwarp_jpegenc_plan_ex(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, void* table, size_t table_bytes);

/* Progressive files (jpegprogenc_blocks.hpp): progressive is NULL or one flag (0 / 1) per image.  An image with
 * progressive[i] = 1 is written as Image.save(..., progressive=True) writes it, whatever optimize[i] says (libjpeg forces
 * optimised tables there): SOF2, jpeg_simple_progression's script (colour: ten scans, Cr before Cb; grey: six), in front of
 * every scan the DHT(s) of its own optimal table(s), a DRI where the scan's restart interval (restart_rows x ITS MCUs per row)
 * differs from the last one written, and its SOS; the scan data is jcphuff.c's, end-of-band runs flushed at 0x7FFF blocks and
 * above 937 pending correction bits, RSTn numbered from 0 in every scan.  With progressive = NULL or all zero the table is
 * attwarp_jpegenc_plan_ex's byte for byte.  Otherwise header.reserved is the offset / 16 of a record of the progressive
 * images and their segments (one per scan and restart interval) at the table's end; such an image owns no entropy unit
 * (header.nunits does not count it) and its transform units follow the others.  attwarp_jpegenc_encode (unchanged) adds
 * eight launches: histogram clear; a summary of every block of the AC scans (one wave per block); one lane per segment
 * walking the summaries, which resolves the end-of-band runs; one lane per block counting its symbols; tables (one workgroup
 * per image); one lane per block placing and writing its bits; a scan of the pieces' lengths per image; the write, which
 * stuffs.  All are capturable.  Scratch grows by 13 bytes per block and scan.
 * attwarp_jpegenc_bound_prog(..., 0) is attwarp_jpegenc_bound_ex; with progressive = 1 it prices every block of every scan at
 * 16-bit symbols, every byte as stuffed, and ten DHTs at 277 bytes.  Limits: the plain family's, with the
 * restart interval of EVERY scan <= 65535 (luma scans walk up to twice the MCUs per row; libjpeg clamps silently instead), and
 * at most 2^24 segments per call. */
ATTWARP_API size_t attwarp_jpegenc_bound_prog(int H, int W, int C, int quality, int subsampling, int restart_rows, int optimize, int progressive);
ATTWARP_API size_t attwarp_jpegenc_table_bytes_prog(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, const int32_t* progressive);
ATTWARP_API int attwarp_jpegenc_plan_prog(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, const int32_t* progressive,
                       void* table, size_t table_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ATTWARP_H */
