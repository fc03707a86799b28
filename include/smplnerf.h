/* smplnerf.h - C-ABI of libsmplnerf_hip.so: the MI355X (gfx950) NeRF ray-march path.
 *
 * Drop-in boundary for the hot path of HannesStark/SMPL-NeRF (citations are reference file:line):
 *
 *   snerf_searchsorted_f32   replaces  torchsearchsorted.searchsorted
 *                            (torchsearchsorted/src/torchsearchsorted/searchsorted.py:20-53; native
 *                            searchsorted_cpu_wrapper.cpp:82-122, searchsorted_cuda_kernel.cu:84-141)
 *   snerf_posenc_f32         replaces  PositionalEncoder.encode            (utils.py:114-131)
 *   snerf_composite_fwd_f32  replaces  raw2outputs                         (utils.py:134-191)
 *   snerf_sample_pdf_f32     replaces  sample_pdf + fine_sampling          (utils.py:194-264)
 *   snerf_mlp_*              replaces  RenderRayNet.forward                (models/render_ray_net.py:42-61)
 *                            fused with the positional encoding of its inputs as used by
 *                            NerfPipeline.forward                          (models/nerf_pipeline.py:29-41, :49-60)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host; buffers are borrowed
 *     for the duration of the call only; outputs are caller-allocated; nothing is retained.
 *   - `stream` is a hipStream_t (pass PyTorch's current stream); all work is enqueued
 *     asynchronously on it, no call synchronises the device.
 *   - return value: 0 on success, <0 = SNERF_E_*; nothing throws across the ABI.
 *     snerf_last_error_string() describes the last failure on the calling thread.
 *   - row-major, densely packed fp32 tensors; indices are int64 (torch.long) like the reference.
 *   - re-entrant and thread-safe; calls act on the calling thread's current HIP device.
 *
 * State.  The library keeps no caller-visible state between calls.  What it does keep, process-wide:
 *   - the error text of the last failure, per thread (snerf_last_error_string);
 *   - two HIP events per host thread and device, created at the first training call that is given an auxiliary stream
 *     (fork / join of the concurrent backward; snerf_shutdown() destroys them);
 *   - per HIP device ordinal (up to 64 devices): the CU count and, per kernel, whether its dynamic-LDS limit was
 *     raised (hipFuncSetAttribute is per device) - so one process may drive several GPUs through the library;
 *   - environment variables, read ONCE at the first call that consults them: SNERF_LAT, SNERF_MLP_FOLD, SNERF_WARP_FOLD,
 *     SNERF_RCCL_LIB and the debugging aid SNERF_DEBUG_POISON_LDS.  INTEGRATION.md ("Environment variables") describes them and
 *     the Python host's; a release build can ignore all of them (results are identical under every setting, up to the summation
 *     order of the folded per-ray columns).
 */
#ifndef SMPLNERF_H
#define SMPLNERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_VERSION 109 /* 0.1.2: + snerf_searchsorted (all scalar types), snerf_posenc_bwd_f32,
                             snerf_composite_bwd_all_f32; composite forward accepts any N
                             0.1.3: same entry points; descriptors accept any width <= 256 and n_layers >= 1; fp32 inference
                             folds per-ray inputs (dirs_per_sample bit 1 = SNERF_FWD_NO_RAY_FOLD keeps the per-sample form)
                             0.1.4: + the training step as one call (snerf_nerf_train_step_f32 / _grads_f32, snerf_adam_step_f32,
                             snerf_mlp_stream_slots), snerf_dy_contract_f32; the per-ray fold tables moved from stream-ordered allocations inside
                             the library to caller workspaces (snerf_mlp_fwd_ws_f32, snerf_warp_fwd_ws_f32): the library allocates nothing
                             0.1.5: + snerf_render_rays_add_f32 (the single-call render for nets with per-ray additional inputs)
                             0.1.6: + snerf_shutdown; hidden visibility: the entry points of this header are the only dynamic symbols
                             0.1.7: + snerf_comm_*, snerf_nerf_train_step_dp_f32, snerf_smpl_nerf_train_step_dp_f32 (RCCL inside the
                             boundary); latency-class kernels behind the same entry points for small calls
                             0.1.8: + snerf_smpl_nerf_train_grads_aux_f32, snerf_smpl_nerf_train_step_aux_f32 (the smpl_nerf step with an
                             auxiliary stream: small chunks run the coarse chain beside the fine chain); snerf_mlp_desc.width
                             up to 512
                             0.1.9: + snerf_nerf_train_step_dp_ig_f32; the data-parallel steps issue the same collectives on every
                             rank whatever its batch size (B == 0 included); SNERF_RCCL_LIB; snerf_linear_* / snerf_relu_bwd_f32 (any --netwidth)
                             (same version): + snerf_mlp_packed_infer_floats, snerf_mlp_pack_infer_f32, snerf_mlp_fwd_infer_f32 and
                             precision SNERF_FP32_INFER of the render entries: fp32 inference on a stream with the activation-free
                             layers composed (13 % fewer matrix operations); existing entries and streams are unchanged */

#define SNERF_OK 0
#define SNERF_E_BADARG (-1)   /* null pointer, negative size, unsupported shape */
#define SNERF_E_ALIGN (-2)    /* pointer not aligned as documented */
#define SNERF_E_LAUNCH (-3)   /* HIP launch / runtime error */
#define SNERF_E_NODEVICE (-4) /* no gfx950 device visible */

typedef void *snerf_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: the entry points declared here are its only dynamic symbols
 * (tests/test_abi.py: `nm -D --defined-only` lists nothing but snerf_*). */
#if defined(__GNUC__) || defined(__clang__)
#define SNERF_API __attribute__((visibility("default")))
#else
#define SNERF_API
#endif

SNERF_API int snerf_version(void);
SNERF_API const char *snerf_last_error_string(void);
/* Number of visible HIP devices (0 when none); never fails. */
SNERF_API int snerf_device_count(void);
/* Releases what the library holds process-wide (section "State"): the fork / join events of every host thread and device.
 * Optional - a process may simply exit; for hosts that unload the library or count HIP objects.  Must not run concurrently
 * with another call into the library; the next training call creates its events again.  Returns SNERF_OK. */
SNERF_API int snerf_shutdown(void);

/* ---- a6: batched searchsorted --------------------------------------------------------------
 * out[r, c] = #{ k : a[ra, k] <  v[rv, c] }   (side_left != 0, numpy side='left')
 *           = #{ k : a[ra, k] <= v[rv, c] }   (side_left == 0, side='right')
 * rows of `a` must be sorted ascending.  ra = 0 if nrow_a == 1 else r (same for rv): the
 * reference's row broadcast (searchsorted_cpu_wrapper.cpp:109-110).  nrow_a and nrow_v must be
 * equal or one of them 1 (searchsorted.py:23-28).  out: int64 [max(nrow_a,nrow_v), ncol_v]. */
SNERF_API int snerf_searchsorted_f32(const float *a, int64_t nrow_a, int64_t ncol_a,
                           const float *v, int64_t nrow_v, int64_t ncol_v,
                           int64_t *out, int side_left, snerf_stream_t stream);

/* The same for every scalar type the reference dispatches (AT_DISPATCH_ALL_TYPES, searchsorted_cpu_wrapper.cpp:100,
 * searchsorted_cuda_kernel.cu:132); `a` and `v` have the same element type `dtype`. */
#define SNERF_DTYPE_F32 0
#define SNERF_DTYPE_F64 1
#define SNERF_DTYPE_I32 2
#define SNERF_DTYPE_I64 3
#define SNERF_DTYPE_I16 4
#define SNERF_DTYPE_I8 5
#define SNERF_DTYPE_U8 6
SNERF_API int snerf_searchsorted(int dtype, const void *a, int64_t nrow_a, int64_t ncol_a, const void *v, int64_t nrow_v,
                       int64_t ncol_v, int64_t *out, int side_left, snerf_stream_t stream);

/* ---- a1: positional encoding ----------------------------------------------------------------
 * x [n, c] -> out [n, c*(identity + 2*L)], frequency-major: [x] [sin(2^0 x) cos(2^0 x)] ...
 * (utils.py:116-131; no pi factor).  0 <= L <= 30, c >= 1 and a row of at most 16384 floats, in the backward too;
 * anything else is SNERF_E_BADARG. */
SNERF_API int snerf_posenc_f32(const float *x, int64_t n, int c, int L, int identity, float *out,
                     snerf_stream_t stream);

/* Backward of the encoding: d_out [n, c*(identity + 2*L)] -> d_x [n, c] (autograd through utils.py:123-131). */
SNERF_API int snerf_posenc_bwd_f32(const float *x, const float *d_out, int64_t n, int c, int L, int identity, float *d_x,
                         snerf_stream_t stream);

/* ---- a4: alpha compositing --------------------------------------------------------------------
 * raw [B, N, 4] (r, g, b, sigma), z [B, N], dirs: [B, 3] when dirs_per_sample == 0 (the ray
 * direction broadcast over samples) or [B, N, 3]; dists are scaled by ||dirs|| (utils.py:165).
 * noise: nullable [B, N], added to sigma before relu (utils.py:171-173; the caller draws it).
 * rgb [B, 3], weights [B, N], alpha [B, N] (any of the three may be NULL to skip the store).
 * N == 1 reproduces the reference's early return (utils.py:168-169): weights = alpha = 1.  Any N >= 1 (the backward
 * entry points take N <= 4096). */
SNERF_API int snerf_composite_fwd_f32(const float *raw, const float *z, const float *dirs, int dirs_per_sample,
                            const float *noise, int64_t B, int N, int white_background,
                            float *rgb, float *weights, float *alpha, snerf_stream_t stream);

/* Backward of the compositing w.r.t. raw: d_rgb [B,3] -> d_raw [B,N,4] (same raw/z/dirs/noise as the
 * forward call; autograd through utils.py:161-191).  weights/alpha are treated as outputs without
 * gradient (the pipeline detaches what it derives from them, utils.py:260).  N <= 4096.  A per-sample direction of
 * norm 0 gets d_dirs = 0 (torch.norm's subgradient). */
SNERF_API int snerf_composite_bwd_f32(const float *raw, const float *z, const float *dirs, int dirs_per_sample,
                            const float *noise, int64_t B, int N, int white_background,
                            const float *d_rgb, float *d_raw, float *d_dirs /* nullable, [B,N,3]: only with per-sample
                            directions (dists are scaled by their norm, utils.py:165) */, snerf_stream_t stream);

/* The complete backward of raw2outputs (utils.py:134-191 under autograd): gradients arriving at ALL three outputs -
 * d_rgb [B,3], d_weights [B,N], d_alpha [B,N], each nullable (= zeros) - are propagated to d_raw [B,N,4] and, on request,
 * to the directions (d_dirs: [B,N,3] with per-sample directions, [B,3] otherwise; dists are scaled by their norm,
 * utils.py:165) and to the depths (d_z [B,N]; the last interval is the constant 1e10, utils.py:164).  N <= 4096.  N == 1:
 * weights and alpha are constants, d_dirs = d_z = 0. */
SNERF_API int snerf_composite_bwd_all_f32(const float *raw, const float *z, const float *dirs, int dirs_per_sample,
                                const float *noise, int64_t B, int N, int white_background, const float *d_rgb,
                                const float *d_weights, const float *d_alpha, float *d_raw, float *d_dirs /* nullable */,
                                float *d_z /* nullable */, snerf_stream_t stream);

/* ---- ray maps: opacity, expected depth and expected point of every ray (utils.py:184, :187) -------------------------
 * The reference's raw2outputs computes depth_map = sum(weights * z_vals) and acc_map = sum(weights) and drops them; these two
 * entries compute them, and the expected surface point, from what a compositing already returned, and carry a loss on them back
 * to alpha.  alpha [B, N]: the alpha of snerf_composite_fwd_f32 (the `densities` of a pipeline); o, d [B, 3]: ray origins and
 * directions; and exactly one of z [B, N] (the literal mode of utils.py:184) and pts [B, N, 3] (the sample points o + t d, for
 * callers who hold no depths: the parameter is recovered from the points).  1 <= N <= 4096; B == 0 is a no-op.  o and d are read
 * with pts only.  Per ray, operation by operation:
 *   1. t_i = z_i ; with pts: t_i = ((p_i - o) . d) / (d . d), every operation in fp64 on the fp32 inputs, the three products
 *      summed in x, y, z order; t_i = 0 where d . d == 0.
 *   2. u_i = fl32(fl32(1 - alpha_i) + 1e-10f): the factor snerf_composite_fwd_f32 forms (utils.py:176).
 *   3. T_i = prod_{j<i} u_j in fp64 (T_0 = 1), an exclusive prefix product in sample order.
 *   4. w_i = fl32(alpha_i * fl32(T_i)): the bits snerf_composite_fwd_f32 stores as `weights` for the same alpha - the maps belong
 *      to the weights the pipeline composited with.
 *   5. acc = sum_i w_i, depth = sum_i w_i t_i, point = sum_i w_i p_i (point [B, 3]: nullable, with pts only): sums and products
 *      in fp64, each result rounded to fp32 once.
 * N == 1 is the rule as written: T_0 = 1, so acc = alpha_0 and depth = alpha_0 t_0 - with the alpha = 1 of the reference's early
 * return (utils.py:170-171), acc = 1 and depth = t_0.  No disparity (commented out in the reference, NaN for an empty ray), no
 * median depth.  Every element of acc, depth and point is written; no atomics, no allocation; the same bits for any split of the
 * batch.  Added after 0.1.9 without a version bump: a C host finds the two entries with dlsym. */
SNERF_API int snerf_ray_maps_fwd_f32(const float *alpha, const float *z /* nullable */, const float *pts /* nullable */,
                                     const float *o, const float *d, int64_t B, int N, float *acc, float *depth,
                                     float *point /* nullable; needs pts */, snerf_stream_t stream);

/* Backward of the ray maps w.r.t. alpha: d_acc [B], d_depth [B], d_point [B, 3] (each nullable = zeros; d_point with pts only)
 * -> d_alpha [B, N], overwritten.  With G_i = d_acc + d_depth t_i + <d_point, p_i>, T_i as above and w_i = alpha_i T_i (here
 * unrounded), d u / d alpha = -1:
 *   d_alpha_k = T_k G_k - S_k / u_k ,  S_k = sum_{i>k} w_i G_i
 * everything in fp64 and rounded to fp32 once.  S_k is summed as an exclusive suffix (never "inclusive minus the own term": where
 * alpha_k = 1, u_k = 1e-10 and the quotient would multiply that subtraction's rounding by 1e10).  t, p, o and d get no gradient
 * (the hierarchical samples are detached in the reference, utils.py:260).  The result is what snerf_composite_bwd_all_f32 takes
 * as d_alpha. */
SNERF_API int snerf_ray_maps_bwd_f32(const float *alpha, const float *z /* nullable */, const float *pts /* nullable */,
                                     const float *o, const float *d, int64_t B, int N, const float *d_acc /* nullable */,
                                     const float *d_depth /* nullable */, const float *d_point /* nullable; needs pts */,
                                     float *d_alpha, snerf_stream_t stream);

/* ---- a5: inverse-CDF hierarchical sampling + merge + point generation ------------------------------
 * z [B, Nc] coarse depths (ascending), weights [B, Nc] from compositing, u [Nf] = linspace(0,1,Nf)
 * (passed in so that the caller controls its bits, see oracle/nerf_oracle.py:linspace01),
 * o, d [B, 3].  Outputs (each nullable): inds int64 [B, Nf] (searchsorted(cdf,u,'right')),
 * z_samples [B, Nf], z_fine [B, Nc+Nf] ascending, pts [B, Nc+Nf, 3] = o + d * z_fine.
 * 3 <= Nc <= 1024, 1 <= Nf <= 1024 (with fewer than three coarse samples there is no interior weight: the reference's own
 * sample_pdf builds an empty cdf and its gather raises, utils.py:200-221). */
SNERF_API int snerf_sample_pdf_f32(const float *z, const float *weights, const float *u,
                         const float *o, const float *d, int64_t B, int Nc, int Nf,
                         int64_t *inds, float *z_samples, float *z_fine, float *pts,
                         snerf_stream_t stream);

/* Strict variants (SURVEY 8b `strict_cumsum`): index parity with the reference FROM THE SAME WEIGHTS.  The reference's
 * pdf is weights / torch.sum(weights) (utils.py:201); torch's CPU sum is an fp32 cascade over 8-lane vectors, one fixed
 * order on x86 hosts (default, AVX2 and AVX-512 builds alike), and a 1-ulp difference in it moves ~0.1 % of the indices.
 * `tot` [B] = that sum (snerf_reference_sum_f32 below computes it on the device; or (weights[:, 1:-1] + 1e-5).sum(-1) with
 * torch on the CPU); every other step is independent of the evaluation order, so cdf, inds and the samples are then
 * bit-identical to the reference's. */
SNERF_API int snerf_sample_pdf_strict_f32(const float *z, const float *weights, const float *u, const float *o, const float *d,
                                const float *tot, int64_t B, int Nc, int Nf, int64_t *inds, float *z_samples,
                                float *z_fine, float *pts, snerf_stream_t stream);
SNERF_API int snerf_sample_pdf_bins_strict_f32(const float *bins, const float *weights, const float *u, const float *tot, int64_t B,
                                     int Nb, int Nf, int64_t *inds, float *z_samples, snerf_stream_t stream);

/* The literal sample_pdf(bins, weights, args) convention (utils.py:194-228): bins [B, Nb] (coarse
 * midpoints), weights [B, Nb-1] (interior coarse weights) -> inds int64 [B, Nf] (nullable),
 * z_samples [B, Nf].  2 <= Nb <= 1023. */
SNERF_API int snerf_sample_pdf_bins_f32(const float *bins, const float *weights, const float *u, int64_t B,
                              int Nb, int Nf, int64_t *inds, float *z_samples, snerf_stream_t stream);

/* torch.sum(x[b, :n] + add, -1) as torch's CPU kernel evaluates it for a contiguous fp32 row (x86 hosts); 0 <= n <= 32767.
 * x [B, row_stride] (row_stride >= n when B > 1), out [B].  The order (an fp32 cascade over 8-lane vectors with 4 columns and
 * 4 levels) is written out in smpl_nerf_amd/csrc/refsum.h.  The device form runs one wavefront per row; the _host form takes
 * host pointers and runs on the calling thread (no HIP call).  B == 0 is a no-op.  Rows of 32768 elements and more may be
 * split over threads by torch and are not covered.  Added after 0.1.9 without a version bump: a C host detects these two
 * entries and SNERF_REFERENCE_SUM by looking up snerf_reference_sum_f32 with dlsym. */
SNERF_API int snerf_reference_sum_f32(const float *x, int64_t row_stride, int64_t B, int n, float add, float *out,
                                      snerf_stream_t stream);
SNERF_API int snerf_reference_sum_host_f32(const float *x_host, int64_t row_stride, int64_t B, int n, float add, float *out_host);
/* OR into `precision` of snerf_render_rays_f32 / _add_f32 / _smpl_f32 and of the training entries that sample
 * (snerf_nerf_train_{grads,step}[_ig]_f32, snerf_nerf_train_step_dp[_ig]_f32, snerf_smpl_nerf_train_{grads,step}[_aux]_f32,
 * snerf_smpl_nerf_train_step_dp_f32): the hierarchical sampler takes the reference-order sum (strict mode, no host round
 * trip).  Without it the sum is the fp64 one, as before. */
#define SNERF_REFERENCE_SUM 0x100

/* Backward of sample_pdf(bins, weights, args) (utils.py:194-228 under autograd; fine_sampling detaches its result,
 * utils.py:260, so no pipeline needs it): d_z_samples [B, Nf] -> d_bins [B, Nb], d_weights [B, Nb-1], with the forward's
 * searchsorted indices `inds` [B, Nf] held fixed (integers carry no gradient in the reference either). */
SNERF_API int snerf_sample_pdf_bins_bwd_f32(const float *bins, const float *weights, const float *u, const int64_t *inds,
                                  const float *tot /* nullable [B]: the strict forward's normalising sums */,
                                  const float *d_z_samples, int64_t B, int Nb, int Nf, float *d_bins, float *d_weights,
                                  snerf_stream_t stream);

/* ---- a2: RenderRayNet -----------------------------------------------------------------------------
 * Mirrors RenderRayNet.__init__ (models/render_ray_net.py:8): n_layers, width, skips as a bit mask
 * over positional_net indices, use_directional_input; positions_dim / directions_dim are expressed
 * through the encoders that feed them (pos_freqs/pos_identity, dir_freqs/dir_identity; 3 input
 * channels each), additional_input_dim = add_dim per-ray constants appended to the position
 * encoding (train.py:154-159). */
typedef struct snerf_mlp_desc {
    int32_t n_layers;     /* 8 */
    int32_t width;        /* 2 .. 512 (--netwidth, config_parser.py:20).  The kernels are built for trunks of 64, 128, 256 and
                             (0.1.8; one wave per SIMD) 320, 384, 448, 512 features; any other width runs zero-padded inside
                             the next larger one (same results, the cost of that kernel).  The split-precision entry points
                             take 256 only; a net above 256 needs at least 17 input columns in its first layer. */
    int32_t pos_freqs;    /* 10 */
    int32_t pos_identity; /* 0 */
    int32_t dir_freqs;    /* 4 */
    int32_t dir_identity; /* 0 */
    int32_t add_dim;      /* 0 */
    uint32_t skip_mask;   /* bit i set <=> i in skips */
    int32_t use_dir;      /* 1 */
    int32_t add_first;    /* 0: input columns [PE(x) | add] (RenderRayNet(additional_input_dim) fed by train.py:154-159
                             style rows [samples_encoding | extra]); 1: [add | PE(x)], the order the append_smpl_params /
                             append_to_nerf pipelines build (models/append_smpl_params_pipeline.py:49-51) */
} snerf_mlp_desc;

/* Number of floats in the flat parameter vector: weights and biases in state_dict order
 * (positions_pose_input.weight, .bias, positional_net.0.weight, ... rgb_out_layer.bias). */
SNERF_API int64_t snerf_mlp_param_floats(const snerf_mlp_desc *desc);
/* Number of floats of the MFMA-ordered weight stream produced by snerf_mlp_pack_f32. */
SNERF_API int64_t snerf_mlp_packed_floats(const snerf_mlp_desc *desc);
/* params_flat -> packed (both device).  Run once per weight update. */
SNERF_API int snerf_mlp_pack_f32(const snerf_mlp_desc *desc, const float *params_flat, float *packed,
                       snerf_stream_t stream);

/* Fused positional encoding + MLP.  x [n, 3] sample positions; directions dirs: [n/samples_per_ray, 3]
 * when dirs_per_sample == 0 (one per ray, samples of a ray contiguous) or [n, 3]; directions are
 * normalised inside (models/nerf_pipeline.py:33-34).  add: nullable [n/samples_per_ray, add_dim].
 * raw [n, 4] = [rgb | sigma] (models/render_ray_net.py:61).
 * dirs_per_sample is a bit set (other bits: SNERF_E_BADARG): bit 0 = directions per sample; bit 1 (SNERF_FWD_NO_RAY_FOLD,
 * snerf_mlp_fwd_ws_f32 only) = multiply the additional-input columns per sample even when a fold workspace is given, in the
 * order of snerf_mlp_fwd_train_f32 (whose `raw` the call then reproduces bit for bit). */
#define SNERF_FWD_DIRS_PER_SAMPLE 1
#define SNERF_FWD_NO_RAY_FOLD 2
SNERF_API int snerf_mlp_fwd_f32(const snerf_mlp_desc *desc, const float *packed, const float *x,
                      const float *dirs, int dirs_per_sample, const float *add,
                      int64_t n, int samples_per_ray, float *raw, snerf_stream_t stream);

/* The same call with a caller-allocated workspace for the per-ray fold: nets with additional inputs (add_dim > 0) read them
 * as per-RAY constants, so W_add . add is evaluated once per ray into a table of snerf_mlp_fold_workspace_bytes(desc, n,
 * samples_per_ray) bytes (0 when the fold does not apply: no additional inputs, fewer than 8 samples per ray, ...) and added to
 * the accumulators; their k-blocks are skipped (same values up to the summation order of those columns).  workspace NULL
 * (= snerf_mlp_fwd_f32): the per-sample form.  A workspace smaller than needed is SNERF_E_BADARG - the library allocates
 * nothing and never switches form silently.  16-byte aligned. */
SNERF_API int64_t snerf_mlp_fold_workspace_bytes(const snerf_mlp_desc *desc, int64_t n, int samples_per_ray);
SNERF_API int snerf_mlp_fwd_ws_f32(const snerf_mlp_desc *desc, const float *packed, const float *x, const float *dirs,
                         int dirs_per_sample, const float *add, int64_t n, int samples_per_ray, float *raw, void *workspace,
                         int64_t workspace_bytes, snerf_stream_t stream);

/* ---- fp32 inference on the composed stream ------------------------------------------------------------------
 * additional_linear_layer, sigma_out_layer, directional_input and directional_net[0] (models/render_ray_net.py:51-59) follow
 * each other without an activation: for fixed weights, sigma = (w_s W_a) h + (w_s b_a + b_s) and the input of the last ReLU
 * = (W_n W_d1 W_a) h + (W_n W_d2) PE(d) + (W_n (W_d1 b_a + b_d) + b_n), h the last trunk activation.  The inference stream
 * holds the trunk and the rgb head as snerf_mlp_pack_f32 does and these two composed layers (every composed entry a float64
 * sum in a fixed order, rounded once to fp32): 67 slabs instead of 77 for the default net, 2088 instead of 2408 matrix
 * operations per 16 samples - 2 x 525 952 FLOP per evaluation executed for the reference network's 1 215 744.  Results
 * differ from snerf_mlp_fwd_f32's at round-off level (same error class against float64).  Re-pack after every weight update.
 * snerf_mlp_packed_infer_floats: floats of stream + scratch (float64 intermediates behind the stream: the library
 * allocates nothing); 0 - not an error - when there is no inference stream for the net (widths above 256,
 * SNERF_MLP_COMPOSE=0 in the environment): the caller then uses snerf_mlp_pack_f32 / snerf_mlp_fwd_ws_f32.
 * snerf_mlp_fwd_infer_f32: arguments and per-ray fold as snerf_mlp_fwd_ws_f32 (workspace NULL: the per-sample form);
 * small calls equal the same rows of a large call bit for bit.  No training forward reads this stream. */
SNERF_API int64_t snerf_mlp_packed_infer_floats(const snerf_mlp_desc *desc);
SNERF_API int snerf_mlp_pack_infer_f32(const snerf_mlp_desc *desc, const float *params_flat, float *packed_infer,
                             snerf_stream_t stream);
SNERF_API int snerf_mlp_fwd_infer_f32(const snerf_mlp_desc *desc, const float *packed_infer, const float *x, const float *dirs,
                            int dirs_per_sample, const float *add, int64_t n, int samples_per_ray, float *raw, void *workspace,
                            int64_t workspace_bytes, snerf_stream_t stream);
/* `precision` of snerf_render_rays_f32 / _add_f32 / _smpl_f32: the fp32 kernels, packed_* from snerf_mlp_pack_infer_f32
 * (the warp net of _smpl_f32 runs its fp32 kernel on snerf_warp_pack_f32's stream). */
#define SNERF_FP32_INFER 32

/* ---- a2 on the bf16 matrix cores with fp32-class accuracy (split-bf16, inference) -------------------------
 * Every fp32 operand is split into nsplit bf16 parts and the cross terms are accumulated in fp32:
 * nsplit = 3 (6 products, ~2^-24 relative: same parity class as the fp32 kernel, 2.7x less matrix-pipe time),
 * nsplit = 2 (3 products, ~2^-16 relative: RGB within ~8e-5, 5.3x less).  Same inputs/outputs as
 * snerf_mlp_fwd_f32; `packed` comes from snerf_mlp_pack_bf16 with the same nsplit.  Width 256 only.
 * nsplit = SNERF_SPLIT_F16X3 selects two fp16 parts instead (3 products, ~2^-22 relative: raw outputs within the fp32
 * kernel's own tolerance, at the speed of nsplit = 2): operands are scaled by exact powers of two - weights per layer at
 * pack time, activations (and, in the backward, gradients) per sample in the kernel - so that fp16's range is never
 * left.  Accepted wherever an nsplit / precision is: forward, training forward, snerf_render_rays*, and the backward
 * entry points (dgrad with per-sample scales; the wide wgrad GEMMs, which contract over samples, with per-layer scales
 * taken from the exponents the f16x3 training forward leaves behind the rows of `act` and the f16x3 dgrad behind those
 * of `dy`: an f16x3 backward therefore needs the `act` of an f16x3 training forward). */
#define SNERF_SPLIT_F16X3 16
SNERF_API int64_t snerf_mlp_packed_bf16_bytes(const snerf_mlp_desc *desc, int nsplit);
SNERF_API int snerf_mlp_pack_bf16(const snerf_mlp_desc *desc, const float *params_flat, void *packed, int nsplit,
                        snerf_stream_t stream);
SNERF_API int snerf_mlp_fwd_bf16_f32(const snerf_mlp_desc *desc, const void *packed, int nsplit, const float *x,
                           const float *dirs, int dirs_per_sample, const float *add, int64_t n,
                           int samples_per_ray, float *raw, snerf_stream_t stream);
/* The same forward for training: additionally saves every layer input into `act`, in exactly the layout
 * snerf_mlp_fwd_train_f32 writes (act_floats of snerf_mlp_train_sizes), so that snerf_mlp_bwd_f32 /
 * snerf_mlp_bwd_inputs_f32 run on it unchanged (any mix of fp32 / split-bf16 forward and backward works: the buffers are
 * fp32 - except that the f16x3 backward needs the f16x3 forward, see SNERF_SPLIT_F16X3). */
SNERF_API int snerf_mlp_fwd_train_bf16_f32(const snerf_mlp_desc *desc, const void *packed, int nsplit, const float *x,
                                 const float *dirs, int dirs_per_sample, const float *add, int64_t n,
                                 int samples_per_ray, float *raw, float *act, snerf_stream_t stream);

/* The backward on the bf16 matrix cores: dgrad (the transposed network) with split-bf16 operands, fp32 accumulate
 * and fp32 stored d Y, and the wide wgrad GEMMs (the 256x256 and 128x256 layers) with both operands split the same
 * way; the narrow wgrad jobs and the reduction are exact fp32 (SNERF_WGRAD_BF16=0: all of wgrad in fp32).  Same buffers as snerf_mlp_bwd_f32 / _bwd_inputs_f32
 * (sizes from snerf_mlp_train_sizes) except the transposed weight stream, which comes from snerf_mlp_pack_t_bf16. */
SNERF_API int64_t snerf_mlp_packed_t_bf16_bytes(const snerf_mlp_desc *desc, int nsplit, int input_grad);
SNERF_API int snerf_mlp_pack_t_bf16(const snerf_mlp_desc *desc, const float *params_flat, void *packed_t, int nsplit,
                          int input_grad, snerf_stream_t stream);
SNERF_API int snerf_mlp_bwd_bf16_f32(const snerf_mlp_desc *desc, const void *packed_t, int nsplit, const float *act,
                           const float *d_raw, int64_t n, float *dy, float *gpart, float *flat_grad,
                           snerf_stream_t stream);
SNERF_API int snerf_mlp_bwd_inputs_bf16_f32(const snerf_mlp_desc *desc, const void *packed_t, int nsplit, const float *act,
                                  const float *d_raw, const float *x, const float *dirs, int dirs_per_sample,
                                  int samples_per_ray, int64_t n, float *dy, float *gpart, float *flat_grad,
                                  float *d_x, float *d_dirs, snerf_stream_t stream);

/* ---- a2 backward (training) ------------------------------------------------------------------------
 * Buffer sizes for n samples: activations saved by the forward, per-layer output gradients, the
 * transposed weight stream, the split-K partial gradients (gpart_count chunks). */
SNERF_API int snerf_mlp_train_sizes(const snerf_mlp_desc *desc, int64_t n, int64_t *act_floats, int64_t *dy_floats,
                          int64_t *packed_t_floats, int64_t *gpart_floats, int32_t *gpart_count);
/* Where the backward leaves the per-layer output gradients in `dy` (an output, not only scratch: gradients w.r.t.
 * per-ray additional inputs and w.r.t. already-encoded input rows are contractions of these with weight columns, see
 * smpl_nerf_amd/nets.py).  Layers in snerf_mlp_param_floats order (positions_pose_input, positional_net[*],
 * additional_linear_layer, sigma_out_layer, directional_input, directional_net[0], rgb_out_layer); arrays of
 * SNERF_MAX_MLP_LAYERS entries, each nullable.  d Y_l[s, f] (sample s of n, output feature f < n_out[l]) is the float at
 *     dy[((first_row[l] + f / 16) * n + s) * 16 + f % 16]                                   (tile-row-major) */
#define SNERF_MAX_MLP_LAYERS 21
SNERF_API int snerf_mlp_dy_layout(const snerf_mlp_desc *desc, int32_t *n_layers, int32_t *first_row, int32_t *n_out, int32_t *n_in);
/* Gradients w.r.t. inputs that enter a layer through plain weight columns - per-ray additional inputs, already-encoded input
 * rows, the pose rows of the warp net - as contractions of a stored d Y_l with those columns (what autograd leaves in the
 * .grad of x when y = x W^T; models/render_ray_net.py:43-50, models/append_vertices_pipeline.py:30-58):
 *     out[s, out_col0 + c] (+)= sum_{f < n_feat} d Y_l[s, f] * w[f, col0 + c],   c < ncols
 * dy / first_row: the backward's `dy` buffer and the layer's first tile-row (snerf_mlp_dy_layout; the warp net's layer 0 is
 * tile-row 0); w [n_feat, w_stride] row-major = the layer's weight matrix in params_flat (n_feat <= 256).
 * samples_per_ray == 0: one output row per sample, out [n, out_stride].  samples_per_ray > 0: the rows of a ray's samples
 * are summed (the pipelines expand one input row per ray over its samples), out [n / samples_per_ray, out_stride];
 * scratch: snerf_dy_contract_scratch_floats(n, ncols, samples_per_ray) floats.  accumulate != 0: out += (several layers
 * read the same inputs: layer 0 and every skip layer). */
SNERF_API int64_t snerf_dy_contract_scratch_floats(int64_t n, int ncols, int samples_per_ray);
SNERF_API int snerf_dy_contract_f32(const float *dy, int64_t n, int first_row, int n_feat, const float *w, int w_stride, int col0,
                          int ncols, int samples_per_ray, float *out, int64_t out_stride, int out_col0, int accumulate,
                          float *scratch, snerf_stream_t stream);

/* snerf_mlp_fwd_f32 that also saves every layer input into `act` (act_floats): fp32 tile-rows, followed by one
 * sign bit per ReLU output (the masks the split-bf16 dgrad reads instead of the activation rows). */
SNERF_API int snerf_mlp_fwd_train_f32(const snerf_mlp_desc *desc, const float *packed, const float *x,
                            const float *dirs, int dirs_per_sample, const float *add, int64_t n,
                            int samples_per_ray, float *raw, float *act, snerf_stream_t stream);
/* The same for already-encoded rows (RenderRayNet.forward(x) under autograd). */
SNERF_API int snerf_mlp_fwd_encoded_train_f32(const snerf_mlp_desc *desc, const float *packed, const float *x_enc,
                                    int64_t n, int64_t row_floats, float *raw, float *act,
                                    snerf_stream_t stream);
/* params_flat -> transposed weight stream for the dgrad kernel (once per weight update).  input_grad != 0
 * adds the encoder-column transposes snerf_mlp_bwd_inputs_f32 consumes (a different stream: pack one per use). */
SNERF_API int snerf_mlp_pack_t_f32(const snerf_mlp_desc *desc, const float *params_flat, float *packed_t,
                         int input_grad, snerf_stream_t stream);
/* d_raw [n,4] -> flat_grad (snerf_mlp_param_floats floats, state_dict order, OVERWRITTEN): what
 * autograd leaves in .grad of the 26 parameter tensors after (raw * d_raw).sum().backward().
 * dy, gpart: scratch (snerf_mlp_train_sizes).  Three launches: dgrad, split-K wgrad, reduce. */
SNERF_API int snerf_mlp_bwd_f32(const snerf_mlp_desc *desc, const float *packed_t, const float *act,
                      const float *d_raw, int64_t n, float *dy, float *gpart, float *flat_grad,
                      snerf_stream_t stream);

/* snerf_mlp_bwd_f32 that also back-propagates into the inputs of snerf_mlp_fwd_train_f32: d_x [n,3] (through
 * the position encoding of layer 0 and the skip layers) and d_dirs [n,3] (through the direction encoding and
 * the normalisation d/|d|, models/smpl_nerf_pipeline.py:54-56).  Needs the input_grad=1 transposed stream.
 * Encoders of up to 8 position / 8 direction k-blocks of 16 slots (identity columns, up to 16 frequencies); the
 * split-precision variant (snerf_mlp_bwd_inputs_bf16_f32) takes the default-sized ones (<= 4 / 2 k-blocks: L = 10 / 4
 * without identity columns, or smaller). */
SNERF_API int snerf_mlp_bwd_inputs_f32(const snerf_mlp_desc *desc, const float *packed_t, const float *act,
                             const float *d_raw, const float *x, const float *dirs, int dirs_per_sample,
                             int samples_per_ray, int64_t n, float *dy, float *gpart, float *flat_grad,
                             float *d_x, float *d_dirs, snerf_stream_t stream);

/* Same network on already-encoded rows x_enc [n, row_floats] (the literal RenderRayNet.forward(x)
 * signature): positions_pose = x[:, :positions_dim+add_dim], directions = x[:, -directions_dim:]
 * (models/render_ray_net.py:42-43). */
SNERF_API int snerf_mlp_fwd_encoded_f32(const snerf_mlp_desc *desc, const float *packed, const float *x_enc,
                              int64_t n, int64_t row_floats, float *raw, snerf_stream_t stream);

/* ---- a7: WarpFieldNet fused with x' = x + warp and the per-sample view direction ---------------------
 * Mirrors WarpFieldNet.__init__ (models/warp_field_net.py:8-15): linear1 [width, positions_dim+pose_dim],
 * linear2 [3, width]; positions_dim is expressed through the position encoder. */
typedef struct snerf_warp_desc {
    int32_t width;        /* 1 .. 256 (--netwidth_warp); other widths than 256 / 128 run zero-padded; split precision: 256 */
    int32_t pos_freqs;    /* 10 */
    int32_t pos_identity; /* 0 */
    int32_t pose_dim;     /* 40 = encoded pose of the two joints (models/smpl_nerf_pipeline.py:28-30) */
} snerf_warp_desc;
SNERF_API int64_t snerf_warp_param_floats(const snerf_warp_desc *desc); /* linear1.weight, .bias, linear2.weight, .bias */
SNERF_API int64_t snerf_warp_packed_floats(const snerf_warp_desc *desc);
SNERF_API int snerf_warp_pack_f32(const snerf_warp_desc *desc, const float *params_flat, float *packed,
                        snerf_stream_t stream);
/* x [n,3], pose_enc [n/samples_per_ray, pose_dim], o [n/samples_per_ray, 3] ->
 * warp [n,3] = net([PE(x) | pose_enc]) (models/warp_field_net.py:17-21),
 * warped [n,3] = x + warp (models/smpl_nerf_pipeline.py:49), sdirs [n,3] = warped - o (:52-53).
 * warped / sdirs nullable.  With pos_freqs = pos_identity = 0 the net reads only pose_enc rows
 * (x may be NULL): the literal WarpFieldNet.forward(x_rows) with samples_per_ray = 1. */
SNERF_API int snerf_warp_fwd_f32(const snerf_warp_desc *desc, const float *packed, const float *x,
                       const float *pose_enc, const float *o, int64_t n, int samples_per_ray,
                       float *warp, float *warped, float *sdirs, snerf_stream_t stream);

/* With a caller-allocated workspace of snerf_warp_fold_workspace_bytes(desc, n, samples_per_ray) bytes (0: the fold does not
 * apply) the pose columns of linear1 - per-ray constants - are folded into one vector per ray; NULL (= snerf_warp_fwd_f32):
 * the per-sample form; too small: SNERF_E_BADARG.  Same contract as snerf_mlp_fwd_ws_f32. */
SNERF_API int64_t snerf_warp_fold_workspace_bytes(const snerf_warp_desc *desc, int64_t n, int samples_per_ray);
SNERF_API int snerf_warp_fwd_ws_f32(const snerf_warp_desc *desc, const float *packed, const float *x, const float *pose_enc,
                          const float *o, int64_t n, int samples_per_ray, float *warp, float *warped, float *sdirs,
                          void *workspace, int64_t workspace_bytes, snerf_stream_t stream);

/* The same forward on the bf16 matrix cores (split-bf16, always three parts / six products: fp32-class accuracy - the warp
 * moves the sample in front of the 2^9 band of the position encoding).  packed from snerf_warp_pack_bf16
 * (snerf_warp_packed_bf16_bytes bytes).  Fused mode only (x given); width 256. */
SNERF_API int64_t snerf_warp_packed_bf16_bytes(const snerf_warp_desc *desc);
SNERF_API int snerf_warp_pack_bf16(const snerf_warp_desc *desc, const float *params_flat, void *packed, snerf_stream_t stream);
SNERF_API int snerf_warp_fwd_bf16_f32(const snerf_warp_desc *desc, const void *packed, const float *x, const float *pose_enc,
                            const float *o, int64_t n, int samples_per_ray, float *warp, float *warped, float *sdirs,
                            snerf_stream_t stream);

/* Training of the warp net: forward that saves [PE(x) | pose | h] tile-rows, the transposed head, and the
 * backward d_warp [n,3] (= d loss / d warp, the sum of what arrives through warp, warped and sdirs) ->
 * flat_grad (snerf_warp_param_floats floats, state_dict order, overwritten).  Sizes as snerf_mlp_train_sizes. */
SNERF_API int snerf_warp_train_sizes(const snerf_warp_desc *desc, int64_t n, int64_t *act_floats, int64_t *dy_floats,
                           int64_t *packed_t_floats, int64_t *gpart_floats);
SNERF_API int snerf_warp_fwd_train_f32(const snerf_warp_desc *desc, const float *packed, const float *x,
                             const float *pose_enc, const float *o, int64_t n, int samples_per_ray,
                             float *warp, float *warped, float *sdirs, float *act, snerf_stream_t stream);
SNERF_API int snerf_warp_pack_t_f32(const snerf_warp_desc *desc, const float *params_flat, float *packed_t,
                          snerf_stream_t stream);
SNERF_API int snerf_warp_bwd_f32(const snerf_warp_desc *desc, const float *packed_t, const float *act,
                       const float *d_warp, int64_t n, float *dy, float *gpart, float *flat_grad,
                       snerf_stream_t stream);

/* ---- DynamicPipeline: the vertex-attention warp (models/dynamic_pipeline.py:53-74) --------------------------
 * samples [B,S,3], goal / canon [B,V,3] (the body model's goal and canonical vertices), ray_o [B,3] ->
 * warp [B*S,3] = sum_v a_v (canon_v - goal_v) with a = modified_softmax(temperature * relu(radius - |sample - goal_v|))
 * over the V vertices (utils.py:57-60), warped [B*S,3] = sample + warp (:66), sdirs [B*S,3] = warped - ray_o (:70): the
 * trio of snerf_warp_fwd_f32.  No [B,S,V] tensor exists: the softmax is taken with the per-sample maximum m removed.
 * stats [B*S,2] = (m, Z = sum_v exp(x_v - m)) is what the backward reads; NULL when no backward follows.
 * Any B >= 0 (0: no-op), S >= 1, V >= 1; radius > 0, temperature >= 0 (else SNERF_E_BADARG).  Two calls on the same
 * inputs give the same bits. */
SNERF_API int snerf_vertex_warp_fwd_f32(const float *samples, const float *goal, const float *canon, const float *ray_o,
                              int64_t B, int S, int V, float radius, float temperature, float *warp, float *warped,
                              float *sdirs, float *stats, snerf_stream_t stream);
/* Its backward: warp and stats from the forward; d_warp / d_warped / d_sdirs [B*S,3] are the gradients arriving at the
 * three outputs (each nullable, not all: their sum is d loss / d warp) -> d_goal, d_canon [B,V,3] and, unless NULL,
 * d_samples [B,S,3] = the part of d loss / d samples that flows through the attention (warped's own identity term is
 * the caller's).  Every element is written (zeros where nothing is in radius); no atomics: the same bits on every call.
 * torch's conventions: relu' (0) = 0, no gradient through a zero distance. */
SNERF_API int snerf_vertex_warp_bwd_f32(const float *samples, const float *goal, const float *canon, const float *warp,
                              const float *stats, const float *d_warp, const float *d_warped, const float *d_sdirs,
                              int64_t B, int S, int V, float radius, float temperature, float *d_samples, float *d_goal,
                              float *d_canon, snerf_stream_t stream);

/* ---- The image-wise model: linear-attention warp with ONE body per image (solver/image_wise_solver.py:89-105) ----------------
 * samples [B,S,3] (N = B S, flat), goal / canon [V,3] (the one body of the image, shared by every ray), ray_o [B,3] ->
 *   x_sv = max(radius - |sample_s - goal_v|, 0)      D_s = sum_v x_sv + eps      warp_s = (sum_v x_sv (canon_v - goal_v)) / D_s
 * warp [N,3], warped [N,3] = sample + warp, sdirs [N,3] = warped - ray_o[s / S]: the trio of snerf_vertex_warp_fwd_f32.
 * No softmax, no temperature; nothing of size N V or B V exists.  fp32 in and out; the pairs inside the radius are evaluated in
 * float64 (radius and eps are doubles for that reason) and warp is rounded once; warped and sdirs are the fp32 sums of the
 * rounded warp.  stats [N,4] float64 = (D_s, warp_s unrounded) is what the backward reads; NULL when no backward follows.
 * A sample with nothing in its radius has warp = 0 / eps = 0 (with eps = 0 it is the reference's 0 / 0).
 * Any B >= 0 (0: no-op), S >= 1, V >= 1; radius > 0, eps >= 0 (else SNERF_E_BADARG; a bad scalar is an error whatever B is);
 * stats 8-byte aligned (SNERF_E_ALIGN).  Two calls on the same inputs give the same bits. */
SNERF_API int snerf_image_warp_fwd_f32(const float *samples, const float *goal, const float *canon, const float *ray_o,
                              int64_t B, int S, int V, double radius, double eps, float *warp, float *warped, float *sdirs,
                              double *stats, snerf_stream_t stream);
/* Bytes of the backward's workspace for N = B S samples and V vertices: the per-slab partial sums [slabs, V, 6] in float64.  The
 * slab count is a function of N alone (at most 64 slabs of at least 8 chunks of 64 samples), never of the device.  -1 on a bad
 * argument. */
SNERF_API int64_t snerf_image_warp_bwd_workspace_bytes(int64_t N, int V);
/* Its backward: stats from the forward (eps travels in it); d_warp / d_warped / d_sdirs [N,3] are the gradients arriving at the
 * three outputs (each nullable, not all: their sum is d loss / d warp) -> d_goal, d_canon [V,3], summed over all N samples, and,
 * unless NULL, d_samples [N,3] = d loss / d samples: what flows through the attention plus d_warped + d_sdirs, the identity
 * paths of the two derived outputs.  Every element is written (zeros where nothing is in radius) and every workspace word that is
 * read was written by the same call; no atomics, slabs added in slab order, each output rounded to fp32 once: the same bits on
 * every call and every device.  A workspace that is NULL or smaller than snerf_image_warp_bwd_workspace_bytes(B S, V) is
 * SNERF_E_BADARG; stats and workspace 8-byte aligned (SNERF_E_ALIGN).
 * torch's conventions: relu' (0) = 0, no gradient through a zero distance. */
SNERF_API int snerf_image_warp_bwd_f32(const float *samples, const float *goal, const float *canon, const double *stats,
                              const float *d_warp, const float *d_warped, const float *d_sdirs, int64_t B, int S, int V,
                              double radius, void *workspace, int64_t workspace_bytes, float *d_samples, float *d_goal,
                              float *d_canon, snerf_stream_t stream);

/* ---- SmplNerfSolver's canonical-density loss: pdf of a Gaussian mixture (utils.py:72-111, solver/smpl_nerf_solver.py:39-41) ----
 * samples [n,3] (any leading shape, flattened), means [V,3] (one isotropic Gaussian of standard deviation std per canonical body
 * vertex, equal weights) ->
 *   pdf[i]    = factor / V * sum_v exp(-|x_i - mu_v|^2 / (2 std^2)),   factor = 1 / sqrt((2 pi)^3 std^6)   (utils.py:84-110)
 *   dpdf[i,:] = d pdf[i] / d x_i = -factor / (V std^2) * sum_v exp(...) (x_i - mu_v)       [n,3]; NULL: not computed (inference)
 * One pass over the n*V pairs, one hardware exp per pair, nothing of size n*V in memory; no atomics, fixed summation order: two
 * calls give the same bits.  Every element of pdf (and dpdf) is written; a pdf that underflows is 0, not NaN.
 * n >= 0 (0: SNERF_OK whatever the pointers are), V >= 1, std > 0 (NaN refused), V*3 and ceil(n/64) below 2^31; samples, means and
 * pdf non-null - else SNERF_E_BADARG before anything touches a device; a bad scalar is an error whatever n is. */
SNERF_API int snerf_gmm_pdf_f32(const float *samples, const float *means, int64_t n, int V, float std, float *pdf, float *dpdf,
                              snerf_stream_t stream);

/* ---- The SMPL body model: linear blend skinning (Loper et al. 2015) with smplx's conventions --------------------------------
 * What DynamicPipeline and AppendVerticesPipeline call as smpl_model(betas=, body_pose=, global_orient=).vertices, one pose per
 * ray.  B poses, V vertices, J joints, NB shape coefficients, P = 9 (J - 1), K = NB + P:
 *   1  full_pose = [global_orient (3) | body_pose (3 (J - 1))]: J axis-angle vectors r_j
 *   2  angle = |r + 1e-8| (1e-8 added to each component), dir = r / angle, R = I + sin(angle) K + (1 - cos(angle)) K^2, K = skew(dir)
 *   3  pose_feature = R[1:] - I, flattened (joint, row, column): P values
 *   4  v_shaped = v_template + shapedirs betas        5  J_rest = J_regressor v_shaped        6  v_posed = v_shaped + posedirs pose_feature
 *   7  G_0 = [R_0 | J_0], G_j = G_parent [R_j | J_j - J_parent], A_j = [G_j.R | G_j.t - G_j.R J_j]
 *   8  T_v = sum_j W[v,j] A_j        9  vertex_v = T_v [v_posed_v; 1]        10  joints_j = G_j.t
 * The model record: device arrays laid out once at load, and the parent table on the HOST (it is validated before anything is
 * launched and travels in the kernel arguments).
 *   v_template [V,3]
 *   blend      [K, 3V]: row n < NB is shapedirs[:, :, n], row NB + p is posedirs[:, :, p], each flattened (vertex, xyz)
 *   J_template [J,3] = J_regressor v_template and J_dirs [J,3,NB] = J_regressor shapedirs (steps 4-5 folded, in float64)
 *   weights    [V,J]   skinning weights, any sparsity
 *   parents    [J]     HOST int32: parents[0] = -1, 0 <= parents[j] < j
 * 2 <= J <= 32, NB >= 1, K <= 512, V >= 1 - else SNERF_E_BADARG, as for every argument error here, before anything touches a device. */
typedef struct snerf_smpl_model {
    int32_t V, J, NB;
    const float *v_template, *blend, *J_template, *J_dirs, *weights;
    const int32_t *parents;
} snerf_smpl_model;
/* betas [betas_rows, NB] with betas_rows 1 (shared by the batch) or B; body_pose [B, 3 (J - 1)]; global_orient [B,3] or NULL = zeros
 * -> vertices [B,V,3]; joints [B,J,3] unless NULL; rig [B, 12 J + K] = per pose the J transforms A_j (3 x 4, row-major), then betas
 * and pose_feature: the record the vertex stage and the backward read (always written: it is also the forward's own hand-over
 * between its rig and vertex stages).  Nothing else of size B V is read or written.  Any B >= 0 (0: no-op).  Every element of every
 * output is written; two calls give the same bits.  fp32 in and out; the per-pose chain (steps 2, 5, 7, 10: B J work) is evaluated in
 * float64 and rounded once, the sums over K and over the joints are fp32 fused multiply-adds with the template added last. */
SNERF_API int snerf_smpl_lbs_fwd_f32(const snerf_smpl_model *model, const float *betas, int betas_rows, const float *body_pose,
                              const float *global_orient, int64_t B, float *vertices, float *joints, float *rig,
                              snerf_stream_t stream);
/* Bytes of the backward's workspace for B poses (vertex-slice partial sums, their sum, d_betas rows); -1 on a bad argument. */
SNERF_API int64_t snerf_smpl_lbs_bwd_workspace_bytes(const snerf_smpl_model *model, int64_t B);
/* Its backward: the forward's inputs and rig; d_vertices [B,V,3] and d_joints [B,J,3] are the incoming gradients (each nullable, not
 * both) -> d_betas [betas_rows, NB] (with one row: the sum over the batch), d_body_pose [B, 3 (J - 1)], d_global_orient [B,3]; each
 * output nullable, every element of a non-NULL one written.  v_posed and T_v are recomputed: the forward keeps no [B,V] tensor.
 * The sums over the vertices go through vertex slices in the workspace and a fixed-order reduce - no atomics, the same bits on every
 * call.  The Rodrigues formula is differentiated as written in step 2, 1e-8 included: finite at the zero pose. */
SNERF_API int snerf_smpl_lbs_bwd_f32(const snerf_smpl_model *model, const float *betas, int betas_rows, const float *body_pose,
                              const float *global_orient, const float *rig, const float *d_vertices, const float *d_joints,
                              int64_t B, void *workspace, int64_t workspace_bytes, float *d_betas, float *d_body_pose,
                              float *d_global_orient, snerf_stream_t stream);

/* ---- The vertex_sphere model: ray-mesh hits and the sphere warp (datasets/vertex_sphere_dataset.py:84-160) -------------------
 * All hits of R rays on one triangle mesh.  origins, dirs [R,3]; vertices [V,3]; faces [F,3] int32 indices into vertices;
 * max_hits = K in 1 .. 16 -> t_hits [R,K], n_hits [R] int32.
 * Intersection rule: two-sided Moeller-Trumbore in fp32, for triangle (a, b, c) of faces.
 *   e1 = b - a, e2 = c - a, p = d x e2, det = e1 . p.
 *   u = (o - a) . p / det, q = (o - a) x e1, v = d . q / det, t = e2 . q / det.
 *   A hit is det != 0, u >= 0, v >= 0, u + v <= 1, t > 0.
 *   There is no back-face culling: trimesh's intersector is two-sided.
 *   t is in units of |d|.  The reference normalises its directions (:79), so t is the distance it computes with
 *   torch.norm(hit - origin).
 *   Products and sums are kept apart, as the build already does (-ffp-contract=off); a dot product is (x0 y0 + x1 y1) + x2 y2.
 * Outputs: t_hits[r, :] holds the K smallest hit parameters in ascending order, padded with +inf.  n_hits[r] is the total number
 *   of hits.  It may exceed K, and the caller can see that the list was cut.  Every element of both outputs is written.  Two
 *   calls give the same bits.
 * Not promised: a ray through a shared edge or vertex may count once or twice, and nothing is pinned relative to trimesh's own
 *   tolerances.
 * workspace: snerf_ray_mesh_workspace_bytes(F) bytes (36 F: a, e1, e2 per face, written by a pre-pass of every call); nothing of
 *   size R F exists in memory.
 * Argument checks, on the host before any device work: R = 0 is a no-op returning 0, also with null pointers; a bad scalar is an
 *   error whatever R is.  A required null pointer, max_hits outside 1 .. 16, V < 1, F < 1, 3 V or 9 F or ceil(R/64) not below
 *   2^31, and a workspace that is missing or too small are SNERF_E_BADARG with a message naming the argument.  Face indices in
 *   [0, V) are a precondition of this entry (the Python operator rejects a bad table before any launch). */
SNERF_API int64_t snerf_ray_mesh_workspace_bytes(int F);   /* -1 on a bad F */
SNERF_API int snerf_ray_mesh_hits_f32(const float *origins, const float *dirs, const float *vertices, const int32_t *faces, int64_t R,
                              int V, int F, int max_hits, float *t_hits, int32_t *n_hits, void *workspace,
                              int64_t workspace_bytes, snerf_stream_t stream);
/* The first hit of every ray, with its face and where on it (render.py:222-319, get_warp: what create_dataset.py saves as the depth
 * and the warp image of datasets/single_sample_dataset.py).  Inputs, intersection rule, workspace and the order of the host
 * checks are snerf_ray_mesh_hits_f32's; t equals its t_hits[r, 0] with max_hits = 1, bit for bit.
 *   The first hit of ray r is its hit with the smallest t; of hits with equal t it is the one with the smaller face index.
 * -> t [R]: the hit parameter, +inf on a miss; face [R] int32: the index into faces, -1 on a miss; uv [R,2]: u and v of that pair
 *   as the rule divides them, 0 on a miss.  The hit point is (1 - u - v) a + u b + v c.
 * canon, warp, depth: all NULL, or all non-NULL.  canon [V,3] is the same mesh in another (the canonical) pose, and then
 *   depth [R] = t |d|, |d| = sqrtf((dx dx + dy dy) + dz dz): the distance of the hit from the origin, 0 on a miss (the marker of
 *              single_sample_dataset.py:116);
 *   warp [R,3] = ((ca + u (cb - ca)) + v (cc - ca)) - (o + d t) with ca, cb, cc the rows of canon that faces[face] names:
 *              the hit point's way to the same surface point of the canonical body, 0 on a miss.
 *   The reference solves goal_vertices^T x = hit for x per ray and forms canonical_vertices^T x; x = (1 - u - v, u, v) wherever
 *   the face's plane misses the world origin, and its solve is singular where it does not - which is not kept.
 * Every element of every non-NULL output is written; no atomics, nothing of size R F; two calls give the same bits.
 * Argument checks as above (R = 0: SNERF_OK whatever the pointers are); a null t, face or uv and a mix of null and non-null among
 *   canon, warp and depth are SNERF_E_BADARG. */
SNERF_API int snerf_ray_mesh_first_hit_f32(const float *origins, const float *dirs, const float *vertices, const int32_t *faces,
                              int64_t R, int V, int F, const float *canon, float *t, int32_t *face, float *uv, float *warp,
                              float *depth, void *workspace, int64_t workspace_bytes, snerf_stream_t stream);
/* The sphere warp (:128-159).  samples [n,3]; goal, canon [V,3]: ONE body in the goal and in the canonical pose (the data set has
 * one pose per image).  d_v = sqrtf(|p - g_v|^2), the square summed as (dx^2 + dy^2) + dz^2, and the three-way weight
 * w(d) = 1 where d < radius, 0 where d > radius, d itself where they are equal (the reference's two masked assignments leave an
 * equal distance in place).
 *   by_mean = 0 (:147-158)  i = argmin_v d_v, the lowest index on a tie as torch.argmin; warp = w(d_i) (canon_i - goal_i);
 *                           nearest = i; count = (d_i < radius)
 *   by_mean = 1 (:134-145)  warp = sum_v w(d_v) (canon_v - goal_v) / (sum_v w(d_v) + 1e-10), summed in a fixed order;
 *                           count = the number of vertices with d_v < radius; nearest is still the argmin
 * -> warp [n,3]; nearest [n], count [n] int32, each nullable.  Every element of a non-NULL output is written; no atomics; two
 * calls give the same bits.  There is no backward: the warp is data of the batch (data[4]), not differentiated through.
 * n >= 0 (0: SNERF_OK whatever the pointers are), V >= 1, radius finite and positive, 3 V and ceil(n/64) below 2^31; samples,
 * goal, canon, warp non-null - else SNERF_E_BADARG before anything touches a device; a bad scalar is an error whatever n is. */
SNERF_API int snerf_vertex_sphere_warp_f32(const float *samples, const float *goal, const float *canon, int64_t n, int V, float radius,
                              int by_mean, float *warp, int32_t *nearest, int32_t *count, snerf_stream_t stream);

/* ---- The mesh renderer: textured, lit frames of a posed body (create_dataset.py:106-129 through render.py:322-367) ----------------
 * One call renders N frames of H x W pixels of one triangle mesh per frame, seen through pinhole cameras.
 * Inputs: poses [N,4,4] float64 camera-to-world, row-major, and focal, as snerf_raygen_f64 takes them; vertices [Nv,V,3] with
 *   Nv = 1 (one body for all frames) or Nv = N (one per frame); faces [F,3] int32; vf_offsets [V+1], vf_faces [3F] int32: for
 *   every vertex its incident faces in ascending face index, as a CSR table (vertex v owns vf_faces[vf_offsets[v] ..
 *   vf_offsets[v+1])); uv [V,2]: one texture coordinate per vertex; texture [Ht,Wt,3] in [0,1]; args; optionally canon [V,3].
 * Rays: pixel (row j, column i) of frame n has the origin and the direction snerf_raygen_f64 gives ray index (n H + j) W + i:
 *   float32 i - W 0.5 and -(j - H 0.5), float64 divide by focal, float64 rotation summed left to right, rounded once to fp32.  In
 *   camera space these directions have z = -1, so t is the z-depth and t |d| the distance from the camera.
 * Hit: the intersection rule, the first-hit order (the smallest t; the smaller face index on equal t) and the miss markers of
 *   snerf_ray_mesh_first_hit_f32.  t [N,H,W], face [N,H,W] int32, bary [N,H,W,2] (its uv) and, with canon, depth [N,H,W] and
 *   warp [N,H,W,3] equal, bit for bit, what that entry returns for these rays, frame by frame.
 * Image [N,H,W,3], per hit pixel with (u, v) = bary, w0 = (1 - u) - v, (a, b, c) = faces[face], products and sums kept apart,
 *   mix(x) = (w0 x_a + u x_b) + v x_c and dot = (x0 y0 + x1 y1) + x2 y2:
 *     vertex normals  n_v = the sum, over the incident faces of v in CSR order, of e1 x e2 = (b - a) x (c - a), not normalised
 *                     (area-weighted; each cross component is one product minus the other)
 *     normal          m = mix(n);  n = m / sqrtf((mx mx + my my) + mz mz), 0 where that root is 0
 *     light           l = column 2 of the frame's rotation (the camera's +z, towards the viewer) rounded to fp32: a directional
 *                     light at the camera pose, as the reference places it
 *     shade           lambert = fmaxf(0, dot(n, l));  shade = fminf(1, ambient + intensity lambert)
 *     texel           (U, V) = mix(uv);  x = U Wt - 0.5,  y = (1 - V) Ht - 0.5;  x0 = floorf(x), fx = x - x0, columns x0 and x0 + 1
 *                     clamped to [0, Wt - 1]; rows alike from y.  Per channel, rows first:
 *                       top = t[y0][x0] (1 - fx) + t[y0][x1] fx,  bottom = t[y1][x0] (1 - fx) + t[y1][x1] fx,
 *                       texel = top (1 - fy) + bottom fy
 *     pixel           image = texel shade.  A miss pixel gets args->background.
 *   This is a Lambert model.  It is not pyrender's metallic-roughness shader, and nothing is pinned against pyrender or trimesh.
 * The cull: per frame and face a conservative screen-space box decides whether an 8 x 8 pixel tile looks at the face at all.  It is
 *   an optimisation only: every output equals the brute-force walk over all faces bit for bit, which SNERF_RENDER_NO_CULL in
 *   args->flags runs instead.
 * Every element of every non-NULL output is written; no atomics; nothing of size pixels x faces; two calls give the same bits.
 * There is no backward: the frames are data.
 * workspace: snerf_mesh_render_workspace_bytes(N, V, F) bytes = 4 N (13 F + 3 V), written by two pre-passes of every call.
 * Argument checks, on the host before any device work: N < 0, H, W, Ht or Wt < 1, a focal that is not positive and finite, V < 1,
 *   F < 1, 3 V or 9 F not below 2^31 are SNERF_E_BADARG whatever N is; N = 0 is a no-op returning 0, also with null pointers; then Nv
 *   other than 1 or N, a required null pointer, a mix of null and non-null among canon, warp and depth, N times the 8 x 8 tiles of
 *   a frame or 3 Ht Wt not below 2^31, N above 65535, and a workspace that is missing or too small.  Face indices in [0, V) and a
 *   CSR table of this face table are preconditions (the Python operator checks the one and builds the other). */
#define SNERF_RENDER_NO_CULL 1 /* flags: walk all faces for every tile */
typedef struct snerf_mesh_render_args {
    float ambient, intensity; /* shade = min(1, ambient + intensity max(0, n . l)) */
    float background[3];      /* colour of a miss pixel */
    int32_t flags;            /* 0 or SNERF_RENDER_NO_CULL */
} snerf_mesh_render_args;
SNERF_API int64_t snerf_mesh_render_workspace_bytes(int64_t N, int V, int F);   /* -1 on a bad argument */
SNERF_API int snerf_mesh_render_f32(const double *poses, double focal, int64_t N, int H, int W, const float *vertices, int Nv, int V,
                              const int32_t *faces, int F, const int32_t *vf_offsets, const int32_t *vf_faces, const float *uv,
                              const float *texture, int Ht, int Wt, const snerf_mesh_render_args *args, const float *canon,
                              float *image, float *t, int32_t *face, float *bary, float *depth, float *warp, void *workspace,
                              int64_t workspace_bytes, snerf_stream_t stream);

/* ---- The soft silhouette: a coverage image that is differentiable in the vertices (legacy/neural_mesh_renderer.py's use of a
 * differentiable renderer: fit a pose until the drawn body covers a target).  This is SoftRas's probabilistic union,
 * 1 - prod_f (1 - sigmoid(+-d^2 / sigma)), written as a sum of logs; it is not kaolin's rasteriser and nothing is pinned against it.
 * Inputs: poses, focal, N, H, W, vertices [Nv,V,3] (Nv = 1 or N), faces [F,3] as snerf_mesh_render_f32 takes them; sigma in
 *   pixel^2; cutoff (17: softplus(-17) = 4.1e-8); flags 0 or SNERF_RENDER_NO_CULL.
 * Rule, for frame n, with the camera of snerf_mesh_render_f32 (rotation R in float64, origin o rounded to fp32):
 *   projection      per corner v of a face, in float64: p = v - o; c_i = (p0 R[0][i] + p1 R[1][i]) + p2 R[2][i]  (c = R^T p);
 *                   depth = -c2;  x = W 0.5 + focal c0 / depth;  y = H 0.5 - focal c1 / depth;  x and y rounded once to fp32
 *   live face       all three depths > 0 and all six |x|, |y| below 2^30 (the fp32 pair test cannot place anything farther out);
 *                   a face that is not live contributes nothing, forward or backward
 *   sample point    q = (i, j) for the pixel in row j, column i: where that pixel's ray of snerf_raygen_f64 pierces the image plane
 *   pair            for the segments k = 0: p0 p1, 1: p1 p2, 2: p2 p0 from a to b (products and sums kept apart):
 *                     e = b - a;  w = q - a;  ee = ex ex + ey ey;  t = ee > 0 ? min(max((wx ex + wy ey) / ee, 0), 1) : 0;
 *                     r = w - t e;  d2_k = rx rx + ry ry;  edge_k = ex wy - ey wx
 *                   d2 = the smallest d2_k, the lowest k on a tie;
 *                   inside = the three edge_k are all > 0 or all < 0, and q lies in the bounding box of the three corners (which
 *                   exact arithmetic implies; asked of the fp32 signs it keeps a far pixel outside).  Either winding counts; a
 *                   zero-area face is never inside.
 *   decision, fp32  the pair in fp32 gives inside and d2; a pair with !inside and d2 > cutoff sigma (float64 product, d2 widened)
 *                   contributes exactly 0
 *   value, float64  a contributing pair is evaluated again in float64 on the same fp32 corners: d2, its segment k, t and r (the
 *                   fp32 distances cannot tell the nearest segment where the foot point is near a corner, and t shares the
 *                   gradient between two corners);  z = (inside ? d2 : -d2) / sigma with the decision's inside
 *   per pixel       L = the sum of softplus(z_f) = max(z, 0) + log1p(exp(-|z|)) over the contributing faces, in float64: ascending
 *                   face index within each of the 8 slices wave_slice(F, 8, .) of the face axis, the slices' sums added in order;
 *                   silhouette = -expm1(-L), rounded to fp32 once;  transmittance = exp(-L), float64, for the backward
 *   z is C^1 across a triangle's boundary (d2 -> 0 there): a pixel on a vertex or an edge gets sigmoid(0) = 1/2 from that face and
 *   a zero distance gradient.  The only kink is where the nearest segment changes.
 * Backward: d_vertices[b][v] = sum_n sum_{pixels p, faces f} dS_p T_p sigmoid(z_pf) dz_pf/dv, over all frames n when one body is
 *   shared (Nv = 1), over frame b otherwise.  With g = dS T sigmoid(z) (inside ? 2 : -2) / sigma and the nearest segment a -> b of
 *   the pair, d/da = -g (1 - t) r and d/db = -g t r (the clamp and r . e = 0 make the t-terms vanish); the roundings to fp32 pass the
 *   gradient through; through the projection d/dc = (gx focal / depth, -gy focal / depth, (gx c0 - gy c1) focal / depth^2) and
 *   d/dv = R d/dc.  All of it in float64: per (frame, face) the pixels of the face's box in row-major order, 64 interleaved partial
 *   sums added in one fixed order; per vertex its incident corners in CSR order, frames ascending; rounded to fp32 once.
 * The cull: per frame and face the bounding box of the projected corners, widened by sqrt(cutoff sigma) plus a margin for the fp32
 *   roundings and rounded outward.  A pixel outside it contributes exactly 0 under the rule, so skipping the face changes nothing:
 *   every output equals the walk over all faces (SNERF_RENDER_NO_CULL) bit for bit.  The backward always walks boxes.
 * Every element of every output is written; no atomics; nothing of size pixels x faces; two calls give the same bits; the entries
 *   neither allocate nor synchronise.
 * workspace: snerf_soft_silhouette_workspace_bytes(N, V, F) = 112 N F bytes, 8-byte aligned, written by a pre-pass of every call
 *   (the backward does not need the forward's).
 * vf_offsets [V+1], vf_faces [3F], vf_corners [3F] int32: the CSR table of snerf_mesh_render_f32 plus, for each entry, which of
 *   the face's three corners it is (a face that names a vertex twice owns two distinct corners).
 * Argument checks, on the host before any device work: N < 0, H or W < 1, a focal or sigma that is not positive and finite, a
 *   cutoff that is negative or not finite, unknown flags, V < 1, F < 1, 3 V or 9 F not below 2^31 are SNERF_E_BADARG whatever N is;
 *   N = 0 is a no-op returning 0, also with null pointers; then Nv other than 1 or N, a null pointer, N times the 8 x 8 tiles of a
 *   frame not below 2^31, N above 65535, a workspace that is missing, misaligned or too small.  Face indices in [0, V) and a CSR
 *   table of this face table are preconditions. */
SNERF_API int64_t snerf_soft_silhouette_workspace_bytes(int64_t N, int V, int F);   /* -1 on a bad argument */
SNERF_API int snerf_soft_silhouette_fwd_f32(const double *poses, double focal, int64_t N, int H, int W, const float *vertices, int Nv,
                              int V, const int32_t *faces, int F, double sigma, double cutoff, int flags, float *silhouette,
                              double *transmittance, void *workspace, int64_t workspace_bytes, snerf_stream_t stream);
SNERF_API int snerf_soft_silhouette_bwd_f32(const double *poses, double focal, int64_t N, int H, int W, const float *vertices, int Nv,
                              int V, const int32_t *faces, int F, double sigma, double cutoff, int flags, const float *d_silhouette,
                              const double *transmittance, const int32_t *vf_offsets, const int32_t *vf_faces,
                              const int32_t *vf_corners, float *d_vertices, void *workspace, int64_t workspace_bytes,
                              snerf_stream_t stream);

/* ---- Image scores: structural similarity with its backward, and the squared error of MSE / PSNR (util/scores.py:11-48, 88-173) ----
 * x, y: N images of C channels, H x W pixels, fp32, BOTH read through the four element strides (sn, sc, sh, sw): element
 *   (n, c, h, w) lies at n sn + c sc + h sh + w sw, so [N,C,H,W] and channels-last [N,H,W,C] storage run without a copy.
 * win [k]: the 1-D window; the 2-D window is G = win (x) win, applied as a VALID correlation: P = (H-k+1)(W-k+1) windows q.
 * Rule, per image n and channel c:
 *   mu1 = G*x  mu2 = G*y  e11 = G*(x x)  e22 = G*(y y)  e12 = G*(x y)      s11 = e11 - mu1^2  s22 = e22 - mu2^2  s12 = e12 - mu1 mu2
 *   A = mu1^2 + mu2^2 + c1   D = s11 + s22 + c2   L = (2 mu1 mu2 + c1) / A   CS = (2 s12 + c2) / D   S = L CS
 *   ssim[n C + c] = mean_q S     cs[n C + c] = mean_q CS     sqerr[n C + c] = the sum of (x - y)^2 over ALL H W pixels
 *   (c1 = (k1 data_range)^2 and c2 = (k2 data_range)^2 are the caller's; the Gaussian window is the caller's too.)
 * Written: every element of ssim and of each of cs, sqerr that is not NULL.  x == y gives ssim = cs = 1 and sqerr = 0 exactly.
 * workspace: snerf_ssim_workspace_bytes(N, C, H, W, k) bytes, 8-byte aligned: three float64 partial sums per 32 x 32 tile of
 *   windows, added by a second launch.  Nothing of map size is kept.
 * Refused with SNERF_E_BADARG on the host, before anything touches a device: k < 1 or k > 33; H < k or W < k (the message names k,
 *   H and W); c1 or c2 negative or not finite; N or C negative; C, H, W or N C times the tile count at 2^31 or above; with N C > 0
 *   a null x, y, win or ssim (dx, g_ssim for the backward), a workspace that is null or too small.  A bad scalar is an error
 *   whatever N is; with N C == 0 and good scalars both entries return SNERF_OK whatever the pointers are.
 * No atomics, every sum in a fixed order that does not depend on the strides: two calls on the same inputs give the same bits, and
 *   so do two layouts of the same images. */
SNERF_API int64_t snerf_ssim_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int k);   /* -1 on a bad argument */
SNERF_API int snerf_ssim_fwd_f32(const float *x, const float *y, int64_t N, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc,
                              int64_t sh, int64_t sw, const float *win, int k, float c1, float c2, float *ssim, float *cs,
                              float *sqerr, void *workspace, int64_t workspace_bytes, snerf_stream_t stream);
/* Its backward.  g_ssim [N C], g_cs [N C] (NULL: zeros) are the gradients arriving at ssim and cs -> dx, the gradient with respect to
 * x, written with the input strides, every pixel of every image.  Per window w = (g_ssim L + g_cs) / P, u = g_ssim CS / P,
 *   a = u (2 mu2 - 2 mu1 L) / A + w (2 mu1 CS - 2 mu2) / D     b = -w CS / D     c = 2 w / D     (zero outside the valid windows)
 *   dx[p] = (G^T a)[p] + 2 x[p] (G^T b)[p] + y[p] (G^T c)[p]     G^T: the full correlation with the flipped window
 * The window statistics are recomputed from x and y.  The rule is symmetric in (x, y): the gradient with respect to y is this entry
 * called with x and y swapped.  The workspace is checked as the forward's (one buffer serves both); the backward writes none of it.
 * The same refusals and the same determinism as the forward. */
SNERF_API int snerf_ssim_bwd_f32(const float *x, const float *y, int64_t N, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc,
                              int64_t sh, int64_t sw, const float *win, int k, float c1, float c2, const float *g_ssim,
                              const float *g_cs, float *dx, void *workspace, int64_t workspace_bytes, snerf_stream_t stream);

/* ---- SmplEstimator, inference: the fused convolution block and the whole network (models/smpl_estimator.py:6-47, eval mode) ----
 * One block, one launch, contiguous NCHW fp32:
 *   y = [maxpool2x2](relu(scale[co] * conv3x3_pad1(x, w)[co] + shift[co]))
 *   x [N,Ci,H,W], w [Co,Ci,3,3], scale, shift [Co] -> y [N,Co,H,W], or [N,Co,H/2,W/2] with pool != 0.  relu and pool are separate
 *   flags.  With pooling an odd H or W floors as nn.MaxPool2d(2, 2) does: the last row or column takes part in no window.
 * Arithmetic: exact fp32 on the matrix cores.  Every output element is one fused-multiply-add chain over k = ci 9 + ky 3 + kx in
 *   ascending order (zero products stand in for the padding); then one multiplication by scale, one addition of shift.  The chain
 *   depends on Ci alone, so a pixel's value does not depend on N, on the grid or on where it lies in a tile; no atomics; two calls
 *   give the same bits.  Every element of y is written.
 * 1 <= Ci, Co <= 256; H, W >= 1 (with pooling >= 2); N >= 0 (0: SNERF_OK whatever the pointers are); N Ci H W and N Co H W below
 *   2^31; with N > 0 no null pointer - else SNERF_E_BADARG on the host, before anything touches a device, with a message naming the
 *   value; a bad scalar is an error whatever N is. */
SNERF_API int snerf_conv3x3_block_f32(const float *x, int64_t N, int Ci, int64_t H, int64_t W, const float *w, const float *scale,
                              const float *shift, int Co, int relu, int pool, float *y, snerf_stream_t stream);
/* The network.  Device pointers to the tensors of the reference's state_dict, as they are stored: */
typedef struct snerf_conv_bn {
    const float *weight, *bias;                                         /* convN.weight [Co,Ci,3,3], convN.bias [Co] */
    const float *bn_weight, *bn_bias, *running_mean, *running_var;      /* bnN.* [Co] */
    double eps;                                                         /* bnN.eps */
} snerf_conv_bn;
typedef struct snerf_smpl_estimator {
    snerf_conv_bn block[5];                                             /* channels 3 -> 16 -> 32 -> 64 -> 64 -> 128 */
    const float *fc1_weight, *fc1_bias, *fc2_weight, *fc2_bias;         /* [500,8192], [500], [human_size,500], [human_size] */
    int32_t human_size;
} snerf_smpl_estimator;
/* images [N,3,128,128] -> out [N,human_size], eval mode (running statistics, no dropout), in one call of eight launches on `stream`:
 *   the fold of each block's BatchNorm and bias, scale = gamma / sqrt(var + eps), shift = beta + (b - mean) scale, computed on the
 *   device in float64 from the pointers above and rounded once (so a parameter changed in place is seen by the next call);
 *   the five blocks (pooling after blocks 2 .. 5) between two activation buffers; fc1 with ReLU and fc2 on snerf_linear_fwd_f32's
 *   kernel.  Block 5 writes contiguous [N,128,8,8]: the rows of the reference's view(-1, 8 * 8 * 128).
 * workspace: snerf_smpl_estimator_workspace_bytes(N, human_size) bytes (-1 on a bad argument), 16-byte aligned: the fold and the
 *   two buffers.  Nothing is allocated and nothing synchronises: the call can be captured into a graph.  Same inputs, same bits; an
 *   image's row does not depend on the rest of the batch.
 * SNERF_E_BADARG on the host: a null net; human_size < 1; N negative or above 8191 (2^31 activations); an eps that is negative or
 *   not finite; with N > 0 a null pointer in the net, null images or out, a workspace that is null or too small.  SNERF_E_ALIGN: a
 *   workspace that is not 16-byte aligned.  N = 0: SNERF_OK. */
SNERF_API int64_t snerf_smpl_estimator_workspace_bytes(int64_t N, int human_size);
SNERF_API int snerf_smpl_estimator_fwd_f32(const snerf_smpl_estimator *net, const float *images, int64_t N, float *out, void *workspace,
                              int64_t workspace_bytes, snerf_stream_t stream);

/* ---- LPIPS: the VGG16 feature stack and the fused tap distance (util/scores.py:286-456; csrc/conv_block.hip, csrc/lpips.hip) ----
 * The convolution block with a tap: snerf_conv3x3_block_f32's rule, chain and bits, written to the un-pooled map y_full [N,Co,H,W]
 *   when it is not NULL and to the pooled map y_pool [N,Co,H/2,W/2] when it is not NULL, both from the same accumulators in one
 *   launch.  One of the two at least.  1 <= Ci, Co <= 512; H, W >= 1, and >= 2 with y_pool; the other refusals of
 *   snerf_conv3x3_block_f32, on the host, before anything touches a device; a bad scalar is an error whatever N is, N = 0 is
 *   SNERF_OK whatever the pointers are.  For Ci, Co <= 256 either output has the bits snerf_conv3x3_block_f32 gives it.
 *   Above 256 input channels the chain over k is segmented: it starts again at zero every 128 channels (1152 elements) and the
 *   segment sums are added in ascending order, the first to zero - one fp32 chain of 4608 terms measured 8.1 times the fp32 CPU
 *   convolution's error against float64, a chain of 1152 with three additions 4.1 times.  Still one fixed order that depends on Ci
 *   alone. */
SNERF_API int snerf_conv3x3_block_tap_f32(const float *x, int64_t N, int Ci, int64_t H, int64_t W, const float *w, const float *scale,
                              const float *shift, int Co, int relu, float *y_full, float *y_pool, snerf_stream_t stream);
/* The distance of two feature maps fx, fy [N,C,h,w] (contiguous fp32) under channel weights wl [C] -> out [N]:
 *   out[n] = (1 / (h w)) sum_p sum_c wl[c] (x^[c,p] - y^[c,p])^2
 *   normalize != 0: x^[c,p] = fx[c,p] / (sqrt(sum_c fx[c,p]^2) + 1e-10) (ContentLoss.normalize, scores.py:403-411); else x^ = fx.
 * Rule, per pixel p, operation by operation:
 *   s   = sum over c = 0, 1, .. of fx[c,p]^2, accumulated in float64 (the products are exact there), rounded to fp32 once
 *   nx  = sqrt(s) + 1e-10f      fp32: an IEEE square root, then the addition (ny from fy alike)
 *   a   = fx[c,p] / nx          fp32, IEEE division (b = fy[c,p] / ny; without normalize a = fx, b = fy)
 *   d   = a - b,  t = d d       fp32
 *   acc = sum over c = 0, 1, .. of (double)wl[c] (double)t, one float64 fused multiply-add per channel
 *   A tile is 64 consecutive pixels of the flattened h w map; its pixels' acc are added in float64 by the wavefront scan (lane order)
 *   into workspace[n][tile]; a second launch adds an image's tiles - lane l the tiles l, l + 64, .. in that order, then the scan -
 *   divides by h w in float64 and rounds to fp32 once.
 * The difference form: fx == fy gives 0 exactly; a pixel whose features are all zero contributes 0 (nx = 1e-10, a = 0).  No atomics;
 *   two calls give the same bits; an image's value does not depend on the rest of the batch.  Nothing of map size is stored.
 * workspace: snerf_feature_distance_workspace_bytes(N, h, w) bytes (-1 on a bad argument), 8-byte aligned.
 * SNERF_E_BADARG on the host: N negative or above 65535; C, h or w below 1; N C h w at 2^31 or above; with N > 0 a null fx, fy, wl or
 *   out, a workspace that is null or too small.  SNERF_E_ALIGN: a misaligned workspace.  N = 0: SNERF_OK whatever the pointers are. */
SNERF_API int64_t snerf_feature_distance_workspace_bytes(int64_t N, int64_t h, int64_t w);
SNERF_API int snerf_feature_distance_f32(const float *fx, const float *fy, int64_t N, int64_t C, int64_t h, int64_t w, const float *wl,
                              int normalize, float *out, void *workspace, int64_t workspace_bytes, snerf_stream_t stream);
/* The network: device pointers to the tensors of torchvision's vgg16().features and of the reference's lpips_weights.pt. */
typedef struct snerf_conv_wb {
    const float *weight, *bias;                                         /* [Co,Ci,3,3], [Co] */
} snerf_conv_wb;
typedef struct snerf_vgg_lpips {
    snerf_conv_wb conv[13];                                             /* VGG16 order: 2, 2, 3, 3, 3 convolutions per stage */
    int32_t channels[5];                                                /* per stage, each 1 .. 512; VGG16: 64, 128, 256, 512, 512 */
    const float *lin[5];                                                /* lin[l] [channels[l]]: the learned channel weights */
    float mean[3], std[3];                                              /* the input standardisation (ImageNet's for LPIPS) */
} snerf_vgg_lpips;
/* x, y: N frames each of 3 channels, H x W pixels, fp32, both read through the element strides (sn, sc, sh, sw) as snerf_ssim_fwd_f32
 *   reads them -> layers [N,5]: the distance of each tap; total [N] (may be NULL): their fp32 sum in ascending order of the stage.
 * What runs: (v - mean[c]) / std[c] in fp32, a subtraction and then a division as scores.py:394 (not folded into the first
 *   convolution: its zero padding is applied after the standardisation); x and y as ONE batch through the 13 convolutions
 *   (snerf_conv3x3_block_tap_f32's kernel with scale = 1, shift = bias, ReLU); the taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3,
 *   each followed by its distance with normalize on (the kernel of snerf_feature_distance_f32), the first four also pooled in the
 *   same launch.  The entry adds no arithmetic of its own: layers has the bits of the two entries above called one by one.
 * pool5 is not run, its output is unused: H, W >= 16 are accepted, where the reference (which runs it) raises below 32.
 * Inputs are not checked for >= 0: the reference's assert is a device synchronisation.
 * workspace: at least snerf_lpips_workspace_bytes(1, H, W, channels) bytes, 16-byte aligned.  The call walks the batch in chunks of
 *   as many pairs as the workspace holds (snerf_lpips_workspace_bytes(n_pairs, ..) bytes hold n_pairs); the bits do not depend on
 *   the workspace's size.  Nothing is allocated and nothing synchronises: the call - a linear chain of launches - can be captured
 *   into a graph.  Same inputs, same bits; a frame pair's values do not depend on the rest of the batch.
 * SNERF_E_BADARG on the host: a null net; a channel count outside 1 .. 512; a std that is zero or not finite, a mean that is not
 *   finite; H or W below 16; N negative; 2 x the widest layer x H x W at 2^31 or above; with N > 0 a null pointer in the net, null x, y or layers,
 *   a workspace that is null or smaller than one pair's.  SNERF_E_ALIGN: a workspace that is not 16-byte aligned.  N = 0: SNERF_OK. */
SNERF_API int64_t snerf_lpips_workspace_bytes(int64_t n_pairs, int64_t H, int64_t W, const int32_t *channels);   /* -1 on a bad argument */
SNERF_API int snerf_lpips_fwd_f32(const snerf_vgg_lpips *net, const float *x, const float *y, int64_t N, int64_t H, int64_t W, int64_t sn,
                              int64_t sc, int64_t sh, int64_t sw, float *layers, float *total, void *workspace,
                              int64_t workspace_bytes, snerf_stream_t stream);
/* ---- LPIPS as a training loss: the backward to both frames (ContentLoss is a _Loss: differentiable, its weights frozen, scores.py:340)
 * Common to the three entries: contiguous NCHW fp32 unless strides are named; no atomics and no read-modify-write of global memory;
 *   one fixed summation order that depends on the shapes alone; every element of every output that is not NULL is written; nothing
 *   is allocated and nothing synchronises; bad arguments are SNERF_E_BADARG / SNERF_E_ALIGN on the host, before anything touches a
 *   device, with a message naming the value; a bad scalar is an error whatever N is; N = 0 is SNERF_OK whatever the pointers are.
 *
 * The distance gradient: dfx, dfy [N,C,h,w] (either may be NULL, not both) = the gradient of sum_n g[n] out[n] of
 *   snerf_feature_distance_f32 to fx and to fy; g [N].  Rule, per pixel p, operation by operation:
 *   s, r = sqrt(s), nx = r + 1e-10f, a = fx / nx, b = fy / ny, d = a - b     fp32, the forward's own values (ry, ny from fy alike)
 *   gs = (double)g[n] / (h w)              q[c] = ((2 wl[c]) d[c]) gs        float64 from here on
 *   Dx = sum over c = 0, 1, .. of q[c] a[c], Dy = .. q[c] b[c]               one float64 fused multiply-add per channel
 *   dfx[k] = (q[k] - fx[k] (Dx / r)) / nx         dfy[k] = -(q[k] - fy[k] (Dy / ry)) / ny         each rounded to fp32 once
 *   Without normalize: dfx = q, dfy = -q.
 *   The all-zero pixel: where r = 0 the reference's autograd gives NaN (0 / 0 in the square root's backward).  Here the norm term is
 *   taken as 0 there: dfx[k] = q[k] / nx, finite.  In the metric it makes no difference: such a pixel sits at the ReLU's zero in
 *   every channel, and the ReLU's backward masks it to 0, which is why the reference's end-to-end gradient is finite too.
 *   fx == fy gives +0 everywhere.  Either output alone has the bits it has beside the other; a pixel's gradient depends on its own
 *   features and g[n] alone.  Lane = pixel, as in the forward; three passes over the channels (HBM once, the L2 twice); nothing of
 *   map size is stored besides the outputs; no workspace.
 *   SNERF_E_BADARG: the scalar refusals of snerf_feature_distance_f32; with N > 0 both outputs NULL, a null fx, fy, wl or g. */
SNERF_API int snerf_feature_distance_bwd_f32(const float *fx, const float *fy, int64_t N, int64_t C, int64_t h, int64_t w, const float *wl,
                              int normalize, const float *g, float *dfx, float *dfy, snerf_stream_t stream);
/* The ReLU and the 2 x 2 max-pool that may follow it, without BatchNorm, on the post-ReLU map y [N,C,H,W] -> dz [N,C,H,W]:
 *   dz = (y > 0) ? dy_full + route(dy_pool) : 0            dy_full [N,C,H,W], dy_pool [N,C,H/2,W/2]; either may be NULL, not both
 *   route sends a window's gradient to its FIRST maximum in the order (0,0), (0,1), (1,0), (1,1), recomputed from y (the rule of
 *   snerf_bn_relu_pool_bwd_f32, torch's max_pool2d); elsewhere, and at a pixel in no window (an odd extent), it is 0; a NULL
 *   gradient is 0.  One fp32 addition per pixel.  dz may be dy_full: a thread reads the four pixels of its 2 x 2 cell before it
 *   writes them.
 *   SNERF_E_BADARG: N negative; C, H or W below 1, with dy_pool H or W below 2; N C H W at 2^31 or above; with N > 0 both gradients
 *   NULL, a null y or dz. */
SNERF_API int snerf_relu_pool_bwd_f32(const float *y, const float *dy_full, const float *dy_pool, int64_t N, int64_t C, int64_t H, int64_t W,
                              float *dz, snerf_stream_t stream);
/* The whole backward: dx, dy (either may be NULL, not both) = the gradient of sum_n sum_l g_layers[n,l] layers[n,l] of
 *   snerf_lpips_fwd_f32 to the frames x and y, written through the four element strides the frames are read through (which must
 *   put no two elements at one address); g_layers [N,5].  layers [N,5] (may be NULL): the forward's, with its bits.
 * What runs, per chunk of as many pairs as the workspace holds:
 *   the forward with snerf_lpips_fwd_f32's own kernels, keeping the thirteen post-ReLU maps of both frames;
 *   then from the fifth stage down to the first: at a tap the distance gradient (snerf_feature_distance_bwd_f32's kernel), then
 *   snerf_relu_pool_bwd_f32's with the gradient that arrives from the next stage's pooled input as dy_pool (none at the fifth); at
 *   the other eight convolutions snerf_relu_pool_bwd_f32's with dy_full alone; between them the input gradient of a convolution,
 *   dx = conv3x3_pad1(dz, w') with w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx] written into the workspace, on
 *   snerf_conv3x3_block_tap_f32's kernel with scale = 1, shift = 0, no ReLU - up to 512 channels, above 256 with its segmented
 *   chain as it stands; last g / std[c], one fp32 division.
 *   With one of dx, dy NULL the backward runs on that half of the batch only.
 * The entry adds no arithmetic of its own: its outputs have the bits of the entries above called one by one.  They do not depend on
 *   the workspace's size or on the rest of the batch.  A linear chain of launches: it can be captured into a graph.
 * workspace: at least snerf_lpips_bwd_workspace_bytes(1, H, W, channels) bytes, 16-byte aligned; (n_pairs, ..) bytes hold n_pairs a
 *   chunk.  Once a call: w' of the widest convolution and 512 zeros.  Per pair: the thirteen maps of both frames (540 H W floats at
 *   VGG16's widths), two gradient buffers of the widest map (2 x 128 H W), one float64 per 64-pixel tile.
 * Refusals: snerf_lpips_fwd_f32's, and with N > 0 both outputs NULL or a null g_layers. */
SNERF_API int64_t snerf_lpips_bwd_workspace_bytes(int64_t n_pairs, int64_t H, int64_t W, const int32_t *channels);   /* -1 on a bad argument */
SNERF_API int snerf_lpips_bwd_f32(const snerf_vgg_lpips *net, const float *x, const float *y, int64_t N, int64_t H, int64_t W, int64_t sn,
                              int64_t sc, int64_t sh, int64_t sw, const float *g_layers, float *dx, float *dy, float *layers,
                              void *workspace, int64_t workspace_bytes, snerf_stream_t stream);

/* ---- SmplEstimator, training: the block with batch statistics and its backward (csrc/conv_train.hip) --------------------------
 *   z = conv3x3_pad1(x, w) + b              snerf_conv3x3_block_f32 with scale = 1, shift = b, relu = pool = 0 (x 1 is exact)
 *   mean, invstd                            snerf_bn_stats_f32: per channel over M = N H W values, biased variance
 *   y = [maxpool2x2](relu(pre))             snerf_bn_relu_pool_fwd_f32: xhat = (z - mean) invstd, pre = xhat gamma + beta, each
 *                                           operation rounded to fp32; odd extents floor as in the block above
 *   dz, dgamma, dbeta from dy               snerf_bn_relu_pool_bwd_f32: g = dy routed through the pool (the FIRST maximum of a
 *                                           window in the order (0,0), (0,1), (1,0), (1,1); pixels in no window get 0) and the
 *                                           ReLU (0 where pre <= 0), both recomputed from z; dbeta = s1 = sum g, dgamma = s2 =
 *                                           sum g xhat, dz = gamma invstd (g - s1 / M - xhat s2 / M).  Each of dz, dgamma, dbeta
 *                                           may be null and is then not computed.
 *   dx = conv3x3_pad1(dz, w')               snerf_conv3x3_bwd_input_f32: w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx] is written
 *                                           into scratch, then the forward kernel runs: one chain over 9 Co per element of dx
 *   dw, dbias                               snerf_conv3x3_bwd_weight_f32: dw[co][ci][ky][kx] = sum dz[n][co][y][x] xpad[n][ci][y+ky-1]
 *                                           [x+kx-1] on the matrix cores (exact fp32), dbias[co] = sum dz; either may be null
 * Tensors are contiguous NCHW fp32; z, dz [N,C,H,W]; y, dy [N,C,H,W] or [N,C,H/2,W/2]; mean, invstd, gamma, beta, dgamma, dbeta,
 * running_mean, running_var [C].  running_mean / running_var (each nullable) are moved in place as F.batch_norm(training=True)
 * does: running = (1 - momentum) running + momentum stat, with the unbiased variance var M / (M - 1).
 * Sums.  Every per-channel sum (the statistics, s1, s2, dbias) is float64 in a fixed order: slices of consecutive n-major terms,
 *   one partial per (channel, slice) in scratch, one finisher that adds them in slice order; results are rounded once to fp32.
 *   A dw element is, per slice of consecutive (image, 16 x 16 pixel tile) jobs, four fp32 chains over the rows 4 v .. 4 v + 3
 *   (v = 0 .. 3) of the tiles, added in that order, then the slices in float64 in slice order, rounded once.  The slice counts
 *   (snerf_conv3x3_bwd_weight_slices; min(128, ceil(terms / 8192)) for the per-channel sums) depend on the shapes alone, not on
 *   the device: same inputs, same bits.  No atomics, nothing allocated, nothing synchronises.
 * scratch: the *_scratch_floats query of the entry, in floats, 8-byte aligned (SNERF_E_ALIGN otherwise); for the weight gradient
 *   4 Co S floats of dbias partials (S as for snerf_bn_stats_scratch_floats(N, 1, H, W) / 4) and then slices x Co Ci 9 floats.
 * Limits: 1 <= C, Ci, Co <= 256, N >= 0 (0: SNERF_OK whatever the pointers are), element counts below 2^31, H, W >= 1 (>= 2 with
 *   pooling); the statistics and the backward need M = N H W >= 2; eps >= 0 and finite, momentum finite; with N > 0 no null
 *   pointer but the optional ones.  SNERF_E_BADARG on the host, before anything touches a device; the queries return -1. */
SNERF_API int64_t snerf_bn_stats_scratch_floats(int64_t N, int C, int64_t H, int64_t W);
SNERF_API int snerf_bn_stats_f32(const float *z, int64_t N, int C, int64_t H, int64_t W, double eps, double momentum, float *running_mean,
                              float *running_var, float *mean, float *invstd, float *scratch, snerf_stream_t stream);
SNERF_API int snerf_bn_relu_pool_fwd_f32(const float *z, int64_t N, int C, int64_t H, int64_t W, const float *mean, const float *invstd,
                              const float *gamma, const float *beta, int relu, int pool, float *y, snerf_stream_t stream);
SNERF_API int64_t snerf_bn_relu_pool_bwd_scratch_floats(int64_t N, int C, int64_t H, int64_t W, int pool);
SNERF_API int snerf_bn_relu_pool_bwd_f32(const float *z, const float *dy, int64_t N, int C, int64_t H, int64_t W, const float *mean,
                              const float *invstd, const float *gamma, const float *beta, int relu, int pool, float *dz,
                              float *dgamma, float *dbeta, float *scratch, snerf_stream_t stream);
SNERF_API int64_t snerf_conv3x3_bwd_input_scratch_floats(int Ci, int Co);
SNERF_API int snerf_conv3x3_bwd_input_f32(const float *dz, int64_t N, int Co, int64_t H, int64_t W, const float *w, int Ci, float *dx,
                              float *scratch, snerf_stream_t stream);
SNERF_API int64_t snerf_conv3x3_bwd_weight_slices(int64_t N, int Ci, int64_t H, int64_t W, int Co);
SNERF_API int64_t snerf_conv3x3_bwd_weight_scratch_floats(int64_t N, int Ci, int64_t H, int64_t W, int Co);
SNERF_API int snerf_conv3x3_bwd_weight_f32(const float *dz, const float *x, int64_t N, int Ci, int Co, int64_t H, int64_t W, float *dw,
                              float *dbias, float *scratch, snerf_stream_t stream);

/* ---- 8(f)-1: on-device ray generation + stratified coarse sampling --------------------------------------
 * Replaces get_rays (utils.py:50-54) + CoarseSampling (datasets/transforms.py:80-89) + ToTensor (:13-21) for a
 * batch of rays.  poses: fp64 [n_frames, 4, 4] camera-to-world; ray_index int64 [B] = frame*H*W + row*W + col;
 * jitter fp64 [B] = the per-ray np.random.rand() scalar; lower/span fp64 [Nc] = the bin tables of
 * CoarseSampling (lower, upper - lower).  fp64 arithmetic in the reference's order, one rounding to fp32:
 * bit-identical to the numpy path.  Outputs: samples [B,Nc,3], o [B,3], d [B,3], z [B,Nc] fp32. */
SNERF_API int snerf_raygen_f64(const double *poses, int64_t n_frames, int H, int W, double focal, const double *lower,
                     const double *span, int Nc, const int64_t *ray_index, const double *jitter, int64_t B,
                     float *samples, float *o, float *d, float *z, snerf_stream_t stream);

/* ---- a3: the whole NerfPipeline.forward for inference in one call (models/nerf_pipeline.py:14-67) -------------
 * Five launches on `stream`: fused encode+MLP (coarse) -> composite -> inverse-CDF sampler + merge + points ->
 * fused encode+MLP (fine) -> composite.  precision: 0 = fp32 kernel (packed_* from snerf_mlp_pack_f32), 2 / 3 / 16 =
 * split-bf16 / split-fp16 with that nsplit (packed_* from snerf_mlp_pack_bf16), SNERF_FP32_INFER (32) = fp32 kernel, packed_*
 * from snerf_mlp_pack_infer_f32.  Inputs as the Solver hands them over
 * (solver/nerf_solver.py:77-81): ray_samples [B,Nc,3], rays_o [B,3], rays_d [B,3], z_vals [B,Nc]; u [Nf] =
 * linspace(0,1,Nf) (utils.py:204-205); noise_coarse [B,Nc] / noise_fine [B,Nc+Nf] nullable (sigma noise,
 * utils.py:171-173).  Nf == 0 is run_fine = 0: the fine outputs are copies of the coarse ones (:43-44).
 * workspace: snerf_render_rays_workspace_bytes(B, Nc, Nf) bytes, 16-byte aligned.  Outputs: rgb [B,3],
 * rgb_fine [B,3], samples_fine [B,Nc+Nf,3], densities_fine [B,Nc+Nf] (the `alpha` of utils.py:169). */
SNERF_API int64_t snerf_render_rays_workspace_bytes(int64_t B, int Nc, int Nf);
SNERF_API int snerf_render_rays_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse,
                          const snerf_mlp_desc *desc_fine, const void *packed_fine, int precision,
                          const float *ray_samples, const float *rays_o, const float *rays_d, const float *z_vals,
                          const float *u, const float *noise_coarse, const float *noise_fine, int64_t B, int Nc,
                          int Nf, int white_background, void *workspace, float *rgb, float *rgb_fine,
                          float *samples_fine, float *densities_fine, snerf_stream_t stream);

/* ---- 8(f)-4: the same for nets with per-ray additional inputs (models/append_smpl_params_pipeline.py:14-91,
 * append_to_nerf_pipeline.py:14-90 - the paper's headline model) ------------------------------------------------------
 * snerf_render_rays_f32 with additional [B, add_dim] = the pose row of each ray (raw or encoded, :29-37), read by both nets as
 * their `add` input (descriptors with add_dim > 0, add_first as the pipeline has it).  In fp32 the rows are folded into one
 * vector per ray and layer inside the call (snerf_mlp_fwd_ws_f32) - the fold table lives in the workspace:
 * snerf_render_rays_add_workspace_bytes(...) bytes, 16-byte aligned. */
SNERF_API int64_t snerf_render_rays_add_workspace_bytes(const snerf_mlp_desc *desc_coarse, const snerf_mlp_desc *desc_fine, int64_t B, int Nc,
                                              int Nf);
SNERF_API int snerf_render_rays_add_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const snerf_mlp_desc *desc_fine,
                              const void *packed_fine, int precision, const float *ray_samples, const float *rays_o,
                              const float *rays_d, const float *z_vals, const float *additional, const float *u,
                              const float *noise_coarse, const float *noise_fine, int64_t B, int Nc, int Nf, int white_background,
                              void *workspace, float *rgb, float *rgb_fine, float *samples_fine, float *densities_fine,
                              snerf_stream_t stream);

/* ---- a7: the whole SmplNerfPipeline.forward for inference in one call (models/smpl_nerf_pipeline.py:16-100) ------
 * snerf_render_rays_f32 with the warp stage in front of both nets: warp(samples) -> x' = x + warp, per-sample directions
 * x' - o -> net -> composite (coarse: distances scaled by |x' - o| per sample, :63; fine: by the ray direction, :95-98);
 * the hierarchical samples are drawn on the un-warped ray (:68).  pose_enc [B, pose_dim] = the encoded two joint angles
 * (:28-30).  precision as in snerf_render_rays_f32 (the warp net runs fp32 for 0 and three-part split-bf16 otherwise;
 * packed_warp from snerf_warp_pack_f32 / snerf_warp_pack_bf16 accordingly).  Nf >= 1.  workspace:
 * snerf_render_rays_smpl_workspace_bytes bytes.  Outputs: rgb [B,3], rgb_fine [B,3], warp_fine / samples_fine /
 * warped_fine [B,Nc+Nf,3], densities_fine [B,Nc+Nf]. */
SNERF_API int64_t snerf_render_rays_smpl_workspace_bytes(int64_t B, int Nc, int Nf);
SNERF_API int snerf_render_rays_smpl_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse,
                               const snerf_mlp_desc *desc_fine, const void *packed_fine,
                               const snerf_warp_desc *desc_warp, const void *packed_warp, int precision,
                               const float *ray_samples, const float *rays_o, const float *rays_d, const float *z_vals,
                               const float *pose_enc, const float *u, const float *noise_coarse,
                               const float *noise_fine, int64_t B, int Nc, int Nf, int white_background,
                               void *workspace, float *rgb, float *rgb_fine, float *warp_fine, float *samples_fine,
                               float *warped_fine, float *densities_fine, snerf_stream_t stream);

/* ---- a9 + 8(f)-2: the per-batch body of NerfSolver.train as one call (solver/nerf_solver.py:76-87) ---------------------
 *     rgb, rgb_fine, .. = pipeline(batch); loss = MSE(rgb, gt) + MSE(rgb_fine, gt); loss.backward(); Adam.step()
 * (models/nerf_pipeline.py:14-67, solver/nerf_solver.py:48-52, :31-33).  Everything is enqueued on `stream`; nothing is
 * allocated, nothing synchronises, and no argument changes from step to step except the batch pointers (the optimiser's
 * step counter and bias corrections live on the device): the call can be captured into a HIP graph and replayed.
 *
 * Weight streams.  A training step consumes two streams per net - `packed` (snerf_mlp_pack_f32 / snerf_mlp_pack_bf16) and
 * `packed_t` (snerf_mlp_pack_t_f32 / snerf_mlp_pack_t_bf16 with input_grad = 0) - which the caller packs ONCE; afterwards the
 * optimiser step keeps them current: fp32 streams are refreshed in place, element by element, through the slot tables of
 * snerf_mlp_stream_slots (no re-pack launches); split-precision streams (pre-split parts) are re-packed inside the call. */

/* slot_fwd[i] / slot_t[i] (int32, snerf_mlp_param_floats entries each, nullable): index of the float of the fp32 forward /
 * transposed stream that holds parameter i of params_flat, or -1 (biases do not appear in the transposed stream).
 * input_grad selects WHICH transposed stream (snerf_mlp_pack_t_f32's input_grad: 0 for snerf_nerf_train_*, 1 for
 * snerf_smpl_nerf_train_*).  Every parameter occupies at most one float of each stream. */
SNERF_API int snerf_mlp_stream_slots(const snerf_mlp_desc *desc, int32_t *slot_fwd, int32_t *slot_t, int input_grad, snerf_stream_t stream);

/* torch.optim.Adam(params, lr, betas, eps, weight_decay) (amsgrad = False) over ONE flat fp32 parameter buffer - the
 * statements of torch's single-tensor update in their order (solver/nerf_solver.py:11-14, 31-33, 87). */
typedef struct snerf_adam_state {
    float *params;       /* [n_params] */
    const float *grads;  /* [n_params] */
    float *exp_avg;      /* [n_params], zero before the first step */
    float *exp_avg_sq;   /* [n_params], zero before the first step */
    int64_t n_params;
    float *scratch;      /* device, 2 floats per range of a call (64 floats cover the maximum of 32 ranges) */
    double lr, beta1, beta2, eps, weight_decay;
} snerf_adam_state;
/* A run of adjacent parameter tensors that take part in a step.  torch keeps one step counter per parameter tensor and
 * skips tensors whose .grad is None (the fine net with run_fine = 0): leave those out of the ranges.  step: DEVICE int64
 * [n_steps] = the counters of the range's tensors (0 before the first step), all equal on entry - tensors with different
 * counts go into different ranges - and all incremented by the call; the bias corrections use step[0] + 1. */
typedef struct snerf_adam_range {
    int64_t begin, end;  /* parameters [begin, end) of the flat buffer */
    int64_t *step;
    int32_t n_steps;
} snerf_adam_range;
/* A RenderRayNet inside the flat buffer whose weight streams the step keeps current. */
typedef struct snerf_adam_net {
    const snerf_mlp_desc *desc;
    int64_t param_offset; /* its snerf_mlp_param_floats parameters (state_dict order) start at params + param_offset */
    int32_t precision;    /* 0: fp32 streams (refreshed in place); 2 / 3 / SNERF_SPLIT_F16X3: split streams (re-packed) */
    void *packed;         /* nullable: not kept current */
    void *packed_t;       /* nullable */
    const int32_t *slot_fwd, *slot_t; /* snerf_mlp_stream_slots (precision 0 only) */
} snerf_adam_net;
/* One optimiser step on the ranges (HOST array, at most 32) with the streams of at most 8 nets (HOST array) kept current. */
SNERF_API int snerf_adam_step_f32(const snerf_adam_state *state, const snerf_adam_range *ranges_host, int n_ranges,
                        const snerf_adam_net *nets_host, int n_nets, snerf_stream_t stream);

/* The batch as the Solver hands it to the pipeline (solver/nerf_solver.py:77-81) plus what utils.py draws inside. */
typedef struct snerf_nerf_batch {
    const float *ray_samples;  /* [B, Nc, 3] */
    const float *rays_o;       /* [B, 3] */
    const float *rays_d;       /* [B, 3] */
    const float *z_vals;       /* [B, Nc] */
    const float *rgb_truth;    /* [B, 3] */
    const float *u;            /* [Nf] = linspace(0, 1, Nf) (utils.py:204-206); unused with Nf == 0 */
    const float *noise_coarse; /* nullable [B, Nc]: sigma noise (utils.py:171-173) */
    const float *noise_fine;   /* nullable [B, Nc + Nf] */
    const float *additional;   /* [B, add_dim] per-ray additional inputs of nets with add_dim > 0 (the pose rows of
                                  models/append_smpl_params_pipeline.py:29-52, append_to_nerf_pipeline.py:26); else NULL */
    int64_t B;
    int32_t Nc, Nf;            /* Nf == 0 is run_fine = 0: loss = 2 MSE(rgb), no fine gradients (nerf_pipeline.py:43-44) */
    int32_t white_background;
} snerf_nerf_batch;

/* Forward with saved layer inputs, loss, backward: grad_coarse / grad_fine (snerf_mlp_param_floats floats each, state_dict
 * order, OVERWRITTEN; grad_fine untouched with Nf == 0) = what autograd leaves in .grad after loss.backward();
 * loss [3] = {MSE(rgb) + MSE(rgb_fine), MSE(rgb), MSE(rgb_fine)}; rgb / rgb_fine [B, 3] = the rendered colours.
 * precision as in snerf_render_rays_f32 (packed_* / packed_t_* from the matching pack calls).
 * The batch is walked in chunks of rays_per_chunk rays (<= 0 or > B: one chunk): d loss / d rgb of a ray does not depend on
 * the other rays, so forward and backward run chunk by chunk and the parameter gradients are summed in chunk order - the
 * saved activations (21 KB per ray-sample) are sized by the chunk, nothing is recomputed.
 * aux_stream (nullable): a second stream of the caller's.  Chunks of at most 262 144 samples (1024 rays of 64 + 192; the
 * README's 64-ray batches) leave CUs idle in some kernel; there the coarse net's backward - independent of the fine net's, the
 * hierarchical samples being detached (utils.py:260) - is enqueued on aux_stream beside it (forked from and joined back into
 * `stream` with events, also under graph capture).  NULL: everything on `stream`.  Same results either way.
 * workspace: snerf_nerf_train_workspace_bytes(...) bytes, 256-byte aligned. */
SNERF_API int64_t snerf_nerf_train_workspace_bytes(const snerf_mlp_desc *desc_coarse, const snerf_mlp_desc *desc_fine, int64_t B, int Nc,
                                         int Nf, int64_t rays_per_chunk);
SNERF_API int snerf_nerf_train_grads_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                               const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine, int precision,
                               const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace, float *grad_coarse,
                               float *grad_fine, float *loss, float *rgb, float *rgb_fine, snerf_stream_t stream,
                               snerf_stream_t aux_stream);
/* snerf_nerf_train_grads_f32 followed by snerf_adam_step_f32 (single-GPU step; a data-parallel trainer calls the two halves
 * with its gradient all-reduce in between). */
SNERF_API int snerf_nerf_train_step_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                              const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine, int precision,
                              const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace, float *grad_coarse,
                              float *grad_fine, float *loss, float *rgb, float *rgb_fine, const snerf_adam_state *adam,
                              const snerf_adam_range *ranges_host, int n_ranges, const snerf_adam_net *nets_host, int n_nets,
                              snerf_stream_t stream, snerf_stream_t aux_stream);

/* The same with d loss / d batch->additional as one more output (nets with add_dim > 0): what autograd returns for the per-ray pose
 * rows / vertex floats the pipelines expand over a ray's samples (models/append_smpl_params_pipeline.py:29-52,
 * append_to_nerf_pipeline.py:26, append_vertices_pipeline.py:37-58) - the gradient AppendVerticesSolver's second parameter
 * group (solver/append_vertices_solver.py: the pose estimator, lrate_pose) and a goal_pose that requires a gradient are trained
 * from.  d_additional [B, add_dim] is OVERWRITTEN: the stored d Y of layer 0 and of every skip layer of both nets contracted with
 * the weight columns that read the additional inputs (snerf_dy_contract_f32), summed over the samples of each ray.  params_*: the
 * nets' parameters (snerf_mlp_param_floats floats, state_dict order - the weight columns are read from there); the step variant
 * reads them before Adam updates them.  input_grads == NULL or d_additional == NULL: exactly snerf_nerf_train_grads_f32 / _step_f32.
 * The workspace of snerf_nerf_train_workspace_bytes covers the contraction's scratch. */
typedef struct snerf_input_grads {
    float *d_additional;
    const float *params_coarse;
    const float *params_fine; /* unused with Nf == 0 */
} snerf_input_grads;
SNERF_API int snerf_nerf_train_grads_ig_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                  const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine, int precision,
                                  const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace, float *grad_coarse,
                                  float *grad_fine, float *loss, float *rgb, float *rgb_fine, const snerf_input_grads *input_grads,
                                  snerf_stream_t stream, snerf_stream_t aux_stream);
SNERF_API int snerf_nerf_train_step_ig_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                 const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine, int precision,
                                 const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace, float *grad_coarse,
                                 float *grad_fine, float *loss, float *rgb, float *rgb_fine, const snerf_adam_state *adam,
                                 const snerf_adam_range *ranges_host, int n_ranges, const snerf_adam_net *nets_host, int n_nets,
                                 const snerf_input_grads *input_grads, snerf_stream_t stream, snerf_stream_t aux_stream);

/* ---- a7 + a9: SmplNerfSolver.train's per-batch body as one call (solver/smpl_nerf_solver.py:76-89 with the default loss,
 * models/smpl_nerf_pipeline.py:16-100, human_pose_encoding = 1) ------------------------------------------------------
 * snerf_nerf_train_* with the warp stage in front of both nets and its backward behind them: warp forward (saving its rows)
 * -> net on (x', x' - o) -> compositing (coarse: scaled per sample by |x' - o|; fine: by the ray direction) -> ... -> MSE ->
 * compositing backward (coarse: also into x' - o) -> net backward INTO its inputs (snerf_mlp_bwd_inputs_*: packed_t_* are the
 * input_grad = 1 streams) -> d warp = d x' + d (x' - o) -> warp backward; the warp net's gradient is the sum over its two
 * evaluations.  pose_enc [B, pose_dim] = the encoded two joint angles (:28-30).  The warp net trains in fp32 in every
 * precision mode.  In the split-precision modes the nets' input gradients exist for encoders of at most 4 position / 2
 * direction k-blocks of 16 slots (the defaults: 10 / 4 frequencies without identity columns); wider ones are SNERF_E_BADARG
 * here - run those nets with precision 0 (the Python trainer takes its autograd path, which routes that dgrad to fp32).  grad_warp: snerf_warp_param_floats floats.  Ray chunks, workspace, loss, rgb as in snerf_nerf_train_grads_f32.
 * The step variant runs snerf_adam_step_f32 and then re-packs the warp net's two streams (packed_warp from snerf_warp_pack_f32,
 * packed_t_warp from snerf_warp_pack_t_f32) from its parameters at params + warp_param_offset. */
SNERF_API int64_t snerf_smpl_nerf_train_workspace_bytes(const snerf_mlp_desc *desc_coarse, const snerf_mlp_desc *desc_fine,
                                              const snerf_warp_desc *desc_warp, int64_t B, int Nc, int Nf, int64_t rays_per_chunk);
SNERF_API int snerf_smpl_nerf_train_grads_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                    const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                    const snerf_warp_desc *desc_warp, const float *packed_warp, const float *packed_t_warp,
                                    int precision, const snerf_nerf_batch *batch, const float *pose_enc, int64_t rays_per_chunk,
                                    void *workspace, float *grad_coarse, float *grad_fine, float *grad_warp, float *loss, float *rgb,
                                    float *rgb_fine, snerf_stream_t stream);
SNERF_API int snerf_smpl_nerf_train_step_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                   const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                   const snerf_warp_desc *desc_warp, float *packed_warp, float *packed_t_warp, int precision,
                                   const snerf_nerf_batch *batch, const float *pose_enc, int64_t rays_per_chunk, void *workspace,
                                   float *grad_coarse, float *grad_fine, float *grad_warp, float *loss, float *rgb, float *rgb_fine,
                                   const snerf_adam_state *adam, const snerf_adam_range *ranges_host, int n_ranges,
                                   const snerf_adam_net *nets_host, int n_nets, int64_t warp_param_offset, snerf_stream_t stream);
/* packed_warp / packed_t_warp (each nullable) from the warp net's parameters at params + warp_param_offset: what a
 * data-parallel caller runs behind snerf_adam_step_f32. */
SNERF_API int snerf_warp_repack_f32(const snerf_warp_desc *desc_warp, const float *params, int64_t n_params, int64_t warp_param_offset,
                          float *packed_warp, float *packed_t_warp, snerf_stream_t stream);

/* ---- a2 / a7 for ANY width: nn.Linear as stand-alone fp32 MFMA GEMMs (0.1.9) -----------------------------------------------
 * config_parser.py:20,24,30 accept any --netwidth / --netwidth_fine / --netwidth_warp.  The fused kernels above cover
 * RenderRayNet up to 512 features and WarpFieldNet up to 256; wider nets run one nn.Linear at a time with the activations in HBM,
 * as models/render_ray_net.py:42-61 / models/warp_field_net.py:17-21 do, through these entries.  Weights are read in the
 * reference's own layout: w is [m, k] = [out, in] row-major with leading dimension ldw (a slice of the flat parameter vector; a
 * column block of a wider matrix - the two input blocks of a skip layer - is w + offset with the full matrix's ldw).  All matrices
 * row-major fp32 with explicit leading dimensions (in floats); exact fp32 (v_mfma_f32_16x16x4_f32).
 *   snerf_linear_fwd_f32         y[n, m]  (+)= x[n, k] w^T, then + bias[m] (nullable), then ReLU (relu != 0)
 *   snerf_linear_bwd_input_f32   dx[n, k] (+)= dy[n, m] w
 *   snerf_linear_bwd_weight_f32  dw[m, k] (+)= dy^T x and db[m] (+)= column sums of dy (db nullable); the sum over the samples is
 *                                split into slices whose partials go through `scratch`
 *                                (snerf_linear_bwd_weight_scratch_floats(n, m, k) floats) and are added in slice order
 *   snerf_relu_bwd_f32           dy[i, j] = y[i, j] > 0 ? dy[i, j] : 0, in place
 * (accumulate != 0: += instead of =). */
SNERF_API int snerf_linear_fwd_f32(const float *x, int64_t n, int k, int64_t ldx, const float *w, int64_t ldw, int m, const float *bias,
                         int accumulate, int relu, float *y, int64_t ldy, snerf_stream_t stream);
SNERF_API int snerf_linear_bwd_input_f32(const float *dy, int64_t n, int m, int64_t lddy, const float *w, int64_t ldw, int k, int accumulate,
                               float *dx, int64_t lddx, snerf_stream_t stream);
SNERF_API int64_t snerf_linear_bwd_weight_scratch_floats(int64_t n, int m, int k);
SNERF_API int snerf_linear_bwd_weight_f32(const float *dy, int64_t n, int m, int64_t lddy, const float *x, int64_t ldx, int k, int accumulate,
                                float *dw, int64_t lddw, float *db, float *scratch, snerf_stream_t stream);
SNERF_API int snerf_relu_bwd_f32(float *dy, const float *y, int64_t n, int m, int64_t lddy, int64_t ldy, snerf_stream_t stream);

/* ---- 8(e): the data-parallel step as one call ---------------------------------------------------------------------------
 * Rays of independent images shard over the GPUs of a node, one process per GPU; the only exchange of the path is the average of
 * the replicated nets' gradients.  snerf_comm_t is an ncclComm_t of RCCL (bound at run time: librccl.so.1 is loaded by the first
 * snerf_comm_* / *_dp_* call, the copy the process already holds if there is one).  A host with its own communicator passes it
 * as is; one without creates it here: rank 0 calls snerf_comm_unique_id, hands the SNERF_COMM_ID_BYTES bytes to the other ranks
 * by whatever channel it has (a file, MPI, torch.distributed's store), and every rank calls snerf_comm_init_rank - collective,
 * with its HIP device current.  snerf_comm_destroy(NULL) is a no-op. */
typedef void *snerf_comm_t; /* ncclComm_t */
#define SNERF_COMM_ID_BYTES 128
SNERF_API int snerf_comm_unique_id(void *id_host);
SNERF_API int snerf_comm_init_rank(const void *id_host, int world_size, int rank, snerf_comm_t *comm);
SNERF_API int snerf_comm_destroy(snerf_comm_t comm);
SNERF_API int snerf_comm_info(snerf_comm_t comm, int32_t *world_size, int32_t *rank);
/* buf[0 .. n) <- its average over the ranks, in place, enqueued on `stream` (ncclAllReduce, ncclAvg, fp32). */
SNERF_API int snerf_comm_allreduce_avg_f32(snerf_comm_t comm, float *buf, int64_t n, snerf_stream_t stream);
/* snerf_nerf_train_step_f32 / snerf_smpl_nerf_train_step_f32 with the gradient average between the backward and the optimiser:
 * ... -> backward -> ncclAllReduce(ncclAvg) of adam->grads[0 .. adam->n_params) - the trainer's flat gradient buffer, which holds
 * grad_coarse / grad_fine (/ grad_warp) as segments and is the same size on every rank -> Adam.  The collectives of a nerf step
 * are the same two on every rank whatever its batch size, chunking and streams (0.1.9): the coarse net's segment, then the rest
 * of the buffer (one grouped launch), both on `stream` behind the join of the concurrent backward - one communicator never has
 * collectives in flight on two streams; the smpl_nerf steps issue one all-reduce of the whole buffer on `stream`.  batch->B == 0 is valid here (a rank whose
 * shard ran out): zero gradient, zero loss, the same collectives, the optimiser step.  Nothing is synchronised; every rank must
 * make the same calls in the same order (RCCL's rule).  Graph-capturable.  SNERF_RCCL_LIB=<path> (read at the first call)
 * names the library to bind instead of librccl.so.1. */
SNERF_API int snerf_nerf_train_step_dp_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                 const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine, int precision,
                                 const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace, float *grad_coarse,
                                 float *grad_fine, float *loss, float *rgb, float *rgb_fine, const snerf_adam_state *adam,
                                 const snerf_adam_range *ranges_host, int n_ranges, const snerf_adam_net *nets_host, int n_nets,
                                 snerf_comm_t comm, snerf_stream_t stream, snerf_stream_t aux_stream);
/* snerf_nerf_train_step_ig_f32 with the gradient average: the data-parallel step of the pose-conditioned pipelines whose
 * estimator / goal_pose is trained too (BASELINE configs[4]; solver/append_vertices_solver.py:26-31, 77-82: the lrate_pose group).
 * input_grads->d_additional [B, add_dim] holds THIS rank's rows (per-ray data: nothing to average); the caller continues its
 * autograd from them into the estimator and averages that module's gradient segment with snerf_comm_allreduce_avg_f32 before
 * its optimiser step.  Same collectives, in the same order, as snerf_nerf_train_step_dp_f32. */
SNERF_API int snerf_nerf_train_step_dp_ig_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                    const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine, int precision,
                                    const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace, float *grad_coarse,
                                    float *grad_fine, float *loss, float *rgb, float *rgb_fine, const snerf_adam_state *adam,
                                    const snerf_adam_range *ranges_host, int n_ranges, const snerf_adam_net *nets_host, int n_nets,
                                    const snerf_input_grads *input_grads, snerf_comm_t comm, snerf_stream_t stream,
                                    snerf_stream_t aux_stream);
SNERF_API int snerf_smpl_nerf_train_step_dp_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                      const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                      const snerf_warp_desc *desc_warp, float *packed_warp, float *packed_t_warp, int precision,
                                      const snerf_nerf_batch *batch, const float *pose_enc, int64_t rays_per_chunk, void *workspace,
                                      float *grad_coarse, float *grad_fine, float *grad_warp, float *loss, float *rgb, float *rgb_fine,
                                      const snerf_adam_state *adam, const snerf_adam_range *ranges_host, int n_ranges,
                                      const snerf_adam_net *nets_host, int n_nets, int64_t warp_param_offset, snerf_comm_t comm,
                                      snerf_stream_t stream);

/* The smpl_nerf step with an auxiliary stream (0.1.8).  As snerf_smpl_nerf_train_grads_f32 / _step_f32 / _step_dp_f32 with one more
 * argument: aux_stream (may be NULL or == stream: then exactly those calls).  For chunks of at most 262144 fine-pass samples
 * (snerf_smpl_nerf_train_workspace_bytes already counts the second scratch set under that rule) the coarse chain of the backward -
 * compositing, coarse net dgrad + wgrad, the warp net's backward on the coarse samples - runs on aux_stream beside the fine chain on
 * `stream`, forked and joined with events inside the call; the coarse chain's warp-net gradient is added behind the join in the order
 * of the sequential form, so the results are bit-identical with and without aux_stream.  comm (step form; may be NULL): the flat
 * gradient buffer adam->grads is averaged over the ranks (ncclAllReduce, ncclAvg) between the backward and Adam.
 * Replaces: solver/smpl_nerf_solver.py:76-89 per batch, as the entry points it extends. */
SNERF_API int snerf_smpl_nerf_train_grads_aux_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                        const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                        const snerf_warp_desc *desc_warp, const float *packed_warp, const float *packed_t_warp,
                                        int precision, const snerf_nerf_batch *batch, const float *pose_enc, int64_t rays_per_chunk,
                                        void *workspace, float *grad_coarse, float *grad_fine, float *grad_warp, float *loss, float *rgb,
                                        float *rgb_fine, snerf_stream_t stream, snerf_stream_t aux_stream);
SNERF_API int snerf_smpl_nerf_train_step_aux_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                       const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                       const snerf_warp_desc *desc_warp, float *packed_warp, float *packed_t_warp, int precision,
                                       const snerf_nerf_batch *batch, const float *pose_enc, int64_t rays_per_chunk, void *workspace,
                                       float *grad_coarse, float *grad_fine, float *grad_warp, float *loss, float *rgb, float *rgb_fine,
                                       const snerf_adam_state *adam, const snerf_adam_range *ranges_host, int n_ranges,
                                       const snerf_adam_net *nets_host, int n_nets, int64_t warp_param_offset, snerf_comm_t comm,
                                       snerf_stream_t stream, snerf_stream_t aux_stream);

#ifdef __cplusplus
}
#endif
#endif /* SMPLNERF_H */
