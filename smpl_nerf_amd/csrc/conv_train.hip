// SmplEstimator's convolution block in training mode (models/smpl_estimator.py:35-39 under nn.Module.train()):
//
//   z = conv3x3_pad1(x, w) + b          csrc/conv_block.hip's kernel with scale = 1, shift = b, no ReLU, no pool (x 1 is exact)
//   mean, invstd = batch statistics of z per channel over M = N H W elements (biased variance), running statistics moved in place
//   y = [maxpool2x2](relu((z - mean) invstd gamma + beta))
// and its backward, given dy: dgamma, dbeta, dz, then dx = conv3x3_pad1(dz, w') and dW, db.  Contiguous NCHW fp32.
//
// Elementwise arithmetic, the same expression in the forward and in both backward passes (so they agree on every mask and argmax):
//   xhat = (z - mean) * invstd      pre = xhat * gamma + beta      fp32, one rounding per operation (-ffp-contract=off)
// Pool rule: the gradient of a window goes to the FIRST position (0,0), (0,1), (1,0), (1,1) that holds the window's maximum of
// relu(pre) (torch's `val > maxval` scan); ReLU rule: gradient 0 where pre <= 0.  Nothing is stored for either: the backward passes
// recompute pre from z.
//
// Per-channel sums (the statistics, s1 = sum g and s2 = sum g xhat, db = sum dz) - ONE skeleton, float64, no atomics:
//   the n-major index m = n Q + q over the channel's N Q terms (Q = H W, or Ho Wo windows for the pooled backward) is cut into
//   S = red_slices(N Q) = min(128, ceil(N Q / 8192)) slices of L = ceil(N Q / S) consecutive terms.  A workgroup of 256 threads owns
//   one (channel, slice): thread t adds terms lo + t, lo + t + 256, .. in ascending order; the 64 lanes of a wave are added by a DPP
//   scan (snerf_common.h wave_sum: a fixed tree); thread 0 adds the four waves in wave order and writes the partial.  A finisher adds
//   the S partials of a channel in slice order.  Everything depends on the shapes alone.
//   Statistics: sum z and sum z^2 in float64; mean = sum / M, var = max(sum2 / M - mean^2, 0) in float64, each result rounded once.
//
// Weight gradient - the MFMA kernel.  dW[co][ci][ky][kx] = sum_{n,y,x} dz[n][co][y][x] xpad[n][ci][y + ky - 1][x + kx - 1] on
// v_mfma_f32_16x16x4_f32 (exact fp32, an fmaf chain), the reduction index being the PIXEL:
//   per tap (ky, kx):  D_tap[co][ci] += sum_k A[co][k] B_tap[k][ci]      A = dz[co][pixel], B_tap = xpad[ci][pixel + tap]
// Tile.  A workgroup of 4 waves owns 16 MT output channels (MT = 1, 2 by Co) x 16 input channels x 9 taps = 9 MT accumulator tiles
// PER WAVE and walks a fixed slice of (image, 16 x 16 pixel tile) jobs.  Wave w multiplies rows 4 w .. 4 w + 3 of every pixel tile:
// 16 steps of 4 consecutive pixels of a row; per step MT A reads and 9 B reads feed 9 MT MFMAs on independent accumulators.  The
// accumulators stay in registers across the slice; then waves 1, 2, 3 hand theirs to wave 0 through LDS, which adds them in wave
// order and writes the slice's partial tile.  A finisher adds the partials in slice order in float64 and rounds once.
// LDS per job (all of it written for every job - halo zeros, channels past Ci / Co and pixels past the image included):
//   s_in [16][18][20] + 2  the input tile with its halo as in the forward kernel, plane pitch 362 = 10 mod 32: a B read's 32-lane
//                          half is 16 channels x 2 adjacent pixels = banks 10 ci + k, all distinct
//   s_dz [16 MT][258]      the dz tile, row pitch 258 = 2 mod 32: an A read's half is 16 channels x 2 pixels = banks 2 co + k
// Summation order of a dW element: per slice and wave one chain over that wave's pixels, jobs ascending, rows ascending, 4 pixels
// per step left to right; then wave 0 + 1 + 2 + 3; then the slices ascending.  The slice count is
// wgrad_slices = min(jobs, ceil(512 / column groups)) re-divided evenly - a function of the shapes, not of the CU count.
#include <math.h>

#include <algorithm>

#include "conv_block.h"

namespace snerf {

typedef float tf4 __attribute__((ext_vector_type(4)));

// ---- the reduction skeleton --------------------------------------------------------------------------------------------------------
constexpr int RED_THREADS = 256;
constexpr int RED_MAX_SLICES = 128;
constexpr int64_t RED_TERMS = 8192;
static int red_slices(int64_t terms) { return (int)std::max<int64_t>(1, std::min<int64_t>(RED_MAX_SLICES, (terms + RED_TERMS - 1) / RED_TERMS)); }

struct BnArgs {
    const float *z, *dy, *mean, *invstd, *gamma, *beta;
    int C, H, W, Ho, Wo;     // Ho, Wo: the extents of y / dy (H / 2, W / 2 with pooling)
    int relu, pool;
};

__device__ __forceinline__ float bn_xhat(float z, float mean, float invstd) { return __fmul_rn(__fsub_rn(z, mean), invstd); }
__device__ __forceinline__ float bn_pre(float xhat, float gamma, float beta) { return __fadd_rn(__fmul_rn(xhat, gamma), beta); }

// the 2 x 2 window at (2 oy, 2 ox) of plane zc: xhat of its four positions, the pooled value, and the position the gradient goes to
// (-1: nowhere, the ReLU holds it back)
__device__ __forceinline__ float pool_window(const BnArgs &G, const float *zc, int oy, int ox, float mean, float invstd, float gamma, float beta,
                                             float (&xh)[4], int &winner) {
    float best = 0.f, pre_best = 0.f;
    winner = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        xh[d] = bn_xhat(zc[(int64_t)(2 * oy + (d >> 1)) * G.W + 2 * ox + (d & 1)], mean, invstd);
        const float pre = bn_pre(xh[d], gamma, beta), v = G.relu ? fmaxf(pre, 0.f) : pre;
        if (d == 0 || v > best) best = v, pre_best = pre, winner = d;
    }
    if (G.relu && !(pre_best > 0.f)) winner = -1;
    return best;
}

// term (n, c, q) of a per-channel sum: a += .., b += ..
struct StatsTerm {
    const float *z;
    int C, Q;
    __device__ __forceinline__ void operator()(int n, int c, int q, double &a, double &b) const {
        const double v = (double)z[((int64_t)n * C + c) * Q + q];
        a += v, b += v * v;
    }
};
struct SumTerm {     // db = sum dz
    const float *z;
    int C, Q;
    __device__ __forceinline__ void operator()(int n, int c, int q, double &a, double &) const { a += (double)z[((int64_t)n * C + c) * Q + q]; }
};
struct BwdTerm {     // s1 = sum g, s2 = sum g xhat; q is a pixel, or a pool window
    BnArgs G;
    __device__ __forceinline__ void operator()(int n, int c, int q, double &a, double &b) const {
        const float mean = G.mean[c], invstd = G.invstd[c], gamma = G.gamma[c], beta = G.beta[c];
        const float *zc = G.z + ((int64_t)n * G.C + c) * G.H * G.W;
        const float g = G.dy[((int64_t)n * G.C + c) * G.Ho * G.Wo + q];
        if (G.pool) {
            const int oy = (int)((unsigned)q / (unsigned)G.Wo), ox = q - oy * G.Wo;
            float xh[4];
            int winner;
            pool_window(G, zc, oy, ox, mean, invstd, gamma, beta, xh, winner);
#pragma unroll
            for (int d = 0; d < 4; ++d)
                if (d == winner) a += (double)g, b += (double)g * (double)xh[d];
        } else {
            const float xh = bn_xhat(zc[q], mean, invstd);
            if (!G.relu || bn_pre(xh, gamma, beta) > 0.f) a += (double)g, b += (double)g * (double)xh;
        }
    }
};

// partial[(c S + s) 2 + {0, 1}] of the terms [s L, min((s + 1) L, N Q)) of channel c = blockIdx.y, s = blockIdx.x
template <class Term>
__global__ __launch_bounds__(RED_THREADS) void reduce_partials_kernel(Term term, int Q, int terms, int L, double *partial) {
    __shared__ double s_a[RED_THREADS / WAVE], s_b[RED_THREADS / WAVE];
    const int tid = threadIdx.x, c = blockIdx.y, s = blockIdx.x;
    const unsigned lo = (unsigned)s * (unsigned)L, hi = min(lo + (unsigned)L, (unsigned)terms);     // (unsigned: terms + 256 may pass 2^31)
    double a = 0.0, b = 0.0;
    for (unsigned i = lo + tid; i < hi; i += RED_THREADS) {
        const unsigned n = i / (unsigned)Q;
        term((int)n, c, (int)(i - n * (unsigned)Q), a, b);
    }
    a = wave_sum(a), b = wave_sum(b);
    if ((tid & 63) == 0) s_a[tid >> 6] = a, s_b[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        double ta = s_a[0], tb = s_b[0];
#pragma unroll
        for (int w = 1; w < RED_THREADS / WAVE; ++w) ta += s_a[w], tb += s_b[w];
        double *p = partial + ((int64_t)c * gridDim.x + s) * 2;
        p[0] = ta, p[1] = tb;
    }
}

__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double *partial, int C, int S, double M, double eps, double momentum,
                                                              float *running_mean, float *running_var, float *mean, float *invstd) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int s = 0; s < S; ++s) a += partial[((int64_t)c * S + s) * 2], b += partial[((int64_t)c * S + s) * 2 + 1];
    const double mu = a / M, var = fmax(b / M - mu * mu, 0.0);
    mean[c] = (float)mu;
    invstd[c] = (float)(1.0 / sqrt(var + eps));
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mu);
    if (running_var) running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * M / (M - 1.0)));
}

// dbeta = s1, dgamma = s2, rounded once; coef[2 c] = s1 / M, coef[2 c + 1] = s2 / M in float64 for the second pass
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double *partial, int C, int S, double M, float *dgamma, float *dbeta, double *coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int s = 0; s < S; ++s) a += partial[((int64_t)c * S + s) * 2], b += partial[((int64_t)c * S + s) * 2 + 1];
    if (dbeta) dbeta[c] = (float)a;
    if (dgamma) dgamma[c] = (float)b;
    coef[2 * c] = a / M, coef[2 * c + 1] = b / M;
}

__global__ __launch_bounds__(256) void sum_finish_kernel(const double *partial, int C, int S, float *out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += partial[((int64_t)c * S + s) * 2];
    out[c] = (float)a;
}

// ---- apply: y = [pool](relu(pre)), one thread per element of y ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_apply_kernel(BnArgs G, float *y, int total) {
    const unsigned at = blockIdx.x * 256u + threadIdx.x;
    if (at >= (unsigned)total) return;
    const int i = (int)at;
    const int Qo = G.Ho * G.Wo, nc = (int)((unsigned)i / (unsigned)Qo), q = i - nc * Qo, c = nc % G.C;
    const float mean = G.mean[c], invstd = G.invstd[c], gamma = G.gamma[c], beta = G.beta[c];
    const float *zc = G.z + (int64_t)nc * G.H * G.W;
    if (G.pool) {
        const int oy = (int)((unsigned)q / (unsigned)G.Wo), ox = q - oy * G.Wo;
        float xh[4];
        int winner;
        y[i] = pool_window(G, zc, oy, ox, mean, invstd, gamma, beta, xh, winner);
    } else {
        const float pre = bn_pre(bn_xhat(zc[q], mean, invstd), gamma, beta);
        y[i] = G.relu ? fmaxf(pre, 0.f) : pre;
    }
}

// ---- backward, second pass: dz = gamma invstd (g - s1 / M - xhat s2 / M), float64 from the fp32 xhat, rounded once -----------------
// One thread per pixel, or with pooling per 2 x 2 cell of the ceil(H / 2) x ceil(W / 2) cells that cover the map: a cell past Ho or
// Wo is no window, its pixels have g = 0 (their dz is not 0: the batch statistics tie every pixel of a channel together).
__global__ __launch_bounds__(256) void bn_bwd_dz_kernel(BnArgs G, const double *coef, float *dz, int Hc, int Wc, int total) {
    const unsigned at = blockIdx.x * 256u + threadIdx.x;
    if (at >= (unsigned)total) return;
    const int i = (int)at;
    const int Qc = Hc * Wc, nc = (int)((unsigned)i / (unsigned)Qc), q = i - nc * Qc, c = nc % G.C;
    const float mean = G.mean[c], invstd = G.invstd[c], gamma = G.gamma[c], beta = G.beta[c];
    const double k = (double)gamma * (double)invstd, c1 = coef[2 * c], c2 = coef[2 * c + 1];
    const float *zc = G.z + (int64_t)nc * G.H * G.W;
    float *dzc = dz + (int64_t)nc * G.H * G.W;
    if (G.pool) {
        const int cy = (int)((unsigned)q / (unsigned)Wc), cx = q - cy * Wc;
        if (cy < G.Ho && cx < G.Wo) {
            float xh[4];
            int winner;
            pool_window(G, zc, cy, cx, mean, invstd, gamma, beta, xh, winner);
            const double g = (double)G.dy[(int64_t)nc * G.Ho * G.Wo + (int64_t)cy * G.Wo + cx];
#pragma unroll
            for (int d = 0; d < 4; ++d)
                dzc[(int64_t)(2 * cy + (d >> 1)) * G.W + 2 * cx + (d & 1)] = (float)(k * ((d == winner ? g : 0.0) - c1 - (double)xh[d] * c2));
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int py = 2 * cy + (d >> 1), px = 2 * cx + (d & 1);
                if (py < G.H && px < G.W) {
                    const int64_t o = (int64_t)py * G.W + px;
                    dzc[o] = (float)(k * (0.0 - c1 - (double)bn_xhat(zc[o], mean, invstd) * c2));
                }
            }
        }
    } else {
        const float xh = bn_xhat(zc[q], mean, invstd);
        const double g = (!G.relu || bn_pre(xh, gamma, beta) > 0.f) ? (double)G.dy[(int64_t)nc * G.H * G.W + q] : 0.0;
        dzc[q] = (float)(k * (g - c1 - (double)xh * c2));
    }
}

// ---- input gradient: w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx], and the forward kernel's scale = 1, shift = 0 ------------------
__global__ __launch_bounds__(256) void conv_flip_kernel(const float *w, int Ci, int Co, float *wt, float *ones, float *zeros) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Ci) ones[i] = 1.f, zeros[i] = 0.f;
    if (i >= Ci * Co * 9) return;
    const int r = i % 9, co = (i / 9) % Co, ci = i / (9 * Co);
    wt[i] = w[((int64_t)co * Ci + ci) * 9 + 8 - r];
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------------
constexpr int CT_TILE = 16, CT_HALO = CT_TILE + 2, CT_LW = 20;
constexpr int CT_CI = 16;                               // input channels per workgroup
constexpr int CT_PLANE = CT_HALO * CT_LW + 2;           // 362 = 10 mod 32
constexpr int CT_DP = CT_TILE * CT_TILE + 2;            // 258 = 2 mod 32
constexpr int CT_THREADS = 256;
constexpr int CT_TARGET = 512;                          // workgroups a call aims at: two per CU of the largest part, so that one loads while
                                                        // the other multiplies (a constant: the slices do not depend on the device)

struct WgradArgs {
    const float *dz, *x;
    float *partial;               // [slices][Co][Ci 9]
    int Ci, Co, H, W;
    int tiles_x, tiles, ci_groups;
    int jobs, jobs_per_slice;     // (image, tile) pairs; a slice is jobs_per_slice consecutive ones
};

static int wgrad_mt(int Co) { return Co <= 16 ? 1 : 2; }
static int wgrad_columns(int Ci, int Co) { return ((Co + 16 * wgrad_mt(Co) - 1) / (16 * wgrad_mt(Co))) * ((Ci + CT_CI - 1) / CT_CI); }
static void wgrad_split(int64_t N, int Ci, int Co, int64_t H, int64_t W, int64_t *jobs, int64_t *per_slice, int64_t *slices) {
    *jobs = N * ((H + CT_TILE - 1) / CT_TILE) * ((W + CT_TILE - 1) / CT_TILE);
    const int cols = wgrad_columns(Ci, Co);
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(*jobs, (CT_TARGET + cols - 1) / cols));
    *per_slice = std::max<int64_t>(1, (*jobs + want - 1) / want);
    *slices = std::max<int64_t>(1, (*jobs + *per_slice - 1) / *per_slice);
}

template <int MT>
__global__ __launch_bounds__(CT_THREADS) void conv3x3_wgrad_kernel(WgradArgs G) {
    __shared__ float s_in[CT_CI * CT_PLANE];
    __shared__ float s_dz[16 * MT * CT_DP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j16 = lane & 15, kq = lane >> 4;
    const int slice = blockIdx.x, cg = blockIdx.y % G.ci_groups, og = blockIdx.y / G.ci_groups;
    const int ci0 = cg * CT_CI, co0 = og * 16 * MT;
    const int job_lo = slice * G.jobs_per_slice, job_hi = min(job_lo + G.jobs_per_slice, G.jobs);
    const int64_t plane = (int64_t)G.H * G.W;
    tf4 acc[MT][9];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[m][t] = tf4{0.f, 0.f, 0.f, 0.f};
    for (int job = job_lo; job < job_hi; ++job) {
        const int n = job / G.tiles, tile = job - n * G.tiles, ty = tile / G.tiles_x, tx = tile - ty * G.tiles_x;
        const int y0 = ty * CT_TILE, x0 = tx * CT_TILE;
        __syncthreads();   // the previous job has been read
        {   // input tile: thread = (plane tid >> 5 (+ 8), column tid & 31 < 18), 18 rows each; zeros outside the image and past Ci
            const int xx = tid & 31, gx = x0 + xx - 1;
            if (xx < CT_HALO) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int c = (tid >> 5) + 8 * h;
                    const bool col = ci0 + c < G.Ci && gx >= 0 && gx < G.W;
                    const float *xp = G.x + ((int64_t)n * G.Ci + ci0 + c) * plane + gx;
#pragma unroll
                    for (int j = 0; j < CT_HALO; ++j) {
                        const int gy = y0 + j - 1;
                        float v = 0.f;
                        if (col && gy >= 0 && gy < G.H) v = xp[(int64_t)gy * G.W];
                        s_in[c * CT_PLANE + j * CT_LW + xx] = v;
                    }
                }
            }
            // dz tile: thread = pixel (tid >> 4, tid & 15), one channel per step; zeros past the image and past Co
            const int py = tid >> 4, px = tid & 15;
            const bool in = y0 + py < G.H && x0 + px < G.W;
            const float *dp = G.dz + ((int64_t)n * G.Co + co0) * plane + (int64_t)(y0 + py) * G.W + x0 + px;
#pragma unroll 8
            for (int c = 0; c < 16 * MT; ++c) {
                float v = 0.f;
                if (in && co0 + c < G.Co) v = dp[(int64_t)c * plane];
                s_dz[c * CT_DP + tid] = v;
            }
        }
        __syncthreads();
        // lane (j16, kq): A = dz[co0 + 16 m + j16][pixel kq of the step], B = xpad[ci0 + j16][that pixel + tap]
        const float *pa = s_dz + j16 * CT_DP + wave * 64 + kq;
        const float *pb = s_in + j16 * CT_PLANE + (wave * 4) * CT_LW + kq;
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const int row = s >> 2, px0 = (s & 3) * 4;
            float a[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) a[m] = pa[m * 16 * CT_DP + row * 16 + px0];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float b = pb[(row + t / 3) * CT_LW + px0 + t % 3];
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b, acc[m][t], 0, 0, 0);
            }
        }
    }
    // waves 1, 2, 3 -> wave 0 through LDS (s_dz holds 16 MT 258 >= 9 MT 256 floats), added in wave order
    float *s_x = s_dz;
    for (int w = 1; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s_x[((m * 9 + t) * 4 + r) * 64 + lane] = acc[m][t][r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[m][t][r] = __fadd_rn(acc[m][t][r], s_x[((m * 9 + t) * 4 + r) * 64 + lane]);
        }
    }
    if (wave != 0) return;
    // D layout: acc[m][t][r] = dW[co0 + 16 m + 4 kq + r][ci0 + j16][tap t]
    const int ci = ci0 + j16;
    if (ci >= G.Ci) return;
    float *out = G.partial + (int64_t)slice * G.Co * G.Ci * 9;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + 16 * m + 4 * kq + r;
            if (co >= G.Co) continue;
#pragma unroll
            for (int t = 0; t < 9; ++t) out[((int64_t)co * G.Ci + ci) * 9 + t] = acc[m][t][r];
        }
}

__global__ __launch_bounds__(256) void wgrad_finish_kernel(const float *partial, int count, int S, float *dw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += (double)partial[(int64_t)s * count + i];
    dw[i] = (float)a;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// the scalar checks of a BatchNorm entry: conv_check's limits on one channel count, and M = N H W >= 2 for N > 0
static int bn_check(const char *what, int64_t N, int C, int64_t H, int64_t W, int pool, int64_t *Ho, int64_t *Wo) {
    if (int rc = conv_check(what, N, C, H, W, C, pool, Ho, Wo)) return rc;
    if (N > 0 && N * H * W < 2)
        return fail(SNERF_E_BADARG, "%s: M = N H W = %lld: batch statistics need more than one value per channel", what, (long long)(N * H * W));
    return SNERF_OK;
}

template <class Term>
static int reduce_launch(const char *what, const Term &term, int64_t N, int C, int64_t Q, double *partial, hipStream_t s) {
    const int64_t terms = N * Q;
    const int S = red_slices(terms), L = (int)((terms + S - 1) / S);
    hipLaunchKernelGGL(reduce_partials_kernel<Term>, dim3(S, C), dim3(RED_THREADS), 0, s, term, (int)Q, (int)terms, L, partial);
    return check_launch(what);
}

}  // namespace snerf

using namespace snerf;

extern "C" int64_t snerf_bn_stats_scratch_floats(int64_t N, int C, int64_t H, int64_t W) {
    int64_t Ho, Wo;
    if (bn_check("bn_stats_scratch_floats", N, C, H, W, 0, &Ho, &Wo)) return SNERF_E_BADARG;
    return 4 * (int64_t)C * red_slices(N * H * W);     // [C][S] pairs of doubles
}

extern "C" int snerf_bn_stats_f32(const float *z, int64_t N, int C, int64_t H, int64_t W, double eps, double momentum, float *running_mean,
                                  float *running_var, float *mean, float *invstd, float *scratch, snerf_stream_t stream) {
    int64_t Ho, Wo;
    if (int rc = bn_check("bn_stats", N, C, H, W, 0, &Ho, &Wo)) return rc;
    if (!(eps >= 0.0) || !isfinite(eps)) return fail(SNERF_E_BADARG, "bn_stats: eps = %g is negative or not finite", eps);
    if (!isfinite(momentum)) return fail(SNERF_E_BADARG, "bn_stats: momentum = %g is not finite", momentum);
    if (N == 0) return SNERF_OK;
    if (!z || !mean || !invstd || !scratch)
        return fail(SNERF_E_BADARG, "bn_stats: null pointer (%s)", !z ? "z" : !mean ? "mean" : !invstd ? "invstd" : "scratch");
    if (!aligned(scratch, 8)) return fail(SNERF_E_ALIGN, "bn_stats: scratch %p is not 8-byte aligned", (void *)scratch);
    hipStream_t s = (hipStream_t)stream;
    double *partial = reinterpret_cast<double *>(scratch);
    const int64_t Q = H * W;
    if (int rc = reduce_launch("bn_stats(partials)", StatsTerm{z, C, (int)Q}, N, C, Q, partial, s)) return rc;
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, partial, C, red_slices(N * Q), (double)(N * Q), eps, momentum,
                       running_mean, running_var, mean, invstd);
    return check_launch("bn_stats(finish)");
}

extern "C" int snerf_bn_relu_pool_fwd_f32(const float *z, int64_t N, int C, int64_t H, int64_t W, const float *mean, const float *invstd,
                                          const float *gamma, const float *beta, int relu, int pool, float *y, snerf_stream_t stream) {
    int64_t Ho, Wo;
    if (int rc = conv_check("bn_relu_pool_fwd", N, C, H, W, C, pool, &Ho, &Wo)) return rc;
    if (N == 0) return SNERF_OK;
    if (!z || !mean || !invstd || !gamma || !beta || !y)
        return fail(SNERF_E_BADARG, "bn_relu_pool_fwd: null pointer (%s)", !z ? "z" : !mean ? "mean" : !invstd ? "invstd" : !gamma ? "gamma" : !beta ? "beta" : "y");
    const BnArgs G{z, nullptr, mean, invstd, gamma, beta, C, (int)H, (int)W, (int)Ho, (int)Wo, relu ? 1 : 0, pool ? 1 : 0};
    const int64_t total = N * C * Ho * Wo;
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, y, (int)total);
    return check_launch("bn_relu_pool_fwd");
}

extern "C" int64_t snerf_bn_relu_pool_bwd_scratch_floats(int64_t N, int C, int64_t H, int64_t W, int pool) {
    int64_t Ho, Wo;
    if (bn_check("bn_relu_pool_bwd_scratch_floats", N, C, H, W, pool, &Ho, &Wo)) return SNERF_E_BADARG;
    return 4 * (int64_t)C * red_slices(N * Ho * Wo) + 4 * (int64_t)C;     // [C][S] pairs of doubles, then [C] pairs
}

extern "C" int snerf_bn_relu_pool_bwd_f32(const float *z, const float *dy, int64_t N, int C, int64_t H, int64_t W, const float *mean,
                                          const float *invstd, const float *gamma, const float *beta, int relu, int pool, float *dz,
                                          float *dgamma, float *dbeta, float *scratch, snerf_stream_t stream) {
    int64_t Ho, Wo;
    if (int rc = bn_check("bn_relu_pool_bwd", N, C, H, W, pool, &Ho, &Wo)) return rc;
    if (N == 0) return SNERF_OK;
    if (!z || !dy || !mean || !invstd || !gamma || !beta || !scratch)
        return fail(SNERF_E_BADARG, "bn_relu_pool_bwd: null pointer (%s)",
                    !z ? "z" : !dy ? "dy" : !mean ? "mean" : !invstd ? "invstd" : !gamma ? "gamma" : !beta ? "beta" : "scratch");
    if (!aligned(scratch, 8)) return fail(SNERF_E_ALIGN, "bn_relu_pool_bwd: scratch %p is not 8-byte aligned", (void *)scratch);
    if (!dz && !dgamma && !dbeta) return SNERF_OK;
    hipStream_t s = (hipStream_t)stream;
    const BnArgs G{z, dy, mean, invstd, gamma, beta, C, (int)H, (int)W, (int)Ho, (int)Wo, relu ? 1 : 0, pool ? 1 : 0};
    const int64_t Qo = Ho * Wo;
    const int S = red_slices(N * Qo);
    double *partial = reinterpret_cast<double *>(scratch), *coef = partial + 2 * (int64_t)C * S;
    if (int rc = reduce_launch("bn_relu_pool_bwd(partials)", BwdTerm{G}, N, C, Qo, partial, s)) return rc;
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, partial, C, S, (double)(N * H * W), dgamma, dbeta, coef);
    if (int rc = check_launch("bn_relu_pool_bwd(finish)")) return rc;
    if (!dz) return SNERF_OK;
    const int Hc = pool ? (int)((H + 1) / 2) : (int)H, Wc = pool ? (int)((W + 1) / 2) : (int)W;
    const int64_t total = N * C * Hc * Wc;
    hipLaunchKernelGGL(bn_bwd_dz_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, G, coef, dz, Hc, Wc, (int)total);
    return check_launch("bn_relu_pool_bwd(dz)");
}

extern "C" int64_t snerf_conv3x3_bwd_input_scratch_floats(int Ci, int Co) {
    int64_t Ho, Wo;
    if (conv_check("conv3x3_bwd_input_scratch_floats", 0, Ci, 1, 1, Co, 0, &Ho, &Wo)) return SNERF_E_BADARG;
    return (int64_t)Ci * Co * 9 + 2 * (int64_t)Ci;     // w', then scale = 1 and shift = 0 per input channel
}

extern "C" int snerf_conv3x3_bwd_input_f32(const float *dz, int64_t N, int Co, int64_t H, int64_t W, const float *w, int Ci, float *dx,
                                           float *scratch, snerf_stream_t stream) {
    int64_t Ho, Wo;
    if (int rc = conv_check("conv3x3_bwd_input", N, Ci, H, W, Co, 0, &Ho, &Wo)) return rc;
    if (N == 0) return SNERF_OK;
    if (!dz || !w || !dx || !scratch) return fail(SNERF_E_BADARG, "conv3x3_bwd_input: null pointer (%s)", !dz ? "dz" : !w ? "w" : !dx ? "dx" : "scratch");
    hipStream_t s = (hipStream_t)stream;
    const int count = Ci * Co * 9;
    float *wt = scratch, *ones = scratch + count, *zeros = ones + Ci;
    hipLaunchKernelGGL(conv_flip_kernel, dim3((count + 255) / 256), dim3(256), 0, s, w, Ci, Co, wt, ones, zeros);
    if (int rc = check_launch("conv3x3_bwd_input(flip)")) return rc;
    return conv_launch("conv3x3_bwd_input", dz, N, Co, (int)H, (int)W, wt, ones, zeros, Ci, 0, 0, dx, s);
}

extern "C" int64_t snerf_conv3x3_bwd_weight_slices(int64_t N, int Ci, int64_t H, int64_t W, int Co) {
    int64_t Ho, Wo, jobs, per, slices;
    if (conv_check("conv3x3_bwd_weight_slices", N, Ci, H, W, Co, 0, &Ho, &Wo)) return SNERF_E_BADARG;
    wgrad_split(N, Ci, Co, H, W, &jobs, &per, &slices);
    return N == 0 ? 0 : slices;
}

extern "C" int64_t snerf_conv3x3_bwd_weight_scratch_floats(int64_t N, int Ci, int64_t H, int64_t W, int Co) {
    const int64_t slices = snerf_conv3x3_bwd_weight_slices(N, Ci, H, W, Co);
    if (slices < 0) return SNERF_E_BADARG;
    return 4 * (int64_t)Co * red_slices(N * H * W) + slices * Co * Ci * 9;     // db's [Co][S] pairs of doubles, then the partial tiles
}

extern "C" int snerf_conv3x3_bwd_weight_f32(const float *dz, const float *x, int64_t N, int Ci, int Co, int64_t H, int64_t W, float *dw,
                                            float *dbias, float *scratch, snerf_stream_t stream) {
    int64_t Ho, Wo;
    if (int rc = conv_check("conv3x3_bwd_weight", N, Ci, H, W, Co, 0, &Ho, &Wo)) return rc;
    if (N == 0) return SNERF_OK;
    if (!dz || (dw && !x) || !scratch) return fail(SNERF_E_BADARG, "conv3x3_bwd_weight: null pointer (%s)", !dz ? "dz" : !scratch ? "scratch" : "x");
    if (!aligned(scratch, 8)) return fail(SNERF_E_ALIGN, "conv3x3_bwd_weight: scratch %p is not 8-byte aligned", (void *)scratch);
    if (!dw && !dbias) return SNERF_OK;
    hipStream_t s = (hipStream_t)stream;
    int64_t jobs, per, slices;
    wgrad_split(N, Ci, Co, H, W, &jobs, &per, &slices);
    const int count = Co * Ci * 9;
    double *partial = reinterpret_cast<double *>(scratch);
    float *tiles = scratch + 4 * (int64_t)Co * red_slices(N * H * W);
    if (dw) {
        WgradArgs G{dz, x, tiles, Ci, Co, (int)H, (int)W, 0, 0, (Ci + CT_CI - 1) / CT_CI, (int)jobs, (int)per};
        G.tiles_x = (int)((W + CT_TILE - 1) / CT_TILE);
        G.tiles = G.tiles_x * (int)((H + CT_TILE - 1) / CT_TILE);
        const dim3 grid((unsigned)slices, (unsigned)wgrad_columns(Ci, Co));
        if (wgrad_mt(Co) == 1) hipLaunchKernelGGL(conv3x3_wgrad_kernel<1>, grid, dim3(CT_THREADS), 0, s, G);
        else hipLaunchKernelGGL(conv3x3_wgrad_kernel<2>, grid, dim3(CT_THREADS), 0, s, G);
        if (int rc = check_launch("conv3x3_bwd_weight(tiles)")) return rc;
        hipLaunchKernelGGL(wgrad_finish_kernel, dim3((count + 255) / 256), dim3(256), 0, s, tiles, count, (int)slices, dw);
        if (int rc = check_launch("conv3x3_bwd_weight(finish)")) return rc;
    }
    if (dbias) {
        const int64_t Q = H * W;
        if (int rc = reduce_launch("conv3x3_bwd_weight(db partials)", SumTerm{dz, Co, (int)Q}, N, Co, Q, partial, s)) return rc;
        hipLaunchKernelGGL(sum_finish_kernel, dim3((Co + 255) / 256), dim3(256), 0, s, partial, Co, red_slices(N * Q), dbias);
        return check_launch("conv3x3_bwd_weight(db finish)");
    }
    return SNERF_OK;
}
