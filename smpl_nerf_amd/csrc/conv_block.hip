// SmplEstimator's convolution block as one launch, and the whole network as one call (models/smpl_estimator.py:6-47, eval mode).
//
//   y = [maxpool2x2](relu(scale[co] * conv3x3_pad1(x, w)[co] + shift[co]))          x [N,Ci,H,W], w [Co,Ci,3,3], contiguous fp32
//
// Implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32, an fmaf chain): D[co][pixel] = sum_k W[co][k] X[k][pixel] with
// k = ci 9 + ky 3 + kx, K = 9 Ci.  A = the weights (row = output channel), B = the input patches (column = pixel).
//
// Tile.  A workgroup of 4 waves owns 16 x 16 output pixels of one image and 16 MT output channels (MT = 1, 2, 4 by Co).  A wave owns
// an 8 x 8 quadrant = 4 x 4 pool windows.  Its 4 B tiles are the 4 positions (dy, dx) of a pool window: column p = lane & 15 of tile
// (dy, dx) is pixel (2 (p >> 2) + dy, 2 (p & 3) + dx) of the quadrant.  So the four pixels of a window are four accumulators of ONE
// lane, and the epilogue - scale, shift, ReLU, the 2 x 2 max - stays in registers; with pooling on the un-pooled map is never stored,
// unless the caller asks for it as well (snerf_conv3x3_block_tap_f32: both maps from the same accumulators in one launch).
//
// LDS.  The reduction is walked in chunks of 8 input channels = 72 elements = 18 MFMA steps.  Per chunk:
//   s_in [8][18][20]  the 16 x 16 input tile with its one-pixel halo; positions outside the image and channels past Ci are written
//                     as zeros.  Row pitch 20: the 16 lanes of one k read banks 8 py + 2 px (all distinct, even), the 16 lanes of
//                     the next k (one column further) the odd ones.
//   s_w  [16 MT][74]  the weight slice, zero past Ci 9.  Row pitch 74 = 10 mod 32: 16 channels x 2 k on 32 distinct banks.
// Every word a step reads is written for every chunk.  The next chunk is loaded into registers before the current one is multiplied.
// Summation order.  Every output element is ONE accumulator chain over k = 0, 1, .. in steps of 4, padded with zero products up to
// the next multiple of 4 after 9 Ci (the chunks before the last hold 72 = 18 x 4 elements).  The chain depends on Ci alone: not on
// N, not on the grid, not on where the pixel lies in a tile.  No atomics.
// Above 256 input channels (the tap entry and the LPIPS stack alone: up to 512) the chain is segmented: it starts again at zero every
// 128 channels = 1152 elements, and the segment sums are added in ascending order, the first to zero.  One chain of 4608 fp32 terms
// measured 8.1 times the fp32 CPU convolution's error against float64 on random inputs (the rule of DESIGN.md section 8g allows 8);
// up to 256 channels the chain, and so every bit, is what it was.
#include <math.h>

#include <algorithm>

#include "conv_block.h"

namespace snerf {

typedef float cf4 __attribute__((ext_vector_type(4)));

constexpr int CB_TILE = 16;                   // output pixels per workgroup and dimension
constexpr int CB_CI = 8;                      // input channels per chunk
constexpr int CB_KC = CB_CI * 9;              // reduction elements per chunk
constexpr int CB_STEPS = CB_KC / 4;           // MFMA steps per chunk
constexpr int CB_HALO = CB_TILE + 2;
constexpr int CB_LW = 20;                     // row pitch of the input tile
constexpr int CB_PLANE = CB_HALO * CB_LW;
constexpr int CB_WP = CB_KC + 2;              // row pitch of the weight slice
constexpr int CB_THREADS = 256;
constexpr int CB_GRID_X = 1 << 16;             // (image, tile) pairs per grid row: 2^16 x 256 threads stays below HIP's 2^32 per dimension

struct ConvArgs {
    const float *x, *w, *scale, *shift;
    float *y_full, *y_pool;       // the un-pooled map [N,Co,H,W] and the pooled one [N,Co,Hp,Wp]; either may be null, not both
    int Ci, Co, H, W, Hp, Wp;     // Hp, Wp = H / 2, W / 2
    int tiles_x, tiles;           // 16 x 16 tiles per row and per image
    int64_t jobs;                 // N tiles
    int relu;
};

// A chunk travels global memory -> registers -> LDS, so that the next chunk's loads are in flight while this one multiplies.  The
// thread -> element maps keep every address one base plus a constant per load:
//   input tile   thread = (plane tid >> 5, column tid & 31 < 18), one load per halo row: 18 words, a row of 18 columns per plane coalesced
//   weight slice thread = (channel tid / TPR, part tid % TPR) with TPR = 16 / MT threads per channel, KPT = ceil(72 / TPR) consecutive k each
constexpr int CB_IN_REGS = CB_HALO;
template <int MT>
constexpr int CB_W_REGS = (CB_KC * MT + 15) / 16;

template <int MT>
__device__ __forceinline__ void conv_chunk_load(const ConvArgs &G, const float *xn, int c0, int y0, int x0, int co0, int tid,
                                                float (&rin)[CB_IN_REGS], float (&rw)[CB_W_REGS<MT>]) {
    const int cc = min(CB_CI, G.Ci - c0), kc = cc * 9;
    const int c = tid >> 5, xx = tid & 31, gx = x0 + xx - 1;
    const bool col = xx < CB_HALO && c < cc && gx >= 0 && gx < G.W;   // outside the image or past the last channel: zero
    const float *xp = xn + (int64_t)(c0 + c) * G.H * G.W + gx;
#pragma unroll
    for (int j = 0; j < CB_IN_REGS; ++j) {
        const int gy = y0 + j - 1;
        float v = 0.f;
        if (col && gy >= 0 && gy < G.H) v = xp[(int64_t)gy * G.W];
        rin[j] = v;
    }
    constexpr int TPR = 16 / MT, KPT = CB_W_REGS<MT>;
    const int co = tid / TPR, k0 = (tid % TPR) * KPT;
    const float *wp = G.w + (int64_t)(co0 + co) * (G.Ci * 9) + c0 * 9 + k0;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        float v = 0.f;
        if (co0 + co < G.Co && k0 + j < kc) v = wp[j];
        rw[j] = v;
    }
}
template <int MT>
__device__ __forceinline__ void conv_chunk_store(float *s_in, float *s_w, int tid, const float (&rin)[CB_IN_REGS], const float (&rw)[CB_W_REGS<MT>]) {
    const int c = tid >> 5, xx = tid & 31;
    if (xx < CB_HALO) {
#pragma unroll
        for (int j = 0; j < CB_IN_REGS; ++j) s_in[c * CB_PLANE + j * CB_LW + xx] = rin[j];
    }
    constexpr int TPR = 16 / MT, KPT = CB_W_REGS<MT>;
    const int co = tid / TPR, k0 = (tid % TPR) * KPT;
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if (k0 + j < CB_KC) s_w[co * CB_WP + k0 + j] = rw[j];
}

template <int MT, bool SEG>
__global__ __launch_bounds__(CB_THREADS) void conv3x3_block_kernel(ConvArgs G) {
    __shared__ float s_in[CB_CI * CB_PLANE];
    __shared__ float s_w[16 * MT * CB_WP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = lane & 15, kq = lane >> 4, py = p >> 2, px = p & 3, qy = wave >> 1, qx = wave & 1;
    // (image, pixel tile) = blockIdx.z 2^16 + blockIdx.x: up to 2^31 of them, which one grid dimension of 256-thread workgroups cannot hold
    const int64_t job = (int64_t)blockIdx.z * CB_GRID_X + blockIdx.x;
    if (job >= G.jobs) return;   // (the whole workgroup, before any barrier)
    const int64_t n = job / G.tiles;
    const int tile = (int)(job - n * G.tiles), ty = tile / G.tiles_x, tx = tile - ty * G.tiles_x;
    const int y0 = ty * CB_TILE, x0 = tx * CB_TILE, co0 = blockIdx.y * 16 * MT;
    // where reduction element 4 s + kq of a chunk lies in s_in, relative to the pixel it is applied at
    int koff[CB_STEPS];
#pragma unroll
    for (int s = 0; s < CB_STEPS; ++s) {
        const int k = 4 * s + kq, c = k / 9, r = k - 9 * c, ky = r / 3;
        koff[s] = c * CB_PLANE + ky * CB_LW + (r - 3 * ky);
    }
    cf4 acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[m][d] = cf4{0.f, 0.f, 0.f, 0.f};
    cf4 base[SEG ? MT : 1][4];   // SEG: the sum of the segments before this one
    if constexpr (SEG) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int d = 0; d < 4; ++d) base[m][d] = cf4{0.f, 0.f, 0.f, 0.f};
    }
    const float *xn = G.x + n * G.Ci * (int64_t)G.H * G.W;
    const float *pb = s_in + (qy * 8 + 2 * py) * CB_LW + qx * 8 + 2 * px;
    const float *pa = s_w + p * CB_WP + kq;
    float rin[CB_IN_REGS], rw[CB_W_REGS<MT>];
    conv_chunk_load<MT>(G, xn, 0, y0, x0, co0, tid, rin, rw);
    for (int c0 = 0; c0 < G.Ci; c0 += CB_CI) {
        const int steps = (min(CB_CI, G.Ci - c0) * 9 + 3) >> 2;
        __syncthreads();   // the previous chunk has been read
        conv_chunk_store<MT>(s_in, s_w, tid, rin, rw);
        __syncthreads();
        if (c0 + CB_CI < G.Ci) conv_chunk_load<MT>(G, xn, c0 + CB_CI, y0, x0, co0, tid, rin, rw);
        if constexpr (SEG) {
            if (c0 > 0 && c0 % CB_SEG_C == 0) {   // (uniform) a new segment: its chain starts at zero
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int d = 0; d < 4; ++d) base[m][d] = base[m][d] + acc[m][d], acc[m][d] = cf4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int s = 0; s < CB_STEPS; ++s) {
            if (s < steps) {   // (uniform: the last chunk of a Ci that is no multiple of 8 is shorter)
                const float *q = pb + koff[s];
                const float b00 = q[0], b01 = q[1], b10 = q[CB_LW], b11 = q[CB_LW + 1];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const float a = pa[m * 16 * CB_WP + 4 * s];
                    acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b00, acc[m][0], 0, 0, 0);
                    acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b01, acc[m][1], 0, 0, 0);
                    acc[m][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b10, acc[m][2], 0, 0, 0);
                    acc[m][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b11, acc[m][3], 0, 0, 0);
                }
            }
        }
    }
    if constexpr (SEG) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[m][d] = base[m][d] + acc[m][d];
    }
    // D layout: acc[m][2 dy + dx][r] = channel co0 + 16 m + 4 kq + r at pixel (y0 + 8 qy + 2 py + dy, x0 + 8 qx + 2 px + dx)
    const int oy = y0 + 8 * qy + 2 * py, ox = x0 + 8 * qx + 2 * px;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + 16 * m + 4 * kq + r;
            if (co >= G.Co) continue;
            const float sc = G.scale ? G.scale[co] : 1.f, sh = G.shift[co];   // (no scale: x 1 is exact, the bits of a vector of ones)
            float v[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                v[d] = __fadd_rn(__fmul_rn(acc[m][d][r], sc), sh);
                if (G.relu) v[d] = fmaxf(v[d], 0.f);
            }
            if (G.y_pool) {
                float *yc = G.y_pool + (n * G.Co + co) * (int64_t)G.Hp * G.Wp;
                if ((oy >> 1) < G.Hp && (ox >> 1) < G.Wp) yc[(int64_t)(oy >> 1) * G.Wp + (ox >> 1)] = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            }
            if (G.y_full) {   // the tap: the same four values, before the max
                float *yc = G.y_full + (n * G.Co + co) * (int64_t)G.H * G.W;
#pragma unroll
                for (int d = 0; d < 4; ++d)
                    if (oy + (d >> 1) < G.H && ox + (d & 1) < G.W) yc[(int64_t)(oy + (d >> 1)) * G.W + ox + (d & 1)] = v[d];
            }
        }
}

// BatchNorm (running statistics) and the convolution's bias as one scale and shift per channel, in float64, rounded once:
//   scale = gamma / sqrt(var + eps)      shift = beta + (b - mean) scale
struct FoldArgs {
    const float *bias[5], *gamma[5], *beta[5], *mean[5], *var[5];
    double eps[5];
    int channels[5], offset[5];
    float *scale, *shift;
};
__global__ __launch_bounds__(256) void estimator_fold_kernel(FoldArgs F) {
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < F.channels[b]; c += 256) {
        const double sc = (double)F.gamma[b][c] / sqrt((double)F.var[b][c] + F.eps[b]);
        F.scale[F.offset[b] + c] = (float)sc;
        F.shift[F.offset[b] + c] = (float)((double)F.beta[b][c] + ((double)F.bias[b][c] - (double)F.mean[b][c]) * sc);
    }
}

static bool below_2_31(int64_t a, int64_t b, int64_t c, int64_t d) {
    return (unsigned __int128)a * (unsigned __int128)b * (unsigned __int128)c * (unsigned __int128)d < ((unsigned __int128)1 << 31);
}

// the scalar checks of a block (an error whatever N is); *Ho, *Wo: the extents of y
int conv_check(const char *what, int64_t N, int Ci, int64_t H, int64_t W, int Co, int pool, int64_t *Ho, int64_t *Wo, int max_c) {
    if (Ci < 1 || Ci > max_c) return fail(SNERF_E_BADARG, "%s: Ci = %d is outside 1 .. %d", what, Ci, max_c);
    if (Co < 1 || Co > max_c) return fail(SNERF_E_BADARG, "%s: Co = %d is outside 1 .. %d", what, Co, max_c);
    if (N < 0) return fail(SNERF_E_BADARG, "%s: N = %lld is negative", what, (long long)N);
    const int64_t lo = pool ? 2 : 1;
    if (H < lo || H > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: H = %lld is outside %d .. 2^31 - 1%s", what, (long long)H, (int)lo, pool ? " (pooling)" : "");
    if (W < lo || W > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: W = %lld is outside %d .. 2^31 - 1%s", what, (long long)W, (int)lo, pool ? " (pooling)" : "");
    *Ho = pool ? H / 2 : H, *Wo = pool ? W / 2 : W;
    if (N > 0x7fffffffLL || !below_2_31(N, Ci, H, W) || !below_2_31(N, Co, H, W))
        return fail(SNERF_E_BADARG, "%s: N Ci H W or N Co H W = %lld x (%d | %d) x %lld x %lld reaches 2^31 elements", what, (long long)N, Ci, Co,
                    (long long)H, (long long)W);
    return SNERF_OK;
}

// one block on checked arguments, N > 0, to either or both of its outputs
int conv_launch_tap(const char *what, const float *x, int64_t N, int Ci, int H, int W, const float *w, const float *scale,
                    const float *shift, int Co, int relu, float *y_full, float *y_pool, hipStream_t s) {
    ConvArgs G{x, w, scale, shift, y_full, y_pool, Ci, Co, H, W, H / 2, W / 2, 0, 0, 0, relu ? 1 : 0};
    G.tiles_x = (W + CB_TILE - 1) / CB_TILE;
    G.tiles = G.tiles_x * ((H + CB_TILE - 1) / CB_TILE);
    G.jobs = N * G.tiles;                                        // (<= N H W < 2^31)
    // 16 MT channels per workgroup: the widest tile (the most reuse of an input tile) that still gives every CU two workgroups; the
    // chain of an output element is the same in all three, so the choice changes no bit
    const int n_cu = device_cu_count(what);
    if (n_cu < 1) return n_cu;
    int mt = Co <= 16 ? 1 : Co <= 32 ? 2 : 4;
    while (mt > 1 && G.jobs * ((Co + 16 * mt - 1) / (16 * mt)) < 2 * (int64_t)n_cu) mt >>= 1;
    const dim3 grid((unsigned)std::min<int64_t>(G.jobs, CB_GRID_X), (unsigned)((Co + 16 * mt - 1) / (16 * mt)),
                    (unsigned)((G.jobs + CB_GRID_X - 1) / CB_GRID_X));   // z <= 2^15
    if (Ci > CB_MAX_C) {   // the segmented chain
        if (mt == 1) hipLaunchKernelGGL((conv3x3_block_kernel<1, true>), grid, dim3(CB_THREADS), 0, s, G);
        else if (mt == 2) hipLaunchKernelGGL((conv3x3_block_kernel<2, true>), grid, dim3(CB_THREADS), 0, s, G);
        else hipLaunchKernelGGL((conv3x3_block_kernel<4, true>), grid, dim3(CB_THREADS), 0, s, G);
    } else if (mt == 1) hipLaunchKernelGGL((conv3x3_block_kernel<1, false>), grid, dim3(CB_THREADS), 0, s, G);
    else if (mt == 2) hipLaunchKernelGGL((conv3x3_block_kernel<2, false>), grid, dim3(CB_THREADS), 0, s, G);
    else hipLaunchKernelGGL((conv3x3_block_kernel<4, false>), grid, dim3(CB_THREADS), 0, s, G);
    return check_launch(what);
}
int conv_launch(const char *what, const float *x, int64_t N, int Ci, int H, int W, const float *w, const float *scale, const float *shift,
                int Co, int relu, int pool, float *y, hipStream_t s) {
    return conv_launch_tap(what, x, N, Ci, H, W, w, scale, shift, Co, relu, pool ? nullptr : y, pool ? y : nullptr, s);
}

// ---- the network: models/smpl_estimator.py:14-30 -------------------------------------------------------------------------------
constexpr int EST_CI[5] = {3, 16, 32, 64, 64}, EST_CO[5] = {16, 32, 64, 64, 128}, EST_POOL[5] = {0, 1, 1, 1, 1};
constexpr int EST_SIDE = 128, EST_FLAT = 8 * 8 * 128, EST_HIDDEN = 500;
constexpr int64_t EST_FOLD_FLOATS = 1024;                     // scale at [0, 512), shift at [512, 1024): 304 channels each
constexpr int64_t EST_A = 16 * 128 * 128, EST_B = 32 * 64 * 64;   // floats per image of the two activation buffers
constexpr int64_t EST_MAX_N = ((int64_t)1 << 31) / EST_A - 1;

}  // namespace snerf

extern "C" int snerf_conv3x3_block_f32(const float *x, int64_t N, int Ci, int64_t H, int64_t W, const float *w, const float *scale,
                                       const float *shift, int Co, int relu, int pool, float *y, snerf_stream_t stream) {
    using namespace snerf;
    int64_t Ho, Wo;
    if (int rc = conv_check("conv3x3_block", N, Ci, H, W, Co, pool, &Ho, &Wo)) return rc;
    if (N == 0) return SNERF_OK;
    if (!x || !w || !scale || !shift || !y)
        return fail(SNERF_E_BADARG, "conv3x3_block: null pointer (%s)", !x ? "x" : !w ? "w" : !scale ? "scale" : !shift ? "shift" : "y");
    return conv_launch("conv3x3_block", x, N, Ci, (int)H, (int)W, w, scale, shift, Co, relu, pool, y, (hipStream_t)stream);
}

extern "C" int snerf_conv3x3_block_tap_f32(const float *x, int64_t N, int Ci, int64_t H, int64_t W, const float *w, const float *scale,
                                           const float *shift, int Co, int relu, float *y_full, float *y_pool, snerf_stream_t stream) {
    using namespace snerf;
    int64_t Ho, Wo;
    if (int rc = conv_check("conv3x3_block_tap", N, Ci, H, W, Co, y_pool != nullptr, &Ho, &Wo, CB_TAP_MAX_C)) return rc;
    if (N == 0) return SNERF_OK;
    if (!y_full && !y_pool) return fail(SNERF_E_BADARG, "conv3x3_block_tap: y_full and y_pool are both null: one output at least");
    if (!x || !w || !scale || !shift)
        return fail(SNERF_E_BADARG, "conv3x3_block_tap: null pointer (%s)", !x ? "x" : !w ? "w" : !scale ? "scale" : "shift");
    return conv_launch_tap("conv3x3_block_tap", x, N, Ci, (int)H, (int)W, w, scale, shift, Co, relu, y_full, y_pool, (hipStream_t)stream);
}

extern "C" int64_t snerf_smpl_estimator_workspace_bytes(int64_t N, int human_size) {
    using namespace snerf;
    if (N < 0 || N > EST_MAX_N) return fail(SNERF_E_BADARG, "smpl_estimator_workspace_bytes: N = %lld is outside 0 .. %lld", (long long)N, (long long)EST_MAX_N);
    if (human_size < 1) return fail(SNERF_E_BADARG, "smpl_estimator_workspace_bytes: human_size = %d is below 1", human_size);
    return 4 * (EST_FOLD_FLOATS + N * (EST_A + EST_B));
}

extern "C" int snerf_smpl_estimator_fwd_f32(const snerf_smpl_estimator *net, const float *images, int64_t N, float *out, void *workspace,
                                            int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    if (!net) return fail(SNERF_E_BADARG, "smpl_estimator_fwd: null net");
    const int64_t need = snerf_smpl_estimator_workspace_bytes(N, net->human_size);
    if (need < 0) return SNERF_E_BADARG;
    for (int b = 0; b < 5; ++b)
        if (!(net->block[b].eps >= 0.0) || !isfinite(net->block[b].eps))
            return fail(SNERF_E_BADARG, "smpl_estimator_fwd: eps of bn%d = %g is negative or not finite", b + 1, net->block[b].eps);
    if (N == 0) return SNERF_OK;
    FoldArgs F;
    for (int b = 0, off = 0; b < 5; off += EST_CO[b], ++b) {
        const snerf_conv_bn &c = net->block[b];
        if (!c.weight || !c.bias || !c.bn_weight || !c.bn_bias || !c.running_mean || !c.running_var)
            return fail(SNERF_E_BADARG, "smpl_estimator_fwd: null pointer in block %d", b + 1);
        F.bias[b] = c.bias, F.gamma[b] = c.bn_weight, F.beta[b] = c.bn_bias, F.mean[b] = c.running_mean, F.var[b] = c.running_var;
        F.eps[b] = c.eps, F.channels[b] = EST_CO[b], F.offset[b] = off;
    }
    if (!net->fc1_weight || !net->fc1_bias || !net->fc2_weight || !net->fc2_bias) return fail(SNERF_E_BADARG, "smpl_estimator_fwd: null pointer in fc1 / fc2");
    if (!images || !out) return fail(SNERF_E_BADARG, "smpl_estimator_fwd: null pointer (%s)", !images ? "images" : "out");
    if (!workspace || workspace_bytes < need)
        return fail(SNERF_E_BADARG, "smpl_estimator_fwd: workspace of %lld bytes, need %lld", (long long)(workspace ? workspace_bytes : 0), (long long)need);
    if (!aligned(workspace, 16)) return fail(SNERF_E_ALIGN, "smpl_estimator_fwd: workspace %p is not 16-byte aligned", workspace);
    hipStream_t s = (hipStream_t)stream;
    float *fold = static_cast<float *>(workspace), *buf[2] = {fold + EST_FOLD_FLOATS, fold + EST_FOLD_FLOATS + N * EST_A};
    F.scale = fold, F.shift = fold + EST_FOLD_FLOATS / 2;
    hipLaunchKernelGGL(estimator_fold_kernel, dim3(5), dim3(256), 0, s, F);
    if (int rc = check_launch("smpl_estimator_fwd(fold)")) return rc;
    const float *in = images;
    int side = EST_SIDE;
    for (int b = 0; b < 5; ++b) {   // block b writes buf[b & 1]; block 5 leaves [N, 128, 8, 8] = the rows of view(-1, 8 * 8 * 128) in buf[0]
        if (int rc = conv_launch("smpl_estimator_fwd(conv)", in, N, EST_CI[b], side, side, net->block[b].weight, F.scale + F.offset[b],
                                 F.shift + F.offset[b], EST_CO[b], 1, EST_POOL[b], buf[b & 1], s))
            return rc;
        in = buf[b & 1];
        if (EST_POOL[b]) side /= 2;
    }
    if (int rc = snerf_linear_fwd_f32(buf[0], N, EST_FLAT, EST_FLAT, net->fc1_weight, EST_FLAT, EST_HIDDEN, net->fc1_bias, 0, 1, buf[1], EST_HIDDEN, stream))
        return rc;
    return snerf_linear_fwd_f32(buf[1], N, EST_HIDDEN, EST_HIDDEN, net->fc2_weight, EST_HIDDEN, net->human_size, net->fc2_bias, 0, 0, out,
                                net->human_size, stream);
}
