// LPIPS (util/scores.py:286-456: ContentLoss with normalize_features, as LPIPS() configures it) on a VGG16-shaped feature stack:
// the distance between two feature maps, and the whole metric as one call; then its backward to both frames (ContentLoss is a _Loss
// with frozen weights): the distance gradient, the ReLU / max-pool backward, and the walk of a chunk forward and back - in the second
// half of this file.  The convolutions are csrc/conv_block.hip's.
//
// Distance of two maps fx, fy [N,C,h,w] with channel weights wl [C], per image n:
//   out[n] = (1 / (h w)) sum_p sum_c wl[c] (x^[c,p] - y^[c,p])^2        x^[c,p] = fx[c,p] / (sqrt(sum_c fx[c,p]^2) + 1e-10)
// (scores.py:372, :403-411; without `normalize` x^ = fx).  The rule, operation by operation, per pixel p:
//   s   = the sum over c = 0, 1, .. of fx[c,p]^2 in float64 (the products are exact there), rounded to fp32 once
//   nx  = sqrt(s) + 1e-10f                      fp32, IEEE square root, then the addition              (ny from fy alike)
//   a   = fx[c,p] / nx,  b = fy[c,p] / ny       fp32, IEEE divisions                                  (a = fx, b = fy without normalize)
//   d   = a - b,  t = d d                       fp32
//   acc = the sum over c = 0, 1, .. of (double)wl[c] (double)t in float64, one fma per channel
// The difference form: fx == fy gives d = 0 and out = 0 exactly; a pixel whose features are all zero has nx = 1e-10, a = 0.
// Pixels: a tile is 64 consecutive pixels of the flattened h w map, one per lane (coalesced along w); the tile's sum goes through
// the wave's DPP scan in float64 to workspace[n][tile]; a second launch adds an image's tiles in a fixed order (lane l takes tiles
// l, l + 64, ..., then the scan), divides by h w in float64 and rounds to fp32 once.
//
// Mapping.  Workgroup = one wave = one tile of one image.  Two passes over c: the norms, then the differences; a tile's working set is
// 64 pixels x C channels x 2 maps (256 KB at C = 512), so the second pass is served by the L2.  Nothing of map size is stored, no
// atomics, no LDS; an image's value depends on its own pixels alone, and two calls give the same bits.
#include <math.h>

#include <algorithm>

#include "conv_block.h"

namespace snerf {

constexpr int FD_TILE = WAVE;                       // pixels per workgroup
constexpr float LPIPS_EPS = 1e-10f;                 // scores.py:179
constexpr int LPIPS_MIN_SIDE = 16;                  // four pools leave the fifth stage one pixel at least
constexpr int VGG_CONVS[5] = {2, 2, 3, 3, 3};

struct DistArgs {
    const float *fx, *fy, *wl;
    int C, hw, tiles, normalize;
    double *part;   // [N][tiles]
};

__global__ __launch_bounds__(FD_TILE) void feature_distance_kernel(DistArgs A) {
    const int tile = blockIdx.x, n = blockIdx.y, p = tile * FD_TILE + (int)threadIdx.x;
    const bool in = p < A.hw;
    const int64_t base = (int64_t)n * A.C * A.hw + (in ? p : 0);
    const float *x = A.fx + base, *y = A.fy + base;
    float nx = 1.f, ny = 1.f;
    if (A.normalize) {
        double sx = 0.0, sy = 0.0;
#pragma unroll 4
        for (int c = 0; c < A.C; ++c) {
            const double a = (double)x[(int64_t)c * A.hw], b = (double)y[(int64_t)c * A.hw];
            sx = fma(a, a, sx), sy = fma(b, b, sy);
        }
        nx = __fadd_rn(__fsqrt_rn((float)sx), LPIPS_EPS), ny = __fadd_rn(__fsqrt_rn((float)sy), LPIPS_EPS);
    }
    double acc = 0.0;
#pragma unroll 4
    for (int c = 0; c < A.C; ++c) {
        float a = x[(int64_t)c * A.hw], b = y[(int64_t)c * A.hw];
        if (A.normalize) a = __fdiv_rn(a, nx), b = __fdiv_rn(b, ny);
        const float d = __fsub_rn(a, b), t = __fmul_rn(d, d);
        acc = fma((double)A.wl[c], (double)t, acc);
    }
    const double sum = wave_sum(in ? acc : 0.0);
    if (threadIdx.x == 0) A.part[(int64_t)n * A.tiles + tile] = sum;
}

// one wave per image: out[n out_stride] = the sum of its tiles / (h w); with `total`, total[n] = the ascending fp32 sum of the
// n_total values out[n out_stride - (n_total - 1)] .. out[n out_stride] (the stage distances of one image: the last of them is this one)
__global__ __launch_bounds__(WAVE) void feature_distance_reduce_kernel(const double *part, int tiles, double pixels, float *out,
                                                                        int out_stride, float *total, int n_total) {
    const int lane = threadIdx.x, n = blockIdx.x;
    const double *p = part + (int64_t)n * tiles;
    double s = 0.0;
    for (int t = lane; t < tiles; t += WAVE) s += p[t];
    s = wave_sum(s);
    if (lane != 0) return;
    const float v = (float)(s / pixels);
    float *o = out + (int64_t)n * out_stride;
    *o = v;
    if (total) {
        float sum = n_total > 1 ? o[1 - n_total] : v;
        for (int l = 2 - n_total; l < 0; ++l) sum = __fadd_rn(sum, o[l]);
        if (n_total > 1) sum = __fadd_rn(sum, v);
        total[n] = sum;
    }
}

static int64_t dist_tiles(int64_t h, int64_t w) { return (h * w + FD_TILE - 1) / FD_TILE; }

static int dist_check(const char *op, int64_t N, int64_t C, int64_t h, int64_t w) {
    if (N < 0) return fail(SNERF_E_BADARG, "%s: N = %lld is negative", op, (long long)N);
    if (C < 1 || C > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: C = %lld is outside 1 .. 2^31 - 1", op, (long long)C);
    if (h < 1 || h > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: h = %lld is outside 1 .. 2^31 - 1", op, (long long)h);
    if (w < 1 || w > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: w = %lld is outside 1 .. 2^31 - 1", op, (long long)w);
    if (N > 65535) return fail(SNERF_E_BADARG, "%s: N = %lld is above 65535 images a call", op, (long long)N);
    if ((unsigned __int128)std::max<int64_t>(N, 1) * (unsigned __int128)C * (unsigned __int128)h * (unsigned __int128)w >= ((unsigned __int128)1 << 31))
        return fail(SNERF_E_BADARG, "%s: N C h w = %lld x %lld x %lld x %lld reaches 2^31 elements", op, (long long)N, (long long)C, (long long)h,
                    (long long)w);
    return SNERF_OK;
}

// the two launches on checked arguments, N > 0: out[n out_stride], n < N
static int dist_launch(const char *op, const float *fx, const float *fy, int N, int C, int h, int w, const float *wl, int normalize,
                       float *out, int out_stride, float *total, int n_total, double *part, hipStream_t s) {
    const int tiles = (int)dist_tiles(h, w);
    DistArgs A{fx, fy, wl, C, h * w, tiles, normalize ? 1 : 0, part};
    hipLaunchKernelGGL(feature_distance_kernel, dim3((unsigned)tiles, (unsigned)N), dim3(FD_TILE), 0, s, A);
    hipLaunchKernelGGL(feature_distance_reduce_kernel, dim3((unsigned)N), dim3(WAVE), 0, s, (const double *)part, tiles,
                       (double)h * (double)w, out, out_stride, total, n_total);
    return check_launch(op);
}

// (v - mean[c]) / std[c] (scores.py:394: a subtraction, then a division) of m frames of x and m frames of y, read through the
// element strides, into one contiguous batch [2 m,3,H,W]: x's frames first
struct NormArgs {
    const float *x, *y;
    int64_t sn, sc, sh, sw;
    int m, H, W;
    float mean[3], std[3];
    float *out;
};
__global__ __launch_bounds__(256) void lpips_normalize_kernel(NormArgs A) {
    const int hw = A.H * A.W, p = blockIdx.x * 256 + (int)threadIdx.x, c = blockIdx.y, i = blockIdx.z;
    if (p >= hw) return;
    const int h = p / A.W, w = p - h * A.W;
    const float *src = i < A.m ? A.x + (int64_t)i * A.sn : A.y + (int64_t)(i - A.m) * A.sn;
    const float v = src[(int64_t)c * A.sc + (int64_t)h * A.sh + (int64_t)w * A.sw];
    A.out[((int64_t)i * 3 + c) * hw + p] = __fdiv_rn(__fsub_rn(v, A.mean[c]), A.std[c]);
}

// floats and partial sums one image pair needs: two activation buffers of F floats, one of P (the normalised input, the pooled maps)
struct LpipsPlan {
    int64_t F, P, tiles, bytes;   // per pair
    int64_t max_pairs;            // pairs a chunk may hold: 2 m (widest layer) H W stays below 2^31
};
static int lpips_plan(const char *op, int64_t H, int64_t W, const int32_t *channels, LpipsPlan &L) {
    if (!channels) return fail(SNERF_E_BADARG, "%s: channels is null", op);
    for (int l = 0; l < 5; ++l)
        if (channels[l] < 1 || channels[l] > CB_TAP_MAX_C)
            return fail(SNERF_E_BADARG, "%s: channels[%d] = %d is outside 1 .. %d", op, l, channels[l], CB_TAP_MAX_C);
    if (H < LPIPS_MIN_SIDE || H > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: H = %lld is outside %d .. 2^31 - 1", op, (long long)H, LPIPS_MIN_SIDE);
    if (W < LPIPS_MIN_SIDE || W > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: W = %lld is outside %d .. 2^31 - 1", op, (long long)W, LPIPS_MIN_SIDE);
    unsigned __int128 F = 0, P = (unsigned __int128)6 * H * W;
    int64_t h = H, w = W, cmax = 3;
    for (int l = 0; l < 5; ++l, h /= 2, w /= 2) {
        F = std::max(F, (unsigned __int128)2 * channels[l] * h * w);
        if (l < 4) P = std::max(P, (unsigned __int128)2 * channels[l] * (h / 2) * (w / 2));
        cmax = std::max<int64_t>(cmax, channels[l]);
    }
    const unsigned __int128 per_image = (unsigned __int128)cmax * H * W;
    if (2 * per_image >= ((unsigned __int128)1 << 31))
        return fail(SNERF_E_BADARG, "%s: 2 x %lld channels x H W = %lld x %lld reaches 2^31 elements", op, (long long)cmax, (long long)H, (long long)W);
    L.F = (int64_t)F, L.P = (int64_t)P, L.tiles = dist_tiles(H, W);
    L.bytes = (4 * (2 * L.F + L.P) + 8 * L.tiles + 15) / 16 * 16;
    L.max_pairs = std::min<int64_t>((int64_t)((((unsigned __int128)1 << 31) - 1) / (2 * per_image)), 32767);
    return SNERF_OK;
}

// the checks both entries share, after the plan's: the scalars of the net (an error whatever N is), then with N > 0 its pointers
static int lpips_check_scalars(const char *op, const snerf_vgg_lpips *net, int64_t N) {
    for (int c = 0; c < 3; ++c) {
        if (!isfinite(net->std[c]) || net->std[c] == 0.f) return fail(SNERF_E_BADARG, "%s: std[%d] = %g is zero or not finite", op, c, (double)net->std[c]);
        if (!isfinite(net->mean[c])) return fail(SNERF_E_BADARG, "%s: mean[%d] = %g is not finite", op, c, (double)net->mean[c]);
    }
    if (N < 0) return fail(SNERF_E_BADARG, "%s: N = %lld is negative", op, (long long)N);
    return SNERF_OK;
}
static int lpips_check_net(const char *op, const snerf_vgg_lpips *net) {
    for (int i = 0; i < 13; ++i)
        if (!net->conv[i].weight || !net->conv[i].bias) return fail(SNERF_E_BADARG, "%s: null pointer in convolution %d", op, i + 1);
    for (int l = 0; l < 5; ++l)
        if (!net->lin[l]) return fail(SNERF_E_BADARG, "%s: null pointer (lin[%d])", op, l);
    return SNERF_OK;
}

// ---- the backward: LPIPS as a training loss ---------------------------------------------------------------------------------------
// The gradient of sum_n g[n] out[n] of the distance above to fx and to fy.  Per pixel p, with the forward's own fp32 s, r = sqrt(s),
// nx = r + 1e-10f, a = fx / nx, b = fy / ny, d = a - b, and everything after them in float64:
//   gs  = (double)g[n] / (h w)                           q[c] = ((2 wl[c]) d[c]) gs
//   Dx  = the sum over c = 0, 1, .. of q[c] a[c], one fma per channel             (Dy with b)
//   dfx[k] = (q[k] - fx[k] (Dx / r)) / nx                dfy[k] = -(q[k] - fy[k] (Dy / ry)) / ny          each rounded to fp32 once
// (a = fx / nx has da[c]/dfx[k] = [c == k] / nx - fx[c] fx[k] / (nx^2 r).)  Where r = 0 - a pixel whose features are all zero, where
// autograd's 0 / 0 is NaN - the norm term is taken as 0: dfx[k] = q[k] / nx.  Without normalize dfx = q, dfy = -q.  d = 0 gives +0.
// Mapping: lane = pixel, one wave per 64-pixel tile as the forward; three passes over c (the norms, the two dot products, the
// outputs), the first from HBM, the others from the L2; nothing of map size is stored besides the outputs; no reduction across
// lanes, so a pixel's gradient depends on its own features and g[n] alone.
struct DistBwdArgs {
    const float *fx, *fy, *wl, *g;
    float *dfx, *dfy;   // either may be null, not both
    int C, hw, normalize, g_stride;
    double pixels;
};

__global__ __launch_bounds__(FD_TILE) void feature_distance_bwd_kernel(DistBwdArgs A) {
    const int n = blockIdx.y, p = blockIdx.x * FD_TILE + (int)threadIdx.x;
    if (p >= A.hw) return;
    const int64_t base = (int64_t)n * A.C * A.hw + p;
    const float *x = A.fx + base, *y = A.fy + base;
    float *ox = A.dfx ? A.dfx + base : nullptr, *oy = A.dfy ? A.dfy + base : nullptr;
    const double gs = (double)A.g[(int64_t)n * A.g_stride] / A.pixels;
    if (!A.normalize) {
#pragma unroll 4
        for (int c = 0; c < A.C; ++c) {
            const float d = __fsub_rn(x[(int64_t)c * A.hw], y[(int64_t)c * A.hw]);
            const double q = 2.0 * (double)A.wl[c] * (double)d * gs;
            if (ox) ox[(int64_t)c * A.hw] = (float)(q + 0.0);
            if (oy) oy[(int64_t)c * A.hw] = (float)(0.0 - q);
        }
        return;
    }
    double sx = 0.0, sy = 0.0;
#pragma unroll 4
    for (int c = 0; c < A.C; ++c) {
        const double a = (double)x[(int64_t)c * A.hw], b = (double)y[(int64_t)c * A.hw];
        sx = fma(a, a, sx), sy = fma(b, b, sy);
    }
    const float rx = __fsqrt_rn((float)sx), ry = __fsqrt_rn((float)sy);
    const float nx = __fadd_rn(rx, LPIPS_EPS), ny = __fadd_rn(ry, LPIPS_EPS);
    double Dx = 0.0, Dy = 0.0;
#pragma unroll 4
    for (int c = 0; c < A.C; ++c) {
        const float a = __fdiv_rn(x[(int64_t)c * A.hw], nx), b = __fdiv_rn(y[(int64_t)c * A.hw], ny);
        const double q = 2.0 * (double)A.wl[c] * (double)__fsub_rn(a, b) * gs;
        Dx = fma(q, (double)a, Dx), Dy = fma(q, (double)b, Dy);
    }
    // (r = 0: the norm term is taken as 0)
    const double ux = rx > 0.f ? Dx / (double)rx : 0.0, uy = ry > 0.f ? Dy / (double)ry : 0.0;
#pragma unroll 4
    for (int c = 0; c < A.C; ++c) {
        const float xc = x[(int64_t)c * A.hw], yc = y[(int64_t)c * A.hw];
        const double q = 2.0 * (double)A.wl[c] * (double)__fsub_rn(__fdiv_rn(xc, nx), __fdiv_rn(yc, ny)) * gs;
        if (ox) ox[(int64_t)c * A.hw] = (float)((q - (double)xc * ux) / (double)nx + 0.0);
        if (oy) oy[(int64_t)c * A.hw] = (float)(0.0 - (q - (double)yc * uy) / (double)ny);
    }
}

static int dist_bwd_launch(const char *op, const float *fx, const float *fy, int N, int C, int h, int w, const float *wl, int normalize,
                           const float *g, int g_stride, float *dfx, float *dfy, hipStream_t s) {
    DistBwdArgs A{fx, fy, wl, g, dfx, dfy, C, h * w, normalize ? 1 : 0, g_stride, (double)h * (double)w};
    hipLaunchKernelGGL(feature_distance_bwd_kernel, dim3((unsigned)dist_tiles(h, w), (unsigned)N), dim3(FD_TILE), 0, s, A);
    return check_launch(op);
}

// dz = (y > 0) ? dy_full + route(dy_pool) : 0 on the post-ReLU map y [N,C,H,W]: the ReLU and the 2 x 2 max-pool that may follow it,
// without BatchNorm.  route sends a window's gradient to its FIRST maximum in the order (0,0), (0,1), (1,0), (1,1), recomputed from y
// (csrc/conv_train.hip's rule, torch's `val > maxval` scan); a pixel in no window (an odd extent) gets 0 from it.  One fp32 addition
// per pixel, the routed term being 0 away from the maximum.  One thread per 2 x 2 cell of the ceil(H / 2) x ceil(W / 2) cells that
// cover the map: it reads its own four dy_full before it writes its four dz, so dz may be dy_full.
struct ReluPoolBwdArgs {
    const float *y, *dy_full, *dy_pool;   // either gradient may be null, not both
    float *dz;
    int H, W, Hp, Wp, Hc, Wc;
};
__global__ __launch_bounds__(256) void relu_pool_bwd_kernel(ReluPoolBwdArgs A, unsigned total) {
    const unsigned at = blockIdx.x * 256u + threadIdx.x;
    if (at >= total) return;
    const unsigned Qc = (unsigned)(A.Hc * A.Wc), nc = at / Qc, q = at - nc * Qc;
    const int cy = (int)(q / (unsigned)A.Wc), cx = (int)(q - (unsigned)cy * (unsigned)A.Wc);
    const int64_t plane = (int64_t)nc * A.H * A.W;
    float v[4], full[4];
    bool in[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int py = 2 * cy + (d >> 1), px = 2 * cx + (d & 1);
        in[d] = py < A.H && px < A.W;
        const int64_t o = plane + (int64_t)py * A.W + px;
        v[d] = in[d] ? A.y[o] : 0.f;
        full[d] = in[d] && A.dy_full ? A.dy_full[o] : 0.f;
    }
    int winner = -1;
    float g = 0.f;
    if (A.dy_pool && cy < A.Hp && cx < A.Wp) {   // a window: all four pixels lie in the map
        float best = v[0];
        winner = 0;
#pragma unroll
        for (int d = 1; d < 4; ++d)
            if (v[d] > best) best = v[d], winner = d;
        g = A.dy_pool[(int64_t)nc * A.Hp * A.Wp + (int64_t)cy * A.Wp + cx];
    }
#pragma unroll
    for (int d = 0; d < 4; ++d)
        if (in[d])
            A.dz[plane + (int64_t)(2 * cy + (d >> 1)) * A.W + 2 * cx + (d & 1)] = v[d] > 0.f ? __fadd_rn(full[d], d == winner ? g : 0.f) : 0.f;
}

static int relu_pool_check(const char *op, int64_t N, int64_t C, int64_t H, int64_t W, bool pool) {
    if (N < 0) return fail(SNERF_E_BADARG, "%s: N = %lld is negative", op, (long long)N);
    if (C < 1 || C > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: C = %lld is outside 1 .. 2^31 - 1", op, (long long)C);
    const int lo = pool ? 2 : 1;
    if (H < lo || H > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: H = %lld is outside %d .. 2^31 - 1%s", op, (long long)H, lo, pool ? " (dy_pool)" : "");
    if (W < lo || W > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: W = %lld is outside %d .. 2^31 - 1%s", op, (long long)W, lo, pool ? " (dy_pool)" : "");
    if (N > 0x7fffffffLL || (unsigned __int128)std::max<int64_t>(N, 1) * (unsigned __int128)C * (unsigned __int128)H * (unsigned __int128)W >= ((unsigned __int128)1 << 31))
        return fail(SNERF_E_BADARG, "%s: N C H W = %lld x %lld x %lld x %lld reaches 2^31 elements", op, (long long)N, (long long)C, (long long)H,
                    (long long)W);
    return SNERF_OK;
}

static int relu_pool_bwd_launch(const char *op, const float *y, const float *dy_full, const float *dy_pool, int64_t N, int C, int H, int W,
                                float *dz, hipStream_t s) {
    ReluPoolBwdArgs A{y, dy_full, dy_pool, dz, H, W, H / 2, W / 2, (H + 1) / 2, (W + 1) / 2};
    const int64_t total = N * C * A.Hc * A.Wc;   // (<= N C H W < 2^31)
    hipLaunchKernelGGL(relu_pool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, A, (unsigned)total);
    return check_launch(op);
}

// w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx]: the input gradient of a convolution is the forward kernel on w' (csrc/conv_train.hip's
// rule); zeros [Ci] is that launch's shift
__global__ __launch_bounds__(256) void lpips_flip_kernel(const float *w, int Ci, int Co, float *wt, float *zeros) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Ci) zeros[i] = 0.f;
    if (i >= Ci * Co * 9) return;
    const int r = i % 9, co = (i / 9) % Co, ci = i / (9 * Co);
    wt[i] = w[((int64_t)co * Ci + ci) * 9 + 8 - r];
}

// the backward of lpips_normalize_kernel: g [images,3,H,W] / std[c], a division, written through the element strides; with both
// outputs the first m images are dx's, the next m dy's
struct UnnormArgs {
    const float *g;
    float *dx, *dy;
    int64_t sn, sc, sh, sw;
    int m, H, W;
    float std[3];
};
__global__ __launch_bounds__(256) void lpips_unnormalize_kernel(UnnormArgs A) {
    const int hw = A.H * A.W, p = blockIdx.x * 256 + (int)threadIdx.x, c = blockIdx.y, i = blockIdx.z;
    if (p >= hw) return;
    const int h = p / A.W, w = p - h * A.W;
    float *dst = A.dx && i < A.m ? A.dx + (int64_t)i * A.sn : A.dy + (int64_t)(A.dx ? i - A.m : i) * A.sn;
    dst[(int64_t)c * A.sc + (int64_t)h * A.sh + (int64_t)w * A.sw] = __fdiv_rn(A.g[((int64_t)i * 3 + c) * hw + p], A.std[c]);
}

// floats a pair needs on top of LpipsPlan: the thirteen post-ReLU maps of both frames (K) and two gradient buffers of G floats, which
// in the forward walk hold the standardised input and the pooled maps; once a call: the flipped weights of the widest convolution
// and a shift of zeros
struct LpipsBwdPlan {
    LpipsPlan L;
    int64_t K, G, fixed_bytes, pair_bytes;
};
static int lpips_bwd_plan(const char *op, int64_t H, int64_t W, const int32_t *channels, LpipsBwdPlan &B) {
    if (int rc = lpips_plan(op, H, W, channels, B.L)) return rc;
    int64_t h = H, w = W, ci = 3, wt = 0;
    B.K = 0;
    for (int l = 0; l < 5; ++l, h /= 2, w /= 2) {
        B.K += (int64_t)VGG_CONVS[l] * 2 * channels[l] * h * w;
        wt = std::max<int64_t>(wt, std::max<int64_t>(ci, channels[l]) * channels[l] * 9);
        ci = channels[l];
    }
    B.G = std::max<int64_t>(B.L.F, 6 * H * W);
    B.fixed_bytes = (4 * (wt + CB_TAP_MAX_C) + 15) / 16 * 16;
    B.pair_bytes = (4 * (B.K + 2 * B.G) + 8 * B.L.tiles + 15) / 16 * 16;
    return SNERF_OK;
}

}  // namespace snerf

extern "C" int64_t snerf_feature_distance_workspace_bytes(int64_t N, int64_t h, int64_t w) {
    using namespace snerf;
    if (dist_check("feature_distance_workspace_bytes", N, 1, h, w)) return -1;
    return N * dist_tiles(h, w) * (int64_t)sizeof(double);
}

extern "C" int snerf_feature_distance_f32(const float *fx, const float *fy, int64_t N, int64_t C, int64_t h, int64_t w, const float *wl,
                                          int normalize, float *out, void *workspace, int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    if (int rc = dist_check("feature_distance", N, C, h, w)) return rc;
    if (N == 0) return SNERF_OK;
    if (!fx || !fy || !wl || !out)
        return fail(SNERF_E_BADARG, "feature_distance: null pointer (%s)", !fx ? "fx" : !fy ? "fy" : !wl ? "wl" : "out");
    const int64_t need = N * dist_tiles(h, w) * (int64_t)sizeof(double);
    if (!workspace || workspace_bytes < need)
        return fail(SNERF_E_BADARG, "feature_distance: workspace of %lld bytes, need %lld", (long long)(workspace ? workspace_bytes : 0), (long long)need);
    if (!aligned(workspace, 8)) return fail(SNERF_E_ALIGN, "feature_distance: workspace %p is not 8-byte aligned", workspace);
    return dist_launch("feature_distance", fx, fy, (int)N, (int)C, (int)h, (int)w, wl, normalize, out, 1, nullptr, 0, (double *)workspace,
                       (hipStream_t)stream);
}

extern "C" int64_t snerf_lpips_workspace_bytes(int64_t n_pairs, int64_t H, int64_t W, const int32_t *channels) {
    using namespace snerf;
    LpipsPlan L;
    if (n_pairs < 0) return fail(SNERF_E_BADARG, "lpips_workspace_bytes: n_pairs = %lld is negative", (long long)n_pairs);
    if (lpips_plan("lpips_workspace_bytes", H, W, channels, L)) return -1;
    if (n_pairs > 0x7fffffffffffffffLL / L.bytes) return fail(SNERF_E_BADARG, "lpips_workspace_bytes: n_pairs = %lld overflows", (long long)n_pairs);
    return n_pairs * L.bytes;
}

extern "C" int snerf_lpips_fwd_f32(const snerf_vgg_lpips *net, const float *x, const float *y, int64_t N, int64_t H, int64_t W, int64_t sn,
                                   int64_t sc, int64_t sh, int64_t sw, float *layers, float *total, void *workspace, int64_t workspace_bytes,
                                   snerf_stream_t stream) {
    using namespace snerf;
    if (!net) return fail(SNERF_E_BADARG, "lpips_fwd: null net");
    LpipsPlan L;
    if (int rc = lpips_plan("lpips_fwd", H, W, net->channels, L)) return rc;
    if (int rc = lpips_check_scalars("lpips_fwd", net, N)) return rc;
    if (N == 0) return SNERF_OK;
    if (int rc = lpips_check_net("lpips_fwd", net)) return rc;
    if (!x || !y || !layers) return fail(SNERF_E_BADARG, "lpips_fwd: null pointer (%s)", !x ? "x" : !y ? "y" : "layers");
    if (!workspace || workspace_bytes < L.bytes)
        return fail(SNERF_E_BADARG, "lpips_fwd: workspace of %lld bytes, need %lld for one image pair", (long long)(workspace ? workspace_bytes : 0),
                    (long long)L.bytes);
    if (!aligned(workspace, 16)) return fail(SNERF_E_ALIGN, "lpips_fwd: workspace %p is not 16-byte aligned", workspace);
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunk = std::min(std::min(N, workspace_bytes / L.bytes), L.max_pairs);
    // the chunk's buffers: stage l runs P -> A -> B [-> A], its last convolution writing the tap and, pooled, the next stage's input to P
    float *A = static_cast<float *>(workspace), *B = A + chunk * L.F, *P = B + chunk * L.F;
    double *part = reinterpret_cast<double *>(P + chunk * L.P);   // (8-byte aligned: F and P are even)
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int m = (int)std::min(chunk, N - n0);
        NormArgs Z{x + n0 * sn, y + n0 * sn, sn, sc, sh, sw, m, (int)H, (int)W, {net->mean[0], net->mean[1], net->mean[2]},
                   {net->std[0], net->std[1], net->std[2]}, P};
        hipLaunchKernelGGL(lpips_normalize_kernel, dim3((unsigned)((H * W + 255) / 256), 3, (unsigned)(2 * m)), dim3(256), 0, s, Z);
        if (int rc = check_launch("lpips_fwd(normalize)")) return rc;
        const float *in = P;
        int h = (int)H, w = (int)W, ci = 3, conv = 0;
        for (int l = 0; l < 5; ++l, h /= 2, w /= 2) {
            const int co = net->channels[l];
            float *bufs[2] = {A, B};
            for (int j = 0; j < VGG_CONVS[l]; ++j, ++conv) {
                const bool last = j == VGG_CONVS[l] - 1;
                float *full = bufs[j & 1];   // (the last convolution's `full` is the tap)
                if (int rc = conv_launch_tap("lpips_fwd(conv)", in, 2 * m, ci, h, w, net->conv[conv].weight, nullptr /* scale = 1 */, net->conv[conv].bias, co, 1,
                                             full, last && l < 4 ? P : nullptr, s))
                    return rc;
                in = full, ci = co;
            }
            const int64_t map = (int64_t)co * h * w;
            if (int rc = dist_launch("lpips_fwd(distance)", in, in + m * map, m, co, h, w, net->lin[l], 1, layers + n0 * 5 + l, 5,
                                     l == 4 && total ? total + n0 : nullptr, 5, part, s))
                return rc;
            in = P;
        }
    }
    return SNERF_OK;
}

extern "C" int snerf_feature_distance_bwd_f32(const float *fx, const float *fy, int64_t N, int64_t C, int64_t h, int64_t w, const float *wl,
                                              int normalize, const float *g, float *dfx, float *dfy, snerf_stream_t stream) {
    using namespace snerf;
    if (int rc = dist_check("feature_distance_bwd", N, C, h, w)) return rc;
    if (N == 0) return SNERF_OK;
    if (!dfx && !dfy) return fail(SNERF_E_BADARG, "feature_distance_bwd: dfx and dfy are both null: one output at least");
    if (!fx || !fy || !wl || !g) return fail(SNERF_E_BADARG, "feature_distance_bwd: null pointer (%s)", !fx ? "fx" : !fy ? "fy" : !wl ? "wl" : "g");
    return dist_bwd_launch("feature_distance_bwd", fx, fy, (int)N, (int)C, (int)h, (int)w, wl, normalize, g, 1, dfx, dfy, (hipStream_t)stream);
}

extern "C" int snerf_relu_pool_bwd_f32(const float *y, const float *dy_full, const float *dy_pool, int64_t N, int64_t C, int64_t H, int64_t W,
                                       float *dz, snerf_stream_t stream) {
    using namespace snerf;
    if (int rc = relu_pool_check("relu_pool_bwd", N, C, H, W, dy_pool != nullptr)) return rc;
    if (N == 0) return SNERF_OK;
    if (!dy_full && !dy_pool) return fail(SNERF_E_BADARG, "relu_pool_bwd: dy_full and dy_pool are both null: one gradient at least");
    if (!y || !dz) return fail(SNERF_E_BADARG, "relu_pool_bwd: null pointer (%s)", !y ? "y" : "dz");
    return relu_pool_bwd_launch("relu_pool_bwd", y, dy_full, dy_pool, N, (int)C, (int)H, (int)W, dz, (hipStream_t)stream);
}

extern "C" int64_t snerf_lpips_bwd_workspace_bytes(int64_t n_pairs, int64_t H, int64_t W, const int32_t *channels) {
    using namespace snerf;
    LpipsBwdPlan B;
    if (n_pairs < 0) return fail(SNERF_E_BADARG, "lpips_bwd_workspace_bytes: n_pairs = %lld is negative", (long long)n_pairs);
    if (lpips_bwd_plan("lpips_bwd_workspace_bytes", H, W, channels, B)) return -1;
    if (n_pairs > (0x7fffffffffffffffLL - B.fixed_bytes) / B.pair_bytes)
        return fail(SNERF_E_BADARG, "lpips_bwd_workspace_bytes: n_pairs = %lld overflows", (long long)n_pairs);
    return B.fixed_bytes + n_pairs * B.pair_bytes;
}

extern "C" int snerf_lpips_bwd_f32(const snerf_vgg_lpips *net, const float *x, const float *y, int64_t N, int64_t H, int64_t W, int64_t sn,
                                   int64_t sc, int64_t sh, int64_t sw, const float *g_layers, float *dx, float *dy, float *layers,
                                   void *workspace, int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    if (!net) return fail(SNERF_E_BADARG, "lpips_bwd: null net");
    LpipsBwdPlan B;
    if (int rc = lpips_bwd_plan("lpips_bwd", H, W, net->channels, B)) return rc;
    if (int rc = lpips_check_scalars("lpips_bwd", net, N)) return rc;
    if (N == 0) return SNERF_OK;
    if (int rc = lpips_check_net("lpips_bwd", net)) return rc;
    if (!dx && !dy) return fail(SNERF_E_BADARG, "lpips_bwd: dx and dy are both null: one output at least");
    if (!x || !y || !g_layers) return fail(SNERF_E_BADARG, "lpips_bwd: null pointer (%s)", !x ? "x" : !y ? "y" : "g_layers");
    const int64_t need = B.fixed_bytes + B.pair_bytes;
    if (!workspace || workspace_bytes < need)
        return fail(SNERF_E_BADARG, "lpips_bwd: workspace of %lld bytes, need %lld for one image pair", (long long)(workspace ? workspace_bytes : 0),
                    (long long)need);
    if (!aligned(workspace, 16)) return fail(SNERF_E_ALIGN, "lpips_bwd: workspace %p is not 16-byte aligned", workspace);
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunk = std::min(std::min(N, (workspace_bytes - B.fixed_bytes) / B.pair_bytes), B.L.max_pairs);
    // once a call: w' and the zero shift; per chunk: the tile sums, the thirteen maps, the two gradient buffers
    float *wt = static_cast<float *>(workspace), *zeros = wt + (B.fixed_bytes / 4 - CB_TAP_MAX_C);
    double *part = reinterpret_cast<double *>(static_cast<char *>(workspace) + B.fixed_bytes);
    float *maps[13], *at = reinterpret_cast<float *>(part + chunk * B.L.tiles);
    int hs[5], ws[5], first[5];
    for (int l = 0, conv = 0, h = (int)H, w = (int)W; l < 5; ++l, h /= 2, w /= 2) {
        hs[l] = h, ws[l] = w, first[l] = conv;
        for (int j = 0; j < VGG_CONVS[l]; ++j, ++conv) maps[conv] = at, at += chunk * 2 * net->channels[l] * h * w;
    }
    float *GA = at, *GB = GA + chunk * B.G;
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int m = (int)std::min(chunk, N - n0);
        // forward, with the forward entry's kernels: the standardised input in GA, the pooled maps in GB, every post-ReLU map kept
        NormArgs Z{x + n0 * sn, y + n0 * sn, sn, sc, sh, sw, m, (int)H, (int)W, {net->mean[0], net->mean[1], net->mean[2]},
                   {net->std[0], net->std[1], net->std[2]}, GA};
        hipLaunchKernelGGL(lpips_normalize_kernel, dim3((unsigned)((H * W + 255) / 256), 3, (unsigned)(2 * m)), dim3(256), 0, s, Z);
        if (int rc = check_launch("lpips_bwd(normalize)")) return rc;
        const float *in = GA;
        for (int l = 0, ci = 3; l < 5; ++l) {
            const int co = net->channels[l], h = hs[l], w = ws[l];
            for (int j = 0; j < VGG_CONVS[l]; ++j) {
                const int conv = first[l] + j;
                const bool last = j == VGG_CONVS[l] - 1;
                if (int rc = conv_launch_tap("lpips_bwd(conv)", in, 2 * m, ci, h, w, net->conv[conv].weight, nullptr /* scale = 1 */, net->conv[conv].bias, co,
                                             1, maps[conv], last && l < 4 ? GB : nullptr, s))
                    return rc;
                in = maps[conv], ci = co;
            }
            if (layers)
                if (int rc = dist_launch("lpips_bwd(distance)", in, in + (int64_t)m * co * h * w, m, co, h, w, net->lin[l], 1, layers + n0 * 5 + l, 5, nullptr,
                                         0, part, s))
                    return rc;
            in = GB;
        }
        // backward over the frames that want a gradient: both halves of the batch, or one.  U holds the gradient being worked on, V
        // receives the next one; `pooled` is the gradient to a stage's pooled input, met again at the tap before it
        const int gb = dx && dy ? 2 * m : m, half = dx ? 0 : m;
        float *U = GA, *V = GB;
        const float *pooled = nullptr;
        for (int l = 4; l >= 0; --l) {
            const int co = net->channels[l], h = hs[l], w = ws[l];
            const int64_t map = (int64_t)co * h * w;
            const float *tap = maps[first[l] + VGG_CONVS[l] - 1];
            if (int rc = dist_bwd_launch("lpips_bwd(distance)", tap, tap + m * map, m, co, h, w, net->lin[l], 1, g_layers + n0 * 5 + l, 5, dx ? U : nullptr,
                                         dy ? U + (dx ? m * map : 0) : nullptr, s))
                return rc;
            if (int rc = relu_pool_bwd_launch("lpips_bwd(relu, pool)", tap + half * map, U, pooled, gb, co, h, w, U, s)) return rc;
            for (int j = VGG_CONVS[l] - 1; j >= 0; --j) {
                const int conv = first[l] + j, ci = j > 0 ? co : l > 0 ? net->channels[l - 1] : 3;
                const int count = ci * co * 9;
                hipLaunchKernelGGL(lpips_flip_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, net->conv[conv].weight, ci, co, wt, zeros);
                if (int rc = check_launch("lpips_bwd(flip)")) return rc;
                if (int rc = conv_launch_tap("lpips_bwd(conv')", U, gb, co, h, w, wt, nullptr /* scale = 1 */, zeros, ci, 0, V, nullptr, s)) return rc;
                if (j > 0)
                    if (int rc = relu_pool_bwd_launch("lpips_bwd(relu)", maps[conv - 1] + half * map, V, nullptr, gb, co, h, w, V, s)) return rc;
                std::swap(U, V);
            }
            pooled = U;        // [gb, ci, h, w]: the stage before pools to these extents
            std::swap(U, V);
        }
        UnnormArgs R{pooled, dx ? dx + n0 * sn : nullptr, dy ? dy + n0 * sn : nullptr, sn, sc, sh, sw, m, (int)H, (int)W,
                     {net->std[0], net->std[1], net->std[2]}};
        hipLaunchKernelGGL(lpips_unnormalize_kernel, dim3((unsigned)((H * W + 255) / 256), 3, (unsigned)gb), dim3(256), 0, s, R);
        if (int rc = check_launch("lpips_bwd(standardisation)")) return rc;
    }
    return SNERF_OK;
}
