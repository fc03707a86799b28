// Structural similarity of two image batches (util/scores.py:88-173: ssim, _ssim_per_channel), its backward, and the squared error the
// MSE and PSNR scores need (scores.py:28, 47-48) - without the reference's five grouped conv2d calls and their [N,C,H,W] temporaries.
// Per image n and channel c, with the separable window G = win (x) win of size k applied as a VALID correlation (P = OH OW windows q,
// OH = H - k + 1, OW = W - k + 1):
//   mu1 = G*x   mu2 = G*y   e11 = G*(x x)   e22 = G*(y y)   e12 = G*(x y)
//   s11 = e11 - mu1^2   s22 = e22 - mu2^2   s12 = e12 - mu1 mu2
//   A = mu1^2 + mu2^2 + c1      D = s11 + s22 + c2
//   L = (2 mu1 mu2 + c1) / A    CS = (2 s12 + c2) / D    S = L CS
//   ssim[n,c] = mean_q S        cs[n,c] = mean_q CS        sqerr[n,c] = sum over all H W pixels of (x - y)^2
// Backward, for the upstream gradients gS[n,c] and gC[n,c]: per window w = (gS L + gC) / P, u = gS CS / P,
//   a = u (2 mu2 - 2 mu1 L) / A + w (2 mu1 CS - 2 mu2) / D      b = -w CS / D      c = 2 w / D      (zero outside the valid windows)
//   dx[p] = (G^T a)[p] + 2 x[p] (G^T b)[p] + y[p] (G^T c)[p]      G^T: the full correlation with the flipped window
// S and CS are symmetric in (x, y): dy is the same kernel called with the two images swapped.  The backward recomputes the window
// statistics from x and y; the forward keeps nothing of map size.
//
// Arithmetic.  Every filter tap is one fmaf, taps in ascending order, the horizontal pass first and the vertical pass second, so a
// moment depends on its window's pixels alone - not on the tile it falls into or on the strides the image is stored with.  The squares
// mu1^2, mu2^2, mu1 mu2 are rounded products (they are shared by A and by the numerator of L), s = fmaf(-mu, mu, e), sums as written
// above from left to right, both quotients IEEE divisions.  With x == y all three s and all three products agree bit for bit, so
// L = CS = S = 1 exactly.  No shift is subtracted before the moments: the cancellation in s = e - mu^2 is what the bound of
// tests/ssim_ref.py (16 u cond, cond = (e11 + e22) / D) allows for.  Tile partial sums and (x - y)^2 are accumulated in float64.
//
// Mapping.  Workgroup = 256 lanes = one tile; LDS planes have an odd pitch (rows r, r + 1, r + 2, r + 3 then start on different
// banks modulo 4 while a lane's four-column group steps by 4: the 32 lanes of a ds_read_b32 / ds_write_b32 group meet 32 banks).
//   forward  tile = 32 x 32 windows.  (1) the (31 + k)^2 patches of x and y -> LDS (zeros outside the image); the tile owns the
//            input pixels [32 ty, 32 ty + 32) x [32 tx, 32 tx + 32) - the last tile of a dimension also the rest up to H or W, which
//            its patch covers - and sums their (x - y)^2.  (2) horizontal pass: five planes [31 + k][32], a lane = one row and four
//            adjacent columns, the k + 3 patch values read once and slid over the four sums.  (3) vertical pass into registers: a
//            lane = one column and four rows.  (4) L, CS, S; the three tile sums go through the DPP scan of each wave and then in
//            wave order to workspace[n c][tile] (three doubles).  A second launch adds the tiles of an image in a fixed order
//            (lane l takes tiles l, l + 64, ..., then the wave scan) and divides by P.
//   backward tile = 32 x 32 INPUT pixels (16 x 16 for k >= 29, whose planes would not fit the 160 KB).  (1) the (30 + 2k)^2 patches;
//            (2) horizontal and (3) vertical pass over the (31 + k)^2 windows the tile's pixels lie in, then a, b, c -> three planes
//            that take the patches' place (the tile's own x, y are in registers by then); (4) horizontal and (5) vertical pass with
//            the flipped window, the latter into registers; dx is written with the input strides.
// Per window of the forward, read off the source at k = 11: about 240 vector instructions (5 fmaf per tap and pass - the horizontal
// pass runs (31 + k) / 32 = 1.31 plane rows per window row - plus the products, two IEEE divisions and the staging) and about 27 LDS
// words read, 10 written; the inputs are 8 bytes per pixel and channel, read once plus the halo.  VALU is the nearest bound.
// No atomics, no read-modify-write of global memory, every sum in a fixed order: two calls give the same bits.  Every output element
// is written; every LDS word that is read has been written.
#include <math.h>

#include "snerf_common.h"
#include "ssim_tiles.h"

namespace snerf {

constexpr int SSIM_RED = 12;   // doubles at the start of the dynamic LDS: three sums x four waves

constexpr __host__ __device__ int ssim_odd(int n) { return n | 1; }

// forward LDS: patches x, y [PR][PP], five planes [PR][HP]
struct SsimFwdLds {
    int PR, PP, HP, hplane, floats;
};
constexpr __host__ __device__ SsimFwdLds ssim_fwd_lds(int k) {
    const int PR = SSIM_TILE + k - 1, PP = ssim_odd(PR), HP = ssim_odd(SSIM_TILE);
    return {PR, PP, HP, PR * HP, 2 * PR * PP + 5 * PR * HP};
}
// backward LDS: region 0 = patches x, y [PR][PP], later a, b, c [WR][WP]; region 1 = five planes [PR][HP], later three [WR][TP]
struct SsimBwdLds {
    int PR, PP, WR, WP, HP, TP, hplane, aplane, tplane, r0, floats;
};
constexpr __host__ __device__ SsimBwdLds ssim_bwd_lds(int T, int k) {
    const int PR = T + 2 * k - 2, PP = ssim_odd(PR), WR = T + k - 1, WP = ssim_odd(WR), HP = WP, TP = ssim_odd(T);
    const int r0 = 2 * PR * PP > 3 * WR * WP ? 2 * PR * PP : 3 * WR * WP;
    return {PR, PP, WR, WP, HP, TP, PR * HP, WR * WP, WR * TP, r0, r0 + 5 * PR * HP};
}
constexpr int ssim_lds_bytes(int floats) { return SSIM_RED * (int)sizeof(double) + floats * (int)sizeof(float); }
static_assert(ssim_lds_bytes(ssim_fwd_lds(SSIM_MAX_K).floats) <= SSIM_LDS_BYTES, "ssim forward: LDS");
static_assert(ssim_lds_bytes(ssim_bwd_lds(SSIM_TILE, SSIM_BWD_SMALL_FROM_K - 1).floats) <= SSIM_LDS_BYTES &&
                  ssim_lds_bytes(ssim_bwd_lds(SSIM_TILE, SSIM_BWD_SMALL_FROM_K).floats) > SSIM_LDS_BYTES,
              "ssim backward: SSIM_BWD_SMALL_FROM_K is the first window size whose 32 x 32 tile does not fit");
static_assert(ssim_lds_bytes(ssim_bwd_lds(SSIM_BWD_TILE_SMALL, SSIM_MAX_K).floats) <= SSIM_LDS_BYTES, "ssim backward: LDS of the small tile");
// (region 1 holds the three planes [WR][TP] as well: WR <= PR, TP <= HP)

struct SsimArgs {
    const float *x, *y, *win;
    int64_t sn, sc, sh, sw;
    int C, H, W, OH, OW, k, tiles_y, tiles_x;
    float c1, c2;
    double *part;                 // forward: [N C][tiles][3]
    const float *g_ssim, *g_cs;   // backward
    float *dx;
};

// R consecutive outputs of NQ quantities along a pass: out[o] = sum_t wt[t] in[o + t] with wt = win, or win flipped; t ascending.
// load(j, v) hands over the NQ inputs at position j = 0 .. k + R - 2, each read once.  KT > 0: k = KT at compile time.
template <int KT, int NQ, int R, bool FLIP, class Load>
__device__ __forceinline__ void ssim_slide(const float *win, int k, Load &&load, float (&acc)[R][NQ]) {
#pragma unroll
    for (int o = 0; o < R; ++o)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[o][q] = 0.f;
    auto step = [&](int j) {
        float v[NQ];
        load(j, v);
#pragma unroll
        for (int o = 0; o < R; ++o) {
            const int t = j - o;
            if (t >= 0 && t < k) {
                const float w = win[FLIP ? k - 1 - t : t];
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[o][q] = fmaf(w, v[q], acc[o][q]);
            }
        }
    };
    if constexpr (KT > 0) {
#pragma unroll
        for (int j = 0; j < KT + R - 1; ++j) step(j);
    } else {
        for (int j = 0; j < k + R - 1; ++j) step(j);
    }
}

// horizontal pass of the five moments: hp[q][r][c] = sum_t win[t] f_q(px[r][c + t], py[r][c + t]), r < rows, c < ocols = pcols - k + 1
template <int KT>
__device__ __forceinline__ void ssim_hpass5(const float *px, const float *py, int ppitch, int rows, int pcols, int ocols, float *hp,
                                            int hpitch, int hplane, const float *win, int k) {
    const int groups = (ocols + 3) >> 2;
    for (int item = threadIdx.x; item < rows * groups; item += SSIM_THREADS) {
        const int r = item / groups, c0 = (item - r * groups) * 4;
        const float *rx = px + r * ppitch + c0, *ry = py + r * ppitch + c0;
        float acc[4][5];
        ssim_slide<KT, 5, 4, false>(
            win, k,
            [&](int j, float(&v)[5]) {
                const bool in = c0 + j < pcols;   // (past the row's end: only the outputs past ocols would take it)
                const float a = in ? rx[j] : 0.f, b = in ? ry[j] : 0.f;
                v[0] = a, v[1] = b, v[2] = a * a, v[3] = b * b, v[4] = a * b;
            },
            acc);
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (c0 + o < ocols) {
#pragma unroll
                for (int q = 0; q < 5; ++q) hp[q * hplane + r * hpitch + c0 + o] = acc[o][q];
            }
    }
}

// vertical pass of the five moments of the windows (r0 .. r0 + 3, col): acc[o] = (mu1, mu2, e11, e22, e12)
template <int KT>
__device__ __forceinline__ void ssim_vpass5(const float *hp, int hpitch, int hplane, int prows, int col, int r0, const float *win, int k,
                                            float (&acc)[4][5]) {
    ssim_slide<KT, 5, 4, false>(
        win, k,
        [&](int j, float(&v)[5]) {
            const bool in = r0 + j < prows;
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] = in ? hp[q * hplane + (r0 + j) * hpitch + col] : 0.f;
        },
        acc);
}

// what a window's five moments give: the header's formulas, in this order
struct SsimWindow {
    float mu1, mu2, A, D, L, CS;
};
__device__ __forceinline__ SsimWindow ssim_window(const float (&m)[5], float c1, float c2) {
    const float mu1 = m[0], mu2 = m[1];
    const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
    const float s11 = fmaf(-mu1, mu1, m[2]), s22 = fmaf(-mu2, mu2, m[3]), s12 = fmaf(-mu1, mu2, m[4]);
    const float A = (m11 + m22) + c1, D = (s11 + s22) + c2;
    return {mu1, mu2, A, D, (2.f * m12 + c1) / A, (2.f * s12 + c2) / D};
}

struct SsimTile {
    int nc, ty, tx;
    int64_t base;
};
__device__ __forceinline__ SsimTile ssim_tile(const SsimArgs &A) {
    const int tiles = A.tiles_y * A.tiles_x, b = (int)blockIdx.x;
    const int nc = b / tiles, t = b - nc * tiles, ty = t / A.tiles_x;
    return {nc, ty, t - ty * A.tiles_x, (int64_t)(nc / A.C) * A.sn + (int64_t)(nc % A.C) * A.sc};
}

template <int KT>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_fwd_kernel(SsimArgs A) {
    extern __shared__ double ssim_lds[];
    constexpr int T = SSIM_TILE;
    const int k = KT > 0 ? KT : A.k;
    const SsimFwdLds G = ssim_fwd_lds(k);
    float *px = reinterpret_cast<float *>(ssim_lds + SSIM_RED), *py = px + G.PR * G.PP, *hp = py + G.PR * G.PP;
    const int tid = threadIdx.x;
    const SsimTile tl = ssim_tile(A);
    const int y0 = tl.ty * T, x0 = tl.tx * T;
    const int own_h = tl.ty == A.tiles_y - 1 ? A.H - y0 : T, own_w = tl.tx == A.tiles_x - 1 ? A.W - x0 : T;   // (<= PR: the patch covers them)

    double sq = 0.0;
    for (int i = tid; i < G.PR * G.PR; i += SSIM_THREADS) {
        const int r = i / G.PR, c = i - r * G.PR, gy = y0 + r, gx = x0 + c;
        float xv = 0.f, yv = 0.f;
        if (gy < A.H && gx < A.W) {
            const int64_t off = tl.base + (int64_t)gy * A.sh + (int64_t)gx * A.sw;
            xv = A.x[off], yv = A.y[off];
            if (r < own_h && c < own_w) {
                const double d = (double)xv - (double)yv;
                sq += d * d;
            }
        }
        px[r * G.PP + c] = xv, py[r * G.PP + c] = yv;
    }
    __syncthreads();
    ssim_hpass5<KT>(px, py, G.PP, G.PR, G.PR, T, hp, G.HP, G.hplane, A.win, k);
    __syncthreads();

    const int col = tid & (T - 1), r0 = (tid >> 5) * 4;
    float acc[4][5];
    ssim_vpass5<KT>(hp, G.HP, G.hplane, G.PR, col, r0, A.win, k, acc);
    float sS = 0.f, sC = 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const SsimWindow w = ssim_window(acc[o], A.c1, A.c2);
        const bool valid = y0 + r0 + o < A.OH && x0 + col < A.OW;
        sS += valid ? w.L * w.CS : 0.f;
        sC += valid ? w.CS : 0.f;
    }
    // the tile's three sums: each wave's through the DPP scan, then the four waves in wave order
    const double v[3] = {wave_sum((double)sS), wave_sum((double)sC), wave_sum(sq)};
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) ssim_lds[(tid >> 6) * 3 + q] = v[q];
    }
    __syncthreads();
    if (tid < 3) A.part[(int64_t)blockIdx.x * 3 + tid] = ((ssim_lds[tid] + ssim_lds[3 + tid]) + ssim_lds[6 + tid]) + ssim_lds[9 + tid];
}

// one wave per (n, c): lane l adds the tiles l, l + 64, ... in that order, the DPP scan adds the lanes
__global__ __launch_bounds__(WAVE) void ssim_reduce_kernel(const double *part, int tiles, double windows, float *ssim, float *cs, float *sqerr) {
    const int lane = threadIdx.x;
    const double *p = part + (int64_t)blockIdx.x * tiles * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int t = lane; t < tiles; t += WAVE) {
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += p[(int64_t)t * 3 + q];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q] = wave_sum(s[q]);
    if (lane != 0) return;
    ssim[blockIdx.x] = (float)(s[0] / windows);
    if (cs) cs[blockIdx.x] = (float)(s[1] / windows);
    if (sqerr) sqerr[blockIdx.x] = (float)s[2];
}

template <int KT, int T>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_bwd_kernel(SsimArgs A) {
    extern __shared__ double ssim_lds[];
    constexpr int R = T * T / SSIM_THREADS;   // pixels per lane: a column's R consecutive rows
    static_assert(R * SSIM_THREADS == T * T && T % 4 == 0, "ssim backward: tile");
    const int k = KT > 0 ? KT : A.k;
    const SsimBwdLds G = ssim_bwd_lds(T, k);
    float *px = reinterpret_cast<float *>(ssim_lds + SSIM_RED), *py = px + G.PR * G.PP, *abc = px, *hp = px + G.r0, *tp = hp;
    const int tid = threadIdx.x;
    const SsimTile tl = ssim_tile(A);
    const int y0 = tl.ty * T, x0 = tl.tx * T, wy0 = y0 - (k - 1), wx0 = x0 - (k - 1);   // first pixel; first window and patch pixel

    for (int i = tid; i < G.PR * G.PR; i += SSIM_THREADS) {
        const int r = i / G.PR, c = i - r * G.PR, gy = wy0 + r, gx = wx0 + c;
        float xv = 0.f, yv = 0.f;
        if (gy >= 0 && gy < A.H && gx >= 0 && gx < A.W) {
            const int64_t off = tl.base + (int64_t)gy * A.sh + (int64_t)gx * A.sw;
            xv = A.x[off], yv = A.y[off];
        }
        px[r * G.PP + c] = xv, py[r * G.PP + c] = yv;
    }
    __syncthreads();
    const int col = tid % T, r0 = (tid / T) * R;
    float xc[R], yc[R];   // the lane's own pixels: the patches are overwritten below
#pragma unroll
    for (int o = 0; o < R; ++o) {
        xc[o] = px[(k - 1 + r0 + o) * G.PP + k - 1 + col];
        yc[o] = py[(k - 1 + r0 + o) * G.PP + k - 1 + col];
    }
    ssim_hpass5<KT>(px, py, G.PP, G.PR, G.PR, G.WR, hp, G.HP, G.hplane, A.win, k);
    __syncthreads();

    // the windows' a, b, c: lane = a column of windows and four rows
    const double windows = (double)A.OH * (double)A.OW;
    const float gs = (float)((double)A.g_ssim[tl.nc] / windows), gc = A.g_cs ? (float)((double)A.g_cs[tl.nc] / windows) : 0.f;
    const int wgroups = (G.WR + 3) >> 2;
    for (int item = tid; item < wgroups * G.WR; item += SSIM_THREADS) {
        const int rg = item / G.WR, wc = item - rg * G.WR, wr0 = rg * 4;
        float acc[4][5];
        ssim_vpass5<KT>(hp, G.HP, G.hplane, G.PR, wc, wr0, A.win, k, acc);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (wr0 + o >= G.WR) continue;
            const int qy = wy0 + wr0 + o, qx = wx0 + wc;
            float a = 0.f, b = 0.f, c = 0.f;
            if (qy >= 0 && qy < A.OH && qx >= 0 && qx < A.OW) {
                const SsimWindow s = ssim_window(acc[o], A.c1, A.c2);
                const float w = fmaf(gs, s.L, gc), u = gs * s.CS;
                a = u * (2.f * s.mu2 - 2.f * s.mu1 * s.L) / s.A + w * (2.f * s.mu1 * s.CS - 2.f * s.mu2) / s.D;
                b = -(w * s.CS) / s.D;
                c = 2.f * w / s.D;
            }
            float *out = abc + (wr0 + o) * G.WP + wc;
            out[0] = a, out[G.aplane] = b, out[2 * G.aplane] = c;
        }
    }
    __syncthreads();

    // G^T, horizontal: tp[q][wr][j] = sum_s win[k - 1 - s] abc[q][wr][j + s], j < T
    for (int item = tid; item < G.WR * (T / 4); item += SSIM_THREADS) {
        const int wr = item / (T / 4), c0 = (item - wr * (T / 4)) * 4;
        const float *row = abc + wr * G.WP + c0;
        float acc[4][3];
        ssim_slide<KT, 3, 4, true>(
            A.win, k,
            [&](int j, float(&v)[3]) {   // c0 + j <= T - 1 + k - 1 = WR - 1
#pragma unroll
                for (int q = 0; q < 3; ++q) v[q] = row[q * G.aplane + j];
            },
            acc);
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int q = 0; q < 3; ++q) tp[q * G.tplane + wr * G.TP + c0 + o] = acc[o][q];
    }
    __syncthreads();

    // G^T, vertical, into registers: pixel (r0 + o, col) takes the rows r0 + o .. r0 + o + k - 1 of tp
    float acc[R][3];
    ssim_slide<KT, 3, R, true>(
        A.win, k,
        [&](int j, float(&v)[3]) {   // r0 + j <= T - R + k + R - 2 = WR - 1
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = tp[q * G.tplane + (r0 + j) * G.TP + col];
        },
        acc);
#pragma unroll
    for (int o = 0; o < R; ++o) {
        const int gy = y0 + r0 + o, gx = x0 + col;
        if (gy < A.H && gx < A.W)
            A.dx[tl.base + (int64_t)gy * A.sh + (int64_t)gx * A.sw] = fmaf(yc[o], acc[o][2], fmaf(2.f * xc[o], acc[o][1], acc[o][0]));
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct SsimShape {
    int64_t NC, tiles_y, tiles_x;   // forward tiles
};
// the checks both entries and the workspace query share; fills `s`
static int ssim_check_shape(const char *op, int64_t N, int64_t C, int64_t H, int64_t W, int k, SsimShape &s) {
    if (N < 0 || C < 0) return fail(SNERF_E_BADARG, "%s: N and C must not be negative", op);
    if (k < 1 || k > SSIM_MAX_K) return fail(SNERF_E_BADARG, "%s: the window size k = %d must be 1 .. %d", op, k, SSIM_MAX_K);
    if (H < k || W < k)
        return fail(SNERF_E_BADARG, "%s: the window (k = %d) can't be greater than the image (H = %lld, W = %lld)", op, k, (long long)H, (long long)W);
    if (H > 0x7fffffffLL - 4 * SSIM_MAX_K || W > 0x7fffffffLL - 4 * SSIM_MAX_K || C > 0x7fffffffLL)
        return fail(SNERF_E_BADARG, "%s: C, H and W must be below 2^31", op);
    s.NC = N * C;
    s.tiles_y = (H - k + 1 + SSIM_TILE - 1) / SSIM_TILE;
    s.tiles_x = (W - k + 1 + SSIM_TILE - 1) / SSIM_TILE;
    // the backward's tiles over the input pixels are the most a launch of either entry has (its small tile: 16)
    const int64_t by = (H + SSIM_BWD_TILE_SMALL - 1) / SSIM_BWD_TILE_SMALL, bx = (W + SSIM_BWD_TILE_SMALL - 1) / SSIM_BWD_TILE_SMALL;
    if (by * bx > 0x7fffffffLL || (s.NC > 0 && by * bx > 0x7fffffffLL / s.NC) || (C > 0 && N > 0x7fffffffLL / C))
        return fail(SNERF_E_BADARG, "%s: N C times the number of tiles must be below 2^31", op);
    return SNERF_OK;
}
static int64_t ssim_ws_bytes(const SsimShape &s) { return s.NC * s.tiles_y * s.tiles_x * 3 * (int64_t)sizeof(double); }

static int ssim_check_call(const char *op, float c1, float c2, const void *x, const void *y, const void *win, const void *out, const char *out_name,
                           const SsimShape &s, const void *workspace, int64_t workspace_bytes) {
    if (!(c1 >= 0.f) || !(c2 >= 0.f) || !(c1 <= 3.4028234663852886e38f) || !(c2 <= 3.4028234663852886e38f))
        return fail(SNERF_E_BADARG, "%s: c1 and c2 must be finite and not negative", op);
    if (s.NC == 0) return 1;   // nothing to do
    if (!x || !y || !win || !out) return fail(SNERF_E_BADARG, "%s: null pointer (x, y, win, %s)", op, out_name);
    if (!workspace || workspace_bytes < ssim_ws_bytes(s))
        return fail(SNERF_E_BADARG, "%s: workspace missing or smaller than snerf_ssim_workspace_bytes()", op);
    if (!aligned(workspace, 8)) return fail(SNERF_E_ALIGN, "%s: workspace must be 8-byte aligned", op);
    return SNERF_OK;
}

template <int KT>
static int ssim_bwd_launch(const SsimArgs &A0, int64_t NC, hipStream_t s) {
    SsimArgs A = A0;
    const bool small = A.k >= SSIM_BWD_SMALL_FROM_K;
    const int T = small ? SSIM_BWD_TILE_SMALL : SSIM_TILE;
    A.tiles_y = (A.H + T - 1) / T, A.tiles_x = (A.W + T - 1) / T;
    const dim3 grid((unsigned)(NC * A.tiles_y * A.tiles_x)), block(SSIM_THREADS);
    const int lds = ssim_lds_bytes(ssim_bwd_lds(T, A.k).floats);
    if constexpr (KT == 0 || KT >= SSIM_BWD_SMALL_FROM_K)
        if (small) return launch_lds_limit<ssim_bwd_kernel<KT, SSIM_BWD_TILE_SMALL>>("ssim_bwd", grid, block, lds, SSIM_LDS_BYTES, s, A);
    return launch_lds_limit<ssim_bwd_kernel<KT, SSIM_TILE>>("ssim_bwd", grid, block, lds, SSIM_LDS_BYTES, s, A);
}

}  // namespace snerf

extern "C" int64_t snerf_ssim_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int k) {
    using namespace snerf;
    SsimShape s;
    if (ssim_check_shape("ssim_workspace_bytes", N, C, H, W, k, s)) return -1;
    return ssim_ws_bytes(s);
}

extern "C" int snerf_ssim_fwd_f32(const float *x, const float *y, int64_t N, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc,
                                  int64_t sh, int64_t sw, const float *win, int k, float c1, float c2, float *ssim, float *cs, float *sqerr,
                                  void *workspace, int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    SsimShape sp;
    if (int rc = ssim_check_shape("ssim_fwd", N, C, H, W, k, sp)) return rc;
    if (int rc = ssim_check_call("ssim_fwd", c1, c2, x, y, win, ssim, "ssim", sp, workspace, workspace_bytes)) return rc < 0 ? rc : SNERF_OK;
    hipStream_t s = (hipStream_t)stream;
    const int tiles = (int)(sp.tiles_y * sp.tiles_x);
    SsimArgs A{x, y, win, sn, sc, sh, sw, (int)C, (int)H, (int)W, (int)(H - k + 1), (int)(W - k + 1), k, (int)sp.tiles_y, (int)sp.tiles_x,
               c1, c2, (double *)workspace, nullptr, nullptr, nullptr};
    const dim3 grid((unsigned)(sp.NC * tiles)), block(SSIM_THREADS);
    const int lds = ssim_lds_bytes(ssim_fwd_lds(k).floats), limit = ssim_lds_bytes(ssim_fwd_lds(SSIM_MAX_K).floats);
    if (int rc = k == 11 ? launch_lds_limit<ssim_fwd_kernel<11>>("ssim_fwd", grid, block, lds, limit, s, A)
                         : launch_lds_limit<ssim_fwd_kernel<0>>("ssim_fwd", grid, block, lds, limit, s, A))
        return rc;
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3((unsigned)sp.NC), dim3(WAVE), 0, s, (const double *)workspace, tiles,
                       (double)A.OH * (double)A.OW, ssim, cs, sqerr);
    return check_launch("ssim_fwd");
}

extern "C" int snerf_ssim_bwd_f32(const float *x, const float *y, int64_t N, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc,
                                  int64_t sh, int64_t sw, const float *win, int k, float c1, float c2, const float *g_ssim, const float *g_cs,
                                  float *dx, void *workspace, int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    SsimShape sp;
    if (int rc = ssim_check_shape("ssim_bwd", N, C, H, W, k, sp)) return rc;
    if (int rc = ssim_check_call("ssim_bwd", c1, c2, x, y, win, dx, "dx", sp, workspace, workspace_bytes)) return rc < 0 ? rc : SNERF_OK;
    if (!g_ssim) return fail(SNERF_E_BADARG, "ssim_bwd: null pointer (g_ssim)");
    SsimArgs A{x, y, win, sn, sc, sh, sw, (int)C, (int)H, (int)W, (int)(H - k + 1), (int)(W - k + 1), k, 0, 0,
               c1, c2, nullptr, g_ssim, g_cs, dx};
    if (int rc = k == 11 ? ssim_bwd_launch<11>(A, sp.NC, (hipStream_t)stream) : ssim_bwd_launch<0>(A, sp.NC, (hipStream_t)stream)) return rc;
    return check_launch("ssim_bwd");
}
