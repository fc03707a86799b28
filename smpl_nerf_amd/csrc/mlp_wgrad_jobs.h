// The rules the weight-gradient (wgrad) kernels of mlp_train.hip and mlp_train_bf16.hip share, each in one place:
// which (layer, segment, block) is job k of a launch, the f16x3 operand scales of a job, where a workgroup's tile-rows
// come from, the samples of a chunk, and the format of a partial (writers, and the inverse mlp_wgrad_reduce_kernel reads).
// Nothing of the dgrad side lives here (mlp_train_device.h).
#pragma once
#include "mlp_device.h"

namespace snerf {

struct WgradArgs {
    const float *act;
    const float *dy;
    float *part;  // [G][gp_floats]
    int64_t n;
    int64_t chunk;  // samples per K-split, multiple of 16
    const int *xstat, *ystat;  // f16x3 wide wgrad: exponents of the largest |X| entering / |dY| leaving forward layer l
    int fold;                  // fp32 step: narrow pairs that share an operand with a wide job ride with it (wgrad_kind)
};

// ------------------------------------------------------------------------------------------------
// which pairs are wide, narrow or folded
// ------------------------------------------------------------------------------------------------
// A (layer, input segment) pair is "wide" when it fills the 16-wave workgroup of mlp_wgrad_kernel with real work
// (the 256x256 layers and the 128x256 one); the narrow pairs - encoder columns, heads, the 128x128 layer: 15 % of
// the FLOPs - go to mlp_wgrad_direct_kernel, whose independent single-wave workgroups have no per-stage barrier.
// (Measured: sending the narrow pairs with >= 8 output tiles through mlp_wgrad_kernel's LDS stages instead, which
// would read dY and X from HBM once per job rather than 2-4 times, is 0.3 ms per 10^6 samples SLOWER - the re-reads
// of concurrently running blocks hit L2.)
__host__ __device__ inline bool wgrad_wide(const Layer &Ly, int s) { return Ly.t_out >= 8 && Ly.seg[s].nkb >= 16; }
// Folding (fp32 steps).  The narrow pairs are bound by HBM, not by the matrix pipe: a single-wave 4x4-tile job needs 2 KB of
// operands per 16 MFMAs and the 20 narrow jobs of the default net move 8.7 KB per sample - while most of those bytes are
// ALREADY staged in LDS by a wide job: the direction-encoding columns of directional_input contract the same d Y rows as
// the layer's 256-column job (only 2 more X tile-rows), and the sigma head contracts the same X rows (`o`) as that job (one
// more d Y tile-row).  mlp_wgrad_kernel computes those as extra accumulator tiles of that (half-length) job: no extra d Y / X
// traffic beyond the few extra rows, no extra barrier - and 6 of the 20 narrow jobs (2 KB per sample) disappear.
//   xseg fold: the narrow segment (<= 4 k-blocks) of directional_input, which also has a wide segment -> extra X rows
//   sigma fold: the 1-row sigma head -> extra d Y row of directional_input's hidden-segment job (same X rows, same width)
__host__ __device__ inline int wgrad_first_wide_seg(const Layer &Ly) {
    for (int s = 0; s < Ly.nseg; ++s)
        if (wgrad_wide(Ly, s)) return s;
    return -1;
}
// Only directional_input's job (8 output tiles = half the MFMAs of a 256 x 256 job for the same operand traffic) carries
// folded tiles.  (Measured r03: letting the 16-tile skip layers carry their position-encoding columns as well - +25 % MFMAs
// in that one job - made the wide kernel 17 % SLOWER: it breaks the whole-rounds schedule of 9 equal jobs x 113 chunks on
// 256 CUs.  Those columns stay direct jobs.)
__host__ __device__ inline int wgrad_fold_xseg(const Plan &P, int l, int fold = 1) {   // folded segment of layer l, or -1
    const Layer &Ly = P.layer[l];
    if (wgrad_first_wide_seg(Ly) < 0) return -1;
    if (!(Ly.t_out == 8 && l == P.n_hidden + 3 && P.nlayers == P.n_hidden + 6)) return -1;
    for (int s = 0; s < Ly.nseg; ++s)
        if (!wgrad_wide(Ly, s) && Ly.seg[s].nkb >= 1 && Ly.seg[s].nkb <= 4) return s;
    return -1;
}
__host__ __device__ inline bool wgrad_fold_sigma(const Plan &P) {
    const int nh = P.n_hidden;
    if (P.nlayers != nh + 6) return false;   // a RenderRayNet plan (the warp net's two-layer plan has no heads)
    const Layer &Ls = P.layer[nh + 2], &Ld = P.layer[nh + 3];
    return Ls.t_out == 1 && Ls.nseg == 1 && wgrad_first_wide_seg(Ld) == 0 && Ld.seg[0].nkb == Ls.seg[0].nkb && Ld.seg[0].nkb == 16 &&
           Ld.t_out == 8;
}
// (Measured r03: the 8-tile job - half the MFMAs of a 16-tile job per sample - lasts 0.7, not 0.5, of a 16-tile
// workgroup; giving it double chunks to "equalise" made the launch 19 % slower.  Per stage a workgroup pays ~20 % of a
// 16-tile stage that does not overlap with its MFMAs.)
// how the pair (layer l, segment s) is computed: 0 = wide job, 1 = rides with a wide job, 2 = direct narrow job
__host__ __device__ inline int wgrad_kind(const Plan &P, int l, int s, int fold) {
    if (wgrad_wide(P.layer[l], s)) return 0;
    if (fold) {
        if (wgrad_fold_xseg(P, l, fold) == s) return 1;
        if (l == P.n_hidden + 2 && wgrad_fold_sigma(P)) return 1;
    }
    return 2;
}

// ------------------------------------------------------------------------------------------------
// the job walk: job k of a launch -> (layer, segment, block).  Kernels, job counts and the host's table all go through it
// ------------------------------------------------------------------------------------------------
// jobs of a pair.  Wide: groups of <= 16 output tiles x groups of <= 16 input k-blocks (a 512 x 512 layer: 2 x 2 jobs);
// narrow: 4x4-tile blocks
__host__ __device__ inline int wgrad_wide_jobs(const Layer &Ly, int s) {
    return wgrad_wide(Ly, s) ? ((Ly.t_out + 15) / 16) * ((Ly.seg[s].nkb + 15) / 16) : 0;
}
__host__ __device__ inline int wgrad_narrow_jobs(const Plan &P, int l, int s, int fold) {
    return wgrad_kind(P, l, s, fold) == 2 ? ((P.layer[l].t_out + 3) / 4) * ((P.layer[l].seg[s].nkb + 3) / 4) : 0;
}
// The pairs in job order; kb0 = k-blocks of the layer in front of segment s.  visit(l, s, kb0) returns true to stop there.
template <class F>
__host__ __device__ __forceinline__ void wgrad_each_pair(const Plan &P, F &&visit) {
    for (int l = 0; l < P.nlayers; ++l) {
        int kb0 = 0;
        for (int s = 0; s < P.layer[l].nseg; ++s) {
            if (visit(l, s, kb0)) return;
            kb0 += P.layer[l].seg[s].nkb;
        }
    }
}
__host__ __device__ inline int wgrad_jobs(const Plan &P) {
    int jobs = 0;
    wgrad_each_pair(P, [&](int l, int s, int) { jobs += wgrad_wide_jobs(P.layer[l], s); return false; });
    return jobs;
}
__host__ __device__ inline int wgrad_direct_jobs(const Plan &P, int fold = 0) {
    int jobs = 0;
    wgrad_each_pair(P, [&](int l, int s, int) { jobs += wgrad_narrow_jobs(P, l, s, fold); return false; });
    return jobs;
}
struct WgradWideJob {
    int l, s, kb0;   // the pair, and the layer's k-blocks in front of the segment
    int ib, jb;      // output tiles 16*ib .., k-blocks 16*jb .. of the segment
};
struct WgradNarrowJob {
    int l, s, kb0;
    int bi, bj;      // output tiles 4*bi .., k-blocks 4*bj .. of the segment
};
// block k of a pair's jobs: a row of blocks per output-tile group
__host__ __device__ __forceinline__ void wgrad_wide_block(const Layer &Ly, int s, int k, int &ib, int &jb) {
    const int nkg = (Ly.seg[s].nkb + 15) / 16;
    ib = k / nkg;
    jb = k - ib * nkg;
}
__host__ __device__ __forceinline__ void wgrad_narrow_block(const Layer &Ly, int s, int k, int &bi, int &bj) {
    const int nbj = (Ly.seg[s].nkb + 3) / 4;
    bi = k / nbj;
    bj = k - bi * nbj;
}
// job < wgrad_jobs(P).  ONE_TILE_GROUP: the caller knows that no layer has more than 16 output tiles, so every pair has one
// group of output tiles - ib == 0, jb == the job within the pair - and the decode needs neither the product nor the division
template <bool ONE_TILE_GROUP = false>
__host__ __device__ __forceinline__ WgradWideJob wgrad_wide_job(const Plan &P, int job) {
    WgradWideJob J{0, 0, 0, 0, 0};
    wgrad_each_pair(P, [&](int l, int s, int kb0) {
        const int cnt = ONE_TILE_GROUP ? (wgrad_wide(P.layer[l], s) ? (P.layer[l].seg[s].nkb + 15) / 16 : 0) : wgrad_wide_jobs(P.layer[l], s);
        if (job >= cnt) {
            job -= cnt;
            return false;
        }
        J.l = l, J.s = s, J.kb0 = kb0;
        if (ONE_TILE_GROUP) J.jb = job;
        else wgrad_wide_block(P.layer[l], s, job, J.ib, J.jb);
        return true;
    });
    return J;
}
// job < wgrad_direct_jobs(P, fold)
__host__ __device__ __forceinline__ WgradNarrowJob wgrad_narrow_job(const Plan &P, int fold, int job) {
    WgradNarrowJob J{0, 0, 0, 0, 0};
    wgrad_each_pair(P, [&](int l, int s, int kb0) {
        const int cnt = wgrad_narrow_jobs(P, l, s, fold);
        if (job >= cnt) {
            job -= cnt;
            return false;
        }
        J.l = l, J.s = s, J.kb0 = kb0;
        wgrad_narrow_block(P.layer[l], s, job, J.bi, J.bj);
        return true;
    });
    return J;
}
// the bias sums of a layer ride with the jobs of its first non-empty input segment (their first k-block group / block column)
__host__ __device__ __forceinline__ int wgrad_bias_seg(const Layer &Ly) {
    int s = 0;
    while (s < Ly.nseg && Ly.seg[s].nkb == 0) ++s;
    return s;
}

// ------------------------------------------------------------------------------------------------
// f16x3: the operand scales of a job
// ------------------------------------------------------------------------------------------------
// f16x3 statistics (STAT_INTS ints behind the rows of act / dy): exponent of the largest |X| entering forward layer l
// through its hidden segment at [l], of the largest encoder / additional-input column at [STAT_ENC]; of the largest |dY|
// of forward layer l at [l].  Encoded directions are <= 1.
constexpr int STAT_ENC = STAT_INTS - 1;
__host__ __device__ inline int xstat_index(const Plan &P, int l, int s) {   // -1: exponent 0 (direction encoding)
    const Seg &sg = P.layer[l].seg[s];
    if (sg.type == SEG_HIDDEN) return l == P.n_hidden + 2 ? P.n_hidden + 3 : l;   // the sigma head reads what directional_input reads
    if (sg.type == SEG_PE && l == P.n_hidden + 3) return -1;
    return STAT_ENC;
}
// X and dY of a job are scaled by sx, sy = 2^(14 - exponent of their largest value over all samples) and the result by `unscale`
// (why per job and not per sample: mlp_train_bf16.hip, above mlp_wgrad_bf16_kernel)
struct WgradScales {
    float sx, sy, unscale;
};
__device__ __forceinline__ WgradScales wgrad_f16_scales(const Plan &P, const WgradArgs &A, int l, int s) {
    // X scale: the statistic of THIS segment (xstat_index: the layer's hidden input, or the encoder / additional-input
    // columns).  r04: this read xstat[l] - the hidden input's - for every wide job of the layer; with encoded pose columns
    // (1380 of them: wide jobs of their own) layer 0 has no hidden input, its statistic is unset and the scale was 2^114
    // (found by tools/ab/fuzz_train.py in chunked f16x3 steps)
    const int xi = xstat_index(P, l, s);
    const int ex = 14 - (xi < 0 ? 0 : min(max(A.xstat[xi], -100), 100)), ey = 14 - min(max(A.ystat[l], -100), 100);
    return {__builtin_ldexpf(1.f, ex), __builtin_ldexpf(1.f, ey), __builtin_ldexpf(1.f, -(ex + ey))};
}

// ------------------------------------------------------------------------------------------------
// the tile-rows a wave of a wide job brings into LDS
// ------------------------------------------------------------------------------------------------
// Wave `wave` brings LDS rows ROWS_PER_WAVE * wave + q (rows 0..15 = dY tile-rows ti0 .. of layer l, 16..31 = X tile-rows
// 16*jb .. of segment s).  Rows the job does not have re-load the job's first dY row (finite filler), so that every wave
// issues the same number of pieces per stage and one counted vmcnt serves all waves.
// (dy, act, n as scalars, not as WgradArgs: with the struct the prologue of mlp_wgrad_f16_kernel came out 23 instructions longer
// and the kernel 1.5 % slower.)
template <int ROWS_PER_WAVE>
__device__ __forceinline__ void wgrad_row_sources(const Plan &P, const TrainLayout &L, const float *dy, const float *act, int64_t n,
                                                  int l, int s, int ti0, int jb, int n_rows_y, int n_rows_x, int wave,
                                                  const float *(&row_src)[ROWS_PER_WAVE]) {
#pragma unroll
    for (int q = 0; q < ROWS_PER_WAVE; ++q) {
        const int r = ROWS_PER_WAVE * wave + q;
        int64_t grow = L.dy[l] + ti0;
        if (r < 16) {
            if (r < n_rows_y) grow = L.dy[l] + ti0 + r;
            row_src[q] = dy + grow * n * 16;
        } else if (r - 16 < n_rows_x) {
            row_src[q] = act + (int64_t)(seg_act_row(P, L, l, s) + 16 * jb + (r - 16)) * n * 16;
        } else {
            row_src[q] = dy + grow * n * 16;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the samples of a chunk (blockIdx.y)
// ------------------------------------------------------------------------------------------------
struct WgradChunk {
    int64_t begin, end;
    // begin < end: a chunk behind the end of the buffer has no stages at all.  r04: without this the difference went
    // negative and the masked loop of mlp_wgrad_kernel ran stages -k .. -1 - a = 0 against whatever the LDS held, which is 0
    // unless that is a NaN: the first process on a freshly booted GPU got NaN gradients, everybody else the right ones.
    // tools/ab/nan_hunt.py
    __device__ __forceinline__ int stages(int stage) const { return begin < end ? (int)((end - begin + stage - 1) / stage) : 0; }
    __device__ __forceinline__ int whole_stages(int stage) const { return begin < end ? (int)((end - begin) / stage) : 0; }
};
__device__ __forceinline__ WgradChunk wgrad_chunk(const WgradArgs &A) {
    const int64_t begin = (int64_t)blockIdx.y * A.chunk;
    return {begin, min(A.n, begin + A.chunk)};
}

// ------------------------------------------------------------------------------------------------
// the format of a partial
// ------------------------------------------------------------------------------------------------
// A layer's block of a chunk's partial (`part` = A.part + chunk * L.gp_floats + L.gp[l]): t_out x nkb tiles of 16 x 16 as
// [ti][tj][64 lanes][4] - the MFMA D layout: lane (j = lane & 15, g = lane >> 4) holds rows 4g .. 4g+3 of column (slot) j -
// then the t_out * 16 bias sums.
__device__ __forceinline__ int64_t partial_tile_offset(int nkb, int ti, int tj, int lane) {
    return ((int64_t)(ti * nkb + tj) * 64 + lane) * 4;
}
__device__ __forceinline__ void store_partial_tile(float *part, int nkb, int ti, int tj, int lane, f4 v) {
    *reinterpret_cast<f4 *>(part + partial_tile_offset(nkb, ti, tj, lane)) = v;
}
__device__ __forceinline__ int64_t partial_bias_offset(int t_out, int nkb) { return (int64_t)t_out * nkb * 256; }
// v: this lane's sum of feature (lane & 15) of dY tile-row `tile_row` over its share of the samples (the four lanes that
// share a feature hold a quarter each)
__device__ __forceinline__ void store_bias_sums(float *part, int t_out, int nkb, int tile_row, int lane, float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < 16) part[partial_bias_offset(t_out, nkb) + tile_row * 16 + lane] = v;
}
// The inverse, for mlp_wgrad_reduce_kernel: element `rel` of a layer's block is register r of lane `lane` of tile (ti, tj)
// - true - or bias sum rel - partial_bias_offset - false
__device__ __forceinline__ bool partial_tile_element(int t_out, int nkb, int rel, int &ti, int &tj, int &lane, int &r) {
    if (rel >= (int)partial_bias_offset(t_out, nkb)) return false;
    const int tile = rel >> 8;
    r = rel & 3, lane = (rel >> 2) & 63;
    ti = tile / nkb, tj = tile - ti * nkb;
    return true;
}

}  // namespace snerf
