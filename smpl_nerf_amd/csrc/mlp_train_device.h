// Shared between the fp32 dgrad kernel (mlp_train.hip) and the split-bf16 one (mlp_train_bf16.hip): kernel
// arguments and the backward of the positional encoding.  (The weight-gradient side: mlp_wgrad_jobs.h.)
#pragma once
#include "mlp_device.h"

namespace snerf {

struct BwdArgs {
    const float *packed_t;
    const float *act;
    const float *d_raw;  // [n,4]
    float *dy;
    int64_t n;
    int n_hidden;
    int act_x1, act_h2, act_mask;
    int dy_rows;       // f16x3 dgrad: the per-layer |dY| exponents go behind this many tile-rows of `dy`
    int dy_sig, dy_din, dy_dn0, dy_rgb;  // dy of forward layer l <= nh+1 is l*T
    // input gradients (INPUT_GRAD kernels only)
    const float *x, *dirs;  // forward inputs: positions [n,3], directions [n/spr,3] or [n,3]
    float *d_x, *d_dirs;    // [n,3] each: d loss / d position, d loss / d (un-normalised) direction
    int dirs_per_sample, spr;
    unsigned skip_mask;
    int pos_L, pos_id, pos_nkb, dir_L, dir_id, dir_nkb, use_dir;
    int total_slabs;   // split-bf16 kernel: slabs of the transposed stream (persistent workgroups wrap around)
    int64_t n_tiles;   // split-bf16 kernel: 128-sample tiles
};

// Backward of the positional encoding (utils.py:127-131) for the slots this lane holds: dpe[kb][2u], [2u+1] are
// the gradients of (first, second) of unit p = 4*(2kb+u)+g.  Adds this lane's share to (dx, dy, dz).
template <int NKB>
__device__ __forceinline__ void pe_backward(const f4 (&dpe)[NKB], int nkb, float x, float y, float z, int L, int ident,
                                            int g, float &dx, float &dy, float &dz) {
    const int nid = ident ? 3 : 0;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        if (kb >= nkb) break;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int p = 4 * (2 * kb + u) + g;
            const float d0 = dpe[kb][2 * u], d1 = dpe[kb][2 * u + 1];
            float val = 0.f;
            int c = -1;
            if (p < nid) {
                c = p;
                val = d0;
            } else if (p - nid < 3 * L) {
                const int pp = p - nid, k = pp / 3;
                c = pp - 3 * k;
                const float v = c == 0 ? x : (c == 1 ? y : z);
                float sn, cs;
                sincosf(ldexpf(v, k), &sn, &cs);
                val = ldexpf(cs * d0 - sn * d1, k);  // d/dv sin(2^k v) = 2^k cos, d/dv cos(2^k v) = -2^k sin
            }
            dx += c == 0 ? val : 0.f;
            dy += c == 1 ? val : 0.f;
            dz += c == 2 ? val : 0.f;
        }
    }
}
__device__ __forceinline__ float sum_over_g(float v) {  // the 4 lanes (g = 0..3) that share a sample
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

struct WgradArgs;   // mlp_wgrad_jobs.h
// mlp_train_bf16.hip: the narrow jobs with two fp16 parts (f16x3 training)
int launch_wgrad_direct_f16(const Plan &P, const TrainLayout &L, const WgradArgs &W, int jobs, int G, hipStream_t s);
// mlp_train_bf16.hip: the wide jobs with split-bf16 operands (nsplit parts each)
int launch_wgrad_wide_bf16(const Plan &P, const TrainLayout &L, const WgradArgs &W, int jobs, int G, int nsplit, hipStream_t s);

// ---- host: what launch_bwd (mlp_train.hip) and launch_bwd_bf16 (mlp_train_bf16.hip) check and fill alike ----
// `what` prefixes every error text; max_pos_nkb / max_dir_nkb: the encoder k-blocks the caller's INPUT_GRAD kernels hold
inline int check_bwd_args(const char *what, const Plan &P, const MlpBwdCall &c, int max_pos_nkb, int max_dir_nkb) {
    if (c.n < 0) return fail(SNERF_E_BADARG, "%s: negative n", what);
    if (c.n == 0) return SNERF_OK;   // (an empty call is valid with any pointers: the caller returns before it touches them)
    if (!c.packed_t || !c.act || !c.d_raw || !c.dy || !c.gpart || !c.flat_grad) return fail(SNERF_E_BADARG, "%s: null pointer", what);
    if (!aligned(c.packed_t, 16) || !aligned(c.act, 16) || !aligned(c.d_raw, 16) || !aligned(c.dy, 16) || !aligned(c.gpart, 16))
        return fail(SNERF_E_ALIGN, "%s: buffers must be 16-byte aligned", what);
    if (c.d_x != nullptr) {
        if (!c.x || !c.d_dirs || (c.desc->use_dir && !c.dirs) || c.spr < 1)
            return fail(SNERF_E_BADARG, "%s: input gradients need x, dirs, d_x, d_dirs", what);
        if (P.pos_nkb > max_pos_nkb || P.dir_nkb > max_dir_nkb)
            return fail(SNERF_E_BADARG, "%s: input gradients support at most %d position / %d direction encoder k-blocks", what,
                        max_pos_nkb, max_dir_nkb);
    }
    return SNERF_OK;
}
// everything of BwdArgs but the split-bf16 kernel's total_slabs / n_tiles / dy_rows
inline BwdArgs fill_bwd_args(const Plan &P, const TrainLayout &L, const MlpBwdCall &c) {
    const snerf_mlp_desc *desc = c.desc;
    const int nh = P.n_hidden;
    BwdArgs A{};
    A.packed_t = reinterpret_cast<const float *>(c.packed_t);
    A.act = c.act;
    A.d_raw = c.d_raw;
    A.dy = c.dy;
    A.n = c.n;
    A.n_hidden = nh;
    A.act_x1 = L.x[1];
    A.act_h2 = L.h2;
    A.act_mask = L.mask;
    A.dy_sig = L.dy[nh + 2];
    A.dy_din = L.dy[nh + 3];
    A.dy_dn0 = L.dy[nh + 4];
    A.dy_rgb = L.dy[nh + 5];
    A.x = c.x;
    A.dirs = c.dirs;
    A.d_x = c.d_x;
    A.d_dirs = c.d_dirs;
    A.dirs_per_sample = c.dirs_per_sample ? 1 : 0;
    A.spr = c.spr < 1 ? 1 : c.spr;
    A.skip_mask = desc->skip_mask;
    A.pos_L = desc->pos_freqs;
    A.pos_id = desc->pos_identity ? 1 : 0;
    A.pos_nkb = P.pos_nkb;
    A.dir_L = desc->dir_freqs;
    A.dir_id = desc->dir_identity ? 1 : 0;
    A.dir_nkb = P.dir_nkb;
    A.use_dir = desc->use_dir ? 1 : 0;
    return A;
}

}  // namespace snerf
