// Kernel arguments of the 2-layer WarpFieldNet (models/warp_field_net.py:8-22) for warp.hip / warp_bf16.hip; its plan
// (make_warp_plan) lives with the other host-side layout logic in mlp_plan.h.  Below the arguments: what the forward entries of
// both files check and fill alike, and the precision dispatch of the one-call render entries.
#pragma once
#include "mlp_device.h"

namespace snerf {

struct WarpArgs {
    const float *packed;
    const float *x;     // [n,3] or null (encoded mode: every input column comes from `add`)
    const float *add;   // pose encoding [n/spr, add_dim]
    const float *o;     // [n/spr, 3] ray origins or null
    float *warp, *warped, *sdirs;  // [n,3] each, warped/sdirs nullable
    int64_t n;
    int spr;
    int pos_L, pos_id, pos_nkb, add_dim, add_nkb;
    float *act;  // training: tile-row-major [pe | pose | h] (see warp_train_layout)
    int l1_slab;        // first slab of linear2 in the stream (resident kernel)
    int64_t n_tiles;    // sample tiles (resident kernel: persistent workgroups)
    const float *ray_bias;   // resident inference kernel: [n/spr][WIDTH] = linear1.bias + linear1[:, pose columns] . pose_enc, or null
};

// ---- host ----
// one forward call of the net: the members up to `stream` are set by every caller, the others only where needed
struct WarpFwdCall {
    const snerf_warp_desc *desc;
    const void *packed;    // the fp32 stream or the split-bf16 one
    const float *x, *pose_enc, *o;
    int64_t n;
    int spr;
    float *warp, *warped, *sdirs;
    snerf_stream_t stream;
    float *act = nullptr;          // training forward (fp32): the activation buffer
    void *workspace = nullptr;     // fp32 inference: room for the per-ray pose fold (snerf_warp_fold_workspace_bytes)
    int64_t workspace_bytes = 0;
};
// what both forwards check alike (n == 0: SNERF_OK, the caller returns); x_always: the split-bf16 entry requires x in every
// call, the fp32 ones where the net has position columns or `warped` is asked for
inline int check_warp_fwd_args(const char *what, const Plan &P, const WarpFwdCall &c, bool x_always) {
    if (c.n < 0 || c.spr < 1) return fail(SNERF_E_BADARG, "%s: bad n/samples_per_ray", what);
    if (c.n == 0) return SNERF_OK;
    if (!c.packed || !c.warp || (x_always && !c.x)) return fail(SNERF_E_BADARG, "%s: null pointer", what);
    if (P.pos_dim && !c.x) return fail(SNERF_E_BADARG, "%s: x is null", what);
    if (P.add_dim && !c.pose_enc) return fail(SNERF_E_BADARG, "%s: pose_enc is null", what);
    if (c.warped && !c.x) return fail(SNERF_E_BADARG, "%s: warped requested without x", what);
    if (c.sdirs && (!c.warped || !c.o)) return fail(SNERF_E_BADARG, "%s: sdirs needs warped and o", what);
    if (!aligned(c.packed, 16)) return fail(SNERF_E_ALIGN, "%s: packed must be 16-byte aligned", what);
    return SNERF_OK;
}
// everything of WarpArgs but what belongs to one kernel (l1_slab, n_tiles, ray_bias)
inline WarpArgs fill_warp_args(const Plan &P, const WarpFwdCall &c) {
    WarpArgs A{};
    A.packed = reinterpret_cast<const float *>(c.packed);
    A.x = c.x;
    A.add = c.pose_enc;
    A.o = c.o;
    A.warp = c.warp;
    A.warped = c.warped;
    A.sdirs = c.sdirs;
    A.n = c.n;
    A.spr = c.spr;
    A.pos_L = c.desc->pos_freqs;
    A.pos_id = c.desc->pos_identity ? 1 : 0;
    A.pos_nkb = P.pos_nkb;
    A.add_dim = P.add_dim;
    A.add_nkb = P.add_nkb;
    A.act = c.act;
    return A;
}
// defined in warp.hip / warp_bf16.hip: the bodies of snerf_warp_fwd_f32, _fwd_ws_f32, _fwd_train_f32 and of snerf_warp_fwd_bf16_f32
int launch_warp_fwd(const WarpFwdCall &c);
int launch_warp_fwd_bf16(const WarpFwdCall &c);
// `precision` of the one-call entries: 0 = the fp32 kernels, otherwise the split-bf16 one (which has one format)
// (SNERF_FP32_INFER concerns the render nets' stream: the warp net runs its fp32 kernels)
inline int warp_forward(int precision, const WarpFwdCall &c) { return (precision == 0 || precision == SNERF_FP32_INFER) ? launch_warp_fwd(c) : launch_warp_fwd_bf16(c); }

}  // namespace snerf
