"""sha256 of every output array of a fixed, seeded table of calls into the host entries of the two fused networks.

    python tools/net_entry_digest.py > digest.txt

The table reaches every host decision in front of RenderRayNet and WarpFieldNet (csrc/mlp*.hip, warp*.hip, render.hip,
train_step.hip): which kernel a call runs, with which tile size, with or without the per-ray fold, in which precision.  It uses
smpl_nerf_amd._lib and the C ABI alone, so the same file runs in a checkout of any commit with the same include/smplnerf.h: two
commits compute the same bits iff their outputs are the same text.  Outputs are zero-filled before a call, every call is made twice
into fresh buffers, and an array whose two digests differ is marked UNSTABLE (such an array cannot be compared between commits).
The shapes are the smallest that flip each decision (tests/test_gpu_ring_launch.py: 70 samples, and 64 x CUs + 70).
"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from smpl_nerf_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
L = _lib.load()
N_SMALL = 70
N_LARGE = 64 * torch.cuda.get_device_properties(DEV).multi_processor_count + N_SMALL
F16X3 = _lib.SPLIT_F16X3
NO_RAY_FOLD = 2          # include/smplnerf.h SNERF_FWD_NO_RAY_FOLD


def ok(rc):
    assert rc >= 0, (rc, L.snerf_last_error_string())
    return rc


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def zeros(n, dtype=torch.float32):
    return torch.zeros(int(n), dtype=dtype, device=DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def samples(seed, n):     # tests/test_gpu_ring_launch.py: _samples
    rng = np.random.default_rng(seed)
    return (rng.uniform(-2, 2, (n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32),
            rng.normal(size=(n, 4)).astype(np.float32))


def mlp_desc(width, add_dim=0, pos_freqs=10, pos_identity=0):
    return _lib.MlpDesc(8, width, pos_freqs, pos_identity, 4, 0, add_dim, 1 << 4, 1, 0)


def net_params(desc, seed):
    """Flat parameters of a size that keeps every activation of order one."""
    n = ok(L.snerf_mlp_param_floats(desc)) if isinstance(desc, _lib.MlpDesc) else ok(L.snerf_warp_param_floats(desc))
    rng = np.random.default_rng(seed)
    return dev((rng.standard_normal(n) * (1.5 / np.sqrt(desc.width))).astype(np.float32))


class Out:
    """Collects the digests of one call's output arrays; run() makes the call twice."""

    def __init__(self):
        self.lines = []

    def run(self, tag, call):
        a, b = call(), call()
        torch.cuda.synchronize()
        for name in a:
            da, db = (hashlib.sha256(t[name].cpu().numpy().tobytes()).hexdigest() for t in (a, b))
            nonzero = bool((a[name] != 0).any())
            self.lines.append(f"{tag:<58} {name:<10} {da}{'' if da == db else '  UNSTABLE'}{'' if nonzero else '  (all zero)'}")


def packed_fwd(desc, params, nsplit):
    if nsplit == 0:
        p = zeros(ok(L.snerf_mlp_packed_floats(desc)))
        ok(L.snerf_mlp_pack_f32(desc, ptr(params), ptr(p), None))
    else:
        p = zeros(ok(L.snerf_mlp_packed_bf16_bytes(desc, nsplit)), torch.uint8)
        ok(L.snerf_mlp_pack_bf16(desc, ptr(params), ptr(p), nsplit, None))
    return p


def train_sizes(desc, n):
    v = [ctypes.c_int64() for _ in range(4)]
    cnt = ctypes.c_int32()
    ok(L.snerf_mlp_train_sizes(desc, n, *[ctypes.byref(x) for x in v], ctypes.byref(cnt)))
    return [x.value for x in v]


def packed_bwd(desc, params, nsplit, input_grad, n):
    if nsplit == 0:
        p = zeros(train_sizes(desc, n)[2])
        ok(L.snerf_mlp_pack_t_f32(desc, ptr(params), ptr(p), input_grad, None))
    else:
        p = zeros(ok(L.snerf_mlp_packed_t_bf16_bytes(desc, nsplit, input_grad)), torch.uint8)
        ok(L.snerf_mlp_pack_t_bf16(desc, ptr(params), ptr(p), nsplit, input_grad, None))
    return p


def mlp_forward(out, tag, desc, n, seed, nsplit=0, spr=1, dps=0, train=False, encoded=False, workspace=False):
    params = net_params(desc, seed)
    packed = packed_fwd(desc, params, nsplit)
    pts, dirs, _ = samples(seed, n)
    rng = np.random.default_rng(seed + 1)
    add = dev(rng.standard_normal((n // spr, desc.add_dim)).astype(np.float32)) if desc.add_dim else None
    per_sample = dps & 1
    x, d = dev(pts), dev(dirs if per_sample else dirs[: n // spr])
    if encoded:
        row = 60 + 24 + desc.add_dim
        x = dev(rng.uniform(-1, 1, (n, row)).astype(np.float32))
    ws_bytes = ok(L.snerf_mlp_fold_workspace_bytes(desc, n, spr)) if workspace else 0
    act_floats = train_sizes(desc, n)[0]

    def call():
        raw, act, ws = zeros(n * 4), zeros(act_floats if train else 0), zeros(ws_bytes, torch.uint8)
        if encoded and train:
            ok(L.snerf_mlp_fwd_encoded_train_f32(desc, ptr(packed), ptr(x), n, row, ptr(raw), ptr(act), None))
        elif encoded:
            ok(L.snerf_mlp_fwd_encoded_f32(desc, ptr(packed), ptr(x), n, row, ptr(raw), None))
        elif nsplit and train:
            ok(L.snerf_mlp_fwd_train_bf16_f32(desc, ptr(packed), nsplit, ptr(x), ptr(d), dps, ptr(add), n, spr, ptr(raw), ptr(act), None))
        elif nsplit:
            ok(L.snerf_mlp_fwd_bf16_f32(desc, ptr(packed), nsplit, ptr(x), ptr(d), dps, ptr(add), n, spr, ptr(raw), None))
        elif train:
            ok(L.snerf_mlp_fwd_train_f32(desc, ptr(packed), ptr(x), ptr(d), dps, ptr(add), n, spr, ptr(raw), ptr(act), None))
        elif workspace:
            ok(L.snerf_mlp_fwd_ws_f32(desc, ptr(packed), ptr(x), ptr(d), dps, ptr(add), n, spr, ptr(raw), ptr(ws), ws_bytes, None))
        else:
            ok(L.snerf_mlp_fwd_f32(desc, ptr(packed), ptr(x), ptr(d), dps, ptr(add), n, spr, ptr(raw), None))
        return {"raw": raw, "act": act} if train else {"raw": raw}

    out.run(tag, call)


def mlp_backward(out, tag, desc, n, seed, nsplit=0, inputs=False):
    params = net_params(desc, seed)
    packed, packed_t = packed_fwd(desc, params, nsplit), packed_bwd(desc, params, nsplit, 1 if inputs else 0, n)
    pts, dirs, gout = samples(seed, n)
    x, d, d_raw = dev(pts), dev(dirs), dev(gout)
    act_floats, dy_floats, _, gpart_floats = train_sizes(desc, n)
    n_params = ok(L.snerf_mlp_param_floats(desc))

    def call():
        raw, act, dy, gpart, grad = zeros(n * 4), zeros(act_floats), zeros(dy_floats), zeros(gpart_floats), zeros(n_params)
        d_x, d_d = zeros(n * 3), zeros(n * 3)
        if nsplit:
            ok(L.snerf_mlp_fwd_train_bf16_f32(desc, ptr(packed), nsplit, ptr(x), ptr(d), 1, None, n, 1, ptr(raw), ptr(act), None))
            if inputs:
                ok(L.snerf_mlp_bwd_inputs_bf16_f32(desc, ptr(packed_t), nsplit, ptr(act), ptr(d_raw), ptr(x), ptr(d), 1, 1, n, ptr(dy),
                                                   ptr(gpart), ptr(grad), ptr(d_x), ptr(d_d), None))
            else:
                ok(L.snerf_mlp_bwd_bf16_f32(desc, ptr(packed_t), nsplit, ptr(act), ptr(d_raw), n, ptr(dy), ptr(gpart), ptr(grad), None))
        else:
            ok(L.snerf_mlp_fwd_train_f32(desc, ptr(packed), ptr(x), ptr(d), 1, None, n, 1, ptr(raw), ptr(act), None))
            if inputs:
                ok(L.snerf_mlp_bwd_inputs_f32(desc, ptr(packed_t), ptr(act), ptr(d_raw), ptr(x), ptr(d), 1, 1, n, ptr(dy), ptr(gpart),
                                              ptr(grad), ptr(d_x), ptr(d_d), None))
            else:
                ok(L.snerf_mlp_bwd_f32(desc, ptr(packed_t), ptr(act), ptr(d_raw), n, ptr(dy), ptr(gpart), ptr(grad), None))
        res = {"dy": dy, "flat_grad": grad}
        if inputs:
            res.update(d_x=d_x, d_dirs=d_d)
        return res

    out.run(tag, call)


def warp_sizes(desc, n):
    v = [ctypes.c_int64() for _ in range(4)]
    ok(L.snerf_warp_train_sizes(desc, n, *[ctypes.byref(x) for x in v]))
    return [x.value for x in v]


def warp_net(out, tag, width, pose_dim, n, spr, seed, mode):
    """mode: inference, fold (inference with the workspace), train (training forward and backward), bf16"""
    desc = _lib.WarpDesc(width, 10, 0, pose_dim)
    params = net_params(desc, seed)
    pts, _, gout = samples(seed, n)
    rng = np.random.default_rng(seed + 1)
    x, o = dev(pts), dev(rng.uniform(-1, 1, (n // spr, 3)).astype(np.float32))
    pose = dev(rng.standard_normal((n // spr, pose_dim)).astype(np.float32))
    d_warp = dev(gout[:, :3])
    if mode == "bf16":
        packed = zeros(ok(L.snerf_warp_packed_bf16_bytes(desc)), torch.uint8)
        ok(L.snerf_warp_pack_bf16(desc, ptr(params), ptr(packed), None))
    else:
        packed = zeros(ok(L.snerf_warp_packed_floats(desc)))
        ok(L.snerf_warp_pack_f32(desc, ptr(params), ptr(packed), None))
    act_floats, dy_floats, pt_floats, gpart_floats = warp_sizes(desc, n)
    packed_t = zeros(pt_floats)
    ok(L.snerf_warp_pack_t_f32(desc, ptr(params), ptr(packed_t), None))
    ws_bytes = ok(L.snerf_warp_fold_workspace_bytes(desc, n, spr)) if mode == "fold" else 0
    n_params = ok(L.snerf_warp_param_floats(desc))

    def call():
        w, wd, sd = zeros(n * 3), zeros(n * 3), zeros(n * 3)
        head = (desc, ptr(packed), ptr(x), ptr(pose), ptr(o), n, spr, ptr(w), ptr(wd), ptr(sd))
        res = {"warp": w, "warped": wd, "sdirs": sd}
        if mode == "bf16":
            ok(L.snerf_warp_fwd_bf16_f32(*head, None))
        elif mode == "fold":
            ws = zeros(ws_bytes, torch.uint8)
            ok(L.snerf_warp_fwd_ws_f32(*head, ptr(ws), ws_bytes, None))
        elif mode == "train":
            act, dy, gpart, grad = zeros(act_floats), zeros(dy_floats), zeros(gpart_floats), zeros(n_params)
            ok(L.snerf_warp_fwd_train_f32(*head, ptr(act), None))
            ok(L.snerf_warp_bwd_f32(desc, ptr(packed_t), ptr(act), ptr(d_warp), n, ptr(dy), ptr(gpart), ptr(grad), None))
            res.update(act=act, dy=dy, flat_grad=grad)
        else:
            ok(L.snerf_warp_fwd_f32(*head, None))
        return res

    out.run(tag, call)


def ray_batch(seed, B, Nc, Nf):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
    d = rng.normal(size=(B, 3)).astype(np.float32)
    z = np.sort(rng.uniform(0.5, 3.0, (B, Nc)).astype(np.float32), axis=1)
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).astype(np.float32)
    u = np.sort(rng.uniform(0, 1, (B, Nf)).astype(np.float32), axis=1)
    rgb = rng.uniform(0, 1, (B, 3)).astype(np.float32)
    return {k: dev(v) for k, v in dict(o=o, d=d, z=z, pts=pts, u=u, rgb=rgb).items()}


def render_and_train(out, B=64, Nc=8, Nf=8):
    desc, wdesc = mlp_desc(256), _lib.WarpDesc(256, 10, 0, 40)
    pc, pf, pw = net_params(desc, 11), net_params(desc, 12), net_params(wdesc, 13)
    b = ray_batch(14, B, Nc, Nf)
    pose = dev(np.random.default_rng(15).standard_normal((B, 40)).astype(np.float32))
    packed_w, packed_tw = zeros(ok(L.snerf_warp_packed_floats(wdesc))), zeros(warp_sizes(wdesc, B * (Nc + Nf))[2])
    ok(L.snerf_warp_pack_f32(wdesc, ptr(pw), ptr(packed_w), None))
    ok(L.snerf_warp_pack_t_f32(wdesc, ptr(pw), ptr(packed_tw), None))
    packed_w16 = zeros(ok(L.snerf_warp_packed_bf16_bytes(wdesc)), torch.uint8)
    ok(L.snerf_warp_pack_bf16(wdesc, ptr(pw), ptr(packed_w16), None))
    n_params, n_warp = ok(L.snerf_mlp_param_floats(desc)), ok(L.snerf_warp_param_floats(wdesc))
    N = Nc + Nf
    batch = _lib.NerfBatch(ptr(b["pts"]), ptr(b["o"]), ptr(b["d"]), ptr(b["z"]), ptr(b["rgb"]), ptr(b["u"]), None, None, None, B, Nc, Nf, 0)
    for prec in (0, 3):
        fc, ff = packed_fwd(desc, pc, prec), packed_fwd(desc, pf, prec)

        def render():
            ws = zeros(ok(L.snerf_render_rays_workspace_bytes(B, Nc, Nf)), torch.uint8)
            rgb, rgb_f, pts_f, dens = zeros(B * 3), zeros(B * 3), zeros(B * N * 3), zeros(B * N)
            ok(L.snerf_render_rays_f32(desc, ptr(fc), desc, ptr(ff), prec, ptr(b["pts"]), ptr(b["o"]), ptr(b["d"]), ptr(b["z"]),
                                       ptr(b["u"]), None, None, B, Nc, Nf, 0, ptr(ws), ptr(rgb), ptr(rgb_f), ptr(pts_f), ptr(dens), None))
            return {"rgb": rgb, "rgb_fine": rgb_f, "samples": pts_f, "densities": dens}

        def render_smpl():
            ws = zeros(ok(L.snerf_render_rays_smpl_workspace_bytes(B, Nc, Nf)), torch.uint8)
            rgb, rgb_f, dens = zeros(B * 3), zeros(B * 3), zeros(B * N)
            w_f, pts_f, wd_f = zeros(B * N * 3), zeros(B * N * 3), zeros(B * N * 3)
            ok(L.snerf_render_rays_smpl_f32(desc, ptr(fc), desc, ptr(ff), wdesc, ptr(packed_w16 if prec else packed_w), prec, ptr(b["pts"]),
                                            ptr(b["o"]), ptr(b["d"]), ptr(b["z"]), ptr(pose), ptr(b["u"]), None, None, B, Nc, Nf, 0, ptr(ws),
                                            ptr(rgb), ptr(rgb_f), ptr(w_f), ptr(pts_f), ptr(wd_f), ptr(dens), None))
            return {"rgb": rgb, "rgb_fine": rgb_f, "warp": w_f, "samples": pts_f, "warped": wd_f, "densities": dens}

        def train(smpl):
            tc, tf = (packed_bwd(desc, p, prec, 1 if smpl else 0, B * N) for p in (pc, pf))
            if smpl:
                ws = zeros(ok(L.snerf_smpl_nerf_train_workspace_bytes(desc, desc, wdesc, B, Nc, Nf, 0)), torch.uint8)
            else:
                ws = zeros(ok(L.snerf_nerf_train_workspace_bytes(desc, desc, B, Nc, Nf, 0)), torch.uint8)
            gc, gf, gw, loss, rgb, rgb_f = zeros(n_params), zeros(n_params), zeros(n_warp), zeros(3), zeros(B * 3), zeros(B * 3)
            nets = (desc, ptr(fc), ptr(tc), desc, ptr(ff), ptr(tf))
            if smpl:
                ok(L.snerf_smpl_nerf_train_grads_f32(*nets, wdesc, ptr(packed_w), ptr(packed_tw), prec, ctypes.byref(batch), ptr(pose), 0,
                                                     ptr(ws), ptr(gc), ptr(gf), ptr(gw), ptr(loss), ptr(rgb), ptr(rgb_f), None))
                return {"grad_c": gc, "grad_f": gf, "grad_warp": gw, "loss": loss, "rgb": rgb, "rgb_fine": rgb_f}
            ok(L.snerf_nerf_train_grads_f32(*nets, prec, ctypes.byref(batch), 0, ptr(ws), ptr(gc), ptr(gf), ptr(loss), ptr(rgb),
                                            ptr(rgb_f), None, None))
            return {"grad_c": gc, "grad_f": gf, "loss": loss, "rgb": rgb, "rgb_fine": rgb_f}

        out.run(f"render_rays B {B} Nc {Nc} Nf {Nf} precision {prec}", render)
        out.run(f"render_rays_smpl B {B} Nc {Nc} Nf {Nf} precision {prec}", render_smpl)
        out.run(f"nerf_train_grads B {B} Nc {Nc} Nf {Nf} precision {prec}", lambda: train(False))
        out.run(f"smpl_nerf_train_grads B {B} Nc {Nc} Nf {Nf} precision {prec}", lambda: train(True))


def main():
    out = Out()
    for width in (64, 128, 256, 320, 512):
        for n in (1, N_SMALL, N_LARGE):
            for encoded in (False, True):
                mlp_forward(out, f"mlp fwd width {width} n {n} {'encoded' if encoded else 'fused'}", mlp_desc(width), n, width + n % 97,
                            encoded=encoded)
    n_rays = (N_LARGE + 15) // 16 + 1
    d_add = mlp_desc(256, add_dim=6)
    mlp_forward(out, "mlp fwd width 256 add 6 rays of 16, workspace (fold)", d_add, 16 * n_rays, 21, spr=16, workspace=True)
    mlp_forward(out, "mlp fwd width 256 add 6 rays of 16, no workspace", d_add, 16 * n_rays, 21, spr=16)
    mlp_forward(out, "mlp fwd width 256 add 6 rays of 16, workspace, NO_RAY_FOLD", d_add, 16 * n_rays, 21, spr=16, dps=NO_RAY_FOLD,
                workspace=True)
    mlp_forward(out, "mlp fwd width 256 per-sample directions", mlp_desc(256), N_LARGE, 22, dps=1)
    for n in (N_SMALL, N_LARGE):
        mlp_forward(out, f"mlp fwd train width 256 n {n}", mlp_desc(256), n, 23, train=True)
        mlp_forward(out, f"mlp fwd train width 256 n {n} encoded", mlp_desc(256), n, 23, train=True, encoded=True)
    for nsplit in (2, 3, F16X3):
        mlp_forward(out, f"mlp fwd nsplit {nsplit} n {N_LARGE}", mlp_desc(256), N_LARGE, 24, nsplit=nsplit)
        mlp_forward(out, f"mlp fwd train nsplit {nsplit} n {N_LARGE}", mlp_desc(256), N_LARGE, 24, nsplit=nsplit, train=True)
    for n in (N_SMALL, N_LARGE):
        for inputs in (False, True):
            mlp_backward(out, f"mlp bwd width 256 n {n}{' + inputs' if inputs else ''}", mlp_desc(256), n, 31, inputs=inputs)
    mlp_backward(out, f"mlp bwd width 512 n {N_SMALL}", mlp_desc(512), N_SMALL, 32)
    mlp_backward(out, f"mlp bwd width 256 n {N_LARGE} + inputs, 8 position k-blocks", mlp_desc(256, pos_freqs=16, pos_identity=1), N_LARGE,
                 33, inputs=True)
    for nsplit in (2, 3, F16X3):
        for inputs in (False, True):
            mlp_backward(out, f"mlp bwd nsplit {nsplit} n {N_LARGE}{' + inputs' if inputs else ''}", mlp_desc(256), N_LARGE, 34,
                         nsplit=nsplit, inputs=inputs)
    n_w = 16 * n_rays
    for width, pose in ((128, 40), (256, 40), (128, 240)):
        for mode in ("inference", "fold", "train"):
            warp_net(out, f"warp width {width} pose {pose} n {n_w} {mode}", width, pose, n_w, 16, 41, mode)
    warp_net(out, f"warp width 256 pose 40 n {N_SMALL} inference", 256, 40, N_SMALL, 1, 42, "inference")
    warp_net(out, f"warp width 256 pose 40 n {n_w} bf16", 256, 40, n_w, 16, 41, "bf16")
    render_and_train(out)
    print("\n".join(out.lines))
    unstable = sum("UNSTABLE" in ln for ln in out.lines)
    print(f"# {len(out.lines)} arrays, {unstable} unstable", file=sys.stderr)


if __name__ == "__main__":
    main()
