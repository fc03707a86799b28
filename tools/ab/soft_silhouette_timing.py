"""Measurement: ops.soft_silhouette (snerf_soft_silhouette_fwd_f32 / _bwd_f32) at one 128 x 128 and one 256 x 256 frame of the
13 776-face body stand-in (the triangle soup of tools/first_hit_timing.py: SMPL's face count and face size) at sigma = 1: forward,
and forward + backward, with the cull and without it; one whole fit iteration (LBS, silhouette, L1 loss, backward, Adam) on the
20 480-face surface body; and - in the same run - two yardsticks: ops.render_mesh on the same scene (the same walk with a cheaper
pair) and the torch restatement of the rule (tests/soft_silhouette_ref.py) in fp32 on the same GPU, forward + backward, at the
largest of 32, 64, 128 that fits in memory, with its peak memory beside the op's workspace.

All calls are timed interleaved, `--rounds` repetitions each, every one event-timed after warm-up over a window of 0.3 s or more.
Reported: every repetition, the median, and the spread (max - min) / median.

    python tools/ab/soft_silhouette_timing.py [--out FILE] [--reps 5] [--rounds 3]

Quoted in DESIGN.md; a run is kept in profiles/soft_silhouette_timing.txt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import soft_silhouette_ref as SS
import vertex_sphere_ref as SR
from smpl_nerf_amd import _lib, ops
from smpl_nerf_amd import synthetic as syn
from smpl_nerf_amd.body_model import SmplBodyModel
from smpl_nerf_amd.silhouette_fit import SilhouetteFitter
from smpl_nerf_amd.synthetic_smpl import smooth_texture, surface_smpl_arrays, surface_uv

FACES, ANGLE = 13776, np.pi / 3


def _window_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("soft_silhouette_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    pose = syn.sphere_pose(10.0, 25.0, 2.4)
    v, f = SR.triangle_soup(FACES, 5, pose[:3, 3])
    poses1, vg, fg, uvg, tex = T(pose[None]), T(v), T(f), T(surface_uv(v, 3)), T(smooth_texture(4))
    vgrad = vg.clone().requires_grad_(True)
    body = SmplBodyModel.from_arrays(**surface_smpl_arrays(3, level=5)).to(dev)
    focal = lambda side: float(.5 * side / np.tan(.5 * ANGLE))

    def fwd(side, cull):
        with torch.no_grad():
            return ops.soft_silhouette(poses1, focal(side), side, side, vg, fg, cull=cull, faces_checked=True)

    def both(side, cull):
        vgrad.grad = None
        ops.soft_silhouette(poses1, focal(side), side, side, vgrad, fg, cull=cull, faces_checked=True).sum().backward()
        return vgrad.grad

    def fit_step(side):
        fitter = SilhouetteFitter(body, pose[None], focal(side), side, side)
        with torch.no_grad():
            target = (fitter.silhouette(None, torch.full((1, 69), 0.1, device=dev)) > 0.5).float()
        state = torch.zeros(1, 69, device=dev, requires_grad=True)
        optim = torch.optim.Adam([state], lr=1e-2)

        def step():
            optim.zero_grad()
            fitter.loss(target, None, state).backward()
            optim.step()
        return step

    calls = {}
    for side in (128, 256):
        calls[f"{side}: render_mesh, cull (yardstick)"] = lambda side=side: ops.render_mesh(poses1, focal(side), side, side, vg, fg, uvg, tex, faces_checked=True)
        calls[f"{side}: render_mesh, no cull"] = lambda side=side: ops.render_mesh(poses1, focal(side), side, side, vg, fg, uvg, tex, cull=False, faces_checked=True)
        for cull in (True, False):
            calls[f"{side}: forward, {'cull' if cull else 'no cull'}"] = lambda side=side, cull=cull: fwd(side, cull)
            calls[f"{side}: forward + backward, {'cull' if cull else 'no cull'}"] = lambda side=side, cull=cull: both(side, cull)
        calls[f"{side}: fit iteration, 20480 faces"] = fit_step(side)

    # the torch restatement in fp32 on this GPU, forward + backward, at the largest size that fits
    restated, peak = None, 0
    for side in (128, 64, 32):
        try:
            def torch_both(side=side):
                x = vg.clone().requires_grad_(True)
                SS.silhouette(pose[None], focal(side), side, side, x, f, 1.0, 17.0, torch.float32).sum().backward()
                return x.grad
            torch.cuda.reset_peak_memory_stats()
            torch_both()
            torch.cuda.synchronize()
            restated, peak = side, torch.cuda.max_memory_allocated()
            calls[f"{side}: torch restatement fp32, forward + backward"] = torch_both
            calls[f"{side}: forward + backward, cull (beside the restatement)"] = lambda side=side: both(side, True)
            break
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()

    reps = {}
    for name, fn in calls.items():                    # warm-up, and the calls a 0.3 s window takes
        fn()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(a.reps, int(300.0 / max(_window_ms(fn, a.reps), 1e-3)) + 1)
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):                         # interleaved: a drift of the clocks meets all alike
        for name, fn in calls.items():
            ms[name].append(_window_ms(fn, reps[name]))
    same = all(bool(torch.equal(fwd(s, True), fwd(s, False))) and bool(torch.equal(both(s, True).clone(), both(s, False))) for s in (128, 256))
    covered = {s: float((fwd(s, True) > 0.5).float().mean()) for s in (128, 256)}
    lines = [f"soft silhouette at one frame of {FACES} faces, sigma = 1, {torch.cuda.get_device_name(0)}; ms per call: device events over windows of at "
             f"least 0.3 s after warm-up, {a.rounds} repetitions each, interleaved; pixels covered (S > 1/2): {covered}; cull and no cull equal "
             f"bit for bit, forward and gradient: {same}",
             f"{'':58s} {'repetitions (ms)':>{10 * a.rounds}s}   median ms   spread"]
    med = {}
    for name in calls:
        med[name] = float(np.median(ms[name]))
        lines.append(f"{name:58s} {''.join(f'{x:10.4f}' for x in ms[name])}   {med[name]:9.4f}   {(max(ms[name]) - min(ms[name])) / med[name]:.4f}")
    for side in (128, 256):
        y = med[f"{side}: render_mesh, cull (yardstick)"]
        lines.append(f"{side}: forward, cull / render_mesh, cull = {med[f'{side}: forward, cull'] / y:.3f}; forward, no cull / render_mesh, no cull = "
                     f"{med[f'{side}: forward, no cull'] / med[f'{side}: render_mesh, no cull']:.3f}; cull / no cull, forward = "
                     f"{med[f'{side}: forward, cull'] / med[f'{side}: forward, no cull']:.3f}")
    if restated:
        nbytes = _lib.load().snerf_soft_silhouette_workspace_bytes(1, len(v), FACES)
        r = med[f"{restated}: torch restatement fp32, forward + backward"] / med[f"{restated}: forward + backward, cull (beside the restatement)"]
        lines.append(f"torch restatement at {restated} x {restated}: peak memory {peak / 2 ** 30:.2f} GiB against a workspace of {nbytes / 2 ** 20:.2f} MiB; "
                     f"restatement / op, forward + backward = {r:.1f}")
    else:
        lines.append("torch restatement: does not fit at 32 x 32")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_out:
            f_out.write(text + "\n")


if __name__ == "__main__":
    main()
