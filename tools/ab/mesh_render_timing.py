"""Measurement: ops.render_mesh (snerf_mesh_render_f32) at one 128 x 128 frame of the 13 776-face body stand-in (the triangle soup of
tools/first_hit_timing.py: SMPL's face count and face size), with the cull and without it, 100 frames in one call, and - in the same
run - the parent's path for one frame: RayGenerator.batch plus ops.ray_mesh_first_hit, and that first-hit call alone (the yardstick).
Also a closed surface (the bumpy ellipsoid at level 5, 20 480 faces), with and without the cull.

All calls are timed interleaved, `--rounds` repetitions each, every one event-timed after warm-up over a window of 0.3 s or more
(the method and the counts of tools/first_hit_timing.py).  Reported: the median of each, the ratio to the yardstick's median and the
yardstick's own spread (max - min) / median over its repetitions - a ratio inside 1 +- spread is no measured difference.

    python tools/ab/mesh_render_timing.py [--out FILE] [--reps 10] [--rounds 3]

Quoted in DESIGN.md and the README; a run is kept in profiles/mesh_render_timing.txt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import vertex_sphere_ref as SR
from smpl_nerf_amd import ops
from smpl_nerf_amd import synthetic as syn
from smpl_nerf_amd.raygen import RayGenerator
from smpl_nerf_amd.synthetic_smpl import smooth_texture, surface_uv

SIDE, FACES, FRAMES, ANGLE = 128, 13776, 100, np.pi / 3


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_render_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    pose = syn.sphere_pose(10.0, 25.0, 2.4)
    focal = float(.5 * SIDE / np.tan(.5 * ANGLE))
    v, f = SR.triangle_soup(FACES, 5, pose[:3, 3])
    vs, fs = SR.body_mesh(5, 5)
    poses1 = T(pose[None])
    poses100 = T(np.stack([syn.sphere_pose(10.0, 3.6 * k, 2.4) for k in range(FRAMES)]))
    vg, fg, uvg, tex = T(v), T(f), T(surface_uv(v, 3)), T(smooth_texture(4))
    vsg, fsg, uvsg = T(vs), T(fs), T(surface_uv(vs, 3))
    gen = RayGenerator(pose[None], SIDE, SIDE, ANGLE, 1.0, 4.0, 1, dev)
    index, jitter = torch.arange(SIDE * SIDE, device=dev), torch.zeros(SIDE * SIDE, device=dev, dtype=torch.float64)
    _, og, dg, _, _ = gen.batch(index, jitter)

    def parent():
        _, o, d, _, _ = gen.batch(index, jitter)
        return ops.ray_mesh_first_hit(o, d, vg, fg, faces_checked=True)

    calls = {"ray_mesh_first_hit alone": lambda: ops.ray_mesh_first_hit(og, dg, vg, fg, faces_checked=True),
             "raygen + ray_mesh_first_hit": parent,
             "render_mesh, cull": lambda: ops.render_mesh(poses1, focal, SIDE, SIDE, vg, fg, uvg, tex, faces_checked=True),
             "render_mesh, no cull": lambda: ops.render_mesh(poses1, focal, SIDE, SIDE, vg, fg, uvg, tex, cull=False, faces_checked=True),
             f"render_mesh, cull, {FRAMES} frames": lambda: ops.render_mesh(poses100, focal, SIDE, SIDE, vg, fg, uvg, tex, faces_checked=True),
             "surface 20480: first hit alone": lambda: ops.ray_mesh_first_hit(og, dg, vsg, fsg, faces_checked=True),
             "surface 20480: render, cull": lambda: ops.render_mesh(poses1, focal, SIDE, SIDE, vsg, fsg, uvsg, tex, faces_checked=True),
             "surface 20480: render, no cull": lambda: ops.render_mesh(poses1, focal, SIDE, SIDE, vsg, fsg, uvsg, tex, cull=False, faces_checked=True)}
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
    t, face, uv = ops.ray_mesh_first_hit(og, dg, vg, fg)
    culled = ops.render_mesh(poses1, focal, SIDE, SIDE, vg, fg, uvg, tex)
    brute = ops.render_mesh(poses1, focal, SIDE, SIDE, vg, fg, uvg, tex, cull=False)
    same_hit = bool(torch.equal(culled.t.view(-1), t)) and bool(torch.equal(culled.face.view(-1), face)) and bool(torch.equal(culled.bary.view(-1, 2), uv))
    same_cull = all(bool(torch.equal(x, y)) for x, y in zip(culled[:4], brute[:4]))
    yard = ms["ray_mesh_first_hit alone"]
    med = float(np.median(yard))
    spread = (max(yard) - min(yard)) / med
    lines = [f"mesh renderer at one {SIDE} x {SIDE} frame of {FACES} faces, {torch.cuda.get_device_name(0)}; ms per call: device events over windows "
             f"of at least 0.3 s after warm-up, {a.rounds} repetitions each, interleaved; pixels that hit {float((face >= 0).float().mean()):.2f}; "
             f"render t / face / bary equal to ray_mesh_first_hit's bit for bit: {same_hit}; cull and no cull equal bit for bit: {same_cull}",
             f"{'':36s} {'repetitions (ms)':>{10 * a.rounds}s}   median ms   ratio to the yardstick"]
    for name in calls:
        m = float(np.median(ms[name]))
        lines.append(f"{name:36s} {''.join(f'{x:10.4f}' for x in ms[name])}   {m:9.4f}   {m / med:.4f}")
    lines.append(f"spread of the yardstick (ray_mesh_first_hit alone), (max - min) / median over its repetitions: {spread:.4f}")
    m = {name: float(np.median(x)) for name, x in ms.items()}
    lines.append(f"render_mesh, cull against the yardstick: ratio {m['render_mesh, cull'] / med:.4f} - "
                 f"{'no slower' if m['render_mesh, cull'] <= med * (1 + spread) else 'SLOWER'} beyond the spread")
    lines.append(f"render_mesh, cull against no cull: ratio {m['render_mesh, cull'] / m['render_mesh, no cull']:.4f} - "
                 f"{'not slower' if m['render_mesh, cull'] <= m['render_mesh, no cull'] * (1 + spread) else 'SLOWER'}")
    lines.append(f"{FRAMES} frames in one call: {m[f'render_mesh, cull, {FRAMES} frames'] / FRAMES:.4f} ms per frame")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_out:
            f_out.write(text + "\n")


if __name__ == "__main__":
    main()
