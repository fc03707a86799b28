"""Measurement: ops.ray_mesh_first_hit (snerf_ray_mesh_first_hit_f32), with and without `canon`, next to ops.ray_mesh_hits with
K = 1 (snerf_ray_mesh_hits_f32, the yardstick: the same walk over the same pairs, keeping one t per ray) at the size of one
128 x 128 image of the reference: 128^2 rays x 13 776 faces.  The three are timed interleaved, three repetitions each, every one
event-timed after warm-up over a window of 0.3 s or more.  Reported: the median of each, the ratio to the yardstick's median and
the yardstick's own spread (max - min) / median over its repetitions - a ratio inside 1 +- spread is no measured difference.

    python tools/first_hit_timing.py [--out FILE] [--reps 10] [--rounds 3]

Quoted in DESIGN.md and the README; a run is kept in profiles/first_hit_timing.txt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import single_sample_ref as SS
import vertex_sphere_ref as SR
from smpl_nerf_amd import ops

RAYS, FACES = 128 * 128, 13776


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
        raise SystemExit("first_hit_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    cam = SR.camera_position(1)
    v, f = SR.triangle_soup(FACES, 5, cam)
    o, d = SR.camera_rays(RAYS, v, 1)
    og, dg, vg, fg, cg = (torch.from_numpy(x).to(dev) for x in (o, d, v, f, SS.canon_of(v)))
    calls = {"ray_mesh_hits K=1": lambda: ops.ray_mesh_hits(og, dg, vg, fg, 1, faces_checked=True),
             "ray_mesh_first_hit": lambda: ops.ray_mesh_first_hit(og, dg, vg, fg, faces_checked=True),
             "ray_mesh_first_hit, canon": lambda: ops.ray_mesh_first_hit(og, dg, vg, fg, canon=cg, faces_checked=True)}
    reps = {}
    for name, fn in calls.items():                    # warm-up, and the calls a 0.3 s window takes
        fn()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(a.reps, int(300.0 / max(_window_ms(fn, a.reps), 1e-3)) + 1)
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):                         # interleaved: a drift of the clocks meets all three alike
        for name, fn in calls.items():
            ms[name].append(_window_ms(fn, reps[name]))
    t1, n1 = ops.ray_mesh_hits(og, dg, vg, fg, 1)
    t, face, uv, warp, depth = ops.ray_mesh_first_hit(og, dg, vg, fg, canon=cg)
    same = bool(torch.equal(t, t1[:, 0])) and bool(torch.equal(face >= 0, n1 > 0))
    yard = ms["ray_mesh_hits K=1"]
    med = float(np.median(yard))
    spread = (max(yard) - min(yard)) / med
    pairs = RAYS * FACES
    lines = [f"first hit at one 128 x 128 image ({RAYS} rays x {FACES} faces), {torch.cuda.get_device_name(0)}; ms per call: device events over windows of "
             f"at least 0.3 s after warm-up, {a.rounds} repetitions each, interleaved; rays that hit {float((face >= 0).float().mean()):.2f}; "
             f"t equal to the K=1 hit list's bit for bit: {same}",
             f"{'':28s} {'repetitions (ms)':>{9 * a.rounds}s}   median ms   G pairs/s   ratio to the yardstick"]
    for name in calls:
        m = float(np.median(ms[name]))
        lines.append(f"{name:28s} {''.join(f'{x:9.4f}' for x in ms[name])}   {m:9.4f}   {pairs / m / 1e6:9.1f}   {m / med:.4f}")
    lines.append(f"spread of the yardstick, (max - min) / median over its repetitions: {spread:.4f}")
    for name in list(calls)[1:]:
        ratio = float(np.median(ms[name])) / med
        lines.append(f"{name}: ratio {ratio:.4f} is {'inside' if abs(ratio - 1) <= spread else 'OUTSIDE'} 1 +- {spread:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_out:
            f_out.write(text + "\n")


if __name__ == "__main__":
    main()
