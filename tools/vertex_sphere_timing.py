"""Measurement: the two operators of the vertex_sphere data set at the size of one 128 x 128 image of the reference -
ops.ray_mesh_hits (snerf_ray_mesh_hits_f32) on 128^2 rays x 13 776 faces with K = 1 and K = 8, and ops.vertex_sphere_warp
(snerf_vertex_sphere_warp_f32) on 128^2 x 64 samples x 6890 vertices in both modes - as ms per call and achieved pairs per second,
next to the fp32 torch restatement of the same arithmetic (tests/vertex_sphere_ref.py) on the host CPU at a size that fits its
[rays, faces] / [samples, vertices] tensors.  That restatement is this project's own brute force, NOT trimesh (which the reference
calls one ray at a time and which is not installed here): it says what a vectorised CPU walk of the same pairs costs, nothing about
the reference's run time.  GPU calls are event-timed after warm-up over windows of 0.3 s or more; the CPU ones by the host clock.

    python tools/vertex_sphere_timing.py [--out FILE] [--reps 10]

Quoted in DESIGN.md and the README; a run is kept in profiles/vertex_sphere_timing.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import vertex_sphere_ref as SR
from smpl_nerf_amd import ops

RAYS, SAMPLES, FACES, VERTS = 128 * 128, 64, 13776, 6890
FP32 = 157.3e12          # vector fp32 FLOP/s of an MI355X (data sheet): 78.6e12 lane-instructions per second


def _window_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def event_ms(fn, reps, window_ms=300.0):
    """ms per call over at least `reps` calls and at least window_ms of device time (a call here is a fraction of a millisecond:
    ten of them would measure the clock), after two warm-up calls."""
    fn()
    fn()
    torch.cuda.synchronize()
    first = _window_ms(fn, reps)
    return _window_ms(fn, max(reps, int(window_ms / max(first, 1e-3)) + 1))


def host_ms(fn, reps=3):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-rays", type=int, default=256)
    ap.add_argument("--cpu-samples", type=int, default=2048)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vertex_sphere_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    T = torch.from_numpy
    cam = SR.camera_position(1)
    v, f = SR.triangle_soup(FACES, 5, cam)
    o, d = SR.camera_rays(RAYS, v, 1)
    lines = [f"vertex_sphere operators at one 128 x 128 image, {torch.cuda.get_device_name(0)}; ms per call (device events over at least {a.reps} calls and 0.3 s, "
             f"after warm-up), pairs = rays x faces or samples x vertices; CPU rows: the fp32 torch restatement (ours, not trimesh) on "
             f"{torch.get_num_threads()} host threads",
             f"lane-instruction peak of the chip {FP32 / 2 / 1e12:.1f}e12 /s: a pair costs about 45 (ray-mesh) or 10 (sphere warp) vector instructions"]
    og, dg, vg, fg = (T(x).to(dev) for x in (o, d, v, f))
    for K in (1, 8):
        ms = event_ms(lambda: ops.ray_mesh_hits(og, dg, vg, fg, K, faces_checked=True), a.reps)
        t, n = ops.ray_mesh_hits(og, dg, vg, fg, K)
        pairs = RAYS * FACES
        lines.append(f"ray_mesh_hits   {RAYS} rays x {FACES} faces, K={K}:      {ms:9.3f} ms   {pairs / ms / 1e6:8.1f} G pairs/s   "
                     f"(rays that hit {float((n > 0).float().mean()):.2f}, mean hits {float(n.float().mean()):.1f}, most {int(n.max())})")
    sub = slice(0, a.cpu_rays)
    oc, dc, vc = T(o[sub]), T(d[sub]), T(v)
    ms = host_ms(lambda: SR.ray_mesh_hits(oc, dc, vc, f, 8))
    t_cpu, n_cpu = SR.ray_mesh_hits(oc, dc, vc, f, 8)
    t_gpu, n_gpu = ops.ray_mesh_hits(og[sub], dg[sub], vg, fg, 8)
    lines.append(f"  CPU restatement {a.cpu_rays} rays x {FACES} faces, K=8:         {ms:9.3f} ms   {a.cpu_rays * FACES / ms / 1e6:8.3f} G pairs/s   "
                 f"(hit counts equal to the kernel's on {int((n_gpu.cpu().numpy() == n_cpu).sum())} of {a.cpu_rays} rays)")

    n_samples = RAYS * SAMPLES
    samples, goal, canon = SR.warp_inputs(n_samples, VERTS, 0.01, 1)
    sg, gg, cg = (T(x).to(dev) for x in (samples, goal, canon))
    for mean in (False, True):
        for radius in (0.01, 0.05):
            ms = event_ms(lambda: ops.vertex_sphere_warp(sg, gg, cg, radius, by_mean=mean), a.reps)
            w, i, k = ops.vertex_sphere_warp(sg, gg, cg, radius, by_mean=mean, want_indices=True)
            lines.append(f"vertex_sphere_warp {n_samples} samples x {VERTS} vertices, {'mean   ' if mean else 'nearest'} r={radius}: {ms:9.3f} ms   "
                         f"{n_samples * VERTS / ms / 1e6:8.1f} G pairs/s   (samples moved {float((w.abs().amax(-1) > 0).float().mean()):.3f})")
    sc, gc, cc = T(samples[:a.cpu_samples]), T(goal), T(canon)
    for mean in (False, True):
        ms = host_ms(lambda: SR.sphere_warp(sc, gc, cc, 0.01, mean))
        lines.append(f"  CPU restatement {a.cpu_samples} samples x {VERTS} vertices, {'mean   ' if mean else 'nearest'} r=0.01:   {ms:9.3f} ms   "
                     f"{a.cpu_samples * VERTS / ms / 1e6:8.3f} G pairs/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_out:
            f_out.write(text + "\n")


if __name__ == "__main__":
    main()
