"""Measurement: the image-wise model's warp (ops.image_wise_warp, ONE body for all rays) at a training batch and at a whole image,
next to the two things a user could do without it:
  (a) ops.vertex_attention_warp on the same samples with the body expanded to [B, V, 3] and the vertex gradients summed over B
      (another attention - a softmax - but the same pair walk, and the only per-ray kernel there was), and
  (b) the reference's expression in eager torch on the GPU, chunked over rays so that its [rays, S, V] tensors fit.
Every figure is the median of per-call device-event times after warm-up calls, with the spread (min .. max) of the same calls;
peak extra memory is torch's allocator peak over one call minus what was allocated before it.

    python tools/image_warp_timing.py [--out FILE] [--rays 4096 16384] [--reps 15]

Quoted in DESIGN.md; a run is kept in profiles/image_warp_timing.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from smpl_nerf_amd import _lib, ops

S, V, RADIUS, EPS, TEMPERATURE = 64, 6890, 0.01, 1e-5, 10000.0


def inputs(B, dev, seed=1):
    """One body ~ N(0, 0.3), samples in its box, every third one planted within the radius of a goal vertex (as in the tests)."""
    rng = np.random.default_rng(seed)
    goal = rng.normal(0, 0.3, (V, 3)).astype(np.float32)
    canon = rng.normal(0, 0.3, (V, 3)).astype(np.float32)
    samples = rng.uniform(-0.6, 0.6, (B, S, 3))
    vid = rng.integers(0, V, (B, S))
    planted = goal[vid] + rng.normal(0, 0.4 * RADIUS, (B, S, 3))
    mask = (np.arange(S)[None, :] + np.arange(B)[:, None]) % 3 == 0
    samples[mask] = planted[mask]
    ray_o = rng.normal(0, 2.0, (B, 3)).astype(np.float32)
    return [torch.from_numpy(a).to(dev) for a in (samples.astype(np.float32), goal, canon, ray_o)]


def eager(p, g, c, o, rays_per_chunk):
    """solver/image_wise_solver.py:89-105 in torch ops, a chunk of rays at a time."""
    outs = []
    for i in range(0, p.shape[0], rays_per_chunk):
        pp = p[i:i + rays_per_chunk]
        x = torch.relu(RADIUS - torch.norm(pp[:, :, None, :] - g[None, None, :, :], dim=-1))
        a = x / (x.sum(-1, keepdim=True) + EPS)
        outs.append((a[..., None] * (c - g)[None, None, :, :]).sum(dim=-2))
    warp = torch.cat(outs)
    warped = p + warp
    return warp, warped, warped - o[:, None, :]


def timed(fn, reps, warmup=2):
    """(median, min, max) ms over `reps` calls, one device-event pair per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms)), min(ms), max(ms)


def peak_extra_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def fmt(t):
    return f"{t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rays", type=int, nargs="+", default=[4096, 128 * 128])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--eager-chunk", type=int, default=32, help="rays per chunk of the eager form (32 rays: a 0.17 GB [32,64,6890,3] difference)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_warp_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = [f"image-wise warp, S={S} V={V} radius={RADIUS} eps={EPS}, {torch.cuda.get_device_name(0)}; median ms per call (min .. max) "
             f"of {a.reps} calls, one device-event pair each, after 2 warm-up calls"]
    for B in a.rays:
        p, g, c, o = inputs(B, dev)
        pairs = B * S * V
        dw = torch.randn(B * S, 3, device=dev)
        gg, cc = g.clone().requires_grad_(True), c.clone().requires_grad_(True)

        def train(samples_too=False):
            pp = p.clone().requires_grad_(samples_too)
            out = ops.image_wise_warp(pp, gg, cc, o, RADIUS, EPS)
            gg.grad = cc.grad = None
            (out[0] * dw).sum().backward()

        def per_ray(backward=True):      # yardstick (a)
            ge, ce = (t[None].expand(B, V, 3).contiguous().requires_grad_(backward) for t in (g, c))
            out = ops.vertex_attention_warp(p, ge, ce, o, RADIUS, TEMPERATURE)
            if backward:
                (out[0] * dw).sum().backward()
                return ge.grad.sum(0), ce.grad.sum(0)

        with torch.no_grad():
            fwd = timed(lambda: ops.image_wise_warp(p, g, c, o, RADIUS, EPS), a.reps)
            warp = ops.image_wise_warp(p, g, c, o, RADIUS, EPS)[0]
            fwd_a = timed(lambda: per_ray(False), a.reps)
            eag = timed(lambda: eager(p, g, c, o, a.eager_chunk), 3, warmup=1)
            ew = eager(p, g, c, o, a.eager_chunk)[0]
            agree = float((ew.reshape(-1, 3) - warp).abs().max() / ew.abs().max())
        both, both_s, both_a = timed(train, a.reps), timed(lambda: train(True), a.reps), timed(per_ray, a.reps)
        mem, mem_a = peak_extra_mb(train), peak_extra_mb(per_ray)
        ws = lib.snerf_image_warp_bwd_workspace_bytes(B * S, V)
        hit = float((warp.abs().amax(-1) > 0).float().mean())
        verdict = "no slower than (a) beyond (a)'s spread" if both[0] <= both_a[2] else "SLOWER than (a) beyond (a)'s spread"
        lines += [f"B={B}: {pairs:.3e} pairs, {hit:.2f} of the samples have a vertex in radius",
                  f"  forward (inference, no stats)             {fmt(fwd)}   {pairs / fwd[0] * 1e3:.3e} pairs/s",
                  f"  forward + backward (vertex grads)         {fmt(both)}   (incl. torch's own ops of the step)",
                  f"  forward + backward (+ d_samples)          {fmt(both_s)}",
                  f"  (a) per-ray op, body expanded: forward    {fmt(fwd_a)}",
                  f"  (a) forward + backward + sum over B       {fmt(both_a)}   ours is {verdict}: {both_a[0] / both[0]:.2f} x",
                  f"  (b) eager torch, {a.eager_chunk} rays per chunk, forward {fmt(eag)}   = {eag[0] / fwd[0]:.1f} x the kernel; max |difference| / max |warp| {agree:.2e}",
                  f"  peak extra memory of forward + backward: ours {mem:.1f} MB (workspace {ws / 2 ** 20:.1f} MB = slabs V 48 B, stats {B * S * 32 / 2 ** 20:.1f} MB = N 32 B), "
                  f"(a) {mem_a:.1f} MB (four [B, V, 3] tensors: {4 * B * V * 12 / 2 ** 20:.1f} MB)"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
