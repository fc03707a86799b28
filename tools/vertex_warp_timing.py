"""Measurement: the vertex-attention warp of DynamicPipeline (ops.vertex_attention_warp) at a training batch and at a small one,
next to the same computation in eager torch on the GPU (chunked over rays so that its [rays, S, V] tensors fit: what a user had to
write before the op existed) and to the pipeline's MLP forward on the same batch.  Event-timed after warm-up.

    python tools/vertex_warp_timing.py [--out FILE] [--rays 4096 64] [--reps 20]

Quoted in DESIGN.md; a run is kept in profiles/vertex_warp_timing.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from smpl_nerf_amd import ops, synthetic as syn
from smpl_nerf_amd.nets import RenderRayNet

S, V, RADIUS, TEMPERATURE = 64, 6890, 0.01, 10000.0


def inputs(B, dev, seed=1):
    """Bodies ~ N(0, 0.3), samples in their box, every third one planted within the radius of a goal vertex (as in the tests)."""
    rng = np.random.default_rng(seed)
    goal = rng.normal(0, 0.3, (B, V, 3)).astype(np.float32)
    canon = rng.normal(0, 0.3, (B, V, 3)).astype(np.float32)
    samples = rng.uniform(-0.6, 0.6, (B, S, 3))
    vid = rng.integers(0, V, (B, S))
    planted = goal[np.arange(B)[:, None], vid] + rng.normal(0, 0.4 * RADIUS, (B, S, 3))
    mask = (np.arange(S)[None, :] + np.arange(B)[:, None]) % 3 == 0
    samples[mask] = planted[mask]
    ray_o = rng.normal(0, 2.0, (B, 3)).astype(np.float32)
    return [torch.from_numpy(a).to(dev) for a in (samples.astype(np.float32), goal, canon, ray_o)]


def eager(p, g, c, o, rays_per_chunk):
    """models/dynamic_pipeline.py:51-70 in torch ops with the per-sample maximum taken out, a chunk of rays at a time."""
    outs = []
    for i in range(0, p.shape[0], rays_per_chunk):
        pp, gg, cc = p[i:i + rays_per_chunk], g[i:i + rays_per_chunk], c[i:i + rays_per_chunk]
        x = TEMPERATURE * torch.relu(RADIUS - torch.norm(pp[:, :, None, :] - gg[:, None, :, :], dim=-1))
        m = x.max(dim=-1, keepdim=True)[0].detach()
        e = torch.exp(x - m)
        a = (e - torch.exp(-m)) / e.sum(dim=-1, keepdim=True)
        outs.append((a[..., None] * (cc - gg)[:, None, :, :]).sum(dim=-2))
    warp = torch.cat(outs)
    warped = p + warp
    return warp, warped, warped - o[:, None, :]


def event_ms(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
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
    ap.add_argument("--rays", type=int, nargs="+", default=[4096, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--eager-chunk", type=int, default=32, help="rays per chunk of the eager form (32 rays: a 0.17 GB [32,64,6890,3] difference and several 56 MB [32,64,6890] temporaries)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vertex_warp_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    net = RenderRayNet(8, 256, 60, 24, skips=[4])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scene_net_params(401).items()})
    net = net.to(dev)
    enc = (ops.PositionalEncoder(10, 0), ops.PositionalEncoder(4, 0))
    lines = [f"vertex-attention warp, S={S} V={V} radius={RADIUS} temperature={TEMPERATURE}, {torch.cuda.get_device_name(0)}; "
             f"ms per call (device events, {a.reps} calls after 2 warm-up calls)"]
    for B in a.rays:
        p, g, c, o = inputs(B, dev)
        pairs = B * S * V
        with torch.no_grad():
            fwd = event_ms(lambda: ops.vertex_attention_warp(p, g, c, o, RADIUS, TEMPERATURE), a.reps)
            warp, warped, sdirs = ops.vertex_attention_warp(p, g, c, o, RADIUS, TEMPERATURE)
            mlp = event_ms(lambda: net.forward_fused(warped, sdirs, S, *enc), a.reps)
            eag = event_ms(lambda: eager(p, g, c, o, a.eager_chunk), max(2, a.reps // 10))
            ew = eager(p, g, c, o, a.eager_chunk)[0]
            agree = float((ew.reshape(-1, 3) - warp).abs().max() / ew.abs().max())
        gg, cc = g.clone().requires_grad_(True), c.clone().requires_grad_(True)
        dw = torch.randn(B * S, 3, device=dev)

        def train(samples_too=False):
            pp = p.clone().requires_grad_(samples_too)
            out = ops.vertex_attention_warp(pp, gg, cc, o, RADIUS, TEMPERATURE)
            gg.grad = cc.grad = None
            (out[0] * dw).sum().backward()

        with torch.no_grad():
            fwd_stats = event_ms(lambda: ops._vertex_warp_launch(p, g, c, o, RADIUS, TEMPERATURE, True), a.reps)
        both = event_ms(train, a.reps)
        both_s = event_ms(lambda: train(True), a.reps)
        hit = float((warp.abs().amax(-1) > 0).float().mean())
        lines += [f"B={B}: {pairs:.3e} pairs, {hit:.2f} of the samples have a vertex in radius",
                  f"  forward (inference, no stats)        {fwd:9.3f} ms   {pairs / fwd * 1e3:.3e} pairs/s",
                  f"  forward (with stats)                 {fwd_stats:9.3f} ms",
                  f"  forward + backward (vertex grads)    {both:9.3f} ms   backward alone ~{both - fwd_stats:.3f} ms (incl. torch's own ops of the step)",
                  f"  forward + backward (+ d_samples)     {both_s:9.3f} ms",
                  f"  eager torch, {a.eager_chunk} rays per chunk, forward {eag:9.3f} ms   = {eag / fwd:.1f} x the kernel; max |difference| / max |warp| {agree:.2e}",
                  f"  RenderRayNet forward, same batch     {mlp:9.3f} ms   warp / MLP = {fwd / mlp:.2f}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
