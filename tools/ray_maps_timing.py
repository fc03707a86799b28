"""Measurement: the ray maps (ops.ray_maps = snerf_ray_maps_fwd_f32 / snerf_ray_maps_bwd_f32) on one 128 x 128 frame (16 384 rays x
192 samples) and on 100 such frames, forward and forward + backward, in the depths mode and in the points mode - next to, in the
same run, snerf_composite_fwd_f32 on the same shape (the yardstick: it streams 20 + 8 bytes per sample through the same scan) and
the rule in torch ops on the same GPU.  Device events around windows of at least 0.3 s after warm-up; every variant is measured
three times, the variants interleaved, and reported as the median with its spread.  Achieved bandwidth = the bytes the algorithm
needs per sample (computed here from the shapes) over the call's time.

    python tools/ray_maps_timing.py [--out FILE] [--frames 1 100] [--window 0.3]

Quoted in DESIGN.md 8m; a run is kept in profiles/ray_maps_timing.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from smpl_nerf_amd import _lib, ops

RAYS, N = 128 * 128, 192


def inputs(B, dev, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    raw = torch.randn(B, N, 4, device=dev, generator=g)
    raw[..., 3] *= 2.0
    z = torch.sort(2.0 + 4.0 * torch.rand(B, N, device=dev, generator=g), -1)[0]
    o = torch.randn(B, 3, device=dev, generator=g)
    d = torch.randn(B, 3, device=dev, generator=g)
    pts = o[:, None, :] + z[..., None] * d[:, None, :]
    return raw, z, o, d, pts


def torch_rule(alpha, o, d, z=None, pts=None):
    """The rule in fp32 torch ops (tests/ray_maps_ref.ray_maps), differentiable by autograd."""
    if pts is None:
        t = z
    else:
        t = ((pts - o[:, None, :]) * d[:, None, :]).sum(-1) / (d * d).sum(-1)[:, None]
    u = 1. - alpha + 1e-10
    w = alpha * torch.cumprod(torch.cat([torch.ones_like(u[:, :1]), u[:, :-1]], -1), -1)
    return w.sum(-1), (w * t).sum(-1), None if pts is None else (w[..., None] * pts).sum(-2)


def window_ms(fn, seconds):
    """ms per call of fn over one event-timed window of at least `seconds` (the count from a timed probe call)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    reps = max(3, int(seconds * 1e3 / max(t0.elapsed_time(t1), 1e-3)) + 1)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 100])
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ray_maps_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    lines = [f"ray maps, {N} samples per ray, {torch.cuda.get_device_name(0)}; ms per call: median of 3 interleaved windows of >= "
             f"{a.window} s (device events, after warm-up) [min .. max]; GB/s = algorithmic bytes per sample / time"]
    for frames in a.frames:
        B = RAYS * frames
        raw, z, o, d, pts = inputs(B, dev)
        with torch.no_grad():
            _, _, alpha = ops.composite(raw, z, d, False)
        ga, gd, gp = torch.randn(B, device=dev), torch.randn(B, device=dev), torch.randn(B, 3, device=dev)
        a_req = alpha.clone().requires_grad_(True)

        def composite_fwd():
            with torch.no_grad():
                ops.composite(raw, z, d, False)

        def fwd(**kw):
            def run():
                with torch.no_grad():
                    ops.ray_maps(alpha, o, d, **kw)
            return run

        def both(rule, **kw):
            def run():
                a_req.grad = None
                m = rule(a_req, o, d, **kw)
                loss = (m[0] * ga).sum() + (m[1] * gd).sum()
                if m[2] is not None:
                    loss = loss + (m[2] * gp).sum()
                loss.backward()
            return run

        def torch_fwd(**kw):
            def run():
                with torch.no_grad():
                    torch_rule(alpha, o, d, **kw)
            return run

        ops_rule = lambda al, o_, d_, z=None, pts=None: ops.ray_maps(al, o_, d_, z_vals=z, samples=pts)
        # name -> (callable, algorithmic bytes per sample; None: a composition of torch kernels, no single figure)
        variants = {
            "composite forward (raw 16 + z 4 read, weights 4 + alpha 4 written)": (composite_fwd, 28),
            "ray maps forward, depths (alpha 4 + z 4)": (fwd(z_vals=z), 8),
            "ray maps forward, points (alpha 4 + pts 12)": (fwd(samples=pts), 16),
            "ray maps forward + backward, depths (+ alpha 4 x 2 + z 4 + d alpha 4; torch's loss ops)": (both(ops_rule, z=z), 24),
            "ray maps forward + backward, points (+ alpha 4 x 2 + pts 12 + d alpha 4; torch's loss ops)": (both(ops_rule, pts=pts), 40),
            "torch ops forward, depths": (torch_fwd(z=z), None),
            "torch ops forward, points": (torch_fwd(pts=pts), None),
            "torch ops forward + backward, depths": (both(torch_rule, z=z), None),
            "torch ops forward + backward, points": (both(torch_rule, pts=pts), None),
        }
        for fn, _ in variants.values():      # warm-up of every shape and kernel the windows use
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(3):
            for k, (fn, _) in variants.items():
                times[k].append(window_ms(fn, a.window))
        lines.append(f"{frames} frame(s): {B} rays, {B * N:.3e} samples")
        med = {}
        for k, (fn, nbytes) in variants.items():
            lo, m, hi = sorted(times[k])
            med[k] = m
            bw = "" if nbytes is None else f"   {B * N * nbytes / m * 1e-6:8.1f} GB/s"
            lines.append(f"  {k:<92s} {m:9.4f} ms  [{lo:.4f} .. {hi:.4f}]{bw}")
        keys = list(variants)
        lines.append(f"  ray maps forward / composite forward: depths {med[keys[1]] / med[keys[0]]:.2f}, points {med[keys[2]] / med[keys[0]]:.2f};"
                     f"  torch ops / ray maps: forward {med[keys[5]] / med[keys[1]]:.1f} (depths) {med[keys[6]] / med[keys[2]]:.1f} (points),"
                     f" forward + backward {med[keys[7]] / med[keys[3]]:.1f} (depths) {med[keys[8]] / med[keys[4]]:.1f} (points)")
        del raw, z, o, d, pts, alpha, a_req, ga, gd, gp, variants
        torch.cuda.empty_cache()
    lines.append(f"C-ABI calls made: {_lib.CALLS}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
