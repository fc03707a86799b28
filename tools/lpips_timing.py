"""Measurement: LPIPS (ops.lpips = snerf_lpips_fwd_f32) at VGG16's full width on 1 and 100 frame pairs of 128 x 128 and of 256 x 256,
next to the same stack in eager torch ops (conv2d, relu, max_pool2d and the reference's normalisation and distance,
util/scores.py:356-411) on the same GPU in the same run.  Device events around windows of at least 0.3 s after warm-up; three
repetitions per figure, the two paths interleaved; the median and the spread of each.  Also the peak memory of either path on the
largest case.  The weights are seeded He-scaled normals: the time does not depend on their values.

    python tools/lpips_timing.py [--out FILE] [--frames 1 100] [--sizes 128 256] [--window 0.3]

Quoted in DESIGN.md section 8k; a run is kept in profiles/lpips_timing.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from smpl_nerf_amd import _lib, lpips, ops

CHANNELS = (64, 128, 256, 512, 512)


def make_net(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    convs, ci = [], 3
    for co, n in zip(CHANNELS, lpips.VGG16_STAGES):
        for _ in range(n):
            convs.append((torch.randn(co, ci, 3, 3, generator=g) * (2. / (9 * ci)) ** 0.5, 0.1 * torch.randn(co, generator=g)))
            ci = co
    return lpips.VggLpips(convs, [torch.randn(co, generator=g).abs() for co in CHANNELS]).to(dev)


def torch_lpips(x, y, net):
    """The reference's forward in eager torch ops: per-image loss [N]."""
    mean, std = (torch.tensor(v, device=x.device).view(1, -1, 1, 1) for v in (net.mean, net.std))

    def feats(v):
        v = (v - mean) / std
        out, i = [], 0
        for l, n in enumerate(lpips.VGG16_STAGES):
            for _ in range(n):
                v = F.relu(F.conv2d(v, getattr(net, f"conv{i}_weight"), getattr(net, f"conv{i}_bias"), padding=1))
                i += 1
            out.append(v / (torch.sqrt(torch.sum(v ** 2, dim=1, keepdim=True)) + 1e-10))
            if l < 4:
                v = F.max_pool2d(v, 2, 2)
        return out
    fx, fy = feats(x), feats(y)
    return torch.cat([(((a - b) ** 2) * getattr(net, f"lin{l}").view(1, -1, 1, 1)).mean(dim=[2, 3]) for l, (a, b) in enumerate(zip(fx, fy))],
                     dim=1).sum(dim=1)


def interleaved_ms(fns, seconds, repetitions=3):
    """ms per call of each of `fns`: `repetitions` windows of at least `seconds` each, the functions taking turns."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = []
    for fn in fns:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0.record()
        for _ in range(3):
            fn()
        t1.record()
        torch.cuda.synchronize()
        reps.append(max(3, int(np.ceil(seconds * 1e3 / max(t0.elapsed_time(t1) / 3, 1e-3)))))
    out = [[] for _ in fns]
    for _ in range(repetitions):
        for i, fn in enumerate(fns):
            t0.record()
            for _ in range(reps[i]):
                fn()
            t1.record()
            torch.cuda.synchronize()
            out[i].append(t0.elapsed_time(t1) / reps[i])
    return [(float(np.median(v)), (max(v) - min(v)) / float(np.median(v)), r) for v, r in zip(out, reps)]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 100])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    net = make_net(dev)
    lines = []

    def emit(*new):      # every line as it is measured: printed, and the file rewritten
        lines.extend(new)
        print("\n".join(new), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"LPIPS at full width {list(CHANNELS)}, {torch.cuda.get_device_name(0)}; ms per call: the median of three device-event windows of "
             f"at least {a.window} s (spread = (max - min) / median), device path and eager torch interleaved, after warm-up")
    fmt = lambda v: f"{v[0]:10.4f} ms  (spread {100 * v[1]:4.1f} %, {v[2]} calls per window)"      # noqa: E731
    with torch.no_grad():
        for s in a.sizes:
            for n in a.frames:
                rng = np.random.default_rng(s + n)
                x = torch.from_numpy(rng.uniform(0, 1, (n, 3, s, s)).astype(np.float32)).to(dev)
                y = (x + 0.05 * torch.randn_like(x)).clamp(0, 1)
                hip, eager = interleaved_ms([lambda: ops.lpips(x, y, net, reduction='none'), lambda: torch_lpips(x, y, net)], a.window)
                got, want = ops.lpips(x, y, net, reduction='none'), torch_lpips(x, y, net)
                agree = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
                emit(f"{n} frame pair(s) of {s} x {s}:",
                          f"  ops.lpips (snerf_lpips_fwd_f32)   {fmt(hip)}   {n / hip[0] * 1e3:9.1f} pairs/s",
                          f"  eager torch ops                   {fmt(eager)}   {n / eager[0] * 1e3:9.1f} pairs/s   = {eager[0] / hip[0]:.2f} x the device path; "
                     f"max relative difference {agree:.2e}")
        s, n = max(a.sizes), max(a.frames)
        x = torch.rand(n, 3, s, s, device=dev)
        y = (x + 0.05 * torch.randn_like(x)).clamp(0, 1)
        one = _lib.load().snerf_lpips_workspace_bytes(1, s, s, net.record(dev).channels)
        pairs = max(1, min(n, ops.LPIPS_WORKSPACE_BYTES // one))
        m_hip, m_eager = peak_mb(lambda: ops.lpips(x, y, net, reduction='none')), peak_mb(lambda: torch_lpips(x, y, net))
        emit(f"peak memory above the inputs and weights, {n} pairs of {s} x {s}: ops.lpips {m_hip:.1f} MB (the workspace of {pairs} pairs a chunk: "
                  f"{pairs * one / 1e6:.1f} MB of the {ops.LPIPS_WORKSPACE_BYTES / 1e6:.0f} MB cap; one pair needs {one / 1e6:.1f} MB); "
             f"eager torch {m_eager:.1f} MB = {m_eager / m_hip:.1f} x")


if __name__ == "__main__":
    main()
