"""Measurement: LPIPS as a loss - forward plus backward to the rendered frame (ops.lpips_loss: snerf_lpips_fwd_f32, then
snerf_lpips_bwd_f32, which walks the stack forward again and back) at VGG16's full width on 1 and 100 frame pairs of 128 x 128 and of
256 x 256, next to the same stack in eager torch ops under autograd on the same GPU in the same run.  tools/lpips_timing.py's method:
device events around windows of at least 0.3 s after warm-up; three repetitions per figure, the two paths interleaved; the median
and the spread of each.  Also the peak memory of either path on every case, and the workspace one pair needs.

    python tools/lpips_bwd_timing.py [--out FILE] [--frames 1 100] [--sizes 128 256] [--window 0.3]

Quoted in DESIGN.md section 8k; a run is kept in profiles/lpips_bwd_timing.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from lpips_timing import CHANNELS, interleaved_ms, make_net, peak_mb, torch_lpips
from smpl_nerf_amd import _lib, ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 100])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bwd_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    net = make_net(dev)
    lib = _lib.load()
    lines = []

    def emit(*new):      # every line as it is measured: printed, and the file rewritten
        lines.extend(new)
        print("\n".join(new), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"LPIPS as a loss at full width {list(CHANNELS)}, {torch.cuda.get_device_name(0)}: the mean over the batch, forward plus backward to the "
         f"first frame; ms per call: the median of three device-event windows of at least {a.window} s (spread = (max - min) / median), device "
         "path and eager torch autograd interleaved, after warm-up")
    fmt = lambda v: f"{v[0]:10.4f} ms  (spread {100 * v[1]:4.1f} %, {v[2]} calls per window)"      # noqa: E731
    for s in a.sizes:
        for n in a.frames:
            rng = np.random.default_rng(s + n)
            x = torch.from_numpy(rng.uniform(0, 1, (n, 3, s, s)).astype(np.float32)).to(dev).requires_grad_(True)
            y = (x.detach() + 0.05 * torch.randn_like(x)).clamp(0, 1)

            def hip_step():
                x.grad = None
                ops.lpips_loss(x, y, net).backward()
                return x.grad

            def eager_step():
                x.grad = None
                torch_lpips(x, y, net).mean().backward()
                return x.grad

            hip, eager = interleaved_ms([hip_step, eager_step], a.window)
            got, want = hip_step().clone(), eager_step().clone()
            # the gradient of a ReLU / max-pool stack is discontinuous: where a pre-activation lies within fp32 rounding of zero (or two
            # values of a window of each other) two fp32 paths mask or route differently, and a patch the size of that unit's
            # receptive field differs - hence the median beside the maximum
            diff, top = (got - want).abs(), want.abs().max().clamp_min(1e-30)
            agree, typical = float(diff.max() / top), float(diff.median() / top)
            fixed, one = (lib.snerf_lpips_bwd_workspace_bytes(k, s, s, net.record(dev).channels) for k in (0, 1))
            pairs = max(1, min(n, (ops.LPIPS_WORKSPACE_BYTES - fixed) // (one - fixed)))
            m_hip, m_eager = peak_mb(hip_step), peak_mb(eager_step)
            emit(f"{n} frame pair(s) of {s} x {s}:",
                 f"  ops.lpips_loss, forward + backward    {fmt(hip)}   {n / hip[0] * 1e3:9.1f} pairs/s",
                 f"  eager torch ops under autograd        {fmt(eager)}   {n / eager[0] * 1e3:9.1f} pairs/s   = {eager[0] / hip[0]:.2f} x the device path; "
                 f"|difference| of the gradients / max |gradient|: median {typical:.2e}, max {agree:.2e}",
                 f"  peak memory above the inputs and weights: ops.lpips_loss {m_hip:.1f} MB ({pairs} pair(s) a chunk in the backward: "
                 f"{(fixed + pairs * (one - fixed)) / 1e6:.1f} MB of workspace; one pair needs {(one - fixed) / 1e6:.1f} MB and a call "
                 f"{fixed / 1e6:.1f} MB); eager torch {m_eager:.1f} MB = {m_eager / m_hip:.1f} x")
            del x, y, got, want, diff
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
