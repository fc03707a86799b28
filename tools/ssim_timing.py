"""Measurement: the image scores (ops.ssim = snerf_ssim_fwd_f32 / snerf_ssim_bwd_f32) on 100 frames of 128 x 128 x 3 and of
256 x 256 x 3, k = 11 - forward (the call of ops.image_scores: ssim, cs, sqerr), one backward (dx), and the step of a D-SSIM loss
(forward, dx) - next to the same scores in torch ops on the same GPU (five grouped conv2d and their autograd: tests/ssim_ref.py's
restatement).  Device events around windows of at least 0.3 s after warm-up; three windows per figure, the median and the spread.

    python tools/ssim_timing.py [--out FILE] [--frames 100] [--sizes 128 256] [--window 0.3]

Quoted in DESIGN.md section 8e; a run is kept in profiles/ssim_timing.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from smpl_nerf_amd import ops

K, SIGMA = 11, 1.5


def torch_ssim(x, y, G, c1, c2):
    """util/scores.py:152-173 in torch ops on [N,C,H,W]: per-channel ssim [N,C]."""
    C = x.shape[1]
    conv = lambda t: F.conv2d(t, weight=G, stride=1, padding=0, groups=C)      # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11, s22, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu1_mu2
    cs = (2 * s12 + c2) / (s11 + s22 + c2)
    return (((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1)) * cs).mean(dim=(-1, -2))


def window_ms(fn, seconds):
    """ms per call over a window of at least `seconds`: the call count comes from a first timed pass."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(5):
        fn()
    t1.record()
    torch.cuda.synchronize()
    reps = max(5, int(np.ceil(seconds * 1e3 / max(t0.elapsed_time(t1) / 5, 1e-3))))
    out = []
    for _ in range(3):
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    return float(np.median(out)), (max(out) - min(out)) / float(np.median(out)), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    win = torch.from_numpy(ops.ssim_window(K, SIGMA)).to(dev)
    G = (win[:, None] * win[None, :])[None, None].repeat(3, 1, 1, 1)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    lines = [f"image scores, {a.frames} frames x 3 channels, k = {K}, {torch.cuda.get_device_name(0)}; ms per call: the median of three "
             f"device-event windows of at least {a.window} s (spread = (max - min) / median), after warm-up"]
    for s in a.sizes:
        rng = np.random.default_rng(s)
        frames = rng.uniform(0, 1, (a.frames, s, s, 3)).astype(np.float32)
        r = torch.from_numpy(frames).to(dev)                                          # channels-last, as the trainer's frames lie
        t = (r + 0.05 * torch.randn_like(r)).clamp(0, 1)
        x, y = r.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2)
        xc, yc = x.contiguous(), y.contiguous()
        windows = a.frames * 3 * (s - K + 1) ** 2
        gs = torch.full((a.frames, 3), 1.0 / (3 * a.frames), device=dev)
        xg = xc.clone().requires_grad_(True)

        def step_hip():
            xg.grad = None
            (1 - ops.ssim(xg, yc)).backward()

        def step_torch():
            xg.grad = None
            (1 - torch_ssim(xg, yc, G, c1, c2).mean()).backward()

        with torch.no_grad():
            f_cl = window_ms(lambda: ops.image_scores(r, t), a.window)
            f_cf = window_ms(lambda: ops._ssim_fwd(xc, yc, win, c1, c2, True, True), a.window)
            b_cf = window_ms(lambda: ops._ssim_bwd(xc, yc, win, c1, c2, gs, None), a.window)
            b_cl = window_ms(lambda: ops._ssim_bwd(x, y, win, c1, c2, gs, None), a.window)
            f_t = window_ms(lambda: torch_ssim(xc, yc, G, c1, c2), a.window)
            agree = float((torch_ssim(xc, yc, G, c1, c2) - ops._ssim_fwd(xc, yc, win, c1, c2, False, False)[0]).abs().max())
        s_hip, s_t = window_ms(step_hip, a.window), window_ms(step_torch, a.window)
        fmt = lambda v: f"{v[0]:9.4f} ms  (spread {100 * v[1]:4.1f} %, {v[2]} calls per window)"      # noqa: E731
        lines += [f"{s} x {s}: {windows:.3e} windows, {a.frames * 3 * s * s * 8 / 1e6:.1f} MB of input",
                  f"  forward, channels-first (ssim, cs, sqerr)        {fmt(f_cf)}   {windows / f_cf[0] * 1e3:.3e} windows/s",
                  f"  image_scores on channels-last frames             {fmt(f_cl)}   (the forward and torch's ops on [N,3] results)",
                  f"  backward to one image, channels-first            {fmt(b_cf)}   {windows / b_cf[0] * 1e3:.3e} windows/s",
                  f"  backward to one image, channels-last             {fmt(b_cl)}",
                  f"  1 - ssim and its gradient to x (forward + backward) {fmt(s_hip)}",
                  f"  torch ops, forward (five grouped conv2d)         {fmt(f_t)}   = {f_t[0] / f_cf[0]:.1f} x the kernel; max |difference| {agree:.2e}",
                  f"  torch ops, 1 - ssim and its gradient to x        {fmt(s_t)}   = {s_t[0] / s_hip[0]:.1f} x the kernels"]
        # which bound: the counts per forward window are read off csrc/ssim.hip at k = 11, not measured
        cus, ghz, valu, lds_r, lds_w = torch.cuda.get_device_properties(0).multi_processor_count, 2.4, 240, 27, 10
        clocks = f_cf[0] * 1e-3 * ghz * 1e9 * cus / windows
        lines += [f"  forward per window and CU: {clocks:.2f} clocks at {ghz} GHz x {cus} CUs; read off the source: {valu} vector instructions "
                  f"= {valu / 128:.2f} clocks (128 lanes per clock), {lds_r} LDS words read + {lds_w} written = {lds_r / 32 + lds_w / 16:.2f} clocks "
                  f"(32 / 16 words per clock), {a.frames * 3 * s * s * 8 / f_cf[0] / 1e9:.2f} TB/s of input -> VALU is the nearest bound, at "
                  f"{valu / 128 / clocks:.2f} of it"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
