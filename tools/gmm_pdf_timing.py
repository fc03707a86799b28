"""Measurement: the Gaussian-mixture pdf of SmplNerfSolver's canonical-density loss (ops.gaussian_mixture_pdf =
snerf_gmm_pdf_f32) at a training batch and at the reference's quick-start batch, with and without the sample gradient, next to the
same forward in eager torch on the GPU (chunked over samples so that its [samples, V, 3] tensor fits: what an unmodified solver would
run) and to the fine RenderRayNet forward of the same batch.  Event-timed after warm-up.

    python tools/gmm_pdf_timing.py [--out FILE] [--rays 4096 64] [--reps 20]

Quoted in DESIGN.md; a run is kept in profiles/gmm_pdf_timing.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from smpl_nerf_amd import ops, synthetic as syn
from smpl_nerf_amd.nets import RenderRayNet

S, V, STD = 192, 6890, 0.07       # 64 + 128 samples per ray, the SMPL vertex count, the parser's gmm_std


def inputs(B, dev, seed=1):
    """Means ~ N(0, 0.3) (a body-sized cloud), samples in their box, every other one within a std of a mean, ray origins."""
    rng = np.random.default_rng(seed)
    means = rng.normal(0, 0.3, (V, 3)).astype(np.float32)
    samples = rng.uniform(-0.6, 0.6, (B, S, 3)).astype(np.float32)
    near = means[rng.integers(0, V, (B, S))] + rng.normal(0, STD, (B, S, 3)).astype(np.float32)
    mask = (np.arange(S)[None, :] + np.arange(B)[:, None]) % 2 == 0
    samples[mask] = near[mask]
    ray_o = rng.normal(0, 2.0, (B, 3)).astype(np.float32)
    return [torch.from_numpy(a).to(dev) for a in (samples, means, ray_o)]


def eager(x, mu, rows):
    """utils.py:105-110 in torch ops, `rows` samples at a time."""
    var = STD ** 2
    factor = 1 / np.sqrt((2 * np.pi) ** 3 * var ** 3)
    flat, out = x.reshape(-1, 3), []
    for i in range(0, flat.shape[0], rows):
        diff = flat[i:i + rows, None, :] - mu[None, :, :]
        probs = factor * torch.exp(-0.5 * torch.sum(diff ** 2, dim=-1) / var)
        out.append(torch.sum(probs, dim=-1) / probs.shape[-1])
    return torch.cat(out).reshape(x.shape[:-1])


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
    ap.add_argument("--eager-rows", type=int, default=4096, help="samples per chunk of the eager form (4096 rows: a 0.34 GB [4096,6890,3] difference)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gmm_pdf_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    net = RenderRayNet(8, 256, 60, 24, skips=[4])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scene_net_params(401).items()})
    net = net.to(dev)
    enc = (ops.PositionalEncoder(10, 0), ops.PositionalEncoder(4, 0))
    lines = [f"Gaussian-mixture pdf, S={S} V={V} std={STD}, {torch.cuda.get_device_name(0)}; "
             f"ms per call (device events, {a.reps} calls after 2 warm-up calls)"]
    for B in a.rays:
        x, mu, o = inputs(B, dev)
        pairs = B * S * V
        with torch.no_grad():
            fwd = event_ms(lambda: ops.gaussian_mixture_pdf(x, mu, STD), a.reps)
            grad = event_ms(lambda: ops._gmm_launch(x, mu, STD, True), a.reps)
            pdf = ops.gaussian_mixture_pdf(x, mu, STD)
            eag = event_ms(lambda: eager(x, mu, a.eager_rows), max(2, a.reps // 10))
            agree = float((eager(x, mu, a.eager_rows) - pdf).abs().max() / pdf.abs().max())
            sdirs = (x - o[:, None, :]).reshape(-1, 3).contiguous()
            mlp = event_ms(lambda: net.forward_fused(x.reshape(-1, 3), sdirs, S, *enc), a.reps)
        xg = x.clone().requires_grad_(True)
        target = torch.rand(B, S, device=dev)

        def loss_step():
            xg.grad = None
            torch.nn.functional.mse_loss(ops.gaussian_mixture_pdf(xg, mu, STD), target).backward()

        step = event_ms(loss_step, a.reps)
        lines += [f"B={B}: {pairs:.3e} pairs",
                  f"  forward, pdf only (inference)          {fwd:9.3f} ms   {pairs / fwd * 1e3:.3e} pairs/s",
                  f"  forward, pdf and dpdf (training)       {grad:9.3f} ms   {pairs / grad * 1e3:.3e} pairs/s",
                  f"  mse_loss(pdf, target) and its backward {step:9.3f} ms   (the kernel once, then torch's own ops)",
                  f"  eager torch, {a.eager_rows} samples per chunk      {eag:9.3f} ms   = {eag / fwd:.1f} x the kernel; max |difference| / max pdf {agree:.2e}",
                  f"  fine RenderRayNet forward, same batch  {mlp:9.3f} ms   pdf / MLP = {fwd / mlp:.2f}, with dpdf {grad / mlp:.2f}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
