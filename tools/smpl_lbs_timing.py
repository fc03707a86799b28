"""Measurement: the SMPL body model (ops.smpl_lbs = snerf_smpl_lbs_fwd_f32 / _bwd_f32) with one pose per ray at the reference's
2048-ray batch and at a small one, forward and forward + backward, next to the same computation by the fp32 torch restatement
(tests/smpl_lbs_ref.py: what smplx runs, eager, with its [B,V,3,3] transforms) on the same GPU - ms and peak allocated memory - and
against the two rooflines of the chip; then one DynamicPipeline training step with the module against the same step with the torch
restatement as body model.  Event-timed after warm-up.

    python tools/smpl_lbs_timing.py [--out FILE] [--poses 2048 64] [--reps 20]

Quoted in DESIGN.md; a run is kept in profiles/smpl_lbs_timing.txt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import smpl_lbs_ref as SR
from smpl_nerf_amd import ops, synthetic as syn
from smpl_nerf_amd.body_model import SmplBodyModel
from smpl_nerf_amd.synthetic_smpl import IndexPoseEstimator, random_smpl_arrays

V, J, NB = 6890, 24, 10
K = NB + 9 * (J - 1)
HBM, FP32 = 8.0e12, 157.3e12          # bytes/s and vector fp32 FLOP/s of an MI355X (data sheet)


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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--poses", type=int, nargs="+", default=[2048, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-rays", type=int, default=2048)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smpl_lbs_timing: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    arrays = random_smpl_arrays(1, V, J, NB)
    model = SmplBodyModel.from_arrays(**arrays).to(dev)
    eager = SR.TorchBodyModel(arrays).to(dev)
    mb = model.kernel_buffers()
    model_bytes = sum(t.numel() * 4 for t in (model.v_template, model.blend, model.weights))
    lines = [f"SMPL linear blend skinning, V={V} J={J} NB={NB} (K={K}), one pose per ray, {torch.cuda.get_device_name(0)}; ms per call "
             f"(device events, {a.reps} calls after 2 warm-up calls); peak = torch.cuda.max_memory_allocated above the inputs, MB",
             f"rooflines: {HBM / 1e12:.0f} TB/s on the algorithmic bytes (B V 12 + the model, {model_bytes / 2 ** 20:.1f} MB, once), "
             f"{FP32 / 1e12:.1f} TFLOP/s (vector fp32) on 2 K 3V B FLOP (the blend contraction alone)"]
    for B in a.poses:
        full = torch.from_numpy(SR.poses(B, J, seed=2)).to(dev)
        pose, orient = full[:, 1:].reshape(B, -1).contiguous(), full[:, 0].contiguous()
        betas = torch.randn(B, NB, device=dev)
        dv = torch.randn(B, V, 3, device=dev)
        leaves = [t.clone().requires_grad_(True) for t in (betas, pose, orient)]

        def fwd_k():
            with torch.no_grad():
                return ops.smpl_lbs(mb, betas, pose, orient)[0]

        def fwd_t():
            with torch.no_grad():
                return SR.lbs(_arrays(eager), betas, pose, orient)[0]

        def both_k():
            for t in leaves:
                t.grad = None
            (ops.smpl_lbs(mb, *leaves)[0] * dv).sum().backward()

        def both_t():
            for t in leaves:
                t.grad = None
            (SR.lbs(_arrays(eager), *leaves)[0] * dv).sum().backward()

        def loss_only():          # what both forms share: the product with dv, its sum and that sum's backward
            x = dv.clone().requires_grad_(True)
            (x * dv).sum().backward()

        r = {n: (event_ms(f, a.reps), peak_mb(f)) for n, f in
             (("fwd_k", fwd_k), ("fwd_t", fwd_t), ("both_k", both_k), ("both_t", both_t), ("loss", loss_only))}
        agree = float((fwd_k() - fwd_t()).abs().max() / fwd_t().abs().max())
        bytes_io, flop = B * V * 12 + model_bytes, 2.0 * K * 3 * V * B
        f_ms, b_ms = r["fwd_k"][0], r["both_k"][0] - r["fwd_k"][0] - r["loss"][0]
        bw, fl = bytes_io / (f_ms * 1e-3) / HBM, flop / (f_ms * 1e-3) / FP32
        lines += [f"B={B}:",
                  f"  kernels, forward                      {r['fwd_k'][0]:9.3f} ms   peak {r['fwd_k'][1]:9.1f} MB   {bw:.3f} of {HBM / 1e12:.0f} TB/s, "
                  f"{fl:.3f} of the fp32 peak: nearer the {'compute' if fl > bw else 'bandwidth'} roofline",
                  f"  torch restatement, forward            {r['fwd_t'][0]:9.3f} ms   peak {r['fwd_t'][1]:9.1f} MB   = {r['fwd_t'][0] / r['fwd_k'][0]:.1f} x the kernels; "
                  f"max |difference| / max |vertex| {agree:.2e}",
                  f"  kernels, forward + backward           {r['both_k'][0]:9.3f} ms   peak {r['both_k'][1]:9.1f} MB   (torch's own product, sum and their backward: "
                  f"{r['loss'][0]:.3f} ms of it; backward alone ~{b_ms:.3f} ms: {bytes_io / (max(b_ms, 1e-6) * 1e-3) / HBM:.3f} of {HBM / 1e12:.0f} TB/s, "
                  f"{2 * flop / (max(b_ms, 1e-6) * 1e-3) / FP32:.3f} of the fp32 peak on its two contractions)",
                  f"  torch restatement, forward + backward {r['both_t'][0]:9.3f} ms   peak {r['both_t'][1]:9.1f} MB   = {r['both_t'][0] / r['both_k'][0]:.1f} x the kernels",
                  f"  peak memory, torch - kernels: forward {r['fwd_t'][1] - r['fwd_k'][1]:.1f} MB, with backward {r['both_t'][1] - r['both_k'][1]:.1f} MB; "
                  f"the [B,V,16] transform tensor is {B * V * 64 / 2 ** 20:.1f} MB"]
    lines += step_lines(dev, arrays, a.step_rays, a.reps)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def _arrays(m):
    d = {k: getattr(m, k) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
    d["parents"] = m.parents
    return d


def step_lines(dev, arrays, B, reps, S=64, images=10):
    """One DataParallelTrainer step of DynamicPipeline (net and estimator poses trained, autograd path) with either body model."""
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.pipelines import DynamicPipeline, PipelineArgs
    from smpl_nerf_amd.trainer import DataParallelTrainer
    data = syn.frame_batch(h=128, w=128, phi=4.0, theta=-20.0, seed=13, n_coarse=S)
    sub = (np.arange(B) * 7 + 3) % (128 * 128)
    idx = np.arange(B) % images
    batch = [torch.from_numpy(data[i][sub]).to(dev) for i in range(4)] + [torch.from_numpy(idx).to(dev), torch.from_numpy(data[4][sub]).to(dev)]
    poses = syn.human_poses((41, 38), 10, 60, images)
    out = []
    for name, body in (("SmplBodyModel (kernels)", SmplBodyModel.from_arrays(**arrays)), ("torch restatement", SR.TorchBodyModel(arrays))):
        net = RenderRayNet(8, 256, 60, 24, skips=[4])
        net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scene_net_params(401).items()})
        est = IndexPoseEstimator(torch.from_numpy(poses), torch.zeros(1, NB), trainable_poses=True)
        pipe = DynamicPipeline(net.to(dev), net, est.to(dev), body.to(dev), PipelineArgs(run_fine=1), ops.PositionalEncoder(10, 0), ops.PositionalEncoder(4, 0))
        tr = DataParallelTrainer(pipe, [pipe.model_coarse, pipe.smpl_estimator], lr=2e-5)
        ms, peak = event_ms(lambda: tr.step(batch), reps), peak_mb(lambda: tr.step(batch))
        out.append(f"  DynamicPipeline training step, {B} rays x {S} samples, body model = {name:24s} {ms:9.3f} ms   peak {peak:9.1f} MB")
        tr.close()
    return out


if __name__ == "__main__":
    main()
