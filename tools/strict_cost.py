"""Measurement: what strict mode (args.strict_cumsum = 1, the sampler's normalising sum in torch's CPU order on the device) costs
against the default fp64 sum.  Default and strict run in alternating pairs, each bracketed by device events:

  * the single-call render of a 128 x 128 frame (64 + 128 samples, fp32);
  * the sampler at 16 384 rays: ops.hierarchical_samples, default against strict (the device sum, then the kernel that takes
    it), and snerf_reference_sum_f32 on its own;
  * the one-call training step at the reference's 64-ray batch.

    python tools/strict_cost.py [--pairs 20]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -d DIR -o strict -- python tools/strict_cost.py` (a separate run)
and read sample_pdf_kernel<..., false> / <..., true> from the stats.  Numbers quoted in DESIGN.md section 3.4."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from smpl_nerf_amd import _lib, ops
from smpl_nerf_amd import synthetic as syn
from smpl_nerf_amd.nets import RenderRayNet
from smpl_nerf_amd.ops import PositionalEncoder
from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs
from smpl_nerf_amd.trainer import DataParallelTrainer

dev = torch.device("cuda:0")


def net(p):
    m = RenderRayNet(8, 256, 60, 24, skips=[4])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return m.to(dev)


def pairs(fn_default, fn_strict, n, reps):
    """Alternating (default, strict) pairs of `reps` calls each, device events around each half; medians in ms per call."""
    for f in (fn_default, fn_strict):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res = ([], [])
    for _ in range(n):
        for k, f in enumerate((fn_default, fn_strict)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            res[k].append(e0.elapsed_time(e1) / reps)
    d, s = float(np.median(res[0])), float(np.median(res[1]))
    return d, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    a = ap.parse_args()
    assert ops.device_reference_sum_ok(), "strict mode would take the host round trip on this host"
    pc, pf = syn.make_scene_nets(101)
    enc = (PositionalEncoder(10, 0), PositionalEncoder(4, 0))

    # single-call render, 128 x 128 frame
    pipe = NerfPipeline(net(pc), net(pf), PipelineArgs(), *enc).eval()
    frame = [torch.from_numpy(x).to(dev) for x in syn.frame_batch(128, 128, seed=7)]

    def render(strict):
        def f():
            pipe.args.strict_cumsum = strict
            with torch.no_grad():
                pipe(frame)
        return f
    d, s = pairs(render(0), render(1), a.pairs, 5)
    print(f"render 128x128 (64+128, fp32, one call): default {d:.4f} ms  strict {s:.4f} ms  ratio {s / d:.4f}")

    # the sampler alone, 16 384 rays
    x, o, dd, z = frame[:4]
    B, Nc = z.shape
    with torch.no_grad():
        raw = pipe.model_coarse.forward_fused(x, dd, Nc, *enc)
        _, w, _ = ops.composite(raw.view(B, Nc, 4), z, dd, False)
    lib = _lib.load()
    tot = torch.empty(B, device=dev)
    wi = w[:, 1:-1]

    def refsum():
        lib.snerf_reference_sum_f32(wi.data_ptr(), wi.stride(0), B, Nc - 2, 1e-5, tot.data_ptr(), _lib.current_stream())
    d, s = pairs(lambda: ops.hierarchical_samples(o, dd, z, w, 128), lambda: ops.hierarchical_samples(o, dd, z, w, 128, strict=True),
                 a.pairs, 20)
    print(f"hierarchical_samples 16384 rays: default {d * 1e3:.1f} us  strict (sum + kernel) {s * 1e3:.1f} us  ratio {s / d:.4f}")
    d2, s2 = pairs(refsum, refsum, a.pairs, 50)
    print(f"snerf_reference_sum_f32 16384 rows of 62: {0.5 * (d2 + s2) * 1e3:.2f} us")

    # one-call training step, 64 rays
    batch = [torch.from_numpy(v[np.arange(0, 16384, 256)]).to(dev) for v in syn.frame_batch(128, 128, seed=7)]
    trs = []
    for strict in (0, 1):
        p2 = NerfPipeline(net(pc).train(), net(pf).train(), PipelineArgs(strict_cumsum=strict), *enc)
        trs.append(DataParallelTrainer(p2, [p2.model_coarse, p2.model_fine], lr=1e-5))
    d, s = pairs(lambda: trs[0].step(batch), lambda: trs[1].step(batch), a.pairs, 20)
    print(f"one-call training step, 64 rays: default {d:.4f} ms  strict {s:.4f} ms  ratio {s / d:.4f}")


if __name__ == "__main__":
    main()
