#!/usr/bin/env python3
"""Golden vectors for DynamicPipeline (models/dynamic_pipeline.py) from the reference itself, with the synthetic body model /
index estimator standing in for smplx + the SMPL .pkl (1000 vertices: the reference builds [B, S, V] tensors).
    python tests/golden/make_golden_dynamic.py    # writes g17_dynamic.npz
The inputs are rebuilt from seeds by tests/vertex_warp_ref.py (g17_inputs); the file holds the seeds' table, the index arrays
and what the reference computed.  Case a: the parser's defaults (warp_radius 0.01, warp_temperature 10000) - forward outputs,
and whether the reference's own fp32 backward stayed finite (recorded, not asserted).  Case b: warp_temperature 2000, where it
does - forward outputs, the MSE loss and goal_poses.grad."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import make_golden as MG
import vertex_warp_ref as VR
from smpl_nerf_amd.synthetic_smpl import IndexPoseEstimator

t = MG.t


def main():
    U, RenderRayNet, _, _, _ = MG._import_reference()
    from models.dynamic_pipeline import DynamicPipeline
    batch_np, poses, body, params = VR.g17_inputs()
    pe, de = U.PositionalEncoder(10, 0), U.PositionalEncoder(4, 0)
    batch = [t(a) for a in batch_np]
    g = {"config": np.array(json.dumps(VR.G17)), "images": batch_np[4]}
    for case, temperature in VR.G17["cases"].items():
        net = MG.load_params(RenderRayNet(8, 256, 60, 24, skips=[4]), params)
        est = IndexPoseEstimator(t(poses), torch.zeros(1, 10), trainable_poses=True)
        args = MG.Args(run_fine=0, warp_radius=VR.G17["radius"], warp_temperature=temperature)
        pipe = DynamicPipeline(net, net, est, body, args, pe, de)
        pipe.global_orient, pipe.canonical_pose = torch.zeros([1, 3]), torch.zeros([1, 69])
        rgb, rgb2, warp, samples, warped, dens = pipe(batch)
        assert rgb is rgb2 and samples is batch[0]
        loss = torch.nn.functional.mse_loss(rgb, batch[5])
        loss.backward()
        grad = est.goal_poses.grad.numpy()
        for nm, o in (("rgb", rgb), ("warp", warp), ("warped", warped), ("densities", dens)):
            g[f"{case}_{nm}"] = o.detach().numpy()
        g[f"{case}_loss"] = np.array([loss.item()])
        g[f"{case}_grad_finite"] = np.array([int(np.isfinite(grad).all())])
        if case == "b":
            assert np.isfinite(grad).all(), "case b is the one whose reference gradient is meant to be finite"
            g["b_goal_poses_grad"] = grad
        print(case, "loss", loss.item(), "grad finite", bool(np.isfinite(grad).all()), "max|warp|", float(warp.abs().max()),
              "samples moved", int((warp.abs().amax(-1) > 0).sum()))
    MG.save("g17_dynamic.npz", **g)


if __name__ == "__main__":
    main()
