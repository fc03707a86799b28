#!/usr/bin/env python3
"""Golden vectors for VertexSpherePipeline (models/vertex_sphere_pipeline.py) from the reference itself, on the CPU.
    python tests/golden/make_golden_vertex_sphere.py    # writes g19_vertex_sphere.npz
The inputs are rebuilt from seeds by tests/vertex_sphere_ref.py (g19_inputs): a dozen rays x 64 samples with a warp that moves
every third sample, the net from a seed.  The file holds the seeds' table and what the reference computed: rgb, warped samples,
densities and the MSE loss."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import make_golden as MG
import vertex_sphere_ref as SR

t = MG.t


def main():
    U, RenderRayNet, _, _, _ = MG._import_reference()
    from models.vertex_sphere_pipeline import VertexSpherePipeline
    batch_np, params = SR.g19_inputs()
    pe, de = U.PositionalEncoder(10, 0), U.PositionalEncoder(4, 0)
    batch = [t(a) for a in batch_np]
    net = MG.load_params(RenderRayNet(8, 256, 60, 24, skips=[4]), params)
    pipe = VertexSpherePipeline(net, net, MG.Args(run_fine=0), pe, de)
    with torch.no_grad():
        rgb, rgb2, warp, samples, warped, dens = pipe(batch)
    assert rgb is rgb2 and samples is batch[0] and warp is batch[4]
    loss = torch.nn.functional.mse_loss(rgb, batch[5])
    moved = (batch[4].abs().amax(-1) > 0).float().mean().item()
    print("loss", loss.item(), "share of samples moved", moved, "max|warp|", float(batch[4].abs().max()))
    assert 0.3 <= moved <= 0.37
    MG.save("g19_vertex_sphere.npz", config=np.array(json.dumps(SR.G19)), rgb=rgb.numpy(), warped=warped.numpy(),
            densities=dens.numpy(), loss=np.array([loss.item()]))


if __name__ == "__main__":
    main()
