#!/usr/bin/env python3
"""Golden vectors for SingleSamplePipeline (models/singe_sample_pipeline.py, SmplPipeline) from the reference itself, on the CPU.
    python tests/golden/make_golden_single_sample.py    # writes g21_single_sample.npz
The inputs are rebuilt from seeds by tests/single_sample_ref.py (g21_inputs): 130 rays with one sample each and a warp that moves
every third one, the net from a seed.  The file holds the seeds' table and what the reference computed: rgb and the MSE loss."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import make_golden as MG
import single_sample_ref as SS

t = MG.t


def main():
    U, RenderRayNet, _, _, _ = MG._import_reference()
    from models.singe_sample_pipeline import SmplPipeline
    batch_np, params = SS.g21_inputs()
    batch = [t(a) for a in batch_np]
    net = MG.load_params(RenderRayNet(8, 256, 60, 24, skips=[4]), params)
    pipe = SmplPipeline(net, MG.Args(run_fine=0), U.PositionalEncoder(10, 0), U.PositionalEncoder(4, 0))
    with torch.no_grad():
        rgb, rgb2 = pipe(batch)
    assert rgb is rgb2 and tuple(rgb.shape) == (SS.G21["B"], 3)
    loss = torch.nn.functional.mse_loss(rgb, batch[5])
    moved = (batch[4].abs().amax(-1) > 0).float().mean().item()
    print("loss", loss.item(), "share of rays moved", moved, "rgb std", float(rgb.std()))
    assert 0.3 <= moved <= 0.37
    MG.save("g21_single_sample.npz", config=np.array(json.dumps(SS.G21)), rgb=rgb.numpy(), loss=np.array([loss.item()]))


if __name__ == "__main__":
    main()
