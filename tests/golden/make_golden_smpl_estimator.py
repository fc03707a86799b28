#!/usr/bin/env python3
"""Golden vectors for SmplEstimator (models/smpl_estimator.py:6-47) from the reference itself, eval mode, fp32, CPU.
    python tests/golden/make_golden_smpl_estimator.py    # writes g24_smpl_estimator.npz
The parameters are tests/smpl_estimator_ref.state(GOLDEN_SEED, human_size) loaded into the reference's module, the images
smpl_estimator_ref.images(GOLDEN_IMAGE_SEED, 2).  No weights are stored (fc1 alone is 16 MB): a test rebuilds them from the seed.
    out/2, out/69        the module's output [2, human_size]
    block/1 .. block/5   the [:, ::8, ::8] slice of each block's output for image 0 (what the next convolution, or the flatten, is given)
    keys, shapes         the module's state_dict: names, and shapes as rows of 4 padded with -1   (human_size 69)
Nothing of the reference is copied: the file holds arrays only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import make_golden as MG
import smpl_estimator_ref as ER


def main():
    sys.path.insert(0, MG.REF)
    from models.smpl_estimator import SmplEstimator
    torch.set_grad_enabled(False)
    x = torch.from_numpy(ER.images(ER.GOLDEN_IMAGE_SEED, ER.GOLDEN_N))
    g = {}
    for hs in (2, 69):
        model = SmplEstimator(hs)
        model.load_state_dict(ER.tensors(ER.state(ER.GOLDEN_SEED, hs)))
        model.eval()
        seen = {}
        hooks = [getattr(model, f"conv{i + 1}").register_forward_pre_hook(lambda m, a, i=i: seen.__setitem__(i, a[0])) for i in range(1, 5)]
        hooks.append(model.pool.register_forward_hook(lambda m, a, out: seen.__setitem__(5, out)))      # (the last call stays)
        g[f"out/{hs}"] = model(x).numpy()
        for h in hooks:
            h.remove()
        if hs == 69:
            for i in range(1, 6):
                g[f"block/{i}"] = np.ascontiguousarray(seen[i][0, :, ::8, ::8].numpy())
            sd = model.state_dict()
            g["keys"] = np.array(list(sd))
            g["shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()], np.int64)
        print(f"human_size {hs}: out {g[f'out/{hs}'].shape} max|out| {np.abs(g[f'out/{hs}']).max():.4f}")
    MG.save(ER.GOLDEN, **g)


if __name__ == "__main__":
    main()
