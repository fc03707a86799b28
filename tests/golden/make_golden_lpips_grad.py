#!/usr/bin/env python3
"""Golden gradients for LPIPS as a loss (util/scores.py:286-411) from the reference itself: its ContentLoss under autograd, on the
VGG16-shaped nn.Sequential and the seeded weights of make_golden_lpips.py.
    python tests/golden/make_golden_lpips_grad.py    # writes g28_lpips_grad.npz
Per case of lpips_ref.CASES, with the seeded g_layers of lpips_bwd_ref.case_g (uniform in [0.5, 1.5]):
    <case>/checksum               lpips_ref.checksum of the case's weights
    <case>/g_layers               [N,5] fp32
    <case>/dx, <case>/dy          the float64 gradients of sum g_layers[n,l] layers[n,l] to the frames, layers[:, l] being one
                                  ContentLoss per tap (layers=(tap,), weights=[lin[l]], normalize_features=True, reduction='none')  [N,3,H,W]
    yardstick_grad                the largest E(fp32 gradient, float64 gradient) over the cases and both frames: what the reference's
                                  own fp32 backward is off by
The frames are not stored: lpips_ref.images regenerates them from the seeds.  Nothing of the reference is copied: arrays only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import lpips_bwd_ref as BR
import lpips_ref as LR
import make_golden as MG
from make_golden_lpips import sequential


def main():
    MG._stub("cv2")
    tv = MG._stub("torchvision")
    tv.models = MG._stub("torchvision.models", vgg16=None, vgg19=None)
    sys.path.insert(0, MG.REF)
    from util import scores as S
    g, worst = {}, 0.0
    for name, (channels, H, W, N, wseed, iseed, same) in LR.CASES.items():
        w = LR.weights(wseed, channels)
        x, y = LR.images(iseed, N, H, W, same)
        gl = BR.case_g(name)
        g[f"{name}/checksum"], g[f"{name}/g_layers"] = np.float64(LR.checksum(w)), gl
        grads = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            seq = sequential(w, dtype)
            lin = [torch.from_numpy(v).to(dtype).view(1, -1, 1, 1) for v in w["lin"]]
            xt, yt = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (x, y))
            cols = [S.ContentLoss(feature_extractor=seq, layers=(tap,), weights=[lin[l]], normalize_features=True, reduction='none')(xt, yt)
                    for l, tap in enumerate(LR.TAPS)]
            (torch.stack(cols, dim=1) * torch.from_numpy(gl).to(dtype)).sum().backward()
            assert xt.grad.dtype == dtype and all(p.grad is None for p in seq.parameters())      # the weights are frozen (scores.py:340)
            grads[tag] = (xt.grad.numpy(), yt.grad.numpy())
        g[f"{name}/dx"], g[f"{name}/dy"] = grads["f64"]
        assert np.isfinite(grads["f64"][0]).all() and np.isfinite(grads["f64"][1]).all() and np.isfinite(grads["f32"][0]).all()
        e = max(LR.E(grads["f32"][i], grads["f64"][i]) for i in (0, 1))
        worst = max(worst, e)
        print(f"{name}: max|dx| {np.abs(grads['f64'][0]).max():.3e}  max|dy| {np.abs(grads['f64'][1]).max():.3e}  E(f32 gradients) {e:.3e}")
        if same:
            assert not grads["f64"][0].any() and not grads["f64"][1].any() and not grads["f32"][0].any()
    g["yardstick_grad"] = np.float64(worst)
    print(f"yardstick_grad: {worst:.3e}")
    MG.save(BR.GOLDEN, **g)
    assert os.path.getsize(os.path.join(HERE, BR.GOLDEN)) < 1 << 20


if __name__ == "__main__":
    main()
