#!/usr/bin/env python3
"""Golden vectors for LPIPS (util/scores.py:286-456) from the reference itself, without its downloads: ContentLoss takes any callable
feature stack and any list of weights, so it is run on a VGG16-shaped nn.Sequential with the seeded weights of tests/lpips_ref.py.
    python tests/golden/make_golden_lpips.py    # writes g26_lpips.npz
Per case of lpips_ref.CASES and per arithmetic (f32: the inputs as they are; f64: inputs and weights cast to float64):
    <case>/x, y                   the frames [N,3,H,W], fp32
    <case>/checksum               lpips_ref.checksum of the case's weights (the weights themselves are not stored)
    <case>/<f32|f64>/total        ContentLoss(feature_extractor=<Sequential>, layers=('3','8','15','22','29'), weights=lin,
                                  normalize_features=True, reduction='none')(x, y)                                          [N]
    <case>/<f32|f64>/layers       the same, one ContentLoss per tap: layers=(tap,), weights=[lin[l]]                                      [N,5]
    yardstick                     the largest E(f32 layers, f64 layers) over the cases: what the reference's own fp32 run is off by
Every case has H, W >= 32: the reference runs pool5, which raises below.  Nothing of the reference is copied: arrays only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch
import torch.nn as nn

import lpips_ref as LR
import make_golden as MG


def sequential(w, dtype):
    mods, i = [], 0
    for l, n in enumerate(LR.STAGES):
        for _ in range(n):
            a, b = w["conv"][i]
            conv = nn.Conv2d(a.shape[1], a.shape[0], 3, padding=1)
            conv.weight.data, conv.bias.data = torch.from_numpy(a).to(dtype), torch.from_numpy(b).to(dtype)
            mods += [conv, nn.ReLU(inplace=False)]
            i += 1
        mods.append(nn.MaxPool2d(2, 2))
    seq = nn.Sequential(*mods)
    assert [k for k, m in seq._modules.items() if isinstance(m, nn.Conv2d)] == [str(j) for j in LR.CONV_INDEX]
    return seq


def main():
    MG._stub("cv2")
    tv = MG._stub("torchvision")
    tv.models = MG._stub("torchvision.models", vgg16=None, vgg19=None)
    sys.path.insert(0, MG.REF)
    from util import scores as S
    torch.set_grad_enabled(False)
    g, worst = {}, 0.0
    for name, (channels, H, W, N, wseed, iseed, same) in LR.CASES.items():
        w = LR.weights(wseed, channels)
        x, y = LR.images(iseed, N, H, W, same)
        g[f"{name}/x"], g[f"{name}/y"], g[f"{name}/checksum"] = x, y, np.float64(LR.checksum(w))
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            seq = sequential(w, dtype)
            lin = [torch.from_numpy(v).to(dtype).view(1, -1, 1, 1) for v in w["lin"]]
            xt, yt = torch.from_numpy(x).to(dtype), torch.from_numpy(y).to(dtype)
            total = S.ContentLoss(feature_extractor=seq, layers=LR.TAPS, weights=lin, normalize_features=True, reduction='none')(xt, yt)
            cols = [S.ContentLoss(feature_extractor=seq, layers=(tap,), weights=[lin[l]], normalize_features=True, reduction='none')(xt, yt)
                    for l, tap in enumerate(LR.TAPS)]
            g[f"{name}/{tag}/total"], g[f"{name}/{tag}/layers"] = total.numpy(), torch.stack(cols, dim=1).numpy()
            assert total.dtype == dtype and g[f"{name}/{tag}/layers"].shape == (N, 5)
        e = LR.E(g[f"{name}/f32/layers"], g[f"{name}/f64/layers"])
        et = LR.E(g[f"{name}/f32/total"], g[f"{name}/f64/total"])
        worst = max(worst, e)
        print(f"{name}: total f64 {g[f'{name}/f64/total']}  E(f32 layers) {e:.3e}  E(f32 total) {et:.3e}")
        if same:
            assert not g[f"{name}/f32/layers"].any() and not g[f"{name}/f64/layers"].any()
    g["yardstick"] = np.float64(worst)
    print(f"yardstick: {worst:.3e}")
    MG.save(LR.GOLDEN, **g)
    assert os.path.getsize(os.path.join(HERE, LR.GOLDEN)) < 1 << 20


if __name__ == "__main__":
    main()
