#!/usr/bin/env python3
"""Golden vectors for the image scores (util/scores.py: img2mse :11-28, img2psnr :30-48, ssim :88-173) from the reference itself.
    python tests/golden/make_golden_scores.py    # writes g20_image_scores.npz
Per case of tests/ssim_ref.py (G20_CASES: the seeded inputs, stored as well) and per arithmetic - the fp32 inputs as they are (f32) and
cast to float64 (f64; the reference's window table is computed in fp32 either way, scores.py:79-86, 117):
    <case>/x, y, params = (k, sigma, data_range)
    <case>/<f32|f64>/ssim_none, cs_none   ssim(x, y, k, sigma, data_range, reduction='none', full=True)        [N]
    <case>/<f32|f64>/ssim_mean            ssim(x, y, k, sigma, data_range)                                     0-d
    <case>/<f32|f64>/mse, psnr            img2mse(x, y), img2psnr(x, y)   (psnr of the inputs divided by data_range: the function is
                                          written for images in [0, 1]; its result is fp32 in both arithmetics, :48)
    <case>/<f32|f64>/dx, dy               autograd of ssim(x, y, k, sigma, data_range) with respect to x and y
Nothing of the reference is copied: the file holds arrays only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import make_golden as MG
import ssim_ref as SR


def main():
    MG._stub("cv2")
    tv = MG._stub("torchvision")
    tv.models = MG._stub("torchvision.models", vgg16=None, vgg19=None)
    sys.path.insert(0, MG.REF)
    from util import scores as S
    torch.set_grad_enabled(True)
    g = {}
    for name, (shape, family, k, sigma, data_range, seed) in SR.G20_CASES.items():
        x, y = SR.images(family, shape, seed, data_range)
        g[f"{name}/x"], g[f"{name}/y"] = x, y
        g[f"{name}/params"] = np.array([k, sigma, data_range], np.float64)
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            xt, yt = torch.from_numpy(x).to(dtype).requires_grad_(True), torch.from_numpy(y).to(dtype).requires_grad_(True)
            none, cs = S.ssim(xt, yt, kernel_size=k, kernel_sigma=sigma, data_range=data_range, reduction='none', full=True)
            mean = S.ssim(xt, yt, kernel_size=k, kernel_sigma=sigma, data_range=data_range)
            mean.backward()
            with torch.no_grad():
                mse, psnr = S.img2mse(xt / data_range, yt / data_range), S.img2psnr(xt / data_range, yt / data_range)
            key = f"{name}/{tag}/"
            g[key + "ssim_none"], g[key + "cs_none"], g[key + "ssim_mean"] = none.detach().numpy(), cs.detach().numpy(), mean.detach().numpy()
            g[key + "mse"], g[key + "psnr"] = mse.numpy(), psnr.numpy().reshape(())
            g[key + "dx"], g[key + "dy"] = xt.grad.numpy(), yt.grad.numpy()
            print(f"{name} {tag}: ssim {none.detach().numpy()} mean {mean.item():.9f} cs {cs.detach().numpy()} mse {mse.item():.6e} "
                  f"psnr {float(psnr):.6f} max|dx| {float(xt.grad.abs().max()):.3e}")
    MG.save("g20_image_scores.npz", **g)
    for name in SR.G20_CASES:
        assert g[name + "/x"].nbytes + g[name + "/y"].nbytes < 50 * 1024, name


if __name__ == "__main__":
    main()
