#!/usr/bin/env python3
"""Golden vectors for the ray maps (utils.py:184, :187) from the reference's own raw2outputs.
    python tests/golden/make_golden_ray_maps.py    # writes g29_ray_maps.npz
For every (B, N) of tests/ray_maps_ref.GOLDEN_SHAPES, on the seeded raw, z and directions of ray_maps_ref.golden_inputs: the
reference's raw2outputs in float32 and in float64, with white_background 0 and 1 - its rgb, weights and density, and depth_map and
acc_map by its own expressions (utils.py:184, :187: the function computes both and drops them) on the weights it returned.  In
float64 also autograd's gradient to raw of sum(g_depth * depth_map) + sum(g_acc * acc_map) (N == 1: the reference's weights are
constants, the gradient is zero).  The expected point has no counterpart in the reference and is not in this file.
Keys: "<B>x<N>/<input>" and "<B>x<N>/<f32|f64>/<output>" (rgb: ".../rgb_wb<0|1>")."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import make_golden as MG
import ray_maps_ref as RR

t = MG.t


def main():
    U = MG._import_reference()[0]
    torch.set_grad_enabled(True)
    g = {}
    for B, N in RR.GOLDEN_SHAPES:
        inp = RR.golden_inputs(B, N)
        key = f"{B}x{N}"
        for k, v in inp.items():
            g[f"{key}/{k}"] = v
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            z = t(inp["z"]).to(dtype)
            dirs = t(inp["dirs"]).to(dtype)[:, None, :].expand(B, N, 3)          # the pipelines' expanded view (nerf_pipeline.py:30-32)
            kept = None
            for wb in (0, 1):
                raw = t(inp["raw"]).to(dtype).requires_grad_(True)
                rgb, weights, density = U.raw2outputs(raw, z, dirs, MG.Args(white_background=wb))
                weights, density = weights.to(dtype), density.to(dtype)          # (N == 1: the reference's float32 ones)
                depth_map = torch.sum(weights * z, -1)                           # utils.py:184
                acc_map = torch.sum(weights, -1)                                 # utils.py:187
                g[f"{key}/{tag}/rgb_wb{wb}"] = rgb.detach().numpy()
                now = [a.detach().numpy() for a in (weights, density, depth_map, acc_map)]
                if kept is None:
                    kept = now
                    for name, a in zip(("weights", "density", "depth_map", "acc_map"), now):
                        g[f"{key}/{tag}/{name}"] = a
                    if dtype == torch.float64:
                        loss = (t(inp["g_depth"]).double() * depth_map).sum() + (t(inp["g_acc"]).double() * acc_map).sum()
                        if loss.requires_grad:
                            loss.backward()
                            g[f"{key}/{tag}/d_raw"] = raw.grad.numpy()
                        else:
                            g[f"{key}/{tag}/d_raw"] = np.zeros((B, N, 4), np.float64)
                else:
                    assert all(np.array_equal(a, b) for a, b in zip(kept, now)), "white_background changed the weights"
            print(key, tag, "acc", kept[3], "depth", kept[2])
        assert N == 1 or np.abs(g[f"{key}/f64/d_raw"][..., 3]).max() > 0
    MG.save("g29_ray_maps.npz", **g)


if __name__ == "__main__":
    main()
