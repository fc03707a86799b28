"""Measurement: the expected depth of a trained field against the depth of the mesh it was trained on.  The synthetic body
(synthetic_smpl.surface_smpl_arrays) is rendered through create_dataset.BodyRenderer from cameras on a circle; a plain NerfPipeline
is trained on those frames for a short run (white background, 64 + 128 samples); DataParallelTrainer.validate_maps renders a
training camera and a held-out one, and io.depth_error compares its depth with ops.render_mesh's t (BodyRenderer's z-depth) for the
same cameras, over the pixels that show the body.  Descriptive: a few hundred steps give a coarse field; no threshold.

    python tools/ray_maps_depth.py [--out FILE] [--steps 1500] [--rays 2048] [--side 64]

A run is kept at the end of profiles/ray_maps_errors.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from smpl_nerf_amd import io as sio
from smpl_nerf_amd import synthetic as syn
from smpl_nerf_amd.body_model import SmplBodyModel
from smpl_nerf_amd.create_dataset import BodyRenderer
from smpl_nerf_amd.nets import RenderRayNet
from smpl_nerf_amd.ops import PositionalEncoder
from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs
from smpl_nerf_amd.raygen import RayGenerator
from smpl_nerf_amd.synthetic_smpl import smooth_texture, surface_smpl_arrays, surface_uv
from smpl_nerf_amd.trainer import DataParallelTrainer

ANGLE, RADIUS, NEAR, FAR = np.pi / 3, 2.4, 1.0, 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--side", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ray_maps_depth: needs the GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    H = W = a.side
    arrays = surface_smpl_arrays(11, level=2)
    body = SmplBodyModel.from_arrays(**arrays).to(dev)
    renderer = BodyRenderer(body, surface_uv(arrays["v_template"], 3), smooth_texture(4), ANGLE, H, W, dev)
    thetas = [-40.0, -30.0, -20.0, -10.0, 0.0, 10.0, 20.0, 30.0, 40.0]
    train_poses = np.stack([syn.sphere_pose(0.0, t, RADIUS) for t in thetas])
    val_poses = np.stack([syn.sphere_pose(0.0, t, RADIUS) for t in (0.0, 15.0)])      # a training camera and a held-out one
    rgb, _ = renderer.frames(train_poses)
    _, val_depth = renderer.frames(val_poses)
    gen = RayGenerator(train_poses, H, W, ANGLE, NEAR, FAR, 64, dev, images=rgb.float() / 255.0)
    val = RayGenerator(val_poses, H, W, ANGLE, NEAR, FAR, 64, dev)
    mc, mf = (RenderRayNet(8, 256, 60, 24, skips=[4]).to(dev).train() for _ in range(2))
    pipe = NerfPipeline(mc, mf, PipelineArgs(white_background=1), PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    tr = DataParallelTrainer(pipe, [mc, mf], lr=5e-4)
    g = torch.Generator(device=dev).manual_seed(1)
    losses = [tr.step(gen.random_batch(a.rays, g)) for _ in range(a.steps)]
    losses = torch.stack(losses).cpu()
    chunk = 2048
    loader = [val.batch(torch.arange(i, min(i + chunk, val.n_rays), device=dev),
                        torch.full((min(i + chunk, val.n_rays) - i,), 0.5, device=dev, dtype=torch.float64)) for i in range(0, val.n_rays, chunk)]
    maps = tr.validate_maps(loader, H, W)
    lines = [f"depth against the mesh: NerfPipeline trained {a.steps} steps x {a.rays} rays on {len(thetas)} frames of {H} x {W} of the synthetic body "
             f"(camera radius {RADIUS}, samples in [{NEAR}, {FAR}]), {torch.cuda.get_device_name(0)}",
             f"  training loss (coarse + fine MSE): first 10 steps {float(losses[:10].mean()):.4f}, last 10 steps {float(losses[-10:].mean()):.4f}"]
    for f, name in enumerate(("training camera (theta 0)", "held-out camera (theta 15)")):
        ref, depth, acc = val_depth[f], maps["depth"][f], maps["acc"][f]
        body_px = ref > 0
        solid = acc > 0.5
        mean, worst = sio.depth_error(depth, ref)
        mean_s, worst_s = sio.depth_error(depth, ref, mask=solid)
        lines += [f"  {name}: {int(body_px.sum())} of {H * W} pixels show the body (mesh z-depth {float(ref[body_px].min()):.3f} .. {float(ref[body_px].max()):.3f}); "
                  f"acc > 0.5 on {int((solid & body_px).sum())} of them and on {int((solid & ~body_px).sum())} background pixels; "
                  f"mean acc {float(acc[body_px].mean()):.3f} on the body, {float(acc[~body_px].mean()):.3f} off it",
                  f"    io.depth_error(validate_maps depth, render_mesh t): mean {mean:.4f} max {worst:.4f} over the body's pixels; "
                  f"mean {mean_s:.4f} max {worst_s:.4f} over those with acc > 0.5"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
