#!/usr/bin/env python3
"""Golden vectors for the image-wise model (--model_type image_wise_dynamic) from the reference itself: its ImageWiseSolver.train
for one epoch on a tiny in-memory loader, with the synthetic linear body standing in for smplx + the SMPL .pkl (1000 vertices:
the reference builds [B, S, V, 3] tensors) and its own DummyImageWiseEstimator.
    python tests/golden/make_golden_image_wise.py    # writes g22_image_wise.npz
The inputs are rebuilt from seeds by tests/image_wise_ref.py (g22_inputs); the file holds the seeds' table and what the reference
computed: per step (2 images x 2 ray batches of half an image: the retained graph of an image is used twice) the loss, the rays of
the batch (the sub-loader shuffles: found by matching the recorded rgb_truth rows to the image's) and the rgb rows in ray order;
at the end arm_angle_l / arm_angle_r, every param_stride-th value of the coarse net's parameters and their Adam step count.
The validation loader is empty, and the reference's own "VAL loss" print then fails on a name it never bound - after the epoch's
training is complete; the maker stops there."""
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import make_golden as MG
import image_wise_ref as IR

t = MG.t


def main():
    U, RenderRayNet, _, _, _ = MG._import_reference()
    for name in ("pyrender", "smplx", "vedo"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
    # the reference's datasets/ has no __init__.py: an installed package of that name would win over it
    pkg = types.ModuleType("datasets")
    pkg.__path__ = [os.path.join(MG.REF, "datasets")]
    sys.modules["datasets"] = pkg
    sys.modules.setdefault("render", types.SimpleNamespace(get_smpl_vertices=None, get_smpl_mesh=None))      # (needs pyrender)
    import solver.image_wise_solver as IWS
    from models.dummy_image_wise_estimator import DummyImageWiseEstimator
    IWS.tensorboard_rerenders = lambda *a, **k: None
    c = IR.G22
    images, body, params = IR.g22_inputs()
    net = MG.load_params(RenderRayNet(8, 256, 60, 24, skips=[4]), params)
    truth = torch.zeros(1, 69)
    truth[0, 38], truth[0, 41] = c["truth_l"], c["truth_r"]
    est = DummyImageWiseEstimator(torch.zeros(1, 38), torch.zeros(1, 2), torch.zeros(1, 27), torch.tensor([[c["arm_angle_l"]]]),
                                  torch.tensor([[c["arm_angle_r"]]]), torch.zeros(1, 10), truth)
    args = MG.Args(run_fine=0, warp_radius=c["radius"], lrate=c["lrate"], lrate_pose=c["lrate_pose"], weight_decay=0, num_epochs=1,
                   batchsize=c["batchsize"], log_iterations=1, number_validation_images=0)
    steps = []

    def recorder(rgb, rgb_truth):
        loss = torch.nn.functional.mse_loss(rgb, rgb_truth)
        steps.append((rgb.detach().numpy().copy(), rgb_truth.detach().numpy().copy(), loss.item()))
        return loss

    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)          # (a real SummaryWriter writes runs/ where it stands)
        try:
            fine = RenderRayNet(8, 256, 60, 24, skips=[4])      # (never run: the loop is coarse only)
            solver = IWS.ImageWiseSolver(net, fine, est, body, U.PositionalEncoder(10, 0), U.PositionalEncoder(4, 0), args,
                                         loss_func=recorder)
            loader = [[t(a)[None] for a in image] for image in images]      # what DataLoader(batch_size=1, shuffle=False) yields
            torch.manual_seed(c["shuffle_seed"])
            try:
                solver.train(loader, [], 0, 0)
            except UnboundLocalError as e:
                assert "iter_per_image_val" in str(e), e
        finally:
            os.chdir(cwd)
    per_image = c["R"] // c["batchsize"]
    assert len(steps) == len(images) * per_image
    g = {"config": np.array(json.dumps(c))}
    rays, rgbs, losses = [], [], []
    for k, (rgb, rgb_truth, loss) in enumerate(steps):
        image_truth = images[k // per_image][4]
        assert len(np.unique(image_truth, axis=0)) == c["R"], "rgb_truth rows must tell the rays of an image apart"
        idx = np.array([int(np.flatnonzero((image_truth == row).all(-1))[0]) for row in rgb_truth])
        order = np.argsort(idx)
        rays.append(idx[order])
        rgbs.append(rgb[order])
        losses.append(loss)
        print("step", k, "loss", loss, "rays", idx[order].tolist())
    g["step_rays"], g["step_rgb"], g["step_loss"] = np.array(rays, np.int64), np.array(rgbs, np.float32), np.array(losses, np.float64)
    g["arm_angle_l"], g["arm_angle_r"] = est.arm_angle_l.detach().numpy().copy(), est.arm_angle_r.detach().numpy().copy()
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy()
    g["param_sample"] = flat[::c["param_stride"]].copy()
    g["adam_steps"] = np.array([int(solver.optim.state[p]["step"]) for p in net.parameters()], np.int64)
    print("arm angles", g["arm_angle_l"], g["arm_angle_r"], "adam steps", set(g["adam_steps"].tolist()))
    MG.save("g22_image_wise.npz", **g)


if __name__ == "__main__":
    main()
