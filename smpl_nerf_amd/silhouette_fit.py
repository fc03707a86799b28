"""Fitting a body's pose to silhouettes without a NeRF or a trained network: pose -> vertices (ops.smpl_lbs) -> soft silhouette
(ops.soft_silhouette) -> photometric loss, and Adam on the pose - what the reference's legacy/neural_mesh_renderer.py (optimize,
optimize_sequence) does with kaolin's differentiable renderer.  The reference blurs both images with a Gaussian; here `sigma`, the
softness of the silhouette in pixel^2, plays that part.  A target for real frames is ops.render_mesh(...).face >= 0 as float."""
from __future__ import annotations

import torch

from . import ops
from .priors import SMPLifyAnglePrior


class SilhouetteFitter:
    """body_model: a SmplBodyModel with .faces, on the GPU; poses [N,4,4] float64 camera-to-world and focal for H x W frames, as
    RayGenerator holds them.  One body seen by N cameras (a multi-view fit) when the pose tensors have one row, N bodies in N
    frames (a batch of frames) when they have N.  photo_loss "L1" (mean |S - target|) or "L2" (the root of the mean square);
    angle_prior_weight^2 times the SMPLify angle prior summed over its four angles, and pose_prior_weight^2 times
    pose_prior(body_pose, betas), are added per body and averaged over the bodies."""

    def __init__(self, body_model, poses, focal, H, W, sigma=1.0, photo_loss="L1", angle_prior_weight=0, pose_prior=None,
                 pose_prior_weight=0):
        if photo_loss not in ("L1", "L2"):
            raise ValueError(f"SilhouetteFitter: photo_loss must be 'L1' or 'L2', got {photo_loss!r}")
        if body_model.faces is None:
            raise ValueError("SilhouetteFitter: the body model has no faces")
        self.body, self.sigma, self.photo_loss = body_model, float(sigma), photo_loss
        self.dev = body_model.v_template.device
        self.poses = torch.as_tensor(poses, dtype=torch.float64).to(self.dev).reshape(-1, 4, 4)
        self.focal, self.H, self.W = float(focal), int(H), int(W)
        self.angle_prior_weight, self.pose_prior_weight = float(angle_prior_weight), float(pose_prior_weight)
        self.angle_prior = SMPLifyAnglePrior().to(self.dev) if angle_prior_weight else None
        self.pose_prior = pose_prior.to(self.dev) if isinstance(pose_prior, torch.nn.Module) else pose_prior

    def silhouette(self, betas, body_pose, global_orient=None, size=None):
        """S [N,H,W] of the posed body; size = (H, W) renders at another size, the focal scaled with the width."""
        H, W = size or (self.H, self.W)
        v = self.body(betas=betas, body_pose=body_pose, global_orient=global_orient).vertices
        return ops.soft_silhouette(self.poses, self.focal * W / self.W, H, W, v[0] if v.shape[0] == 1 else v, self.body.faces,
                                   sigma=self.sigma, faces_checked=True)

    def loss(self, target, betas, body_pose, global_orient=None, size=None):
        S = self.silhouette(betas, body_pose, global_orient, size)
        diff = S - target.to(S.dtype).reshape(S.shape)
        loss = diff.abs().mean() if self.photo_loss == "L1" else (diff ** 2).mean().sqrt()
        if self.angle_prior is not None:
            loss = loss + self.angle_prior_weight ** 2 * self.angle_prior(body_pose).sum(-1).mean()
        if self.pose_prior is not None and self.pose_prior_weight:
            loss = loss + self.pose_prior_weight ** 2 * torch.as_tensor(self.pose_prior(body_pose, betas)).mean()
        return loss

    @staticmethod
    def schedule(iterations, steps, H, W):
        """[(H_i, W_i)] per iteration: full size without steps; else the size starts at size / 2^steps and doubles whenever
        i % int(iterations / steps) == 0, the first such i included - the reference's schedule, stopped at the full size."""
        if not steps:
            return [(H, W)] * iterations
        every = max(int(iterations / steps), 1)
        return [(max(H >> max(steps - i // every, 0), 1), max(W >> max(steps - i // every, 0), 1)) for i in range(iterations)]

    def fit(self, target, iterations=200, lr=1e-2, init=None, free=("body_pose",), angle_indices=None, coarse_to_fine_steps=0):
        """Adam on the tensors named in `free` ("body_pose", "betas", "global_orient"), from `init` (a dict of tensors; what is
        missing starts at zeros, one row).  angle_indices frees only those entries of body_pose.  target [N,H,W], or with
        coarse_to_fine_steps a callable (H, W) -> target.  -> (dict of the fitted tensors, [loss per iteration])."""
        J, NB = self.body.num_joints, self.body.num_betas
        init = dict(init or {})
        B = next((init[k].shape[0] for k in ("body_pose", "global_orient") if k in init), 1)
        state = {"betas": torch.zeros(1, NB), "body_pose": torch.zeros(B, 3 * (J - 1)), "global_orient": torch.zeros(B, 3)}
        for k in state:
            state[k] = (init[k] if k in init else state[k]).detach().to(self.dev, torch.float32).clone()
        unknown = set(free) - set(state)
        if unknown or not free:
            raise ValueError(f"SilhouetteFitter.fit: free must name some of {sorted(state)}, got {free}")
        if coarse_to_fine_steps and not callable(target):
            raise ValueError("SilhouetteFitter.fit: with coarse_to_fine_steps the target must be a callable of (H, W)")
        params = []
        if angle_indices is not None:
            index = torch.as_tensor(angle_indices, dtype=torch.long, device=self.dev)
            angles = state["body_pose"][:, index].clone().requires_grad_(True)
            params.append(angles)
        for k in free:
            if not (k == "body_pose" and angle_indices is not None):
                params.append(state[k].requires_grad_(True))
        optim = torch.optim.Adam(params, lr=lr)
        history = []
        for size in self.schedule(iterations, coarse_to_fine_steps, self.H, self.W):
            optim.zero_grad()
            body_pose = state["body_pose"]
            if angle_indices is not None:
                body_pose = body_pose.clone()
                body_pose[:, index] = angles
            loss = self.loss(target(*size) if callable(target) else target, state["betas"], body_pose, state["global_orient"], size)
            loss.backward()
            optim.step()
            history.append(float(loss.detach()))
        if angle_indices is not None:
            state["body_pose"][:, index] = angles.detach()
        return {k: v.detach() for k, v in state.items()}, history

    def fit_sequence(self, targets, init_pose="zero", **fit_args):
        """One fit per target; init_pose "zero" starts every frame from zeros (or fit_args' init), "last_frame" starts frame k + 1
        from frame k's result.  -> [(fitted, history)] per frame."""
        if init_pose not in ("zero", "last_frame"):
            raise ValueError(f"SilhouetteFitter.fit_sequence: init_pose must be 'zero' or 'last_frame', got {init_pose!r}")
        first = fit_args.pop("init", None)
        out, init = [], first
        for target in targets:
            fitted, history = self.fit(target, init=init, **fit_args)
            out.append((fitted, history))
            init = fitted if init_pose == "last_frame" else first
        return out
