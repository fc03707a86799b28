"""The reference's data-set generator (create_dataset.py) on the device: camera paths (camera.py:113-206), the train / validation
split (utils.py:302-305 after create_dataset.py:14), and per frame what create_dataset.py:106-129 takes from pyrender and trimesh -
the posed body rendered textured and lit, its z-depth, and get_warp's depth and warp images - from one ops.smpl_lbs call and one
ops.render_mesh call per batch of frames.

The frames are NOT pyrender's: the shading is the Lambert rule of include/smplnerf.h (snerf_mesh_render_f32), with one texture
coordinate per vertex and no anti-aliasing.  They show the same body in the same pose through the same camera, which is what a pose
estimator or a NeRF is trained on; nothing is pinned against pyrender pixel by pixel.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import io, ops
from . import synthetic as syn

DATASET_TYPES = ("nerf", "pix2pix", "smpl_nerf", "smpl")


# ------------------------------------------------------------------------------------------------ camera paths
def circle_pose(theta: float, r: float) -> np.ndarray:
    """camera.py:80-83: on the xz-circle of radius r around the y axis; theta = 0 is (0, 0, r)."""
    return syn.pose_matrix(x=r * np.sin(np.radians(theta)), z=r * np.cos(np.radians(theta)), theta=theta)


def sphere_poses(start_angle: float, end_angle: float, number_steps: int, r: float):
    """camera.py:135-141 -> (poses [number_steps^2,4,4], angles [number_steps^2,2] = (phi, theta)): phi runs fastest."""
    phis = np.linspace(start_angle, end_angle, number_steps)
    thetas = np.linspace(start_angle, end_angle, number_steps)
    angles = np.transpose([np.tile(phis, len(thetas)), np.repeat(thetas, len(phis))])
    return np.array([syn.sphere_pose(phi, theta, r) for phi, theta in angles]), angles


def circle_poses(start_angle: float, end_angle: float, number_steps: int, r: float):
    """camera.py:167-169 -> (poses [number_steps,4,4], thetas)."""
    thetas = np.linspace(start_angle, end_angle, number_steps)
    return np.array([circle_pose(theta, r) for theta in thetas]), thetas


def circle_on_sphere_poses(number_steps: int, circle_radius: float, sphere_radius: float, center_theta: float = 0, center_phi: float = 0):
    """camera.py:198-206 -> (poses [number_steps,4,4], angles): a circle of `circle_radius` degrees around (center_phi, center_theta)
    on the sphere of sphere_radius; the first and the last pose coincide, as in the reference."""
    angles = np.linspace(0, np.pi * 2, number_steps)
    poses = [syn.sphere_pose(circle_radius * np.cos(a) + center_phi, circle_radius * np.sin(a) + center_theta, sphere_radius) for a in angles]
    return np.array(poses), angles


def split_indices(size: int, ratio: float):
    """The reference's train / validation split: utils.disjoint_indices (utils.py:302-305) as create_dataset.py runs it, right behind
    its np.random.seed(0) (:14) -> (train_indices, val_indices), unsorted as that function returns them (create_dataset.py:224 sorts
    both).  Drawn from a RandomState(0) of its own: the global generator is left alone."""
    train = np.random.RandomState(0).choice(np.arange(size), int(size * ratio), replace=False)
    return train, np.setdiff1d(np.arange(size), train, assume_unique=True)


# ------------------------------------------------------------------------------------------------ frames
def to_uint8(image):
    """[..., 3] float in [0,1] -> uint8, rounded to nearest."""
    return (image * 255.0 + 0.5).floor().clamp_(0, 255).to(torch.uint8)


class BodyRenderer:
    """body_model: a body_model.SmplBodyModel on `device` with `.faces`; uv [V,2] and texture [Ht,Wt,3] fp32 (arrays or tensors);
    the camera of the data sets: camera_angle_x, H x W pixels.  ambient / intensity / background: the shading constants of
    ops.render_mesh."""

    def __init__(self, body_model, uv, texture, camera_angle_x: float, H: int, W: int, device, ambient: float = 0.3, intensity: float = 0.7,
                 background=(1., 1., 1.)):
        self.device = dev = torch.device(device)
        faces = getattr(body_model, "faces", None)
        if faces is None:
            raise ValueError("BodyRenderer: the body model has no faces (SmplBodyModel.from_arrays(..., faces=...))")
        self.body_model = body_model
        self.faces = faces.to(dev).to(torch.int32).contiguous()
        self.uv = torch.as_tensor(np.asarray(uv), dtype=torch.float32, device=dev).contiguous()
        self.texture = torch.as_tensor(np.asarray(texture), dtype=torch.float32, device=dev).contiguous()
        self.camera_angle_x, self.H, self.W = float(camera_angle_x), int(H), int(W)
        self.focal = float(.5 * self.W / np.tan(.5 * self.camera_angle_x))            # rays_from_images_dataset.py:44
        self.shading = dict(ambient=ambient, intensity=intensity, background=background)
        self._faces_checked = False

    def _betas(self, betas):
        return torch.zeros(1, self.body_model.num_betas, device=self.device) if betas is None else \
            torch.as_tensor(np.asarray(betas) if not isinstance(betas, torch.Tensor) else betas, dtype=torch.float32, device=self.device).reshape(1, -1)

    @torch.no_grad()
    def frames(self, transforms, body_poses=None, betas=None, want_warp: bool = False):
        """transforms [n,4,4] camera-to-world; body_poses [n,69] (None: the canonical body for every frame, the `nerf` type); betas
        [10] or [1,10] -> (rgb uint8 [n,H,W,3], z-depth fp32 [n,H,W] with 0 on a miss - what pyrender returns beside the colour), and
        with want_warp also (depth [n,H,W], warp [n,H,W,3]): get_warp's images (render.py:222-319), the hit's distance from the camera
        and its way to the same surface point of the canonical body, 0 on a miss.  Tensors on the device.  One LBS call and one render
        call for the batch (a second LBS call for the canonical body with want_warp)."""
        dev = self.device
        poses = torch.as_tensor(np.asarray(transforms, np.float64).reshape(-1, 4, 4), device=dev)
        n = poses.shape[0]
        betas = self._betas(betas)
        zero_pose = torch.zeros(1, 3 * (self.body_model.num_joints - 1), device=dev)
        if body_poses is None:
            vertices = self.body_model(betas=betas, body_pose=zero_pose).vertices
        else:
            bp = torch.as_tensor(np.asarray(body_poses) if not isinstance(body_poses, torch.Tensor) else body_poses, dtype=torch.float32,
                                 device=dev).reshape(n, -1)
            vertices = self.body_model(betas=betas, body_pose=bp).vertices
        canon = self.body_model(betas=betas, body_pose=zero_pose).vertices[0] if want_warp else None
        out = ops.render_mesh(poses, self.focal, self.H, self.W, vertices, self.faces, self.uv, self.texture, canon=canon,
                              faces_checked=self._faces_checked, **self.shading)
        self._faces_checked = True
        rgb = to_uint8(out.image)
        zdepth = torch.where(out.face >= 0, out.t, torch.zeros_like(out.t))
        return (rgb, zdepth, out.depth, out.warp) if want_warp else (rgb, zdepth)


def pix2pix_frame(rgb_uint8, zdepth, far: float) -> np.ndarray:
    """create_dataset.py:114-115: the colour frame beside depth / far * 255 as a grey image -> uint8 [H,2W,3]."""
    grey = (np.asarray(zdepth) / far * 255).astype(np.uint8)
    return np.concatenate([np.asarray(rgb_uint8), np.repeat(grey[..., None], 3, axis=-1)], 1)


def write_split(directory, renderer, dataset_type: str, camera_transforms, indices, human_poses=None, betas=None, far: float = 4.8,
                batch_size: int = 32):
    """save_split (create_dataset.py:67-135): the frames `indices` of camera_transforms [n,4,4] (and of human_poses [n,69], for every
    type but `nerf`) as img_<index>.png and transforms.json through io.write_dataset; `smpl` also writes depth_<index>.npy (the
    z-depth) and warp_<index>.npy (get_warp's warp image), `pix2pix` writes pix2pix_frame.  far: twice the camera radius
    (create_dataset.py:170).  renderer: a BodyRenderer, or anything with its .frames and .camera_angle_x.  Returns the image names."""
    if dataset_type not in DATASET_TYPES:
        raise ValueError("This dataset type is unknown")
    indices = [int(i) for i in indices]
    transforms = np.asarray(camera_transforms, np.float64).reshape(-1, 4, 4)[indices]
    posed = dataset_type != "nerf"
    if posed:
        if human_poses is None:
            raise ValueError(f"write_split: the {dataset_type} type needs human_poses")
        human = np.asarray(human_poses, np.float32).reshape(len(camera_transforms), -1)[indices]
    os.makedirs(directory, exist_ok=True)
    images = []
    for b in range(0, len(indices), int(batch_size)):
        sl = slice(b, b + int(batch_size))
        got = renderer.frames(transforms[sl], human[sl] if posed else None, betas, want_warp=dataset_type == "smpl")
        rgb, zdepth = (np.asarray(torch.as_tensor(x).cpu()) for x in got[:2])
        if dataset_type == "pix2pix":
            images += [pix2pix_frame(c, z, far) for c, z in zip(rgb, zdepth)]
        else:
            images += list(rgb)
        if dataset_type == "smpl":
            warp = np.asarray(torch.as_tensor(got[3]).cpu())
            for k, index in enumerate(indices[sl]):
                np.save(os.path.join(directory, "warp_{:03d}.npy".format(index)), warp[k])
                np.save(os.path.join(directory, "depth_{:03d}.npy".format(index)), zdepth[k])
    if posed:
        betas_list = np.zeros(10).tolist() if betas is None else np.asarray(torch.as_tensor(betas).cpu(), np.float64).reshape(-1).tolist()
        return io.write_dataset(directory, images, transforms, renderer.camera_angle_x, human_poses=human, betas=betas_list, indices=indices)
    return io.write_dataset(directory, images, transforms, renderer.camera_angle_x, indices=indices)
