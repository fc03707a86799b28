"""The data set of the single-sample model (datasets/single_sample_dataset.py:17-128, SmplDataset) together with the half of
create_dataset.py that feeds it (:126-128: the depth and the warp image of every frame, from render.py:222-319, get_warp), built on
the device.

The reference makes one trimesh intersector call per image, picks the closest hit of every ray in a Python loop and solves a 3 x 3
system per hit ray in a second one; the result goes through depth_*.npy and warp_*.npy files.  Here an image is three launches:
rays, the body in its goal pose, ops.ray_mesh_first_hit with the canonical body.

Two things differ from the reference on purpose and are not comparable bit for bit:
  * precision - the reference computes rays, hits, depths and warps in float64 and casts to fp32 in __getitem__ (:122-125); this
    port is fp32 throughout (ray origins and directions are RayGenerator's: float64 arithmetic rounded once);
  * nothing is pinned relative to trimesh's edge and vertex tolerances (include/smplnerf.h, snerf_ray_mesh_first_hit_f32).
The warp is formed from the hit's barycentrics, not from the reference's solve of goal_vertices^T x = hit: the same numbers
wherever that system is regular.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .raygen import RayGenerator


class SingleSampleRays:
    """images [n,h,w,3] BGR as cv2.imread returns them (uint8; a floating array is taken as already divided by 255), transforms
    [n,4,4] camera-to-world, camera_angle_x, goal_poses [n,69] (one per image), betas [1,10] or [10], body_model: a
    body_model.SmplBodyModel on `device` with `.faces`; args supplies near and far.

    Per image: rays with the directions of get_rays, NOT normalised (the reference hands these to get_warp and takes the depth as
    the hit's Euclidean distance from the camera), the body in the goal pose and - once - in the zero pose, the first hit of every
    ray with its depth t |d| and its warp to the canonical body, and the one sample of the ray at o + d/|d| depth, or at
    o + d/|d| far where the ray misses the body: depth 0 (:113-119).

    len(), __getitem__ (the reference's 6-tuple, :122-125: ray_sample [3], ray_translation [3], ray_direction [3], human_pose
    [69], warp [3], rgb [3], fp32) and batches(batch_size, shuffle), which yields the 6-lists SingleSamplePipeline takes, on the
    device.  depth [rays] (0 on a miss), face [rays] int32 (-1 on a miss) and uv [rays,2] keep what the first hit returned;
    depth_images() and warp_images() are what create_dataset.py saves per frame."""

    def __init__(self, images, transforms, camera_angle_x: float, goal_poses, betas, body_model, args, device, generator=None):
        dev = self.device = torch.device(device)
        images = np.asarray(images)
        n, self.h, self.w = images.shape[:3]
        transforms = np.asarray(transforms, np.float64).reshape(-1, 4, 4)
        goal_poses = torch.as_tensor(np.asarray(goal_poses), dtype=torch.float32, device=dev).reshape(len(transforms), -1)
        if len(transforms) != n or images.shape[3] != 3:
            raise ValueError("SingleSampleRays: one [h,w,3] image, one transform and one goal pose per frame")
        faces = getattr(body_model, "faces", None)
        if faces is None:
            raise ValueError("SingleSampleRays: the body model has no faces (SmplBodyModel.from_arrays(..., faces=...))")
        scale = 255. if images.dtype == np.uint8 else 1.
        rgb = torch.as_tensor(images.astype(np.float32) / np.float32(scale), device=dev).reshape(n, -1, 3)
        far = float(args.far)
        rays = RayGenerator(transforms, self.h, self.w, camera_angle_x, args.near, args.far, 1, dev)
        betas = torch.as_tensor(np.asarray(betas), dtype=torch.float32, device=dev).reshape(1, -1)
        with torch.no_grad():
            self.canonical = body_model(betas=betas, return_verts=True, body_pose=torch.zeros_like(goal_poses[:1])).vertices[0]    # :83
            faces = faces.to(dev).contiguous()
            R = self.h * self.w
            out = {k: [] for k in ("sample", "o", "d", "warp", "depth", "face", "uv")}
            for i in range(n):
                index = torch.arange(i * R, (i + 1) * R, device=dev)
                _, o, d, _, _ = rays.batch(index, torch.zeros(R, device=dev, dtype=torch.float64))                                     # :69
                goal = body_model(betas=betas, return_verts=True, body_pose=goal_poses[i:i + 1]).vertices[0]
                _, face, uv, warp, depth = ops.ray_mesh_first_hit(o, d, goal, faces, canon=self.canonical, faces_checked=i > 0)      # get_warp
                unit = d / torch.norm(d, dim=-1, keepdim=True)                                                                        # :113
                sample = o + unit * torch.where(depth == 0, torch.full_like(depth, far), depth)[:, None]                              # :116-119
                for k, t in (("sample", sample), ("o", o), ("d", d), ("warp", warp), ("depth", depth), ("face", face), ("uv", uv)):
                    out[k].append(t)
        self.ray_samples, self.rays_translation, self.rays_direction, self.all_warps, self.depth, self.face, self.uv = \
            (torch.cat(out[k]) for k in ("sample", "o", "d", "warp", "depth", "face", "uv"))
        self.human_poses = goal_poses.repeat_interleave(R, dim=0)                                                                      # :73
        self.rgb = rgb.reshape(-1, 3)
        self.generator = generator

    def _tensors(self):
        return self.ray_samples, self.rays_translation, self.rays_direction, self.human_poses, self.all_warps, self.rgb

    def __len__(self) -> int:
        return self.rgb.shape[0]

    def __getitem__(self, index: int):
        return tuple(t[index] for t in self._tensors())

    def batches(self, batch_size: int, shuffle: bool = False):
        """The data set once, in batches of `batch_size` rays (the last one may be shorter): lists [ray_sample, ray_translation,
        ray_direction, human_pose, warp, rgb_truth] on the device.  shuffle: a permutation drawn from the generator."""
        n = len(self)
        order = torch.randperm(n, device=self.device, generator=self.generator) if shuffle else None
        for b in range(0, n, int(batch_size)):
            idx = order[b:b + batch_size] if shuffle else slice(b, b + batch_size)
            yield [t[idx] for t in self._tensors()]

    def depth_images(self):
        """[n,h,w]: depth_*.npy of create_dataset.py:127, all frames."""
        return self.depth.view(-1, self.h, self.w)

    def warp_images(self):
        """[n,h,w,3]: warp_*.npy of create_dataset.py:128, all frames."""
        return self.all_warps.view(-1, self.h, self.w, 3)
