"""The data set of the vertex_sphere model (datasets/vertex_sphere_dataset.py:25-205), built on the device.

The reference's constructor walks every ray of every image through trimesh's intersector in a Python loop (:87-89) and builds
[h w, 6890, 3] distance tensors one sample index at a time (:128-132).  Here an image is five launches: rays, the body in its goal
pose, ops.ray_mesh_hits, the samples, ops.vertex_sphere_warp.

Two things differ from the reference on purpose and are not comparable bit for bit:
  * precision - the reference computes rays, hits, depths, samples and warps in float64 and casts to fp32 in __getitem__ (:200-202);
    this port is fp32 throughout (ray origins and directions are RayGenerator's: float64 arithmetic rounded once, then normalised
    in fp32);
  * random draws - they come from torch's device generator (the `generator` argument), not from numpy's global state and
    torch.distributions on the host: the same seed gives the same data set here, and another one than the reference's.
Nothing is pinned relative to trimesh's edge and vertex tolerances either (include/smplnerf.h, snerf_ray_mesh_hits_f32).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .raygen import RayGenerator, coarse_bin_tables

MAX_PRIOR_HITS = 16      # hits per ray the mixture of coarse_samples_from_prior keeps (the largest list snerf_ray_mesh_hits_f32 returns)


class VertexSphereRays:
    """images [n,h,w,3] BGR as cv2.imread returns them (uint8; a floating array is taken as already divided by 255), transforms
    [n,4,4] camera-to-world, camera_angle_x, goal_poses [n,69] (one per image), betas [1,10] or [10], body_model: a
    body_model.SmplBodyModel on `device` with `.faces`; args supplies near, far, number_coarse_samples, vertex_sphere_radius,
    warp_by_vertex_mean, coarse_samples_from_prior, coarse_samples_from_intersect and std_dev_coarse_sample_prior
    (config_parser.py:35-45); generator: a torch.Generator of `device`.

    Per image, in the reference's order: rays with normalised directions (:75-79), the body in the goal pose (:84), all hits of
    every ray on it (:85-89), z_vals by the four cases of :91-116, samples = o + d z (:120), and the warp of every sample from the
    goal and the canonical (zero-pose) body (:122-159).  The cases of z_vals, N = number_coarse_samples:
      N == 1                           the first hit, or `far` on a miss
      coarse_samples_from_intersect    N sorted draws of Normal(first hit, std); the stratified table on a miss
      coarse_samples_from_prior        N draws, unsorted as in the reference, of the equal-weight mixture of Normal(hit, std) over the
                                       ray's hits (the MAX_PRIOR_HITS nearest are kept); the stratified table on a miss
      otherwise                        the stratified table
    The stratified table z_vals_simple is ONE table for the whole data set: its jitter is a single scalar drawn once (:59), not
    one per ray as CoarseSampling draws - a quirk of the reference, kept.

    len(), __getitem__ (the reference's 6-tuple: ray_samples [N,3], ray_translation [3], ray_direction [3], z_vals [N], warp
    [N,3], rgb [3], fp32) and batches(batch_size, shuffle), which yields the 6-lists VertexSpherePipeline takes, on the device.
    first_hit [rays] (+inf on a miss) and n_hits [rays] keep what the intersector returned."""

    def __init__(self, images, transforms, camera_angle_x: float, goal_poses, betas, body_model, args, device, generator=None):
        dev = self.device = torch.device(device)
        images = np.asarray(images)
        n, self.h, self.w = images.shape[:3]
        transforms = np.asarray(transforms, np.float64).reshape(-1, 4, 4)
        goal_poses = torch.as_tensor(np.asarray(goal_poses), dtype=torch.float32, device=dev).reshape(len(transforms), -1)
        if len(transforms) != n or images.shape[3] != 3:
            raise ValueError("VertexSphereRays: one [h,w,3] image, one transform and one goal pose per frame")
        faces = getattr(body_model, "faces", None)
        if faces is None:
            raise ValueError("VertexSphereRays: the body model has no faces (SmplBodyModel.from_arrays(..., faces=...))")
        scale = 255. if images.dtype == np.uint8 else 1.
        rgb = torch.as_tensor(images.astype(np.float32) / np.float32(scale), device=dev).reshape(n, -1, 3)
        N = self.n_samples = int(args.number_coarse_samples)
        std, far = float(args.std_dev_coarse_sample_prior), float(args.far)
        from_intersect = N > 1 and int(args.coarse_samples_from_intersect) == 1
        from_prior = N > 1 and not from_intersect and int(args.coarse_samples_from_prior) == 1
        rays = RayGenerator(transforms, self.h, self.w, camera_angle_x, args.near, args.far, 1, dev)
        betas = torch.as_tensor(np.asarray(betas), dtype=torch.float32, device=dev).reshape(1, -1)

        def draw(fn, *shape):
            return fn(shape, device=dev, dtype=torch.float32, generator=generator)

        # the stratified table (:53-59): one jitter scalar for the whole data set
        lower, span = coarse_bin_tables(args.near, args.far, N)
        jitter = draw(torch.rand, 1)
        self.z_vals_simple = torch.as_tensor(lower, dtype=torch.float32, device=dev) + torch.as_tensor(span, dtype=torch.float32, device=dev) * jitter
        with torch.no_grad():
            self.canonical = body_model(betas=betas, return_verts=True, body_pose=torch.zeros_like(goal_poses[:1])).vertices[0]    # :47
            faces = faces.to(dev).contiguous()
            R = self.h * self.w
            out = {k: [] for k in ("samples", "o", "d", "z", "warp", "first", "n_hits")}
            for i in range(n):
                index = torch.arange(i * R, (i + 1) * R, device=dev)
                _, o, d, _, _ = rays.batch(index, torch.zeros(R, device=dev, dtype=torch.float64))                                     # :75
                d = d / torch.norm(d, dim=-1, keepdim=True)                                                                           # :79
                goal = body_model(betas=betas, return_verts=True, body_pose=goal_poses[i:i + 1]).vertices[0]                          # :84, :122
                t_hits, n_hits = ops.ray_mesh_hits(o, d, goal, faces, MAX_PRIOR_HITS if from_prior else 1, faces_checked=i > 0)       # :85-89
                hit, first = (n_hits > 0)[:, None], t_hits[:, :1]
                simple = self.z_vals_simple[None, :].expand(R, N)
                if N == 1:
                    z = torch.where(hit, first, torch.full_like(first, far))                                                           # :91-97
                elif from_intersect:
                    z = torch.where(hit, torch.sort(first + std * draw(torch.randn, R, N), dim=-1)[0], simple)                         # :98-107
                elif from_prior:
                    kept = n_hits.clamp(1, MAX_PRIOR_HITS)[:, None].to(torch.float32)
                    which = torch.minimum((draw(torch.rand, R, N) * kept).to(torch.int64), kept.to(torch.int64) - 1)                  # :111
                    z = torch.where(hit, torch.gather(t_hits, 1, which) + std * draw(torch.randn, R, N), simple)                       # :112-115
                else:
                    z = simple                                                                                                         # :108-109
                z = z.contiguous()
                samples = o[:, None, :] + d[:, None, :] * z[:, :, None]                                                               # :120
                warp = ops.vertex_sphere_warp(samples, goal, self.canonical, float(args.vertex_sphere_radius),
                                              by_mean=bool(args.warp_by_vertex_mean))                                                  # :128-159
                for k, t in (("samples", samples), ("o", o), ("d", d), ("z", z), ("warp", warp), ("first", first[:, 0]), ("n_hits", n_hits)):
                    out[k].append(t)
        self.rays_samples, self.rays_translation, self.rays_direction, self.all_z_vals, self.all_warps, self.first_hit, self.n_hits = \
            (torch.cat(out[k]) for k in ("samples", "o", "d", "z", "warp", "first", "n_hits"))
        self.rgb = rgb.reshape(-1, 3)
        self.generator = generator

    def __len__(self) -> int:
        return self.rgb.shape[0]

    def __getitem__(self, index: int):
        return (self.rays_samples[index], self.rays_translation[index], self.rays_direction[index], self.all_z_vals[index],
                self.all_warps[index], self.rgb[index])

    def batches(self, batch_size: int, shuffle: bool = False):
        """The data set once, in batches of `batch_size` rays (the last one may be shorter): lists [ray_samples, ray_translation,
        ray_direction, z_vals, warp, rgb_truth] on the device.  shuffle: a permutation drawn from the generator."""
        n = len(self)
        order = torch.randperm(n, device=self.device, generator=self.generator) if shuffle else None
        for b in range(0, n, int(batch_size)):
            idx = order[b:b + batch_size] if shuffle else slice(b, b + batch_size)
            yield [t[idx] for t in (self.rays_samples, self.rays_translation, self.rays_direction, self.all_z_vals, self.all_warps, self.rgb)]
