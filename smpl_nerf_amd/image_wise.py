"""The data set of the image-wise model (datasets/image_wise_dataset.py:65-154), one image at a time, built on the device.

The reference's __getitem__ walks every ray of the image through trimesh's intersector in a Python loop (:110-139), on a body posed
with the estimator's CURRENT arm angles - the solver trains them, so an image is sampled anew every time it is asked for.  Here an
image is four launches: rays, the body in the estimator's pose, ops.ray_mesh_first_hit or ops.ray_mesh_hits, the samples.

Restated as written, quirks included:
  * get_rays' directions are NOT unit vectors (utils.py; the vertex_sphere data set normalises them, this one does not), and the
    reference takes the METRIC distance |hit - o| as the parameter along them (:118-146): samples = o + d |hit - o|, which lies
    beyond the hit by the factor |d|.  The intersector's parameter t (in units of |d|) is turned into that distance, t |d|.
  * the jitter of the stratified bins is ONE scalar for the whole image (:103), not one per ray.
  * the z_vals it returns are ONE row [S] - the last ray's (:154) - which the solver hands to raw2outputs for every ray;
    image(i, per_ray_z=True) returns the table [R, S] instead.
Not comparable bit for bit, as for the other device data sets (vertex_sphere.py): fp32 throughout, and the draws come from torch's
device generator.  The mixture of coarse_samples_from_prior keeps the MAX_PRIOR_HITS = 16 nearest hits of a ray.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .raygen import RayGenerator, coarse_bin_tables
from .vertex_sphere import MAX_PRIOR_HITS


class ImageWiseRays:
    """images [n,h,w,3] BGR as cv2.imread returns them (uint8; a floating array is taken as already divided by 255), transforms
    [n,4,4] camera-to-world, camera_angle_x, smpl_estimator: `smpl_estimator(1)` returns (pose [1,69], betas) - the module the
    solver trains -, body_model: a module with the call contract of body_model.SmplBodyModel and `.faces`; args supplies near, far,
    number_coarse_samples, coarse_samples_from_prior, coarse_samples_from_intersect and std_dev_coarse_sample_prior
    (config_parser.py:35-45); generator: a torch.Generator of `device`.

    image(i) -> [ray_samples [R,S,3], ray_translation [R,3], ray_direction [R,3], z_vals [S] (or [R,S]), rgb [R,3]], R = h w, fp32
    on the device, without a graph: what the reference's loader yields per image and trainer.ImageWiseTrainer takes.  The z modes,
    S = number_coarse_samples, in the reference's order (:114-138):
      S == 1                           the first hit's distance, or `far` on a miss
      coarse_samples_from_intersect    S sorted draws of Normal(first hit's distance, std); the jittered bins on a miss
      coarse_samples_from_prior        S draws, unsorted as in the reference, of the equal-weight mixture of Normal(distance, std) over
                                       the ray's hits (the MAX_PRIOR_HITS nearest); the jittered bins on a miss
      otherwise                        the jittered inverse-depth bins (:97-103)
    Iterating yields image(0) .. image(n - 1): each epoch of ImageWiseTrainer.fit() samples with the pose trained so far.
    last_first_hit [R] (the first hit's distance, +inf on a miss), last_n_hits [R] and last_z_vals [R,S] keep the last image's."""

    def __init__(self, images, transforms, camera_angle_x: float, smpl_estimator, body_model, args, device, generator=None):
        dev = self.device = torch.device(device)
        images = np.asarray(images)
        n, self.h, self.w = images.shape[:3]
        transforms = np.asarray(transforms, np.float64).reshape(-1, 4, 4)
        if len(transforms) != n or images.shape[3] != 3:
            raise ValueError("ImageWiseRays: one [h,w,3] image and one transform per frame")
        faces = getattr(body_model, "faces", None)
        if faces is None:
            raise ValueError("ImageWiseRays: the body model has no faces (SmplBodyModel.from_arrays(..., faces=...))")
        self.faces, self._faces_checked = faces.to(dev).contiguous(), False
        scale = 255. if images.dtype == np.uint8 else 1.
        self.rgb = torch.as_tensor(images.astype(np.float32) / np.float32(scale), device=dev).reshape(n, -1, 3)
        self.args, self.smpl_estimator, self.body_model, self.generator = args, smpl_estimator, body_model, generator
        self.n_samples = int(args.number_coarse_samples)
        self.rays = RayGenerator(transforms, self.h, self.w, camera_angle_x, args.near, args.far, 1, dev)
        lower, span = coarse_bin_tables(args.near, args.far, self.n_samples)
        self._lower, self._span = (torch.as_tensor(t, dtype=torch.float32, device=dev) for t in (lower, span))
        self.last_first_hit = self.last_n_hits = self.last_z_vals = None

    def __len__(self) -> int:
        return self.rgb.shape[0]

    def __iter__(self):
        return (self.image(i) for i in range(len(self)))

    def _draw(self, fn, *shape):
        return fn(shape, device=self.device, dtype=torch.float32, generator=self.generator)

    @torch.no_grad()
    def image(self, i: int, per_ray_z: bool = False):
        args, dev, S = self.args, self.device, self.n_samples
        R = self.h * self.w
        std, far = float(args.std_dev_coarse_sample_prior), float(args.far)
        from_intersect = S > 1 and int(args.coarse_samples_from_intersect) == 1
        from_prior = S > 1 and not from_intersect and int(args.coarse_samples_from_prior) == 1
        index = torch.arange(i * R, (i + 1) * R, device=dev)
        _, o, d, _, _ = self.rays.batch(index, torch.zeros(R, device=dev, dtype=torch.float64))                  # :93-95
        simple = (self._lower + self._span * self._draw(torch.rand, 1))[None, :].expand(R, S)                     # :97-103
        pose, betas = self.smpl_estimator(1)                                                                       # :106
        goal = self.body_model(betas=betas, return_verts=True, body_pose=pose).vertices[0].contiguous()           # :107
        length = torch.norm(d, dim=-1, keepdim=True)                                                               # (t |d| = |hit - o|, :118)
        if from_prior:
            t_hits, n_hits = ops.ray_mesh_hits(o, d, goal, self.faces, MAX_PRIOR_HITS, faces_checked=self._faces_checked)   # :111
            t_hits = t_hits * length
        else:
            t, face, _ = ops.ray_mesh_first_hit(o, d, goal, self.faces, faces_checked=self._faces_checked)[:3]
            t_hits, n_hits = (t * length[:, 0])[:, None], (face >= 0).to(torch.int32)
        self._faces_checked = True
        hit, first = (n_hits > 0)[:, None], t_hits[:, :1]
        if S == 1:
            z = torch.where(hit, first, torch.full_like(first, far))                                               # :114-120
        elif from_intersect:
            z = torch.where(hit, torch.sort(first + std * self._draw(torch.randn, R, S), dim=-1)[0], simple)       # :121-130
        elif from_prior:
            kept = n_hits.clamp(1, MAX_PRIOR_HITS)[:, None].to(torch.float32)
            which = torch.minimum((self._draw(torch.rand, R, S) * kept).to(torch.int64), kept.to(torch.int64) - 1)   # :134
            z = torch.where(hit, torch.gather(t_hits, 1, which) + std * self._draw(torch.randn, R, S), simple)    # :135-138
        else:
            z = simple                                                                                             # :131-132
        z = z.contiguous()
        samples = o[:, None, :] + d[:, None, :] * z[:, :, None]                                                   # :145
        self.last_first_hit, self.last_n_hits, self.last_z_vals = first[:, 0], n_hits, z
        return [samples, o, d, z if per_ray_z else z[-1].clone(), self.rgb[i]]                                     # :154
