"""Stand-ins for the SMPL assets the reference needs but does not ship (SMPL .pkl, smplx): a linear
"body model" with the call contract AppendVerticesPipeline uses (models/append_vertices_pipeline.py:38-40)
and the index-based pose estimator (models/dummy_smpl_estimator_model.py:6-27), and the arm-angle estimator of
the image-wise model (models/dummy_image_wise_estimator.py).  Torch modules, device
agnostic; used by the golden generator, the tests and the synthetic benchmarks."""
from __future__ import annotations

import types

import numpy as np
import torch


class LinearBodyModel(torch.nn.Module):
    """vertices[b] = V0 + sum_j body_pose[b, j] * Vj for the two animated joints 38 and 41
    (6890 x 3 like SMPL).  `betas`/`global_orient` are accepted and ignored."""

    def __init__(self, seed: int = 0, n_vertices: int = 6890, scale: float = 0.3):
        super().__init__()
        rng = np.random.default_rng(seed)
        self.register_buffer("v0", torch.from_numpy(rng.normal(0, scale, (n_vertices, 3)).astype(np.float32)))
        self.register_buffer("v38", torch.from_numpy(rng.normal(0, scale, (n_vertices, 3)).astype(np.float32)))
        self.register_buffer("v41", torch.from_numpy(rng.normal(0, scale, (n_vertices, 3)).astype(np.float32)))

    def forward(self, betas=None, return_verts=True, body_pose=None, global_orient=None):
        v = (self.v0[None] + body_pose[:, 38, None, None] * self.v38[None]
             + body_pose[:, 41, None, None] * self.v41[None])
        return types.SimpleNamespace(vertices=v)


class IndexPoseEstimator(torch.nn.Module):
    """models/dummy_smpl_estimator_model.py:21-27: x are indices into preset goal poses; betas are shared.
    trainable_poses = True makes goal_poses a trained parameter (the reference's dummy estimator for the dynamic
    pipelines, solver/dynamic_solver.py: the loss reaches the poses through the warp)."""

    def __init__(self, goal_poses, betas, trainable_poses: bool = False):
        super().__init__()
        self.betas = torch.nn.Parameter(betas.data, requires_grad=False)
        self.goal_poses = torch.nn.Parameter(goal_poses.data.clone() if trainable_poses else goal_poses.data,
                                             requires_grad=bool(trainable_poses))

    def forward(self, x):
        return self.goal_poses[x], self.betas.expand(len(x), -1)


class ArmAngleEstimator(torch.nn.Module):
    """The estimator of the image-wise model (models/dummy_image_wise_estimator.py, as train.py:88-95 builds it): ONE pose for the
    image, fixed but for the two arm angles - entries 38 and 41 of the 69 body-pose parameters -, which are trained through the
    warp.  forward(x) ignores x and returns (pose [1, 69], betas [1, NB]).  The attribute names the solver's pose loss reads are
    the reference's: arm_angle_l, arm_angle_r ([1, 1] parameters) and ground_truth_pose [1, 69]."""

    def __init__(self, arm_angle_l: float, arm_angle_r: float, betas=None, ground_truth_pose=None, rest_pose=None):
        super().__init__()
        rest = torch.zeros(1, 69) if rest_pose is None else torch.as_tensor(rest_pose, dtype=torch.float32).reshape(1, 69)
        self.register_buffer("rest_pose", rest.clone())
        self.arm_angle_l = torch.nn.Parameter(torch.tensor([[float(arm_angle_l)]]))
        self.arm_angle_r = torch.nn.Parameter(torch.tensor([[float(arm_angle_r)]]))
        self.betas = torch.nn.Parameter(torch.zeros(1, 10) if betas is None else betas.data.clone().reshape(1, -1), requires_grad=False)
        gt = torch.zeros(1, 69) if ground_truth_pose is None else torch.as_tensor(ground_truth_pose, dtype=torch.float32).reshape(1, 69)
        self.ground_truth_pose = torch.nn.Parameter(gt.clone(), requires_grad=False)

    def forward(self, x=None):
        r = self.rest_pose
        return torch.cat([r[:, :38], self.arm_angle_l, r[:, 39:41], self.arm_angle_r, r[:, 42:]], dim=-1), self.betas


# SMPL's kinematic tree (kintree_table[0] of the published model files, root = -1)
SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)


def random_smpl_arrays(seed: int, n_vertices: int = 6890, n_joints: int = 24, num_betas: int = 10) -> dict:
    """A full synthetic body with the arrays of an SMPL file (for tests and benchmarks; body_model.SmplBodyModel.from_arrays
    takes it as keyword arguments): v_template [V,3] ~ N(0, 0.3), small blend shapes shapedirs [V,3,num_betas] ~ N(0, 0.01) and
    posedirs [V,3,9(J-1)] ~ N(0, 0.003), J_regressor [J,V] with up to 8 non-negative entries per row that sum to 1, weights
    [V,J] with at most 4 non-zeros per vertex that sum to 1, parents [J] = SMPL's 24-joint table (its first J entries; a chain
    beyond 24).  float32 / int32 numpy arrays."""
    rng = np.random.default_rng(seed)
    V, J = int(n_vertices), int(n_joints)
    f = np.float32
    out = {"v_template": rng.normal(0, 0.3, (V, 3)).astype(f),
           "shapedirs": rng.normal(0, 0.01, (V, 3, num_betas)).astype(f),
           "posedirs": rng.normal(0, 0.003, (V, 3, 9 * (J - 1))).astype(f)}
    reg = np.zeros((J, V), np.float64)
    for j in range(J):
        idx = rng.choice(V, size=min(8, V), replace=False)
        w = rng.random(len(idx)) + 0.1
        reg[j, idx] = w / w.sum()
    out["J_regressor"] = reg.astype(f)
    wts = np.zeros((V, J), np.float64)
    for v in range(V):
        idx = rng.choice(J, size=min(4, J), replace=False)
        w = rng.random(len(idx)) + 0.1
        wts[v, idx] = w / w.sum()
    out["weights"] = wts.astype(f)
    out["parents"] = np.array([SMPL_PARENTS[j] if j < len(SMPL_PARENTS) else j - 1 for j in range(J)], np.int32)
    return out


def icosphere(level: int):
    """The unit icosphere after `level` subdivisions: (vertices [V,3] float64 on the unit sphere, faces [F,3] int32, outward
    winding) with V = 12 / 42 / 162 / 642 / 2562 and F = 20 / 80 / 320 / 1280 / 5120 for level 0 .. 4.  A closed surface: every edge
    is shared by exactly two faces."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
             (-g, 0, -1), (-g, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in verts]
    for _ in range(int(level)):
        mid, out = {}, []

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.stack(verts), np.asarray(faces, np.int32)


def bumpy_ellipsoid(level: int, seed: int, radii=(0.25, 0.8, 0.2), bump: float = 0.15):
    """A body-sized closed surface: the icosphere of `level`, its radius modulated by a few low-frequency waves (so that a ray can
    cross it more than twice) and scaled to an ellipsoid.  (vertices [V,3] float32, faces [F,3] int32)."""
    rng = np.random.default_rng(seed)
    v, faces = icosphere(level)
    freq, phase = rng.integers(2, 5, (3, 3)), rng.uniform(0, 2 * np.pi, 3)
    r = 1.0 + bump * sum(np.sin((v * freq[k]).sum(-1) * 1.7 + phase[k]) for k in range(3))
    return (v * r[:, None] * np.asarray(radii)).astype(np.float32), faces


SKIN_LENGTH = 0.25      # surface_smpl_arrays: the length over which a vertex's skinning weights change


def surface_smpl_arrays(seed: int, level: int = 2, n_joints: int = 24, num_betas: int = 10) -> dict:
    """A synthetic body that is a surface, with the arrays of an SMPL file plus `faces` (SmplBodyModel.from_arrays takes the dict
    as keyword arguments): the template is bumpy_ellipsoid(level, seed) - 12 / 42 / 162 / 642 / 2562 vertices - every joint sits
    half-way between the centroid and a patch of the surface, and the skinning weights are a softmax of minus the distance to
    the joints over SKIN_LENGTH, so they vary smoothly over the surface and a posed body is still a surface.  Small blend shapes as in
    random_smpl_arrays."""
    rng = np.random.default_rng(seed)
    f = np.float32
    v, faces = bumpy_ellipsoid(level, seed)
    V, J = len(v), int(n_joints)
    v64 = v.astype(np.float64)
    centre = v64[rng.choice(V, size=J, replace=J > V)]
    patch = np.exp(-((v64[None] - centre[:, None]) ** 2).sum(-1) / 0.1 ** 2)
    reg = 0.5 * patch / patch.sum(1, keepdims=True) + 0.5 / V
    joints = reg @ v64
    logits = -np.linalg.norm(v64[:, None] - joints[None], axis=-1) / SKIN_LENGTH
    wts = np.exp(logits - logits.max(1, keepdims=True))
    return {"v_template": v,
            "shapedirs": rng.normal(0, 0.01, (V, 3, num_betas)).astype(f),
            "posedirs": rng.normal(0, 0.003, (V, 3, 9 * (J - 1))).astype(f),
            "J_regressor": reg.astype(f),
            "weights": (wts / wts.sum(1, keepdims=True)).astype(f),
            "parents": np.array([SMPL_PARENTS[j] if j < len(SMPL_PARENTS) else j - 1 for j in range(J)], np.int32),
            "faces": faces}


def surface_uv(vertices, seed: int = 0) -> np.ndarray:
    """One texture coordinate per vertex, [V,2] float32 in [0,1]: the spherical coordinates of the rest vertices about their
    centroid, U the azimuth over 2 pi and V the polar angle over pi, in a frame rotated by a seeded random rotation (so that the
    seam and the poles do not sit on a symmetry plane of the body).  The reference reads per-vertex uv from its SMPL texture file
    (its mesh is built with process=False); this stands in for it in tests and examples."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    p = (np.asarray(vertices, np.float64) - np.asarray(vertices, np.float64).mean(0)) @ q
    r = np.maximum(np.linalg.norm(p, axis=-1), 1e-12)
    u = np.arctan2(p[:, 1], p[:, 0]) / (2 * np.pi) + 0.5
    v = np.arccos(np.clip(p[:, 2] / r, -1, 1)) / np.pi
    return np.stack([u, v], -1).astype(np.float32)


def smooth_texture(seed: int, height: int = 64, width: int = 64, waves: int = 4) -> np.ndarray:
    """A seeded smooth RGB texture [height,width,3] float32 in [0,1]: per channel a mean plus `waves` low-frequency plane waves,
    periodic in the horizontal direction (the azimuth of surface_uv wraps there)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid((np.arange(height) + 0.5) / height, (np.arange(width) + 0.5) / width, indexing="ij")
    out = np.empty((height, width, 3))
    for c in range(3):
        kx, ky = rng.integers(1, 4, waves), rng.uniform(0.5, 3.0, waves)
        phase, amp = rng.uniform(0, 2 * np.pi, waves), rng.uniform(0.3, 1.0, waves)
        wave = sum(amp[k] * np.sin(2 * np.pi * (kx[k] * xx + ky[k] * yy) + phase[k]) for k in range(waves))
        out[..., c] = 0.55 + 0.4 * wave / np.abs(amp).sum()
    return np.clip(out, 0.0, 1.0).astype(np.float32)
