"""Stand-ins for the SMPL assets the reference needs but does not ship (SMPL .pkl, smplx): a linear
"body model" with the call contract AppendVerticesPipeline uses (models/append_vertices_pipeline.py:38-40)
and the index-based pose estimator (models/dummy_smpl_estimator_model.py:6-27).  Torch modules, device
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
