"""The SMPL body model on the device: what the reference gets from smplx.create(...) (train.py:214, 244, 263) and the dynamic
pipelines call as smpl_model(betas=, return_verts=True, body_pose=, global_orient=).vertices, as an nn.Module over
ops.smpl_lbs (csrc/smpl_lbs.hip).  No smplx, no chumpy."""
from __future__ import annotations

import pickle
import types

import numpy as np
import torch

from . import ops


def _dense(a):
    return np.asarray(a.toarray() if hasattr(a, "toarray") else a)      # (a scipy-sparse J_regressor)


class SmplBodyModel(torch.nn.Module):
    """Standard SMPL linear blend skinning (Loper et al. 2015) with smplx's conventions (include/smplnerf.h lists the steps).

    forward(betas=None, return_verts=True, body_pose=None, global_orient=None) returns an object with `.vertices [B,V,3]` and
    `.joints [B,J,3]`: the call contract of AppendVerticesPipeline and DynamicPipeline.  `.joints` holds the J posed joints of the
    kinematic chain only; the extra joints smplx picks from vertices (nose, eyes, finger tips ...) are not reproduced.  A missing
    argument counts as zeros; betas may have one row for the whole batch.  Differentiable with respect to the three arguments.

    The model arrays are buffers in the kernels' layout (so .to() and state_dict() work): v_template [V,3], blend
    [num_betas + 9(J-1), 3V] (shapedirs then posedirs, one row per coefficient), J_template [J,3] and J_dirs [J,3,num_betas]
    (the joint regressor applied to template and shape directions once, in float64), weights [V,J], parents [J] int32.
    `.faces` is the triangle table [F,3] int32 of the surface (what ops.ray_mesh_hits takes) or None: a non-persistent buffer, so
    it follows .to() and state_dict() does not list it."""

    def __init__(self, v_template, blend, J_template, J_dirs, weights, parents, faces=None):
        super().__init__()
        for name, a in (("v_template", v_template), ("blend", blend), ("J_template", J_template), ("J_dirs", J_dirs), ("weights", weights)):
            self.register_buffer(name, torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)))
        self.register_buffer("parents", torch.as_tensor(np.ascontiguousarray(parents, dtype=np.int32)))
        if faces is not None:
            faces = np.ascontiguousarray(np.asarray(faces).astype(np.int64))
            if faces.ndim != 2 or faces.shape[1] != 3 or len(faces) < 1 or faces.min() < 0 or faces.max() >= self.v_template.shape[0]:
                raise ValueError(f"SmplBodyModel: faces must be [F >= 1, 3] indices into the {self.v_template.shape[0]} vertices")
            faces = torch.as_tensor(faces.astype(np.int32))
        self.register_buffer("faces", faces, persistent=False)
        self._parents_host = None

    @classmethod
    def from_arrays(cls, v_template, shapedirs, posedirs, J_regressor, weights, parents, num_betas=10, faces=None):
        """From the arrays of an SMPL file: v_template [V,3], shapedirs [V,3,>=num_betas], posedirs [V,3,9(J-1)], J_regressor [J,V]
        (dense or scipy-sparse), weights [V,J], parents [J] (the root's entry is replaced by -1: SMPL files store 2^32 - 1); faces
        [F,3] (the files' `f`), optional."""
        v_template, shapedirs, posedirs, weights = (np.asarray(a, np.float64) for a in (v_template, shapedirs, posedirs, weights))
        reg = _dense(J_regressor).astype(np.float64)
        V, J = weights.shape
        if v_template.shape != (V, 3) or shapedirs.ndim != 3 or shapedirs.shape[:2] != (V, 3) or shapedirs.shape[2] < num_betas:
            raise ValueError(f"SmplBodyModel: v_template {v_template.shape} / shapedirs {shapedirs.shape} do not match V={V}, num_betas={num_betas}")
        if posedirs.shape != (V, 3, 9 * (J - 1)):
            raise ValueError(f"SmplBodyModel: posedirs must arrive as [V, 3, 9 (J - 1)] = {(V, 3, 9 * (J - 1))}, got {posedirs.shape}")
        if reg.shape != (J, V):
            raise ValueError(f"SmplBodyModel: J_regressor must be [J, V] = {(J, V)}, got {reg.shape}")
        parents = np.asarray(parents).astype(np.int64).reshape(-1).copy()
        parents[0] = -1
        if len(parents) != J or any(not 0 <= parents[j] < j for j in range(1, J)):
            raise ValueError("SmplBodyModel: parents must have J entries with parents[j] < j")
        shapedirs = shapedirs[:, :, :num_betas]
        blend = np.concatenate([shapedirs.reshape(3 * V, -1).T, posedirs.reshape(3 * V, -1).T], 0)
        return cls(v_template, blend, reg @ v_template, np.einsum("jv,vcn->jcn", reg, shapedirs), weights, parents, faces)

    @classmethod
    def from_file(cls, path, num_betas=10):
        """An SMPL model file: `.npz` (arrays v_template, shapedirs, posedirs, J_regressor, weights, and kintree_table or parents),
        or a `.pkl` that unpickles without chumpy (plain numpy arrays, a scipy-sparse J_regressor, kintree_table).  The triangle table
        `f` (or `faces`) is read when present."""
        path = str(path)
        if path.endswith(".npz"):
            d = dict(np.load(path, allow_pickle=False))
        else:
            try:
                with open(path, "rb") as f:
                    d = pickle.load(f, encoding="latin1")
            except ImportError as e:
                if "chumpy" in str(e):
                    raise RuntimeError(f"{path} needs the chumpy package to unpickle (its arrays are chumpy objects), which this project "
                                       "does not use: convert the file once, where chumpy is installed, with np.savez(out, v_template=..., "
                                       "shapedirs=..., posedirs=..., J_regressor=..., weights=..., kintree_table=...) of plain arrays "
                                       "and load the .npz") from e
                raise
        missing = [k for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights") if k not in d]
        if missing or ("parents" not in d and "kintree_table" not in d):
            raise ValueError(f"{path}: no {missing or ['kintree_table / parents']} in the file")
        parents = d["parents"] if "parents" in d else np.asarray(d["kintree_table"])[0]
        return cls.from_arrays(d["v_template"], d["shapedirs"], d["posedirs"], d["J_regressor"], d["weights"], parents, num_betas,
                               faces=d["f"] if "f" in d else d.get("faces"))

    num_joints = property(lambda self: self.weights.shape[1])
    num_betas = property(lambda self: self.J_dirs.shape[2])

    def _load_from_state_dict(self, *a, **k):
        self._parents_host = None
        return super()._load_from_state_dict(*a, **k)

    def kernel_buffers(self):
        """The mapping ops.smpl_lbs takes; the parent table is read back from the device once."""
        if self._parents_host is None:
            self._parents_host = [int(p) for p in self.parents.cpu()]
        return {"v_template": self.v_template, "blend": self.blend, "J_template": self.J_template, "J_dirs": self.J_dirs,
                "weights": self.weights, "parents": self._parents_host}

    def forward(self, betas=None, return_verts=True, body_pose=None, global_orient=None):
        dev, J = self.v_template.device, self.num_joints
        B = next((t.shape[0] for t in (body_pose, global_orient, betas) if t is not None), 1)
        if betas is None:
            betas = torch.zeros((1, self.num_betas), device=dev)
        if body_pose is None:
            body_pose = torch.zeros((B, 3 * (J - 1)), device=dev)
        vertices, joints = ops.smpl_lbs(self.kernel_buffers(), betas.reshape(betas.shape[0], -1), body_pose.reshape(body_pose.shape[0], -1),
                                        None if global_orient is None else global_orient.reshape(global_orient.shape[0], 3))
        return types.SimpleNamespace(vertices=vertices if return_verts else None, joints=joints)
