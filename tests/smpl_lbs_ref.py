"""Torch (CPU) restatement of SMPL linear blend skinning (Loper et al. 2015) with smplx's conventions, used ONLY by tests and by the
timing tool: the yardstick of csrc/smpl_lbs.hip, in the dtype of its inputs, differentiable by autograd.  Written from the
formulation (the ten steps of include/smplnerf.h), on the arrays of an SMPL file as they arrive - the joint regressor is applied to
v_shaped here, not folded as the kernels' loader does:

   1 full_pose = [global_orient | body_pose]: J axis-angle vectors        2 angle = |r + 1e-8|, dir = r / angle,
   R = I + sin(angle) K + (1 - cos(angle)) K^2, K = skew(dir)             3 pose_feature = (R[1:] - I) flattened (joint, row, column)
   4 v_shaped = v_template + shapedirs betas     5 J_rest = J_regressor v_shaped     6 v_posed = v_shaped + posedirs pose_feature
   7 G_0 = [R_0 | J_0], G_j = G_parent [R_j | J_j - J_parent], A_j = [G_j.R | G_j.t - G_j.R J_j]
   8 T_v = sum_j W[v,j] A_j        9 vertex_v = T_v [v_posed_v; 1]        10 joints_j = G_j.t

Also here: the input builders of the tests, the error measure, and the restatement as an nn.Module with the body-model call contract.
"""
import types

import numpy as np
import torch

F32 = np.float32


def rodrigues(r):
    """[..., 3] axis-angle -> [..., 3, 3], step 2 as written."""
    angle = torch.sqrt(((r + 1e-8) ** 2).sum(-1, keepdim=True))            # [..., 1]
    d = r / angle
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    zero = torch.zeros_like(dx)
    K = torch.stack([zero, -dz, dy, dz, zero, -dx, -dy, dx, zero], -1).reshape(*r.shape[:-1], 3, 3)
    eye = torch.eye(3, dtype=r.dtype, device=r.device)
    s, c = torch.sin(angle)[..., None], torch.cos(angle)[..., None]
    return eye + s * K + (1 - c) * (K @ K)


def lbs(arrays, betas, body_pose, global_orient=None):
    """(vertices [B,V,3], joints [B,J,3]).  arrays: dict of tensors v_template [V,3], shapedirs [V,3,NB], posedirs [V,3,P],
    J_regressor [J,V], weights [V,J] in the working dtype, and parents (J ints).  betas [1 or B, NB], body_pose [B, 3(J-1)],
    global_orient [B,3] or None = zeros."""
    vt, sd, pd, reg, W = (arrays[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights"))
    parents = [int(p) for p in arrays["parents"]]
    B, J = body_pose.shape[0], W.shape[1]
    if global_orient is None:
        global_orient = torch.zeros((B, 3), dtype=body_pose.dtype, device=body_pose.device)
    full = torch.cat([global_orient, body_pose], 1).reshape(B, J, 3)                       # 1
    R = rodrigues(full)                                                                   # 2   [B,J,3,3]
    feat = (R[:, 1:] - torch.eye(3, dtype=R.dtype, device=R.device)).reshape(B, -1)                         # 3
    v_shaped = vt[None] + torch.einsum("vcn,bn->bvc", sd, betas.expand(B, -1))             # 4
    J_rest = torch.einsum("jv,bvc->bjc", reg, v_shaped)                                    # 5
    v_posed = v_shaped + torch.einsum("vcp,bp->bvc", pd, feat)                             # 6
    GR, Gt = [R[:, 0]], [J_rest[:, 0]]                                                     # 7
    for j in range(1, J):
        p = parents[j]
        GR.append(GR[p] @ R[:, j])
        Gt.append((GR[p] @ (J_rest[:, j] - J_rest[:, p])[..., None])[..., 0] + Gt[p])
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)                                        # [B,J,3,3], [B,J,3]
    At = Gt - (GR @ J_rest[..., None])[..., 0]
    TR = torch.einsum("vj,bjrc->bvrc", W, GR)                                              # 8
    Tt = torch.einsum("vj,bjr->bvr", W, At)
    vertices = (TR @ v_posed[..., None])[..., 0] + Tt                                      # 9
    return vertices, Gt                                                                   # 10


class TorchBodyModel(torch.nn.Module):
    """lbs() with the call contract of the pipelines' smpl_model, in the dtype / on the device of its buffers."""

    def __init__(self, arrays):
        super().__init__()
        for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights"):
            self.register_buffer(k, torch.as_tensor(np.asarray(arrays[k])).float())
        self.parents = [int(p) for p in arrays["parents"]]

    def forward(self, betas=None, return_verts=True, body_pose=None, global_orient=None):
        a = {k: getattr(self, k) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
        a["parents"] = self.parents
        B = body_pose.shape[0]
        if betas is None:
            betas = torch.zeros((1, self.shapedirs.shape[2]), dtype=body_pose.dtype, device=body_pose.device)
        v, j = lbs(a, betas, body_pose, global_orient)
        return types.SimpleNamespace(vertices=v, joints=j)


def relative_error(y, y64):
    """E(y) = max|y - y64| / max|y64| (0 when both are all zero)."""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    scale = np.abs(y64).max() if y64.size else 0.0
    err = np.abs(y - y64).max() if y64.size else 0.0
    return 0.0 if err == 0.0 else err / scale


# ------------------------------------------------------------------------------------------------ inputs
def body(V, J=24, NB=10, seed=5, dense=False):
    """random_smpl_arrays as fp32 numpy; dense = every skinning weight non-zero."""
    from smpl_nerf_amd.synthetic_smpl import random_smpl_arrays
    a = random_smpl_arrays(seed, n_vertices=V, n_joints=J, num_betas=NB)
    if dense:
        w = np.random.default_rng(seed + 1).random((V, J)) + 0.05
        a["weights"] = (w / w.sum(1, keepdims=True)).astype(F32)
    return a


def poses(B, J, seed, lo=0.05, hi=2.5):
    """[B, J, 3] fp32 axis-angle vectors with |r| uniform in [lo + margin, hi - margin], random axes."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=(B, J, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    angle = rng.uniform(lo + 0.01, hi - 0.01, (B, J, 1))
    return (axis * angle).astype(F32)


def op_inputs(B, V, J=24, NB=10, seed=1, betas_rows=None, orient=True, dense=False):
    """(arrays, betas [1 or B, NB], body_pose [B, 3(J-1)], global_orient [B,3] or None, d_vertices [B,V,3], d_joints [B,J,3]), fp32 numpy."""
    rng = np.random.default_rng(seed)
    a = body(V, J, NB, seed + 100, dense)
    full = poses(B, J, seed + 200)
    rows = B if betas_rows is None else betas_rows
    betas = rng.normal(0, 1.0, (rows, NB)).astype(F32)
    return (a, betas, full[:, 1:].reshape(B, -1).copy(), full[:, 0].copy() if orient else None,
            rng.normal(0, 1.0, (B, V, 3)).astype(F32), rng.normal(0, 1.0, (B, J, 3)).astype(F32))


def angles(body_pose, global_orient):
    """The J rotation angles per pose as the formula computes them, in float64."""
    full = np.concatenate([np.zeros_like(body_pose[:, :3]) if global_orient is None else global_orient, body_pose], 1).astype(np.float64)
    return np.sqrt(((full.reshape(full.shape[0], -1, 3) + 1e-8) ** 2).sum(-1))


def restated(inputs, dtype, which=("vertices", "joints"), need_grad=True):
    """lbs() on the CPU in `dtype` and, with need_grad, its autograd gradients for incoming gradients on `which`: dict of numpy arrays."""
    a, betas, pose, orient, d_v, d_j = inputs
    A = {k: (torch.from_numpy(np.asarray(v)).to(dtype) if k != "parents" else v) for k, v in a.items()}
    b, p = (torch.from_numpy(x).to(dtype).requires_grad_(need_grad) for x in (betas, pose))
    g = None if orient is None else torch.from_numpy(orient).to(dtype).requires_grad_(need_grad)
    v, j = lbs(A, b, p, g)
    r = {"vertices": v, "joints": j}
    if need_grad:
        loss = 0
        if "vertices" in which:
            loss = loss + (v * torch.from_numpy(d_v).to(dtype)).sum()
        if "joints" in which:
            loss = loss + (j * torch.from_numpy(d_j).to(dtype)).sum()
        loss.backward()
        r.update(d_betas=b.grad, d_body_pose=p.grad)
        if g is not None:
            r["d_global_orient"] = g.grad
    return {k: t.detach().numpy() for k, t in r.items()}
