"""Torch (CPU) restatement of the soft silhouette's rule (include/smplnerf.h, snerf_soft_silhouette_fwd_f32), used ONLY by tests and
tools: the whole rule, vectorised over pixels x faces, in ONE dtype - float64 is the yardstick, float32 the comparison whose own
error sets the device's bound.  The gradient with respect to the vertices comes from autograd.  Also here: the error measure, the
seeded cases of tests/test_gpu_soft_silhouette.py and the conditions those cases rest on.
"""
import functools
import itertools

import numpy as np
import torch

import mesh_render_ref as MR
from smpl_nerf_amd import synthetic as syn

COORD_MAX = 2.0 ** 30
FLOOR = 2.0 ** -22                    # pairs whose liveness flips at the cutoff: each worth at most softplus(-17) = 4.1e-8


def focal_of(W):
    return float(.5 * W / np.tan(.5 * MR.ANGLE))


def project(vertices, pose, focal, H, W):
    """vertices [V,3] (a torch tensor of the working dtype), pose [4,4] float64 numpy -> (xy [V,2], depth [V]): the camera's
    rotation as float64 holds it and its origin rounded to fp32, both then in the working dtype."""
    dt = vertices.dtype
    R = torch.from_numpy(np.ascontiguousarray(pose[:3, :3])).to(vertices)
    o = torch.from_numpy(pose[:3, 3].astype(np.float32)).to(vertices)
    c = (vertices - o) @ R                                                   # R^T (v - o)
    depth = -c[:, 2]
    safe = torch.where(depth > 0, depth, torch.ones_like(depth))             # (a dead face never reaches the sum)
    x = W * 0.5 + focal * c[:, 0] / safe
    y = H * 0.5 - focal * c[:, 1] / safe
    return torch.stack([x, y], -1), depth


def pairs(xy, depth, faces, H, W):
    """Per pixel and face: d2 [P,F] to the nearest segment, d2 of the three segments [P,F,3], inside [P,F], live [F]."""
    dt = xy.dtype
    faces = torch.as_tensor(np.asarray(faces), dtype=torch.int64).to(xy.device)
    P = xy[faces]                                                            # [F,3,2]
    live = (depth[faces] > 0).all(1) & (P.detach().abs() < COORD_MAX).all(2).all(1)
    dummy = torch.tensor([[0., 0.], [1., 0.], [0., 1.]], dtype=dt, device=xy.device)
    P = torch.where(live[:, None, None], P, dummy)
    j, i = torch.meshgrid(torch.arange(H, dtype=dt, device=xy.device), torch.arange(W, dtype=dt, device=xy.device), indexing="ij")
    q = torch.stack([i.reshape(-1), j.reshape(-1)], -1)                      # [P,2]: the sample point of pixel (row j, column i)
    a, b = P, P[:, [1, 2, 0]]
    e = (b - a)[None]                                                        # [1,F,3,2]
    w = q[:, None, None, :] - a[None]                                        # [P,F,3,2]
    ee = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
    dot = w[..., 0] * e[..., 0] + w[..., 1] * e[..., 1]
    t = torch.where(ee > 0, dot / torch.where(ee > 0, ee, torch.ones_like(ee)), torch.zeros_like(dot)).clamp(0, 1)
    r = w - t[..., None] * e
    d2k = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]                       # [P,F,3]
    edge = e[..., 0] * w[..., 1] - e[..., 1] * w[..., 0]
    sign = (edge > 0).all(-1) | (edge < 0).all(-1)
    lo, hi = P.detach().min(1).values[None], P.detach().max(1).values[None]   # [1,F,2]
    in_box = ((q[:, None] >= lo) & (q[:, None] <= hi)).all(-1)
    return d2k.min(-1).values, d2k, sign & in_box, live


def silhouette_frame(vertices, pose, focal, H, W, faces, sigma, cutoff, want_pairs=False):
    xy, depth = project(vertices, pose, focal, H, W)
    d2, d2k, inside, live = pairs(xy, depth, faces, H, W)
    contributes = live[None] & (inside | (d2.detach() <= cutoff * sigma))
    z = torch.where(inside, d2, -d2) / sigma
    L = torch.where(contributes, -torch.nn.functional.logsigmoid(-z), torch.zeros_like(z)).sum(1)      # softplus(z)
    S = (-torch.expm1(-L)).reshape(H, W)
    return (S, d2k.detach(), inside, contributes) if want_pairs else S


def silhouette(poses, focal, H, W, vertices, faces, sigma=1.0, cutoff=17.0, dtype=torch.float64):
    """poses [N,4,4] float64 numpy, vertices a torch tensor [V,3] or [N,V,3] (any dtype and device; may require grad) -> S [N,H,W]
    in `dtype` on that device."""
    v = vertices.to(dtype)
    return torch.stack([silhouette_frame(v if v.dim() == 2 else v[n], np.asarray(poses[n], np.float64), focal, H, W, faces, sigma, cutoff)
                        for n in range(len(poses))])


def with_gradient(poses, focal, H, W, vertices, faces, sigma, cutoff, d_sil, dtype):
    """(S [N,H,W], d_vertices, shaped like vertices) as numpy float64, computed in `dtype`; vertices fp32 numpy."""
    v = torch.from_numpy(np.asarray(vertices, np.float32)).to(dtype).requires_grad_(True)
    S = silhouette(poses, focal, H, W, v, faces, sigma, cutoff, dtype)
    S.backward(torch.from_numpy(np.asarray(d_sil)).to(dtype))
    return S.detach().double().numpy(), v.grad.double().numpy()


def E(y, y64):
    """max|y - y64| / max|y64|"""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    return float(np.abs(y - y64).max() / np.abs(y64).max())


def bound(e32):
    """What the device may err by: 8 times the fp32 CPU restatement's own error, or the floor."""
    return max(8.0 * e32, FLOOR)


# ------------------------------------------------------------------------------------------------ the cases
SIZES = [(8, 8), (9, 13), (32, 32)]                 # one tile, clipped tiles, 16 tiles
FACES = [1, 20, 320, 1280]                          # one wave with work, the tail loop only, whole fours
FRAMES = [(1, 1), (3, 3), (3, 1)]                   # (N, bodies)
SIGMAS = [0.25, 1.0, 4.0]
CASES = [(H, W, F, N, bodies, sigma) for (H, W), F, (N, bodies), sigma in itertools.product(SIZES, FACES, FRAMES, SIGMAS)]


def case_inputs(H, W, F, N, bodies):
    s = MR.scene(H, W, F, N, bodies)
    v = s["vertices"] if bodies > 1 else s["vertices"][0]
    return s["poses"], focal_of(W), v, s["faces"]


def upstream(N, H, W, seed=7):
    """The seeded dS [N,H,W] fp32 of every gradient check."""
    return np.random.default_rng(seed).standard_normal((N, H, W)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(H, W, F, N, bodies, sigma, cutoff=17.0):
    """{dtype: (S, d_vertices)} of a case for float64 and float32, computed once and shared."""
    poses, focal, v, faces = case_inputs(H, W, F, N, bodies)
    dS = upstream(N, H, W)
    return {dt: with_gradient(poses, focal, H, W, v, faces, sigma, cutoff, dS, dt) for dt in (torch.float64, torch.float32)}


def inside_gap(poses, focal, H, W, vertices, faces, sigma, cutoff=17.0):
    """Among the contributing inside pairs of a case, in float64: the smallest relative gap (d_second - d_first) / d_second
    between the two smallest of the three segment distances - what keeps the nearest segment of an inside pair, and with it the
    gradient's branch, the same under fp32 rounding.  +inf when there is no such pair."""
    gap = np.inf
    v = torch.from_numpy(np.asarray(vertices, np.float32)).double()
    for n in range(len(poses)):
        _, d2k, inside, contributes = silhouette_frame(v if v.dim() == 2 else v[n], np.asarray(poses[n], np.float64), focal, H, W, faces,
                                                       sigma, cutoff, want_pairs=True)
        d = d2k[inside & contributes].sqrt().sort(-1).values
        if len(d):
            gap = min(gap, float(((d[:, 1] - d[:, 0]) / d[:, 1]).min()))
    return gap


# ------------------------------------------------------------------------------------------------ the fit
FIT = dict(H=32, W=32, sigma=1.0, lr=1e-2, iterations=40, seed=3, scale=0.25)


def fit_body():
    from smpl_nerf_amd.synthetic_smpl import surface_smpl_arrays
    return surface_smpl_arrays(3, level=2)


def fit_poses(cameras=1):
    return np.stack([syn.sphere_pose(10.0 + 15.0 * k, 25.0 + 70.0 * k, 2.4) for k in range(cameras)])


def fit_true_pose(J):
    """body_pose [1, 3 (J - 1)] drawn from N(0, 0.25^2) with a fixed seed"""
    return (np.random.default_rng(FIT["seed"]).standard_normal((1, 3 * (J - 1))) * FIT["scale"]).astype(np.float32)


def _lbs_arrays(dtype):
    a = fit_body()
    out = {k: torch.from_numpy(np.asarray(a[k])).to(dtype) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
    out["parents"] = [int(p) for p in a["parents"]]
    return out, a["faces"]


def chain_loss(body_pose, target, dtype, cameras=1):
    """The L1 loss of the fit through the CPU chain smpl_lbs_ref.lbs -> silhouette, in `dtype`; body_pose a torch tensor [1, 3 (J - 1)]."""
    import smpl_lbs_ref as LR
    arrays, faces = _lbs_arrays(dtype)
    betas = torch.zeros((1, arrays["shapedirs"].shape[2]), dtype=dtype)
    v = LR.lbs(arrays, betas, body_pose.to(dtype))[0][0]
    S = silhouette(fit_poses(cameras), focal_of(FIT["W"]), FIT["H"], FIT["W"], v, faces, FIT["sigma"], 17.0, dtype)
    return (S - torch.from_numpy(target).to(dtype)).abs().mean()


@functools.lru_cache(maxsize=None)
def fit_target(cameras=1):
    """The float64 silhouette of the true pose, rounded to fp32: [cameras, H, W] numpy."""
    J = len(fit_body()["parents"])
    import smpl_lbs_ref as LR
    arrays, faces = _lbs_arrays(torch.float64)
    v = LR.lbs(arrays, torch.zeros((1, arrays["shapedirs"].shape[2]), dtype=torch.float64), torch.from_numpy(fit_true_pose(J)).double())[0][0]
    return silhouette(fit_poses(cameras), focal_of(FIT["W"]), FIT["H"], FIT["W"], v, faces, FIT["sigma"]).numpy().astype(np.float32)


@functools.lru_cache(maxsize=None)
def cpu_fit(dtype=torch.float64, cameras=1):
    """The loss history of the fit on the CPU chain in `dtype`: zeros, Adam, lr and iterations of FIT."""
    J = len(fit_body()["parents"])
    pose = torch.zeros((1, 3 * (J - 1)), dtype=dtype, requires_grad=True)
    optim = torch.optim.Adam([pose], lr=FIT["lr"])
    history = []
    for _ in range(FIT["iterations"]):
        optim.zero_grad()
        loss = chain_loss(pose, fit_target(cameras), dtype, cameras)
        loss.backward()
        optim.step()
        history.append(float(loss.detach()))
    return history


@functools.lru_cache(maxsize=None)
def chain_gradient(dtype):
    """(loss, d loss / d body_pose [1, 3 (J - 1)] numpy float64) of the L1 loss at half the true pose, through the CPU chain."""
    J = len(fit_body()["parents"])
    pose = torch.from_numpy(0.5 * fit_true_pose(J)).to(dtype).requires_grad_(True)
    loss = chain_loss(pose, fit_target(), dtype)
    loss.backward()
    return float(loss.detach()), pose.grad.double().numpy()
