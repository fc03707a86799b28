"""Torch (CPU) restatement of DynamicPipeline's vertex-attention warp (models/dynamic_pipeline.py:51-70), used ONLY by tests.

    d_v = |p - g_v|     x_v = T relu(r - d_v)     a_v = (exp(x_v) - 1) / sum_u exp(x_u)     warp = sum_v a_v (c_v - g_v)

Two forms, both in the dtype of their inputs and differentiable by autograd:
  * warp_stable():          the per-sample maximum m = max_v x_v taken out, a_v = (exp(x_v - m) - exp(-m)) / sum_u exp(x_u - m) -
                            the yardstick of the GPU tests, in float64 (the truth) and in fp32 (what fp32 arithmetic can be asked for);
  * warp_reference_order(): the reference's own operations in its order (utils.py:57-60: ONE maximum over the whole batch), which
                            tests/test_vertex_warp_host.py pins to the outputs the reference produced (tests/golden/g17_dynamic.npz).
Also here: the inputs of that fixture, rebuilt from its seeds (the fixture stores no input), the planted samples every test of the
op uses, the margins the tests require of their inputs, and the whole pipeline in torch (tests/torch_ref.py for net and compositing).
"""
import numpy as np
import torch

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the op
def _pairs(samples, goal):
    return torch.norm(samples[:, :, None, :] - goal[:, None, :, :], dim=-1)       # [B, S, V]


def _finish(samples, goal, canon, ray_o, a):
    warp = (a[..., None] * (canon - goal)[:, None, :, :]).sum(dim=-2)             # [B, S, 3]
    warped = samples + warp
    return warp, warped, warped - ray_o[:, None, :]


def warp_stable(samples, goal, canon, ray_o, radius, temperature):
    """(warp, warped, sdirs), each [B, S, 3].  m is a constant of the expression (it cancels), so autograd does not follow it."""
    x = temperature * torch.relu(radius - _pairs(samples, goal))
    m = x.max(dim=-1, keepdim=True)[0].detach()
    e = torch.exp(x - m)
    a = (e - torch.exp(-m)) / e.sum(dim=-1, keepdim=True)
    return _finish(samples, goal, canon, ray_o, a)


def warp_reference_order(samples, goal, canon, ray_o, radius, temperature):
    """models/dynamic_pipeline.py:53-66 with utils.py:57-60, operation for operation."""
    x = temperature * torch.relu(-(_pairs(samples, goal) - radius))
    exp = torch.exp(x - torch.max(x))
    a = (exp - torch.exp(-torch.max(x))) / exp.sum(-1, keepdim=True)
    return _finish(samples, goal, canon, ray_o, a)


def relative_error(y, y64):
    """E(y) = max|y - y64| / max|y64| (0 when both are all zero)."""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    scale = np.abs(y64).max() if y64.size else 0.0
    err = np.abs(y - y64).max() if y64.size else 0.0
    return 0.0 if err == 0.0 else err / scale


def input_margins(samples, goal, radius):
    """(min |d - r|, min d) over all pairs, in float64: the gradient is discontinuous at d = r (the ReLU) and at d = 0 (the norm)."""
    d = _pairs(torch.as_tensor(samples, dtype=torch.float64), torch.as_tensor(goal, dtype=torch.float64))
    return float((d - radius).abs().min()), float(d.min())


# ------------------------------------------------------------------------------------------------ inputs
def plant(samples, goal, radius, rng, every=3):
    """About every `every`-th sample replaced by a goal vertex of its ray plus N(0, 0.4 r) noise, so that the attention has
    something in radius (ray samples of a 128 x 128 frame meet a 1 cm ball around a vertex almost never)."""
    B, S, _ = samples.shape
    V = goal.shape[1]
    vid = rng.integers(0, V, (B, S))
    noise = rng.normal(0.0, 0.4 * radius, (B, S, 3))
    mask = (np.arange(S)[None, :] + np.arange(B)[:, None]) % every == 0
    out = np.array(samples, dtype=np.float64)
    planted = np.asarray(goal, np.float64)[np.arange(B)[:, None], vid] + noise
    out[mask] = planted[mask]
    return out.astype(F32)


def op_inputs(B, S, V, radius, seed, spread=0.3):
    """Random bodies (goal, canonical ~ N(0, spread)), samples in the bodies' box with every third one planted, ray origins,
    and three incoming gradients; fp32 numpy."""
    rng = np.random.default_rng(seed)
    goal = rng.normal(0, spread, (B, V, 3)).astype(F32)
    canon = rng.normal(0, spread, (B, V, 3)).astype(F32)
    samples = plant(rng.uniform(-2 * spread, 2 * spread, (B, S, 3)), goal, radius, rng)
    ray_o = rng.normal(0, 2.0, (B, 3)).astype(F32)
    grads = [rng.normal(0, 1.0, (B * S, 3)).astype(F32) for _ in range(3)]
    return samples, goal, canon, ray_o, grads


G17 = dict(B=12, S=64, V=1000, body_seed=17, frame=dict(h=128, w=128, phi=4.0, theta=-20.0, seed=13), net_seed=401,
           plant_seed=171, pose_seed=172, radius=0.01, cases={"a": 10000.0, "b": 2000.0})


def body_vertices_np(body, poses):
    """LinearBodyModel.forward in numpy fp32 (same operations, same order)."""
    v0, v38, v41 = (getattr(body, n).numpy() for n in ("v0", "v38", "v41"))
    return (v0[None] + poses[:, 38, None, None] * v38[None]) + poses[:, 41, None, None] * v41[None]


def g17_inputs():
    """The inputs of tests/golden/g17_dynamic.npz from its seeds: (batch list of fp32 numpy arrays [ray_samples (planted),
    ray_translation, ray_direction, z_vals, image indices, rgb_truth], goal poses [n_images, 69], body model, net parameters)."""
    from smpl_nerf_amd import synthetic as syn
    from smpl_nerf_amd.synthetic_smpl import LinearBodyModel
    c = G17
    data = syn.frame_batch(**c["frame"])
    sub = np.arange(c["B"]) * (128 * 128 // c["B"]) + 37
    images = np.arange(c["B"]) % 10
    poses = syn.human_poses((41, 38), 0, 60, 10)
    poses = (poses + 0.05 * np.random.default_rng(c["pose_seed"]).normal(size=poses.shape)).astype(F32)
    body = LinearBodyModel(seed=c["body_seed"], n_vertices=c["V"])
    goal = body_vertices_np(body, poses[images])
    samples = plant(data[0][sub], goal, c["radius"], np.random.default_rng(c["plant_seed"]))
    batch = [samples, data[1][sub], data[2][sub], data[3][sub], images, data[4][sub]]
    return batch, poses, body, syn.make_scene_net_params(c["net_seed"])


# ------------------------------------------------------------------------------------------------ the pipeline
def dynamic_pipeline(P, body, goal_poses, batch, radius, temperature, form=warp_stable):
    """models/dynamic_pipeline.py:34-83 in torch, in the dtype of P / goal_poses: (rgb, warp, warped, densities).
    P: RenderRayNet parameters (tensors), body: a LinearBodyModel of that dtype, goal_poses: [n_images, 69] tensor (the
    estimator's table; gradients flow to it), batch: the data list as tensors."""
    import torch_ref as TR
    samples, ray_o, _, z, images, _ = batch
    B, S = z.shape
    poses = goal_poses[images]
    canon = body(body_pose=torch.zeros_like(poses)).vertices
    goal = body(body_pose=poses).vertices
    warp, warped, sdirs = form(samples, goal, canon, ray_o, radius, temperature)
    dn = sdirs / torch.norm(sdirs, dim=-1, keepdim=True)
    inp = torch.cat([TR.posenc(warped, 10, 0).view(B * S, -1), TR.posenc(dn, 4, 0).view(B * S, -1)], -1)
    raw = TR.render_ray_net(P, inp).view(B, S, 4)
    rgb, _, dens = TR.raw2outputs(raw, z, sdirs, 0)
    return rgb, warp, warped, dens
