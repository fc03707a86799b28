"""Torch (CPU) restatement of the image-wise model's linear-attention warp (solver/image_wise_solver.py:89-105), used ONLY by tests.

    d_sv = |p_s - g_v|     x_sv = relu(r - d_sv)     a_sv = x_sv / (sum_u x_su + eps)     warp_s = sum_v a_sv (c_v - g_v)

ONE body (g, c: [V, 3] or [1, V, 3]) for all rays.  warp_linear() is the reference's expression in the dtype of its inputs and
differentiable by autograd: in float64 it is the truth of the GPU tests, in fp32 what fp32 arithmetic can be asked for.
closed_form_grads() holds the gradients as csrc/image_warp.hip evaluates them, derived by hand; tests/test_image_warp_host.py
checks them against float64 autograd.  Also here: the planted inputs of the op's tests, the margin they require of their inputs,
and the pipeline in torch (tests/torch_ref.py for net and compositing).
"""
import numpy as np
import torch

from vertex_warp_ref import plant, relative_error  # noqa: F401  (E(y) = max|y - y64| / max|y64|)

F32 = np.float32
EPS = 1e-5


def _pairs(samples, goal):
    return torch.norm(samples[:, :, None, :] - goal.reshape(1, 1, -1, 3), dim=-1)       # [B, S, V]


def warp_linear(samples, goal, canon, ray_o, radius, eps=EPS):
    """(warp, warped, sdirs), each [B, S, 3]; image_wise_solver.py:89-105, operation for operation."""
    x = torch.relu(-(_pairs(samples, goal) - radius))
    a = x / (x.sum(-1, keepdim=True) + eps)
    warp = ((canon - goal).reshape(1, 1, -1, 3) * a[..., None]).sum(dim=-2)
    warped = samples + warp
    return warp, warped, warped - ray_o[:, None, :]


def closed_form_grads(samples, goal, canon, dW, radius, eps=EPS):
    """float64 numpy: (d_goal [V,3], d_canon [V,3], d_samples [B,S,3]) of sum(warp * dW) - the attention path only, without the
    identity terms of warped and sdirs - by the closed forms of csrc/image_warp.hip:
        dx_sv = (dW_s . w_v - dW_s . warp_s) / D_s  where x_sv > 0;   d_canon[v] = sum_s (x_sv / D_s) dW_s;
        d_goal[v] = -d_canon[v] + sum_s dx_sv (p_s - g_v) / d_sv;     d_samples[s] = -sum_v dx_sv (p_s - g_v) / d_sv;
        no distance term from a pair with d = 0."""
    p = np.asarray(samples, np.float64).reshape(-1, 3)
    g, c = np.asarray(goal, np.float64).reshape(-1, 3), np.asarray(canon, np.float64).reshape(-1, 3)
    dW = np.asarray(dW, np.float64).reshape(-1, 3)
    diff = p[:, None, :] - g[None, :, :]
    d = np.sqrt((diff ** 2).sum(-1))
    x = np.maximum(radius - d, 0.0)
    D = x.sum(-1) + eps
    w = c - g
    warp = (x @ w) / D[:, None]
    dx = np.where(x > 0, (dW @ w.T - (dW * warp).sum(-1)[:, None]) / D[:, None], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(d > 0, dx / d, 0.0)
    d_canon = (x / D[:, None]).T @ dW
    dist = (k[:, :, None] * diff).sum(0)
    d_samples = -(k[:, :, None] * diff).sum(1)
    return dist - d_canon, d_canon, d_samples.reshape(np.asarray(samples).shape)


def radius_margin(samples, goal, radius):
    """(min |d - r| / r, min d) over all pairs, in float64: the gradient is discontinuous at d = r (the ReLU) and at d = 0 (the norm)."""
    d = _pairs(torch.as_tensor(samples, dtype=torch.float64), torch.as_tensor(goal, dtype=torch.float64))
    return float((d - radius).abs().min()) / radius, float(d.min())


def op_inputs(B, S, V, radius, seed, spread=0.3):
    """vertex_warp_ref.op_inputs with one body: goal, canonical [V, 3] ~ N(0, spread), samples in the body's box with every third one
    planted within N(0, 0.4 r) of a goal vertex, ray origins, and three incoming gradients [B S, 3]; fp32 numpy."""
    rng = np.random.default_rng(seed)
    goal = rng.normal(0, spread, (V, 3)).astype(F32)
    canon = rng.normal(0, spread, (V, 3)).astype(F32)
    samples = plant(rng.uniform(-2 * spread, 2 * spread, (B, S, 3)), np.broadcast_to(goal, (B, V, 3)), radius, rng)
    ray_o = rng.normal(0, 2.0, (B, 3)).astype(F32)
    grads = [rng.normal(0, 1.0, (B * S, 3)).astype(F32) for _ in range(3)]
    return samples, goal, canon, ray_o, grads


def reference_grads(samples, goal, canon, ray_o, grads, radius, dtype, eps=EPS, use=(0, 1, 2)):
    """warp and the autograd gradients of sum_i sum(out_i * grads[i]), i in `use`, of warp_linear in `dtype`:
    dict of numpy arrays warp [B S, 3], d_goal, d_canon [V, 3], d_samples [B, S, 3] (the identity paths of warped and sdirs included)."""
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)      # noqa: E731
    p, g, c = (T(a).requires_grad_(True) for a in (samples, goal, canon))
    outs = warp_linear(p, g, c, T(ray_o), radius, eps)
    loss = sum((outs[i].reshape(-1, 3) * T(grads[i])).sum() for i in use)
    loss.backward()
    return dict(warp=outs[0].detach().reshape(-1, 3).numpy(), d_goal=g.grad.numpy(), d_canon=c.grad.numpy(), d_samples=p.grad.numpy())


# ------------------------------------------------------------------------------------------------ the fixture's inputs
G22 = dict(R=24, S=32, V=1000, batchsize=12, body_seed=22, net_seed=402, plant_seed=221, shuffle_seed=222, radius=0.01,
           frames=[dict(h=128, w=128, phi=4.0, theta=-20.0), dict(h=128, w=128, phi=40.0, theta=10.0)],
           arm_angle_l=0.17453292, arm_angle_r=0.17453292, truth_l=0.3, truth_r=-0.2, lrate=2e-5, lrate_pose=1e-3, param_stride=1009)


def g22_inputs():
    """The inputs of tests/golden/g22_image_wise.npz from its seeds: (images: per image the fp32 numpy list [ray_samples [R,S,3]
    (a third planted within the radius of a goal vertex of the body at the initial arm angles), ray_translation, ray_direction,
    z_vals [S] (ONE row for the image, as the reference hands to raw2outputs), rgb_truth], body model, net parameters).  The rays of
    an image are R pixels spread over a 128 x 128 frame, their samples at the mid-bin depths (the same row for every ray)."""
    from smpl_nerf_amd import synthetic as syn
    from smpl_nerf_amd.synthetic_smpl import LinearBodyModel
    c = G22
    body = LinearBodyModel(seed=c["body_seed"], n_vertices=c["V"])
    pose = np.zeros((1, 69), F32)
    pose[0, 38], pose[0, 41] = c["arm_angle_l"], c["arm_angle_r"]
    goal = body(body_pose=torch.from_numpy(pose)).vertices.numpy()                      # [1, V, 3]
    rng = np.random.default_rng(c["plant_seed"])
    images = []
    for i, frame in enumerate(c["frames"]):
        data = syn.frame_batch(n_coarse=c["S"], jitter=0.5, **frame)
        sub = np.arange(c["R"]) * (128 * 128 // c["R"]) + 37 + 11 * i
        assert np.array_equal(data[3][sub], np.broadcast_to(data[3][sub[0]], (c["R"], c["S"])))
        samples = plant(data[0][sub], np.broadcast_to(goal, (c["R"], c["V"], 3)), c["radius"], rng)
        images.append([samples, data[1][sub], data[2][sub], data[3][sub[0]].copy(), data[4][sub]])
    return images, body, syn.make_scene_net_params(c["net_seed"])


# ------------------------------------------------------------------------------------------------ the pipeline
def image_wise_forward(P, goal, canon, batch, radius, eps=EPS):
    """image_wise_solver.py:89-116 in torch, in the dtype of its inputs: (rgb, warp, warped, densities).  P: RenderRayNet
    parameters (tensors), goal / canon: the image's body [1, V, 3], batch: (ray_samples, ray_translation, z_vals [S] or [B, S])."""
    import torch_ref as TR
    samples, ray_o, z = batch
    B, S = samples.shape[:2]
    warp, warped, sdirs = warp_linear(samples, goal, canon, ray_o, radius, eps)
    dn = sdirs / torch.norm(sdirs, dim=-1, keepdim=True)
    inp = torch.cat([TR.posenc(warped, 10, 0).view(B * S, -1), TR.posenc(dn, 4, 0).view(B * S, -1)], -1)
    raw = TR.render_ray_net(P, inp).view(B, S, 4)
    rgb, _, dens = TR.raw2outputs(raw, z if z.dim() == 2 else z.expand(B, S), sdirs, 0)
    return rgb, warp, warped, dens


def train_steps(images, body, params, step_rays, dtype, config=None):
    """ImageWiseSolver.train (image_wise_solver.py:64-129) in torch on the CPU, in `dtype`, over the recorded ray batches:
    step_rays [steps, batchsize] are the rays of every step, R // batchsize consecutive steps per image.  Per image the body is
    posed once; per step forward, MSE, backward(retain_graph=True) and one torch.optim.Adam step over two groups (the net at
    lrate, the arm angles at lrate_pose).  Returns dict(step_rgb [steps, batchsize, 3], step_loss [steps], arm_angle_l,
    arm_angle_r, param_sample, adam_steps) like the fixture."""
    import copy
    c = config or G22
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)      # noqa: E731
    P = {k: T(v).requires_grad_(True) for k, v in params.items()}
    b = copy.deepcopy(body).to(dtype)
    arm_l, arm_r = (T([[c[k]]]).requires_grad_(True) for k in ("arm_angle_l", "arm_angle_r"))
    opt = torch.optim.Adam([{"params": list(P.values())}, {"params": [arm_l, arm_r], "lr": c["lrate_pose"]}], lr=c["lrate"],
                           betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    per_image = c["R"] // c["batchsize"]
    rgbs, losses = [], []
    for k, rays in enumerate(np.asarray(step_rays)):
        image = images[k // per_image]
        if k % per_image == 0:
            zero = torch.zeros(1, 69, dtype=dtype)
            pose = torch.cat([zero[:, :38], arm_l, zero[:, 39:41], arm_r, zero[:, 42:]], -1)
            canon, goal = b(body_pose=zero).vertices, b(body_pose=pose).vertices
        batch = (T(image[0][rays]), T(image[1][rays]), T(image[3]))
        rgb = image_wise_forward(P, goal, canon, batch, c["radius"])[0]
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(rgb, T(image[4][rays]))
        loss.backward(retain_graph=True)
        opt.step()
        rgbs.append(rgb.detach().numpy())
        losses.append(loss.item())
    flat = torch.cat([p.detach().reshape(-1) for p in P.values()]).numpy()
    return dict(step_rgb=np.array(rgbs), step_loss=np.array(losses), arm_angle_l=arm_l.detach().numpy(), arm_angle_r=arm_r.detach().numpy(),
                param_sample=flat[::c["param_stride"]], adam_steps=np.array([int(opt.state[p]["step"]) for p in P.values()]))
