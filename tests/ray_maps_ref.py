"""The ray maps (include/smplnerf.h "ray maps"; utils.py:184, :187) as vectorised torch-CPU functions, and the seeded cases the
host and the GPU tests share.

ray_maps() follows the rule operation by operation in the dtype of its inputs: in float64 it is the yardstick, in float32 the
plain-torch restatement whose distance from the yardstick sets the bound of the device tests (the device may not
be worse than eight times what fp32 torch does).  Its backward is autograd's; ray_maps_bwd() is the analytic formula the device
kernel evaluates, held to autograd in tests/test_ray_maps_host.py.
"""
import numpy as np
import torch

# (B, N) of the golden g29_ray_maps.npz
GOLDEN_SHAPES = ((3, 1), (5, 2), (4, 65), (2, 192))
GOLDEN_SEED = 2901


def _dot3(a, b):
    """a . b over the last axis, the three products summed in x, y, z order."""
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def sample_parameter(o, d, pts):
    """Step 1 with points: t = ((p - o) . d) / (d . d), 0 where d . d == 0.  o, d [B,3], pts [B,N,3] -> [B,N]."""
    dd = _dot3(d, d)[:, None]
    num = _dot3(pts - o[:, None, :], d[:, None, :])
    return torch.where(dd == 0, torch.zeros_like(num), num / torch.where(dd == 0, torch.ones_like(dd), dd))


def transmittance(alpha):
    """Steps 2 and 3: (u, T) with u = 1 - alpha + 1e-10 in the dtype of alpha (in float32: fl32(fl32(1 - alpha) + 1e-10f)) and
    T the exclusive prefix product of u."""
    u = 1. - alpha + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(u[:, :1]), u[:, :-1]], -1), -1)
    return u, T


def ray_maps(alpha, o, d, z=None, pts=None):
    """(acc [B], depth [B], point [B,3] or None) of alpha [B,N] and exactly one of z [B,N] and pts [B,N,3]."""
    assert (z is None) != (pts is None)
    t = z if pts is None else sample_parameter(o, d, pts)
    _, T = transmittance(alpha)
    w = alpha * T
    acc = torch.sum(w, -1)
    depth = torch.sum(w * t, -1)
    point = None if pts is None else torch.sum(w[..., None] * pts, -2)
    return acc, depth, point


def ray_maps_bwd(alpha, o, d, z=None, pts=None, d_acc=None, d_depth=None, d_point=None):
    """The analytic d alpha [B,N]: with G_i = d_acc + d_depth t_i + <d_point, p_i> and S_k = sum_{i>k} w_i G_i,
    d alpha_k = T_k G_k - S_k / u_k.  S is the exclusive suffix sum, shifted - not the inclusive one minus its own term."""
    t = z if pts is None else sample_parameter(o, d, pts)
    u, T = transmittance(alpha)
    G = torch.zeros_like(alpha)
    if d_acc is not None:
        G = G + d_acc[:, None]
    if d_depth is not None:
        G = G + d_depth[:, None] * t
    if d_point is not None:
        G = G + _dot3(d_point[:, None, :], pts)
    q = alpha * T * G
    incl = torch.flip(torch.cumsum(torch.flip(q, [-1]), -1), [-1])            # sum_{i>=k}
    S = torch.cat([incl[:, 1:], torch.zeros_like(incl[:, :1])], -1)           # sum_{i>k}: shifted
    return T * G - S / u


def ray_maps_autograd(alpha, o, d, z=None, pts=None, d_acc=None, d_depth=None, d_point=None):
    """((acc, depth, point), d alpha) with autograd's backward of ray_maps() for the given upstream gradients (None = zeros)."""
    a = alpha.detach().clone().requires_grad_(True)
    acc, depth, point = ray_maps(a, o, d, z, pts)
    loss = acc.sum() * 0
    for out, g in ((acc, d_acc), (depth, d_depth), (point, d_point)):
        if g is not None:
            loss = loss + (out * g).sum()
    loss.backward()
    return (acc.detach(), depth.detach(), None if point is None else point.detach()), a.grad


def cast(case, dtype):
    """The tensors of a case in `dtype` (None stays None)."""
    return {k: (v if v is None else v.to(dtype)) for k, v in case.items()}


# ---- seeded cases --------------------------------------------------------------------------------------------------------
def make_case(B, N, seed):
    """Float32 CPU tensors: alpha [B,N] of a plausible march (runs of empty space, thin matter and a few opaque samples; odd rays
    dense, even rays thin, so that long rays keep transmittance to their end), rays, ascending z in [2, 6], pts = o + z d in
    fp32, and the three upstream gradients."""
    g = torch.Generator().manual_seed(seed * 1000003 + B * 4099 + N)
    r = torch.rand(B, N, generator=g)
    scale = torch.where(torch.arange(B) % 2 == 1, torch.tensor(0.9), torch.tensor(min(1.0, 8.0 / N)))[:, None]
    alpha = (r ** 4) * scale
    alpha[torch.rand(B, N, generator=g) < 0.3] = 0.0
    if N >= 8:
        alpha[torch.rand(B, N, generator=g) < 1.0 / N] = 1.0
    o = torch.randn(B, 3, generator=g)
    d = torch.randn(B, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True) * (0.5 + torch.rand(B, 1, generator=g))      # not normalised, like get_rays'
    z = torch.sort(2.0 + 4.0 * torch.rand(B, N, generator=g), -1)[0]
    pts = o[:, None, :] + z[..., None] * d[:, None, :]
    return {"alpha": alpha.float(), "o": o, "d": d, "z": z, "pts": pts, "d_acc": torch.randn(B, generator=g),
            "d_depth": torch.randn(B, generator=g), "d_point": torch.randn(B, 3, generator=g)}


EDGE_ROWS = ("zeros", "first_one", "middle_one", "all_ones", "almost_one", "d_zero")


def make_edge_case(N, seed=77):
    """One ray per EDGE_ROWS name, on make_case's rays: alpha all 0; alpha_0 = 1; alpha = 1 in the middle; alpha = 1 everywhere;
    one alpha of 0.99999994 (the fp32 number below 1: u = fl32(2^-24 + 1e-10)); d = 0 (the points mode's t = 0)."""
    c = make_case(len(EDGE_ROWS), N, seed)
    a = c["alpha"].clamp(max=0.5)
    a[0] = 0.0
    a[1, 0] = 1.0
    a[2, N // 2] = 1.0
    a[3] = 1.0
    a[4, N // 2] = 0.99999994
    c["alpha"] = a
    c["d"][5] = 0.0
    c["pts"] = c["o"][:, None, :] + c["z"][..., None] * c["d"][:, None, :]
    return c


def golden_inputs(B, N):
    """The seeded raw [B,N,4], z [B,N], dirs [B,3] and upstream gradients g_depth, g_acc [B] of the golden's case (float32
    numpy; make_golden_ray_maps.py stores them too)."""
    rng = np.random.default_rng(GOLDEN_SEED + 131 * B + N)
    raw = rng.normal(size=(B, N, 4)).astype(np.float32)
    raw[..., 3] = (rng.normal(size=(B, N)) * (3.0 if N > 2 else 1.0)).astype(np.float32)
    if N >= 65:
        raw[0, N // 3, 3] = 5e3          # an opaque sample: alpha = 1 in the middle of a ray
    z = np.sort(rng.uniform(2.0, 6.0, (B, N)).astype(np.float32), -1)
    dirs = rng.normal(size=(B, 3)).astype(np.float32)
    return {"raw": raw, "z": z, "dirs": dirs, "g_depth": rng.normal(size=B).astype(np.float32),
            "g_acc": rng.normal(size=B).astype(np.float32)}


def raw2alpha(raw, z, dirs):
    """utils.py:161-175 in the dtype of its inputs: the alpha of raw2outputs (N == 1: ones, :170-171)."""
    if z.shape[-1] == 1:
        return torch.ones_like(z)
    dists = z[..., 1:] - z[..., :-1]
    dists = torch.cat([dists, torch.full_like(dists[..., :1], 1e10)], -1) * torch.norm(dirs, dim=-1)[:, None]
    return 1. - torch.exp(-torch.relu(raw[..., 3]) * dists)
