"""Torch (CPU) restatement of the reference's ssim / _ssim_per_channel (util/scores.py:88-173) with a SEPARABLE window given as
win[k], used ONLY by tests: the same code in fp32 and in float64.

    mu1 = G*x  mu2 = G*y  e11 = G*(x x)  e22 = G*(y y)  e12 = G*(x y)          G = win (x) win, valid correlation (F.conv2d, groups = C)
    s11 = e11 - mu1^2  s22 = e22 - mu2^2  s12 = e12 - mu1 mu2
    A = mu1^2 + mu2^2 + c1   D = s11 + s22 + c2   L = (2 mu1 mu2 + c1) / A   CS = (2 s12 + c2) / D   S = L CS
    ssim[n,c] = mean_q S     cs[n,c] = mean_q CS     sqerr[n,c] = sum_pixels (x - y)^2

restated() also differentiates sum(gS ssim + gC cs) by autograd (dx, dy) and, in float64, returns the two CONDITIONING FLOORS the
GPU tests bound the kernel with (u = 2^-24, cond = (e11 + e22) / D per window):

    value floor [N,C]   16 u mean_q cond + 4 u          the forward error of the cancellation e - mu^2, divided by D
    gradient floor      16 u max_p Gamma[p], Gamma = G^T(|u| (2|mu2| + 2|mu1||L|) / A (1 + cond) + cond |w| (2|mu2| + 2|mu1||CS|) / D)
                                                         + 2|x| G^T(cond |b|) + |y| G^T(cond |c|)      (F.conv_transpose2d)
                        - the gradient with every term made absolute and weighted by its conditioning; w = (gS L + gC) / P,
                        u = gS CS / P, b = -w CS / D, c = 2 w / D.  For dy: the same with x and y swapped.

Also here: the seeded image families of the GPU tests, the cases of tests/golden/g20_image_scores.npz and the bound itself."""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
U = 2.0 ** -24
FACTOR = 8.0            # the project's usual factor on the fp32 CPU restatement's own error (tests/test_gpu_gmm.py)
FAMILIES = ("random", "noise", "ramp", "constant", "halfblack")
# name -> (shape, family, k, sigma, data_range, seed)
G20_CASES = {
    "textured": ((2, 3, 24, 29), "noise", 11, 1.5, 1.0, 201),
    "one_window": ((1, 3, 11, 11), "noise", 11, 1.5, 1.0, 202),
    "ramp_k7": ((1, 1, 16, 40), "ramp", 7, 1.5, 1.0, 203),
    "range255": ((1, 3, 20, 23), "noise", 11, 1.5, 255.0, 204),
}


def window(k, sigma):
    """The 1-D window as ops.ssim_window builds it (float64 Gaussian, normalised, rounded to fp32 once)."""
    i = np.arange(k, dtype=np.float64) - (k - 1) / 2.
    g = np.exp(-(i ** 2) / (2. * sigma ** 2))
    return (g / g.sum()).astype(F32)


def constants(data_range=1., k1=0.01, k2=0.03):
    """c1, c2 as the C entry receives them: (k data_range)^2 in Python floats, rounded to fp32."""
    return float(F32((k1 * data_range) ** 2)), float(F32((k2 * data_range) ** 2))


def images(family, shape, seed, data_range=1.):
    """x, y fp32 numpy [N,C,H,W] in [0, data_range] (up to the noise)."""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    if family == "random":
        x, y = rng.uniform(0, 1, shape), rng.uniform(0, 1, shape)
    elif family == "noise":       # a textured image: two waves per channel and pixel noise; y = x + 0.02 noise
        ph = rng.uniform(0, 2 * np.pi, (N, C, 1, 1, 2))
        x = 0.5 + 0.2 * np.sin(0.9 * xx + 0.4 * yy + ph[..., 0]) + 0.15 * np.cos(0.3 * xx - 1.1 * yy + ph[..., 1]) + 0.1 * rng.uniform(-1, 1, shape)
        y = x + 0.02 * rng.normal(0, 1, shape)
    elif family == "ramp":        # smooth: the variances are small against the means
        x = np.broadcast_to(0.1 + 0.8 * (xx / max(W - 1, 1) * 0.7 + yy / max(H - 1, 1) * 0.3), shape) + np.zeros(shape)
        y = x + 0.01 * rng.normal(0, 1, shape)
    elif family == "constant":
        x, y = np.full(shape, 0.9), np.full(shape, 0.3)
    elif family == "halfblack":   # a step edge, and the same edge one pixel further
        x = np.zeros(shape)
        x[..., W // 2:] = 1.0
        y = np.zeros(shape)
        y[..., W // 2 + 1:] = 1.0
    else:
        raise KeyError(family)
    return (x * data_range).astype(F32), (y * data_range).astype(F32)


def upstream(N, C, seed):
    """Random gradients arriving at ssim and cs, fp32 [N,C]."""
    rng = np.random.default_rng(seed + 7)
    return rng.normal(0, 1, (N, C)).astype(F32), rng.normal(0, 1, (N, C)).astype(F32)


def _moments(x, y, G, C):
    conv = lambda t: F.conv2d(t, weight=G, stride=1, padding=0, groups=C)      # noqa: E731
    return conv(x), conv(y), conv(x * x), conv(y * y), conv(x * y)


def _maps(x, y, G, C, c1, c2):
    mu1, mu2, e11, e22, e12 = _moments(x, y, G, C)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11, s22, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu1_mu2
    A, D = mu1_sq + mu2_sq + c1, s11 + s22 + c2
    L, CS = (2 * mu1_mu2 + c1) / A, (2 * s12 + c2) / D
    return dict(mu1=mu1, mu2=mu2, e11=e11, e22=e22, A=A, D=D, L=L, CS=CS)


def restated(x, y, win, c1, c2, gS=None, gC=None, dtype=torch.float64):
    """x, y fp32 numpy [N,C,H,W], win fp32 numpy [k], gS / gC fp32 numpy [N,C] (None: no gradients) -> dict of numpy arrays: ssim,
    cs, sqerr [N,C]; dx, dy [N,C,H,W]; in float64 also value_floor [N,C] and, with gradients, grad_floor_x, grad_floor_y (scalars)."""
    C = x.shape[1]
    w = torch.from_numpy(np.asarray(win)).to(dtype)
    G = (w[:, None] * w[None, :])[None, None].repeat(C, 1, 1, 1)
    xt, yt = torch.from_numpy(x).to(dtype).requires_grad_(gS is not None), torch.from_numpy(y).to(dtype).requires_grad_(gS is not None)
    m = _maps(xt, yt, G, C, c1, c2)
    ssim, cs = (m["L"] * m["CS"]).mean(dim=(-1, -2)), m["CS"].mean(dim=(-1, -2))
    out = {"ssim": ssim.detach().numpy(), "cs": cs.detach().numpy(), "sqerr": ((xt - yt) ** 2).sum(dim=(-1, -2)).detach().numpy()}
    if gS is not None:
        gs, gc = torch.from_numpy(gS).to(dtype), torch.from_numpy(gC).to(dtype)
        (gs * ssim + gc * cs).sum().backward()
        out["dx"], out["dy"] = xt.grad.numpy(), yt.grad.numpy()
    if dtype != torch.float64:
        return out
    with torch.no_grad():
        m = {k: v.detach() for k, v in m.items()}
        cond = (m["e11"] + m["e22"]) / m["D"]
        out["value_floor"] = (16 * U * cond.mean(dim=(-1, -2)) + 4 * U).numpy()
        if gS is not None:
            P = cond.shape[-1] * cond.shape[-2]
            ww = (gs[:, :, None, None] * m["L"] + gc[:, :, None, None]) / P
            uu = gs[:, :, None, None] * m["CS"] / P
            b, c = -ww * m["CS"] / m["D"], 2 * ww / m["D"]
            T = lambda t: F.conv_transpose2d(t, weight=G, stride=1, padding=0, groups=C)      # noqa: E731

            def gamma(p, q, mu_p, mu_q):      # for the gradient to p: mu_p its own mean, mu_q the other image's
                first = (uu.abs() * (2 * mu_q.abs() + 2 * mu_p.abs() * m["L"].abs()) / m["A"] * (1 + cond)
                         + cond * ww.abs() * (2 * mu_q.abs() + 2 * mu_p.abs() * m["CS"].abs()) / m["D"])
                return T(first) + 2 * p.abs() * T(cond * b.abs()) + q.abs() * T(cond * c.abs())

            out["grad_floor_x"] = 16 * U * float(gamma(xt.detach(), yt.detach(), m["mu1"], m["mu2"]).max())
            out["grad_floor_y"] = 16 * U * float(gamma(yt.detach(), xt.detach(), m["mu2"], m["mu1"]).max())
    return out


def hold(tag, got, y32, y64, lines=None, extra=None):
    """The bounds of the module docstring on whatever of ssim, cs, sqerr, dx, dy `got` holds; prints (and appends to `lines`) every
    figure before asserting.  `extra`: name -> further yardstick error allowed (the golden tests' second reference)."""
    failures = []
    for name in ("ssim", "cs", "sqerr", "dx", "dy"):
        if name not in got:
            continue
        g, a, b = np.asarray(got[name], np.float64), np.asarray(y32[name], np.float64), y64[name]
        assert np.isfinite(g).all(), f"{tag} {name}: non-finite values"
        if name in ("ssim", "cs"):
            ek, ec, floor = np.abs(g - b), np.abs(a - b), y64["value_floor"]
        elif name == "sqerr":
            scale = np.where(b == 0, 1.0, np.abs(b))
            ek, ec, floor = np.abs(g - b) / scale, np.abs(a - b) / scale, np.full(b.shape, 4 * U)
        else:
            ek, ec, floor = np.abs(g - b).max(), np.abs(a - b).max(), y64["grad_floor_" + name[1]]
        more = 0.0 if extra is None else extra.get(name, 0.0)
        bound = np.maximum(np.maximum(FACTOR * ec, floor), more)
        worst = int(np.argmax(ek / bound)) if np.ndim(ek) else 0
        pick = lambda v: float(np.reshape(v, -1)[worst]) if np.ndim(v) else float(v)      # noqa: E731
        line = (f"{tag} {name}: kernel error {pick(ek):.3e}  fp32 CPU error {pick(ec):.3e}  floor {pick(floor):.3e}  "
                f"kernel / bound {pick(ek) / pick(bound):.3f}")
        print(line)
        if lines is not None:
            lines.append(line)
        if not np.all(ek <= bound):
            failures.append(line)
    assert not failures, "\n".join(failures)
