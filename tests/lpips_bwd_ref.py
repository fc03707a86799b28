"""The backward of LPIPS restated on the CPU (util/scores.py:286-411: ContentLoss is a _Loss, differentiable to both frames, its
weights frozen) - the yardstick of tests/test_lpips_bwd_host.py and tests/test_gpu_lpips_bwd.py, beside tests/lpips_ref.py.

  g_layers(seed, N)                  the seeded gradients arriving at layers [N,5], uniform in [0.5, 1.5], fp32
  metric_grad64 / metric_grad32      lpips_ref._metric without its no_grad, under autograd: (layers, dx, dy) of
                                     sum g_layers[n,l] layers[n,l], in float64 / fp32
  metric_backward                    the same gradient written out by hand, step by step as include/smplnerf.h states it: the distance
                                     gradient, the ReLU mask and the pool route, the convolution on flipped weights, 1 / std
  distance_grad64 / distance_grad32  one tap's gradient under autograd (NaN at a pixel whose features are all zero)
  distance_grad_rule                 one tap's gradient by the header's rule (the norm term taken as 0 at such a pixel); fwd=np.float32
                                     computes s, r, nx, a, b, d in fp32 as the kernel does, everything after them in float64
  relu_pool_bwd                      dz = (y > 0) ? dy_full + route(dy_pool) : 0, route to the first maximum of a window
  SMALL                              the cases below the reference's 32-pixel limit: the float64 restatement is the truth there

Accuracy rule as in lpips_ref: E = max|v - v64| / max|v64|, a kernel's E at most 8 times the fp32 CPU's."""
import numpy as np
import torch
import torch.nn.functional as F

import lpips_ref as LR

GOLDEN = "g28_lpips_grad.npz"
G_SEED = 2800      # + the case's position in lpips_ref.CASES

# name -> (channels, H, W, N, weight seed, image seed): frames below 32 pixels, which the reference itself refuses
SMALL = {
    "narrow16": ((3, 5, 7, 9, 11), 16, 16, 2, 2631, 2641),        # the smallest frame
    "floors": ((8, 16, 24, 40, 40), 17, 19, 2, 2632, 2642),       # pool floors at every stage
    "segmented": ((16, 32, 257, 300, 264), 16, 18, 1, 2633, 2643),      # above 256 channels: the segmented chain in the input gradient
    "full16": (LR.FULL, 16, 16, 1, 2634, 2644),                   # VGG16's own channel counts
}


def g_layers(seed, N):
    return np.random.RandomState(seed).uniform(0.5, 1.5, (N, 5)).astype(np.float32)


def case_g(name):
    return g_layers(G_SEED + list(LR.CASES).index(name), LR.CASES[name][3])


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
def _features(w, v, dtype, mean, std, keep=None):
    """The taps of lpips_ref._metric's feature stack, un-normalised; keep: a list that receives the thirteen post-ReLU maps."""
    v = LR.standardize(v, dtype, mean, std)
    out, i = [], 0
    for l, n in enumerate(LR.STAGES):
        for _ in range(n):
            a, b = w["conv"][i]
            v = F.relu(F.conv2d(v, torch.from_numpy(a).to(dtype), torch.from_numpy(b).to(dtype), padding=1))
            if keep is not None:
                keep.append(v)
            i += 1
        out.append(v)
        if l < 4:
            v = F.max_pool2d(v, 2, 2)
    return out


def _metric_grad(w, x, y, g, dtype, mean=LR.MEAN, std=LR.STD):
    xt, yt = (torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True) for a in (x, y))
    with torch.enable_grad():
        fx, fy = ([LR._normalize(f) for f in _features(w, v, dtype, mean, std)] for v in (xt, yt))
        cols = [(((a - b) ** 2) * torch.from_numpy(v).to(dtype).view(1, -1, 1, 1)).mean(dim=[2, 3]).sum(dim=1) for a, b, v in zip(fx, fy, w["lin"])]
        layers = torch.stack(cols, dim=1)
        (layers * torch.from_numpy(g).to(dtype)).sum().backward()
    return layers.detach().numpy(), xt.grad.numpy(), yt.grad.numpy()


def metric_grad64(w, x, y, g, **kw):
    return _metric_grad(w, x, y, g, torch.float64, **kw)


def metric_grad32(w, x, y, g, **kw):
    return _metric_grad(w, x, y, g, torch.float32, **kw)


def _distance_grad(fx, fy, wl, g, normalize, dtype):
    fx, fy = (torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True) for a in (fx, fy))
    with torch.enable_grad():
        a, b = (LR._normalize(fx), LR._normalize(fy)) if normalize else (fx, fy)
        out = (((a - b) ** 2) * torch.from_numpy(wl).to(dtype).view(1, -1, 1, 1)).mean(dim=[2, 3]).sum(dim=1)
        (out * torch.from_numpy(g).to(dtype)).sum().backward()
    return fx.grad.numpy(), fy.grad.numpy()


def distance_grad64(fx, fy, wl, g, normalize=True):
    return _distance_grad(fx, fy, wl, g, normalize, torch.float64)


def distance_grad32(fx, fy, wl, g, normalize=True):
    return _distance_grad(fx, fy, wl, g, normalize, torch.float32)


# ---- by hand, as the header states it --------------------------------------------------------------------------------------------------
def distance_grad_rule(fx, fy, wl, g, normalize=True, fwd=np.float64):
    """(dfx, dfy) in float64.  fx, fy [N,C,h,w], wl [C], g [N]."""
    x64, y64 = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    N, C, h, w = x64.shape
    gs = (np.asarray(g, np.float64) / (h * w)).reshape(N, 1, 1, 1)
    w2 = 2.0 * np.asarray(wl, np.float64).reshape(1, C, 1, 1)
    if not normalize:
        q = w2 * (x64.astype(fwd) - y64.astype(fwd)).astype(np.float64) * gs
        return q, -q

    def unit(v64):
        s = (v64 * v64).sum(axis=1, keepdims=True).astype(fwd)      # float64 sum, rounded once
        r = np.sqrt(s)
        n = (r + fwd(LR.EPS)).astype(fwd)
        return r.astype(np.float64), n.astype(np.float64), (v64.astype(fwd) / n).astype(fwd)
    rx, nx, a = unit(x64)
    ry, ny, b = unit(y64)
    q = w2 * (a - b).astype(np.float64) * gs
    Dx, Dy = (q * a.astype(np.float64)).sum(axis=1, keepdims=True), (q * b.astype(np.float64)).sum(axis=1, keepdims=True)
    ux = np.where(rx > 0, Dx / np.where(rx > 0, rx, 1.0), 0.0)      # r = 0: the norm term is taken as 0
    uy = np.where(ry > 0, Dy / np.where(ry > 0, ry, 1.0), 0.0)
    return (q - x64 * ux) / nx, -(q - y64 * uy) / ny


def relu_pool_bwd(y, dy_full=None, dy_pool=None):
    """numpy, in y's dtype: the first maximum of a window in the order (0,0), (0,1), (1,0), (1,1) takes its gradient."""
    y = np.asarray(y)
    N, C, H, W = y.shape
    routed = np.zeros_like(y)
    if dy_pool is not None:
        Hp, Wp = H // 2, W // 2
        win = np.stack([y[:, :, dy:2 * Hp:2, dx:2 * Wp:2] for dy in (0, 1) for dx in (0, 1)], axis=-1)      # [N,C,Hp,Wp,4]
        best, first = win[..., 0].copy(), np.zeros(win.shape[:-1], np.int64)
        for d in range(1, 4):
            more = win[..., d] > best
            best, first = np.where(more, win[..., d], best), np.where(more, d, first)
        for d in range(4):
            routed[:, :, d >> 1:2 * Hp:2, d & 1:2 * Wp:2] = np.where(first == d, np.asarray(dy_pool, y.dtype), 0)
    total = routed if dy_full is None else np.asarray(dy_full, y.dtype) + routed
    return np.where(y > 0, total, 0).astype(y.dtype)


def metric_backward(w, x, y, g, mean=LR.MEAN, std=LR.STD):
    """(dx, dy) in float64: the forward keeping the thirteen maps, then the walk back."""
    dtype, N = torch.float64, x.shape[0]
    maps = []
    with torch.no_grad():
        _features(w, np.concatenate([x, y]), dtype, mean, std, keep=maps)
        conv, pooled = 13, None
        for l in range(4, -1, -1):
            n = LR.STAGES[l]
            tap = maps[conv - 1].numpy()
            u = np.concatenate(distance_grad_rule(tap[:N], tap[N:], w["lin"][l], g[:, l]))
            u = relu_pool_bwd(tap, u, pooled)
            for j in range(n - 1, -1, -1):
                conv -= 1
                flipped = torch.from_numpy(w["conv"][conv][0]).to(dtype).flip(2, 3).transpose(0, 1).contiguous()      # w'[ci][co][ky][kx]
                u = F.conv2d(torch.from_numpy(u), flipped, None, padding=1).numpy()
                if j > 0:
                    u = relu_pool_bwd(maps[conv - 1].numpy(), u, None)
            pooled = u
        d = pooled / np.asarray(std, np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    return d[:N], d[N:]
