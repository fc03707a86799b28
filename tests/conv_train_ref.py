"""Restatement of SmplEstimator's convolution block in TRAINING mode and of the network's training forward with dropout p = 0
(models/smpl_estimator.py:32-47 under nn.Module.train()), in torch CPU ops under autograd - the yardstick of
tests/test_conv_train_host.py and test_gpu_conv_train.py.

  block(x, w, b, gamma, beta, rm, rv, dy, relu, pool, dtype)   y = [maxpool2x2](relu(BN_batch(conv3x3_pad1(x, w) + b))) and, for
        the upstream gradient dy, every gradient; a dict of numpy arrays: y, z (the raw map), mean, invstd (biased variance),
        running_mean, running_var (moved with MOMENTUM, the unbiased variance), dx, dw, db, dgamma, dbeta, dz (the gradient at z),
        pre (the pre-activation), mask (pre > 0) and argmax (per pool window the row-major index of the position its gradient goes
        to: torch's first maximum) - the last two are what the mask condition of the random cases compares between fp32 and float64
  block64 / block32                                            ... in float64 / in fp32
  network(s, x, dout, dtype)                                   the five blocks, flatten, fc1, ReLU, fc2; out, every parameter's
        gradient for the upstream gradient dout, the moved running statistics and per block pre-activation masks and argmaxes
  bn_pool_bwd64(z, dy, relu, pool)                             g, s1, s2 and dz of the block's backward with mean = 0, invstd =
        gamma = 1, beta = 0, in float64 numpy: the pool and ReLU routing written out (the first maximum in the order (0,0), (0,1),
        (1,0), (1,1); gradient 0 where the pre-activation is <= 0; pixels in no window get 0)

E and FACTOR = 8 are smpl_estimator_ref's (DESIGN.md section 8g's rule)."""
import numpy as np
import torch
import torch.nn.functional as F

from smpl_estimator_ref import CHANNELS, E, EPS, FACTOR, POOL  # noqa: F401  (E and FACTOR: for the tests that import this module)

MOMENTUM = 0.1


def _bn_train(z, gamma, beta, rm, rv, momentum, eps):
    """BatchNorm2d's training forward written out, so that mean and invstd can be returned: the same function as
    F.batch_norm(training=True) (tests/test_conv_train_host.py holds it to that)."""
    M = z.shape[0] * z.shape[2] * z.shape[3]
    mean = z.mean((0, 2, 3))
    var = ((z - mean[None, :, None, None]) ** 2).mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(var + eps)
    pre = (z - mean[None, :, None, None]) * invstd[None, :, None, None] * gamma[None, :, None, None] + beta[None, :, None, None]
    with torch.no_grad():
        new_rm = (1 - momentum) * rm + momentum * mean
        new_rv = (1 - momentum) * rv + momentum * var * (M / (M - 1))
    return pre, mean, invstd, new_rm, new_rv


def _argmax(v):
    """first maximum of every 2 x 2 window of v [N,C,H,W] in row-major order: int8 [N,C,H//2,W//2]"""
    N, C, H, W = v.shape
    w = v[:, :, :H // 2 * 2, :W // 2 * 2].reshape(N, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    return np.argmax(w, -1).astype(np.int8)


def block(x, w, b, gamma, beta, rm, rv, dy, relu=True, pool=False, dtype=torch.float64, momentum=MOMENTUM, eps=EPS):
    x, w, b, gamma, beta = (torch.as_tensor(a).to(dtype).clone().requires_grad_(True) for a in (x, w, b, gamma, beta))
    rm, rv = (torch.as_tensor(a).to(dtype) for a in (rm, rv))
    z = F.conv2d(x, w, b, padding=1)
    z.retain_grad()
    pre, mean, invstd, new_rm, new_rv = _bn_train(z, gamma, beta, rm, rv, momentum, eps)
    a = F.relu(pre) if relu else pre
    y = F.max_pool2d(a, 2, 2) if pool else a
    y.backward(torch.as_tensor(dy).to(dtype))
    out = {"y": y, "z": z, "mean": mean, "invstd": invstd, "running_mean": new_rm, "running_var": new_rv, "dx": x.grad, "dw": w.grad,
           "db": b.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "dz": z.grad, "pre": pre}
    out = {k: v.detach().numpy() for k, v in out.items()}
    out["mask"] = out["pre"] > 0
    out["argmax"] = _argmax(np.maximum(out["pre"], 0) if relu else out["pre"]) if pool else None
    return out


def block64(*a, **k):
    return block(*a, dtype=torch.float64, **k)


def block32(*a, **k):
    return block(*a, dtype=torch.float32, **k)


def network(s, x, dout, dtype=torch.float64):
    """s: smpl_estimator_ref.state(..) - the training forward with dropout p = 0 and the backward of dout [N,human_size]."""
    p = {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(True) for k, v in s.items() if "running" not in k and "num_batches" not in k}
    h = torch.as_tensor(x).to(dtype)
    stats, masks, argmaxes = {}, [], []
    for i in range(1, 6):
        z = F.conv2d(h, p[f"conv{i}.weight"], p[f"conv{i}.bias"], padding=1)
        pre, _, _, rm, rv = _bn_train(z, p[f"bn{i}.weight"], p[f"bn{i}.bias"], torch.as_tensor(s[f"bn{i}.running_mean"]).to(dtype),
                                      torch.as_tensor(s[f"bn{i}.running_var"]).to(dtype), MOMENTUM, EPS)
        stats[f"bn{i}.running_mean"], stats[f"bn{i}.running_var"] = rm.numpy(), rv.numpy()
        masks.append(pre.detach().numpy() > 0)
        h = F.relu(pre)
        if POOL[i - 1]:
            argmaxes.append(_argmax(h.detach().numpy()))
            h = F.max_pool2d(h, 2, 2)
        else:
            argmaxes.append(None)
    h = h.reshape(-1, 8 * 8 * 128)
    h = F.relu(F.linear(h, p["fc1.weight"], p["fc1.bias"]))
    out = F.linear(h, p["fc2.weight"], p["fc2.bias"])
    out.backward(torch.as_tensor(dout).to(dtype))
    return {"out": out.detach().numpy(), "grads": {k: v.grad.numpy() for k, v in p.items()}, "stats": stats, "masks": masks, "argmaxes": argmaxes}


def same_choices(a, b):
    """whether two restatements of a block (or of the network) select the same ReLU mask and the same window argmax everywhere"""
    if "masks" in a:
        return all(np.array_equal(m, n) for m, n in zip(a["masks"], b["masks"])) and \
            all((m is None and n is None) or np.array_equal(m, n) for m, n in zip(a["argmaxes"], b["argmaxes"]))
    return np.array_equal(a["mask"], b["mask"]) and (a["argmax"] is None or np.array_equal(a["argmax"], b["argmax"]))


def bn_pool_bwd64(z, dy, relu, pool):
    """The backward of [pool](relu(z)) through a BatchNorm with mean = 0, invstd = gamma = 1, beta = 0 (so xhat = pre = z), loops in
    float64: g [N,C,H,W], s1 [C], s2 [C], dz = g - s1 / M - z s2 / M."""
    z, dy = np.asarray(z, np.float64), np.asarray(dy, np.float64)
    N, C, H, W = z.shape
    g = np.zeros_like(z)
    if pool:
        for oy in range(H // 2):
            for ox in range(W // 2):
                best = np.full((N, C), -np.inf)
                at = np.zeros((N, C), np.int64)
                for d, (dy_, dx_) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    v = z[:, :, 2 * oy + dy_, 2 * ox + dx_]
                    v = np.maximum(v, 0) if relu else v
                    take = v > best                                     # torch's scan: a later position wins only when it is GREATER
                    best, at = np.where(take, v, best), np.where(take, d, at)
                for d, (dy_, dx_) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    pre = z[:, :, 2 * oy + dy_, 2 * ox + dx_]
                    passes = (pre > 0) if relu else np.ones_like(pre, bool)
                    g[:, :, 2 * oy + dy_, 2 * ox + dx_] = np.where((at == d) & passes, dy[:, :, oy, ox], 0.0)
    else:
        g = np.where(z > 0, dy, 0.0) if relu else dy.copy()
    M = N * H * W
    s1, s2 = g.sum((0, 2, 3)), (g * z).sum((0, 2, 3))
    dz = g - s1[None, :, None, None] / M - z * s2[None, :, None, None] / M
    return g, s1, s2, dz
