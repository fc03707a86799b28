"""What tests/test_gpu_composite_fwd.py and tests/test_gpu_posenc.py hold the oldest forward kernels to (composite_fwd_kernel of
csrc/composite.hip; posenc_kernel and posenc_bwd_kernel of csrc/posenc.hip).  CPU only; tests/test_fwd_ops_host.py checks all of
it without a GPU.

The rule, the measure, the compositing inputs and their premises are those of tests/scan_bwd_ref.py, imported and not copied:
    E(kernel) <= max(FACTOR x E(fp32 CPU restatement), FLOOR) per row,   E = max|y - y64| / max|y64|,   FACTOR = 8, FLOOR = 2^-21
A row is one ray of rgb / weights / alpha, or one point of an encoding (of its gradient).

Compositing: the reference is tests/torch_ref.raw2outputs in float64, the yardstick the same in float32.  composite_kernel_np is a
numpy restatement of the kernel's arithmetic as it should be - every fp32 operation of composite.hip's loop in its order, the
exclusive product in float64 rounded per sample, the per-lane sums over the 64-sample chunks followed by the 64-lane tree - with
exp taken in float64 and rounded once.  That it passes the rule on every case is what makes the rule a fair one for a kernel.

Positional encoding: tests/torch_ref.posenc in float64 and float32, autograd of sum(enc * d_out) for the backward."""
from functools import lru_cache

import numpy as np
import torch

import torch_ref as R
from scan_bwd_ref import (COMPOSITE_KINDS, FACTOR, FLOOR, E_rows, composite_case, composite_premises, hold,  # noqa: F401
                          rows_pass)

F32, F64 = np.float32, np.float64
WAVE = 64

# ------------------------------------------------------------------------------------------------ compositing
COMPOSITE_B = 5                                   # one ray more than a workgroup's four
# around the 64-sample chunk and two chunks; 4097: the last chunk is one sample behind 64 carried chunks; 8192: twice what the
# backward accepts (the forward has no upper bound)
COMPOSITE_N = (1, 2, 3, 63, 64, 65, 128, 129, 257, 4096, 4097, 8192)
OUTPUTS = ("rgb", "w", "a")


def composite_sweep():
    """(kind, N, per_sample, white background): every kind at every N with both forms of the directions and both backgrounds;
    N = 1 ignores the directions and takes the per-ray form only"""
    return [(kind, N, ps, wb) for N in COMPOSITE_N for kind in COMPOSITE_KINDS for ps in ((0,) if N == 1 else (0, 1)) for wb in (0, 1)]


@lru_cache(maxsize=None)
def case(kind, N, per_sample, B=COMPOSITE_B):
    return composite_case(kind, B, N, per_sample)


def composite_ref(c, wb, dtype):
    """tests/torch_ref.raw2outputs in `dtype` from the fp32 arrays of case `c`: rgb [B,3], w [B,N], a [B,N] as numpy"""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    B, N = c.z.shape
    dirs = t(c.dirs)
    d = dirs[:, None, :].expand(B, N, 3) if dirs.dim() == 2 else dirs
    rgb, w, a = R.raw2outputs(t(c.raw), t(c.z), d, wb, t(c.noise))
    return dict(rgb=rgb.numpy(), w=w.to(dtype).numpy(), a=a.to(dtype).numpy())


@lru_cache(maxsize=None)
def refs(kind, N, per_sample, wb, B=COMPOSITE_B):
    """(case, float64 reference, fp32 yardstick), computed once and shared; nobody writes to them"""
    c = case(kind, N, per_sample, B)
    out = c, composite_ref(c, wb, torch.float64), composite_ref(c, wb, torch.float32)
    for r in out[1:]:
        for a in r.values():
            a.setflags(write=False)
    return out


def _exp_once(x):
    """exp in float64 of an fp32 argument, rounded once to fp32"""
    return np.exp(x.astype(F64)).astype(F32)


def _exp_f32(x):
    return np.exp(x.astype(F32)).astype(F32)


def _tree64(v):
    """the 64-lane sum of wave_scan_add's last lane: neighbours first, then pairs of pairs, ... (fp32)"""
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(F32)
    return v[..., 0]


def composite_kernel_np(c, wb, exp=_exp_once):
    """composite_fwd_kernel's arithmetic in numpy, operation by operation (see the module docstring); `exp` is the alpha's exp"""
    raw, z = c.raw.astype(F32), c.z.astype(F32)
    B, N = z.shape
    sigmoid = lambda x: (F32(1) / (F32(1) + _exp_once(-x))).astype(F32)
    if N == 1:
        return dict(rgb=sigmoid(raw[:, 0, :3]), w=np.ones((B, 1), F32), a=np.ones((B, 1), F32))
    with np.errstate(over="ignore", under="ignore"):
        d = c.dirs.astype(F32)
        nrm = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F32) + d[..., 2] * d[..., 2]).astype(F32)).astype(F32)
        if nrm.ndim == 1:
            nrm = nrm[:, None]
        dist = np.concatenate([(z[:, 1:] - z[:, :-1]).astype(F32), np.full((B, 1), 1e10, F32)], -1)
        dist = (dist * nrm).astype(F32)
        sig = raw[..., 3] if c.noise is None else (raw[..., 3] + c.noise.astype(F32)).astype(F32)
        a = (F32(1) - exp((-np.maximum(sig, F32(0)) * dist).astype(F32))).astype(F32)
        om = ((F32(1) - a).astype(F32) + F32(1e-10)).astype(F32)
        excl = np.concatenate([np.ones((B, 1), F64), om[:, :-1].astype(F64)], -1)
        T = np.cumprod(excl, -1).astype(F32)
        w = (a * T).astype(F32)
        pad = (-N) % WAVE
        terms = np.concatenate([(w[..., None] * sigmoid(raw[..., :3])).astype(F32), w[..., None]], -1)       # [B, N, 4]
        terms = np.concatenate([terms, np.zeros((B, pad, 4), F32)], 1).reshape(B, -1, WAVE, 4)
        acc = np.zeros((B, WAVE, 4), F32)
        for k in range(terms.shape[1]):                                                                      # a lane's sum over chunks
            acc = (acc + terms[:, k]).astype(F32)
        acc = _tree64(np.moveaxis(acc, 1, -1))                                                               # [B, 4]
        rgb = acc[:, :3]
        if wb:
            rgb = (rgb + (F32(1) - acc[:, 3:4]).astype(F32)).astype(F32)
    return dict(rgb=rgb, w=w, a=a)


def exp_argument(c):
    """the fp32 argument -relu(sigma + noise) * dist of the alpha's exp, as the kernel and the reference form it ([B, N])"""
    z = c.z.astype(F32)
    d = c.dirs.astype(F32)
    nrm = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F32) + d[..., 2] * d[..., 2]).astype(F32)).astype(F32)
    dist = np.concatenate([(z[:, 1:] - z[:, :-1]).astype(F32), np.full((len(z), 1), 1e10, F32)], -1)
    dist = (dist * (nrm[:, None] if nrm.ndim == 1 else nrm)).astype(F32)
    sig = c.raw[..., 3] if c.noise is None else (c.raw[..., 3] + c.noise).astype(F32)
    return (-np.maximum(sig, F32(0)) * dist).astype(F32), sig, dist


# exp(x) < 2^-25 for x <= -17.33, so 1 - exp(x) rounds to 1 whatever the exp's last bits; -104 is where exp itself leaves the
# fp32 range (2^-150 = exp(-103.97)): at or below it alpha is exactly 1 with any exp
ALPHA_ONE_BELOW = -104.0


# ------------------------------------------------------------------------------------------------ positional encoding
# (c, L, identity, n)
POSENC_CASES = ([(3, L, ident, n) for L, ident in ((10, 0), (4, 0), (10, 1), (4, 1)) for n in (1, 63, 64, 65, 130)]   # the 64-point tile
                + [(1, 0, 1, 5), (1, 0, 1, 257)]                             # outdim = 1; identity alone
                + [(69, 10, 0, n) for n in (10, 11, 12, 23)]                 # outdim = 1380, tile of 11 points
                + [(3, 30, 1, 65)]                                           # the largest L the entry takes
                + [(16384, 0, 1, 3), (8192, 1, 0, 3)]                        # outdim = 16384, one point per workgroup
                + [(5, 1, 0, 3)]                                             # a whole call of 30 floats: the scalar store path
                + [(2, 3, 1, 65)])                                           # a full tile of 16-byte stores, then one point of 14 floats
POSENC_MISALIGNED = (3, 4, 1, 65)                                            # out one float past a 16-byte boundary: scalar path
POSENC_BWD_CASES = POSENC_CASES
POSENC_MAX_ROW = 16384
POSENC_TILE = 64
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3e38], F32)


def posenc_tile(c, L, identity):
    return min(POSENC_TILE, POSENC_MAX_ROW // (c * (identity + 2 * L)))


@lru_cache(maxsize=None)
def posenc_inputs(c, L, identity, n, seed=0):
    """x ~ U(-4, 4) [n, c] and d_out ~ N(0, 1) [n, c (identity + 2L)]"""
    rng = np.random.default_rng([c, L, identity, n, seed])
    x = rng.uniform(-4, 4, (n, c)).astype(F32)
    d_out = rng.normal(size=(n, c * (identity + 2 * L))).astype(F32)
    return x, d_out


def posenc_ref(x, L, identity, dtype, d_out=None):
    """tests/torch_ref.posenc in `dtype`; with d_out also the autograd gradient of sum(enc * d_out).  Returns numpy (enc, d_x)."""
    t = torch.from_numpy(np.array(x)).to(dtype).requires_grad_(d_out is not None)
    enc = R.posenc(t, L, identity)
    if d_out is None:
        return enc.numpy(), None
    (d_x,) = torch.autograd.grad((enc * torch.from_numpy(np.array(d_out)).to(dtype)).sum(), [t])
    return enc.detach().numpy(), d_x.numpy()


@lru_cache(maxsize=None)
def posenc_refs(c, L, identity, n):
    """(x, d_out, enc64, d_x64, enc32, d_x32), computed once and shared; nobody writes to them (the inputs stay writable for
    torch.from_numpy's sake)"""
    x, d_out = posenc_inputs(c, L, identity, n)
    out = (x, d_out) + posenc_ref(x, L, identity, torch.float64, d_out) + posenc_ref(x, L, identity, torch.float32, d_out)
    for a in out[2:]:
        a.setflags(write=False)
    return out


def specials_block():
    """[6, 3]: every special in every channel position, next to ordinary values"""
    x = np.tile(np.array([0.5, -1.25, 3.0], F32), (len(SPECIALS), 1))
    for i, s in enumerate(SPECIALS):
        x[i, i % 3] = s
    return np.concatenate([x, SPECIALS.reshape(2, 3)], 0)


def one_block(d_out, c, L, identity, k, cos):
    """d_out with everything but the sin (cos) block of frequency k zeroed"""
    g = np.zeros_like(d_out)
    lo = identity * c + k * 2 * c + (c if cos else 0)
    g[:, lo:lo + c] = d_out[:, lo:lo + c]
    return g
