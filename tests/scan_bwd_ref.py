"""What tests/test_gpu_composite_bwd.py and tests/test_gpu_sample_pdf_bwd.py hold the two ray-wise scan backward kernels to
(composite_bwd_kernel of csrc/composite.hip, sample_pdf_bwd_kernel of csrc/sampler.hip): torch restatements of utils.py:134-191 and
utils.py:200-226 in a dtype of the caller's choice (float64 is the reference, float32 the yardstick), the seeded inputs of every case
with the premises each case rests on, and the error measure.  CPU only; tests/test_scan_bwd_host.py checks all of it without a GPU.

The rule (measure and factor of tests/test_gpu_vertex_warp.py and tests/test_gpu_contract.py, applied per ray): with
E_rows(y, y64) = max|y - y64| / max|y64| over one ray's row of an output, a row passes when
    E(kernel) <= max(FACTOR x E(fp32 CPU restatement), FLOOR),   FACTOR = 8, FLOOR = 2^-21
FLOOR is FACTOR times half an ulp (2^-24) of the row's largest value: where the fp32 restatement happens to be exact the kernel is
still allowed that much.  A row whose y64 is all zero must be all zero from the kernel.  The worst row is what hold() prints."""
from collections import namedtuple

import numpy as np
import torch

import torch_ref as R
from oracle import nerf_oracle as O

F32 = np.float32
FACTOR = 8.0
FLOOR = 2.0 ** -21


# ------------------------------------------------------------------------------------------------ error measure
def _rows(y):
    y = np.asarray(y)
    return y.reshape(y.shape[0], -1).astype(np.float64)


def E_rows(y, y64):
    """per ray max|y - y64| / max|y64|; where y64's row is all zero: 0 if y's row is all zero too, else inf"""
    y, y64 = _rows(y), _rows(y64)
    err, scale = np.abs(y - y64).max(-1), np.abs(y64).max(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))


def rows_pass(ek, ec, y64):
    """the rule, per row (a NaN in the kernel's row makes ek NaN, which passes nothing)"""
    zero = np.abs(_rows(y64)).max(-1) == 0
    return np.where(zero, ek == 0, ek <= np.maximum(FACTOR * ec, FLOOR))


def hold(name, y_kernel, y_cpu32, y64):
    """print the worst row's figures, then assert the rule for every row; returns the worst E(kernel) / E(fp32 CPU)"""
    ek, ec = E_rows(y_kernel, y64), E_rows(y_cpu32, y64)
    ok = rows_pass(ek, ec, y64)
    with np.errstate(divide="ignore", invalid="ignore"):
        excess = np.where(np.isfinite(ek), ek / np.maximum(FACTOR * ec, FLOOR), np.inf)
    r = int(np.argmax(excess))
    scale = np.abs(_rows(y64)).max(-1)
    ratio = ek[r] / ec[r] if ec[r] > 0 else float("inf") if ek[r] > 0 else 0.0
    print(f"{name}: worst row {r} of {len(ek)}: E kernel {ek[r]:.3e}  E fp32 CPU {ec[r]:.3e}  ratio {ratio:.2f}  max|y64| {scale[r]:.3e}"
          f"  ({int((scale == 0).sum())} all-zero rows)")
    assert ok.all(), (f"{name}: rows {np.nonzero(~ok)[0].tolist()} miss E kernel <= max({FACTOR} x E fp32 CPU, 2^-21): "
                      f"E kernel {ek[~ok].tolist()}, E fp32 CPU {ec[~ok].tolist()}")
    return ratio


# ------------------------------------------------------------------------------------------------ compositing
def composite(c, wb, dtype, want=("d_rgb", "d_w", "d_a")):
    """utils.py:134-191 (tests/torch_ref.raw2outputs, with noise) in `dtype` from the fp32 arrays of case `c`, directions [B,3] or
    [B,N,3] as leaves.  Returns rgb, w, a and the gradients d_raw, d_z, d_dirs of sum(rgb d_rgb) + sum(w d_w) + sum(a d_a) over the
    incoming gradients named in `want` (float64 numpy whatever the dtype; zeros where the graph does not reach a leaf)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    raw, z, dirs = (t(a).requires_grad_(True) for a in (c.raw, c.z, c.dirs))
    B, N = c.z.shape
    d = dirs[:, None, :].expand(B, N, 3) if dirs.dim() == 2 else dirs
    rgb, w, a = R.raw2outputs(raw, z, d, wb, None if c.noise is None else t(c.noise))
    loss = sum((out * t(getattr(c, g))).sum() for out, g in ((rgb, "d_rgb"), (w, "d_w"), (a, "d_a")) if g in want and out.requires_grad)
    grads = torch.autograd.grad(loss, [raw, z, dirs], allow_unused=True)
    res = {k: (torch.zeros_like(leaf) if g is None else g).numpy().astype(np.float64)
           for k, g, leaf in zip(("d_raw", "d_z", "d_dirs"), grads, (raw, z, dirs))}
    res.update(rgb=rgb.detach().numpy(), w=w.detach().numpy(), a=a.detach().numpy())
    return res


CompositeCase = namedtuple("CompositeCase", "name raw z dirs noise d_rgb d_w d_a")
SIGMA_MARGIN = 1e-3
COMPOSITE_KINDS = ("mild", "saturated", "planted")


def composite_case(kind, B, N, per_sample, seed=0):
    """raw ~ N(0, 2), z sorted in U(1, 4), directions ~ N(0, 1), d rgb / d weights / d alpha ~ N(0, 1), and
      mild       noise ~ N(0, 1) on sigma
      saturated  sigma = 60 at a tenth of the samples and sigma = 80 along all of ray 1 (B > 1)
      planted    sigma exactly 0 at every third sample of ray 0, ray 2 all sigma = -1, z[3, 1] = z[3, 0], and a zero direction: one
                 sample of ray 4 (per-sample directions) or ray 4 itself (per-ray); ray 1 keeps sigma > 0; on the rays that B has
    A sigma + noise within SIGMA_MARGIN of 0 is moved up by 0.01, so that the ReLU of utils.py:159 takes the same side in fp32 and
    float64 (composite_premises)."""
    assert kind in COMPOSITE_KINDS
    rng = np.random.default_rng([COMPOSITE_KINDS.index(kind), B, N, int(per_sample), seed])
    raw = rng.normal(0, 2, (B, N, 4)).astype(F32)
    z = np.sort(rng.uniform(1, 4, (B, N)).astype(F32), -1)
    dirs = rng.normal(size=(B, N, 3) if per_sample else (B, 3)).astype(F32)
    noise = rng.normal(size=(B, N)).astype(F32) if kind == "mild" else None
    d_rgb, d_w, d_a = (rng.normal(size=s).astype(F32) for s in ((B, 3), (B, N), (B, N)))
    if kind == "saturated":
        r80 = min(1, B - 1)
        raw[r80, :, 3] = 80.0
        others = np.flatnonzero(np.arange(B * N) // N != r80)
        raw[..., 3].reshape(-1)[rng.permutation(others)[:(B * N + 9) // 10]] = 60.0
    s = raw[..., 3] + (0 if noise is None else noise)
    raw[..., 3][np.abs(s) < SIGMA_MARGIN] += F32(0.01)
    if kind == "planted":
        raw[0, ::3, 3] = 0.0
        if B > 1:
            raw[1, :, 3] = np.abs(raw[1, :, 3])          # (one ray that is live at every sample, whatever N and the draw)
        if B > 2:
            raw[2, :, 3] = -1.0
        if B > 3 and N > 1:
            z[3, 1] = z[3, 0]
        if B > 4:
            dirs[(4, N // 2) if per_sample else 4] = 0.0
    return CompositeCase(f"{kind}-B{B}-N{N}-{'smp' if per_sample else 'ray'}", raw, z, dirs, noise, d_rgb, d_w, d_a)


def composite_premises(c):
    """|sigma + noise| >= SIGMA_MARGIN wherever it is not exactly 0, in fp32 and in float64, and z ascending"""
    for dt in (np.float32, np.float64):
        s = c.raw[..., 3].astype(dt) + (0 if c.noise is None else c.noise.astype(dt))
        assert ((s == 0) | (np.abs(s) >= SIGMA_MARGIN)).all(), f"{c.name}: a sigma + noise within {SIGMA_MARGIN} of the ReLU's kink"
    assert (np.diff(c.z, axis=-1) >= 0).all(), f"{c.name}: z is not ascending"


# ------------------------------------------------------------------------------------------------ sample_pdf
def sample_pdf(c, dtype, inds=None):
    """utils.py:200-226 in `dtype` from the fp32 arrays of case `c`, with u and the searchsorted indices as inputs (the kernel's
    backward takes `inds` as an argument, and integers carry no gradient in the reference either): the cdf comes from
    weights + 1e-5 in `dtype`, and so does `denom < 1e-5 -> 1`.  Returns samples, cdf, denom (before the replacement) and the
    gradients d_bins, d_weights of sum(samples d_zs), as float64 numpy."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    bins, w = t(c.bins).requires_grad_(True), t(c.weights).requires_grad_(True)
    B, Nb = c.bins.shape
    inds = torch.from_numpy(np.ascontiguousarray(c.inds if inds is None else inds))
    w1 = w + 1e-5                                                                   # :200
    pdf = w1 / torch.sum(w1, -1, keepdim=True)                                      # :201
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)    # :202-203
    u = t(c.u).expand(B, -1)
    below, above = torch.clamp(inds - 1, min=0), torch.clamp(inds, max=Nb - 1)      # :213-214
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    raw_denom = c1 - c0                                                             # :223
    denom = torch.where(raw_denom < 1e-5, torch.ones_like(raw_denom), raw_denom)    # :224
    samples = b0 + (u - c0) / denom * (b1 - b0)                                     # :225-226
    d_bins, d_w = torch.autograd.grad((samples * t(c.d_zs)).sum(), [bins, w])
    f = lambda a: a.detach().numpy().astype(np.float64)
    return dict(samples=f(samples), cdf=f(cdf), denom=f(raw_denom), d_bins=f(d_bins), d_weights=f(d_w))


SamplerCase = namedtuple("SamplerCase", "name bins weights u d_zs inds cdf32 planted")
KINK = 1e-5
KINK_MARGIN = 4e-7       # several ulps of a cdf entry near 1: what an fp32 difference of two cdf entries can be off by
CUBE_FLOOR = 1.2e-5      # x (Nb - 1), see sampler_case
SAMPLER_KINDS = ("cube", "flat", "spiky")


def sampler_case(kind, B, Nb, Nf, seed=0, u=None):
    """bins sorted in U(1, 4), d z_samples ~ N(0, 1), u = oracle.linspace01(Nf) (or the one given), and weights
      cube   max(rand^3, CUBE_FLOOR (Nb - 1)): weights over three decades, every bin on the active side of `denom < 1e-5`.  The floor
             is what keeps them there: pdf_k = (w_k + 1e-5) / tot with tot <= (Nb - 1)(1 + 1e-5), so a floored weight has
             pdf_k >= 1.2e-5 / 1.00001 > KINK + KINK_MARGIN whatever the other weights are (plain rand^3 comes within 1e-7 of the
             kink at Nb = 1023)
      flat   U(0.5, 1.5)
      spiky  zeros with row % 4 spikes of 20 .. 50, none of them in bins 0 and 1 where Nb >= 6.  A zero-weight bin of a row with a
             spike has pdf 1e-5 / tot <= 5e-7, decisively inactive; as u = linspace hardly ever lands in one, where Nb >= 6 and
             Nf >= 5 two entries of u are the midpoints of bins 0 and 1 of row 1, so that inactive interior pairs are gathered
    The indices are oracle.sample_pdf_detail's on the same fp32 inputs - never a float64 recomputation: at u = 1 the index depends
    on one ulp of the cdf's last entry, and the gradient is genuinely different on either side."""
    assert kind in SAMPLER_KINDS and Nb >= 2 and Nf >= 1
    M = Nb - 1
    rng = np.random.default_rng([SAMPLER_KINDS.index(kind), B, Nb, Nf, seed])
    bins = np.sort(rng.uniform(1, 4, (B, Nb)).astype(F32), -1)
    d_zs = rng.normal(size=(B, Nf)).astype(F32)
    planted = False
    if kind == "cube":
        w = np.maximum(rng.random((B, M)) ** 3, CUBE_FLOOR * M).astype(F32)
    elif kind == "flat":
        w = rng.uniform(0.5, 1.5, (B, M)).astype(F32)
    else:
        w = np.zeros((B, M), F32)
        first = 2 if Nb >= 6 else 0
        for b in range(B):
            n = min(b % 4, M - first)
            w[b, first + rng.permutation(M - first)[:n]] = rng.uniform(20, 50, n).astype(F32)
        planted = u is None and Nb >= 6 and Nf >= 5 and B > 1
    if u is None:
        u = O.linspace01(Nf - 2 if planted else Nf)
        if planted:
            p = O.cdf_from_weights(w[1:2])[0]
            u = np.sort(np.concatenate([u, [F32(0.5) * p[1], F32(0.5) * (p[1] + p[2])]]).astype(F32))
    u = np.asarray(u, F32)
    det = O.sample_pdf_detail(bins, w, Nf, u=u)
    return SamplerCase(f"{kind}-B{B}-Nb{Nb}-Nf{Nf}", bins, w, u, d_zs, det["inds"], det["cdf"], planted)


def gathered_pairs(c):
    below, above = np.maximum(0, c.inds - 1), np.minimum(c.bins.shape[1] - 1, c.inds)
    return below, above


def sampler_premises(c, r64=None):
    """For every gathered pair the float64 denom is at least KINK_MARGIN away from 1e-5, and the fp32 oracle's `denom < 1e-5` flags
    equal the float64 ones.  Returns (smallest distance to the kink, number of inactive pairs with below < above)."""
    r64 = sample_pdf(c, torch.float64) if r64 is None else r64
    below, above = gathered_pairs(c)
    d32 = np.take_along_axis(c.cdf32, above, -1) - np.take_along_axis(c.cdf32, below, -1)
    assert d32.dtype == F32
    margin = np.abs(r64["denom"] - KINK).min()
    assert margin >= KINK_MARGIN, f"{c.name}: a gathered pair's float64 denom is {margin:.2e} away from the kink"
    flags32, flags64 = d32 < F32(KINK), r64["denom"] < KINK
    assert np.array_equal(flags32, flags64), f"{c.name}: {int((flags32 != flags64).sum())} pairs lie on different sides in fp32 and float64"
    if c.planted:
        assert (flags64[1] & (c.inds[1] == 1)).any() and (flags64[1] & (c.inds[1] == 2)).any(), f"{c.name}: the planted u missed bins 0 and 1 of row 1"
    return margin, int((flags64 & (below < above)).sum())


# ------------------------------------------------------------------------------------------------ the GPU files' cases
COMPOSITE_N = (2, 3, 63, 64, 65, 128, 129, 257, 4096)      # around the 64-sample chunk, two chunks, all 64 rows of s_carry
COMPOSITE_B = 5                                            # one ray more than a workgroup's four
SAMPLER_SHAPES = ((2, 1), (2, 5), (3, 7), (63, 128), (64, 64), (65, 65), (129, 200), (191, 128))
SAMPLER_B = 9
SAMPLER_BIG = (1023, 1024)                                 # 96 KiB of LDS: the raised-limit launch (B = 5, flat and spiky)
# the u = 1 sample: seeds of sampler_case("flat", 1, 3, 7, seed) at which the oracle's last index is Nb (the fp32 cdf ends at or below
# 1) and Nb - 1 (it ends one ulp above 1), found by trying seeds 0 .. 59 on the CPU; the fp32 restatement's cdf ends on the same
# side at both (tests/test_scan_bwd_host.py checks that all of this still holds)
U1_SHAPE = (3, 7)
U1_SEED_AT_NB, U1_SEED_BELOW_NB = 0, 51


def composite_sweep():
    """(kind, N, per_sample, white background): the background alternates so that both values meet every N"""
    return [(kind, N, ps, (i + k + ps) % 2) for i, N in enumerate(COMPOSITE_N) for k, kind in enumerate(COMPOSITE_KINDS) for ps in (0, 1)]


def sampler_sweep():
    return [(kind, Nb, Nf) for Nb, Nf in SAMPLER_SHAPES for kind in SAMPLER_KINDS]


def u1_case(seed):
    """one flat ray with d z_samples zero but for the u = 1 sample"""
    c = sampler_case("flat", 1, *U1_SHAPE, seed=seed)
    d_zs = np.zeros_like(c.d_zs)
    d_zs[:, -1] = c.d_zs[:, -1]
    return c._replace(name=f"u1-seed{seed}", d_zs=d_zs)


# the cases of the single tests: (kind, B, N, per_sample) and (kind, B, Nb, Nf)
COMPOSITE_SINGLES = [("mild", 5, 1, 0)] + [("mild", 5, N, ps) for N in (65, 129) for ps in (1, 0)] + [("saturated", 5, 65, 0), ("planted", 5, 129, 0)]
SAMPLER_SINGLES = [(kind, 5) + SAMPLER_BIG for kind in ("flat", "spiky")] + [("cube", 5, 65, 65), ("spiky", 5, 63, 128)]
