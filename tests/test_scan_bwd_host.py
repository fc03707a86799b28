"""tests/scan_bwd_ref.py without a GPU: the float64 restatements against the recorded reference gradients, the numpy oracle and
central differences; the premises of every case that tests/test_gpu_composite_bwd.py and tests/test_gpu_sample_pdf_bwd.py run; and
the error measure on hand-made arrays."""
import numpy as np
import pytest
import torch

import scan_bwd_ref as S
from oracle import nerf_oracle as O
from conftest import load_golden

F64 = torch.float64


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def _g3_case(g3, N, mode, d_rgb, d_w=None, d_a=None):
    z = g3[f"z_N{N}"]
    zeros = np.zeros(z.shape, np.float32)
    return S.CompositeCase(f"g3-N{N}-{mode}", g3[f"raw_N{N}"], z, g3[f"dray_N{N}"] if mode == "ray" else g3[f"dsmp_N{N}"], None, d_rgb,
                           zeros if d_w is None else d_w, zeros if d_a is None else d_a)


# ------------------------------------------------------------------------------------------------ against the recorded gradients
@pytest.mark.parametrize("N", [1, 2, 64, 192, 100])
@pytest.mark.parametrize("wb", [0, 1])
@pytest.mark.parametrize("mode", ["ray", "smp"])
def test_composite64_reproduces_the_recorded_gradients(N, wb, mode):
    """g7 (d rgb only) at the 2e-4 / 2e-6 of test_gpu_grad.test_composite_backward, g14 (all three incoming gradients; d raw, d z,
    d dirs) at the 2e-4 / 2e-5 max|ref| of test_gpu_round3.test_raw2outputs_all_outputs_and_inputs_differentiable; the forward
    values against the numpy oracle at 1e-6."""
    if N == 1 and mode == "smp":
        return                                                      # (N == 1 ignores the directions: no such record)
    g3, g7, g14 = load_golden("g3_raw2outputs.npz"), load_golden("g7_grads.npz"), load_golden("g14_ops_grads.npz")
    c = _g3_case(g3, N, mode, g7[f"c_gout_N{N}"])
    r = S.composite(c, wb, F64, want=("d_rgb",))
    close(r["d_raw"], g7[f"c_draw_N{N}_wb{wb}_{mode}"], 2e-4, 2e-6)
    B = c.z.shape[0]
    d = c.dirs if mode == "smp" else np.broadcast_to(c.dirs[:, None, :], (B, N, 3))
    for got, ref in zip((r["rgb"], r["w"], r["a"]), O.raw2outputs(c.raw, c.z, d, wb)):
        close(got, ref, 0, 1e-6)
    c = _g3_case(g3, N, mode, g14[f"c_grgb_N{N}"], g14[f"c_gw_N{N}"], g14[f"c_ga_N{N}"])
    r = S.composite(c, wb, F64)
    key = f"N{N}_wb{wb}_{mode}"
    for k, ref in (("d_raw", g14[f"c_draw_{key}"]), ("d_z", g14[f"c_dz_{key}"]), ("d_dirs", g14[f"c_ddir_{key}"])):
        close(r[k], ref, 2e-4, 2e-5 * max(np.abs(ref).max(), 1e-12))


def test_sample_pdf_restatement_reproduces_the_recorded_gradients_away_from_the_kink():
    """g16 at the 1e-3 of a row's largest value of test_gpu_round3.test_sample_pdf_is_differentiable, on the rows whose gathered
    pairs all keep KINK_MARGIN from `denom < 1e-5` in float64 and take the side the fp32 oracle takes: 46 of the 48 rows (the other
    two are among g4's adversarial rows, which the old test's 90 % lets through).  The indices are the oracle's from the reference
    host's u and normalising sums, which the recorded samples confirm bit for bit.

    The fp32 restatement meets the record on all 46 to 1e-5, a hundredth of that tolerance (1.9e-6 at worst: two fp32 evaluation
    orders of one function).  The float64 one meets it to 1e-3 on
    43 of them.  On rows 7, 16 and 23 fp32 arithmetic itself is 1.3e-3 .. 2.3e-3 of the row away from float64 (active pairs with
    denom 3.0e-4, 1.6e-5 and 5.4e-5: t = (u - c0) / denom carries the fp32 cdf's rounding, about 2^-24 / denom), and the record
    with it.  That is the reference's own fp32 error - what the rule of the GPU files allows the kernel through E(fp32 CPU)."""
    g = load_golden("g16_sample_pdf_grad.npz")
    bins, w = g["bins"], g["weights"]
    u = torch.linspace(0., 1., steps=128).numpy()
    tot = torch.sum(torch.from_numpy(w) + 1e-5, -1).numpy()
    det = O.sample_pdf_detail(bins, w, 128, u=u, tot=tot)
    np.testing.assert_array_equal(det["samples"], g["samples"])
    c = S.SamplerCase("g16", bins, w, u, g["gout"], det["inds"], det["cdf"], False)
    r, r32 = S.sample_pdf(c, F64), S.sample_pdf(c, torch.float32)
    below, above = S.gathered_pairs(c)
    d32 = np.take_along_axis(c.cdf32, above, -1) - np.take_along_axis(c.cdf32, below, -1)
    active = r["denom"] >= S.KINK
    away = ((np.abs(r["denom"] - S.KINK) >= S.KINK_MARGIN) & ((d32 < np.float32(S.KINK)) != active)).all(-1)
    well = away & (np.maximum(S.E_rows(r32["d_bins"], r["d_bins"]), S.E_rows(r32["d_weights"], r["d_weights"])) <= 1e-3)
    print(f"g16: {int(away.sum())} of {len(away)} rows away from the kink, on {int(well.sum())} of them fp32 is within 1e-3 of float64")
    assert (len(away), away.sum(), well.sum()) == (48, 46, 43) and np.nonzero(away & ~well)[0].tolist() == [7, 16, 23]
    for k in ("d_bins", "d_weights"):
        ref = g[k]
        scale = np.maximum(np.abs(ref).max(-1), 1e-6)
        print(k, "fp32 restatement against the record, worst away row:", (np.abs(r32[k] - ref).max(-1) / scale)[away].max())
        assert (np.abs(r32[k] - ref).max(-1) <= 1e-5 * scale)[away].all(), k
        assert (np.abs(r[k] - ref).max(-1) <= 1e-3 * scale)[well].all(), k


def test_sample_pdf64_forward_is_the_oracles():
    """to 1e-6 where the fp32 oracle itself is that good: up to five bins (its t is off by about 2^-24 / denom, which at 63 bins and
    more is 2e-6 .. 4e-6 of a sample in 1 .. 4)"""
    for kind, Nb, Nf in [a for a in S.sampler_sweep() if a[1] <= 3] + [(kind, 5, 4) for kind in S.SAMPLER_KINDS]:
        c = S.sampler_case(kind, S.SAMPLER_B, Nb, Nf)
        close(S.sample_pdf(c, F64)["samples"], O.sample_pdf(c.bins, c.weights, Nf, u=c.u), 0, 1e-6)


# ------------------------------------------------------------------------------------------------ central differences
def _central(f, x, h):
    g = np.zeros(x.shape)
    for i in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (f(xp) - f(xm)) / (2 * h)
    return g


class _Dbl:
    """a case whose arrays stay float64 (the generators return fp32; the differences need the perturbed values unrounded)"""

    def __init__(self, c, **over):
        self.__dict__.update(c._asdict())
        self.__dict__.update(over)


@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("ps", [0, 1])
@pytest.mark.parametrize("wb", [0, 1])
def test_composite64_gradients_are_the_central_differences(N, ps, wb):
    """mild inputs (|sigma + noise| >= 1e-3, h = 1e-6: no sample crosses the ReLU's kink), z and the directions as leaves"""
    c = S.composite_case("mild", 2, N, ps)
    S.composite_premises(c)
    r = S.composite(c, wb, F64)

    def loss(**over):
        o = S.composite(_Dbl(c, **over), wb, F64)
        return (o["rgb"] * c.d_rgb).sum() + (o["w"] * c.d_w).sum() + (o["a"] * c.d_a).sum()

    for k, name in (("d_raw", "raw"), ("d_z", "z"), ("d_dirs", "dirs")):
        x = getattr(c, name).astype(np.float64)
        fd = _central(lambda v: loss(**{name: v}), x, 1e-6)
        close(r[k], fd, 1e-6, 1e-8 * np.abs(fd).max())


@pytest.mark.parametrize("Nb,Nf", [(3, 7), (5, 4)])
@pytest.mark.parametrize("kind", ["flat", "cube"])
def test_sample_pdf64_gradients_are_the_central_differences(kind, Nb, Nf):
    """flat and cube weights: every pair active and KINK_MARGIN from the kink, so the map is smooth around the inputs (the indices
    stay the inputs they are)"""
    c = S.sampler_case(kind, 3, Nb, Nf)
    S.sampler_premises(c)
    r = S.sample_pdf(c, F64)
    for k, name in (("d_bins", "bins"), ("d_weights", "weights")):
        x = getattr(c, name).astype(np.float64)
        fd = _central(lambda v: (S.sample_pdf(_Dbl(c, **{name: v}), F64)["samples"] * c.d_zs).sum(), x, 1e-6)
        close(r[k], fd, 1e-6, 1e-8 * np.abs(fd).max())


# ------------------------------------------------------------------------------------------------ premises of the GPU cases
def _finite_and_not_all_zero(name, r64, r32, keys, zero_ok=()):
    for k in keys:
        assert np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all(), f"{name}: {k} is not finite in a restatement"
        assert k in zero_ok or np.abs(r64[k]).max() > 0, f"{name}: {k} is zero everywhere"


def test_premises_of_every_composite_case():
    sweep = [(kind, S.COMPOSITE_B, N, ps, wb) for kind, N, ps, wb in S.composite_sweep()]
    assert all({wb for _, _, n, _, wb in sweep if n == N} == {0, 1} for N in S.COMPOSITE_N)
    saturated, underflow = {}, False
    for kind, B, N, ps, wb in sweep + [a + (1,) for a in S.COMPOSITE_SINGLES]:
        c = S.composite_case(kind, B, N, ps)
        S.composite_premises(c)
        r64, r32 = S.composite(c, wb, F64), S.composite(c, wb, torch.float32)
        _finite_and_not_all_zero(c.name, r64, r32, ("d_raw", "d_z", "d_dirs"), zero_ok=("d_z", "d_dirs") if N == 1 else ())
        sig = c.raw[..., 3]
        if kind == "saturated" and N > 1:
            assert (sig == 60).any() and (sig[1] == 80).all()
            saturated[N] = saturated.get(N, 0) + int((r32["a"][:, :-1] == 1).sum())      # om = 1e-10 exactly, with samples behind it
            underflow |= bool((r32["w"][1] == 0).any() and r64["w"][1].min() >= 0)
        if kind == "planted":
            assert (sig[0, ::3] == 0).all() and (sig[2] == -1).all() and c.z[3, 1] == c.z[3, 0]
            assert not r64["d_raw"][2].any() and not r64["d_z"][2].any()              # sigma < 0 everywhere: the ray is empty
            zero_dir = c.dirs[4, N // 2] if ps else c.dirs[4]
            assert not zero_dir.any() and not (r64["d_dirs"][4, N // 2] if ps else r64["d_dirs"][4]).any()
            assert np.abs(r64["d_raw"][0, ::3, 3]).max() == 0                         # relu'(0) = 0
    # up to 129 samples the gaps of z in 1 .. 4 are wide enough for sigma = 60 / 80 to saturate alpha before the last sample
    assert all(saturated[N] > 0 for N in S.COMPOSITE_N if N <= 129) and underflow, saturated


def test_premises_of_every_sampler_case():
    cases = [(kind, S.SAMPLER_B, Nb, Nf) for kind, Nb, Nf in S.sampler_sweep()] + S.SAMPLER_SINGLES
    inactive = 0
    for kind, B, Nb, Nf in cases:
        c = S.sampler_case(kind, B, Nb, Nf)
        r64, r32 = S.sample_pdf(c, F64), S.sample_pdf(c, torch.float32)
        margin, n = S.sampler_premises(c, r64)
        _finite_and_not_all_zero(c.name, r64, r32, ("d_bins", "d_weights"), zero_ok=("d_weights",) if Nb == 2 else ())
        assert c.u[-1] == (1 if Nf > 1 else 0) and ((c.inds[:, -1] >= Nb - 1).all() or Nf == 1)
        if kind == "spiky":
            assert c.planted == (Nb >= 6 and Nf >= 5) and (n >= 2 or not c.planted), c.name
            inactive += n
        else:
            assert n == 0, f"{c.name}: every interior pair of a {kind} case is active"
        if Nb == 2:                                                                   # one weight: pdf = 1 whatever it is
            assert np.abs(r64["d_weights"]).max() < 1e-9 * np.abs(r64["d_bins"]).max()
    assert inactive > 100


def test_the_two_seeds_of_the_u1_sample():
    Nb = S.U1_SHAPE[0]
    for seed, ind, side in ((S.U1_SEED_AT_NB, Nb, lambda last: last <= 1), (S.U1_SEED_BELOW_NB, Nb - 1, lambda last: last > 1)):
        c = S.u1_case(seed)
        S.sampler_premises(c)
        r32, r64 = S.sample_pdf(c, torch.float32), S.sample_pdf(c, F64)
        assert c.u[-1] == 1 and c.inds[0, -1] == ind and side(c.cdf32[0, -1]) and side(np.float32(r32["cdf"][0, -1]))
        g = float(c.d_zs[0, -1])
        assert g != 0 and np.count_nonzero(c.d_zs) == 1
        # index Nb: below = above = Nb - 1; index Nb - 1: the pair is (Nb - 2, Nb - 1) with t = 1 in float64 - g lands on the last bin
        close(r64["d_bins"][0], [0] * (Nb - 1) + [g], 0, 1e-12)


# ------------------------------------------------------------------------------------------------ the measure itself
def test_E_rows_and_the_rule_on_hand_made_arrays():
    y64 = np.array([[1.0, -4.0, 2.0], [0.0, 0.0, 0.0], [0.5, 0.25, 0.0]])
    np.testing.assert_array_equal(S.E_rows(y64, y64), [0, 0, 0])
    one_bad = y64.copy()
    one_bad[0, 2] += 4e-6                                                             # one element of row 0: 1e-6 of the row's 4
    np.testing.assert_allclose(S.E_rows(one_bad, y64), [1e-6, 0, 0], rtol=1e-9)
    exact = y64.copy()                                                                # the restatement is exact: the floor decides
    assert not S.rows_pass(S.E_rows(one_bad, y64), S.E_rows(exact, y64), y64)[0]
    just = y64.copy()
    just[0, 0] += 4 * 2.0 ** -21
    assert S.rows_pass(S.E_rows(just, y64), S.E_rows(exact, y64), y64).all()
    cpu = y64.copy()
    cpu[0, 1] += 4 * 1.3e-7                                                           # 8 x 1.3e-7 > 1e-6: row 0 passes
    assert S.rows_pass(S.E_rows(one_bad, y64), S.E_rows(cpu, y64), y64).all()
    cpu[0, 1] = y64[0, 1] + 4 * 1.2e-7                                                # 8 x 1.2e-7 < 1e-6: it does not
    assert S.rows_pass(S.E_rows(one_bad, y64), S.E_rows(cpu, y64), y64).tolist() == [False, True, True]
    dirty = y64.copy()                                                                # a zero row must be zero from the kernel,
    dirty[1, 1] = 1e-30
    noisy = y64.copy()                                                                # however noisy the restatement is there
    noisy[1] = 1.0
    assert S.E_rows(dirty, y64)[1] == np.inf
    assert S.rows_pass(S.E_rows(dirty, y64), S.E_rows(noisy, y64), y64).tolist() == [True, False, True]
    nan = y64.copy()
    nan[2, 0] = np.nan
    assert S.rows_pass(S.E_rows(nan, y64), S.E_rows(noisy, y64), y64).tolist() == [True, True, False]
    with pytest.raises(AssertionError, match="rows \\[0\\]"):
        S.hold("hand-made", one_bad, exact, y64)
    assert S.hold("hand-made", just, exact, y64) == np.inf
