"""tests/fwd_ops_ref.py without a GPU: the premises of every case that tests/test_gpu_composite_fwd.py and tests/test_gpu_posenc.py
run, the two torch restatements against the numpy oracle on the recorded fixtures, and the condition that makes the rule a fair one
for a kernel: a restatement of composite_fwd_kernel's arithmetic with exp taken in float64 and rounded once passes it on every case.

Measured (pytest -s prints all of it): that restatement's worst row sits at 0.50 of its bound for rgb, 0.31 for weights and 0.22 for
alpha.  With numpy's fp32 exp in its place it misses the rule seven times in the sweep: weights and alpha of mild, N = 3, per-ray on
both backgrounds (rows whose alphas are all small, so that 1 - exp cancels against the row's scale: E = 1.1e-6 against 1.1e-7 for
the yardstick), rgb of mild, N = 8192, per-ray on the black background and of planted, N = 4097, per-sample on both.  So the rule
can tell the two apart.  The fp32 yardstick of the positional encoding is 0.60 x 2^-24 off float64 at every frequency up to 2^29;
its worst backward row is 2e-7 .. 7e-7 at L = 1 .. 30."""
import numpy as np
import pytest
import torch

import fwd_ops_ref as Fw
from oracle import nerf_oracle as O
from conftest import load_golden
from scan_bwd_ref import CompositeCase

F32 = np.float32


# ------------------------------------------------------------------------------------------------ compositing: the cases
def test_the_sweep_covers_what_it_claims():
    sweep = Fw.composite_sweep()
    assert len(sweep) == len(set(sweep)) == 3 * (11 * 4 + 2)
    for N in Fw.COMPOSITE_N:
        for kind in Fw.COMPOSITE_KINDS:
            got = {(ps, wb) for k, n, ps, wb in sweep if (k, n) == (kind, N)}
            assert got == ({(0, 0), (0, 1)} if N == 1 else {(0, 0), (0, 1), (1, 0), (1, 1)})
    assert Fw.COMPOSITE_B == 5 and 4097 == 64 * Fw.WAVE + 1


def test_premises_of_every_composite_case():
    interior_saturation = {}
    for kind, N, ps, wb in Fw.composite_sweep():
        c, r64, r32 = Fw.refs(kind, N, ps, wb)
        Fw.composite_premises(c)
        assert c.z.shape == (5, N) and c.dirs.shape == ((5, N, 3) if ps else (5, 3)) and (c.noise is not None) == (kind == "mild")
        for r in (r64, r32):
            assert all(np.isfinite(r[k]).all() for k in Fw.OUTPUTS) and r["rgb"].shape == (5, 3) and r["w"].shape == r["a"].shape == (5, N)
        if N == 1:
            assert (r64["w"] == 1).all() and (r64["a"] == 1).all()
            continue
        arg, sig, dist = Fw.exp_argument(c)
        if kind == "saturated":
            # ray 1: sigma = 80 throughout; alpha is exactly 1 at its last sample at the least, and where it is 1 before the last
            # sample the next transmittance is 1e-10 times this one (om = 1e-10 exactly)
            assert (sig[1] == 80).all() and (c.raw[..., 3] == 60).any()
            assert r32["a"][1, -1] == 1 and r64["a"][1, -1] == 1 and arg[1, -1] <= Fw.ALPHA_ONE_BELOW
            one = np.flatnonzero(r32["a"][1, :-1] == 1)                 # (fp32: exp(x) < 2^-25; float64 keeps 1 - alpha > 0 longer)
            interior_saturation[N] = interior_saturation.get(N, 0) + len(one)
            if len(one):
                om = ((F32(1) - r32["a"][1]).astype(F32) + F32(1e-10)).astype(F32)
                T = np.cumprod(np.concatenate([[1.0], om[:-1].astype(np.float64)]))
                i = one[0]
                assert om[i] == F32(1e-10) and T[i] > 0 and abs(T[i + 1] / T[i] / 1e-10 - 1) < 1e-7
                assert r64["a"][1, i] > 1 - 2.0 ** -25
        if kind == "planted":
            assert (c.raw[0, ::3, 3] == 0).all() and (c.raw[1, :, 3] > 0).all() and (c.raw[2, :, 3] == -1).all() and c.z[3, 1] == c.z[3, 0]
            assert not (c.dirs[4, N // 2] if ps else c.dirs[4]).any()
            for r in (r64, r32):
                assert not r["a"][0, ::3].any() and not r["w"][0, ::3].any()                     # relu(0) = 0
                assert not r["a"][2].any() and not r["w"][2].any() and (r["rgb"][2] == wb).all()   # a dead ray shows the background
                assert r["a"][3, 0] == 0 and r["w"][3, 0] == 0                                    # equal depths: dist = 0
                if ps:
                    assert r["a"][4, N // 2] == 0 and r["w"][4, N // 2] == 0
                else:
                    assert not r["a"][4].any() and not r["w"][4].any() and (r["rgb"][4] == wb).all()
            assert dist[3, 0] == 0 and (dist[4, N // 2] == 0 if ps else (dist[4] == 0).all())
    # up to 129 samples the gaps of z in 1 .. 4 are wide enough for sigma = 80 to saturate alpha before the last sample
    assert all(interior_saturation[N] > 0 for N in Fw.COMPOSITE_N if 2 <= N <= 129), interior_saturation


# ------------------------------------------------------------------------------------------------ the restatements and the oracle
@pytest.mark.parametrize("N", [1, 2, 64, 192, 100])
def test_raw2outputs_restatements_are_the_oracles_on_g3(N):
    """float64 and float32, to the bars of test_gpu_parity.test_raw2outputs: 1e-6 on rgb, 5e-7 on weights and alpha"""
    g3 = load_golden("g3_raw2outputs.npz")
    for mode in ("ray",) if N == 1 else ("ray", "smp"):
        dirs = g3[f"dray_N{N}"] if mode == "ray" else g3[f"dsmp_N{N}"]
        c = CompositeCase(f"g3-N{N}-{mode}", g3[f"raw_N{N}"], g3[f"z_N{N}"], dirs, None, None, None, None)
        B = len(c.z)
        d = dirs if mode == "smp" else np.broadcast_to(dirs[:, None, :], (B, N, 3))
        for wb in (0, 1):
            want = O.raw2outputs(c.raw, c.z, d, wb)
            for dtype in (torch.float64, torch.float32):
                r = Fw.composite_ref(c, wb, dtype)
                for k, ref, tol in zip(Fw.OUTPUTS, want, (1e-6, 5e-7, 5e-7)):
                    assert r[k].shape == ref.shape and np.abs(r[k].astype(np.float64) - ref).max() <= tol, (mode, wb, dtype, k)
            k = Fw.composite_kernel_np(c, wb)
            for name, ref, tol in zip(Fw.OUTPUTS, want, (1e-6, 5e-7, 5e-7)):
                assert np.abs(k[name].astype(np.float64) - ref).max() <= tol, (mode, wb, "kernel restatement", name)


@pytest.mark.parametrize("L,ident", [(10, 0), (4, 0), (10, 1), (4, 1), (0, 1)])
def test_posenc_restatements_are_the_oracles_on_g1(L, ident):
    """to the 4e-7 of test_gpu_parity.test_posenc, against the record and the numpy oracle"""
    g1 = load_golden("g1_posenc.npz")
    want = g1[f"enc_L{L}_id{ident}"]
    for dtype in (torch.float64, torch.float32):
        enc, _ = Fw.posenc_ref(g1["x"], L, ident, dtype)
        assert enc.shape == want.shape
        assert np.abs(enc.astype(np.float64) - want).max() <= 4e-7 and np.abs(enc.astype(np.float64) - O.PositionalEncoder(L, ident).encode(g1["x"])).max() <= 4e-7


# ------------------------------------------------------------------------------------------------ the rule is a fair one
def _worst(k, r32, r64):
    """{output: (worst E kernel / bound over the rows, rows that miss)}"""
    out = {}
    for o in Fw.OUTPUTS:
        ek, ec = Fw.E_rows(k[o], r64[o]), Fw.E_rows(r32[o], r64[o])
        ok = Fw.rows_pass(ek, ec, r64[o])
        zero = np.abs(r64[o].reshape(len(ek), -1)).max(-1) == 0
        out[o] = (float(np.where(zero, 0.0, ek / np.maximum(Fw.FACTOR * ec, Fw.FLOOR)).max()), [(int(i), float(ek[i]), float(ec[i])) for i in np.flatnonzero(~ok)])
    return out


def test_the_restatement_with_a_once_rounded_double_exp_passes_the_rule_everywhere():
    worst = dict.fromkeys(Fw.OUTPUTS, 0.0)
    misses_f32 = []
    for kind, N, ps, wb in Fw.composite_sweep():
        c, r64, r32 = Fw.refs(kind, N, ps, wb)
        for o, (frac, missed) in _worst(Fw.composite_kernel_np(c, wb), r32, r64).items():
            assert not missed, f"{c.name}-wb{wb} {o}: rows (row, E restatement, E fp32 CPU) {missed} miss the rule"
            worst[o] = max(worst[o], frac)
        for o, (frac, missed) in _worst(Fw.composite_kernel_np(c, wb, Fw._exp_f32), r32, r64).items():
            misses_f32 += [(f"{c.name}-wb{wb}", o) + m for m in missed]
    print("exp in float64 rounded once: worst E / bound " + ", ".join(f"{o} {v:.2f}" for o, v in worst.items()))
    print(f"the same with numpy's fp32 exp misses the rule {len(misses_f32)} times (case, output, row, E, E fp32 CPU):")
    for m in misses_f32:
        print("   ", m)
    assert all(v < 1 for v in worst.values())


def test_kernel_restatement_details():
    """the 64-lane tree is wave_scan_add's last lane; alpha is exactly 1 at and below the stated argument with either exp"""
    v = np.arange(64, dtype=F32)
    assert Fw._tree64(v) == v.sum()
    v = (F32(1) + np.arange(64) * F32(2.0 ** -23)).astype(F32)                 # every pair sum is inexact: the order shows
    tree = v.copy()
    for _ in range(6):
        tree = (tree[0::2] + tree[1::2]).astype(F32)
    assert Fw._tree64(v) == tree[0]
    x = np.array([Fw.ALPHA_ONE_BELOW, -1e3, -1e12, -np.inf], F32)
    assert (Fw._exp_once(x) == 0).all() and (Fw._exp_f32(x) == 0).all()
    assert F32(1) - Fw._exp_once(np.array([-17.4], F32))[0] == 1


# ------------------------------------------------------------------------------------------------ positional encoding
def test_posenc_cases_reach_what_they_claim():
    W = lambda c, L, i: c * (i + 2 * L)
    assert all(W(c, L, i) <= Fw.POSENC_MAX_ROW for c, L, i, n in Fw.POSENC_CASES)
    assert Fw.posenc_tile(3, 10, 0) == Fw.posenc_tile(3, 4, 1) == 64 and W(1, 0, 1) == 1
    assert W(69, 10, 0) == 1380 and Fw.posenc_tile(69, 10, 0) == 11                # n = 10, 11, 12, 23: under, at, over, two tiles + 1
    assert W(16384, 0, 1) == W(8192, 1, 0) == 16384 and Fw.posenc_tile(16384, 0, 1) == Fw.posenc_tile(8192, 1, 0) == 1
    assert (3 * W(5, 1, 0)) % 4 != 0                                               # 30 floats: no 16-byte stores
    assert (64 * W(2, 3, 1)) % 4 == 0 and W(2, 3, 1) % 4 != 0 and (64 * W(2, 3, 1) * 4) % 16 == 0
    assert (64 * W(*Fw.POSENC_MISALIGNED[:3])) % 4 == 0                            # the 16-byte path but for the pointer
    # the refusal the unfixed entry missed: the row width wraps to 4 in 32 bits
    assert (70409300 * (1 + 2 * 30)) % 2 ** 32 == 4 and 70409300 < 2 ** 31
    x = Fw.specials_block()
    assert x.shape == (8, 3) and np.isnan(x).sum() == 2 and np.isinf(x).sum() == 4 and np.signbit(x[x == 0]).sum() == 2


def test_posenc_yardstick_against_float64():
    """x 2^k is exact in fp32 and in float64, so both see the same argument and the fp32 sin / cos owes float64 its own rounding
    only: less than 2^-24, the spacing of fp32 in [0.5, 1), for a faithfully rounded function of values in [-1, 1], at every L the
    entry takes (measured: 0.60 of it at every frequency)"""
    x, _ = Fw.posenc_inputs(3, 30, 0, 4096)
    e64, _ = Fw.posenc_ref(x, 30, 0, torch.float64)
    e32, _ = Fw.posenc_ref(x, 30, 0, torch.float32)
    err = np.abs(e32.astype(np.float64) - e64).reshape(len(x), 30, 6).max((0, 2)) / 2.0 ** -24
    print("fp32 yardstick, forward, in units of 2^-24 by frequency:", np.round(err, 2).tolist())
    assert err.max() <= 1.0
    for L in (1, 4, 10, 16, 24, 30):
        xs, d_out = Fw.posenc_inputs(3, L, 1, 257)
        _, g64 = Fw.posenc_ref(xs, L, 1, torch.float64, d_out)
        _, g32 = Fw.posenc_ref(xs, L, 1, torch.float32, d_out)
        print(f"fp32 yardstick, backward, L = {L}: worst row E {Fw.E_rows(g32, g64).max():.2e}")
        assert np.isfinite(g32).all()


def test_posenc_specials_in_the_yardstick():
    """what the device is held to: NaN from an infinite or NaN argument (3e38 x 2^k is infinite from k = 1), signed zeros, cos 0 = 1"""
    x = Fw.specials_block()
    for ident in (0, 1):
        enc, _ = Fw.posenc_ref(x, 4, ident, torch.float32)
        enc = enc[:, 3 * ident:].reshape(len(x), 4, 2, 3)
        for k in range(4):
            with np.errstate(over="ignore", invalid="ignore"):
                finite = np.isfinite(x * F32(2.0 ** k))
            assert np.array_equal(np.isnan(enc[:, k, 0]), ~finite) and np.array_equal(np.isnan(enc[:, k, 1]), ~finite)
            zero = x == 0
            assert (enc[:, k, 0][zero] == 0).all() and np.array_equal(np.signbit(enc[:, k, 0][zero]), np.signbit(x[zero]))
            assert (enc[:, k, 1][zero] == 1).all()
