"""What tests/test_gpu_contract.py takes for granted, checked on the CPU (tests/contract_ref.py): the packing is the header's formula,
the float64 reference is the definition, the integer cases are exact in fp32 in any summation order, and the real-valued cases have
a yardstick E(contract32) above zero on outputs of magnitude >= 1."""
import numpy as np
import pytest
import torch

import contract_ref as CR


@pytest.mark.parametrize("n,n_feat,first_row,total_rows", [(5, 1, 0, 1), (7, 16, 2, 5), (3, 17, 3, 7), (4, 250, 1, 18), (2, 300, 2, 23)])
def test_packing_is_the_headers_formula(n, n_feat, first_row, total_rows):
    """include/smplnerf.h:311-312: d Y_l[s, f] is the float at dy[((first_row + f / 16) * n + s) * 16 + f % 16]"""
    rng = np.random.default_rng(n_feat)
    dense = rng.normal(size=(n, n_feat)).astype(np.float32)
    buf = CR.pack_tile_rows(dense, first_row, total_rows, n, 1000.0, float("nan"))
    assert buf.dtype == np.float32 and buf.shape == (total_rows, n, 16) and buf.flags["C_CONTIGUOUS"]
    flat = buf.reshape(-1)
    back = np.empty_like(dense)
    for s in range(n):
        for f in range(n_feat):
            back[s, f] = flat[((first_row + f // 16) * n + s) * 16 + f % 16]
    assert np.array_equal(back, dense)
    rows = CR.tile_rows(n_feat)
    layer = buf[first_row:first_row + rows].transpose(1, 0, 2).reshape(n, rows * 16)
    assert np.all(layer[:, n_feat:] == 1000.0) and not np.isnan(layer).any()                # pads: where stated, and nowhere else
    assert np.isnan(buf[:first_row]).all() and np.isnan(buf[first_row + rows:]).all()       # guards: every other tile-row
    assert np.isnan(buf).sum() == (total_rows - rows) * n * 16


@pytest.mark.parametrize("spr", [0, 1, 7, 16])
def test_contract64_is_the_einsum(spr):
    rng = np.random.default_rng(spr)
    n, n_feat, col0, ncols = 112, 70, 3, 21
    dense = rng.normal(size=(n, n_feat)).astype(np.float32)
    w = rng.normal(size=(n_feat + 1, 40)).astype(np.float32)
    w[n_feat] = np.nan                                                                      # (a guard row: never read)
    got = CR.contract64(dense, w, col0, ncols, spr)
    ref = torch.einsum("sf,fc->sc", torch.from_numpy(dense).double(), torch.from_numpy(w[:n_feat, col0:col0 + ncols]).double())
    if spr:
        ref = ref.view(n // spr, spr, ncols).sum(1)
    assert got.dtype == np.float64 and got.shape == tuple(ref.shape)
    assert np.abs(got - ref.numpy()).max() <= 1e-12 * np.abs(ref.numpy()).max()
    got32 = CR.contract32(dense, w, col0, ncols, spr)
    assert got32.dtype == np.float32 and CR.relative_error(got32, got) < 1e-5


@pytest.mark.parametrize("case", CR.integer_cases() + CR.GRID_STRIDE, ids=lambda c: c.name)
def test_integer_cases_are_exact_in_fp32(case):
    """|dY|, |w| <= 3 and |prior out| <= 5: every partial sum, in any order, is an integer of magnitude at most
    9 n_feat max(spr, 1) + 5 < 2^24, so fp32 adds them without rounding and the kernel must equal float64 bit for bit."""
    assert CR.integer_bound(case) < CR.INT_LIMIT
    assert 9 * case.n_feat * max(case.spr, 1) + 5 == CR.integer_bound(case)
    n = case.n if case.n > 0 else CR.grid_stride_n(case, 8)      # (the bound does not depend on n; 8 CUs keep this quick)
    dense, wc, prior = CR.integer_inputs(case, n)
    assert np.abs(dense).max() <= 3 and np.abs(wc).max() <= 3 and np.abs(prior).max() <= 5
    assert all(np.array_equal(a, np.rint(a)) for a in (dense, wc, prior))
    w = CR.weight_block(case, wc)
    y64 = CR.contract64(dense, w, case.col0, case.ncols, case.spr)
    assert np.abs(y64).max() + 5 <= CR.integer_bound(case)
    assert np.array_equal(CR.contract32(dense, w, case.col0, case.ncols, case.spr).astype(np.float64), y64)
    assert y64.shape == prior.shape and (case.n_feat < 16 or np.abs(y64).max() > 0)


def test_the_case_lists_are_the_ones_the_paths_need():
    assert len(CR.instance_cases()) == 45
    for spr, _ in CR.MODES:      # both values of accumulate meet every mode
        assert {c.accumulate for c in CR.instance_cases() if c.spr == spr} == {0, 1}
    assert all(c.n % c.spr == 0 for c in CR.integer_cases() + CR.REAL_CASES if c.spr)
    assert [CR.workgroups_per_cu(c.n_feat, c.ncols) for c in CR.GRID_STRIDE] == [2, 1, 1]
    for c in CR.GRID_STRIDE:
        n = CR.grid_stride_n(c, 256)
        tiles = (n + 15) // 16
        assert tiles > 2 * 4 * CR.workgroups_per_cu(c.n_feat, c.ncols) * 256 and (n % 16 == 0 if c.spr else n % 16 == 11)
    assert len({c.name for c in CR.integer_cases() + CR.GRID_STRIDE + CR.REAL_CASES}) == len(CR.integer_cases() + CR.GRID_STRIDE + CR.REAL_CASES)


@pytest.mark.parametrize("case", CR.REAL_CASES, ids=lambda c: c.name)
def test_real_cases_have_a_yardstick(case):
    """E(contract32) > 0 (the bound 8 E of the GPU test is never 0) on outputs of magnitude >= 1."""
    dense, wc = CR.real_inputs(case, case.n)
    w = CR.weight_block(case, wc)
    y64 = CR.contract64(dense, w, case.col0, case.ncols, case.spr)
    e32 = CR.relative_error(CR.contract32(dense, w, case.col0, case.ncols, case.spr), y64)
    print(f"{case.name}: E fp32 CPU {e32:.3e}  max|y64| {np.abs(y64).max():.3e}")
    assert np.abs(y64).max() >= 1.0
    assert 0.0 < e32 < 1e-5


def test_scratch_sizes_as_documented():
    assert CR.scratch_floats(80, 69, 0) == 0 and CR.scratch_floats(80, 69, 16) == 5 * 69 and CR.scratch_floats(63, 69, 7) == 63 * 69
