"""What tests/test_gpu_mlp_exact.py takes for granted, checked on the CPU (tests/exact_net_ref.py): every case meets the exactness bound
and the coverage conditions on its float64 reference alone, a float32 torch run of the same network on the same data equals that
reference entry for entry (an independent proof that the data is exact in fp32), the generator makes what it says, and the
comparison names what the builder needs.  profiles/mlp_exact_cases.txt is the record of every case's headroom."""
import numpy as np
import pytest
import torch

import exact_net_ref as E
import torch_ref as R

IDS = lambda c: c.name


@pytest.mark.parametrize("case", E.ALL_CASES, ids=IDS)
def test_preconditions_hold_on_the_float64_reference(case):
    m = E.assert_preconditions(case, E.SPLIT_MAX_OPERAND if case is E.NET_SPLIT else None)
    print(E.describe(case))
    assert m["max_abs_sum"] < 2 ** 24 and m["empty_tiles"] == 0


def _same(what, got32, want64):
    assert got32.dtype == torch.float32
    assert np.array_equal(got32.detach().numpy().astype(np.float64), want64), what


@pytest.mark.parametrize("case", E.NET_CASES, ids=IDS)
def test_render_net_in_float32_on_the_cpu_equals_float64(case):
    state, rows, d_raw = E.render_net_data(case)
    ref = E.render_net_reference(case)
    P = {k: torch.from_numpy(v).clone().requires_grad_() for k, v in state.items()}
    x = torch.from_numpy(rows).clone().requires_grad_()
    kw = {k: v for k, v in E.net_kw(case).items() if k != "width"}
    raw = R.render_ray_net(P, x, **kw)
    (raw * torch.from_numpy(d_raw)).sum().backward()
    _same("raw", raw, ref.out)
    _same("d rows", x.grad, ref.d_rows)
    assert set(P) == set(ref.grads)
    for k, v in P.items():
        _same(k, v.grad, ref.grads[k])


@pytest.mark.parametrize("case", E.WARP_CASES + [E.WARP_FUSED], ids=IDS)
def test_warp_net_in_float32_on_the_cpu_equals_float64(case):
    state, rows, d_out = E.warp_net_data(case)
    ref = E.warp_net_reference(case)
    P = {k: torch.from_numpy(v).clone().requires_grad_() for k, v in state.items()}
    if case.spr:
        x, pose, o = (torch.from_numpy(v) for v in rows)
        leaf = pose.clone().requires_grad_()
        full = torch.cat([x, leaf.repeat_interleave(case.spr, 0)], 1)
    else:
        leaf = full = torch.from_numpy(rows).clone().requires_grad_()
    warp = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(full, P["linear1.weight"], P["linear1.bias"])),
                                      P["linear2.weight"], P["linear2.bias"])
    if case.spr:
        warped = x + warp
        sdirs = warped - o.repeat_interleave(case.spr, 0)
        g = [torch.from_numpy(v) for v in d_out]
        (warp * g[0] + warped * g[1] + sdirs * g[2]).sum().backward()
        _same("warped", warped, ref.extra["warped"])
        _same("sdirs", sdirs, ref.extra["sdirs"])
    else:
        (warp * torch.from_numpy(d_out)).sum().backward()
    _same("warp", warp, ref.out)
    _same("d rows", leaf.grad, ref.d_rows)
    for k, v in P.items():
        _same(k, v.grad, ref.grads[k])


@pytest.mark.parametrize("case", [E.NET_DEFAULT[333], E.NET_WIDTHS[1], E.NET_INPUTS[0], E.NET_SPLIT, E.WARP_CASES[5]], ids=IDS)
def test_generator_makes_what_it_says(case):
    """integers only; every weight row r entries of +-1 (ceil(n_in / n_out) where r rows cannot reach every column), the heads dense,
    no input column without a non-zero, biases in 0 .. 2, rows and output gradients in -2 .. 2; the same data on every call"""
    state, rows, d_out = (E.render_net_data if isinstance(case, E.NetCase) else E.warp_net_data)(case)
    again = (E.render_net_data if isinstance(case, E.NetCase) else E.warp_net_data)(case)
    for name, v in state.items():
        assert v.dtype == np.float32 and np.array_equal(v, again[0][name])
        if name.endswith(".bias"):
            assert set(np.unique(v)) <= {0.0, 1.0, 2.0}
            continue
        n_out, n_in = v.shape
        assert set(np.unique(v)) <= {-1.0, 0.0, 1.0} and (v != 0).any(0).all()
        per_row = (v != 0).sum(1)
        want = n_in if n_out <= 3 else max(case.r, -(-n_in // n_out))
        assert (per_row == want).all(), (name, want, per_row.min(), per_row.max())
    for v in (rows, d_out):
        assert v.dtype == np.float32 and np.array_equal(v, np.rint(v)) and np.abs(v).max() == 2
    assert np.array_equal(rows, again[1]) and np.array_equal(d_out, again[2])
    if isinstance(case, E.NetCase):
        assert list(state) == [f"{n}.{s}" for n, _, _ in E.render_net_shapes(*case[1:8]) for s in ("weight", "bias")]


def test_the_case_lists_are_the_ones_the_paths_need():
    assert [c.n for c in E.NET_CASES[:4]] == [1, 77, 333, 1100] and all(c[1:8] == (8, 256, 60, 24, 0, (4,), 1) for c in E.NET_CASES[:4])
    assert [-(-c.n // 128) for c in E.NET_CASES[:4]] == [1, 1, 3, 9]                   # wgrad chunks of 128 samples
    assert [E.wgrad_splits(c.n) for c in E.NET_CASES[:4]] == [(1, 1), (1, 1), (3, 3), (9, 9)]
    assert E.wgrad_splits(3584) == (28, 28) and E.wgrad_splits(E.NET_TWO_SPLITS.n) == (26, 33)      # wide / narrow chunk counts differ
    assert E.NET_TWO_SPLITS[1:8] == E.NET_DEFAULT[333][1:8]
    assert all(c.n % 16 for c in E.ALL_CASES if c.n > 128)                             # a ragged last chunk
    assert [(c.width, c.n_layers, c.skips) for c in E.NET_WIDTHS] == [(128, 4, (1,)), (64, 16, (3, 9)), (512, 3, (1,)), (320, 2, ()),
                                                                      (100, 2, ()), (256, 1, ())]
    assert E.WIDE_512.width == 512 and E.NET_WIDTHS[4].positions_dim == 63
    assert E.NET_INPUTS[0].additional_input_dim == 69 and E.NET_INPUTS[1].use_directional_input == 0
    assert sorted({(c.width, c.row_len, c.n) for c in E.WARP_CASES}) == sorted(
        (w, r, n) for w in (256, 128, 100) for r in (40, 69) for n in (1, 77, 333))
    assert E.WARP_FUSED.spr == 4 and E.WARP_FUSED.row_len == 3 + 40
    names = [c.name for c in E.ALL_CASES]
    assert len(set(names)) == len(names)


def test_assert_exact_names_tensor_index_tile_and_values():
    want = np.arange(40 * 50, dtype=np.float64).reshape(40, 50)
    E.assert_exact("same", want.astype(np.float32), want)
    got = want.astype(np.float32)
    got[17, 35] += 1
    got[33, 2] -= 2
    with pytest.raises(AssertionError) as e:
        E.assert_exact("d positional_net.3.weight", got, want)
    msg = str(e.value)
    assert "d positional_net.3.weight" in msg and "(17, 35)" in msg and "tile (1, 2)" in msg and "2 of 2000" in msg
    assert repr(got[17, 35]) in msg and repr(np.float32(want[17, 35])) in msg and "(2, 0)" in msg
    with pytest.raises(AssertionError, match="not representable"):
        E.assert_exact("x", np.zeros(1, np.float32), np.array([2.0 ** 24 + 1]))
    with pytest.raises(AssertionError, match=r"1 of 3 entries differ \(1 non-finite values\), first at \(1,\)"):
        E.assert_exact("x", np.array([0, np.nan, 0], np.float32), np.zeros(3))
    with pytest.raises(AssertionError, match="not representable"):
        E.assert_exact("x", np.zeros(1, np.float32), np.array([np.inf]))
    with pytest.raises(AssertionError):
        E.assert_exact("x", np.zeros(1, np.float64), np.zeros(1))


def test_preconditions_see_what_they_are_for():
    """the conditions can fail: a single sample with balanced signs misses the coverage (why that case has 70 % of its signs +1), the
    default net at n = 333 has operands above 255, and the largest case uses more than a hundredth of the 2^24 there are"""
    m = E.preconditions(E.NET_DEFAULT[1100])
    assert 2 ** 24 / 100 < m["max_abs_sum"] < 2 ** 24
    thin = E.NET_DEFAULT[1]._replace(name="net-256x8-n1-balanced", p_plus=0.5, seed=1)
    with pytest.raises(AssertionError):
        E.assert_preconditions(thin)
    with pytest.raises(AssertionError):
        E.assert_preconditions(E.NET_DEFAULT[333], max_operand=255)


def test_profile_is_the_record_of_these_cases():
    """profiles/mlp_exact_cases.txt holds what this run measures (rewrite it with `python tests/exact_net_ref.py`)"""
    with open(E.PROFILE) as f:
        assert f.read() == E.profile_text()
