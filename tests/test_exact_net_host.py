"""What tests/test_gpu_mlp_exact.py takes for granted, checked on the CPU (tests/exact_net_ref.py): every case meets the exactness bound
and the coverage conditions on its float64 reference alone, a float32 torch run of the same network on the same data equals that
reference entry for entry (an independent proof that the data is exact in fp32), the generator makes what it says, and the
comparison names what the builder needs.  profiles/mlp_exact_cases.txt is the record of every case's headroom.  Likewise for the
inference cases (tests/test_gpu_mlp_infer_exact.py) and for the split-precision cases whose low operand parts are not zero
(tests/test_gpu_mlp_split_exact.py: premises (a) - (f) on the three training GEMMs, profiles/mlp_split_exact_cases.txt)."""
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


@pytest.mark.parametrize("case", E.WARP_CASES + E.WARP_INFER_FUSED, ids=IDS)
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


# ---- the inference cases of tests/test_gpu_mlp_infer_exact.py --------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.ALL_INFER_CASES, ids=IDS)
def test_inference_preconditions_hold_on_the_float64_reference(case):
    """the forward bound (through the composed maps and over the composition's own sums too), integer composed entries, a zero
    pre-activation, the ReLU shares, every feature seen active and inactive, no weight tile without an entry, varied outputs"""
    m = E.assert_infer_preconditions(case)
    print(E.describe_infer(case))
    assert m["max_abs_sum"] < 2 ** 24 and m["empty_tiles"] == 0 and m["composed_ok"]
    assert (E.infer_reference(case).composed is not None) == (case.net.width <= 256)


def _forward32(case, composed):
    """raw of the case in float32 torch on the CPU: the network as it stands, or its trunk followed by the composed maps"""
    net, ref = case.net, E.infer_reference(case)
    state, _, rows = E.infer_data(case)
    P, x = {k: torch.from_numpy(v) for k, v in state.items()}, torch.from_numpy(rows)
    kw = {k: v for k, v in E.net_kw(net).items() if k != "width"}
    if not composed:
        return R.render_ray_net(P, x, **kw)
    lin = torch.nn.functional.linear
    pp, dd = x[:, :net.positions_dim + net.additional_input_dim], x[:, x.shape[1] - net.directions_dim:]
    h = torch.relu(lin(pp, P["positions_pose_input.weight"], P["positions_pose_input.bias"]))
    for i in range(net.n_layers - 1):
        h = torch.relu(lin(torch.cat([h, pp], 1) if i in net.skips else h, P[f"positional_net.{i}.weight"], P[f"positional_net.{i}.bias"]))
    sw, sb, dw, db = (torch.from_numpy(v.astype(np.float32)) for v in ref.composed.entries)
    e = torch.relu(lin(torch.cat([h, dd], 1) if net.use_directional_input else h, dw, db))
    return torch.cat([lin(e, P["rgb_out_layer.weight"], P["rgb_out_layer.bias"]), lin(h, sw, sb)], 1)


@pytest.mark.parametrize("case", E.ALL_INFER_CASES, ids=IDS)
def test_inference_net_in_float32_on_the_cpu_equals_float64(case):
    """the uncomposed network, and (widths up to 256) the trunk followed by the composed maps, both against the UNCOMPOSED float64"""
    ref = E.infer_reference(case)
    _same("raw", _forward32(case, False), ref.out)
    if ref.composed is not None:
        _same("raw through the composed maps", _forward32(case, True), ref.out)


def test_direction_normalisation_gives_unit_axes_exactly():
    """sqrtf((ux ux + uy uy) + uz uz) and the division, in fp32 operation by operation: s e_i -> sign(s) e_i for every s the cases use;
    a direction off the axes (1, 1, 0) does not normalise to integers, so the premise is not vacuous"""
    for s in (-4.0, -2.0, -1.0, 1.0, 2.0, 4.0):
        d = s * np.eye(3, dtype=np.float32)
        got = E.direction_premise(d)
        assert got.dtype == np.float32 and np.array_equal(got, np.sign(d))
    assert not np.array_equal(E.direction_premise(np.array([[1.0, 1.0, 0.0]])), np.array([[1.0, 1.0, 0.0]], np.float32))
    for case in E.FUSED_CASES + [E.SPLIT_FIRST] + list(E.SPLIT_LAST.values()):
        _, inputs, rows = E.infer_data(case)
        d = inputs["d"]
        assert d.shape[0] == (case.net.n if case.per_sample else case.net.n // case.spr)
        assert ((d != 0).sum(1) == 1).all() and set(np.unique(np.abs(d))) <= {0.0, 1.0, 2.0, 4.0}
        dn = E.direction_premise(d)
        assert np.array_equal(dn, np.sign(d))
        assert np.array_equal(rows[:, -3:], dn if len(dn) == case.net.n else np.repeat(dn, case.spr, 0))
        assert np.abs(inputs["x"]).max() == 2 * case.mult and np.array_equal(inputs["x"], np.rint(inputs["x"]))
        assert {tuple(abs(v) for v in r) for r in np.unique(np.sign(d), axis=0)} == {(1, 0, 0), (0, 1, 0), (0, 0, 1)}


def test_fused_rows_are_what_the_kernel_assembles():
    """rows = [positions | additional of the ray] or [additional | positions], then the direction of the ray or of the sample"""
    for case in E.FUSED_ADD + E.FUSED_RAYS:
        _, inp, rows = E.infer_data(case)
        n, spr, a = case.net.n, case.spr, case.net.additional_input_dim
        ray = np.arange(n) // spr
        assert inp["x"].shape == (n, 3) and rows.shape == (n, 3 + a + 3)
        x0 = a if case.add_first else 0
        assert np.array_equal(rows[:, x0:x0 + 3], inp["x"])
        if a:
            a0 = 0 if case.add_first else 3
            assert inp["add"].shape == (n // spr, a) and np.array_equal(rows[:, a0:a0 + a], inp["add"][ray])
        assert np.array_equal(rows[:, -3:], np.sign(inp["d"][np.arange(n) if case.per_sample else ray]))
    assert [(c.spr, c.per_sample) for c in E.FUSED_RAYS] == [(4, 0), (24, 0), (4, 1)]
    assert [(c.spr, c.add_first) for c in E.FUSED_ADD] == [(24, 1), (24, 0), (4, 1), (4, 0)]


def test_big_rows_are_rows_of_the_pool():
    for case, n in ((E.FUSED_POOL, 8192 + 5), (E.FUSED_ADD[0], 24 * 100), (E.INFER_DEFAULT[333], 1000), (E.FUSED_RAYS[2], 4 * 77)):
        _, pool, _ = E.infer_data(case)
        inp, idx = E.big_rows(case, n, 3)
        assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < case.net.n and len(np.unique(idx)) > min(n, case.net.n) // 3
        again, idx2 = E.big_rows(case, n, 3)
        assert np.array_equal(idx, idx2) and all(np.array_equal(inp[k], again[k]) for k in inp if inp[k] is not None)
        if case.entry == "encoded":
            assert np.array_equal(inp["rows"], pool["rows"][idx])
            continue
        assert np.array_equal(inp["x"], pool["x"][idx])
        ray = idx[::case.spr] // case.spr
        assert np.array_equal(idx, (ray[:, None] * case.spr + np.arange(case.spr)).ravel())         # whole rays
        assert np.array_equal(inp["d"], pool["d"][idx if case.per_sample else ray])
        if pool["add"] is not None:
            assert np.array_equal(inp["add"], pool["add"][ray])
    inp, idx = E.big_rows(E.FUSED_POOL, E.FUSED_POOL.net.n, 0)
    assert np.array_equal(idx, np.arange(E.FUSED_POOL.net.n))                                       # the pool itself, every row once


@pytest.mark.parametrize("n_cu", [256, 304, 64])
def test_launch_forms_of_the_sizes_derived_from_the_compute_unit_count(n_cu):
    """the restated lat_choose / lat_split (csrc/mlp_lat.hip) on the sizes the GPU test derives from the device's CU count: every
    branch of lat_split is reached - one workgroup per CU, two paired ones, the mixed launch, a remainder launch, a ragged size - the
    hybrid size is whole throughput rounds plus a latency remainder, and with SNERF_LAT=0 the sizes are 64- and 128-sample tiles"""
    assert E.lat_limits() == (4, 2) and E.encoder_kblocks(0, 1) == 1 and E.encoder_kblocks(10, 0) == 4 and E.encoder_kblocks(4, 0) == 2
    seen = set()
    for label, n, kinds in E.lat_sizes(n_cu):
        mode, got, tile = E.launch_form(n, n_cu)
        assert (mode, got, tile) == (1, kinds, 0), (label, n, mode, got)
        seen |= set(got) | ({"remainder"} if len(got) == 2 else set()) | ({"ragged"} if n % 16 else set())
    assert seen == {"single", "paired", "mixed", "remainder", "ragged"}
    n = E.hybrid_size(n_cu)
    assert E.launch_form(n, n_cu) == (2, ["single"], 128) and E.lat_choose_infer(n, n_cu) == (2, 128 * n_cu)
    sizes = E.throughput_sizes(n_cu)
    assert [E.launch_form(n, n_cu, lat=False)[2] for _, n in sizes] == [64 if n <= 64 * n_cu else 128 for _, n in sizes]
    assert sizes[2][1] == 128 * n_cu and sizes[3][1] > 2 * 128 * n_cu and sizes[3][1] % 128
    if n_cu == 256:          # the figures of the comments in csrc/mlp_lat.hip: 4096 samples latency, 32 768 and 153 600 not alone
        assert E.lat_choose_infer(4096, 256)[0] == 1 and E.lat_choose_infer(32768, 256)[0] == 0
        assert [q["kind"] for q in E.lat_split(512, 256, 4, 2, True)] == ["paired"]
        assert E.lat_split(1029, 256, 4, 2, True)[1] == dict(kind="single", S=1, grid=5, passes=1, tile_off=1024, tile_end=1029)


@pytest.mark.parametrize("mode", sorted(E.SPLIT_MODES))
def test_split_precision_premises(mode):
    """first-part case: every layer input at most 255, so its own first part in every mode (no second part anywhere); last-part case:
    every layer input recombines exactly from the parts the mode keeps, a non-zero share of them has a non-zero last part, and the
    sums of absolute terms stay below 2^24 with the inputs entering as their parts"""
    first, last = E.split_premise(E.SPLIT_FIRST, mode), E.split_premise(E.SPLIT_LAST[mode], mode)
    assert E.infer_preconditions(E.SPLIT_FIRST)["max_act"] <= E.SPLIT_MAX_OPERAND
    assert first["exact"] and first["last_share"] == 0 and first["max_abs_sum"] < 2 ** 24
    ref = E.infer_reference(E.SPLIT_FIRST)
    assert all(np.array_equal(E.split_parts(l.a, mode)[0], l.a) for l in ref.layers)
    assert last["exact"] and last["last_share"] > 0 and last["max_abs_sum"] < 2 ** 24
    # the split can fail: one part too few loses the inputs of the last-part case
    big = E.infer_reference(E.SPLIT_LAST[mode]).layers[-2].a
    assert not np.array_equal(sum(E.split_parts(big, mode)[:-1]), big)
    assert np.array_equal(E._bf16_rne(np.array([257.0, 255.0, -3.0], np.float32)), np.array([256.0, 255.0, -3.0], np.float32))
    assert np.array_equal(E._f16_rtz(np.array([2049.0, 4095.0, -4095.0, 2.0 ** -25], np.float32)),
                          np.array([2048.0, 4094.0, -4094.0, 0.0], np.float32))


def test_fused_warp_case_with_the_fold_meets_the_preconditions():
    case = E.WARP_FUSED_FOLD
    m = E.assert_preconditions(case)
    assert case.spr == 8 and case.n % case.spr == 0 and case.row_len == E.WARP_FUSED.row_len and m["max_act"] <= E.SPLIT_MAX_OPERAND
    assert E.preconditions(E.WARP_FUSED)["max_act"] <= E.SPLIT_MAX_OPERAND          # (every input its own first bf16 part)


def test_inference_profile_is_the_record_of_these_cases():
    """profiles/mlp_infer_exact_cases.txt holds what this run measures (rewrite it with `python tests/exact_net_ref.py`)"""
    with open(E.INFER_PROFILE) as f:
        assert f.read() == E.infer_profile_text()
    names = [c.name for c in E.ALL_INFER_CASES]
    assert len(set(names)) == len(names)
    assert sorted({c.net.width for c in E.INFER_CASES}) == [64, 100, 128, 200, 256, 320, 384, 448, 512, 576]


# ---- the split-precision cases with non-zero low parts of tests/test_gpu_mlp_split_exact.py -----------------------------------------------
@pytest.mark.parametrize("case", E.ALL_RICH_CASES + E.RICH_WARP_CASES, ids=IDS)
def test_low_part_premises_hold_on_the_float64_reference(case):
    """(a) every operand of every split GEMM - forward, dgrad, wgrad per layer - recombines exactly from the parts the mode keeps;
    (b) every product outside the mode's term table is zero; (c) every sum of absolute part-products is below 2^24; (e) a
    pre-activation is exactly zero and every ReLU feature of the rich layer is two-sided; (f, first half) the sum over the kept terms
    of the restated parts is the float64 reference; (d, per case) the terms the family is named for are non-zero in the rich layer's
    own GEMMs.  No family had to be dropped for any l*."""
    m = E.assert_rich_premises(case)
    print(E.describe_rich(case))
    for kind, terms in E.RICH_AT_LSTAR.get(case.family, {}).items():
        if case.rich is None or (kind == "dgrad" and case.rich in ("positions_pose_input", "linear1", "linear2")):
            continue
        for t in terms:
            assert (kind, None, "l*", t) in m["covered"], (case.name, kind, t)
    if case.family in ("X2", "G2"):          # (two-part modes: the last part is the second)
        assert m["last_a" if case.g_mult > 1 else "last_b"] > 0.25


@pytest.mark.parametrize("mode", sorted(E.RICH_CASES))
def test_low_part_families_reach_every_kind_of_gemm(mode):
    """(d, over the sweep): forward, dgrad, wide wgrad jobs and - f16x3, where they are split - narrow wgrad jobs each see the term a family
    is named for with a non-zero product; at least one wide-job and one narrow-job l* per family with a rich layer; n = 77 and 333"""
    families = sorted({c.family for c in E.RICH_CASES[mode]})
    assert families == {"bf16x6": ["G2X2", "W2G2", "W2X2", "W3", "W65793"]}.get(mode, ["G2", "W2", "X2"])
    for family in families:
        cases = [c for c in E.RICH_CASES[mode] if c.family == family]
        covered = set().union(*[{(k, j, t) for k, j, _, t in E.rich_premises(c)["covered"]} for c in cases])
        for want in E.rich_over_sweep(mode, family):
            assert want in covered, (mode, family, want)
        assert {c.net.n for c in cases} == {77, 333}
        rich = {c.rich for c in cases}
        assert rich == {None} or (rich & {"positional_net.1", "positional_net.4", "additional_linear_layer", "directional_input"} and
                                  rich & {"positions_pose_input", "directional_net.0", "rgb_out_layer"})
        assert all(c.q == {"W3": E.RICH_Q[mode], "W65793": 65793}.get(family, E.TWO_PART_Q[mode]) for c in cases if c.rich)
    sweep = [c for c in E.RICH_CASES[mode] if c.family in ("W3", "W2")]
    assert [(c.rich, c.net.n, c.net.n_layers) for c in sweep] == E.RICH_SWEEP
    assert sweep[-1].net.skips == (1,) and sweep[-1].rich == "positional_net.1" and sweep[2].net.skips == (4,)


@pytest.mark.parametrize("mode", sorted(E.RICH_CASES))
def test_dropping_a_kept_term_leaves_the_float64_reference(mode):
    """(f, second half): with any one kept term left out of the forward, the dgrad or the wgrad, the emulation differs from float64 in
    a case of the family named for that term - a kernel that loses the term cannot pass the GPU test"""
    ns = E.SPLIT_MODES[mode][0]
    assert set(E.RICH_SENSITIVE[ns]) == {(kind, t) for kind in ("fwd", "dgrad", "wgrad") for t in E.TERMS[ns]}
    for (kind, t), family in E.RICH_SENSITIVE[ns].items():
        cases = [c for c in E.RICH_CASES[mode] if c.family == family]
        assert any(not E.emulation_is_reference(c, mode, (kind, t)) for c in cases), (mode, kind, t, family)


def test_the_restated_split_and_the_constants():
    """257, 131329 and 2049 need every part of their mode under the pack kernels' rounding; 65793 = 65536 + 256 + 1 does NOT need three
    bf16 parts under round-to-nearest-even (66048 - 255), and no integer below 2^17 does; the f16x3 weight exponent takes the largest
    |w| of the layer to [2^14, 2^15); the term tables are those of mlp_bf16_device.h"""
    parts = lambda q, mode: [float(p[0, 0]) for p in E.weight_parts(np.array([[q, -1.0]]), mode)]
    assert parts(257, "bf16x3") == [256, 1] and parts(257, "bf16x6") == [256, 1, 0]
    assert parts(131329, "bf16x6") == [131072, 256, 1] and parts(65793, "bf16x6") == [66048, -255, 0]
    assert parts(2049, "f16x3") == [2048, 1] and parts(3 * 2049, "f16x3") == [6148, -1]          # (RNE on the weights: 6147 -> 6148)
    rng = np.random.default_rng(0)
    some = rng.integers(1, 2 ** 17, 4096).astype(np.float64)[None]
    assert not E.weight_parts(some, "bf16x6")[2].any() and np.array_equal(sum(E.weight_parts(some, "bf16x6")), some)
    w = np.array([[3.0, -2049.0, 0.0]])
    p = E.weight_parts(w, "f16x3")
    assert np.array_equal(sum(p), w) and np.array_equal(p[0] * 8, [[24.0, -16384.0, 0.0]])
    assert [float(v[0, 0]) for v in E.operand_parts(np.array([[6147.0]]), "f16x3", 12)] == [6144, 3]        # (truncation on the operands)
    assert [float(v[0, 0]) for v in E.split_parts(np.array([[6147.0, 9000.0]]), "f16x3")] == [6144, 3]
    assert E.TERMS[2] == ((1, 0), (0, 1), (0, 0)) and E.TERMS[3] == ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
    assert E.wgrad_is_wide(256, 256) and E.wgrad_is_wide(128, 256) and not E.wgrad_is_wide(128, 128) and not E.wgrad_is_wide(256, 3)
    assert not E.wgrad_is_wide(1, 256) and not E.wgrad_is_wide(3, 128)


def test_the_low_part_generator_makes_what_it_says():
    case = E.RICH_CASES["bf16x6"][2]
    state, inp, rows, d_raw = E.rich_data(case)
    assert case.rich == "positional_net.4" and case.q == 131329 and case.g_every == 16
    for name, n_out, n_in in E.render_net_shapes(*case.net[1:8]):
        w, b = state[name + ".weight"], state[name + ".bias"]
        assert w.shape == (n_out, n_in) and w.dtype == b.dtype == np.float32 and np.array_equal(b, np.rint(b))
        per_row = (w != 0).sum(1)
        assert (per_row == (E.HEAD_ENTRIES if n_out <= 3 else 2 if name == case.rich else 1)).all(), name
        assert set(np.unique(np.abs(w))) == {0.0, float(case.q) if name == case.rich else 1.0}
        used = (w != 0).sum(0)
        assert n_out <= 3 or used.max() - used.min() <= (2 if name == case.rich else 1) or name == case.rich, name
        assert n_in <= 256 or (w[:, 256:] != 0).any(0).all()          # the input columns of a skip layer / the directions are used
    assert set(np.unique(inp["x"])) == {-1.0, 0.0, 1.0} and np.array_equal(rows[:, :3], inp["x"])
    assert np.array_equal(rows[:, 3:], E.direction_premise(inp["d"]))
    live = np.nonzero(d_raw.any(1))[0]
    assert (live % 16 == 8).all() and len(live) >= 333 // 16 - 4 and set(np.unique(d_raw)) == {-1.0, 0.0, 1.0}
    again = E.rich_data.__wrapped__(case)
    assert all(np.array_equal(state[k], again[0][k]) for k in state) and np.array_equal(d_raw, again[3])
    x2 = E.rich_data(E.RICH_CASES["f16x3"][9])
    assert E.RICH_CASES["f16x3"][9].family == "X2" and set(np.unique(np.abs(x2[1]["x"]))) == {0.0, 2049.0}


@pytest.mark.parametrize("case", E.RICH_TEETH, ids=IDS)
def test_two_part_emulation_of_three_part_cases_leaves_float64(case):
    """the cases of the GPU test's teeth: emulated with the parts and terms of bf16x3, raw differs from the float64 reference"""
    assert case.mode == "bf16x6" and case.family in ("W3", "W2X2")
    raw, _, _ = E.split_emulate(case, "bf16x3")
    assert (raw != E.rich_reference(case).out).mean() > 0.1
    assert {c.family for c in E.RICH_TEETH} == {"W3", "W2X2"}


def test_split_profile_is_the_record_of_these_cases():
    """profiles/mlp_split_exact_cases.txt holds what this run measures (rewrite it with `python tests/exact_net_ref.py`)"""
    with open(E.SPLIT_PROFILE) as f:
        assert f.read() == E.split_profile_text()
    names = [c.name for c in E.ALL_RICH_CASES + E.RICH_WARP_CASES]
    assert len(set(names)) == len(names)


def test_profile_is_the_record_of_these_cases():
    """profiles/mlp_exact_cases.txt holds what this run measures (rewrite it with `python tests/exact_net_ref.py`)"""
    with open(E.PROFILE) as f:
        assert f.read() == E.profile_text()
