"""tests/sampler_fwd_ref.py without a GPU: the premises of every case that tests/test_gpu_sample_pdf_fwd.py runs.  Nothing here is a
tolerance: the shape edges come from the launcher's formulas in csrc/sampler.hip (restated in sampler_fwd_ref), the exactness of the
sums is checked with math.fsum, and the oracle is held bit for bit to a literal torch restatement of the reference.  pytest -s prints
the counts; profiles/sample_pdf_fwd_cases.txt is their record."""
import numpy as np
import pytest

import sampler_fwd_ref as R

F32 = np.float32


@pytest.fixture(scope="module")
def table():
    return {c.name: R.counts(c.name) for c in R.CASES}


# ------------------------------------------------------------------------------------------------ the shapes sit on their edges
def test_the_shapes_sit_on_the_launchers_edges():
    assert R.round4(1) == R.round4(4) == 4 and R.round4(5) == 8 and R.round4(0) == 0
    lds = lambda s: R.lds_bytes(*s)
    # the formula of the issue: 16 * (round4(3 Nc - 2 + Nf) + round4(Nc + Nf))
    for Nc, Nf in R.SHAPES + R.TIE_SHAPES:
        assert lds((Nc, Nf)) == 16 * (R.round4(3 * Nc - 2 + Nf) + R.round4(Nc + Nf)) == R.WAVES * R.per_wave(Nc, Nf) * 4
    assert lds((512, 1024)) == 65536 and not R.raised(512, 1024)
    assert lds((513, 1024)) == 65664 and R.raised(513, 1024)
    assert lds((1024, 1024)) == 96 * 1024 and lds((1024, 1)) == 65600 and R.raised(1024, 1)
    assert lds((200, 700)) == 35200 and 35200 // 1024 == 34      # the largest shape of the older forward tests: 34 KiB
    assert max(lds((Nc, Nf)) for Nc in (1023, 1024) for Nf in (1023, 1024)) == 96 * 1024      # the entry's limit
    # the vector store's condition: n_in >= 3 * 64 with Nt = 96 on both sides; a last staged chunk of 32 samples
    assert R.n_in(47, 49) == 188 and not R.vector_store(47, 49) and R.n_in(48, 48) == 192 and R.vector_store(48, 48)
    assert 47 + 49 == 48 + 48 == 96 and 96 % 4 == 0 and 96 % R.WAVE == 32
    small = [(3, 1), (4, 2), (5, 5), (9, 7), (10, 8), (17, 3)]
    assert [Nc - 1 for Nc, _ in small] == [2, 3, 4, 8, 9, 16] and not any(R.vector_store(*s) for s in small)
    assert [Nc - 2 for Nc, _ in [(65, 63), (66, 129), (67, 64), (130, 65)]] == [63, 64, 65, 128]    # the scan's chunks
    assert (66 + 129) % 4 != 0 and not R.vector_store(66, 129)
    assert R.vector_store(64, 128) and R.vector_store(1024, 1024) and R.vector_store(512, 1024) and not R.vector_store(513, 1024)
    assert (2048 % R.WAVE, (512 + 1024) % R.WAVE) == (0, 0)
    assert [R.instance(*s) for s in R.SHAPES].count("64+128") == 1
    assert [Nc - 2 for Nc, _ in R.TIE_SHAPES] == [4, 8, 64, 16]


def test_every_family_runs_at_every_crossed_shape():
    names = set(R.CASE)
    assert len(names) == len(R.CASES)
    for Nc, Nf in R.SHAPES:
        assert R._name(Nc, Nf, *R.BASE) in names
    for Nc, Nf in R.CROSS:
        for zf in R.Z_FAMILIES:
            assert R._name(Nc, Nf, zf, R.BASE[1], R.BASE[2]) in names
        for wf in R.W_FAMILIES:
            assert R._name(Nc, Nf, R.BASE[0], wf, R.BASE[2]) in names
        for uf in R.U_FAMILIES:
            assert R._name(Nc, Nf, R.BASE[0], R.BASE[1], uf) in names
    assert all(c.B == 9 == 2 * R.WAVES + 1 for c in R.CASES)
    print(f"{len(R.CASES)} cases")


def test_the_inputs_are_what_the_families_say():
    for c in R.CASES:
        x = R.inputs(c.name)
        assert (x.w >= 0).all() and (x.w <= 1).all()
        inc = (x.z[:, :-1] <= x.z[:, 1:]).all(-1)
        if c.zfam in ("jitter", "grid"):
            assert (np.diff(x.z) > 0).all()
        elif c.zfam == "runs":
            assert inc.all() and (np.diff(x.z) == 0).any(-1).all()
        elif c.zfam == "equal":
            assert (x.z == x.z[:, :1]).all()
        elif c.zfam == "descending":
            assert (np.diff(x.z) < 0).all()
        elif c.zfam == "shuffled":
            assert inc[0::2].all() and not inc[1::2].any()
        elif c.zfam == "special":
            assert np.isnan(x.z[0]).sum() == 1 and x.z[1, -1] == np.inf and np.isfinite(x.z[2:]).all() and x.d[2, 1] == 0
        interior = x.w[:, 1:-1]
        if c.wfam in ("zero", "ends"):
            assert not interior.any() and ((x.w[:, 0] == 1).all() and (x.w[:, -1] == 1).all()) == (c.wfam == "ends")
        elif c.wfam == "plateau":
            assert (interior == interior[0, 0]).all() and interior[0, 0] > 0
        elif c.wfam.startswith("spike"):
            at = {"spike_first": 0, "spike_mid": (c.Nc - 2) // 2, "spike_last": c.Nc - 3}[c.wfam]
            assert (interior[:, at] == 1).all() and interior.sum() == c.B
        elif c.wfam == "alternating":
            assert set(np.unique(interior)) <= {F32(0), F32(0.5)} and (interior[:, 0] == 0.5).all()
        elif c.wfam == "tiny":
            assert set(np.unique(x.w)) == {F32(1e-30), F32(1e-5)} and F32(1e-30) + R.EPS == R.EPS
        if c.ufam == "sorted01" and c.Nf > 1:
            assert x.u[0] == 0 and x.u[-1] == 1 and (np.diff(x.u) >= 0).all()
        elif c.ufam == "unsorted":
            assert (np.diff(x.u) < 0).any() and (x.u == 0).any() and (x.u == 1).any()


# ------------------------------------------------------------------------------------------------ the sums are order-free
def test_the_sums_are_order_free():
    done = {}
    for c in R.CASES:
        key = (c.wfam, c.Nc, c.B)
        if key not in done:
            done[key] = R.sums_are_order_free(*key)
    print(f"{len(done)} sets of weights, {sum(done.values())} prefixes, all exact in float64")
    assert len(done) >= len(R.W_FAMILIES) * len(R.CROSS)


def test_rand4_rows_of_64_and_1024_are_order_free():
    """the check of the issue: 100 rows each"""
    for Nc in (64, 1024):
        assert R.sums_are_order_free("rand4", Nc, 100) == 2 * 100 * (Nc - 2)


# ------------------------------------------------------------------------------------------------ the ties exist
def test_the_ties_exist(table):
    for Nc, Nf in R.TIE_SHAPES:
        name = R._name(Nc, Nf, "grid", "plateau", "linspace")
        k = table[name]
        print(R.describe(name))
        if (Nc, Nf) == (18, 33):
            assert k["cdf_ties_ray0"] == 17 and k["on_coarse"] > 0
        else:
            assert k["cdf_ties_ray0"] == Nf
        assert k["cdf_ties"] == 9 * k["cdf_ties_ray0"] and k["on_bin"] > 0
    assert table[R._name(18, 33, "grid", "plateau", "linspace")]["on_coarse"] >= 9 * 8      # (u = k / 32 with k odd: half way between two bins)
    assert sum(table[c.name]["on_coarse"] > 0 for c in R.CASES) >= 4 and sum(table[c.name]["cdf_ties"] > 0 for c in R.CASES) >= 8


def test_the_cdf_neighbours_sit_on_both_sides_of_an_entry_and_on_it():
    seen = 0
    for c in R.CASES:
        if c.ufam != "cdf_neighbours":
            continue
        x, e = R.inputs(c.name), R.expected(c.name)
        cdf = e.cdf[0]
        on = [v for v in cdf if (x.u == v).any() and (x.u == np.nextafter(v, F32(-np.inf))).any() and (x.u == np.nextafter(v, F32(np.inf))).any()]
        assert len(on) >= min(2, c.Nf // 3), c.name
        assert cdf[0] in on and x.u.min() < 0                                      # below the first entry: the index 0
        # ray 0's index steps up exactly at the entry: 'right' counts it
        for v in on:
            i_dn, i_on = (e.inds[0][x.u == t][0] for t in (np.nextafter(v, F32(-np.inf)), v))
            assert i_on >= i_dn + 1 and i_on == (cdf <= v).sum() and i_dn == (cdf < v).sum(), (c.name, v)
        assert (e.inds[0] == 0).any()
        seen += 1
    assert seen == 2 * len(R.CROSS)


# ------------------------------------------------------------------------------------------------ both sides of denom < 1e-5
def test_both_sides_of_the_denominators_threshold(table):
    for c in R.CASES:
        if c.wfam in R.DENOM_FAMILIES:
            k = table[c.name]
            print(f"{c.name:<44} denom < 1e-5: {k['denom_small']:>5}   >= 1e-5: {k['denom_large']:>5}")
            assert k["denom_small"] > 0 and k["denom_large"] > 0, c.name


# ------------------------------------------------------------------------------------------------ each ray takes the path intended
def test_each_ray_takes_the_path_intended(table):
    for c in R.CASES:
        x, e = R.inputs(c.name), R.expected(c.name)
        fast = R.ray_paths(x, e)
        if c.ufam == "unsorted":
            assert (np.diff(x.z) > 0).all() and not fast.any(), c.name           # sorted z: only sorted_s sends them to the rank sort
        elif c.zfam == "descending":
            assert not fast.any()
        elif c.zfam == "shuffled":
            assert fast[0::2].all() and not fast[1::2].any(), c.name
            assert table[c.name]["mixed_groups"] == 2                             # both full workgroups; the third holds ray 8 alone
        elif c.zfam == "special":
            assert not fast[0] and not fast[1] and fast[2:].all(), c.name
        elif c.zfam in ("jitter", "grid", "runs", "equal"):
            assert fast.all(), c.name
    assert R.instance(64, 128) == "64+128"
    runtime_fallback = [c.name for c in R.CASES if R.instance(c.Nc, c.Nf) == "runtime" and table[c.name]["fallback_rays"]]
    assert any(R.CASE[n].ufam == "unsorted" for n in runtime_fallback) and any(R.raised(R.CASE[n].Nc, R.CASE[n].Nf) for n in runtime_fallback)


# ------------------------------------------------------------------------------------------------ the oracle is the reference's
def _same(name, what, got, want):
    np.testing.assert_array_equal(got, want, err_msg=f"{name}: {what}")
    if got.dtype == F32:
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), f"{name}: {what} (bits)"


@pytest.mark.parametrize("name", [c.name for c in R.CASES if not R.has_specials(R.inputs(c.name))])
def test_the_oracle_is_the_references(name):
    x = R.inputs(name)
    tot, inds, samples, z_fine, pts = R.torch_reference(x)
    e = R.oracle(x, tot)
    _same(name, "inds", inds, e.inds)
    _same(name, "samples", samples, e.samples)
    _same(name, "z_fine", z_fine, e.z_fine)
    _same(name, "pts", pts, e.pts)


def test_nan_and_infinity_sort_last_in_the_oracle():
    names = [c.name for c in R.CASES if R.has_specials(R.inputs(c.name))]
    assert len(names) == len(R.CROSS)
    for name in names:
        for strict in (False, True):
            e = R.expected(name, strict)
            nan = np.isnan(e.z_fine)
            assert nan[0].any() and not nan[2:].any(), name
            for r in np.flatnonzero(nan.any(-1)):
                k = int(nan[r].sum())
                assert nan[r, -k:].all() and not nan[r, :-k].any()                 # the NaNs come last
                assert (e.z_fine[r, :-k - 1] <= e.z_fine[r, 1:-k]).all()
            assert np.isinf(e.z_fine[1]).any() and np.isfinite(e.pts[2, :, 1]).all()
            np.testing.assert_array_equal(e.z_fine, e.z_fine.copy())                # NaNs compare equal by position


def test_the_strict_sums_differ_from_the_default_by_one_ulp():
    for c in R.CASES:
        w = R.inputs(c.name).w
        a, b = R.default_tot(w).view(np.int32).astype(np.int64), R.strict_tot(w).view(np.int32).astype(np.int64)
        assert ((b - a)[0::3] == 1).all() and ((b - a)[1::3] == -1).all() and ((b - a)[2::3] == 0).all()
    changed = sum(not np.array_equal(R.expected(c.name).samples, R.expected(c.name, True).samples) for c in R.CASES)
    print(f"the one-ulp sums change the samples of {changed} of {len(R.CASES)} cases")
    assert changed > len(R.CASES) // 2


# ------------------------------------------------------------------------------------------------ the record
def test_profile_is_the_record_of_these_cases():
    """profiles/sample_pdf_fwd_cases.txt holds what this run computes (rewrite its table with `python tests/sampler_fwd_ref.py`)"""
    with open(R.PROFILE) as f:
        text = f.read()
    assert R.stable_part(text) == R.stable_part(R.profile_text())
    assert R.RUN_MARK in text
