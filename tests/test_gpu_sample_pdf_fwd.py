"""sample_pdf_kernel (csrc/sampler.hip) against oracle.nerf_oracle bit for bit, through the C entries snerf_sample_pdf_f32,
snerf_sample_pdf_strict_f32, snerf_sample_pdf_bins_f32 and snerf_sample_pdf_bins_strict_f32 as ops.hierarchical_samples,
ops.sample_pdf, the single-call render and the one-call training step reach it.

The cases, their expected outputs and the premises that license equality (float64 sums that no order can change, a literal torch
restatement of the reference that gives the oracle's bits) are those of tests/sampler_fwd_ref.py, all of which
tests/test_sampler_fwd_host.py checks on the CPU.  Every comparison is np.testing.assert_array_equal: no tolerance, no case left out.
The indices, the samples, the merged depths and the points sit between canaries in the test's own buffers (Guarded of
tests/test_gpu_composite_bwd.py with a NaN of its own payload inside, so that a NaN the kernel owes counts as written; for the int64
indices its integer twin with -7 inside): every element must be written and no canary touched.  One line per case is printed before
its comparison (pytest -s; profiles/sample_pdf_fwd_cases.txt holds the table of the cases, a run, and what four one-line mutations of
the kernel and its launcher did to this module).

The shapes (sampler_fwd_ref.SHAPES) sit on the edges of the launcher's formulas: row lengths of a power of two and one off it in the
runtime count_below, the 64-entry chunks of the fp64 scan, n_in = 188 against 192 at the vector store's condition, 65 536 B of LDS
against 65 664 B at the raised limit, and 96 KiB.  The families put rays on the rank sort by an unsorted z and by an unsorted u with
a sorted z, beside fast rays in one workgroup, NaN and infinity into z, u on cdf entries and on their fp32 neighbours, samples on
coarse depths, and the gathered pairs on both sides of `denom < 1e-5`."""
from functools import lru_cache
from itertools import combinations

import numpy as np
import pytest
import torch

import sampler_fwd_ref as R
from oracle import nerf_oracle as O
from test_gpu_composite_bwd import CANARY, E_BADARG, GUARD, OK, Guarded, T

pytestmark = pytest.mark.gpu
F32 = np.float32
OUTPUTS = ("inds", "z_samples", "z_fine", "pts")
SUBSETS = [s for n in (1, 2, 3, 4) for s in combinations(OUTPUTS, n)]
SENTINEL, ICANARY = -7, 12345          # an index is 0 .. Nb


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class GuardedInt(Guarded):
    """Guarded for the int64 indices: -7 between two runs of canaries"""

    def __init__(self, dev, shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.all = torch.full((GUARD + self.n + GUARD,), ICANARY, device=dev, dtype=torch.int64)
        self.t = self.all[GUARD:GUARD + self.n]
        self.t.fill_(SENTINEL)

    def result(self, name):
        out, canaries = self._split()
        assert (canaries == ICANARY).all(), f"{name}: a canary was overwritten"
        assert not (out == SENTINEL).any(), f"{name}: {int((out == SENTINEL).sum())} of {out.size} elements were not written"
        return out

    def untouched(self):
        out, canaries = self._split()
        return bool((canaries == ICANARY).all() and (out == SENTINEL).all())


class GuardedNaN(Guarded):
    """Guarded whose NaN carries a payload no arithmetic produces, so that a NaN the kernel owes (a NaN or an infinity among the
    depths) counts as written; `off` floats past a 16-byte boundary"""
    FILL = 0x7FC0DEAD

    def __init__(self, dev, shape, off=0):
        self.shape, self.n, self.lo = shape, int(np.prod(shape)), GUARD + off
        self.all = torch.full((self.lo + self.n + GUARD,), CANARY, device=dev)
        self.t = self.all[self.lo:self.lo + self.n]
        self.t.view(torch.int32).fill_(self.FILL)
        assert self.t.data_ptr() % 16 == 4 * off and bool(torch.isnan(self.t).all())

    def _split(self):
        a = self.all.cpu().numpy()
        return a[self.lo:self.lo + self.n].reshape(self.shape), np.concatenate([a[:self.lo], a[self.lo + self.n:]])

    def result(self, name):
        out, canaries = self._split()
        assert (canaries == CANARY).all(), f"{name}: a canary was overwritten"
        unwritten = out.view(np.uint32) == self.FILL
        assert not unwritten.any(), f"{name}: {int(unwritten.sum())} of {out.size} elements were not written"
        return out

    def untouched(self):
        out, canaries = self._split()
        return bool((canaries == CANARY).all() and (out.view(np.uint32) == self.FILL).all())


def same(name, what, got, want):
    """equal values with NaNs equal by position, and for floats without NaN equal bits"""
    np.testing.assert_array_equal(got, want, err_msg=f"{name}: {what}")
    if got.dtype == F32:
        ok = ~np.isnan(want)
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32)[ok], np.ascontiguousarray(want).view(np.uint32)[ok]), f"{name}: {what} (bits)"


class Call:
    """one call of a merged entry on rays `rays` of inputs x (all of them by default): device inputs, guarded outputs, the launch and
    the checked results.  `tot` [B] selects the strict entry; `off` names the outputs placed one float off 16-byte alignment."""

    def __init__(self, dev, name, x, want=OUTPUTS, tot=None, rays=None, off=()):
        from smpl_nerf_amd import _lib
        self.lib, self.name = _lib.load(), name
        cut = lambda a: T(None if a is None else (a if rays is None else a[rays]), dev)
        self.z, self.w, self.o, self.d, self.tot = cut(x.z), cut(x.w), cut(x.o), cut(x.d), cut(tot)
        self.u = T(x.u, dev)
        self.B, self.Nc, self.Nf = self.z.shape[0], self.z.shape[1], len(x.u)
        Nt = self.Nc + self.Nf
        shapes = dict(inds=(self.B, self.Nf), z_samples=(self.B, self.Nf), z_fine=(self.B, Nt), pts=(self.B, Nt, 3))
        self.out = {k: GuardedInt(dev, shapes[k]) if k == "inds" else GuardedNaN(dev, shapes[k], int(k in off)) for k in want}

    def run(self, strict=None, **over):
        from smpl_nerf_amd._lib import current_stream, ptr
        p = lambda k: ptr(self.out[k].t) if k in self.out else None
        a = dict(z=ptr(self.z), w=ptr(self.w), u=ptr(self.u), o=ptr(self.o), d=ptr(self.d), tot=ptr(self.tot), B=self.B, Nc=self.Nc, Nf=self.Nf)
        a.update(over)
        strict = self.tot is not None if strict is None else strict
        outs = (p("inds"), p("z_samples"), p("z_fine"), p("pts"), current_stream())
        with torch.cuda.device(self.z.device):
            if strict:
                rc = self.lib.snerf_sample_pdf_strict_f32(a["z"], a["w"], a["u"], a["o"], a["d"], a["tot"], a["B"], a["Nc"], a["Nf"], *outs)
            else:
                rc = self.lib.snerf_sample_pdf_f32(a["z"], a["w"], a["u"], a["o"], a["d"], a["B"], a["Nc"], a["Nf"], *outs)
        torch.cuda.synchronize()
        return rc

    def results(self):
        assert self.run() == OK, self.lib.snerf_last_error_string()
        return {k: o.result(f"{self.name} {k}") for k, o in self.out.items()}

    def untouched(self):
        return all(o.untouched() for o in self.out.values())


class BinsCall:
    """one call of a literal sample_pdf(bins, weights) entry: bins [B, Nb], interior weights [B, Nb - 1]"""

    def __init__(self, dev, name, x, tot=None):
        from smpl_nerf_amd import _lib
        self.lib, self.name = _lib.load(), name
        self.bins, self.w, self.u, self.tot = T(R.bins_of(x.z), dev), T(x.w[:, 1:-1], dev), T(x.u, dev), T(tot, dev)
        self.B, self.Nb, self.Nf = self.bins.shape[0], self.bins.shape[1], len(x.u)
        assert self.w.is_contiguous() and self.w.shape == (self.B, self.Nb - 1)
        self.out = dict(inds=GuardedInt(dev, (self.B, self.Nf)), z_samples=GuardedNaN(dev, (self.B, self.Nf)))

    def run(self, strict=None, **over):
        from smpl_nerf_amd._lib import current_stream, ptr
        a = dict(bins=ptr(self.bins), w=ptr(self.w), u=ptr(self.u), tot=ptr(self.tot), B=self.B, Nb=self.Nb, Nf=self.Nf)
        a.update(over)
        strict = self.tot is not None if strict is None else strict
        outs = (ptr(self.out["inds"].t), ptr(self.out["z_samples"].t), current_stream())
        with torch.cuda.device(self.bins.device):
            if strict:
                rc = self.lib.snerf_sample_pdf_bins_strict_f32(a["bins"], a["w"], a["u"], a["tot"], a["B"], a["Nb"], a["Nf"], *outs)
            else:
                rc = self.lib.snerf_sample_pdf_bins_f32(a["bins"], a["w"], a["u"], a["B"], a["Nb"], a["Nf"], *outs)
        torch.cuda.synchronize()
        return rc

    results, untouched = Call.results, Call.untouched


@lru_cache(maxsize=None)
def run_case(dev, name, strict=False):
    """the four outputs of one case, launched once and shared by the tests that read them"""
    x = R.inputs(name)
    got = Call(dev, name, x, tot=R.strict_tot(x.w) if strict else None).results()
    for a in got.values():
        a.setflags(write=False)
    return got


def hold(name, got, e, keys=OUTPUTS):
    """every output is compared before any of them fails the test"""
    want = dict(inds=e.inds, z_samples=e.samples, z_fine=e.z_fine, pts=e.pts)
    failed = []
    for k in keys:
        try:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, got[k].dtype)
            same(name, k, got[k], want[k])
        except AssertionError as err:
            failed.append(str(err)[:600])
    assert not failed, "\n".join(failed)


ALL = [c.name for c in R.CASES]


# ---------------------------------------------------------------------------------------------- 1. every case against the oracle
@pytest.mark.parametrize("name", ALL)
def test_every_case_is_the_oracles(dev, name):
    """the kernel's own fp64 sum is the oracle's default"""
    c, k = R.CASE[name], R.counts(name)
    print(f"{name}: {R.lds_bytes(c.Nc, c.Nf)} B of LDS{' (raised)' if R.raised(c.Nc, c.Nf) else ''}, {'vector' if R.vector_store(c.Nc, c.Nf) else 'dword'} stores, "
          f"{R.instance(c.Nc, c.Nf)} instance, rank sort on {k['fallback_rays']} of {c.B} rays; inds, z_samples, z_fine, pts against the oracle")
    hold(name, run_case(dev, name), R.expected(name))


@pytest.mark.parametrize("name", ALL)
def test_every_case_is_the_oracles_with_a_given_sum(dev, name):
    """the strict entry with a `tot` one ulp off the fp64 sum on two rays of three, the same `tot` to the oracle: the entry reads it"""
    e = R.expected(name, True)
    print(f"{name}: strict, samples that differ from the default sum's: {int((e.samples != R.expected(name).samples).sum())} of {e.samples.size}")
    hold(name + " strict", run_case(dev, name, True), e)


# ---------------------------------------------------------------------------------------------- 2. the bins entries
@pytest.mark.parametrize("name", ALL)
def test_the_bins_entries(dev, name):
    """sample_pdf(bins, weights) on the bins and the interior weights of the same cases - Nb = 2, 64, 65 and 1023 with Nf = 1024 among
    them: the merged entry's and the oracle's indices and samples, with the kernel's own sum and with a given one"""
    c, x = R.CASE[name], R.inputs(name)
    print(f"{name}: bins entries, Nb {c.Nc - 1} Nf {c.Nf}, own sum and given sum; inds, z_samples against the oracle and the merged entry")
    for strict in (False, True):
        got = BinsCall(dev, name, x, tot=R.strict_tot(x.w) if strict else None).results()
        hold(f"{name} bins{' strict' if strict else ''}", got, R.expected(name, strict), ("inds", "z_samples"))
        merged = run_case(dev, name, strict)
        for k in ("inds", "z_samples"):
            same(name, f"bins entry against the merged entry, {k}", got[k], merged[k])


def test_the_bins_cases_reach_their_edges():
    nb = {(R.CASE[n].Nc - 1, R.CASE[n].Nf) for n in ALL}
    assert {2, 64, 65} <= {a for a, _ in nb} and (1023, 1024) in nb and (1023, 1) in nb


# ---------------------------------------------------------------------------------------------- 3. output subsets
@pytest.mark.parametrize("shape", [(9, 7), (48, 48), (64, 128)], ids=str)
@pytest.mark.parametrize("want", SUBSETS, ids=lambda s: "+".join(s))
def test_output_subsets(dev, want, shape):
    """each of the 15 non-empty subsets of (inds, z_samples, z_fine, pts), the others null, gives the bits of the four-output call -
    with neither z_fine nor pts the kernel returns before the merge"""
    name = R._name(*shape, "shuffled", "rand4", "linspace") if shape != (48, 48) else R._name(*shape, *R.BASE)
    full = run_case(dev, name)
    part = Call(dev, name, R.inputs(name), want=want).results()
    assert tuple(part) == want
    for k in want:
        same(name, f"{k} of {'+'.join(want)}", part[k], full[k])


@pytest.mark.parametrize("shape", [(9, 7), (48, 48), (64, 128)], ids=str)
def test_no_output_is_ok_and_writes_nothing(dev, shape):
    name = R._name(*shape, *R.BASE)
    x = R.inputs(name)
    for tot in (None, R.strict_tot(x.w)):
        call = Call(dev, name, x, tot=tot)
        outs, call.out = call.out, {}                          # four null pointers
        assert call.run() == OK
        call.out = outs
        assert call.untouched()


# ---------------------------------------------------------------------------------------------- 4. alignment
@pytest.mark.parametrize("off", [("z_fine",), ("pts",), ("z_fine", "pts")], ids=lambda s: "+".join(s))
@pytest.mark.parametrize("shape", [(48, 48), (1024, 1024)], ids=str)
def test_misaligned_outputs_take_the_dword_stores_to_the_same_bits(dev, shape, off):
    """z_fine / pts one float off 16-byte alignment: the dword stores, the bits of the aligned call's vector stores - at (48, 48) the
    staging loop's last chunk is 32 samples, at (1024, 1024) the launch raises the LDS limit"""
    name = R._name(*shape, *R.BASE)
    assert R.vector_store(*shape)
    aligned = run_case(dev, name)
    got = Call(dev, name, R.inputs(name), off=off).results()
    for k in OUTPUTS:
        same(name, f"{k} with {'+'.join(off)} misaligned", got[k], aligned[k])


# ---------------------------------------------------------------------------------------------- 5. rows and the batch; two runs
@pytest.mark.parametrize("shape", [(66, 129), (64, 128)], ids=str)
def test_rows_do_not_depend_on_the_batch(dev, shape):
    """ray k alone (B = 1) is ray k of the batch of nine, for the fast rays and the rank-sorted ones of the shuffled family"""
    name = R._name(*shape, "shuffled", "rand4", "linspace")
    x, full = R.inputs(name), run_case(dev, name)
    for k in range(R.CASE[name].B):
        one = Call(dev, f"{name} ray {k}", x, rays=[k]).results()
        for key in OUTPUTS:
            same(name, f"ray {k} alone, {key}", one[key], full[key][k:k + 1])
    for rays in ([0, 1, 2, 3], [3, 2, 1, 0, 8]):                                  # a full workgroup; the rays in another order
        part = Call(dev, f"{name} rays {rays}", x, rays=rays).results()
        for key in OUTPUTS:
            same(name, f"rays {rays}, {key}", part[key], full[key][rays])


@pytest.mark.parametrize("name", [R._name(66, 129, "shuffled", "rand4", "linspace"), R._name(64, 128, "special", "rand4", "linspace"),
                                  R._name(1024, 1024, "jitter", "rand4", "unsorted")])
def test_two_runs_give_the_same_bits(dev, name):
    a, b = run_case(dev, name), Call(dev, name, R.inputs(name)).results()
    for k in OUTPUTS:
        assert np.array_equal(a[k].view(np.uint32 if k != "inds" else np.int64), b[k].view(np.uint32 if k != "inds" else np.int64)), k


# ---------------------------------------------------------------------------------------------- 6. small and large calls interleaved
def test_small_and_large_calls_interleaved(dev):
    """the raised limit belongs to the function: a small launch after a 96 KiB one, and the 96 KiB one again, give the oracle's bits"""
    big, small = R._name(1024, 1024, *R.BASE), R._name(9, 7, *R.BASE)
    for name in (big, small, big, R._name(513, 1024, *R.BASE), small, R._name(512, 1024, *R.BASE), R._name(1024, 1, *R.BASE)):
        x = R.inputs(name)
        hold(name, Call(dev, name, x).results(), R.expected(name))
        hold(name + " bins", BinsCall(dev, name, x).results(), R.expected(name), ("inds", "z_samples"))


# ---------------------------------------------------------------------------------------------- 7. arguments
REFUSALS = [("Nc = 2", dict(Nc=2)), ("Nc = 1025", dict(Nc=1025)), ("Nf = 0", dict(Nf=0)), ("Nf = 1025", dict(Nf=1025)), ("B < 0", dict(B=-1)),
            ("null z", dict(z=None)), ("null weights", dict(w=None)), ("null u", dict(u=None)), ("pts without o", dict(o=None)),
            ("pts without d", dict(d=None))]


@pytest.mark.parametrize("strict", [0, 1], ids=["plain", "strict"])
@pytest.mark.parametrize("name,over", REFUSALS, ids=[n for n, _ in REFUSALS])
def test_refusals_return_before_any_launch(dev, name, over, strict):
    case = R._name(9, 7, *R.BASE)
    x = R.inputs(case)
    call = Call(dev, case, x, tot=R.strict_tot(x.w) if strict else None)
    assert call.run(**over) == E_BADARG, name
    assert call.lib.snerf_last_error_string()
    assert call.untouched(), f"{name}: the refused call wrote something"


def test_the_strict_entries_refuse_a_null_tot(dev):
    case = R._name(9, 7, *R.BASE)
    x = R.inputs(case)
    for call in (Call(dev, case, x), BinsCall(dev, case, x)):
        assert call.run(strict=True) == E_BADARG and call.lib.snerf_last_error_string() and call.untouched()


@pytest.mark.parametrize("strict", [0, 1], ids=["plain", "strict"])
@pytest.mark.parametrize("name,over", [("Nb = 1", dict(Nb=1)), ("Nb = 1024", dict(Nb=1024)), ("Nf = 0", dict(Nf=0)), ("Nf = 1025", dict(Nf=1025)),
                                       ("B < 0", dict(B=-1)), ("null bins", dict(bins=None)), ("null weights", dict(w=None)), ("null u", dict(u=None))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_the_bins_entries_refuse(dev, name, over, strict):
    case = R._name(9, 7, *R.BASE)
    x = R.inputs(case)
    call = BinsCall(dev, case, x, tot=R.strict_tot(x.w) if strict else None)
    assert call.run(**over) == E_BADARG, name
    assert call.lib.snerf_last_error_string()
    assert call.untouched(), f"{name}: the refused call wrote something"


def test_pts_absent_needs_no_o_and_d(dev):
    name = R._name(9, 7, *R.BASE)
    call = Call(dev, name, R.inputs(name), want=("inds", "z_samples", "z_fine"))
    assert call.run(o=None, d=None) == OK
    full = run_case(dev, name)
    for k, o in call.out.items():
        same(name, k, o.result(k), full[k])


def test_an_empty_batch_is_ok_and_writes_nothing(dev):
    name = R._name(9, 7, *R.BASE)
    x = R.inputs(name)
    for tot in (None, R.strict_tot(x.w)):
        call = Call(dev, name, x, tot=tot)
        assert call.run(B=0) == OK and call.untouched()
        assert call.run(B=0, z=None, w=None, u=None, o=None, d=None) == OK and call.untouched()
        bins = BinsCall(dev, name, x, tot=tot)
        assert bins.run(B=0) == OK and bins.run(B=0, bins=None, w=None, u=None) == OK and bins.untouched()


# ---------------------------------------------------------------------------------------------- 8. the front end makes this call
@pytest.mark.parametrize("name", [R._name(18, 33, "grid", "plateau", "linspace"), R._name(66, 129, "jitter", "rand4", "unsorted"),
                                  R._name(64, 128, "shuffled", "rand4", "linspace"), R._name(513, 1024, "grid", "plateau", "cdf_neighbours")])
def test_the_front_end_makes_this_call(dev, name):
    """ops.hierarchical_samples and ops.sample_pdf with the case's u in ops._U_CACHE: the C entry's bits, with and without `tot`"""
    from smpl_nerf_amd import ops
    x, Nf = R.inputs(name), R.CASE[name].Nf
    k = R.counts(name)
    assert k["cdf_ties"] > 9 or k["fallback_rays"]
    key = (Nf, str(dev))
    before = ops._U_CACHE.get(key)
    ops._U_CACHE[key] = T(x.u, dev)
    try:
        for strict in (False, True):
            direct = run_case(dev, name, strict)
            tot = T(R.strict_tot(x.w), dev) if strict else None
            r = ops.hierarchical_samples(T(x.o, dev), T(x.d, dev), T(x.z, dev), T(x.w, dev), Nf, want_inds=True, want_samples=True, tot=tot)
            for kk in OUTPUTS:
                same(name, f"hierarchical_samples {kk}", r[kk].cpu().numpy(), direct[kk])
            r = ops.hierarchical_samples(T(x.o, dev), T(x.d, dev), T(x.z, dev), T(x.w, dev), Nf, tot=tot)
            assert r["inds"] is None and r["z_samples"] is None
            for kk in ("z_fine", "pts"):
                same(name, f"hierarchical_samples without inds, {kk}", r[kk].cpu().numpy(), direct[kk])
        with torch.no_grad():
            zs = ops.sample_pdf(T(R.bins_of(x.z), dev), T(x.w, dev)[:, 1:-1], O.Args(number_fine_samples=Nf))
        same(name, "ops.sample_pdf", zs.cpu().numpy(), run_case(dev, name)["z_samples"])
    finally:
        if before is None:
            ops._U_CACHE.pop(key, None)
        else:
            ops._U_CACHE[key] = before
