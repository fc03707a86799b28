"""sample_pdf_bwd_kernel (csrc/sampler.hip) against float64, through the C entry snerf_sample_pdf_bins_bwd_f32 as ops._SamplePdfGrad
calls it, with the indices of oracle.sample_pdf_detail (which the forward tests hold the forward kernel to bit for bit).

The reference is tests/scan_bwd_ref.sample_pdf in float64, the yardstick the same restatement in fp32, and d bins and d weights are
held per ray to E(kernel) <= max(8 E(fp32 CPU), 2^-21) - the rule of tests/scan_bwd_ref.py, whose cases and premises (every gathered
pair decisively on one side of `denom < 1e-5`, the same side in fp32 and float64) tests/test_scan_bwd_host.py checks on the CPU.  Every
figure is printed before the assert (pytest -s; profiles/scan_bwd_errors.txt holds a run).  d bins and d weights are NaN-filled and sit
between canaries in the test's own buffers: every element must be written and no canary touched.

The shapes: one weight (Nb = 2, whose gradient is zero in exact arithmetic), Nb on both sides of the 64-entry scan chunk, Nf = 1 and
Nf off a multiple of 64, nine rays (a multiple of a workgroup's four plus one), and Nb = 1023 with Nf = 1024: 96 KiB of LDS, the
raised-limit launch.

Measured on an MI355X (profiles/scan_bwd_errors.txt has every figure), worst row of each of the 30 calls of the rule: d bins
E kernel 3.9e-8 .. 4.3e-5 against 1.4e-8 .. 1.5e-4 for the fp32 CPU restatement, a ratio of 0.28 .. 5.20; d weights 8.9e-8 .. 4.6e-5
against 5.2e-8 .. 4.9e-5, a ratio of 0.64 .. 3.11 (both grow with Nb: t = (u - c0) / denom carries the fp32 cdf's rounding over denom).
At Nb = 2 with Nf = 1 both are exactly zero or exact; at Nb = 2 with Nf = 5 and at the u = 1 sample with index Nb - 1 the float64
d weights are themselves round-off (1e-11 and less) of a gradient that is zero in exact arithmetic, which the fp32 restatement
misses as widely as the kernel does."""
import numpy as np
import pytest
import torch

import scan_bwd_ref as S
from oracle import nerf_oracle as O
from test_gpu_composite_bwd import E_BADARG, OK, Guarded, T

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def tot_f32(c):
    """the fp32 of the float64 sum of weights + 1e-5: what the kernel computes where no `tot` is given (and the oracle with it)"""
    return np.sum((c.weights + F32(1e-5)).astype(np.float64), -1).astype(F32)


class Call:
    """one backward call on the first `rays` rays of case `c`, inside the guards of test_gpu_composite_bwd.Guarded"""

    def __init__(self, dev, c, tot=None, rays=None, inds=None):
        from smpl_nerf_amd import _lib
        self.lib, self.c = _lib.load(), c
        self.B, self.Nb, self.Nf = (len(c.bins) if rays is None else rays), c.bins.shape[1], len(c.u)
        cut = lambda a: T(None if a is None else a[:self.B], dev)
        self.bins, self.w, self.d_zs, self.inds, self.tot = cut(c.bins), cut(c.weights), cut(c.d_zs), cut(c.inds if inds is None else inds), cut(tot)
        assert self.inds.dtype == torch.int64
        self.u = T(c.u, dev)
        self.out = dict(d_bins=Guarded(dev, (self.B, self.Nb)), d_weights=Guarded(dev, (self.B, self.Nb - 1)))

    def run(self, **over):
        from smpl_nerf_amd._lib import current_stream, ptr
        a = dict(bins=ptr(self.bins), Nb=self.Nb, Nf=self.Nf)
        a.update(over)
        with torch.cuda.device(self.bins.device):
            rc = self.lib.snerf_sample_pdf_bins_bwd_f32(a["bins"], ptr(self.w), ptr(self.u), ptr(self.inds), ptr(self.tot), ptr(self.d_zs), self.B,
                                                        a["Nb"], a["Nf"], ptr(self.out["d_bins"].t), ptr(self.out["d_weights"].t), current_stream())
        torch.cuda.synchronize()
        return rc

    def results(self):
        assert self.run() == OK, self.lib.snerf_last_error_string()
        return {k: o.result(f"{self.c.name} {k}") for k, o in self.out.items()}

    def untouched(self):
        return all(o.untouched() for o in self.out.values())


def hold_case(dev, c, **kw):
    r64, r32 = S.sample_pdf(c, torch.float64), S.sample_pdf(c, torch.float32)
    S.sampler_premises(c, r64)
    got = Call(dev, c, **kw).results()
    for k in got:
        S.hold(f"{c.name} {k}", got[k], r32[k], r64[k])
    return got


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


# ---------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("kind,Nb,Nf", S.sampler_sweep(), ids=lambda v: str(v))
def test_shape_sweep(dev, kind, Nb, Nf):
    hold_case(dev, S.sampler_case(kind, S.SAMPLER_B, Nb, Nf))


# ---------------------------------------------------------------------------------------------- single cases
@pytest.mark.parametrize("kind", ["flat", "spiky"])
def test_the_raised_lds_limit(dev, kind):
    """Nb = 1023, Nf = 1024: 4 x (2048 + 4096) floats = 96 KiB of LDS per workgroup"""
    hold_case(dev, S.sampler_case(kind, 5, *S.SAMPLER_BIG))


def test_tot_given_or_summed_in_the_kernel(dev):
    c = S.sampler_case("cube", 5, 65, 65)
    summed = hold_case(dev, c)
    tot = tot_f32(c)
    assert same_bits(Call(dev, c, tot=tot).results(), summed)
    hold_case(dev, c._replace(name=c.name + "-tot-one-ulp-up"), tot=np.nextafter(tot, F32(np.inf)))


@pytest.mark.parametrize("seed,at_nb", [(S.U1_SEED_AT_NB, True), (S.U1_SEED_BELOW_NB, False)], ids=["index-Nb", "index-Nb-1"])
def test_the_u1_sample(dev, seed, at_nb):
    """d z_samples is zero but for the u = 1 sample, whose index is Nb (the fp32 cdf ends at or below 1: below = above = Nb - 1, and
    all of g lands on the last bin) or Nb - 1 (it ends one ulp above 1: the pair (Nb - 2, Nb - 1) shares g by t = (1 - c0) / (c1 - c0),
    which is 1 in float64 and 2^-23 / denom short of it in fp32) - whichever the oracle's index says, against float64 with that
    index"""
    c = S.u1_case(seed)
    Nb = c.bins.shape[1]
    assert c.u[-1] == 1 and c.inds[0, -1] == (Nb if at_nb else Nb - 1)
    got = hold_case(dev, c)
    g = c.d_zs[0, -1]
    if at_nb:
        assert not got["d_bins"][0, :-1].any() and not got["d_weights"].any()
    else:
        assert not got["d_bins"][0, :-2].any()
    assert abs(got["d_bins"][0].astype(np.float64).sum() - g) <= 2.0 ** -22 * abs(g)          # d b0 + d b1 = g (1 - t) + g t


def test_rows_do_not_depend_on_the_batch(dev):
    c = S.sampler_case("spiky", 5, 63, 128)
    full = Call(dev, c).results()
    for rays in (1, 4):
        part = Call(dev, c, rays=rays).results()
        assert same_bits(part, {k: v[:rays] for k, v in full.items()}), rays


def test_two_runs_give_the_same_bits(dev):
    """no atomics: every lane owns its bins and walks the samples in order"""
    c = S.sampler_case("spiky", 5, 63, 128)
    a, b = Call(dev, c).results(), Call(dev, c).results()
    assert all(np.isfinite(v).all() for v in a.values()) and same_bits(a, b)


@pytest.mark.parametrize("name,over", [("Nb = 1", dict(Nb=1)), ("Nb = 1024", dict(Nb=1024)), ("Nf = 0", dict(Nf=0)), ("Nf = 1025", dict(Nf=1025)),
                                       ("NULL bins", dict(bins=None))])
def test_refusals_return_before_any_launch(dev, name, over):
    """snerf_sample_pdf_bins_bwd_f32 checks these before it sizes the launch, so nothing runs on the device"""
    call = Call(dev, S.sampler_case("flat", 5, 65, 65))
    assert call.run(**over) == E_BADARG, name
    assert call.lib.snerf_last_error_string()
    assert call.untouched(), f"{name}: the refused call wrote something"


@pytest.mark.parametrize("strict", [0, 1])
def test_the_autograd_wrapper_makes_this_call(dev, strict):
    """ops.sample_pdf under autograd with the case's u (two planted entries) in ops._U_CACHE: the forward kernel's indices are the
    oracle's, and d bins / d weights are the direct call's bit for bit - with `tot` absent, or in strict mode the sums of
    ops.reference_normalising_sum in the forward and in the backward"""
    from smpl_nerf_amd import ops
    c = S.sampler_case("spiky", 5, 63, 128)
    Nb, Nf = c.bins.shape[1], len(c.u)
    tot, inds = None, c.inds
    if strict:
        tot = ops.reference_normalising_sum(T(c.weights, dev)).cpu().numpy()
        inds = O.sample_pdf_detail(c.bins, c.weights, Nf, u=c.u, tot=tot)["inds"]
    direct = Call(dev, c, tot=tot, inds=inds).results()
    key = (Nf, str(dev))
    before = ops._U_CACHE.get(key)
    ops._U_CACHE[key] = T(c.u, dev)
    try:
        bins, w = T(c.bins, dev).requires_grad_(True), T(c.weights, dev).requires_grad_(True)
        out = ops.sample_pdf(bins, w, O.Args(number_fine_samples=Nf, strict_cumsum=strict))
        np.testing.assert_array_equal(out.detach().cpu().numpy(), O.sample_pdf(c.bins, c.weights, Nf, u=c.u, tot=tot))
        out.backward(T(c.d_zs, dev))
        assert same_bits(dict(d_bins=bins.grad.cpu().numpy(), d_weights=w.grad.cpu().numpy()), direct)
    finally:
        if before is None:
            ops._U_CACHE.pop(key, None)
        else:
            ops._U_CACHE[key] = before
