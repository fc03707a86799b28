"""composite_fwd_kernel (csrc/composite.hip) against float64, through the C entry snerf_composite_fwd_f32 as ops._composite_launch,
the single-call render and the one-call training step reach it.

The reference is tests/torch_ref.raw2outputs in float64, the yardstick the same in fp32, and each of rgb, weights and alpha is held
per ray to E(kernel) <= max(8 E(fp32 CPU), 2^-21): the rule, the inputs and the premises of tests/scan_bwd_ref.py, with the cases of
tests/fwd_ops_ref.py, all of which tests/test_fwd_ops_host.py checks on the CPU - among them that a restatement of this kernel with
exp taken in float64 and rounded once passes the rule on every case (worst row at 0.50 of its bound) while one with an fp32 exp
misses it seven times.  Every figure is printed before the assert (pytest -s; profiles/fwd_ops_errors.txt holds a run).  rgb,
weights and alpha are NaN-filled and sit between canaries in the test's own buffers (Guarded of tests/test_gpu_composite_bwd.py):
every element must be written and no canary touched.

The shapes: N = 1 (utils.py:168-169), 2, 3, both sides of the 64-sample chunk and of two chunks, 257, 4096, 4097 (the last chunk is
one sample behind 64 carried chunks) and 8192 (twice what the backward accepts), with five rays - one more than a workgroup's four -
both forms of the directions and both backgrounds.

Measured on an MI355X (profiles/fwd_ops_errors.txt has every figure), worst row of each call of the rule: rgb E kernel
1.8e-8 .. 6.6e-7 against 1.7e-8 .. 5.5e-7 for the fp32 CPU restatement, a ratio of 0.60 .. 8.65; weights 0 .. 3.0e-6 against
0 .. 3.0e-6, up to 2.78; alpha 0 .. 1.9e-6 against 0 .. 2.0e-6, up to 1.52.  The one ratio above 8 (rgb of saturated N = 257 per-ray
on black) is a row 1.6e-7 off, inside the floor, where the restatement happens to be within 1.8e-8.

What the sweep found before the kernel was changed: 13 cases missed the rule, all of them at N >= 4096.  The weights were
1.2e-5 .. 1.3e-5 off at N = 4096 and 4097 and 1.9e-5 .. 2.8e-5 at N = 8192 where the fp32 CPU restatement is 6e-7 .. 1.7e-6 off
(ratios up to 45), and rgb of planted N = 4096 per-sample on white 6.3e-7 against 7.6e-8: the drift tests/test_gpu_composite_bwd.py
records for the backward.  expf's error on the device has a non-zero mean, 1 - alpha carries it into the transmittance once per live
sample, and the error of a late weight grows with N.  The forward now takes the alpha's exp in double and rounds it once, as the
backward does; everything else is fp32 in the reference's order (profiles/fwd_ops_timing.txt: 9.2 -> 9.7 us and 18.9 -> 20.8 us at
16 384 rays of 64 and 192 samples, the 128 x 128 frame unchanged at 31.38 ms)."""
from functools import lru_cache
from itertools import combinations

import numpy as np
import pytest
import torch

import fwd_ops_ref as Fw
from oracle import nerf_oracle as O
from test_gpu_composite_bwd import E_ALIGN, E_BADARG, OK, Guarded, T

pytestmark = pytest.mark.gpu
NAMES = dict(rgb="rgb", w="weights", a="alpha")
SUBSETS = [s for n in (1, 2, 3) for s in combinations(Fw.OUTPUTS, n)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Call:
    """one forward call on the first `rays` rays of case `c`: device inputs, guarded outputs, the launch and the checked results"""

    def __init__(self, dev, c, wb, want=Fw.OUTPUTS, rays=None, noise="case", dirs="case"):
        from smpl_nerf_amd import _lib
        self.lib, self.c, self.wb = _lib.load(), c, wb
        self.B, self.N = (len(c.z) if rays is None else rays), c.z.shape[1]
        cut = lambda a: T(None if a is None else a[:self.B], dev)
        self.raw, self.z = cut(c.raw), cut(c.z)
        self.dirs = cut(c.dirs if isinstance(dirs, str) else dirs)
        self.noise = cut(c.noise if isinstance(noise, str) else noise)
        self.per_sample = int(self.dirs is not None and self.dirs.dim() == 3)
        shapes = dict(rgb=(self.B, 3), w=(self.B, self.N), a=(self.B, self.N))
        self.out = {k: Guarded(dev, shapes[k]) for k in want}

    def run(self, **over):
        from smpl_nerf_amd._lib import current_stream, ptr
        p = lambda k: ptr(self.out[k].t) if k in self.out else None
        a = dict(raw=ptr(self.raw), z=ptr(self.z), dirs=ptr(self.dirs), B=self.B, N=self.N)
        a.update(over)
        with torch.cuda.device(self.raw.device):
            rc = self.lib.snerf_composite_fwd_f32(a["raw"], a["z"], a["dirs"], self.per_sample, ptr(self.noise), a["B"], a["N"], self.wb,
                                                  p("rgb"), p("w"), p("a"), current_stream())
        torch.cuda.synchronize()
        return rc

    def results(self):
        assert self.run() == OK, self.lib.snerf_last_error_string()
        return {k: o.result(f"{self.c.name} {NAMES[k]}") for k, o in self.out.items()}

    def untouched(self):
        return all(o.untouched() for o in self.out.values())


@lru_cache(maxsize=None)
def run_case(dev, kind, N, per_sample, wb):
    """the three outputs of one case of the sweep, launched once and shared by the tests that read them"""
    c, _, _ = Fw.refs(kind, N, per_sample, wb)
    Fw.composite_premises(c)
    got = Call(dev, c, wb).results()
    for a in got.values():
        a.setflags(write=False)
    return got


def hold_case(dev, kind, N, per_sample, wb):
    c, r64, r32 = Fw.refs(kind, N, per_sample, wb)
    got = run_case(dev, kind, N, per_sample, wb)
    failed = []
    for k in Fw.OUTPUTS:                                  # all three figures are printed before any of them fails the test
        try:
            Fw.hold(f"{c.name}-wb{wb} {NAMES[k]}", got[k], r32[k], r64[k])
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    return got


# ---------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("kind,N,per_sample,wb", Fw.composite_sweep(), ids=lambda v: str(v))
def test_shape_sweep(dev, kind, N, per_sample, wb):
    hold_case(dev, kind, N, per_sample, wb)


# ---------------------------------------------------------------------------------------------- single cases
@pytest.mark.parametrize("kind", Fw.COMPOSITE_KINDS)
def test_one_sample_per_ray(dev, kind):
    """utils.py:168-169: rgb = sigmoid(raw.rgb), weights and alpha are ones; the directions are not read, so a null pointer is
    accepted and changes nothing"""
    for wb in (0, 1):
        got = hold_case(dev, kind, 1, 0, wb)
        assert (bits(got["w"]) == bits(np.float32(1))).all() and (bits(got["a"]) == bits(np.float32(1))).all()
        c, _, _ = Fw.refs(kind, 1, 0, wb)
        call = Call(dev, c, wb, dirs=None)
        assert call.dirs is None
        null = call.results()
        for k in Fw.OUTPUTS:
            assert np.array_equal(bits(null[k]), bits(got[k])), k


@pytest.mark.parametrize("kind,N,per_sample,wb", [a for a in Fw.composite_sweep() if a[1] in (2, 3, 64, 65, 129, 4097)], ids=lambda v: str(v))
def test_exact_facts(dev, kind, N, per_sample, wb):
    """what holds without a tolerance, whatever exp the kernel uses"""
    c, _, _ = Fw.refs(kind, N, per_sample, wb)
    got = run_case(dev, kind, N, per_sample, wb)
    arg, sig, dist = Fw.exp_argument(c)
    dead = (sig <= 0) | (dist == 0)                       # relu(sigma + noise) = 0, equal depths, a zero direction: exp(-0) = 1
    assert dead.any() or kind == "saturated"
    assert (bits(got["a"])[dead] == 0).all() and (bits(got["w"])[dead] == 0).all()
    nrm = np.sqrt((c.dirs.astype(np.float64) ** 2).sum(-1))
    if kind == "planted":
        assert dead[0, ::3].all() and dead[2].all() and dead[3, 0] and (dead[4, N // 2] if per_sample else dead[4].all())
        for ray in (2,) if per_sample else (2, 4):        # sigma = -1 throughout; a zero per-ray direction: the background alone
            assert (bits(got["rgb"][ray]) == bits(np.float32(wb))).all(), ray
    one = arg <= Fw.ALPHA_ONE_BELOW
    assert one.any() and (bits(got["a"])[one] == bits(np.float32(1))).all()
    last = (sig[:, -1] > 0) & ((nrm[:, -1] if per_sample else nrm) != 0)
    assert last.any() and (bits(got["a"][:, -1])[last] == bits(np.float32(1))).all()
    assert (got["a"] >= 0).all() and (got["a"] <= 1).all() and (got["w"] >= 0).all() and (got["w"] <= got["a"]).all()


@pytest.mark.parametrize("kind,N,per_sample", [("mild", 65, 1), ("saturated", 129, 0), ("planted", 1, 0)])
@pytest.mark.parametrize("want", SUBSETS, ids=lambda s: "+".join(s))
def test_output_subsets(dev, want, kind, N, per_sample):
    """each of the seven non-empty subsets of (rgb, weights, alpha), the others null, gives the bits of the three-output call (the
    one-call step passes weights = alpha = nullptr for its fine pass)"""
    c, _, _ = Fw.refs(kind, N, per_sample, 1)
    full = run_case(dev, kind, N, per_sample, 1)
    part = Call(dev, c, 1, want=want).results()
    assert tuple(part) == want
    for k in want:
        assert np.array_equal(bits(part[k]), bits(full[k])), k


@pytest.mark.parametrize("kind,N", [("mild", 65), ("planted", 129), ("saturated", 2)])
def test_per_ray_directions_are_the_repeated_per_sample_ones(dev, kind, N):
    c, _, _ = Fw.refs(kind, N, 0, 1)
    per_ray = run_case(dev, kind, N, 0, 1)
    call = Call(dev, c, 1, dirs=np.repeat(c.dirs[:, None, :], N, 1))
    assert call.per_sample == 1
    per_sample = call.results()
    for k in Fw.OUTPUTS:
        assert np.array_equal(bits(per_sample[k]), bits(per_ray[k])), k


@pytest.mark.parametrize("per_sample", [0, 1])
def test_null_noise_is_zero_noise(dev, per_sample):
    """saturated and planted cases carry no noise; sigma + 0 is sigma (a -0 becomes +0: equal values, and relu hides the sign)"""
    for kind in ("saturated", "planted"):
        c, _, _ = Fw.refs(kind, 65, per_sample, 0)
        assert c.noise is None
        zero = Call(dev, c, 0, noise=np.zeros(c.z.shape, np.float32)).results()
        null = run_case(dev, kind, 65, per_sample, 0)
        for k in Fw.OUTPUTS:
            assert np.array_equal(zero[k], null[k]), k


@pytest.mark.parametrize("kind,N,per_sample", [("saturated", 65, 0), ("mild", 129, 1), ("planted", 4097, 0)])
def test_rows_do_not_depend_on_the_batch(dev, kind, N, per_sample):
    """B = 1, 4, 5 (a partly filled workgroup, a full one, one ray into the next): the same rays give the same bits"""
    c, _, _ = Fw.refs(kind, N, per_sample, 1)
    full = run_case(dev, kind, N, per_sample, 1)
    for rays in (1, 4):
        part = Call(dev, c, 1, rays=rays).results()
        for k in Fw.OUTPUTS:
            assert np.array_equal(bits(part[k]), bits(full[k][:rays])), (rays, k)


def test_two_runs_give_the_same_bits(dev):
    for kind, N, ps in (("planted", 129, 0), ("mild", 4097, 1)):
        c, _, _ = Fw.refs(kind, N, ps, 0)
        a, b = run_case(dev, kind, N, ps, 0), Call(dev, c, 0).results()
        for k in Fw.OUTPUTS:
            assert np.isfinite(a[k]).all() and np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("name,N,over,code", [
    ("N = 0", 65, dict(N=0), E_BADARG),
    ("B < 0", 65, dict(B=-1), E_BADARG),
    ("null raw", 65, dict(raw=None), E_BADARG),
    ("null z", 65, dict(z=None), E_BADARG),
    ("null dirs at N = 2", 2, dict(dirs=None), E_BADARG),
    ("misaligned raw", 65, "misalign", E_ALIGN),
])
def test_refusals_return_before_any_launch(dev, name, N, over, code):
    c, _, _ = Fw.refs("mild", N, 0, 1)
    call = Call(dev, c, 1)
    if over == "misalign":
        over = dict(raw=call.raw.data_ptr() + 4)
    assert call.run(**over) == code, name
    assert call.lib.snerf_last_error_string()
    assert call.untouched(), f"{name}: the refused call wrote something"


def test_an_empty_batch_is_ok_and_writes_nothing(dev):
    c, _, _ = Fw.refs("mild", 65, 0, 1)
    call = Call(dev, c, 1)
    assert call.run(B=0) == OK and call.untouched()
    assert call.run(B=0, raw=None, z=None, dirs=None) == OK and call.untouched()


@pytest.mark.parametrize("kind,N,per_sample,wb", [("mild", 65, 0, 1), ("planted", 129, 1, 0), ("saturated", 1, 0, 1)])
def test_the_front_end_makes_this_call(dev, kind, N, per_sample, wb):
    """ops.composite and ops.raw2outputs under no_grad: the C entry's bits (per-ray directions also as the pipelines' expanded view)"""
    from smpl_nerf_amd import ops
    c, _, _ = Fw.refs(kind, N, per_sample, wb)
    direct = run_case(dev, kind, N, per_sample, wb)
    raw, z, dirs = T(c.raw, dev), T(c.z, dev), T(c.dirs, dev)
    forms = [dirs] if per_sample else [dirs, dirs[:, None, :].expand(len(c.z), N, 3)]
    with torch.no_grad():
        outs = [ops.composite(raw, z, d, bool(wb), noise=T(c.noise, dev)) for d in forms]
        if c.noise is None:
            outs += [ops.raw2outputs(raw, z, d, O.Args(white_background=wb)) for d in forms]
    for out in outs:
        for k, t in zip(Fw.OUTPUTS, out):
            assert tuple(t.shape) == direct[k].shape and np.array_equal(bits(t.cpu().numpy()), bits(direct[k])), k
