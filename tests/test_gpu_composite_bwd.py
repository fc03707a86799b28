"""composite_bwd_kernel (csrc/composite.hip) against float64, through the C entries snerf_composite_bwd_all_f32 / snerf_composite_bwd_f32
as ops._CompositeFn calls them.

The reference is tests/scan_bwd_ref.composite in float64, the yardstick the same restatement in fp32, and every output (d raw, d z,
d dirs) is held per ray to E(kernel) <= max(8 E(fp32 CPU), 2^-21) - the rule of tests/scan_bwd_ref.py, whose cases and premises
tests/test_scan_bwd_host.py checks on the CPU.  Every figure is printed before the assert (pytest -s; profiles/scan_bwd_errors.txt
holds a run).  d raw, d z and d dirs are NaN-filled and sit between canaries in the test's own buffers: every element must be
written and no canary touched.

The shapes: N on both sides of the 64-sample chunk and of two chunks (63 .. 65, 128, 129: at 65 and 129 the last chunk is one sample
and the hand-off of d z across the chunk boundary has nothing beside it), 257, and 4096 (all 64 rows of s_carry), with five rays - one
more than a workgroup's four.

Measured on an MI355X (profiles/scan_bwd_errors.txt has every figure), worst row of each call of the rule: d raw E kernel
5.1e-8 .. 1.1e-6 against 3.4e-8 .. 1.1e-6 for the fp32 CPU restatement, a ratio of 0.87 .. 3.56; d z 3.2e-9 .. 4.8e-7 against
3.2e-9 .. 3.7e-7, 0.49 .. 19.56; d dirs 4.2e-8 .. 5.3e-6 against 1.4e-8 .. 9.2e-7, 0.79 .. 15.28.  The four ratios above 8 (d z of
mild N = 3 per-ray; d dirs of saturated N = 2 per-ray, planted N = 63 per-sample and planted N = 129 per-ray) are rows where the
kernel is 1.4e-7 .. 2.7e-7 off, inside the floor, and the restatement happens to be within 3e-8.  In the saturated N = 2
per-sample case the only live d z / d dirs row is 4e-102 in float64 and flushes to zero in the kernel and in the restatement alike
(E = 1 for both).

What the sweep found at N = 4096 before the kernel was changed: ratios of 8.5 .. 16.8 (d raw of mild per-ray, d dirs of mild
per-sample and of planted per-ray).  expf's error on the device has a mean of about a tenth of an ulp, 1 - alpha = exp(-sigma dist)
carries it into the transmittance once per live sample, and after 4096 samples T was 1.3e-5 off where unbiased rounding leaves 8e-7;
the backward now rounds a double exp once and keeps the 1e-10 of 1 - alpha + 1e-10 in double.  Its per-ray d dirs, a sum of terms
of both signs 10 to 1000 times larger than the sum, was accumulated in fp32 (4.85e-7 at N = 129 where the floor is 4.77e-7); it is
now accumulated in double like the kernel's other sums."""
import numpy as np
import pytest
import torch

import scan_bwd_ref as S

pytestmark = pytest.mark.gpu
CANARY = 12345.0
GUARD = 16                      # floats: 64 bytes, so that d raw stays 16-byte aligned behind its canaries
OK, E_BADARG, E_ALIGN = 0, -1, -2
ALL = ("d_rgb", "d_w", "d_a")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def T(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


class Guarded:
    """an output buffer of the test's own: NaN between two runs of canaries"""

    def __init__(self, dev, shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.all = torch.full((GUARD + self.n + GUARD,), CANARY, device=dev)
        self.t = self.all[GUARD:GUARD + self.n]
        self.t.fill_(float("nan"))

    def _split(self):
        a = self.all.cpu().numpy()
        return a[GUARD:GUARD + self.n].reshape(self.shape), np.concatenate([a[:GUARD], a[GUARD + self.n:]])

    def result(self, name):
        out, canaries = self._split()
        assert (canaries == CANARY).all(), f"{name}: a canary was overwritten"
        assert not np.isnan(out).any(), f"{name}: {int(np.isnan(out).sum())} of {out.size} elements were not written"
        return out

    def untouched(self):
        out, canaries = self._split()
        return bool((canaries == CANARY).all() and np.isnan(out).all())


class Call:
    """one backward call on the first `rays` rays of case `c`: device inputs, guarded outputs, the launch and the checked results"""

    def __init__(self, dev, c, wb, use=ALL, d_z=True, d_dirs=True, rays=None):
        from smpl_nerf_amd import _lib
        self.lib, self.c, self.wb = _lib.load(), c, wb
        self.B, self.N = (len(c.z) if rays is None else rays), c.z.shape[1]
        self.per_sample = int(c.dirs.ndim == 3)
        cut = lambda a: T(None if a is None else a[:self.B], dev)
        self.raw, self.z, self.dirs, self.noise = cut(c.raw), cut(c.z), cut(c.dirs), cut(c.noise)
        self.g = {k: cut(getattr(c, k)) if k in use else None for k in ALL}
        self.out = dict(d_raw=Guarded(dev, (self.B, self.N, 4)))
        if d_z:
            self.out["d_z"] = Guarded(dev, (self.B, self.N))
        if d_dirs:
            self.out["d_dirs"] = Guarded(dev, tuple(self.dirs.shape))

    def run(self, entry="all", **over):
        from smpl_nerf_amd._lib import current_stream, ptr
        p = lambda k: ptr(self.out[k].t) if k in self.out else None
        a = dict(raw=ptr(self.raw), N=self.N, B=self.B, d_dirs=p("d_dirs"))
        a.update(over)
        head = (a["raw"], ptr(self.z), ptr(self.dirs), self.per_sample, ptr(self.noise), a["B"], a["N"], self.wb, ptr(self.g["d_rgb"]))
        with torch.cuda.device(self.raw.device):
            if entry == "all":
                rc = self.lib.snerf_composite_bwd_all_f32(*head, ptr(self.g["d_w"]), ptr(self.g["d_a"]), p("d_raw"), a["d_dirs"], p("d_z"),
                                                          current_stream())
            else:
                rc = self.lib.snerf_composite_bwd_f32(*head, p("d_raw"), a["d_dirs"], current_stream())
        torch.cuda.synchronize()
        return rc

    def results(self, entry="all"):
        assert self.run(entry) == OK, self.lib.snerf_last_error_string()
        return {k: o.result(f"{self.c.name} {k}") for k, o in self.out.items()}

    def untouched(self):
        return all(o.untouched() for o in self.out.values())


def hold_case(dev, c, wb, **kw):
    S.composite_premises(c)
    got = Call(dev, c, wb, **kw).results()
    want = kw.get("use", ALL)
    r64, r32 = S.composite(c, wb, torch.float64, want), S.composite(c, wb, torch.float32, want)
    for k in got:
        S.hold(f"{c.name}-wb{wb} {k}", got[k], r32[k], r64[k])
    return got


# ---------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("kind,N,per_sample,wb", S.composite_sweep(), ids=lambda v: str(v))
def test_shape_sweep(dev, kind, N, per_sample, wb):
    hold_case(dev, S.composite_case(kind, S.COMPOSITE_B, N, per_sample), wb)


# ---------------------------------------------------------------------------------------------- single cases
def test_one_sample_per_ray(dev):
    """utils.py:168-169: rgb = sigmoid(raw.rgb), weights and alpha are constants, the directions and z are not read"""
    c = S.composite_case("mild", 5, 1, 0)
    got = hold_case(dev, c, 1)
    assert not got["d_raw"][..., 3].any() and not got["d_z"].any() and not got["d_dirs"].any()
    assert np.abs(got["d_raw"][..., :3]).min() > 0


@pytest.mark.parametrize("N", [65, 129])
@pytest.mark.parametrize("kw", [dict(use=("d_rgb",)), dict(use=("d_w",)), dict(use=("d_a",)), dict(d_z=False), dict(d_dirs=False)],
                         ids=["only-d_rgb", "only-d_w", "only-d_a", "no-d_z", "no-d_dirs"])
def test_one_gradient_absent_at_a_time(dev, N, kw):
    """a NULL d weights / d alpha / d rgb is a zero gradient; a NULL d z / d dirs is an output nobody wants (mild: sigma + noise in
    the backward; per-sample directions)"""
    c = S.composite_case("mild", 5, N, 1)
    got = hold_case(dev, c, 1, **kw)
    if kw.get("use") == ("d_rgb",):                  # the entry that takes d rgb alone is the same kernel: the same bits
        call = Call(dev, c, 1, use=("d_rgb",), d_z=False)
        alone = call.results("rgb")
        for k in alone:
            assert np.array_equal(alone[k].view(np.uint32), got[k].view(np.uint32)), k


@pytest.mark.parametrize("N", [65, 129])
def test_per_ray_directions_one_gradient_absent(dev, N):
    c = S.composite_case("mild", 5, N, 0)
    for kw in (dict(use=("d_w",)), dict(d_z=False), dict(d_dirs=False)):
        hold_case(dev, c, 1, **kw)


def test_rows_do_not_depend_on_the_batch(dev):
    """B = 1, 4, 5 (a partly filled workgroup, a full one, one ray into the next): the same rays give the same bits"""
    c = S.composite_case("saturated", 5, 65, 0)
    full = Call(dev, c, 1).results()
    for rays in (1, 4):
        part = Call(dev, c, 1, rays=rays).results()
        for k in full:
            assert np.array_equal(part[k].view(np.uint32), full[k][:rays].view(np.uint32)), (rays, k)


def test_two_runs_give_the_same_bits(dev):
    c = S.composite_case("planted", 5, 129, 0)
    a, b = Call(dev, c, 0).results(), Call(dev, c, 0).results()
    for k in a:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("name,entry,over,code", [
    ("N = 4097", "all", dict(N=4097), E_BADARG),
    ("N = 0", "all", dict(N=0), E_BADARG),
    ("misaligned raw", "all", "misalign", E_ALIGN),
    ("per-ray d_dirs through snerf_composite_bwd_f32", "rgb", dict(), E_BADARG),
])
def test_refusals_return_before_any_launch(dev, name, entry, over, code):
    """launch_composite_bwd checks these before the launch (and snerf_composite_bwd_f32 before it gets there), so nothing runs on
    the device and the buffers stay as they were"""
    c = S.composite_case("mild", 5, 65, 0)
    call = Call(dev, c, 1, d_z=(entry == "all"))
    if over == "misalign":
        over = dict(raw=call.raw.data_ptr() + 4)
    assert call.run(entry, **over) == code, name
    assert call.lib.snerf_last_error_string()
    assert call.untouched(), f"{name}: the refused call wrote something"


def test_the_autograd_wrapper_makes_this_call(dev):
    """ops.composite with per-ray directions that require grad: d raw, d z and d dirs are the direct call's, bit for bit"""
    from smpl_nerf_amd import ops
    c = S.composite_case("mild", 5, 65, 0)
    direct = Call(dev, c, 1).results()
    raw, z, dirs = (T(a, dev).requires_grad_(True) for a in (c.raw, c.z, c.dirs))
    rgb, w, a = ops.composite(raw, z, dirs, True, noise=T(c.noise, dev))
    torch.autograd.backward([rgb, w, a], [T(c.d_rgb, dev), T(c.d_w, dev), T(c.d_a, dev)])
    for k, leaf in (("d_raw", raw), ("d_z", z), ("d_dirs", dirs)):
        assert np.array_equal(leaf.grad.cpu().numpy().view(np.uint32), direct[k].view(np.uint32)), k
