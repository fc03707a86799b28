"""posenc_kernel and posenc_bwd_kernel (csrc/posenc.hip) against float64, through the C entries snerf_posenc_f32 and
snerf_posenc_bwd_f32 as ops.PositionalEncoder calls them.

The reference is tests/torch_ref.posenc in float64 (autograd of sum(enc * d_out) for the backward), the yardstick the same in fp32,
and every point's row of the encoding and of d x is held to E(kernel) <= max(8 E(fp32 CPU), 2^-21), the rule of
tests/scan_bwd_ref.py.  The cases are those of tests/fwd_ops_ref.py, whose claims tests/test_fwd_ops_host.py checks on the CPU: the
reference's encoders around the 64-point tile, rows of 1, 1380 (a tile of 11 points) and 16384 floats (one point per workgroup),
L = 30 (arguments of 2e9 rad), both store paths and the hand-over between them, a misaligned output.  The outputs are NaN-filled and
sit between canaries in the test's own buffers (Guarded of tests/test_gpu_composite_bwd.py): every element must be written and no
canary touched.  Every figure is printed before the assert (pytest -s; profiles/fwd_ops_errors.txt holds a run).

Measured on an MI355X (profiles/fwd_ops_errors.txt has every figure), worst row of each call of the rule: the encoding E kernel
1.1e-8 .. 6.8e-8 against 8.2e-9 .. 3.6e-8 for the fp32 CPU restatement, a ratio of 1.10 .. 2.26 - at L = 30 as at L = 4: the device's
sincosf reduces an argument of 2e9 rad as well as one of 4; d x 4.7e-8 .. 5.0e-7 against 4.5e-9 .. 2.4e-7, 0.61 .. 25.8.  The five
ratios above 8 are rows 8.7e-8 .. 2.3e-7 off, inside the floor, where the restatement happens to be within 1e-8; the largest error
above the floor is 4.99e-7 (L = 4 with the identity, n = 63) against 8.4e-8.  The finite sines and cosines of the specials block
are within 4.1e-8 of float64 (fp32 CPU: 3.0e-8).  Nothing in either kernel had to change; the host checks of both entries did (a row
width formed in 32 bits before it was bounded, none at all in the backward), before the refusals below were first run."""
import numpy as np
import pytest
import torch

import fwd_ops_ref as Fw
from test_gpu_composite_bwd import CANARY, E_BADARG, GUARD, OK, Guarded, T

pytestmark = pytest.mark.gpu
UNWRITTEN = 54321.0                    # where NaN is a result (the specials): no sin, cos or coordinate of the block


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Shifted(Guarded):
    """Guarded with the output `lead` floats past its 64-byte aligned place, and a fill of the caller's choice"""

    def __init__(self, dev, shape, lead=0, fill=float("nan")):
        self.shape, self.n, self.lo, self.fill = shape, int(np.prod(shape)), GUARD + lead, fill
        self.all = torch.full((self.lo + self.n + GUARD,), CANARY, device=dev)
        self.t = self.all[self.lo:self.lo + self.n]
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 4 * lead % 16

    def _split(self):
        a = self.all.cpu().numpy()
        return a[self.lo:self.lo + self.n].reshape(self.shape), np.concatenate([a[:self.lo], a[self.lo + self.n:]])

    def result(self, name):
        if np.isnan(self.fill):
            return super().result(name)
        out, canaries = self._split()
        assert (canaries == CANARY).all(), f"{name}: a canary was overwritten"
        assert not (out == self.fill).any(), f"{name}: {int((out == self.fill).sum())} of {out.size} elements were not written"
        return out

    def untouched(self):
        out, canaries = self._split()
        return bool((canaries == CANARY).all() and (np.isnan(out).all() if np.isnan(self.fill) else (out == self.fill).all()))


class Call:
    """both entries on x [n, c]: device inputs, guarded outputs, the launches and the checked results"""

    def __init__(self, dev, x, L, identity, d_out=None, lead=0, fill=float("nan")):
        from smpl_nerf_amd import _lib
        self.lib, self.L, self.identity = _lib.load(), L, identity
        self.n, self.c = x.shape
        self.width = self.c * (identity + 2 * L)
        self.name = f"c{self.c}-L{L}-id{identity}-n{self.n}" + (f"-lead{lead}" if lead else "")
        self.x, self.d_out = T(x, dev), T(d_out, dev)
        self.enc = Shifted(dev, (self.n, self.width), lead, fill)
        self.d_x = Shifted(dev, (self.n, self.c))

    def run(self, bwd=False, **over):
        from smpl_nerf_amd._lib import current_stream, ptr
        a = dict(n=self.n, c=self.c, L=self.L, identity=self.identity)
        a.update(over)
        with torch.cuda.device(self.x.device):
            if bwd:
                rc = self.lib.snerf_posenc_bwd_f32(ptr(self.x), ptr(self.d_out), a["n"], a["c"], a["L"], a["identity"], ptr(self.d_x.t),
                                                   current_stream())
            else:
                rc = self.lib.snerf_posenc_f32(ptr(self.x), a["n"], a["c"], a["L"], a["identity"], ptr(self.enc.t), current_stream())
        torch.cuda.synchronize()
        return rc

    def forward(self):
        assert self.run() == OK, self.lib.snerf_last_error_string()
        return self.enc.result(self.name + " enc")

    def backward(self):
        assert self.run(bwd=True) == OK, self.lib.snerf_last_error_string()
        return self.d_x.result(self.name + " d_x")


def hold_forward(dev, c, L, identity, n, lead=0):
    x, _, e64, _, e32, _ = Fw.posenc_refs(c, L, identity, n)
    call = Call(dev, x, L, identity, lead=lead)
    got = call.forward()
    if identity:
        assert np.array_equal(bits(got[:, :c]), bits(x)), "the identity columns are not x"
    if L:
        Fw.hold(call.name + " enc", got, e32, e64)
    else:
        assert np.array_equal(bits(got), bits(x))
    return got


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("c,L,identity,n", Fw.POSENC_CASES, ids=lambda v: str(v))
def test_forward(dev, c, L, identity, n):
    hold_forward(dev, c, L, identity, n)


def test_forward_into_a_misaligned_output(dev):
    """out one float past a 16-byte boundary: every tile takes the scalar stores; the bits are those of the aligned call"""
    c, L, identity, n = Fw.POSENC_MISALIGNED
    assert np.array_equal(bits(hold_forward(dev, c, L, identity, n, lead=1)), bits(hold_forward(dev, c, L, identity, n)))


@pytest.mark.parametrize("identity", [0, 1])
def test_specials(dev, identity):
    """+0, -0, +inf, -inf, NaN and 3e38 (infinite from the second frequency): NaN exactly where the fp32 CPU restatement has NaN,
    sin(+-0 2^k) a zero of the same sign, cos of a zero exactly 1, the identity columns the coordinates' own bits, and the finite
    sines and cosines (of ordinary values and of 3e38) within 2^-21 of float64, the rule's floor for a row whose largest value is 1"""
    x, L = Fw.specials_block(), 4
    e32, _ = Fw.posenc_ref(x, L, identity, torch.float32)
    e64, _ = Fw.posenc_ref(x, L, identity, torch.float64)
    got = Call(dev, x, L, identity, fill=UNWRITTEN).forward()
    assert np.isnan(e32).any() and np.array_equal(np.isnan(got), np.isnan(e32))
    if identity:
        assert np.array_equal(bits(got[:, :3]), bits(x))
    fin = np.isfinite(e32) & (np.abs(e64) <= 1)
    err = np.abs(got[fin].astype(np.float64) - e64[fin])
    print(f"specials id{identity}: worst finite element {err.max():.3e} off float64 (fp32 CPU {np.abs(e32[fin] - e64[fin]).max():.3e})")
    assert fin.sum() >= 8 * 3 * 2 and (err <= Fw.FLOOR).all()
    blocks = got[:, 3 * identity:].reshape(len(x), L, 2, 3)
    zero = x == 0
    assert zero.sum() == 4 and np.signbit(x[zero]).sum() == 2
    for k in range(L):
        assert np.array_equal(bits(blocks[:, k, 0][zero]), bits(x[zero])), f"sin(+-0 x 2^{k}) is not the zero it was given"
        assert (bits(blocks[:, k, 1][zero]) == bits(np.float32(1))).all(), f"cos(+-0 x 2^{k}) is not 1"


# ---------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("c,L,identity,n", Fw.POSENC_BWD_CASES, ids=lambda v: str(v))
def test_backward(dev, c, L, identity, n):
    x, d_out, _, g64, _, g32 = Fw.posenc_refs(c, L, identity, n)
    call = Call(dev, x, L, identity, d_out)
    got = call.backward()
    if L:
        Fw.hold(call.name + " d_x", got, g32, g64)
    else:
        assert np.array_equal(bits(got), bits(d_out)), "with the identity alone d x is d out"


@pytest.mark.parametrize("c,L,identity,n,k", [(3, 10, 1, 65, 0), (3, 10, 1, 65, 9), (3, 4, 0, 130, 2), (69, 10, 0, 12, 7), (3, 30, 1, 65, 29)],
                         ids=lambda v: str(v))
def test_backward_of_a_single_block(dev, c, L, identity, n, k):
    """d out non-zero in the sin block of one frequency, then in its cos block: d x = 2^k d sin cos(2^k x), -2^k d cos sin(2^k x)"""
    x, d_out = Fw.posenc_inputs(c, L, identity, n)
    for cos in (0, 1):
        g = Fw.one_block(d_out, c, L, identity, k, cos)
        assert np.count_nonzero(g) == n * c
        _, g64 = Fw.posenc_ref(x, L, identity, torch.float64, g)
        _, g32 = Fw.posenc_ref(x, L, identity, torch.float32, g)
        call = Call(dev, x, L, identity, g)
        Fw.hold(f"{call.name} d_x from the {'cos' if cos else 'sin'} block of k = {k}", call.backward(), g32, g64)


# ---------------------------------------------------------------------------------------------- batch, determinism, autograd
@pytest.mark.parametrize("c,L,identity,n", [(3, 10, 1, 130), (69, 10, 0, 23), (2, 3, 1, 65)], ids=lambda v: str(v))
def test_rows_do_not_depend_on_the_batch_and_two_runs_give_the_same_bits(dev, c, L, identity, n):
    """the first point alone, the points short of the last tile and all of them: equal bits, forward and backward"""
    x, d_out = Fw.posenc_inputs(c, L, identity, n)
    full = Call(dev, x, L, identity, d_out)
    enc, d_x = full.forward(), full.backward()
    again = Call(dev, x, L, identity, d_out)
    assert np.array_equal(bits(again.forward()), bits(enc)) and np.array_equal(bits(again.backward()), bits(d_x))
    tile = Fw.posenc_tile(c, L, identity)
    for m in (1, tile - 1, tile + 1, (n - 1) // tile * tile):
        part = Call(dev, x[:m], L, identity, d_out[:m])
        assert np.array_equal(bits(part.forward()), bits(enc[:m])) and np.array_equal(bits(part.backward()), bits(d_x[:m])), m


@pytest.mark.parametrize("c,L,identity,n", [(3, 10, 0, 65), (3, 4, 1, 130), (1, 0, 1, 5)], ids=lambda v: str(v))
def test_the_autograd_wrapper_makes_these_calls(dev, c, L, identity, n):
    from smpl_nerf_amd.ops import PositionalEncoder
    x, d_out = Fw.posenc_inputs(c, L, identity, n)
    direct = Call(dev, x, L, identity, d_out)
    enc, d_x = direct.forward(), direct.backward()
    leaf = T(x, dev).requires_grad_(True)
    out = PositionalEncoder(L, bool(identity)).encode(leaf)
    assert out.requires_grad and np.array_equal(bits(out.detach().cpu().numpy()), bits(enc))
    out.backward(T(d_out, dev))
    assert np.array_equal(bits(leaf.grad.cpu().numpy()), bits(d_x))
    with torch.no_grad():
        assert np.array_equal(bits(PositionalEncoder(L, bool(identity)).encode(T(x, dev)).cpu().numpy()), bits(enc))


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name,over", [
    ("L = 31", dict(L=31)),
    ("L = -1", dict(L=-1)),
    ("c = 0", dict(c=0)),
    ("n < 0", dict(n=-1)),
    ("a row of 16385 floats", dict(c=16385, L=0, identity=1)),
    ("a row width that wraps to 4 in 32 bits", dict(c=70409300, L=30, identity=1)),
])
def test_refusals_return_before_any_launch(dev, name, over):
    """both entries check these before the launch, so nothing runs on the device and the buffers stay as they were"""
    x, d_out = Fw.posenc_inputs(3, 4, 1, 65)
    call = Call(dev, x, 4, 1, d_out)
    for bwd in (False, True):
        assert call.run(bwd=bwd, **over) == E_BADARG, (name, bwd)
        assert call.lib.snerf_last_error_string()
    assert call.enc.untouched() and call.d_x.untouched(), f"{name}: a refused call wrote something"


def test_no_points_is_ok_and_writes_nothing(dev):
    x, d_out = Fw.posenc_inputs(3, 4, 1, 65)
    call = Call(dev, x, 4, 1, d_out)
    assert call.run(n=0) == OK and call.run(bwd=True, n=0) == OK
    assert call.enc.untouched() and call.d_x.untouched()
