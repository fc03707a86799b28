"""The forms of snerf_linear_* (csrc/linear.hip) that layered.py uses or the header allows and test_linear_gemms_against_torch
(tests/test_gpu_round6.py) does not reach: every leading dimension wider than its matrix (a skip layer's column block has
ldw = w.stride(0)), accumulate = 1 in dgrad and wgrad, the k = 0 bias-only form, and the empty batch.

Two kinds of input, as in tests/test_gpu_contract.py: integers in -3 .. 3 (prior contents of an accumulated output in -5 .. 5), whose
sums stay below 2^24 (9 max(n, k, m) + 8 <= 36 881), so the result must equal float64 exactly in any order; and N(0, 1) inputs held to
the tolerance of test_linear_gemms_against_torch, 2e-6 sqrt(K + 1) (max|ref| + 1) for a reduction of length K.  The padding columns of
every input hold NaN (a read of one shows in the result), those of every output a canary that must survive; an output that is not
accumulated into starts as NaN."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CANARY = 12345.0
OK, E_BADARG = 0, -1
SHAPES = [(100, 130, 65), (513, 60, 70), (4097, 3, 5)]      # (n, k, m); the last has more than one wgrad slice
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def draw(rng, kind, shape, prior=False):
    if kind == "integer":
        return rng.integers(-5, 6, shape).astype(np.float32) if prior else rng.integers(-3, 4, shape).astype(np.float32)
    return rng.normal(size=shape).astype(np.float32)


class Padded:
    """a [rows, cols] matrix inside a [rows + 1, ld] buffer: `fill` in the padding columns and in the guard row after the last"""

    def __init__(self, dev, block, ld, fill):
        rows, cols = block.shape
        self.rows, self.cols, self.ld = rows, cols, ld
        self.before = np.full((rows + 1, ld), fill, np.float32)
        self.before[:rows, :cols] = block
        self.t = torch.from_numpy(self.before).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def block(self):
        """the matrix now, after checking that nothing around it changed"""
        now = self.t.cpu().numpy()
        outside = np.ones(now.shape, bool)
        outside[:self.rows, :self.cols] = False
        assert np.array_equal(now[outside], self.before[outside]), "a padding column or guard row was overwritten"
        return now[:self.rows, :self.cols]

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.before, equal_nan=True)


def hold(kind, got, ref, K, what):
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = float(np.abs(got.astype(np.float64) - ref).max())
    if kind == "integer":
        assert np.abs(ref).max() < 2 ** 24
        assert err == 0.0, f"{what}: max abs error {err} on integer inputs (exact in fp32)"
    else:
        tol = 2e-6 * np.sqrt(K + 1) * float(np.abs(ref).max() + 1)
        assert err <= tol, f"{what}: max abs error {err:.3e} > {tol:.3e}"


def wgrad_scratch(dev, lib, n, m, k):
    size = int(lib.snerf_linear_bwd_weight_scratch_floats(n, m, k))
    assert size >= m * k + m
    return Padded(dev, np.full((1, size), NAN, np.float32), size + 16, CANARY)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n,k,m", SHAPES)
@pytest.mark.parametrize("kind", ["integer", "real"])
def test_leading_dimensions_and_accumulate(dev, kind, n, k, m, accumulate):
    """ldx = k + 6, ldw = k + 7, ldy = m + 3, lddy = m + 5, lddx = k + 2, lddw = k + 9 in forward, dgrad, wgrad and the ReLU backward;
    with accumulate = 1, y, dx, dw and db add to their prior contents."""
    from smpl_nerf_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng([n, k, m, accumulate, kind == "real"])
    x, w, b, dy = draw(rng, kind, (n, k)), draw(rng, kind, (m, k)), draw(rng, kind, (m,)), draw(rng, kind, (n, m))
    if kind == "real":
        w = (w / np.sqrt(k)).astype(np.float32)
    x64, w64, b64, dy64 = (a.astype(np.float64) for a in (x, w, b, dy))
    X, W, DY = Padded(dev, x, k + 6, NAN), Padded(dev, w, k + 7, NAN), Padded(dev, dy, m + 5, NAN)
    B = torch.from_numpy(b).to(dev)

    def prior(shape):
        return draw(rng, kind, shape, prior=True) if accumulate else np.full(shape, NAN, np.float32)

    def base(p):
        return p.astype(np.float64) if accumulate else 0.0

    # forward: y (+)= x w^T + b, relu
    py = prior((n, m))
    Y = Padded(dev, py, m + 3, CANARY)
    assert lib.snerf_linear_fwd_f32(X.ptr, n, k, X.ld, W.ptr, W.ld, m, B.data_ptr(), accumulate, 1, Y.ptr, Y.ld, s) == OK
    y = Y.block()
    hold(kind, y, np.maximum(base(py) + x64 @ w64.T + b64, 0.0), k, "forward")
    # dgrad: dx (+)= dy w
    pdx = prior((n, k))
    DX = Padded(dev, pdx, k + 2, CANARY)
    assert lib.snerf_linear_bwd_input_f32(DY.ptr, n, m, DY.ld, W.ptr, W.ld, k, accumulate, DX.ptr, DX.ld, s) == OK
    hold(kind, DX.block(), base(pdx) + dy64 @ w64, m, "dgrad")
    # wgrad: dw (+)= dy^T x, db (+)= column sums of dy
    pdw, pdb = prior((m, k)), prior((1, m))
    DW, DB, S = Padded(dev, pdw, k + 9, CANARY), Padded(dev, pdb, m + 4, CANARY), wgrad_scratch(dev, lib, n, m, k)
    assert lib.snerf_linear_bwd_weight_f32(DY.ptr, n, m, DY.ld, X.ptr, X.ld, k, accumulate, DW.ptr, DW.ld, DB.ptr, S.ptr, s) == OK
    hold(kind, DW.block(), base(pdw) + dy64.T @ x64, n, "wgrad")
    hold(kind, DB.block(), base(pdb) + dy64.sum(0)[None], n, "bias gradient")
    S.block()
    # ReLU backward in place: lddy != ldy, the mask is the forward's output
    G = Padded(dev, dy, m + 5, CANARY)
    assert lib.snerf_relu_bwd_f32(G.ptr, Y.ptr, n, m, G.ld, Y.ld, s) == OK
    assert np.array_equal(G.block(), np.where(y > 0, dy, np.float32(0.0)))
    assert 0 < int((y > 0).sum()) < y.size
    assert X.unchanged() and W.unchanged() and DY.unchanged()


@pytest.mark.parametrize("kind", ["integer", "real"])
def test_bias_only_form(dev, kind):
    """k = 0 (layered.py: the bias alone wants its gradient): the forward gives y = act(bias), the wgrad with x = dw = NULL gives db
    only, and there is no dgrad."""
    from smpl_nerf_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    n, m = 513, 70
    rng = np.random.default_rng([n, m, kind == "real"])
    b, dy = draw(rng, kind, (m,)), draw(rng, kind, (n, m))
    B = torch.from_numpy(b).to(dev)
    none = torch.full((16,), NAN, device=dev)                  # x and w of a k = 0 forward: non-null, never read
    for relu in (0, 1):
        Y = Padded(dev, np.full((n, m), NAN, np.float32), m + 3, CANARY)
        assert lib.snerf_linear_fwd_f32(none.data_ptr(), n, 0, 0, none.data_ptr(), 0, m, B.data_ptr(), 0, relu, Y.ptr, Y.ld, s) == OK
        want = np.broadcast_to(np.maximum(b, 0) if relu else b, (n, m))
        assert np.array_equal(Y.block(), want)
    assert (b < 0).any() and (b > 0).any()
    Y = Padded(dev, np.full((n, m), NAN, np.float32), m + 3, CANARY)
    assert lib.snerf_linear_fwd_f32(none.data_ptr(), n, 0, 0, none.data_ptr(), 0, m, None, 0, 0, Y.ptr, Y.ld, s) == OK
    assert np.array_equal(Y.block(), np.zeros((n, m), np.float32))
    DY = Padded(dev, dy, m + 5, NAN)
    for accumulate in (0, 1):
        pdb = draw(rng, kind, (1, m), prior=True) if accumulate else np.full((1, m), NAN, np.float32)
        DB, S = Padded(dev, pdb, m + 4, CANARY), wgrad_scratch(dev, lib, n, m, 0)
        assert lib.snerf_linear_bwd_weight_f32(DY.ptr, n, m, DY.ld, None, 0, 0, accumulate, None, 0, DB.ptr, S.ptr, s) == OK
        hold(kind, DB.block(), (pdb.astype(np.float64) if accumulate else 0.0) + dy.astype(np.float64).sum(0)[None], n, "bias gradient alone")
        S.block()
    DX = Padded(dev, np.full((n, 1), NAN, np.float32), 4, CANARY)
    assert lib.snerf_linear_bwd_input_f32(DY.ptr, n, m, DY.ld, none.data_ptr(), 0, 0, 0, DX.ptr, DX.ld, s) == E_BADARG
    assert DX.unchanged()


@pytest.mark.parametrize("n,k,m", SHAPES[:2])
def test_empty_batch(dev, n, k, m):
    """n = 0: the wgrad zeroes exactly the m x k block of a padded dw (the 2-D memset honours lddw) and db, and leaves both alone
    when they accumulate; forward and dgrad return SNERF_OK and write nothing."""
    from smpl_nerf_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng([k, m])
    one = torch.full((1, max(k, m) + 16), NAN, device=dev)      # the operands of an empty batch: non-null, never read
    for accumulate in (0, 1):
        pdw, pdb = draw(rng, "integer", (m, k), prior=True) + 7, draw(rng, "integer", (1, m), prior=True) + 7       # (no zeros)
        DW, DB, S = Padded(dev, pdw, k + 9, CANARY), Padded(dev, pdb, m + 4, CANARY), wgrad_scratch(dev, lib, 0, m, k)
        assert lib.snerf_linear_bwd_weight_f32(one.data_ptr(), 0, m, m + 5, one.data_ptr(), k + 6, k, accumulate, DW.ptr, DW.ld, DB.ptr,
                                               S.ptr, s) == OK
        torch.cuda.synchronize()
        assert np.array_equal(DW.block(), pdw if accumulate else np.zeros_like(pdw))
        assert np.array_equal(DB.block(), pdb if accumulate else np.zeros_like(pdb))
        assert S.unchanged()
    W = Padded(dev, draw(rng, "integer", (m, k)), k + 7, NAN)
    Y, DX = Padded(dev, np.full((4, m), 3.0, np.float32), m + 3, CANARY), Padded(dev, np.full((4, k), 3.0, np.float32), k + 2, CANARY)
    assert lib.snerf_linear_fwd_f32(one.data_ptr(), 0, k, k + 6, W.ptr, W.ld, m, None, 0, 1, Y.ptr, Y.ld, s) == OK
    assert lib.snerf_linear_bwd_input_f32(one.data_ptr(), 0, m, m + 5, W.ptr, W.ld, k, 0, DX.ptr, DX.ld, s) == OK
    torch.cuda.synchronize()
    assert Y.unchanged() and DX.unchanged()
