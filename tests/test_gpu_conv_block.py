"""The fused conv-BN-ReLU-pool block on the GPU: csrc/conv_block.hip through ops.conv3x3_block and through the C entry on an output
buffer full of NaNs (every element of y is written, whatever SNERF_TEST_POISON_EMPTY is).

Yardstick: tests/smpl_estimator_ref.py - block64 (float64 CPU) and block32 (fp32 CPU, unfused) on the same fp32 inputs.
  exact cases   x integers in [-4, 4], weights integers in [-2, 2], scale one of 0.5, 1, 2, shift integer: every partial sum is an
                integer below 9 x 256 x 8 < 2^24, so fp32 is exact in ANY order - the kernel must equal block64 bit for bit.
  random cases  E = max|y - y64| / max|y64|; E(kernel) <= 8 E(block32) (DESIGN.md section 8g's rule).  Both are printed per case
                (pytest -s; profiles/conv_block_errors.txt holds a run on an MI355X).
Shapes [N, Ci, H, W, Co, pool]: all halo; one pool window; odd extents that floor; one channel chunk exactly; ragged in every
dimension without pooling; eight channel chunks and two channel tiles; several pixel tiles with the halo across their edges; the
estimator's first block; an empty batch."""
import functools

import numpy as np
import pytest
import torch

import smpl_estimator_ref as ER
from smpl_nerf_amd import _lib, ops

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1, 1, 1, 0), (1, 3, 2, 2, 16, 1), (2, 3, 5, 7, 16, 1), (1, 16, 8, 8, 32, 1), (3, 5, 17, 33, 17, 0), (1, 64, 16, 16, 128, 1),
          (2, 32, 64, 64, 64, 1), (1, 3, 128, 128, 16, 0), (0, 3, 8, 8, 16, 1)]
NO_RELU = {(2, 3, 5, 7, 16, 1), (3, 5, 17, 33, 17, 0)}
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def inputs(shape, kind, seed=1):
    N, Ci, H, W, Co, _ = shape
    rng = np.random.default_rng(seed + 1000 * sum(shape))
    f32 = np.float32
    if kind == "exact":
        return (rng.integers(-4, 5, (N, Ci, H, W)).astype(f32), rng.integers(-2, 3, (Co, Ci, 3, 3)).astype(f32),
                rng.choice(np.array([0.5, 1.0, 2.0], f32), Co), rng.integers(-3, 4, Co).astype(f32))
    return (rng.standard_normal((N, Ci, H, W)).astype(f32), (rng.standard_normal((Co, Ci, 3, 3)) / np.sqrt(9 * Ci)).astype(f32),
            rng.uniform(0.5, 1.5, Co).astype(f32), rng.uniform(-0.5, 0.5, Co).astype(f32))


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """block64 and block32 of a case, computed once and shared (read-only)."""
    relu, pool = shape not in NO_RELU, bool(shape[5])
    return ER.block64(*inputs(shape, kind), relu, pool), ER.block32(*inputs(shape, kind), relu, pool)


def on_gpu(dev, x, w, scale, shift, relu, pool):
    """The C entry on a y that starts as NaNs, and ops.conv3x3_block: the same bits."""
    xt, wt, st, ht = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, w, scale, shift))
    N, Ci, H, W = x.shape
    Co = w.shape[0]
    y = torch.full((N, Co, H // 2, W // 2) if pool else (N, Co, H, W), float("nan"), device=dev)
    rc = _lib.load().snerf_conv3x3_block_f32(xt.data_ptr(), N, Ci, H, W, wt.data_ptr(), st.data_ptr(), ht.data_ptr(), Co, int(relu), int(pool),
                                             y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().snerf_last_error_string()
    with torch.no_grad():
        y2 = ops.conv3x3_block(xt, wt, st, ht, relu=relu, pool=pool)
    assert y2.shape == y.shape and torch.equal(y, y2) and not bool(torch.isnan(y).any())
    return y.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_on_integer_inputs(dev, shape):
    relu, pool = shape not in NO_RELU, bool(shape[5])
    y64, y32 = reference(shape, "exact")
    got = on_gpu(dev, *inputs(shape, "exact"), relu, pool)
    assert got.shape == y64.shape and got.dtype == np.float32
    assert np.array_equal(y32.astype(np.float64), y64)      # (the premise: fp32 is exact here)
    np.testing.assert_array_equal(got.astype(np.float64), y64)
    if shape[0] and not relu:
        assert (y64 < 0).any()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_inputs_within_8x_the_fp32_cpu_error(dev, shape):
    relu, pool = shape not in NO_RELU, bool(shape[5])
    y64, y32 = reference(shape, "random")
    got = on_gpu(dev, *inputs(shape, "random"), relu, pool)
    e, e32 = ER.E(got, y64), ER.E(y32, y64)
    print(f"conv3x3_block {list(shape)} relu={int(relu)}: E kernel {e:.3e}   E fp32 CPU {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32) if e32 else 0.0:.3f}")
    assert e <= ER.FACTOR * e32, (shape, e, e32)


def test_an_image_does_not_depend_on_its_batch(dev):
    for shape in ((3, 5, 17, 33, 17, 0), (2, 32, 64, 64, 64, 1)):
        x, w, scale, shift = inputs(shape, "random")
        whole = on_gpu(dev, x, w, scale, shift, True, bool(shape[5]))
        for n in range(shape[0]):
            alone = on_gpu(dev, x[n:n + 1], w, scale, shift, True, bool(shape[5]))
            assert np.array_equal(alone[0], whole[n]), (shape, n)


@pytest.mark.parametrize("pool", [0, 1])
def test_a_map_does_not_depend_on_where_it_lies_in_a_larger_run(dev, pool):
    """A 12 x 22 map alone, and the same map inside a 64 x 70 one at (even) offsets that are no multiple of the 16-pixel tile, a ring
    of zeros around it (the small run's padding) and other content beyond: the same bits - the summation order of a pixel does not
    depend on the grid or on the pixel's place in a tile."""
    shape = (2, 11, 12, 22, 40, pool)
    x, w, scale, shift = inputs(shape, "random")
    small = on_gpu(dev, x, w, scale, shift, True, bool(pool))
    for oy, ox in ((6, 18), (26, 44), (50, 2)):
        big = np.random.default_rng(oy).standard_normal((2, 11, 64, 70)).astype(np.float32)
        big[:, :, oy - 1:oy + 13, ox - 1:ox + 23] = 0
        big[:, :, oy:oy + 12, ox:ox + 22] = x
        out = on_gpu(dev, big, w, scale, shift, True, bool(pool))
        cut = out[:, :, oy // 2:oy // 2 + 6, ox // 2:ox // 2 + 11] if pool else out[:, :, oy:oy + 12, ox:ox + 22]
        assert np.array_equal(cut, small), (oy, ox)


def test_layouts_grad_and_bad_shapes(dev):
    x, w, scale, shift = (torch.from_numpy(a).to(dev) for a in inputs((2, 3, 5, 7, 16, 1), "random"))
    with torch.no_grad():
        base = ops.conv3x3_block(x, w, scale, shift, pool=True)
        cl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # channels-last storage: made contiguous by the op
        assert not cl.is_contiguous() and torch.equal(ops.conv3x3_block(cl, w, scale, shift, pool=True), base)
        assert tuple(base.shape) == (2, 16, 2, 3)
    with pytest.raises(RuntimeError, match="training kernels"):
        ops.conv3x3_block(x, w.clone().requires_grad_(True), scale, shift)
    with torch.no_grad():      # (no graph is recorded here, so a parameter passes)
        assert torch.equal(ops.conv3x3_block(x, w.clone().requires_grad_(True), scale, shift, pool=True), base)
        with pytest.raises(RuntimeError):
            ops.conv3x3_block(x, w[:, :2], scale, shift)
        with pytest.raises(RuntimeError):
            ops.conv3x3_block(x, w, scale[:3], shift)
        with pytest.raises(RuntimeError, match="H = 1"):
            ops.conv3x3_block(x[:, :, :1], w, scale, shift, pool=True)
        with pytest.raises(RuntimeError, match="float32"):
            ops.conv3x3_block(x.double(), w, scale, shift)


def test_more_image_tiles_than_one_grid_dimension_holds(dev):
    """N = 2^24 + 3 images of one pixel: N tiles x 256 threads is past the 2^32 threads of a grid dimension, so the (image, tile) pairs
    spread over two dimensions.  Integer data, one product per output: exact against float64 in numpy."""
    N, Co = 2 ** 24 + 3, 2
    rng = np.random.default_rng(7)
    x = rng.integers(-4, 5, (N, 1, 1, 1)).astype(np.float32)
    w = rng.integers(-2, 3, (Co, 1, 3, 3)).astype(np.float32)
    w[:, 0, 1, 1] = (2, -1)                                          # the one weight an all-halo pixel meets
    scale, shift = np.array([0.5, 2.0], np.float32), np.array([1.0, -3.0], np.float32)
    xt, wt, st, ht = (torch.from_numpy(a).to(dev) for a in (x, w, scale, shift))
    with torch.no_grad():
        y = ops.conv3x3_block(xt, wt, st, ht, relu=False)
    want = x.reshape(N, 1).astype(np.float64) * w[:, 0, 1, 1].astype(np.float64)[None, :] * scale[None, :] + shift[None, :]
    got = y.cpu().numpy().reshape(N, Co)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.astype(np.float64), want)
