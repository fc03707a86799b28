"""LPIPS on the GPU: the convolution block with a tap (csrc/conv_block.hip), the tap distance and the whole metric (csrc/lpips.hip)
through smpl_nerf_amd.ops, against tests/lpips_ref.py and what the reference itself computed (tests/golden/g26_lpips.npz).

  exact      integer inputs and weights in -8 .. 8: every partial sum stays below 9 x 512 x 64 < 2^24, so fp32 is exact in any order
             and the kernel must equal the float64 block bit for bit.
  held       E = max|v - v64| / max|v64| <= smpl_estimator_ref.FACTOR (8) x E of the fp32 CPU restatement on the same inputs
             (DESIGN.md section 8g); for the golden cases the yardstick is the largest E of the reference's own fp32 outputs over all
             cases (stored in the file; a single case's value is too noisy).
Every figure is printed before it is asserted (pytest -s; profiles/lpips_errors.txt holds a run on an MI355X)."""
import functools

import numpy as np
import pytest
import torch

import lpips_ref as LR
import smpl_estimator_ref as ER
from conftest import load_golden
from smpl_nerf_amd import _lib, lpips, ops

pytestmark = pytest.mark.gpu
GUARD = 64      # floats of NaN on either side of an output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def up(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- the convolution with a tap ----------------------------------------------------------------------------------------------
TAP_CHANNELS = [(3, 64), (257, 300), (512, 512)]
TAP_MAPS = [(2, 2), (9, 13), (17, 16)]


@functools.lru_cache(maxsize=None)
def tap_inputs(Ci, Co, H, W, N, kind):
    rng = np.random.RandomState(Ci + 7 * Co + 31 * H + 101 * W + 1009 * N)
    f32 = np.float32
    if kind == "exact":
        return (rng.randint(-8, 9, (N, Ci, H, W)).astype(f32), rng.randint(-8, 9, (Co, Ci, 3, 3)).astype(f32),
                rng.choice(np.array([0.5, 1.0, 2.0], f32), Co), rng.randint(-3, 4, Co).astype(f32))
    return (rng.standard_normal((N, Ci, H, W)).astype(f32), (rng.standard_normal((Co, Ci, 3, 3)) * np.sqrt(2. / (9 * Ci))).astype(f32),
            rng.uniform(0.5, 1.5, Co).astype(f32), rng.uniform(-0.5, 0.5, Co).astype(f32))


def guarded(dev, shape):
    """A buffer of NaNs with GUARD floats on either side of the output it holds."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()) and not bool(torch.isnan(buf[GUARD:-GUARD]).any())


def tap_entry(dev, xt, wt, st, ht, relu, want_full, want_pool):
    """The C entry on guarded outputs that start as NaNs."""
    N, Ci, H, W = xt.shape
    Co = wt.shape[0]
    fb, full = guarded(dev, (N, Co, H, W)) if want_full else (None, None)
    pb, pool = guarded(dev, (N, Co, H // 2, W // 2)) if want_pool else (None, None)
    rc = _lib.load().snerf_conv3x3_block_tap_f32(xt.data_ptr(), N, Ci, H, W, wt.data_ptr(), st.data_ptr(), ht.data_ptr(), Co, int(relu),
                                                 full.data_ptr() if want_full else None, pool.data_ptr() if want_pool else None,
                                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().snerf_last_error_string()
    torch.cuda.synchronize()
    for b in (fb, pb):
        assert b is None or guards_intact(b)
    return full, pool


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", TAP_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cc", TAP_CHANNELS, ids=lambda s: f"{s[0]}-{s[1]}")
def test_tap_exact_on_integer_inputs(dev, cc, hw, N):
    x, w, scale, shift = tap_inputs(*cc, *hw, N, "exact")
    f64, p64 = LR.tap64(x, w, scale, shift)
    f32, _ = LR.tap32(x, w, scale, shift)
    assert np.array_equal(f32.astype(np.float64), f64)      # (the premise: fp32 is exact here)
    t = up(dev, x, w, scale, shift)
    full, pool = tap_entry(dev, *t, True, True, True)
    np.testing.assert_array_equal(full.cpu().numpy().astype(np.float64), f64)
    np.testing.assert_array_equal(pool.cpu().numpy().astype(np.float64), p64)
    assert torch.equal(pool, torch.nn.functional.max_pool2d(full, 2, 2))
    # each output alone: the same bits; and through the op
    alone_full, none = tap_entry(dev, *t, True, True, False)
    none2, alone_pool = tap_entry(dev, *t, True, False, True)
    assert none is None and none2 is None and torch.equal(alone_full, full) and torch.equal(alone_pool, pool)
    with torch.no_grad():
        of, op = ops.conv3x3_block_tap(*t)
    assert torch.equal(of, full) and torch.equal(op, pool)


@pytest.mark.parametrize("relu", [True, False])
def test_tap_has_the_bits_of_conv3x3_block(dev, relu):
    x, w, scale, shift = tap_inputs(64, 128, 17, 16, 3, "random")
    t = up(dev, x, w, scale, shift)
    with torch.no_grad():
        full, pool = ops.conv3x3_block_tap(*t, relu=relu)
        assert torch.equal(full, ops.conv3x3_block(*t, relu=relu, pool=False)) and torch.equal(pool, ops.conv3x3_block(*t, relu=relu, pool=True))
        only_full, none = ops.conv3x3_block_tap(*t, relu=relu, pool=False)
    assert none is None and torch.equal(only_full, full)
    assert (full < 0).any().item() != relu


def test_tap_random_inputs_at_512_within_8x_the_fp32_cpu_error(dev):
    x, w, scale, shift = tap_inputs(512, 512, 9, 13, 1, "random")
    (f64, p64), (f32, p32) = LR.tap64(x, w, scale, shift), LR.tap32(x, w, scale, shift)
    full, pool = tap_entry(dev, *up(dev, x, w, scale, shift), True, True, True)
    for name, got, y64, y32 in (("full", full, f64, f32), ("pool", pool, p64, p32)):
        e, e32 = LR.E(got.cpu().numpy(), y64), LR.E(y32, y64)
        print(f"conv3x3_block_tap [1,512,9,13]->512 {name}: E kernel {e:.3e}   E fp32 CPU {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32):.3f}")
    assert LR.E(full.cpu().numpy(), f64) <= ER.FACTOR * LR.E(f32, f64) and LR.E(pool.cpu().numpy(), p64) <= ER.FACTOR * LR.E(p32, p64)


def test_tap_refuses_tensors_that_require_grad(dev):
    x, w, scale, shift = up(dev, *tap_inputs(3, 64, 2, 2, 1, "random"))
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.conv3x3_block_tap(x, w.requires_grad_(True), scale, shift)
    with torch.no_grad():
        ops.conv3x3_block_tap(x, w, scale, shift)


# ---- the distance ------------------------------------------------------------------------------------------------------------------
DIST_C = [1, 3, 64, 512]
DIST_MAPS = [(1, 1), (2, 3), (9, 13), (33, 65)]      # the last: 34 tiles of partial sums an image


@functools.lru_cache(maxsize=None)
def dist_inputs(C, h, w, N):
    """Post-ReLU-like features: |normal| with a third of the values zero; fy differs from fx."""
    rng = np.random.RandomState(C + 17 * h + 257 * w + 4099 * N)
    def one():
        return (np.abs(rng.standard_normal((N, C, h, w))) * (rng.uniform(0, 1, (N, C, h, w)) > 1 / 3)).astype(np.float32)
    return one(), one(), np.abs(rng.standard_normal(C)).astype(np.float32)


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "plain"])
@pytest.mark.parametrize("C", DIST_C)
def test_distance_within_8x_the_fp32_cpu_error(dev, C, normalize):
    """E over all outputs of a family (one C, every map size and batch size): a single scalar's fp32 error is too noisy a yardstick."""
    got, v64, v32 = [], [], []
    for h, w in DIST_MAPS:
        for N in (1, 3):
            fx, fy, wl = dist_inputs(C, h, w, N)
            with torch.no_grad():
                out = ops.feature_distance(*up(dev, fx, fy, wl), normalize=normalize)
            assert out.shape == (N,) and out.dtype == torch.float32
            got.append(out.cpu().numpy()), v64.append(LR.distance64(fx, fy, wl, normalize)), v32.append(LR.distance32(fx, fy, wl, normalize))
    got, v64, v32 = (np.concatenate(a) for a in (got, v64, v32))
    e, e32 = LR.E(got, v64), LR.E(v32, v64)
    print(f"feature_distance C={C} normalize={int(normalize)}: E kernel {e:.3e}   E fp32 CPU {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32):.3f}")
    assert np.isfinite(got).all() and e32 > 0 and e <= ER.FACTOR * e32


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "plain"])
def test_distance_zero_on_equal_maps_and_zero_pixels(dev, normalize):
    for C in DIST_C:
        for h, w in DIST_MAPS:
            fx, fy, wl = dist_inputs(C, h, w, 3)
            fx, fy = fx.copy(), fy.copy()
            fx[:, :, 0, 0] = 0                      # a pixel whose features are all zero
            fy[1] = 0                               # an image that is entirely zero
            tx, ty, tw = up(dev, fx, fy, wl)
            with torch.no_grad():
                same = ops.feature_distance(tx, tx.clone(), tw, normalize=normalize)
                zero = ops.feature_distance(torch.zeros_like(tx), torch.zeros_like(tx), tw, normalize=normalize)
                out = ops.feature_distance(tx, ty, tw, normalize=normalize)
            assert not bits(same).any() and not bits(zero).any(), (C, h, w)      # +0.0 exactly
            assert bool(torch.isfinite(out).all()) and bool((out >= 0).all()), (C, h, w)


def test_distance_batch_independence_and_determinism(dev):
    for C, (h, w) in ((3, (9, 13)), (512, (9, 13)), (64, (33, 65))):
        fx, fy, wl = up(dev, *dist_inputs(C, h, w, 3))
        with torch.no_grad():
            a, b = ops.feature_distance(fx, fy, wl), ops.feature_distance(fx, fy, wl)
            alone = torch.cat([ops.feature_distance(fx[i:i + 1], fy[i:i + 1], wl) for i in range(3)])
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(alone))


# ---- the whole metric ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_on(dev, seed, channels):
    w = LR.weights(seed, channels)
    return w, lpips.VggLpips.from_state(LR.features_state(w), [torch.from_numpy(v) for v in w["lin"]]).to(dev)


def composed(dev, w, x, y):
    """The metric as ops.conv3x3_block_tap and ops.feature_distance called one by one, on the CPU's (IEEE) standardisation."""
    v = LR.standardize(np.concatenate([x, y])).to(dev)
    N, i, cols = x.shape[0], 0, []
    with torch.no_grad():
        for l, n in enumerate(LR.STAGES):
            for j in range(n):
                a, b = up(dev, *w["conv"][i])
                last = j == n - 1
                full, pool = ops.conv3x3_block_tap(v, a, torch.ones_like(b), b, relu=True, full=True, pool=last and l < 4)
                v, i = full, i + 1
            cols.append(ops.feature_distance(full[:N], full[N:], up(dev, w["lin"][l])[0]))
            v = pool
    return torch.stack(cols, dim=1)


def test_metric_is_the_composition_of_its_ops(dev):
    channels, H, W, N, wseed, iseed, _ = LR.CASES["odd"]
    w, net = net_on(dev, wseed, channels)
    x, y = LR.images(iseed, N, H, W)
    xt, yt = up(dev, x, y)
    layers, total = ops.lpips_layers(xt, yt, net)
    want = composed(dev, w, x, y)
    assert layers.shape == (N, 5) and np.array_equal(bits(layers), bits(want))
    asc = layers[:, 0]
    for l in range(1, 5):
        asc = asc + layers[:, l]
    assert np.array_equal(bits(total), bits(asc))
    # channels-last views, the workspace of one pair, a lone image: the same bits
    xl, yl = (t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for t in (xt, yt))
    assert xl.stride() != xt.stride()
    l2, t2 = ops.lpips_layers(xl, yl, net)
    l3, t3 = ops.lpips_layers(xt, yt, net, max_pairs=1)
    l4, t4 = ops.lpips_layers(xt[1:2], yt[1:2], net)
    l5, t5 = ops.lpips_layers(xt, yt, net)
    for a, b in ((l2, layers), (t2, total), (l3, layers), (t3, total), (l4, layers[1:2]), (t4, total[1:2]), (l5, layers), (t5, total)):
        assert np.array_equal(bits(a), bits(b))


def test_metric_graph_replay_has_the_same_bits(dev):
    channels, H, W, N, wseed, iseed, _ = LR.CASES["odd"]
    _, net = net_on(dev, wseed, channels)
    xt, yt = up(dev, *LR.images(iseed, N, H, W))
    one = _lib.load().snerf_lpips_workspace_bytes(1, H, W, net.record(dev).channels)
    ws = torch.empty((2 * one,), device=dev, dtype=torch.uint8)      # two pairs a chunk: N = 3 runs as 2 + 1
    eager, eager_total = ops.lpips_layers(xt, yt, net, workspace=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layers, total = ops.lpips_layers(xt, yt, net, workspace=ws)
    layers.fill_(float("nan")), total.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(layers), bits(eager)) and np.array_equal(bits(total), bits(eager_total))


@pytest.mark.parametrize("case", list(LR.CASES))
def test_metric_against_the_reference_outputs(dev, case):
    g = load_golden(LR.GOLDEN)
    channels, H, W, N, wseed, iseed, same = LR.CASES[case]
    w, net = net_on(dev, wseed, channels)
    assert LR.checksum(w) == float(g[f"{case}/checksum"])
    layers, total = ops.lpips_layers(*up(dev, g[f"{case}/x"], g[f"{case}/y"]), net)
    yard = float(g["yardstick"])
    e, e_ref = LR.E(layers.cpu().numpy(), g[f"{case}/f64/layers"]), LR.E(g[f"{case}/f32/layers"], g[f"{case}/f64/layers"])
    et = LR.E(total.cpu().numpy(), g[f"{case}/f64/total"])
    print(f"lpips {case} {list(channels)} {N}x{H}x{W}: E kernel layers {e:.3e} total {et:.3e}   E reference fp32 (this case) {e_ref:.3e}   "
          f"yardstick {yard:.3e}   kernel / bound {e / (ER.FACTOR * yard):.3f}")
    if same:
        assert not bits(layers).any() and not bits(total).any()
    assert e <= ER.FACTOR * yard


def test_metric_on_a_16x16_frame_at_full_width(dev):
    """The smallest frame (the fifth stage is one pixel): the reference itself raises here, so the float64 restatement stands in."""
    w, net = net_on(dev, 2620, LR.FULL)
    x, y = LR.images(2621, 2, 16, 16)
    v64, v32 = LR.metric64(w, x, y), LR.metric32(w, x, y)
    layers, _ = ops.lpips_layers(*up(dev, x, y), net)
    e, e32 = LR.E(layers.cpu().numpy(), v64), LR.E(v32, v64)
    print(f"lpips 16x16 full width: E kernel {e:.3e}   E fp32 CPU {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32):.3f}")
    assert e32 > 0 and e <= ER.FACTOR * e32


# ---- the front end -------------------------------------------------------------------------------------------------------------------
def test_front_end_reductions_scores_and_grad_refusal(dev):
    channels, H, W, N, wseed, iseed, _ = LR.CASES["odd"]
    _, net = net_on(dev, wseed, channels)
    xt, yt = up(dev, *LR.images(iseed, N, H, W))
    layers, total = ops.lpips_layers(xt, yt, net)
    none = ops.lpips(xt, yt, net, reduction='none')
    assert none.shape == (N,) and torch.equal(none, total)
    assert torch.equal(ops.lpips(xt, yt, net), total.mean(dim=0)) and torch.equal(ops.lpips(xt, yt, net, reduction='sum'), total.sum(dim=0))
    val, per = ops.lpips(xt, yt, net, reduction='mean', per_layer=True)
    assert torch.equal(val, total.mean(dim=0)) and per.shape == (5,) and torch.equal(per, layers.mean(dim=0))
    assert torch.equal(ops.lpips(xt, yt, net, reduction='none', per_layer=True)[1], layers)
    assert torch.equal(net(xt, yt), total.mean(dim=0))
    with pytest.raises(KeyError):
        ops.lpips(xt, yt, net, reduction='median')
    # image_scores: frames [N,H,W,3]; without `lpips` the keys are what they were
    r, t = xt.permute(0, 2, 3, 1).contiguous(), yt.permute(0, 2, 3, 1).contiguous()
    plain, scored = ops.image_scores(r, t), ops.image_scores(r, t, lpips=net)
    assert sorted(plain) == ["mse", "psnr", "ssim"] and sorted(scored) == ["lpips", "mse", "psnr", "ssim"]
    assert torch.equal(scored["lpips"], total.mean(dim=0)) and all(torch.equal(plain[k], scored[k]) for k in plain)
    assert torch.equal(ops.image_scores(xt, yt, channels_first=True, lpips=net)["lpips"], total.mean(dim=0))
    # forward only
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.lpips(xt.clone().requires_grad_(True), yt, net)
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.feature_distance(xt.clone().requires_grad_(True), yt, torch.ones(3, device=dev))
    with torch.no_grad():
        assert torch.equal(ops.lpips(xt.clone().requires_grad_(True), yt, net, reduction='none'), total)
    with pytest.raises(RuntimeError, match="16"):
        ops.lpips(xt[:, :, :15], yt[:, :, :15], net)
