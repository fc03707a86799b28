"""LPIPS as a training loss on the GPU: the distance gradient, the ReLU / max-pool backward and the whole backward (csrc/lpips.hip)
through smpl_nerf_amd.ops, against tests/lpips_bwd_ref.py and the gradients the reference itself computed under autograd
(tests/golden/g28_lpips_grad.npz).

  exact      integer inputs: the ReLU / pool backward is a selection and one addition, so it must equal the restatement bit for bit.
  held       E = max|v - v64| / max|v64| <= smpl_estimator_ref.FACTOR (8) x E of the fp32 CPU autograd on the same inputs (DESIGN.md
             section 8g); for the golden cases the yardstick is the largest E of the reference's own fp32 gradients over all cases
             (stored in the file).  No pixel and no case is left out of a comparison.
  contract   the same bits whatever the workspace, the batch around a pair, the layout, a graph replay or a second call; the entry's
             gradients are the composition of its four entries.
Every figure is printed before it is asserted (pytest -s; profiles/lpips_bwd_errors.txt holds a run on an MI355X)."""
import functools

import numpy as np
import pytest
import torch

import lpips_bwd_ref as BR
import lpips_ref as LR
import smpl_estimator_ref as ER
from conftest import load_golden
from smpl_nerf_amd import _lib, lpips, ops
from smpl_nerf_amd.trainer import HipAdam

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


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a.contiguous()), bits(b.contiguous()))


def guarded(dev, shape):
    """A buffer of NaNs with GUARD floats on either side of the output it holds."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()) and not bool(torch.isnan(buf[GUARD:-GUARD]).any())


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the distance gradient -----------------------------------------------------------------------------------------------------------
DIST_C = [3, 64, 512]
DIST_MAPS = [(1, 1), (5, 7), (8, 8), (9, 13)]      # a lone pixel, part of a tile, one tile, a tile and its tail


@functools.lru_cache(maxsize=None)
def dist_inputs(C, h, w, N):
    """Post-ReLU-like features: |normal| with a third of the values zero, but no pixel that is zero in every channel (autograd, the
    yardstick here, gives NaN there: test_distance_grad_at_zero_pixels_and_on_equal_maps has those)."""
    rng = np.random.RandomState(3 * C + 17 * h + 257 * w + 4099 * N)
    def one():
        f = (np.abs(rng.standard_normal((N, C, h, w))) * (rng.uniform(0, 1, (N, C, h, w)) > 1 / 3)).astype(np.float32)
        f[:, 0][f.max(axis=1) == 0] = 1
        return f
    return one(), one(), np.abs(rng.standard_normal(C)).astype(np.float32), rng.uniform(0.5, 1.5, N).astype(np.float32)


def dist_entry(dev, fx, fy, wl, g, normalize, want_fx=True, want_fy=True):
    """The C entry on guarded outputs that start as NaNs."""
    N, C, h, w = fx.shape
    bx, dfx = guarded(dev, fx.shape) if want_fx else (None, None)
    by, dfy = guarded(dev, fx.shape) if want_fy else (None, None)
    rc = _lib.load().snerf_feature_distance_bwd_f32(fx.data_ptr(), fy.data_ptr(), N, C, h, w, wl.data_ptr(), int(normalize), g.data_ptr(),
                                                    dfx.data_ptr() if want_fx else None, dfy.data_ptr() if want_fy else None, stream())
    assert rc == 0, _lib.load().snerf_last_error_string()
    torch.cuda.synchronize()
    for b in (bx, by):
        assert b is None or guards_intact(b)
    return dfx, dfy


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "plain"])
@pytest.mark.parametrize("C", DIST_C)
def test_distance_grad_within_8x_the_fp32_cpu_error(dev, C, normalize):
    """E over all outputs of a family (one C, every map size and batch size, both gradients)."""
    got, v64, v32 = [], [], []
    for h, w in DIST_MAPS:
        for N in (1, 2, 3):
            fx, fy, wl, g = dist_inputs(C, h, w, N)
            t = up(dev, fx, fy, wl, g)
            dfx, dfy = dist_entry(dev, *t, normalize)
            # each output alone has the bits it has beside the other; the op is the entry
            ax, none = dist_entry(dev, *t, normalize, want_fy=False)
            none2, ay = dist_entry(dev, *t, normalize, want_fx=False)
            ox, oy = ops.feature_distance_bwd(*t, normalize=normalize)
            assert none is None and none2 is None and same_bits(ax, dfx) and same_bits(ay, dfy) and same_bits(ox, dfx) and same_bits(oy, dfy)
            got += [dfx.cpu().numpy().ravel(), dfy.cpu().numpy().ravel()]
            v64 += [a.ravel() for a in BR.distance_grad64(fx, fy, wl, g, normalize)]
            v32 += [a.ravel() for a in BR.distance_grad32(fx, fy, wl, g, normalize)]
    got, v64, v32 = (np.concatenate(a) for a in (got, v64, v32))
    e, e32 = LR.E(got, v64), LR.E(v32, v64)
    print(f"feature_distance_bwd C={C} normalize={int(normalize)}: E kernel {e:.3e}   E fp32 CPU autograd {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32):.3f}")
    assert np.isfinite(got).all() and np.isfinite(v64).all() and e32 > 0 and e <= ER.FACTOR * e32


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "plain"])
def test_distance_grad_at_zero_pixels_and_on_equal_maps(dev, normalize):
    for C in DIST_C:
        for h, w in DIST_MAPS:
            fx, fy, wl, g = dist_inputs(C, h, w, 3)
            fx, fy = fx.copy(), fy.copy()
            fx[:, :, 0, 0] = 0                      # a pixel whose features are all zero
            fy[1] = 0                               # an image that is entirely zero
            tx, ty, tw, tg = up(dev, fx, fy, wl, g)
            dfx, dfy = dist_entry(dev, tx, ty, tw, tg, normalize)
            assert bool(torch.isfinite(dfx).all()) and bool(torch.isfinite(dfy).all()), (C, h, w)
            # the stated rule, on the kernel's own fp32 s, r, nx, a, b, d: at a zero pixel the norm term is 0 and nothing cancels, so the
            # float64 expression rounded once is within an fp32 ulp or two of the restatement's
            rx, ry = BR.distance_grad_rule(fx, fy, wl, g, normalize, fwd=np.float32)
            zx, zy = np.zeros(fx.shape, bool), np.zeros(fx.shape, bool)
            zx[:, :, 0, 0], zy[1] = True, True
            np.testing.assert_allclose(dfx.cpu().numpy()[zx], rx[zx], rtol=1e-6, atol=0)
            np.testing.assert_allclose(dfy.cpu().numpy()[zy], ry[zy], rtol=1e-6, atol=0)
            # the other pixels (the zero pixels' gradients, 1e10 times theirs, would hide them in E): within fp32 of the rule - 1e-5
            # leaves room for an fp32 rounding of s that falls the other way under numpy's summation order, carried through the C terms
            for got, want, z in ((dfx, rx, zx), (dfy, ry, zy)):
                if not z.all():
                    assert LR.E(got.cpu().numpy()[~z], want[~z]) <= 1e-5, (C, h, w)
            sx, sy = dist_entry(dev, tx, tx.clone(), tw, tg, normalize)
            assert not bits(sx).any() and not bits(sy).any(), (C, h, w)      # fx == fy: +0.0 everywhere


# ---- the ReLU / max-pool backward ----------------------------------------------------------------------------------------------------
def relu_entry(dev, y, dy_full, dy_pool, alias=False):
    N, C, H, W = y.shape
    if alias:
        buf, dz = guarded(dev, y.shape)
        dz.copy_(dy_full)
        dy_full = dz
    else:
        buf, dz = guarded(dev, y.shape)
    rc = _lib.load().snerf_relu_pool_bwd_f32(y.data_ptr(), None if dy_full is None else dy_full.data_ptr(),
                                             None if dy_pool is None else dy_pool.data_ptr(), N, C, H, W, dz.data_ptr(), stream())
    assert rc == 0, _lib.load().snerf_last_error_string()
    torch.cuda.synchronize()
    assert guards_intact(buf)
    return dz


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 2, 2, 2), (2, 3, 5, 7), (1, 4, 16, 16), (1, 1, 33, 65), (2, 64, 9, 13)], ids=str)
def test_relu_pool_bwd_exact_on_integer_inputs(dev, shape):
    """y in 0 .. 3: windows full of equal positive values and of zeros; odd extents leave a row and a column outside every window."""
    N, C, H, W = shape
    rng = np.random.RandomState(H + 31 * W + 1009 * C)
    y = rng.randint(0, 4, shape).astype(np.float32)
    y[0, 0, :2, :2] = 2      # (a window of four equal positive values, whatever the seed)
    dy_full, dy_pool = rng.randint(-8, 9, shape).astype(np.float32), rng.randint(-8, 9, (N, C, H // 2, W // 2)).astype(np.float32)
    ty, tf, tp = up(dev, y, dy_full, dy_pool)
    want = BR.relu_pool_bwd(y, dy_full, None)
    assert np.array_equal(relu_entry(dev, ty, tf, None).cpu().numpy(), want)
    assert np.array_equal(relu_entry(dev, ty, tf, None, alias=True).cpu().numpy(), want)
    assert torch.equal(ops.relu_pool_bwd(ty, tf), torch.from_numpy(want).to(dev))
    if min(H, W) < 2:
        return
    both, pool = BR.relu_pool_bwd(y, dy_full, dy_pool), BR.relu_pool_bwd(y, None, dy_pool)
    assert np.array_equal(relu_entry(dev, ty, tf, tp).cpu().numpy(), both)
    assert np.array_equal(relu_entry(dev, ty, tf, tp, alias=True).cpu().numpy(), both)
    assert np.array_equal(relu_entry(dev, ty, None, tp).cpu().numpy(), pool)
    assert torch.equal(ops.relu_pool_bwd(ty, tf, tp), torch.from_numpy(both).to(dev))
    assert torch.equal(ops.relu_pool_bwd(ty, dy_pool=tp), torch.from_numpy(pool).to(dev))
    inplace = tf.clone()
    assert ops.relu_pool_bwd(ty, inplace, tp, inplace=True) is inplace and torch.equal(inplace, torch.from_numpy(both).to(dev))
    # the gradient of a window reaches exactly one pixel, unless its maximum is the ReLU's zero
    routed = torch.nn.functional.avg_pool2d(torch.from_numpy(pool), 2, 2) * 4
    assert torch.equal(routed, torch.from_numpy(np.where(torch.nn.functional.max_pool2d(torch.from_numpy(y), 2, 2).numpy() > 0, dy_pool, 0)))


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_on(dev, seed, channels):
    w = LR.weights(seed, channels)
    return w, lpips.VggLpips.from_state(LR.features_state(w), [torch.from_numpy(v) for v in w["lin"]]).to(dev)


@pytest.mark.parametrize("case", list(LR.CASES))
def test_gradients_against_the_reference(dev, case):
    g = load_golden(BR.GOLDEN)
    channels, H, W, N, wseed, iseed, same = LR.CASES[case]
    w, net = net_on(dev, wseed, channels)
    assert LR.checksum(w) == float(g[f"{case}/checksum"])
    x, y = LR.images(iseed, N, H, W, same)
    dx, dy, _ = ops.lpips_bwd(*up(dev, x, y), net, up(dev, g[f"{case}/g_layers"])[0])
    yard = float(g["yardstick_grad"])
    ex, ey = LR.E(dx.cpu().numpy(), g[f"{case}/dx"]), LR.E(dy.cpu().numpy(), g[f"{case}/dy"])
    print(f"lpips_bwd {case} {list(channels)} {N}x{H}x{W}: E kernel dx {ex:.3e} dy {ey:.3e}   yardstick {yard:.3e}   "
          f"kernel / bound {max(ex, ey) / (ER.FACTOR * yard):.3f}")
    if same:
        assert not bits(dx).any() and not bits(dy).any()
    assert dx.shape == (N, 3, H, W) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dy).all())
    assert ex <= ER.FACTOR * yard and ey <= ER.FACTOR * yard


@pytest.mark.parametrize("case", list(BR.SMALL))
def test_gradients_below_the_reference_limit(dev, case):
    """Frames the reference refuses (its pool5 raises below 32 pixels): the float64 autograd restatement is the truth, and its own fp32
    run on the case the yardstick."""
    channels, H, W, N, wseed, iseed = BR.SMALL[case]
    w, net = net_on(dev, wseed, channels)
    x, y = LR.images(iseed, N, H, W)
    gl = BR.g_layers(wseed, N)
    (_, x64, y64), (_, x32, y32) = BR.metric_grad64(w, x, y, gl), BR.metric_grad32(w, x, y, gl)
    dx, dy, _ = ops.lpips_bwd(*up(dev, x, y), net, up(dev, gl)[0])
    for name, got, v64, v32 in (("dx", dx, x64, x32), ("dy", dy, y64, y32)):
        e, e32 = LR.E(got.cpu().numpy(), v64), LR.E(v32, v64)
        print(f"lpips_bwd {case} {list(channels)} {N}x{H}x{W} {name}: E kernel {e:.3e}   E fp32 CPU autograd {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32):.3f}")
    assert np.isfinite(x64).all() and np.isfinite(y64).all() and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dy).all())
    for got, v64, v32 in ((dx, x64, x32), (dy, y64, y32)):
        assert LR.E(v32, v64) > 0 and LR.E(got.cpu().numpy(), v64) <= ER.FACTOR * LR.E(v32, v64)


# ---- the contract --------------------------------------------------------------------------------------------------------------------
def composed_backward(dev, w, x, y, gl):
    """The backward as ops.conv3x3_block_tap, ops.feature_distance_bwd and ops.relu_pool_bwd called one by one, between the CPU's
    (IEEE) standardisation and division by std."""
    v = LR.standardize(np.concatenate([x, y])).to(dev)
    N, maps, conv = x.shape[0], [], 0
    for l, n in enumerate(LR.STAGES):
        for j in range(n):
            a, b = up(dev, *w["conv"][conv])
            full, pool = ops.conv3x3_block_tap(v, a, torch.ones_like(b), b, relu=True, full=True, pool=j == n - 1 and l < 4)
            maps.append(full)
            v, conv = full, conv + 1
        v = pool
    pooled = None
    for l in range(4, -1, -1):
        tap = maps[conv - 1]
        u = torch.cat(ops.feature_distance_bwd(tap[:N], tap[N:], up(dev, w["lin"][l])[0], gl[:, l]))
        u = ops.relu_pool_bwd(tap, u, pooled, inplace=True)
        for j in range(LR.STAGES[l] - 1, -1, -1):
            conv -= 1
            flipped = up(dev, w["conv"][conv][0])[0].flip(2, 3).transpose(0, 1).contiguous()
            ci = flipped.shape[0]
            u, _ = ops.conv3x3_block_tap(u, flipped, torch.ones(ci, device=dev), torch.zeros(ci, device=dev), relu=False, full=True, pool=False)
            if j > 0:
                u = ops.relu_pool_bwd(maps[conv - 1], u)
        pooled = u
    d = torch.from_numpy(pooled.cpu().numpy() / np.asarray(LR.STD, np.float32).reshape(1, 3, 1, 1))
    return d[:N].to(dev), d[N:].to(dev)


@pytest.mark.parametrize("case", ["odd", "segmented"])
def test_entry_is_the_composition_of_its_entries(dev, case):
    channels, H, W, N, wseed, iseed = (LR.CASES[case][:6] if case in LR.CASES else BR.SMALL[case])
    w, net = net_on(dev, wseed, channels)
    x, y = LR.images(iseed, N, H, W)
    xt, yt, gl = up(dev, x, y, BR.g_layers(wseed, N))
    dx, dy, layers = ops.lpips_bwd(xt, yt, net, gl, want_layers=True)
    with torch.no_grad():
        cx, cy = composed_backward(dev, w, x, y, gl)
    assert same_bits(dx, cx) and same_bits(dy, cy)
    assert same_bits(layers, ops.lpips_layers(xt, yt, net)[0])      # the forward's, with its bits


def test_same_bits_whatever_the_workspace_batch_layout_and_call(dev):
    channels, H, W, N, wseed, iseed, _ = LR.CASES["odd"]
    _, net = net_on(dev, wseed, channels)
    xt, yt, gl = up(dev, *LR.images(iseed, N, H, W), BR.g_layers(wseed, N))
    dx, dy, layers = ops.lpips_bwd(xt, yt, net, gl, want_layers=True)
    fwd = ops.lpips_layers(xt, yt, net)[0]
    runs = {
        "a workspace of one pair": ops.lpips_bwd(xt, yt, net, gl, want_layers=True, max_pairs=1),
        "two pairs a chunk (2 + 1)": ops.lpips_bwd(xt, yt, net, gl, want_layers=True, max_pairs=2),
        "a second call": ops.lpips_bwd(xt, yt, net, gl, want_layers=True),
    }
    for name, (ax, ay, al) in runs.items():
        assert same_bits(ax, dx) and same_bits(ay, dy) and same_bits(al, layers) and same_bits(al, fwd), name
    # a pair alone
    ax, ay, al = ops.lpips_bwd(xt[1:2], yt[1:2], net, gl[1:2], want_layers=True)
    assert same_bits(ax, dx[1:2]) and same_bits(ay, dy[1:2]) and same_bits(al, layers[1:2])
    # channels-last frames: read and written through their strides, no copy
    xl, yl = (t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for t in (xt, yt))
    lx, ly, _ = ops.lpips_bwd(xl, yl, net, gl)
    assert lx.stride() == xl.stride() != xt.stride() and same_bits(lx, dx) and same_bits(ly, dy)
    # one output alone: that half of the batch only, the same bits
    ox, none, _ = ops.lpips_bwd(xt, yt, net, gl, want_y=False)
    none2, oy, _ = ops.lpips_bwd(xt, yt, net, gl, want_x=False, max_pairs=2)
    assert none is None and none2 is None and same_bits(ox, dx) and same_bits(oy, dy)


def test_graph_replay_has_the_same_bits(dev):
    channels, H, W, N, wseed, iseed, _ = LR.CASES["odd"]
    _, net = net_on(dev, wseed, channels)
    xt, yt, gl = up(dev, *LR.images(iseed, N, H, W), BR.g_layers(wseed, N))
    q = _lib.load().snerf_lpips_bwd_workspace_bytes
    ch = net.record(dev).channels
    ws = torch.empty((q(2, H, W, ch),), device=dev, dtype=torch.uint8)      # two pairs a chunk: N = 3 runs as 2 + 1
    ex, ey, el = ops.lpips_bwd(xt, yt, net, gl, want_layers=True, workspace=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dx, dy, layers = ops.lpips_bwd(xt, yt, net, gl, want_layers=True, workspace=ws)
    for t in (dx, dy, layers):
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(dx, ex) and same_bits(dy, ey) and same_bits(layers, el)


def test_loss_front_end(dev):
    channels, H, W, N, wseed, iseed, _ = LR.CASES["odd"]
    _, net = net_on(dev, wseed, channels)
    xt, yt = up(dev, *LR.images(iseed, N, H, W))
    ones = torch.ones((N, 5), device=dev)
    dx, dy, _ = ops.lpips_bwd(xt, yt, net, ones)
    for reduction, scale in (("none", 1.0), ("sum", 1.0), ("mean", 1.0 / N)):
        x, y = xt.clone().requires_grad_(True), yt.clone().requires_grad_(True)
        value, per = ops.lpips_loss(x, y, net, reduction=reduction, per_layer=True)
        want, want_per = ops.lpips(xt, yt, net, reduction=reduction, per_layer=True)
        assert value.requires_grad and same_bits(value, want) and same_bits(per, want_per)      # the value of ops.lpips, bit for bit
        value.sum().backward()
        gx, gy, _ = ops.lpips_bwd(xt, yt, net, ones * scale)
        assert same_bits(x.grad, gx) and same_bits(y.grad, gy)
    assert same_bits(ops.lpips_loss(xt.clone().requires_grad_(True), yt, net), ops.lpips(xt, yt, net))
    # per-layer gradients arrive too; one frame alone; the module form; channels-last
    x = xt.clone().requires_grad_(True)
    value, per = ops.lpips_loss(x, yt, net, reduction='none', per_layer=True)
    weights = torch.arange(1., 6., device=dev)
    (value.sum() + (per * weights).sum()).backward()
    assert same_bits(x.grad, ops.lpips_bwd(xt, yt, net, ones + weights, want_y=False)[0])
    y = yt.clone().requires_grad_(True)
    net.loss(xt, y, reduction='sum').backward()
    assert same_bits(y.grad, dy)
    xl = xt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    ops.lpips_loss(xl, yt, net, reduction='sum').backward()
    assert same_bits(xl.grad, dx)
    # no graph is asked for: ops.lpips; and once differentiable
    with torch.no_grad():
        assert not ops.lpips_loss(xt.clone().requires_grad_(True), yt, net).requires_grad
    assert not ops.lpips_loss(xt, yt, net).requires_grad and same_bits(ops.lpips_loss(xt, yt, net), ops.lpips(xt, yt, net))
    x = xt.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(ops.lpips_loss(x, yt, net), x, create_graph=True)
    assert not gx.requires_grad and gx.grad_fn is None      # no second derivative is recorded
    with pytest.raises(RuntimeError, match="16"):
        ops.lpips_loss(xt[:, :, :15].clone().requires_grad_(True), yt[:, :, :15], net)
    # the metric still refuses
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.lpips(xt.clone().requires_grad_(True), yt, net)


def test_adam_on_a_frame_lowers_the_loss(dev):
    _, net = net_on(dev, 2631, (3, 5, 7, 9, 11))
    x0, y0 = LR.images(2651, 1, 16, 16)
    flat_p, yt = torch.from_numpy(x0).to(dev).reshape(-1).clone(), torch.from_numpy(y0).to(dev)
    flat_g = torch.zeros_like(flat_p)
    x = flat_p.view(1, 3, 16, 16).requires_grad_(True)
    opt = HipAdam([x], flat_p, flat_g, [flat_g.view(1, 3, 16, 16)], lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = ops.lpips_loss(x, yt, net)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("lpips_loss under Adam, 16 x 16:", " ".join(f"{v:.5f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
