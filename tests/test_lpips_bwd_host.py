"""LPIPS as a training loss, without a GPU: the host-side refusals and the workspace arithmetic of the backward's C entries
(csrc/lpips.hip); the float64 autograd restatement of tests/lpips_bwd_ref.py against the gradients the reference itself computed
(tests/golden/g28_lpips_grad.npz); and the backward written out by hand, as include/smplnerf.h states it, against that autograd."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_bwd_ref as BR
import lpips_ref as LR
from conftest import load_golden
from smpl_nerf_amd import _lib, build, lpips, ops
from test_lpips_host import _net

BAD, ALIGN = -1, -2      # SNERF_E_BADARG, SNERF_E_ALIGN


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return load_golden(BR.GOLDEN)


def test_symbols_are_exported_and_prototyped(lib):
    text = open(_lib.HERE + "/../include/smplnerf.h").read()
    for name, nargs in (("snerf_feature_distance_bwd_f32", 12), ("snerf_relu_pool_bwd_f32", 9), ("snerf_lpips_bwd_workspace_bytes", 4),
                        ("snerf_lpips_bwd_f32", 17)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name + "(" in text
    assert callable(ops.lpips_loss) and callable(ops.feature_distance_bwd) and callable(ops.relu_pool_bwd) and callable(lpips.VggLpips.loss)


# ---- refusals: before anything touches a device (there is none here; the non-null pointers are small numbers) ------------------------
def _dist(lib, fx=8, fy=8, N=1, C=4, h=5, w=7, wl=8, normalize=1, g=8, dfx=8, dfy=8):
    return lib.snerf_feature_distance_bwd_f32(fx, fy, N, C, h, w, wl, normalize, g, dfx, dfy, None)


def test_feature_distance_bwd_refusals(lib):
    err = lib.snerf_last_error_string
    assert _dist(lib, N=-1) == BAD and b"N = -1" in err()
    assert _dist(lib, C=0) == BAD and b"C = 0" in err()
    assert _dist(lib, h=0) == BAD and b"h = 0" in err()
    assert _dist(lib, w=0) == BAD and b"w = 0" in err()
    assert _dist(lib, N=65536) == BAD and b"65535" in err()
    assert _dist(lib, N=16, C=2 ** 16, h=64, w=32) == BAD and b"2^31" in err()
    assert _dist(lib, dfx=None, dfy=None) == BAD and b"both null" in err()
    for name in ("fx", "fy", "wl", "g"):
        assert _dist(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    assert _dist(lib, N=0, fx=None, fy=None, wl=None, g=None, dfx=None, dfy=None) == 0      # N = 0: whatever the pointers are
    assert _dist(lib, N=0, C=0) == BAD                                                      # a bad scalar whatever N is


def _relu(lib, y=8, dy_full=8, dy_pool=8, N=1, C=4, H=5, W=7, dz=8):
    return lib.snerf_relu_pool_bwd_f32(y, dy_full, dy_pool, N, C, H, W, dz, None)


def test_relu_pool_bwd_refusals(lib):
    err = lib.snerf_last_error_string
    assert _relu(lib, N=-1) == BAD and b"N = -1" in err()
    assert _relu(lib, C=0) == BAD and b"C = 0" in err()
    assert _relu(lib, H=0, dy_pool=None) == BAD and b"H = 0" in err()
    assert _relu(lib, W=0, dy_pool=None) == BAD and b"W = 0" in err()
    assert _relu(lib, H=1) == BAD and b"H = 1" in err() and b"dy_pool" in err()             # a pooled gradient needs a window
    assert _relu(lib, W=1) == BAD and b"W = 1" in err()
    assert _relu(lib, N=2 ** 20, C=2, H=32, W=32) == BAD and b"2^31" in err()
    assert _relu(lib, H=2 ** 31) == BAD and _relu(lib, N=2 ** 40) == BAD
    assert _relu(lib, dy_full=None, dy_pool=None) == BAD and b"both null" in err()
    for name in ("y", "dz"):
        assert _relu(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    assert _relu(lib, N=0, y=None, dy_full=None, dy_pool=None, dz=None) == 0
    assert _relu(lib, N=0, y=None, dy_full=None, dy_pool=None, dz=None, H=1, W=1) == 0
    assert _relu(lib, N=0, C=0) == BAD and _relu(lib, N=0, H=1) == BAD


def _bwd(lib, net, x=8, y=8, N=1, H=32, W=48, g=8, dx=8, dy=8, layers=8, ws=16, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.snerf_lpips_bwd_workspace_bytes(1, max(H, 16), max(W, 16), net.channels), 0)
    return lib.snerf_lpips_bwd_f32(net, x, y, N, H, W, 3 * H * W, H * W, W, 1, g, dx, dy, layers, ws, ws_bytes, None)


def test_lpips_bwd_refusals_mirror_the_forward(lib):
    err = lib.snerf_last_error_string
    assert lib.snerf_lpips_bwd_f32(None, 8, 8, 1, 32, 32, 3072, 1024, 32, 1, 8, 8, 8, 8, 16, 1 << 30, None) == BAD and b"null net" in err()
    assert _bwd(lib, _net(channels=(64, 128, 256, 512, 513))) == BAD and b"channels[4] = 513" in err() and b"lpips_bwd" in err()
    assert _bwd(lib, _net(channels=(0, 128, 256, 512, 512))) == BAD and b"channels[0] = 0" in err()
    assert _bwd(lib, _net(std=(0.229, 0.0, 0.225))) == BAD and b"std[1]" in err()
    assert _bwd(lib, _net(std=(float("nan"), 0.224, 0.225))) == BAD and b"std[0]" in err()
    assert _bwd(lib, _net(mean=(0.485, float("inf"), 0.406))) == BAD and b"mean[1]" in err()
    assert _bwd(lib, _net(), H=15) == BAD and b"H = 15" in err()
    assert _bwd(lib, _net(), W=15) == BAD and b"W = 15" in err()
    assert _bwd(lib, _net(), N=-1) == BAD and b"N = -1" in err()
    assert _bwd(lib, _net(), dx=None, dy=None) == BAD and b"both null" in err()
    for name in ("x", "y", "g"):
        assert _bwd(lib, _net(), **{name: None}) == BAD and f"({name}".encode() in err(), name
    for name in ("weight0", "bias0", "weight12", "bias7", "lin0", "lin4"):
        assert _bwd(lib, _net(**{name: True})) == BAD and b"null pointer" in err(), name
    need = lib.snerf_lpips_bwd_workspace_bytes(1, 32, 48, _net().channels)
    assert _bwd(lib, _net(), ws=None) == BAD and b"workspace" in err()
    assert _bwd(lib, _net(), ws_bytes=need - 1) == BAD and b"workspace" in err() and str(need).encode() in err()
    assert _bwd(lib, _net(), ws=8) == ALIGN and b"16-byte aligned" in err()
    assert _bwd(lib, _net(weight3=True), N=0, x=None, y=None, g=None, dx=None, dy=None, layers=None, ws=None, ws_bytes=0) == 0
    assert _bwd(lib, _net(std=(0., 1., 1.)), N=0) == BAD and _bwd(lib, _net(), N=0, H=8) == BAD


def test_lpips_bwd_workspace_arithmetic(lib):
    q = lib.snerf_lpips_bwd_workspace_bytes
    ch = (ctypes.c_int32 * 5)(*LR.FULL)
    H, W = 128, 128
    # once a call: w' of the widest convolution and 512 zeros.  Per pair: the thirteen maps of both frames (2 x (2 x 64 + 2 x 128 / 4 +
    # 3 x 256 / 16 + 3 x 512 / 64 + 3 x 512 / 256) = 540 H W floats), two gradient buffers of the widest map, a float64 per tile
    fixed, one = q(0, H, W, ch), q(1, H, W, ch)
    assert fixed == 4 * (512 * 512 * 9 + 512) and one - fixed == 4 * (540 * H * W + 2 * 128 * H * W) + 8 * (H * W // 64)
    assert q(100, H, W, ch) == fixed + 100 * (one - fixed) and one % 16 == 0
    # a narrow stack on odd extents: the gradient to the input (6 H W) is the widest map
    narrow = (ctypes.c_int32 * 5)(1, 3, 2, 2, 2)
    H, W = 17, 35
    K = 2 * (2 * 1 * 17 * 35 + 2 * 3 * 8 * 17 + 3 * 2 * 4 * 8 + 3 * 2 * 2 * 4 + 3 * 2 * 1 * 2)
    assert q(0, H, W, narrow) == (4 * (3 * 3 * 9 + 512) + 15) // 16 * 16      # (stage 2's second convolution, 3 -> 3, is the widest)
    assert q(1, H, W, narrow) - q(0, H, W, narrow) == (4 * (K + 2 * 6 * H * W) + 8 * ((H * W + 63) // 64) + 15) // 16 * 16
    assert q(-1, 32, 32, ch) == -1 and q(1, 15, 32, ch) == -1 and q(1, 32, 15, ch) == -1 and q(1, 32, 32, None) == -1
    assert q(1, 32, 32, (ctypes.c_int32 * 5)(64, 128, 256, 513, 512)) == -1 and q(1, 2 ** 11, 2 ** 10, ch) == -1


# ---- the restatements ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(LR.CASES))
def test_float64_autograd_is_the_reference(golden, case):
    channels, H, W, N, wseed, iseed, same = LR.CASES[case]
    w = LR.weights(wseed, channels)
    assert LR.checksum(w) == float(golden[f"{case}/checksum"]), "the seeded weight recipe of lpips_ref.weights has drifted"
    g = BR.case_g(case)
    assert np.array_equal(g, golden[f"{case}/g_layers"]) and g.min() >= 0.5 and g.max() <= 1.5
    x, y = LR.images(iseed, N, H, W, same)
    layers, dx, dy = BR.metric_grad64(w, x, y, g)
    ex, ey = LR.E(dx, golden[f"{case}/dx"]), LR.E(dy, golden[f"{case}/dy"])
    print(f"{case}: E(autograd64 dx, reference f64) {ex:.3e}  dy {ey:.3e}")
    assert LR.E(layers, LR.metric64(w, x, y)) <= 1e-13 and ex <= 1e-12 and ey <= 1e-12
    if same:
        assert not dx.any() and not dy.any() and not golden[f"{case}/dx"].any()


def _all_cases():
    return [(name, c[:6]) for name, c in LR.CASES.items()] + [(name, c) for name, c in BR.SMALL.items()]


@pytest.mark.parametrize("name,case", _all_cases(), ids=[n for n, _ in _all_cases()])
def test_backward_by_hand_is_float64_autograd(name, case):
    """Every case, odd extents and frames with all-zero tap pixels included: there the rule's 0 and autograd's NaN both end at the
    ReLU's mask, and the end-to-end gradients are finite and equal."""
    channels, H, W, N, wseed, iseed = case
    w = LR.weights(wseed, channels)
    x, y = LR.images(iseed, N, H, W, name == "same")
    g = BR.case_g(name) if name in LR.CASES else BR.g_layers(wseed, N)
    _, dx, dy = BR.metric_grad64(w, x, y, g)
    hx, hy = BR.metric_backward(w, x, y, g)
    maps = []
    with torch.no_grad():
        BR._features(w, x, torch.float64, LR.MEAN, LR.STD, keep=maps)
    zero_pixels = int((maps[1].numpy().max(axis=1) == 0).sum())
    ex, ey = LR.E(hx, dx), LR.E(hy, dy)
    print(f"{name}: {zero_pixels} all-zero pixels at the first tap of x   E(by hand, autograd64) dx {ex:.3e} dy {ey:.3e}")
    assert np.isfinite(dx).all() and np.isfinite(dy).all() and np.isfinite(hx).all() and np.isfinite(hy).all()
    assert ex <= 1e-12 and ey <= 1e-12
    if name in ("odd", "narrow16"):
        assert zero_pixels > 0      # (the narrow stacks are the ones that hold such pixels)


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "plain"])
def test_distance_rule_is_autograd_away_from_zero_pixels_and_finite_at_them(normalize):
    rng = np.random.RandomState(11)
    fx, fy, wl, g = (np.abs(rng.standard_normal(s)).astype(np.float32) for s in ((2, 6, 5, 7), (2, 6, 5, 7), (6,), (2,)))
    fx[:, 1::2] *= rng.uniform(0, 1, fx[:, 1::2].shape) > 0.4
    ax, ay = BR.distance_grad64(fx, fy, wl, g, normalize)
    rx, ry = BR.distance_grad_rule(fx, fy, wl, g, normalize)
    assert LR.E(rx, ax) <= 1e-12 and LR.E(ry, ay) <= 1e-12
    # the fp32 steps of the rule stay within fp32 of the float64 ones
    sx, sy = BR.distance_grad_rule(fx, fy, wl, g, normalize, fwd=np.float32)
    assert 0 < LR.E(sx, ax) < 1e-5 and 0 < LR.E(sy, ay) < 1e-5
    # fx == fy: zeros
    assert not any(v.any() for v in BR.distance_grad_rule(fx, fx, wl, g, normalize))
    # a pixel whose features are all zero: autograd's 0 / 0, the rule's q / nx
    fx[0, :, 2, 3] = 0
    ax, _ = BR.distance_grad64(fx, fy, wl, g, normalize)
    rx, ry = BR.distance_grad_rule(fx, fy, wl, g, normalize)
    assert np.isfinite(rx).all() and np.isfinite(ry).all()
    if normalize:
        assert np.isnan(ax[0, :, 2, 3]).all()
        b = fy[0, :, 2, 3].astype(np.float64)
        b = b / (np.sqrt((b * b).sum()) + 1e-10)
        assert np.allclose(rx[0, :, 2, 3], 2 * wl * (0 - b) * (float(g[0]) / 35) / 1e-10, rtol=1e-12, atol=0)
    keep = np.ones(fx.shape, bool)
    keep[0, :, 2, 3] = False
    assert np.allclose(rx[keep], ax[keep], rtol=1e-10, atol=1e-18)


def test_relu_pool_bwd_restatement_is_autograd_and_ties_go_to_the_first():
    rng = np.random.RandomState(12)
    for H, W in ((4, 6), (5, 7), (1, 1), (2, 3)):
        # distinct values: autograd's route is unambiguous
        y = rng.permutation(2 * 3 * H * W).reshape(2, 3, H, W).astype(np.float64) - 10
        y = np.maximum(y, 0)
        dy_full, dy_pool = rng.standard_normal(y.shape), rng.standard_normal((2, 3, H // 2, W // 2))
        pre = torch.from_numpy(np.where(y > 0, y, -1.0)).requires_grad_(True)
        with torch.enable_grad():
            out = F.relu(pre)
            loss = (out * torch.from_numpy(dy_full)).sum()
            if min(H, W) >= 2:
                loss = loss + (F.max_pool2d(out, 2, 2) * torch.from_numpy(dy_pool)).sum()
            loss.backward()
        got = BR.relu_pool_bwd(y, dy_full, dy_pool if min(H, W) >= 2 else None)
        # (a window whose maximum is 0 holds four masked pixels: wherever autograd routes it, the mask returns 0)
        assert np.array_equal(got, pre.grad.numpy()), (H, W)
    y = np.array([[[[3., 3., 1.], [3., 3., 2.], [0., 5., 5.]]]])
    dz = BR.relu_pool_bwd(y, None, np.array([[[[7.]]]]))
    assert np.array_equal(dz, [[[[7., 0, 0], [0, 0, 0], [0, 0, 0]]]])      # the first of four equal maxima; the odd row and column: 0
    dz = BR.relu_pool_bwd(y, np.ones_like(y), np.array([[[[7.]]]]))
    assert np.array_equal(dz, [[[[8., 1, 1], [1, 1, 1], [0, 1, 1]]]])      # the ReLU's zero masks dy_full too


def test_yardstick_is_the_goldens_own(golden):
    yard = float(golden["yardstick_grad"])
    assert 1e-6 < yard < 1e-5      # an fp32 backward through thirteen convolutions: a few 1e-6
    for case in LR.CASES:
        assert golden[f"{case}/dx"].dtype == np.float64 and golden[f"{case}/dx"].shape == (LR.CASES[case][3], 3) + LR.CASES[case][1:3]


def test_cpu_tensors_are_refused_by_the_ops():
    w = LR.weights(7, (3, 5, 7, 9, 11))
    net = lpips.VggLpips.from_state(LR.features_state(w), w["lin"])
    x = torch.rand(1, 3, 16, 16)
    for call in (lambda: ops.lpips_loss(x.clone().requires_grad_(True), x, net), lambda: ops.lpips_loss(x, x, net),
                 lambda: net.loss(x.clone().requires_grad_(True), x),
                 lambda: ops.feature_distance_bwd(torch.rand(1, 4, 3, 3), torch.rand(1, 4, 3, 3), torch.ones(4), torch.ones(1)),
                 lambda: ops.relu_pool_bwd(torch.rand(1, 4, 4, 4), torch.rand(1, 4, 4, 4)),
                 lambda: ops.lpips_bwd(x, x, net, torch.ones(1, 5))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(KeyError):
        ops.lpips_loss(x, x, net, reduction='median')
