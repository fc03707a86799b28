"""LPIPS without a GPU: the host-side refusals of the new C entries (csrc/conv_block.hip, csrc/lpips.hip) and their workspace
arithmetic; the seeded weight recipe and the float64 restatement of tests/lpips_ref.py against what the reference itself computed
(tests/golden/g26_lpips.npz); and the Python front end's loading (smpl_nerf_amd/lpips.py)."""
import ctypes

import numpy as np
import pytest
import torch

import lpips_ref as LR
from conftest import load_golden
from smpl_nerf_amd import _lib, build, lpips, ops

BAD, ALIGN = -1, -2      # SNERF_E_BADARG, SNERF_E_ALIGN


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return load_golden(LR.GOLDEN)


def test_symbols_are_exported_and_prototyped(lib):
    text = open(_lib.HERE + "/../include/smplnerf.h").read()
    for name, nargs in (("snerf_conv3x3_block_tap_f32", 13), ("snerf_feature_distance_workspace_bytes", 3), ("snerf_feature_distance_f32", 12),
                        ("snerf_lpips_workspace_bytes", 4), ("snerf_lpips_fwd_f32", 15)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name + "(" in text
    assert "typedef struct snerf_vgg_lpips {" in text
    # 13 x 2 pointers, 5 int32 padded to 8, 5 pointers, 6 floats
    assert ctypes.sizeof(_lib.VggLpipsNet) == 13 * 16 + 24 + 5 * 8 + 24


def _tap(lib, x=8, N=1, Ci=3, H=8, W=8, w=8, scale=8, shift=8, Co=16, relu=1, y_full=8, y_pool=8):
    return lib.snerf_conv3x3_block_tap_f32(x, N, Ci, H, W, w, scale, shift, Co, relu, y_full, y_pool, None)


def test_conv_tap_refusals(lib):
    """Before anything touches a device: there is none here.  (The non-null pointers are the number 8: nothing may read through them.)"""
    err = lib.snerf_last_error_string
    for bad in (0, 513, -1):
        assert _tap(lib, Ci=bad) == BAD and f"Ci = {bad}".encode() in err() and b"512" in err()
        assert _tap(lib, Co=bad) == BAD and f"Co = {bad}".encode() in err()
    assert _tap(lib, y_full=None, y_pool=None) == BAD and b"both null" in err()
    assert _tap(lib, y_full=None, y_pool=None, N=0) == 0                         # N = 0: whatever the pointers are
    assert _tap(lib, H=1) == BAD and b"H = 1" in err() and b"pool" in err()      # y_pool needs a window
    assert _tap(lib, W=1) == BAD and b"W = 1" in err()
    assert _tap(lib, H=0, y_pool=None) == BAD and _tap(lib, W=0, y_pool=None) == BAD and _tap(lib, N=-1) == BAD and b"N = -1" in err()
    for name in ("x", "w", "scale", "shift"):
        assert _tap(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    assert _tap(lib, N=2 ** 20, Ci=2, H=32, W=32) == BAD and b"2^31" in err()
    assert _tap(lib, H=2 ** 31) == BAD and _tap(lib, N=2 ** 40) == BAD
    assert _tap(lib, N=0, x=None, w=None, scale=None, shift=None, y_full=None) == 0
    assert _tap(lib, N=0, x=None, w=None, scale=None, shift=None, y_pool=None, H=1, W=1, Ci=512, Co=512) == 0
    assert _tap(lib, N=0, Ci=0) == BAD and _tap(lib, N=0, H=1) == BAD
    # the existing entry keeps its own limit and message
    assert lib.snerf_conv3x3_block_f32(8, 1, 257, 8, 8, 8, 8, 8, 16, 1, 0, 8, None) == BAD and b"Ci = 257 is outside 1 .. 256" in err()
    assert lib.snerf_conv3x3_block_f32(8, 1, 3, 8, 8, 8, 8, 8, 512, 1, 0, 8, None) == BAD and b"Co = 512 is outside 1 .. 256" in err()


def _dist(lib, fx=8, fy=8, N=1, C=4, h=5, w=7, wl=8, normalize=1, out=8, ws=8, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.snerf_feature_distance_workspace_bytes(max(N, 0), max(h, 1), max(w, 1)), 0)
    return lib.snerf_feature_distance_f32(fx, fy, N, C, h, w, wl, normalize, out, ws, ws_bytes, None)


def test_feature_distance_refusals_and_workspace(lib):
    err = lib.snerf_last_error_string
    q = lib.snerf_feature_distance_workspace_bytes
    assert q(1, 1, 1) == 8 and q(1, 8, 8) == 8 and q(1, 5, 13) == 16 and q(3, 33, 65) == 3 * 34 * 8 and q(0, 4, 4) == 0
    assert q(-1, 4, 4) == -1 and q(1, 0, 4) == -1 and q(1, 4, 0) == -1 and q(65536, 4, 4) == -1 and q(1, 2 ** 31, 1) == -1
    assert q(2, 2 ** 16, 2 ** 15) == -1                                                    # 2^31 pixels
    assert _dist(lib, N=-1) == BAD and b"N = -1" in err()
    assert _dist(lib, C=0) == BAD and b"C = 0" in err()
    assert _dist(lib, h=0) == BAD and b"h = 0" in err()
    assert _dist(lib, w=0) == BAD and b"w = 0" in err()
    assert _dist(lib, N=16, C=2 ** 16, h=64, w=32) == BAD and b"2^31" in err()
    for name in ("fx", "fy", "wl", "out"):
        assert _dist(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    assert _dist(lib, ws=None) == BAD and b"workspace" in err()
    assert _dist(lib, ws_bytes=7) == BAD and b"workspace" in err()
    assert _dist(lib, ws=4) == ALIGN and b"8-byte aligned" in err()
    assert _dist(lib, N=0, fx=None, fy=None, wl=None, out=None, ws=None, ws_bytes=0) == 0
    assert _dist(lib, N=0, C=0) == BAD                                                      # a bad scalar whatever N is


def _net(channels=LR.FULL, std=(0.229, 0.224, 0.225), mean=(0.485, 0.456, 0.406), **null):
    net = _lib.VggLpipsNet()
    for i in range(13):
        net.conv[i] = _lib.ConvWb(8, 8)
    for l in range(5):
        net.channels[l], net.lin[l] = channels[l], 8
    for c in range(3):
        net.mean[c], net.std[c] = mean[c], std[c]
    for name in null:
        kind, i = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
        if kind == "lin":
            net.lin[i] = None
        else:
            setattr(net.conv[i], kind, None)
    return net


def _fwd(lib, net, x=8, y=8, N=1, H=32, W=48, layers=8, total=8, ws=16, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.snerf_lpips_workspace_bytes(1, max(H, 16), max(W, 16), net.channels), 0)
    return lib.snerf_lpips_fwd_f32(net, x, y, N, H, W, 3 * H * W, H * W, W, 1, layers, total, ws, ws_bytes, None)


def test_lpips_workspace_arithmetic(lib):
    ch = (ctypes.c_int32 * 5)(*LR.FULL)
    q = lib.snerf_lpips_workspace_bytes
    # per pair: two buffers of the largest activation of the batch of 2 (stage 1: 2 x 64 x H x W), one of the largest pooled map or
    # the standardised input (2 x 64 x H/2 x W/2 > 6 H W), one float64 per 64-pixel tile of the first tap; a multiple of 16
    H, W = 128, 128
    F, P, tiles = 2 * 64 * H * W, 2 * 64 * (H // 2) * (W // 2), H * W // 64
    one = q(1, H, W, ch)
    assert one == 4 * (2 * F + P) + 8 * tiles and one % 16 == 0
    assert q(100, H, W, ch) == 100 * one and q(0, H, W, ch) == 0
    # a narrow stack on odd extents: stage 2 at 3 channels is larger than stage 1 at 1; the input (6 H W) is the largest of P
    narrow = (ctypes.c_int32 * 5)(1, 3, 2, 2, 2)
    H, W = 17, 35
    F = max(2 * 1 * H * W, 2 * 3 * (H // 2) * (W // 2))
    assert q(1, H, W, narrow) == (4 * (2 * F + 6 * H * W) + 8 * ((H * W + 63) // 64) + 15) // 16 * 16
    assert q(-1, 32, 32, ch) == -1 and q(1, 15, 32, ch) == -1 and q(1, 32, 15, ch) == -1 and q(1, 32, 32, None) == -1
    assert q(1, 32, 32, (ctypes.c_int32 * 5)(64, 128, 256, 513, 512)) == -1 and q(1, 32, 32, (ctypes.c_int32 * 5)(0, 1, 1, 1, 1)) == -1
    assert q(1, 2 ** 11, 2 ** 10, ch) == -1                                                # 2 x 512 x H W reaches 2^31


def test_lpips_refusals(lib):
    err = lib.snerf_last_error_string
    assert lib.snerf_lpips_fwd_f32(None, 8, 8, 1, 32, 32, 3072, 1024, 32, 1, 8, 8, 16, 1 << 30, None) == BAD and b"null net" in err()
    assert _fwd(lib, _net(channels=(64, 128, 256, 512, 513))) == BAD and b"channels[4] = 513" in err()
    assert _fwd(lib, _net(channels=(0, 128, 256, 512, 512))) == BAD and b"channels[0] = 0" in err()
    assert _fwd(lib, _net(std=(0.229, 0.0, 0.225))) == BAD and b"std[1]" in err()
    assert _fwd(lib, _net(std=(float("nan"), 0.224, 0.225))) == BAD and b"std[0]" in err()
    assert _fwd(lib, _net(std=(0.229, 0.224, float("inf")))) == BAD and b"std[2]" in err()
    assert _fwd(lib, _net(), H=15) == BAD and b"H = 15" in err()
    assert _fwd(lib, _net(), W=15) == BAD and b"W = 15" in err()
    assert _fwd(lib, _net(), N=-1) == BAD
    for name in ("x", "y", "layers"):
        assert _fwd(lib, _net(), **{name: None}) == BAD and f"({name})".encode() in err(), name
    for name in ("weight0", "bias0", "weight12", "bias7", "lin0", "lin4"):
        assert _fwd(lib, _net(**{name: True})) == BAD and b"null pointer" in err(), name
    need = lib.snerf_lpips_workspace_bytes(1, 32, 48, _net().channels)
    assert _fwd(lib, _net(), ws=None) == BAD and b"workspace" in err()
    assert _fwd(lib, _net(), ws_bytes=need - 1) == BAD and b"workspace" in err()
    assert _fwd(lib, _net(), ws=8) == ALIGN and b"16-byte aligned" in err()
    # N = 0 is a no-op whatever the pointers are; a bad scalar is an error whatever N is
    assert _fwd(lib, _net(weight3=True), N=0, x=None, y=None, layers=None, total=None, ws=None, ws_bytes=0) == 0
    assert _fwd(lib, _net(std=(0., 1., 1.)), N=0) == BAD and _fwd(lib, _net(), N=0, H=8) == BAD


@pytest.mark.parametrize("case", list(LR.CASES))
def test_weight_recipe_and_restatement_against_the_reference(golden, case):
    """The float64 restatement IS the reference (1e-12 relative, per layer), on weights whose checksum names a drift of the recipe."""
    channels, H, W, N, wseed, iseed, same = LR.CASES[case]
    w = LR.weights(wseed, channels)
    assert LR.checksum(w) == float(golden[f"{case}/checksum"]), "the seeded weight recipe of lpips_ref.weights has drifted"
    x, y = LR.images(iseed, N, H, W, same)
    assert np.array_equal(x, golden[f"{case}/x"]) and np.array_equal(y, golden[f"{case}/y"])
    got, want = LR.metric64(w, x, y), golden[f"{case}/f64/layers"]
    e, et = LR.E(got, want), LR.E(got.sum(1), golden[f"{case}/f64/total"])
    print(f"{case}: E(metric64 layers, reference f64) {e:.3e}  total {et:.3e}")
    assert got.shape == (N, 5) and e <= 1e-12 and et <= 1e-12
    if same:
        assert not got.any() and not LR.metric32(w, x, y).any()


def test_yardstick_is_the_goldens_own(golden):
    worst = max(LR.E(golden[f"{c}/f32/layers"], golden[f"{c}/f64/layers"]) for c in LR.CASES)
    assert worst == float(golden["yardstick"]) and 0 < worst < 1e-5


def test_distance_restatement_is_one_layer_of_the_metric():
    rng = np.random.RandomState(5)
    fx, fy, wl = (np.abs(rng.standard_normal(s)).astype(np.float32) for s in ((2, 6, 5, 7), (2, 6, 5, 7), (6,)))
    fx[0, :, 2, 3] = 0
    d = LR.distance64(fx, fy, wl)
    a, b = fx.astype(np.float64), fy.astype(np.float64)
    a, b = a / (np.sqrt((a * a).sum(1, keepdims=True)) + 1e-10), b / (np.sqrt((b * b).sum(1, keepdims=True)) + 1e-10)
    assert np.allclose(d, (((a - b) ** 2) * wl[None, :, None, None]).sum(1).mean((1, 2)), rtol=1e-13, atol=0)
    assert not LR.distance64(fx, fx, wl).any() and not LR.distance32(fx, fx, wl, normalize=False).any()


@pytest.mark.parametrize("keys", ["features", "bare"])
@pytest.mark.parametrize("lin_shape", ["flat", "nchw", "chw"])
def test_from_state_key_forms_and_lin_shapes(keys, lin_shape):
    w = LR.weights(7, (3, 5, 7, 9, 11))
    state = LR.features_state(w)
    if keys == "features":
        state = {"features." + k: v for k, v in state.items()}
        state["classifier.0.weight"], state["classifier.0.bias"] = torch.zeros(4, 4), torch.zeros(4)
    shape = {"flat": lambda c: (c,), "nchw": lambda c: (1, c, 1, 1), "chw": lambda c: (c, 1, 1)}[lin_shape]
    net = lpips.VggLpips.from_state(state, [torch.from_numpy(v).reshape(shape(v.size)) for v in w["lin"]])
    assert net.channels == (3, 5, 7, 9, 11) and net.mean == lpips.IMAGENET_MEAN == LR.MEAN and net.std == lpips.IMAGENET_STD == LR.STD
    for i, (a, b) in enumerate(w["conv"]):
        assert np.array_equal(getattr(net, f"conv{i}_weight").numpy(), a) and np.array_equal(getattr(net, f"conv{i}_bias").numpy(), b)
    for l, v in enumerate(w["lin"]):
        assert tuple(getattr(net, f"lin{l}").shape) == (v.size,) and np.array_equal(getattr(net, f"lin{l}").numpy(), v)
    assert not list(net.parameters())                       # buffers: nothing is trained
    rec = net.record(torch.device("cpu"))
    assert list(rec.channels) == [3, 5, 7, 9, 11] and rec.conv[12].weight == net.conv12_weight.data_ptr() and rec.lin[4] == net.lin4.data_ptr()
    assert [rec.mean[c] for c in range(3)] == [np.float32(v) for v in LR.MEAN]


def test_from_state_refuses_what_does_not_fit():
    w = LR.weights(7, (3, 5, 7, 9, 11))
    state = LR.features_state(w)
    with pytest.raises(KeyError, match="28.weight"):
        lpips.VggLpips.from_state({k: v for k, v in state.items() if not k.startswith("28.")}, w["lin"])
    with pytest.raises(ValueError, match=r"lin\[2\]"):
        lpips.VggLpips.from_state(state, [w["lin"][0], w["lin"][1], w["lin"][0], w["lin"][3], w["lin"][4]])
    with pytest.raises(ValueError, match="5 lin"):
        lpips.VggLpips.from_state(state, w["lin"][:4])


def test_from_files_round_trip_and_missing_path(tmp_path):
    w = LR.weights(9, (2, 3, 4, 5, 6))
    vgg, lin = str(tmp_path / "vgg16.pth"), str(tmp_path / "lpips_weights.pt")
    torch.save({"features." + k: v for k, v in LR.features_state(w).items()}, vgg)
    torch.save([torch.from_numpy(v).view(1, -1, 1, 1) for v in w["lin"]], lin)
    net = lpips.VggLpips.from_files(vgg, lin)
    assert net.channels == (2, 3, 4, 5, 6) and np.array_equal(net.lin3.numpy(), w["lin"][3])
    missing = str(tmp_path / "nowhere" / "vgg16.pth")
    with pytest.raises(FileNotFoundError, match="nowhere"):
        lpips.VggLpips.from_files(missing, lin)
    with pytest.raises(FileNotFoundError, match="no_lin.pt"):
        lpips.VggLpips.from_files(vgg, str(tmp_path / "no_lin.pt"))


def test_cpu_tensors_are_refused_by_the_ops():
    w = LR.weights(7, (3, 5, 7, 9, 11))
    net = lpips.VggLpips.from_state(LR.features_state(w), w["lin"])
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.lpips(x, x, net)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.feature_distance(torch.rand(1, 4, 3, 3), torch.rand(1, 4, 3, 3), torch.ones(4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.conv3x3_block_tap(x, torch.rand(4, 3, 3, 3), torch.ones(4), torch.ones(4))
