"""The image scores without a GPU: the restatement the GPU tests measure with (tests/ssim_ref.py) against what the reference itself
computed (tests/golden/g20_image_scores.npz), and the host-side argument checks of the three C entries (csrc/ssim.hip).

The restatement in float64 differs from the reference's float64 run in one thing: the reference computes its k x k window table in
fp32 (scores.py:79-86), the restatement takes win (x) win of the fp32 1-D window in float64 - a perturbation of a few 2^-24 per
weight.  It is held to the SAME floors the kernel is held to (ssim_ref: 16 u mean cond + 4 u per value, 16 u max Gamma per gradient),
so a restatement that stated another function would fail here before it misjudged a kernel.  Measured: values 2e-9 .. 5e-7 against
floors of 9e-6 .. 2e-4, gradients at 1e-3 of their floors at most."""
import numpy as np
import pytest
import torch

import ssim_ref as SR
from conftest import load_golden
from smpl_nerf_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("name", list(SR.G20_CASES))
def test_restatement_against_the_reference_outputs(name):
    g = load_golden("g20_image_scores.npz")
    shape, family, k, sigma, data_range, seed = SR.G20_CASES[name]
    x, y = SR.images(family, shape, seed, data_range)
    assert np.array_equal(x, g[f"{name}/x"]) and np.array_equal(y, g[f"{name}/y"]), "the seeded inputs are not the stored ones"
    assert tuple(g[f"{name}/params"]) == (k, sigma, data_range)
    N, C = shape[:2]
    gS, gC = np.full((N, C), 1.0 / (N * C), np.float32), np.zeros((N, C), np.float32)      # d mean_n mean_c ssim
    r = SR.restated(x, y, SR.window(k, sigma), *SR.constants(data_range), gS, gC, torch.float64)
    ref = {key: g[f"{name}/f64/{key}"] for key in ("ssim_none", "cs_none", "ssim_mean", "mse", "dx", "dy")}
    floor = r["value_floor"].mean(1)
    for key, mine in (("ssim_none", r["ssim"].mean(1)), ("cs_none", r["cs"].mean(1))):
        err = np.abs(mine - ref[key])
        print(f"{name} {key}: |restatement - reference| {err.max():.3e}  floor {floor.min():.3e}")
        assert ref[key].shape == (N,) and np.all(err <= floor), (key, err, floor)
    assert abs(r["ssim"].mean() - ref["ssim_mean"]) <= floor.mean() and ref["ssim_mean"].shape == ()
    for key in ("dx", "dy"):
        err, fl = np.abs(r[key] - ref[key]).max(), r["grad_floor_" + key[1]]
        print(f"{name} {key}: max|restatement - reference| {err:.3e}  floor {fl:.3e}  max|reference| {np.abs(ref[key]).max():.3e}")
        assert err <= fl, (key, err, fl)
    mse = r["sqerr"].sum() / x.size / data_range ** 2
    assert abs(mse - ref["mse"]) <= 4 * SR.U * ref["mse"]
    # the fp32 run of the reference is an fp32 evaluation of the same function: within the bound an fp32 kernel gets
    f32 = g[f"{name}/f32/ssim_none"]
    r32 = SR.restated(x, y, SR.window(k, sigma), *SR.constants(data_range), None, None, torch.float32)
    assert np.all(np.abs(f32 - ref["ssim_none"]) <= np.maximum(SR.FACTOR * np.abs(r32["ssim"].mean(1) - r["ssim"].mean(1)), floor))


def test_window_and_tile_constants():
    from smpl_nerf_amd import ops
    for k, sigma in ((11, 1.5), (7, 1.5), (4, 0.8), (1, 1.5), (33, 5.0)):
        w = ops.ssim_window(k, sigma)
        assert w.dtype == np.float32 and w.shape == (k,) and np.array_equal(w, SR.window(k, sigma)) and abs(float(w.sum()) - 1) <= k * SR.U
    t = ops.SSIM_TILES
    assert t["SSIM_TILE"] >= 8 and t["SSIM_MAX_K"] >= 11 and t["SSIM_BWD_TILE_SMALL"] <= t["SSIM_TILE"] and t["SSIM_BWD_SMALL_FROM_K"] > 11


def _fwd(lib, x=8, y=8, N=1, C=3, H=20, W=20, win=8, k=11, c1=1e-4, c2=9e-4, ssim=8, ws=8, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.snerf_ssim_workspace_bytes(N, C, H, W, k), 0)
    return lib.snerf_ssim_fwd_f32(x, y, N, C, H, W, C * H * W, H * W, W, 1, win, k, c1, c2, ssim, None, None, ws, ws_bytes, None)


def _bwd(lib, x=8, y=8, N=1, C=3, H=20, W=20, win=8, k=11, c1=1e-4, c2=9e-4, g=8, dx=8, ws=8, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.snerf_ssim_workspace_bytes(N, C, H, W, k), 0)
    return lib.snerf_ssim_bwd_f32(x, y, N, C, H, W, C * H * W, H * W, W, 1, win, k, c1, c2, g, None, dx, ws, ws_bytes, None)


def test_argument_validation_happens_on_the_host(lib):
    """Every refusal comes before anything touches a device: this runs where there is none.  (The non-null pointers are the number 8:
    nothing may read through them.)"""
    from smpl_nerf_amd import ops
    cap = ops.SSIM_TILES["SSIM_MAX_K"]
    err = lib.snerf_last_error_string
    for call in (_fwd, _bwd):
        assert call(lib, H=10) == -1 and b"H = 10" in err() and b"W = 20" in err() and b"k = 11" in err()
        assert call(lib, W=10) == -1 and b"W = 10" in err()
        assert call(lib, k=0) == -1 and b"window size" in err()
        assert call(lib, k=cap + 1, H=64, W=64) == -1 and b"window size" in err()
        assert call(lib, c2=float("nan")) == -1 and b"c2" in err()
        assert call(lib, c1=-1e-4) == -1 and call(lib, c1=float("inf")) == -1
        assert call(lib, N=-1) == -1
        for name in ("x", "y", "win", "ws"):
            assert call(lib, **{name: None}) == -1, name
        need = lib.snerf_ssim_workspace_bytes(1, 3, 20, 20, 11)
        assert need > 0 and call(lib, ws_bytes=need - 1) == -1 and b"workspace" in err()
        assert call(lib, H=2 ** 31, W=11) == -1 and call(lib, N=2 ** 40, H=64, W=64) == -1      # extents / tile counts beyond int32
        # N C == 0: nothing to do, whatever the pointers are
        assert call(lib, N=0, x=None, y=None, win=None, ws=None, ws_bytes=0) == 0
        assert call(lib, C=0, x=None, y=None, win=None, ws=None, ws_bytes=0) == 0
        assert call(lib, N=0, k=0) == -1                                                         # a bad scalar is an error whatever N is
    assert _fwd(lib, ssim=None) == -1 and _bwd(lib, dx=None) == -1 and _bwd(lib, g=None) == -1
    assert lib.snerf_ssim_workspace_bytes(1, 3, 10, 20, 11) == -1 and lib.snerf_ssim_workspace_bytes(1, 3, 20, 20, 0) == -1


def test_workspace_bytes_is_monotone_in_the_tile_count(lib):
    from smpl_nerf_amd import ops
    T, k = ops.SSIM_TILES["SSIM_TILE"], 11
    one = lib.snerf_ssim_workspace_bytes(1, 1, k, k, k)
    assert one > 0
    for tiles_y in range(1, 4):
        for tiles_x in range(1, 4):
            for H, W in ((T * (tiles_y - 1) + 1 + k - 1, T * (tiles_x - 1) + 1 + k - 1), (T * tiles_y + k - 1, T * tiles_x + k - 1)):
                assert lib.snerf_ssim_workspace_bytes(1, 1, H, W, k) == one * tiles_y * tiles_x, (H, W)
                assert lib.snerf_ssim_workspace_bytes(2, 3, H, W, k) == 6 * one * tiles_y * tiles_x
    assert lib.snerf_ssim_workspace_bytes(1, 1, T + k, k, k) == 2 * one                                      # one window past the tile
    assert lib.snerf_ssim_workspace_bytes(0, 3, 20, 20, k) == 0


def test_cpu_tensors_are_rejected():
    from smpl_nerf_amd import ops
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ssim(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.image_scores(x.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1))
