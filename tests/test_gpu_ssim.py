"""The image scores on the GPU: csrc/ssim.hip through ops.ssim / ops.image_scores / DataParallelTrainer.validate_scores.

Yardstick: tests/ssim_ref.py - the torch restatement in float64 (y64) and in fp32 (y32) of the same fp32 inputs and the same fp32
window.  Bounds, with u = 2^-24 and cond = (e11 + e22) / D per window in float64 - derived there, never taken from the kernel:
    ssim, cs per (n, c)   |kernel - y64| <= max(8 |y32 - y64|, 16 u mean_q cond + 4 u)
    dx, dy (max norm)     max|kernel - y64| <= max(8 max|y32 - y64|, 16 u max_p Gamma[p])
    sqerr, relative       <= max(8 E32, 4 u)
Every test prints kernel error, fp32 CPU error, floor and kernel / bound per quantity before it asserts (pytest -s;
profiles/ssim_errors.txt holds a run on an MI355X: the kernel at 0.13 of its bound at worst for the values - constant 0.9 against
constant 0.3, error 1.2e-4 beside 1.1e-4 of the fp32 CPU restatement and a floor of 9.5e-4 - and at 0.045 for the gradients).

Shapes: the operator cases cover one window, extents below the window plus tile, several tiles, even and small windows; the extents
T - 1, T, T + 1 (T = ops.SSIM_TILES['SSIM_TILE']) of the forward's window tiles and of the backward's pixel tiles in each dimension
alone; and window sizes on both sides of the backward's switch to its small tile.  Each runs with five image families."""
import functools

import numpy as np
import pytest
import torch

import ssim_ref as SR
from conftest import load_golden
from smpl_nerf_amd import ops

pytestmark = pytest.mark.gpu
T_ = ops.SSIM_TILES["SSIM_TILE"]
SMALL_K = ops.SSIM_TILES["SSIM_BWD_SMALL_FROM_K"]
CASES = [(2, 3, 11, 11, 11), (1, 3, 12, 43, 11), (1, 1, 43, 12, 11), (2, 3, 45, 77, 11), (1, 2, 9, 5, 3), (1, 3, 33, 33, 7), (1, 1, 8, 9, 4)]
CASES += [(1, 1, e + 10, 12, 11) for e in (T_ - 1, T_)] + [(1, 1, 12, e + 10, 11) for e in (T_ - 1, T_)]      # window extents (T + 1: above)
CASES += [(1, 1, T_ - 1, T_, 11), (1, 1, T_, T_ - 1, 11), (1, 1, T_ + 1, T_ + 1, 11)]                          # pixel extents of the backward
CASES += [(1, 1, SMALL_K + 6, SMALL_K + 18, SMALL_K - 1), (1, 1, SMALL_K + 7, SMALL_K + 1, SMALL_K),           # the backward's two tiles
          (1, 2, 40, 50, ops.SSIM_TILES["SSIM_MAX_K"])]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def N_(t):
    return t.detach().cpu().numpy()


def sigma_of(k):
    return 1.5 if k >= 7 else 0.8


@functools.lru_cache(maxsize=None)
def case(shape, family, k, data_range=1.0, seed=1, same=False):
    """Inputs, upstream gradients and both CPU restatements of one case, computed once and shared (read-only)."""
    x, y = SR.images(family, shape, seed, data_range)
    if same:
        y = x.copy()
    gS, gC = SR.upstream(shape[0], shape[1], seed)
    win, (c1, c2) = SR.window(k, sigma_of(k)), SR.constants(data_range)
    return (x, y, gS, gC), SR.restated(x, y, win, c1, c2, gS, gC, torch.float32), SR.restated(x, y, win, c1, c2, gS, gC, torch.float64)


def on_gpu(dev, x, y, gS, gC, k, data_range=1.0, arrange=lambda t: t):
    """ssim, cs, sqerr [N,C] and dx, dy of sum(gS ssim + gC cs); `arrange` lays a device tensor out (strides) before the call."""
    xt, yt = (arrange(torch.from_numpy(a).to(dev)).requires_grad_(True) for a in (x, y))
    ssim, cs, _ = ops._ssim_per_channel(xt, yt, k, sigma_of(k), data_range, 0.01, 0.03)
    assert ssim.grad_fn is not None and tuple(ssim.shape) == tuple(cs.shape) == x.shape[:2]
    (torch.from_numpy(gS).to(dev) * ssim + torch.from_numpy(gC).to(dev) * cs).sum().backward()
    with torch.no_grad():
        ssim2, cs2, sqerr = ops._ssim_per_channel(xt, yt, k, sigma_of(k), data_range, 0.01, 0.03, want_sqerr=True)
    assert ssim2.grad_fn is None and torch.equal(ssim2, ssim) and torch.equal(cs2, cs)
    return {"ssim": N_(ssim), "cs": N_(cs), "sqerr": N_(sqerr), "dx": N_(xt.grad), "dy": N_(yt.grad)}


@pytest.mark.parametrize("family", SR.FAMILIES)
@pytest.mark.parametrize("shape_k", CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward_and_both_gradients(dev, shape_k, family):
    shape, k = shape_k[:4], shape_k[4]
    (x, y, gS, gC), y32, y64 = case(shape, family, k)
    SR.hold(f"{list(shape)} k={k} {family}", on_gpu(dev, x, y, gS, gC, k), y32, y64)


@pytest.mark.parametrize("family", ("noise", "constant"))
def test_data_range_255(dev, family):
    shape, k = (1, 3, 20, 23), 11
    (x, y, gS, gC), y32, y64 = case(shape, family, k, 255.0)
    SR.hold(f"{list(shape)} k={k} {family} range 255", on_gpu(dev, x, y, gS, gC, k, 255.0), y32, y64)


@pytest.mark.parametrize("family", ("random", "ramp", "constant", "halfblack"))
@pytest.mark.parametrize("shape_k", [(2, 3, 45, 77, 11), (1, 3, 33, 33, 7), (1, 1, 8, 9, 4)], ids=lambda c: "x".join(map(str, c)))
def test_identical_images(dev, shape_k, family):
    """x == y: ssim == cs == 1 exactly and sqerr == 0; the gradient vanishes up to the gradient floor."""
    shape, k = shape_k[:4], shape_k[4]
    (x, y, gS, gC), y32, y64 = case(shape, family, k, same=True)
    got = on_gpu(dev, x, y, gS, gC, k)
    assert np.all(got["ssim"] == 1) and np.all(got["cs"] == 1) and np.all(got["sqerr"] == 0), (got["ssim"], got["cs"], got["sqerr"])
    for name in ("dx", "dy"):
        worst, floor = np.abs(got[name]).max(), y64["grad_floor_" + name[1]]
        print(f"{list(shape)} k={k} {family} x == y {name}: max|kernel| {worst:.3e}  max|y64| {np.abs(y64[name]).max():.3e}  floor {floor:.3e}")
        assert worst <= floor      # (the exact gradient at x == y is zero: both scores are at their maximum)


def test_layouts_and_repeated_calls_give_the_same_bits(dev):
    """Channels-last storage, a non-contiguous slice, x and y of different strides: the bits of the contiguous channels-first run;
    and the same bits on a second call."""
    shape, k = (2, 3, 45, 77), 11
    (x, y, gS, gC), _, _ = case(shape, "noise", k)
    base = on_gpu(dev, x, y, gS, gC, k)

    def channels_last(t):
        out = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert out.stride()[1] == 1 and not out.is_contiguous()
        return out

    def sliced(t):
        big = torch.full((2, 4, 50, 90), float("nan"), device=t.device)
        big[:, 1:, 2:47, 5:82] = t
        out = big[:, 1:, 2:47, 5:82]
        assert not out.is_contiguous()
        return out

    flip = [True]

    def mixed(t):      # x channels-first, y channels-last: the operator brings y to x's strides
        flip[0] = not flip[0]
        return channels_last(t) if flip[0] else t

    for name, arrange in (("again", lambda t: t), ("channels-last", channels_last), ("slice", sliced), ("mixed", mixed)):
        got = on_gpu(dev, x, y, gS, gC, k, arrange=arrange)
        for key in base:
            assert np.array_equal(got[key], base[key]), (name, key, np.abs(got[key] - base[key]).max())


def test_null_g_cs_is_zeros_and_one_sided_gradients(dev):
    shape, k = (1, 3, 33, 33), 7
    (x, y, gS, gC), _, _ = case(shape, "noise", k)
    xt, yt, gs = (torch.from_numpy(a).to(dev) for a in (x, y, gS))
    win, (c1, c2) = torch.from_numpy(SR.window(k, sigma_of(k))).to(dev), SR.constants()
    a = ops._ssim_bwd(xt, yt, win, c1, c2, gs, None)
    b = ops._ssim_bwd(xt, yt, win, c1, c2, gs, torch.zeros_like(gs))
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # only y wants a gradient: one backward launch, and it is dy of the two-sided run
    both = on_gpu(dev, x, y, gS, np.zeros_like(gC), k)
    yg = yt.clone().requires_grad_(True)
    from smpl_nerf_amd import _lib
    before = _lib.CALLS
    ssim, cs, _ = ops._ssim_per_channel(xt, yg, k, sigma_of(k), 1.0, 0.01, 0.03)
    (gs * ssim).sum().backward()
    assert _lib.CALLS - before == 2 and np.array_equal(N_(yg.grad), both["dy"])
    assert np.array_equal(N_(ops._ssim_bwd(yt, xt, win, c1, c2, gs, None)), both["dy"])      # dy = the entry with the images swapped


def test_errors_and_conventions(dev):
    x = torch.rand(2, 3, 16, 20, device=dev)
    y = (x + 0.05 * torch.rand_like(x)).clamp(0, 1)
    with pytest.raises(ValueError, match="Kernel size"):
        ops.ssim(x[..., :10], y[..., :10])                        # scores.py:148-150
    with pytest.raises(ValueError, match="Kernel size"):
        ops.ssim(x[:, :, :10], y[:, :, :10])
    with pytest.raises(RuntimeError):
        ops.ssim(x[0], y[0])
    with pytest.raises(RuntimeError):
        ops.ssim(x.double(), y.double())
    with pytest.raises(RuntimeError, match="kernel_size"):
        ops.ssim(torch.rand(1, 1, 40, 40, device=dev), torch.rand(1, 1, 40, 40, device=dev), kernel_size=ops.SSIM_TILES["SSIM_MAX_K"] + 1)
    with pytest.raises(KeyError):
        ops.ssim(x, y, reduction="median")
    none, cs = ops.ssim(x, y, reduction="none", full=True)
    assert tuple(none.shape) == tuple(cs.shape) == (2,) and none.grad_fn is None
    mean, total = ops.ssim(x, y), ops.ssim(x, y, reduction="sum")
    assert mean.dim() == 0 and total.dim() == 0 and not isinstance(mean, tuple)
    assert torch.equal(mean, none.mean(dim=0)) and torch.equal(total, none.sum(dim=0))
    assert tuple(ops.ssim(x[:0], y[:0], reduction="none").shape) == (0,)


# ---------------------------------------------------------------------------------------------- the reference's own outputs
@pytest.mark.parametrize("name", list(SR.G20_CASES))
def test_against_the_reference_outputs(dev, name):
    """g20: ops.ssim and its autograd gradients, ops.image_scores' mse and psnr against what the reference computed in float64.
    Bound: max(8 |reference fp32 - reference f64|, 8 |restatement f64 - reference f64|, the floors)."""
    g = load_golden("g20_image_scores.npz")
    shape, family, k, sigma, data_range, seed = SR.G20_CASES[name]
    x, y = g[f"{name}/x"], g[f"{name}/y"]
    N, C = shape[:2]
    gS, gC = np.full((N, C), 1.0 / (N * C), np.float32), np.zeros((N, C), np.float32)
    r64 = SR.restated(x, y, SR.window(k, sigma), *SR.constants(data_range), gS, gC, torch.float64)
    f32, f64 = ({key: g[f"{name}/{tag}/{key}"] for key in ("ssim_none", "cs_none", "ssim_mean", "mse", "psnr", "dx", "dy")} for tag in ("f32", "f64"))
    xt, yt = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (x, y))
    kw = dict(kernel_size=k, kernel_sigma=sigma, data_range=data_range)
    mean = ops.ssim(xt, yt, **kw)
    mean.backward()
    none, cs = ops.ssim(xt.detach(), yt.detach(), reduction="none", full=True, **kw)
    assert tuple(none.shape) == f64["ssim_none"].shape and tuple(cs.shape) == f64["cs_none"].shape and tuple(mean.shape) == f64["ssim_mean"].shape
    got = {"ssim": N_(none), "cs": N_(cs), "dx": N_(xt.grad), "dy": N_(yt.grad)}
    ref32 = {"ssim": f32["ssim_none"], "cs": f32["cs_none"], "dx": f32["dx"], "dy": f32["dy"]}
    ref64 = {"ssim": f64["ssim_none"], "cs": f64["cs_none"], "dx": f64["dx"], "dy": f64["dy"],
             "value_floor": r64["value_floor"].mean(1), "grad_floor_x": r64["grad_floor_x"], "grad_floor_y": r64["grad_floor_y"]}
    restatement = {"ssim": SR.FACTOR * np.abs(r64["ssim"].mean(1) - f64["ssim_none"]), "cs": SR.FACTOR * np.abs(r64["cs"].mean(1) - f64["cs_none"]),
                   "dx": SR.FACTOR * np.abs(r64["dx"] - f64["dx"]).max(), "dy": SR.FACTOR * np.abs(r64["dy"] - f64["dy"]).max()}
    SR.hold(f"g20 {name}", got, ref32, ref64, extra=restatement)
    err = abs(float(mean.detach()) - float(f64["ssim_mean"]))
    assert err <= max(SR.FACTOR * abs(float(f32["ssim_mean"]) - float(f64["ssim_mean"])), float(ref64["value_floor"].mean())), err

    # mse and psnr.  The reference scored the images divided by their range (in float64 exact up to 1e-16); here the images are scored
    # as they are: mse = range^2 x the reference's, psnr = the reference's - 20 log10(range).
    R = data_range
    sc = ops.image_scores(xt.detach().permute(0, 2, 3, 1).contiguous(), yt.detach().permute(0, 2, 3, 1).contiguous(), **kw)
    assert all(v.dim() == 0 and v.is_cuda for v in sc.values()) and sorted(sc) == ["mse", "psnr", "ssim"]
    cf = ops.image_scores(xt.detach(), yt.detach(), channels_first=True, **kw)
    assert all(torch.equal(sc[key], cf[key]) for key in sc) and torch.equal(sc["ssim"], mean.detach())
    mse64 = float(f64["mse"])
    e32 = abs(float(f32["mse"]) - mse64) / mse64
    rel = max(SR.FACTOR * e32, 4 * SR.U)
    ek = abs(float(sc["mse"]) / R ** 2 - mse64) / mse64
    psnr_k, psnr64 = float(sc["psnr"]) + 20.0 * np.log10(R), -10.0 * np.log(mse64) / np.log(10.0)
    print(f"g20 {name} mse: kernel error {ek:.3e}  reference fp32 error {e32:.3e}  bound {rel:.3e};  psnr: kernel {psnr_k:.9f}  "
          f"float64 {psnr64:.9f}  reference {float(f64['psnr']):.9f}")
    assert ek <= rel
    assert abs(psnr_k - psnr64) <= 10.0 / np.log(10.0) * rel
    # the reference's own psnr is an fp32 number in both arithmetics (scores.py:48 divides by an fp32 tensor: -10 ln(mse) and ln(10)
    # rounded to fp32, then the quotient - three roundings of 2^-24 relative each)
    assert abs(psnr_k - float(f64["psnr"])) <= 10.0 / np.log(10.0) * rel + 3 * SR.U * abs(psnr64)


# ---------------------------------------------------------------------------------------------- the trainer
def test_validate_scores(dev):
    """validate_scores on a synthetic frame loader: the loss of validate(), psnr equal to validate()'s host value within the mse bound,
    ssim equal to ops.ssim on validate()'s frames bit for bit."""
    from smpl_nerf_amd import synthetic as syn
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs
    from smpl_nerf_amd.raygen import RayGenerator
    from smpl_nerf_amd.trainer import DataParallelTrainer, FrameLoader
    h, w = 24, 32
    poses = np.stack([syn.sphere_pose(phi, 10.0, 2.4) for phi in (0.0, 40.0)])
    images = np.stack([syn.procedural_image(h, w, phi, 10.0) for phi in (0.0, 40.0)]).astype(np.float32)
    gen = RayGenerator(poses, h, w, np.pi / 3, 1.0, 4.0, 64, dev, images=images)
    nets = []
    for p in syn.make_scene_nets(101):
        m = RenderRayNet(8, 256, 60, 24, skips=[4])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
        nets.append(m.to(dev))
    tr = DataParallelTrainer(NerfPipeline(nets[0], nets[1], PipelineArgs(), PositionalEncoder(10, 0), PositionalEncoder(4, 0)), nets, lr=5e-4)
    val_loss, psnr, frames = tr.validate(FrameLoader(gen, [0, 1], 256), h, w)
    val_loss2, scores = tr.validate_scores(FrameLoader(gen, [0, 1], 256), h, w)
    assert val_loss2 == val_loss and frames.shape == (2, h, w, 3) and sorted(scores) == ["mse", "psnr", "ssim"]
    truth = torch.from_numpy(images).to(dev)
    want = ops.ssim(torch.from_numpy(frames).to(dev).permute(0, 3, 1, 2), truth.permute(0, 3, 1, 2))
    assert torch.equal(scores["ssim"], want) and 0 < float(want) < 1
    mse64 = float(np.mean((frames.astype(np.float64) - images.astype(np.float64)) ** 2))
    print(f"validate_scores: mse {float(scores['mse']):.9e} (host {mse64:.9e})  psnr {float(scores['psnr']):.7f} (validate() {psnr:.7f})  ssim {float(want):.7f}")
    assert abs(float(scores["mse"]) - mse64) <= 4 * SR.U * mse64
    assert abs(float(scores["psnr"]) - psnr) <= 10.0 / np.log(10.0) * 4 * SR.U
    assert tr.validate_scores(FrameLoader(gen, [0], 256), h + 1, w)[1] is None and tr.validate_scores([], h, w) == (0.0, None)
