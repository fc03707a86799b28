"""The ray maps on the GPU (csrc/ray_maps.hip, ops.ray_maps, NerfPipeline.ray_maps, DataParallelTrainer.validate_maps).

Yardstick: the float64 restatement (tests/ray_maps_ref.py) of the same fp32 inputs, and the reference's own float64 depth_map and
acc_map (g29_ray_maps.npz); never the kernel.  Bound of every output (the convention of 8l): with
E = max|fp32 torch-CPU restatement - yardstick|, the device's distance from the yardstick is at most max(8 E, 2^-22 max|yardstick|)
- the device may not be worse than eight times what plain fp32 torch does; the floor keeps a case the restatement gets exactly
from demanding 0.  Run with -s for the measured error / bound ratios (profiles/ray_maps_errors.txt)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ray_maps_ref as RR
from conftest import load_golden
from smpl_nerf_amd import _lib, ops
from smpl_nerf_amd import synthetic as syn

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 128, 129, 192, 4096)
BS = (1, 5, 67)
FLOOR = 2.0 ** -22
_REF = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def T(x, dev):
    return None if x is None else x.to(dev)


def hold(name, got, want64, rest32):
    """got (device result, any device) against the yardstick under max(8 E(rest32), 2^-22 max|want64|); returns err / bound."""
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{name}: not finite"
    err = float((got - want64).abs().max())
    E = float((rest32.double() - want64).abs().max())
    bound = max(8 * E, FLOOR * float(want64.abs().max()))
    ratio = err / bound if bound > 0 else 0.0
    print(f"  {name}: err {err:.2e}  E(fp32 restatement) {E:.2e}  bound {bound:.2e}  err/bound {ratio:.3f}")
    assert err <= bound, (name, err, bound)
    return ratio


def grads_of(case, mode, which=("d_acc", "d_depth", "d_point")):
    return {k: (case[k] if k in which and (k != "d_point" or mode == "pts") else None) for k in ("d_acc", "d_depth", "d_point")}


def reference(case, mode, which=("d_acc", "d_depth", "d_point")):
    """((acc, depth, point), d alpha) of the restatement in float64 and in float32."""
    out = []
    for dtype in (torch.float64, torch.float32):
        c = RR.cast(case, dtype)
        kw = dict(z=c["z"]) if mode == "z" else dict(pts=c["pts"])
        out.append(RR.ray_maps_autograd(c["alpha"], c["o"], c["d"], **kw, **grads_of(c, mode, which)))
    return out


def shared_reference(B, N, mode):
    key = (B, N, mode)
    if key not in _REF:
        case = RR.make_case(B, N, 11)
        _REF[key] = (case,) + tuple(reference(case, mode))
    return _REF[key]


def device_maps(case, mode, dev, want_point=True, which=("d_acc", "d_depth", "d_point")):
    """The two C entries, called directly: (acc, depth, point or None, d alpha)."""
    lib = _lib.load()
    c = {k: T(v, dev).contiguous() for k, v in case.items()}
    B, N = c["alpha"].shape
    z, pts = (c["z"], None) if mode == "z" else (None, c["pts"])
    acc, depth = torch.empty(B, device=dev), torch.empty(B, device=dev)
    point = torch.empty(B, 3, device=dev) if (mode == "pts" and want_point) else None
    d_alpha = torch.empty(B, N, device=dev)
    g = grads_of(c, mode, which)
    if not want_point:
        g["d_point"] = None
    s = _lib.current_stream()
    p = _lib.ptr
    _lib.check(lib.snerf_ray_maps_fwd_f32(p(c["alpha"]), p(z), p(pts), p(c["o"]), p(c["d"]), B, N, p(acc), p(depth), p(point), s), "fwd")
    _lib.check(lib.snerf_ray_maps_bwd_f32(p(c["alpha"]), p(z), p(pts), p(c["o"]), p(c["d"]), B, N, p(g["d_acc"]), p(g["d_depth"]),
                                          p(g["d_point"]), p(d_alpha), s), "bwd")
    torch.cuda.synchronize()
    return acc, depth, point, d_alpha


def hold_all(tag, got, ref64, ref32):
    (acc64, depth64, point64), da64 = ref64
    (acc32, depth32, point32), da32 = ref32
    acc, depth, point, d_alpha = got
    r = [hold(f"{tag} acc", acc, acc64, acc32), hold(f"{tag} depth", depth, depth64, depth32),
         hold(f"{tag} d_alpha", d_alpha, da64, da32)]
    if point is not None:
        r.append(hold(f"{tag} point", point, point64, point32))
    return max(r)


# ---- forward and backward against the float64 restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("z", "pts"))
@pytest.mark.parametrize("N", NS)
def test_maps_and_gradient_against_float64(dev, N, mode):
    """acc, depth, point and d alpha for B in (1, 5, 67): one ray, a part of a workgroup, several workgroups with a ragged last one;
    N below, at and above the 64-sample chunk, and at the limit.  In the points mode also without the point (point and d_point
    NULL): the other outputs keep their bits."""
    worst = 0.0
    for B in BS:
        case, ref64, ref32 = shared_reference(B, N, mode)
        got = device_maps(case, mode, dev)
        worst = max(worst, hold_all(f"{mode} B={B} N={N}", got, ref64, ref32))
        if mode == "pts":
            (_, d64), (_, d32) = reference(case, mode, which=("d_acc", "d_depth"))
            acc, depth, point, d_alpha = device_maps(case, mode, dev, want_point=False)
            assert point is None and torch.equal(acc, got[0]) and torch.equal(depth, got[1])
            worst = max(worst, hold(f"{mode} B={B} N={N} d_alpha without point", d_alpha, d64, d32))
    print(f"ray_maps {mode} N={N}: worst err/bound {worst:.3f}")


def test_ops_function_is_the_entries(dev):
    """ops.ray_maps under autograd gives the bits of the two entries called directly, in both modes; under no_grad it keeps no
    graph; point is None in the depths mode."""
    case = RR.make_case(5, 129, 11)
    for mode in ("z", "pts"):
        acc, depth, point, d_alpha = device_maps(case, mode, dev)
        a = T(case["alpha"], dev).requires_grad_(True)
        kw = dict(z_vals=T(case["z"], dev)) if mode == "z" else dict(samples=T(case["pts"], dev))
        m = ops.ray_maps(a, T(case["o"], dev), T(case["d"], dev), **kw)
        assert isinstance(m, ops.RayMaps) and (m.point is None) == (mode == "z")
        loss = (m.acc * T(case["d_acc"], dev)).sum() + (m.depth * T(case["d_depth"], dev)).sum()
        if mode == "pts":
            loss = loss + (m.point * T(case["d_point"], dev)).sum()
            assert torch.equal(m.point, point)
        loss.backward()
        assert torch.equal(m.acc, acc) and torch.equal(m.depth, depth) and torch.equal(a.grad, d_alpha)
        with torch.no_grad():
            n = ops.ray_maps(a, T(case["o"], dev), T(case["d"], dev), **kw)
        assert n.acc.grad_fn is None and not n.depth.requires_grad and torch.equal(n.acc, acc)
    with pytest.raises(RuntimeError, match="exactly one"):
        ops.ray_maps(a, T(case["o"], dev), T(case["d"], dev))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ray_maps(case["alpha"], case["o"], case["d"], z_vals=case["z"])
    with pytest.raises(RuntimeError, match="4096"):
        ops.ray_maps(torch.zeros(2, 4097, device=dev), T(case["o"][:2], dev), T(case["d"][:2], dev), z_vals=torch.zeros(2, 4097, device=dev))
    empty = ops.ray_maps(torch.zeros(0, 7, device=dev), torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev),
                         samples=torch.zeros(0, 7, 3, device=dev))
    assert empty.acc.shape == (0,) and empty.point.shape == (0, 3)


# ---- edge rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (2, 65, 192))
def test_edge_rows(dev, N):
    """RR.EDGE_ROWS, each ray under its own bound and finite: alpha all 0 (acc = depth = 0 and d alpha_k = G_k, exactly what
    fl32 gives of G), alpha_0 = 1, alpha = 1 in the middle, alpha = 1 everywhere (u = 1e-10: the quotient of the backward), one
    alpha of 0.99999994, d = 0 in the points mode."""
    case = RR.make_edge_case(N)
    for mode in ("z", "pts"):
        ref64, ref32 = reference(case, mode)
        got = device_maps(case, mode, dev)
        for r, name in enumerate(RR.EDGE_ROWS):
            row = lambda ref: (tuple(None if t is None else t[r:r + 1] for t in ref[0]), ref[1][r:r + 1])
            hold_all(f"edge {name} {mode} N={N}", tuple(None if t is None else t[r:r + 1] for t in got), row(ref64), row(ref32))
        acc, depth, point, d_alpha = (None if t is None else t.cpu() for t in got)
        assert acc[0] == 0 and depth[0] == 0
        c = RR.cast(case, torch.float64)
        t = c["z"] if mode == "z" else RR.sample_parameter(c["o"], c["d"], c["pts"])
        G = c["d_acc"][:, None] + c["d_depth"][:, None] * t
        if mode == "pts":
            G = G + (c["d_point"][:, None, :] * c["pts"]).sum(-1)
            assert depth[5] == 0          # d = 0: t = 0
        assert float((d_alpha[0].double() - G[0]).abs().max()) <= 2.0 ** -23 * float(G[0].abs().max())      # one rounding of G
        if N > 2:
            assert acc[3] == 1            # opaque from the first sample on


def test_each_upstream_gradient_alone_and_none(dev):
    case = RR.make_case(5, 129, 13)
    for which in (("d_acc",), ("d_depth",), ("d_point",)):
        (_, d64), (_, d32) = reference(case, "pts", which)
        d_alpha = device_maps(case, "pts", dev, which=which)[3]
        hold(f"only {which[0]}", d_alpha, d64, d32)
    for mode in ("z", "pts"):
        d_alpha = device_maps(case, mode, dev, which=())[3]
        assert torch.equal(d_alpha, torch.zeros_like(d_alpha)), "all three gradients NULL: d alpha must be exactly 0"


def test_nan_alpha_stays_in_its_ray(dev):
    case = RR.make_case(9, 129, 17)
    clean = device_maps(case, "pts", dev)
    case["alpha"][4, 70] = float("nan")
    acc, depth, point, d_alpha = device_maps(case, "pts", dev)
    others = [r for r in range(9) if r != 4]
    assert torch.isnan(acc[4]) and torch.isnan(depth[4]) and torch.isnan(point[4]).all()
    for got, ref in zip((acc, depth, point, d_alpha), clean):
        assert torch.equal(got[others], ref[others])


# ---- against the golden: the reference's own raw2outputs ------------------------------------------------------------------------
def _cpu_chain(g, k, dtype):
    """raw -> alpha (utils.py:161-175) -> maps in `dtype` on the CPU, with the gradient of the golden's loss to raw."""
    raw = torch.from_numpy(g[f"{k}/raw"]).to(dtype).requires_grad_(True)
    z, dirs = torch.from_numpy(g[f"{k}/z"]).to(dtype), torch.from_numpy(g[f"{k}/dirs"]).to(dtype)
    acc, depth, _ = RR.ray_maps(RR.raw2alpha(raw, z, dirs), None, None, z=z)
    loss = (torch.from_numpy(g[f"{k}/g_depth"]).to(dtype) * depth).sum() + (torch.from_numpy(g[f"{k}/g_acc"]).to(dtype) * acc).sum()
    if loss.requires_grad:
        loss.backward()
    return acc.detach(), depth.detach(), raw.grad if raw.grad is not None else torch.zeros_like(raw)


@pytest.mark.parametrize("B,N", RR.GOLDEN_SHAPES)
@pytest.mark.parametrize("wb", (0, 1))
def test_chain_against_the_reference(dev, B, N, wb):
    """ops.composite then ops.ray_maps(z_vals=...) on the golden's raw: acc and depth against the reference's float64 acc_map and
    depth_map, the chain's gradient to raw against the reference's float64 autograd; E from the torch-CPU fp32 chain."""
    g = load_golden("g29_ray_maps.npz")
    k = f"{B}x{N}"
    raw = torch.from_numpy(g[f"{k}/raw"]).to(dev).requires_grad_(True)
    z, dirs = torch.from_numpy(g[f"{k}/z"]).to(dev), torch.from_numpy(g[f"{k}/dirs"]).to(dev)
    rgb, weights, alpha = ops.composite(raw, z, dirs, bool(wb))
    m = ops.ray_maps(alpha, torch.zeros(B, 3, device=dev), dirs, z_vals=z)
    ((torch.from_numpy(g[f"{k}/g_depth"]).to(dev) * m.depth).sum() + (torch.from_numpy(g[f"{k}/g_acc"]).to(dev) * m.acc).sum()).backward()
    acc32, depth32, draw32 = _cpu_chain(g, k, torch.float32)
    hold(f"golden {k} wb{wb} acc", m.acc, torch.from_numpy(g[f"{k}/f64/acc_map"]), acc32)
    hold(f"golden {k} wb{wb} depth", m.depth, torch.from_numpy(g[f"{k}/f64/depth_map"]), depth32)
    hold(f"golden {k} wb{wb} d_raw", raw.grad, torch.from_numpy(g[f"{k}/f64/d_raw"]), draw32)
    # the fp32 chain is a fair stand-in for the reference's own fp32 run
    assert float((acc32 - torch.from_numpy(g[f"{k}/f32/acc_map"])).abs().max()) <= 4e-7


# ---- consistency with the compositing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", ((67, 192), (5, 65), (3, 4096)))
def test_maps_belong_to_the_composited_weights(dev, B, N):
    """acc against the float64 sum of the weights ops.composite returned, rounded once: at most 1 ulp (the kernel rebuilds the
    weights' bits; only the order of its float64 sum differs).  rgb(white_background = 1) - rgb(white_background = 0) is
    1 - sum(weights) in every channel: the device's difference against 1 - acc within 8 E, E = the distance of the fp32 CPU
    compositing's own difference from the float64 1 - acc."""
    from oracle import torch_cpu_path as TP
    gen = torch.Generator().manual_seed(31 + N)
    raw = torch.randn(B, N, 4, generator=gen)
    raw[..., 3] = torch.randn(B, N, generator=gen) * (40.0 / N)
    z = torch.sort(2.0 + 4.0 * torch.rand(B, N, generator=gen), -1)[0]
    dirs = torch.randn(B, 3, generator=gen)
    rgb0, weights, alpha = ops.composite(T(raw, dev), T(z, dev), T(dirs, dev), False)
    rgb1, _, _ = ops.composite(T(raw, dev), T(z, dev), T(dirs, dev), True)
    m = ops.ray_maps(alpha, torch.zeros(B, 3, device=dev), T(dirs, dev), z_vals=T(z, dev))
    want = weights.cpu().double().sum(-1).float()
    ulps = ((m.acc.cpu().double() - want.double()).abs() / torch.from_numpy(np.spacing(want.numpy())).double()).max()
    print(f"  B={B} N={N}: acc vs fl32(float64 sum of the composited weights): {float(ulps):.2f} ulp")
    assert float(ulps) <= 1.0
    acc64 = RR.ray_maps(alpha.cpu().double(), None, None, z=z.double())[0]
    cpu = [TP.raw2outputs(raw, z, dirs[:, None, :].expand(B, N, 3), SimpleNamespace(sigma_noise_std=0., white_background=wb))[0]
           for wb in (0, 1)]
    E = float(((cpu[1] - cpu[0]).double() - (1 - acc64)[:, None]).abs().max())
    err = float(((rgb1 - rgb0).cpu().double() - (1 - m.acc.cpu().double())[:, None]).abs().max())
    bound = max(8 * E, FLOOR)
    print(f"  B={B} N={N}: (rgb_wb1 - rgb_wb0) - (1 - acc): {err:.2e}, E(fp32 CPU compositing) {E:.2e}, err/bound {err / bound:.3f}")
    assert err <= bound


# ---- pipelines ----------------------------------------------------------------------------------------------------------------
def _net(dev, params):
    from smpl_nerf_amd.nets import RenderRayNet
    m = RenderRayNet(8, 256, 60, 24, skips=[4])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.to(dev)


def _pipeline(dev, kind):
    from smpl_nerf_amd.nets import WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs, SmplNerfPipeline
    pc, pf = syn.make_scene_nets(101)
    args = PipelineArgs(number_fine_samples=8)
    pe, de = PositionalEncoder(10, 0), PositionalEncoder(4, 0)
    if kind == "nerf":
        return NerfPipeline(_net(dev, pc), _net(dev, pf), args, pe, de)
    mw = WarpFieldNet(8, 256, 60, 40)
    mw.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_warp_field_params(103, out_scale=0.05).items()})
    return SmplNerfPipeline(_net(dev, pc), _net(dev, pf), mw.to(dev), args, pe, de, PositionalEncoder(10, 0))


def _rays(dev, n, kind, h=8, w=8, n_coarse=8):
    b = [torch.from_numpy(a[:n]).to(dev) for a in syn.frame_batch(h, w, n_coarse=n_coarse, seed=3)]
    if kind == "smpl":
        pose = torch.from_numpy(syn.human_poses()[np.arange(n) % 10].astype(np.float32)).to(dev)
        return b[:4] + [pose, b[4]]
    return b


def _hold_pipeline_maps(tag, m, out, data):
    samples, dens = ((out[2], out[3]) if len(out) == 4 else (out[3], out[5]))
    case = {"alpha": dens.detach().cpu(), "o": data[1].cpu(), "d": data[2].cpu(), "pts": samples.detach().cpu()}
    (a64, d64, p64), (a32, d32, p32) = [RR.ray_maps(*(RR.cast(case, dt)[k] for k in ("alpha", "o", "d")), pts=RR.cast(case, dt)["pts"])
                                        for dt in (torch.float64, torch.float32)]
    refs = ((a64, a32), (d64, d32), (p64, p32))
    for name, got, (r64, r32) in zip(("acc", "depth", "point"), m, refs):
        hold(f"{tag} {name}", got, r64, r32)
    return [(r64, bound_of(r64, r32)) for r64, r32 in refs]


def bound_of(want64, rest32):
    return max(8 * float((rest32.double() - want64).abs().max()), FLOOR * float(want64.abs().max()))


@pytest.mark.parametrize("kind", ("nerf", "smpl"))
def test_pipeline_ray_maps(dev, kind):
    """5 rays x 8 + 8 samples: ray_maps(data, pipeline(data)) under no_grad (the single-call render) and with autograd on (the
    five launches), each against the float64 restatement on its own densities and samples and the two against each other; the
    depth lies inside the ray's sample range; a loss on depth and acc reaches every net."""
    pipe = _pipeline(dev, kind)
    data = _rays(dev, 5, kind)
    with torch.no_grad():
        out_s = pipe(data)
        m_s = pipe.ray_maps(data, out_s)
    assert m_s.depth.grad_fn is None and m_s.acc.shape == (5,) and m_s.point.shape == (5, 3)
    ref_s = _hold_pipeline_maps(f"{kind} single call", m_s, out_s, data)
    out_a = pipe(data)
    m_a = pipe.ray_maps(data, out_a)
    ref_a = _hold_pipeline_maps(f"{kind} launches", m_a, out_a, data)
    # The two paths against each other.  The maps are a pure function of (densities, samples): where both paths return the same
    # bits of those (NerfPipeline with nets in training mode) the maps are the same bits; where the pipeline's inference and
    # training kernels differ in the last bits of the densities (SmplNerfPipeline: the per-ray fold of the warp net's inference
    # form; measured on an MI355X: acc differs by 5.2e-6 between the paths at 8 E = 9.5e-7) the maps may differ by what their
    # float64 yardsticks differ by, and beyond that by no more than the two bounds together.
    pick = lambda out: (out[2], out[3]) if len(out) == 4 else (out[3], out[5])
    same_inputs = all(torch.equal(a, b) for a, b in zip(pick(out_s), pick(out_a)))
    print(f"  {kind}: densities and samples of the two paths are {'the same bits' if same_inputs else 'not the same bits'}")
    for name, got_s, got_a, (y_s, b_s), (y_a, b_a) in zip(("acc", "depth", "point"), m_s, m_a, ref_s, ref_a):
        if same_inputs:
            assert torch.equal(got_s, got_a), name
        gap = float(((got_a.detach().cpu().double() - got_s.cpu().double()) - (y_a - y_s)).abs().max())
        print(f"  {kind} launches - single call, {name}: {float((got_a.detach() - got_s).abs().max()):.2e}; beyond the yardsticks' own "
              f"difference {gap:.2e}, bound {b_s + b_a:.2e}")
        assert gap <= b_s + b_a, (name, gap, b_s, b_a)
    # t is the z-depth of the generated rays: inside the sample range (frame_batch: near 1, far 4)
    assert float(m_s.acc.min()) >= 0 and float(m_s.depth.min()) >= 0 and float(m_s.depth.max()) <= 4.0 * 1.001
    (m_a.depth.sum() + m_a.acc.sum()).backward()
    # (the maps are the fine compositing's: the coarse net only places the samples, which are detached, utils.py:260)
    nets = [pipe.model_fine] + ([pipe.model_warp_field] if kind == "smpl" else [])
    for net in nets:
        grads = [p.grad for p in net.parameters()]
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
        assert any(float(g.abs().max()) > 0 for g in grads)


def test_single_sample_pipeline_ray_maps(dev):
    """N == 1: acc = 1, depth = the parameter of the one sample on its ray, point = the sample."""
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import PipelineArgs, SingleSamplePipeline
    pipe = SingleSamplePipeline(_net(dev, syn.make_scene_nets(101)[0]), PipelineArgs(run_fine=0), PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    c = RR.make_case(5, 1, 19)
    o, d, sample = T(c["o"], dev), T(c["d"], dev), T(c["pts"][:, 0], dev)
    data = [sample, o, d, torch.zeros(5, 69, device=dev), 0.01 * torch.ones(5, 3, device=dev), torch.zeros(5, 3, device=dev)]
    with torch.no_grad():
        out = pipe(data)
        m = pipe.ray_maps(data, out)
    assert len(out) == 2 and torch.equal(m.acc, torch.ones(5, device=dev)) and torch.equal(m.point, sample)
    ones = torch.ones(5, 1)
    (_, d64, _), (_, d32, _) = [RR.ray_maps(ones.to(dt), c["o"].to(dt), c["d"].to(dt), pts=c["pts"].to(dt)) for dt in (torch.float64, torch.float32)]
    hold("single sample depth", m.depth, d64, d32)


def test_validate_maps_shapes(dev):
    from smpl_nerf_amd.trainer import DataParallelTrainer
    pipe = _pipeline(dev, "nerf")
    tr = DataParallelTrainer(pipe, [pipe.model_coarse, pipe.model_fine])
    frames = [_rays(dev, 64, "nerf"), _rays(dev, 64, "nerf")]
    loader = [[t[i:i + 32] for t in f] for f in frames for i in (0, 32)]
    maps = tr.validate_maps(loader, 8, 8)
    assert set(maps) == {"rgb", "depth", "acc"}
    assert maps["rgb"].shape == (2, 8, 8, 3) and maps["depth"].shape == (2, 8, 8) and maps["acc"].shape == (2, 8, 8)
    assert all(v.is_cuda and not v.requires_grad and bool(torch.isfinite(v).all()) for v in maps.values())
    assert torch.equal(maps["depth"][0], maps["depth"][1])
    with pytest.raises(ValueError):
        tr.validate_maps(loader[:1], 8, 8)


# ---- determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("z", "pts"))
def test_same_bits_twice_split_and_replayed(dev, mode):
    """Two calls, the batch split at rows 1 and 33, and a captured-graph replay on one stream: the same bits."""
    case = RR.make_case(67, 129, 23)
    whole = device_maps(case, mode, dev)
    again = device_maps(case, mode, dev)
    for a, b in zip(whole, again):
        assert a is None or torch.equal(a, b)
    parts = [device_maps({k: v[lo:hi] for k, v in case.items()}, mode, dev) for lo, hi in ((0, 1), (1, 33), (33, 67))]
    for i, a in enumerate(whole):
        assert a is None or torch.equal(a, torch.cat([p[i] for p in parts]))
    a = T(case["alpha"], dev)
    o, d = T(case["o"], dev), T(case["d"], dev)
    kw = dict(z_vals=T(case["z"], dev)) if mode == "z" else dict(samples=T(case["pts"], dev))
    lib = _lib.load()
    ga, gd = T(case["d_acc"], dev), T(case["d_depth"], dev)
    gp = T(case["d_point"], dev) if mode == "pts" else None
    d_alpha = torch.zeros_like(a)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream), torch.no_grad():
        ops.ray_maps(a, o, d, **kw)          # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            m = ops.ray_maps(a, o, d, **kw)
            _lib.check(lib.snerf_ray_maps_bwd_f32(_lib.ptr(a), _lib.ptr(kw.get("z_vals")), _lib.ptr(kw.get("samples")), _lib.ptr(o), _lib.ptr(d),
                                                  67, 129, _lib.ptr(ga), _lib.ptr(gd), _lib.ptr(gp), _lib.ptr(d_alpha),
                                                  _lib.current_stream()), "bwd")
        for t in (m.acc, m.depth, d_alpha):
            t.zero_()
        graph.replay()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert torch.equal(m.acc, whole[0]) and torch.equal(m.depth, whole[1]) and torch.equal(d_alpha, whole[3])
    if mode == "pts":
        assert torch.equal(m.point, whole[2])
