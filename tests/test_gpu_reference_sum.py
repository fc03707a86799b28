"""Strict mode on the device (snerf_reference_sum_f32, SNERF_REFERENCE_SUM): the reference's normalising sum computed by the
sampler itself - bit for bit torch's CPU sum, the fixture host's sample indices with no host round trip, and strict inference
and training through the single-call render and the one-call step."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from smpl_nerf_amd import _lib, ops
from smpl_nerf_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def no_host_sum(monkeypatch):
    """Strict mode must not fall back to the host round trip here."""
    assert ops.device_reference_sum_ok()

    def forbidden(*a, **k):
        raise AssertionError("strict mode took the host round trip")
    monkeypatch.setattr(ops, "_host_normalising_sum", forbidden)


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def test_device_entry_equals_torch_sum_bit_for_bit(dev):
    lib = _lib.load()
    rng = np.random.default_rng(11)
    lengths = list(range(0, 1101)) + [2047, 4096, 8191, 8192, 8193, 16384, 32767]
    for i, n in enumerate(lengths):
        B = 4096 if n in (1, 7, 8, 62, 63, 126, 190, 513, 1022) else (1, 3, 8, 37)[i % 4]
        stride = n + 1 + (i % 3)
        x = (10.0 ** rng.uniform(-3, 3, size=(B, stride))).astype(F32)
        if B > 4:
            x[1], x[2] = 0, F32(0.37)
            x[3, :] = 0
            x[3, 1::2] = F32(977.3)
        xd = T(x, dev)
        out = torch.full((B,), float("nan"), device=dev)
        for add in (0.0, 1e-5):
            assert lib.snerf_reference_sum_f32(xd.data_ptr(), stride, B, n, add, out.data_ptr(), _lib.current_stream()) == 0
            want = torch.sum(torch.from_numpy(x)[:, :n] + add, -1).numpy()
            assert np.array_equal(_bits(N(out)), _bits(want)), (n, B, add)


def test_strict_sampler_on_the_device_is_the_fixture_host_bit_for_bit(dev, no_host_sum):
    """g4 with no `tot`: inds, samples, merged depths and points equal the reference's for the main shape and the four extra
    shapes; the literal sample_pdf(bins, weights, strict_cumsum=1) equals the reference's samples."""
    g = load_golden("g4_sampler.npz")
    shapes = [("", 128)] + [(f"_{nc}_{nf}", nf) for nc, nf in ((16, 8), (32, 64), (64, 64), (48, 200))]
    for key, nf in shapes:
        u = g["u"][0] if key == "" else g["u" + key]
        ops._U_CACHE[(nf, str(dev))] = T(u, dev)
        try:
            r = ops.hierarchical_samples(T(g["o" + key], dev), T(g["d" + key], dev), T(g["z" + key], dev), T(g["w" + key], dev), nf,
                                         want_inds=True, want_samples=True, strict=True)
            if key == "":
                np.testing.assert_array_equal(N(r["inds"]), g["inds"])
                np.testing.assert_array_equal(N(r["z_samples"]), g["z_samples"])
                np.testing.assert_array_equal(N(r["z_fine"]), g["z_fine"])
                np.testing.assert_array_equal(N(r["pts"]), g["pts_fine"])
                z_mid = (F32(0.5) * (g["z"][:, 1:] + g["z"][:, :-1])).astype(F32)
                zs = ops.sample_pdf(T(z_mid, dev), T(g["w"][:, 1:-1], dev), _Args(number_fine_samples=128, strict_cumsum=1))
                np.testing.assert_array_equal(N(zs), g["z_samples"])
            else:
                np.testing.assert_array_equal(N(r["z_fine"]), g["zf" + key])
                np.testing.assert_array_equal(N(r["pts"]), g["pf" + key])
        finally:
            ops._U_CACHE.pop((nf, str(dev)), None)


class _Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_strict_sample_pdf_backward_uses_the_device_sum(dev, monkeypatch):
    """The autograd sample_pdf in strict mode: values and gradients equal those of the host-supplied sum."""
    g = load_golden("g16_sample_pdf_grad.npz")
    runs = []
    for device_sum in (True, False):
        monkeypatch.setattr(ops, "_REFSUM_OK", None if device_sum else False)
        bins = T(g["bins"], dev).requires_grad_(True)
        w = T(g["weights"], dev).requires_grad_(True)
        out = ops.sample_pdf(bins, w, _Args(number_fine_samples=128, strict_cumsum=1))
        (out * T(g["gout"], dev)).sum().backward()
        runs.append((N(out), N(bins.grad), N(w.grad)))
    np.testing.assert_array_equal(runs[0][0], g["samples"])
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------ single-call strict render
def _net(dev, params, n_add=0):
    from smpl_nerf_amd.nets import RenderRayNet
    m = RenderRayNet(8, 256, 60, 24, n_add, skips=[4]) if n_add else RenderRayNet(8, 256, 60, 24, skips=[4])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.to(dev)


def _pipeline(kind, dev, prec):
    from smpl_nerf_amd.nets import WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder as PE
    from smpl_nerf_amd.pipelines import AppendSmplParamsPipeline, NerfPipeline, PipelineArgs, SmplNerfPipeline
    args = PipelineArgs(strict_cumsum=1)
    if kind == "nerf":
        pc, pf = syn.make_scene_nets(101)
        pipe = NerfPipeline(_net(dev, pc), _net(dev, pf), args, PE(10, 0), PE(4, 0))
    elif kind == "smpl":
        pc, pf = syn.make_scene_nets(101)
        mw = WarpFieldNet(8, 256, 60, 40)
        mw.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_warp_field_params(103, out_scale=0.3).items()})
        pipe = SmplNerfPipeline(_net(dev, pc), _net(dev, pf), mw.to(dev), args, PE(10, 0), PE(4, 0), PE(10, 0))
    else:
        args.human_pose_encoding = 0
        nets = [_net(dev, syn.make_scene_net_params(s, add_first=True, additional_input_dim=69), 69) for s in (301, 303)]
        pipe = AppendSmplParamsPipeline(nets[0], nets[1], args, PE(10, 0), PE(4, 0), PE(10, 0))
    return pipe.set_precision(prec).eval()


def _data(kind, dev, n_rays, seed=11):
    data = syn.frame_batch(128, 128, phi=3.0, theta=-10.0, seed=seed)
    sub = np.arange(0, 16384, 16384 // n_rays)[:n_rays]
    d = [T(a[sub], dev) for a in data[:4]]
    if kind == "nerf":
        return d + [T(data[4][sub], dev)]
    pose = T(syn.human_poses()[np.arange(n_rays) % 10].astype(F32), dev)
    return d + [pose, T(data[4][sub], dev)]


def _cpu_sample_pdf(bins, weights, nf):
    """utils.py:194-228 on the CPU with torch's own kernels (torch.searchsorted for the torchsearchsorted extension)."""
    weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = torch.linspace(0., 1., steps=nf).expand(list(cdf.shape[:-1]) + [nf]).contiguous()
    inds = torch.searchsorted(cdf.contiguous(), u, right=True)
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)
    g = torch.stack([below, above], -1)
    shape = [g.shape[0], g.shape[1], cdf.shape[-1]]
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(shape), 2, g)
    bins_g = torch.gather(bins.unsqueeze(1).expand(shape), 2, g)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_g[..., 0]) / denom
    return bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])


@pytest.mark.parametrize("prec", ["fp32", "bf16x6"])
@pytest.mark.parametrize("kind", ["nerf", "smpl", "append"])
def test_strict_inference_is_one_call_and_equals_the_five_call_forward(dev, kind, prec, no_host_sum):
    pipe = _pipeline(kind, dev, prec)
    data = _data(kind, dev, 256)
    with torch.no_grad():
        assert pipe._single_call_ok(data)
        calls = _lib.CALLS
        one = pipe(data)
        assert _lib.CALLS - calls == 1
        five = pipe._forward_calls(data)
    torch.cuda.synchronize()
    assert len(one) == len(five)
    for a, b in zip(one, five):
        assert torch.equal(a, b)
    if kind != "nerf":
        return
    # the fine samples are o + d * sort(cat(z, S)) with S torch's CPU sample_pdf of the device's own coarse weights
    x, o, d, z, _ = data
    B, Nc = z.shape
    with torch.no_grad():
        raw = pipe.model_coarse.forward_fused(x, d, Nc, pipe.position_encoder, pipe.direction_encoder)
        _, w, _ = ops.composite(raw.view(B, Nc, 4), z, d, False)
    zc, wc, oc, dc = (t.cpu() for t in (z, w, o, d))
    S = _cpu_sample_pdf(0.5 * (zc[..., 1:] + zc[..., :-1]), wc[..., 1:-1], 128)
    zf, _ = torch.sort(torch.cat([zc, S], -1), -1)
    pts = oc[..., None, :] + dc[..., None, :] * zf[..., :, None]
    assert torch.equal(one[2].cpu(), pts)


def test_the_flag_reaches_the_kernel(dev):
    """A 16 384-ray frame: strict and default single-call renders sample some ray differently (the two sums differ by an ulp
    in about half the rows)."""
    pipe = _pipeline("nerf", dev, "fp32")
    data = _data("nerf", dev, 16384, seed=5)
    with torch.no_grad():
        strict = pipe(data)[2]
        pipe.args.strict_cumsum = 0
        default = pipe(data)[2]
    assert not torch.equal(strict, default)


# ------------------------------------------------------------------------------------------ one-call strict training
def _trainer(kind, dev, one_call, lr=1e-3):
    from smpl_nerf_amd.trainer import DataParallelTrainer
    pipe = _pipeline(kind, dev, "fp32").train()
    models = [pipe.model_coarse, pipe.model_fine] + ([pipe.model_warp_field] if kind == "smpl" else [])
    return DataParallelTrainer(pipe, models, lr=lr, one_call=one_call), pipe


@pytest.mark.parametrize("kind", ["nerf", "smpl"])
def test_strict_one_call_step_equals_the_strict_autograd_step(dev, kind, no_host_sum):
    runs = []
    for one_call in (None, False):
        tr, pipe = _trainer(kind, dev, one_call)
        tr.rays_per_chunk = 0
        batch = _data(kind, dev, 192 if kind == "nerf" else 100)
        took = []
        real = tr._step_one_call
        tr._step_one_call = lambda *a: (took.append(1), real(*a))[1]
        steps = 3 if kind == "nerf" else 2
        losses = [float(tr.step(batch)) for _ in range(steps)]
        assert (len(took) == steps) == (one_call is None)
        runs.append((losses, [p.detach().clone() for p in tr.params]))
    # (the tolerances of test_one_call_step_equals_the_autograd_step / test_smpl_nerf_one_call_step_equals_the_autograd_step)
    np.testing.assert_allclose(runs[0][0][:1], runs[1][0][:1], rtol=2e-6, atol=1e-8)
    np.testing.assert_allclose(runs[0][0][1:], runs[1][0][1:], rtol=2e-6 if kind == "nerf" else 2e-4, atol=1e-8)
    for pa, pb in zip(runs[0][1], runs[1][1]):
        assert float((pa - pb).abs().max()) <= (2e-5 if kind == "nerf" else 3e-4)


def test_strict_one_call_step_in_a_hip_graph(dev, no_host_sum):
    tr, _ = _trainer("nerf", dev, None)
    eager, _ = _trainer("nerf", dev, None)
    batch = _data("nerf", dev, 64)
    for _ in range(2):
        tr.step(batch), eager.step(batch)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tr.step(batch)
        eager.step(batch)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        loss = tr.step(batch)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    for _ in range(3):
        want = eager.step(batch)
    assert float(loss) == float(want)
    for a, b in zip(tr.params, eager.params):
        assert torch.equal(a, b)
