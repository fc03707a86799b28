"""Round-4 GPU parity: the per-batch body of NerfSolver.train (solver/nerf_solver.py:76-87) as one C-ABI call
(snerf_nerf_train_step_f32 / _grads_f32 + snerf_adam_step_f32, include/smplnerf.h) against the reference's fixtures (g7: three
Adam steps of the reference; g15 runs through the same entry in test_gpu_round3.py), against torch.optim.Adam, and against
the autograd form of the same step."""
import ctypes

import numpy as np
import pytest
import torch

import torch_ref as R
from oracle import nerf_oracle as O
from smpl_nerf_amd import _lib
from smpl_nerf_amd import synthetic as syn
from conftest import load_golden

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "bf16x6", "f16x3"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def _net(dev, params, precision="fp32", **kw):
    from smpl_nerf_amd.nets import RenderRayNet
    net = RenderRayNet(kw.get("n_layers", 8), kw.get("width", 256), 60, 24, skips=list(kw.get("skips", (4,))))
    if params is not None:
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net.precision = precision
    return net.to(dev).train()


def _trainer(dev, prec="fp32", one_call=None, lr=5e-4, weight_decay=0.0, **args_kw):
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs
    from smpl_nerf_amd.trainer import DataParallelTrainer
    pc, pf = syn.make_scene_nets(101)
    mc, mf = _net(dev, pc, prec), _net(dev, pf, prec)
    pipe = NerfPipeline(mc, mf, PipelineArgs(**args_kw), PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    tr = DataParallelTrainer(pipe, [mc, mf], lr=lr, weight_decay=weight_decay, one_call=one_call)
    return tr, pipe, mc, mf


def _batch(dev, n=256, seed=7, stride=None):
    data = syn.frame_batch(128, 128, seed=seed)
    sub = np.arange(0, 16384, stride or (16384 // n))[:n]
    return [T(a[sub], dev) for a in data]


# ------------------------------------------------------------------------------------------ slot tables
@pytest.mark.parametrize("shape", [dict(), dict(n_layers=4, width=128, skips=(1,)), dict(n_layers=2, width=100, skips=()),
                                   dict(n_layers=8, width=64, skips=(2, 5))])
def test_stream_slot_tables_point_at_every_parameter(dev, shape):
    """snerf_mlp_stream_slots: packed[slot_fwd[i]] and packed_t[slot_t[i]] hold parameter i after a pack; every weight and
    bias sits in the forward stream exactly once; the streams hold nothing else (their other floats are zero padding)."""
    lib = _lib.load()
    net = _net(dev, None, **shape)
    from smpl_nerf_amd.ops import PositionalEncoder
    desc = net.desc_for_encoders(PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    n = int(lib.snerf_mlp_param_floats(desc))
    g = torch.Generator(device="cpu").manual_seed(3)
    flat = (torch.rand(n, generator=g) + 0.5).to(dev)                 # no zeros: padding is recognisable
    packed = torch.empty(int(lib.snerf_mlp_packed_floats(desc)), device=dev)
    nt = ctypes.c_int64()
    _lib.check(lib.snerf_mlp_train_sizes(desc, 0, None, None, ctypes.byref(nt), None, None), "sizes")
    packed_t = torch.zeros(nt.value, device=dev)     # (sized for the input-gradient stream; this one is shorter)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.snerf_mlp_pack_f32(desc, flat.data_ptr(), packed.data_ptr(), s), "pack")
    _lib.check(lib.snerf_mlp_pack_t_f32(desc, flat.data_ptr(), packed_t.data_ptr(), 0, s), "pack_t")
    sf = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(lib.snerf_mlp_stream_slots(desc, sf.data_ptr(), st.data_ptr(), 0, s), "slots")
    sf, st = sf.long(), st.long()
    assert int(sf.min()) >= 0 and int(sf.unique().numel()) == n       # every parameter, each at its own float
    assert torch.equal(packed[sf], flat)
    assert int((packed != 0).sum()) == n
    has = st >= 0
    assert torch.equal(packed_t[st[has]], flat[has])
    assert int((packed_t[: nt.value] != 0).sum()) == int(has.sum()) == int(st[has].unique().numel())
    # biases never enter the transposed stream; the hidden-column weights and the sigma head do
    off = 0
    for p in net._ordered_params():
        if p.dim() == 1:
            assert not bool(has[off:off + p.numel()].any())
        off += p.numel()
    assert int(has.sum()) > 0


# ------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_hip_adam_follows_torch_adam(dev, wd):
    """snerf_adam_step_f32 against torch.optim.Adam on the CPU (the reference's optimiser, solver/nerf_solver.py:31-33): the
    same statements in the same order - parameters and both moments agree to fp32 round-off over several steps, the weight
    streams are refreshed in place bit for bit, a checkpoint moves between the two optimisers, and a parameter without a
    gradient is skipped (its step count does not advance) like torch skips it."""
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.trainer import HipAdam, flatten_parameters_
    lib = _lib.load()
    torch.manual_seed(5)
    net = _net(dev, None)
    extra = torch.nn.Linear(7, 5).to(dev)                       # a second module: parameters outside any weight stream
    flat_p, flat_g, segments, order = flatten_parameters_([net, extra])
    views, off = [], 0
    for p in order:
        views.append(flat_g[off:off + p.numel()].view(p.shape))
        off += p.numel()
    opt = HipAdam(order, flat_p, flat_g, views, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ref_params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in order]
    ref = torch.optim.Adam(ref_params, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    desc = net.desc_for_encoders(PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    packed, packed_t = net.packed_weights(desc, training=True), net.packed_weights_t(desc, False)
    n = int(lib.snerf_mlp_param_floats(desc))
    sf, st = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    _lib.check(lib.snerf_mlp_stream_slots(desc, sf.data_ptr(), st.data_ptr(), 0, torch.cuda.current_stream().cuda_stream), "slots")
    nets = (_lib.AdamNet * 1)(_lib.AdamNet(ctypes.pointer(desc), segments[0][1], 0, packed.data_ptr(), packed_t.data_ptr(),
                                           sf.data_ptr(), st.data_ptr()))
    gen = torch.Generator().manual_seed(11)
    for step in range(6):
        skip_extra = step in (1, 2)                               # `extra` has no gradient on two of the steps
        for p, q in zip(order, ref_params):
            if skip_extra and any(p is e for e in extra.parameters()):
                p.grad, q.grad = None, None
                continue
            gcpu = torch.randn(p.shape, generator=gen) * (10.0 ** float(torch.randint(-4, 1, (1,), generator=gen)))
            p.grad, q.grad = gcpu.to(dev), gcpu.clone()
        opt.step(nets, 1)
        ref.step()
    torch.cuda.synchronize()
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert sorted(sd["state"]) == sorted(rsd["state"])
    n_par = n_diff = 0
    for i in sd["state"]:
        assert float(sd["state"][i]["step"]) == float(rsd["state"][i]["step"])
        # both moments bit for bit (the kernel fuses the multiply-adds torch's CPU kernels fuse) ...
        for key in ("exp_avg", "exp_avg_sq"):
            a, b = sd["state"][i][key].cpu().numpy(), rsd["state"][i][key].numpy()
            if wd == 0.0:
                assert np.array_equal(a, b), key
            else:       # (the decayed gradient reads the parameters, which differ in the last place here and there)
                close(a, b, 1e-6, 1e-9 if key == "exp_avg" else 1e-12)
    # ... and the parameters to the last place: torch's CPU `sqrt` is a vectorised routine that is not correctly rounded on
    # every host (0.65 % of the square roots differ from IEEE sqrt in the build container, 1.4 % on the GPU box's host), so a
    # percent of the elements per step land one unit in the last place apart - host-dependent, not reproducible by any kernel
    for p, q in zip(order, ref_params):
        a, b = p.detach().cpu().numpy(), q.detach().numpy()
        close(a, b, 1e-6, 6e-8)
        n_par += a.size
        n_diff += int((a != b).sum())
    assert n_diff <= 0.15 * n_par, (n_diff, n_par)
    assert int(opt.steps[len(order) - 1]) == 4 and int(opt.steps[0]) == 6
    # the streams were refreshed in place: equal to a fresh pack of the new parameters
    fresh, fresh_t = torch.empty_like(packed), torch.empty_like(packed_t)
    s = torch.cuda.current_stream().cuda_stream
    seg = flat_p[segments[0][1]:segments[0][1] + n]
    _lib.check(lib.snerf_mlp_pack_f32(desc, seg.data_ptr(), fresh.data_ptr(), s), "pack")
    _lib.check(lib.snerf_mlp_pack_t_f32(desc, seg.data_ptr(), fresh_t.data_ptr(), 0, s), "pack_t")
    used_t = int(st.max()) + 1          # (the buffer is sized for the longer input-gradient stream: its tail is never written)
    assert torch.equal(packed, fresh) and torch.equal(packed_t[:used_t], fresh_t[:used_t])
    # checkpoints move between the optimisers (torch's own state_dict format)
    ref2 = torch.optim.Adam([torch.nn.Parameter(q.detach().clone()) for q in ref_params], lr=1.0)
    ref2.load_state_dict(sd)
    assert ref2.param_groups[0]["lr"] == 3e-3 and float(ref2.state[ref2.param_groups[0]["params"][0]]["step"]) == 6.0
    opt2 = HipAdam(order, flat_p, flat_g, views)
    opt2.load_state_dict(rsd)
    assert torch.equal(opt2.steps.cpu(), opt.steps.cpu()) and opt2.param_groups[0]["lr"] == 3e-3
    close(opt2.exp_avg.cpu().numpy(), opt.exp_avg.cpu().numpy(), 2e-6, 1e-12)


# ------------------------------------------------------------------------------------------ the one-call step
@pytest.mark.parametrize("prec", PRECISIONS)
def test_one_call_step_matches_the_reference_three_adam_steps(dev, prec):
    """g7 (the reference's NerfSolver body: forward, MSE coarse + fine, backward, Adam, three times) through
    DataParallelTrainer.step = snerf_nerf_train_step_f32: losses, first-step gradients, parameters after three steps."""
    g7 = load_golden("g7_grads.npz")
    tr, pipe, mc, mf = _trainer(dev, prec)
    data = syn.frame_batch(128, 128, seed=7)
    batch = [T(a[g7["t_sub"]], dev) for a in data]
    assert tr._one_call_state() is not None
    losses = []
    for step in range(3):
        losses.append(float(tr.step(batch)))
        if step == 0:
            close(tr.last_outputs[0].cpu().numpy(), g7["t_rgb0"], 0, 1e-5)
            close(tr.last_outputs[1].cpu().numpy(), g7["t_rgb_fine0"], 0, 1e-4)
            for name, m in (("coarse", mc), ("fine", mf)):
                for k, p in m.named_parameters():
                    ref = g7[f"t_grad0/{name}.{k}"]
                    scale = max(np.abs(ref[2:]).max(), ref[1] / np.sqrt(p.numel()), 1e-12)
                    close(R.digest(p.grad), ref, 5e-3, 2e-3 * scale)
    close(losses, g7["t_losses"], 1e-4, 1e-6)
    for name, m in (("coarse", mc), ("fine", mf)):
        for k, p in m.named_parameters():
            close(R.digest(p)[2:], g7[f"t_param3/{name}.{k}"][2:], 0, 3e-4)
    # inference after the steps reads the streams the optimiser kept current: equal to a net built from the new parameters
    with torch.no_grad():
        out = pipe(batch)
        mc2, mf2 = _net(dev, None, prec), _net(dev, None, prec)
        mc2.load_state_dict(mc.state_dict()), mf2.load_state_dict(mf.state_dict())
        from smpl_nerf_amd.pipelines import NerfPipeline
        out2 = NerfPipeline(mc2, mf2, pipe.args, pipe.position_encoder, pipe.direction_encoder)(batch)
    assert torch.equal(out[0], out2[0]) and torch.equal(out[1], out2[1])


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", [dict(), dict(white_background=1), dict(sigma_noise_std=1.0)])
def test_one_call_step_equals_the_autograd_step(dev, prec, cfg):
    """The same three steps through (a) one call and (b) the autograd form (HIP forward / backward through
    torch.autograd.Function, torch's MSE, the same HipAdam): with one chunk the kernels and their order are the same, so
    losses, gradients and parameters agree to round-off of the loss gradient."""
    runs = []
    for one_call in (None, False):
        tr, pipe, mc, mf = _trainer(dev, prec, one_call=one_call, lr=1e-3, **cfg)
        tr.rays_per_chunk = 0
        batch = _batch(dev, 192)
        torch.manual_seed(9)                      # sigma noise: same draws in both forms (coarse first, then fine)
        losses = [float(tr.step(batch)) for _ in range(3)]
        runs.append((losses, [p.grad.clone() for p in tr.params], [p.detach().clone() for p in tr.params]))
        assert (tr._one_call_state() is not None) == (one_call is None)
    close(runs[0][0], runs[1][0], 2e-6, 1e-8)
    # r06: the one-call step of a small batch splits its weight-gradient jobs for each net's share of the chip (the coarse net's
    # backward runs beside the fine net's), the autograd form's launches each split for the whole chip: the same sums in another
    # order.  A tensor whose gradient is a near-total cancellation (white background: the last layers of the coarse net, norm 1e-9
    # against 1e-2 for the others) carries that round-off at full size - hence the term relative to the largest tensor.
    top = max(float(gb.norm()) for gb in runs[1][1])
    for ga, gb in zip(runs[0][1], runs[1][1]):
        assert float((ga - gb).norm()) <= 2e-5 * float(gb.norm()) + 1e-7 * top + 1e-12
    for pa, pb in zip(runs[0][2], runs[1][2]):
        assert float((pa - pb).abs().max()) <= 2e-5


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_ray_chunks_sum_to_the_whole_batch(dev, prec):
    """rays_per_chunk: forward + backward chunk by chunk (ragged last chunk) gives the gradient of the whole batch up to the
    order of the fp32 sums; loss and rendered colours are those of the single-chunk step."""
    lib = _lib.load()
    res = []
    for chunk in (0, 100, 64):
        tr, pipe, mc, mf = _trainer(dev, prec)
        tr.rays_per_chunk = chunk
        batch = _batch(dev, 250, stride=37)
        loss = float(tr.step(batch))
        res.append((loss, tr._flat_g.clone(), tr.last_outputs[0].clone(), tr.last_outputs[1].clone(), tr._oc["ws"].numel()))
    for loss, g, rc, rf, _ in res[1:]:
        close([loss], [res[0][0]], 1e-6, 0)
        assert torch.equal(rc, res[0][2]) and torch.equal(rf, res[0][3])
        assert float((g - res[0][1]).norm()) <= 2e-5 * float(res[0][1].norm())
    assert res[2][4] < res[1][4] < res[0][4]          # the workspace is sized by the chunk
    d = mc.desc_for_encoders(pipe.position_encoder, pipe.direction_encoder)
    assert lib.snerf_nerf_train_workspace_bytes(d, d, 250, 64, 128, 64) == res[2][4]


def test_one_call_step_with_run_fine_0(dev):
    """Q10: run_fine = 0 - loss = 2 MSE(rgb), the fine net gets no gradient, is not updated and its step counters stay 0
    (torch.optim.Adam skips parameters whose .grad is None)."""
    g7 = load_golden("g7_grads.npz")
    tr, pipe, mc, mf = _trainer(dev, run_fine=0)
    data = syn.frame_batch(128, 128, seed=7)
    batch = [T(a[g7["t_sub"]], dev) for a in data]
    before = [p.detach().clone() for p in mf.parameters()]
    loss = tr.step(batch)
    close([float(loss)], g7["t_coarse_only_loss"], 1e-5, 1e-7)
    assert all(p.grad is None for p in mf.parameters()) and all(p.grad is not None for p in mc.parameters())
    assert all(torch.equal(a, b) for a, b in zip(before, mf.parameters()))
    assert torch.equal(tr.last_outputs[0], tr.last_outputs[1])
    steps = tr.optim.steps.cpu().tolist()
    index = {id(p): i for i, p in enumerate(tr.params)}
    assert all(steps[index[id(p)]] == 1 for p in mc.parameters()) and all(steps[index[id(p)]] == 0 for p in mf.parameters())
    for k, p in mc.named_parameters():
        ref = g7[f"t_coarse_only_grad/coarse.{k}"] if f"t_coarse_only_grad/coarse.{k}" in g7 else None
        if ref is not None:
            scale = max(np.abs(ref[2:]).max(), ref[1] / np.sqrt(p.numel()), 1e-12)
            close(R.digest(p.grad), ref, 5e-3, 2e-3 * scale)
    # the fine net joins later: its first update is torch's first update (step count 1 for it, 3 for the coarse net)
    pipe.args.run_fine = 1
    tr.step(batch), tr.step(batch)
    steps = tr.optim.steps.cpu().tolist()
    assert all(steps[index[id(p)]] == 3 for p in mc.parameters()) and all(steps[index[id(p)]] == 2 for p in mf.parameters())


def test_one_call_step_in_a_hip_graph(dev):
    """The one-call step allocates nothing inside the library, never synchronises and keeps its step counter on the device:
    captured into a graph (torch.cuda.graph drives hipStreamBeginCapture on the stream the library launches on) and
    replayed, it walks the same trajectory as eager steps."""
    tr, pipe, mc, mf = _trainer(dev)
    batch = _batch(dev, 64)         # (a batch small enough for the coarse backward to run on the auxiliary stream: fork / join are captured too)
    eager, _, emc, emf = _trainer(dev)
    for _ in range(2):
        tr.step(batch), eager.step(batch)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tr.step(batch)                                # warm-up on the capture stream
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
    # (capture itself does not execute: 2 + 1 + 3 replays = 6 steps on both sides)
    assert float(loss) == float(want)
    for a, b in zip(tr.params, eager.params):
        assert torch.equal(a, b)
    assert int(tr.optim.steps[0]) == 6


@pytest.mark.parametrize("rays", [64, 800])
@pytest.mark.parametrize("prec", ["fp32", "bf16x6"])
def test_small_batches_run_the_coarse_backward_on_the_auxiliary_stream(dev, prec, rays, monkeypatch):
    """Chunks of <= 262 144 samples (up to 1024 rays; the README's 64-ray batches): the coarse net's backward runs beside the fine net's on
    the trainer's second stream (include/smplnerf.h: aux_stream) - the same kernels on their own scratch buffers, so the
    trajectory equals the single-stream one bit for bit."""
    lib = _lib.load()
    finals = []
    for aux in ("1", "0"):
        monkeypatch.setenv("SNERF_TRAIN_AUX_STREAM", aux)
        tr, pipe, mc, mf = _trainer(dev, prec, lr=1e-3)
        batch = _batch(dev, rays)
        losses = [float(tr.step(batch)) for _ in range(4)]
        assert (tr._oc["aux"] is not None) == (aux == "1")
        finals.append((losses, [p.detach().clone() for p in tr.params]))
    assert finals[0][0] == finals[1][0] and finals[0][0][3] < finals[0][0][0]
    for a, b in zip(finals[0][1], finals[1][1]):
        assert torch.equal(a, b)
    d = mc.desc_for_encoders(pipe.position_encoder, pipe.direction_encoder)
    # the second set of backward scratch buffers exists only where the concurrent form applies (a pure size rule)
    assert lib.snerf_nerf_train_workspace_bytes(d, d, 64, 64, 128, 0) > 64 * lib.snerf_nerf_train_workspace_bytes(d, d, 4096, 64, 128, 0) // 4096


def test_trainer_falls_back_to_autograd_where_the_one_call_step_does_not_apply(dev):
    """A custom loss, a frozen parameter or a pipeline other than NerfPipeline take the autograd path (same optimiser)."""
    from smpl_nerf_amd.trainer import DataParallelTrainer, HipAdam
    tr, pipe, mc, mf = _trainer(dev)
    assert isinstance(tr.optim, HipAdam) and tr._one_call_state() is not None
    tr2 = DataParallelTrainer(pipe, [mc, mf], loss_func=torch.nn.L1Loss())
    assert tr2._one_call_state() is None
    batch = _batch(dev, 64)
    l0 = float(tr2.step(batch))
    l1 = float(tr2.step(batch))
    assert np.isfinite(l0) and l1 < l0


def test_shuffled_epochs_visit_every_ray_once(dev):
    """RayBatchLoader(shuffle=True) = DataLoader(shuffle=True) of train.py:100: one epoch is a permutation of the rank's rays."""
    from smpl_nerf_amd.raygen import RayGenerator
    from smpl_nerf_amd.trainer import RayBatchLoader
    poses = np.stack([syn.sphere_pose(10.0 * i, 5.0 * i, 2.4) for i in range(3)])
    h = w = 16
    images = np.random.default_rng(0).random((3, h, w, 3)).astype(np.float32)
    gen = RayGenerator(poses, h, w, np.pi / 3, 1.0, 4.0, 64, dev, images=images)
    loader = RayBatchLoader(gen, 100, seed=3, shuffle=True)
    assert len(loader) == 8                                   # 768 rays: 7 full batches + one of 68
    seen = []
    for epoch in range(2):
        truth = torch.cat([b[-1] for b in loader])
        sizes = [b[0].shape[0] for b in loader]
        assert sizes[:-1] == [100] * 7 and sizes[-1] == 68
        # every pixel of every frame exactly once (pixels are distinct random triples)
        a = np.sort(truth.cpu().numpy().view([("", np.float32)] * 3).ravel())
        b = np.sort(images.reshape(-1, 3).view([("", np.float32)] * 3).ravel())
        assert np.array_equal(a, b)
        seen.append(truth)
    assert not torch.equal(seen[0], seen[1])                  # a new permutation per epoch
    assert len(RayBatchLoader(gen, 100, iterations=3, shuffle=True)) == 3
    with pytest.raises(ValueError):
        RayGenerator.for_rank(poses, h, w, np.pi / 3, 1.0, 4.0, 64, dev, world=4, rank=3)


# ------------------------------------------------------------------------------------------ fold workspaces (b-2 boundary)
def test_per_ray_fold_tables_live_in_the_callers_workspace(dev):
    """the library allocates nothing.  snerf_mlp_fwd_ws_f32 / snerf_warp_fwd_ws_f32 take the per-ray fold
    table as a caller workspace of snerf_*_fold_workspace_bytes bytes: exactly that many bytes are written (guard bands), NULL
    is the per-sample form (= snerf_mlp_fwd_f32 / snerf_warp_fwd_f32, same values up to the summation order of the folded
    columns), a workspace that is too small is an error and not a silent switch of form."""
    from smpl_nerf_amd.nets import RenderRayNet, WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(3)
    rays, spr = 37, 24
    n = rays * spr
    x = (torch.rand(n, 3, device=dev) - 0.5) * 3
    d = torch.randn(rays, 3, device=dev)
    net = RenderRayNet(8, 256, 60, 24, additional_input_dim=69, skips=[4]).to(dev)
    desc = net.desc_for_encoders(PositionalEncoder(10, 0), PositionalEncoder(4, 0), add_first=True)
    add = torch.randn(rays, 69, device=dev)
    packed = net.packed_weights(desc)
    need = int(lib.snerf_mlp_fold_workspace_bytes(desc, n, spr))
    assert need == rays * 2 * 256 * 4                             # layer 0 and the skip layer: one 256-vector per ray each
    assert lib.snerf_mlp_fold_workspace_bytes(desc, rays * 4, 4) == 0          # fewer than 8 samples per ray: no fold
    plain_desc = RenderRayNet(8, 256, 60, 24, skips=[4]).desc_for_encoders(PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    assert lib.snerf_mlp_fold_workspace_bytes(plain_desc, n, spr) == 0         # no additional inputs: nothing to fold
    band = 1024
    buf = torch.full((need + 2 * band,), 0xA5, dtype=torch.uint8, device=dev)
    raw_ws, raw_plain, raw_nofold = (torch.zeros(n, 4, device=dev) for _ in range(3))
    args = (desc, packed.data_ptr(), x.data_ptr(), d.data_ptr())
    _lib.check(lib.snerf_mlp_fwd_ws_f32(*args, 0, add.data_ptr(), n, spr, raw_ws.data_ptr(), buf.data_ptr() + band, need, s), "ws")
    _lib.check(lib.snerf_mlp_fwd_f32(*args, 0, add.data_ptr(), n, spr, raw_plain.data_ptr(), s), "plain")
    _lib.check(lib.snerf_mlp_fwd_ws_f32(*args, 2, add.data_ptr(), n, spr, raw_nofold.data_ptr(), buf.data_ptr() + band, need, s), "nofold")
    torch.cuda.synchronize()
    assert bool((buf[:band] == 0xA5).all()) and bool((buf[band + need:] == 0xA5).all())
    assert not bool((buf[band:band + need] == 0xA5).all())        # the table was written there
    assert torch.equal(raw_plain, raw_nofold)                     # SNERF_FWD_NO_RAY_FOLD: the per-sample form even with a workspace
    scale = float(raw_plain.abs().max())
    assert 0 < float((raw_ws - raw_plain).abs().max()) <= 2e-5 * scale
    untouched = torch.full((n, 4), 7.0, device=dev)
    rc = lib.snerf_mlp_fwd_ws_f32(*args, 0, add.data_ptr(), n, spr, untouched.data_ptr(), buf.data_ptr() + band, need - 4, s)
    assert rc == -1 and b"snerf_mlp_fold_workspace_bytes" in lib.snerf_last_error_string()
    assert lib.snerf_mlp_fwd_ws_f32(*args, 4, add.data_ptr(), n, spr, untouched.data_ptr(), None, 0, s) == -1   # unknown bit
    torch.cuda.synchronize()
    assert bool((untouched == 7.0).all())
    # the warp net: one 256-vector per ray
    mw = WarpFieldNet(8, 256, 60, 40).to(dev)
    wdesc = _lib.WarpDesc(256, 10, 0, 40)
    wpacked = mw._packed(wdesc)
    pose = torch.randn(rays, 40, device=dev)
    o = torch.randn(rays, 3, device=dev)
    wneed = int(lib.snerf_warp_fold_workspace_bytes(wdesc, n, spr))
    assert wneed == rays * 256 * 4
    wbuf = torch.full((wneed + 2 * band,), 0xA5, dtype=torch.uint8, device=dev)
    outs = [[torch.zeros(n, 3, device=dev) for _ in range(3)] for _ in range(2)]
    wargs = (wdesc, wpacked.data_ptr(), x.data_ptr(), pose.data_ptr(), o.data_ptr(), n, spr)
    _lib.check(lib.snerf_warp_fwd_ws_f32(*wargs, *[t.data_ptr() for t in outs[0]], wbuf.data_ptr() + band, wneed, s), "warp ws")
    _lib.check(lib.snerf_warp_fwd_f32(*wargs, *[t.data_ptr() for t in outs[1]], s), "warp plain")
    torch.cuda.synchronize()
    assert bool((wbuf[:band] == 0xA5).all()) and bool((wbuf[band + wneed:] == 0xA5).all())
    for a, b in zip(*outs):
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))
    rc = lib.snerf_warp_fwd_ws_f32(*wargs, *[t.data_ptr() for t in outs[0]], wbuf.data_ptr() + band, wneed - 4, s)
    assert rc == -1 and b"snerf_warp_fold_workspace_bytes" in lib.snerf_last_error_string()


def test_c_host_training_example(dev, tmp_path):
    """examples/c_host/train_steps.c - plain C99, the C-ABI plus the HIP runtime, no Python in the process - runs the same
    optimisation steps as DataParallelTrainer.step (ray chunks included): losses and final parameters bit for bit."""
    import os
    import shutil
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not shutil.which("gcc") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc / ROCm headers not available")
    exe = str(tmp_path / "train_steps")
    lib = os.path.join(root, "smpl_nerf_amd", "csrc", "libsmplnerf_hip.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "c_host", "train_steps.c"), lib,
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe],
                   check=True)
    from smpl_nerf_amd.ops import uniform_u
    steps, chunk, lr = 4, 100, 1e-3
    tr, pipe, mc, mf = _trainer(dev, lr=lr)
    tr.rays_per_chunk = chunk
    batch = _batch(dev, 250, stride=37)
    B, Nc, Nf = batch[3].shape[0], batch[3].shape[1], 128
    blob = struct.pack("<5id", 0x534e5254, B, Nc, Nf, 0, lr)
    for m in (mc, mf):
        blob += bytes(m.desc_for_encoders(pipe.position_encoder, pipe.direction_encoder, False))
    for m in (mc, mf):
        blob += torch.cat([p.detach().reshape(-1) for p in m._ordered_params()]).cpu().numpy().tobytes()
    for t in batch:
        blob += t.cpu().numpy().astype(np.float32).tobytes()
    blob += uniform_u(Nf, dev).cpu().numpy().astype(np.float32).tobytes()
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(blob)
    r = subprocess.run([exe, str(fin), str(fout), str(steps), str(chunk)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(fout.read_bytes(), dtype=np.float32)
    losses = [float(tr.step(batch)) for _ in range(steps)]
    want = np.concatenate([np.asarray(losses, np.float32)] +
                          [torch.cat([p.detach().reshape(-1) for p in m._ordered_params()]).cpu().numpy() for m in (mc, mf)])
    assert got.shape == want.shape and np.array_equal(got[:steps], want[:steps]) and losses[-1] < losses[0]
    assert np.array_equal(got[steps:], want[steps:])


# ------------------------------------------------------------------------------------------ shapes, ragged sizes, guard bands
@pytest.mark.parametrize("shape", [dict(n_layers=4, width=128, skips=(1,), B=37, Nc=32, Nf=48, chunk=16, wb=1),
                                   dict(n_layers=2, width=64, skips=(), B=5, Nc=16, Nf=16, chunk=0, wb=0),
                                   dict(n_layers=8, width=256, skips=(4,), B=1, Nc=64, Nf=128, chunk=0, wb=0),
                                   dict(n_layers=3, width=100, skips=(0, 1), B=129, Nc=64, Nf=128, chunk=50, wb=0),
                                   dict(n_layers=8, width=256, skips=(), B=300, Nc=8, Nf=200, chunk=128, wb=1)])
def test_one_call_step_over_network_and_batch_shapes(dev, shape):
    """The one-call step against the autograd form for other depths / widths (zero-padded into the 64 / 128 / 256 kernels) /
    skip masks, ragged ray counts (B = 1, 37, 129: partial tiles, ragged last chunk) and sample counts other than 64 + 128
    (the sampler's generic instance): two steps, losses and parameters."""
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs
    from smpl_nerf_amd.trainer import DataParallelTrainer
    B, Nc, Nf = shape["B"], shape["Nc"], shape["Nf"]
    rng = np.random.default_rng(B + Nc)
    o = rng.normal(0, 0.2, (B, 3)).astype(np.float32) + np.array([0, 0, 2.4], np.float32)
    d = rng.normal(0, 0.3, (B, 3)).astype(np.float32) + np.array([0, 0, -1], np.float32)
    z = np.sort(rng.uniform(1.0, 4.0, (B, Nc)).astype(np.float32), -1)
    samples = o[:, None, :] + d[:, None, :] * z[:, :, None]
    gt = rng.uniform(0, 1, (B, 3)).astype(np.float32)
    batch = [T(a, dev) for a in (samples.astype(np.float32), o, d, z, gt)]
    runs = []
    for one_call in (None, False):
        torch.manual_seed(shape.get("seed", 21))
        nets = []
        for _ in range(2):
            from smpl_nerf_amd.nets import RenderRayNet
            m = RenderRayNet(shape["n_layers"], shape["width"], 60, 24, skips=list(shape["skips"])).to(dev).train()
            with torch.no_grad():
                m.sigma_out_layer.weight.mul_(20.0)          # densities that composite to something
            nets.append(m)
        pipe = NerfPipeline(nets[0], nets[1], PipelineArgs(white_background=shape["wb"], number_fine_samples=Nf),
                            PositionalEncoder(10, 0), PositionalEncoder(4, 0))
        tr = DataParallelTrainer(pipe, nets, lr=1e-3, one_call=one_call)
        tr.rays_per_chunk = shape["chunk"]
        losses = [float(tr.step(batch))]
        grads = [p.grad.clone() for p in tr.params]           # of the first step: same parameters on both sides
        losses.append(float(tr.step(batch)))
        assert (tr._one_call_state() is not None) == (one_call is None)
        runs.append((losses, grads, [p.detach().clone() for p in tr.params]))
    close(runs[0][0][:1], runs[1][0][:1], 2e-6, 1e-8)      # the same forward
    close(runs[0][0][1:], runs[1][0][1:], 1e-4, 1e-8)      # after one update from gradients summed in another order (chunks)
    assert all(np.isfinite(runs[0][0]))
    for ga, gb in zip(runs[0][1], runs[1][1]):
        assert float((ga - gb).norm()) <= 5e-5 * float(gb.norm()) + 1e-10
    # two Adam steps of 1e-3 each.  The coarse net's parameters follow the same trajectory to round-off.  The fine net's second
    # gradient is taken on hierarchical samples drawn from the coarse net's weights after the first step: a last-bit difference
    # there moves samples across the sampler's 1e-5 bin-mass switch (utils.py:224) and the second gradients agree to ~1e-3 only
    # (tools/ab/shape_debug.py prints it per tensor) - which Adam, normalising each step to ~lr, turns into parameter differences
    # of a few 1e-4 for a handful of elements: bounded by the two steps themselves, and 99 % of every tensor within 2e-4
    half = len(runs[0][2]) // 2
    for i, (pa, pb) in enumerate(zip(runs[0][2], runs[1][2])):
        d = (pa - pb).abs().reshape(-1).float()
        if i < half:
            assert float(d.max()) <= 2e-6
        else:
            assert float(d.max()) <= 2 * 1e-3 + 1e-6
            assert float(torch.quantile(d[:: max(1, d.numel() // 100000)], 0.99)) <= 2e-4


@pytest.mark.parametrize("prec", PRECISIONS)
def test_guard_bands_around_the_one_call_step(dev, prec):
    """Every buffer the trainer hands to snerf_nerf_train_step_f32 - workspace (activations, d Y, partials, the second set
    of the concurrent backward), loss / colour outputs, slot tables, weight streams - inside pattern bands: ragged batches
    (1, 37, 64 rays), one chunk and ragged chunks, run_fine = 0; no band is touched."""
    from test_gpu_round2 import _GuardBands
    total = 0
    with _GuardBands() as g:
        for B, chunk, run_fine in ((1, 0, 1), (37, 16, 1), (64, 0, 1), (37, 0, 0)):
            tr, pipe, mc, mf = _trainer(dev, prec if run_fine else "fp32", run_fine=run_fine)
            tr.rays_per_chunk = chunk
            batch = [t[:B].contiguous() for t in _batch(dev, 64)]
            for _ in range(2):
                loss = tr.step(batch)
            assert bool(torch.isfinite(loss))
            total += g.check()
    assert total > 20


# ------------------------------------------------------------------------------------------ a7: SmplNerfPipeline as one call
def _smpl_trainer(dev, prec="fp32", one_call=None, lr=1e-3, **args_kw):
    from smpl_nerf_amd.nets import WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import PipelineArgs, SmplNerfPipeline
    from smpl_nerf_amd.trainer import DataParallelTrainer
    pc, pf = syn.make_scene_nets(101)
    mc, mf = _net(dev, pc, prec), _net(dev, pf, prec)
    mw = WarpFieldNet(8, 256, 60, 40)
    mw.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_warp_field_params(103, out_scale=0.3).items()})
    mw.precision = prec
    mw = mw.to(dev).train()
    pipe = SmplNerfPipeline(mc, mf, mw, PipelineArgs(human_pose_encoding=1, **args_kw), PositionalEncoder(10, 0), PositionalEncoder(4, 0),
                            PositionalEncoder(10, 0))
    tr = DataParallelTrainer(pipe, [mc, mf, mw], lr=lr, one_call=one_call)
    return tr, pipe


def _smpl_batch(dev, n):
    b = _batch(dev, n, stride=61)
    pose = T(syn.human_poses()[np.arange(n) % 10].astype(np.float32), dev)
    return b[:4] + [pose, b[4]]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", [dict(chunk=0), dict(chunk=48, white_background=1), dict(chunk=0, run_fine=0)])
def test_smpl_nerf_one_call_step_equals_the_autograd_step(dev, prec, cfg):
    """SmplNerfSolver's per-batch body (solver/smpl_nerf_solver.py:76-89, default loss) through snerf_smpl_nerf_train_step_f32
    against the autograd form of the same pipeline (itself pinned to the reference's gradients, g11): warp net evaluated twice,
    nets back-propagating into their inputs, the coarse compositing into x' - o; losses, first-step gradients of all three
    nets, parameters after two steps; ray chunks; run_fine = 0."""
    cfg = dict(cfg)
    chunk = cfg.pop("chunk")
    runs = []
    for one_call in (None, False):
        tr, pipe = _smpl_trainer(dev, prec, one_call=one_call, **cfg)
        tr.rays_per_chunk = chunk
        batch = _smpl_batch(dev, 100)
        losses = [float(tr.step(batch))]
        grads = [None if p.grad is None else p.grad.clone() for p in tr.params]
        losses.append(float(tr.step(batch)))
        assert (tr._one_call_state() is not None) == (one_call is None)
        runs.append((losses, grads, [p.detach().clone() for p in tr.params]))
    close(runs[0][0][:1], runs[1][0][:1], 2e-6, 1e-8)
    close(runs[0][0][1:], runs[1][0][1:], 2e-4, 1e-8)
    for ga, gb in zip(runs[0][1], runs[1][1]):
        assert (ga is None) == (gb is None)
        if ga is not None:
            assert float((ga - gb).norm()) <= 1e-4 * float(gb.norm()) + 1e-10
    # (Adam's first steps move every parameter by ~lr x sign(gradient): where a gradient element is round-off around zero the
    # two forms may step in opposite directions - bounded by the two steps themselves in the split modes)
    for pa, pb in zip(runs[0][2], runs[1][2]):
        assert float((pa - pb).abs().max()) <= (3e-4 if prec == "fp32" else 2.5e-3)


@pytest.mark.parametrize("prec", ["fp32", "bf16x6"])
@pytest.mark.parametrize("wb", [0, 1])
def test_smpl_nerf_one_call_step_vs_the_reference_gradients(dev, wb, prec):
    """The same batch, nets and loss as tests/golden/make_golden_smpl_grad.py (g11: the reference's SmplNerfPipeline
    under autograd, models/smpl_nerf_pipeline.py:38-98) - here through snerf_smpl_nerf_train_step_f32 directly: loss, the digests
    of all three nets' gradients, every element of the warp net's gradient."""
    from smpl_nerf_amd.nets import WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import PipelineArgs, SmplNerfPipeline
    from smpl_nerf_amd.trainer import DataParallelTrainer
    g6, g = load_golden("g6_smpl_nerf_pipeline.npz"), load_golden("g11_smpl_grads.npz")
    pc, pf = syn.make_scene_nets(101)
    mc, mf = _net(dev, pc, prec), _net(dev, pf, prec)
    mw = WarpFieldNet(8, 256, 60, 40)
    mw.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_warp_field_params(103, out_scale=0.3).items()})
    mw.precision = prec
    mw = mw.to(dev).train()
    pipe = SmplNerfPipeline(mc, mf, mw, PipelineArgs(white_background=wb), PositionalEncoder(10, 0), PositionalEncoder(4, 0),
                            PositionalEncoder(10, 0))
    tr = DataParallelTrainer(pipe, [mc, mf, mw], lr=1e-7)
    assert tr._one_call_state() is not None
    data = syn.frame_batch(128, 128, phi=5.0, theta=15.0, seed=9)
    d = [T(a[g6["sub"]], dev) for a in data[:4]] + [T(g6["goal_pose"], dev), T(data[4][g6["sub"]], dev)]
    loss = float(tr.step(d))
    loose = 1.0
    close([loss], g[f"loss_wb{wb}"], 1e-5 * loose, 1e-7)
    for name, m in (("coarse", mc), ("fine", mf), ("warp", mw)):
        for k, p in m.named_parameters():
            ref = g[f"grad_wb{wb}/{name}.{k}"]
            assert p.grad is not None, (name, k)
            scale = max(np.abs(ref[2:]).max(), ref[1] / np.sqrt(p.numel()), 1e-12)
            close(R.digest(p.grad), ref, 2e-2 * loose, 1e-2 * loose * scale)
    for k, p in mw.named_parameters():
        ref = g[f"warpfull_wb{wb}/{k}"].astype(np.float64)
        got = p.grad.cpu().numpy().astype(np.float64)
        assert np.linalg.norm(got - ref) <= 1e-2 * loose * np.linalg.norm(ref), (k, np.linalg.norm(got - ref) / np.linalg.norm(ref))


def test_smpl_nerf_split_precision_with_identity_columns_takes_the_autograd_path(dev):
    """Found by tools/ab/fuzz_train.py: the split-precision dgrad returns input gradients for the default-sized encoders only, so
    a bf16x6 / f16x3 SmplNerfPipeline whose position encoder has identity columns (5 k-blocks) trains through the autograd path
    (nets.py routes that one dgrad to the fp32 kernels) instead of failing in the one call; fp32 nets keep the one call."""
    from smpl_nerf_amd.nets import RenderRayNet, WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import PipelineArgs, SmplNerfPipeline
    from smpl_nerf_amd.trainer import DataParallelTrainer
    batch = _smpl_batch(dev, 40)
    for prec, one_call in (("f16x3", False), ("fp32", True)):
        torch.manual_seed(5)
        pe, de = PositionalEncoder(10, 1), PositionalEncoder(4, 0)
        nets = [RenderRayNet(4, 256, 3 * pe.output_dim, 3 * de.output_dim, skips=[2]).to(dev).train() for _ in range(2)]
        mw = WarpFieldNet(3, 128, 3 * pe.output_dim, 40).to(dev).train()
        for m in nets:
            m.precision = prec
        pipe = SmplNerfPipeline(nets[0], nets[1], mw, PipelineArgs(), pe, de, PositionalEncoder(10, 0))
        tr = DataParallelTrainer(pipe, nets + [mw], lr=1e-4)
        assert (tr._one_call_state() is not None) == one_call
        losses = [float(tr.step(batch)) for _ in range(2)]
        assert all(np.isfinite(losses))
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in mw.parameters())


def _poison_the_allocator(dev):
    """Every cached block the caching allocator hands out next holds NaNs."""
    blocks = [torch.full((2 ** k,), float("nan"), device=dev) for k in (28, 26, 24)]
    blocks += [torch.full((2 ** k,), float("nan"), device=dev) for k in range(6, 24) for _ in range(4)]
    del blocks


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("kind", ["nerf", "smpl_nerf"])
@pytest.mark.parametrize("one_call", [None, False])
def test_training_steps_read_nothing_they_did_not_write(dev, kind, prec, one_call):
    """Workspaces, activation / d Y buffers, partials and gradient buffers come from torch's caching allocator uninitialised; with
    every cached block full of NaNs beforehand (and again before each step) three steps of either form of the step still give
    finite losses and gradients - for the default encoders and for encoders with identity columns (a fifth k-block)."""
    from smpl_nerf_amd.nets import RenderRayNet, WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs, SmplNerfPipeline
    from smpl_nerf_amd.trainer import DataParallelTrainer
    for ident in (0, 1):
        torch.manual_seed(5)
        _poison_the_allocator(dev)
        pe, de = PositionalEncoder(10, ident), PositionalEncoder(4, 0)
        nets = [RenderRayNet(4, 256, 3 * pe.output_dim, 3 * de.output_dim, skips=[2]).to(dev).train() for _ in range(2)]
        for m in nets:
            m.precision = prec
        if kind == "smpl_nerf":
            mw = WarpFieldNet(3, 128, 3 * pe.output_dim, 40).to(dev).train()
            pipe = SmplNerfPipeline(nets[0], nets[1], mw, PipelineArgs(), pe, de, PositionalEncoder(10, 0))
            models, batch = nets + [mw], _smpl_batch(dev, 40)
        else:
            pipe = NerfPipeline(nets[0], nets[1], PipelineArgs(), pe, de)
            models, batch = nets, _batch(dev, 40, stride=61)
        tr = DataParallelTrainer(pipe, models, lr=1e-4, one_call=one_call)
        for _ in range(3):
            _poison_the_allocator(dev)
            assert np.isfinite(float(tr.step(batch)))
        for m in models:
            for k, p in m.named_parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (kind, prec, ident, k)
        del tr, pipe, models, nets


@pytest.mark.parametrize("tool", ["lds_poison_sweep.py", "nan_hunt.py"])
def test_no_kernel_depends_on_what_the_lds_held_before(dev, tool):
    """SNERF_DEBUG_POISON_LDS=1 (csrc/snerf_common.h): every checked launch is followed by a kernel that fills the LDS of every CU
    with NaNs, so a kernel that reads LDS it has not written computes with NaNs instead of the previous kernel's leftovers.
    The regression behind it: the wide fp32 wgrad multiplied zeros with stale LDS for chunks behind the end of the buffer -
    exact unless the LDS held NaNs, which it does for the first process on a freshly booted GPU (tools/ab/nan_hunt.py found
    it).  Forward + backward over sample counts with ragged / empty trailing chunks in three precisions, and three training
    steps of every pipeline / precision / form of the step, in a process of their own (the switch is read once)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SNERF_DEBUG_POISON_LDS="1", SNERF_TRAIN_AUX_STREAM="0")   # the poison kernel runs on the NULL stream
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ab", tool)] + (["1"] if tool == "nan_hunt.py" else []),
                       capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last in ("bad: 0", "non-finite gradient tensors seen: 0"), r.stdout[-3000:]


@pytest.mark.parametrize("tool,count,seed", [("fuzz_train.py", 40, 11), ("fuzz_render.py", 40, 12)])
def test_randomised_sweeps_agree(dev, tool, count, seed):
    """tools/ab/fuzz_train.py (the one-call step against the autograd form) and fuzz_render.py (inference against the CPU torch
    restatement of the reference) over random depth / width / skips / encoders / ray and sample counts / chunks / precisions /
    pipelines: a small fixed-seed slice of the sweeps that found this round's two gaps."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ab", tool), str(count), str(seed)], capture_output=True, text=True,
                       timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == f"{count} of {count} cases agree", r.stdout[-3000:]


def test_gradients_do_not_depend_on_how_the_samples_are_chunked(dev):
    """tools/ab/chunk_consistency.py: the parameter gradients of one backward over n samples equal the sum of two backwards over
    an uneven split of them, for n from 5 to a million (every chunk-count rule and small-call kernel variant of the wgrad /
    dgrad launchers), in the three precisions and for the warp net."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ab", "chunk_consistency.py")], capture_output=True, text=True,
                       timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "bad: 0", r.stdout[-3000:]


def test_smpl_nerf_one_call_step_in_a_hip_graph(dev):
    """snerf_smpl_nerf_train_step_f32 (warp stage, both nets, Adam, the warp net's re-pack) captured into a HIP graph and
    replayed walks the trajectory of eager steps - like test_one_call_step_in_a_hip_graph for the plain pipeline."""
    tr, _ = _smpl_trainer(dev, lr=1e-4)
    eager, _ = _smpl_trainer(dev, lr=1e-4)
    batch = _smpl_batch(dev, 64)
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
    assert tr._one_call_state() is not None and float(loss) == float(want)
    for a, b in zip(tr.params, eager.params):
        assert torch.equal(a, b)


def test_smpl_nerf_one_call_step_keeps_inference_current(dev):
    """After one-call steps the pipeline's inference (forward and the single-call render) reads the streams the step kept
    current - the warp net's are re-packed inside the call - and equals a pipeline built from the new parameters."""
    tr, pipe = _smpl_trainer(dev)
    batch = _smpl_batch(dev, 64)
    for _ in range(3):
        tr.step(batch)
    tr2, pipe2 = _smpl_trainer(dev)
    for a, b in zip(tr.models, tr2.models):
        b.load_state_dict(a.state_dict())
    with torch.no_grad():
        o1, o2 = pipe(batch), pipe2(batch)
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("kind", ["append_smpl_params", "append_smpl_params_encoded", "append_to_nerf"])
def test_pose_conditioned_pipelines_one_call_step_equals_the_autograd_step(dev, prec, kind):
    """f-4 (the paper's headline model): AppendSmplParamsPipeline / AppendToNerfPipeline - per-ray pose columns in front of the
    encoding, raw or encoded (models/append_smpl_params_pipeline.py:29-52, append_to_nerf_pipeline.py:26) - train through
    snerf_nerf_train_step_f32 with batch.additional; against the autograd form (pinned to the reference by g10): losses,
    first-step gradients, ray chunks.  A pose that wants its own gradient keeps the autograd path."""
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import AppendSmplParamsPipeline, AppendToNerfPipeline, PipelineArgs
    from smpl_nerf_amd.trainer import DataParallelTrainer
    enc = kind.endswith("encoded")
    add_dim = {"append_smpl_params": 69, "append_smpl_params_encoded": 69 * 20, "append_to_nerf": 2}[kind]
    runs = []
    batch = _smpl_batch(dev, 100)
    for one_call in (None, False):
        params = [syn.make_scene_net_params(s, add_first=True, additional_input_dim=add_dim) for s in (301, 303)]
        nets = []
        for p in params:
            m = RenderRayNet(8, 256, 60, 24, add_dim, skips=[4])
            m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
            m.precision = prec
            nets.append(m.to(dev).train())
        cls = AppendToNerfPipeline if kind == "append_to_nerf" else AppendSmplParamsPipeline
        pipe = cls(nets[0], nets[1], PipelineArgs(human_pose_encoding=1 if enc else 0), PositionalEncoder(10, 0), PositionalEncoder(4, 0),
                   PositionalEncoder(10, 0))
        tr = DataParallelTrainer(pipe, nets, lr=1e-3, one_call=one_call)
        tr.rays_per_chunk = 37
        losses = [float(tr.step(batch))]
        grads = [p.grad.clone() for p in tr.params]
        losses.append(float(tr.step(batch)))
        assert (tr._one_call_state() is not None) == (one_call is None)
        runs.append((losses, grads))
    # d loss / d goal_pose requested: the step must not swallow it (a fresh trainer: at this learning rate two steps drive the
    # synthetic scene's densities below zero everywhere, after which every gradient is exactly 0 - DESIGN section 5)
    tr = DataParallelTrainer(pipe, nets, lr=1e-6)
    b2 = list(batch)
    b2[4] = batch[4].clone().requires_grad_(True)
    tr.step(b2)
    assert tr._one_call_state() is not None and b2[4].grad is not None
    close(runs[0][0][:1], runs[1][0][:1], 2e-6, 1e-8)
    close(runs[0][0][1:], runs[1][0][1:], 2e-4, 1e-8)
    for ga, gb in zip(runs[0][1], runs[1][1]):
        assert float((ga - gb).norm()) <= 1e-4 * float(gb.norm()) + 1e-10


@pytest.mark.parametrize("prec", ["fp32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("kind", ["append_smpl_params", "append_smpl_params_encoded", "append_to_nerf"])
def test_pose_conditioned_pipelines_render_in_one_call(dev, prec, kind):
    """snerf_render_rays_add_f32 (8(f)-4, the paper's headline model): the single-call render with the pose rows as per-ray
    additional inputs equals forward() bit for bit - rgb, rgb_fine, the fine samples and densities - also with run_fine = 0,
    white background and a ragged ray count."""
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import AppendSmplParamsPipeline, AppendToNerfPipeline, PipelineArgs
    enc = kind.endswith("encoded")
    add_dim = {"append_smpl_params": 69, "append_smpl_params_encoded": 69 * 20, "append_to_nerf": 2}[kind]
    nets = []
    for seed in (301, 303):
        m = RenderRayNet(8, 256, 60, 24, add_dim, skips=[4])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scene_net_params(seed, add_first=True, additional_input_dim=add_dim).items()})
        m.precision = prec
        nets.append(m.to(dev).eval())
    cls = AppendToNerfPipeline if kind == "append_to_nerf" else AppendSmplParamsPipeline
    for B, cfg in ((257, dict()), (64, dict(run_fine=0)), (100, dict(white_background=1, number_fine_samples=37))):
        pipe = cls(nets[0], nets[1], PipelineArgs(human_pose_encoding=1 if enc else 0, **cfg), PositionalEncoder(10, 0),
                   PositionalEncoder(4, 0), PositionalEncoder(10, 0))
        batch = _smpl_batch(dev, B)
        with torch.no_grad():
            a, b = pipe(batch), pipe.render_rays(batch)
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x, y)
    # plain nets are refused by this entry, posed nets by the plain one
    lib = _lib.load()
    d = nets[0].desc_for_encoders(PositionalEncoder(10, 0), PositionalEncoder(4, 0), True)
    assert lib.snerf_render_rays_workspace_bytes(16, 64, 128) < lib.snerf_render_rays_add_workspace_bytes(d, d, 16, 64, 128) or prec != "fp32"


@pytest.mark.parametrize("chunk", [0, 7])
@pytest.mark.parametrize("prec", ["f16x3", "bf16x6"])
def test_split_precision_steps_with_encoded_pose_columns_follow_the_fp32_step(dev, prec, chunk):
    """Regression (found by tools/ab/fuzz_train.py): with the ENCODED pose (69 x 20 = 1380 per-ray columns) the additional
    inputs are wide weight-gradient jobs of their own; the f16 wide kernels scaled them by the statistic of the layer's hidden
    input - unset at layer 0, a chunk's accident at the skip layer - and returned 1 % / 29 % errors there.  The gradients of a
    split-precision step (whole batch and ray chunks, encoders with identity columns) against the fp32 step's, relative to the
    largest gradient tensor."""
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import AppendSmplParamsPipeline, PipelineArgs
    from smpl_nerf_amd.trainer import DataParallelTrainer
    batch = _smpl_batch(dev, 31)

    def grads(precision, rays_per_chunk):
        torch.manual_seed(1438)
        pe, de = PositionalEncoder(10, 1), PositionalEncoder(4, 1)
        nets = []
        for _ in range(2):
            m = RenderRayNet(5, 256, 3 * pe.output_dim, 3 * de.output_dim, 69 * 20, skips=[3]).to(dev).train()
            with torch.no_grad():
                m.sigma_out_layer.weight.mul_(20.0)
            m.precision = precision
            nets.append(m)
        pipe = AppendSmplParamsPipeline(nets[0], nets[1], PipelineArgs(number_fine_samples=5, human_pose_encoding=1), pe, de,
                                        PositionalEncoder(10, 0))
        tr = DataParallelTrainer(pipe, nets, lr=1e-6)
        tr.rays_per_chunk = rays_per_chunk
        tr.step(batch)
        assert tr._one_call_state() is not None
        return [p.grad.clone() for p in nets[0].parameters()]      # the coarse net: independent of the fine samples

    ref = grads("fp32", 0)
    top = max(float(r.norm()) for r in ref)
    assert top > 0
    for g, r in zip(grads(prec, chunk), ref):
        assert bool(torch.isfinite(g).all()) and float((g - r).norm()) <= 1e-4 * top


@pytest.mark.parametrize("prec", ["fp32", "bf16x6"])
def test_append_vertices_one_call_step_equals_the_autograd_step(dev, prec):
    """a8 / configs[4]: AppendVerticesPipeline with a frozen estimator and body model (the vertex floats the nets read are
    per-ray constants, quirk Q7) trains through snerf_nerf_train_step_f32 with batch.additional; the dead vertices_net
    parameters get no gradient and are not updated, like in the reference."""
    from test_gpu_round2 import _av_pipeline
    from smpl_nerf_amd.trainer import DataParallelTrainer
    b = _batch(dev, 100, stride=53)
    images = (torch.arange(100, device=dev) % 10)
    batch = b[:4] + [images, b[4]]
    runs = []
    for one_call in (None, False):
        pipe, _ = _av_pipeline(dev, prec, n_poses=10, run_fine=1)
        nets = [pipe.model_coarse.train(), pipe.model_fine.train()]
        tr = DataParallelTrainer(pipe, nets, lr=1e-4, one_call=one_call)
        tr.rays_per_chunk = 64
        dead = [p.detach().clone() for p in nets[0].vertices_net.parameters()]
        losses = [float(tr.step(batch))]
        grads = [None if p.grad is None else p.grad.clone() for p in tr.params]
        losses.append(float(tr.step(batch)))
        assert (tr._one_call_state() is not None) == (one_call is None)
        assert all(p.grad is None for p in nets[0].vertices_net.parameters())
        assert all(torch.equal(a, p) for a, p in zip(dead, nets[0].vertices_net.parameters()))
        runs.append((losses, grads))
    close(runs[0][0][:1], runs[1][0][:1], 2e-6, 1e-8)
    close(runs[0][0][1:], runs[1][0][1:], 2e-4, 1e-8)
    for ga, gb in zip(runs[0][1], runs[1][1]):
        assert (ga is None) == (gb is None)
        if ga is not None:
            assert float((ga - gb).norm()) <= 1e-4 * float(gb.norm()) + 1e-10
    # (r05: a TRAINED estimator stays on the one-call path too - d loss / d vertices comes back from the call:
    # tests/test_gpu_round5.py::test_trained_estimator_and_pose_gradients_through_the_one_call_step)
    pipe, _ = _av_pipeline(dev, prec, n_poses=10, run_fine=1)
    pipe.smpl_estimator.goal_poses.requires_grad_(True)
    tr = DataParallelTrainer(pipe, [pipe.model_coarse, pipe.model_fine, pipe.smpl_estimator], lr=1e-4)
    assert tr._one_call_state() is not None
    tr.step(batch)
    assert float(pipe.smpl_estimator.goal_poses.grad.abs().max()) > 0


@pytest.mark.parametrize("kind", ["nerf", "smpl_nerf"])
def test_the_two_halves_of_the_step_equal_the_one_call(dev, kind):
    """With several ranks the step runs as snerf_*_train_grads_f32 -> all-reduce of the flat gradient -> snerf_adam_step_f32
    (-> snerf_warp_repack_f32): forced here on one rank (the all-reduce over no group is the identity), the trajectory equals
    the single call's bit for bit, run_fine = 0 included (the idle fine net then contributes zeros and is stepped, like every
    rank's would be - DESIGN section 7)."""
    finals = []
    for split in (False, True):
        if kind == "nerf":
            tr, pipe, _, _ = _trainer(dev, lr=1e-4)
            batch = _batch(dev, 96)
        else:
            tr, pipe = _smpl_trainer(dev, lr=1e-4)
            batch = _smpl_batch(dev, 96)
        tr._sync = split
        tr.rays_per_chunk = 40
        losses = [float(tr.step(batch)) for _ in range(3)]
        with torch.no_grad():
            out = pipe(batch)
        finals.append((losses, [p.detach().clone() for p in tr.params], out[1].clone()))
    assert finals[0][0] == finals[1][0]
    for a, b in zip(finals[0][1], finals[1][1]):
        assert torch.equal(a, b)
    assert torch.equal(finals[0][2], finals[1][2])
