"""SMPL linear blend skinning on the GPU (csrc/smpl_lbs.hip, ops.smpl_lbs, body_model.SmplBodyModel) and the two pipelines on top.

Error measure (as tests/test_gpu_vertex_warp.py): E(y) = max|y - y64| / max|y64|, y64 the float64 restatement (tests/smpl_lbs_ref.py)
of the same fp32 inputs.  Bound: E(kernel) <= max(8 E(fp32 CPU restatement), 2^-23), both sides computed in the test - the yardstick
is never the kernel.  8 is that file's factor for a re-ordered sum (here the sums have 217 and up to 24 terms); 2^-23 is one fp32 ulp of
the largest value, for the cases where the fp32 restatement happens to be exact.  Every test prints its figures before it asserts
(pytest -s; profiles/smpl_lbs_errors.txt holds a run).

Shapes: the issue's six, then the edges of the kernels' tiles - 16 poses x 128 vertices forward, 8 poses x 256 vertices backward, the
64-coefficient staging of the blend (K = 217 crosses it three times; K = 19 does not fill it), one and several vertex tiles per
backward slice ([2, 6890]: 27 tiles in 16 slices).  For gradient cases every joint's rotation angle lies in [0.05, 2.5] rad, asserted on
the CPU: near 0 the 1e-8 formula is ill-conditioned in fp32 for kernel and yardstick alike.  No case is left out.

Measured on an MI355X (profiles/smpl_lbs_errors.txt has every figure): E kernel / E fp32 CPU is 0.27 .. 1.0 for the vertices (3.8e-8 ..
1.7e-7), 0.11 .. 1.0 for the joints, 0.17 .. 0.63 for d_body_pose, 0.11 .. 1.5 for d_global_orient, 0.06 .. 3.0 for d_betas (8.8e-7 at
most); DynamicPipeline: loss 0.6, pose gradient 0.016 (2.5e-6 against 1.6e-4), third trainer step 1.5."""

import numpy as np
import pytest
import torch

import smpl_lbs_ref as SR
import vertex_warp_ref as VR

pytestmark = pytest.mark.gpu
FACTOR, ULP = 8.0, 2.0 ** -23
SHAPES = [(1, 1), (2, 63), (3, 65), (5, 257), (65, 130), (2, 6890)]
TILE_EDGES = [(8, 128), (9, 129), (15, 127), (16, 256), (17, 257), (33, 255), (7, 513)]
GRADS = ("d_betas", "d_body_pose", "d_global_orient")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def model_on(dev, arrays, NB):
    from smpl_nerf_amd.body_model import SmplBodyModel
    return SmplBodyModel.from_arrays(**arrays, num_betas=NB).to(dev)


def on_gpu(dev, inputs, which=("vertices", "joints"), need_grad=True, model=None):
    from smpl_nerf_amd import ops
    a, betas, pose, orient, d_v, d_j = inputs
    model = model or model_on(dev, a, betas.shape[1])
    b, p = (torch.from_numpy(x).to(dev).requires_grad_(need_grad) for x in (betas, pose))
    g = None if orient is None else torch.from_numpy(orient).to(dev).requires_grad_(need_grad)
    v, j = ops.smpl_lbs(model.kernel_buffers(), b, p, g)
    B = pose.shape[0]
    assert tuple(v.shape) == (B, a["weights"].shape[0], 3) and tuple(j.shape) == (B, a["weights"].shape[1], 3)
    r = {"vertices": v, "joints": j}
    if need_grad:
        loss = 0
        if "vertices" in which:
            loss = loss + (v * torch.from_numpy(d_v).to(dev)).sum()
        if "joints" in which:
            loss = loss + (j * torch.from_numpy(d_j).to(dev)).sum()
        loss.backward()
        r.update(d_betas=b.grad, d_body_pose=p.grad)
        if g is not None:
            r["d_global_orient"] = g.grad
    return {k: N(t) for k, t in r.items()}


def hold(tag, got, y32, y64, names):
    worst = 0.0
    for k in names:
        ek, ec = SR.relative_error(got[k], y64[k]), SR.relative_error(y32[k], y64[k])
        print(f"{tag} {k}: E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  max|y64| {np.abs(y64[k]).max():.3e}")
        assert got[k].shape == y64[k].shape and np.isfinite(got[k]).all(), f"{tag} {k}: shape or non-finite values"
        assert ek <= max(FACTOR * ec, ULP), f"{tag} {k}: E kernel {ek:.3e} > max({FACTOR} x E fp32 CPU {ec:.3e}, 2^-23)"
        worst = max(worst, ek / ec if ec else 0.0)
    return worst


def angles_ok(inputs):
    ang = SR.angles(inputs[2], inputs[3])
    if inputs[3] is None:
        ang = ang[:, 1:]
    assert ang.min() >= 0.05 and ang.max() <= 2.5, f"rotation angles {ang.min():.3f} .. {ang.max():.3f} leave [0.05, 2.5]"


def case(dev, tag, inputs, which=("vertices", "joints")):
    angles_ok(inputs)
    y64, y32 = SR.restated(inputs, torch.float64, which), SR.restated(inputs, torch.float32, which)
    got = on_gpu(dev, inputs, which)
    names = ("vertices", "joints") + tuple(k for k in GRADS if k in y64)
    for k in names[2:]:
        assert np.abs(y64[k]).max() > 0, f"{tag}: {k} is zero, the case would test nothing"
    return hold(tag, got, y32, y64, names)


@pytest.mark.parametrize("B,V", SHAPES + TILE_EDGES)
def test_forward_and_backward_shapes(dev, B, V):
    """vertices, joints and the three gradients, incoming gradients on both outputs; J = 24, NB = 10, betas with B rows."""
    case(dev, f"[{B},{V}]", SR.op_inputs(B, V, seed=1))


@pytest.mark.parametrize("which", [("vertices",), ("joints",)])
def test_one_incoming_gradient(dev, which):
    case(dev, f"only d {which[0]}", SR.op_inputs(3, 65, seed=2), which)


def test_short_chain_one_beta(dev):
    """J = 3 (a root and two joints), NB = 1: K = 19 does not fill one staging chunk."""
    case(dev, "J=3 NB=1", SR.op_inputs(5, 130, J=3, NB=1, seed=3))


def test_longest_chain(dev):
    """J = 32, the bound of the rig kernels' arrays and of the transform tile; NB = 16: K = 295 (two rounds of the backward's k lanes)."""
    case(dev, "J=32 NB=16", SR.op_inputs(3, 65, J=32, NB=16, seed=8))


def test_shared_betas(dev):
    """betas with one row: d_betas is the sum over the batch (in the kernels; more than 256 poses: every lane of the row sum adds twice)."""
    case(dev, "betas [1,NB] B=9", SR.op_inputs(9, 65, seed=4, betas_rows=1))
    case(dev, "betas [1,NB] B=300", SR.op_inputs(300, 3, seed=4, betas_rows=1))


def test_expanded_betas_are_read_as_one_row(dev):
    """estimator.betas.expand(B, -1), as the pipelines pass it: the gradient arrives at the one row."""
    from smpl_nerf_amd import ops
    inputs = SR.op_inputs(9, 65, seed=4, betas_rows=1)
    a, betas, pose, orient, d_v, d_j = inputs
    y64, y32 = SR.restated(inputs, torch.float64, ("vertices",)), SR.restated(inputs, torch.float32, ("vertices",))
    row = torch.from_numpy(betas).to(dev).requires_grad_(True)
    v, _ = ops.smpl_lbs(model_on(dev, a, 10).kernel_buffers(), row.expand(9, -1), torch.from_numpy(pose).to(dev), torch.from_numpy(orient).to(dev))
    (v * torch.from_numpy(d_v).to(dev)).sum().backward()
    hold("expanded betas", {"vertices": N(v), "d_betas": N(row.grad)}, y32, y64, ("vertices", "d_betas"))


def test_without_global_orient(dev):
    case(dev, "global_orient None", SR.op_inputs(5, 130, seed=5, orient=False))


def test_dense_skinning_weights(dev):
    inputs = SR.op_inputs(5, 257, seed=6, dense=True)
    assert (inputs[0]["weights"] > 0).all()
    case(dev, "dense weights", inputs)


def test_zero_pose(dev):
    """The canonical call of DynamicPipeline: the forward is held like every other, the backward must be finite everywhere."""
    a, betas, pose, orient, d_v, d_j = SR.op_inputs(3, 257, seed=7)
    inputs = (a, betas, np.zeros_like(pose), np.zeros_like(orient), d_v, d_j)
    y64, y32 = SR.restated(inputs, torch.float64, need_grad=False), SR.restated(inputs, torch.float32, need_grad=False)
    got = on_gpu(dev, inputs)
    hold("zero pose", got, y32, y64, ("vertices", "joints"))
    for k in GRADS:
        print(f"zero pose {k}: max |.| {np.abs(got[k]).max():.3e}")
        assert np.isfinite(got[k]).all(), k


def test_two_runs_are_bit_identical(dev):
    for B, V, rows in ((17, 257, None), (300, 3, 1), (2, 6890, None)):
        inputs = SR.op_inputs(B, V, seed=1, betas_rows=rows)
        model = model_on(dev, inputs[0], 10)
        a, b = on_gpu(dev, inputs, model=model), on_gpu(dev, inputs, model=model)
        for k in a:
            assert np.array_equal(a[k], b[k]), (B, V, k)


def test_empty_batch(dev):
    a, betas, pose, orient, d_v, d_j = SR.op_inputs(1, 65, seed=1)
    got = on_gpu(dev, (a, betas[:1], pose[:0], orient[:0], d_v[:0], d_j[:0]))
    assert got["vertices"].shape == (0, 65, 3) and got["joints"].shape == (0, 24, 3)
    assert got["d_body_pose"].shape == (0, 69) and got["d_global_orient"].shape == (0, 3)
    assert np.array_equal(got["d_betas"], np.zeros((1, 10), np.float32))
    got = on_gpu(dev, (a, betas[:1], pose[:0], None, d_v[:0], d_j[:0]), need_grad=False)
    assert got["vertices"].shape == (0, 65, 3)


def test_every_output_element_is_written(dev):
    """What SNERF_TEST_POISON_EMPTY=1 does to the whole suite, here for these calls: every tensor torch.empty hands out starts as NaNs
    (workspaces as 0xff bytes) - no NaN may survive in any output, with every combination of optional pointers."""
    import conftest
    saved = torch.empty, torch.empty_like, torch.Tensor.new_empty
    conftest._poison_torch_empty()
    try:
        for inputs, which in ((SR.op_inputs(17, 257, seed=1), ("vertices", "joints")), (SR.op_inputs(9, 130, seed=2, betas_rows=1), ("vertices",)),
                              (SR.op_inputs(9, 130, seed=2, orient=False), ("joints",)), (SR.op_inputs(2, 6890, seed=1), ("vertices", "joints"))):
            probe = torch.empty(4, device=dev)
            assert torch.isnan(probe).all(), "the poison is not in place"
            got = on_gpu(dev, inputs, which)
            for k, v in got.items():
                assert np.isfinite(v).all(), k
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = saved


def test_no_grad_call_agrees_and_keeps_nothing(dev):
    from smpl_nerf_amd import ops
    a, betas, pose, orient, _, _ = SR.op_inputs(5, 257, seed=1)
    mb = model_on(dev, a, 10).kernel_buffers()
    b, p, g = (torch.from_numpy(x).to(dev) for x in (betas, pose, orient))
    with torch.no_grad():
        plain = ops.smpl_lbs(mb, b, p, g)
    tracked = ops.smpl_lbs(mb, b, p.clone().requires_grad_(True), g)
    assert all(t.grad_fn is None for t in plain) and all(t.grad_fn is not None for t in tracked)
    assert all(torch.equal(x, y) for x, y in zip(plain, tracked))


# ---------------------------------------------------------------------------------------------- the pipelines
DP = dict(V=257, B=6, S=16, images=3, body_seed=31, net_seed=401, plant_seed=33, pose_seed=34, radius=0.01, temperature=2000.0,
          frame=dict(h=128, w=128, phi=4.0, theta=-20.0, seed=13, n_coarse=16))


@pytest.fixture(scope="module")
def dp_inputs():
    """(batch of fp32 numpy arrays, goal poses [3, 69], body arrays, net parameters): 6 rays of 3 images, 16 samples each, every third
    sample planted within the warp radius of a goal vertex (float64 yardstick vertices)."""
    from smpl_nerf_amd import synthetic as syn
    from smpl_nerf_amd.synthetic_smpl import random_smpl_arrays
    c = DP
    data = syn.frame_batch(**c["frame"])
    sub = np.arange(c["B"]) * (128 * 128 // c["B"]) + 37
    images = np.arange(c["B"]) % c["images"]
    poses = syn.human_poses((41, 38), 20, 60, c["images"])
    poses = (poses + 0.05 * np.random.default_rng(c["pose_seed"]).normal(size=poses.shape)).astype(np.float32)
    arrays = random_smpl_arrays(c["body_seed"], n_vertices=c["V"])
    body64 = SR.TorchBodyModel(arrays).double()
    goal = N(body64(body_pose=torch.from_numpy(poses[images]).double()).vertices).astype(np.float32)
    samples = VR.plant(data[0][sub], goal, c["radius"], np.random.default_rng(c["plant_seed"]))
    batch = [samples, data[1][sub], data[2][sub], data[3][sub], images, data[4][sub]]
    near, zero = VR.input_margins(samples, goal, c["radius"])
    assert near >= 4e-6 and zero >= 1e-4, f"the inputs sit on a discontinuity of the warp's gradient: |d - r| {near:.2e}, d {zero:.2e}"
    ang = SR.angles(poses, None).reshape(c["images"], 24)[:, (1 + 38 // 3, 1 + 41 // 3)]
    assert ang.min() >= 0.05 and ang.max() <= 2.5, "the two animated joints leave [0.05, 2.5] rad"
    return batch, poses, arrays, syn.make_scene_net_params(c["net_seed"])


def _pipeline(dev, dp_inputs):
    from smpl_nerf_amd.body_model import SmplBodyModel
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import DynamicPipeline, PipelineArgs
    from smpl_nerf_amd.synthetic_smpl import IndexPoseEstimator
    batch_np, poses, arrays, params = dp_inputs
    net = RenderRayNet(8, 256, 60, 24, skips=[4])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    est = IndexPoseEstimator(torch.from_numpy(poses), torch.zeros(1, 10), trainable_poses=True)
    args = PipelineArgs(run_fine=1, warp_radius=DP["radius"], warp_temperature=DP["temperature"], number_coarse_samples=DP["S"])
    body = SmplBodyModel.from_arrays(**arrays)
    return DynamicPipeline(net.to(dev), net, est.to(dev), body.to(dev), args, PositionalEncoder(10, 0), PositionalEncoder(4, 0))


def _cpu_pipeline(dp_inputs, dtype):
    """(parameters, poses tensor, loss closure) of the CPU chain smpl_lbs_ref -> vertex_warp_ref -> torch_ref in `dtype`; the loss is the
    trainer's: MSE of the coarse and of the fine colour, which are one tensor in this pipeline."""
    batch_np, poses, arrays, params = dp_inputs
    P = {k: torch.from_numpy(v).to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    gp = torch.from_numpy(poses).to(dtype).clone().requires_grad_(True)
    body = SR.TorchBodyModel(arrays).to(dtype)
    batch = [torch.from_numpy(a) if a.dtype.kind in "iu" else torch.from_numpy(a).to(dtype) for a in batch_np]
    return P, gp, lambda: 2 * torch.nn.functional.mse_loss(VR.dynamic_pipeline(P, body, gp, batch, DP["radius"], DP["temperature"])[0], batch[5])


def test_dynamic_pipeline_loss_and_pose_gradient(dev, dp_inputs):
    """pose -> vertices -> warp -> net -> pixels and back, all project kernels: the loss and d loss / d goal_poses of the two animated
    joints (columns 38 and 41) by the float64 rule."""
    from smpl_nerf_amd.trainer import DataParallelTrainer
    pipe = _pipeline(dev, dp_inputs)
    batch = [torch.from_numpy(a).to(dev) for a in dp_inputs[0]]
    tr = DataParallelTrainer(pipe, [pipe.model_coarse, pipe.smpl_estimator], lr=2e-5)
    out = pipe(batch)
    assert [tuple(o.shape) for o in out[:3]] == [(6, 3), (6, 3), (6, 16, 3)]
    loss = tr.batch_loss(out, batch)
    loss.backward()
    got = {"loss": np.array([loss.item()]), "grad": N(pipe.smpl_estimator.goal_poses.grad)[:, (38, 41)]}
    ys = []
    for dtype in (torch.float64, torch.float32):
        P, gp, step = _cpu_pipeline(dp_inputs, dtype)
        l = step()
        l.backward()
        ys.append({"loss": np.array([l.item()]), "grad": N(gp.grad)[:, (38, 41)]})
    assert np.abs(ys[0]["grad"]).max() > 0 and np.abs(N(out[2])).max() > 0, "nothing is warped: the case would test nothing"
    hold("DynamicPipeline", got, ys[1], ys[0], ("loss", "grad"))


def test_dynamic_pipeline_three_trainer_steps(dev, dp_inputs):
    """Net and estimator poses trained together by DataParallelTrainer (the autograd path: the body model is a module in front of the
    warp): the loss of the third step against the same three Adam steps on the CPU chain."""
    from smpl_nerf_amd.trainer import DataParallelTrainer
    lr = 2e-5           # (as tests/test_gpu_vertex_warp.py: at the reference's 5e-4 one Adam step empties the synthetic scene)
    pipe = _pipeline(dev, dp_inputs)
    batch = [torch.from_numpy(a).to(dev) for a in dp_inputs[0]]
    tr = DataParallelTrainer(pipe, [pipe.model_coarse, pipe.smpl_estimator], lr=lr)
    got = [tr.step(batch).item() for _ in range(3)]
    ys = []
    for dtype in (torch.float64, torch.float32):
        P, gp, step = _cpu_pipeline(dp_inputs, dtype)
        opt = torch.optim.Adam(list(P.values()) + [gp], lr=lr)
        traj = []
        for _ in range(3):
            opt.zero_grad()
            l = step()
            l.backward()
            opt.step()
            traj.append(l.item())
        ys.append(np.array(traj))
    print(f"three steps: kernel {got}, float64 {ys[0].tolist()}")
    assert float(np.abs(N(pipe.smpl_estimator.goal_poses) - dp_inputs[1]).max()) > 0, "the poses were not trained"
    hold("three trainer steps", {"loss": np.array(got[2:])}, {"loss": ys[1][2:]}, {"loss": ys[0][2:]}, ("loss",))


def test_append_vertices_pipeline_renders_with_the_module(dev):
    """AppendVerticesPipeline with SmplBodyModel as its smpl_model: it renders, and the vertices it was handed are the yardstick's
    (the rest of that path is unchanged)."""
    from smpl_nerf_amd import synthetic as syn
    from smpl_nerf_amd.body_model import SmplBodyModel
    from smpl_nerf_amd.nets import AppendVerticesNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import AppendVerticesPipeline, PipelineArgs
    from smpl_nerf_amd.synthetic_smpl import IndexPoseEstimator, random_smpl_arrays
    arrays = random_smpl_arrays(41, n_vertices=130)
    poses = SR.poses(3, 24, seed=42)[:, 1:].reshape(3, 69)
    body = SmplBodyModel.from_arrays(**arrays).to(dev)
    seen = {}
    body.register_forward_hook(lambda m, a, out: seen.update(vertices=out.vertices))          # (returns None: the output stays)
    torch.manual_seed(0)
    mc = AppendVerticesNet(8, 256, 60, 24, 3 * 130, skips=[4]).to(dev)
    mf = AppendVerticesNet(8, 256, 60, 24, 3 * 130, skips=[4]).to(dev)
    est = IndexPoseEstimator(torch.from_numpy(poses), torch.zeros(1, 10)).to(dev)
    args = PipelineArgs(number_coarse_samples=16, number_fine_samples=8)
    pipe = AppendVerticesPipeline(mc, mf, est, body, args, PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    data = syn.frame_batch(h=16, w=16, n_coarse=16, seed=3)
    sub = np.arange(6) * 40 + 3
    images = np.arange(6) % 3
    batch = [torch.from_numpy(data[i][sub]).to(dev) for i in range(4)] + [torch.from_numpy(images).to(dev), torch.from_numpy(data[4][sub]).to(dev)]
    with torch.no_grad():
        out = pipe(batch)
    assert tuple(out[0].shape) == (6, 3) and tuple(out[1].shape) == (6, 3) and all(torch.isfinite(o).all() for o in out[:2])
    inputs = (arrays, np.zeros((1, 10), np.float32), poses[images], np.zeros((6, 3), np.float32), None, None)
    y64, y32 = SR.restated(inputs, torch.float64, need_grad=False), SR.restated(inputs, torch.float32, need_grad=False)
    hold("AppendVerticesPipeline", {"vertices": N(seen["vertices"])}, y32, y64, ("vertices",))
