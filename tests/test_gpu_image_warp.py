"""The image-wise model on the GPU: its warp (csrc/image_warp.hip, ops.image_wise_warp), ImageWisePipeline, ImageWiseTrainer and the
ImageWiseRays data set.

Error measure: E(y) = max|y - y64| / max|y64|, y64 the float64 restatement (tests/image_wise_ref.py) of the same fp32 inputs.
Bound: E(kernel) <= 8 E(fp32 CPU restatement), both computed in the test - the yardstick is never the kernel (the policy of
tests/test_gpu_vertex_warp.py).  Every test prints its figures before it asserts (pytest -s; profiles/image_warp_errors.txt holds a
run).

Measured on an MI355X: the kernel evaluates the pairs inside the radius in float64 and rounds every output once, so its E is 6e-9 ..
5.5e-8 on every output of every case of the op and E kernel / E fp32 CPU is at most 1.0 (the fp32 CPU: 6e-9 .. 1.3e-5).  Against the
reference's own training run (g22): rgb 4.2e-6 against the fp32 CPU restatement's 1.8e-6, loss 9.8e-7 against 1.6e-7, the net's
parameters 4.7e-8 against 4.7e-8, both arm angles bit for bit - as the restatement's are, so the bound there is zero.

No sample is left out of a comparison: every case asserts on its float64 inputs that no pair lies within a relative 1e-4 of the
radius (the ReLU's kink, where fp32 and float64 may decide differently) and none within 1e-4 of a vertex (the norm's); SEEDS holds
the first seed of tests/image_wise_ref.op_inputs for which that is so (seed 1 but for one case)."""
import numpy as np
import pytest
import torch

import image_wise_ref as IR

pytestmark = pytest.mark.gpu
FACTOR = 8.0
RAGGED_SLABS = (17, 63, 70)       # 1071 samples = 17 chunks: slabs of 8, 8 and 1 chunks, the last chunk 47 samples
SHAPES = [(1, 1, 1), (1, 1, 5), (2, 7, 63), (3, 65, 17), (1, 64, 64), (5, 64, 65), (1, 100, 6890), RAGGED_SLABS]
RADII = [0.01, 0.05, 10.0]
PLANT = {0.01: 0.01, 0.05: 0.05, 10.0: 0.01}        # r = 10: planted as for 1 cm, every vertex in radius
SEEDS = {((5, 64, 65), 0.05): 2}
NAMES = ("warp", "d_goal", "d_canon", "d_samples")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def case_inputs(shape, radius):
    inputs = IR.op_inputs(*shape, PLANT[radius], SEEDS.get((tuple(shape), radius), 1))
    margin, dmin = IR.radius_margin(inputs[0], inputs[1], radius)
    assert margin > 1e-4 and dmin >= 1e-4, f"the inputs sit on a discontinuity of the gradient: |d - r| / r {margin:.2e}, d {dmin:.2e}"
    return inputs


def on_gpu(dev, inputs, radius, which=(0, 1, 2), want_samples=True, lead=False, eps=IR.EPS):
    """The op and its backward: dict of numpy arrays, d_samples with the identity paths as autograd returns it."""
    from smpl_nerf_amd import ops
    samples, goal, canon, ray_o, grads = inputs
    p, g, c, o = (torch.from_numpy(a).to(dev) for a in (samples, goal, canon, ray_o))
    if lead:
        g, c = g[None], c[None]
    g.requires_grad_(True)
    c.requires_grad_(True)
    p.requires_grad_(want_samples)
    out = ops.image_wise_warp(p, g, c, o, radius, eps)
    B, S = samples.shape[:2]
    assert all(tuple(t.shape) == (B * S, 3) for t in out)
    sum((out[i] * torch.from_numpy(grads[i]).to(dev)).sum() for i in which).backward()
    assert g.grad.shape == g.shape and c.grad.shape == c.shape
    # the layout of ops.vertex_attention_warp: the two derived outputs are the fp32 sums of the first, exactly
    assert torch.equal(out[1].view(B, S, 3), p.detach() + out[0].view(B, S, 3))
    assert torch.equal(out[2].view(B, S, 3), out[1].view(B, S, 3) - o[:, None, :])
    r = {"warp": out[0], "warped": out[1], "sdirs": out[2], "d_goal": g.grad.reshape(-1, 3), "d_canon": c.grad.reshape(-1, 3)}
    if want_samples:
        r["d_samples"] = p.grad
    return {k: N(v) for k, v in r.items()}


def restated(inputs, radius, dtype, which=(0, 1, 2)):
    return IR.reference_grads(*inputs, radius, dtype, use=which)


def hold(tag, got, y32, y64, names):
    for k in names:
        ek, ec = IR.relative_error(got[k], y64[k]), IR.relative_error(y32[k], y64[k])
        print(f"{tag} {k}: E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  max|y64| {np.abs(y64[k]).max():.3e}")
        assert np.isfinite(got[k]).all(), f"{tag} {k}: non-finite values"
        assert ek <= FACTOR * ec, f"{tag} {k}: E kernel {ek:.3e} > {FACTOR} x E fp32 CPU {ec:.3e}"


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("B,S,V", SHAPES)
def test_forward_and_backward_shapes(dev, B, S, V, radius):
    """warp, d_goal, d_canon, d_samples with all three incoming gradients: the quad tail, a ragged chunk, empty wave slices, more than
    one vertex tile, 6890 vertices, and three sample slabs of which the last is ragged."""
    from smpl_nerf_amd import _lib
    if (B, S, V) == RAGGED_SLABS:
        assert _lib.load().snerf_image_warp_bwd_workspace_bytes(B * S, V) == 3 * V * 48 and (B * S) % 64 and -(-B * S // 64) % 8
    inputs = case_inputs((B, S, V), radius)
    y64, y32 = restated(inputs, radius, torch.float64), restated(inputs, radius, torch.float32)
    got = on_gpu(dev, inputs, radius)
    got["d_samples"] = got["d_samples"].reshape(B, S, 3)
    if B * S > 1 or radius == 10.0:
        assert (np.abs(y64["warp"]).max(-1) > 0).any(), "no sample is in any radius: the case would test nothing"
    if radius == 10.0:
        assert IR.radius_margin(inputs[0], inputs[1], radius)[0] > 0.5      # every vertex, far from the rim
    hold(f"[{B},{S},{V}] r={radius}", got, y32, y64, NAMES)


def test_d_goal_equals_the_expanded_body_summed_over_the_rays(dev):
    """What a user of the per-ray op has to do: the body expanded to [B, V, 3], the float64 gradient summed over B."""
    import vertex_warp_ref as VR
    B, S, V, radius = 5, 64, 65, 0.01
    inputs = case_inputs((B, S, V), radius)
    samples, goal, canon, ray_o, grads = inputs
    y = {}
    for dtype in (torch.float64, torch.float32):
        T = lambda a: torch.tensor(a, dtype=dtype)      # noqa: E731
        g = T(goal)[None].expand(B, V, 3).clone().requires_grad_(True)
        c = T(canon)[None].expand(B, V, 3).clone().requires_grad_(True)
        x = torch.relu(radius - VR._pairs(T(samples), g))
        a = x / (x.sum(-1, keepdim=True) + IR.EPS)
        out = VR._finish(T(samples), g, c, T(ray_o), a)
        sum((out[i].reshape(-1, 3) * T(grads[i])).sum() for i in range(3)).backward()
        y[dtype] = {"d_goal": g.grad.sum(0).numpy(), "d_canon": c.grad.sum(0).numpy()}
    hold("expanded body", on_gpu(dev, inputs, radius), y[torch.float32], y[torch.float64], ("d_goal", "d_canon"))


def test_no_sample_in_any_radius(dev):
    """warp == 0 exactly (0 / eps), the samples unmoved, all gradients zero: every element is written."""
    samples, goal, canon, ray_o, grads = IR.op_inputs(3, 70, 130, 0.01, seed=2)
    samples = (samples + np.float32(5.0)).astype(np.float32)                 # the body lives within ~1.5 of the origin
    assert IR.radius_margin(samples, goal, 0.01)[0] > 100.0
    got = on_gpu(dev, (samples, goal, canon, ray_o, grads), 0.01)
    for k in ("warp", "d_goal", "d_canon"):
        assert np.array_equal(got[k], np.zeros_like(got[k])), k
    assert np.array_equal(got["warped"], samples.reshape(-1, 3))
    assert np.array_equal(got["d_samples"], (grads[1] + grads[2]).reshape(samples.shape))      # only the identity paths


def test_sample_exactly_on_a_vertex(dev):
    """d = 0: finite gradients and no distance term from that pair (torch.norm's convention), as float64 autograd has it."""
    radius = 0.05
    samples, goal, canon, ray_o, grads = IR.op_inputs(2, 9, 40, radius, seed=5)
    samples[1, 3] = goal[7]
    samples[0, 0] = goal[0]
    inputs = (samples, goal, canon, ray_o, grads)
    margin, dmin = IR.radius_margin(samples, goal, radius)
    assert margin > 1e-4 and dmin == 0.0
    y64, y32 = restated(inputs, radius, torch.float64), restated(inputs, radius, torch.float32)
    got = on_gpu(dev, inputs, radius)
    hold("d = 0", got, y32, y64, NAMES)
    # a lone pair at d = 0: x = r, warp = w r / (r + eps), and the only gradient of the goal vertex is through w
    one = (goal[:1].copy(), goal[:1], canon[:1], ray_o[:1], [g[:1] for g in grads])
    got = on_gpu(dev, (one[0][None], *one[1:]), radius, which=(0,))
    a = np.float32(radius) / (np.float32(radius) + np.float32(IR.EPS))
    assert np.allclose(got["d_canon"], a * one[4][0], rtol=1e-6, atol=0) and np.array_equal(got["d_goal"], -got["d_canon"])
    assert np.array_equal(got["d_samples"], np.zeros((1, 1, 3), np.float32))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_backward_with_one_incoming_gradient(dev, which):
    """Only d warp, only d warped or only d sdirs arrives, and the samples need no gradient (d_samples NULL)."""
    inputs = case_inputs((5, 64, 65), 0.01)
    y64, y32 = restated(inputs, 0.01, torch.float64, (which,)), restated(inputs, 0.01, torch.float32, (which,))
    got = on_gpu(dev, inputs, 0.01, (which,), want_samples=False)
    hold(f"only gradient {which}", got, y32, y64, ("d_goal", "d_canon"))


def test_no_grad_call_keeps_nothing_and_agrees(dev):
    from smpl_nerf_amd import ops
    samples, goal, canon, ray_o, _ = case_inputs((5, 64, 65), 0.01)
    p, g, c, o = (torch.from_numpy(a).to(dev) for a in (samples, goal, canon, ray_o))
    with torch.no_grad():
        plain = ops.image_wise_warp(p, g, c, o, 0.01)
    tracked = ops.image_wise_warp(p, g.clone().requires_grad_(True), c, o, 0.01)
    assert all(t.grad_fn is None for t in plain) and all(t.grad_fn is not None for t in tracked)
    assert all(torch.equal(a, b) for a, b in zip(plain, tracked))


@pytest.mark.parametrize("radius", [0.01, 10.0])
def test_two_runs_and_both_body_shapes_are_bit_identical(dev, radius):
    """Forward, d_goal, d_canon and d_samples: the same bits twice, and with the body as [V, 3] and as [1, V, 3]."""
    inputs = case_inputs(RAGGED_SLABS, radius)
    a, b, c = on_gpu(dev, inputs, radius), on_gpu(dev, inputs, radius), on_gpu(dev, inputs, radius, lead=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], c[k]), k


def test_operator_refuses_more_than_one_body(dev):
    from smpl_nerf_amd import ops
    p, g, o = torch.rand(2, 5, 3, device=dev), torch.rand(2, 9, 3, device=dev), torch.rand(2, 3, device=dev)
    with pytest.raises(RuntimeError, match="one body"):
        ops.image_wise_warp(p, g, g, o, 0.01)
    with pytest.raises(RuntimeError, match="must match"):
        ops.image_wise_warp(p, g[0], g[0], o[:1], 0.01)


# ---------------------------------------------------------------------------------------------- ImageWisePipeline / ImageWiseTrainer
def _trainer(dev):
    import copy
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import ImageWisePipeline, PipelineArgs
    from smpl_nerf_amd.synthetic_smpl import ArmAngleEstimator
    from smpl_nerf_amd.trainer import ImageWiseTrainer
    c = IR.G22
    images, body, params = IR.g22_inputs()
    net = RenderRayNet(8, 256, 60, 24, skips=[4])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    truth = torch.zeros(1, 69)
    truth[0, 38], truth[0, 41] = c["truth_l"], c["truth_r"]
    est = ArmAngleEstimator(c["arm_angle_l"], c["arm_angle_r"], ground_truth_pose=truth)
    args = PipelineArgs(run_fine=0, warp_radius=c["radius"])
    pipe = ImageWisePipeline(net.to(dev), net, est.to(dev), copy.deepcopy(body).to(dev), args, PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    return ImageWiseTrainer(pipe, lr=c["lrate"], lr_pose=c["lrate_pose"]), [[torch.from_numpy(a).to(dev) for a in im] for im in images]


@pytest.fixture(scope="module")
def g22():
    import json
    from conftest import load_golden
    g = load_golden("g22_image_wise.npz")
    assert json.loads(str(g["config"])) == IR.G22, "the fixture was generated with other seeds than image_wise_ref.G22"
    images, body, params = IR.g22_inputs()
    return g, IR.train_steps(images, body, params, g["step_rays"], torch.float32)


def test_pipeline_outputs_and_depth_row(dev):
    """DynamicPipeline's return tuple; one [S] row of depths and the same row for every ray give the same bits; no body, no batch."""
    trainer, images = _trainer(dev)
    pipe, c = trainer.pipeline, IR.G22
    batch = next(trainer.ray_batches(images[0], c["batchsize"]))
    with pytest.raises(RuntimeError, match="pose_image"):
        pipe(batch)
    with torch.no_grad():
        goal, canon = pipe.pose_image()
        assert tuple(goal.shape) == tuple(canon.shape) == (1, c["V"], 3)
        out = pipe(batch)
        wide = pipe(batch[:3] + [batch[3][None].expand(c["batchsize"], c["S"]).contiguous()] + batch[4:])
    B, S = c["batchsize"], c["S"]
    assert out[0] is out[1] and out[3] is batch[0]
    assert [tuple(o.shape) for o in out] == [(B, 3), (B, 3), (B, S, 3), (B, S, 3), (B, S, 3), (B, S)]
    assert all(torch.equal(a, b) for a, b in zip(out, wide))
    assert (out[2].abs().amax(-1) > 0).sum() >= B * S // 4, "the planted samples did not move"


def test_trainer_against_the_reference(dev, g22):
    """The reference's ImageWiseSolver.train for one epoch (2 images x 2 ray batches: the posed body of an image serves two
    backward passes) against the same steps of ImageWiseTrainer: per-step rgb and loss, the final arm angles, a sample of the
    net's parameters and the step counts.  E against the fixture; bound 8 x the E of the fp32 CPU restatement driven through
    the same steps, measured here against the same fixture."""
    g, cpu = g22
    c = IR.G22
    trainer, images = _trainer(dev)
    pipe = trainer.pipeline
    per_image = c["R"] // c["batchsize"]
    rgbs, losses, pose = [], [], []
    for k, rays in enumerate(g["step_rays"]):
        if k % per_image == 0:
            pipe.pose_image()
        im = images[k // per_image]
        idx = torch.from_numpy(rays).to(dev)
        loss = trainer.step([im[0][idx], im[1][idx], im[2][idx], im[3], im[4][idx]])
        rgbs.append(N(trainer.last_outputs[0]))
        losses.append(loss.item())
        pose.append(float(trainer.last_pose_loss))
    est = pipe.smpl_estimator
    flat = N(torch.cat([p.reshape(-1) for p in pipe.model_coarse.parameters()]))
    got = {"step_rgb": np.array(rgbs), "step_loss": np.array(losses), "arm_angle_l": N(est.arm_angle_l), "arm_angle_r": N(est.arm_angle_r),
           "param_sample": flat[::c["param_stride"]]}
    print("losses", losses, "fixture", g["step_loss"].tolist(), "pose losses", pose)
    print("arm angles", got["arm_angle_l"].ravel(), got["arm_angle_r"].ravel(), "fixture", g["arm_angle_l"].ravel(), g["arm_angle_r"].ravel())
    assert set(trainer.optim.steps.tolist()) == set(trainer.pose_optim.steps.tolist()) == set(g["adam_steps"].tolist()) == {len(losses)}
    assert g["step_loss"][-1] < g["step_loss"][0] and losses[-1] < losses[0], "the loss did not fall over the recorded steps"
    truth_pose = (est.arm_angle_l.item() - c["truth_l"]) ** 2 + (est.arm_angle_r.item() - c["truth_r"]) ** 2
    assert abs(pose[-1] - truth_pose) <= 1e-6 * truth_pose
    assert float(np.abs(got["arm_angle_l"] - np.float32(c["arm_angle_l"])).max()) > 1e-3, "the pose was not trained"
    hold("g22", got, cpu, g, ("step_rgb", "step_loss", "param_sample", "arm_angle_l", "arm_angle_r"))


def test_validation_runs_without_a_graph(dev):
    trainer, images = _trainer(dev)
    loss, rgb = trainer.validate_image(images[1], IR.G22["batchsize"])
    assert np.isfinite(loss) and tuple(rgb.shape) == (IR.G22["R"], 3) and rgb.grad_fn is None
    assert trainer.pipeline.goal_vertices.grad_fn is None and set(trainer.optim.steps.tolist()) == {0}


# ---------------------------------------------------------------------------------------------- ImageWiseRays
FRAMES = [(10.0, 15.0), (10.0, 55.0)]      # (phi, theta): cameras none of whose 12 x 12 rays the first-hit margins name (asserted below)
STD = 0.03


def _data_set(dev, seed=5, **kw):
    from smpl_nerf_amd import synthetic as syn
    from smpl_nerf_amd.body_model import SmplBodyModel
    from smpl_nerf_amd.image_wise import ImageWiseRays
    from smpl_nerf_amd.pipelines import PipelineArgs
    from smpl_nerf_amd.synthetic_smpl import ArmAngleEstimator, surface_smpl_arrays
    body = SmplBodyModel.from_arrays(**surface_smpl_arrays(11, level=2)).to(dev)
    est = ArmAngleEstimator(0.3, -0.2).to(dev)
    h = w = 12
    images = (np.stack([syn.procedural_image(h, w, p, t) for p, t in FRAMES]) * 255).astype(np.uint8)
    transforms = np.stack([syn.sphere_pose(p, t, 2.4) for p, t in FRAMES])
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    args = PipelineArgs(near=1.0, far=4.0, std_dev_coarse_sample_prior=STD, **kw)
    return ImageWiseRays(images, transforms, 0.6, est, body, args, dev, generator=gen), body, est, images


def test_data_set_one_sample_is_the_first_hit_distance(dev):
    """S = 1: z is the metric distance |hit - o| of the first hit along get_rays' un-normalised directions, `far` on a miss,
    against the float64 restatement of the same fp32 rays and body.  No ray is left out: the margins' rays are asserted absent."""
    import single_sample_ref as SS
    ds, body, est, images = _data_set(dev, number_coarse_samples=1)
    assert len(ds) == 2
    pose, betas = est(1)
    goal = N(body(betas=betas, body_pose=pose).vertices[0])
    f = N(body.faces)
    for i in range(2):
        samples, o, d, z, rgb = ds.image(i, per_ray_z=True)
        assert [tuple(t.shape) for t in (samples, o, d, z, rgb)] == [(144, 1, 3), (144, 3), (144, 3), (144, 1), (144, 3)]
        assert all(t.dtype == torch.float32 and t.grad_fn is None for t in (samples, o, d, z, rgb))
        assert np.array_equal(N(rgb), images[i].reshape(-1, 3).astype(np.float32) / np.float32(255))
        assert float((torch.linalg.vector_norm(d.double(), dim=-1) - 1).abs().max()) > 1e-3      # get_rays' directions: not unit vectors
        assert torch.equal(samples, o[:, None, :] + d[:, None, :] * z[:, :, None])
        assert tuple(ds.image(i)[3].shape) == (1,) and torch.equal(ds.image(i)[3], z[-1])         # the reference's one row: the last ray's
        oi, di = N(o), N(d)
        left_out, gap = SS.first_hit_margin(oi, di, goal, f)
        assert left_out.sum() == 0, f"frame {i}: {int(left_out.sum())} rays sit on a margin of the first-hit rule"
        y64, y32 = (SS.first_hit(*(torch.from_numpy(a).to(dt) for a in (oi, di, goal)), f, torch.from_numpy(goal).to(dt))["depth"]
                    for dt in (torch.float64, torch.float32))
        hit = y64 > 0
        got = N(z[:, 0])
        assert 20 <= hit.sum() <= 120 and np.array_equal(N(ds.last_n_hits) > 0, hit)
        assert np.array_equal(got[~hit], np.full((~hit).sum(), 4.0, np.float32))
        ek, ec = IR.relative_error(got[hit], y64[hit]), IR.relative_error(y32[hit], y64[hit])
        print(f"data set frame {i}: hit {int(hit.sum())} of 144, smallest gap {gap:.2e}; z E kernel {ek:.3e}  E fp32 CPU {ec:.3e}")
        assert ek <= FACTOR * ec


@pytest.mark.parametrize("mode", ["coarse_samples_from_intersect", "coarse_samples_from_prior"])
def test_data_set_gaussian_modes(dev, mode):
    """Sorted rows (from_intersect), finite values, a hit ray's mean within 6 std / sqrt(S) of its first hit (from_intersect) or of
    the mean of its hits (from_prior: the equal-weight mixture; their spread adds to the variance), and the jittered bins - ONE
    jitter for the image - on every ray without a hit.  The same seed gives the same bits."""
    S = 64
    ds = _data_set(dev, number_coarse_samples=S, **{mode: 1})[0]
    again = _data_set(dev, number_coarse_samples=S, **{mode: 1})[0]
    from smpl_nerf_amd.raygen import coarse_bin_tables
    lower, span = (torch.as_tensor(t, dtype=torch.float32, device=dev) for t in coarse_bin_tables(1.0, 4.0, S))
    for i in range(2):
        samples, o, d, z, _ = ds.image(i, per_ray_z=True)
        assert all(torch.equal(a, b) for a, b in zip((samples, z), (lambda im: (im[0], im[3]))(again.image(i, per_ray_z=True))))
        assert tuple(z.shape) == (144, S) and bool(torch.isfinite(z).all()) and bool(torch.isfinite(samples).all())
        hit = ds.last_n_hits > 0
        assert 20 <= int(hit.sum()) <= 120
        first = ds.last_first_hit
        if mode == "coarse_samples_from_intersect":
            assert bool((z[hit][:, 1:] >= z[hit][:, :-1]).all())
            centre, spread2 = first[hit], torch.zeros_like(first[hit])
        else:
            from smpl_nerf_amd import ops
            pose, betas = ds.smpl_estimator(1)
            goal = ds.body_model(betas=betas, body_pose=pose).vertices[0]
            t_hits, n_hits = ops.ray_mesh_hits(o, d, goal, ds.faces, 16)
            assert torch.equal(n_hits, ds.last_n_hits) and int(n_hits.max()) <= 16 and int(n_hits.max()) >= 2
            t_hits = torch.where(torch.isfinite(t_hits), t_hits * torch.norm(d, dim=-1, keepdim=True), torch.zeros_like(t_hits))
            n = n_hits.clamp(min=1)[:, None].float()
            centre = (t_hits.sum(1, keepdim=True) / n)[hit][:, 0]
            mask = (torch.arange(16, device=dev)[None, :] < n_hits[:, None])
            spread2 = (((t_hits - t_hits.sum(1, keepdim=True) / n) ** 2 * mask).sum(1, keepdim=True) / n)[hit][:, 0]
        off = (z[hit].mean(1) - centre).abs() / torch.sqrt((STD ** 2 + spread2) / S)
        print(f"{mode} frame {i}: hit {int(hit.sum())}, largest |row mean - centre| / (sigma / sqrt(S)) = {float(off.max()):.2f}")
        assert float(off.max()) <= 6.0
        # a ray with no hit gets the jittered bins: lower + span * u with ONE u in [0, 1) for the whole image
        miss = z[~hit]
        assert bool((miss == miss[:1]).all())
        u = ((miss[0] - lower) / span)
        assert 0.0 <= float(u.min()) and float(u.max()) < 1.0 and float(u.max() - u.min()) < 1e-4


def test_fit_trains_the_pose_through_the_skinned_body(dev):
    """The whole loop on the device: ImageWiseRays samples every image with the estimator's current pose, ImageWiseTrainer.fit poses
    the skinned body (the SMPL kernels of body_model.SmplBodyModel) once per image and back-propagates both ray batches of the
    image through it."""
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import ImageWisePipeline
    from smpl_nerf_amd.trainer import ImageWiseTrainer
    from smpl_nerf_amd import synthetic as syn
    ds, body, est, _ = _data_set(dev, number_coarse_samples=8, coarse_samples_from_intersect=1, warp_radius=0.05, run_fine=0)
    net = RenderRayNet(8, 256, 60, 24, skips=[4])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scene_net_params(402).items()})
    pipe = ImageWisePipeline(net.to(dev), net, est, body, ds.args, PositionalEncoder(10, 0), PositionalEncoder(4, 0))
    trainer = ImageWiseTrainer(pipe, lr=2e-5, lr_pose=1e-3)
    before = (est.arm_angle_l.item(), est.arm_angle_r.item())
    hist = trainer.fit(ds, val_images=[ds.image(0)], num_epochs=1, batch_size=72, log=lambda *a: None)
    assert all(len(v) == 1 and np.isfinite(v[0]) for v in hist.values()) and hist["train_loss"][0] > 0
    assert set(trainer.optim.steps.tolist()) == set(trainer.pose_optim.steps.tolist()) == {4}          # 2 images x 2 batches of 72 rays
    after = (est.arm_angle_l.item(), est.arm_angle_r.item())
    print("fit:", hist, "arm angles", before, "->", after)
    assert all(np.isfinite(a) and a != b for a, b in zip(after, before)), "the loss did not reach the arm angles"
