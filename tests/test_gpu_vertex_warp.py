"""The vertex-attention warp (csrc/vertex_warp.hip, ops.vertex_attention_warp) and DynamicPipeline on the GPU.

Error measure: E(y) = max|y - y64| / max|y64|, y64 the float64 stable restatement (tests/vertex_warp_ref.py) of the same fp32 inputs.
Bound: E(kernel) <= 8 E(fp32 CPU restatement), both computed in the test - the yardstick is never the kernel.  The factor covers
another summation order over up to 6890 terms and re-ordered distance arithmetic, which the temperature amplifies.  Every test prints
its figures before it asserts (pytest -s; profiles/vertex_warp_errors.txt holds a run).

Measured on an MI355X (profiles/vertex_warp_errors.txt has every figure): E kernel / E fp32 CPU is 0.1 .. 2.6 over the cases of the op
(warp 7e-9 .. 8e-7, gradients 2e-8 .. 4e-6; [2,7,63] at T = 1e4 is ill-conditioned for both: 5e-4 against 9e-4), 4.0 for the pipeline's
loss (1.5e-7, one ulp), 0.95 .. 1.0 for d loss / d goal_poses (2.7e-4 and 2.1e-3 for both: the MLP's input gradients) and 0.9 for the
loss of three Adam steps.

Inputs keep away from the two places where the gradient is discontinuous: |d - r| >= 4e-6 (the ReLU; about 16 ulp of the largest
coordinate) and d >= 1e-4 (the norm), asserted on the CPU for every case; no case is left out."""
import numpy as np
import pytest
import torch

import vertex_warp_ref as VR
from conftest import load_golden

pytestmark = pytest.mark.gpu
FACTOR = 8.0
SHAPES = [(1, 1, 1), (2, 7, 63), (3, 64, 65), (2, 65, 1000), (1, 100, 6890), (5, 64, 257)]
REGIMES = [(0.01, 1e4), (0.05, 100.0)]        # the defaults (a hit is rare, x up to 100); many hits per sample, small x


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def restated(inputs, radius, temperature, dtype, which, want_samples=True):
    """The stable restatement and its autograd gradients on the CPU: dict of numpy arrays."""
    samples, goal, canon, ray_o, grads = inputs
    p, g, c, o = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (samples, goal, canon, ray_o))
    out = VR.warp_stable(p, g, c, o, radius, temperature)
    sum((out[i].reshape(-1, 3) * torch.from_numpy(grads[i]).to(dtype)).sum() for i in which).backward()
    r = {"warp": out[0], "warped": out[1], "sdirs": out[2], "d_goal": g.grad, "d_canon": c.grad}
    if want_samples:
        r["d_samples"] = p.grad
    return {k: N(v) for k, v in r.items()}


def on_gpu(dev, inputs, radius, temperature, which, want_samples=True):
    from smpl_nerf_amd import ops
    samples, goal, canon, ray_o, grads = inputs
    p, g, c, o = (torch.from_numpy(a).to(dev) for a in (samples, goal, canon, ray_o))
    g.requires_grad_(True)
    c.requires_grad_(True)
    p.requires_grad_(want_samples)
    out = ops.vertex_attention_warp(p, g, c, o, radius, temperature)
    assert all(tuple(t.shape) == (samples.shape[0] * samples.shape[1], 3) for t in out)
    sum((out[i] * torch.from_numpy(grads[i]).to(dev)).sum() for i in which).backward()
    r = {"warp": out[0], "warped": out[1], "sdirs": out[2], "d_goal": g.grad, "d_canon": c.grad}
    if want_samples:
        r["d_samples"] = p.grad
    B, S = samples.shape[:2]
    # the two derived outputs are the fp32 sums of the first, exactly
    assert torch.equal(out[1].view(B, S, 3), p.detach() + out[0].view(B, S, 3))
    assert torch.equal(out[2].view(B, S, 3), out[1].view(B, S, 3) - o[:, None, :])
    return {k: N(v).reshape(restated_shape(k, samples, goal)) for k, v in r.items()}


def restated_shape(name, samples, goal):
    return goal.shape if name in ("d_goal", "d_canon") else samples.shape


def hold(tag, got, y32, y64, names):
    worst = 0.0
    for k in names:
        ek, ec = VR.relative_error(got[k], y64[k]), VR.relative_error(y32[k], y64[k])
        print(f"{tag} {k}: E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  max|y64| {np.abs(y64[k]).max():.3e}")
        assert np.isfinite(got[k]).all(), f"{tag} {k}: non-finite values"
        assert ek <= FACTOR * ec, f"{tag} {k}: E kernel {ek:.3e} > {FACTOR} x E fp32 CPU {ec:.3e}"
        worst = max(worst, ek / ec if ec else 0.0)
    return worst


def margins_ok(inputs, radius):
    near, zero = VR.input_margins(inputs[0], inputs[1], radius)
    assert near >= 4e-6 and zero >= 1e-4, f"the inputs sit on a discontinuity of the gradient: |d - r| {near:.2e}, d {zero:.2e}"


@pytest.mark.parametrize("radius,temperature", REGIMES)
@pytest.mark.parametrize("B,S,V", SHAPES)
def test_forward_and_backward_shapes(dev, B, S, V, radius, temperature):
    """warp, d_samples, d_goal, d_canon with all three incoming gradients, at sizes around the 64-sample chunk, the 16 vertex slices
    of the forward and the 64-vertex tiles of the backward."""
    inputs = VR.op_inputs(B, S, V, radius, seed=1)
    margins_ok(inputs, radius)
    y64 = restated(inputs, radius, temperature, torch.float64, (0, 1, 2))
    y32 = restated(inputs, radius, temperature, torch.float32, (0, 1, 2))
    got = on_gpu(dev, inputs, radius, temperature, (0, 1, 2))
    if V > 1:
        assert (np.abs(y64["warp"]).max(-1) > 0).any(), "no sample is in any radius: the case would test nothing"
    hold(f"[{B},{S},{V}] r={radius} T={temperature}", got, y32, y64, ("warp", "d_samples", "d_goal", "d_canon"))


def test_no_sample_in_any_radius(dev):
    """Exact zeros everywhere (and the samples unmoved), all finite: every element is written."""
    samples, goal, canon, ray_o, grads = VR.op_inputs(3, 70, 130, 0.01, seed=2)
    samples = (samples + np.float32(5.0)).astype(np.float32)                 # the bodies live within ~1.5 of the origin
    inputs = (samples, goal, canon, ray_o, grads)
    assert VR.input_margins(samples, goal, 0.01)[0] > 1.0
    got = on_gpu(dev, inputs, 0.01, 1e4, (0, 1, 2))
    for k in ("warp", "d_goal", "d_canon"):
        assert np.array_equal(got[k], np.zeros_like(got[k])), k
    assert np.array_equal(got["warped"], samples)
    assert np.array_equal(got["d_samples"], (grads[1] + grads[2]).reshape(samples.shape))      # only the identity paths


def test_every_vertex_in_radius(dev):
    inputs = VR.op_inputs(2, 33, 150, 0.01, seed=3)        # (planted as for the 1 cm radius: the bodies and samples span ~2.5)
    margins_ok(inputs, 10.0)
    assert VR.input_margins(inputs[0], inputs[1], 10.0)[0] > 5.0              # all of them, far from the rim
    y64 = restated(inputs, 10.0, 0.5, torch.float64, (0, 1, 2))
    y32 = restated(inputs, 10.0, 0.5, torch.float32, (0, 1, 2))
    got = on_gpu(dev, inputs, 10.0, 0.5, (0, 1, 2))
    hold("all in radius", got, y32, y64, ("warp", "d_samples", "d_goal", "d_canon"))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_backward_with_one_incoming_gradient(dev, which):
    """Only d warp, only d warped or only d sdirs arrives, and the samples need no gradient (d_samples NULL)."""
    inputs = VR.op_inputs(3, 64, 65, 0.01, seed=1)
    margins_ok(inputs, 0.01)
    y64 = restated(inputs, 0.01, 1e4, torch.float64, (which,), want_samples=False)
    y32 = restated(inputs, 0.01, 1e4, torch.float32, (which,), want_samples=False)
    got = on_gpu(dev, inputs, 0.01, 1e4, (which,), want_samples=False)
    hold(f"only gradient {which}", got, y32, y64, ("d_goal", "d_canon"))


def test_no_grad_call_keeps_nothing_and_agrees(dev):
    from smpl_nerf_amd import ops
    samples, goal, canon, ray_o, _ = VR.op_inputs(5, 64, 257, 0.01, seed=1)
    p, g, c, o = (torch.from_numpy(a).to(dev) for a in (samples, goal, canon, ray_o))
    with torch.no_grad():
        plain = ops.vertex_attention_warp(p, g, c, o, 0.01, 1e4)
    tracked = ops.vertex_attention_warp(p, g.clone().requires_grad_(True), c, o, 0.01, 1e4)
    assert all(t.grad_fn is None for t in plain) and all(t.grad_fn is not None for t in tracked)
    assert all(torch.equal(a, b) for a, b in zip(plain, tracked))


@pytest.mark.parametrize("radius,temperature", REGIMES)
def test_two_runs_are_bit_identical(dev, radius, temperature):
    inputs = VR.op_inputs(5, 100, 257, radius, seed=1)
    a = on_gpu(dev, inputs, radius, temperature, (0, 1, 2))
    b = on_gpu(dev, inputs, radius, temperature, (0, 1, 2))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- DynamicPipeline
def _pipeline(dev, params, poses, body, temperature, trainable=True):
    import copy
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import DynamicPipeline, PipelineArgs
    from smpl_nerf_amd.synthetic_smpl import IndexPoseEstimator
    net = RenderRayNet(8, 256, 60, 24, skips=[4])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    est = IndexPoseEstimator(torch.from_numpy(poses), torch.zeros(1, 10), trainable_poses=trainable)
    args = PipelineArgs(run_fine=1, warp_radius=VR.G17["radius"], warp_temperature=temperature)     # (coarse only whatever run_fine says)
    return DynamicPipeline(net.to(dev), net, est.to(dev), copy.deepcopy(body).to(dev), args, PositionalEncoder(10, 0), PositionalEncoder(4, 0))


def _cpu_pipeline_step(params, poses, body, batch_np, temperature, dtype):
    """(loss, d loss / d goal_poses, parameters, poses tensor) of the torch restatement of the whole pipeline."""
    import copy
    P = {k: torch.from_numpy(v).to(dtype).clone().requires_grad_(True) for k, v in params.items()}      # (clones: the steps write)
    gp = torch.from_numpy(poses).to(dtype).clone().requires_grad_(True)
    b = copy.deepcopy(body).to(dtype)
    batch = [torch.from_numpy(a) if a.dtype.kind in "iu" else torch.from_numpy(a).to(dtype) for a in batch_np]
    return P, gp, lambda: torch.nn.functional.mse_loss(VR.dynamic_pipeline(P, b, gp, batch, VR.G17["radius"], temperature)[0], batch[5])


@pytest.fixture(scope="module")
def g17():
    return load_golden("g17_dynamic.npz"), VR.g17_inputs()


@pytest.mark.parametrize("case", ["a", "b"])
def test_dynamic_pipeline_against_the_reference(dev, g17, case):
    """Forward against what the reference rendered (the tolerances SmplNerfPipeline's coarse outputs are held to), then loss and
    d loss / d goal_poses by the float64 rule.  Case a is the parser's default temperature, where the reference's own fp32 backward
    divides by sums of numbers near e^-88 (its finiteness is recorded in the fixture, not relied on); case b the milder one whose
    reference gradient the fixture holds."""
    g, (batch_np, poses, body, params) = g17
    temperature = VR.G17["cases"][case]
    pipe = _pipeline(dev, params, poses, body, temperature)
    batch = [torch.from_numpy(a).to(dev) for a in batch_np]
    with torch.no_grad():
        out = pipe(batch)
    assert out[0] is out[1] and out[3] is batch[0]
    assert [tuple(o.shape) for o in out] == [(12, 3), (12, 3), (12, 64, 3), (12, 64, 3), (12, 64, 3), (12, 64)]
    for i, name, tol in ((0, "rgb", 1e-5), (2, "warp", 2e-6), (4, "warped", 2e-6), (5, "densities", 5e-5)):
        err = float(np.abs(N(out[i]).astype(np.float64) - g[f"{case}_{name}"]).max())
        print(f"case {case} {name}: max abs error against the reference {err:.3e} (tolerance {tol})")
        assert err <= tol, (name, err)
    loss = torch.nn.functional.mse_loss(pipe(batch)[0], batch[5])
    loss.backward()
    got = {"loss": np.array([loss.item()]), "grad": N(pipe.smpl_estimator.goal_poses.grad)}
    ys = []
    for dtype in (torch.float64, torch.float32):
        P, gp, step = _cpu_pipeline_step(params, poses, body, batch_np, temperature, dtype)
        l = step()
        l.backward()
        ys.append({"loss": np.array([l.item()]), "grad": N(gp.grad)})
    assert np.isfinite(got["grad"]).all() and np.abs(ys[0]["grad"]).max() > 0
    print(f"case {case}: reference's own fp32 gradient finite: {int(g[f'{case}_grad_finite'][0])}; loss {got['loss'][0]:.8f} "
          f"(reference {g[f'{case}_loss'][0]:.8f})")
    assert abs(got["loss"][0] - g[f"{case}_loss"][0]) <= 1e-5
    if case == "b":
        print(f"case b: E of the reference's fp32 gradient {VR.relative_error(g['b_goal_poses_grad'], ys[0]['grad']):.3e}")
    hold(f"case {case}", got, ys[1], ys[0], ("loss", "grad"))


def test_three_adam_steps(dev, g17):
    """NeRF and estimator poses trained together through the warp: the loss trajectory against the same three steps in float64."""
    g, (batch_np, poses, body, params) = g17
    temperature, lr = VR.G17["cases"]["a"], 2e-5      # (at the reference's 5e-4 one Adam step empties this synthetic scene: sigma <= 0 everywhere)
    pipe = _pipeline(dev, params, poses, body, temperature)
    batch = [torch.from_numpy(a).to(dev) for a in batch_np]
    opt = torch.optim.Adam([p for p in pipe.parameters() if p.requires_grad], lr=lr)
    got = []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(pipe(batch)[0], batch[5])
        loss.backward()
        opt.step()
        got.append(loss.item())
    ys = []
    for dtype in (torch.float64, torch.float32):
        P, gp, step = _cpu_pipeline_step(params, poses, body, batch_np, temperature, dtype)
        opt = torch.optim.Adam(list(P.values()) + [gp], lr=lr)
        traj = []
        for _ in range(3):
            opt.zero_grad()
            l = step()
            l.backward()
            opt.step()
            traj.append(l.item())
        ys.append(np.array(traj))
    assert got[2] < got[0], "three steps did not lower the loss"
    assert float(np.abs(N(pipe.smpl_estimator.goal_poses) - poses).max()) > 0, "the poses were not trained"
    hold("three Adam steps", {"loss": np.array(got)}, {"loss": ys[1]}, {"loss": ys[0]}, ("loss",))
