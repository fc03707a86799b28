"""CPU-side checks of the image-wise model's warp (csrc/image_warp.hip, ops.image_wise_warp): the closed-form gradients the kernels
evaluate equal float64 autograd of the reference's expression, the three C entry points exist, agree with the header and the
ctypes table and validate their arguments before touching a device, and the workspace query's arithmetic.  No GPU needed,
nothing launched."""
import re

import numpy as np
import pytest
import torch

import image_wise_ref as IR
from smpl_nerf_amd import _lib, build

ENTRIES = (("snerf_image_warp_fwd_f32", 14), ("snerf_image_warp_bwd_workspace_bytes", 2), ("snerf_image_warp_bwd_f32", 17))


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("B,S,V,radius,seed", [(3, 17, 40, 0.05, 1), (2, 9, 7, 10.0, 2), (5, 8, 300, 0.01, 3)])
def test_closed_form_gradients_equal_float64_autograd(B, S, V, radius, seed):
    """Bound 1e-12 relative to the largest element of each gradient: both sides are float64, the orders of summation differ."""
    samples, goal, canon, ray_o, grads = IR.op_inputs(B, S, V, radius, seed)
    samples[0, 0] = goal[V // 2]                           # one sample exactly on a vertex: d = 0, no distance term
    margin, dmin = IR.radius_margin(samples, goal, radius)
    assert margin > 1e-4 and dmin == 0.0
    ref = IR.reference_grads(samples, goal, canon, ray_o, grads, radius, torch.float64, use=(0,))
    assert (np.abs(ref["warp"]).max(-1) > 0).sum() >= (B * S) // 4          # the attention is exercised
    d_goal, d_canon, d_samples = IR.closed_form_grads(samples, goal, canon, grads[0], radius)
    for name, mine in (("d_goal", d_goal), ("d_canon", d_canon), ("d_samples", d_samples)):
        e = IR.relative_error(mine, ref[name])
        print(f"closed form {name} B={B} S={S} V={V} r={radius}: E = {e:.3e}")
        assert np.abs(ref[name]).max() > 0 and e <= 1e-12, (name, e)


def test_body_shapes_and_identity_paths_of_the_restatement():
    samples, goal, canon, ray_o, grads = IR.op_inputs(2, 5, 11, 0.05, 4)
    T = torch.from_numpy
    a = IR.warp_linear(T(samples), T(goal), T(canon), T(ray_o), 0.05)
    b = IR.warp_linear(T(samples), T(goal)[None], T(canon)[None], T(ray_o), 0.05)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(a[1], T(samples) + a[0]) and torch.equal(a[2], a[1] - T(ray_o)[:, None, :])
    # all three incoming gradients: the closed forms plus the identity paths of warped and sdirs
    ref = IR.reference_grads(samples, goal, canon, ray_o, grads, 0.05, torch.float64)
    dW = sum(g.astype(np.float64) for g in grads)
    d_goal, d_canon, d_samples = IR.closed_form_grads(samples, goal, canon, dW, 0.05)
    ident = (grads[1].astype(np.float64) + grads[2]).reshape(samples.shape)
    assert IR.relative_error(d_samples + ident, ref["d_samples"]) <= 1e-12
    assert IR.relative_error(d_goal, ref["d_goal"]) <= 1e-12 and IR.relative_error(d_canon, ref["d_canon"]) <= 1e-12


def test_symbols_are_exported_and_prototyped(lib):
    text = open(_lib.HERE + "/../include/smplnerf.h").read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in ENTRIES:
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", code)
        assert proto and len(proto.group(1).split(",")) == nargs, name
    assert "image_warp.hip" in build.SOURCES
    assert lib.snerf_version() == 109


def test_workspace_query(lib):
    q = lib.snerf_image_warp_bwd_workspace_bytes

    def slabs(n):
        chunks = (n + 63) // 64
        per = max(8, (chunks + 63) // 64)
        return (chunks + per - 1) // per

    for n, v in ((0, 5), (1, 1), (64 * 8, 3), (64 * 8 + 1, 3), (64 * 64, 6890), (17 * 64 - 17, 70), (128 * 128 * 64, 6890),
                 (128 * 128 * 64 + 1, 6890)):
        assert q(n, v) == slabs(n) * v * 48, (n, v)
    assert slabs(64 * 64) == 8 and slabs(128 * 128 * 64) == 64 and slabs(17 * 64 - 17) == 3       # > 1 slab at 64 rays; a ragged third
    assert q(128 * 128 * 64, 6890) == 64 * 6890 * 48                                               # O(slabs V): 21 MB, whatever B is
    assert q(-1, 5) == -1 and b"N" in lib.snerf_last_error_string()
    assert q(10, 0) == -1 and b"V" in lib.snerf_last_error_string()
    assert q(1 << 40, 5) == -1


def test_argument_validation_happens_on_the_host(lib):
    N = None
    one = 8        # any non-null "pointer": validation never dereferences
    big = 1 << 40

    def fwd(B=4, S=64, V=10, r=0.01, eps=1e-5, ptrs=(one,) * 7):
        return lib.snerf_image_warp_fwd_f32(*ptrs[:4], B, S, V, r, eps, *ptrs[4:], N, N)

    def bwd(B=4, S=64, V=10, r=0.01, ins=(one,) * 4, grads=(one, N, N), ws=(one, big), outs=(N, one, one)):
        return lib.snerf_image_warp_bwd_f32(*ins, *grads, B, S, V, r, *ws, *outs, N)

    # B = 0: a no-op that returns 0, also with no GPU and null pointers
    assert fwd(B=0, ptrs=(N,) * 7) == 0 and bwd(B=0, ins=(N,) * 4, grads=(N,) * 3, ws=(N, 0), outs=(N,) * 3) == 0
    for f in (fwd, bwd):
        assert f(r=0.0) == -1 and b"radius" in lib.snerf_last_error_string()
        assert f(r=-1.0) == -1 and f(r=float("nan")) == -1
        assert f(B=-1) == -1 and f(S=0) == -1 and f(V=0) == -1
        assert f(B=0, r=0.0) == -1                                     # a bad scalar is an error whatever B is
        assert f(B=1 << 40, S=1 << 30) == -1 and b"too large" in lib.snerf_last_error_string()
    assert fwd(eps=-1e-5) == -1 and b"eps" in lib.snerf_last_error_string()
    assert fwd(eps=float("nan")) == -1 and fwd(B=0, eps=-1.0) == -1
    assert fwd(B=0, eps=0.0, ptrs=(N,) * 7) == 0                       # eps = 0 is allowed
    for i in range(7):                                                 # every required pointer of the forward
        assert fwd(ptrs=tuple(N if j == i else one for j in range(7))) == -1 and b"null" in lib.snerf_last_error_string()
    for i in range(4):
        assert bwd(ins=tuple(N if j == i else one for j in range(4))) == -1 and b"null" in lib.snerf_last_error_string()
    assert bwd(outs=(N, N, one)) == -1 and bwd(outs=(N, one, N)) == -1
    assert bwd(grads=(N, N, N)) == -1 and b"gradient" in lib.snerf_last_error_string()
    need = lib.snerf_image_warp_bwd_workspace_bytes(4 * 64, 10)
    assert need == 10 * 48
    assert bwd(ws=(one, need - 1)) == -1 and b"workspace" in lib.snerf_last_error_string()
    assert bwd(ws=(N, need)) == -1 and b"workspace" in lib.snerf_last_error_string()
    # stats and the workspace hold float64
    assert lib.snerf_image_warp_fwd_f32(*(one,) * 4, 4, 64, 10, 0.01, 1e-5, *(one,) * 3, 12, N) == -2
    assert bwd(ws=(12, big)) == -2 and bwd(ins=(one, one, one, 12)) == -2 and b"aligned" in lib.snerf_last_error_string()


def test_operator_rejects_what_it_cannot_run():
    from smpl_nerf_amd import ops
    x, g, o = torch.rand(2, 5, 3), torch.rand(9, 3), torch.rand(2, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.image_wise_warp(x, g, g, o, 0.01)


def test_restatement_reproduces_the_reference_run():
    """tests/golden/g22_image_wise.npz holds the reference's own ImageWiseSolver.train over 2 images x 2 ray batches (fp32, CPU).
    The fp32 restatement driven through the same steps is the same arithmetic up to fp32 round-off of another order of operations
    in the net (tests/torch_ref.py) and of another CPU's kernels: 1e-5 of the largest colour - what the pipelines' coarse outputs are
    held to against their fixtures - through four Adam steps; the arm angles move by lrate_pose per step, whatever the gradient's
    size is, to 1e-6.  The float64 run differs from the fp32 fixture by the fixture's own round-off."""
    import json
    from conftest import load_golden
    g = load_golden("g22_image_wise.npz")
    c = IR.G22
    assert json.loads(str(g["config"])) == c, "the fixture was generated with other seeds than image_wise_ref.G22"
    images, body, params = IR.g22_inputs()
    per_image = c["R"] // c["batchsize"]
    assert g["step_rays"].shape == (len(images) * per_image, c["batchsize"]) and per_image == 2       # the retained graph is used twice
    for k in range(0, len(g["step_rays"]), per_image):                                                 # the batches of an image cover it
        assert sorted(np.concatenate(g["step_rays"][k:k + per_image]).tolist()) == list(range(c["R"]))
    assert set(g["adam_steps"].tolist()) == {len(g["step_rays"])}
    assert g["step_loss"][-1] < g["step_loss"][0]
    assert abs(float(g["arm_angle_l"].ravel()[0]) - c["arm_angle_l"]) > c["lrate_pose"]                          # the pose was trained
    # a third of the samples sit within the radius of a vertex of the body at the initial arm angles
    pose = torch.zeros(1, 69)
    pose[0, 38], pose[0, 41] = c["arm_angle_l"], c["arm_angle_r"]
    goal = body(body_pose=pose).vertices
    w = IR.warp_linear(torch.from_numpy(images[0][0]), goal, body(body_pose=torch.zeros(1, 69)).vertices, torch.from_numpy(images[0][1]), c["radius"])[0]
    assert (w.abs().amax(-1) > 0).sum() >= c["R"] * c["S"] // 4
    for dtype, tol in ((torch.float32, 1e-5), (torch.float64, 2e-5)):
        r = IR.train_steps(images, body, params, g["step_rays"], dtype)
        figures = {k: IR.relative_error(r[k], g[k]) for k in ("step_rgb", "step_loss", "param_sample", "arm_angle_l", "arm_angle_r")}
        print(dtype, {k: f"{v:.2e}" for k, v in figures.items()})
        assert figures["step_rgb"] <= tol and figures["step_loss"] <= tol and figures["param_sample"] <= 1e-6
        assert figures["arm_angle_l"] <= 1e-6 and figures["arm_angle_r"] <= 1e-6
        assert np.array_equal(r["adam_steps"], g["adam_steps"])
