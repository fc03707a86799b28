"""CPU-side checks of the vertex-attention warp (DynamicPipeline): the torch restatement the GPU tests measure against reproduces
what the reference computed (tests/golden/g17_dynamic.npz), the two C entry points exist and validate their arguments before
touching a device, and the drop-in rebinds models.dynamic_pipeline.  No GPU needed, nothing launched."""
import importlib
import json
import sys

import numpy as np
import pytest
import torch

import vertex_warp_ref as VR
from conftest import load_golden
from smpl_nerf_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def g17():
    g = load_golden("g17_dynamic.npz")
    assert json.loads(str(g["config"])) == VR.G17, "the fixture was generated with other seeds than vertex_warp_ref.G17"
    batch, poses, body, params = VR.g17_inputs()
    assert np.array_equal(batch[4], g["images"])
    T = torch.from_numpy
    goal = body(body_pose=T(poses[batch[4]])).vertices
    canon = body(body_pose=torch.zeros(len(batch[4]), 69)).vertices
    return g, batch, goal, canon


@pytest.mark.parametrize("case", ["a", "b"])
def test_restatement_reproduces_the_reference(g17, case):
    """fp32 on the CPU: the reference-order form is the reference's own arithmetic (equal to round-off of another CPU's exp), the
    stable form - another maximum, the same sums - agrees with it to fp32 round-off of the largest warp."""
    g, batch, goal, canon = g17
    T = torch.from_numpy
    temperature = VR.G17["cases"][case]
    scale = np.abs(g[f"{case}_warp"]).max()
    assert scale > 0.1 and (np.abs(g[f"{case}_warp"]).max(-1) > 0).sum() > 100      # the attention is exercised
    w, wd, _ = VR.warp_reference_order(T(batch[0]), goal, canon, T(batch[1]), VR.G17["radius"], temperature)
    assert np.abs(w.numpy() - g[f"{case}_warp"]).max() <= 2e-6 * scale
    assert np.abs(wd.numpy() - g[f"{case}_warped"]).max() <= 1e-6 * np.abs(g[f"{case}_warped"]).max()
    w, wd, _ = VR.warp_stable(T(batch[0]), goal, canon, T(batch[1]), VR.G17["radius"], temperature)
    assert np.abs(w.numpy() - g[f"{case}_warp"]).max() <= 4e-6 * scale
    assert np.abs(wd.numpy() - g[f"{case}_warped"]).max() <= 2e-6 * np.abs(g[f"{case}_warped"]).max()
    # untouched samples are exactly untouched in both
    still = np.abs(g[f"{case}_warp"]).max(-1) == 0
    assert still.any() and np.array_equal(wd.numpy()[still], batch[0][still])


def test_symbols_are_exported_and_prototyped(lib):
    for name, nargs in (("snerf_vertex_warp_fwd_f32", 14), ("snerf_vertex_warp_bwd_f32", 17)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    text = open(_lib.HERE + "/../include/smplnerf.h").read()
    assert "snerf_vertex_warp_fwd_f32(" in text and "snerf_vertex_warp_bwd_f32(" in text
    assert lib.snerf_version() == 109


def test_argument_validation_happens_on_the_host(lib):
    N = None
    one = 8        # any non-null "pointer": validation never dereferences

    def fwd(B=4, S=64, V=10, r=0.01, temp=1e4, ptrs=(one,) * 7):
        return lib.snerf_vertex_warp_fwd_f32(*ptrs[:4], B, S, V, r, temp, *ptrs[4:], N, N)

    def bwd(B=4, S=64, V=10, r=0.01, temp=1e4, ins=(one,) * 5, grads=(one, N, N), outs=(N, one, one)):
        return lib.snerf_vertex_warp_bwd_f32(*ins, *grads, B, S, V, r, temp, *outs, N)

    # B = 0: a no-op that returns 0, also with no GPU and null pointers
    assert fwd(B=0, ptrs=(N,) * 7) == 0 and bwd(B=0, ins=(N,) * 5, grads=(N,) * 3, outs=(N,) * 3) == 0
    for f in (fwd, bwd):
        assert f(r=0.0) == -1 and b"radius" in lib.snerf_last_error_string()
        assert f(r=-1.0) == -1 and f(r=float("nan")) == -1
        assert f(temp=-1.0) == -1 and b"temperature" in lib.snerf_last_error_string()
        assert f(B=-1) == -1 and f(S=0) == -1 and f(V=0) == -1
        assert f(B=0, r=0.0) == -1                                     # a bad scalar is an error whatever B is
    for i in range(7):                                                 # every required pointer of the forward
        assert fwd(ptrs=tuple(N if j == i else one for j in range(7))) == -1 and b"null" in lib.snerf_last_error_string()
    for i in range(5):
        assert bwd(ins=tuple(N if j == i else one for j in range(5))) == -1
    assert bwd(outs=(N, N, one)) == -1 and bwd(outs=(N, one, N)) == -1
    assert bwd(grads=(N, N, N)) == -1 and b"gradient" in lib.snerf_last_error_string()


def test_operator_rejects_what_it_cannot_run():
    from smpl_nerf_amd import ops
    x, g, o = torch.rand(2, 5, 3), torch.rand(2, 9, 3), torch.rand(2, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vertex_attention_warp(x, g, g, o, 0.01, 1e4)


def test_pipeline_args_and_trainable_estimator():
    from smpl_nerf_amd.pipelines import DynamicPipeline, PipelineArgs
    from smpl_nerf_amd.synthetic_smpl import IndexPoseEstimator
    a = PipelineArgs()
    assert (a.warp_radius, a.warp_temperature) == (0.01, 10000)          # config_parser.py:47-49
    assert PipelineArgs.reference_defaults().warp_radius == 0.01
    poses = torch.zeros(3, 69)
    fixed, trained = IndexPoseEstimator(poses, torch.zeros(1, 10)), IndexPoseEstimator(poses, torch.zeros(1, 10), trainable_poses=True)
    assert not fixed.goal_poses.requires_grad and trained.goal_poses.requires_grad and not trained.betas.requires_grad
    assert trained.goal_poses.data_ptr() != poses.data_ptr()             # training must not write into the caller's table
    pipe = DynamicPipeline(torch.nn.Identity(), torch.nn.Identity(), trained, torch.nn.Identity(), a, None, None)
    assert pipe._single_call_ok([None] * 6) is False
    assert [n for n, _ in pipe.named_parameters() if "goal_poses" in n] == ["smpl_estimator.goal_poses"]


def test_dropin_rebinds_the_dynamic_pipeline(tmp_path):
    """A stand-in checkout with the reference's layout: models/dynamic_pipeline.py and a solver that copies the class."""
    root = tmp_path / "checkout"
    for rel, src in {"utils.py": "def raw2outputs(*a, **k):\n    raise NotImplementedError\n",
                     "models/nerf_pipeline.py": "class NerfPipeline:\n    pass\n",
                     "models/dynamic_pipeline.py": ("from models.nerf_pipeline import NerfPipeline\n\n\n"
                                                    "class DynamicPipeline(NerfPipeline):\n    pass\n"),
                     "solver/dynamic_solver.py": ("from models.dynamic_pipeline import DynamicPipeline\n\n\n"
                                                  "class DynamicSolver:\n    pass\n")}.items():
        (root / rel).parent.mkdir(parents=True, exist_ok=True)
        (root / rel).write_text(src)
    top = ("utils", "models", "solver", "torchsearchsorted")
    from smpl_nerf_amd import dropin, pipelines
    before = set(sys.modules)
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k.split(".")[0] in top}
    saved_path, saved_meta = list(sys.path), list(sys.meta_path)
    try:
        for k in list(saved):
            sys.modules.pop(k, None)
        dropin._installed = False
        dropin._originals.clear()
        dropin.install(str(root))
        DS = importlib.import_module("solver.dynamic_solver")           # `from models.dynamic_pipeline import DynamicPipeline`
        assert DS.DynamicPipeline is pipelines.DynamicPipeline
        assert importlib.import_module("models.dynamic_pipeline").DynamicPipeline is pipelines.DynamicPipeline
        assert issubclass(pipelines.DynamicPipeline, importlib.import_module("models.nerf_pipeline").NerfPipeline)
    finally:
        sys.meta_path[:] = saved_meta
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k.split(".")[0] in top]:
            sys.modules.pop(k, None)
        sys.modules.update({k: v for k, v in saved.items() if v is not None})
        dropin._installed = False
        for k in set(sys.modules) - before:
            if k.split(".")[0] in top:
                sys.modules.pop(k, None)
