"""CPU-side checks of the first hit and the single-sample model: the restatement the GPU tests measure against
(tests/single_sample_ref.py) agrees with the form the reference gives the warp and with the hit lists' restatement, breaks ties
toward the smaller face index and reproduces what the reference's pipeline computed (tests/golden/g21_single_sample.npz); the
operator and the C entry refuse what they cannot run before anything touches a device; the drop-in knows the reference's module.
No GPU needed, nothing launched."""
import functools
import importlib
import json
import sys

import numpy as np
import pytest
import torch

import single_sample_ref as SS
import vertex_sphere_ref as SR
from conftest import load_golden
from smpl_nerf_amd import _lib, build
from smpl_nerf_amd.single_sample import SingleSampleRays

case = functools.lru_cache(maxsize=None)(SS.case_inputs)          # the cases of tests/test_gpu_first_hit.py


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("R,F", [(130, 20), (130, 320), (130, 1280), (65, 13776)])
def test_the_barycentric_warp_is_the_reference_solve(R, F):
    """float64: canonical_vertices^T solve(goal_vertices^T, hit) against (1 - u - v, u, v) . canonical vertices, on every kept hit
    ray - what lets the kernel restate get_warp without the solve."""
    o, d, v, f, canon = case(R, F)
    left_out, _ = SS.first_hit_margin(o, d, v, f)
    h = SS.first_hit(*(torch.from_numpy(a).double() for a in (o, d, v)), f, torch.from_numpy(canon).double())
    keep = ~left_out & (h["face"] >= 0)
    assert keep.sum() >= 0.2 * R
    diff = float(np.abs(SS.get_warp_solve(o, d, v, f, canon) - h["warp"])[keep].max())
    print(f"solve against barycentrics R={R} F={F}: max |difference| {diff:.2e} over {int(keep.sum())} rays; "
          f"largest condition number {SS.solve_condition(o, d, v, f):.2e}")
    assert diff <= 1e-10


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("R,F", [(65, 20), (130, 1280), (65, 13776)])
def test_the_first_hit_is_the_head_of_the_hit_list(R, F, dtype):
    o, d, v, f, canon = case(R, F)
    args = [torch.from_numpy(a).to(dtype) for a in (o, d, v)]
    h = SS.first_hit(*args, f, torch.from_numpy(canon).to(dtype))
    t, n = SR.ray_mesh_hits(*args, f, 1)
    assert h["t"].dtype == t.dtype and np.array_equal(h["t"], t[:, 0]) and np.array_equal(h["face"] >= 0, n > 0)
    miss = h["face"] < 0
    assert np.isposinf(h["t"][miss]).all() and not h["uv"][miss].any() and not h["warp"][miss].any() and not h["depth"][miss].any()


def test_depth_is_t_times_the_length_of_the_direction():
    o, d, v, f, canon = case(65, 320)
    a = SS.first_hit(*(torch.from_numpy(x).double() for x in (o, d, v)), f, torch.from_numpy(canon).double())
    b = SS.first_hit(torch.from_numpy(o).double(), torch.from_numpy(d).double() * 3, torch.from_numpy(v).double(), f,
                     torch.from_numpy(canon).double())                                     # (scaled in float64: no rounding of d)
    hit = a["face"] >= 0
    assert np.array_equal(a["face"], b["face"]) and np.abs(b["t"][hit] * 3 / a["t"][hit] - 1).max() < 1e-12
    assert np.abs(b["depth"][hit] / a["depth"][hit] - 1).max() < 1e-12 and np.abs(b["warp"] - a["warp"]).max() < 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_tie_goes_to_the_smaller_face_index(dtype):
    o, d, v, f, canon = SS.tie_case()
    args = [torch.from_numpy(a).to(dtype) for a in (o, d, v)]
    hit, t = SR.ray_mesh_pairs(*args, f)[:2]
    assert hit[:, 3].all() and hit[:, 7].all() and hit.sum() == 10 and torch.equal(t[:, 3], t[:, 7])         # the tie is exact
    h = SS.first_hit(*args, f, torch.from_numpy(canon).to(dtype))
    assert (h["face"] == 3).all()
    swapped = canon.copy()
    swapped[9:12], swapped[21:24] = canon[21:24], canon[9:12]
    other = SS.first_hit(*args, f, torch.from_numpy(swapped).to(dtype))
    assert np.abs(h["warp"] - other["warp"]).min() > 1e-4          # the warp tells the two faces apart
    assert "smaller face index" in open(_lib.HERE + "/../include/smplnerf.h").read()      # the header states the rule


def test_the_operator_refuses_before_loading_the_library(monkeypatch):
    from smpl_nerf_amd import ops
    assert hasattr(ops, "ray_mesh_first_hit")
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    v, f = SR.body_mesh(0, 1)
    o, d = SR.camera_rays(5, v, 1)
    T = torch.from_numpy
    with pytest.raises(RuntimeError, match="int32"):
        ops.ray_mesh_first_hit(T(o), T(d), T(v), T(f).long())
    for bad_index in (len(v), -1):
        bad = f.copy()
        bad[3, 1] = bad_index
        with pytest.raises(RuntimeError, match="outside"):
            ops.ray_mesh_first_hit(T(o), T(d), T(v), T(bad), canon=T(v))
    with pytest.raises(RuntimeError, match="canon"):
        ops.ray_mesh_first_hit(T(o), T(d), T(v), T(f), canon=T(v[:-1]))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ray_mesh_first_hit(T(o), T(d), T(v), T(f))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ray_mesh_first_hit(T(o), T(d), T(v), T(f), canon=T(v), faces_checked=True)


def test_the_entry_is_exported_and_prototyped(lib):
    name = "snerf_ray_mesh_first_hit_f32"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 16
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert name + "(" in open(_lib.HERE + "/../include/smplnerf.h").read()


def test_the_entry_validates_on_the_host(lib):
    N, one = None, 8        # any non-null "pointer": validation never dereferences

    def first(R=5, V=9, F=4, ptrs=(one,) * 4, canon=N, outs=(one,) * 3, warp=N, depth=N, ws=one, ws_bytes=36 * 4):
        return lib.snerf_ray_mesh_first_hit_f32(*ptrs, R, V, F, canon, *outs, warp, depth, ws, ws_bytes, N)

    assert first(R=0, ptrs=(N,) * 4, outs=(N,) * 3, ws=N, ws_bytes=0) == 0         # R = 0: a no-op, also with null pointers
    assert first(R=0, canon=one) == 0                                               # ... before any pointer is looked at
    assert first(R=0, V=0) == -1 and first(R=0, F=0) == -1                          # a bad scalar is an error whatever R is
    assert first(F=0) == -1 and b"F" in lib.snerf_last_error_string()
    assert first(V=0) == -1 and b"V" in lib.snerf_last_error_string()
    assert first(R=-1) == -1 and b"R" in lib.snerf_last_error_string()
    for i in range(4):
        assert first(ptrs=tuple(N if j == i else one for j in range(4))) == -1 and b"null" in lib.snerf_last_error_string()
    for i in range(3):
        assert first(outs=tuple(N if j == i else one for j in range(3))) == -1 and b"null" in lib.snerf_last_error_string()
    for canon, warp, depth in ((one, N, one), (one, one, N), (N, one, one), (one, N, N), (N, one, N), (N, N, one)):
        assert first(canon=canon, warp=warp, depth=depth) == -1 and b"all null or all non-null" in lib.snerf_last_error_string()
    assert first(ws=N) == -1 and b"workspace" in lib.snerf_last_error_string()
    assert first(ws_bytes=36 * 4 - 1) == -1 and b"workspace" in lib.snerf_last_error_string()
    assert first(canon=one, warp=one, depth=one, ws_bytes=36 * 4 - 1) == -1 and b"workspace" in lib.snerf_last_error_string()
    # the order of the checks is the hit lists': a bad F before a null pointer, a null pointer before the workspace
    assert first(F=0, ptrs=(N,) * 4, ws=N) == -1 and b"F must" in lib.snerf_last_error_string()
    assert first(ptrs=(N,) * 4, ws=N) == -1 and b"null" in lib.snerf_last_error_string()


def test_restated_pipeline_reproduces_the_reference():
    """fp32 on the CPU: the restated pipeline is the reference's own arithmetic up to the round-off of another sum order in the
    net (1e-5, the tolerance g19's rgb is held to)."""
    g = load_golden("g21_single_sample.npz")
    assert json.loads(str(g["config"])) == SS.G21, "the fixture was generated with other seeds than single_sample_ref.G21"
    batch_np, params = SS.g21_inputs()
    T = torch.from_numpy
    moved = np.abs(batch_np[4]).max(-1) > 0
    assert [a.shape for a in batch_np] == [(130, 3), (130, 3), (130, 3), (130, 69), (130, 3), (130, 3)]
    assert np.array_equal(moved, np.arange(130) % 3 == 0) and g["rgb"].std() > 0.05                          # no flat image
    with torch.no_grad():
        rgb = SS.single_sample_pipeline({k: T(v) for k, v in params.items()}, [T(a) for a in batch_np])
    err = float(np.abs(rgb.numpy() - g["rgb"]).max())
    print(f"restated pipeline against the reference: max abs error {err:.2e}")
    assert err <= 1e-5
    assert abs(torch.nn.functional.mse_loss(rgb, T(batch_np[5])).item() - g["loss"][0]) <= 1e-6


def test_the_pipeline_has_the_reference_constructor_and_no_single_call():
    from smpl_nerf_amd.pipelines import PipelineArgs, SingleSamplePipeline
    net = torch.nn.Identity()
    pipe = SingleSamplePipeline(net, PipelineArgs(), None, None)
    assert pipe.model_coarse is net and pipe._single_call_ok([None] * 6) is False


def test_the_data_set_refuses_what_it_cannot_build():
    """Before anything touches a device: a frame count that does not match, a body without faces."""
    from smpl_nerf_amd.pipelines import PipelineArgs
    images, transforms, poses = np.zeros((2, 4, 4, 3), np.uint8), np.stack([np.eye(4)] * 2), np.zeros((2, 69), np.float32)
    body = type("Body", (), {"faces": None})()
    with pytest.raises(ValueError, match="faces"):
        SingleSampleRays(images, transforms, 0.6, poses, np.zeros(10, np.float32), body, PipelineArgs(near=1.0, far=4.0), "cpu")
    with pytest.raises(ValueError, match="one transform"):
        SingleSampleRays(images[:1], transforms, 0.6, poses, np.zeros(10, np.float32), body, PipelineArgs(near=1.0, far=4.0), "cpu")


def test_dropin_rebinds_the_single_sample_pipeline(tmp_path):
    """A stand-in checkout with the reference's layout: models/singe_sample_pipeline.py (its spelling) and a solver that copies the
    class."""
    from smpl_nerf_amd import dropin, pipelines
    assert dropin.REPLACEMENTS["models.singe_sample_pipeline"] == {"SmplPipeline": pipelines.SingleSamplePipeline}
    root = tmp_path / "checkout"
    for rel, src in {"utils.py": "def raw2outputs(*a, **k):\n    raise NotImplementedError\n",
                     "models/singe_sample_pipeline.py": "class SmplPipeline:\n    pass\n",
                     "solver/smpl_solver.py": "from models.singe_sample_pipeline import SmplPipeline\n\n\nclass SmplSolver:\n    pass\n"}.items():
        (root / rel).parent.mkdir(parents=True, exist_ok=True)
        (root / rel).write_text(src)
    top = ("utils", "models", "solver", "torchsearchsorted")
    before = set(sys.modules)
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k.split(".")[0] in top}
    saved_path, saved_meta = list(sys.path), list(sys.meta_path)
    try:
        for k in list(saved):
            sys.modules.pop(k, None)
        dropin._installed = False
        dropin._originals.clear()
        dropin.install(str(root))
        assert importlib.import_module("solver.smpl_solver").SmplPipeline is pipelines.SingleSamplePipeline
        assert importlib.import_module("models.singe_sample_pipeline").SmplPipeline is pipelines.SingleSamplePipeline
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
