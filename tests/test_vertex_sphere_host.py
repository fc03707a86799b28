"""CPU-side checks of the vertex_sphere model: the torch restatement the GPU tests measure against reproduces what the reference
computed (tests/golden/g19_vertex_sphere.npz), the three C entry points exist and validate their arguments before touching a
device, the operators refuse what they cannot run, and the Python surface (arguments, body model faces, synthetic surface body,
drop-in) is in place.  No GPU needed, nothing launched."""
import importlib
import json
import sys

import numpy as np
import pytest
import torch

import vertex_sphere_ref as SR
from conftest import load_golden
from smpl_nerf_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_restatement_reproduces_the_reference():
    """fp32 on the CPU: the restated pipeline is the reference's own arithmetic up to the round-off of another sum order in the
    net (the tolerances the GPU pipeline is held to)."""
    g = load_golden("g19_vertex_sphere.npz")
    assert json.loads(str(g["config"])) == SR.G19, "the fixture was generated with other seeds than vertex_sphere_ref.G19"
    batch_np, params = SR.g19_inputs()
    T = torch.from_numpy
    moved = np.abs(batch_np[4]).max(-1) > 0
    assert 0.3 <= moved.mean() <= 0.37 and g["densities"].max() > 0.1 and g["rgb"].std() > 0.01       # the fixture is no empty scene
    with torch.no_grad():
        rgb, warped, dens = SR.vertex_sphere_pipeline({k: T(v) for k, v in params.items()}, [T(a) for a in batch_np])
    assert np.abs(rgb.numpy() - g["rgb"]).max() <= 1e-5
    assert np.abs(warped.numpy() - g["warped"]).max() <= 2e-6
    assert np.abs(dens.numpy() - g["densities"]).max() <= 5e-5
    assert abs(torch.nn.functional.mse_loss(rgb, T(batch_np[5])).item() - g["loss"][0]) <= 1e-6
    assert np.array_equal(warped.numpy()[~moved], batch_np[0][~moved])


def test_symbols_are_exported_and_prototyped(lib):
    for name, nargs in (("snerf_ray_mesh_hits_f32", 13), ("snerf_ray_mesh_workspace_bytes", 1), ("snerf_vertex_sphere_warp_f32", 11)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    text = open(_lib.HERE + "/../include/smplnerf.h").read()
    assert all(n + "(" in text for n in ("snerf_ray_mesh_hits_f32", "snerf_ray_mesh_workspace_bytes", "snerf_vertex_sphere_warp_f32"))
    assert lib.snerf_version() == 109


def test_ray_mesh_argument_validation_happens_on_the_host(lib):
    N, one = None, 8        # any non-null "pointer": validation never dereferences
    assert lib.snerf_ray_mesh_workspace_bytes(13776) == 36 * 13776 and lib.snerf_ray_mesh_workspace_bytes(1) == 36
    assert lib.snerf_ray_mesh_workspace_bytes(0) == -1 and b"F" in lib.snerf_last_error_string()

    def hits(R=5, V=9, F=4, K=3, ptrs=(one,) * 4, outs=(one, one), ws=one, ws_bytes=36 * 4):
        return lib.snerf_ray_mesh_hits_f32(*ptrs, R, V, F, K, *outs, ws, ws_bytes, N)

    assert hits(R=0, ptrs=(N,) * 4, outs=(N, N), ws=N, ws_bytes=0) == 0            # R = 0: a no-op, also with null pointers
    for K in (0, 17, -1):
        assert hits(K=K) == -1 and b"max_hits" in lib.snerf_last_error_string()
    assert hits(R=0, K=17) == -1 and hits(R=0, V=0) == -1 and hits(R=0, F=0) == -1  # a bad scalar is an error whatever R is
    assert hits(V=0) == -1 and b"V" in lib.snerf_last_error_string()
    assert hits(F=0) == -1 and b"F" in lib.snerf_last_error_string()
    assert hits(R=-1) == -1 and b"R" in lib.snerf_last_error_string()
    for i in range(4):                                                              # every required input pointer
        assert hits(ptrs=tuple(N if j == i else one for j in range(4))) == -1 and b"null" in lib.snerf_last_error_string()
    assert hits(outs=(N, one)) == -1 and hits(outs=(one, N)) == -1
    assert hits(ws=N) == -1 and b"workspace" in lib.snerf_last_error_string()
    assert hits(ws_bytes=36 * 4 - 1) == -1 and b"workspace" in lib.snerf_last_error_string()


def test_sphere_warp_argument_validation_happens_on_the_host(lib):
    N, one = None, 8

    def warp(n=5, V=9, r=0.01, mean=0, ptrs=(one,) * 3, out=one):
        return lib.snerf_vertex_sphere_warp_f32(*ptrs, n, V, r, mean, out, N, N, N)

    assert warp(n=0, ptrs=(N,) * 3, out=N) == 0
    for r in (0.0, -1.0, float("nan"), float("inf")):
        for mean in (0, 1):
            assert warp(r=r, mean=mean) == -1 and b"radius" in lib.snerf_last_error_string()
    assert warp(n=0, r=0.0) == -1 and warp(n=0, V=0) == -1
    assert warp(V=0) == -1 and b"V" in lib.snerf_last_error_string()
    assert warp(n=-1) == -1
    for i in range(3):
        assert warp(ptrs=tuple(N if j == i else one for j in range(3))) == -1 and b"null" in lib.snerf_last_error_string()
    assert warp(out=N) == -1 and b"null" in lib.snerf_last_error_string()


def test_operators_reject_what_they_cannot_run():
    from smpl_nerf_amd import ops
    v, f = SR.body_mesh(0, 1)
    o, d = SR.camera_rays(5, v, 1)
    T = torch.from_numpy
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ray_mesh_hits(T(o), T(d), T(v), T(f))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vertex_sphere_warp(T(o), T(v), T(v), 0.01)
    with pytest.raises(RuntimeError, match="int32"):
        ops.ray_mesh_hits(T(o), T(d), T(v), T(f).long())
    bad = f.copy()
    bad[3, 1] = len(v)
    with pytest.raises(RuntimeError, match="outside"):
        ops.ray_mesh_hits(T(o), T(d), T(v), T(bad))
    bad[3, 1] = -1
    with pytest.raises(RuntimeError, match="outside"):
        ops.ray_mesh_hits(T(o), T(d), T(v), T(bad))


def test_pipeline_args_defaults():
    from smpl_nerf_amd.pipelines import PipelineArgs
    for a in (PipelineArgs(), PipelineArgs.reference_defaults()):                  # config_parser.py:35-45
        assert (a.vertex_sphere_radius, a.warp_by_vertex_mean, a.coarse_samples_from_prior, a.coarse_samples_from_intersect,
                a.std_dev_coarse_sample_prior) == (0.01, 0, 0, 0, 0.03)


def test_body_model_faces_stay_out_of_the_state_dict():
    from smpl_nerf_amd.body_model import SmplBodyModel
    from smpl_nerf_amd.synthetic_smpl import random_smpl_arrays, surface_smpl_arrays
    arrays = surface_smpl_arrays(3, level=1)
    plain = SmplBodyModel.from_arrays(**{k: v for k, v in arrays.items() if k != "faces"})
    body = SmplBodyModel.from_arrays(**arrays)
    assert plain.faces is None and SmplBodyModel.from_arrays(**random_smpl_arrays(1, n_vertices=30)).faces is None
    assert body.faces.dtype == torch.int32 and tuple(body.faces.shape) == (80, 3) and np.array_equal(body.faces.numpy(), arrays["faces"])
    assert list(body.state_dict()) == list(plain.state_dict()) and "faces" not in body.state_dict()
    assert "faces" in dict(body.named_buffers())
    with pytest.raises(ValueError, match="faces"):
        SmplBodyModel.from_arrays(**dict(arrays, faces=arrays["faces"] + 1))


def test_body_model_reads_faces_from_a_file(tmp_path):
    from smpl_nerf_amd.body_model import SmplBodyModel
    from smpl_nerf_amd.synthetic_smpl import surface_smpl_arrays
    a = surface_smpl_arrays(4, level=0)
    faces = a.pop("faces")
    np.savez(tmp_path / "with.npz", f=faces.astype(np.uint32), **a)
    np.savez(tmp_path / "without.npz", **a)
    assert np.array_equal(SmplBodyModel.from_file(tmp_path / "with.npz").faces.numpy(), faces)
    assert SmplBodyModel.from_file(tmp_path / "without.npz").faces is None


@pytest.mark.parametrize("level,V", [(0, 12), (1, 42), (2, 162), (3, 642)])
def test_surface_body_is_a_closed_mesh(level, V):
    from smpl_nerf_amd.synthetic_smpl import surface_smpl_arrays
    a = surface_smpl_arrays(7, level=level)
    f = a["faces"]
    assert a["v_template"].shape == (V, 3) and f.shape == (20 * 4 ** level, 3) and f.dtype == np.int32
    assert f.min() == 0 and f.max() == V - 1
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 2).all(), "every edge is shared by exactly two faces"
    directed = {(int(x), int(y)) for tri in f for x, y in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))}
    assert len(directed) == 3 * len(f) and all((y, x) in directed for x, y in directed)      # consistently wound
    w = a["weights"]
    assert w.shape == (V, 24) and np.allclose(w.sum(1), 1, atol=1e-6) and (w >= 0).all()
    assert np.allclose(a["J_regressor"].sum(1), 1, atol=1e-5)
    # smooth skinning: a softmax of -distance / SKIN_LENGTH moves by at most |x - y| / (2 SKIN_LENGTH) between two points
    from smpl_nerf_amd.synthetic_smpl import SKIN_LENGTH
    v = a["v_template"].astype(np.float64)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        step = np.linalg.norm(v[f[:, i]] - v[f[:, j]], axis=1)
        assert (np.abs(w[f[:, i]] - w[f[:, j]]).max(1) <= step / (2 * SKIN_LENGTH) + 1e-6).all()


def test_run_fine_is_not_implemented():
    from smpl_nerf_amd.pipelines import PipelineArgs, VertexSpherePipeline
    pipe = VertexSpherePipeline(torch.nn.Identity(), torch.nn.Identity(), PipelineArgs(run_fine=1), None, None)
    assert pipe._single_call_ok([None] * 6) is False
    with pytest.raises(NotImplementedError, match="true warp for the fine samples"):
        pipe([torch.zeros(2, 4, 3), torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2, 4, 3), torch.zeros(2, 3)])


def test_dropin_rebinds_the_vertex_sphere_pipeline(tmp_path):
    """A stand-in checkout with the reference's layout: models/vertex_sphere_pipeline.py and a solver that copies the class."""
    root = tmp_path / "checkout"
    for rel, src in {"utils.py": "def raw2outputs(*a, **k):\n    raise NotImplementedError\n",
                     "models/nerf_pipeline.py": "class NerfPipeline:\n    pass\n",
                     "models/vertex_sphere_pipeline.py": ("from models.nerf_pipeline import NerfPipeline\n\n\n"
                                                          "class VertexSpherePipeline(NerfPipeline):\n    pass\n"),
                     "solver/vertex_sphere_solver.py": ("from models.vertex_sphere_pipeline import VertexSpherePipeline\n\n\n"
                                                        "class VertexSphereSolver:\n    pass\n")}.items():
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
        VS = importlib.import_module("solver.vertex_sphere_solver")
        assert VS.VertexSpherePipeline is pipelines.VertexSpherePipeline
        assert importlib.import_module("models.vertex_sphere_pipeline").VertexSpherePipeline is pipelines.VertexSpherePipeline
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


@pytest.mark.parametrize("by_mean", [False, True])
def test_restated_warp_keeps_the_equality_quirk(by_mean):
    """One vertex at distance exactly r, one inside, one outside: the equal distance weighs as itself (quirk Q12)."""
    goal = torch.tensor([[0.5, 0.0, 0.0], [0.0, 0.25, 0.0], [0.0, 0.0, 3.0]], dtype=torch.float64)
    canon = goal + torch.tensor([[1.0, 2.0, 3.0], [0.5, 0.5, 0.5], [9.0, 9.0, 9.0]], dtype=torch.float64)
    p = torch.zeros(1, 3, dtype=torch.float64)
    if by_mean:      # r = 0.5: vertex 0 on the rim (weight 0.5), vertex 1 inside (1), vertex 2 outside (0)
        w, nearest, count = SR.sphere_warp(p, goal, canon, 0.5, True)
        want = (0.5 * torch.tensor([1.0, 2.0, 3.0]) + torch.tensor([0.5, 0.5, 0.5])) / (1.5 + 1e-10)
        assert torch.allclose(w[0], want.double(), atol=1e-12) and int(nearest) == 1 and int(count) == 1
    else:            # r = 0.25: the nearest vertex sits on the rim and its warp is scaled by 0.25
        w, nearest, count = SR.sphere_warp(p, goal, canon, 0.25, False)
        assert torch.allclose(w[0], 0.25 * torch.tensor([0.5, 0.5, 0.5]).double()) and int(nearest) == 1 and int(count) == 0
