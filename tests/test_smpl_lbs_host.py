"""CPU-side checks of the SMPL body model: the torch restatement the GPU tests measure against (tests/smpl_lbs_ref.py) is what the
formulation says, the C entry points exist and validate their arguments before touching a device, the loaders of
body_model.SmplBodyModel read what they should, and the module fits the pipelines' and the trainer's expectations.  No GPU needed,
nothing launched."""
import ctypes
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import smpl_lbs_ref as SR
from smpl_nerf_amd import _lib, build
from smpl_nerf_amd.body_model import SmplBodyModel
from smpl_nerf_amd.synthetic_smpl import SMPL_PARENTS, random_smpl_arrays

NAMES = ("snerf_smpl_lbs_fwd_f32", "snerf_smpl_lbs_bwd_workspace_bytes", "snerf_smpl_lbs_bwd_f32")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def T64(a):
    return {k: (torch.from_numpy(np.asarray(v)).double() if k != "parents" else v) for k, v in a.items()}


# ---------------------------------------------------------------------------------------------- the yardstick itself
def test_zero_pose_and_zero_betas_give_the_template():
    a = T64(SR.body(65))
    v, j = SR.lbs(a, torch.zeros(1, 10).double(), torch.zeros(2, 69).double(), torch.zeros(2, 3).double())
    assert float((v - a["v_template"][None]).abs().max()) <= 1e-6          # (the 1e-8 of Rodrigues is the only difference)
    assert float((j - (a["J_regressor"] @ a["v_template"])[None]).abs().max()) <= 1e-6


def test_global_orient_alone_rotates_about_the_root_joint():
    a = T64(SR.body(65))
    r = torch.tensor([[0.3, -1.1, 0.7], [2.0, 0.1, -0.4]]).double()
    v, j = SR.lbs(a, torch.zeros(1, 10).double(), torch.zeros(2, 69).double(), r)
    # an independent rotation matrix: the matrix exponential of the skew matrix
    K = torch.zeros(2, 3, 3).double()
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -r[:, 2], r[:, 1], r[:, 2], -r[:, 0], -r[:, 1], r[:, 0]
    R = torch.matrix_exp(K)
    J0 = (a["J_regressor"] @ a["v_template"])[0]
    want = torch.einsum("brc,vc->bvr", R, a["v_template"] - J0) + J0
    assert float((v - want).abs().max()) <= 1e-6
    assert float((j[:, 0] - J0).abs().max()) <= 1e-12


def test_restatement_passes_gradcheck():
    a = T64(SR.body(9, J=4, NB=2))
    full = torch.from_numpy(SR.poses(2, 4, seed=3)).double()
    betas = torch.randn(2, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    pose, orient = full[:, 1:].reshape(2, -1).clone().requires_grad_(True), full[:, 0].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda b, p, g: SR.lbs(a, b, p, g), (betas, pose, orient), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_synthetic_body():
    a = random_smpl_arrays(0)
    assert a["v_template"].shape == (6890, 3) and a["shapedirs"].shape == (6890, 3, 10) and a["posedirs"].shape == (6890, 3, 207)
    assert tuple(a["parents"]) == SMPL_PARENTS and a["J_regressor"].shape == (24, 6890) and a["weights"].shape == (6890, 24)
    assert (a["J_regressor"] >= 0).all() and np.allclose(a["J_regressor"].sum(1), 1, atol=1e-6) and ((a["J_regressor"] > 0).sum(1) <= 8).all()
    assert (a["weights"] >= 0).all() and np.allclose(a["weights"].sum(1), 1, atol=1e-6) and ((a["weights"] > 0).sum(1) <= 4).all()
    assert all(v.dtype == (np.int32 if k == "parents" else np.float32) for k, v in a.items())
    b = random_smpl_arrays(0)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    small = random_smpl_arrays(1, n_vertices=1, n_joints=3)
    assert small["weights"].shape == (1, 3) and tuple(small["parents"]) == (-1, 0, 0)


# ---------------------------------------------------------------------------------------------- the C entries
def test_symbols_are_exported_and_prototyped(lib):
    header = open(_lib.HERE + "/../include/smplnerf.h").read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name + "(" in header
    assert "typedef struct snerf_smpl_model" in header
    assert lib.snerf_version() == 109


def test_argument_validation_happens_on_the_host(lib):
    """Every call below either has B = 0 or fails a check: none passes validation with these stand-in pointers, so nothing is ever
    launched, GPU or not (a row count of 1 being accepted is held on the GPU with real tensors, test_gpu_smpl_lbs.py::test_shared_betas)."""
    Z = None
    one = 8        # any non-null "pointer": validation never dereferences device pointers

    def model(V=65, J=24, NB=10, parents=SMPL_PARENTS, **ptrs):
        p = {k: one for k in ("v_template", "blend", "J_template", "J_dirs", "weights")}
        p.update(ptrs)
        host = (ctypes.c_int32 * max(len(parents), 1))(*parents) if parents is not None else None
        m = _lib.SmplModel(V, J, NB, p["v_template"], p["blend"], p["J_template"], p["J_dirs"], p["weights"], host)
        m._keep = host
        return m

    def fwd(m, B=4, rows=4, betas=one, pose=one, orient=one, vertices=one, joints=Z, rig=one):
        return lib.snerf_smpl_lbs_fwd_f32(ctypes.byref(m) if m is not None else None, betas, rows, pose, orient, B, vertices, joints, rig, Z)

    def bwd(m, B=4, rows=4, betas=one, pose=one, orient=one, rig=one, d_v=one, d_j=Z, ws=one, ws_bytes=1 << 40):
        return lib.snerf_smpl_lbs_bwd_f32(ctypes.byref(m) if m is not None else None, betas, rows, pose, orient, rig, d_v, d_j, B, ws, ws_bytes,
                                          Z, one, Z, Z)

    def size(m, B=4):
        return lib.snerf_smpl_lbs_bwd_workspace_bytes(ctypes.byref(m) if m is not None else None, B)

    def err():
        return lib.snerf_last_error_string()

    good = model()
    # B = 0: a no-op that returns 0, also with no GPU and null pointers
    assert fwd(good, B=0, betas=Z, pose=Z, vertices=Z, rig=Z) == 0
    assert bwd(good, B=0, rows=0, betas=Z, pose=Z, rig=Z, d_v=Z, ws=Z, ws_bytes=0) == 0
    for call in (fwd, bwd):
        assert call(None) == -1 and b"model" in err()
        assert call(good, B=-1) == -1 and b"B " in err()
        for V in (0, -5):
            assert call(model(V=V)) == -1 and b"V " in err()
        for J in (1, 0, 33):
            assert call(model(J=J, parents=(-1,) + tuple(range(max(J - 1, 0))))) == -1 and b"J " in err()
        assert call(model(NB=0)) == -1 and b"NB" in err()
        assert call(model(NB=512)) == -1 and b"NB" in err()              # NB + 9 (J - 1) above the kernels' 512
        for rows in (0, 2, 3, 5):
            assert call(good, rows=rows) == -1 and b"betas" in err()
        for name in ("v_template", "blend", "J_template", "J_dirs", "weights"):
            assert call(model(**{name: Z})) == -1 and b"model" in err()
        assert call(model(parents=None)) == -1
        for bad in ((0,) + SMPL_PARENTS[1:], SMPL_PARENTS[:5] + (5,) + SMPL_PARENTS[6:], SMPL_PARENTS[:7] + (9,) + SMPL_PARENTS[8:],
                    SMPL_PARENTS[:3] + (-1,) + SMPL_PARENTS[4:]):
            assert call(model(parents=bad)) == -1 and b"parents" in err()
        assert call(good, betas=Z) == -1 and call(good, pose=Z) == -1 and call(good, rig=Z) == -1
        assert call(good, B=0, rows=7) == 0                              # nothing to read: no rows to count
    assert fwd(good, vertices=Z) == -1 and b"null" in err()
    assert bwd(good, d_v=Z, d_j=Z) == -1 and b"gradient" in err()
    assert bwd(good, ws=Z) == -1 and b"workspace" in err()
    assert bwd(good, ws_bytes=size(good) - 1) == -1 and b"workspace" in err()
    assert size(None) == -1 and size(model(V=0)) == -1 and size(good, B=-1) == -1
    E = 12 * 24 + 10 + 207
    assert size(good, B=0) == 0 and size(good) >= 4 * (2 * 4 * E + 4 * 10) and size(good) % 4 == 0
    assert size(model(V=6890), B=2048) <= 2048 * 6890 * 16 * 4 // 8          # far below the reference's [B,V,4,4] transforms


# ---------------------------------------------------------------------------------------------- the module
def test_from_arrays_lays_the_model_out_for_the_kernels():
    a = SR.body(65)
    m = SmplBodyModel.from_arrays(**a)
    assert isinstance(m, torch.nn.Module) and not list(m.parameters())      # nothing trained: the trainer does not treat it as upstream
    assert sorted(dict(m.named_buffers())) == ["J_dirs", "J_template", "blend", "parents", "v_template", "weights"]
    assert m.blend.shape == (217, 195) and m.blend.dtype == torch.float32 and m.parents.dtype == torch.int32
    assert np.array_equal(m.blend[3].numpy(), a["shapedirs"][:, :, 3].reshape(-1))
    assert np.array_equal(m.blend[10 + 100].numpy(), a["posedirs"][:, :, 100].reshape(-1))
    reg = a["J_regressor"].astype(np.float64)
    assert np.array_equal(m.J_template.numpy(), (reg @ a["v_template"].astype(np.float64)).astype(np.float32))
    assert np.array_equal(m.J_dirs.numpy(), np.einsum("jv,vcn->jcn", reg, a["shapedirs"].astype(np.float64)).astype(np.float32))
    assert m.kernel_buffers()["parents"] == list(SMPL_PARENTS) and m.num_joints == 24 and m.num_betas == 10
    m2 = SmplBodyModel.from_arrays(**SR.body(65, seed=9))
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(m.buffers(), m2.buffers()))
    assert SmplBodyModel.from_arrays(**a, num_betas=4).blend.shape == (211, 195)
    root = dict(a, parents=np.array((2 ** 32 - 1,) + SMPL_PARENTS[1:], np.uint32))       # the root's entry in the published files
    assert SmplBodyModel.from_arrays(**root).kernel_buffers()["parents"][0] == -1
    with pytest.raises(ValueError, match="posedirs"):
        SmplBodyModel.from_arrays(**dict(a, posedirs=a["posedirs"].reshape(195, 207).T))
    with pytest.raises(ValueError, match="parents"):
        SmplBodyModel.from_arrays(**dict(a, parents=np.array((-1, 1) + SMPL_PARENTS[2:])))
    with pytest.raises(RuntimeError, match="GPU"):
        m(body_pose=torch.zeros(2, 69))                                    # no CPU path


def test_from_file_round_trips(tmp_path):
    import scipy.sparse
    a = SR.body(65)
    want = SmplBodyModel.from_arrays(**a)
    kin = np.stack([np.array((2 ** 32 - 1,) + SMPL_PARENTS[1:], np.uint32), np.arange(24, dtype=np.uint32)])
    np.savez(tmp_path / "body.npz", **{k: v for k, v in a.items() if k != "parents"}, kintree_table=kin)
    np.savez(tmp_path / "body_parents.npz", **a)
    with open(tmp_path / "body.pkl", "wb") as f:
        pickle.dump({"v_template": a["v_template"].astype(np.float64), "shapedirs": a["shapedirs"].astype(np.float64),
                     "posedirs": a["posedirs"].astype(np.float64), "J_regressor": scipy.sparse.csc_matrix(a["J_regressor"].astype(np.float64)),
                     "weights": a["weights"].astype(np.float64), "kintree_table": kin, "f": np.zeros((3, 3), np.uint32)}, f, protocol=2)
    for name in ("body.npz", "body_parents.npz", "body.pkl"):
        got = SmplBodyModel.from_file(tmp_path / name)
        for (k, x), y in zip(want.named_buffers(), got.buffers()):
            assert torch.equal(x, y), (name, k)
    with pytest.raises(ValueError, match="posedirs"):
        np.savez(tmp_path / "short.npz", **{k: v for k, v in a.items() if k != "posedirs"})
        SmplBodyModel.from_file(tmp_path / "short.npz")


def test_a_pickle_that_needs_chumpy_says_so(tmp_path):
    assert "chumpy" not in sys.modules
    fake = types.ModuleType("chumpy")

    class Ch:
        pass

    Ch.__module__, Ch.__qualname__, fake.Ch = "chumpy", "Ch", Ch
    sys.modules["chumpy"] = fake
    try:
        with open(tmp_path / "chumpy_body.pkl", "wb") as f:
            pickle.dump({"v_template": Ch()}, f, protocol=2)
    finally:
        del sys.modules["chumpy"]
    with pytest.raises(RuntimeError, match=r"chumpy.*\.npz"):
        SmplBodyModel.from_file(tmp_path / "chumpy_body.pkl")
