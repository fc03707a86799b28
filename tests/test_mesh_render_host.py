"""CPU-side checks of the mesh renderer and the data-set driver (smpl_nerf_amd/create_dataset.py): the camera paths and the split are
the reference's, the vertex-to-face table lists what it must, write_split and io.load_dataset round-trip for all four data-set types
(the renderer replaced by a stub), the C entry and the operator refuse what they cannot run before anything touches a device, and the
scenes of tests/test_gpu_mesh_render.py keep the margins their float64 comparison needs.  No GPU needed, nothing launched."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mesh_render_ref as MR
from conftest import load_golden
from smpl_nerf_amd import _lib, build
from smpl_nerf_amd import create_dataset as CD
from smpl_nerf_amd import io as sio
from smpl_nerf_amd import synthetic as syn
from smpl_nerf_amd import synthetic_smpl


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_camera_paths_are_the_reference(capsys):
    g = load_golden("g25_camera_paths.npz")
    cfg = json.loads(str(g["config"]))
    assert cfg["sphere"]["number_steps"] == 3 and cfg["circle"]["number_steps"] == 5 and cfg["circle_on_sphere"]["number_steps"] == 7
    assert cfg["circle_on_sphere"]["center_theta"] != 0 and cfg["circle_on_sphere"]["center_phi"] != 0             # off-centre
    for name, fn in (("sphere", CD.sphere_poses), ("circle", CD.circle_poses), ("circle_on_sphere", CD.circle_on_sphere_poses)):
        poses, angles = fn(**cfg[name])
        assert poses.dtype == np.float64 and poses.shape == g[name + "_poses"].shape
        assert np.abs(poses - g[name + "_poses"]).max() <= 1e-12, name
        assert np.abs(np.asarray(angles) - g[name + "_angles"]).max() <= 1e-12, name
    assert g["sphere_poses"].shape == (9, 4, 4) and g["circle_poses"].shape == (5, 4, 4) and g["circle_on_sphere_poses"].shape == (7, 4, 4)


@pytest.mark.parametrize("size", [10, 100])
def test_split_indices_are_the_reference(size):
    state = np.random.get_state()
    try:
        np.random.seed(0)                                                                   # create_dataset.py:14
        train = np.random.choice(np.arange(size), int(size * 0.8), replace=False)            # utils.py:303
        val = np.setdiff1d(np.arange(size), train, assume_unique=True)                       # utils.py:304
    finally:
        np.random.set_state(state)
    got = CD.split_indices(size, 0.8)
    assert np.array_equal(got[0], train) and np.array_equal(got[1], val)
    assert len(got[0]) == int(size * 0.8) and sorted(np.concatenate(got)) == list(range(size))


@pytest.mark.parametrize("level", [0, 2])
def test_vertex_face_table_lists_the_incident_faces_in_ascending_order(level):
    from smpl_nerf_amd import ops
    v, f = synthetic_smpl.icosphere(level)
    offsets, vf = ops.vertex_face_table(torch.from_numpy(f), len(v))
    assert offsets.dtype == np.int32 and vf.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == 3 * len(f) == len(vf)
    for vertex in range(len(v)):
        mine = vf[offsets[vertex]:offsets[vertex + 1]]
        assert list(mine) == [i for i, face in enumerate(f) if vertex in face], vertex
        assert len(mine) in (5, 6)
    assert MR.vertex_faces(f, len(v)) == [list(vf[offsets[i]:offsets[i + 1]]) for i in range(len(v))]


class StubRenderer:
    """What write_split asks of a BodyRenderer: seeded frames that tell their index and pose."""
    camera_angle_x, H, W = 0.9, 6, 5

    def __init__(self):
        self.calls = []

    def frames(self, transforms, body_poses=None, betas=None, want_warp=False):
        n = len(transforms)
        self.calls.append((n, body_poses is not None, want_warp))
        key = np.asarray(transforms)[:, 0, 3]
        rgb = np.stack([np.full((self.H, self.W, 3), int(round(k)) % 256, np.uint8) for k in key])
        rgb[:, 0, 0] = [10, 20, 30]
        depth = np.stack([np.full((self.H, self.W), 1.2 + 0.1 * i, np.float32) for i in range(n)])
        depth[:, 0, 0] = 0
        if not want_warp:
            return torch.from_numpy(rgb), torch.from_numpy(depth)
        return torch.from_numpy(rgb), torch.from_numpy(depth), torch.from_numpy(depth * 2), torch.from_numpy(np.repeat(depth[..., None], 3, -1) * 3)


@pytest.mark.parametrize("kind", CD.DATASET_TYPES)
def test_write_split_round_trips_through_load_dataset(tmp_path, kind):
    n = 7
    transforms = np.stack([syn.pose_matrix(x=20 + 3 * i, y=0.5, z=2.0, theta=4.0 * i) for i in range(n)])
    human = syn.human_poses((41, 38), -30, 30, n)
    indices = [5, 0, 3]
    stub = StubRenderer()
    names = CD.write_split(str(tmp_path), stub, kind, transforms, indices, human_poses=None if kind == "nerf" else human, far=4.8,
                           batch_size=2)
    assert names == ["img_005.png", "img_000.png", "img_003.png"]
    assert stub.calls == [(2, kind != "nerf", kind == "smpl"), (1, kind != "nerf", kind == "smpl")]
    td = json.load(open(tmp_path / "transforms.json"))
    keys = {"camera_angle_x", "image_transform_map"} | (set() if kind == "nerf" else {"image_pose_map", "betas", "expression"})
    assert set(td) == keys and td["camera_angle_x"] == 0.9 and set(td["image_transform_map"]) == set(names)
    ds = sio.load_dataset(str(tmp_path))
    assert ds["names"] == sorted(names)
    order = [indices[names.index(nm)] for nm in ds["names"]]                                  # load_dataset sorts by name
    assert np.array_equal(ds["poses"], transforms[order])
    if kind == "nerf":
        assert ds["human_poses"] is None
    else:
        assert np.array_equal(ds["human_poses"], human[order]) and len(ds["betas"]) == 10 and len(ds["expression"]) == 10
    W = StubRenderer.W
    assert ds["images"].shape == (3, 6, 2 * W if kind == "pix2pix" else W, 3)
    for k, index in enumerate(order):
        rgb = ds["images"][k][:, :W, ::-1]                                                     # BGR -> RGB
        assert (rgb[1:] == (20 + 3 * index) % 256).all() and list(rgb[0, 0]) == [10, 20, 30]
    if kind == "pix2pix":
        for k, index in enumerate(order):
            place = indices.index(index) % 2                                                   # its place in its batch of 2
            grey = ds["images"][k][:, W:]
            want = np.uint8(np.float32(1.2 + 0.1 * place) / 4.8 * 255)
            assert (grey[1:] == want).all() and (grey[0, 0] == 0).all() and (grey[..., 0] == grey[..., 2]).all()
    npy = sorted(p for p in os.listdir(tmp_path) if p.endswith(".npy"))
    if kind == "smpl":
        assert npy == sorted(f"{w}_{i:03d}.npy" for w in ("depth", "warp") for i in indices)
        d, w = np.load(tmp_path / "depth_003.npy"), np.load(tmp_path / "warp_003.npy")
        assert d.shape == (6, W) and w.shape == (6, W, 3) and d[0, 0] == 0 and np.allclose(w[1, 1], 3 * d[1, 1])
    else:
        assert npy == []


def test_write_split_refuses_what_it_cannot_write(tmp_path):
    with pytest.raises(ValueError, match="unknown"):
        CD.write_split(str(tmp_path), StubRenderer(), "video", np.eye(4)[None], [0])
    with pytest.raises(ValueError, match="human_poses"):
        CD.write_split(str(tmp_path), StubRenderer(), "smpl", np.eye(4)[None], [0])


def test_synthetic_uv_and_texture_are_seeded_and_in_range():
    v = synthetic_smpl.surface_smpl_arrays(11, level=2)["v_template"]
    uv, tex = synthetic_smpl.surface_uv(v, 3), synthetic_smpl.smooth_texture(4, 24, 40)
    assert uv.shape == (len(v), 2) and uv.dtype == np.float32 and uv.min() >= 0 and uv.max() <= 1 and uv.std(0).min() > 0.1
    assert tex.shape == (24, 40, 3) and tex.dtype == np.float32 and tex.min() >= 0 and tex.max() <= 1 and tex.std() > 0.05
    assert np.array_equal(uv, synthetic_smpl.surface_uv(v, 3)) and np.array_equal(tex, synthetic_smpl.smooth_texture(4, 24, 40))
    assert not np.array_equal(uv, synthetic_smpl.surface_uv(v, 4)) and not np.array_equal(tex, synthetic_smpl.smooth_texture(5, 24, 40))


def test_the_operator_refuses_before_loading_the_library(monkeypatch):
    from smpl_nerf_amd import ops
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    s = MR.scene(8, 8, 20)
    T = torch.from_numpy
    poses, v, f, uv, tex = T(s["poses"]), T(s["vertices"][0]), T(s["faces"]), T(s["uv"]), T(s["texture"])
    with pytest.raises(RuntimeError, match="int32"):
        ops.render_mesh(poses, 7.0, 8, 8, v, f.long(), uv, tex)
    bad = f.clone()
    bad[3, 1] = len(v)
    with pytest.raises(RuntimeError, match="outside"):
        ops.render_mesh(poses, 7.0, 8, 8, v, bad, uv, tex)
    with pytest.raises(RuntimeError, match="float64"):
        ops.render_mesh(poses.float(), 7.0, 8, 8, v, f, uv, tex)
    with pytest.raises(RuntimeError, match="bodies"):
        ops.render_mesh(poses, 7.0, 8, 8, torch.stack([v, v]), f, uv, tex)
    with pytest.raises(RuntimeError, match="uv"):
        ops.render_mesh(poses, 7.0, 8, 8, v, f, uv[:-1], tex)
    with pytest.raises(RuntimeError, match="canon"):
        ops.render_mesh(poses, 7.0, 8, 8, v, f, uv, tex, canon=v[:-1])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.render_mesh(poses, 7.0, 8, 8, v, f, uv, tex)


def test_the_entries_are_exported_and_prototyped(lib):
    header = open(_lib.HERE + "/../include/smplnerf.h").read()
    for name, nargs in (("snerf_mesh_render_f32", 27), ("snerf_mesh_render_workspace_bytes", 3)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and name + "(" in header
    assert "SNERF_RENDER_NO_CULL 1" in header and _lib.RENDER_NO_CULL == 1 and ctypes.sizeof(_lib.MeshRenderArgs) == 24
    assert "not pyrender's metallic-roughness shader" in header and lib.snerf_version() == 109
    assert lib.snerf_mesh_render_workspace_bytes(3, 12, 20) == 4 * 3 * (13 * 20 + 3 * 12)
    assert lib.snerf_mesh_render_workspace_bytes(0, 12, 20) == 0
    assert lib.snerf_mesh_render_workspace_bytes(1, 0, 20) == -1 and lib.snerf_mesh_render_workspace_bytes(1, 12, 0) == -1
    assert lib.snerf_mesh_render_workspace_bytes(-1, 12, 20) == -1
    assert lib.snerf_mesh_render_workspace_bytes(1, 12, (1 << 31) // 9 + 1) == -1 and b"F" in lib.snerf_last_error_string()


def test_the_entry_validates_on_the_host(lib):
    N, one = None, 8        # any non-null "pointer": validation never dereferences
    args = _lib.MeshRenderArgs(0.0, 1.0, (ctypes.c_float * 3)(1, 1, 1), 0)
    ws_bytes = 4 * 2 * (13 * 4 + 3 * 9)
    names = "poses vertices faces vf_offsets vf_faces uv texture image t face bary".split()

    def render(n=2, H=9, W=13, Nv=1, V=9, F=4, Ht=5, Wt=6, focal=7.0, a=ctypes.byref(args), canon=N, depth=N, warp=N, ws=one, nbytes=ws_bytes,
               **null):
        p = {k: (N if null.get(k) else one) for k in names}
        return lib.snerf_mesh_render_f32(p["poses"], focal, n, H, W, p["vertices"], Nv, V, p["faces"], F, p["vf_offsets"], p["vf_faces"],
                                         p["uv"], p["texture"], Ht, Wt, a, canon, p["image"], p["t"], p["face"], p["bary"], depth, warp, ws,
                                         nbytes, N)

    err = lib.snerf_last_error_string
    assert render(n=0, a=N, ws=N, nbytes=0, **{k: True for k in names}) == 0                  # N = 0: a no-op, also with null pointers
    assert render(n=0, canon=one) == 0 and render(n=0, Nv=5) == 0                              # ... before anything else is looked at
    assert render(n=-1) == -1 and b"N" in err()
    for bad in ("H", "W", "Ht", "Wt"):
        assert render(**{bad: 0}) == -1 and b"at least 1" in err() and render(n=0, **{bad: 0}) == -1      # a bad scalar whatever N is
    for focal in (0.0, -1.0, float("nan"), float("inf")):
        assert render(focal=focal) == -1 and b"focal" in err()
    assert render(V=0) == -1 and b"V must" in err() and render(F=0) == -1 and b"F must" in err() and render(n=0, F=0) == -1
    assert render(F=(1 << 31) // 9 + 1) == -1 and b"below 2^31" in err()
    assert render(Nv=3) == -1 and b"Nv" in err() and render(Nv=0) == -1 and render(n=3, Nv=2, nbytes=1 << 20) == -1
    for k in names:
        assert render(**{k: True}) == -1 and b"null" in err(), k
    assert render(a=N) == -1 and b"null" in err()
    for canon, warp, depth in ((one, N, one), (one, one, N), (N, one, one), (one, N, N), (N, one, N), (N, N, one)):
        assert render(canon=canon, warp=warp, depth=depth) == -1 and b"all null or all non-null" in err()
    assert render(ws=N) == -1 and b"workspace" in err()
    assert render(nbytes=ws_bytes - 1) == -1 and b"workspace" in err()
    assert render(canon=one, warp=one, depth=one, nbytes=ws_bytes - 1) == -1 and b"workspace" in err()
    assert render(n=1 << 20, H=1 << 14, W=1 << 14) == -1 and b"2^31" in err()                  # N x tiles
    assert render(n=65536, H=8, W=8, nbytes=1 << 40) == -1 and b"65536" in err()
    assert render(Ht=1 << 15, Wt=1 << 15) == -1 and b"2^31" in err()
    # the order: a bad scalar before a null pointer, a null pointer before the workspace
    assert render(F=0, poses=True, ws=N) == -1 and b"F must" in err()
    assert render(poses=True, ws=N) == -1 and b"null" in err()


@pytest.mark.parametrize("case", MR.F64_CASES)
def test_the_float64_cases_keep_their_margins(case):
    """Before a kernel runs, with the float64 reference alone: at most 2 % of a case's hit pixels sit where fp32 may decide a pair
    or order two hits otherwise (single_sample_ref.first_hit_margin), and enough pixels hit."""
    s = MR.scene(*case)
    y64 = MR.render(s, torch.float64)
    hit = y64["face"] >= 0
    out = MR.left_out(s) & hit
    print(f"{case}: {int(hit.sum())} of {hit.size} pixels hit, {int(out.sum())} left out")
    assert hit.sum() >= 0.1 * hit.size and out.sum() <= 0.02 * hit.sum()
    # the fp32 restatement agrees with the float64 one where nothing is left out: the yardstick and the comparison are one rule
    y32 = MR.render(s, torch.float32)
    keep = hit & ~out
    assert np.array_equal(y32["face"][keep], y64["face"][keep])
    assert np.abs(y32["image"][keep] - y64["image"][keep]).max() < 1e-4 and y64["image"][keep].std() > 0.05
    assert (y64["image"][~hit] == np.asarray(MR.SHADING["background"], np.float32).astype(np.float64)).all()
