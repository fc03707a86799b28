"""The mesh renderer on the GPU (csrc/mesh_render.hip, ops.render_mesh), create_dataset.BodyRenderer and estimator.rendered_batches.

Three yardsticks, none of them the kernel under test:
  * the hit outputs (t, face, bary, depth, warp) against ops.ray_mesh_first_hit on the rays RayGenerator makes for the same poses:
    bit for bit, with and without the cull;
  * the image against the fp32 numpy restatement of the normals and the shading (tests/mesh_render_ref.py) evaluated on the
    device's own face and bary: bit for bit, background included;
  * everything against the float64 restatement end to end, on the pixels single_sample_ref.first_hit_margin does not name (at most
    2 % of the hit pixels, asserted on the CPU in tests/test_mesh_render_host.py): the float64 face, and an image error of at most
    twice the fp32 CPU restatement's own, E(y) = max|y - y64| / max|y64| on the same pixels.
Every test prints its figures before it asserts (pytest -s; profiles/mesh_render_errors.txt holds a run)."""
import numpy as np
import pytest
import torch

import mesh_render_ref as MR
import single_sample_ref as SS
import vertex_sphere_ref as SR
from smpl_nerf_amd import synthetic as syn

pytestmark = pytest.mark.gpu

# the kernel's edges: one 8 x 8 tile, clipped tiles on both edges, 16 tiles; one face slice (F = 1), slices of 3 (tail loop only),
# whole fours; one frame, three frames with a body each, three frames of one body
SIZES = [(8, 8), (9, 13), (32, 32)]
FACES = [1, 20, 320, 1280]
SCENES = [(H, W, F, 1, 1) for H, W in SIZES for F in FACES] + [(9, 13, F, 3, b) for F in FACES for b in (3, 1)] + [(32, 32, 1280, 3, 3)]
HIT_KEYS = ("t", "face", "bary", "depth", "warp")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def focal_of(W):
    return float(.5 * W / np.tan(.5 * MR.ANGLE))


def on_device(dev, s):
    T = torch.from_numpy
    v = T(s["vertices"]).to(dev)
    return dict(poses=T(s["poses"]).to(dev), vertices=v if len(v) > 1 else v[0], faces=T(s["faces"]).to(dev), uv=T(s["uv"]).to(dev),
                texture=T(s["texture"]).to(dev), canon=T(SS.canon_of(s["vertices"][0])).to(dev))


def render(dev, s, canon=True, **kw):
    from smpl_nerf_amd import ops
    d = on_device(dev, s)
    out = ops.render_mesh(d["poses"], focal_of(s["W"]), s["H"], s["W"], d["vertices"], d["faces"], d["uv"], d["texture"],
                          canon=d["canon"] if canon else None, **dict(MR.SHADING, **kw))
    n, H, W = len(s["poses"]), s["H"], s["W"]
    shapes = dict(image=(n, H, W, 3), t=(n, H, W), face=(n, H, W), bary=(n, H, W, 2), depth=(n, H, W), warp=(n, H, W, 3))
    for k, x in out._asdict().items():
        if x is None:
            assert not canon and k in ("depth", "warp")
            continue
        assert tuple(x.shape) == shapes[k] and x.dtype == (torch.int32 if k == "face" else torch.float32) and x.grad_fn is None, k
    return {k: N(x) for k, x in out._asdict().items() if x is not None}


def first_hits(dev, s):
    """The parent's path, frame by frame: RayGenerator.batch, then ops.ray_mesh_first_hit with the same canon."""
    from smpl_nerf_amd import ops
    from smpl_nerf_amd.raygen import RayGenerator
    d = on_device(dev, s)
    n, H, W = len(s["poses"]), s["H"], s["W"]
    gen = RayGenerator(s["poses"], H, W, MR.ANGLE, 1.0, 4.0, 1, dev)
    assert gen.focal == focal_of(W)
    out = {k: [] for k in HIT_KEYS}
    for i in range(n):
        index = torch.arange(i * H * W, (i + 1) * H * W, device=dev)
        _, o, dirs, _, _ = gen.batch(index, torch.zeros(H * W, device=dev, dtype=torch.float64))
        v = d["vertices"] if d["vertices"].dim() == 2 else d["vertices"][i]
        t, face, uv, warp, depth = ops.ray_mesh_first_hit(o, dirs, v, d["faces"], canon=d["canon"])
        for k, x in zip(HIT_KEYS, (t, face, uv, depth, warp)):
            out[k].append(N(x))
    return {k: np.stack(x).reshape((n, H, W) + x[0].shape[1:]) for k, x in out.items()}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def hold_hits(tag, dev, s, min_hits=1):
    want = first_hits(dev, s)
    for cull in (True, False):
        got = render(dev, s, cull=cull)
        hits = int((got["face"] >= 0).sum())
        print(f"{tag} cull={cull}: {hits} of {got['face'].size} pixels hit")
        assert hits >= min_hits, f"{tag}: nothing to compare"
        for k in HIT_KEYS:
            assert same_bits(got[k], want[k]), f"{tag} cull={cull}: {k} differs from ray_mesh_first_hit on {int((got[k] != want[k]).sum())} elements"
    return got


def restated_image(s, got, dtype=np.float32):
    return np.stack([MR.shade(s["vertices"][n if len(s["vertices"]) > 1 else 0], s["faces"], s["uv"], s["texture"], s["poses"][n],
                              got["face"][n], got["bary"][n], dtype, **MR.SHADING).reshape(s["H"], s["W"], 3) for n in range(len(s["poses"]))])


# ---------------------------------------------------------------------------------------------- the hit
@pytest.mark.parametrize("H,W,F,frames,bodies", SCENES)
def test_hits_are_the_first_hit_kernels_bit_for_bit(dev, H, W, F, frames, bodies):
    s = MR.scene(H, W, F, frames, bodies)
    got = hold_hits(f"{H}x{W} F={F} N={frames} bodies={bodies}", dev, s)
    miss = got["face"] < 0
    assert np.isposinf(got["t"][miss]).all() and not got["bary"][miss].any() and not got["depth"][miss].any() and not got["warp"][miss].any()
    assert (got["image"][miss] == np.asarray(MR.SHADING["background"], np.float32)).all()


def test_the_walks_real_length(dev):
    """One 128 x 128 frame on the 13 776-face soup: 1722 faces per wave."""
    got = hold_hits("128x128 F=13776", dev, MR.scene(128, 128, 13776), min_hits=1000)
    assert len(np.unique(got["face"])) > 500


def test_a_camera_inside_the_mesh(dev):
    v, f = MR.mesh(320)
    s = MR.custom_scene([syn.pose_matrix(x=0.02, y=0.1, z=-0.03, phi=20.0, theta=50.0)], v, f, 9, 13)
    got = hold_hits("camera inside", dev, s)
    assert (got["face"] >= 0).all()                                           # a closed surface seen from inside: every pixel hits


def test_faces_that_cross_the_camera_plane(dev):
    """A camera just outside the surface looking along it, and one inside near the wall: faces with corners on both sides of the
    camera plane, whose boxes are 'everything'."""
    v, f = MR.mesh(1280)
    top = float(v[:, 0].max())
    poses = [syn.pose_matrix(x=top + 0.02, y=0.05, z=0.0, theta=0.0), syn.pose_matrix(x=0.0, y=0.5, z=0.1, phi=-60.0)]
    for p in poses:                                                           # (asserted here, not supposed: corners on both sides)
        depth = -((v.astype(np.float64) - p[:3, 3]) @ p[:3, :3])[:, 2]
        crossing = ((depth[f] > 0).any(1) & (depth[f] <= 0).any(1)).sum()
        assert crossing >= 10, crossing
    hold_hits("faces across the camera plane", dev, MR.custom_scene(poses, v, f, 32, 32), min_hits=50)


def test_one_large_triangle_with_a_vertex_behind_the_camera(dev):
    v = np.array([[-1.0, -1.2, -1.0], [1.1, -1.0, -1.0], [0.1, 0.6, 3.5]], np.float32)
    s = MR.custom_scene([syn.pose_matrix(z=2.4)], v, [[0, 1, 2]], 32, 32)
    got = hold_hits("vertex behind the camera", dev, s, min_hits=100)
    assert (got["face"] < 0).any()


def test_a_tie_goes_to_the_smaller_face_index(dev):
    o, d, v, f, canon = SS.tie_case()
    s = MR.custom_scene([syn.pose_matrix(x=float(o[0, 0]), y=float(o[0, 1]), z=float(o[0, 2]))], v, f, 32, 32)
    got = hold_hits("tie", dev, s, min_hits=20)
    hit = got["face"] >= 0
    assert (got["face"][hit] == 3).all()                                      # faces 3 and 7 coincide: the same t, the smaller index


# ---------------------------------------------------------------------------------------------- the image
@pytest.mark.parametrize("H,W,F,frames,bodies", [(8, 8, 1, 1, 1), (9, 13, 20, 3, 3), (32, 32, 320, 1, 1), (32, 32, 1280, 3, 1), (32, 32, 1280, 3, 3)])
def test_the_image_is_the_fp32_restatement_bit_for_bit(dev, H, W, F, frames, bodies):
    s = MR.scene(H, W, F, frames, bodies)
    got = render(dev, s)
    want = restated_image(s, got)
    hit = got["face"] >= 0
    diff = np.abs(got["image"].astype(np.float64) - want)
    print(f"image {H}x{W} F={F} N={frames} bodies={bodies}: {int(hit.sum())} hit pixels, max |kernel - fp32 restatement| {diff.max():.3e}, "
          f"elements that differ {int((got['image'] != want).sum())}; image std {got['image'][hit].std():.3f}")
    assert hit.any() and (~hit).any() and got["image"][hit].std() > 0.02
    assert same_bits(got["image"], want.astype(np.float32))


@pytest.mark.parametrize("case", MR.F64_CASES)
def test_against_float64_end_to_end(dev, case):
    s = MR.scene(*case)
    got = render(dev, s)
    y64, y32 = MR.render(s, torch.float64), MR.render(s, torch.float32)
    shape = got["face"].shape
    face64, hit = y64["face"].reshape(shape), (y64["face"] >= 0).reshape(shape)
    out = MR.left_out(s).reshape(shape) & hit
    keep = hit & ~out
    print(f"float64 {case}: {int(hit.sum())} hit pixels, {int(out.sum())} left out")
    assert out.sum() <= 0.02 * hit.sum()
    assert np.array_equal(got["face"][~out], face64[~out])
    for name, g, a, b in (("image", got["image"], y32["image"].reshape(shape + (3,)), y64["image"].reshape(shape + (3,))),
                          ("t", got["t"], y32["t"].reshape(shape), y64["t"].reshape(shape)),
                          ("bary", got["bary"], y32["bary"].reshape(shape + (2,)), y64["bary"].reshape(shape + (2,)))):
        ek, ec = SR.relative_error(g[keep], b[keep]), SR.relative_error(a[keep], b[keep])
        print(f"float64 {case}: {name:5s} E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  ratio {ek / ec if ec else 0.0:.2f}")
        assert ek <= 2.0 * ec, f"{name}: E kernel {ek:.3e} > 2 x E fp32 CPU {ec:.3e}"


# ---------------------------------------------------------------------------------------------- the call
def test_two_calls_give_equal_bits(dev):
    s = MR.scene(32, 32, 1280, 3, 3)
    a, b = render(dev, s), render(dev, s)
    assert all(same_bits(a[k], b[k]) for k in a)


def test_poisoned_lds_and_poisoned_empty_change_nothing(dev):
    """SNERF_DEBUG_POISON_LDS=1 (the library fills all LDS with NaNs after every launch) and SNERF_TEST_POISON_EMPTY=1 (conftest
    starts every torch.empty as NaNs / 0xff / -1): the same bits.  Both are read once per process, hence one child."""
    import os
    import subprocess
    import sys
    import tempfile
    base = render(dev, MR.scene(9, 13, 320, 3, 3))
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, numpy as np, torch; sys.path[:0] = [%r, %r]; import conftest; import mesh_render_ref as MR; "
            "import test_gpu_mesh_render as T; probe = torch.empty(4, device='cuda:0'); assert bool(torch.isnan(probe).all()); "
            "np.savez(sys.argv[1], **T.render(torch.device('cuda:0'), MR.scene(9, 13, 320, 3, 3)))" % (os.path.dirname(here), here))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npz")
        env = dict(os.environ, SNERF_DEBUG_POISON_LDS="1", SNERF_TEST_POISON_EMPTY="1")
        subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=300, cwd=here)
        child = dict(np.load(path))
    assert sorted(child) == sorted(base) and all(same_bits(base[k], child[k]) for k in base)


@pytest.mark.parametrize("canon", [False, True])
def test_the_call_writes_every_element_and_nothing_else(dev, canon):
    """The C entry on outputs and a workspace cut out of larger buffers full of a marker: the guard bands stay, every element
    between them is written - miss pixels included - and the result is the operator's."""
    import ctypes
    from smpl_nerf_amd import _lib, ops
    lib = _lib.load()
    s = MR.scene(9, 13, 320, 3, 3)
    d = on_device(dev, s)
    n, H, W, V, F, pad = 3, 9, 13, s["vertices"].shape[1], len(s["faces"]), 64
    sizes = {"image": n * H * W * 3, "t": n * H * W, "face": n * H * W, "bary": n * H * W * 2, "depth": n * H * W, "warp": n * H * W * 3}
    bufs = {k: torch.full((pad + m + pad,), -7, device=dev, dtype=torch.int32 if k == "face" else torch.float32) for k, m in sizes.items()}
    nbytes = lib.snerf_mesh_render_workspace_bytes(n, V, F)
    assert nbytes == 4 * n * (13 * F + 3 * V)
    sizes["ws"], bufs["ws"] = nbytes // 4, torch.full((pad + nbytes // 4 + pad,), -7.0, device=dev)
    p = {k: b[pad:].data_ptr() for k, b in bufs.items()}
    off, vf = (torch.from_numpy(a).to(dev) for a in ops.vertex_face_table(s["faces"], V))
    args = _lib.MeshRenderArgs(MR.SHADING["ambient"], MR.SHADING["intensity"], (ctypes.c_float * 3)(*MR.SHADING["background"]), 0)
    rc = lib.snerf_mesh_render_f32(d["poses"].data_ptr(), focal_of(W), n, H, W, d["vertices"].data_ptr(), 3, V, d["faces"].data_ptr(), F,
                                   off.data_ptr(), vf.data_ptr(), d["uv"].data_ptr(), d["texture"].data_ptr(), 24, 40, ctypes.byref(args),
                                   d["canon"].data_ptr() if canon else None, p["image"], p["t"], p["face"], p["bary"],
                                   p["depth"] if canon else None, p["warp"] if canon else None, p["ws"], nbytes, _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert (b[:pad] == -7).all() and (b[pad + sizes[k]:] == -7).all(), k
    if not canon:
        assert (bufs["warp"] == -7).all() and (bufs["depth"] == -7).all()
    want = render(dev, s, canon=canon)
    assert (want["face"] < 0).any()
    for k, x in want.items():
        got = N(bufs[k][pad:pad + sizes[k]]).reshape(x.shape)
        assert not (got == -7).any(), k
        assert same_bits(got, x), k


def test_the_entry_replays_from_a_graph(dev):
    """One linear capture of the C entry (three launches on one stream, no branches): the replay gives the bits of the eager call,
    also after the outputs have been overwritten."""
    import ctypes
    from smpl_nerf_amd import _lib, ops
    lib = _lib.load()
    s = MR.scene(9, 13, 320, 3, 3)
    d = on_device(dev, s)
    n, H, W, V, F = 3, 9, 13, s["vertices"].shape[1], len(s["faces"])
    want = render(dev, s)
    out = dict(image=torch.zeros(n, H, W, 3, device=dev), t=torch.zeros(n, H, W, device=dev), face=torch.zeros(n, H, W, device=dev, dtype=torch.int32),
               bary=torch.zeros(n, H, W, 2, device=dev), depth=torch.zeros(n, H, W, device=dev), warp=torch.zeros(n, H, W, 3, device=dev))
    nbytes = lib.snerf_mesh_render_workspace_bytes(n, V, F)
    ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    off, vf = (torch.from_numpy(a).to(dev) for a in ops.vertex_face_table(s["faces"], V))
    args = _lib.MeshRenderArgs(MR.SHADING["ambient"], MR.SHADING["intensity"], (ctypes.c_float * 3)(*MR.SHADING["background"]), 0)

    def call():
        rc = lib.snerf_mesh_render_f32(d["poses"].data_ptr(), focal_of(W), n, H, W, d["vertices"].data_ptr(), 3, V, d["faces"].data_ptr(), F,
                                       off.data_ptr(), vf.data_ptr(), d["uv"].data_ptr(), d["texture"].data_ptr(), 24, 40, ctypes.byref(args),
                                       d["canon"].data_ptr(), out["image"].data_ptr(), out["t"].data_ptr(), out["face"].data_ptr(),
                                       out["bary"].data_ptr(), out["depth"].data_ptr(), out["warp"].data_ptr(), ws.data_ptr(), nbytes,
                                       _lib.current_stream())
        assert rc == 0

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for x in out.values():
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, x in out.items():
        assert same_bits(N(x), want[k]), k


# ---------------------------------------------------------------------------------------------- the data-set driver
def _renderer(dev, H=16, W=16):
    from smpl_nerf_amd.body_model import SmplBodyModel
    from smpl_nerf_amd.create_dataset import BodyRenderer
    from smpl_nerf_amd.synthetic_smpl import smooth_texture, surface_smpl_arrays, surface_uv
    arrays = surface_smpl_arrays(11, level=2)
    body = SmplBodyModel.from_arrays(**arrays).to(dev)
    return BodyRenderer(body, surface_uv(arrays["v_template"], 3), smooth_texture(4), MR.ANGLE, H, W, dev), body


def test_body_renderer_frames(dev):
    """Two arm poses through two cameras: the frames differ where the arm moved, and get_warp's depth image is
    SingleSampleRays.depth_images() of the same frames bit for bit; the z-depth is that depth over |d|."""
    from smpl_nerf_amd.pipelines import PipelineArgs
    from smpl_nerf_amd.single_sample import SingleSampleRays
    renderer, body = _renderer(dev)
    transforms = np.stack([syn.sphere_pose(0.0, t, 2.4) for t in (15.0, 40.0)])
    poses = syn.human_poses((41, 38), 0, 60, 3)[1:]
    rgb, zdepth, depth, warp = renderer.frames(transforms, poses, np.zeros(10, np.float32), want_warp=True)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (2, 16, 16, 3) and tuple(zdepth.shape) == (2, 16, 16) and tuple(warp.shape) == (2, 16, 16, 3)
    two = renderer.frames(transforms, poses)
    assert len(two) == 2 and torch.equal(two[0], rgb) and torch.equal(two[1], zdepth)
    ds = SingleSampleRays(N(rgb), transforms, MR.ANGLE, poses, np.zeros((1, 10), np.float32), body, PipelineArgs(near=1.0, far=4.0), dev)
    hit = ds.depth_images() > 0
    print(f"BodyRenderer: {int(hit.sum())} of {hit.numel()} pixels hit")
    assert 20 <= int(hit.sum()) <= 400
    assert torch.equal(depth, ds.depth_images()) and torch.equal(warp, ds.warp_images())            # bit for bit, every pixel
    assert torch.equal(zdepth > 0, hit)
    norm = torch.linalg.vector_norm(ds.rays_direction.double(), dim=-1).view(2, 16, 16)
    ratio = (zdepth.double() * norm / ds.depth_images().double())[hit]
    assert float((ratio - 1).abs().max()) < 4e-7                                                        # t = depth / |d| to fp32 rounding
    # the same camera, the other arm pose: the frames differ, and only where a body is in one of them
    a = renderer.frames(transforms[:1], poses[:1])
    b = renderer.frames(transforms[:1], poses[1:])
    moved = (a[0] != b[0]).any(-1)[0]
    body_pixels = ((a[1] > 0) | (b[1] > 0))[0]
    print(f"BodyRenderer: {int(moved.sum())} pixels differ between the two arm poses, {int(body_pixels.sum())} show a body")
    assert int(moved.sum()) >= 3 and not bool((moved & ~body_pixels).any())
    assert (a[0][0][~(a[1][0] > 0)] == 255).all()                                                       # white background
    # the canonical body for every frame (the `nerf` type)
    c = renderer.frames(transforms)
    assert tuple(c[0].shape) == (2, 16, 16, 3) and int((c[1] > 0).sum()) >= 20


def test_three_training_steps_on_rendered_batches(dev):
    from smpl_nerf_amd import estimator as E
    renderer, _ = _renderer(dev, 128, 128)
    rng = np.random.default_rng(3)

    def sampler(n):
        poses = np.zeros((n, 69), np.float32)
        poses[:, [38, 41]] = rng.uniform(-1.0, 1.0, (n, 2))
        return poses

    transforms = np.stack([syn.sphere_pose(0.0, t, 2.4) for t in (0.0, 20.0, 40.0)])
    torch.manual_seed(0)
    model = E.SmplEstimator(69).to(dev)
    optim = torch.optim.Adam(model.parameters(), lr=1e-4)
    seen = []

    def loader():
        for images, truth in E.rendered_batches(renderer, sampler, transforms, None, 4, 3):
            assert images.is_cuda and tuple(images.shape) == (4, 3, 128, 128) and images.dtype == torch.float32 and tuple(truth.shape) == (4, 69)
            assert 0.0 <= float(images.min()) and float(images.max()) <= 1.0 and float(images.std()) > 0.01
            seen.append(images)
            yield images, truth

    loss = E.train_epoch(model, loader(), optim)
    print(f"three steps on rendered batches: mean loss {loss:.6f}")
    assert len(seen) == 3 and np.isfinite(loss) and not torch.equal(seen[0], seen[1])
