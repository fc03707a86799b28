"""The first hit of a ray on a mesh on the GPU (csrc/ray_mesh.hip, ops.ray_mesh_first_hit), SingleSamplePipeline and the
SingleSampleRays data set.

Yardstick: the float64 restatement (tests/single_sample_ref.py) of the same fp32 inputs; never the kernel.  The face, the miss
pattern (-1, +inf, zero uv, warp and depth) are compared exactly, values by E(kernel) <= 8 E(fp32 CPU restatement) with
E(y) = max|y - y64| / max|y64| (the measure and the factor of tests/test_gpu_vertex_sphere.py).  Every test prints its figures
before it asserts (pytest -s; profiles/first_hit_errors.txt holds a run).

Margins, asserted on the CPU before a kernel runs: a ray is left out when vertex_sphere_ref.ambiguous_rays names it (fp32 may
decide one of its pairs otherwise) or when its two smallest float64 hit parameters are closer than 1e-4 (fp32 may order them
otherwise: t is of order 2, its fp32 rounding 2e-7, the arithmetic's error some 1e-6); at most 5 % of a case's rays.  Measured on the
CPU: 0, 0, 0, 0, 1, 2, 2 and 5 rays of 63 .. 130 left out, all by the first rule; the smallest gap kept is 1.36e-4 (the soup)."""
import functools

import numpy as np
import pytest
import torch

import single_sample_ref as SS
import vertex_sphere_ref as SR
from conftest import load_golden

pytestmark = pytest.mark.gpu
FACTOR = 8.0

# the kernel's edges: 64-ray chunks (1 = one lane, 63 a short chunk, 65 two chunks, 130 three); 8 face slices walked four per wait
# (F = 1: one slice; 20: slices of 3, tail loop only; 320 / 1280: whole fours)
CASES = [(R, F) for R in (1, 63, 65, 130) for F in (1, 20, 320, 1280)] + [(65, 13776)]
VALUES = ("t", "uv", "depth", "warp")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(R, F, scale=1.0, away=False):
    """Inputs, margins and both restatements of one (R, F), computed once: dict of numpy arrays."""
    o, d, v, f, canon = SS.case_inputs(R, F, scale, away)
    c = {"o": o, "d": d, "v": v, "f": f, "canon": canon}
    c["left_out"], c["gap"] = SS.first_hit_margin(o, d, v, f)
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        c[name] = SS.first_hit(*(torch.from_numpy(a).to(dt) for a in (o, d, v)), f, torch.from_numpy(c["canon"]).to(dt))
    return c


def run(dev, c, canon=True, **kw):
    from smpl_nerf_amd import ops
    o, d, v, f = (torch.from_numpy(c[k]).to(dev) for k in ("o", "d", "v", "f"))
    out = ops.ray_mesh_first_hit(o.requires_grad_(True), d, v.requires_grad_(True), f,
                                 canon=torch.from_numpy(c["canon"]).to(dev).requires_grad_(True) if canon else None, **kw)
    R = len(c["o"])
    assert len(out) == (5 if canon else 3) and all(x.grad_fn is None and not x.requires_grad for x in out)
    assert [tuple(x.shape) for x in out] == [(R,), (R,), (R, 2), (R, 3), (R,)][:len(out)]
    assert out[1].dtype == torch.int32 and all(x.dtype == torch.float32 for i, x in enumerate(out) if i != 1)
    return dict(zip(("t", "face", "uv", "warp", "depth"), (N(x) for x in out)))


def hold(tag, c, got, min_hit_share=0.2):
    keep, y64, y32 = ~c["left_out"], c["64"], c["32"]
    hit = y64["face"] >= 0
    share = float(hit.mean())
    print(f"{tag}: rays that hit {share:.2f}, left out {int((~keep).sum())} of {len(keep)}, smallest gap kept {c['gap']:.2e}")
    assert (~keep).sum() <= 0.05 * len(keep), f"{tag}: too many rays sit on an edge: choose another seed"
    assert share >= min_hit_share, f"{tag}: only {share:.2f} of the rays hit"
    assert np.array_equal(got["face"][keep], y64["face"][keep]), f"{tag}: faces differ on rays {np.nonzero(keep & (got['face'] != y64['face']))[0][:8]}"
    miss = got["face"] < 0                                                  # the miss pattern, on ALL rays, by the kernel's own face
    assert np.isposinf(got["t"][miss]).all() and np.isfinite(got["t"][~miss]).all() and (got["t"][~miss] > 0).all(), f"{tag}: t"
    assert not got["uv"][miss].any() and (got["face"][~miss] < len(c["f"])).all(), f"{tag}: uv of a miss"
    if "warp" in got:
        assert not got["warp"][miss].any() and not got["depth"][miss].any() and (got["depth"][~miss] > 0).all(), f"{tag}: warp / depth of a miss"
    sel = keep & hit
    for name in VALUES:
        if name in got and sel.any():
            ek, ec = SR.relative_error(got[name][sel], y64[name][sel]), SR.relative_error(y32[name][sel], y64[name][sel])
            print(f"{tag}: {name:5s} E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  ratio {ek / ec if ec else 0.0:.2f}")
            assert ek <= FACTOR * ec, f"{tag}: {name}: E kernel {ek:.3e} > {FACTOR} x E fp32 CPU {ec:.3e}"


# ---------------------------------------------------------------------------------------------- the first hit
@pytest.mark.parametrize("R,F", CASES)
def test_first_hit(dev, R, F):
    c = case(R, F)
    assert c["left_out"].sum() <= 0.05 * R                          # (before the kernel runs)
    hold(f"first hit R={R} F={F}", c, run(dev, c))


@pytest.mark.parametrize("R,F", [(1, 1), (63, 20), (65, 320), (130, 1280), (65, 13776)])
def test_t_is_the_head_of_the_hit_list_and_canon_changes_nothing(dev, R, F):
    from smpl_nerf_amd import ops
    c = case(R, F)
    with_canon, without = run(dev, c), run(dev, c, canon=False, faces_checked=True)
    t_hits, n_hits = ops.ray_mesh_hits(*(torch.from_numpy(c[k]).to(dev) for k in ("o", "d", "v", "f")), max_hits=1)
    assert np.array_equal(with_canon["t"], N(t_hits)[:, 0])                 # all rays, bit for bit
    assert np.array_equal(with_canon["face"] >= 0, N(n_hits) > 0)
    assert all(np.array_equal(with_canon[k], without[k]) for k in ("t", "face", "uv"))


def test_two_runs_are_bit_identical(dev):
    c = case(130, 1280)
    a, b = run(dev, c), run(dev, c)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_a_tie_goes_to_the_smaller_face_index(dev):
    o, d, v, f, canon = SS.tie_case()
    c = {"o": o, "d": d, "v": v, "f": f, "canon": canon}
    got = run(dev, c)
    want = SS.first_hit(*(torch.from_numpy(a) for a in (o, d, v)), f, torch.from_numpy(canon))
    assert (want["face"] == 3).all() and np.array_equal(got["face"], want["face"])
    assert np.array_equal(got["t"], want["t"]) and np.abs(got["warp"] - want["warp"]).max() < 1e-5       # face 3's canon, not face 7's


def test_directions_need_not_be_normalised(dev):
    """With d scaled by 3: the same face and the same point of it, t a third, and the same depth - the sample of the data set sits
    at t |d| along the unit direction."""
    c3, c1 = case(65, 320, scale=3.0), case(65, 320)
    got = run(dev, c3)
    hold("first hit, directions x 3", c3, got)
    both = ~(c3["left_out"] | c1["left_out"]) & (c1["64"]["face"] >= 0)
    base = run(dev, c1)
    assert np.array_equal(got["face"][both], base["face"][both])
    for name, want in (("uv", c1["64"]["uv"]), ("t", c1["64"]["t"] / 3), ("depth", c1["64"]["depth"])):
        ek = SR.relative_error(got[name][both], want[both])
        ec = SR.relative_error(c3["32"][name][both], want[both])
        print(f"directions x 3: {name:5s} against the unscaled float64 E kernel {ek:.3e}  E fp32 CPU {ec:.3e}")
        assert ek <= FACTOR * ec


def test_rays_aimed_away_hit_nothing(dev):
    c = case(130, 320, away=True)
    assert (c["64"]["face"] == -1).all() and not c["left_out"].any()
    got = run(dev, c)
    assert (got["face"] == -1).all() and np.isposinf(got["t"]).all()
    assert not got["uv"].any() and not got["warp"].any() and not got["depth"].any()


@pytest.mark.parametrize("canon", [False, True])
def test_the_call_writes_nothing_but_its_outputs(dev, canon):
    """The C entry on outputs and a workspace cut out of larger buffers: the canaries around them stay, every element between
    them is written."""
    from smpl_nerf_amd import _lib
    lib = _lib.load()
    c, pad, R, F = case(65, 320), 64, 65, 320
    o, d, v, f, cn = (torch.from_numpy(c[k]).to(dev) for k in ("o", "d", "v", "f", "canon"))
    sizes = {"t": R, "face": R, "uv": 2 * R, "warp": 3 * R, "depth": R}
    bufs = {k: torch.full((pad + n + pad,), -7, device=dev, dtype=torch.int32 if k == "face" else torch.float32) for k, n in sizes.items()}
    nbytes = lib.snerf_ray_mesh_workspace_bytes(F)
    sizes["ws"], bufs["ws"] = nbytes // 4, torch.full((pad + nbytes // 4 + pad,), -7.0, device=dev)
    p = {k: b[pad:].data_ptr() for k, b in bufs.items()}
    rc = lib.snerf_ray_mesh_first_hit_f32(o.data_ptr(), d.data_ptr(), v.data_ptr(), f.data_ptr(), R, len(c["v"]), F,
                                          cn.data_ptr() if canon else None, p["t"], p["face"], p["uv"], p["warp"] if canon else None,
                                          p["depth"] if canon else None, p["ws"], nbytes, _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert (b[:pad] == -7).all() and (b[pad + sizes[k]:] == -7).all(), k
    if not canon:
        assert (bufs["warp"] == -7).all() and (bufs["depth"] == -7).all()
    got = {k: N(bufs[k][pad:pad + sizes[k]]) for k in (sizes if canon else ("t", "face", "uv")) if k != "ws"}
    got["uv"] = got["uv"].reshape(R, 2)
    assert not any((x == -7).any() for x in got.values())
    if canon:
        got["warp"] = got["warp"].reshape(R, 3)
    hold(f"first hit into cut-out buffers, canon={canon}", c, got)


# ---------------------------------------------------------------------------------------------- SingleSamplePipeline
@pytest.fixture(scope="module")
def g21():
    return load_golden("g21_single_sample.npz"), SS.g21_inputs()


def _pipeline(dev, params):
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import PipelineArgs, SingleSamplePipeline
    net = RenderRayNet(8, 256, 60, 24, skips=[4])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net = net.to(dev).train()
    return SingleSamplePipeline(net, PipelineArgs(run_fine=0), PositionalEncoder(10, 0), PositionalEncoder(4, 0)), net


def test_pipeline_against_the_reference(dev, g21):
    """rgb by the 8 x rule, measured against the float64 restatement, with two fp32 comparisons: what the reference computed on
    the CPU (the golden) and the fp32 torch restatement (which reproduces the golden: tests/test_first_hit_host.py)."""
    g, (batch_np, params) = g21
    pipe, _ = _pipeline(dev, params)
    batch = [torch.from_numpy(a).to(dev) for a in batch_np]
    with torch.no_grad():
        out = pipe(batch)
        rendered = pipe.render_rays(batch)
    assert len(out) == 2 and out[0] is out[1] and tuple(out[0].shape) == (130, 3) and torch.equal(rendered[0], out[0])
    ys = [N(SS.single_sample_pipeline({k: torch.from_numpy(v).to(dt) for k, v in params.items()}, [torch.from_numpy(a).to(dt) for a in batch_np]))
          for dt in (torch.float64, torch.float32)]
    rgb = N(out[0])
    ek, ec = SR.relative_error(rgb, ys[0]), SR.relative_error(ys[1], ys[0])
    eg = SR.relative_error(g["rgb"], ys[0])
    print(f"pipeline rgb against float64: E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  ratio {ek / ec if ec else 0.0:.2f}  E reference (golden) {eg:.3e}; "
          f"max |kernel - golden| {np.abs(rgb - g['rgb']).max():.3e}")
    assert ek <= FACTOR * ec and ek <= FACTOR * eg      # (the golden is the reference's own fp32 evaluation: the second comparison)
    loss = torch.nn.functional.mse_loss(out[0], batch[5]).item()
    print(f"pipeline loss {loss:.8f} (reference {g['loss'][0]:.8f})")
    assert abs(loss - g["loss"][0]) <= 1e-5


def test_three_adam_steps(dev, g21):
    """The colour field trained under the trainer (autograd path, the library's Adam): the loss of three steps against the same
    three steps of the restated pipeline in float64."""
    from smpl_nerf_amd.trainer import DataParallelTrainer, HipAdam
    _, (batch_np, params) = g21
    lr = 2e-5
    pipe, net = _pipeline(dev, params)
    tr = DataParallelTrainer(pipe, [net], lr=lr)
    assert isinstance(tr.optim, HipAdam) and tr._one_call_state() is None
    batch = [torch.from_numpy(a).to(dev) for a in batch_np]
    got = np.array([tr.step(batch).item() for _ in range(3)])
    ys = []
    for dtype in (torch.float64, torch.float32):
        P = {k: torch.from_numpy(v).to(dtype).clone().requires_grad_(True) for k, v in params.items()}
        b = [torch.from_numpy(a).to(dtype) for a in batch_np]
        opt = torch.optim.Adam(list(P.values()), lr=lr)
        traj = []
        for _ in range(3):
            opt.zero_grad()
            loss = 2 * torch.nn.functional.mse_loss(SS.single_sample_pipeline(P, b), b[5])       # rgb is rgb_fine: nerf_solver.py:48-52
            loss.backward()
            opt.step()
            traj.append(loss.item())
        ys.append(np.array(traj))
    ek, ec = SR.relative_error(got, ys[0]), SR.relative_error(ys[1], ys[0])
    print(f"three Adam steps: losses {got}; E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  ratio {ek / ec if ec else 0.0:.2f}")
    assert got[2] < got[0], "three steps did not lower the loss"
    assert ek <= FACTOR * ec


# ---------------------------------------------------------------------------------------------- SingleSampleRays
def _data_set(dev):
    from smpl_nerf_amd import synthetic as syn
    from smpl_nerf_amd.body_model import SmplBodyModel
    from smpl_nerf_amd.pipelines import PipelineArgs
    from smpl_nerf_amd.single_sample import SingleSampleRays
    from smpl_nerf_amd.synthetic_smpl import surface_smpl_arrays
    body = SmplBodyModel.from_arrays(**surface_smpl_arrays(11, level=2)).to(dev)
    h = w = 16
    # (no camera at theta = 0: pixel column 8 of an even width looks along x = 0, the body's symmetry plane, which holds mesh edges -
    # 13 of its 16 rays run along one and are ambiguous by construction)
    images = (np.stack([syn.procedural_image(h, w, 0.0, t) for t in (15.0, 40.0)]) * 255).astype(np.uint8)
    transforms = np.stack([syn.sphere_pose(0.0, t, 2.4) for t in (15.0, 40.0)])
    poses = syn.human_poses((41, 38), 0, 60, 3)[1:]           # (both frames posed: in the zero pose the warp is zero and E has no scale)
    a = PipelineArgs(near=1.0, far=4.0)
    return SingleSampleRays(images, transforms, 0.6, poses, np.zeros((1, 10), np.float32), body, a, dev), body, poses, images


def test_data_set(dev):
    ds, body, poses, images = _data_set(dev)
    again = _data_set(dev)[0]
    assert len(ds) == 512
    item = ds[300]
    assert [tuple(t.shape) for t in item] == [(3,), (3,), (3,), (69,), (3,), (3,)] and all(t.dtype == torch.float32 for t in item)
    assert np.array_equal(N(item[5]), images.reshape(-1, 3)[300].astype(np.float32) / np.float32(255))
    assert np.array_equal(N(item[3]), poses[1]) and torch.equal(item[4], ds.all_warps[300]) and torch.equal(item[0], ds.ray_samples[300])
    assert tuple(ds.depth.shape) == (512,) and tuple(ds.face.shape) == (512,) and ds.face.dtype == torch.int32 and tuple(ds.uv.shape) == (512, 2)
    assert tuple(ds.depth_images().shape) == (2, 16, 16) and tuple(ds.warp_images().shape) == (2, 16, 16, 3)
    assert torch.equal(ds.depth_images().reshape(-1), ds.depth) and torch.equal(ds.warp_images().reshape(-1, 3), ds.all_warps)
    hit = ds.face >= 0
    print(f"data set: {int(hit.sum())} of 512 rays hit the body")
    assert 20 <= int(hit.sum()) <= 400 and torch.equal(hit, ds.depth > 0)
    # the directions are get_rays': not normalised; the sample sits at depth (far on a miss) along the unit direction
    o, d = ds.rays_translation, ds.rays_direction
    assert float((torch.linalg.vector_norm(d.double(), dim=-1) - 1).abs().max()) > 1e-3
    unit = d / torch.norm(d, dim=-1, keepdim=True)
    assert torch.equal(ds.ray_samples[hit], (o + unit * ds.depth[:, None])[hit])
    assert torch.equal(ds.ray_samples[~hit], (o + unit * 4.0)[~hit])
    # warp and depth against the restatement of the same fp32 rays and bodies, frame by frame
    betas = torch.zeros(1, 10, device=dev)
    canon = body(betas=betas, body_pose=torch.zeros(1, 69, device=dev)).vertices[0]
    assert torch.equal(ds.canonical, canon)
    f = N(body.faces)
    for i in range(2):
        sl = slice(256 * i, 256 * (i + 1))
        goal = body(betas=betas, body_pose=torch.from_numpy(poses[i:i + 1]).to(dev)).vertices[0]
        oi, di, vi, ci = N(o[sl]), N(d[sl]), N(goal), N(canon)
        left_out, _ = SS.first_hit_margin(oi, di, vi, f)
        y64, y32 = (SS.first_hit(*(torch.from_numpy(a).to(dt) for a in (oi, di, vi)), f, torch.from_numpy(ci).to(dt))
                    for dt in (torch.float64, torch.float32))
        keep = ~left_out
        sel = keep & (y64["face"] >= 0)
        print(f"data set frame {i}: left out {int(left_out.sum())} of 256, hit {int(sel.sum())}")
        assert left_out.sum() <= 0.05 * 256 and sel.sum() >= 10
        assert np.array_equal(N(ds.face[sl])[keep], y64["face"][keep])
        for name, got in (("depth", N(ds.depth[sl])), ("warp", N(ds.all_warps[sl])), ("uv", N(ds.uv[sl]))):
            ek, ec = SR.relative_error(got[sel], y64[name][sel]), SR.relative_error(y32[name][sel], y64[name][sel])
            print(f"data set frame {i}: {name:5s} E kernel {ek:.3e}  E fp32 CPU {ec:.3e}")
            assert ek <= FACTOR * ec
    assert float(ds.all_warps[hit].abs().amax()) > 1e-3                      # the second frame's pose moves the surface
    batches = list(ds.batches(200))
    assert [len(b[0]) for b in batches] == [200, 200, 112] and all(len(b) == 6 and all(t.is_cuda for t in b) for b in batches)
    assert torch.equal(torch.cat([b[4] for b in batches]), ds.all_warps) and tuple(batches[0][3].shape) == (200, 69)
    for name in ("ray_samples", "rays_translation", "rays_direction", "human_poses", "all_warps", "depth", "face", "uv", "rgb"):
        assert torch.equal(getattr(ds, name), getattr(again, name)), name     # twice: the same bits
