"""The vertex_sphere model on the GPU: ray-mesh hits (csrc/ray_mesh.hip, ops.ray_mesh_hits), the sphere warp
(csrc/vertex_sphere.hip, ops.vertex_sphere_warp), VertexSpherePipeline and the VertexSphereRays data set.

Yardstick: the float64 restatement (tests/vertex_sphere_ref.py) of the same fp32 inputs; never the kernel.  Counts, indices and the
+inf padding are compared exactly, values by E(kernel) <= 8 E(fp32 CPU restatement) with E(y) = max|y - y64| / max|y64| (the measure
and the factor of tests/test_gpu_vertex_warp.py: re-ordered fp32 arithmetic).  Every test prints its figures before it asserts
(pytest -s; profiles/vertex_sphere_errors.txt holds a run).

Margins, asserted on the CPU before a kernel runs.  Ray-mesh: a ray is left out when, in float64, some face has its smallest
barycentric within 1e-4 of zero while t > -1e-3, lies inside the triangle with |t| < 1e-3, or has |det| < 1e-7 (fp32 may decide
such a pair otherwise); at most 5 % of a case's rays.  Sphere warp: |d - r| >= 4e-6 over all pairs (the figure of the vertex-warp
tests), no case left out; the argmin is compared where the two smallest distances are 4e-6 apart, at most 5 % of the samples left
out of the index comparison only.

Measured on an MI355X (profiles/vertex_sphere_errors.txt has every figure): the hit lists' E kernel equals E fp32 CPU in every case
(7e-8 .. 3.8e-7, ratio 1.00: the kernel's arithmetic is the restatement's, operation for operation), 0 .. 5 rays of a case left out;
the mean-mode warp 3.0e-8 .. 1.8e-7 at 1.00 .. 1.16 x; the pipeline against g19 rgb 1.8e-7, warped 0, densities 1.8e-5; the losses of
three Adam steps 1.5e-6 against 1.0e-6 (1.45 x)."""
import functools

import numpy as np
import pytest
import torch

import vertex_sphere_ref as SR
from conftest import load_golden

pytestmark = pytest.mark.gpu
FACTOR = 8.0
INF = float("inf")

# meshes by face count (cam: where the rays start): one triangle, the bumpy ellipsoid at levels 0 .. 3, and - near real size - SMPL's
# face count as a soup of small triangles none of which the camera sees edge-on (vertex_sphere_ref.triangle_soup says why)
MESHES = {1: lambda cam: SR.one_triangle(5), 20: lambda cam: SR.body_mesh(0, 5), 80: lambda cam: SR.body_mesh(1, 5),
          320: lambda cam: SR.body_mesh(2, 5), 1280: lambda cam: SR.body_mesh(3, 5), 13776: lambda cam: SR.triangle_soup(13776, 5, cam)}
# the kernel's edges: 64-ray chunks (63 / 65 / 130 = three chunks); 8 face slices walked four faces per wait (F = 1: one slice; 20:
# slices of 3, tail loop only; 80: slices of 10, both loops; 320 / 1280: whole fours); list capacities 1 / 4 / 8 / 16 (K on either side)
RAY_CASES = [(R, F, K) for R in (1, 63, 65, 130) for F in (1, 20, 320, 1280) for K in (1, 3, 16)] + \
            [(65, 80, K) for K in (1, 4, 5, 8, 9)] + [(65, 13776, 16)]
RAY_SEEDS = {(1, 1): 3}          # (R, F) -> the seed of its rays where seed 1 does not keep to the margins' cap or its one ray hits nothing


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def ray_case(R, F, scale=1.0, away=False):
    """Inputs and both restatements of one (R, F), computed once and shared by the K's: dict of numpy arrays."""
    seed = RAY_SEEDS.get((R, F), 1)
    v, f = MESHES[F](SR.camera_position(seed))
    o, d = SR.camera_rays(R, v, seed, away=away)
    d = (d * np.float32(scale)).astype(np.float32)
    c = {"o": o, "d": d, "v": v, "f": f, "ambiguous": SR.ambiguous_rays(o, d, v, f)}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        args = [torch.from_numpy(a).to(dt) for a in (o, d, v)]
        c["t" + name], c["n" + name] = SR.ray_mesh_hits(*args, f, 16)
    return c


def run_hits(dev, c, K, **kw):
    from smpl_nerf_amd import ops
    t, n = ops.ray_mesh_hits(*(torch.from_numpy(c[k]).to(dev) for k in ("o", "d", "v", "f")), max_hits=K, **kw)
    assert t.dtype == torch.float32 and n.dtype == torch.int32 and tuple(t.shape) == (len(c["o"]), K) and tuple(n.shape) == (len(c["o"]),)
    return N(t), N(n)


def hold_hits(tag, c, K, t, n, min_hit_share=0.1):
    keep = ~c["ambiguous"]
    left_out = int(c["ambiguous"].sum())
    t64, t32, n64 = c["t64"][:, :K], c["t32"][:, :K], c["n64"]
    share = float((n64 > 0).mean())
    print(f"{tag}: rays that hit {share:.2f}, most hits on a ray {int(n64.max())}, left out {left_out} of {len(keep)}")
    assert left_out <= 0.05 * len(keep), f"{tag}: {left_out} of {len(keep)} rays sit on an edge: choose another seed"
    assert share >= min_hit_share, f"{tag}: only {share:.2f} of the rays hit"
    assert np.array_equal(n[keep], n64[keep]), f"{tag}: hit counts differ on rays {np.nonzero(keep & (n != n64))[0][:8]}"
    assert np.array_equal(np.isinf(t[keep]), np.isinf(t64[keep])) and (t[np.isinf(t)] > 0).all(), f"{tag}: padding"
    assert np.array_equal(np.isinf(t64[keep]), np.arange(K)[None, :] >= n64[keep][:, None])
    fin = keep[:, None] & np.isfinite(t64)
    if fin.any():
        ek, ec = SR.relative_error(t[fin], t64[fin]), SR.relative_error(t32[fin], t64[fin])
        print(f"{tag}: E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  ratio {ek / ec if ec else 0.0:.2f}")
        assert ek <= FACTOR * ec, f"{tag}: E kernel {ek:.3e} > {FACTOR} x E fp32 CPU {ec:.3e}"
    assert (t[:, 1:] >= t[:, :-1]).all(), f"{tag}: the list is not ascending"


# ---------------------------------------------------------------------------------------------- ray-mesh hits
def test_the_cases_reach_deep_rays_and_cut_lists():
    """Over the whole set (float64, which the kernel's counts must equal): some ray crosses the surface four times or more, and
    some count exceeds its K."""
    most = max(int(ray_case(R, F)["n64"][~ray_case(R, F)["ambiguous"]].max()) for R, F, _ in RAY_CASES)
    cut = any((ray_case(R, F)["n64"][~ray_case(R, F)["ambiguous"]] > K).any() for R, F, K in RAY_CASES)
    print(f"most hits on one ray over the set: {most}; some list cut: {cut}")
    assert most >= 4 and cut


@pytest.mark.parametrize("R,F,K", RAY_CASES)
def test_ray_mesh_hits(dev, R, F, K):
    c = ray_case(R, F)
    assert c["ambiguous"].sum() <= 0.05 * R                         # (before the kernel runs)
    t, n = run_hits(dev, c, K)
    hold_hits(f"hits R={R} F={F} K={K}", c, K, t, n)


def test_rays_aimed_away_hit_nothing(dev):
    c = ray_case(130, 320, away=True)
    assert (c["n64"] == 0).all() and not c["ambiguous"].any()
    t, n = run_hits(dev, c, 3)
    assert (n == 0).all() and np.array_equal(t, np.full((130, 3), INF, np.float32))


def test_directions_need_not_be_normalised(dev):
    """t is in units of |d|: with d scaled by 2.5 every hit parameter shrinks by 2.5, under the same rule and the same bound."""
    c, c1 = ray_case(65, 320, scale=2.5), ray_case(65, 320)
    t, n = run_hits(dev, c, 3)
    hold_hits("hits, directions x 2.5", c, 3, t, n)
    both = ~(c["ambiguous"] | c1["ambiguous"])
    assert np.array_equal(c["n64"][both], c1["n64"][both])
    fin = both[:, None] & np.isfinite(c1["t64"][:, :3])
    assert np.abs(c["t64"][:, :3][fin] * 2.5 / c1["t64"][:, :3][fin] - 1).max() < 1e-6        # (the fp32 inputs differ by a rounding of d)


def test_two_hit_runs_are_bit_identical_and_the_check_can_be_skipped(dev):
    c = ray_case(130, 1280)
    a, b = run_hits(dev, c, 16), run_hits(dev, c, 16, faces_checked=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    from smpl_nerf_amd import ops
    bad = c["f"].copy()
    bad[7, 2] = len(c["v"])
    with pytest.raises(RuntimeError, match="outside"):
        ops.ray_mesh_hits(*(torch.from_numpy(x).to(dev) for x in (c["o"], c["d"], c["v"], bad)))


def test_hits_write_nothing_but_their_outputs(dev):
    """The C entry on outputs and a workspace cut out of larger buffers: the canaries around them stay, every element between
    them is written."""
    from smpl_nerf_amd import _lib
    lib = _lib.load()
    c, K, pad = ray_case(65, 80), 5, 64
    R, F = 65, 80
    o, d, v, f = (torch.from_numpy(c[k]).to(dev) for k in ("o", "d", "v", "f"))
    tbuf = torch.full((pad + R * K + pad,), -7.0, device=dev)
    nbuf = torch.full((pad + R + pad,), -7, device=dev, dtype=torch.int32)
    nbytes = lib.snerf_ray_mesh_workspace_bytes(F)
    wbuf = torch.full((pad + nbytes // 4 + pad,), -7.0, device=dev)
    rc = lib.snerf_ray_mesh_hits_f32(o.data_ptr(), d.data_ptr(), v.data_ptr(), f.data_ptr(), R, len(c["v"]), F, K,
                                     tbuf[pad:].data_ptr(), nbuf[pad:].data_ptr(), wbuf[pad:].data_ptr(), nbytes, _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    for buf, n in ((tbuf, R * K), (nbuf, R), (wbuf, nbytes // 4)):
        assert (buf[:pad] == -7).all() and (buf[pad + n:] == -7).all()
    t, n = N(tbuf[pad:pad + R * K]).reshape(R, K), N(nbuf[pad:pad + R])
    assert (n >= 0).all() and not (t == -7).any()
    hold_hits("hits into cut-out buffers", c, K, t, n)


# ---------------------------------------------------------------------------------------------- the sphere warp
WARP_SHAPES = [(1, 1), (7, 63), (64, 65), (65, 1000), (192, 6890)]
WARP_SEEDS = {(192, 6890, 0.05): 2}         # (n, V, radius) -> the seed where seed 1 puts a pair within 4e-6 of the sphere
WARP_REGIMES = [0.01, 0.05]       # the default (a vertex in the sphere is rare: samples are planted), many vertices per sphere


@functools.lru_cache(maxsize=None)
def warp_case(n, V, radius, seed=None, shift=0.0, plant=None):
    """Inputs, margins and both restatements in both modes, computed once; plant: the radius the planted samples are made for."""
    seed = WARP_SEEDS.get((n, V, radius), 1) if seed is None else seed
    samples, goal, canon = SR.warp_inputs(n, V, plant or radius, seed)
    samples = (samples + np.float32(shift)).astype(np.float32)
    near, gap = SR.warp_margins(samples, goal, radius)
    c = {"samples": samples, "goal": goal, "canon": canon, "near": near, "gap": gap}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        for mean in (False, True):
            w, i, k = SR.sphere_warp(*(torch.from_numpy(a).to(dt) for a in (samples, goal, canon)), radius, mean)
            c[f"warp{name}{int(mean)}"], c[f"nearest{name}"], c[f"count{name}{int(mean)}"] = w.numpy(), i.numpy(), k.numpy()
    return c


def run_warp(dev, c, radius, by_mean):
    from smpl_nerf_amd import ops
    p, g, k = (torch.from_numpy(c[x]).to(dev).requires_grad_(x != "samples") for x in ("samples", "goal", "canon"))
    warp, nearest, count = ops.vertex_sphere_warp(p, g, k, radius, by_mean=by_mean, want_indices=True)
    assert warp.grad_fn is None and not warp.requires_grad and warp.shape == p.shape and warp.dtype == torch.float32
    assert nearest.dtype == count.dtype == torch.int32 and nearest.shape == count.shape == p.shape[:-1]
    alone = ops.vertex_sphere_warp(p, g, k, radius, by_mean=by_mean)
    assert torch.equal(alone, warp)                                  # (the indices are optional outputs of the same launch)
    return N(warp), N(nearest), N(count)


def hold_warp(tag, c, radius, by_mean, got):
    warp, nearest, count = got
    m = int(by_mean)
    assert c["near"] >= 4e-6, f"{tag}: a pair sits on the sphere: |d - r| {c['near']:.2e}"
    sure = c["gap"] >= 4e-6
    print(f"{tag}: min |d - r| {c['near']:.2e}; samples with a vertex inside {int((c['count64' + str(m)] > 0).sum())} of {len(sure)}; "
          f"left out of the index comparison {int((~sure).sum())}")
    assert (~sure).sum() <= 0.05 * len(sure)
    assert np.array_equal(count, c[f"count64{m}"]), f"{tag}: counts"
    assert np.array_equal(nearest[sure], c["nearest64"][sure]), f"{tag}: nearest vertex"
    assert np.isfinite(warp).all()
    if by_mean:
        y64, y32 = c["warp641"], c["warp321"]
        ek, ec = SR.relative_error(warp, y64), SR.relative_error(y32, y64)
        print(f"{tag}: E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  ratio {ek / ec if ec else 0.0:.2f}  max|y64| {np.abs(y64).max():.3e}")
        assert ek <= FACTOR * ec, f"{tag}: E kernel {ek:.3e} > {FACTOR} x E fp32 CPU {ec:.3e}"
        assert np.array_equal(warp[count == 0], np.zeros_like(warp[count == 0]))
    else:
        full = c["canon"][nearest] - c["goal"][nearest]                     # fp32, the kernel's own index (exact where sure)
        want = np.where((count > 0)[:, None], full, np.zeros_like(full))
        assert np.array_equal(warp, want), f"{tag}: the warp is neither canon_i - goal_i nor zero"


@pytest.mark.parametrize("by_mean", [False, True])
@pytest.mark.parametrize("radius", WARP_REGIMES)
@pytest.mark.parametrize("n,V", WARP_SHAPES)
def test_sphere_warp(dev, n, V, radius, by_mean):
    """Sizes around the 64-sample chunk and the 16 vertex slices walked four per wait (V = 1: one slice; 63: slices of 4, the last
    short; 65: slices of 5, both loops; 1000, 6890)."""
    c = warp_case(n, V, radius)
    if V > 1:
        assert (c["count641"] > 0).any(), "no vertex is in any sphere: the case would test nothing"
    if radius == 0.05 and V >= 1000:
        assert c["count641"].max() >= 3                                    # many vertices per sphere
    hold_warp(f"warp n={n} V={V} r={radius} mean={int(by_mean)}", c, radius, by_mean, run_warp(dev, c, radius, by_mean))


@pytest.mark.parametrize("by_mean", [False, True])
def test_no_vertex_in_any_sphere(dev, by_mean):
    c = warp_case(70, 130, 0.01, seed=2, shift=5.0)                         # the body lives within ~1.5 of the origin
    assert c["near"] > 1.0
    warp, nearest, count = run_warp(dev, c, 0.01, by_mean)
    assert np.array_equal(warp, np.zeros_like(warp)) and (count == 0).all()
    assert np.array_equal(nearest[c["gap"] >= 4e-6], c["nearest64"][c["gap"] >= 4e-6])


def test_every_vertex_in_the_sphere(dev):
    c = warp_case(33, 150, 10.0, seed=3, plant=0.01)              # (bodies and samples span ~2.5)
    assert c["near"] > 5.0 and (c["count641"] == 150).all()
    hold_warp("warp, all in the sphere, mean", c, 10.0, True, run_warp(dev, c, 10.0, True))
    hold_warp("warp, all in the sphere, nearest", c, 10.0, False, run_warp(dev, c, 10.0, False))


@pytest.mark.parametrize("by_mean", [False, True])
def test_two_warp_runs_are_bit_identical(dev, by_mean):
    c = warp_case(192, 6890, 0.05)
    a, b = run_warp(dev, c, 0.05, by_mean), run_warp(dev, c, 0.05, by_mean)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_warp_keeps_the_leading_shape(dev):
    from smpl_nerf_amd import ops
    c = warp_case(192, 6890, 0.05)
    p, g, k = (torch.from_numpy(c[x]).to(dev) for x in ("samples", "goal", "canon"))
    flat = ops.vertex_sphere_warp(p, g, k, 0.05)
    w, i, n = ops.vertex_sphere_warp(p.view(3, 64, 3), g, k, 0.05, want_indices=True)
    assert tuple(w.shape) == (3, 64, 3) and tuple(i.shape) == tuple(n.shape) == (3, 64) and torch.equal(w.view(-1, 3), flat)


# ---------------------------------------------------------------------------------------------- VertexSpherePipeline
@pytest.fixture(scope="module")
def g19():
    return load_golden("g19_vertex_sphere.npz"), SR.g19_inputs()


def _pipeline(dev, params, **args):
    from smpl_nerf_amd.nets import RenderRayNet
    from smpl_nerf_amd.ops import PositionalEncoder
    from smpl_nerf_amd.pipelines import PipelineArgs, VertexSpherePipeline
    net = RenderRayNet(8, 256, 60, 24, skips=[4])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net = net.to(dev).train()
    return VertexSpherePipeline(net, net, PipelineArgs(run_fine=0, **args), PositionalEncoder(10, 0), PositionalEncoder(4, 0)), net


def test_pipeline_against_the_reference(dev, g19):
    """Forward against what the reference rendered on the CPU, at the tolerances DynamicPipeline's outputs are held to."""
    g, (batch_np, params) = g19
    pipe, _ = _pipeline(dev, params)
    batch = [torch.from_numpy(a).to(dev) for a in batch_np]
    with torch.no_grad():
        out = pipe(batch)
    assert out[0] is out[1] and out[2] is batch[4] and out[3] is batch[0]
    assert [tuple(o.shape) for o in out] == [(12, 3), (12, 3), (12, 64, 3), (12, 64, 3), (12, 64, 3), (12, 64)]
    for i, name, tol in ((0, "rgb", 1e-5), (4, "warped", 2e-6), (5, "densities", 5e-5)):
        err = float(np.abs(N(out[i]).astype(np.float64) - g[name]).max())
        print(f"pipeline {name}: max abs error against the reference {err:.3e} (tolerance {tol})")
        assert err <= tol, (name, err)
    loss = torch.nn.functional.mse_loss(out[0], batch[5]).item()
    print(f"pipeline loss {loss:.8f} (reference {g['loss'][0]:.8f})")
    assert abs(loss - g["loss"][0]) <= 1e-5


def test_three_adam_steps(dev, g19):
    """The NeRF trained in canonical space under the trainer (autograd path, the library's Adam): the loss of three steps against
    the same three steps of the restated pipeline in float64."""
    from smpl_nerf_amd.trainer import DataParallelTrainer, HipAdam
    _, (batch_np, params) = g19
    lr = 2e-5          # (at the reference's 5e-4 one Adam step empties this synthetic scene, as in tests/test_gpu_vertex_warp.py)
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
            loss = 2 * torch.nn.functional.mse_loss(SR.vertex_sphere_pipeline(P, b)[0], b[5])      # rgb is rgb_fine: nerf_solver.py:48-52
            loss.backward()
            opt.step()
            traj.append(loss.item())
        ys.append(np.array(traj))
    ek, ec = SR.relative_error(got, ys[0]), SR.relative_error(ys[1], ys[0])
    print(f"three Adam steps: losses {got}; E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  ratio {ek / ec if ec else 0.0:.2f}")
    assert got[2] < got[0], "three steps did not lower the loss"
    assert ek <= FACTOR * ec


def test_one_step_with_the_mixture_term(dev, g19):
    """SmplNerfTrainer reads warped samples and densities at out[4] / out[5] of this pipeline's tuple too: --use_gmm_loss 1 runs."""
    from smpl_nerf_amd.trainer import SmplNerfTrainer
    _, (batch_np, params) = g19
    pipe, net = _pipeline(dev, params, use_gmm_loss=1, restrict_gmm_loss=0)
    means = np.random.default_rng(5).normal(0, 0.3, (200, 3)).astype(np.float32)
    tr = SmplNerfTrainer(pipe, [net], means, lr=2e-5)
    before = net.positions_pose_input.weight.detach().clone()
    loss = tr.step([torch.from_numpy(a).to(dev) for a in batch_np])
    colour, term = tr.last_terms
    print(f"one step with the mixture term: loss {loss.item():.6f} = colours {colour.item():.6f} + term {term.item():.6f}")
    assert torch.isfinite(loss) and term is not None and term.item() > 0
    assert all(torch.isfinite(p).all() for p in net.parameters()) and not torch.equal(before, net.positions_pose_input.weight)


# ---------------------------------------------------------------------------------------------- VertexSphereRays
def _data_set(dev, seed, n_samples=64, **args):
    from smpl_nerf_amd import synthetic as syn
    from smpl_nerf_amd.body_model import SmplBodyModel
    from smpl_nerf_amd.pipelines import PipelineArgs
    from smpl_nerf_amd.synthetic_smpl import surface_smpl_arrays
    from smpl_nerf_amd.vertex_sphere import VertexSphereRays
    body = SmplBodyModel.from_arrays(**surface_smpl_arrays(11, level=2)).to(dev)
    h = w = 16
    images = (np.stack([syn.procedural_image(h, w, 0.0, t) for t in (0.0, 40.0)]) * 255).astype(np.uint8)
    transforms = np.stack([syn.sphere_pose(0.0, t, 2.4) for t in (0.0, 40.0)])
    poses = syn.human_poses((41, 38), 0, 60, 2)
    a = PipelineArgs(near=1.0, far=4.0, number_coarse_samples=n_samples, vertex_sphere_radius=0.08, **args)
    gen = torch.Generator(device=dev).manual_seed(seed)
    return VertexSphereRays(images, transforms, 0.6, poses, np.zeros((1, 10), np.float32), body, a, dev, gen), body, poses, a, images


def test_data_set_shapes_rays_and_warps(dev):
    from smpl_nerf_amd import ops
    ds, body, poses, args, images = _data_set(dev, 3)
    assert len(ds) == 512
    item = ds[300]
    assert [tuple(t.shape) for t in item] == [(64, 3), (3,), (3,), (64,), (64, 3), (3,)] and all(t.dtype == torch.float32 for t in item)
    assert np.array_equal(N(item[5]), images.reshape(-1, 3)[300].astype(np.float32) / np.float32(255))
    norm = torch.linalg.vector_norm(ds.rays_direction.double(), dim=-1)
    assert float((norm - 1).abs().max()) <= 2e-7                                   # |dir| = 1 to fp32
    assert torch.equal(ds.rays_samples, ds.rays_translation[:, None, :] + ds.rays_direction[:, None, :] * ds.all_z_vals[:, :, None])
    hit = ds.n_hits > 0
    print(f"data set: {int(hit.sum())} of 512 rays hit the body; samples moved {int((ds.all_warps.abs().amax(-1) > 0).sum())}")
    assert 20 <= int(hit.sum()) <= 400 and (ds.all_warps.abs().amax(-1) > 0).any()
    # neither sampling switch is set: every ray carries the one stratified table
    assert torch.equal(ds.all_z_vals, ds.z_vals_simple[None, :].expand(512, 64)) and float(ds.z_vals_simple[0]) >= 1.0
    assert float(ds.z_vals_simple[-1]) <= 4.0 and bool((ds.z_vals_simple[1:] > ds.z_vals_simple[:-1]).all())
    # the stored warps are the operator's, bit for bit, image by image
    betas = torch.zeros(1, 10, device=dev)
    for i in range(2):
        goal = body(betas=betas, body_pose=torch.from_numpy(poses[i:i + 1]).to(dev)).vertices[0]
        canon = body(betas=betas, body_pose=torch.zeros(1, 69, device=dev)).vertices[0]
        assert torch.equal(ds.canonical, canon)
        sl = slice(256 * i, 256 * (i + 1))
        assert torch.equal(ds.all_warps[sl], ops.vertex_sphere_warp(ds.rays_samples[sl], goal, canon, args.vertex_sphere_radius))
        t, n = ops.ray_mesh_hits(ds.rays_translation[sl], ds.rays_direction[sl], goal, body.faces, 1)
        assert torch.equal(t[:, 0], ds.first_hit[sl]) and torch.equal(n, ds.n_hits[sl])
    batches = list(ds.batches(200))
    assert [len(b[0]) for b in batches] == [200, 200, 112] and all(len(b) == 6 and all(t.is_cuda for t in b) for b in batches)
    assert torch.equal(torch.cat([b[4] for b in batches]), ds.all_warps)
    shuffled = list(ds.batches(512, shuffle=True))[0]             # one batch: a permutation of the rays
    key, all_keys = shuffled[0][:, 0, 1], ds.rays_samples[:, 0, 1]
    assert not torch.equal(key, all_keys) and torch.equal(torch.sort(key)[0], torch.sort(all_keys)[0])


def test_data_set_one_sample_per_ray(dev):
    ds = _data_set(dev, 3, n_samples=1)[0]
    hit = ds.n_hits > 0
    assert tuple(ds.all_z_vals.shape) == (512, 1) and tuple(ds.rays_samples.shape) == (512, 1, 3) and hit.any() and (~hit).any()
    assert torch.equal(ds.all_z_vals[hit, 0], ds.first_hit[hit]) and (ds.all_z_vals[~hit, 0] == 4.0).all()
    assert torch.isinf(ds.first_hit[~hit]).all() and torch.isfinite(ds.first_hit[hit]).all()


def test_data_set_samples_around_the_first_hit(dev):
    ds = _data_set(dev, 3, coarse_samples_from_intersect=1)[0]
    hit = ds.n_hits > 0
    z = ds.all_z_vals
    assert bool((z[:, 1:] >= z[:, :-1]).all())                                     # sorted, hit or miss
    off = (z[hit].double().mean(1) - ds.first_hit[hit].double()).abs().max().item()
    print(f"samples from the first hit: max |mean(z) - first hit| {off:.4f} over {int(hit.sum())} rays (bound 0.02 = 5 sigma / sqrt(64) at sigma 0.03)")
    assert off <= 0.02
    assert torch.equal(z[~hit], ds.z_vals_simple[None, :].expand(int((~hit).sum()), 64))      # miss rays: the shared table
    assert float(z[hit].std(dim=1).min()) > 0.01                                   # draws, not copies of the mean


def test_data_set_samples_from_the_prior(dev):
    from smpl_nerf_amd import ops
    ds, body, poses, args, _ = _data_set(dev, 3, coarse_samples_from_prior=1)
    hit = ds.n_hits > 0
    z = ds.all_z_vals
    assert torch.equal(z[~hit], ds.z_vals_simple[None, :].expand(int((~hit).sum()), 64))
    assert not bool((z[hit][:, 1:] >= z[hit][:, :-1]).all())                       # unsorted, as in the reference
    # every draw lies within 6 sigma of one of its ray's hits, and a ray with two hits far apart draws around both
    both = 0
    for i in range(2):
        sl = slice(256 * i, 256 * (i + 1))
        goal = body(betas=torch.zeros(1, 10, device=dev), body_pose=torch.from_numpy(poses[i:i + 1]).to(dev)).vertices[0]
        t, n = ops.ray_mesh_hits(ds.rays_translation[sl], ds.rays_direction[sl], goal, body.faces, 16)
        assert torch.equal(n, ds.n_hits[sl])
        h = n > 0
        away = (z[sl][h][:, :, None] - t[h][:, None, :]).abs().amin(-1)            # [hit rays, 64]: distance to the nearest hit
        assert float(away.max()) <= 6 * args.std_dev_coarse_sample_prior
        two = (n == 2) & (t[:, 1] - t[:, 0] > 0.3)
        near_first = (z[sl][two] - t[two][:, :1]).abs() < 0.15
        both += int((near_first.any(1) & (~near_first).any(1)).sum())
    print(f"samples from the prior: rays with draws around both of two hits: {both}")
    assert both > 0


def test_the_same_seed_gives_the_same_data_set(dev):
    a, b, c = (_data_set(dev, s, coarse_samples_from_intersect=1)[0] for s in (3, 3, 4))
    for name in ("rays_samples", "all_z_vals", "all_warps", "rays_direction", "z_vals_simple"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(a.all_z_vals, c.all_z_vals)
