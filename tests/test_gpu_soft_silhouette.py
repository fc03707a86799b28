"""The soft silhouette on the GPU (csrc/soft_silhouette.hip, ops.soft_silhouette) and the fit built on it (silhouette_fit.py).

The yardstick is the rule restated in torch on the CPU (tests/soft_silhouette_ref.py) in float64, with the vertex gradient from
autograd; E(y) = max|y - y64| / max|y64|, and the device may err by max(8 x E(fp32 CPU restatement), 2^-22) - the floor covers
pairs whose liveness flips at the cutoff, each worth at most 4.1e-8.  Every test prints its figures before it asserts (pytest -s;
profiles/soft_silhouette_errors.txt holds a run)."""
import numpy as np
import pytest
import torch

import mesh_render_ref as MR
import smpl_lbs_ref as LR
import soft_silhouette_ref as SR
from smpl_nerf_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
PAD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def run(dev, poses, focal, H, W, v, faces, sigma=1.0, cutoff=17.0, dS=None, cull=True):
    """ops.soft_silhouette and, with dS, its vertex gradient -> (S, d_vertices or None) fp32 numpy."""
    from smpl_nerf_amd import ops
    vt = torch.from_numpy(np.asarray(v, np.float32)).to(dev).requires_grad_(dS is not None)
    S = ops.soft_silhouette(torch.from_numpy(np.asarray(poses, np.float64)).to(dev), focal, H, W, vt,
                            torch.from_numpy(np.asarray(faces, np.int32)).to(dev), sigma=sigma, cutoff=cutoff, cull=cull)
    assert tuple(S.shape) == (len(poses), H, W) and S.dtype == torch.float32
    if dS is None:
        assert S.grad_fn is None
        return N(S), None
    S.backward(torch.from_numpy(dS).to(dev))
    assert vt.grad.shape == vt.shape
    return N(S), N(vt.grad)


class Entries:
    """The two C entries on outputs and a workspace cut out of larger buffers full of NaNs."""

    def __init__(self, dev, poses, focal, H, W, v, faces, sigma, cutoff, dS):
        from smpl_nerf_amd import _lib, ops
        self.lib, self._lib = _lib.load(), _lib
        v = np.asarray(v, np.float32)
        v = v[None] if v.ndim == 2 else v
        self.n, self.Nv, self.V, self.Fc, self.H, self.W = len(poses), v.shape[0], v.shape[1], len(faces), H, W
        self.focal, self.sigma, self.cutoff = focal, sigma, cutoff
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.poses, self.v, self.faces, self.dS = T(np.asarray(poses, np.float64)), T(v), T(np.asarray(faces, np.int32)), T(dS)
        self.table = [T(a) for a in ops.vertex_corner_table(faces, self.V)]
        self.nbytes = self.lib.snerf_soft_silhouette_workspace_bytes(self.n, self.V, self.Fc)
        assert self.nbytes == 112 * self.n * self.Fc
        self.sizes = dict(S=self.n * H * W, T=self.n * H * W, dv=v.size, ws=self.nbytes // 8)
        self.bufs = {k: torch.full((PAD + m + PAD,), float("nan"), device=dev, dtype=F32 if k in ("S", "dv") else F64) for k, m in self.sizes.items()}

    def p(self, k):
        return self.bufs[k][PAD:].data_ptr()

    def forward(self, flags=0):
        rc = self.lib.snerf_soft_silhouette_fwd_f32(self.poses.data_ptr(), self.focal, self.n, self.H, self.W, self.v.data_ptr(), self.Nv, self.V,
                                                    self.faces.data_ptr(), self.Fc, self.sigma, self.cutoff, flags, self.p("S"), self.p("T"),
                                                    self.p("ws"), self.nbytes, self._lib.current_stream())
        assert rc == 0, self.lib.snerf_last_error_string()

    def backward(self):
        off, vf, vc = self.table
        rc = self.lib.snerf_soft_silhouette_bwd_f32(self.poses.data_ptr(), self.focal, self.n, self.H, self.W, self.v.data_ptr(), self.Nv, self.V,
                                                    self.faces.data_ptr(), self.Fc, self.sigma, self.cutoff, 0, self.dS.data_ptr(), self.p("T"),
                                                    off.data_ptr(), vf.data_ptr(), vc.data_ptr(), self.p("dv"), self.p("ws"), self.nbytes,
                                                    self._lib.current_stream())
        assert rc == 0, self.lib.snerf_last_error_string()

    def out(self, k):
        return N(self.bufs[k][PAD:PAD + self.sizes[k]])

    def guards_intact(self):
        return all(bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[PAD + self.sizes[k]:]).all()) for k, b in self.bufs.items())


def hold_bound(tag, got_S, got_g, ref):
    (S64, g64), (S32, g32) = ref[F64], ref[F32]
    for name, got, y32, y64 in (("silhouette", got_S, S32, S64), ("d_vertices", got_g, g32, g64)):
        ek, ec = LR.relative_error(got, y64), LR.relative_error(y32, y64)
        print(f"{tag}: {name:10s} E device {ek:.3e}  E fp32 CPU {ec:.3e}  bound {SR.bound(ec):.3e}  max|y64| {np.abs(y64).max():.3e}")
        assert np.isfinite(got).all() and ek <= SR.bound(ec), f"{tag} {name}: E device {ek:.3e} > {SR.bound(ec):.3e}"


# ---------------------------------------------------------------------------------------------- the shapes
@pytest.mark.parametrize("H,W,F,frames,bodies,sigma", SR.CASES)
def test_a_shape(dev, H, W, F, frames, bodies, sigma):
    """Forward and backward against float64 at the bound; culled against brute force, two calls, and a graph replay of the C
    entries bit for bit; NaN guard bands around the outputs and the workspace intact, every element between them written."""
    tag = f"{H}x{W} F={F} N={frames} bodies={bodies} sigma={sigma}"
    poses, focal, v, faces = SR.case_inputs(H, W, F, frames, bodies)
    dS = SR.upstream(frames, H, W)
    S, g = run(dev, poses, focal, H, W, v, faces, sigma, dS=dS)
    hold_bound(tag, S, g, SR.reference(H, W, F, frames, bodies, sigma))
    for what, (S2, g2) in (("brute force", run(dev, poses, focal, H, W, v, faces, sigma, dS=dS, cull=False)),
                           ("a second call", run(dev, poses, focal, H, W, v, faces, sigma, dS=dS))):
        assert same_bits(S, S2) and same_bits(g, g2), f"{tag}: {what} differs"
    assert same_bits(S, run(dev, poses, focal, H, W, v, faces, sigma)[0])                      # no_grad: the same frames

    e = Entries(dev, poses, focal, H, W, v, faces, sigma, 17.0, dS)
    e.forward()
    e.backward()
    torch.cuda.synchronize()
    assert e.guards_intact(), f"{tag}: a guard band was written"
    assert same_bits(e.out("S").reshape(S.shape), S) and same_bits(e.out("dv").reshape(g.shape), g)
    assert not np.isnan(e.out("T")).any() and np.allclose(1.0 - e.out("T").reshape(S.shape), S, atol=1e-6)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e.forward()
        e.backward()
    for k in ("S", "T", "dv"):
        e.bufs[k][PAD:PAD + e.sizes[k]].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(e.out("S").reshape(S.shape), S) and same_bits(e.out("dv").reshape(g.shape), g), f"{tag}: the graph replay differs"
    assert e.guards_intact()


def test_the_brute_force_entry_writes_the_same_transmittance(dev):
    poses, focal, v, faces = SR.case_inputs(9, 13, 320, 3, 3)
    a, b = (Entries(dev, poses, focal, 9, 13, v, faces, 1.0, 17.0, SR.upstream(3, 9, 13)) for _ in range(2))
    a.forward(0)
    b.forward(1)
    torch.cuda.synchronize()
    assert np.array_equal(a.out("T").view(np.int64), b.out("T").view(np.int64)) and same_bits(a.out("S"), b.out("S"))


# ---------------------------------------------------------------------------------------------- the edges
def hold_custom(tag, dev, poses, v, faces, H, W, sigma=1.0, dS=None):
    poses, focal = np.asarray(poses, np.float64).reshape(-1, 4, 4), SR.focal_of(W)
    dS = SR.upstream(len(poses), H, W) if dS is None else dS
    S, g = run(dev, poses, focal, H, W, v, faces, sigma, dS=dS)
    S2, g2 = run(dev, poses, focal, H, W, v, faces, sigma, dS=dS, cull=False)
    assert same_bits(S, S2) and same_bits(g, g2), f"{tag}: brute force differs"
    ref = {dt: SR.with_gradient(poses, focal, H, W, v, faces, sigma, 17.0, dS, dt) for dt in (F64, F32)}
    hold_bound(tag, S, g, ref)
    return S, g


def test_a_camera_inside_the_mesh(dev):
    v, f = MR.mesh(320)
    S, _ = hold_custom("camera inside", dev, [syn.pose_matrix(x=0.02, y=0.1, z=-0.03, phi=20.0, theta=50.0)], v, f, 9, 13)
    assert (S >= 0.5 - 2.0 ** -16).all()                                     # a closed surface seen from inside covers every pixel


def test_faces_with_a_corner_behind_the_camera_contribute_nothing(dev):
    v = np.array([[-1.0, -1.2, -1.0], [1.1, -1.0, -1.0], [0.1, 0.6, 3.5]], np.float32)
    S, g = hold_custom("one corner behind", dev, [syn.pose_matrix(z=2.4)], v, [[0, 1, 2]], 32, 32)
    assert not S.any() and not g.any()
    # ... and beside live ones: the mesh across the camera plane
    v, f = MR.mesh(1280)
    pose = syn.pose_matrix(x=float(v[:, 0].max()) + 0.02, y=0.05, z=0.0, theta=0.0)
    depth = -((v.astype(np.float64) - pose[:3, 3]) @ pose[:3, :3])[:, 2]
    assert ((depth[f] > 0).any(1) & (depth[f] <= 0).any(1)).sum() >= 10
    S, g = hold_custom("faces across the camera plane", dev, [pose], v, f, 32, 32)
    assert S.max() > 0.5 and np.abs(g).max() > 0


def test_a_zero_area_face_and_a_zero_length_edge(dev):
    """Faces with a repeated vertex - a zero-length edge, and with it a zero area - beside a regular one: finite, and the
    restatement's at the bound.  Their two remaining segments coincide, and either names the same two vertices with the same
    shares, so the vertex gradient does not depend on which is taken.  Then a zero-area face of three distinct collinear vertices:
    its segments overlap without naming the same corners, which of them is the nearest is a tie that rounding decides in any
    arithmetic, float64 included, so only its silhouette is compared; its gradient must be finite."""
    v = np.array([[-0.4, -0.3, 0.0], [0.5, -0.2, 0.1], [0.05, 0.45, 0.0], [0.05, -0.25, 0.05]], np.float32)
    pose = [syn.sphere_pose(10.0, 25.0, 2.4)]
    S, g = hold_custom("zero-length edges", dev, pose, v, [[2, 2, 0], [1, 1, 1], [3, 0, 0], [0, 1, 2]], 32, 32)
    assert S.max() > 0.5 and np.abs(g).max() > 0
    v[3] = 0.5 * (v[0] + v[1])                                               # collinear with 0 and 1
    poses, focal = np.asarray(pose), SR.focal_of(32)
    dS = SR.upstream(1, 32, 32)
    S, g = run(dev, poses, focal, 32, 32, v, [[0, 1, 3]], dS=dS)
    S2, g2 = run(dev, poses, focal, 32, 32, v, [[0, 1, 3]], dS=dS, cull=False)
    S64, S32 = (SR.with_gradient(poses, focal, 32, 32, v, [[0, 1, 3]], 1.0, 17.0, dS, dt)[0] for dt in (F64, F32))
    ek, ec = LR.relative_error(S, S64), LR.relative_error(S32, S64)
    print(f"collinear face: silhouette E device {ek:.3e}  E fp32 CPU {ec:.3e}  max S {S.max():.4f}  max|gradient| {np.abs(g).max():.3e}")
    assert same_bits(S, S2) and same_bits(g, g2) and np.isfinite(g).all() and 0.3 < S.max() <= 0.5 and ek <= SR.bound(ec)


def test_a_vertex_exactly_on_a_pixel(dev):
    """The identity camera looks down -z; a vertex on its axis projects to (W/2, H/2), a sample point for even H and W."""
    v = np.array([[0.0, 0.0, -2.0], [0.9, 0.1, -2.0], [0.2, 0.8, -2.5]], np.float32)
    H = W = 16
    dS = np.zeros((1, H, W), np.float32)
    dS[0, H // 2, W // 2] = 1.0
    S, g = hold_custom("vertex on a pixel", dev, [np.eye(4)], v, [[0, 1, 2]], H, W, dS=dS)
    print(f"vertex on a pixel: S = {S[0, H // 2, W // 2]!r}, |gradient| = {np.abs(g).max():.3e}")
    assert abs(float(S[0, H // 2, W // 2]) - 0.5) <= 2.0 ** -23 and np.isfinite(g).all()
    assert not g.any()                                                       # d = 0: a zero distance gradient


def test_a_mesh_outside_every_box(dev):
    v, f = MR.mesh(320)
    pose = syn.sphere_pose(10.0, 25.0, 2.4)
    far = v + (pose[:3, :3] @ np.array([40.0, 0.0, 0.0])).astype(np.float32)   # 40 units along the camera's x: far off the frame
    S, g = hold_custom("outside every box", dev, [pose], far, f, 32, 32)
    assert not S.any() and not g.any()


def test_the_upstream_gradient(dev):
    poses, focal, v, faces = SR.case_inputs(32, 32, 320, 1, 1)
    _, g = run(dev, poses, focal, 32, 32, v, faces, dS=np.zeros((1, 32, 32), np.float32))
    assert not g.any()                                                       # dS = 0: exactly 0
    S = run(dev, poses, focal, 32, 32, v, faces)[0]
    j, i = np.unravel_index(np.argmin(np.abs(S[0] - 0.5)), S[0].shape)         # a pixel on the outline
    dS = np.zeros((1, 32, 32), np.float32)
    dS[0, j, i] = 1.5
    _, g = hold_custom("one pixel's gradient", dev, poses, v, faces, 32, 32, dS=dS)
    assert np.abs(g).max() > 0


# ---------------------------------------------------------------------------------------------- against the existing renderer
@pytest.mark.parametrize("sigma", SR.SIGMAS)
def test_a_hit_pixel_is_at_least_half_covered(dev, sigma):
    """Where ops.render_mesh reports a hit on a face in front of the camera, S >= 1/2 - 2^-16: a pixel inside a face has
    D >= 1/2, and where the two inside tests disagree d < 2^-10 px at coordinates below 2^9, so D >= 1/2 - 2^-22 / sigma."""
    from smpl_nerf_amd import ops
    s = MR.scene(32, 32, 1280, 3, 3)
    T = lambda a: torch.from_numpy(a).to(dev)
    focal = SR.focal_of(32)
    frames = ops.render_mesh(T(s["poses"]), focal, 32, 32, T(s["vertices"]), T(s["faces"]), T(s["uv"]), T(s["texture"]))
    S = run(dev, s["poses"], focal, 32, 32, s["vertices"], s["faces"], sigma)[0]
    face = N(frames.face)
    front = np.zeros(face.shape, bool)
    for n in range(3):
        depth = SR.project(torch.from_numpy(s["vertices"][n]).double(), s["poses"][n], focal, 32, 32)[1].numpy()
        live = (depth[s["faces"]] > 0).all(1)
        front[n] = (face[n] >= 0) & live[np.maximum(face[n], 0)]
    print(f"sigma={sigma}: {int(front.sum())} hit pixels, min S on them {S[front].min():.6f}, max S off them {S[~front].max():.6f}")
    assert front.sum() > 300 and (S[front] >= 0.5 - 2.0 ** -16).all()


# ---------------------------------------------------------------------------------------------- the chain and the fit
@pytest.fixture(scope="module")
def body(dev):
    from smpl_nerf_amd.body_model import SmplBodyModel
    return SmplBodyModel.from_arrays(**SR.fit_body()).to(dev)


def fitter(body, cameras=1, **kw):
    from smpl_nerf_amd.silhouette_fit import SilhouetteFitter
    return SilhouetteFitter(body, SR.fit_poses(cameras), SR.focal_of(SR.FIT["W"]), SR.FIT["H"], SR.FIT["W"], sigma=SR.FIT["sigma"], **kw)


def test_the_chain_from_the_pose_to_the_loss(dev, body):
    """d L1 / d body_pose through ops.smpl_lbs and ops.soft_silhouette against the float64 CPU chain, the fp32 CPU chain the yardstick."""
    from smpl_nerf_amd import ops
    J = body.num_joints
    pose = torch.from_numpy(0.5 * SR.fit_true_pose(J)).to(dev).requires_grad_(True)
    v = body(body_pose=pose).vertices[0]
    S = ops.soft_silhouette(torch.from_numpy(SR.fit_poses()).to(dev), SR.focal_of(32), 32, 32, v, body.faces)
    loss = (S - torch.from_numpy(SR.fit_target()).to(dev)).abs().mean()
    loss.backward()
    (l64, g64), (l32, g32) = SR.chain_gradient(F64), SR.chain_gradient(F32)
    ek, ec = LR.relative_error(N(pose.grad), g64), LR.relative_error(g32, g64)
    print(f"chain: loss device {float(loss):.8f} float64 {l64:.8f} fp32 CPU {l32:.8f}; d body_pose E device {ek:.3e}  E fp32 CPU {ec:.3e}  "
          f"bound {SR.bound(ec):.3e}  max|g64| {np.abs(g64).max():.3e}")
    assert ek <= SR.bound(ec)


def test_the_fit_recovers_a_pose(dev, body):
    h64 = SR.cpu_fit(F64)
    print(f"fit, float64 CPU: {h64[0]:.5f} -> {h64[-1]:.5f} (ratio {h64[-1] / h64[0]:.3f})")
    assert h64[-1] <= 0.25 * h64[0]
    target = torch.from_numpy(SR.fit_target()).to(dev)
    fitted, history = fitter(body).fit(target, iterations=SR.FIT["iterations"], lr=SR.FIT["lr"])
    print(f"fit, device: {history[0]:.5f} -> {history[-1]:.5f} (ratio {history[-1] / history[0]:.3f})")
    assert len(history) == 40 and tuple(fitted["body_pose"].shape) == (1, 3 * (body.num_joints - 1)) and fitted["body_pose"].abs().max() > 0
    assert history[-1] <= 0.5 * history[0]


def test_a_fit_through_three_cameras(dev, body):
    target = torch.from_numpy(SR.fit_target(3)).to(dev)
    _, history = fitter(body, 3, photo_loss="L2").fit(target, iterations=SR.FIT["iterations"], lr=SR.FIT["lr"])
    print(f"fit, three cameras, L2: {history[0]:.5f} -> {history[-1]:.5f}")
    assert np.isfinite(history).all() and history[-1] < history[0]


def test_a_fit_of_named_angles_only(dev, body):
    target = torch.from_numpy(SR.fit_target()).to(dev)
    index = [3, 4, 5, 30]
    fitted, history = fitter(body).fit(target, iterations=10, lr=SR.FIT["lr"], angle_indices=index)
    pose = N(fitted["body_pose"])[0]
    rest = np.delete(pose, index)
    print(f"fit, four angles: {history[0]:.5f} -> {history[-1]:.5f}, angles {pose[index]}")
    assert np.isfinite(history).all() and not rest.any() and pose[index].all()


def test_a_fit_with_the_priors_switched_on(dev, body):
    from smpl_nerf_amd.priors import MaxMixturePrior
    rng = np.random.default_rng(11)
    A = rng.standard_normal((6, 69, 69)) * 0.05
    prior = MaxMixturePrior.from_arrays(rng.standard_normal((6, 69)) * 0.2, A @ A.transpose(0, 2, 1) + 0.05 * np.eye(69), np.full(6, 1 / 6))
    target = torch.from_numpy(SR.fit_target()).to(dev)
    plain, with_priors = fitter(body), fitter(body, angle_prior_weight=0.1, pose_prior=prior, pose_prior_weight=0.05)
    grads = []
    for f in (plain, with_priors):
        pose = torch.zeros(1, 69, device=dev, requires_grad=True)
        f.loss(target, torch.zeros(1, 10, device=dev), pose).backward()
        grads.append(N(pose.grad))
    moved = np.abs(grads[1] - grads[0])
    print(f"priors: the gradient at zero moves by up to {moved.max():.3e}; on the angle prior's entries {moved[0, [52, 55, 9, 12]]}")
    assert (moved[0, [52, 55, 9, 12]] > 0).all() and (moved > 0).sum() > 60
    _, history = with_priors.fit(target, iterations=10, lr=SR.FIT["lr"])
    assert np.isfinite(history).all()


def test_a_sequence_starts_from_the_last_frame(dev, body):
    f = fitter(body)
    targets = [torch.from_numpy(SR.fit_target()).to(dev), torch.from_numpy(SR.fit_target()).to(dev).flip(-1).contiguous()]
    out = f.fit_sequence(targets, init_pose="last_frame", iterations=5, lr=SR.FIT["lr"])
    (first, _), (_, h2) = out
    with torch.no_grad():
        want = float(f.loss(targets[1], first["betas"], first["body_pose"], first["global_orient"]))
    zero = f.fit_sequence(targets, init_pose="zero", iterations=5, lr=SR.FIT["lr"])
    print(f"sequence: frame 2 starts at {h2[0]:.6f} (from frame 1's result: {want:.6f}; from zeros: {zero[1][1][0]:.6f})")
    assert h2[0] == want and zero[1][1][0] != want and zero[0][1] == out[0][1]
