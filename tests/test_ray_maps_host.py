"""The ray maps without a GPU: the float64 restatement (tests/ray_maps_ref.py) against the reference's own depth_map / acc_map
(g29_ray_maps.npz), the analytic backward the kernel evaluates against autograd, and what the two C entries refuse on the host
(include/smplnerf.h "ray maps").  Nothing is launched."""
import numpy as np
import pytest
import torch

import ray_maps_ref as RR
from smpl_nerf_amd import _lib, build

SHAPES = ((1, 1), (3, 2), (2, 63), (2, 64), (3, 65), (2, 192), (2, 1030))


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("B,N", RR.GOLDEN_SHAPES)
def test_float64_restatement_equals_the_reference(golden, B, N):
    """On the reference's float64 density and its z: acc and depth of the restatement are the reference's acc_map and depth_map
    (its own expressions on its own weights) to 1e-12; so are the weights the restatement rebuilds from the density."""
    g = golden("g29_ray_maps.npz")
    k = f"{B}x{N}"
    alpha, z = torch.from_numpy(g[f"{k}/f64/density"]), torch.from_numpy(g[f"{k}/z"]).double()
    acc, depth, point = RR.ray_maps(alpha, None, None, z=z)
    assert point is None and acc.dtype == torch.float64
    for name, got in (("acc_map", acc), ("depth_map", depth)):
        err = float(np.abs(got.numpy() - g[f"{k}/f64/{name}"]).max())
        print(f"{k} {name}: max|restatement - reference| {err:.2e}")
        assert err <= 1e-12
    _, T = RR.transmittance(alpha)
    assert float(np.abs((alpha * T).numpy() - g[f"{k}/f64/weights"]).max()) <= 1e-12
    # the alpha the restatement of utils.py:161-175 gives is the reference's density
    a = RR.raw2alpha(torch.from_numpy(g[f"{k}/raw"]).double(), z, torch.from_numpy(g[f"{k}/dirs"]).double())
    assert float(np.abs(a.numpy() - g[f"{k}/f64/density"]).max()) <= 1e-12


def _bwd_cases():
    for B, N in SHAPES:
        yield f"{B}x{N}", RR.make_case(B, N, 5)
    for N in (2, 65, 192):
        yield f"edge{N}", RR.make_edge_case(N)          # alpha = 1 at the first sample, in the middle, everywhere; ...


@pytest.mark.parametrize("mode", ("z", "pts"))
def test_analytic_backward_equals_autograd(mode):
    """d alpha_k = T_k G_k - S_k / u_k with the shifted suffix sum, against autograd through the float64 restatement: 1e-12 of
    the largest gradient of the case, on every case - the rows with alpha = 1 (u = 1e-10) included."""
    for name, case in _bwd_cases():
        c = RR.cast(case, torch.float64)
        kw = dict(z=c["z"]) if mode == "z" else dict(pts=c["pts"])
        grads = dict(d_acc=c["d_acc"], d_depth=c["d_depth"], d_point=c["d_point"] if mode == "pts" else None)
        _, want = RR.ray_maps_autograd(c["alpha"], c["o"], c["d"], **kw, **grads)
        got = RR.ray_maps_bwd(c["alpha"], c["o"], c["d"], **kw, **grads)
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        print(f"{name} {mode}: max|analytic - autograd| {err:.2e}, scale {scale:.2e}")
        assert torch.isfinite(got).all() and scale > 0
        assert err <= 1e-12 * scale, (name, mode, err, scale)


def test_restatement_edges():
    """What the rule says at its edges, in float64: alpha all 0 gives acc = depth = 0 and d alpha_k = G_k; N == 1 with alpha = 1
    gives acc = 1 and depth = t_0; a ray of d = 0 has t = 0."""
    c = RR.cast(RR.make_edge_case(65), torch.float64)
    (acc, depth, point), da = RR.ray_maps_autograd(c["alpha"], c["o"], c["d"], pts=c["pts"], d_acc=c["d_acc"], d_depth=c["d_depth"],
                                                   d_point=c["d_point"])
    assert acc[0] == 0 and depth[0] == 0 and (point[0] == 0).all()
    t = RR.sample_parameter(c["o"], c["d"], c["pts"])
    G = c["d_acc"][:, None] + c["d_depth"][:, None] * t + (c["d_point"][:, None, :] * c["pts"]).sum(-1)
    # (float64 keeps the 1e-10 that fl32(1 + 1e-10f) = 1 drops: T_k = (1 + 1e-10)^k, at most 1 + 65e-10 here)
    assert float((da[0] - G[0]).abs().max()) <= 66e-10 * float(G[0].abs().max())
    c32 = RR.cast(c, torch.float32)
    da32 = RR.ray_maps_bwd(c32["alpha"], c32["o"], c32["d"], z=c32["z"], d_acc=c32["d_acc"], d_depth=c32["d_depth"])
    assert torch.equal(da32[0], c32["d_acc"][0] + c32["d_depth"][0] * c32["z"][0])      # in fp32, as the kernel has it: T = 1, S = 0
    assert (t[5] == 0).all() and depth[5] == 0
    assert float((t[:5] - c["z"][:5]).abs().max()) <= 1e-6           # pts = o + z d in fp32
    one = RR.cast(RR.make_case(3, 1, 9), torch.float64)
    acc, depth, _ = RR.ray_maps(torch.ones_like(one["alpha"]), one["o"], one["d"], z=one["z"])
    assert (acc == 1).all() and torch.equal(depth, one["z"][:, 0])


def test_entries_exist(lib):
    assert hasattr(lib, "snerf_ray_maps_fwd_f32") and hasattr(lib, "snerf_ray_maps_bwd_f32")
    assert lib.snerf_version() == 109          # added without a version bump: a C host looks them up


P = 64      # a fake address: every call below is refused, or empty, before anything is read


def _fwd(lib, z=P, pts=None, B=4, N=8, point=None):
    rc = lib.snerf_ray_maps_fwd_f32(P, z, pts, P, P, B, N, P, P, point, None)
    return rc, lib.snerf_last_error_string()


def _bwd(lib, z=P, pts=None, B=4, N=8, d_point=None):
    rc = lib.snerf_ray_maps_bwd_f32(P, z, pts, P, P, B, N, P, P, d_point, P, None)
    return rc, lib.snerf_last_error_string()


@pytest.mark.parametrize("call", (_fwd, _bwd), ids=("fwd", "bwd"))
def test_entries_refuse_on_the_host(lib, call):
    assert call(lib, B=0)[0] == 0                                           # B == 0 is a no-op
    assert call(lib, z=None, pts=P, B=0)[0] == 0
    for kw, text in ((dict(N=0), b"1 <= N <= 4096"), (dict(N=4097), b"1 <= N <= 4096"), (dict(B=-1), b"B >= 0"),
                     (dict(z=P, pts=P), b"exactly one of z and pts"), (dict(z=None, pts=None), b"exactly one of z and pts")):
        rc, err = call(lib, **kw)
        assert rc == -1 and text in err, (kw, rc, err)
    which = "point" if call is _fwd else "d_point"
    rc, err = call(lib, **{which: P})
    assert rc == -1 and b"needs pts" in err, (rc, err)


def test_null_pointers_are_refused(lib):
    assert lib.snerf_ray_maps_fwd_f32(None, P, None, P, P, 4, 8, P, P, None, None) == -1
    assert b"alpha is null" in lib.snerf_last_error_string()
    assert lib.snerf_ray_maps_fwd_f32(P, P, None, P, P, 4, 8, None, P, None, None) == -1
    assert lib.snerf_ray_maps_fwd_f32(P, None, P, None, P, 4, 8, P, P, None, None) == -1
    assert b"pts needs o and d" in lib.snerf_last_error_string()
    assert lib.snerf_ray_maps_bwd_f32(P, P, None, P, P, 4, 8, None, None, None, None, None) == -1
    assert b"d_alpha is null" in lib.snerf_last_error_string()


def test_depth_error():
    from smpl_nerf_amd import io as sio
    ref = np.array([[0., 2., np.inf], [4., 0., 1.]])
    got = np.array([[9., 2.5, 9.], [3., 9., 1.]])
    assert sio.depth_error(got, ref) == (0.5, 1.0)
    assert sio.depth_error(torch.from_numpy(got), torch.from_numpy(ref), mask=np.array([[1, 1, 1], [0, 1, 1]])) == (0.25, 0.5)
    assert all(np.isnan(v) for v in sio.depth_error(got, np.zeros_like(ref)))
    with pytest.raises(ValueError):
        sio.depth_error(got, ref[:1])
