"""CPU-side checks of the soft silhouette: the float64 restatement (tests/soft_silhouette_ref.py) differentiates as central
differences say, the conditions the GPU cases rest on hold for every case, the header states the rule, the corner table lists what
it must, and the entries and the operator refuse what they cannot run before anything touches a device.  No GPU needed."""
import numpy as np
import pytest
import torch

import soft_silhouette_ref as SR
from smpl_nerf_amd import _lib, build

F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("case", [(8, 8, 20, 1, 1, 1.0), (9, 13, 320, 3, 1, 0.25), (9, 13, 20, 3, 3, 4.0)])
def test_the_restatements_gradient_is_the_central_difference(case):
    H, W, F, N, bodies, sigma = case
    poses, focal, v, faces = SR.case_inputs(H, W, F, N, bodies)
    dS = SR.upstream(N, H, W).astype(np.float64)
    _, g = SR.with_gradient(poses, focal, H, W, v, faces, sigma, 17.0, dS, F64)

    def value(x):
        return float((SR.silhouette(poses, focal, H, W, torch.from_numpy(x), faces, sigma, 17.0, F64).numpy() * dS).sum())

    flat = np.argsort(-np.abs(g).reshape(-1))[:6]                                       # the six largest entries
    h, worst = 1e-6, 0.0
    for k in flat:
        step = np.zeros(g.size)
        step[k] = h
        x = v.astype(np.float64)
        numeric = (value(x + step.reshape(x.shape)) - value(x - step.reshape(x.shape))) / (2 * h)
        worst = max(worst, abs(numeric - g.reshape(-1)[k]) / np.abs(g).max())
    print(f"{case}: autograd against central differences, worst {worst:.3e} of max|g| = {np.abs(g).max():.3e}")
    assert np.abs(g).max() > 0 and worst < 1e-6


@pytest.mark.parametrize("H,W,F,N,bodies", sorted({c[:5] for c in SR.CASES}))
def test_inside_pairs_keep_their_nearest_segment(H, W, F, N, bodies):
    """Among the contributing inside pairs the two smallest segment distances differ by a relative 1e-4 at least, against fp32
    roundings of about 1e-6: the device and float64 take the same branch of the only kink the rule has."""
    poses, focal, v, faces = SR.case_inputs(H, W, F, N, bodies)
    gap = min(SR.inside_gap(poses, focal, H, W, v, faces, sigma) for sigma in SR.SIGMAS)
    print(f"{H}x{W} F={F} N={N} bodies={bodies}: smallest relative gap {gap:.3e}")
    assert gap >= 1e-4


def test_the_float64_fit_converges():
    h = SR.cpu_fit(F64)
    print(f"float64 fit: {h[0]:.5f} -> {h[-1]:.5f}, ratio {h[-1] / h[0]:.3f}")
    assert len(h) == 40 and h[-1] <= 0.25 * h[0]


def test_the_header_states_the_rule(lib):
    header = " ".join(open(_lib.HERE + "/../include/smplnerf.h").read().replace("*", " ").split())     # (comment lines joined)
    for name, nargs in (("snerf_soft_silhouette_workspace_bytes", 3), ("snerf_soft_silhouette_fwd_f32", 18), ("snerf_soft_silhouette_bwd_f32", 22)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and name + "(" in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for phrase in ("x = W 0.5 + focal c0 / depth", "y = H 0.5 - focal c1 / depth", "q = (i, j)", "all three depths > 0",
                   "t = ee > 0 ? min(max((wx ex + wy ey) / ee, 0), 1) : 0", "edge_k = ex wy - ey wx", "the lowest k on a tie",
                   "a zero-area face is never inside", "d2 > cutoff sigma", "z = (inside ? d2 : -d2) / sigma", "max(z, 0) + log1p(exp(-|z|))",
                   "silhouette = -expm1(-L)", "transmittance = exp(-L)", "dS_p T_p sigmoid(z_pf)", "SNERF_RENDER_NO_CULL) bit for bit",
                   "no atomics", "112 N F bytes"):
        assert phrase in header, phrase
    assert lib.snerf_version() == 109


def test_the_corner_table():
    from smpl_nerf_amd import ops
    from smpl_nerf_amd.synthetic_smpl import bumpy_ellipsoid
    _, f = bumpy_ellipsoid(2, 5)
    f = np.concatenate([f, [[4, 4, 7], [9, 3, 9]]]).astype(np.int32)                    # two faces that name a vertex twice
    V = int(f.max()) + 1
    off, vf, vc = ops.vertex_corner_table(f, V)
    off2, vf2 = ops.vertex_face_table(f, V)
    assert np.array_equal(off, off2) and np.array_equal(vf, vf2) and vc.dtype == np.int32 and len(vc) == 3 * len(f)
    seen = set()
    for v in range(V):
        rows = list(zip(vf[off[v]:off[v + 1]], vc[off[v]:off[v + 1]]))
        assert rows == sorted(rows) and all(f[face, corner] == v for face, corner in rows)
        seen.update(rows)
    assert len(seen) == 3 * len(f)                                                      # every corner once: distinct for a repeated vertex


def test_the_entries_validate_on_the_host(lib):
    N, one = None, 8        # any non-null "pointer": validation never dereferences
    fwd_names, bwd_names = "poses vertices faces silhouette transmittance".split(), "poses vertices faces d_silhouette transmittance vf_offsets vf_faces vf_corners d_vertices".split()
    ws_bytes = 112 * 2 * 4

    def fwd(n=2, H=9, W=13, Nv=1, V=9, F=4, focal=7.0, sigma=1.0, cutoff=17.0, flags=0, ws=one, nbytes=ws_bytes, **null):
        p = {k: (N if null.get(k) else one) for k in fwd_names}
        return lib.snerf_soft_silhouette_fwd_f32(p["poses"], focal, n, H, W, p["vertices"], Nv, V, p["faces"], F, sigma, cutoff, flags,
                                                 p["silhouette"], p["transmittance"], ws, nbytes, N)

    def bwd(n=2, H=9, W=13, Nv=1, V=9, F=4, focal=7.0, sigma=1.0, cutoff=17.0, flags=0, ws=one, nbytes=ws_bytes, **null):
        p = {k: (N if null.get(k) else one) for k in bwd_names}
        return lib.snerf_soft_silhouette_bwd_f32(p["poses"], focal, n, H, W, p["vertices"], Nv, V, p["faces"], F, sigma, cutoff, flags,
                                                 p["d_silhouette"], p["transmittance"], p["vf_offsets"], p["vf_faces"], p["vf_corners"],
                                                 p["d_vertices"], ws, nbytes, N)

    err = lib.snerf_last_error_string
    for call, names in ((fwd, fwd_names), (bwd, bwd_names)):
        assert call(n=0, ws=N, nbytes=0, **{k: True for k in names}) == 0                # N = 0: a no-op, also with null pointers
        assert call(n=0, Nv=5) == 0
        assert call(n=-1) == -1 and b"N" in err()
        for bad in ("H", "W"):
            assert call(**{bad: 0}) == -1 and b"at least 1" in err() and call(n=0, **{bad: 0}) == -1     # a bad scalar whatever N is
        for x in (0.0, -1.0, float("nan"), float("inf")):
            assert call(focal=x) == -1 and b"focal" in err()
            assert call(sigma=x) == -1 and b"sigma" in err() and call(n=0, sigma=x) == -1
        for x in (-1e-9, float("nan"), float("inf")):
            assert call(cutoff=x) == -1 and b"cutoff" in err()
        assert call(flags=2) == -1 and b"flags" in err()
        assert call(V=0) == -1 and b"V must" in err() and call(F=0) == -1 and b"F must" in err() and call(n=0, F=0) == -1
        assert call(F=(1 << 31) // 9 + 1) == -1 and b"below 2^31" in err()
        assert call(Nv=3) == -1 and b"Nv" in err() and call(Nv=0) == -1
        for k in names:
            assert call(**{k: True}) == -1 and b"null" in err(), k
        assert call(ws=N) == -1 and b"workspace" in err()
        assert call(ws=4) == -1 and b"workspace" in err()                                # misaligned
        assert call(nbytes=ws_bytes - 1) == -1 and b"workspace" in err()
        assert call(n=1 << 20, H=1 << 14, W=1 << 14) == -1 and b"2^31" in err()          # N x tiles
        assert call(n=65536, H=8, W=8, nbytes=1 << 40) == -1 and b"65536" in err()
    assert lib.snerf_soft_silhouette_workspace_bytes(3, 12, 20) == 112 * 3 * 20 and lib.snerf_soft_silhouette_workspace_bytes(0, 12, 20) == 0
    assert lib.snerf_soft_silhouette_workspace_bytes(1, 0, 20) == -1 and lib.snerf_soft_silhouette_workspace_bytes(1, 12, 0) == -1
    assert lib.snerf_soft_silhouette_workspace_bytes(-1, 12, 20) == -1


def test_the_operator_refuses_before_loading_the_library(monkeypatch):
    from smpl_nerf_amd import ops
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    poses, focal, v, f = SR.case_inputs(8, 8, 20, 1, 1)
    T = torch.from_numpy
    poses, v, f = T(poses), T(v), T(f)
    with pytest.raises(RuntimeError, match="soft_silhouette: `faces` must be int32"):
        ops.soft_silhouette(poses, focal, 8, 8, v, f.long())
    bad = f.clone()
    bad[3, 1] = len(v)
    with pytest.raises(RuntimeError, match="outside"):
        ops.soft_silhouette(poses, focal, 8, 8, v, bad)
    with pytest.raises(RuntimeError, match="float64"):
        ops.soft_silhouette(poses.float(), focal, 8, 8, v, f)
    with pytest.raises(RuntimeError, match="bodies"):
        ops.soft_silhouette(poses, focal, 8, 8, torch.stack([v, v]), f)
    with pytest.raises(RuntimeError, match="at least 1"):
        ops.soft_silhouette(poses, focal, 0, 8, v, f)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.soft_silhouette(poses, focal, 8, 8, v, f)
