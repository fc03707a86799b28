"""Torch (CPU) restatement of the vertex_sphere model's two operators and of its pipeline, used ONLY by tests and tools.

  * ray_mesh_pairs / ray_mesh_hits: brute-force two-sided Moeller-Trumbore over all [R, F] pairs, the rule of include/smplnerf.h
    (snerf_ray_mesh_hits_f32) operation for operation, in the dtype of its inputs;
  * sphere_warp: the two modes of datasets/vertex_sphere_dataset.py:128-159 with the equality quirk (a distance equal to the radius
    weighs as itself), in the dtype of its inputs.
Run in float64 they are the yardstick, run in fp32 the comparison.  Also here: the seeded input generators (bumpy icospheres, camera
rays aimed into the body's box, planted samples), the margins the GPU tests require of their inputs, the inputs of
tests/golden/g19_vertex_sphere.npz rebuilt from its seeds, and VertexSpherePipeline.forward in torch.
"""
import numpy as np
import torch

from vertex_warp_ref import relative_error  # noqa: F401  (E(y) = max|y - y64| / max|y64|: the measure of tests/test_gpu_vertex_warp.py)

F32 = np.float32


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(x, y):
    return torch.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                        x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


# ------------------------------------------------------------------------------------------------ ray-mesh hits
def ray_mesh_pairs(origins, dirs, vertices, faces):
    """(hit [R,F] bool, t, u, v, det [R,F]) of every ray-triangle pair, in the dtype of origins."""
    faces = torch.as_tensor(faces).long()
    a, b, c = (vertices[faces[:, k]] for k in range(3))
    e1, e2 = (b - a)[None], (c - a)[None]                     # [1,F,3]
    o, d = origins[:, None, :], dirs[:, None, :]              # [R,1,3]
    p = _cross(d, e2)
    det = _dot(e1, p)
    s = o - a[None]
    u = _dot(s, p) / det
    q = _cross(s, e1)
    v = _dot(d, q) / det
    t = _dot(e2, q) / det
    hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    return hit, t, u, v, det


def ray_mesh_hits(origins, dirs, vertices, faces, max_hits):
    """(t_hits [R,K]: the K smallest hit parameters ascending, +inf padded; n_hits [R] int32) as numpy arrays."""
    hit, t = ray_mesh_pairs(origins, dirs, vertices, faces)[:2]
    t = torch.where(hit, t, torch.full_like(t, float("inf")))
    K = int(max_hits)
    if t.shape[1] < K:
        t = torch.cat([t, torch.full((t.shape[0], K - t.shape[1]), float("inf"), dtype=t.dtype)], 1)
    return torch.sort(t, dim=1)[0][:, :K].numpy(), hit.sum(1).to(torch.int32).numpy()


def ambiguous_rays(origins, dirs, vertices, faces):
    """The rays whose hit list float32 arithmetic may decide otherwise, in float64: some face has its smallest barycentric
    (u, v or 1 - u - v) within 1e-4 of zero while t > -1e-3, or lies inside the triangle with |t| < 1e-3, or has |det| < 1e-7.
    bool [R] numpy."""
    f64 = [torch.as_tensor(np.asarray(x), dtype=torch.float64) for x in (origins, dirs, vertices)]
    _, t, u, v, det = ray_mesh_pairs(*f64, faces)
    low = torch.minimum(torch.minimum(u, v), 1 - u - v)
    rim = (low.abs() <= 1e-4) & (t > -1e-3)
    grazing = (low >= 0) & (t.abs() < 1e-3)
    flat = det.abs() < 1e-7
    return (rim | grazing | flat).any(1).numpy()


# ------------------------------------------------------------------------------------------------ the sphere warp
def distances(samples, goal):
    """d [n,V] = sqrt((dx^2 + dy^2) + dz^2), in the dtype of samples."""
    diff = samples[:, None, :] - goal[None, :, :]
    return torch.sqrt((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2])


def sphere_warp(samples, goal, canon, radius, by_mean):
    """(warp [n,3], nearest [n], count [n]) of datasets/vertex_sphere_dataset.py:128-159, its operations in its order."""
    d = distances(samples, goal)
    warp = canon - goal                                                        # :133
    nearest = torch.argmin(d, dim=-1)                                          # :147
    if by_mean:
        count = (d < radius).sum(1)
        assignments = d.clone()                                                # :135
        outside, inside = assignments > radius, assignments < radius           # :136-137
        assignments[outside] = 0                                               # :139 (an equal distance stays: quirk Q12)
        assignments[inside] = 1                                                # :140
        w = (warp[None] * assignments[:, :, None]).sum(dim=1)                  # :142-143
        return w / (assignments.sum(dim=1)[:, None] + 1e-10), nearest, count   # :144
    assignments = d[torch.arange(len(d)), nearest].clone()                     # :148
    count = (assignments < radius).long()
    outside, inside = assignments > radius, assignments < radius               # :150-151
    assignments[outside] = 0
    assignments[inside] = 1
    return warp[nearest] * assignments[:, None], nearest, count                # :156-158


def warp_margins(samples, goal, radius):
    """In float64: (min over all pairs of |d - r|, per sample the gap between its two smallest distances - inf with one vertex)."""
    d = distances(torch.as_tensor(samples, dtype=torch.float64), torch.as_tensor(goal, dtype=torch.float64))
    two = torch.sort(d, dim=1)[0][:, :2]
    gap = two[:, 1] - two[:, 0] if d.shape[1] > 1 else torch.full((len(d),), float("inf"), dtype=torch.float64)
    return float((d - radius).abs().min()), gap.numpy()


# ------------------------------------------------------------------------------------------------ inputs
def body_mesh(level, seed):
    """The bumpy ellipsoid of smpl_nerf_amd.synthetic_smpl: (vertices [V,3] fp32, faces [F,3] int32); level 0 .. 4 has
    20 / 80 / 320 / 1280 / 5120 faces."""
    from smpl_nerf_amd.synthetic_smpl import bumpy_ellipsoid
    return bumpy_ellipsoid(level, seed)


def one_triangle(seed):
    rng = np.random.default_rng(seed)
    v = (np.array([[-0.3, -0.6, 0.0], [0.3, -0.5, 0.05], [0.0, 0.7, -0.05]]) + rng.normal(0, 0.02, (3, 3))).astype(F32)
    return v, np.array([[0, 1, 2]], np.int32)


def triangle_soup(n_faces, seed, toward, size=0.03, box=(0.25, 0.8, 0.2), max_tilt=60.0):
    """n_faces small random triangles spread through the body's box: SMPL's face count and face size without its surface.  Every
    triangle is well shaped and its plane is tilted by at most max_tilt degrees from facing the point `toward` (the camera), so none
    is seen edge-on:
    on a closed surface of this face size a third of 65 rays from one camera see SOME silhouette face with |det| < 1e-7 (15 .. 24
    of 65 on the level-4 ellipsoid over six seeds), which the margins of the GPU tests leave out and their 5 % cap forbids."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1, 1, (n_faces, 3)) * np.asarray(box)
    n = np.asarray(toward, np.float64)[None] - centre
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    helper = np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    a = np.cross(n, helper)
    a /= np.linalg.norm(a, axis=-1, keepdims=True)
    b = np.cross(n, a)
    tilt, turn = np.radians(rng.uniform(0, max_tilt, n_faces)), rng.uniform(0, 2 * np.pi, n_faces)
    side = np.cos(turn)[:, None] * a + np.sin(turn)[:, None] * b
    a2 = np.cos(tilt)[:, None] * side + np.sin(tilt)[:, None] * n                 # the plane's first axis, tilted out of the facing plane
    b2 = np.cross(n, side)                                                         # its second axis stays in it
    # corners at 120 degrees +- 25 and size x (0.7 .. 1.3) from the centre: no sliver, whose |det| would be tiny for every ray
    phi = rng.uniform(0, 2 * np.pi, (n_faces, 1)) + np.radians([0.0, 120.0, 240.0]) + np.radians(rng.uniform(-25, 25, (n_faces, 3)))
    xy = (size * rng.uniform(0.7, 1.3, (n_faces, 3)))[..., None] * np.stack([np.cos(phi), np.sin(phi)], -1)
    v = centre[:, None, :] + xy[..., :1] * a2[:, None, :] + xy[..., 1:] * b2[:, None, :]
    return v.reshape(-1, 3).astype(F32), np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def camera_position(seed, radius=2.4):
    rng = np.random.default_rng(seed)
    az, el = rng.uniform(0, 2 * np.pi), rng.uniform(-0.4, 0.4)
    return radius * np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])


def camera_rays(R, vertices, seed, radius=2.4, away=False):
    """R rays from a camera on the sphere of `radius` (camera_position(seed)), each aimed at a random point of the body's bounding
    box (shrunk to 80 %); normalised directions.  away: the same rays pointing the other way (no hit).  (origins, dirs) fp32."""
    cam = camera_position(seed, radius)
    rng = np.random.default_rng([seed, 1])
    lo, hi = np.asarray(vertices, np.float64).min(0), np.asarray(vertices, np.float64).max(0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    target = mid + 0.8 * half * rng.uniform(-1, 1, (R, 3))
    d = target - cam
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.broadcast_to(cam, (R, 3)).astype(F32).copy(), (-d if away else d).astype(F32)


def warp_inputs(n, V, radius, seed, spread=0.3):
    """goal, canon ~ N(0, spread) [V,3]; n samples in the body's box, every third one planted at a goal vertex plus
    N(0, 0.4 radius) noise, so that a 1 cm sphere has something in it.  fp32 numpy."""
    rng = np.random.default_rng(seed)
    goal = rng.normal(0, spread, (V, 3)).astype(F32)
    canon = rng.normal(0, spread, (V, 3)).astype(F32)
    samples = rng.uniform(-2 * spread, 2 * spread, (n, 3))
    planted = goal[rng.integers(0, V, n)].astype(np.float64) + rng.normal(0, 0.4 * radius, (n, 3))
    mask = np.arange(n) % 3 == 0
    samples[mask] = planted[mask]
    return samples.astype(F32), goal, canon


# ------------------------------------------------------------------------------------------------ the pipeline
G19 = dict(B=12, S=64, frame=dict(h=128, w=128, phi=30.0, theta=-10.0, seed=19), net_seed=419, warp_seed=191, warp_std=0.05)


def g19_inputs():
    """The inputs of tests/golden/g19_vertex_sphere.npz from its seeds: (batch [ray_samples, ray_translation, ray_direction, z_vals,
    warp, rgb_truth] as fp32 numpy arrays, net parameters).  Every third sample carries a warp ~ N(0, warp_std), the others none."""
    from smpl_nerf_amd import synthetic as syn
    c = G19
    data = syn.frame_batch(**c["frame"])
    sub = np.arange(c["B"]) * (128 * 128 // c["B"]) + 41
    rng = np.random.default_rng(c["warp_seed"])
    warp = rng.normal(0, c["warp_std"], (c["B"], c["S"], 3))
    moved = (np.arange(c["S"])[None, :] + np.arange(c["B"])[:, None]) % 3 == 0
    warp[~moved] = 0.0
    batch = [data[0][sub], data[1][sub], data[2][sub], data[3][sub], warp.astype(F32), data[4][sub]]
    return batch, syn.make_scene_net_params(c["net_seed"])


def vertex_sphere_pipeline(P, batch, wb=0):
    """models/vertex_sphere_pipeline.py:25-48 in torch, in the dtype of P: (rgb, warped, densities).  P: RenderRayNet parameters
    (tensors), batch: the data list as tensors."""
    import torch_ref as TR
    samples, ray_o, _, z, warp, _ = batch
    B, S = z.shape
    warped = samples + warp
    sdirs = warped - ray_o[:, None, :]
    dn = sdirs / torch.norm(sdirs, dim=-1, keepdim=True)
    inp = torch.cat([TR.posenc(warped, 10, 0).view(B * S, -1), TR.posenc(dn, 4, 0).view(B * S, -1)], -1)
    raw = TR.render_ray_net(P, inp).view(B, S, 4)
    rgb, _, dens = TR.raw2outputs(raw, z, sdirs, wb)
    return rgb, warped, dens
