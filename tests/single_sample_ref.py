"""Torch (CPU) restatement of the first hit of a ray on a mesh and of the single-sample pipeline, used ONLY by tests and tools.

  * first_hit: the rule of include/smplnerf.h (snerf_ray_mesh_first_hit_f32) operation for operation, on the pairs of
    vertex_sphere_ref.ray_mesh_pairs, in the dtype of its inputs.  Run in float64 it is the yardstick, run in fp32 the comparison;
  * get_warp_solve: the form the reference gives the warp (render.py:291-301: a 3 x 3 solve per hit ray), in float64;
  * first_hit_margin: the rays the GPU tests leave out;
  * the seeded inputs of the tests (meshes and rays are vertex_sphere_ref's), the constructed tie, the inputs of
    tests/golden/g21_single_sample.npz rebuilt from its seeds, and SmplPipeline.forward in torch.
"""
import numpy as np
import torch

import vertex_sphere_ref as SR
from vertex_sphere_ref import relative_error  # noqa: F401

F32 = np.float32


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def first_hit(origins, dirs, vertices, faces, canon):
    """dict of numpy arrays in the dtype of origins: t [R] (+inf on a miss), face [R] int32 (-1), uv [R,2] (0), depth [R] (0),
    warp [R,3] (0).  The smallest t over the hitting faces, the first index among equal ones (torch.argmin)."""
    faces = torch.as_tensor(np.asarray(faces)).long()
    hit, t, u, v, _ = SR.ray_mesh_pairs(origins, dirs, vertices, faces)
    inf = torch.full_like(t, float("inf"))
    face = torch.argmin(torch.where(hit, t, inf), dim=1)
    any_hit = hit.any(1)
    row = torch.arange(len(origins))
    zero = torch.zeros((), dtype=origins.dtype)
    tb = torch.where(any_hit, t[row, face], zero)                       # (finite stand-in on a miss: the results are masked below)
    ub, vb = torch.where(any_hit, u[row, face], zero), torch.where(any_hit, v[row, face], zero)
    dx, dy, dz = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    depth = tb * torch.sqrt((dx * dx + dy * dy) + dz * dz)
    ca, cb, cc = (canon[faces[face][:, k]] for k in range(3))
    canon_point = (ca + ub[:, None] * (cb - ca)) + vb[:, None] * (cc - ca)
    hit_point = origins + dirs * tb[:, None]
    warp = torch.where(any_hit[:, None], canon_point - hit_point, zero)
    return {"t": torch.where(any_hit, tb, inf[:, 0]).numpy(), "face": torch.where(any_hit, face, -torch.ones_like(face)).to(torch.int32).numpy(),
            "uv": torch.stack([ub, vb], -1).numpy(), "depth": torch.where(any_hit, depth, zero).numpy(), "warp": warp.numpy()}


def get_warp_solve(origins, dirs, vertices, faces, canon):
    """warp [R,3] float64 numpy by the reference's form (render.py:291-301) on the float64 first hit: x solves
    goal_vertices^T x = hit point, the canonical point is canonical_vertices^T x; zero on a miss."""
    o, d, vt, cn = (_t(x, torch.float64) for x in (origins, dirs, vertices, canon))
    h = first_hit(o, d, vt, faces, cn)
    o, d, vt, cn, faces = o.numpy(), d.numpy(), vt.numpy(), cn.numpy(), np.asarray(faces)
    warp = np.zeros((len(o), 3))
    for r in np.nonzero(h["face"] >= 0)[0]:
        p = o[r] + d[r] * h["t"][r]
        vertex_indices = faces[h["face"][r]]
        x = np.linalg.solve(vt[vertex_indices].T, p)
        warp[r] = cn[vertex_indices].T.dot(x) - p
    return warp


def solve_condition(origins, dirs, vertices, faces):
    """The largest 2-norm condition number of goal_vertices^T over the hit faces (float64)."""
    o, d, vt = (_t(x, torch.float64) for x in (origins, dirs, vertices))
    face = first_hit(o, d, vt, faces, vt)["face"]
    return max((np.linalg.cond(vt.numpy()[np.asarray(faces)[f]].T) for f in face[face >= 0]), default=0.0)


def first_hit_margin(origins, dirs, vertices, faces):
    """The rays left out, bool [R] numpy: those vertex_sphere_ref.ambiguous_rays names, and those whose two smallest float64 hit
    parameters are closer than 1e-4 (fp32 may order them otherwise).  Also returns the smallest such gap over the other rays."""
    ambiguous = SR.ambiguous_rays(origins, dirs, vertices, faces)
    t2 = SR.ray_mesh_hits(*(_t(x, torch.float64) for x in (origins, dirs, vertices)), faces, 2)[0]
    with np.errstate(invalid="ignore"):
        gap = t2[:, 1] - t2[:, 0]                                      # inf with one hit, nan with none
    close = np.nan_to_num(gap, nan=np.inf) < 1e-4
    rest = gap[~(ambiguous | close) & np.isfinite(gap)]
    return ambiguous | close, (float(rest.min()) if len(rest) else float("inf"))


def canon_of(vertices, seed=7):
    """canon = vertices + N(0, 0.05), fp32."""
    return (np.asarray(vertices, np.float64) + np.random.default_rng(seed).normal(0, 0.05, np.shape(vertices))).astype(F32)


# meshes by face count (cam: where the rays start): one triangle, the bumpy ellipsoid at levels 0, 2 and 3, and SMPL's face count as a
# soup of small triangles none of which the camera sees edge-on (vertex_sphere_ref.triangle_soup says why)
MESHES = {1: lambda cam: SR.one_triangle(5), 20: lambda cam: SR.body_mesh(0, 5), 320: lambda cam: SR.body_mesh(2, 5),
          1280: lambda cam: SR.body_mesh(3, 5), 13776: lambda cam: SR.triangle_soup(13776, 5, cam)}
RAY_SEEDS = {(1, 1): 3}          # (R, F) -> the seed of its rays where seed 1's one ray hits nothing


def case_inputs(R, F, scale=1.0, away=False):
    """(origins, dirs, vertices, faces, canon) of the case (R rays, F faces), fp32 / int32; dirs scaled by `scale` in fp32."""
    seed = RAY_SEEDS.get((R, F), 1)
    v, f = MESHES[F](SR.camera_position(seed))
    o, d = SR.camera_rays(R, v, seed, away=away)
    return o, (d * F32(scale)).astype(F32), v, f, canon_of(v)


def tie_case():
    """Two coincident triangles as faces 3 and 7 of a 10-face table (their vertices are separate rows with equal coordinates: the
    same arithmetic, so exactly equal t), the other eight far off the rays; 5 rays through the pair.  canon differs between the
    two copies, so the warp tells which face was taken.  (origins, dirs, vertices, faces, canon) fp32 / int32."""
    rng = np.random.default_rng(37)
    tri = np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, -0.1], [0.0, 0.7, 0.05]])
    vertices = np.zeros((30, 3))
    for f in range(10):
        vertices[3 * f:3 * f + 3] = tri if f in (3, 7) else tri * 0.1 + [5.0 + f, 5.0, 0.0]
    faces = np.arange(30, dtype=np.int32).reshape(10, 3)
    target = tri.mean(0) + rng.uniform(-0.08, 0.08, (5, 3)) * [1, 1, 0]
    origins = np.broadcast_to([0.1, -0.2, 2.4], (5, 3)).copy()
    dirs = target - origins
    canon = vertices + rng.normal(0, 0.05, vertices.shape)
    return origins.astype(F32), dirs.astype(F32), vertices.astype(F32), faces, canon.astype(F32)


# ------------------------------------------------------------------------------------------------ the pipeline
G21 = dict(B=130, frame=dict(h=128, w=128, phi=20.0, theta=35.0, seed=21), sample=23, net_seed=421, warp_seed=211, warp_std=0.05)


def g21_inputs():
    """The inputs of tests/golden/g21_single_sample.npz from its seeds: (batch [ray_sample [B,3], ray_translation, ray_direction,
    goal_pose [B,69], warp [B,3], rgb_truth] as fp32 numpy arrays, net parameters).  Every third ray carries a warp ~ N(0, warp_std),
    the others none; the sample of a ray is one of its stratified ones."""
    from smpl_nerf_amd import synthetic as syn
    c = G21
    data = syn.frame_batch(**c["frame"])
    sub = np.arange(c["B"]) * (128 * 128 // c["B"]) + 41
    warp = np.random.default_rng(c["warp_seed"]).normal(0, c["warp_std"], (c["B"], 3))
    warp[np.arange(c["B"]) % 3 != 0] = 0.0
    pose = np.repeat(syn.human_poses((41, 38), 0, 60, 2)[1:], c["B"], axis=0)
    batch = [data[0][sub, c["sample"]], data[1][sub], data[2][sub], pose, warp.astype(F32), data[4][sub]]
    return [np.ascontiguousarray(a, F32) for a in batch], syn.make_scene_net_params(c["net_seed"])


def single_sample_pipeline(P, batch):
    """models/singe_sample_pipeline.py:27-40 in torch, in the dtype of P: rgb [B,3].  P: RenderRayNet parameters (tensors), batch:
    the data list as tensors."""
    import torch_ref as TR
    sample, ray_o, _, _, warp, _ = batch
    warped = sample + warp
    sdirs = warped - ray_o
    dn = sdirs / torch.norm(sdirs, dim=-1, keepdim=True)
    raw = TR.render_ray_net(P, torch.cat([TR.posenc(warped, 10, 0), TR.posenc(dn, 4, 0)], -1))
    return torch.sigmoid(raw[..., :3])
