"""Numpy / torch (CPU) restatement of the mesh renderer's rule (include/smplnerf.h, snerf_mesh_render_f32), used ONLY by tests and
tools.  The hit comes through single_sample_ref.first_hit; the vertex normals, the shading and the texture lookup are written
operation by operation in the dtype asked for: float32 is the comparison (the kernel must reproduce it bit for bit from its own
face and bary), float64 the yardstick.  Also here: the seeded scenes of tests/test_gpu_mesh_render.py and the margins they need.
"""
import functools

import numpy as np
import torch

import single_sample_ref as SS
import vertex_sphere_ref as SR
from smpl_nerf_amd import synthetic as syn
from smpl_nerf_amd import synthetic_smpl

F32 = np.float32
ANGLE = np.pi / 3
SHADING = dict(ambient=0.3, intensity=0.9, background=(0.25, 0.5, 0.75))      # (0.3 + 0.9 lambert reaches the clamp at 1)


def rays(poses, H, W, camera_angle_x=ANGLE):
    """(origins, dirs) [N, H W, 3] fp32: utils.py:50-54 in float64, rounded once - what RayGenerator makes."""
    o, d = zip(*(syn.camera_rays(H, W, np.asarray(p, np.float64), camera_angle_x) for p in poses))
    return np.stack(o).astype(F32), np.stack(d).astype(F32)


def vertex_faces(faces, V):
    """Per vertex the list of its incident faces in ascending face index, straight from the definition."""
    table = [[] for _ in range(V)]
    for f, corners in enumerate(np.asarray(faces)):
        for c in corners:
            table[int(c)].append(f)
    return table


def vertex_normals(vertices, faces, dtype):
    """n_v = the sum over the incident faces of v, in ascending face index, of e1 x e2 (not normalised), accumulated from 0 one
    face at a time in `dtype`."""
    v = np.asarray(vertices, dtype)
    faces = np.asarray(faces)
    a, b, c = (v[faces[:, k]] for k in range(3))
    e1, e2 = b - a, c - a
    cross = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(dtype)
    table = vertex_faces(faces, len(v))
    n = np.zeros((len(v), 3), dtype)
    for rank in range(max(len(t) for t in table)):
        rows = np.array([i for i, t in enumerate(table) if len(t) > rank], np.int64)
        n[rows] = n[rows] + cross[[table[i][rank] for i in rows]]
    return n


def _mix(w0, u, v, x, faces_hit):
    xa, xb, xc = (x[faces_hit[:, k]] for k in range(3))
    return (w0[:, None] * xa + u[:, None] * xb) + v[:, None] * xc


def shade(vertices, faces, uv, texture, pose, face, bary, dtype, ambient, intensity, background):
    """image [R,3] in `dtype` from the hit (face [R] int, bary [R,2]) of one frame, by the header's rule."""
    faces = np.asarray(faces)
    face, bary = np.asarray(face).reshape(-1), np.asarray(bary, dtype).reshape(-1, 2)
    tex, uv = np.asarray(texture, dtype), np.asarray(uv, dtype)
    Ht, Wt = tex.shape[:2]
    image = np.broadcast_to(np.asarray(background, F32).astype(dtype), (len(face), 3)).copy()
    hit = face >= 0
    if not hit.any():
        return image
    fh = faces[face[hit]]
    one, half, zero = dtype(1), dtype(0.5), dtype(0)
    u, v = bary[hit, 0], bary[hit, 1]
    w0 = (one - u) - v
    m = _mix(w0, u, v, vertex_normals(vertices, faces, dtype), fh)
    length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(length[:, None] == 0, zero, m / length[:, None]).astype(dtype)
    light = np.asarray(pose, np.float64)[:3, 2].astype(F32).astype(dtype)
    lambert = np.maximum(zero, (n[:, 0] * light[0] + n[:, 1] * light[1]) + n[:, 2] * light[2])
    shade_ = np.minimum(one, dtype(F32(ambient)) + dtype(F32(intensity)) * lambert)
    UV = _mix(w0, u, v, uv, fh)
    x, y = UV[:, 0] * dtype(Wt) - half, (one - UV[:, 1]) * dtype(Ht) - half
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    c0, c1 = np.clip(xf.astype(np.int64), 0, Wt - 1), np.clip(xf.astype(np.int64) + 1, 0, Wt - 1)
    r0, r1 = np.clip(yf.astype(np.int64), 0, Ht - 1), np.clip(yf.astype(np.int64) + 1, 0, Ht - 1)
    top = tex[r0, c0] * (one - fx) + tex[r0, c1] * fx
    bottom = tex[r1, c0] * (one - fx) + tex[r1, c1] * fx
    image[hit] = (top * (one - fy) + bottom * fy) * shade_[:, None]
    return image.astype(dtype)


def render(scene, dtype):
    """The whole rule on the CPU in `dtype` (a torch dtype): dict of numpy arrays face [N,R], t, bary [N,R,2], image [N,R,3]."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    o, d = rays(scene["poses"], scene["H"], scene["W"])
    out = {k: [] for k in ("face", "t", "bary", "image")}
    for n in range(len(scene["poses"])):
        v = scene["vertices"][n if len(scene["vertices"]) > 1 else 0]
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        h = SS.first_hit(T(o[n]), T(d[n]), T(v), scene["faces"], T(v))
        img = shade(v, scene["faces"], scene["uv"], scene["texture"], scene["poses"][n], h["face"], h["uv"], npdt, **SHADING)
        for k, x in (("face", h["face"]), ("t", h["t"]), ("bary", h["uv"]), ("image", img)):
            out[k].append(x)
    return {k: np.stack(x) for k, x in out.items()}


def left_out(scene):
    """bool [N,R]: the pixels single_sample_ref.first_hit_margin names, frame by frame."""
    o, d = rays(scene["poses"], scene["H"], scene["W"])
    return np.stack([SS.first_hit_margin(o[n], d[n], scene["vertices"][n if len(scene["vertices"]) > 1 else 0], scene["faces"])[0]
                     for n in range(len(scene["poses"]))])


# ------------------------------------------------------------------------------------------------ scenes
CAMERAS = [(10.0, 25.0), (5.0, 60.0), (-12.0, 200.0)]           # (phi, theta) of the three frames, on a sphere around the body
MESH_SEEDS = (5, 6, 8)


@functools.lru_cache(maxsize=None)
def mesh(F, seed=5):
    """(vertices fp32, faces int32) by face count: one triangle, the bumpy ellipsoid at levels 0, 2 and 3, or the 13 776-face soup
    facing the first camera."""
    if F == 13776:
        return SR.triangle_soup(F, seed, syn.sphere_pose(*CAMERAS[0], 1.5)[:3, 3])
    return {1: lambda: SR.one_triangle(seed), 20: lambda: SR.body_mesh(0, seed), 320: lambda: SR.body_mesh(2, seed),
            1280: lambda: SR.body_mesh(3, seed)}[F]()


@functools.lru_cache(maxsize=None)
def scene(H, W, F, N=1, bodies=1, radius=1.5):
    """dict: poses [N,4,4] float64, vertices [bodies,V,3] fp32 (bodies = 1 or N: distinct seeds), faces, uv, texture, H, W."""
    poses = np.stack([syn.sphere_pose(phi, theta, radius) for phi, theta in CAMERAS[:N]])
    meshes = [mesh(F, MESH_SEEDS[k]) for k in range(bodies)]
    vertices = np.stack([m[0] for m in meshes])
    return dict(poses=poses, vertices=vertices, faces=meshes[0][1], uv=synthetic_smpl.surface_uv(vertices[0], 3),
                texture=synthetic_smpl.smooth_texture(4, 24, 40), H=H, W=W)


def custom_scene(poses, vertices, faces, H, W):
    vertices = np.asarray(vertices, F32)
    vertices = vertices[None] if vertices.ndim == 2 else vertices
    return dict(poses=np.asarray(poses, np.float64).reshape(-1, 4, 4), vertices=vertices, faces=np.asarray(faces, np.int32),
                uv=synthetic_smpl.surface_uv(vertices[0], 3), texture=synthetic_smpl.smooth_texture(4, 24, 40), H=H, W=W)


# the float64 end-to-end cases (at most 32 x 32 x 1280): (H, W, F, N, bodies)
F64_CASES = [(8, 8, 20, 1, 1), (9, 13, 320, 3, 3), (32, 32, 320, 1, 1), (32, 32, 1280, 3, 1)]
