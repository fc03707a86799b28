// What ray_mesh.hip (rays given in memory) and mesh_render.hip (rays of a pinhole camera, made in the kernel) share: the nine floats
// (a, e1, e2) of a face, the pair rule of two-sided Moeller-Trumbore in fp32 with its first-hit order, and what a first hit gathers
// from the canonical body.  One text, so that the renderer's t, face, (u, v), depth and warp are the first-hit kernel's bit for bit.
#pragma once
#include <math.h>

#include "pair_walk.h"

namespace snerf {

constexpr int RM_WAVES = 8;       // waves of a ray-chunk workgroup: the face slices

__device__ __forceinline__ float dot3(float x0, float x1, float x2, float y0, float y1, float y2) { return x0 * y0 + x1 * y1 + x2 * y2; }

// T[0..8] = (a, e1 = b - a, e2 = c - a) of face f
__device__ __forceinline__ void rm_face(const float *vertices, const int32_t *faces, int f, float (&T)[9]) {
    const float *a = vertices + (int64_t)faces[f * 3 + 0] * 3, *b = vertices + (int64_t)faces[f * 3 + 1] * 3,
                *c = vertices + (int64_t)faces[f * 3 + 2] * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        T[i] = a[i];
        T[3 + i] = b[i] - a[i];
        T[6 + i] = c[i] - a[i];
    }
}

// one ray of a lane
struct RmRay {
    float ox, oy, oz, dx, dy, dz;
};

// The pair rule, for all kernels: the ray against T, the nine floats (a, e1, e2) of one face at a wave-uniform address;
// hit(t, u, v) runs for a pair that is one.
template <class Hit>
__device__ __forceinline__ void rm_pair(const RmRay &y, const float *T, Hit &&hit) {
    const float px = y.dy * T[8] - y.dz * T[7], py = y.dz * T[6] - y.dx * T[8], pz = y.dx * T[7] - y.dy * T[6];   // p = d x e2
    const float det = dot3(T[3], T[4], T[5], px, py, pz);
    const float sx = y.ox - T[0], sy = y.oy - T[1], sz = y.oz - T[2];
    const float un = dot3(sx, sy, sz, px, py, pz);
    const float qx = sy * T[5] - sz * T[4], qy = sz * T[3] - sx * T[5], qz = sx * T[4] - sy * T[3];   // q = s x e1
    const float vn = dot3(y.dx, y.dy, y.dz, qx, qy, qz);
    // the wide test: u and v through the hardware reciprocal (1 ulp), 1e-5 to spare; a tiny det goes to the exact rule as it is
    const float inv = __builtin_amdgcn_rcpf(det);
    const float ur = un * inv, vr = vn * inv;
    const bool maybe = (ur >= -1e-5f && vr >= -1e-5f && ur + vr <= 1.f + 1e-5f) || fabsf(det) < 1e-30f;
    if (maybe && det != 0.f) {
        const float u = un / det, v = vn / det;
        if (u >= 0.f && v >= 0.f && u + v <= 1.f) {
            const float t = dot3(T[6], T[7], T[8], qx, qy, qz) / det;
            if (t > 0.f) hit(t, u, v);
        }
    }
}

// a lane's nearest hit so far: replaced only on a strict t <, so of equal t the pair seen first - the smaller face index - stays
struct RmFirst {
    float t = INFINITY, u = 0.f, v = 0.f;
    int face = -1;
    __device__ __forceinline__ void take(float t_, int face_, float u_, float v_) {
        if (t_ < t) t = t_, face = face_, u = u_, v = v_;
    }
};

// wave 0 after the barrier: the other waves' nearest hits (part[w]: t, face (its bits), u, v) in wave order = ascending face order
__device__ __forceinline__ void rm_merge_first(RmFirst &b, const float (&part)[RM_WAVES][4][WAVE], int lane) {
    for (int w = 1; w < RM_WAVES; ++w) b.take(part[w][0][lane], __float_as_int(part[w][1][lane]), part[w][2][lane], part[w][3][lane]);
}

// depth = t |d| and warp = (ca + u (cb - ca) + v (cc - ca)) - (o + d t) of a hit; zeros on a miss
__device__ __forceinline__ void rm_canon(const RmRay &y, const RmFirst &b, const int32_t *faces, const float *canon, float &depth,
                                         float (&warp)[3]) {
    depth = warp[0] = warp[1] = warp[2] = 0.f;
    if (b.face < 0) return;
    const float *ca = canon + (int64_t)faces[b.face * 3 + 0] * 3, *cb = canon + (int64_t)faces[b.face * 3 + 1] * 3,
                *cc = canon + (int64_t)faces[b.face * 3 + 2] * 3;
    depth = b.t * sqrtf(dist2(y.dx, y.dy, y.dz));
    warp[0] = ((ca[0] + b.u * (cb[0] - ca[0])) + b.v * (cc[0] - ca[0])) - (y.ox + y.dx * b.t);
    warp[1] = ((ca[1] + b.u * (cb[1] - ca[1])) + b.v * (cc[1] - ca[1])) - (y.oy + y.dy * b.t);
    warp[2] = ((ca[2] + b.u * (cb[2] - ca[2])) + b.v * (cc[2] - ca[2])) - (y.oz + y.dz * b.t);
}

}  // namespace snerf
