// All hits of R rays on one triangle mesh (datasets/vertex_sphere_dataset.py:84-116 asks trimesh for them, one ray at a time):
// two-sided Moeller-Trumbore in fp32.  For the ray (o, d) and the triangle (a, b, c):
//   e1 = b - a    e2 = c - a    p = d x e2    det = e1 . p    s = o - a    u = s . p / det    q = s x e1    v = d . q / det
//   t = e2 . q / det           a hit is  det != 0,  u >= 0,  v >= 0,  u + v <= 1,  t > 0           (no back-face culling)
// t_hits[r, :] = the K smallest t of ray r in ascending order, padded with +inf; n_hits[r] = the number of hits, which may exceed K.
//
// Mapping: a pre-pass writes (a, e1, e2) per face into the workspace (36 F bytes, once per call).  Main kernel: workgroup = 64-ray
// chunk, lane = ray; its 8 waves split the faces and read the nine floats of a face at wave-uniform addresses (through the scalar
// cache: one load per wave, not per lane), four faces per wait: the walk of pair_walk.h.  Each lane keeps
// its K smallest t as a sorted register list plus a count; the per-wave lists meet in LDS and wave 0 merges them in wave order.
// Nothing of size R F exists in memory; no atomics; the K smallest of a set do not depend on the order: two calls give the same bits.
//
// What bounds it: the VALU.  A pair costs the two cross products, three dot products and the test - about 45 vector instructions,
// products and sums kept apart (-ffp-contract=off) - against 36 bytes per face from the scalar cache per WAVE, four faces per wait;
// the three divisions of the rule run only for the pairs that pass a test on u and v formed with the hardware reciprocal, widened
// by 1e-5 so that it never decides: the decision is taken on the divided values.
#include <math.h>

#include "pair_walk.h"

namespace snerf {

constexpr int RM_WAVES = 8;       // waves of a ray-chunk workgroup: the face slices
constexpr int RM_MAX_HITS = 16;   // largest K

struct RmArgs {
    const float *origins, *dirs, *tri;   // tri [F, 9]: a, e1, e2
    float *t_hits;
    int32_t *n_hits;
    int64_t R;
    int F, K;
};

__global__ __launch_bounds__(256) void ray_mesh_faces_kernel(const float *vertices, const int32_t *faces, int F, float *tri) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float *a = vertices + (int64_t)faces[f * 3 + 0] * 3, *b = vertices + (int64_t)faces[f * 3 + 1] * 3,
                *c = vertices + (int64_t)faces[f * 3 + 2] * 3;
    float *o = tri + (int64_t)f * 9;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = a[i];
        o[3 + i] = b[i] - a[i];
        o[6 + i] = c[i] - a[i];
    }
}

// the sorted list of the KC smallest values seen: a new value sinks in by one compare-and-swap per slot
template <int KC>
__device__ __forceinline__ void rm_insert(float (&list)[KC], float t) {
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        const float lo = fminf(list[i], t), hi = fmaxf(list[i], t);
        list[i] = lo;
        t = hi;
    }
}

__device__ __forceinline__ float dot3(float x0, float x1, float x2, float y0, float y1, float y2) { return x0 * y0 + x1 * y1 + x2 * y2; }

template <int KC>
__global__ __launch_bounds__(RM_WAVES * 64) void ray_mesh_hits_kernel(RmArgs A) {
    __shared__ float part[RM_WAVES][KC][WAVE];
    __shared__ int cnt[RM_WAVES][WAVE];
    const int lane = lane_id(), wave = wave_index();
    const int64_t r = (int64_t)blockIdx.x * WAVE + lane;
    const bool valid = r < A.R;
    const int64_t rr = tail_index(r, A.R, valid);
    const float ox = A.origins[rr * 3 + 0], oy = A.origins[rr * 3 + 1], oz = A.origins[rr * 3 + 2];
    const float dx = A.dirs[rr * 3 + 0], dy = A.dirs[rr * 3 + 1], dz = A.dirs[rr * 3 + 2];
    const Slice sl = wave_slice(A.F, RM_WAVES, wave);
    float list[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) list[i] = INFINITY;
    int hits = 0;

    auto pair = [&](const float *T) {   // T: the nine floats of one face, wave-uniform
        const float px = dy * T[8] - dz * T[7], py = dz * T[6] - dx * T[8], pz = dx * T[7] - dy * T[6];   // p = d x e2
        const float det = dot3(T[3], T[4], T[5], px, py, pz);
        const float sx = ox - T[0], sy = oy - T[1], sz = oz - T[2];
        const float un = dot3(sx, sy, sz, px, py, pz);
        const float qx = sy * T[5] - sz * T[4], qy = sz * T[3] - sx * T[5], qz = sx * T[4] - sy * T[3];   // q = s x e1
        const float vn = dot3(dx, dy, dz, qx, qy, qz);
        // the wide test: u and v through the hardware reciprocal (1 ulp), 1e-5 to spare; a tiny det goes to the exact rule as it is
        const float inv = __builtin_amdgcn_rcpf(det);
        const float ur = un * inv, vr = vn * inv;
        const bool maybe = (ur >= -1e-5f && vr >= -1e-5f && ur + vr <= 1.f + 1e-5f) || fabsf(det) < 1e-30f;
        if (maybe && det != 0.f) {
            const float u = un / det, v = vn / det;
            if (u >= 0.f && v >= 0.f && u + v <= 1.f) {
                const float t = dot3(T[6], T[7], T[8], qx, qy, qz) / det;
                if (t > 0.f) {
                    ++hits;
                    rm_insert<KC>(list, t);
                }
            }
        }
    };

    // (the walk indexes tri in 32 bits: the host refuses 9 F at 2^31 and above)
    walk4<9>(
        A.tri, sl.lo, sl.hi,
        [&](int, const float *T) {
#pragma unroll
            for (int j = 0; j < 4; ++j) pair(T + 9 * j);
        },
        [&](int, const float *T) { pair(T); });

#pragma unroll
    for (int i = 0; i < KC; ++i) part[wave][i][lane] = list[i];
    cnt[wave][lane] = hits;
    __syncthreads();
    if (wave != 0 || !valid) return;
    for (int w = 1; w < RM_WAVES; ++w) {
        hits += cnt[w][lane];
#pragma unroll
        for (int i = 0; i < KC; ++i) rm_insert<KC>(list, part[w][i][lane]);
    }
    A.n_hits[r] = hits;
#pragma unroll
    for (int i = 0; i < KC; ++i)
        if (i < A.K) A.t_hits[r * A.K + i] = list[i];
}

template <int KC>
static void rm_launch(const RmArgs &A, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(ray_mesh_hits_kernel<KC>, dim3(blocks), dim3(RM_WAVES * 64), 0, s, A);
}

}  // namespace snerf

extern "C" int64_t snerf_ray_mesh_workspace_bytes(int F) {
    using namespace snerf;
    if (check_walk_count("ray_mesh_workspace_bytes", "F", F, 9)) return -1;
    return (int64_t)F * 9 * (int64_t)sizeof(float);
}

extern "C" int snerf_ray_mesh_hits_f32(const float *origins, const float *dirs, const float *vertices, const int32_t *faces, int64_t R,
                                       int V, int F, int max_hits, float *t_hits, int32_t *n_hits, void *workspace,
                                       int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    if (R < 0) return fail(SNERF_E_BADARG, "ray_mesh_hits: R must not be negative");
    if (max_hits < 1 || max_hits > RM_MAX_HITS) return fail(SNERF_E_BADARG, "ray_mesh_hits: max_hits must be 1 .. %d", RM_MAX_HITS);
    if (int rc = check_walk_count("ray_mesh_hits", "V", V, 3)) return rc;
    if (int rc = check_walk_count("ray_mesh_hits", "F", F, 9)) return rc;
    if (R == 0) return SNERF_OK;
    if (!origins || !dirs || !vertices || !faces || !t_hits || !n_hits)
        return fail(SNERF_E_BADARG, "ray_mesh_hits: null pointer (origins, dirs, vertices, faces, t_hits, n_hits)");
    if (!workspace || workspace_bytes < (int64_t)F * 9 * (int64_t)sizeof(float))
        return fail(SNERF_E_BADARG, "ray_mesh_hits: workspace missing or smaller than snerf_ray_mesh_workspace_bytes()");
    int64_t blocks;
    if (int rc = chunk_blocks("ray_mesh_hits", "R", R, blocks)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *tri = (float *)workspace;
    hipLaunchKernelGGL(ray_mesh_faces_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, vertices, faces, F, tri);
    RmArgs A{origins, dirs, tri, t_hits, n_hits, R, F, max_hits};
    if (max_hits == 1) rm_launch<1>(A, (unsigned)blocks, s);
    else if (max_hits <= 4) rm_launch<4>(A, (unsigned)blocks, s);
    else if (max_hits <= 8) rm_launch<8>(A, (unsigned)blocks, s);
    else rm_launch<16>(A, (unsigned)blocks, s);
    return check_launch("ray_mesh_hits");
}
