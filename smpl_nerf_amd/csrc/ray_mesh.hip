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
//
// The first hit (render.py:222-319, get_warp: one intersector call, then two Python loops over the rays): the same walk and the same
// pair rule (rm_pair of ray_mesh_pair.h, shared with mesh_render.hip), but a lane keeps (t, face, u, v) of its nearest hit, replaced only on a strict
// t <.  A wave walks its slice in ascending face order, the slices ascend with the wave index and wave 0 merges in wave order with the
// same strict <, so equal t goes to the smaller face index.  The face index is the walk's own counter.  With `canon` wave 0 then
// gathers, per hit ray, the three indices of its face and nine floats of the canonical body: depth = t |d| and
// warp = (ca + u (cb - ca) + v (cc - ca)) - (o + d t).  The extra state is written inside the hit branch only.
#include "ray_mesh_pair.h"

namespace snerf {

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
    float T[9];
    rm_face(vertices, faces, f, T);
#pragma unroll
    for (int i = 0; i < 9; ++i) tri[(int64_t)f * 9 + i] = T[i];
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

__device__ __forceinline__ RmRay rm_load_ray(const float *origins, const float *dirs, int64_t rr) {
    return {origins[rr * 3 + 0], origins[rr * 3 + 1], origins[rr * 3 + 2], dirs[rr * 3 + 0], dirs[rr * 3 + 1], dirs[rr * 3 + 2]};
}

template <int KC>
__global__ __launch_bounds__(RM_WAVES * 64) void ray_mesh_hits_kernel(RmArgs A) {
    __shared__ float part[RM_WAVES][KC][WAVE];
    __shared__ int cnt[RM_WAVES][WAVE];
    const int lane = lane_id(), wave = wave_index();
    const int64_t r = (int64_t)blockIdx.x * WAVE + lane;
    const bool valid = r < A.R;
    const RmRay y = rm_load_ray(A.origins, A.dirs, tail_index(r, A.R, valid));
    const Slice sl = wave_slice(A.F, RM_WAVES, wave);
    float list[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) list[i] = INFINITY;
    int hits = 0;

    auto pair = [&](const float *T) {
        rm_pair(y, T, [&](float t, float, float) {
            ++hits;
            rm_insert<KC>(list, t);
        });
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

struct RmFirstArgs {
    const float *origins, *dirs, *tri, *canon;   // canon [V, 3] or null: then warp and depth are null too
    const int32_t *faces;
    float *t, *uv, *warp, *depth;
    int32_t *face;
    int64_t R;
    int F;
};

__global__ __launch_bounds__(RM_WAVES * 64) void ray_mesh_first_hit_kernel(RmFirstArgs A) {
    __shared__ float part[RM_WAVES][4][WAVE];   // t, face (its bits), u, v of each wave's nearest hit
    const int lane = lane_id(), wave = wave_index();
    const int64_t r = (int64_t)blockIdx.x * WAVE + lane;
    const bool valid = r < A.R;
    const RmRay y = rm_load_ray(A.origins, A.dirs, tail_index(r, A.R, valid));
    const Slice sl = wave_slice(A.F, RM_WAVES, wave);
    RmFirst best;

    auto pair = [&](int f, const float *T) { rm_pair(y, T, [&](float t, float u, float v) { best.take(t, f, u, v); }); };

    walk4<9>(
        A.tri, sl.lo, sl.hi,
        [&](int f, const float *T) {
#pragma unroll
            for (int j = 0; j < 4; ++j) pair(f + j, T + 9 * j);
        },
        [&](int f, const float *T) { pair(f, T); });

    put_partials(part[wave], lane, best.t, __int_as_float(best.face), best.u, best.v);
    __syncthreads();
    if (wave != 0 || !valid) return;
    rm_merge_first(best, part, lane);
    A.t[r] = best.t;
    A.face[r] = best.face;
    A.uv[r * 2 + 0] = best.u;
    A.uv[r * 2 + 1] = best.v;
    if (!A.canon) return;
    float depth, warp[3];
    rm_canon(y, best, A.faces, A.canon, depth, warp);
    A.depth[r] = depth;
    A.warp[r * 3 + 0] = warp[0];
    A.warp[r * 3 + 1] = warp[1];
    A.warp[r * 3 + 2] = warp[2];
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

// The checks both entries make, in one order; bad_pointers: what is wrong with the entry's own pointers, or null - looked at only
// with R > 0.  On SNERF_OK with R > 0 the pre-pass has been launched and `blocks` is the grid.
static int rm_prepare(const char *op, const char *bad_pointers, const float *vertices, const int32_t *faces, int64_t R, int V, int F,
                      void *workspace, int64_t workspace_bytes, hipStream_t s, int64_t &blocks) {
    using namespace snerf;
    if (int rc = check_walk_count(op, "V", V, 3)) return rc;
    if (int rc = check_walk_count(op, "F", F, 9)) return rc;
    if (R == 0) return SNERF_OK;
    if (bad_pointers) return fail(SNERF_E_BADARG, "%s: %s", op, bad_pointers);
    if (!workspace || workspace_bytes < (int64_t)F * 9 * (int64_t)sizeof(float))
        return fail(SNERF_E_BADARG, "%s: workspace missing or smaller than snerf_ray_mesh_workspace_bytes()", op);
    if (int rc = chunk_blocks(op, "R", R, blocks)) return rc;
    hipLaunchKernelGGL(ray_mesh_faces_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, vertices, faces, F, (float *)workspace);
    return SNERF_OK;
}

extern "C" int snerf_ray_mesh_hits_f32(const float *origins, const float *dirs, const float *vertices, const int32_t *faces, int64_t R,
                                       int V, int F, int max_hits, float *t_hits, int32_t *n_hits, void *workspace,
                                       int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    if (R < 0) return fail(SNERF_E_BADARG, "ray_mesh_hits: R must not be negative");
    if (max_hits < 1 || max_hits > RM_MAX_HITS) return fail(SNERF_E_BADARG, "ray_mesh_hits: max_hits must be 1 .. %d", RM_MAX_HITS);
    hipStream_t s = (hipStream_t)stream;
    int64_t blocks = 0;
    const char *bad = !origins || !dirs || !vertices || !faces || !t_hits || !n_hits ? "null pointer (origins, dirs, vertices, faces, t_hits, n_hits)" : nullptr;
    if (int rc = rm_prepare("ray_mesh_hits", bad, vertices, faces, R, V, F, workspace, workspace_bytes, s, blocks)) return rc;
    if (R == 0) return SNERF_OK;
    RmArgs A{origins, dirs, (const float *)workspace, t_hits, n_hits, R, F, max_hits};
    if (max_hits == 1) rm_launch<1>(A, (unsigned)blocks, s);
    else if (max_hits <= 4) rm_launch<4>(A, (unsigned)blocks, s);
    else if (max_hits <= 8) rm_launch<8>(A, (unsigned)blocks, s);
    else rm_launch<16>(A, (unsigned)blocks, s);
    return check_launch("ray_mesh_hits");
}

extern "C" int snerf_ray_mesh_first_hit_f32(const float *origins, const float *dirs, const float *vertices, const int32_t *faces, int64_t R,
                                            int V, int F, const float *canon, float *t, int32_t *face, float *uv, float *warp, float *depth,
                                            void *workspace, int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    if (R < 0) return fail(SNERF_E_BADARG, "ray_mesh_first_hit: R must not be negative");
    hipStream_t s = (hipStream_t)stream;
    int64_t blocks = 0;
    const char *bad = !origins || !dirs || !vertices || !faces || !t || !face || !uv ? "null pointer (origins, dirs, vertices, faces, t, face, uv)"
                      : (canon && warp && depth) || (!canon && !warp && !depth) ? nullptr
                                                                                : "canon, warp and depth must be all null or all non-null";
    if (int rc = rm_prepare("ray_mesh_first_hit", bad, vertices, faces, R, V, F, workspace, workspace_bytes, s, blocks)) return rc;
    if (R == 0) return SNERF_OK;
    RmFirstArgs A{origins, dirs, (const float *)workspace, canon, faces, t, uv, warp, depth, face, R, F};
    hipLaunchKernelGGL(ray_mesh_first_hit_kernel, dim3((unsigned)blocks), dim3(RM_WAVES * 64), 0, s, A);
    return check_launch("ray_mesh_first_hit");
}
