// The skeleton of the brute-force "pair walk" kernels (vertex_warp.hip, image_warp.hip, vertex_sphere.hip, gmm_pdf.hip, ray_mesh.hip): every lane
// holds one sample or ray, a workgroup is one 64-lane chunk of them, and its waves split the other axis - the items: vertices,
// means, faces - into consecutive slices which each wave reads at wave-uniform addresses (the compiler reads them through the scalar
// cache: one load per wave, not per lane).  The per-wave partials meet in LDS as part[WAVES][Q][64] and wave 0 combines them in wave
// order; how they combine is each kernel's own business.  Here: what at least two of the five files share.  (gmm_pdf.hip and
// vertex_sphere.hip write the loop of walk4 out themselves: their kernels measured slower with their bodies in functors.)
#pragma once
#include "snerf_common.h"

namespace snerf {

// ---- device ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// the element a lane loads: its own, or - the lanes past the end - the last one, which exists; those lanes store nothing
template <class I>
__device__ __forceinline__ I tail_index(I i, I n, bool valid) { return valid ? i : n - 1; }

// |p - g|^2 in the order ((dx dx + dy dy) + dz dz); the build keeps products and sums apart (-ffp-contract=off)
__device__ __forceinline__ float dist2(float dx, float dy, float dz) { return dx * dx + dy * dy + dz * dz; }

// The items [lo, hi) of wave `wave` of `waves`: ceil(n / waves) each, both ends clamped to n.  The slices of the waves 0 .. waves - 1
// are consecutive, disjoint and cover [0, n); with n < waves the last waves get the empty [n, n).
struct Slice {
    int lo, hi;
};
constexpr __host__ __device__ Slice wave_slice(int n, int waves, int wave) {
    const int per = (n + waves - 1) / waves;
    const int lo = wave * per < n ? wave * per : n;
    return {lo, lo + per < n ? lo + per : n};
}
constexpr bool slices_tile(int n, int waves) {
    int end = 0;
    for (int w = 0; w < waves; ++w) {
        const Slice s = wave_slice(n, waves, w);
        if (s.lo != end || s.hi < s.lo || s.hi > n) return false;
        end = s.hi;
    }
    return end == n;
}
template <int... Ns>
constexpr bool slices_tile_all() { return ((slices_tile(Ns, 8) && slices_tile(Ns, 16)) && ...); }
static_assert(slices_tile_all<0, 1, 15, 16, 17, 63, 65, 6890>(), "wave_slice: the slices of a workgroup's waves must tile [0, n)");

// The items [v0, v1) of `base` (N floats each, wave-uniform addresses), four per wait: quad(v, t) gets the 4 N floats of the items
// v .. v + 3, requested together - a wave waits for the scalar cache once per four items - and one(v, t) the N floats of each of
// the last 0 .. 3.  The index arithmetic is 32-bit: the host refuses N times the item count at 2^31 and above (check_walk_count).
template <int N, class Quad, class One>
__device__ __forceinline__ void walk4(const float *base, int v0, int v1, Quad &&quad, One &&one) {
    int v = v0;
    for (; v + 4 <= v1; v += 4) {
        float t[4 * N];
#pragma unroll
        for (int k = 0; k < 4 * N; ++k) t[k] = base[v * N + k];
        quad(v, t);
    }
    for (; v < v1; ++v) {
        float t[N];
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = base[v * N + k];
        one(v, t);
    }
}

// f(v, gx, gy, gz, dx, dy, dz, d2) for the vertices [v0, v1) of g that can matter to the sample (px, py, pz) of a lane (vertex_warp.hip,
// image_warp.hip): walk4 hands them over four at a time, the four squared distances share ONE test against r2, and f - which decides
// per vertex - runs for all four when any is below it (WAVE_UNIFORM: when any lane's is) and for each of the last 0 .. 3 vertices.
template <bool WAVE_UNIFORM, class F>
__device__ __forceinline__ void radius_walk(const float *g, int v0, int v1, float px, float py, float pz, float r2, F &&f) {
    walk4<3>(
        g, v0, v1,
        [&](int v, const float *t) {
            float dx[4], dy[4], dz[4], d2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dx[j] = px - t[3 * j];
                dy[j] = py - t[3 * j + 1];
                dz[j] = pz - t[3 * j + 2];
                d2[j] = dist2(dx[j], dy[j], dz[j]);
            }
            const bool any = fminf(fminf(d2[0], d2[1]), fminf(d2[2], d2[3])) < r2;
            if (WAVE_UNIFORM ? __builtin_amdgcn_ballot_w64(any) != 0 : any) {
#pragma unroll
                for (int j = 0; j < 4; ++j) f(v + j, t[3 * j], t[3 * j + 1], t[3 * j + 2], dx[j], dy[j], dz[j], d2[j]);
            }
        },
        [&](int v, const float *t) {
            const float dx = px - t[0], dy = py - t[1], dz = pz - t[2];
            f(v, t[0], t[1], t[2], dx, dy, dz, dist2(dx, dy, dz));
        });
}

// a lane's partials x... into rows 0, 1, ... of its wave's part[wave]
template <int Q, class E, class... T>
__device__ __forceinline__ void put_partials(E (&part)[Q][WAVE], int lane, T... x) {
    static_assert(sizeof...(T) <= Q, "more partials than rows");
    int q = 0;
    ((part[q++][lane] = x), ...);
}

// ---- host: the argument checks the walks rest on; `op` and `name` go into the error text ---------------------------------------------
// the distance test's threshold: above r^2 by more than the roundings of d^2 and of the square root can move a pair
inline float pair_r2_test(float radius) { return (float)((double)radius * (double)radius * (1.0 + 1e-6)); }

// `count` walked items of `stride` floats: at least one, and indexed in 32 bits
inline int check_walk_count(const char *op, const char *name, int count, int stride) {
    if (count >= 1 && (int64_t)count * stride <= 0x7fffffffLL) return SNERF_OK;
    return fail(SNERF_E_BADARG, "%s: %s must be at least 1 and %d %s below 2^31", op, name, stride, name);
}

// blocks = the 64-lane chunks of n samples or rays, one workgroup each: a grid dimension
inline int chunk_blocks(const char *op, const char *name, int64_t n, int64_t &blocks) {
    blocks = (n + WAVE - 1) / WAVE;
    return blocks <= 0x7fffffffLL ? SNERF_OK : fail(SNERF_E_BADARG, "%s: %s too large", op, name);
}

}  // namespace snerf
