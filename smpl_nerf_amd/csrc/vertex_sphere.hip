// The deterministic ("true") warp of the vertex_sphere model (datasets/vertex_sphere_dataset.py:128-159) without its
// [h w, 6890, 3] distance tensors.  For the sample p, the goal vertices g_v, the canonical vertices c_v and r = vertex_sphere_radius:
//   d_v = sqrtf(|p - g_v|^2), the square summed as (dx dx + dy dy) + dz dz
//   w(d) = 1 where d < r, 0 where d > r and d itself where d == r   (the reference's two masked assignments leave an equal distance
//          in place: quirk Q12)
//   by_mean = 0 (:147-158)   i = argmin_v d_v (lowest index on a tie, as torch.argmin)   warp = w(d_i) (c_i - g_i)   count = (d_i < r)
//   by_mean = 1 (:134-145)   warp = sum_v w(d_v) (c_v - g_v) / (sum_v w(d_v) + 1e-10)    count = #{v: d_v < r}     nearest = argmin
// The warp is data of the batch (data[4]), not a function the loss is differentiated through: there is no backward.
//
// Mapping (pair_walk.h; the four-per-wait loop is written out here, see the kernel): workgroup = 64-sample chunk, lane = sample; its
// 16 waves split the vertices and read them at wave-uniform addresses through the scalar cache, four per wait.  A pair costs the
// squared distance and one test (VALU-bound, about 10 instructions); the square root is taken only where the squared distance is
// below the smallest seen so far (the argmin is decided on the roots: two squares can share a root, and then the lower index keeps
// it) or below a threshold a little above r^2 (the weight is decided on the root).  The per-wave partials meet in LDS and wave 0
// combines them in wave order: the sums run in a fixed order, no atomics, two calls give the same bits.
#include <math.h>

#include "pair_walk.h"

namespace snerf {

constexpr int VS_WAVES = 16;

struct VsArgs {
    const float *samples, *goal, *canon;
    float *warp;
    int32_t *nearest, *count;
    int64_t n;
    int V;
    float radius, r2_test;
};

template <bool MEAN>
__global__ __launch_bounds__(VS_WAVES * 64) void vertex_sphere_warp_kernel(VsArgs A) {
    __shared__ float part[VS_WAVES][MEAN ? 7 : 2][WAVE];   // best d, best index; count, sum of weights, numerator xyz
    const int lane = lane_id(), wave = wave_index();
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool valid = i < A.n;
    const int64_t ii = tail_index(i, A.n, valid);
    const float px = A.samples[ii * 3 + 0], py = A.samples[ii * 3 + 1], pz = A.samples[ii * 3 + 2];
    const float *g = A.goal, *c = A.canon;
    const Slice sl = wave_slice(A.V, VS_WAVES, wave);
    float best_d2 = INFINITY, best_d = INFINITY, cnt = 0.f, sw = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
    int best_i = sl.lo < A.V ? sl.lo : 0;   // (an empty slice: a vertex that exists; its best_d = inf never wins)

    auto vertex = [&](int v, float gx, float gy, float gz, float d2) {
        if (d2 < best_d2) {   // a smaller square: its root is smaller or the same, and only a smaller one takes the place
            const float d = sqrtf(d2);
            if (d < best_d) {
                best_d = d;
                best_i = v;
            }
            best_d2 = d2;
        }
        if (MEAN && d2 < A.r2_test) {   // (r2_test is a little above r^2: the weight is decided on the root)
            const float d = sqrtf(d2);
            const float w = d < A.radius ? 1.f : (d > A.radius ? 0.f : d);
            cnt += d < A.radius ? 1.f : 0.f;
            sw += w;
            n0 += w * (c[v * 3 + 0] - gx);
            n1 += w * (c[v * 3 + 1] - gy);
            n2 += w * (c[v * 3 + 2] - gz);
        }
    };

    // Its own four-per-wait loop, not walk4: with the test of four in a lambda the mean-mode kernel measured 1.0 % slower on an MI355X.
    int v = sl.lo;
    for (; v + 4 <= sl.hi; v += 4) {
        float t[12], d2[4];
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = g[v * 3 + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) d2[j] = dist2(px - t[3 * j], py - t[3 * j + 1], pz - t[3 * j + 2]);
        const float m = fminf(fminf(d2[0], d2[1]), fminf(d2[2], d2[3]));   // one test of four: the running minimum or the weight's threshold
        if (m < best_d2 || (MEAN && m < A.r2_test)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) vertex(v + j, t[3 * j], t[3 * j + 1], t[3 * j + 2], d2[j]);
        }
    }
    for (; v < sl.hi; ++v) {
        const float gx = g[v * 3 + 0], gy = g[v * 3 + 1], gz = g[v * 3 + 2];
        vertex(v, gx, gy, gz, dist2(px - gx, py - gy, pz - gz));
    }

    const float best_bits = __builtin_bit_cast(float, best_i);
    if constexpr (MEAN) put_partials(part[wave], lane, best_d, best_bits, cnt, sw, n0, n1, n2);
    else put_partials(part[wave], lane, best_d, best_bits);
    __syncthreads();
    if (wave != 0 || !valid) return;
    for (int w = 1; w < VS_WAVES; ++w) {   // in wave order = in vertex order: the lowest index keeps a tie
        const float d = part[w][0][lane];
        if (d < best_d) {
            best_d = d;
            best_i = __builtin_bit_cast(int, part[w][1][lane]);
        }
        if (MEAN) {
            cnt += part[w][2][lane];
            sw += part[w][3][lane];
            n0 += part[w][4][lane];
            n1 += part[w][5][lane];
            n2 += part[w][6][lane];
        }
    }
    float *wp = A.warp + i * 3;
    if (MEAN) {
        const float den = sw + 1e-10f;
        wp[0] = n0 / den;
        wp[1] = n1 / den;
        wp[2] = n2 / den;
    } else {
        const float w = best_d < A.radius ? 1.f : (best_d > A.radius ? 0.f : best_d);
        cnt = best_d < A.radius ? 1.f : 0.f;
        wp[0] = w * (c[best_i * 3 + 0] - g[best_i * 3 + 0]);
        wp[1] = w * (c[best_i * 3 + 1] - g[best_i * 3 + 1]);
        wp[2] = w * (c[best_i * 3 + 2] - g[best_i * 3 + 2]);
    }
    if (A.nearest) A.nearest[i] = best_i;
    if (A.count) A.count[i] = (int32_t)cnt;
}

}  // namespace snerf

extern "C" int snerf_vertex_sphere_warp_f32(const float *samples, const float *goal, const float *canon, int64_t n, int V, float radius,
                                            int by_mean, float *warp, int32_t *nearest, int32_t *count, snerf_stream_t stream) {
    using namespace snerf;
    if (n < 0) return fail(SNERF_E_BADARG, "vertex_sphere_warp: n must not be negative");
    if (int rc = check_walk_count("vertex_sphere_warp", "V", V, 3)) return rc;
    if (!(radius > 0.f) || !(radius <= 3.4028234663852886e38f)) return fail(SNERF_E_BADARG, "vertex_sphere_warp: radius must be finite and positive");
    if (n == 0) return SNERF_OK;
    if (!samples || !goal || !canon || !warp) return fail(SNERF_E_BADARG, "vertex_sphere_warp: null pointer (samples, goal, canon, warp)");
    int64_t blocks;
    if (int rc = chunk_blocks("vertex_sphere_warp", "n", n, blocks)) return rc;
    VsArgs A{samples, goal, canon, warp, nearest, count, n, V, radius, pair_r2_test(radius)};
    hipStream_t s = (hipStream_t)stream;
    if (by_mean) hipLaunchKernelGGL(vertex_sphere_warp_kernel<true>, dim3((unsigned)blocks), dim3(VS_WAVES * 64), 0, s, A);
    else hipLaunchKernelGGL(vertex_sphere_warp_kernel<false>, dim3((unsigned)blocks), dim3(VS_WAVES * 64), 0, s, A);
    return check_launch("vertex_sphere_warp");
}
