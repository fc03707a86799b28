// Vertex-attention warp of DynamicPipeline (models/dynamic_pipeline.py:53-74), forward and backward, without the [B, S, V]
// tensors of the reference.  For ray b, sample s (position p), vertex v (goal g_v, canonical c_v), r = warp_radius, T = temperature:
//   d_v = |p - g_v|      x_v = T max(r - d_v, 0)      a_v = (exp(x_v) - 1) / sum_u exp(x_u)      (utils.py:57-60, its max cancels)
//   warp = sum_v a_v (c_v - g_v)      warped = p + warp      sdirs = warped - o_b
// evaluated with the per-sample maximum m = max_v x_v taken out: a_v = (exp(x_v - m) - exp(-m)) / Z, Z = sum_u exp(x_u - m).
// A vertex outside the radius has x = 0: nothing in the numerator, exp(-m) in Z - so only the pairs inside the radius ("hits",
// rare: the radius is 1 cm on a 2 m body) ever meet sqrt or exp.  All other pairs cost the distance test: three subtractions,
// three products, two sums, one compare (VALU-bound, 9 instructions per pair).
//
// Mapping, all three kernels: lane = sample, a wave walks vertices with the walk of pair_walk.h.
//   forward          workgroup = (ray, 64-sample chunk); its 16 waves split the vertices, each keeps an online (m, sum, numerator)
//                    per lane; the partials meet in LDS and wave 0 combines them in wave order.  A 64-ray batch is 64 x 16 waves.
//   backward, verts  a wave owns 64 consecutive vertices of a ray and loops over the sample chunks; a vertex with a hit is summed
//                    over the lanes by the DPP scan (fixed order) and added into the accumulator of the lane that owns the vertex;
//                    the tile is written once, zeros included.  No atomics, no read-modify-write of global memory.
//   backward, samples  as the forward: workgroup = (ray, chunk), partial sums over vertex slices combined in LDS in wave order.
// Two calls give the same bits.  The backward reads m, Z and warp from the forward, so it is one pass per output.
#include "pair_walk.h"

namespace snerf {

constexpr int VW_WAVES = 16;    // waves of a (ray, sample chunk) workgroup: the vertex slices
constexpr int VW_BWD_WAVES = 4; // waves of a vertex-gradient workgroup: 64 vertices each

struct VwArgs {
    const float *samples, *goal, *canon, *ray_o;
    float *warp, *warped, *sdirs, *stats;
    int S, V, chunks;
    float radius, temperature, r2_test;
};

struct VwBwdArgs {
    const float *samples, *goal, *canon, *warp, *stats, *dw0, *dw1, *dw2;
    float *d_samples, *d_goal, *d_canon;
    int S, V, chunks, groups;
    float radius, temperature, r2_test;
};

__global__ __launch_bounds__(VW_WAVES * 64) void vertex_warp_fwd_kernel(VwArgs A) {
    __shared__ float part[VW_WAVES][6][WAVE];   // m, sum, hits, numerator xyz of every wave's vertex slice
    const int lane = lane_id(), wave = wave_index();
    const int64_t ray = blockIdx.x / A.chunks;
    const int chunk = (int)(blockIdx.x - ray * A.chunks);
    const int s = chunk * WAVE + lane;
    const bool valid = s < A.S;
    const int64_t sample = ray * A.S + tail_index(s, A.S, valid);
    const float px = A.samples[sample * 3 + 0], py = A.samples[sample * 3 + 1], pz = A.samples[sample * 3 + 2];
    const float *g = A.goal + ray * A.V * 3, *c = A.canon + ray * A.V * 3;
    const Slice sl = wave_slice(A.V, VW_WAVES, wave);
    float m = 0.f, sum = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f, hits = 0.f;
    radius_walk<false>(g, sl.lo, sl.hi, px, py, pz, A.r2_test, [&](int v, float gx, float gy, float gz, float, float, float, float d2) {
        if (d2 < A.r2_test) {   // (r2_test is a little above r^2: the exact decision is the one below)
            const float xr = A.radius - sqrtf(d2);
            if (xr > 0.f) {
                const float x = A.temperature * xr;
                if (x > m) {    // new maximum: everything so far shrinks by exp(m - x)
                    const float k = expf(m - x);
                    sum *= k;
                    n0 *= k;
                    n1 *= k;
                    n2 *= k;
                    m = x;
                }
                const float e = expf(x - m), t = e - expf(-m);
                sum += e;
                hits += 1.f;
                n0 += t * (c[v * 3 + 0] - gx);
                n1 += t * (c[v * 3 + 1] - gy);
                n2 += t * (c[v * 3 + 2] - gz);
            }
        }
    });
    put_partials(part[wave], lane, m, sum, hits, n0, n1, n2);
    __syncthreads();
    if (wave != 0) return;
    float M = 0.f;
    for (int w = 0; w < VW_WAVES; ++w) M = fmaxf(M, part[w][0][lane]);
    float Z = 0.f, nh = 0.f, w0 = 0.f, w1 = 0.f, w2 = 0.f;
    for (int w = 0; w < VW_WAVES; ++w) {
        const float k = expf(part[w][0][lane] - M);
        Z += part[w][1][lane] * k;
        nh += part[w][2][lane];
        w0 += part[w][3][lane] * k;
        w1 += part[w][4][lane] * k;
        w2 += part[w][5][lane] * k;
    }
    Z += ((float)A.V - nh) * expf(-M);   // the vertices outside the radius: exp(0 - M) each
    if (!valid) return;
    w0 /= Z;
    w1 /= Z;
    w2 /= Z;
    const float qx = px + w0, qy = py + w1, qz = pz + w2;
    const float *o = A.ray_o + ray * 3;
    float *wp = A.warp + sample * 3, *q = A.warped + sample * 3, *sd = A.sdirs + sample * 3;
    wp[0] = w0;
    wp[1] = w1;
    wp[2] = w2;
    q[0] = qx;
    q[1] = qy;
    q[2] = qz;
    sd[0] = qx - o[0];
    sd[1] = qy - o[1];
    sd[2] = qz - o[2];
    if (A.stats) {
        A.stats[sample * 2 + 0] = M;
        A.stats[sample * 2 + 1] = Z;
    }
}

// what the backward kernels read per sample: position, dW = d warp + d warped + d sdirs, dW . warp, m, Z, exp(-m)
struct VwSample {
    float px, py, pz, d0, d1, d2, dww, m, Z, em;
};
__device__ __forceinline__ VwSample vw_load_sample(const VwBwdArgs &A, int64_t sample) {
    VwSample q;
    q.px = A.samples[sample * 3 + 0];
    q.py = A.samples[sample * 3 + 1];
    q.pz = A.samples[sample * 3 + 2];
    q.d0 = q.d1 = q.d2 = 0.f;
    const float *dws[3] = {A.dw0, A.dw1, A.dw2};
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (dws[i]) {
            q.d0 += dws[i][sample * 3 + 0];
            q.d1 += dws[i][sample * 3 + 1];
            q.d2 += dws[i][sample * 3 + 2];
        }
    const float *wp = A.warp + sample * 3;
    q.dww = q.d0 * wp[0] + q.d1 * wp[1] + q.d2 * wp[2];
    q.m = A.stats[sample * 2 + 0];
    q.Z = A.stats[sample * 2 + 1];
    q.em = expf(-q.m);
    return q;
}

// d_canon[b,v] = sum_s a_sv dW_s;  d_goal[b,v] = -d_canon[b,v] + sum_s T dx_sv (p_s - g_v) / d_sv  with
// dx_sv = exp(x_sv - m_s) / Z_s (dW_s . (c_v - g_v) - dW_s . warp_s)  where x_sv > 0  (d x / d g = +T (p - g) / d)
__global__ __launch_bounds__(VW_BWD_WAVES * 64) void vertex_warp_bwd_vertices_kernel(VwBwdArgs A) {
    const int lane = lane_id(), wave = wave_index();
    const int64_t ray = blockIdx.x / A.groups;
    const int group = (int)(blockIdx.x - ray * A.groups);
    const int tile0 = (group * VW_BWD_WAVES + wave) * WAVE;
    if (tile0 >= A.V) return;   // wave-uniform; the kernel has no barrier
    const int nv = A.V - tile0 < WAVE ? A.V - tile0 : WAVE;
    const float *g = A.goal + (ray * A.V + tile0) * 3, *c = A.canon + (ray * A.V + tile0) * 3;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;   // of vertex tile0 + lane
    for (int chunk = 0; chunk < A.chunks; ++chunk) {
        const int s = chunk * WAVE + lane;
        const bool valid = s < A.S;
        const VwSample q = vw_load_sample(A, ray * A.S + tail_index(s, A.S, valid));
        radius_walk<true>(g, 0, nv, q.px, q.py, q.pz, A.r2_test, [&](int vi, float gx, float gy, float gz, float dx, float dy, float dz, float d2) {
            const bool near = valid && d2 < A.r2_test;
            if (__builtin_amdgcn_ballot_w64(near) == 0) return;   // wave-uniform
            float a = 0.f, k = 0.f;
            if (near) {
                const float d = sqrtf(d2), xr = A.radius - d;
                if (xr > 0.f) {
                    const float e = expf(A.temperature * xr - q.m);
                    const float wx = c[vi * 3 + 0] - gx, wy = c[vi * 3 + 1] - gy, wz = c[vi * 3 + 2] - gz;
                    a = (e - q.em) / q.Z;
                    const float dxv = (e / q.Z) * ((q.d0 * wx + q.d1 * wy + q.d2 * wz) - q.dww);
                    k = d > 0.f ? A.temperature * dxv / d : 0.f;   // (no gradient through a zero distance: torch.norm's convention)
                }
            }
            const float t0 = wave_sum(a * q.d0), t1 = wave_sum(a * q.d1), t2 = wave_sum(a * q.d2);
            const float u0 = wave_sum(k * dx), u1 = wave_sum(k * dy), u2 = wave_sum(k * dz);
            if (lane == vi) {
                c0 += t0;
                c1 += t1;
                c2 += t2;
                g0 += u0;
                g1 += u1;
                g2 += u2;
            }
        });
    }
    if (lane < nv) {
        float *dc = A.d_canon + (ray * A.V + tile0 + lane) * 3, *dg = A.d_goal + (ray * A.V + tile0 + lane) * 3;
        dc[0] = c0;
        dc[1] = c1;
        dc[2] = c2;
        dg[0] = g0 - c0;
        dg[1] = g1 - c1;
        dg[2] = g2 - c2;
    }
}

// d_samples[b,s] = -sum_v T dx_sv (p_s - g_v) / d_sv
__global__ __launch_bounds__(VW_WAVES * 64) void vertex_warp_bwd_samples_kernel(VwBwdArgs A) {
    __shared__ float part[VW_WAVES][3][WAVE];
    const int lane = lane_id(), wave = wave_index();
    const int64_t ray = blockIdx.x / A.chunks;
    const int chunk = (int)(blockIdx.x - ray * A.chunks);
    const int s = chunk * WAVE + lane;
    const bool valid = s < A.S;
    const int64_t sample = ray * A.S + tail_index(s, A.S, valid);
    const VwSample q = vw_load_sample(A, sample);
    const float *g = A.goal + ray * A.V * 3, *c = A.canon + ray * A.V * 3;
    const Slice sl = wave_slice(A.V, VW_WAVES, wave);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    radius_walk<false>(g, sl.lo, sl.hi, q.px, q.py, q.pz, A.r2_test, [&](int v, float gx, float gy, float gz, float dx, float dy, float dz, float d2) {
        if (d2 < A.r2_test) {
            const float d = sqrtf(d2), xr = A.radius - d;
            if (xr > 0.f && d > 0.f) {
                const float e = expf(A.temperature * xr - q.m);
                const float wx = c[v * 3 + 0] - gx, wy = c[v * 3 + 1] - gy, wz = c[v * 3 + 2] - gz;
                const float dxv = (e / q.Z) * ((q.d0 * wx + q.d1 * wy + q.d2 * wz) - q.dww);
                const float k = A.temperature * dxv / d;
                s0 += k * dx;
                s1 += k * dy;
                s2 += k * dz;
            }
        }
    });
    put_partials(part[wave], lane, s0, s1, s2);
    __syncthreads();
    if (wave != 0 || !valid) return;
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    for (int w = 0; w < VW_WAVES; ++w) {
        r0 += part[w][0][lane];
        r1 += part[w][1][lane];
        r2 += part[w][2][lane];
    }
    float *ds = A.d_samples + sample * 3;
    ds[0] = -r0;
    ds[1] = -r1;
    ds[2] = -r2;
}

// shared argument checks; returns 1 when there is nothing to do (B == 0)
static int vw_check(const char *what, int64_t B, int S, int V, float radius, float temperature, int64_t &chunks) {
    if (B < 0 || S < 1 || V < 1) return fail(SNERF_E_BADARG, "%s: need B >= 0, S >= 1 and V >= 1", what);
    if (!(radius > 0.f)) return fail(SNERF_E_BADARG, "%s: radius must be positive", what);
    if (!(temperature >= 0.f)) return fail(SNERF_E_BADARG, "%s: temperature must not be negative", what);
    chunks = ((int64_t)S + WAVE - 1) / WAVE;
    if (int rc = check_walk_count(what, "V", V, 3)) return rc;
    return B == 0 ? 1 : 0;
}

}  // namespace snerf

extern "C" int snerf_vertex_warp_fwd_f32(const float *samples, const float *goal, const float *canon, const float *ray_o, int64_t B,
                                         int S, int V, float radius, float temperature, float *warp, float *warped, float *sdirs,
                                         float *stats, snerf_stream_t stream) {
    using namespace snerf;
    int64_t chunks;
    if (int rc = vw_check("vertex_warp_fwd", B, S, V, radius, temperature, chunks)) return rc < 0 ? rc : SNERF_OK;
    if (!samples || !goal || !canon || !ray_o || !warp || !warped || !sdirs) return fail(SNERF_E_BADARG, "vertex_warp_fwd: null pointer");
    if (B * chunks > 0x7fffffffLL) return fail(SNERF_E_BADARG, "vertex_warp_fwd: B too large");
    VwArgs A{samples, goal, canon, ray_o, warp, warped, sdirs, stats, S, V, (int)chunks, radius, temperature, pair_r2_test(radius)};
    hipLaunchKernelGGL(vertex_warp_fwd_kernel, dim3((unsigned)(B * chunks)), dim3(VW_WAVES * 64), 0, (hipStream_t)stream, A);
    return check_launch("vertex_warp_fwd");
}

extern "C" int snerf_vertex_warp_bwd_f32(const float *samples, const float *goal, const float *canon, const float *warp,
                                         const float *stats, const float *d_warp, const float *d_warped, const float *d_sdirs,
                                         int64_t B, int S, int V, float radius, float temperature, float *d_samples, float *d_goal,
                                         float *d_canon, snerf_stream_t stream) {
    using namespace snerf;
    int64_t chunks;
    if (int rc = vw_check("vertex_warp_bwd", B, S, V, radius, temperature, chunks)) return rc < 0 ? rc : SNERF_OK;
    if (!samples || !goal || !canon || !warp || !stats || !d_goal || !d_canon) return fail(SNERF_E_BADARG, "vertex_warp_bwd: null pointer");
    if (!d_warp && !d_warped && !d_sdirs) return fail(SNERF_E_BADARG, "vertex_warp_bwd: no incoming gradient");
    const int64_t groups = ((int64_t)V + VW_BWD_WAVES * WAVE - 1) / (VW_BWD_WAVES * WAVE);
    if (B * chunks > 0x7fffffffLL || B * groups > 0x7fffffffLL) return fail(SNERF_E_BADARG, "vertex_warp_bwd: B too large");
    VwBwdArgs A{samples, goal, canon, warp, stats, d_warp, d_warped, d_sdirs, d_samples, d_goal, d_canon, S, V, (int)chunks, (int)groups,
                radius, temperature, pair_r2_test(radius)};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vertex_warp_bwd_vertices_kernel, dim3((unsigned)(B * groups)), dim3(VW_BWD_WAVES * 64), 0, s, A);
    if (d_samples) hipLaunchKernelGGL(vertex_warp_bwd_samples_kernel, dim3((unsigned)(B * chunks)), dim3(VW_WAVES * 64), 0, s, A);
    return check_launch("vertex_warp_bwd");
}
