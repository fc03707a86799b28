// Linear-attention warp of the image-wise model (solver/image_wise_solver.py:89-105), forward and backward: ONE body per image,
// shared by every ray of the batch, without the [B, S, V] tensors of the reference and without a [B, V, 3] copy of the body.
// For sample s of the flat N = B S (position p_s, ray s / S), vertex v (goal g_v, canonical c_v, w_v = c_v - g_v), r = warp_radius:
//   d_sv = |p_s - g_v|      x_sv = max(r - d_sv, 0)      D_s = sum_v x_sv + eps      warp_s = (sum_v x_sv w_v) / D_s
//   warped_s = p_s + warp_s      sdirs_s = warped_s - o_(s / S)
// No softmax, no temperature, no exponential: only the pairs inside the radius meet a square root.  All other pairs cost the
// fp32 distance test of radius_walk (pair_walk.h).
//
// Arithmetic: the pairs that pass the test ("hits", rare: the radius is 1 cm on a 2 m body) are evaluated in float64 from the fp32
// inputs - distance, x, the sums over the vertices and over the samples, the quotient - and every output is rounded to fp32 ONCE.
// The linear attention has no exponential to hide behind: a sample with one vertex in radius has warp = w x / (x + eps), and its
// gradient dW . (w - warp) / D cancels to eps / D of its operands, so fp32 intermediates cost three digits there.  stats carries
// D and warp in float64 to the backward for that reason.  The cost is on the hit path only; the walk itself is fp32.
//
// Mapping: lane = sample in the forward and the sample gradient, lane = sample with a wave per vertex tile in the vertex gradient.
//   forward          workgroup = one 64-sample chunk of the flat N; its 8 waves split the vertices, each keeps (sum x, sum x w)
//                    per lane; the partials meet in LDS and wave 0 adds them in wave order.
//   backward, verts  the reduction over ALL samples into one [V, 3] body.  Workgroup = (vertex tile group, sample slab); a wave owns
//                    64 consecutive vertices and loops over the 64-sample chunks of its slab; a vertex with a sample near it is
//                    summed over the lanes by the DPP scan (fixed order) and added into the accumulator of the lane that owns the
//                    vertex.  The tile's partial (d_canon, distance term) goes to workspace[slab][v][6], zeros included, and a
//                    second kernel adds the slabs in slab order.  The slab count depends on N alone (iw_slabs): the same inputs
//                    give the same bits on any device.  No atomics, no read-modify-write of global memory.
//   backward, samples  as the forward: partial sums over vertex slices combined in LDS in wave order.
// The backward reads D and warp from the forward (stats), so it is one pass per output.
#include "pair_walk.h"

namespace snerf {

constexpr int IW_WAVES = 8;           // waves of a sample-chunk workgroup: the vertex slices (8: 256 VGPRs for the float64 hit path)
constexpr int IW_BWD_WAVES = 4;       // waves of a vertex-gradient workgroup: 64 vertices each
constexpr int IW_MAX_SLABS = 64;      // sample slabs of the vertex gradient, at most ...
constexpr int IW_MIN_SLAB_CHUNKS = 8; // ... of at least this many 64-sample chunks each (but the last)

// The sample slabs of the vertex gradient: `per` consecutive chunks each, the last one possibly shorter, never empty.
// 128 x 128 x 64 samples: 16384 chunks, 64 slabs of 256 -> 64 x 108 waves for 6890 vertices (6.75 per SIMD of a 1024-SIMD device);
// a 64-ray x 64-sample batch: 64 chunks, 8 slabs of 8.
struct Slabs {
    int64_t per, count;
};
constexpr __host__ __device__ Slabs iw_slabs(int64_t chunks) {
    const int64_t even = (chunks + IW_MAX_SLABS - 1) / IW_MAX_SLABS;
    const int64_t per = even > IW_MIN_SLAB_CHUNKS ? even : IW_MIN_SLAB_CHUNKS;
    return {per, (chunks + per - 1) / per};
}
static_assert(iw_slabs(1).count == 1 && iw_slabs(8).count == 1 && iw_slabs(9).count == 2 && iw_slabs(64).count == 8 &&
                  iw_slabs(16384).count == 64 && iw_slabs(16385).per == 257 && iw_slabs(16385).count == 64,
              "iw_slabs: at most IW_MAX_SLABS slabs, none empty");

struct IwArgs {
    const float *samples, *goal, *canon, *ray_o;
    float *warp, *warped, *sdirs;
    double *stats;
    int64_t N;
    int S, V;
    double radius, eps;
    float r2_test;
};

struct IwBwdArgs {
    const float *samples, *goal, *canon, *dw0, *dw1, *dw2;
    const double *stats;
    float *d_samples, *d_goal, *d_canon;
    double *partial;
    int64_t N, chunks, slab_chunks;
    int V, slabs;
    double radius;
    float r2_test;
};

// x = r - |p - g| of a pair that passed the fp32 test, in float64 from the fp32 coordinates (the differences are exact there);
// d gets the distance.  The exact decision is the caller's x > 0 (r2_test is a little above r^2).
__device__ __forceinline__ double iw_x(double radius, float px, float py, float pz, float gx, float gy, float gz, double &ex, double &ey,
                                       double &ez, double &d) {
    ex = (double)px - (double)gx;
    ey = (double)py - (double)gy;
    ez = (double)pz - (double)gz;
    d = sqrt(ex * ex + ey * ey + ez * ez);
    return radius - d;
}

__global__ __launch_bounds__(IW_WAVES * 64) void image_warp_fwd_kernel(IwArgs A) {
    __shared__ double part[IW_WAVES][4][WAVE];   // sum x, sum x w (xyz) of every wave's vertex slice
    const int lane = lane_id(), wave = wave_index();
    const int64_t s = (int64_t)blockIdx.x * WAVE + lane;
    const bool valid = s < A.N;
    const int64_t sample = tail_index(s, A.N, valid);
    const float px = A.samples[sample * 3 + 0], py = A.samples[sample * 3 + 1], pz = A.samples[sample * 3 + 2];
    const float *c = A.canon;
    const Slice sl = wave_slice(A.V, IW_WAVES, wave);
    double sum = 0., n0 = 0., n1 = 0., n2 = 0.;
    radius_walk<false>(A.goal, sl.lo, sl.hi, px, py, pz, A.r2_test, [&](int v, float gx, float gy, float gz, float, float, float, float d2) {
        if (d2 < A.r2_test) {
            double ex, ey, ez, d;
            const double x = iw_x(A.radius, px, py, pz, gx, gy, gz, ex, ey, ez, d);
            if (x > 0.) {
                sum += x;
                n0 += x * ((double)c[v * 3 + 0] - (double)gx);
                n1 += x * ((double)c[v * 3 + 1] - (double)gy);
                n2 += x * ((double)c[v * 3 + 2] - (double)gz);
            }
        }
    });
    put_partials(part[wave], lane, sum, n0, n1, n2);
    __syncthreads();
    if (wave != 0 || !valid) return;
    double D = 0., w0 = 0., w1 = 0., w2 = 0.;
    for (int w = 0; w < IW_WAVES; ++w) {
        D += part[w][0][lane];
        w0 += part[w][1][lane];
        w1 += part[w][2][lane];
        w2 += part[w][3][lane];
    }
    D += A.eps;
    w0 /= D;
    w1 /= D;
    w2 /= D;
    const float f0 = (float)w0, f1 = (float)w1, f2 = (float)w2;
    const float qx = px + f0, qy = py + f1, qz = pz + f2;   // (fp32 sums of the fp32 outputs: warped = samples + warp bit for bit)
    const float *o = A.ray_o + (sample / A.S) * 3;
    float *wp = A.warp + sample * 3, *q = A.warped + sample * 3, *sd = A.sdirs + sample * 3;
    wp[0] = f0;
    wp[1] = f1;
    wp[2] = f2;
    q[0] = qx;
    q[1] = qy;
    q[2] = qz;
    sd[0] = qx - o[0];
    sd[1] = qy - o[1];
    sd[2] = qz - o[2];
    if (A.stats) {
        double *st = A.stats + sample * 4;
        st[0] = D;
        st[1] = w0;
        st[2] = w1;
        st[3] = w2;
    }
}

// what the backward kernels read per sample: position, dW = d warp + d warped + d sdirs, dW . warp, D
struct IwSample {
    float px, py, pz;
    double d0, d1, d2, dww, D;
};
__device__ __forceinline__ IwSample iw_load_sample(const IwBwdArgs &A, int64_t sample) {
    IwSample q;
    q.px = A.samples[sample * 3 + 0];
    q.py = A.samples[sample * 3 + 1];
    q.pz = A.samples[sample * 3 + 2];
    q.d0 = q.d1 = q.d2 = 0.;
    const float *dws[3] = {A.dw0, A.dw1, A.dw2};
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (dws[i]) {
            q.d0 += (double)dws[i][sample * 3 + 0];
            q.d1 += (double)dws[i][sample * 3 + 1];
            q.d2 += (double)dws[i][sample * 3 + 2];
        }
    const double *st = A.stats + sample * 4;
    q.D = st[0];
    q.dww = q.d0 * st[1] + q.d1 * st[2] + q.d2 * st[3];
    return q;
}

// partial[slab][v] = (sum_s (x_sv / D_s) dW_s,  sum_s dx_sv (p_s - g_v) / d_sv) over the samples s of the slab, with
// dx_sv = (dW_s . w_v - dW_s . warp_s) / D_s  where x_sv > 0   (d x / d g = +(p - g) / d)
__global__ __launch_bounds__(IW_BWD_WAVES * 64) void image_warp_bwd_vertices_kernel(IwBwdArgs A) {
    const int lane = lane_id(), wave = wave_index();
    const int slab = blockIdx.y;
    const int tile0 = ((int)blockIdx.x * IW_BWD_WAVES + wave) * WAVE;
    if (tile0 >= A.V) return;   // wave-uniform; the kernel has no barrier
    const int nv = A.V - tile0 < WAVE ? A.V - tile0 : WAVE;
    const float *g = A.goal + (int64_t)tile0 * 3, *c = A.canon + (int64_t)tile0 * 3;
    const int64_t chunk0 = slab * A.slab_chunks;
    const int64_t chunk1 = chunk0 + A.slab_chunks < A.chunks ? chunk0 + A.slab_chunks : A.chunks;
    double c0 = 0., c1 = 0., c2 = 0., g0 = 0., g1 = 0., g2 = 0.;   // of vertex tile0 + lane
    for (int64_t chunk = chunk0; chunk < chunk1; ++chunk) {
        const int64_t s = chunk * WAVE + lane;
        const bool valid = s < A.N;
        const IwSample q = iw_load_sample(A, tail_index(s, A.N, valid));
        radius_walk<true>(g, 0, nv, q.px, q.py, q.pz, A.r2_test, [&](int vi, float gx, float gy, float gz, float, float, float, float d2) {
            const bool near = valid && d2 < A.r2_test;
            if (__builtin_amdgcn_ballot_w64(near) == 0) return;   // wave-uniform
            double a = 0., k = 0., ex = 0., ey = 0., ez = 0.;
            if (near) {
                double d;
                const double x = iw_x(A.radius, q.px, q.py, q.pz, gx, gy, gz, ex, ey, ez, d);
                if (x > 0.) {
                    const double wx = (double)c[vi * 3 + 0] - (double)gx, wy = (double)c[vi * 3 + 1] - (double)gy,
                                 wz = (double)c[vi * 3 + 2] - (double)gz;
                    a = x / q.D;
                    const double dxv = ((q.d0 * wx + q.d1 * wy + q.d2 * wz) - q.dww) / q.D;
                    k = d > 0. ? dxv / d : 0.;   // (no gradient through a zero distance: torch.norm's convention)
                }
            }
            const double t0 = wave_sum(a * q.d0), t1 = wave_sum(a * q.d1), t2 = wave_sum(a * q.d2);
            const double u0 = wave_sum(k * ex), u1 = wave_sum(k * ey), u2 = wave_sum(k * ez);
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
        double *p = A.partial + ((int64_t)slab * A.V + tile0 + lane) * 6;
        p[0] = c0;
        p[1] = c1;
        p[2] = c2;
        p[3] = g0;
        p[4] = g1;
        p[5] = g2;
    }
}

// d_canon[v] = sum over the slabs, in slab order, of the first half; d_goal[v] = (the same sum of the distance term) - d_canon[v],
// each rounded to fp32 once.  One thread per (vertex, component).
__global__ __launch_bounds__(256) void image_warp_bwd_reduce_kernel(IwBwdArgs A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)A.V * 3) return;
    const int64_t v = i / 3;
    const int j = (int)(i - v * 3);
    double dc = 0., dg = 0.;
    for (int slab = 0; slab < A.slabs; ++slab) {
        const double *p = A.partial + ((int64_t)slab * A.V + v) * 6;
        dc += p[j];
        dg += p[3 + j];
    }
    A.d_canon[i] = (float)dc;
    A.d_goal[i] = (float)(dg - dc);
}

// d_samples[s] = d warped_s + d sdirs_s - sum_v dx_sv (p_s - g_v) / d_sv: the identity paths of the two derived outputs included
__global__ __launch_bounds__(IW_WAVES * 64) void image_warp_bwd_samples_kernel(IwBwdArgs A) {
    __shared__ double part[IW_WAVES][3][WAVE];
    const int lane = lane_id(), wave = wave_index();
    const int64_t s = (int64_t)blockIdx.x * WAVE + lane;
    const bool valid = s < A.N;
    const int64_t sample = tail_index(s, A.N, valid);
    const IwSample q = iw_load_sample(A, sample);
    const float *c = A.canon;
    const Slice sl = wave_slice(A.V, IW_WAVES, wave);
    double s0 = 0., s1 = 0., s2 = 0.;
    radius_walk<false>(A.goal, sl.lo, sl.hi, q.px, q.py, q.pz, A.r2_test, [&](int v, float gx, float gy, float gz, float, float, float, float d2) {
        if (d2 < A.r2_test) {
            double ex, ey, ez, d;
            const double x = iw_x(A.radius, q.px, q.py, q.pz, gx, gy, gz, ex, ey, ez, d);
            if (x > 0. && d > 0.) {
                const double wx = (double)c[v * 3 + 0] - (double)gx, wy = (double)c[v * 3 + 1] - (double)gy,
                             wz = (double)c[v * 3 + 2] - (double)gz;
                const double k = ((q.d0 * wx + q.d1 * wy + q.d2 * wz) - q.dww) / q.D / d;
                s0 += k * ex;
                s1 += k * ey;
                s2 += k * ez;
            }
        }
    });
    put_partials(part[wave], lane, s0, s1, s2);
    __syncthreads();
    if (wave != 0 || !valid) return;
    double r[3] = {0., 0., 0.};
    for (int w = 0; w < IW_WAVES; ++w) {
        r[0] += part[w][0][lane];
        r[1] += part[w][1][lane];
        r[2] += part[w][2][lane];
    }
    float *ds = A.d_samples + sample * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double id = 0.;
        if (A.dw1) id += (double)A.dw1[sample * 3 + j];
        if (A.dw2) id += (double)A.dw2[sample * 3 + j];
        ds[j] = (float)(id - r[j]);
    }
}

// shared argument checks; returns 1 when there is nothing to do (B == 0); N = B S and its 64-sample chunks otherwise
static int iw_check(const char *what, int64_t B, int S, int V, double radius, int64_t &N, int64_t &chunks) {
    if (B < 0 || S < 1 || V < 1) return fail(SNERF_E_BADARG, "%s: need B >= 0, S >= 1 and V >= 1", what);
    if (!(radius > 0.)) return fail(SNERF_E_BADARG, "%s: radius must be positive", what);
    if (int rc = check_walk_count(what, "V", V, 3)) return rc;
    if (B > 0x7fffffffLL * WAVE / S) return fail(SNERF_E_BADARG, "%s: B too large", what);
    N = B * S;
    if (int rc = chunk_blocks(what, "B", N, chunks)) return rc;
    return B == 0 ? 1 : 0;
}

static int64_t iw_workspace_bytes(int64_t chunks, int V) { return iw_slabs(chunks).count * V * 6 * (int64_t)sizeof(double); }

}  // namespace snerf

extern "C" int snerf_image_warp_fwd_f32(const float *samples, const float *goal, const float *canon, const float *ray_o, int64_t B,
                                        int S, int V, double radius, double eps, float *warp, float *warped, float *sdirs,
                                        double *stats, snerf_stream_t stream) {
    using namespace snerf;
    int64_t N = 0, chunks = 0;
    const int rc = iw_check("image_warp_fwd", B, S, V, radius, N, chunks);
    if (rc < 0) return rc;
    if (!(eps >= 0.)) return fail(SNERF_E_BADARG, "image_warp_fwd: eps must not be negative");
    if (rc) return SNERF_OK;
    if (!samples || !goal || !canon || !ray_o || !warp || !warped || !sdirs) return fail(SNERF_E_BADARG, "image_warp_fwd: null pointer");
    if ((uintptr_t)stats & 7) return fail(SNERF_E_ALIGN, "image_warp_fwd: stats must be 8-byte aligned");
    IwArgs A{samples, goal, canon, ray_o, warp, warped, sdirs, stats, N, S, V, radius, eps, pair_r2_test((float)radius)};
    hipLaunchKernelGGL(image_warp_fwd_kernel, dim3((unsigned)chunks), dim3(IW_WAVES * 64), 0, (hipStream_t)stream, A);
    return check_launch("image_warp_fwd");
}

extern "C" int64_t snerf_image_warp_bwd_workspace_bytes(int64_t N, int V) {
    using namespace snerf;
    int64_t chunks = 0;
    if (N < 0) return fail(SNERF_E_BADARG, "image_warp_bwd_workspace_bytes: N must not be negative"), -1;
    if (check_walk_count("image_warp_bwd_workspace_bytes", "V", V, 3) || chunk_blocks("image_warp_bwd_workspace_bytes", "N", N, chunks))
        return -1;
    return iw_workspace_bytes(chunks, V);
}

extern "C" int snerf_image_warp_bwd_f32(const float *samples, const float *goal, const float *canon, const double *stats,
                                        const float *d_warp, const float *d_warped, const float *d_sdirs, int64_t B, int S, int V,
                                        double radius, void *workspace, int64_t workspace_bytes, float *d_samples, float *d_goal,
                                        float *d_canon, snerf_stream_t stream) {
    using namespace snerf;
    int64_t N = 0, chunks = 0;
    if (int rc = iw_check("image_warp_bwd", B, S, V, radius, N, chunks)) return rc < 0 ? rc : SNERF_OK;
    if (!samples || !goal || !canon || !stats || !d_goal || !d_canon) return fail(SNERF_E_BADARG, "image_warp_bwd: null pointer");
    if (!d_warp && !d_warped && !d_sdirs) return fail(SNERF_E_BADARG, "image_warp_bwd: no incoming gradient");
    if (!workspace || workspace_bytes < iw_workspace_bytes(chunks, V))
        return fail(SNERF_E_BADARG, "image_warp_bwd: workspace missing or smaller than snerf_image_warp_bwd_workspace_bytes()");
    if (((uintptr_t)workspace | (uintptr_t)stats) & 7) return fail(SNERF_E_ALIGN, "image_warp_bwd: stats and workspace must be 8-byte aligned");
    const Slabs sl = iw_slabs(chunks);
    const int64_t groups = ((int64_t)V + IW_BWD_WAVES * WAVE - 1) / (IW_BWD_WAVES * WAVE);
    IwBwdArgs A{samples, goal, canon, d_warp, d_warped, d_sdirs, stats, d_samples, d_goal, d_canon, (double *)workspace,
                N, chunks, sl.per, V, (int)sl.count, radius, pair_r2_test((float)radius)};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(image_warp_bwd_vertices_kernel, dim3((unsigned)groups, (unsigned)sl.count), dim3(IW_BWD_WAVES * 64), 0, s, A);
    hipLaunchKernelGGL(image_warp_bwd_reduce_kernel, dim3((unsigned)(((int64_t)V * 3 + 255) / 256)), dim3(256), 0, s, A);
    if (d_samples) hipLaunchKernelGGL(image_warp_bwd_samples_kernel, dim3((unsigned)chunks), dim3(IW_WAVES * 64), 0, s, A);
    return check_launch("image_warp_bwd");
}
