// snerf_ray_maps_fwd_f32 / snerf_ray_maps_bwd_f32 - the other pictures of a ray march: opacity, expected depth and expected
// point of every ray, from the per-sample alpha a compositing returned (utils.py:184, :187; include/smplnerf.h "ray maps").
//
//   t_i = z_i                              or   ((p_i - o) . d) / (d . d)  in fp64 (0 where d . d == 0)
//   u_i = fl32(fl32(1 - alpha_i) + 1e-10f)                                     (composite.hip: the forward's `om`)
//   T_i = prod_{j<i} u_j   in fp64 ;  w_i = fl32(alpha_i * fl32(T_i))          (the bits snerf_composite_fwd_f32 stores)
//   acc = sum w_i ;  depth = sum w_i t_i ;  point = sum w_i p_i                (fp64 sums, rounded once)
//
// HBM-bound streaming: 4 + 4 (z) or 4 + 12 (pts) bytes per sample and 24 + 8 .. 20 per ray.  One 64-lane wavefront owns a ray
// and walks it in chunks of 64 samples: alpha and z are 256 B wave loads; the points of a chunk are 768 contiguous bytes, read
// as three 256 B wave loads into a per-wave LDS row and taken from there three floats per lane (a stride of 3 dwords meets
// every bank once per 32 lanes).  The transmittance is composite.hip's fp64 wave prefix product with a scalar carry.
#include "snerf_common.h"

namespace snerf {

constexpr int RM_THREADS = 256;                 // 4 rays per workgroup
constexpr int RM_WAVES = RM_THREADS / WAVE;
constexpr int RM_MAX_CHUNKS = 64;               // N <= 4096, the compositing backward's limit

// what a lane knows of its sample
struct RmSample {
    float a;        // alpha (0 past the end of the ray)
    double u;       // the transmittance factor (1 past the end)
    double t;       // the sample parameter
    double px, py, pz;
};

// The ray's o, d as fp64 and 1 / (d . d) replaced by a flag: t = ((p - o) . d) / dd, 0 where dd == 0.
struct RmRay {
    double ox, oy, oz, dx, dy, dz, dd;
};

__device__ __forceinline__ RmRay rm_ray(const float *__restrict__ o, const float *__restrict__ d, int64_t ray) {
    RmRay r;
    r.ox = (double)o[ray * 3 + 0], r.oy = (double)o[ray * 3 + 1], r.oz = (double)o[ray * 3 + 2];
    r.dx = (double)d[ray * 3 + 0], r.dy = (double)d[ray * 3 + 1], r.dz = (double)d[ray * 3 + 2];
    r.dd = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    return r;
}

// Sample c0 + lane of the ray at `base`.  PTS: the chunk's points go through s_p (this wave's 192 floats); the caller's loop may
// call this again at once - the fence in front of the stores orders them behind the previous chunk's reads.
template <bool PTS>
__device__ __forceinline__ RmSample rm_sample(const float *__restrict__ alpha, const float *__restrict__ z,
                                              const float *__restrict__ pts, const RmRay &ray, int64_t base, int c0, int N,
                                              int lane, float *s_p) {
    const int i = c0 + lane;
    const bool ok = i < N;
    RmSample s;
    s.a = ok ? alpha[base + i] : 0.f;
    s.u = ok ? (double)__fadd_rn(__fsub_rn(1.0f, s.a), 1e-10f) : 1.0;
    s.t = s.px = s.py = s.pz = 0.0;
    if constexpr (PTS) {
        const int cnt = 3 * min(WAVE, N - c0);          // floats of this chunk: 1 .. 192
        const float *src = pts + (base + c0) * 3;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int j = lane + k * WAVE;
            if (j < cnt) s_p[j] = src[j];
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (ok) {
            s.px = (double)s_p[3 * lane + 0], s.py = (double)s_p[3 * lane + 1], s.pz = (double)s_p[3 * lane + 2];
            if (ray.dd != 0.0)
                s.t = ((s.px - ray.ox) * ray.dx + (s.py - ray.oy) * ray.dy + (s.pz - ray.oz) * ray.dz) / ray.dd;
        }
    } else {
        if (ok) s.t = (double)z[base + i];
    }
    return s;
}

template <bool PTS>
__global__ __launch_bounds__(RM_THREADS) void ray_maps_fwd_kernel(
    const float *__restrict__ alpha, const float *__restrict__ z, const float *__restrict__ pts, const float *__restrict__ o,
    const float *__restrict__ d, int64_t B, int N, float *__restrict__ acc_out, float *__restrict__ depth_out,
    float *__restrict__ point_out) {
    __shared__ float s_pts[PTS ? RM_WAVES : 1][PTS ? 3 * WAVE : 1];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * RM_WAVES + wave;
    if (ray >= B) return;  // wave-uniform
    const int64_t base = ray * N;
    RmRay rr = {};
    if constexpr (PTS) rr = rm_ray(o, d, ray);

    double carry = 1.0;  // product of u over all previous chunks
    double acc = 0.0, dep = 0.0, qx = 0.0, qy = 0.0, qz = 0.0;
    for (int c0 = 0; c0 < N; c0 += WAVE) {
        const RmSample s = rm_sample<PTS>(alpha, z, pts, rr, base, c0, N, lane, s_pts[PTS ? wave : 0]);
        const double incl = wave_scan_mul(s.u);
        const double excl = wave_shift_up1(incl, 1.0);
        const float T = (float)(carry * excl);          // composite_fwd_kernel, operation by operation
        carry *= wave_last(incl);
        const double w = c0 + lane < N ? (double)__fmul_rn(s.a, T) : 0.0;   // (past the end a = 0, but T may be a NaN)
        acc += w;
        dep += w * s.t;
        if constexpr (PTS) {
            qx += w * s.px;
            qy += w * s.py;
            qz += w * s.pz;
        }
    }
    acc = wave_sum(acc);
    dep = wave_sum(dep);
    if constexpr (PTS) {
        if (point_out) {   // kernel-uniform
            qx = wave_sum(qx);
            qy = wave_sum(qy);
            qz = wave_sum(qz);
        }
    }
    if (lane == 0) {
        acc_out[ray] = (float)acc;
        depth_out[ray] = (float)dep;
        if constexpr (PTS) {
            if (point_out) {
                point_out[ray * 3 + 0] = (float)qx;
                point_out[ray * 3 + 1] = (float)qy;
                point_out[ray * 3 + 2] = (float)qz;
            }
        }
    }
}

// ---- backward: (d acc [B], d depth [B], d point [B,3]) -> d alpha [B,N] -----------------------------------------------------
// With G_i = d acc + d depth * t_i + <d point, p_i> (everything that arrives at w_i), w_i = alpha_i T_i and d u / d alpha = -1:
//   d alpha_k = T_k G_k - S_k / u_k ,   S_k = sum_{i>k} w_i G_i                   (T_i holds u_k for every i > k)
// all in fp64, rounded once.  S_k is an EXCLUSIVE reverse scan, shifted: "inclusive minus own term" leaves an absolute error of
// an ulp of w_k G_k in S_k, which the quotient multiplies by 1e10 where alpha_k = 1 (u_k = 1e-10: an opaque body).  The lanes of
// a chunk are reversed (lane <-> 63 - lane), scanned forward with the DPP scans and shifted up by one; the later chunks' sum is
// a scalar carry.  A forward sweep over alpha alone leaves the transmittance carried into every chunk in LDS, as
// composite_bwd_kernel has it.  HBM: alpha is read twice, z / pts once, d alpha written once.
template <bool PTS>
__global__ __launch_bounds__(RM_THREADS) void ray_maps_bwd_kernel(
    const float *__restrict__ alpha, const float *__restrict__ z, const float *__restrict__ pts, const float *__restrict__ o,
    const float *__restrict__ d, int64_t B, int N, const float *__restrict__ d_acc, const float *__restrict__ d_depth,
    const float *__restrict__ d_point, float *__restrict__ d_alpha) {
    __shared__ double s_carry[RM_WAVES][RM_MAX_CHUNKS];
    __shared__ float s_pts[PTS ? RM_WAVES : 1][PTS ? 3 * WAVE : 1];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * RM_WAVES + wave;
    if (ray >= B) return;  // wave-uniform
    const int64_t base = ray * N;
    RmRay rr = {};
    if constexpr (PTS) rr = rm_ray(o, d, ray);
    const double ga = d_acc ? (double)d_acc[ray] : 0.0;
    const double gd = d_depth ? (double)d_depth[ray] : 0.0;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if constexpr (PTS) {
        if (d_point) gx = (double)d_point[ray * 3 + 0], gy = (double)d_point[ray * 3 + 1], gz = (double)d_point[ray * 3 + 2];
    }

    // forward sweep: the transmittance carried into each chunk (every lane keeps the value; lane 0 stores it)
    const int nchunk = (N + WAVE - 1) / WAVE;      // <= RM_MAX_CHUNKS: checked on the host
    double carry = 1.0;
    for (int c = 0; c < nchunk; ++c) {
        if (lane == 0) s_carry[wave][c] = carry;
        const int i = c * WAVE + lane;
        const double u = i < N ? (double)__fadd_rn(__fsub_rn(1.0f, alpha[base + i]), 1e-10f) : 1.0;
        carry *= wave_last(wave_scan_mul(u));
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");

    // reverse sweep
    double suffix = 0.0;   // sum of w_i G_i over the chunks behind this one
    for (int c = nchunk - 1; c >= 0; --c) {
        const RmSample s = rm_sample<PTS>(alpha, z, pts, rr, base, c * WAVE, N, lane, s_pts[PTS ? wave : 0]);
        const double incl = wave_scan_mul(s.u);
        const double T = s_carry[wave][c] * wave_shift_up1(incl, 1.0);
        const double w = (double)s.a * T;
        double G = ga + gd * s.t;
        if constexpr (PTS) G += gx * s.px + gy * s.py + gz * s.pz;
        const int i = c * WAVE + lane;
        const double q = i < N ? w * G : 0.0;
        const double rev = wave_scan_add(__shfl(q, 63 - lane, 64));   // lane l: q of lanes 63-l .. 63
        const double after = __shfl(wave_shift_up1(rev, 0.0), 63 - lane, 64) + suffix;   // sum_{i>k} of this chunk + the rest
        suffix += wave_last(rev);
        if (i < N) d_alpha[base + i] = (float)(T * G - after / s.u);
    }
}

static int ray_maps_check(const char *what, const float *alpha, const float *z, const float *pts, const float *o, const float *d,
                          int64_t B, int N, int64_t *grid) {
    if (B < 0 || N < 1 || N > WAVE * RM_MAX_CHUNKS) return fail(SNERF_E_BADARG, "%s: need B >= 0 and 1 <= N <= 4096", what);
    if ((z != nullptr) == (pts != nullptr)) return fail(SNERF_E_BADARG, "%s: exactly one of z and pts must be given", what);
    *grid = (B + RM_WAVES - 1) / RM_WAVES;
    if (*grid > 0x7fffffffLL) return fail(SNERF_E_BADARG, "%s: B too large", what);
    if (B == 0) return SNERF_OK;
    if (!alpha) return fail(SNERF_E_BADARG, "%s: alpha is null", what);
    if (pts && (!o || !d)) return fail(SNERF_E_BADARG, "%s: pts needs o and d", what);
    return SNERF_OK;
}

}  // namespace snerf

extern "C" int snerf_ray_maps_fwd_f32(const float *alpha, const float *z, const float *pts, const float *o, const float *d,
                                      int64_t B, int N, float *acc, float *depth, float *point, snerf_stream_t stream) {
    using namespace snerf;
    int64_t grid = 0;
    if (int rc = ray_maps_check("ray_maps", alpha, z, pts, o, d, B, N, &grid)) return rc;
    if (point && !pts) return fail(SNERF_E_BADARG, "ray_maps: point needs pts");
    if (B == 0) return SNERF_OK;
    if (!acc || !depth) return fail(SNERF_E_BADARG, "ray_maps: acc/depth is null");
    if (pts)
        hipLaunchKernelGGL(ray_maps_fwd_kernel<true>, dim3((unsigned)grid), dim3(RM_THREADS), 0, (hipStream_t)stream, alpha, z, pts,
                           o, d, B, N, acc, depth, point);
    else
        hipLaunchKernelGGL(ray_maps_fwd_kernel<false>, dim3((unsigned)grid), dim3(RM_THREADS), 0, (hipStream_t)stream, alpha, z, pts,
                           o, d, B, N, acc, depth, point);
    return check_launch("ray_maps_fwd");
}

extern "C" int snerf_ray_maps_bwd_f32(const float *alpha, const float *z, const float *pts, const float *o, const float *d,
                                      int64_t B, int N, const float *d_acc, const float *d_depth, const float *d_point,
                                      float *d_alpha, snerf_stream_t stream) {
    using namespace snerf;
    int64_t grid = 0;
    if (int rc = ray_maps_check("ray_maps_bwd", alpha, z, pts, o, d, B, N, &grid)) return rc;
    if (d_point && !pts) return fail(SNERF_E_BADARG, "ray_maps_bwd: d_point needs pts");
    if (B == 0) return SNERF_OK;
    if (!d_alpha) return fail(SNERF_E_BADARG, "ray_maps_bwd: d_alpha is null");
    if (pts)
        hipLaunchKernelGGL(ray_maps_bwd_kernel<true>, dim3((unsigned)grid), dim3(RM_THREADS), 0, (hipStream_t)stream, alpha, z, pts,
                           o, d, B, N, d_acc, d_depth, d_point, d_alpha);
    else
        hipLaunchKernelGGL(ray_maps_bwd_kernel<false>, dim3((unsigned)grid), dim3(RM_THREADS), 0, (hipStream_t)stream, alpha, z, pts,
                           o, d, B, N, d_acc, d_depth, d_point, d_alpha);
    return check_launch("ray_maps_bwd");
}
