// Density of an equal-weight isotropic Gaussian mixture (utils.py:72-111: GaussianMixture.pdf, the canonical-density term of
// SmplNerfSolver's loss, solver/smpl_nerf_solver.py:39-41) and its gradient to the samples, without the reference's [B, N, V, 3] tensors.
// For sample x_i and the V means mu_v (one per canonical body vertex), s = std:
//   pdf[i]    = factor / V sum_v exp(-|x_i - mu_v|^2 / (2 s^2))                      factor = 1 / sqrt((2 pi)^3 s^6)
//   dpdf[i,:] = d pdf[i] / d x_i = -factor / (V s^2) sum_v exp(...) (x_i - mu_v)
// Dense: every pair costs an exponential (the vertex warp of vertex_warp.hip only meets one inside its radius).  Per pair and lane:
// three subtractions, the squared distance from the differences (a product and two fmaf), one product with the folded constant
// k2 = -log2(e) / (2 s^2), ONE hardware exp2, one sum - and with the gradient three fmaf.  The two scalings happen once per sample.
//
// Mapping: the means are shared by all samples, so the op is flat over n samples.  Lane = sample, workgroup = 64 samples x 16 waves; the
// waves split the means and walk their slice at wave-uniform addresses (scalar-cache loads: four means = twelve floats per wait).  Every
// lane keeps FOUR independent accumulator sets per slice (mean j of a group of four goes to set j): a sum over 6890 means is 64 chains
// of about 108 terms, which keeps both the dependency chains and the rounding chains short.  The partials meet in LDS and wave 0 adds
// them in wave order.  No atomics, no read-modify-write of global memory, every sum has a fixed order: two calls give the same bits.
// Every output element is written; every LDS word that is read has been written.
#include "snerf_common.h"

namespace snerf {

constexpr int GMM_WAVES = 16;   // waves of a 64-sample workgroup: the slices of the means

struct GmmArgs {
    const float *samples, *means;
    float *pdf, *dpdf;
    int64_t n;
    int V;
    float k2;          // -log2(e) / (2 std^2)
    float scale;       // factor / V
    float grad_scale;  // -factor / (V std^2)
};

// one exponential per pair: v_exp_f32 (2^x; an argument below -126 gives 0, -inf gives 0)
__device__ __forceinline__ float gmm_weight(float k2, float dx, float dy, float dz) {
    return __builtin_amdgcn_exp2f(k2 * fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

template <bool GRAD>
__global__ __launch_bounds__(GMM_WAVES * 64) void gmm_pdf_kernel(GmmArgs A) {
    constexpr int Q = GRAD ? 4 : 1;   // sums per lane: the weights and, with the gradient, weight x (x - mu)
    __shared__ float part[GMM_WAVES][Q][WAVE];
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool valid = i < A.n;
    const int64_t sample = valid ? i : A.n - 1;   // the tail loads an element that exists and stores nothing
    const float px = A.samples[sample * 3 + 0], py = A.samples[sample * 3 + 1], pz = A.samples[sample * 3 + 2];
    const float *__restrict__ mu = A.means;
    const int per = (A.V + GMM_WAVES - 1) / GMM_WAVES;
    const int v0 = wave * per < A.V ? wave * per : A.V, v1 = v0 + per < A.V ? v0 + per : A.V;
    float e[4] = {0.f, 0.f, 0.f, 0.f}, gx[4] = {0.f, 0.f, 0.f, 0.f}, gy[4] = {0.f, 0.f, 0.f, 0.f}, gz[4] = {0.f, 0.f, 0.f, 0.f};
    int v = v0;
    for (; v + 4 <= v1; v += 4) {
        float t[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = mu[v * 3 + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dx = px - t[3 * j], dy = py - t[3 * j + 1], dz = pz - t[3 * j + 2];
            const float w = gmm_weight(A.k2, dx, dy, dz);
            e[j] += w;
            if (GRAD) {
                gx[j] = fmaf(w, dx, gx[j]);
                gy[j] = fmaf(w, dy, gy[j]);
                gz[j] = fmaf(w, dz, gz[j]);
            }
        }
    }
    for (int j = 0; v < v1; ++v, ++j) {   // at most three means left: sets 0, 1, 2
        const float dx = px - mu[v * 3 + 0], dy = py - mu[v * 3 + 1], dz = pz - mu[v * 3 + 2];
        const float w = gmm_weight(A.k2, dx, dy, dz);
        e[j] += w;
        if (GRAD) {
            gx[j] = fmaf(w, dx, gx[j]);
            gy[j] = fmaf(w, dy, gy[j]);
            gz[j] = fmaf(w, dz, gz[j]);
        }
    }
    part[wave][0][lane] = (e[0] + e[1]) + (e[2] + e[3]);
    if (GRAD) {
        part[wave][1][lane] = (gx[0] + gx[1]) + (gx[2] + gx[3]);
        part[wave][2][lane] = (gy[0] + gy[1]) + (gy[2] + gy[3]);
        part[wave][3][lane] = (gz[0] + gz[1]) + (gz[2] + gz[3]);
    }
    __syncthreads();
    if (wave != 0 || !valid) return;
    float r[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {   // pairs of waves first, then the pairs in wave order
        float s = 0.f;
        for (int w = 0; w < GMM_WAVES; w += 2) s += part[w][q][lane] + part[w + 1][q][lane];
        r[q] = s;
    }
    A.pdf[sample] = A.scale * r[0];
    if (GRAD) {
        float *d = A.dpdf + sample * 3;
        d[0] = A.grad_scale * r[1];
        d[1] = A.grad_scale * r[2];
        d[2] = A.grad_scale * r[3];
    }
}

}  // namespace snerf

extern "C" int snerf_gmm_pdf_f32(const float *samples, const float *means, int64_t n, int V, float std, float *pdf, float *dpdf,
                                 snerf_stream_t stream) {
    using namespace snerf;
    if (n < 0) return fail(SNERF_E_BADARG, "gmm_pdf: n must not be negative");
    if (V < 1) return fail(SNERF_E_BADARG, "gmm_pdf: V must be at least 1");
    if (!(std > 0.f)) return fail(SNERF_E_BADARG, "gmm_pdf: std must be positive");
    if ((int64_t)V * 3 > 0x7fffffffLL) return fail(SNERF_E_BADARG, "gmm_pdf: V too large");
    const int64_t blocks = (n + WAVE - 1) / WAVE;
    if (blocks > 0x7fffffffLL) return fail(SNERF_E_BADARG, "gmm_pdf: n too large");
    if (n == 0) return SNERF_OK;
    if (!samples) return fail(SNERF_E_BADARG, "gmm_pdf: samples is a null pointer");
    if (!means) return fail(SNERF_E_BADARG, "gmm_pdf: means is a null pointer");
    if (!pdf) return fail(SNERF_E_BADARG, "gmm_pdf: pdf is a null pointer");
    // the constants in double (utils.py:84-86: var = std^2, cov_det = var^3, factor = 1 / sqrt((2 pi)^3 cov_det))
    const double pi = 3.14159265358979323846, log2e = 1.44269504088896340736;
    const double var = (double)std * (double)std, factor = 1.0 / __builtin_sqrt((2.0 * pi) * (2.0 * pi) * (2.0 * pi) * var * var * var);
    GmmArgs A{samples, means, pdf, dpdf, n, V, (float)(-log2e / (2.0 * var)), (float)(factor / V), (float)(-factor / (V * var))};
    const dim3 grid((unsigned)blocks), block(GMM_WAVES * 64);
    if (dpdf) hipLaunchKernelGGL(gmm_pdf_kernel<true>, grid, block, 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(gmm_pdf_kernel<false>, grid, block, 0, (hipStream_t)stream, A);
    return check_launch("gmm_pdf");
}
