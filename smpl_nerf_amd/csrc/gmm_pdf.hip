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
// waves split the means by the slice rule of pair_walk.h and walk their slice at wave-uniform addresses (scalar-cache loads: four means
// = twelve floats per wait; the loop is written out here, see the kernel).  Every
// lane keeps FOUR independent accumulator sets per slice (mean j of a group of four goes to set j): a sum over 6890 means is 64 chains
// of about 108 terms, which keeps both the dependency chains and the rounding chains short.  The partials meet in LDS and wave 0 adds
// them in wave order.  No atomics, no read-modify-write of global memory, every sum has a fixed order: two calls give the same bits.
// Every output element is written; every LDS word that is read has been written.
#include "pair_walk.h"

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
    const int lane = lane_id(), wave = wave_index();
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool valid = i < A.n;
    const int64_t sample = tail_index(i, A.n, valid);
    const float px = A.samples[sample * 3 + 0], py = A.samples[sample * 3 + 1], pz = A.samples[sample * 3 + 2];
    const Slice sl = wave_slice(A.V, GMM_WAVES, wave);   // (V < 16: the empty slices of the last waves contribute zeros)
    float e[4] = {0.f, 0.f, 0.f, 0.f}, gx[4] = {0.f, 0.f, 0.f, 0.f}, gy[4] = {0.f, 0.f, 0.f, 0.f}, gz[4] = {0.f, 0.f, 0.f, 0.f};
    // Its own four-per-wait loop, not walk4: with the loop's body in a lambda the compiler pairs the four means' arithmetic another way
    // (35 vector instructions per group of four instead of 32) and the kernel with the gradient measured 3.9 % slower on an MI355X.
    const float *mu = A.means;
    int v = sl.lo;
    for (; v + 4 <= sl.hi; v += 4) {
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
    for (int j = 0; v < sl.hi; ++v, ++j) {   // at most three means left: sets 0, 1, 2
        const float dx = px - mu[v * 3 + 0], dy = py - mu[v * 3 + 1], dz = pz - mu[v * 3 + 2];
        const float w = gmm_weight(A.k2, dx, dy, dz);
        e[j] += w;
        if (GRAD) {
            gx[j] = fmaf(w, dx, gx[j]);
            gy[j] = fmaf(w, dy, gy[j]);
            gz[j] = fmaf(w, dz, gz[j]);
        }
    }
    auto sum4 = [](const float(&x)[4]) { return (x[0] + x[1]) + (x[2] + x[3]); };
    if constexpr (GRAD) put_partials(part[wave], lane, sum4(e), sum4(gx), sum4(gy), sum4(gz));
    else put_partials(part[wave], lane, sum4(e));
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
    if (int rc = check_walk_count("gmm_pdf", "V", V, 3)) return rc;
    if (!(std > 0.f)) return fail(SNERF_E_BADARG, "gmm_pdf: std must be positive");
    int64_t blocks;
    if (int rc = chunk_blocks("gmm_pdf", "n", n, blocks)) return rc;
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
