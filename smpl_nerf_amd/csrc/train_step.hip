// The per-batch body of NerfSolver.train (solver/nerf_solver.py:76-87) as ONE C-ABI call:
//
//     rgb, rgb_fine, ... = pipeline(batch)            models/nerf_pipeline.py:14-67 (activations saved)
//     loss = MSE(rgb, gt) + MSE(rgb_fine, gt)         solver/nerf_solver.py:48-52
//     loss.backward()                                 autograd through compositing and both RenderRayNets
//     Adam.step()                                     solver/nerf_solver.py:31-33, 87 (torch.optim.Adam, one group)
//
// Pure sequencing of the library's own kernels on the caller's stream plus three small ones that live here: the MSE
// value / gradient, the Adam update over the flat parameter buffer, and the slot tables through which that update writes
// every new weight straight into the MFMA-ordered forward stream and the transposed dgrad stream (no re-pack launches).
// No allocation, no host synchronisation, no step-dependent host scalars (the step counter and the bias corrections live on
// the device): the call can be captured into a HIP graph.
//
// Ray chunks.  The loss is a mean over rays, so d loss / d rgb of a ray does not depend on the other rays of the batch:
// the batch is walked in chunks of `rays_per_chunk` rays - forward, loss gradient, backward per chunk, parameter gradients
// summed over the chunks in chunk order - and the saved layer inputs / d Y buffers (21 KB per sample) are sized by the
// chunk, not by the batch.  Nothing is recomputed (the autograd form needs the whole forward before any backward; the
// reference keeps 2.6 MB per ray alive).
#include <mutex>
#include <thread>
#include <vector>

#include "mlp_device.h"

namespace snerf {

static int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

// ------------------------------------------------------------------------------------------------
// slot tables: parameter i of params_flat -> its element of the forward / transposed fp32 stream (or -1)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fwd_slot_table_kernel(Plan P, int32_t *__restrict__ slot) {
    const int slab = blockIdx.x;
    int li = 0;
    while (li + 1 < P.nlayers && slab >= P.layer[li + 1].first_slab) ++li;
    const Layer &Ly = P.layer[li];
    const int sl = slab - Ly.first_slab;
    for (int e = threadIdx.x; e < SLAB_FLOATS; e += 256) {
        const int64_t src = fwd_slab_src(Ly, sl, e);
        if (src >= 0) slot[src] = slab * SLAB_FLOATS + e;
    }
}
__global__ __launch_bounds__(256) void bwd_slot_table_kernel(Plan P, BwdPlan B, int32_t *__restrict__ slot) {
    const int slab = blockIdx.x;
    int bi = 0;
    while (bi + 1 < B.nl && slab >= B.layer[bi + 1].first_slab) ++bi;
    const BwdLayer &Bl = B.layer[bi];
    const int sl = slab - Bl.first_slab;
    for (int e = threadIdx.x; e < SLAB_FLOATS; e += 256) {
        const int64_t src = bwd_slab_src(P, Bl, sl, e);
        if (src >= 0) slot[src] = slab * SLAB_FLOATS + e;
    }
}

// ------------------------------------------------------------------------------------------------
// loss: MSE(rgb, gt) + MSE(rgb_fine, gt), mean over all B * 3 values each (nn.MSELoss(), solver/nerf_solver.py:48-52)
// ------------------------------------------------------------------------------------------------
// One workgroup per chunk (a chunk is a few thousand rays): d rgb = (2 / (3 B)) (rgb - gt) like mse_loss_backward, the sums
// of squares in fp64, accumulated over the chunks in chunk order (deterministic).  fine == nullptr is run_fine = 0: the
// pipeline returns `rgb` twice (models/nerf_pipeline.py:43-44), so the loss is 2 MSE(rgb) and both gradients land on rgb.
constexpr int MSE_THREADS = 1024;
__global__ __launch_bounds__(MSE_THREADS) void mse_grad_kernel(const float *__restrict__ rgb_c, const float *__restrict__ rgb_f,
                                                               const float *__restrict__ gt, int64_t count, float norm,
                                                               float *__restrict__ d_c, float *__restrict__ d_f,
                                                               double *__restrict__ acc, int first, int last, double inv_total,
                                                               float *__restrict__ loss_out) {
    __shared__ double s_sum[2][MSE_THREADS / WAVE];
    double sc = 0.0, sf = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += MSE_THREADS) {
        const float t = gt[i];
        const float ec = __fsub_rn(rgb_c[i], t);
        const float gc = __fmul_rn(norm, ec);
        sc += (double)ec * (double)ec;
        if (rgb_f) {
            const float ef = __fsub_rn(rgb_f[i], t);
            d_f[i] = __fmul_rn(norm, ef);
            d_c[i] = gc;
            sf += (double)ef * (double)ef;
        } else {
            d_c[i] = __fadd_rn(gc, gc);
        }
    }
    sc = wave_sum(sc);
    sf = wave_sum(sf);
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    if (lane == 0) s_sum[0][wave] = sc, s_sum[1][wave] = sf;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tc = 0.0, tf = 0.0;
        for (int w = 0; w < MSE_THREADS / WAVE; ++w) tc += s_sum[0][w], tf += s_sum[1][w];
        if (!rgb_f) tf = tc;
        tc += first ? 0.0 : acc[0];
        tf += first ? 0.0 : acc[1];
        acc[0] = tc;
        acc[1] = tf;
        if (last) {
            const float lc = (float)(tc * inv_total), lf = (float)(tf * inv_total);
            loss_out[0] = __fadd_rn(lc, lf);
            loss_out[1] = lc;
            loss_out[2] = lf;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam, amsgrad = False, maximize = False; solver/nerf_solver.py:11-14, 31-33)
// ------------------------------------------------------------------------------------------------
// The statements of torch's single-tensor update in their order, in fp32 with the Python scalars rounded to fp32 where
// torch hands them to a kernel, and with the fused multiply-adds torch's CPU kernels (the reference's optimiser runs there)
// contain - add(alpha), lerp_ and addcmul_ are `fmadd`s in ATen's vectorised code; established by bit comparison with
// torch.optim.Adam on the CPU (tools/ab/adam_debug.py; tests/test_gpu_round4.py holds both moments to equality; the parameters
// land within one unit in the last place - torch's vectorised CPU sqrt is not correctly rounded on every host, IEEE sqrt here):
//     grad = fma(weight_decay, param, grad)                        (only if weight_decay != 0)
//     exp_avg     = fma(1 - beta1, grad - exp_avg, exp_avg)        lerp_
//     exp_avg_sq  = fma((1 - beta2) * grad, grad, exp_avg_sq * beta2)
//     denom       = sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps
//     param       = param + (-(lr / (1 - beta1^t)) * exp_avg) / denom
// t and the two step-dependent scalars live on the device (a captured graph replays with the right values).  torch keeps one
// step counter per parameter TENSOR (a tensor whose .grad is None is skipped and does not count): a range carries the counters
// of its tensors, all equal on entry, all incremented here.
constexpr int ADAM_MAX_RANGES = 32;
struct AdamRanges {
    int n;
    int64_t *step[ADAM_MAX_RANGES];
    int n_steps[ADAM_MAX_RANGES];
};
__global__ __launch_bounds__(64) void adam_scalars_kernel(AdamRanges R, double lr, double beta1, double beta2, float *__restrict__ scal) {
    const int r = blockIdx.x;
    const int64_t t = R.step[r][0] + 1;     // (read by every lane before any lane writes: one wave, in lock-step)
    for (int i = threadIdx.x; i < R.n_steps[r]; i += 64) R.step[r][i] = t;
    if (threadIdx.x == 0) {
        const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
        scal[2 * r + 0] = (float)(-(lr / bc1));
        scal[2 * r + 1] = (float)sqrt(bc2);
    }
}

constexpr int ADAM_MAX_NETS = 8;
struct AdamNet {
    int64_t begin, end;          // this net's kernel-ordered parameters inside the flat buffer
    float *packed, *packed_t;    // fp32 streams refreshed in place (nullable)
    const int32_t *slot_fwd, *slot_t;
};
struct AdamArgs {
    float *p;
    const float *g;
    float *m, *v;
    const float *scal;
    float w1, beta2, w2, eps, wd;
    int n_nets;
    AdamNet net[ADAM_MAX_NETS];
};

__global__ __launch_bounds__(256) void adam_kernel(AdamArgs A, int64_t begin, int64_t end, int range) {
    const int64_t i = begin + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= end) return;
    const float neg_step = A.scal[2 * range], bc2_sqrt = A.scal[2 * range + 1];
    float p = A.p[i], g = A.g[i];
    if (A.wd != 0.f) g = __fmaf_rn(A.wd, p, g);
    float m = A.m[i], v = A.v[i];
    m = __fmaf_rn(A.w1, __fsub_rn(g, m), m);
    v = __fmaf_rn(__fmul_rn(A.w2, g), g, __fmul_rn(v, A.beta2));
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), A.eps);
    p = __fadd_rn(p, __fdiv_rn(__fmul_rn(neg_step, m), denom));
    A.m[i] = m;
    A.v[i] = v;
    A.p[i] = p;
#pragma unroll
    for (int k = 0; k < ADAM_MAX_NETS; ++k) {
        if (k >= A.n_nets) break;
        const AdamNet &N = A.net[k];
        if (i >= N.begin && i < N.end) {
            const int64_t j = i - N.begin;
            if (N.packed) {
                const int s = N.slot_fwd[j];
                if (s >= 0) N.packed[s] = p;
            }
            if (N.packed_t) {
                const int s = N.slot_t[j];
                if (s >= 0) N.packed_t[s] = p;
            }
        }
    }
}

static bool split_code(int precision) { return precision == 2 || precision == 3 || precision == SNERF_SPLIT_F16X3; }

}  // namespace snerf

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
extern "C" int snerf_mlp_stream_slots(const snerf_mlp_desc *desc, int32_t *slot_fwd, int32_t *slot_t, int input_grad,
                                      snerf_stream_t stream) {
    using namespace snerf;
    Plan P;
    if (int rc = plan_for("mlp_stream_slots", desc, P)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (slot_fwd) {
        if (hipMemsetAsync(slot_fwd, 0xff, (size_t)P.param_floats * sizeof(int32_t), s) != hipSuccess)
            return fail(SNERF_E_LAUNCH, "mlp_stream_slots: memset failed");
        hipLaunchKernelGGL(fwd_slot_table_kernel, dim3(P.total_slabs), dim3(256), 0, s, P, slot_fwd);
        if (int rc = check_launch("mlp_stream_slots(fwd)")) return rc;
    }
    if (slot_t) {
        BwdPlan B;
        make_bwd_plan(P, B, input_grad != 0);
        if (hipMemsetAsync(slot_t, 0xff, (size_t)P.param_floats * sizeof(int32_t), s) != hipSuccess)
            return fail(SNERF_E_LAUNCH, "mlp_stream_slots: memset failed");
        hipLaunchKernelGGL(bwd_slot_table_kernel, dim3(B.total_slabs), dim3(256), 0, s, P, B, slot_t);
        if (int rc = check_launch("mlp_stream_slots(t)")) return rc;
    }
    return SNERF_OK;
}

extern "C" int snerf_adam_step_f32(const snerf_adam_state *st, const snerf_adam_range *ranges_host, int n_ranges,
                                   const snerf_adam_net *nets_host, int n_nets, snerf_stream_t stream) {
    using namespace snerf;
    if (!st || !st->params || !st->grads || !st->exp_avg || !st->exp_avg_sq || !st->scratch)
        return fail(SNERF_E_BADARG, "adam_step: null pointer in the optimiser state");
    if (st->n_params < 0 || n_ranges < 0 || n_ranges > ADAM_MAX_RANGES || n_nets < 0 || n_nets > ADAM_MAX_NETS)
        return fail(SNERF_E_BADARG, "adam_step: bad n_params / n_ranges / n_nets (at most %d ranges, %d nets)", ADAM_MAX_RANGES,
                    ADAM_MAX_NETS);
    if ((n_ranges && !ranges_host) || (n_nets && !nets_host)) return fail(SNERF_E_BADARG, "adam_step: null range / net array");
    if (n_ranges == 0) return SNERF_OK;
    AdamRanges R{};
    R.n = n_ranges;
    for (int r = 0; r < n_ranges; ++r) {
        const snerf_adam_range &g = ranges_host[r];
        if (g.begin < 0 || g.end > st->n_params || g.begin > g.end || !g.step || g.n_steps < 1)
            return fail(SNERF_E_BADARG, "adam_step: range %d: outside the parameter buffer, or no step counters", r);
        R.step[r] = g.step;
        R.n_steps[r] = g.n_steps;
    }
    if (!(st->lr >= 0.0) || !(st->eps >= 0.0) || !(st->beta1 >= 0.0 && st->beta1 < 1.0) || !(st->beta2 >= 0.0 && st->beta2 < 1.0) ||
        !(st->weight_decay >= 0.0))
        return fail(SNERF_E_BADARG, "adam_step: invalid hyper-parameters (torch.optim.Adam's own checks)");
    hipStream_t s = (hipStream_t)stream;
    AdamArgs A{};
    A.p = st->params;
    A.g = st->grads;
    A.m = st->exp_avg;
    A.v = st->exp_avg_sq;
    A.scal = st->scratch;
    A.w1 = (float)(1.0 - st->beta1);
    A.beta2 = (float)st->beta2;
    A.w2 = (float)(1.0 - st->beta2);
    A.eps = (float)st->eps;
    A.wd = (float)st->weight_decay;
    Plan P;
    char who_net[32];
    for (int k = 0; k < n_nets; ++k) {
        const snerf_adam_net &N = nets_host[k];
        snprintf(who_net, sizeof who_net, "adam_step: net %d", k);
        if (int rc = plan_for(who_net, N.desc, P)) return rc;
        if (N.param_offset < 0 || N.param_offset + P.param_floats > st->n_params)
            return fail(SNERF_E_BADARG, "adam_step: net %d does not lie inside the flat parameter buffer", k);
        if (N.precision != 0 && !split_code(N.precision)) return fail(SNERF_E_BADARG, "adam_step: net %d: bad precision code", k);
        AdamNet &D = A.net[A.n_nets];
        D.begin = N.param_offset;
        D.end = N.param_offset + P.param_floats;
        if (N.precision == 0) {   // fp32 streams: refreshed in place by the update kernel
            D.packed = reinterpret_cast<float *>(N.packed);
            D.packed_t = reinterpret_cast<float *>(N.packed_t);
            D.slot_fwd = N.slot_fwd;
            D.slot_t = N.slot_t;
            if ((D.packed && !D.slot_fwd) || (D.packed_t && !D.slot_t))
                return fail(SNERF_E_BADARG, "adam_step: net %d: an fp32 stream needs its slot table (snerf_mlp_stream_slots)", k);
            if (D.packed || D.packed_t) ++A.n_nets;
        }
    }
    hipLaunchKernelGGL(adam_scalars_kernel, dim3(n_ranges), dim3(64), 0, s, R, st->lr, st->beta1, st->beta2, st->scratch);
    if (int rc = check_launch("adam_step(scalars)")) return rc;
    for (int r = 0; r < n_ranges; ++r) {
        const int64_t b = ranges_host[r].begin, e = ranges_host[r].end;
        if (b == e) continue;
        const int64_t grid = (e - b + 255) / 256;
        if (grid > 0x7fffffffLL) return fail(SNERF_E_BADARG, "adam_step: range too large");
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)grid), dim3(256), 0, s, A, b, e, r);
        if (int rc = check_launch("adam_step")) return rc;
    }
    // split-precision streams hold pre-split parts (and, f16x3, per-layer scales): re-packed from the new parameters
    for (int k = 0; k < n_nets; ++k) {
        const snerf_adam_net &N = nets_host[k];
        if (N.precision == 0) continue;
        const float *pf = st->params + N.param_offset;
        int rc;
        if (N.packed && (rc = snerf_mlp_pack_bf16(N.desc, pf, N.packed, N.precision, stream))) return rc;
        if (N.packed_t && (rc = snerf_mlp_pack_t_bf16(N.desc, pf, N.packed_t, N.precision, 0, stream))) return rc;
    }
    return SNERF_OK;
}

namespace snerf {

struct TrainWs {
    int64_t raw_c, weights_c, z_fine, pts_f, raw_f, d_rgb_c, d_rgb_f, d_raw, act_c, act_f, dy, gpart, loss_acc;
    int64_t d_raw2, dy2, gpart2;   // second set for the coarse net's backward when it runs beside the fine net's (small chunks)
    int64_t contract;              // scratch of the d loss / d additional-inputs contraction (nets with add_dim > 0)
    bool concurrent;
    int64_t total;
};

// Chunks of at most this many samples (coarse + fine of a ray) leave much of the chip idle in some kernel (a 64-ray batch is 96
// workgroups of 128 samples; at 800 rays the coarse passes fill 1.56 rounds of the CUs): there the backward of the coarse
// net - independent of the fine net's: the hierarchical samples are detached, utils.py:260 - runs beside it on the caller's
// auxiliary stream.  A pure size rule, so that the workspace size does not depend on the device.  Measured (tools/ab/
// conc_ab.sh, ms per step without / with): 128 rays 1.49 / 1.33, 256: 2.42 / 2.29-2.35, 512: 4.00 / 3.96, 800: 6.60 / 6.45-6.48,
// 1024: 7.80 / 7.83, 2048: 15.29 / 15.21 - above 1024 rays nothing is left to fill, and the second d Y buffer would cost memory.
constexpr int64_t CONCURRENT_MAX_FINE_SAMPLES = 1024 * 256;
// the same rule for the smpl_nerf step (its coarse chain carries the warp net's backward as well).  Measured r05 with the rule
// lifted (coarse chain beside the fine chain at every chunk size): 4096 rays 34.00 -> 33.72 ms per step, 2048 rays the same
// fraction, for 1.8 GB more workspace - both chains are bound by the matrix pipe there, nothing is left to fill.
constexpr int64_t SMPL_CONCURRENT_MAX_FINE_SAMPLES = CONCURRENT_MAX_FINE_SAMPLES;

// fork / join events of the concurrent backward: one pair per host thread and device (include/smplnerf.h "State"), kept in a
// registry so that snerf_shutdown() can destroy them
struct EventPair {
    std::thread::id tid;
    int dev;
    hipEvent_t ev[2];
};
static std::mutex &event_mutex() {
    static std::mutex m;
    return m;
}
static std::vector<EventPair> &event_registry() {
    static std::vector<EventPair> v;
    return v;
}
static int fork_join_events(hipEvent_t &fork, hipEvent_t &join) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return fail(SNERF_E_LAUNCH, "nerf_train: cannot query the current device");
    const std::thread::id me = std::this_thread::get_id();
    std::lock_guard<std::mutex> lock(event_mutex());
    for (const EventPair &p : event_registry())
        if (p.tid == me && p.dev == dev) {
            fork = p.ev[0];
            join = p.ev[1];
            return SNERF_OK;
        }
    EventPair p{me, dev, {nullptr, nullptr}};
    for (int k = 0; k < 2; ++k)
        if (hipEventCreateWithFlags(&p.ev[k], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (k == 1) (void)hipEventDestroy(p.ev[0]);
            return fail(SNERF_E_LAUNCH, "nerf_train: cannot create an event");
        }
    event_registry().push_back(p);
    fork = p.ev[0];
    join = p.ev[1];
    return SNERF_OK;
}
void destroy_fork_join_events() {
    std::lock_guard<std::mutex> lock(event_mutex());
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (const EventPair &p : event_registry()) {
        (void)hipSetDevice(p.dev);
        (void)hipEventDestroy(p.ev[0]);
        (void)hipEventDestroy(p.ev[1]);
    }
    event_registry().clear();
    if (have_cur) (void)hipSetDevice(cur);
    (void)hipGetLastError();
}

static int train_ws(const snerf_mlp_desc *dc, const snerf_mlp_desc *df, int64_t chunk, int Nc, int Nf, TrainWs &w, bool two_streams = true,
                    int64_t concurrent_max = CONCURRENT_MAX_FINE_SAMPLES) {
    const int64_t N = Nc + Nf;
    int64_t act_c = 0, dy_c = 0, gp_c = 0, act_f = 0, dy_f = 0, gp_f = 0;
    int rc;
    if ((rc = snerf_mlp_train_sizes(dc, chunk * Nc, &act_c, &dy_c, nullptr, &gp_c, nullptr))) return rc;
    if (Nf > 0 && (rc = snerf_mlp_train_sizes(df, chunk * N, &act_f, &dy_f, nullptr, &gp_f, nullptr))) return rc;
    int64_t off = 0;
    auto take = [&](int64_t floats) {
        const int64_t o = off;
        off += align256(floats * 4);
        return o;
    };
    w.raw_c = take(chunk * Nc * 4);
    w.weights_c = take(chunk * Nc);
    w.z_fine = take(Nf > 0 ? chunk * N : 0);
    w.pts_f = take(Nf > 0 ? chunk * N * 3 : 0);
    w.raw_f = take(Nf > 0 ? chunk * N * 4 : 0);
    w.d_rgb_c = take(chunk * 3);
    w.d_rgb_f = take(chunk * 3);
    w.d_raw = take(chunk * N * 4);
    w.act_c = take(act_c);
    w.act_f = take(act_f);
    w.dy = take(dy_c > dy_f ? dy_c : dy_f);
    w.gpart = take(gp_c > gp_f ? gp_c : gp_f);
    w.loss_acc = take(4);
    w.concurrent = two_streams && Nf > 0 && chunk * N <= concurrent_max;
    w.d_raw2 = take(w.concurrent ? chunk * Nc * 4 : 0);
    w.dy2 = take(w.concurrent ? dy_c : 0);
    w.gpart2 = take(w.concurrent ? gp_c : 0);
    // d loss / d additional inputs (snerf_*_ig_f32): the per-ray partial sums of the contraction (contract.hip)
    int64_t cs = 0;
    if (dc->add_dim > 0) {
        cs = snerf_dy_contract_scratch_floats(chunk * Nc, dc->add_dim, Nc);
        if (Nf > 0) {
            const int64_t cf = snerf_dy_contract_scratch_floats(chunk * N, dc->add_dim, (int)N);
            cs = cf > cs ? cf : cs;
        }
        if (cs < 0) return (int)cs;
    }
    w.contract = take(cs);
    w.total = off;
    return SNERF_OK;
}

// d loss / d additional inputs of one net for one chunk: the stored d Y_l of layer 0 and of every skip layer contracted with the
// weight columns that read the additional inputs, summed over the samples of a ray (contract.hip; what autograd does through
// models/render_ray_net.py:43-50 and the `expand` of the pose rows, models/append_smpl_params_pipeline.py:29-52).  out: [rays, add_dim]
// rows of this chunk; overwrite: the first contraction of the chunk overwrites, the others accumulate.
static int contract_additional(const snerf_mlp_desc *desc, const float *params, const float *dy, int64_t n, int spr, float *out,
                               bool overwrite, float *scratch, snerf_stream_t stream) {
    Plan P;
    if (int rc = plan_for("nerf_train_grads", desc, P)) return rc;
    TrainLayout L;
    make_train_layout(P, L);
    bool first = overwrite;
    for (int l = 0; l < P.nlayers; ++l)
        for (int sg = 0; sg < P.layer[l].nseg; ++sg) {
            const Seg &seg = P.layer[l].seg[sg];
            if (seg.type != SEG_ADD) continue;
            const Layer &Ly = P.layer[l];
            const int rc = snerf_dy_contract_f32(dy, n, L.dy[l], Ly.n_out, params + Ly.w_off, Ly.n_in, seg.col_off, seg.ncols, spr, out,
                                                 seg.ncols, 0, first ? 0 : 1, scratch, stream);
            if (rc) return rc;
            first = false;
        }
    return SNERF_OK;
}

static int64_t effective_chunk(int64_t B, int64_t rays_per_chunk) {
    if (rays_per_chunk <= 0 || rays_per_chunk > B) return B > 0 ? B : 1;
    return rays_per_chunk;
}

}  // namespace snerf

extern "C" int64_t snerf_nerf_train_workspace_bytes(const snerf_mlp_desc *desc_coarse, const snerf_mlp_desc *desc_fine, int64_t B,
                                                    int Nc, int Nf, int64_t rays_per_chunk) {
    using namespace snerf;
    if (!desc_coarse || B < 0 || Nc < 1 || Nf < 0 || (Nf > 0 && !desc_fine))
        return fail(SNERF_E_BADARG, "nerf_train_workspace_bytes: bad arguments");
    TrainWs w{};
    if (int rc = train_ws(desc_coarse, desc_fine, effective_chunk(B, rays_per_chunk), Nc, Nf, w)) return rc;
    return w.total;
}

namespace snerf {
// dp_comm.hip
int dp_allreduce_avg(snerf_comm_t comm, float *buf, int64_t begin, int64_t end, int64_t skip_begin, int64_t skip_end, hipStream_t stream,
                     const char *what);

// ------------------------------------------------------------------------------------------------
// the argument record of the training entries: everything a gradient half reads, by name.  Every exported entry fills one
// and hands it to nerf_train_grads / smpl_nerf_train_grads; the step entries go on to finish_step.
// ------------------------------------------------------------------------------------------------
struct NetArgs {
    const snerf_mlp_desc *desc;
    const void *packed, *packed_t;
    float *grad;
};
struct WarpArgs {
    const snerf_warp_desc *desc;
    float *packed, *packed_t;    // read by the gradient half; re-packed behind Adam by the step entries
    float *grad;
    const float *pose_enc;
};
struct TrainArgs {
    NetArgs coarse, fine;
    WarpArgs warp;               // the smpl_nerf form only
    int precision;               // may carry SNERF_REFERENCE_SUM
    const snerf_nerf_batch *batch;
    int64_t rays_per_chunk;
    void *workspace;
    float *loss, *rgb, *rgb_fine;
    snerf_stream_t stream, aux_stream;
    // comm != NULL (the data-parallel step): the flat gradient buffer flat_g[0 .. flat_n), which holds the nets' gradients as
    // segments, is averaged over the ranks between the backward and Adam
    snerf_comm_t comm;
    float *flat_g;
    int64_t flat_n;
    const snerf_input_grads *input_grads;
};
struct AdamCall {
    const snerf_adam_state *adam;
    const snerf_adam_range *ranges_host;
    int n_ranges;
    const snerf_adam_net *nets_host;
    int n_nets;
};

// What follows the gradient half in a step entry.  smpl_who != NULL is the smpl_nerf form: its one collective (comm != NULL: the
// whole flat buffer; the nerf form issues its two inside the gradient half, behind the last chunk), Adam, the warp net's streams
// re-packed from the new parameters.
static int finish_step(const TrainArgs &a, const AdamCall &o, const char *smpl_who = nullptr, int64_t warp_param_offset = 0) {
    int rc;
    if (smpl_who && a.comm && (rc = dp_allreduce_avg(a.comm, a.flat_g, 0, a.flat_n, 0, 0, (hipStream_t)a.stream, smpl_who))) return rc;
    if ((rc = snerf_adam_step_f32(o.adam, o.ranges_host, o.n_ranges, o.nets_host, o.n_nets, a.stream))) return rc;
    if (!smpl_who) return SNERF_OK;
    return snerf_warp_repack_f32(a.warp.desc, o.adam ? o.adam->params : nullptr, o.adam ? o.adam->n_params : 0, warp_param_offset,
                                 a.warp.packed, a.warp.packed_t, a.stream);
}

// A rank of a data-parallel step whose shard ran out (B == 0; RayBatchLoader allows unequal shards): zero gradient, zero loss.
// It still takes part in the step's collectives, in the order every other rank issues them: the caller goes on to those.
static int dp_empty_shard(const TrainArgs &a, const char *who) {
    hipStream_t s = (hipStream_t)a.stream;
    if (hipMemsetAsync(a.flat_g, 0, (size_t)a.flat_n * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(a.loss, 0, 3 * sizeof(float), s) != hipSuccess)
        return fail(SNERF_E_LAUNCH, "%s: memset failed", who);
    return SNERF_OK;
}

// ------------------------------------------------------------------------------------------------
// what the two gradient halves share (`who` is the entry-name prefix of the error texts)
// ------------------------------------------------------------------------------------------------
struct Shape {
    int precision;    // without SNERF_REFERENCE_SUM
    bool refsum;
    int64_t B, chunk;
    int Nc, Nf, N;
};
// min_B = 0 admits the empty shard of a data-parallel step
static int decode_shape(const TrainArgs &a, int64_t min_B, const char *who, Shape &sh) {
    sh.refsum = (a.precision & SNERF_REFERENCE_SUM) != 0;
    sh.precision = a.precision & ~SNERF_REFERENCE_SUM;
    if (sh.precision != 0 && !split_code(sh.precision))
        return fail(SNERF_E_BADARG, "%s: precision must be 0 (fp32), 2 (bf16x3), 3 (bf16x6) or 16 (f16x3)", who);
    if (!a.batch) return fail(SNERF_E_BADARG, "%s: batch is null", who);
    sh.B = a.batch->B;
    sh.Nc = a.batch->Nc, sh.Nf = a.batch->Nf, sh.N = sh.Nc + sh.Nf;
    if (sh.B < min_B || sh.Nc < 1 || sh.Nf < 0) return fail(SNERF_E_BADARG, "%s: need B >= 1, Nc >= 1, Nf >= 0", who);
    sh.chunk = effective_chunk(sh.B, a.rays_per_chunk);
    return SNERF_OK;
}
static int check_workspace_and_width(const TrainArgs &a, const Shape &sh, const char *who) {
    if (!aligned(a.workspace, 256)) return fail(SNERF_E_ALIGN, "%s: workspace must be 256-byte aligned", who);
    if (sh.precision != 0 && (a.coarse.desc->width != 256 || (sh.Nf > 0 && a.fine.desc->width != 256)))
        return fail(SNERF_E_BADARG, "%s: the split-precision kernels exist for width 256", who);
    return SNERF_OK;
}

// typed view of a carved workspace.  set[0]: the scratch of a net's backward; set[1]: the coarse net's own set when its backward
// runs beside the fine net's (TrainWs::concurrent)
struct BwdSet {
    float *d_raw, *dy, *gpart;
};
struct TrainBufs {
    float *raw_c, *weights_c, *z_fine, *pts_f, *raw_f, *d_rgb_c, *d_rgb_f, *act_c, *act_f, *contract;
    double *loss_acc;
    BwdSet set[2];
};
static float *at(void *workspace, int64_t off) { return reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + off); }
static TrainBufs carve(const TrainWs &w, void *ws) {
    TrainBufs m;
    m.raw_c = at(ws, w.raw_c), m.weights_c = at(ws, w.weights_c), m.z_fine = at(ws, w.z_fine), m.pts_f = at(ws, w.pts_f);
    m.raw_f = at(ws, w.raw_f), m.d_rgb_c = at(ws, w.d_rgb_c), m.d_rgb_f = at(ws, w.d_rgb_f), m.act_c = at(ws, w.act_c);
    m.act_f = at(ws, w.act_f), m.contract = at(ws, w.contract);
    m.loss_acc = reinterpret_cast<double *>(at(ws, w.loss_acc));
    m.set[0] = {at(ws, w.d_raw), at(ws, w.dy), at(ws, w.gpart)};
    m.set[1] = {at(ws, w.d_raw2), at(ws, w.dy2), at(ws, w.gpart2)};
    return m;
}

// small chunks with an auxiliary stream: the coarse net's backward (the smpl_nerf form: the whole coarse chain) beside the fine
// net's, on the second scratch set.  fork / join enqueue nothing when `on` is false.
struct Concurrent {
    bool on;
    hipEvent_t ev_fork, ev_join;
    hipStream_t s, aux;
    snerf_stream_t stream_c;    // where the coarse backward runs
    int fork(const char *who) const {
        if (on && (hipEventRecord(ev_fork, s) != hipSuccess || hipStreamWaitEvent(aux, ev_fork, 0) != hipSuccess))
            return fail(SNERF_E_LAUNCH, "%s: cannot fork onto the auxiliary stream", who);
        return SNERF_OK;
    }
    int join(const char *who) const {
        if (on && (hipEventRecord(ev_join, aux) != hipSuccess || hipStreamWaitEvent(s, ev_join, 0) != hipSuccess))
            return fail(SNERF_E_LAUNCH, "%s: cannot join the auxiliary stream", who);
        return SNERF_OK;
    }
};
static int concurrent_setup(const TrainArgs &a, const TrainWs &w, Concurrent &c) {
    c.on = w.concurrent && a.aux_stream && a.aux_stream != a.stream;
    c.ev_fork = c.ev_join = nullptr;
    c.s = (hipStream_t)a.stream, c.aux = (hipStream_t)a.aux_stream;
    c.stream_c = c.on ? a.aux_stream : a.stream;
    return c.on ? fork_join_events(c.ev_fork, c.ev_join) : SNERF_OK;
}

// the rays [r0, r0 + b) of the batch and of the outputs
struct Chunk {
    int64_t r0, b;
    bool first, last;
    const float *x, *o, *d, *z, *gt, *nz_c, *nz_f;
    float *rgb_c, *rgb_f;
};
static Chunk chunk_of(const TrainArgs &a, const Shape &sh, int64_t r0) {
    const snerf_nerf_batch *t = a.batch;
    Chunk c;
    c.r0 = r0;
    c.b = (sh.B - r0 < sh.chunk) ? sh.B - r0 : sh.chunk;
    c.first = r0 == 0, c.last = r0 + c.b >= sh.B;
    c.x = t->ray_samples + r0 * sh.Nc * 3, c.d = t->rays_d + r0 * 3, c.z = t->z_vals + r0 * sh.Nc, c.gt = t->rgb_truth + r0 * 3;
    c.o = t->rays_o ? t->rays_o + r0 * 3 : nullptr;
    c.nz_c = t->noise_coarse ? t->noise_coarse + r0 * sh.Nc : nullptr;
    c.nz_f = t->noise_fine ? t->noise_fine + r0 * sh.N : nullptr;
    c.rgb_c = a.rgb + r0 * 3, c.rgb_f = a.rgb_fine + r0 * 3;
    return c;
}

// loss value and d loss / d rgb of a chunk (solver/nerf_solver.py:48-52, 85-86)
static int launch_loss(const TrainArgs &a, const Shape &sh, const TrainBufs &m, const Chunk &c, const char *what) {
    const float norm = (float)(2.0 / (3.0 * (double)sh.B));      // mse_loss_backward: 2 / numel
    const double inv_total = 1.0 / (3.0 * (double)sh.B);
    hipLaunchKernelGGL(mse_grad_kernel, dim3(1), dim3(MSE_THREADS), 0, (hipStream_t)a.stream, c.rgb_c, sh.Nf > 0 ? c.rgb_f : nullptr, c.gt,
                       c.b * 3, norm, m.d_rgb_c, m.d_rgb_f, m.loss_acc, c.first ? 1 : 0, c.last ? 1 : 0, inv_total, a.loss);
    return check_launch(what);
}

// run_fine = 0: the pipeline returns `rgb` twice (models/nerf_pipeline.py:43-44)
static int copy_rgb_fine(const TrainArgs &a, const Shape &sh, const char *who) {
    if (sh.Nf == 0 && a.rgb_fine != a.rgb &&
        hipMemcpyAsync(a.rgb_fine, a.rgb, (size_t)sh.B * 3 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)a.stream) != hipSuccess)
        return fail(SNERF_E_LAUNCH, "%s: device copy failed", who);
    return SNERF_OK;
}

// (data-parallel step) the coarse net's gradient as a segment [c0, c1) of the flat buffer
static int coarse_segment(const TrainArgs &a, int64_t &c0, int64_t &c1) {
    const int64_t pc = snerf_mlp_param_floats(a.coarse.desc);
    c0 = a.coarse.grad - a.flat_g;
    c1 = c0 + pc;
    if (pc < 1 || c0 < 0 || c1 > a.flat_n) return fail(SNERF_E_BADARG, "nerf_train_step_dp: grad_coarse must lie inside adam->grads[0 .. n_params)");
    return SNERF_OK;
}

// The gradient half of the nerf form.  With comm, the collectives of the step are issued behind the last chunk's backward.
static int nerf_train_grads(const TrainArgs &a) {
    const char *const who = "nerf_train_grads", *const who_dp = "nerf_train_step_dp";
    const NetArgs &C = a.coarse, &F = a.fine;
    const snerf_nerf_batch *batch = a.batch;
    const snerf_input_grads *ig = a.input_grads;
    Shape sh;
    int rc;
    if ((rc = decode_shape(a, a.comm ? 0 : 1, who, sh))) return rc;
    const int64_t B = sh.B;
    const int Nc = sh.Nc, Nf = sh.Nf, N = sh.N, precision = sh.precision;
    int64_t cb0 = 0, cb1 = 0;
    if (a.comm && B == 0) {
        if (!a.flat_g || a.flat_n < 1 || !C.desc || !C.grad || !a.loss) return fail(SNERF_E_BADARG, "nerf_train_step_dp: null pointer");
        if ((rc = coarse_segment(a, cb0, cb1))) return rc;
        if ((rc = dp_empty_shard(a, who_dp))) return rc;
        if ((rc = dp_allreduce_avg(a.comm, a.flat_g, cb0, cb1, 0, 0, (hipStream_t)a.stream, who_dp))) return rc;
        return dp_allreduce_avg(a.comm, a.flat_g, 0, a.flat_n, cb0, cb1, (hipStream_t)a.stream, who_dp);
    }
    if (!C.desc || !C.packed || !C.packed_t || !batch->ray_samples || !batch->rays_d || !batch->z_vals || !batch->rgb_truth ||
        !a.workspace || !C.grad || !a.loss || !a.rgb || !a.rgb_fine)
        return fail(SNERF_E_BADARG, "nerf_train_grads: null pointer");
    if (Nf > 0 && (!F.desc || !F.packed || !F.packed_t || !F.grad || !batch->rays_o || !batch->u))
        return fail(SNERF_E_BADARG, "nerf_train_grads: the fine pass needs desc_fine, its streams, grad_fine, rays_o and u");
    const int add_dim = C.desc->add_dim;
    if (Nf > 0 && F.desc->add_dim != add_dim)
        return fail(SNERF_E_BADARG, "nerf_train_grads: both nets must read the same per-ray additional inputs (add_dim %d vs %d)", add_dim,
                    F.desc->add_dim);
    if (add_dim && !batch->additional) return fail(SNERF_E_BADARG, "nerf_train_grads: the nets have additional inputs but batch->additional is null");
    float *d_add = ig ? ig->d_additional : nullptr;
    if (d_add && (!add_dim || !ig->params_coarse || (Nf > 0 && !ig->params_fine)))
        return fail(SNERF_E_BADARG, "nerf_train_grads: d_additional needs nets with additional inputs and their parameters (params_coarse / params_fine)");
    if ((rc = check_workspace_and_width(a, sh, who))) return rc;
    TrainWs w{};
    if ((rc = train_ws(C.desc, F.desc, sh.chunk, Nc, Nf, w))) return rc;
    const TrainBufs m = carve(w, a.workspace);
    Concurrent cc;
    if ((rc = concurrent_setup(a, w, cc))) return rc;
    const BwdSet &sf = m.set[0], &sc = m.set[cc.on ? 1 : 0];
    if (a.comm) {
        if (!a.flat_g || a.flat_n < 1) return fail(SNERF_E_BADARG, "nerf_train_step_dp: no flat gradient buffer");
        if ((rc = coarse_segment(a, cb0, cb1))) return rc;
        const int64_t pf = Nf > 0 ? snerf_mlp_param_floats(F.desc) : 0;
        if (Nf > 0 && (F.grad - a.flat_g < 0 || F.grad - a.flat_g + pf > a.flat_n))
            return fail(SNERF_E_BADARG, "nerf_train_step_dp: grad_fine must lie inside adam->grads[0 .. n_params)");
    }
    const snerf_stream_t stream = a.stream;
    const int wb = batch->white_background ? 1 : 0;
    auto fwd_train = [&](const NetArgs &n, const float *x, const float *dirs, const float *add, int64_t cnt, int spr, float *raw, float *act) {
        MlpFwdCall c{n.desc, n.packed, x, dirs, 0, add, cnt, spr, raw, stream};
        c.act = act;
        c.train = true;
        return mlp_forward(precision, c);
    };
    auto bwd = [&](const NetArgs &n, const float *act, const BwdSet &t, int64_t cnt, bool accumulate, snerf_stream_t st, int64_t n_beside) {
        MlpBwdCall c{n.desc, n.packed_t, act, t.d_raw, cnt, t.dy, t.gpart, n.grad, st};
        c.accumulate = accumulate;
        c.n_beside = n_beside;
        return mlp_backward(precision, c);
    };
    // (the weight-gradient launches of a chunk small enough for the concurrent backward split their jobs for each net's share of the
    // chip - by the size rule alone, with or without an auxiliary stream: the summation order, hence every bit of the gradients,
    // does not depend on the streams the caller brings)
    for (int64_t r0 = 0; r0 < B; r0 += sh.chunk) {
        const Chunk c = chunk_of(a, sh, r0);
        const int64_t b = c.b;
        const float *add = add_dim ? batch->additional + r0 * add_dim : nullptr;   // per-ray constants (append_smpl_params_pipeline.py:29-52)
        // forward (models/nerf_pipeline.py:29-65) with every layer input saved
        if ((rc = fwd_train(C, c.x, c.d, add, b * Nc, Nc, m.raw_c, m.act_c))) return rc;
        if ((rc = snerf_composite_fwd_f32(m.raw_c, c.z, c.d, 0, c.nz_c, b, Nc, wb, c.rgb_c, Nf > 0 ? m.weights_c : nullptr, nullptr, stream)))
            return rc;
        if (Nf > 0) {
            if ((rc = sample_pdf_merged(sh.refsum, c.z, m.weights_c, batch->u, c.o, c.d, b, Nc, Nf, nullptr, nullptr, m.z_fine, m.pts_f, stream)))
                return rc;
            if ((rc = fwd_train(F, m.pts_f, c.d, add, b * N, N, m.raw_f, m.act_f))) return rc;
            if ((rc = snerf_composite_fwd_f32(m.raw_f, m.z_fine, c.d, 0, c.nz_f, b, N, wb, c.rgb_f, nullptr, nullptr, stream))) return rc;
        }
        if ((rc = launch_loss(a, sh, m, c, "nerf_train_grads(mse)"))) return rc;
        // backward: compositing, then dgrad + wgrad + reduce of each net (the hierarchical samples are detached, utils.py:260)
        if ((rc = cc.fork(who))) return rc;
        if (Nf > 0) {
            if ((rc = snerf_composite_bwd_f32(m.raw_f, m.z_fine, c.d, 0, c.nz_f, b, N, wb, m.d_rgb_f, sf.d_raw, nullptr, stream))) return rc;
            if ((rc = bwd(F, m.act_f, sf, b * N, r0 > 0, stream, w.concurrent ? b * Nc : 0))) return rc;
            if (d_add && (rc = contract_additional(F.desc, ig->params_fine, sf.dy, b * N, N, d_add + r0 * add_dim, true, m.contract, stream)))
                return rc;
        }
        if ((rc = snerf_composite_bwd_f32(m.raw_c, c.z, c.d, 0, c.nz_c, b, Nc, wb, m.d_rgb_c, sc.d_raw, nullptr, cc.stream_c))) return rc;
        if ((rc = bwd(C, m.act_c, sc, b * Nc, r0 > 0, cc.stream_c, w.concurrent ? b * N : 0))) return rc;
        if ((rc = cc.join(who))) return rc;
        // The collectives of the step are the same two on every rank, whatever its batch size, chunking and streams (RCCL matches
        // collectives by issue order and size; ADVICE r05: the concurrent form depends on the rank's own B): first the coarse net's
        // segment [cb0, cb1), then the rest of the flat buffer - both on `stream`, behind the join.
        // (r06, late: both on `stream`, behind the join.  r05 put the coarse bucket on the auxiliary stream beside the fine net's
        // backward - two collectives of ONE communicator in flight on two streams.  That has never run on more than one rank, it buys
        // the overlap of a 2.4 MB all-reduce, and it is the one pattern of the step RCCL does not promise to order for us: one stream.)
        if (a.comm && c.last && (rc = dp_allreduce_avg(a.comm, a.flat_g, cb0, cb1, 0, 0, cc.s, who_dp))) return rc;
        if (a.comm && c.last && (rc = dp_allreduce_avg(a.comm, a.flat_g, 0, a.flat_n, cb0, cb1, cc.s, who_dp))) return rc;
        // the coarse net's share of d loss / d additional inputs: behind the join (the two backwards may have run side by side; the
        // coarse net's d Y buffer is its own then), added to the fine net's
        if (d_add && (rc = contract_additional(C.desc, ig->params_coarse, sc.dy, b * Nc, Nc, d_add + r0 * add_dim, Nf == 0, m.contract, stream)))
            return rc;
    }
    return copy_rgb_fine(a, sh, who);
}

}  // namespace snerf

extern "C" int snerf_nerf_train_grads_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                          const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                          int precision, const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace,
                                          float *grad_coarse, float *grad_fine, float *loss, float *rgb, float *rgb_fine,
                                          snerf_stream_t stream, snerf_stream_t aux_stream) {
    snerf::TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream, a.aux_stream = aux_stream;
    return snerf::nerf_train_grads(a);
}

extern "C" int snerf_nerf_train_grads_ig_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                             const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                             int precision, const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace,
                                             float *grad_coarse, float *grad_fine, float *loss, float *rgb, float *rgb_fine,
                                             const snerf_input_grads *input_grads, snerf_stream_t stream, snerf_stream_t aux_stream) {
    snerf::TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream, a.aux_stream = aux_stream;
    a.input_grads = input_grads;
    return snerf::nerf_train_grads(a);
}

extern "C" int snerf_nerf_train_step_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                         const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                         int precision, const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace,
                                         float *grad_coarse, float *grad_fine, float *loss, float *rgb, float *rgb_fine,
                                         const snerf_adam_state *adam, const snerf_adam_range *ranges_host, int n_ranges,
                                         const snerf_adam_net *nets_host, int n_nets, snerf_stream_t stream, snerf_stream_t aux_stream) {
    snerf::TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream, a.aux_stream = aux_stream;
    if (int rc = snerf::nerf_train_grads(a)) return rc;
    return snerf::finish_step(a, {adam, ranges_host, n_ranges, nets_host, n_nets});
}

extern "C" int snerf_nerf_train_step_ig_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                            const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                            int precision, const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace,
                                            float *grad_coarse, float *grad_fine, float *loss, float *rgb, float *rgb_fine,
                                            const snerf_adam_state *adam, const snerf_adam_range *ranges_host, int n_ranges,
                                            const snerf_adam_net *nets_host, int n_nets, const snerf_input_grads *input_grads,
                                            snerf_stream_t stream, snerf_stream_t aux_stream) {
    snerf::TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream, a.aux_stream = aux_stream;
    a.input_grads = input_grads;
    // (the contraction reads the parameters: it runs inside the gradient half, before Adam moves them)
    if (int rc = snerf::nerf_train_grads(a)) return rc;
    return snerf::finish_step(a, {adam, ranges_host, n_ranges, nets_host, n_nets});
}

extern "C" int snerf_nerf_train_step_dp_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                            const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                            int precision, const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace,
                                            float *grad_coarse, float *grad_fine, float *loss, float *rgb, float *rgb_fine,
                                            const snerf_adam_state *adam, const snerf_adam_range *ranges_host, int n_ranges,
                                            const snerf_adam_net *nets_host, int n_nets, snerf_comm_t comm, snerf_stream_t stream,
                                            snerf_stream_t aux_stream) {
    using namespace snerf;
    if (!comm) return fail(SNERF_E_BADARG, "nerf_train_step_dp: comm is null (the single-GPU step is snerf_nerf_train_step_f32)");
    if (!adam || !adam->grads || adam->n_params < 1) return fail(SNERF_E_BADARG, "nerf_train_step_dp: adam / adam->grads is null");
    TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream, a.aux_stream = aux_stream;
    a.comm = comm, a.flat_g = const_cast<float *>(adam->grads), a.flat_n = adam->n_params;
    if (int rc = nerf_train_grads(a)) return rc;
    return finish_step(a, {adam, ranges_host, n_ranges, nets_host, n_nets});
}

extern "C" int snerf_nerf_train_step_dp_ig_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                               const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                               int precision, const snerf_nerf_batch *batch, int64_t rays_per_chunk, void *workspace,
                                               float *grad_coarse, float *grad_fine, float *loss, float *rgb, float *rgb_fine,
                                               const snerf_adam_state *adam, const snerf_adam_range *ranges_host, int n_ranges,
                                               const snerf_adam_net *nets_host, int n_nets, const snerf_input_grads *input_grads,
                                               snerf_comm_t comm, snerf_stream_t stream, snerf_stream_t aux_stream) {
    using namespace snerf;
    if (!comm) return fail(SNERF_E_BADARG, "nerf_train_step_dp_ig: comm is null (the single-GPU step is snerf_nerf_train_step_ig_f32)");
    if (!adam || !adam->grads || adam->n_params < 1) return fail(SNERF_E_BADARG, "nerf_train_step_dp_ig: adam / adam->grads is null");
    TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream, a.aux_stream = aux_stream;
    a.comm = comm, a.flat_g = const_cast<float *>(adam->grads), a.flat_n = adam->n_params;
    a.input_grads = input_grads;
    // (the contraction reads the parameters and the stored d Y: inside the gradient half, before the average and before Adam)
    if (int rc = nerf_train_grads(a)) return rc;
    return finish_step(a, {adam, ranges_host, n_ranges, nets_host, n_nets});
}

// ------------------------------------------------------------------------------------------------
// SmplNerfSolver.train's per-batch body (solver/smpl_nerf_solver.py:76-89 with the default loss; models/smpl_nerf_pipeline.py:16-100)
// ------------------------------------------------------------------------------------------------
namespace snerf {

// out = a + b (+ c): d loss / d warp = what arrives at the warped samples through the net's positions, through its
// per-sample view directions x' - o (and, in the coarse stage, through the compositing's distance scale |x' - o|)
__global__ __launch_bounds__(256) void sum3_kernel(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ c,
                                                   int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = __fadd_rn(a[i], b[i]);
    if (c) v = __fadd_rn(v, c[i]);
    out[i] = v;
}

struct SmplTrainWs {
    TrainWs base;
    int64_t warp_c, warped_c, sdirs_c, warp_f, warped_f, sdirs_f, act_wc, act_wf, d_x, d_dirs, d_cdirs, d_warp, dy_w, gpart_w;
    int64_t d_x2, d_dirs2, d_warp2, dy_w2, gpart_w2, grad_warp2;   // the coarse chain's own set (base.concurrent)
    int64_t total;
};

// a += b, element by element (the coarse chain's warp-net gradient joins the fine chain's in the order of the sequential form)
__global__ __launch_bounds__(256) void add_inplace_kernel(float *__restrict__ a, const float *__restrict__ b, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = __fadd_rn(a[i], b[i]);
}

static int smpl_train_ws(const snerf_mlp_desc *dc, const snerf_mlp_desc *df, const snerf_warp_desc *dw, int64_t chunk, int Nc, int Nf,
                         SmplTrainWs &w) {
    int rc;
    // small chunks: the coarse chain (compositing, net, warp net) has its own scratch set and may run beside the fine chain; both end
    // in the warp net's gradient, so the coarse chain's goes to a buffer of its own that is added behind the join
    if ((rc = train_ws(dc, df, chunk, Nc, Nf, w.base, true, SMPL_CONCURRENT_MAX_FINE_SAMPLES))) return rc;
    const int64_t N = Nc + Nf, nmax = chunk * (Nf > 0 ? N : Nc);
    int64_t act_c = 0, act_f = 0, dy_c = 0, dy_f = 0, gp_c = 0, gp_f = 0;
    if ((rc = snerf_warp_train_sizes(dw, chunk * Nc, &act_c, &dy_c, nullptr, &gp_c))) return rc;
    if (Nf > 0 && (rc = snerf_warp_train_sizes(dw, chunk * N, &act_f, &dy_f, nullptr, &gp_f))) return rc;
    int64_t off = align256(w.base.total);
    auto take = [&](int64_t floats) {
        const int64_t o = off;
        off += align256(floats * 4);
        return o;
    };
    w.warp_c = take(chunk * Nc * 3);
    w.warped_c = take(chunk * Nc * 3);
    w.sdirs_c = take(chunk * Nc * 3);
    w.warp_f = take(Nf > 0 ? chunk * N * 3 : 0);
    w.warped_f = take(Nf > 0 ? chunk * N * 3 : 0);
    w.sdirs_f = take(Nf > 0 ? chunk * N * 3 : 0);
    w.act_wc = take(act_c);
    w.act_wf = take(act_f);
    w.d_x = take(nmax * 3);
    w.d_dirs = take(nmax * 3);
    w.d_cdirs = take(chunk * Nc * 3);
    w.d_warp = take(nmax * 3);
    w.dy_w = take(dy_c > dy_f ? dy_c : dy_f);
    w.gpart_w = take(gp_c > gp_f ? gp_c : gp_f);
    const bool two = w.base.concurrent;
    const int64_t nw = snerf_warp_param_floats(dw);
    if (nw < 0) return (int)nw;
    w.d_x2 = take(two ? chunk * Nc * 3 : 0);
    w.d_dirs2 = take(two ? chunk * Nc * 3 : 0);
    w.d_warp2 = take(two ? chunk * Nc * 3 : 0);
    w.dy_w2 = take(two ? dy_c : 0);
    w.gpart_w2 = take(two ? gp_c : 0);
    w.grad_warp2 = take(two ? nw : 0);
    w.total = off;
    return SNERF_OK;
}

}  // namespace snerf

extern "C" int64_t snerf_smpl_nerf_train_workspace_bytes(const snerf_mlp_desc *desc_coarse, const snerf_mlp_desc *desc_fine,
                                                         const snerf_warp_desc *desc_warp, int64_t B, int Nc, int Nf,
                                                         int64_t rays_per_chunk) {
    using namespace snerf;
    if (!desc_coarse || !desc_warp || B < 0 || Nc < 1 || Nf < 0 || (Nf > 0 && !desc_fine))
        return fail(SNERF_E_BADARG, "smpl_nerf_train_workspace_bytes: bad arguments");
    SmplTrainWs w{};
    if (int rc = smpl_train_ws(desc_coarse, desc_fine, desc_warp, effective_chunk(B, rays_per_chunk), Nc, Nf, w)) return rc;
    return w.total;
}

namespace snerf {

// typed view of the smpl_nerf workspace.  set[0] / set[1] as in TrainBufs: set[1] is the coarse chain's own (base.concurrent)
struct WarpBwdSet {
    float *d_x, *d_dirs, *d_warp, *dy_w, *gpart_w;
};
struct SmplTrainBufs {
    TrainBufs base;
    float *warp_c, *warped_c, *sdirs_c, *warp_f, *warped_f, *sdirs_f, *act_wc, *act_wf, *d_cdirs, *grad_warp2;
    WarpBwdSet set[2];
};
static SmplTrainBufs carve(const SmplTrainWs &w, void *ws) {
    SmplTrainBufs m;
    m.base = carve(w.base, ws);
    m.warp_c = at(ws, w.warp_c), m.warped_c = at(ws, w.warped_c), m.sdirs_c = at(ws, w.sdirs_c), m.warp_f = at(ws, w.warp_f);
    m.warped_f = at(ws, w.warped_f), m.sdirs_f = at(ws, w.sdirs_f), m.act_wc = at(ws, w.act_wc), m.act_wf = at(ws, w.act_wf);
    m.d_cdirs = at(ws, w.d_cdirs), m.grad_warp2 = at(ws, w.grad_warp2);
    m.set[0] = {at(ws, w.d_x), at(ws, w.d_dirs), at(ws, w.d_warp), at(ws, w.dy_w), at(ws, w.gpart_w)};
    m.set[1] = {at(ws, w.d_x2), at(ws, w.d_dirs2), at(ws, w.d_warp2), at(ws, w.dy_w2), at(ws, w.gpart_w2)};
    return m;
}

// The gradient half of the smpl_nerf form.  aux_stream (may be NULL): small chunks run the coarse chain there beside the fine chain
// on `stream` - same results either way.  The step's collective follows in finish_step.
static int smpl_nerf_train_grads(const TrainArgs &a) {
    const char *const who = "smpl_nerf_train_grads";
    const NetArgs &C = a.coarse, &F = a.fine;
    const WarpArgs &W = a.warp;
    const snerf_nerf_batch *batch = a.batch;
    if (a.comm && batch && batch->B == 0) {
        if (!a.loss) return fail(SNERF_E_BADARG, "smpl_nerf_train_step_dp: loss is null");
        return dp_empty_shard(a, "smpl_nerf_train_step_dp");
    }
    Shape sh;
    int rc;
    if ((rc = decode_shape(a, 1, who, sh))) return rc;
    const int64_t B = sh.B;
    const int Nc = sh.Nc, Nf = sh.Nf, N = sh.N, precision = sh.precision;
    if (!C.desc || !C.packed || !C.packed_t || !W.desc || !W.packed || !W.packed_t || !batch->ray_samples || !batch->rays_o ||
        !batch->rays_d || !batch->z_vals || !batch->rgb_truth || !W.pose_enc || !a.workspace || !C.grad || !W.grad || !a.loss || !a.rgb ||
        !a.rgb_fine)
        return fail(SNERF_E_BADARG, "smpl_nerf_train_grads: null pointer");
    if (Nf > 0 && (!F.desc || !F.packed || !F.packed_t || !F.grad || !batch->u))
        return fail(SNERF_E_BADARG, "smpl_nerf_train_grads: the fine pass needs desc_fine, its streams, grad_fine and u");
    if (C.desc->add_dim || (Nf > 0 && F.desc->add_dim)) return fail(SNERF_E_BADARG, "smpl_nerf_train_grads: nets with additional inputs are not covered");
    if (!C.desc->use_dir || (Nf > 0 && !F.desc->use_dir))
        return fail(SNERF_E_BADARG, "smpl_nerf_train_grads: the nets read per-sample view directions (use_dir = 1)");
    if ((rc = check_workspace_and_width(a, sh, who))) return rc;
    SmplTrainWs w{};
    if ((rc = smpl_train_ws(C.desc, F.desc, W.desc, sh.chunk, Nc, Nf, w))) return rc;
    const SmplTrainBufs ms = carve(w, a.workspace);
    const TrainBufs &m = ms.base;
    Concurrent cc;
    if ((rc = concurrent_setup(a, w.base, cc))) return rc;
    const bool concurrent = cc.on;
    const BwdSet &sf = m.set[0], &sc = m.set[concurrent ? 1 : 0];
    const WarpBwdSet &wf = ms.set[0], &wc = ms.set[concurrent ? 1 : 0];
    float *grad_warp_c = concurrent ? ms.grad_warp2 : W.grad;
    const int64_t n_warp = snerf_warp_param_floats(W.desc);
    if (n_warp < 0) return (int)n_warp;
    const snerf_stream_t stream = a.stream, stream_c = cc.stream_c;
    const int wb = batch->white_background ? 1 : 0;
    const int pose_dim = W.desc->pose_dim;
    auto fwd_train = [&](const NetArgs &n, const float *x, const float *sd, int64_t cnt, int spr, float *raw, float *act) {
        MlpFwdCall c{n.desc, n.packed, x, sd, 1, nullptr, cnt, spr, raw, stream};
        c.act = act;
        c.train = true;
        return mlp_forward(precision, c);
    };
    auto bwd_inputs = [&](const NetArgs &n, const float *act, const BwdSet &t, const float *x, const float *sd, int64_t cnt, int spr,
                          const WarpBwdSet &u, bool accumulate, snerf_stream_t st) {
        MlpBwdCall c{n.desc, n.packed_t, act, t.d_raw, cnt, t.dy, t.gpart, n.grad, st, x, sd, 1, spr, u.d_x, u.d_dirs};
        c.accumulate = accumulate;
        c.beside_another_net = concurrent;
        c.n_beside = w.base.concurrent ? (spr == Nc ? cnt / Nc * N : cnt / N * Nc) : 0;
        return mlp_backward(precision, c);
    };
    auto sum3 = [&](const float *p, const float *q, const float *r, int64_t cnt, float *out, snerf_stream_t st) {
        hipLaunchKernelGGL(sum3_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (hipStream_t)st, p, q, r, cnt, out);
        return check_launch("smpl_nerf_train_grads(sum)");
    };
    for (int64_t r0 = 0; r0 < B; r0 += sh.chunk) {
        const Chunk c = chunk_of(a, sh, r0);
        const int64_t b = c.b;
        const float *pe = W.pose_enc + r0 * pose_dim;
        const bool acc = r0 > 0;
        // coarse stage: warp the given samples, net on (x', x' - o), compositing scaled per sample by |x' - o| (:38-63)
        if ((rc = snerf_warp_fwd_train_f32(W.desc, W.packed, c.x, pe, c.o, b * Nc, Nc, ms.warp_c, ms.warped_c, ms.sdirs_c, ms.act_wc, stream)))
            return rc;
        if ((rc = fwd_train(C, ms.warped_c, ms.sdirs_c, b * Nc, Nc, m.raw_c, m.act_c))) return rc;
        if ((rc = snerf_composite_fwd_f32(m.raw_c, c.z, ms.sdirs_c, 1, c.nz_c, b, Nc, wb, c.rgb_c, Nf > 0 ? m.weights_c : nullptr, nullptr, stream)))
            return rc;
        if (Nf > 0) {   // hierarchical samples on the un-warped ray (:68), then the fine stage (:71-98)
            if ((rc = sample_pdf_merged(sh.refsum, c.z, m.weights_c, batch->u, c.o, c.d, b, Nc, Nf, nullptr, nullptr, m.z_fine, m.pts_f, stream)))
                return rc;
            if ((rc = snerf_warp_fwd_train_f32(W.desc, W.packed, m.pts_f, pe, c.o, b * N, N, ms.warp_f, ms.warped_f, ms.sdirs_f, ms.act_wf, stream)))
                return rc;
            if ((rc = fwd_train(F, ms.warped_f, ms.sdirs_f, b * N, N, m.raw_f, m.act_f))) return rc;
            if ((rc = snerf_composite_fwd_f32(m.raw_f, m.z_fine, c.d, 0, c.nz_f, b, N, wb, c.rgb_f, nullptr, nullptr, stream))) return rc;
        }
        if ((rc = launch_loss(a, sh, m, c, "smpl_nerf_train_grads(mse)"))) return rc;
        if ((rc = cc.fork(who))) return rc;
        bool warp_acc = acc;
        if (Nf > 0) {   // fine: the compositing is scaled by the ray direction (an input), the net back-propagates into x' and x' - o
            if ((rc = snerf_composite_bwd_f32(m.raw_f, m.z_fine, c.d, 0, c.nz_f, b, N, wb, m.d_rgb_f, sf.d_raw, nullptr, stream))) return rc;
            if ((rc = bwd_inputs(F, m.act_f, sf, ms.warped_f, ms.sdirs_f, b * N, N, wf, acc, stream))) return rc;
            if ((rc = sum3(wf.d_x, wf.d_dirs, nullptr, b * N * 3, wf.d_warp, stream))) return rc;
            if ((rc = launch_warp_bwd(W.desc, W.packed_t, ms.act_wf, wf.d_warp, b * N, wf.dy_w, wf.gpart_w, W.grad, stream, warp_acc))) return rc;
            warp_acc = true;
        }
        // coarse: the compositing's distance scale |x' - o| depends on the warp as well (:63)
        if ((rc = snerf_composite_bwd_f32(m.raw_c, c.z, ms.sdirs_c, 1, c.nz_c, b, Nc, wb, m.d_rgb_c, sc.d_raw, ms.d_cdirs, stream_c))) return rc;
        if ((rc = bwd_inputs(C, m.act_c, sc, ms.warped_c, ms.sdirs_c, b * Nc, Nc, wc, acc, stream_c))) return rc;
        if ((rc = sum3(wc.d_x, wc.d_dirs, ms.d_cdirs, b * Nc * 3, wc.d_warp, stream_c))) return rc;
        if ((rc = launch_warp_bwd(W.desc, W.packed_t, ms.act_wc, wc.d_warp, b * Nc, wc.dy_w, wc.gpart_w, grad_warp_c, stream_c,
                                  concurrent ? false : warp_acc)))
            return rc;
        if (concurrent) {   // (concurrent implies Nf > 0: grad_warp holds the fine chain's sum by now)
            if ((rc = cc.join(who))) return rc;
            hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)((n_warp + 255) / 256)), dim3(256), 0, cc.s, W.grad, grad_warp_c, n_warp);
            if ((rc = check_launch("smpl_nerf_train_grads(add)"))) return rc;
        }
    }
    return copy_rgb_fine(a, sh, who);
}

}  // namespace snerf

extern "C" int snerf_smpl_nerf_train_grads_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                               const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                               const snerf_warp_desc *desc_warp, const float *packed_warp, const float *packed_t_warp,
                                               int precision, const snerf_nerf_batch *batch, const float *pose_enc,
                                               int64_t rays_per_chunk, void *workspace, float *grad_coarse, float *grad_fine,
                                               float *grad_warp, float *loss, float *rgb, float *rgb_fine, snerf_stream_t stream) {
    snerf::TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    // (the gradient half only reads the warp net's streams)
    a.warp = {desc_warp, const_cast<float *>(packed_warp), const_cast<float *>(packed_t_warp), grad_warp, pose_enc};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream;
    return snerf::smpl_nerf_train_grads(a);
}

extern "C" int snerf_smpl_nerf_train_grads_aux_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse,
                                                   const void *packed_t_coarse, const snerf_mlp_desc *desc_fine, const void *packed_fine,
                                                   const void *packed_t_fine, const snerf_warp_desc *desc_warp, const float *packed_warp,
                                                   const float *packed_t_warp, int precision, const snerf_nerf_batch *batch,
                                                   const float *pose_enc, int64_t rays_per_chunk, void *workspace, float *grad_coarse,
                                                   float *grad_fine, float *grad_warp, float *loss, float *rgb, float *rgb_fine,
                                                   snerf_stream_t stream, snerf_stream_t aux_stream) {
    snerf::TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    // (the gradient half only reads the warp net's streams)
    a.warp = {desc_warp, const_cast<float *>(packed_warp), const_cast<float *>(packed_t_warp), grad_warp, pose_enc};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream, a.aux_stream = aux_stream;
    return snerf::smpl_nerf_train_grads(a);
}

// comm (may be NULL): the flat gradient buffer is averaged over the ranks between the backward and Adam
extern "C" int snerf_smpl_nerf_train_step_aux_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                                  const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                                  const snerf_warp_desc *desc_warp, float *packed_warp, float *packed_t_warp, int precision,
                                                  const snerf_nerf_batch *batch, const float *pose_enc, int64_t rays_per_chunk,
                                                  void *workspace, float *grad_coarse, float *grad_fine, float *grad_warp, float *loss,
                                                  float *rgb, float *rgb_fine, const snerf_adam_state *adam,
                                                  const snerf_adam_range *ranges_host, int n_ranges, const snerf_adam_net *nets_host,
                                                  int n_nets, int64_t warp_param_offset, snerf_comm_t comm, snerf_stream_t stream,
                                                  snerf_stream_t aux_stream) {
    using namespace snerf;
    if (comm && (!adam || !adam->grads || adam->n_params < 1))
        return fail(SNERF_E_BADARG, "smpl_nerf_train_step_aux: the data-parallel step needs adam->grads");
    TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    a.warp = {desc_warp, packed_warp, packed_t_warp, grad_warp, pose_enc};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream, a.aux_stream = aux_stream;
    if (comm) a.comm = comm, a.flat_g = const_cast<float *>(adam->grads), a.flat_n = adam->n_params;
    if (int rc = smpl_nerf_train_grads(a)) return rc;
    return finish_step(a, {adam, ranges_host, n_ranges, nets_host, n_nets}, "smpl_nerf_train_step_aux", warp_param_offset);
}

extern "C" int snerf_smpl_nerf_train_step_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                              const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                              const snerf_warp_desc *desc_warp, float *packed_warp, float *packed_t_warp, int precision,
                                              const snerf_nerf_batch *batch, const float *pose_enc, int64_t rays_per_chunk,
                                              void *workspace, float *grad_coarse, float *grad_fine, float *grad_warp, float *loss,
                                              float *rgb, float *rgb_fine, const snerf_adam_state *adam,
                                              const snerf_adam_range *ranges_host, int n_ranges, const snerf_adam_net *nets_host,
                                              int n_nets, int64_t warp_param_offset, snerf_stream_t stream) {
    using namespace snerf;
    TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    a.warp = {desc_warp, packed_warp, packed_t_warp, grad_warp, pose_enc};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream;
    if (int rc = smpl_nerf_train_grads(a)) return rc;
    return finish_step(a, {adam, ranges_host, n_ranges, nets_host, n_nets}, "smpl_nerf_train_step", warp_param_offset);
}

extern "C" int snerf_smpl_nerf_train_step_dp_f32(const snerf_mlp_desc *desc_coarse, const void *packed_coarse, const void *packed_t_coarse,
                                                 const snerf_mlp_desc *desc_fine, const void *packed_fine, const void *packed_t_fine,
                                                 const snerf_warp_desc *desc_warp, float *packed_warp, float *packed_t_warp, int precision,
                                                 const snerf_nerf_batch *batch, const float *pose_enc, int64_t rays_per_chunk,
                                                 void *workspace, float *grad_coarse, float *grad_fine, float *grad_warp, float *loss,
                                                 float *rgb, float *rgb_fine, const snerf_adam_state *adam,
                                                 const snerf_adam_range *ranges_host, int n_ranges, const snerf_adam_net *nets_host,
                                                 int n_nets, int64_t warp_param_offset, snerf_comm_t comm, snerf_stream_t stream) {
    using namespace snerf;
    if (!comm) return fail(SNERF_E_BADARG, "smpl_nerf_train_step_dp: comm is null (the single-GPU step is snerf_smpl_nerf_train_step_f32)");
    if (!adam || !adam->grads || adam->n_params < 1) return fail(SNERF_E_BADARG, "smpl_nerf_train_step_dp: adam / adam->grads is null");
    TrainArgs a{};
    a.coarse = {desc_coarse, packed_coarse, packed_t_coarse, grad_coarse};
    a.fine = {desc_fine, packed_fine, packed_t_fine, grad_fine};
    a.warp = {desc_warp, packed_warp, packed_t_warp, grad_warp, pose_enc};
    a.precision = precision, a.batch = batch, a.rays_per_chunk = rays_per_chunk, a.workspace = workspace;
    a.loss = loss, a.rgb = rgb, a.rgb_fine = rgb_fine, a.stream = stream;
    a.comm = comm, a.flat_g = const_cast<float *>(adam->grads), a.flat_n = adam->n_params;
    if (int rc = smpl_nerf_train_grads(a)) return rc;
    return finish_step(a, {adam, ranges_host, n_ranges, nets_host, n_nets}, "smpl_nerf_train_step_dp", warp_param_offset);
}

extern "C" int snerf_warp_repack_f32(const snerf_warp_desc *desc_warp, const float *params, int64_t n_params, int64_t warp_param_offset,
                                     float *packed_warp, float *packed_t_warp, snerf_stream_t stream) {
    using namespace snerf;
    const int64_t nw = snerf_warp_param_floats(desc_warp);
    if (nw < 0) return (int)nw;
    if (!params || warp_param_offset < 0 || warp_param_offset + nw > n_params)
        return fail(SNERF_E_BADARG, "warp_repack: the warp net does not lie inside the flat parameter buffer");
    int rc;
    if (packed_warp && (rc = snerf_warp_pack_f32(desc_warp, params + warp_param_offset, packed_warp, stream))) return rc;
    if (packed_t_warp && (rc = snerf_warp_pack_t_f32(desc_warp, params + warp_param_offset, packed_t_warp, stream))) return rc;
    return SNERF_OK;
}
