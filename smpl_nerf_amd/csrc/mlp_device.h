// Device-side building blocks shared by the forward (mlp.hip) and training (mlp_train.hip) kernels: the two slab pipes - SlabPipeDma
// (L2 -> LDS by global_load_lds into a 4-slot ring: the headline inference kernel of width 256 and every kernel of the widths above
// 256) and SlabPipe (L2 -> registers -> 3-slot LDS ring: training forward and dgrad up to width 256) -, the k-block MFMA step, the
// layer walker and the in-register positional-encoding operands.  See mlp_plan.h for the operand algebra.  Host side: the plan
// preamble of every entry (plan_for), the call records and precision dispatch of the two directions, the forward checks and fill.
#pragma once
#include <type_traits>
#include "snerf_common.h"
#include "mlp_plan.h"

namespace snerf {

typedef float f4 __attribute__((ext_vector_type(4)));

struct TrainLayout;
// defined in mlp_train.hip: split-K wgrad + fixed-order reduce for any (Plan, TrainLayout)
// n_beside: samples of ANOTHER net's weight gradient that runs on a second stream at the same time (train_step.hip: the coarse
// net's backward beside the fine net's), 0 = this launch has the chip to itself - small calls then split their jobs for their
// share of the CUs, n / (n + n_beside), so that both nets' workgroups are resident in one round
int launch_wgrad(const Plan &P, const TrainLayout &L, const float *act, const float *dy, int64_t n, float *gpart,
                 float *flat_grad, hipStream_t s, int wide_nsplit = 0, bool accumulate = false, int64_t n_beside = 0);
// ---- host: the preamble of every entry that takes a descriptor, of either net: null check, plan, "<what>: <why>" when the plan
// refuses it.  (Here and not beside make_plan: mlp_plan.h stays free of the HIP headers, tests/native/plan_sanitize.cpp compiles it
// alone.)
inline int make_plan(const snerf_warp_desc &d, Plan &P, const char *&why, int kw) { return make_warp_plan(d, P, why, kw); }
template <class Desc>
int plan_for(const char *what, const Desc *desc, Plan &P, int kw = 16) {
    const char *why;
    if (!desc) return fail(SNERF_E_BADARG, "%s: desc is null", what);
    if (make_plan(*desc, P, why, kw) != 0) return fail(SNERF_E_BADARG, "%s: %s", what, why);
    return SNERF_OK;
}
// ... of the fp32 inference entries: the composed plan (mlp_plan.h: make_plan_infer)
inline int plan_infer_for(const char *what, const snerf_mlp_desc *desc, Plan &P) {
    const char *why;
    if (!desc) return fail(SNERF_E_BADARG, "%s: desc is null", what);
    if (make_plan_infer(*desc, P, why) != 0) return fail(SNERF_E_BADARG, "%s: %s", what, why);
    return SNERF_OK;
}
// ... of the split-precision entries, whose kernels exist for width 256 alone
template <class Desc>
int plan_for_256(const char *what, const Desc *desc, Plan &P, int kw) {
    if (int rc = plan_for(what, desc, P, kw)) return rc;
    if (desc->width != 256) return fail(SNERF_E_BADARG, "%s: the split-bf16 path supports width 256 only", what);
    return SNERF_OK;
}

// ---- one call of a RenderRayNet, forward or backward: what the C-ABI entries and the one-call render / training entries hand to
// the implementations below.  The members up to `stream` are set by every caller, in this order; the others only where needed.
struct MlpFwdCall {
    const snerf_mlp_desc *desc;
    const void *packed;    // the fp32 stream or a split-precision one
    const float *x, *dirs;
    int dirs_per_sample;   // a boolean; the fp32 inference alone reads the bit set of SNERF_FWD_*
    const float *add;
    int64_t n;
    int spr;
    float *raw;
    snerf_stream_t stream;
    float *act = nullptr;          // training forward (`train`): the activation buffer
    bool train = false;
    void *workspace = nullptr;     // fp32 inference: room for the per-ray fold table (snerf_mlp_fold_workspace_bytes)
    int64_t workspace_bytes = 0;
    bool infer = false;            // fp32 inference on the composed stream: `packed` comes from snerf_mlp_pack_infer_f32
};
struct MlpBwdCall {
    const snerf_mlp_desc *desc;
    const void *packed_t;
    const float *act, *d_raw;
    int64_t n;
    float *dy, *gpart, *flat_grad;
    snerf_stream_t stream;
    const float *x = nullptr, *dirs = nullptr;   // input gradients (d_x != null): the forward inputs ...
    int dirs_per_sample = 0, spr = 1;
    float *d_x = nullptr, *d_dirs = nullptr;     // ... and their gradients
    bool accumulate = false;           // flat_grad += instead of = (train_step.hip)
    bool beside_another_net = false;   // the caller runs another net's backward on a second stream at the same time (train_step.hip)
    int64_t n_beside = 0;              // ... on this many samples (launch_wgrad)
};
// defined in mlp.hip / mlp_bf16.hip: the bodies of snerf_mlp_fwd_f32, _fwd_ws_f32, _fwd_train_f32 and of their split-precision twins
int launch_mlp_fwd(const MlpFwdCall &c);
int launch_mlp_fwd_bf16(int nsplit, const MlpFwdCall &c);
// defined in mlp_train.hip / mlp_train_bf16.hip: dgrad + wgrad + reduce of one net on n samples (the bodies of snerf_mlp_bwd_f32 /
// snerf_mlp_bwd_inputs_f32 and their split-precision twins)
int launch_bwd(const MlpBwdCall &c);
int launch_bwd_bf16(int nsplit, const MlpBwdCall &c);
// `precision` of the one-call entries: 0 = the fp32 kernels, SNERF_FP32_INFER = the fp32 kernels on the composed inference stream
// (render entries only), otherwise the nsplit of the split-precision ones
inline int mlp_forward(int precision, const MlpFwdCall &c) {
    if (precision == SNERF_FP32_INFER) {
        MlpFwdCall ci = c;
        ci.infer = true;
        return launch_mlp_fwd(ci);
    }
    return precision == 0 ? launch_mlp_fwd(c) : launch_mlp_fwd_bf16(precision, c);
}
inline int mlp_backward(int precision, const MlpBwdCall &c) { return precision == 0 ? launch_bwd(c) : launch_bwd_bf16(precision, c); }
// defined in warp.hip: the body of snerf_warp_bwd_f32
int launch_warp_bwd(const snerf_warp_desc *desc, const float *packed_t, const float *act, const float *d_warp, int64_t n, float *dy,
                    float *gpart, float *flat_grad, snerf_stream_t stream, bool accumulate = false);
// defined in mlp_lat.hip: the latency-class kernels of small calls, and which form a call takes (mode 0: the throughput kernel alone,
// 1: the latency kernels alone, 2: the throughput kernel on the first n_main samples - whole rounds of the chip - and the latency
// kernels on the rest)
struct LatChoice {
    int mode;
    int64_t n_main;
};
struct FwdArgs;
struct BwdArgs;
template <bool TRAIN>
LatChoice lat_choose_fwd(const Plan &P, int64_t n);
template <bool TRAIN>
int launch_fwd_lat(const Plan &P, const FwdArgs &A, hipStream_t s, int64_t first_sample);
LatChoice lat_choose_bwd(const Plan &P, int64_t n, bool input_grad, bool beside_another_net = false);
int launch_bwd_lat(const Plan &P, const BwdArgs &A, hipStream_t s, int64_t first_sample);
// defined in mlp.hip: packs params_flat into the slab stream described by `P` (any plan; a composed plan takes its composed layers
// from `composed_params`)
int launch_pack(const Plan &P, const float *params_flat, float *packed, hipStream_t s, const char *what, const float *composed_params = nullptr);

// ------------------------------------------------------------------------------------------------
// forward kernel
// ------------------------------------------------------------------------------------------------
struct FwdArgs {
    const float *packed;
    const float *x;      // [n,3] positions, or x_enc [n, enc_stride] when ENCODED
    const float *dirs;   // [n/spr,3] or [n,3]
    const float *add;    // [n/spr, add_dim] or null
    float *raw;          // [n,4]
    int64_t n;
    int spr;             // samples per ray
    int dirs_per_sample;
    int n_hidden;        // positional_net layers
    unsigned skip_mask;
    int pos_L, pos_id, pos_nkb, pos_dim;
    int dir_L, dir_id, dir_nkb, dir_dim;
    int add_dim, add_nkb, add_first;
    int use_dir;
    int enc_stride;
    // training only: activation buffer in tile-row-major layout (mlp_plan.h TrainLayout)
    float *act;
    int act_pe, act_add, act_dpe, act_x1, act_o, act_h1, act_h2, act_mask;
    // inference with per-ray additional inputs (FOLD instantiation): fold[(ray * fold_slots + slot) * WIDTH + o] =
    // sum_c W_l[o, add columns] * add[ray][c] for layer 0 (slot 0) and the skip layers in order (mlp.hip: mlp_add_fold_kernel)
    const float *fold;
    int fold_slots;
    int no_fold;         // (host only) the caller asked for the per-sample form: SNERF_FWD_NO_RAY_FOLD
    float *fold_ws;      // (host only) caller's workspace for the per-ray fold table, or null: per-sample form
    int64_t fold_ws_bytes;
    int act_rows;      // f16x3 training forward: the per-layer |X| exponents go behind this many tile-rows of `act`
    // split-bf16 training forward only: encoder / additional k-block counts of the 16-wide (fp32) plan, which
    // defines the activation layout the backward kernels read
    int pos_nkb16, add_nkb16, dir_nkb16;
    int total_slabs;   // slabs of the weight stream (persistent workgroups wrap around)
    int64_t n_tiles;   // sample tiles (NWAVES x 16 samples)
    int composed;      // inference on the stream of make_plan_infer: behind the trunk come sigma', dir-net' (ReLU) and the rgb head
};

// ---- host: what every forward entry (mlp.hip, mlp_bf16.hip) checks and fills alike; `what` prefixes every error text ----
// encoded: x holds whole encoded rows - no rays, hence no samples_per_ray, dirs or add.  (n == 0 is valid with any pointers:
// SNERF_OK, and the caller returns before it touches them.)
inline int check_fwd_args(const char *what, const Plan &P, const MlpFwdCall &c, bool encoded = false) {
    if (c.n < 0 || c.spr < 1) return fail(SNERF_E_BADARG, "%s: bad n%s", what, encoded ? "" : "/samples_per_ray");
    if (c.n == 0) return SNERF_OK;
    if (!c.packed || !c.x || !c.raw || (c.train && !c.act)) return fail(SNERF_E_BADARG, "%s: null pointer", what);
    if (!encoded && c.desc->use_dir && !c.dirs) return fail(SNERF_E_BADARG, "%s: dirs is null", what);
    if (!encoded && P.add_dim && !c.add) return fail(SNERF_E_BADARG, "%s: add is null", what);
    if (!aligned(c.packed, 16) || !aligned(c.raw, 16) || (c.train && !aligned(c.act, 16)))
        return fail(SNERF_E_ALIGN, "%s: packed/raw%s must be 16-byte aligned", what, c.train ? "/act" : "");
    return SNERF_OK;
}
// everything of FwdArgs that the call, the descriptor and the plan determine; left to the launches: total_slabs, n_tiles, the fold
inline FwdArgs fill_fwd_args(const Plan &P, const MlpFwdCall &c) {
    const snerf_mlp_desc *desc = c.desc;
    FwdArgs A{};
    A.packed = reinterpret_cast<const float *>(c.packed);
    A.x = c.x;
    A.dirs = c.dirs;
    A.add = c.add;
    A.raw = c.raw;
    A.n = c.n;
    A.spr = c.spr;
    A.dirs_per_sample = c.dirs_per_sample ? 1 : 0;
    A.n_hidden = P.n_hidden;
    A.skip_mask = desc->skip_mask;
    A.pos_L = desc->pos_freqs;
    A.pos_id = desc->pos_identity ? 1 : 0;
    A.pos_nkb = P.pos_nkb;
    A.pos_dim = P.pos_dim;
    A.dir_L = desc->dir_freqs;
    A.dir_id = desc->dir_identity ? 1 : 0;
    A.dir_nkb = P.dir_nkb;
    A.dir_dim = P.dir_dim;
    A.add_dim = P.add_dim;
    A.add_nkb = P.add_nkb;
    A.add_first = (P.add_dim && desc->add_first) ? 1 : 0;
    A.use_dir = desc->use_dir ? 1 : 0;
    A.enc_stride = P.pos_dim + P.add_dim + (desc->use_dir ? P.dir_dim : 0);
    A.composed = P.composed;
    return A;
}
// the activation buffer of a training forward; P16: the 16-wide plan, whose TrainLayout (mlp_plan.h) the backward kernels read
inline void set_train_layout(FwdArgs &A, const Plan &P16, float *act) {
    TrainLayout L;
    make_train_layout(P16, L);
    A.act = act;
    A.act_pe = L.pe;
    A.act_add = L.add;
    A.act_dpe = L.dpe;
    A.act_x1 = L.x[1];
    A.act_o = L.o;
    A.act_h1 = L.h1;
    A.act_h2 = L.h2;
    A.act_mask = L.mask;
    A.act_rows = L.act_rows;
}

// one tile (16 features of this lane's sample) <-> the tile-row-major activation buffer
__device__ __forceinline__ void store_tile(float *buf, int row, int64_t n, int64_t sample, int g, f4 v) {
    __builtin_nontemporal_store(v, reinterpret_cast<f4 *>(buf + ((int64_t)row * n + sample) * 16 + 4 * g));
}
template <int N>
__device__ __forceinline__ void store_tiles(float *buf, int row0, int64_t n, int64_t sample, int g, const f4 (&tiles)[N]) {
#pragma unroll
    for (int t = 0; t < N; ++t) store_tile(buf, row0 + t, n, sample, g, tiles[t]);
}
__device__ __forceinline__ f4 load_tile(const float *buf, int row, int64_t n, int64_t sample, int g) {
    return *reinterpret_cast<const f4 *>(buf + ((int64_t)row * n + sample) * 16 + 4 * g);
}

// ReLU sign mask of one layer output for the split-bf16 dgrad kernel: bit 4 t + r of this lane's 64-bit word is
// (tiles[t][r] > 0).  Mask `idx` lives in tile-row mask_row + idx / 2, floats (idx & 1) * 8 + 2 g of the sample.
__device__ __forceinline__ uint2 *mask_ptr(const float *buf, int mask_row, int idx, int64_t n, int64_t sample, int g) {
    return reinterpret_cast<uint2 *>(const_cast<float *>(buf) + ((int64_t)(mask_row + (idx >> 1)) * n + sample) * 16 +
                                     (idx & 1) * 8 + 2 * g);
}
// 32-tile layers (width 512): mask `idx` is tile-row mask_row + idx, 16 bytes per lane group
__device__ __forceinline__ uint4 *mask_ptr4(const float *buf, int mask_row, int idx, int64_t n, int64_t sample, int g) {
    return reinterpret_cast<uint4 *>(const_cast<float *>(buf) + ((int64_t)(mask_row + idx) * n + sample) * 16 + 4 * g);
}
// ROW_PER_MASK: the layout of a net with 32-tile layers (also for its 16-tile directional branch, which stores two words there)
template <int N, bool ROW_PER_MASK = (N > 16)>
__device__ __forceinline__ void store_mask(float *buf, int mask_row, int idx, int64_t n, int64_t sample, int g,
                                           const f4 (&tiles)[N]) {
    static_assert(N <= 32, "up to four mask words");
    static_assert(N <= 16 || ROW_PER_MASK, "four words need a tile-row of their own");
    constexpr int NWORDS = N <= 16 ? 2 : 4;
    unsigned w[NWORDS];
#pragma unroll
    for (int q = 0; q < NWORDS; ++q) w[q] = 0u;
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // x > 0 <=> its bit pattern, read as a signed integer, is > 0: clamp to {0, 1} and shift into place
            const int bit = min(max(__float_as_int(tiles[t][r]), 0), 1);
            w[t >> 3] |= static_cast<unsigned>(bit) << (((t & 7) << 2) | r);
        }
    // the address is formed here, not hoisted to the top of the tile (where it would cost two registers per layer)
    asm volatile("" : "+v"(sample));
    if constexpr (N <= 16 && ROW_PER_MASK) {
        *reinterpret_cast<uint2 *>(mask_ptr4(buf, mask_row, idx, n, sample, g)) = uint2{w[0], w[1]};
    } else if constexpr (N <= 16) {
        *mask_ptr(buf, mask_row, idx, n, sample, g) = uint2{w[0], w[1]};
    } else {   // 32 tiles: four words per lane, one mask per tile-row (TrainLayout::mask)
        *mask_ptr4(buf, mask_row, idx, n, sample, g) = uint4{w[0], w[1], w[2], w[3]};
    }
}

// The weight ring of a kernel is dynamic LDS, 99 or 132 KiB: a launch gets 64 KiB unless the limit is raised per kernel once
// (snerf_common.h: launch_lds).  A kernel names its pipe through the traits behind the two pipes (FwdPipe / BwdPipe / WarpPipe), and
// its launch takes the LDS size from the same type.

// Streams the slab sequence global -> registers -> LDS ring (3 slots).
template <int NT>
struct SlabPipe {
    static constexpr int RING_BYTES = 3 * SLAB_FLOATS * 4;   // 99 KiB
    static constexpr int NA = SLAB_A_FLOATS / 4 / NT;  // f4 per thread in the A region (NT=256: 4, 512: 2)
    const f4 *g;   // this thread's read cursor in the packed stream
    const f4 *g0;  // ... and its position at slab 0: persistent kernels run the stream once per sample tile and wrap
    int src, total;
    float *ring;
    f4 st[NA], st_aux;
    f4 pa0, pa1;  // first A-operand pair of the next k-block, prefetched (see kblock)
    int tid, rd, wr;

    __device__ __forceinline__ void load() {
#pragma unroll
        for (int i = 0; i < NA; ++i) st[i] = g[i * NT];
        if (tid < 64) st_aux = g[SLAB_A_FLOATS / 4];
        g += SLAB_FLOATS / 4;
        if (++src == total) {
            src = 0;
            g = g0;
        }
    }
    __device__ __forceinline__ void store(int slot) {
        f4 *d = reinterpret_cast<f4 *>(ring + slot * SLAB_FLOATS) + tid;
#pragma unroll
        for (int i = 0; i < NA; ++i) d[i * NT] = st[i];
        if (tid < 64) d[SLAB_A_FLOATS / 4] = st_aux;
    }
    // total_slabs: length of the stream for kernels that run it repeatedly (one pass per sample tile); a one-pass kernel
    // leaves the default and reads on into the zero padding slabs
    __device__ __forceinline__ void prologue(const float *packed, float *ring_, int tid_, int total_slabs = 0x7fffffff) {
        ring = ring_;
        tid = tid_;
        g = g0 = reinterpret_cast<const f4 *>(packed) + tid;
        src = 0;
        total = total_slabs;
        load(); store(0);
        load(); store(1);
        load();
        rd = 0;
        wr = 2;
        __syncthreads();
        const f4 *np = reinterpret_cast<const f4 *>(ring) + (tid & 63);
        pa0 = np[0];
        pa1 = np[64];
    }
    __device__ __forceinline__ const float *acquire() const { return ring + rd * SLAB_FLOATS; }
    __device__ __forceinline__ const float *peek_next() const { return ring + (rd == 2 ? 0 : rd + 1) * SLAB_FLOATS; }
    // the two halves of release(): stage() may run anywhere inside the current slab's MFMAs (slot `wr` has been free since the
    // barrier that ended the previous slab), advance() ends the slab
    __device__ __forceinline__ void stage() {
        store(wr);
        load();
    }
    __device__ __forceinline__ void advance() {
        __syncthreads();
        rd = rd == 2 ? 0 : rd + 1;
        wr = wr == 2 ? 0 : wr + 1;
    }
    __device__ __forceinline__ void release() {
        stage();
        advance();
    }
    __device__ __forceinline__ void drain() {}   // (loads into registers: nothing of this pipe can land after the kernel)
};

// The same interface with the slabs copied global -> LDS by DMA (`global_load_lds_dwordx4`, 16 B per lane: one instruction moves
// a 1 KiB piece) into a 4-slot ring: no staging registers and a fraction of the instructions per slab of the register-staged
// pipe.  Each issued piece blocks the issuing wave for ~60 cycles (DESIGN_HISTORY 3.1).
//
// The DMA instructions are inline asm, and so are the waits and the barrier that end a slab.  Issued through the builtin, hipcc
// counts every piece as a pending LDS write: `__syncthreads()` then drains the ring with `s_waitcnt vmcnt(0)` at every slab, and
// with a raw barrier instead every LDS-read wait of the kernel degrades to `lgkmcnt(0)` (the pending "flat" operation makes the
// counter unordered for the compiler), which serialises the A-operand prefetch of kblock() - as it did behind stage() in every
// slab of the builtin form, which also spent a v_readfirstlane and a 64-bit add per piece.  Hidden from the compiler, a slab's
// pieces are one M0 write and four instructions with immediate offsets, cost it no wait and no register (the 8-wave kernel:
// 223 -> 199 VGPRs); their completion is counted here by hand.  That, not the longer landing time, is what the headline kernel
// gained (37.3 -> 35.9 ms per frame; with `vmcnt(0)` at the barrier the asm form measures the same: DESIGN_HISTORY 3.1).
// tests/test_weight_ring_isa.py holds the compiled kernel to the waits described here.
//
// Ring, while slab p is consumed (period p, barrier to barrier): p+1 resident, p+2 landing (issued in period p-1), p+3 issued
// by stage() into the slot of p-1.  advance() ends period p with `s_waitcnt vmcnt(N)`, N = this wave's pieces of ONE slab
// (PPW, + 1 for wave 0: the aux block), `s_waitcnt lgkmcnt(0)` and a raw `s_barrier`.  The safety argument, in counts:
//   * vmcnt counts a wave's outstanding vector memory operations, loads and stores alike.  All the argument needs of the
//     hardware is that LOADS (LDS-DMA pieces included) complete in issue order among themselves; stores may complete in any
//     order.  Every period issues exactly one stage() (LayerRun::step / skip / finish: one stage() per advance(), partial slabs
//     of the sigma / rgb / directional layers included), so at advance() of period p the N pieces of slab p+3 have been issued
//     behind the pieces of slab p+2.  If a piece of p+2 were still outstanding, so would be all N newer pieces of p+3, and the
//     count would be at least N + 1: `vmcnt(N)` cannot pass.  Whatever else the kernel body has outstanding (the next tile's
//     inputs, the result store, additional-input or encoded operands, activation stores of a training forward) only adds to
//     the count: the wait can then last longer than slab p+2 needs (it also waits for some pieces of p+3: slower, never wrong),
//     never shorter.  A hipcc wait for one of ITS loads is `vmcnt(k)` with k counting only the later operations it knows:
//     the pieces it does not know only add to the count, so that is an over-wait, too.
//   * RAW: slab p+2 is complete in LDS once EVERY wave has passed its vmcnt(N) of period p, i.e. behind the barrier ending period
//     p.  Its first read is the peek_next() prefetch (A pair, and the second bias block of 32-tile layers) in period p+1.  The
//     prologue waits for slabs 0 .. 2 with vmcnt(0) before its barrier.
//   * WAR: slot (p-1) & 3 is overwritten by pieces issued in period p.  The last LDS reads of slab p-1 are issued in period p-1
//     (program order: LDS reads and the asm statements do not cross, "memory"), and `lgkmcnt(0)` ahead of the barrier ending p-1
//     retires them in every wave - wherever hipcc put the MFMAs that consume them.  The pair prefetched across the barrier reads
//     slab p, which is not overwritten before period p+1.
//   * The stream of a persistent kernel wraps around (issue(): src == total) with the ring rolling on: the same counts hold across
//     tiles.  drain() waits for the slabs issued ahead of the last one consumed before the workgroup's LDS is given back.
template <int NT>
struct SlabPipeDma {
    static constexpr int RING_BYTES = 4 * SLAB_FLOATS * 4;   // 132 KiB
    static constexpr int NW = NT / 64;
    static constexpr int PIECES = SLAB_A_FLOATS / 256;   // 1 KiB pieces of the A region (32); the aux block is one more (wave 0)
    static constexpr int PPW = PIECES / NW;
    static_assert(PIECES % NW == 0 && PPW % 4 == 0, "pieces divide over the waves, in groups of four");
    const float *g, *g0;   // this lane's cursor in the stream (slab `src`, piece wave * PPW, lane's 16 B) and its position at slab 0
    int src, total;
    float *ring;
    f4 pa0, pa1;
    int tid, rd, wr;
    unsigned lds0;   // LDS byte address of this wave's first piece in slot 0
    bool w0;

    // NP (1 or 4) consecutive 1 KiB pieces, global `src` (this lane's 16 B) -> LDS byte address `dst` (wave-uniform; the hardware adds
    // lane * 16 B, and the instruction offset moves both addresses).  M0 carries the LDS address; the compiler owns it, so it is
    // written in the statement that reads it and restored.
    template <int NP>
    __device__ __forceinline__ static void dma(const float *src, unsigned dst) {
        static_assert(NP == 1 || NP == 4, "one piece or four");
        unsigned keep;
        if constexpr (NP == 4)
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                         "global_load_lds_dwordx4 %1, off\n\t"
                         "global_load_lds_dwordx4 %1, off offset:1024\n\t"
                         "global_load_lds_dwordx4 %1, off offset:2048\n\t"
                         "global_load_lds_dwordx4 %1, off offset:3072\n\t"
                         "s_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
        else
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                         "global_load_lds_dwordx4 %1, off\n\t"
                         "s_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    }
    __device__ __forceinline__ void issue(int slot) {
        // this wave's first piece in the slot (wave-uniform; said so where hipcc cannot prove it of `slot`)
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + slot * (SLAB_FLOATS * 4));
#pragma unroll
        for (int i = 0; i < PPW; i += 4) dma<4>(g + i * 256, dst + i * 1024);
        if (w0) dma<1>(g + SLAB_A_FLOATS, dst + SLAB_A_FLOATS * 4);   // wave-uniform (wave 0: dst is the slot's first byte)
        g += SLAB_FLOATS;
        if (++src == total) {
            src = 0;
            g = g0;
        }
    }
    __device__ __forceinline__ void prologue(const float *packed, float *ring_, int tid_, int total_slabs = 0x7fffffff) {
        ring = ring_;
        tid = tid_;
        w0 = __builtin_amdgcn_readfirstlane(tid_ >> 6) == 0;
        lds0 = __builtin_amdgcn_readfirstlane(
            (unsigned)(size_t)(__attribute__((address_space(3))) float *)ring_ + (unsigned)(tid_ >> 6) * (PPW * 1024));
        g = g0 = packed + (tid_ >> 6) * PPW * 256 + (tid_ & 63) * 4;   // (wave 0: the slab's first byte + the lane's 16)
        src = 0;
        total = total_slabs;
        issue(0);
        issue(1);
        issue(2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        rd = 0;
        wr = 3;
        __syncthreads();   // (a bare s_barrier: hipcc knows of no pending operation)
        const f4 *np = reinterpret_cast<const f4 *>(ring) + (tid & 63);
        pa0 = np[0];
        pa1 = np[64];
    }
    __device__ __forceinline__ const float *acquire() const { return ring + rd * SLAB_FLOATS; }
    __device__ __forceinline__ const float *peek_next() const { return ring + ((rd + 1) & 3) * SLAB_FLOATS; }
    __device__ __forceinline__ void stage() { issue(wr); }
    __device__ __forceinline__ void advance() {
        // all but this wave's newest slab has landed (see above); never vmcnt(0), never __syncthreads() here
        if (w0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW + 1) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        rd = (rd + 1) & 3;
        wr = (wr + 1) & 3;
    }
    __device__ __forceinline__ void release() {
        stage();
        advance();
    }
    // end of the kernel: the slabs issued ahead of the last one consumed are still landing in this workgroup's LDS
    __device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// Which kernel takes which pipe - stated here once, for the kernel bodies (the type of their `pipe`) and for their launches (the
// dynamic LDS they ask for is Pipe::RING_BYTES of the same alias).  r05 measurements, DESIGN_HISTORY.md; the A/B switches that
// selected the pipes are gone, the patches under tools/ab/ are the record.
// Forward, training forward (TRAIN) and the per-ray fold kernel (TRAIN = false) - mlp.hip: the widths above 256 (one wave per SIMD)
// and the 8-wave inference kernels of width 256 stream their slabs by DMA into the 4-slot ring; the others - the training forward
// and the 4-wave tiles of small calls up to width 256 - measured no gain from it and keep the register-staged 3-slot ring.
template <int WIDTH, int NWAVES, bool TRAIN>
using FwdPipe = std::conditional_t<(WIDTH > 256 || (!TRAIN && WIDTH == 256 && NWAVES == 8)), SlabPipeDma<NWAVES * 64>, SlabPipe<NWAVES * 64>>;
// dgrad (mlp_train.hip): DMA for the widths above 256 only
template <int WIDTH, int NWAVES>
using BwdPipe = std::conditional_t<(WIDTH > 256), SlabPipeDma<NWAVES * 64>, SlabPipe<NWAVES * 64>>;
// the slab-streaming warp forward (warp.hip)
template <int NWAVES>
using WarpPipe = SlabPipe<NWAVES * 64>;

// per-lane view of the sample this lane works for
struct SampleCtx {
    float px, py, pz;  // position
    float dx, dy, dz;  // normalised direction
    const float *enc;  // row of x_enc (ENCODED) or null
    const float *add;  // row of add or null
    int g;
};

__device__ __forceinline__ void pe_unit(float x, float y, float z, int L, int ident, int p, float &a, float &b) {
    const int nid = ident ? 3 : 0;
    a = 0.f;
    b = 0.f;
    if (p < nid) {
        a = p == 0 ? x : (p == 1 ? y : z);
        return;
    }
    const int pp = p - nid;
    if (pp >= 3 * L) return;
    const int k = pp / 3, c = pp - 3 * k;
    const float v = c == 0 ? x : (c == 1 ? y : z);
    sincosf(ldexpf(v, k), &a, &b);  // 2^k * v is exact: same argument bits as utils.py:127
}

// B operand (4 k-steps) of PE k-block kb for this lane
template <bool ENCODED>
__device__ __forceinline__ f4 pe_operand(const SampleCtx &c, bool is_dir, int L, int ident, int kb, int enc_off) {
    f4 b;
    if (ENCODED) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = pe_slot_col(L, ident, kb, c.g, r);
            b[r] = col >= 0 ? c.enc[enc_off + col] : 0.f;
        }
    } else {
        const float x = is_dir ? c.dx : c.px, y = is_dir ? c.dy : c.py, z = is_dir ? c.dz : c.pz;
        float s0, c0, s1, c1;
        pe_unit(x, y, z, L, ident, 4 * (2 * kb) + c.g, s0, c0);
        pe_unit(x, y, z, L, ident, 4 * (2 * kb + 1) + c.g, s1, c1);
        b = f4{s0, c0, s1, c1};
    }
    return b;
}

__device__ __forceinline__ f4 add_operand(const SampleCtx &c, int add_dim, int kb) {
    f4 b;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int col = 16 * kb + 4 * c.g + r;
        b[r] = col < add_dim ? c.add[col] : 0.f;
    }
    return b;
}

// One k-block: T_OUT x (ds_read_b128 + 4 MFMA).  Tiles are walked in pairs so that consecutive MFMAs
// never share an accumulator (dependent latency of 16x16x4 is 40 cycles vs 32 issue).
// One k-block: T_OUT x (ds_read_b128 + 4 MFMA), software-pipelined: the A values of tile pair p+1 are read
// from LDS while the 8 MFMAs of pair p issue, and the first pair of the NEXT k-block (`next`, possibly in the
// next slab) is read during the last pair - so a wave never waits on an LDS read between MFMAs.  Tiles are
// walked in pairs so that consecutive MFMAs never share an accumulator (dependent latency of 16x16x4 is 40
// cycles vs 32 issue).  (pa0, pa1) carry the prefetched first pair from k-block to k-block.
// The hazard of this placement: the read at the top of a pair may be given the accumulator quad that the previous pair's last
// MFMA still reads as SrcC (hipcc renames the result into dead A registers), and then stands behind 7 - 8 wait states of `s_nop`
// that no MFMA covers.  The 8-wave inference kernels of width 256, where that cost 1.6 % of the frame, go through kblock_deep()
// below, which avoids it (tests/test_mfma_gap_isa.py holds them to it); every other kernel keeps this form, unchanged.
// mid(): called once between two tile pairs early in the block (LayerRun: the staging of the slab after next, so that its LDS
// writes and global loads issue between MFMAs instead of behind the slab's last one)
struct NoMid {
    __device__ __forceinline__ void operator()() const {}
};
template <int T_OUT, class Mid = NoMid>
__device__ __forceinline__ void kblock(const float *a_kb, const float *a_next, f4 b, f4 (&acc)[T_OUT], f4 &pa0, f4 &pa1,
                                       int lane, Mid mid = Mid{}) {
    const f4 *ap = reinterpret_cast<const f4 *>(a_kb) + lane;
    const f4 *np = reinterpret_cast<const f4 *>(a_next) + lane;
    if constexpr (T_OUT == 1) {
        const f4 a = pa0;
        pa0 = np[0];
        pa1 = np[64];
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc[0], 0, 0, 0);
    } else {
        f4 a0 = pa0, a1 = pa1;
#pragma unroll
        for (int to = 0; to < T_OUT; to += 2) {
            f4 n0, n1;
            if (to + 2 < T_OUT) {
                n0 = ap[(to + 2) * 64];
                n1 = ap[(to + 3) * 64];
            } else {
                n0 = np[0];
                n1 = np[64];
            }
            // pin the schedule: the two LDS reads of the NEXT pair issue first, then the 8 MFMAs of this pair
            // alternating between the two accumulators (hipcc otherwise sinks the reads to their first use and
            // groups the MFMAs by accumulator, which exposes both the LDS and the 40-cycle dependent latency)
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // 2 DS reads
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[r], b[r], acc[to], 0, 0, 0);
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                acc[to + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[r], b[r], acc[to + 1], 0, 0, 0);
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (to == (T_OUT >= 8 ? 2 : 0)) {
                mid();
                __builtin_amdgcn_sched_barrier(0);
            }
            a0 = n0;
            a1 = n1;
        }
        pa0 = a0;
        pa1 = a1;
    }
}

// kblock() with the prefetch TWO tile pairs ahead and pinned behind the pair's 2nd MFMA (T_OUT >= 8; the 8-wave inference kernels
// of width 256: LayerRun<.., DEEP>).  Why: hipcc lets the last MFMA of an accumulation chain - and many a pair's last MFMA in the
// middle of one - write its result into the A-operand registers that just died and hands the old accumulator quad to the next
// ds_read_b128.  With the reads at the top of the next pair (kblock()) that read stands right behind the MFMA that still reads
// those registers as SrcC, and the hazard recognizer separates the two with `s_nop 6` / `s_nop 7`: 28 - 32 clocks that no MFMA
// covers, in 1 gap of 20.  Two MFMAs further on the quad has been read and the `s_nop` is gone or short enough (<= 6 wait
// states = 24 clocks + the MFMA's own 8) to fit beside the MFMA in front of it.  Reading one pair ahead from there would make every
// wait a full `lgkmcnt(0)` (nothing younger in flight at the top of a pair); two pairs ahead, a third A pair (8 VGPRs), the wait
// at the top of pair p+1 leaves the reads of pair p+2 in flight (`lgkmcnt(2)`) and every read has 14 MFMAs to land.
// (pa0, pa1) = the next pair as in kblock(); (pb0, pb1) = the pair behind it (LayerRun primes it per layer).  The MFMA order of
// every accumulator is kblock()'s.  tests/test_mfma_gap_isa.py holds the compiled kernels to this; tests/test_weight_ring_isa.py
// to the counted waits.
template <int T_OUT, class Mid = NoMid>
__device__ __forceinline__ void kblock_deep(const float *a_kb, const float *a_next, f4 b, f4 (&acc)[T_OUT], f4 &pa0, f4 &pa1,
                                            f4 &pb0, f4 &pb1, int lane, Mid mid = Mid{}) {
    static_assert(T_OUT >= 8 && T_OUT % 2 == 0, "two pairs ahead stay inside this k-block and the next one");
    const f4 *ap = reinterpret_cast<const f4 *>(a_kb) + lane;
    const f4 *np = reinterpret_cast<const f4 *>(a_next) + lane;
    f4 a0 = pa0, a1 = pa1, b0 = pb0, b1 = pb1;
#pragma unroll
    for (int to = 0; to < T_OUT; to += 2) {
        f4 n0, n1;
        if (to + 4 < T_OUT) {
            n0 = ap[(to + 4) * 64];
            n1 = ap[(to + 5) * 64];
        } else {   // the first two pairs of the next k-block (`a_next`: possibly in the next slab, or the next layer's first)
            n0 = np[(to + 4 - T_OUT) * 64];
            n1 = np[(to + 5 - T_OUT) * 64];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[r], b[r], acc[to], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
            acc[to + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[r], b[r], acc[to + 1], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
            if (r == 0) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // the 2 DS reads of pair to/2 + 2, behind the 2nd MFMA
        }
        __builtin_amdgcn_sched_barrier(0);
        if (to == 2) {
            mid();
            __builtin_amdgcn_sched_barrier(0);
        }
        a0 = b0;
        a1 = b1;
        b0 = n0;
        b1 = n1;
    }
    pa0 = a0;
    pa1 = a1;
    pb0 = b0;
    pb1 = b1;
}

// Walks the k-blocks of one layer through the slab pipe (either one: PIPE).  A slab is released (the next slab staged - SlabPipe: the
// registers written to LDS and the next global loads issued; SlabPipeDma: the DMA pieces of slab p+3 issued -, workgroup barrier)
// as soon as its last k-block has been issued; the first A pair of the following slab was read before that barrier - legal
// because slab p+1 has been resident and visible since the barrier that ended slab p-1 (the 3-slot ring holds p, p+1 and the slot
// being filled with p+2; the 4-slot ring p, p+1, p+2 landing and the slot of p+3).
// DEEP (T_OUT >= 8): the k-blocks go through kblock_deep(); the second prefetched pair lives here, per layer - primed from the
// layer's first k-block (resident: the layer starts in `slab`), dropped at the layer's end (the last pair's read of the block
// behind the layer stays inside that slab's A region: tiles 2 and 3).
template <bool DEEP>
struct DeepPair {};
template <>
struct DeepPair<true> {
    f4 pb0, pb1;   // the A-operand pair behind (pipe.pa0, pipe.pa1)
};
template <int T_OUT, int NT, class PIPE, bool DEEP = false>
struct LayerRun : DeepPair<DEEP> {
    static constexpr int KPS = SLAB_TILES / T_OUT;
    static_assert(!DEEP || T_OUT >= 8, "kblock_deep");
    PIPE &pipe;
    const float *slab;
    int kbl;  // k-block index inside the current slab
    int lane;

    __device__ __forceinline__ LayerRun(PIPE &p, int lane_) : pipe(p), slab(p.acquire()), kbl(0), lane(lane_) {
        if constexpr (DEEP) prime(slab);
    }
    // DEEP: (pb0, pb1) = tiles 2 and 3 of the k-block at `kb` - whose tiles 0 and 1 are in (pipe.pa0, pipe.pa1)
    __device__ __forceinline__ void prime(const float *kb) {
        const f4 *p = reinterpret_cast<const f4 *>(kb) + lane;
        this->pb0 = p[2 * 64];
        this->pb1 = p[3 * 64];
    }
    // bias -> accumulator init (aux block of the layer's first slab: bias[16*to + 4*g + r])
    __device__ __forceinline__ void init(f4 (&acc)[T_OUT]) {
        const f4 *aux = reinterpret_cast<const f4 *>(slab + SLAB_A_FLOATS) + (lane >> 4);
#pragma unroll
        for (int to = 0; to < (T_OUT < 16 ? T_OUT : 16); ++to) acc[to] = aux[to * 4];
        if constexpr (T_OUT > 16) {   // tiles 16 .. : the bias block of the layer's second slab (resident: LayerRun above)
            const f4 *aux2 = reinterpret_cast<const f4 *>(pipe.peek_next() + SLAB_A_FLOATS) + (lane >> 4);
#pragma unroll
            for (int to = 16; to < T_OUT; ++to) acc[to] = aux2[(to - 16) * 4];
        }
    }
    __device__ __forceinline__ void step(f4 b, f4 (&acc)[T_OUT]) {
        const float *cur = slab + kbl * (T_OUT * 256);
        const float *nxt = (kbl + 1 < KPS) ? cur + T_OUT * 256 : pipe.peek_next();
        if constexpr (T_OUT >= 8) {
            const bool last = kbl + 1 == KPS;     // the slab's last k-block carries the staging between its MFMAs
            auto mid = [&]() __attribute__((always_inline)) {
                if (last) pipe.stage();
            };
            if constexpr (DEEP) kblock_deep<T_OUT>(cur, nxt, b, acc, pipe.pa0, pipe.pa1, this->pb0, this->pb1, lane, mid);
            else kblock<T_OUT>(cur, nxt, b, acc, pipe.pa0, pipe.pa1, lane, mid);
            if (++kbl == KPS) {
                pipe.advance();
                slab = pipe.acquire();
                kbl = 0;
            }
        } else {
            kblock<T_OUT>(cur, nxt, b, acc, pipe.pa0, pipe.pa1, lane);
            if (++kbl == KPS) {
                pipe.release();
                slab = pipe.acquire();
                kbl = 0;
            }
        }
    }
    // a k-block of the stream that is not multiplied (FOLD: the additional-input columns arrive as a per-ray vector):
    // advance like step() and re-prime the A-operand prefetch from the block behind it
    __device__ __forceinline__ void skip() {
        const float *cur = slab + kbl * (T_OUT * 256);
        const f4 *np = reinterpret_cast<const f4 *>((kbl + 1 < KPS) ? cur + T_OUT * 256 : pipe.peek_next()) + lane;
        pipe.pa0 = np[0];
        pipe.pa1 = np[64];
        if constexpr (DEEP) {
            this->pb0 = np[2 * 64];
            this->pb1 = np[3 * 64];
        }
        if (++kbl == KPS) {
            pipe.release();
            slab = pipe.acquire();
            kbl = 0;
        }
    }
    // end of the layer: a partially consumed slab is dropped (its tail is padding) and the prefetched pair
    // re-read from the slab the next layer starts in
    __device__ __forceinline__ void finish() {
        if (kbl != 0) {
            const f4 *np = reinterpret_cast<const f4 *>(pipe.peek_next()) + lane;
            pipe.pa0 = np[0];
            pipe.pa1 = np[64];
            pipe.release();
        }
    }
};

template <int N>
__device__ __forceinline__ void relu_into(f4 (&dst)[N], const f4 (&src)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        dst[i][0] = fmaxf(src[i][0], 0.f);
        dst[i][1] = fmaxf(src[i][1], 0.f);
        dst[i][2] = fmaxf(src[i][2], 0.f);
        dst[i][3] = fmaxf(src[i][3], 0.f);
    }
}
template <int N>
__device__ __forceinline__ void copy_into(f4 (&dst)[N], const f4 (&src)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) dst[i] = src[i];
}


}  // namespace snerf
