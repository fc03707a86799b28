// Shared host/device helpers for libsmplnerf_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include <atomic>
#include <type_traits>

#include "../../include/smplnerf.h"

namespace snerf {

// thread-local error text behind snerf_last_error_string()
char *err_buf();
int fail(int code, const char *fmt, ...);

// SNERF_DEBUG_POISON_LDS=1 (debug aid, tests/test_gpu_round4.py): after every checked launch a kernel on the NULL stream
// fills the LDS of every CU with NaNs, so that a kernel that reads LDS it has not written meets NaNs instead of whatever
// the previous kernel left there (the first process on a freshly booted GPU meets arbitrary bits).
void debug_poison_lds();
inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SNERF_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    debug_poison_lds();
    return SNERF_OK;
}

// ---- process-wide state of the library (all of it; include/smplnerf.h "State") ------------------------------------
// The CU count and hipFuncAttributeMaxDynamicSharedMemorySize are PER DEVICE: both are cached per HIP device ordinal of
// the calling thread's current device, so one process may drive several GPUs through the library.
constexpr int MAX_DEVICES = 64;
// CU count of the current device (cached per device); returns < 1 and sets the error text on failure
int device_cu_count(const char *what);
// "dynamic LDS limit of this kernel raised to N bytes on device d" - one per kernel instantiation (function-local static)
struct LdsRaised {
    std::atomic<int> bytes[MAX_DEVICES];
};
// raises the limit once per (kernel, device); idempotent, a race only repeats the driver call.  Returns 0 or SNERF_E_LAUNCH.
int raise_dynamic_lds(const void *kernel, int bytes, LdsRaised &state, const char *what);
// The launch of a kernel whose dynamic LDS may exceed the 64 KiB every launch gets: raises the limit of `Kernel` to `limit_bytes`
// (once per device: the LdsRaised is a static of the instantiation, i.e. of the kernel; 0 = this launch needs no raise) and launches
// with `lds_bytes`.  A kernel whose launches differ in size passes ONE constant limit, so that every raise of a kernel asks for the
// same value and threads that race only repeat the driver call.  Returns SNERF_OK or the error of the raise (`what` names the
// caller in its text); the launch itself is checked by the caller's check_launch(), which may stand behind several launches.
template <auto Kernel, class... Args>
int launch_lds_limit(const char *what, dim3 grid, dim3 block, int lds_bytes, int limit_bytes, hipStream_t s, const Args &...args) {
    static LdsRaised raised;
    if (limit_bytes > 0)
        if (int rc = raise_dynamic_lds(reinterpret_cast<const void *>(Kernel), limit_bytes, raised, what)) return rc;
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, s, args...);
    return SNERF_OK;
}
// ... for a kernel whose launches all ask for the same size: the limit is that size
template <auto Kernel, class... Args>
int launch_lds(const char *what, dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const Args &...args) {
    return launch_lds_limit<Kernel>(what, grid, block, lds_bytes, lds_bytes, s, args...);
}

// ---- host: which instantiation a call runs ----------------------------------------------------------------------------------------
// f(std::integral_constant<int, W>{}) for the W of the list that is `width`
template <int W0, int... Ws, class F>
int with_width(int width, F &&f) {
    if (width == W0) return f(std::integral_constant<int, W0>{});
    if constexpr (sizeof...(Ws) > 0) return with_width<Ws...>(width, f);
    else return fail(SNERF_E_BADARG, "no kernel of width %d", width);
}
// the kernel widths of a RenderRayNet plan (mlp_plan.h make_plan: P.width) and of a WarpFieldNet plan (make_warp_plan).  (The order
// of a list is the order in which a translation unit emits its kernels: the one the hand-written ladders had.)
template <class F>
int with_mlp_width(int width, F &&f) { return with_width<320, 384, 448, 512, 256, 128, 64>(width, f); }
template <class F>
int with_warp_width(int width, F &&f) { return with_width<256, 128>(width, f); }

// Waves per sample tile (16 samples per wave) of a forward or dgrad call of a net of kernel width `width` on the throughput
// kernels.  8 waves = 128 samples per workgroup, one workgroup per CU, 2 waves per SIMD.  The widths above 256 run one wave per SIMD
// (20 .. 32-tile chains need the whole register file).  Small calls (the README's 64-ray batches: 4096 + 12 288 samples): while
// 64-sample tiles still fit one round of the chip the 4-wave form finishes in about half the time of a 128-sample tile's pass
// through the weight stream - a call of up to 64 x CUs samples is one tile's latency, not throughput (same per-sample
// arithmetic: bit-identical results; r04: dgrad 290 -> 190 us at 4096 samples).
constexpr int FWD_WAVES = 8;
inline int tile_waves(int width, int64_t n, int n_cu) { return (width > 256 || n <= (int64_t)64 * n_cu) ? 4 : FWD_WAVES; }

// Tuning knobs: environment variables read ONCE, at the first call that consults them (INTEGRATION.md lists every knob of the
// library and of the Python host).  r06: the A/B switches of rounds 2-5 whose experiments are decided are gone (their patches
// and scripts under tools/ab/ are the record); what is left switches the per-ray folds and the composed stream of inference off.
struct Tuning {
    bool warp_fold;   // SNERF_WARP_FOLD=0   warp inference: pose k-blocks per sample instead of the per-ray fold
    bool mlp_fold;    // SNERF_MLP_FOLD=0    fp32 inference: per-ray additional inputs as k-blocks per sample
    bool mlp_compose; // SNERF_MLP_COMPOSE=0 fp32 inference: no composed stream (snerf_mlp_packed_infer_floats returns 0: the regular one)
};
const Tuning &tuning();

// sampler.hip: snerf_sample_pdf_f32's merged form for the render / training entries; refsum = the normalising sum in the
// reference's order (SNERF_REFERENCE_SUM ORed into their precision), computed in the kernel
int sample_pdf_merged(bool refsum, const float *z, const float *weights, const float *u, const float *o, const float *d, int64_t B,
                      int Nc, int Nf, int64_t *inds, float *z_samples, float *z_fine, float *pts, snerf_stream_t stream);

__host__ __device__ inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

constexpr int WAVE = 64;

// ---- wave-level primitives (64-wide wavefronts) ------------------------------------------------
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Wavefront scans and sums on the DPP network (row_shr within rows of 16 lanes, row_bcast:15 / :31 across rows - the GFX9
// sequence): one VALU move per 32 bits and step instead of a ds_bpermute with its index arithmetic.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_take(float identity, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, identity), __builtin_bit_cast(int, v), CTRL,
                                                                 ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_take(double identity, double v) {
    const long long o = __builtin_bit_cast(long long, identity), x = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)x, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(x >> 32), CTRL, ROW_MASK, 0xf, false);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// inclusive prefix sum / product over the 64 lanes (lanes without a source take the identity)
template <class T>
__device__ __forceinline__ T wave_scan_add(T v, int /*lane*/ = 0) {
    v += dpp_take<0x111, 0xf>(T(0), v);   // row_shr:1
    v += dpp_take<0x112, 0xf>(T(0), v);   // row_shr:2
    v += dpp_take<0x114, 0xf>(T(0), v);   // row_shr:4
    v += dpp_take<0x118, 0xf>(T(0), v);   // row_shr:8
    v += dpp_take<0x142, 0xa>(T(0), v);   // row_bcast:15 -> rows 1, 3
    v += dpp_take<0x143, 0xc>(T(0), v);   // row_bcast:31 -> rows 2, 3
    return v;
}
template <class T>
__device__ __forceinline__ T wave_scan_mul(T v, int /*lane*/ = 0) {
    v *= dpp_take<0x111, 0xf>(T(1), v);
    v *= dpp_take<0x112, 0xf>(T(1), v);
    v *= dpp_take<0x114, 0xf>(T(1), v);
    v *= dpp_take<0x118, 0xf>(T(1), v);
    v *= dpp_take<0x142, 0xa>(T(1), v);
    v *= dpp_take<0x143, 0xc>(T(1), v);
    return v;
}
__device__ __forceinline__ float wave_last(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63)); }
__device__ __forceinline__ double wave_last(double v) {
    const long long x = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), 63);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// lane i <- lane i-1 (wave_shr:1); lane 0 takes `first`
template <class T>
__device__ __forceinline__ T wave_shift_up1(T v, T first) { return dpp_take<0x138, 0xf>(first, v); }
// the sum over the 64 lanes, in every lane (a scan whose last lane is broadcast through an SGPR)
__device__ __forceinline__ float wave_sum(float v) { return wave_last(wave_scan_add(v)); }
__device__ __forceinline__ double wave_sum(double v) { return wave_last(wave_scan_add(v)); }

}  // namespace snerf
