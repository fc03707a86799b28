// The soft silhouette of a posed triangle mesh and its gradient with respect to the vertices (legacy/neural_mesh_renderer.py asks
// kaolin's differentiable renderer for it; this is NOT kaolin's rule): per pixel the probabilistic union of SoftRas,
// 1 - prod_f (1 - sigmoid(+-d^2 / sigma)), written as a float64 sum of softplus terms.  The rule is the one written out in
// include/smplnerf.h (snerf_soft_silhouette_fwd_f32), operation by operation.
//
// Precision: the projection of every vertex runs once per frame and face in float64 (pre-pass) and is rounded once to fp32; the
// pair test - three segment distances, three edge functions: is the pixel inside, is the pair within the cutoff - runs in fp32 on
// those corners, products and sums kept apart (-ffp-contract=off); a pair that contributes has its distance, nearest segment, t and
// r recomputed in float64 on the same corners; z, softplus, sigmoid, every sum and the chain rule through the projection run in
// float64.
//
// Forward mapping (mesh_render.hip's): workgroup = one 8 x 8 pixel tile of one frame, lane = pixel, its 8 waves split the faces
// (wave_slice), walk them at wave-uniform addresses (walk4; the culled walk takes eight boxes per wait while eight are left), each
// lane keeps a float64 L, the partials meet in LDS and wave 0 adds them in wave order.
//
// Pre-pass (per call, into the workspace): per frame and face the six fp32 projected coordinates (NaN for a face that is not live)
// and the box of ss_box below.
//
// The cull: a pair outside the rule's cutoff contributes exactly 0, so a tile may skip every face whose box misses it: every
// output equals the brute-force walk (SNERF_RENDER_NO_CULL) bit for bit.
//
// Backward, face-major, no atomics: one wave per (frame, face) walks the pixels of the face's box, clipped to the image, in
// row-major order - lane l takes pixels l, l + 64, ... -, each lane keeps six float64 partials (the gradient with respect to the three
// projected corners), the wave adds them over its lanes in one fixed order (wave_sum), takes them through the projection and writes
// nine float64 to the workspace.  A gather, one thread per (body, vertex), adds the vertex's corners in CSR order - frames ascending
// for a shared body - and rounds once.
#include "mesh_tile.h"

namespace snerf {

constexpr int SS_WAVES = 8;                    // forward: waves of a workgroup = slices of the face axis
constexpr int SS_BWD_WAVES = 4;                // backward: faces (waves) of a workgroup
constexpr double SS_COORD_MAX = 1073741824.0;  // 2^30: a projected coordinate at or beyond it makes the face not live

// ---- the pair rule ------------------------------------------------------------------------------------------------------------
// The squared distance from q to the segment a -> a + e, with w = q - a: t = clamp((w . e) / (e . e), 0, 1), 0 for a zero-length edge
// (fmax drops a NaN); r = w - t e.  In fp32 for the decision, in float64 for the value.
template <class T>
struct SsSeg {
    T d2, t, rx, ry;
};
template <class T>
__device__ __forceinline__ SsSeg<T> ss_segment(T ex, T ey, T wx, T wy) {
    const T ee = ex * ex + ey * ey;
    const T t = ee > T(0) ? fmin(fmax((wx * ex + wy * ey) / ee, T(0)), T(1)) : T(0);
    SsSeg<T> s;
    s.t = t;
    s.rx = wx - t * ex;
    s.ry = wy - t * ey;
    s.d2 = s.rx * s.rx + s.ry * s.ry;
    return s;
}

// Pixel (qx, qy) against the projected corners P = (x0, y0, x1, y1, x2, y2) in the arithmetic T: the nearest of the segments
// 0: p0 p1, 1: p1 p2, 2: p2 p0 (the lower index on a tie) and, with EDGES, whether the pixel is inside.
template <class T>
struct SsPair {
    SsSeg<T> s;
    int seg;
    bool inside;
};
template <class T, bool EDGES>
__device__ __forceinline__ SsPair<T> ss_pair(T qx, T qy, const float *P) {
    T ex[3], ey[3], wx[3], wy[3], edge[3];
    SsSeg<T> s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = k == 2 ? 0 : k + 1;
        ex[k] = (T)P[2 * k1] - (T)P[2 * k];
        ey[k] = (T)P[2 * k1 + 1] - (T)P[2 * k + 1];
        wx[k] = qx - (T)P[2 * k];
        wy[k] = qy - (T)P[2 * k + 1];
        edge[k] = ex[k] * wy[k] - ey[k] * wx[k];
        s[k] = ss_segment(ex[k], ey[k], wx[k], wy[k]);
    }
    // (selects on scalars: a struct chosen by index would go through scratch memory)
    const bool take1 = s[1].d2 < s[0].d2;
    const T d01 = take1 ? s[1].d2 : s[0].d2;
    const bool take2 = s[2].d2 < d01;
    SsPair<T> p;
    p.seg = take2 ? 2 : take1 ? 1 : 0;
    p.s.d2 = take2 ? s[2].d2 : d01;
    p.s.t = take2 ? s[2].t : take1 ? s[1].t : s[0].t;
    p.s.rx = take2 ? s[2].rx : take1 ? s[1].rx : s[0].rx;
    p.s.ry = take2 ? s[2].ry : take1 ? s[1].ry : s[0].ry;
    p.inside = false;
    if constexpr (EDGES) {
        const bool sign = (edge[0] > T(0) && edge[1] > T(0) && edge[2] > T(0)) || (edge[0] < T(0) && edge[1] < T(0) && edge[2] < T(0));
        // (what exact arithmetic implies, asked of the fp32 signs: a pixel inside a triangle lies in its corners' bounding box)
        const bool in_box = qx >= fmin((T)P[0], fmin((T)P[2], (T)P[4])) && qx <= fmax((T)P[0], fmax((T)P[2], (T)P[4])) &&
                            qy >= fmin((T)P[1], fmin((T)P[3], (T)P[5])) && qy <= fmax((T)P[1], fmax((T)P[3], (T)P[5]));
        p.inside = sign && in_box;
    }
    return p;
}

// The decision, in fp32: is the pixel inside, and does the pair contribute - it does unless it is outside and beyond the cutoff
// (a NaN distance is refused too).
struct SsTest {
    bool inside, contributes;
};
__device__ __forceinline__ SsTest ss_test(int i, int j, const float *P, double cut2) {
    const SsPair<float> p = ss_pair<float, true>((float)i, (float)j, P);
    return {p.inside, p.inside || (double)p.s.d2 <= cut2};
}
// The value of a contributing pair, in float64 on the same fp32 corners: the fp32 distances leave the nearest segment open where a
// pixel's foot point is near a vertex (d2 moves by eps where t moves by sqrt(eps)), and t shares the gradient between two corners.
__device__ __forceinline__ SsPair<double> ss_value(int i, int j, const float *P) { return ss_pair<double, false>((double)i, (double)j, P); }
__device__ __forceinline__ double ss_z(bool inside, double d2, double sigma) { return (inside ? d2 : -d2) / sigma; }
__device__ __forceinline__ double ss_softplus(double z) { return fmax(z, 0.0) + log1p(exp(-fabs(z))); }
__device__ __forceinline__ double ss_sigmoid(double z) {
    const double e = exp(-fabs(z));
    return (z >= 0.0 ? 1.0 : e) / (1.0 + e);
}

// ---- the projection, float64 ---------------------------------------------------------------------------------------------------
// c = R^T (v - o), depth = -c.z, x = W/2 + focal c.x / depth, y = H/2 - focal c.y / depth
struct SsProj {
    double c[3], depth, x, y;
};
__device__ __forceinline__ SsProj ss_project(const float *v, const MrCamera &C, double focal, int H, int W) {
    double p[3];
    SsProj s;
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = (double)v[i] - (double)C.o[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) s.c[i] = p[0] * C.R[0][i] + p[1] * C.R[1][i] + p[2] * C.R[2][i];
    s.depth = -s.c[2];
    s.x = W * 0.5 + focal * s.c[0] / s.depth;
    s.y = H * 0.5 - focal * s.c[1] / s.depth;
    return s;
}

// The box of a live face: the bounding box of its three projected corners, widened by `reach` = sqrt(cutoff sigma) pixels plus a
// margin for the fp32 roundings of the pair test, rounded outward to whole pixels.  A pixel outside it is farther than `reach` from
// the triangle by more than the margin, and outside the corners' own box, so the pair rule finds it outside and beyond the cutoff:
// exactly 0.  The margin: every fp32 intermediate of a segment distance carries a relative error of a few 2^-24 on quantities
// bounded by twice M = the largest coordinate magnitude among the corners, W and H; the computed distance is within 16 2^-24 M of
// the true one, and the margin is 1 + 2^-18 M.  A face that is not live gets the empty box.
__device__ __forceinline__ void ss_box(const SsProj (&s)[3], bool live, int H, int W, double reach, int32_t (&box)[4]) {
    box[0] = box[2] = INT32_MAX;
    box[1] = box[3] = INT32_MIN;
    if (!live) return;
    const double x0 = fmin(s[0].x, fmin(s[1].x, s[2].x)), x1 = fmax(s[0].x, fmax(s[1].x, s[2].x));
    const double y0 = fmin(s[0].y, fmin(s[1].y, s[2].y)), y1 = fmax(s[0].y, fmax(s[1].y, s[2].y));
    const double M = fmax(fmax(fmax(fabs(x0), fabs(x1)), fmax(fabs(y0), fabs(y1))), (double)max(H, W));
    const double m = reach + 1.0 + M * 3.814697265625e-06;
    const double lim = 2147483000.0;
    box[0] = (int32_t)fmax(floor(x0 - m), -lim);
    box[1] = (int32_t)fmin(ceil(x1 + m), lim);
    box[2] = (int32_t)fmax(floor(y0 - m), -lim);
    box[3] = (int32_t)fmin(ceil(y1 + m), lim);
}

__device__ __forceinline__ bool ss_live(const SsProj (&s)[3]) {
    bool live = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) live = live && s[k].depth > 0.0 && fabs(s[k].x) < SS_COORD_MAX && fabs(s[k].y) < SS_COORD_MAX;
    return live;   // (a NaN fails every comparison)
}

// pre-pass: grid (ceil(F / 256), N); frame n of body min(n, Nv - 1)
__global__ __launch_bounds__(256) void soft_silhouette_faces_kernel(const float *vertices, const int32_t *faces, const double *poses, int Nv,
                                                                    int V, int F, int H, int W, double focal, double reach, float *proj,
                                                                    int32_t *box) {
    const int f = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (f >= F) return;
    const float *vt = vertices + (int64_t)(Nv == 1 ? 0 : n) * V * 3;
    const MrCamera C = mr_camera(poses, n);
    SsProj s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = ss_project(vt + (int64_t)faces[f * 3 + k] * 3, C, focal, H, W);
    const bool live = ss_live(s);
    float *P = proj + ((int64_t)n * F + f) * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P[2 * k] = live ? (float)s[k].x : NAN;
        P[2 * k + 1] = live ? (float)s[k].y : NAN;
    }
    int32_t b[4];
    ss_box(s, live, H, W, reach, b);
#pragma unroll
    for (int i = 0; i < 4; ++i) box[((int64_t)n * F + f) * 4 + i] = b[i];
}

struct SsArgs {
    const float *proj;         // [N,F,6]     workspace
    const int32_t *box;        // [N,F,4]     workspace: x0, x1, y0, y1 (inclusive)
    float *silhouette;         // [N,H,W]
    double *transmittance;     // [N,H,W]
    double sigma, cut2;
    int F, H, W, tiles_x, tiles_y;
};

template <bool CULL>
__global__ __launch_bounds__(SS_WAVES * 64) void soft_silhouette_fwd_kernel(SsArgs A) {
    __shared__ double part[SS_WAVES][1][WAVE];
    const int lane = lane_id(), wave = wave_index();
    const MrTile tl = mr_tile(blockIdx.x, A.tiles_x, A.tiles_y, A.H, A.W, lane);
    const Slice sl = wave_slice(A.F, SS_WAVES, wave);
    const float *proj = A.proj + (int64_t)tl.n * A.F * 6;
    double L = 0.0;
    auto pair = [&](const float *P) {
        if (P[0] != P[0]) return;   // not live (wave-uniform)
        const SsTest test = ss_test(tl.i, tl.j, P, A.cut2);
        if (test.contributes) L += ss_softplus(ss_z(test.inside, ss_value(tl.i, tl.j, P).s.d2, A.sigma));
    };

    if constexpr (CULL) {
        const int px0 = tl.x0(), px1 = tl.x1(A.W), py0 = tl.y0(), py1 = tl.y1(A.H);
        auto boxed = [&](int f, const float *b) {
            const int x0 = __float_as_int(b[0]), x1 = __float_as_int(b[1]), y0 = __float_as_int(b[2]), y1 = __float_as_int(b[3]);
            if (x0 <= px1 && x1 >= px0 && y0 <= py1 && y1 >= py0) {
                float P[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) P[k] = proj[f * 6 + k];
                pair(P);
            }
        };
        // (the walk indexes box and proj in 32 bits: the host refuses 9 F at 2^31 and above)
        const float *boxes = reinterpret_cast<const float *>(A.box + (int64_t)tl.n * A.F * 4);
        int f8 = sl.lo;
        for (; f8 + 8 <= sl.hi; f8 += 8) {
            float b[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) b[k] = boxes[f8 * 4 + k];
#pragma unroll
            for (int q = 0; q < 8; ++q) boxed(f8 + q, b + 4 * q);
        }
        walk4<4>(
            boxes, f8, sl.hi,
            [&](int f, const float *b) {
#pragma unroll
                for (int q = 0; q < 4; ++q) boxed(f + q, b + 4 * q);
            },
            [&](int f, const float *b) { boxed(f, b); });
    } else {
        walk4<6>(
            proj, sl.lo, sl.hi,
            [&](int, const float *P) {
#pragma unroll
                for (int q = 0; q < 4; ++q) pair(P + 6 * q);
            },
            [&](int, const float *P) { pair(P); });
    }

    put_partials(part[wave], lane, L);
    __syncthreads();
    if (wave != 0 || !tl.valid) return;
    double sum = part[0][0][lane];
#pragma unroll
    for (int w = 1; w < SS_WAVES; ++w) sum += part[w][0][lane];
    const int64_t r = ((int64_t)tl.n * A.H + tl.j) * A.W + tl.i;
    A.silhouette[r] = (float)(-expm1(-sum));
    A.transmittance[r] = exp(-sum);
}

// backward 1: grid (ceil(F / SS_BWD_WAVES), N), one wave per (frame, face) -> grads [N,F,3,3] float64
__global__ __launch_bounds__(SS_BWD_WAVES * 64) void soft_silhouette_bwd_faces_kernel(const float *vertices, const int32_t *faces,
                                                                                      const double *poses, int Nv, int V, int F, int H, int W,
                                                                                      double focal, double sigma, double cut2, const float *proj,
                                                                                      const int32_t *box, const float *d_silhouette,
                                                                                      const double *transmittance, double *grads) {
    const int lane = lane_id(), f = blockIdx.x * SS_BWD_WAVES + wave_index(), n = blockIdx.y;
    if (f >= F) return;
    const int32_t *b = box + ((int64_t)n * F + f) * 4;
    const int x0 = max(b[0], 0), x1 = min(b[1], W - 1), y0 = max(b[2], 0), y1 = min(b[3], H - 1);
    double *out = grads + ((int64_t)n * F + f) * 9;
    if (x0 > x1 || y0 > y1) {   // not live, or a box that misses the image (wave-uniform)
        if (lane < 9) out[lane] = 0.0;
        return;
    }
    float P[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) P[k] = proj[((int64_t)n * F + f) * 6 + k];
    const int bw = x1 - x0 + 1;
    const int count = bw * (y1 - y0 + 1);   // (at most H W, which the host keeps below 2^31)
    const float *dS = d_silhouette + (int64_t)n * H * W;
    const double *T = transmittance + (int64_t)n * H * W;
    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // d loss / d (x0, y0, x1, y1, x2, y2)
    for (int idx = lane; idx < count; idx += WAVE) {
        const int row = idx / bw, i = x0 + (idx - row * bw), j = y0 + row;
        const SsTest test = ss_test(i, j, P, cut2);
        if (!test.contributes) continue;
        const SsPair<double> p = ss_value(i, j, P);
        const int64_t r = (int64_t)j * W + i;
        // dS T sigmoid(z) dz/dd2, then d d2 / d a = -2 (1 - t) r and d d2 / d b = -2 t r for the nearest segment a -> b
        const double w = (double)dS[r] * T[r] * ss_sigmoid(ss_z(test.inside, p.s.d2, sigma)) * ((test.inside ? 2.0 : -2.0) / sigma);
        const double ta = 1.0 - p.s.t, tb = p.s.t, rx = p.s.rx, ry = p.s.ry;
        // corner k is the a of segment k and the b of segment k - 1
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double share = p.seg == k ? ta : p.seg == (k + 2) % 3 ? tb : 0.0;
            g[2 * k] -= w * share * rx;
            g[2 * k + 1] -= w * share * ry;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = wave_sum(g[k]);
    // through the projection: x = W/2 + focal c.x / depth, y = H/2 - focal c.y / depth, depth = -c.z, c = R^T (v - o)
    const float *vt = vertices + (int64_t)(Nv == 1 ? 0 : n) * V * 3;
    const MrCamera C = mr_camera(poses, n);
    double dv[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const SsProj s = ss_project(vt + (int64_t)faces[f * 3 + k] * 3, C, focal, H, W);
        const double a = focal / s.depth;
        const double gc[3] = {g[2 * k] * a, -g[2 * k + 1] * a, (g[2 * k] * s.c[0] - g[2 * k + 1] * s.c[1]) * a / s.depth};
#pragma unroll
        for (int i = 0; i < 3; ++i) dv[3 * k + i] = C.R[i][0] * gc[0] + C.R[i][1] * gc[1] + C.R[i][2] * gc[2];
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = dv[k];
    }
}

// backward 2: grid (ceil(V / 256), Nv), one thread per (body, vertex)
__global__ __launch_bounds__(256) void soft_silhouette_gather_kernel(const double *grads, const int32_t *vf_offsets, const int32_t *vf_faces,
                                                                     const int32_t *vf_corners, int N, int Nv, int V, int F,
                                                                     float *d_vertices) {
    const int v = blockIdx.x * 256 + threadIdx.x, body = blockIdx.y;
    if (v >= V) return;
    const int n0 = Nv == 1 ? 0 : body, n1 = Nv == 1 ? N : body + 1;
    const int k0 = vf_offsets[v], k1 = vf_offsets[v + 1];
    double s[3] = {0.0, 0.0, 0.0};
    for (int n = n0; n < n1; ++n)
        for (int k = k0; k < k1; ++k) {
            const double *g = grads + (((int64_t)n * F + vf_faces[k]) * 3 + vf_corners[k]) * 3;
            s[0] += g[0];
            s[1] += g[1];
            s[2] += g[2];
        }
    float *o = d_vertices + ((int64_t)body * V + v) * 3;
    o[0] = (float)s[0];
    o[1] = (float)s[1];
    o[2] = (float)s[2];
}

// workspace layout: proj [N,F,6] fp32, box [N,F,4] int32, grads [N,F,9] float64 (the backward's)
static int64_t ss_bytes(int64_t N, int64_t F) { return N * F * (10 * 4 + 9 * 8); }

struct SsWorkspace {
    float *proj;
    int32_t *box;
    double *grads;
};

// the checks both entries share, then the pre-pass; N == 0 returns SNERF_OK with `done` set
static int ss_prepare(const char *op, const double *poses, double focal, int64_t N, int H, int W, const float *vertices, int Nv, int V,
                      const int32_t *faces, int F, double sigma, double cutoff, int flags, bool pointers, void *workspace,
                      int64_t workspace_bytes, hipStream_t s, SsWorkspace &ws, bool &done) {
    done = true;
    if (N < 0) return fail(SNERF_E_BADARG, "%s: N must not be negative", op);
    if (H < 1 || W < 1) return fail(SNERF_E_BADARG, "%s: H and W must be at least 1", op);
    if (!(focal > 0.0) || !(focal < INFINITY)) return fail(SNERF_E_BADARG, "%s: focal must be positive and finite", op);
    if (!(sigma > 0.0) || !(sigma < INFINITY)) return fail(SNERF_E_BADARG, "%s: sigma must be positive and finite", op);
    if (!(cutoff >= 0.0) || !(cutoff < INFINITY)) return fail(SNERF_E_BADARG, "%s: cutoff must be finite and not negative", op);
    if (flags & ~SNERF_RENDER_NO_CULL) return fail(SNERF_E_BADARG, "%s: flags must be 0 or SNERF_RENDER_NO_CULL", op);
    if (int rc = check_walk_count(op, "V", V, 3)) return rc;
    if (int rc = check_walk_count(op, "F", F, 9)) return rc;
    if (N == 0) return SNERF_OK;
    if (Nv != 1 && Nv != N) return fail(SNERF_E_BADARG, "%s: Nv must be 1 or N", op);
    if (!poses || !vertices || !faces || !pointers) return fail(SNERF_E_BADARG, "%s: null pointer", op);
    if ((int64_t)mr_tiles(W) * mr_tiles(H) * N > 0x7fffffffLL || N > 65535 || N * (int64_t)F > INT64_MAX / 128 ||
        (int64_t)H * W > 0x7fffffffLL - WAVE)
        return fail(SNERF_E_BADARG, "%s: N times the tiles of a frame and H W must stay below 2^31 and N below 65536", op);
    if (!workspace || workspace_bytes < ss_bytes(N, F) || !aligned(workspace, 8))
        return fail(SNERF_E_BADARG, "%s: workspace missing, not 8-byte aligned or smaller than snerf_soft_silhouette_workspace_bytes()", op);
    ws.proj = (float *)workspace;
    ws.box = (int32_t *)(ws.proj + N * (int64_t)F * 6);
    ws.grads = (double *)(ws.box + N * (int64_t)F * 4);
    hipLaunchKernelGGL(soft_silhouette_faces_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)N), dim3(256), 0, s, vertices, faces, poses, Nv, V,
                       F, H, W, focal, sqrt(cutoff * sigma), ws.proj, ws.box);
    done = false;
    return SNERF_OK;
}

}  // namespace snerf

extern "C" int64_t snerf_soft_silhouette_workspace_bytes(int64_t N, int V, int F) {
    using namespace snerf;
    const char *op = "soft_silhouette_workspace_bytes";
    if (N < 0) return fail(SNERF_E_BADARG, "%s: N must not be negative", op), -1;
    if (check_walk_count(op, "V", V, 3) || check_walk_count(op, "F", F, 9)) return -1;
    if (N > 0 && ss_bytes(1, F) > INT64_MAX / N) return fail(SNERF_E_BADARG, "%s: N too large", op), -1;
    return ss_bytes(N, F);
}

extern "C" int snerf_soft_silhouette_fwd_f32(const double *poses, double focal, int64_t N, int H, int W, const float *vertices, int Nv, int V,
                                             const int32_t *faces, int F, double sigma, double cutoff, int flags, float *silhouette,
                                             double *transmittance, void *workspace, int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    const char *op = "soft_silhouette_fwd";
    hipStream_t s = (hipStream_t)stream;
    SsWorkspace ws;
    bool done;
    if (int rc = ss_prepare(op, poses, focal, N, H, W, vertices, Nv, V, faces, F, sigma, cutoff, flags, silhouette && transmittance, workspace,
                            workspace_bytes, s, ws, done))
        return rc;
    if (done) return SNERF_OK;
    const int tiles_x = mr_tiles(W), tiles_y = mr_tiles(H);
    const unsigned blocks = (unsigned)((int64_t)tiles_x * tiles_y * N);
    SsArgs A{ws.proj, ws.box, silhouette, transmittance, sigma, cutoff * sigma, F, H, W, tiles_x, tiles_y};
    if (flags & SNERF_RENDER_NO_CULL) hipLaunchKernelGGL(soft_silhouette_fwd_kernel<false>, dim3(blocks), dim3(SS_WAVES * 64), 0, s, A);
    else hipLaunchKernelGGL(soft_silhouette_fwd_kernel<true>, dim3(blocks), dim3(SS_WAVES * 64), 0, s, A);
    return check_launch(op);
}

extern "C" int snerf_soft_silhouette_bwd_f32(const double *poses, double focal, int64_t N, int H, int W, const float *vertices, int Nv, int V,
                                             const int32_t *faces, int F, double sigma, double cutoff, int flags, const float *d_silhouette,
                                             const double *transmittance, const int32_t *vf_offsets, const int32_t *vf_faces,
                                             const int32_t *vf_corners, float *d_vertices, void *workspace, int64_t workspace_bytes,
                                             snerf_stream_t stream) {
    using namespace snerf;
    const char *op = "soft_silhouette_bwd";
    hipStream_t s = (hipStream_t)stream;
    SsWorkspace ws;
    bool done;
    if (int rc = ss_prepare(op, poses, focal, N, H, W, vertices, Nv, V, faces, F, sigma, cutoff, flags,
                            d_silhouette && transmittance && vf_offsets && vf_faces && vf_corners && d_vertices, workspace, workspace_bytes, s, ws,
                            done))
        return rc;
    if (done) return SNERF_OK;
    hipLaunchKernelGGL(soft_silhouette_bwd_faces_kernel, dim3((unsigned)((F + SS_BWD_WAVES - 1) / SS_BWD_WAVES), (unsigned)N),
                       dim3(SS_BWD_WAVES * 64), 0, s, vertices, faces, poses, Nv, V, F, H, W, focal, sigma, cutoff * sigma, ws.proj, ws.box,
                       d_silhouette, transmittance, ws.grads);
    hipLaunchKernelGGL(soft_silhouette_gather_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)Nv), dim3(256), 0, s, ws.grads, vf_offsets,
                       vf_faces, vf_corners, (int)N, Nv, V, F, d_vertices);
    return check_launch(op);
}
