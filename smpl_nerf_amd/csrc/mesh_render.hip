// N textured, lit frames of a triangle mesh seen through pinhole cameras (create_dataset.py:106-129 asks pyrender for them one frame
// at a time, render.py:322-367): per pixel the first hit of its ray on the posed body - t, face and (u, v) exactly as
// snerf_ray_mesh_first_hit_f32 gives them for the rays of snerf_raygen_f64 - and a Lambert-shaded texture lookup at that point.
// This is NOT pyrender's metallic-roughness shader and nothing is pinned against pyrender or trimesh: the rule is the one written
// out in include/smplnerf.h (snerf_mesh_render_f32), operation by operation.
//
// Rays: made in the kernel, never stored.  Pixel (row j, column i) of frame n has the origin and direction of raygen.hip:46-58 -
// float32 i - W 0.5, float64 divide by focal, float64 rotation summed left to right, rounded once to fp32.
//
// Mapping: workgroup = one 8 x 8 pixel tile of one frame (grid = tiles x frames, clipped at the right and bottom edges), lane =
// pixel; its 8 waves split the faces (wave_slice), walk them (walk4; the culled walk takes eight boxes per wait while eight are
// left) and wave 0 merges the nearest hits in wave order: ray_mesh.hip's first-hit kernel, with the pair rule, the strict < and the merge of ray_mesh_pair.h.
//
// Pre-passes (per call, into the workspace): (1) per body and face the nine floats (a, e1, e2); per frame and face a conservative
// screen-space box in whole pixels - the three corners a, a + e1, a + e2 projected with the frame's camera in float64, widened by
// `margin` pixels per side (see mr_box below for why that is enough, and when a face gets the box "everything" instead);
// (2) per body and vertex the area-weighted normal: the sum over its incident faces, in CSR order, of the un-normalised e1 x e2.
//
// The cull: the walk reads a face's box (four int32 at a wave-uniform address) and tests it against the tile in integer scalar
// arithmetic; only a face whose box meets the tile has its nine floats loaded and the ~45 vector instructions of the pair rule
// run.  It is an optimisation only: every output equals the brute-force walk (SNERF_RENDER_NO_CULL) bit for bit.
//
// Shading runs in wave 0 after the merge, per hit pixel; products and sums kept apart (-ffp-contract=off).  No atomics, nothing of
// size pixels x faces, every element of every output written, two calls give the same bits.
#include "mesh_tile.h"
#include "ray_mesh_pair.h"

namespace snerf {

constexpr int MR_BOX_ALL_LO = INT32_MIN, MR_BOX_ALL_HI = INT32_MAX;

struct MrArgs {
    const double *poses;       // [N,4,4]
    const float *vertices;     // [Nv,V,3]
    const int32_t *faces;      // [F,3]
    const float *tri;          // [Nv,F,9]    workspace
    const int32_t *box;        // [N,F,4]     workspace: x0, x1, y0, y1 (inclusive), or null: no cull
    const float *normals;      // [Nv,V,3]    workspace
    const float *uv, *texture, *canon;
    float *image, *t, *bary, *depth, *warp;
    int32_t *face;
    double focal;
    int N, Nv, V, F, H, W, Ht, Wt, tiles_x, tiles_y;
    float ambient, intensity, bg[3];
};

// The screen-space box of the face T = (a, e1, e2) under camera C, in whole pixels, or "everything".
//
// In exact arithmetic a ray that hits a triangle in front of the camera passes through its projection, so pixel (i, j) lies in
// the bounding box of the three projected corners.  What the pair rule computes in fp32 is three numerators - un, vn and
// det - un - vn, which are D_j D_k times twice the signed area that the pixel spans with an edge of the projected triangle (D: the
// corners' depths) - and a hit needs all three to carry det's sign up to their rounding error E <= 32 eps |d| (|s| (|e1| + |e2|) +
// |e1| |e2|) (8 eps per numerator by the usual bound for a cross and a dot product, the rest to spare).  For a pixel m outside the box
// along x or y one of the three signed areas is at most -A2 m / (2 w) and one at least A2 / 3 (A2: twice the projected area, w: the
// box's larger side; barycentric coordinates sum to 1 and their x- or y-moment is -m), so no rounding can make a hit of it while
//     Dmin^2 A2 min(m / (2 w), 1/3) > E.                                   (*)
// A face that fails (*) - seen edge-on, or a sliver - gets "everything", as does one with a corner at or behind the camera plane or
// a non-finite projection.  m is one pixel; the box is widened by `margin` >= 1 pixel, the rest of which covers the fp32 rounding
// of the ray's direction (the host sets it), and then rounded outward to whole pixels.
__device__ __forceinline__ void mr_box(const float (&T)[9], const MrCamera &C, double focal, int H, int W, double margin, double dmax,
                                       int32_t (&box)[4]) {
    box[0] = box[2] = MR_BOX_ALL_LO;
    box[1] = box[3] = MR_BOX_ALL_HI;
    double px[3], py[3], x[3], y[3], dmin = INFINITY, s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double p[3], c[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = ((double)T[i] + (k ? (double)T[3 * k + i] : 0.0)) - (double)C.o[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = p[0] * C.R[0][i] + p[1] * C.R[1][i] + p[2] * C.R[2][i];   // R^T (p - o)
        const double depth = -c[2];
        if (!(depth > 0.0)) return;
        x[k] = c[0] / depth;
        y[k] = c[1] / depth;
        px[k] = W * 0.5 + focal * x[k];
        py[k] = H * 0.5 - focal * y[k];
        dmin = fmin(dmin, depth);
        s = fmax(s, sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
    }
    const double x0 = fmin(px[0], fmin(px[1], px[2])), x1 = fmax(px[0], fmax(px[1], px[2]));
    const double y0 = fmin(py[0], fmin(py[1], py[2])), y1 = fmax(py[0], fmax(py[1], py[2]));
    if (!(x0 > -1e9 && x1 < 1e9 && y0 > -1e9 && y1 < 1e9)) return;   // (also refuses a NaN)
    const double e1 = sqrt((double)T[3] * T[3] + (double)T[4] * T[4] + (double)T[5] * T[5]);
    const double e2 = sqrt((double)T[6] * T[6] + (double)T[7] * T[7] + (double)T[8] * T[8]);
    const double a2 = fabs((x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0]));
    const double w = fmax(x1 - x0, y1 - y0) / focal, m = 1.0 / focal;
    const double E = 32.0 * 5.9604644775390625e-08 * dmax * (s * (e1 + e2) + e1 * e2);
    if (!(dmin * dmin * a2 * fmin(m / (2.0 * w), 1.0 / 3.0) > E)) return;   // (*)
    box[0] = (int32_t)floor(x0 - margin);
    box[1] = (int32_t)ceil(x1 + margin);
    box[2] = (int32_t)floor(y0 - margin);
    box[3] = (int32_t)ceil(y1 + margin);
}

// pre-pass 1: grid (ceil(F / 256), N); frame n of body min(n, Nv - 1)
__global__ __launch_bounds__(256) void mesh_render_faces_kernel(const float *vertices, const int32_t *faces, const double *poses, int Nv, int V,
                                                                int F, int H, int W, double focal, double margin, double dmax, float *tri,
                                                                int32_t *box) {
    const int f = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (f >= F) return;
    const int body = Nv == 1 ? 0 : n;
    float T[9];
    rm_face(vertices + (int64_t)body * V * 3, faces, f, T);
    if (n < Nv) {
#pragma unroll
        for (int i = 0; i < 9; ++i) tri[((int64_t)body * F + f) * 9 + i] = T[i];
    }
    if (!box) return;
    int32_t b[4];
    mr_box(T, mr_camera(poses, n), focal, H, W, margin, dmax, b);
#pragma unroll
    for (int i = 0; i < 4; ++i) box[((int64_t)n * F + f) * 4 + i] = b[i];
}

// pre-pass 2: grid (ceil(V / 256), Nv); one thread per vertex, its incident faces in CSR order
__global__ __launch_bounds__(256) void mesh_render_normals_kernel(const float *vertices, const int32_t *faces, const int32_t *vf_offsets,
                                                                  const int32_t *vf_faces, int V, float *normals) {
    const int v = blockIdx.x * 256 + threadIdx.x, body = blockIdx.y;
    if (v >= V) return;
    const float *vt = vertices + (int64_t)body * V * 3;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = vf_offsets[v]; k < vf_offsets[v + 1]; ++k) {
        float T[9];
        rm_face(vt, faces, vf_faces[k], T);
        nx = nx + (T[4] * T[8] - T[5] * T[7]);   // e1 x e2
        ny = ny + (T[5] * T[6] - T[3] * T[8]);
        nz = nz + (T[3] * T[7] - T[4] * T[6]);
    }
    float *o = normals + ((int64_t)body * V + v) * 3;
    o[0] = nx;
    o[1] = ny;
    o[2] = nz;
}

// w0 x_a + u x_b + v x_c as ((w0 x_a + u x_b) + v x_c)
__device__ __forceinline__ float mr_mix(float w0, float u, float v, float xa, float xb, float xc) { return (w0 * xa + u * xb) + v * xc; }

// clamp-to-edge texel index of the (already floored) coordinate x0, plus `step`
__device__ __forceinline__ int mr_texel(float x0, int step, int n) {
    const int i = (int)fminf(fmaxf(x0, -1.f), (float)n) + step;   // (fmaxf drops a NaN)
    return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
}

template <bool CULL>
__global__ __launch_bounds__(RM_WAVES * 64) void mesh_render_kernel(MrArgs A) {
    __shared__ float part[RM_WAVES][4][WAVE];   // t, face (its bits), u, v of each wave's nearest hit
    const int lane = lane_id(), wave = wave_index();
    const MrTile tl = mr_tile(blockIdx.x, A.tiles_x, A.tiles_y, A.H, A.W, lane);
    const int n = tl.n, i = tl.i, j = tl.j;
    const bool valid = tl.valid;
    const int body = A.Nv == 1 ? 0 : n;

    // the ray of pixel (j, i): raygen.hip:46-58, operation for operation
    const double *M = A.poses + (int64_t)n * 16;
    const double cx = __ddiv_rn((double)__fsub_rn((float)i, (float)(A.W * 0.5)), A.focal);
    const double cy = __ddiv_rn((double)(-__fsub_rn((float)j, (float)(A.H * 0.5))), A.focal);
    const double cz = -1.0;
    float d[3], o[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        d[r] = (float)__dadd_rn(__dadd_rn(__dmul_rn(cx, M[r * 4 + 0]), __dmul_rn(cy, M[r * 4 + 1])), __dmul_rn(cz, M[r * 4 + 2]));
        o[r] = (float)M[r * 4 + 3];
    }
    const RmRay y{o[0], o[1], o[2], d[0], d[1], d[2]};

    const Slice sl = wave_slice(A.F, RM_WAVES, wave);
    const float *tri = A.tri + (int64_t)body * A.F * 9;
    RmFirst best;
    auto pair = [&](int f, const float *T) { rm_pair(y, T, [&](float t, float u, float v) { best.take(t, f, u, v); }); };

    if constexpr (CULL) {
        // the tile in pixels, clipped; a box meets it when the intervals overlap on both axes (all wave-uniform integers)
        const int px0 = tl.x0(), px1 = tl.x1(A.W), py0 = tl.y0(), py1 = tl.y1(A.H);
        auto boxed = [&](int f, const float *b) {
            const int x0 = __float_as_int(b[0]), x1 = __float_as_int(b[1]), y0 = __float_as_int(b[2]), y1 = __float_as_int(b[3]);
            if (x0 <= px1 && x1 >= px0 && y0 <= py1 && y1 >= py0) {
                float T[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) T[k] = tri[f * 9 + k];
                pair(f, T);
            }
        };
        // (the walk indexes box and tri in 32 bits: the host refuses 9 F at 2^31 and above)
        // Eight boxes per wait while eight are left - the box walk waits on the scalar cache, not on arithmetic - then walk4's fours
        // and ones.
        const float *boxes = reinterpret_cast<const float *>(A.box + (int64_t)n * A.F * 4);
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
        walk4<9>(
            tri, sl.lo, sl.hi,
            [&](int f, const float *T) {
#pragma unroll
                for (int q = 0; q < 4; ++q) pair(f + q, T + 9 * q);
            },
            [&](int f, const float *T) { pair(f, T); });
    }

    put_partials(part[wave], lane, best.t, __int_as_float(best.face), best.u, best.v);
    __syncthreads();
    if (wave != 0 || !valid) return;
    rm_merge_first(best, part, lane);
    const int64_t r = ((int64_t)n * A.H + j) * A.W + i;
    A.t[r] = best.t;
    A.face[r] = best.face;
    A.bary[r * 2 + 0] = best.u;
    A.bary[r * 2 + 1] = best.v;
    if (A.canon) {
        float depth, warp[3];
        rm_canon(y, best, A.faces, A.canon, depth, warp);
        A.depth[r] = depth;
        A.warp[r * 3 + 0] = warp[0];
        A.warp[r * 3 + 1] = warp[1];
        A.warp[r * 3 + 2] = warp[2];
    }

    float rgb[3] = {A.bg[0], A.bg[1], A.bg[2]};
    if (best.face >= 0) {
        const int ia = A.faces[best.face * 3 + 0], ib = A.faces[best.face * 3 + 1], ic = A.faces[best.face * 3 + 2];
        const float u = best.u, v = best.v, w0 = (1.f - u) - v;
        // the normal: interpolated from the un-normalised vertex sums, then normalised; 0 where the sum is 0
        const float *nb = A.normals + (int64_t)body * A.V * 3;
        const float mx = mr_mix(w0, u, v, nb[ia * 3 + 0], nb[ib * 3 + 0], nb[ic * 3 + 0]);
        const float my = mr_mix(w0, u, v, nb[ia * 3 + 1], nb[ib * 3 + 1], nb[ic * 3 + 1]);
        const float mz = mr_mix(w0, u, v, nb[ia * 3 + 2], nb[ib * 3 + 2], nb[ic * 3 + 2]);
        const float len = sqrtf(dist2(mx, my, mz));
        const bool flat = len == 0.f;
        const float nx = flat ? 0.f : mx / len, ny = flat ? 0.f : my / len, nz = flat ? 0.f : mz / len;
        // the light: the camera's +z, towards the viewer
        const float lambert = fmaxf(0.f, dot3(nx, ny, nz, (float)M[0 * 4 + 2], (float)M[1 * 4 + 2], (float)M[2 * 4 + 2]));
        const float shade = fminf(1.f, A.ambient + A.intensity * lambert);
        // the texel: bilinear, clamp to edge, rows first
        const float U = mr_mix(w0, u, v, A.uv[ia * 2 + 0], A.uv[ib * 2 + 0], A.uv[ic * 2 + 0]);
        const float Vt = mr_mix(w0, u, v, A.uv[ia * 2 + 1], A.uv[ib * 2 + 1], A.uv[ic * 2 + 1]);
        const float x = U * (float)A.Wt - 0.5f, yy = (1.f - Vt) * (float)A.Ht - 0.5f;
        const float xf = floorf(x), yf = floorf(yy);
        const float fx = x - xf, fy = yy - yf;
        const int c0 = mr_texel(xf, 0, A.Wt), c1 = mr_texel(xf, 1, A.Wt), r0 = mr_texel(yf, 0, A.Ht), r1 = mr_texel(yf, 1, A.Ht);
        const float *t00 = A.texture + ((int64_t)r0 * A.Wt + c0) * 3, *t01 = A.texture + ((int64_t)r0 * A.Wt + c1) * 3,
                    *t10 = A.texture + ((int64_t)r1 * A.Wt + c0) * 3, *t11 = A.texture + ((int64_t)r1 * A.Wt + c1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = t00[c] * (1.f - fx) + t01[c] * fx, bottom = t10[c] * (1.f - fx) + t11[c] * fx;
            rgb[c] = (top * (1.f - fy) + bottom * fy) * shade;
        }
    }
    A.image[r * 3 + 0] = rgb[0];
    A.image[r * 3 + 1] = rgb[1];
    A.image[r * 3 + 2] = rgb[2];
}

// workspace layout: tri [N,F,9] fp32, box [N,F,4] int32, normals [N,V,3] fp32 (a shared body uses the first of N slots)
static int64_t mr_bytes(int64_t N, int64_t V, int64_t F) { return N * (F * 13 + V * 3) * 4; }

}  // namespace snerf

extern "C" int64_t snerf_mesh_render_workspace_bytes(int64_t N, int V, int F) {
    using namespace snerf;
    if (N < 0) return fail(SNERF_E_BADARG, "mesh_render_workspace_bytes: N must not be negative");
    if (check_walk_count("mesh_render_workspace_bytes", "V", V, 3) || check_walk_count("mesh_render_workspace_bytes", "F", F, 9)) return -1;
    if (N > 0 && mr_bytes(1, V, F) > INT64_MAX / N) return fail(SNERF_E_BADARG, "mesh_render_workspace_bytes: N too large");
    return mr_bytes(N, V, F);
}

extern "C" int snerf_mesh_render_f32(const double *poses, double focal, int64_t N, int H, int W, const float *vertices, int Nv, int V,
                                     const int32_t *faces, int F, const int32_t *vf_offsets, const int32_t *vf_faces, const float *uv,
                                     const float *texture, int Ht, int Wt, const snerf_mesh_render_args *args, const float *canon,
                                     float *image, float *t, int32_t *face, float *bary, float *depth, float *warp, void *workspace,
                                     int64_t workspace_bytes, snerf_stream_t stream) {
    using namespace snerf;
    const char *op = "mesh_render";
    if (N < 0) return fail(SNERF_E_BADARG, "%s: N must not be negative", op);
    if (H < 1 || W < 1 || Ht < 1 || Wt < 1) return fail(SNERF_E_BADARG, "%s: H, W, Ht and Wt must be at least 1", op);
    if (!(focal > 0.0) || !(focal < INFINITY)) return fail(SNERF_E_BADARG, "%s: focal must be positive and finite", op);
    if (int rc = check_walk_count(op, "V", V, 3)) return rc;
    if (int rc = check_walk_count(op, "F", F, 9)) return rc;
    if (N == 0) return SNERF_OK;
    if (Nv != 1 && Nv != N) return fail(SNERF_E_BADARG, "%s: Nv must be 1 or N", op);
    if (!poses || !vertices || !faces || !vf_offsets || !vf_faces || !uv || !texture || !args || !image || !t || !face || !bary)
        return fail(SNERF_E_BADARG, "%s: null pointer (poses, vertices, faces, vf_offsets, vf_faces, uv, texture, args, image, t, face, bary)", op);
    if (!((canon && warp && depth) || (!canon && !warp && !depth)))
        return fail(SNERF_E_BADARG, "%s: canon, warp and depth must be all null or all non-null", op);
    const int tiles_x = mr_tiles(W), tiles_y = mr_tiles(H);
    const int64_t blocks = (int64_t)tiles_x * tiles_y * N;
    if (blocks > 0x7fffffffLL || N > 65535 || (int64_t)Ht * Wt * 3 > 0x7fffffffLL || (int64_t)N * F * 13 > INT64_MAX / 8)
        return fail(SNERF_E_BADARG, "%s: N times the tiles of a frame must stay below 2^31, N below 65536 and 3 Ht Wt below 2^31", op);
    if (!workspace || workspace_bytes < mr_bytes(N, V, F))
        return fail(SNERF_E_BADARG, "%s: workspace missing or smaller than snerf_mesh_render_workspace_bytes()", op);
    hipStream_t s = (hipStream_t)stream;
    const bool cull = !(args->flags & SNERF_RENDER_NO_CULL);
    float *tri = (float *)workspace;
    int32_t *box = (int32_t *)(tri + N * (int64_t)F * 9);
    float *normals = (float *)(box + N * (int64_t)F * 4);
    // |d| of the widest ray, and the margin: one pixel plus what the fp32 rounding of a direction can move its pixel by
    const double hx = 0.5 * W / focal, hy = 0.5 * H / focal, dmax = sqrt(1.0 + hx * hx + hy * hy);
    const double margin = 1.0 + focal * 8.0 * 5.9604644775390625e-08 * dmax * dmax;
    hipLaunchKernelGGL(mesh_render_faces_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)N), dim3(256), 0, s, vertices, faces, poses, Nv, V, F,
                       H, W, focal, margin, dmax, tri, cull ? box : nullptr);
    hipLaunchKernelGGL(mesh_render_normals_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)Nv), dim3(256), 0, s, vertices, faces, vf_offsets,
                       vf_faces, V, normals);
    MrArgs A{poses, vertices, faces, tri, cull ? box : nullptr, normals, uv, texture, canon, image, t, bary, depth, warp, face, focal,
             (int)N, Nv, V, F, H, W, Ht, Wt, tiles_x, tiles_y, args->ambient, args->intensity,
             {args->background[0], args->background[1], args->background[2]}};
    if (cull) hipLaunchKernelGGL(mesh_render_kernel<true>, dim3((unsigned)blocks), dim3(RM_WAVES * 64), 0, s, A);
    else hipLaunchKernelGGL(mesh_render_kernel<false>, dim3((unsigned)blocks), dim3(RM_WAVES * 64), 0, s, A);
    return check_launch(op);
}
