// SMPL linear blend skinning (Loper et al. 2015, smplx's conventions; include/smplnerf.h has the ten steps), forward and backward,
// fp32 in and out.  B poses, V vertices, J joints, NB shape coefficients, P = 9 (J - 1) pose features, K = NB + P, E = 12 J + K.
//
// Rig stage (sizes B J; one thread per pose, the chain is sequential anyway; float64 arithmetic inside, rounded once on the way out):
//   lbs_rig_fwd_kernel   Rodrigues, pose feature, rest joints, chain -> rig [B, E] = [A (J x 3 x 4, row-major) | betas | pose feature]
//                        (the coefficient vector of the blend is stored with the transforms: the vertex kernels read one record) and
//                        joints [B, J, 3].
//   lbs_rig_bwd_kernel   recomputes the chain, then walks it in reverse: d rig [B, E] and d joints -> d body_pose, d global_orient and
//                        d betas rows; the Rodrigues formula is differentiated as written, 1e-8 included.
// Vertex stage (everything with a V in it); the blend is the [B, K] x [K, 3V] contraction, on the vector pipe (v_fma_f32):
//   lbs_vertex_fwd_kernel  workgroup = 128 vertices x 16 poses, lane = vertex.  A lane keeps 3 x 16 accumulators (x, y, z of its vertex
//                        in 16 poses, from zero; the template is added after the sum), walks k, reads its three blend values (coalesced: 768 bytes per wave and k) and the 16
//                        coefficients from LDS at a wave-uniform address (broadcast): one row of the blend matrix serves 16 poses,
//                        consecutive workgroups share the vertex tile (L2).  Then T_v = sum_j W[v,j] A_j over the joints that any
//                        vertex of the wave has a weight on (a wave-uniform mask; skipping a joint whose weights are all zero
//                        leaves out additions of zero), the affine map, and the only [B,V] traffic: vertices written once.
//   lbs_vertex_bwd_kernel  workgroup = 8 poses x a slice of 256-vertex tiles.  Per tile: (1) lane = vertex: v_posed and T_v again,
//                        d_v_posed = T.R^T d_v; d_v and [v_posed] go to LDS; (2) lane = (joint, row, column) of A: sum over the tile's
//                        vertices of W[v,j] d_v[row] [v_posed; 1][column]; (3) d_v_posed replaces d_v in LDS, lane = k: sum over the
//                        tile's 768 columns of blend[k, column] d_v_posed[column].  (2) and (3) accumulate in registers over the
//                        tiles of the slice; the slice's partial goes to the workspace.
//   lbs_reduce_kernel    the slices summed in slice order.  No atomics anywhere; two calls give the same bits.
// The build keeps products and sums apart (-ffp-contract=off): every multiply-add below that is meant as one is written fmaf.
#include "snerf_common.h"

namespace snerf {

constexpr int LBS_MAX_J = 32, LBS_MAX_K = 512;
constexpr int LBS_FPT = 16, LBS_FVT = 128;   // forward tile: poses x vertices (= threads)
constexpr int LBS_BPT = 8, LBS_BVT = 256;    // backward tile: poses x vertices (= threads)
constexpr int LBS_KC = 64;                   // coefficients staged in LDS at a time

struct LbsModel {
    const float *v_template, *blend, *J_template, *J_dirs, *weights;
    int V, J, NB, K, E;
    int parents[LBS_MAX_J];
};

// ---------------------------------------------------------------------------------------------------- rig stage
// The rig stage computes in float64 and rounds what it hands over once (it is B J work, a thousandth of the vertex stage's): A.t = G.t - G.R J
// and its counterparts in the backward cancel, and in fp32 that rounding would be the largest error of the whole model.
using real = double;
// R = I + sin(angle) K + (1 - cos(angle)) K^2,  angle = |r + 1e-8|,  K = skew(r / angle); K^2 in closed form (the same products)
struct LbsRot {
    real angle, dx, dy, dz, s, c;
};
__device__ __forceinline__ LbsRot lbs_rodrigues(real rx, real ry, real rz, real *R) {
    LbsRot q;
    const real ax = rx + 1e-8, ay = ry + 1e-8, az = rz + 1e-8;
    q.angle = sqrt(ax * ax + ay * ay + az * az);
    q.dx = rx / q.angle;
    q.dy = ry / q.angle;
    q.dz = rz / q.angle;
    sincos(q.angle, &q.s, &q.c);
    const real t = 1.0 - q.c, dx = q.dx, dy = q.dy, dz = q.dz;
    R[0] = 1.0 + t * -(dy * dy + dz * dz);
    R[1] = q.s * -dz + t * (dx * dy);
    R[2] = q.s * dy + t * (dx * dz);
    R[3] = q.s * dz + t * (dx * dy);
    R[4] = 1.0 + t * -(dx * dx + dz * dz);
    R[5] = q.s * -dx + t * (dy * dz);
    R[6] = q.s * -dy + t * (dx * dz);
    R[7] = q.s * dx + t * (dy * dz);
    R[8] = 1.0 + t * -(dx * dx + dy * dy);
    return q;
}

// d loss / d r from d loss / d R, through the formula above
__device__ __forceinline__ void lbs_rodrigues_bwd(real rx, real ry, real rz, const real *dR, real *dr) {
    real Rtmp[9];
    const LbsRot q = lbs_rodrigues(rx, ry, rz, Rtmp);
    const real dx = q.dx, dy = q.dy, dz = q.dz, t = 1.0 - q.c;
    const real Km[9] = {0.0, -dz, dy, dz, 0.0, -dx, -dy, dx, 0.0};
    const real K2[9] = {-(dy * dy + dz * dz), dx * dy, dx * dz, dx * dy, -(dx * dx + dz * dz), dy * dz, dx * dz, dy * dz, -(dx * dx + dy * dy)};
    real dsin = 0.0, dq = 0.0, dK[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        dsin += dR[i] * Km[i];
        dq += dR[i] * K2[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            real u = 0.0;   // (dR K^T + K^T dR)[i][j]
#pragma unroll
            for (int m = 0; m < 3; ++m) u += dR[i * 3 + m] * Km[j * 3 + m] + Km[m * 3 + i] * dR[m * 3 + j];
            dK[i * 3 + j] = q.s * dR[i * 3 + j] + t * u;
        }
    const real dd[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    const real r[3] = {rx, ry, rz};
    real dangle = q.c * dsin + q.s * dq;
    dangle -= (dd[0] * r[0] + dd[1] * r[1] + dd[2] * r[2]) / (q.angle * q.angle);
#pragma unroll
    for (int i = 0; i < 3; ++i) dr[i] = dd[i] / q.angle + dangle * ((r[i] + 1e-8) / q.angle);
}

struct LbsRigArgs {
    LbsModel M;
    const float *betas, *body_pose, *global_orient;
    int64_t B;
    int betas_rows;
    // forward
    float *rig, *joints;
    // backward
    const float *d_rig, *d_joints;
    float *d_body_pose, *d_global_orient, *d_betas_rows;
};

// the pose's chain: R [J][9], G [J][12] (3 x 4 row-major), rest joints Jr [J][3]
__device__ void lbs_chain(const LbsRigArgs &a, int64_t b, real (*R)[9], real (*G)[12], real (*Jr)[3]) {
    const LbsModel &M = a.M;
    const float *bet = a.betas + (a.betas_rows == 1 ? 0 : b * M.NB);
    for (int j = 0; j < M.J; ++j) {
        for (int c = 0; c < 3; ++c) {
            real s = M.J_template[j * 3 + c];
            for (int n = 0; n < M.NB; ++n) s = fma(M.J_dirs[(j * 3 + c) * M.NB + n], bet[n], s);
            Jr[j][c] = s;
        }
        real r[3] = {0.0, 0.0, 0.0};
        if (j > 0)
            for (int c = 0; c < 3; ++c) r[c] = a.body_pose[b * 3 * (M.J - 1) + 3 * (j - 1) + c];
        else if (a.global_orient)
            for (int c = 0; c < 3; ++c) r[c] = a.global_orient[b * 3 + c];
        lbs_rodrigues(r[0], r[1], r[2], R[j]);
        if (j == 0) {
            for (int i = 0; i < 3; ++i) {
                for (int c = 0; c < 3; ++c) G[0][i * 4 + c] = R[0][i * 3 + c];
                G[0][i * 4 + 3] = Jr[0][i];
            }
        } else {
            const int p = M.parents[j];
            const real rel[3] = {Jr[j][0] - Jr[p][0], Jr[j][1] - Jr[p][1], Jr[j][2] - Jr[p][2]};
            for (int i = 0; i < 3; ++i) {
                for (int c = 0; c < 3; ++c) {
                    real s = 0.0;
                    for (int m = 0; m < 3; ++m) s = fma(G[p][i * 4 + m], R[j][m * 3 + c], s);
                    G[j][i * 4 + c] = s;
                }
                real s = G[p][i * 4 + 3];
                for (int m = 0; m < 3; ++m) s = fma(G[p][i * 4 + m], rel[m], s);
                G[j][i * 4 + 3] = s;
            }
        }
    }
}

__global__ __launch_bounds__(64) void lbs_rig_fwd_kernel(LbsRigArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const LbsModel &M = a.M;
    real R[LBS_MAX_J][9], G[LBS_MAX_J][12], Jr[LBS_MAX_J][3];
    lbs_chain(a, b, R, G, Jr);
    float *out = a.rig + b * M.E;
    const float *bet = a.betas + (a.betas_rows == 1 ? 0 : b * M.NB);
    for (int n = 0; n < M.NB; ++n) out[12 * M.J + n] = bet[n];
    for (int j = 0; j < M.J; ++j) {
        for (int i = 0; i < 3; ++i) {
            real t = G[j][i * 4 + 3];
            for (int c = 0; c < 3; ++c) {
                out[j * 12 + i * 4 + c] = G[j][i * 4 + c];
                t = fma(-G[j][i * 4 + c], Jr[j][c], t);
            }
            out[j * 12 + i * 4 + 3] = t;
            if (a.joints) a.joints[(b * M.J + j) * 3 + i] = G[j][i * 4 + 3];
        }
        if (j > 0)
            for (int i = 0; i < 9; ++i) out[12 * M.J + M.NB + 9 * (j - 1) + i] = R[j][i] - (i % 4 == 0 ? 1.0 : 0.0);
    }
}

__global__ __launch_bounds__(64) void lbs_rig_bwd_kernel(LbsRigArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const LbsModel &M = a.M;
    real R[LBS_MAX_J][9], G[LBS_MAX_J][12], Jr[LBS_MAX_J][3];
    real dGR[LBS_MAX_J][9], dGt[LBS_MAX_J][3], dJr[LBS_MAX_J][3];
    lbs_chain(a, b, R, G, Jr);
    const float *dA = a.d_rig ? a.d_rig + b * M.E : nullptr;
    for (int j = 0; j < M.J; ++j)
        for (int i = 0; i < 3; ++i) dJr[j][i] = 0.0;
    for (int j = 0; j < M.J; ++j) {
        for (int i = 0; i < 3; ++i) {
            const real dAt = dA ? dA[j * 12 + i * 4 + 3] : 0.0;   // A.t = G.t - G.R Jr
            for (int c = 0; c < 3; ++c) {
                dGR[j][i * 3 + c] = (dA ? dA[j * 12 + i * 4 + c] : 0.0) - dAt * Jr[j][c];
                dJr[j][c] -= G[j][i * 4 + c] * dAt;
            }
            dGt[j][i] = dAt + (a.d_joints ? a.d_joints[(b * M.J + j) * 3 + i] : 0.0);
        }
    }
    for (int j = M.J - 1; j >= 0; --j) {
        real dR[9], dr[3], r[3] = {0.0, 0.0, 0.0};
        if (j > 0) {
            const int p = M.parents[j];
            const real rel[3] = {Jr[j][0] - Jr[p][0], Jr[j][1] - Jr[p][1], Jr[j][2] - Jr[p][2]};
            const float *dpf = dA ? dA + 12 * M.J + M.NB + 9 * (j - 1) : nullptr;
            for (int i = 0; i < 3; ++i)
                for (int c = 0; c < 3; ++c) {
                    real s = dpf ? dpf[i * 3 + c] : 0.0;   // G_j.R = G_p.R R_j
                    for (int m = 0; m < 3; ++m) s = fma(G[p][m * 4 + i], dGR[j][m * 3 + c], s);
                    dR[i * 3 + c] = s;
                }
            for (int i = 0; i < 3; ++i)
                for (int c = 0; c < 3; ++c) {
                    real s = dGR[p][i * 3 + c];
                    for (int m = 0; m < 3; ++m) s = fma(dGR[j][i * 3 + m], R[j][c * 3 + m], s);
                    dGR[p][i * 3 + c] = fma(dGt[j][i], rel[c], s);   // G_j.t = G_p.R rel + G_p.t
                }
            for (int c = 0; c < 3; ++c) {
                real s = 0.0;
                for (int m = 0; m < 3; ++m) s = fma(G[p][m * 4 + c], dGt[j][m], s);
                dJr[j][c] += s;
                dJr[p][c] -= s;
                dGt[p][c] += dGt[j][c];
            }
            for (int c = 0; c < 3; ++c) r[c] = a.body_pose[b * 3 * (M.J - 1) + 3 * (j - 1) + c];
        } else {
            for (int i = 0; i < 9; ++i) dR[i] = dGR[0][i];
            for (int c = 0; c < 3; ++c) dJr[0][c] += dGt[0][c];
            if (a.global_orient)
                for (int c = 0; c < 3; ++c) r[c] = a.global_orient[b * 3 + c];
        }
        float *out = j > 0 ? (a.d_body_pose ? a.d_body_pose + b * 3 * (M.J - 1) + 3 * (j - 1) : nullptr)
                           : (a.d_global_orient ? a.d_global_orient + b * 3 : nullptr);
        if (out) {
            lbs_rodrigues_bwd(r[0], r[1], r[2], dR, dr);
            for (int c = 0; c < 3; ++c) out[c] = dr[c];
        }
    }
    if (a.d_betas_rows)
        for (int n = 0; n < M.NB; ++n) {
            real s = dA ? dA[12 * M.J + n] : 0.0;
            for (int j = 0; j < M.J; ++j)
                for (int c = 0; c < 3; ++c) s = fma(dJr[j][c], M.J_dirs[(j * 3 + c) * M.NB + n], s);
            a.d_betas_rows[b * M.NB + n] = s;
        }
}

// out[n] = sum_b rows[b, n]: thread t of block n sums b = t, t + 256, ... in order, thread 0 the 256 partials in order
__global__ __launch_bounds__(256) void lbs_sum_rows_kernel(const float *rows, int64_t B, int NB, float *out) {
    __shared__ float part[256];
    const int n = blockIdx.x;
    float s = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += 256) s += rows[b * NB + n];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 256; ++i) t += part[i];
        out[n] = t;
    }
}

// ---------------------------------------------------------------------------------------------------- vertex stage
struct LbsVertexArgs {
    LbsModel M;
    const float *rig;
    int64_t B;
    int pose_tiles, vertex_tiles;
    // forward
    float *vertices;
    // backward
    const float *d_vertices;
    float *partial;   // [slices][B][E]
    int slices;
};

// acc[c][p] = v_template[v][c] + (sum_k coef[b0 + p][k] blend[k][3 v + c]) for the PT poses from b0 (poses past B count as zero
// coefficients), k ascending.  `coef_s` [LBS_KC][PT] is staged by the whole workgroup: every thread of it must call this.
template <int PT, int THREADS>
__device__ __forceinline__ void lbs_blend(const LbsModel &M, const float *rig, int64_t B, int64_t b0, int vc, float *coef_s, float (*acc)[PT]) {
    const int64_t N3 = (int64_t)M.V * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < PT; ++p) acc[c][p] = 0.f;
    for (int k0 = 0; k0 < M.K; k0 += LBS_KC) {
        __syncthreads();
        for (int i = threadIdx.x; i < LBS_KC * PT; i += THREADS) {
            const int kk = i / PT, p = i % PT;
            coef_s[i] = (b0 + p < B && k0 + kk < M.K) ? rig[(b0 + p) * M.E + 12 * M.J + k0 + kk] : 0.f;
        }
        __syncthreads();
        const int kend = M.K - k0 < LBS_KC ? M.K - k0 : LBS_KC;
        const float *row = M.blend + (int64_t)k0 * N3 + (int64_t)vc * 3;
#pragma unroll 4
        for (int kk = 0; kk < kend; ++kk, row += N3) {
            const float x = row[0], y = row[1], z = row[2];
            const float4 *cf = reinterpret_cast<const float4 *>(coef_s + kk * PT);
#pragma unroll
            for (int p4 = 0; p4 < PT / 4; ++p4) {
                const float4 c4 = cf[p4];
                const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[0][p4 * 4 + q] = fmaf(cc[q], x, acc[0][p4 * 4 + q]);
                    acc[1][p4 * 4 + q] = fmaf(cc[q], y, acc[1][p4 * 4 + q]);
                    acc[2][p4 * 4 + q] = fmaf(cc[q], z, acc[2][p4 * 4 + q]);
                }
            }
        }
    }
    // the template last: the 217 roundings of the sum happen at the size of the blend shapes (centimetres), not of the body
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = M.v_template[vc * 3 + c];
#pragma unroll
        for (int p = 0; p < PT; ++p) acc[c][p] = t + acc[c][p];
    }
}

// the A records of PT poses from b0 into LDS (zeros past B)
template <int PT, int THREADS>
__device__ __forceinline__ void lbs_stage_A(const LbsModel &M, const float *rig, int64_t B, int64_t b0, float *A_s) {
    const int n = 12 * M.J;
    for (int i = threadIdx.x; i < PT * n; i += THREADS) {
        const int p = i / n, e = i - p * n;
        A_s[i] = b0 + p < B ? rig[(b0 + p) * M.E + e] : 0.f;
    }
}

// T[q][0..12) += w A_s[q][j] for NQ poses
template <int NQ>
__device__ __forceinline__ void lbs_skin_joint(float w, const float *A_j, int pose_stride, float (*T)[12]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const float4 *Ap = reinterpret_cast<const float4 *>(A_j + q * pose_stride);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float4 r = Ap[i];
            T[q][i * 4 + 0] = fmaf(w, r.x, T[q][i * 4 + 0]);
            T[q][i * 4 + 1] = fmaf(w, r.y, T[q][i * 4 + 1]);
            T[q][i * 4 + 2] = fmaf(w, r.z, T[q][i * 4 + 2]);
            T[q][i * 4 + 3] = fmaf(w, r.w, T[q][i * 4 + 3]);
        }
    }
}

// dynamic LDS: A_s [PT][12 J] | coef_s [KC][PT] | W_s [FVT][J | 1]
__global__ __launch_bounds__(LBS_FVT) void lbs_vertex_fwd_kernel(LbsVertexArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lbs_lds[];
    const LbsModel &M = a.M;
    constexpr int PT = LBS_FPT;
    float *A_s = lbs_lds, *coef_s = A_s + PT * 12 * M.J, *W_s = coef_s + LBS_KC * PT;
    const int Jp = M.J | 1;
    const int vt = blockIdx.x / a.pose_tiles, pt = blockIdx.x - vt * a.pose_tiles;
    const int64_t b0 = (int64_t)pt * PT;
    const int v = vt * LBS_FVT + (int)threadIdx.x;
    const int vc = v < M.V ? v : M.V - 1;
    lbs_stage_A<PT, LBS_FVT>(M, a.rig, a.B, b0, A_s);
    {
        const int v0 = vt * LBS_FVT, nv = M.V - v0 < LBS_FVT ? M.V - v0 : LBS_FVT;
        for (int i = threadIdx.x; i < LBS_FVT * M.J; i += LBS_FVT) {   // coalesced: the tile's weights are contiguous
            const int lv = i / M.J, j = i - lv * M.J;
            W_s[lv * Jp + j] = lv < nv ? M.weights[(int64_t)v0 * M.J + i] : 0.f;
        }
    }
    float acc[3][PT];
    lbs_blend<PT, LBS_FVT>(M, a.rig, a.B, b0, vc, coef_s, acc);   // (its barriers also cover A_s and W_s)
    const float *Wv = W_s + threadIdx.x * Jp;
    uint32_t mask = 0;
    for (int j = 0; j < M.J; ++j)
        if (__builtin_amdgcn_ballot_w64(Wv[j] != 0.f) != 0) mask |= 1u << j;
    mask = __builtin_amdgcn_readfirstlane(mask);
#pragma unroll
    for (int p0 = 0; p0 < PT; p0 += 4) {
        if (b0 + p0 >= a.B) break;   // workgroup-uniform
        float T[4][12];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < 12; ++i) T[q][i] = 0.f;
        for (uint32_t m = mask; m; m &= m - 1) {
            const int j = __builtin_ctz(m);
            lbs_skin_joint<4>(Wv[j], A_s + (p0 * M.J + j) * 12, 12 * M.J, T);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = b0 + p0 + q;
            if (b < a.B && v < M.V) {
                const float x = acc[0][p0 + q], y = acc[1][p0 + q], z = acc[2][p0 + q];
                float *o = a.vertices + (b * M.V + v) * 3;
#pragma unroll
                for (int i = 0; i < 3; ++i) o[i] = fmaf(T[q][i * 4], x, fmaf(T[q][i * 4 + 1], y, fmaf(T[q][i * 4 + 2], z, T[q][i * 4 + 3])));
            }
        }
    }
}

// static LDS: dv_s, vp_s [BVT][3][PT] | A_s [PT][12 J] | coef_s [KC][PT]
__global__ __launch_bounds__(LBS_BVT) void lbs_vertex_bwd_kernel(LbsVertexArgs a) {
    constexpr int PT = LBS_BPT, VT = LBS_BVT;
    __shared__ __attribute__((aligned(16))) float dv_s[VT * 3 * PT];
    __shared__ __attribute__((aligned(16))) float vp_s[VT * 3 * PT];
    __shared__ __attribute__((aligned(16))) float A_s[PT * 12 * LBS_MAX_J];
    __shared__ __attribute__((aligned(16))) float coef_s[LBS_KC * PT];
    const LbsModel &M = a.M;
    const int tid = threadIdx.x;
    const int pt = blockIdx.x / a.slices, slice = blockIdx.x - pt * a.slices;
    const int64_t b0 = (int64_t)pt * PT;
    const int64_t N3 = (int64_t)M.V * 3;
    const int nA = 12 * M.J;
    float accA[2][PT], accK[2][PT];   // element tid + 256 i of d_A (12 J <= 384) and of d_coef (K <= 512)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int p = 0; p < PT; ++p) accA[i][p] = accK[i][p] = 0.f;
    lbs_stage_A<PT, VT>(M, a.rig, a.B, b0, A_s);
    for (int vt = slice; vt < a.vertex_tiles; vt += a.slices) {
        const int v0 = vt * VT, nv = M.V - v0 < VT ? M.V - v0 : VT;
        const int v = v0 + tid, vc = v < M.V ? v : M.V - 1;
        float dvp[3][PT];
        {   // (1) lane = vertex
            float acc[3][PT], T[PT][12];
            lbs_blend<PT, VT>(M, a.rig, a.B, b0, vc, coef_s, acc);   // (its first barrier ends the previous tile's phase 3)
#pragma unroll
            for (int q = 0; q < PT; ++q)
#pragma unroll
                for (int i = 0; i < 12; ++i) T[q][i] = 0.f;
            for (int j = 0; j < M.J; ++j) {
                const float w = M.weights[(int64_t)vc * M.J + j];
                if (__builtin_amdgcn_ballot_w64(w != 0.f) != 0) lbs_skin_joint<PT>(w, A_s + j * 12, nA, T);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float4 *dst_d = reinterpret_cast<float4 *>(dv_s + (tid * 3 + c) * PT), *dst_v = reinterpret_cast<float4 *>(vp_s + (tid * 3 + c) * PT);
                float d[PT];
#pragma unroll
                for (int p = 0; p < PT; ++p)
                    d[p] = (b0 + p < a.B && v < M.V) ? a.d_vertices[((b0 + p) * M.V + v) * 3 + c] : 0.f;
#pragma unroll
                for (int p4 = 0; p4 < PT / 4; ++p4) {
                    dst_d[p4] = make_float4(d[p4 * 4], d[p4 * 4 + 1], d[p4 * 4 + 2], d[p4 * 4 + 3]);
                    dst_v[p4] = make_float4(acc[c][p4 * 4], acc[c][p4 * 4 + 1], acc[c][p4 * 4 + 2], acc[c][p4 * 4 + 3]);
                }
#pragma unroll
                for (int p = 0; p < PT; ++p) {   // d_v_posed[i] += T.R[c][i] d_v[c]
                    if (c == 0) dvp[0][p] = dvp[1][p] = dvp[2][p] = 0.f;
#pragma unroll
                    for (int i = 0; i < 3; ++i) dvp[i][p] = fmaf(T[p][c * 4 + i], d[p], dvp[i][p]);
                }
            }
        }
        __syncthreads();
        // (2) lane = element (j, row, col) of d_A
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
            const int e = tid + rd * VT;
            if (e < nA) {
                const int j = e / 12, r = (e % 12) / 4, c = e % 4;
                for (int lv = 0; lv < nv; ++lv) {
                    const float w = M.weights[(int64_t)(v0 + lv) * M.J + j];
                    if (w != 0.f) {
                        const float4 *dp = reinterpret_cast<const float4 *>(dv_s + (lv * 3 + r) * PT);
                        const float4 *xp = reinterpret_cast<const float4 *>(vp_s + (lv * 3 + (c < 3 ? c : 0)) * PT);
#pragma unroll
                        for (int p4 = 0; p4 < PT / 4; ++p4) {
                            const float4 d4 = dp[p4], x4 = xp[p4];
                            const float dd[4] = {d4.x, d4.y, d4.z, d4.w}, xx[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
                            for (int q = 0; q < 4; ++q) accA[rd][p4 * 4 + q] = fmaf(w * dd[q], c < 3 ? xx[q] : 1.f, accA[rd][p4 * 4 + q]);
                        }
                    }
                }
            }
        }
        __syncthreads();
        // (3) d_v_posed into dv_s, lane = k
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 *dst = reinterpret_cast<float4 *>(dv_s + (tid * 3 + c) * PT);
#pragma unroll
            for (int p4 = 0; p4 < PT / 4; ++p4) dst[p4] = make_float4(dvp[c][p4 * 4], dvp[c][p4 * 4 + 1], dvp[c][p4 * 4 + 2], dvp[c][p4 * 4 + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
            const int k = tid + rd * VT;
            if (k < M.K) {
                const float *row = M.blend + (int64_t)k * N3 + (int64_t)v0 * 3;
                const int ncol = nv * 3;
#pragma unroll 4
                for (int col = 0; col < ncol; ++col) {
                    const float bl = row[col];
                    const float4 *dp = reinterpret_cast<const float4 *>(dv_s + col * PT);
#pragma unroll
                    for (int p4 = 0; p4 < PT / 4; ++p4) {
                        const float4 d4 = dp[p4];
                        accK[rd][p4 * 4 + 0] = fmaf(bl, d4.x, accK[rd][p4 * 4 + 0]);
                        accK[rd][p4 * 4 + 1] = fmaf(bl, d4.y, accK[rd][p4 * 4 + 1]);
                        accK[rd][p4 * 4 + 2] = fmaf(bl, d4.z, accK[rd][p4 * 4 + 2]);
                        accK[rd][p4 * 4 + 3] = fmaf(bl, d4.w, accK[rd][p4 * 4 + 3]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        if (b0 + p >= a.B) break;
        float *out = a.partial + ((int64_t)slice * a.B + b0 + p) * M.E;
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
            const int e = tid + rd * VT;
            if (e < nA) out[e] = accA[rd][p];
            if (e < M.K) out[nA + e] = accK[rd][p];
        }
    }
}

__global__ __launch_bounds__(256) void lbs_reduce_kernel(const float *partial, int64_t n, int slices, float *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < slices; ++k) s += partial[k * n + i];
    out[i] = s;
}

// ---------------------------------------------------------------------------------------------------- host
static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// vertex slices of the backward: enough workgroups for the chip at small B, a bounded workspace at large B
static int lbs_slices(int64_t B, int V) {
    const int64_t tiles = ceil_div(V, LBS_BVT), pose_tiles = ceil_div(B, LBS_BPT);
    int64_t s = 2048 / (pose_tiles > 0 ? pose_tiles : 1);
    s = s < 4 ? 4 : s > 16 ? 16 : s;
    return (int)(s < tiles ? s : tiles);
}

// argument checks shared by the three entries; fills M.  Returns 0, or the error
static int lbs_model(const char *what, const snerf_smpl_model *m, int64_t B, LbsModel &M) {
    if (!m) return fail(SNERF_E_BADARG, "%s: model is NULL", what);
    if (B < 0) return fail(SNERF_E_BADARG, "%s: need B >= 0", what);
    if (m->V < 1) return fail(SNERF_E_BADARG, "%s: need V >= 1", what);
    if (m->J < 2 || m->J > LBS_MAX_J) return fail(SNERF_E_BADARG, "%s: need 2 <= J <= %d", what, LBS_MAX_J);
    if (m->NB < 1 || (int64_t)m->NB + 9 * (m->J - 1) > LBS_MAX_K)
        return fail(SNERF_E_BADARG, "%s: need NB >= 1 and NB + 9 (J - 1) <= %d", what, LBS_MAX_K);
    if ((int64_t)m->V * 3 > 0x7fffffffLL / LBS_MAX_J) return fail(SNERF_E_BADARG, "%s: V too large", what);
    if (!m->v_template || !m->blend || !m->J_template || !m->J_dirs || !m->weights || !m->parents)
        return fail(SNERF_E_BADARG, "%s: null pointer in the model", what);
    if (m->parents[0] != -1) return fail(SNERF_E_BADARG, "%s: parents[0] must be -1", what);
    for (int j = 1; j < m->J; ++j)
        if (m->parents[j] < 0 || m->parents[j] >= j) return fail(SNERF_E_BADARG, "%s: parents[%d] must lie in [0, %d)", what, j, j);
    M.v_template = m->v_template;
    M.blend = m->blend;
    M.J_template = m->J_template;
    M.J_dirs = m->J_dirs;
    M.weights = m->weights;
    M.V = m->V;
    M.J = m->J;
    M.NB = m->NB;
    M.K = m->NB + 9 * (m->J - 1);
    M.E = 12 * m->J + M.K;
    for (int j = 0; j < LBS_MAX_J; ++j) M.parents[j] = j < m->J ? m->parents[j] : -1;
    if (ceil_div(B, LBS_BPT) * 16 > 0x7fffffffLL || ceil_div(B, LBS_FPT) * ceil_div(M.V, LBS_FVT) > 0x7fffffffLL)
        return fail(SNERF_E_BADARG, "%s: B too large", what);
    return 0;
}
static int lbs_rows(const char *what, int betas_rows, int64_t B) {
    if (betas_rows != 1 && betas_rows != B) return fail(SNERF_E_BADARG, "%s: betas must have 1 or B rows", what);
    return 0;
}
// floats of the backward's workspace: partial [slices][B][E] | d_rig [B][E] | d_betas rows [B][NB]
static int64_t lbs_ws_floats(const LbsModel &M, int64_t B) { return ((int64_t)lbs_slices(B, M.V) + 1) * B * M.E + B * M.NB; }

}  // namespace snerf

extern "C" int snerf_smpl_lbs_fwd_f32(const snerf_smpl_model *model, const float *betas, int betas_rows, const float *body_pose,
                                      const float *global_orient, int64_t B, float *vertices, float *joints, float *rig,
                                      snerf_stream_t stream) {
    using namespace snerf;
    LbsModel M;
    if (int rc = lbs_model("smpl_lbs_fwd", model, B, M)) return rc;
    if (B == 0) return SNERF_OK;
    if (int rc = lbs_rows("smpl_lbs_fwd", betas_rows, B)) return rc;
    if (!betas || !body_pose || !vertices || !rig) return fail(SNERF_E_BADARG, "smpl_lbs_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    LbsRigArgs R{};
    R.M = M;
    R.betas = betas;
    R.body_pose = body_pose;
    R.global_orient = global_orient;
    R.B = B;
    R.betas_rows = betas_rows;
    R.rig = rig;
    R.joints = joints;
    hipLaunchKernelGGL(lbs_rig_fwd_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, s, R);
    LbsVertexArgs A{};
    A.M = M;
    A.rig = rig;
    A.B = B;
    A.pose_tiles = (int)ceil_div(B, LBS_FPT);
    A.vertex_tiles = (int)ceil_div(M.V, LBS_FVT);
    A.vertices = vertices;
    const int lds = (LBS_FPT * 12 * M.J + LBS_KC * LBS_FPT + LBS_FVT * (M.J | 1)) * (int)sizeof(float);
    hipLaunchKernelGGL(lbs_vertex_fwd_kernel, dim3((unsigned)((int64_t)A.pose_tiles * A.vertex_tiles)), dim3(LBS_FVT), lds, s, A);
    return check_launch("smpl_lbs_fwd");
}

extern "C" int64_t snerf_smpl_lbs_bwd_workspace_bytes(const snerf_smpl_model *model, int64_t B) {
    using namespace snerf;
    LbsModel M;
    if (lbs_model("smpl_lbs_bwd_workspace_bytes", model, B, M)) return -1;
    return lbs_ws_floats(M, B) * (int64_t)sizeof(float);
}

extern "C" int snerf_smpl_lbs_bwd_f32(const snerf_smpl_model *model, const float *betas, int betas_rows, const float *body_pose,
                                      const float *global_orient, const float *rig, const float *d_vertices, const float *d_joints,
                                      int64_t B, void *workspace, int64_t workspace_bytes, float *d_betas, float *d_body_pose,
                                      float *d_global_orient, snerf_stream_t stream) {
    using namespace snerf;
    LbsModel M;
    if (int rc = lbs_model("smpl_lbs_bwd", model, B, M)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {   // nothing to write but the sum over an empty batch
        if (d_betas && betas_rows == 1 && hipMemsetAsync(d_betas, 0, sizeof(float) * M.NB, s) != hipSuccess)
            return fail(SNERF_E_LAUNCH, "smpl_lbs_bwd: memset failed");
        return SNERF_OK;
    }
    if (int rc = lbs_rows("smpl_lbs_bwd", betas_rows, B)) return rc;
    if (!betas || !body_pose || !rig) return fail(SNERF_E_BADARG, "smpl_lbs_bwd: null pointer");
    if (!d_vertices && !d_joints) return fail(SNERF_E_BADARG, "smpl_lbs_bwd: no incoming gradient");
    if (!workspace || workspace_bytes < lbs_ws_floats(M, B) * (int64_t)sizeof(float))
        return fail(SNERF_E_BADARG, "smpl_lbs_bwd: workspace missing or smaller than snerf_smpl_lbs_bwd_workspace_bytes()");
    const int slices = lbs_slices(B, M.V);
    const int64_t n = B * M.E;
    float *partial = (float *)workspace, *d_rig = partial + (int64_t)slices * n, *rows = d_rig + n;
    if (d_vertices) {
        LbsVertexArgs A{};
        A.M = M;
        A.rig = rig;
        A.B = B;
        A.pose_tiles = (int)ceil_div(B, LBS_BPT);
        A.vertex_tiles = (int)ceil_div(M.V, LBS_BVT);
        A.d_vertices = d_vertices;
        A.partial = partial;
        A.slices = slices;
        hipLaunchKernelGGL(lbs_vertex_bwd_kernel, dim3((unsigned)((int64_t)A.pose_tiles * slices)), dim3(LBS_BVT), 0, s, A);
        hipLaunchKernelGGL(lbs_reduce_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, partial, n, slices, d_rig);
    }
    LbsRigArgs R{};
    R.M = M;
    R.betas = betas;
    R.body_pose = body_pose;
    R.global_orient = global_orient;
    R.B = B;
    R.betas_rows = betas_rows;
    R.d_rig = d_vertices ? d_rig : nullptr;
    R.d_joints = d_joints;
    R.d_body_pose = d_body_pose;
    R.d_global_orient = d_global_orient;
    const bool summed = betas_rows == 1 && B > 1;
    R.d_betas_rows = d_betas ? (summed ? rows : d_betas) : nullptr;
    hipLaunchKernelGGL(lbs_rig_bwd_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, s, R);
    if (d_betas && summed) hipLaunchKernelGGL(lbs_sum_rows_kernel, dim3((unsigned)M.NB), dim3(256), 0, s, rows, B, M.NB, d_betas);
    return check_launch("smpl_lbs_bwd");
}
