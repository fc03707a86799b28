// What the two frame kernels that walk pixels x faces share (mesh_render.hip, soft_silhouette.hip): the camera of a frame as the ray
// generator uses it, and the 8 x 8 pixel tile of a workgroup - lane = pixel, grid = tiles x frames, clipped at the right and bottom.
#pragma once
#include "pair_walk.h"

namespace snerf {

constexpr int MR_TILE = 8;                     // a workgroup's pixel tile is MR_TILE x MR_TILE = one lane per pixel
static_assert(MR_TILE * MR_TILE == WAVE, "lane = pixel");

// the camera of frame n as the ray generator uses it: rotation in float64, origin rounded to fp32
struct MrCamera {
    double R[3][3];
    float o[3];
};
__device__ __forceinline__ MrCamera mr_camera(const double *poses, int n) {
    const double *M = poses + (int64_t)n * 16;
    MrCamera c;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c.R[r][k] = M[r * 4 + k];
        c.o[r] = (float)M[r * 4 + 3];
    }
    return c;
}

// Workgroup `block` of a grid of tiles_x tiles_y tiles per frame: its frame n, its tile (tx, ty), the lane's own pixel (i_own,
// j_own) - valid inside the image - and the pixel (i, j) it computes with: its own, or the last column / row, which exists.
struct MrTile {
    int n, tx, ty, i, j;
    bool valid;
    // the tile in pixels, clipped to the image (all wave-uniform)
    __device__ __forceinline__ int x0() const { return tx * MR_TILE; }
    __device__ __forceinline__ int y0() const { return ty * MR_TILE; }
    __device__ __forceinline__ int x1(int W) const { return min(tx * MR_TILE + MR_TILE, W) - 1; }
    __device__ __forceinline__ int y1(int H) const { return min(ty * MR_TILE + MR_TILE, H) - 1; }
};
__device__ __forceinline__ MrTile mr_tile(int block, int tiles_x, int tiles_y, int H, int W, int lane) {
    const int tiles = tiles_x * tiles_y;
    MrTile t;
    t.n = block / tiles;
    const int tile = block - t.n * tiles;
    t.ty = tile / tiles_x;
    t.tx = tile - t.ty * tiles_x;
    const int i_own = t.tx * MR_TILE + (lane & (MR_TILE - 1)), j_own = t.ty * MR_TILE + (lane >> 3);
    t.valid = i_own < W && j_own < H;
    t.i = tail_index(i_own, W, i_own < W);
    t.j = tail_index(j_own, H, j_own < H);
    return t;
}

// host: the tiles of an H x W frame; the grid of N frames is tiles_x tiles_y N workgroups
inline int mr_tiles(int extent) { return (extent + MR_TILE - 1) / MR_TILE; }

}  // namespace snerf
