// The tile extents of csrc/ssim.hip, one `constexpr int NAME = value;` per line: smpl_nerf_amd/ops.py reads this file (ops.SSIM_TILES)
// so that the tests can place their shapes on the tile edges.
#pragma once

namespace snerf {

constexpr int SSIM_THREADS = 256;         // lanes of a workgroup, forward and backward
constexpr int SSIM_TILE = 32;             // forward: a workgroup owns SSIM_TILE x SSIM_TILE windows; backward: as many input pixels
constexpr int SSIM_BWD_TILE_SMALL = 16;   // backward tile side of the windows whose 32 x 32 tile does not fit the LDS
constexpr int SSIM_BWD_SMALL_FROM_K = 29; // ... which are the window sizes from this one up (asserted against the layout in ssim.hip)
constexpr int SSIM_MAX_K = 33;            // largest window size k
constexpr int SSIM_LDS_BYTES = 163840;    // LDS of a CU: the limit both kernels' dynamic LDS is raised to

}  // namespace snerf
