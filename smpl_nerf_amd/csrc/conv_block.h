// What csrc/conv_block.hip shares with csrc/conv_train.hip: the scalar checks of a block and the launch of its forward kernel.
#pragma once
#include "snerf_common.h"

namespace snerf {

constexpr int CB_MAX_C = 256;       // snerf_conv3x3_block_f32 and the training entries
constexpr int CB_SEG_C = 128;       // above CB_MAX_C input channels the accumulation chain restarts every CB_SEG_C channels
constexpr int CB_TAP_MAX_C = 512;   // snerf_conv3x3_block_tap_f32 and the LPIPS stack (csrc/lpips.hip): VGG16's widest layers

// the scalar checks of a block (an error whatever N is); *Ho, *Wo: the extents of y
int conv_check(const char *what, int64_t N, int Ci, int64_t H, int64_t W, int Co, int pool, int64_t *Ho, int64_t *Wo, int max_c = CB_MAX_C);
// one block on checked arguments, N > 0: y = [maxpool2x2](relu(scale conv3x3_pad1(x, w) + shift))
int conv_launch(const char *what, const float *x, int64_t N, int Ci, int H, int W, const float *w, const float *scale, const float *shift,
                int Co, int relu, int pool, float *y, hipStream_t s);
// ... to the un-pooled map y_full [N,Co,H,W] and the pooled one y_pool [N,Co,H/2,W/2] from the same accumulators; either may be null
int conv_launch_tap(const char *what, const float *x, int64_t N, int Ci, int H, int W, const float *w, const float *scale,
                    const float *shift, int Co, int relu, float *y_full, float *y_pool, hipStream_t s);

}  // namespace snerf
