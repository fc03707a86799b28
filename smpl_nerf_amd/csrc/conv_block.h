// What csrc/conv_block.hip shares with csrc/conv_train.hip: the scalar checks of a block and the launch of its forward kernel.
#pragma once
#include "snerf_common.h"

namespace snerf {

constexpr int CB_MAX_C = 256;

// the scalar checks of a block (an error whatever N is); *Ho, *Wo: the extents of y
int conv_check(const char *what, int64_t N, int Ci, int64_t H, int64_t W, int Co, int pool, int64_t *Ho, int64_t *Wo);
// one block on checked arguments, N > 0: y = [maxpool2x2](relu(scale conv3x3_pad1(x, w) + shift))
int conv_launch(const char *what, const float *x, int64_t N, int Ci, int H, int W, const float *w, const float *scale, const float *shift,
                int Co, int relu, int pool, float *y, hipStream_t s);

}  // namespace snerf
