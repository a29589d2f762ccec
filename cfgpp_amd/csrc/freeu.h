// FreeU launcher (freeu_kernel.hip; used by unet.hip): hidden[:, :C_h / 2] *= b and the low-pass of skip scaled by s, in place on
// halo-padded NHWC fp16 tensors of `rows` rows, ONE launch; either pointer may be null.  tw: device copy of freeu_twiddles(H, W) -
// 2 H + 2 W floats {cos 2 pi y / H | sin 2 pi y / H | cos 2 pi x / W | sin 2 pi x / W}, computed in double, rounded to fp32.
#pragma once
#include "common.h"

void freeu_twiddles(int H, int W, float* out);
int freeu_launch(half_t* hidden, int C_h, half_t* skip, int C_s, int rows, int H, int W, float b, float s, const float* tw,
                 hipStream_t st);
