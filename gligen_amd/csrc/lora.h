// Low-rank update of an fp32 weight matrix in place: the merge of a LoRA adapter into a module's parameters, load-time work.
// See lora.hip; entry point in include/gligen_amd_lora.h.
#pragma once
#include "common.h"

namespace gl {

// W [N][K] += scale * up [N][r] @ down [r][K], fp32 device tensors, row-major, in place. A conv weight [Cout][Cin][kh][kw] with
// down [r][Cin][kh][kw] and up [Cout][r][1][1] is the same call with K = Cin kh kw. Any N, K, r >= 1; W must not overlap up or down.
// *launched (may be null) tells whether a kernel was launched: scale == 0 launches none.
int lora_merge_launch(float* W, const float* up, const float* down, int N, int K, int r, float scale, hipStream_t s, int* launched);

}  // namespace gl
