/* gligen_amd_lora.h -- the merge of a LoRA adapter into fp32 parameters in libgligen_amd.so: a low-rank update of a weight matrix in
 * place on the device. Load-time work: the packed engine is rebuilt from the merged parameters afterwards (gligen_amd/lora.py).
 * Conventions as in gligen_amd.h. */
#ifndef GLIGEN_AMD_LORA_H
#define GLIGEN_AMD_LORA_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* W [N][K] += scale * up [N][r] @ down [r][K]: W[n][k] += scale * sum_{i < r} up[n][i] * down[i][k], fp32 device tensors, row-major,
 * in place, no workspace. A conv weight [Cout][Cin][kh][kw] with down [r][Cin][kh][kw] and up [Cout][r][1][1] is the same call with
 * K = Cin * kh * kw.
 * One fp32 accumulator per element takes the ranks in ascending order through fused multiply-adds, and one more fused multiply-add
 * adds scale times it to W: the result does not depend on the grid or on launch order, so two calls give the same bits.
 * scale == 0 launches nothing and leaves W bit for bit. Any N, K, r >= 1.
 * Refused by name: non-positive sizes, and W overlapping up or down. */
int gl_op_lora_merge(gl_ctx* ctx, float* W, const float* up, const float* down, int N, int K, int r, float scale, gl_stream stream);

#ifdef __cplusplus
}
#endif
#endif
