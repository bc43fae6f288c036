/* gligen_amd_norm.h -- the normalisation kernels of gligen_amd/csrc/norm.hip by themselves, on the caller's buffers: the statistics-only
 * GroupNorm (groupnorm_coef_launch: gn_stats_kernel + gn_coef_kernel, or gn_small_coef_kernel<256 | 1024>) and ln_kernel with every field
 * of its parameter block set by the caller. gl_op_groupnorm (gligen_amd.h) runs the full GroupNorm (gn_stats_kernel + gn_apply_kernel, or
 * gn_small_kernel<256 | 1024>) and gl_op_layernorm the dense LayerNorm; the engine reaches the forms declared here only through the conv
 * or the GEMM behind them. These entries exist so that each kernel is held to a float64 reference element by element at ragged sizes
 * (tests/test_norm_gpu.py) -- the engine does not go through them, and no kernel is added. Conventions as in gligen_amd.h: device
 * pointers, bf16 activations, fp32 parameters, row strides in elements.
 *
 * gl_op_groupnorm_coef: the inputs of gl_op_groupnorm (GroupNorm over 32 groups of the channel concat [x0 ; x1], x0 [B][HW][C0], x1
 *                 [B][HW][C1] or null with C1 = 0). Writes coef [B][(C0 + C1) / 8][16] floats: for every 8 consecutive channels their
 *                 a = rstd * gamma, then their c = beta - mean * a, so that y = x * a + c (the consumer applies it, and the SiLU). On the
 *                 two-launch path (HW > 256 or (C0 + C1) / 32 % 4 != 0) these are the bits gl_op_groupnorm's own apply pass uses:
 *                 its output without SiLU is bf16(fma(x, a, c)). *launches (optional) receives the number of kernel launches, 1 or 2.
 * gl_op_layernorm_rows: y [B][Tpad][ldy]: row t < N1 from x [B][N1][ldx], N1 <= t < N1 + N2 from x2 [B][N2][C] (dense), the other rows
 *                 zero; columns [C, ldy) of every row zero. gamma and beta both null: (x - mean) * rstd without the affine part.
 *                 ldx / ldy = 0 stand for C; otherwise >= C and a multiple of 8. C % 8 == 0, C <= 1536, Tpad >= N1 + N2.
 *
 * Both, and gl_op_groupnorm, answer GL_ERR_ARG (2) to a null required pointer and to x0, x1, y, x, x2, gamma, beta or coef that is not
 * 16-byte aligned, GL_ERR_ARG / GL_ERR_UNSUPPORTED (5) to a shape the kernels refuse, and launch nothing then. */
#ifndef GLIGEN_AMD_NORM_H
#define GLIGEN_AMD_NORM_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gl_layernorm_rows_args {
    unsigned struct_size;        /* sizeof(gl_layernorm_rows_args) */
    const void* x;               /* bf16 [B][N1][ldx] */
    const void* x2;              /* bf16 [B][N2][C], or null with N2 = 0 */
    int B, N1, N2, Tpad, C;
    float eps;
    const float* gamma;          /* [C] or null, together with beta */
    const float* beta;
    void* y;                     /* bf16 [B][Tpad][ldy] */
    int ldx, ldy;
} gl_layernorm_rows_args;

int gl_op_groupnorm_coef(gl_ctx* ctx, const void* x0, int C0, const void* x1, int C1, int B, int HW, const float* gamma, const float* beta,
                         float eps, float* coef, int* launches, gl_stream s);
int gl_op_layernorm_rows(gl_ctx* ctx, const gl_layernorm_rows_args* args, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
