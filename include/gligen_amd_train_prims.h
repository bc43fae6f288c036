/* gligen_amd_train_prims.h -- the primitives of the training path in libgligen_amd.so, one entry each: attention, the Linear products,
 * LayerNorm, GroupNorm + SiLU, GEGLU, the dot / MSE reduction and the 3x3 convolutions, forward and backward, exactly as the training
 * step composes them (the same kernels, the same launch helpers, the engine's arena and split-K workspace). They exist so that each primitive can be
 * held to a float64 reference by itself (tests/test_train_prims_gpu.py); the training step does not go through them.
 * Conventions as in gligen_amd.h: fp32 device pointers, work queued on `s`, GL_OK or an error code with gl_last_error(). An output
 * that is NULL is not produced unless it is marked required; a backward output needs the backward's input gradient. */
#ifndef GLIGEN_AMD_TRAIN_PRIMS_H
#define GLIGEN_AMD_TRAIN_PRIMS_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* q [B][Nq][H D], k / v [B][Nk][H D], dout [B][Nq][H D] (NULL: forward only). o [B][Nq][H D] = softmax(q k^T / sqrt(D)) v per head and
 * lse [B][H][Nq] = the rows' log-sum-exp of the scaled scores (both required); dq, dk, dv shaped like q, k, v. dk and dv come
 * together; both NULL selects the training step's dq-only call. D is one of 32, 40, 64, 80, 160. */
int gl_op_train_attention(gl_ctx* ctx, int B, int H, int D, int Nq, int Nk, const float* q, const float* k, const float* v, const float* dout,
                          float* o, float* lse, float* dq, float* dk, float* dv, gl_stream s);

/* y [M][N] = x [M][K] W[N][K]^T + b (b may be NULL); with dy [M][N]: dx [M][K] = dy W, dW [N][K] = dy^T x, db [N] = column sums of
 * dy. Any K and N the training path meets: contraction lengths that are no multiple of 64 take its zero-padded forms. */
int gl_op_train_linear(gl_ctx* ctx, int M, int N, int K, const float* x, const float* W, const float* b, const float* dy, float* y, float* dx,
                       float* dW, float* db, gl_stream s);

/* nn.LayerNorm over C of x [R][C]: y = xhat g + b, xhat [R][C], rstd [R]; with dy [R][C]: dx [R][C] (added to what dx holds when
 * accumulate is not 0), dgamma [C], dbeta [C]. */
int gl_op_train_layernorm(gl_ctx* ctx, int R, int C, float eps, const float* x, const float* g, const float* b, const float* dy, int accumulate,
                          float* y, float* xhat, float* rstd, float* dx, float* dgamma, float* dbeta, gl_stream s);

/* GroupNorm(32 groups) over pixel rows x [B][HW][C], then SiLU when silu is not 0: a, xhat [B][HW][C], rstd [B][32]; with da: dx
 * [B][HW][C] (added to what dx holds when accumulate is not 0). C is a multiple of 32. */
int gl_op_train_groupnorm(gl_ctx* ctx, int B, int HW, int C, int silu, float eps, const float* x, const float* g, const float* b, const float* da,
                          int accumulate, float* a, float* xhat, float* rstd, float* dx, gl_stream s);

/* GEGLU of u [R][2 I] = (val | gate): h [R][I] = val gelu(gate) (erf GELU); with dh [R][I]: du [R][2 I]. */
int gl_op_train_geglu(gl_ctx* ctx, int R, int I, const float* u, const float* dh, float* h, float* du, gl_stream s);

/* out[0] = scale (1 - tanh(alpha[0])^2) sum a b (mode 0: a tanh gate's gradient) or mean((a - b)^2) (mode 1: the loss; alpha is
 * not read) over n elements; out is required. */
int gl_op_train_dot(gl_ctx* ctx, int64_t n, const float* a, const float* b, const float* alpha, float scale, int mode, float* out, gl_stream s);

/* The split-precision 3x3 / pad 1 conv of the ResBlocks and of the two resampling layers over pixel rows x [B][H W][Cin], w_oihw
 * [Cout][Cin][3][3], bias [Cout] (may be NULL). geom 0: stride 1, y [B][H W][Cout]; geom 1: Downsample (stride 2; H and W even), y
 * [B][H/2 W/2][Cout]; geom 2: Upsample (nearest 2x, then the conv), y [B][2H 2W][Cout]. y is required. With dy (shaped like y): dx
 * [B][H W][Cin], the input gradient as the step forms it -- the flipped, channel-exchanged filter on dy (geom 0), on dy zero-inserted at
 * the even positions (geom 1), or on dy followed by 2 x 2 block sums (geom 2). Cin and Cout are multiples of 64; geom 1 and 2 have
 * Cin == Cout. */
int gl_op_train_conv3(gl_ctx* ctx, int B, int H, int W, int Cin, int Cout, int geom, const float* x, const float* w_oihw, const float* bias,
                      const float* dy, float* y, float* dx, gl_stream s);

/* The fp32 direct 3x3 / stride 1 / pad 1 conv of the first and the last conv (any channel counts): y [B][H W][Cout] (required). With dy
 * [B][H W][Cout]: dx [B][H W][n], the data gradient for the input channels [c0, c0 + n) alone (the direct conv over rows c0 .. c0 + n of
 * the flipped, channel-exchanged filter), and dW [Cout][Cin][3][3], the weight gradient (im2col of x, then the Linear weight gradient). */
int gl_op_train_conv_direct(gl_ctx* ctx, int B, int H, int W, int Cin, int Cout, int c0, int n, const float* x, const float* w_oihw,
                            const float* bias, const float* dy, float* y, float* dx, float* dW, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
