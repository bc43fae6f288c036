/* gligen_amd_ffn_rows.h -- the row-local kernels of gligen_amd/csrc/ffn.hip by themselves, on the caller's buffers: ff_rows_kernel in
 * each of its forms (plain, <PRE>, <PRE, POST = 1>, <PRE, POST = 2>) and qkv_rows_kernel (PRE 0 / 1, NP 1 / 3), every field of their
 * parameter blocks set by the caller. gl_op_feedforward, gl_op_ff_chain, gl_op_ff_chain_q and gl_op_proj_attention run the same kernels
 * with dense strides, buffers of their own and an attention launch behind the projections; these entries exist so that each kernel is
 * held to a float64 reference element by element, with strides, padded token counts, the input period and the row statistics the engine
 * uses (tests/test_ffn_rows_gpu.py) -- the engine does not go through them. No kernel is added: a shape or form without a row-local
 * kernel answers GL_ERR_UNSUPPORTED (5), a bad argument GL_ERR_ARG, and nothing else runs in its place. Nothing is allocated except the
 * folded weights and the packed fragment stream, from the context's arena (which the call resets). Conventions as in gligen_amd.h:
 * device pointers, bf16 activations, fp32 parameters, row strides in elements.
 *
 * The kernels exist for C = 320 (H = 8 heads of d = 40) and M % 128 == 0 rows; qkv_rows for T % 128 == 0 rows per sample.
 *
 * gl_op_ff_rows:  h = LN(x) W1^T + b1 (normalize = 1; gamma / beta, when given, are folded into W1 / b1 as gl_op_feedforward does)
 *                 y = res + gate * (val(h) gelu(gate(h)) W2^T + b2)                           -> out [M][ldo], stats_out
 *                 (without res, and without pre, the gate is not read: y is the feed-forward itself)
 *   pre = 1       t = pre_res + pre_gate * (x Wpre^T + pre_b) takes the place of x and of res (res / ldres are not read; normalize must
 *                 be 1). mid_out [M][ld_mid] is WRITTEN (with t) only when |gate| <= 1e-20 -- then the residual is read back from it --
 *                 and is left untouched otherwise.
 *   post = 1      out = post_res + (y Wpost^T + post_b); y itself is not stored. Needs pre = 1.
 *   post = 2      out = y, and q = LN(y) Wq^T + bq (gamma_q / beta_q folded into post_w, post_b is not read) goes to
 *                 q [M / qT][8][qTpad][qDP], row-major per head: token rows [0, qT) and columns [0, 40) are written, nothing else.
 *                 qT % 32 == 0 divides M; qTpad >= qT; qDP >= 40, qDP % 4 == 0. Needs pre = 1.
 *   stats_out     optional, float pairs at stats_out[2 * row * stats_ld]: (sum, sum of squares) of the row's final bf16 outputs in
 *                 `out`.
 *
 * gl_op_qkv_rows: pre = 1: t = pre_res + (x Wpre^T + pre_b) -> mid_out, (sum, sum of squares) of t's bf16 rows -> stats_out [M] (optional);
 *                          q, k, v = LN(t) W^T + bias, always normalised.
 *                 pre = 0: q, k, v = (normalize ? LN(x) : x) W^T + bias; mid_out and stats_out are not written.
 *                 w [np * C][C] = to_q [; to_k ; to_v], bias [np * C] or null (zero); gamma / beta, when given, are folded into both.
 *                 np = 3: q [B H][Tpad_q][DP], k [B H][Tpad_k / 64][DP / 8][64][8], vt [B H][DPV][Tpad_k] in the 32-token form of
 *                 gligen_amd_attention_core.h; np = 1: q alone. Token rows [0, T) and head dims [0, 40) of each are written, nothing
 *                 else: Tpad_q >= T, Tpad_k >= T with Tpad_k % 64 == 0, DP >= 40 with DP % 8 == 0, DPV >= 40.
 *                 in_period: 0, or a multiple of T dividing M: output row m reads row m % in_period of x and pre_res.
 * Alignment: x 16 bytes; every other activation buffer and q 8 bytes; k and vt 16 bytes. */
#ifndef GLIGEN_AMD_FFN_ROWS_H
#define GLIGEN_AMD_FFN_ROWS_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gl_ff_rows_args {
    unsigned struct_size;        /* sizeof(gl_ff_rows_args) */
    int M, C;
    const void* x;               /* bf16 [M][ldx] */
    int ldx;
    int normalize;
    float eps;
    const float* gamma;          /* [C] or null, together with beta */
    const float* beta;
    const float* w1;             /* [8C][C]: value rows, then gate rows */
    const float* b1;             /* [8C] */
    const float* w2;             /* [C][4C] */
    const float* b2;             /* [C] */
    const void* res;             /* bf16 [M][ldres] or null */
    int ldres;
    const float* gate;           /* one float or null */
    void* out;                   /* bf16 [M][ldo] */
    int ldo;
    void* stats_out;             /* or null */
    int stats_ld;
    int pre, post;
    const float* pre_w;          /* [C][C] */
    const float* pre_b;          /* [C] */
    const void* pre_res;         /* bf16 [M][ld_pre_res] */
    int ld_pre_res;
    const float* pre_gate;       /* one float or null */
    void* mid_out;               /* bf16 [M][ld_mid] */
    int ld_mid;
    const float* post_w;         /* [C][C]: Wpost (post = 1) or Wq (post = 2) */
    const float* post_b;         /* [C] (post = 1) */
    const void* post_res;        /* bf16 [M][ld_post_res] (post = 1) */
    int ld_post_res;
    const float* gamma_q;        /* [C] (post = 2) */
    const float* beta_q;
    void* q;                     /* (post = 2) */
    int qDP, qT, qTpad;
} gl_ff_rows_args;

typedef struct gl_qkv_rows_args {
    unsigned struct_size;        /* sizeof(gl_qkv_rows_args) */
    int M, C, H;
    const void* x;               /* bf16 [in_period ? in_period : M][ldx] */
    int ldx;
    int normalize;
    float eps;
    int pre;
    const float* pre_w;          /* [C][C] */
    const float* pre_b;          /* [C] */
    const void* pre_res;         /* bf16 rows as x, [..][ld_pre_res], or null */
    int ld_pre_res;
    void* mid_out;               /* bf16 [M][ld_mid] */
    int ld_mid;
    void* stats_out;             /* float [M][2] or null */
    const float* gamma;          /* [C] or null, together with beta */
    const float* beta;
    int np;                      /* 1 or 3 */
    const float* w;              /* [np C][C] */
    const float* bias;           /* [np C] or null */
    void* q;
    void* k;
    void* vt;
    int DP, DPV, T, Tpad_q, Tpad_k, in_period;
} gl_qkv_rows_args;

int gl_op_ff_rows(gl_ctx* ctx, const gl_ff_rows_args* args, gl_stream s);
int gl_op_qkv_rows(gl_ctx* ctx, const gl_qkv_rows_args* args, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
