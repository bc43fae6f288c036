/* gligen_amd_gemm_plans.h -- run the GEMM / conv launcher of libgligen_amd.so with one named plan, and read back what it ran.
 * Which tile, K split, resident grid and XCD item order a problem gets is decided at run time (shipped table, analytic model,
 * on-device tuner); these entries exist so that every plan the planner can choose is held to a reference by itself
 * (tests/test_gemm_candidates_gpu.py, tests/test_gemm_epilogues_gpu.py) -- the engine does not go through them. They mirror the GL_GEMM_* / GL_CONV_HALO* / GL_WIDE_XCD
 * developer switches (tools/README.md) as calls. Conventions as in gligen_amd.h. The forcing is process-wide: set it before
 * launching, not while other threads launch; the log is per calling thread. */
#ifndef GLIGEN_AMD_GEMM_PLANS_H
#define GLIGEN_AMD_GEMM_PLANS_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tile (tm, tn in units of 32 rows / columns: 4x5, 4x4, 2x5, 2x4, 2x2), the K split (1 .. 32) and the cap on resident
 * workgroups (0: 512) of gemm_p_kernel / gemm_u_kernel. tm = 0: no forced tile (the cap still holds). While a tile is forced, the
 * problems that would go to conv_halo_kernel / gemm_wide_kernel run on gemm_u_kernel. A choice that does not fit a problem (the
 * split leaves fewer than two K tiles per part, the workspace is too small, a tile the epilogue has no form for, a split count such
 * as 6 of 10 K tiles that is the same launch as 5) is NOT an error: that problem is planned as usual -- read the log. */
int gl_gemm_force_plan(int tm, int tn, int splits, int grid_cap);

/* halo_splits / wide_splits: K split of conv_halo_kernel / gemm_wide_kernel (0: automatic). wide_xcd: the wide kernel's item order
 * (-1: by column-tile count, 0 linear, 1 contiguous ranges per XCD). xcd_boxes: gemm_u_kernel's XCD box partition (1 on, 0 linear
 * ranges). halo: eligible 3x3 convs with M >= 256 * halo go to conv_halo_kernel (8; 0: never). wide: what gemm_wide_kernel takes (0
 * nothing, 1 the GEGLU projections, 2 every row GEMM it is eligible for). */
int gl_gemm_force_knobs(int halo_splits, int wide_splits, int wide_xcd, int xcd_boxes, int halo, int wide);

/* Drop gl_gemm_force_plan and put the six knobs back to their defaults (with GL_DEV_SWITCHES=1: to what the environment says). */
int gl_gemm_force_clear(void);

typedef struct gl_gemm_plan_record {
    char kernel[96];      /* kernel name with template arguments, " + splitk_reduce_kernel" behind a split launch */
    int family;           /* 0 gemm_glds_kernel, 1 gemm_p_kernel, 2 gemm_u_kernel, 3 conv_halo_kernel, 4 gemm_wide_kernel, 5 conv8_kernel */
    int M, N, K;
    int tm, tn;           /* tile in units of 32 (halo / wide: tm = 8; conv8_kernel: tm = 8, tn in units of 16) */
    int splits;
    int grid;             /* workgroups launched (gemm_glds_kernel: tiles, times splits in z) */
    int n_items;          /* work items: tiles x splits (gemm_glds_kernel: tiles) */
    int box, rm, rz;      /* p / u: XCD partition (box < 0: linear ranges; else lgm | lgn << 4, rows and splits per box); else 0 */
    int units_per_split;  /* K tiles of 64 per split; conv_halo_kernel, conv8_kernel: chunks of 64 channels per split */
    int xcd;              /* gemm_wide_kernel: item order (1: contiguous ranges per XCD); else 0 */
} gl_gemm_plan_record;

#define GL_GEMM_PLAN_LOG_SIZE 32

/* The launches gemm_launch made on the calling thread since gl_gemm_plan_log_clear: the newest min(launches, 32, max) in launch
 * order into out, their number into *n_written, the launches since the clear into *n_launches (more than 32: the oldest fell out). */
int gl_gemm_plan_log_clear(void);
int gl_gemm_plan_log(gl_gemm_plan_record* out, int max, int* n_written, int* n_launches);

/* The projections of gl_op_attention alone, into the caller's buffers, so that a test can hold q, k and v^T to a reference and see what
 * is not written: one fused launch when xq == xkv (same pointer, C == Ck, Nq == Nk), else the q scatter, the k scatter and the v^T
 * projection. Tokens are padded with zero rows to tq / tk (multiples of 64), and those rows are written.
 *   q  [B H][tq_pad][dp]        row-major; rows >= tq and columns >= d are not written
 *   k  [B H][tk_pad / 64][dp / 8][64][8]   the key-tile layout (element (t, c) at (t / 64, c / 8, t % 64, c % 8)); columns >= d not written
 *   vt [B H][dpv][tk_pad]       feature rows >= d not written; inside every group of 16 tokens (32 when vt_perm32) the quads of 4 tokens
 *                               are stored in the order 0 2 1 3 (0 2 4 6 1 3 5 7)
 * With q, k and vt all NULL only *layout is filled (the sizes to allocate). */
typedef struct gl_attn_proj_layout { int d, dp, dpv, tq, tk, tq_pad, tk_pad, vt_perm32; } gl_attn_proj_layout;
int gl_op_attention_project(gl_ctx* ctx, const void* xq, const void* xkv, int B, int Nq, int Nk, int C, int Ck, int H, const float* wq,
                            const float* wk, const float* wv, void* q, void* k, void* vt, gl_attn_proj_layout* layout, gl_stream s);

/* The second token range of the same buffers (what the fuser's attention does with the grounding tokens behind the visual ones):
 * the fused q, k, v^T launch of x [B][Tr][C] (bf16; Tr % 64 == 0) whose row t of a sample lands at token tok_off + t
 * (tok_off % 64 == 0), with an optional bias [3C] (q | k | v order). q, k, vt are buffers in the layouts above that already exist --
 * typically filled by gl_op_attention_project -- and *layout says how they were laid out (d, dp, dpv, tq_pad, tk_pad, vt_perm32 are read;
 * tok_off + Tr has to fit tq_pad and tk_pad). Nothing but the Tr token rows of the range is written. */
int gl_op_attention_project_range(gl_ctx* ctx, const void* x, int B, int Tr, int tok_off, int C, int H, const float* wq, const float* wk,
                                  const float* wv, const float* bias, void* q, void* k, void* vt, const gl_attn_proj_layout* layout, gl_stream s);

/* One gemm_launch with the engine's split-K workspace and an epilogue filled field by field, so that every epilogue the model's own
 * launches use can run under every plan. The operand: conv = 0, bf16 rows x0 [M][K] (w: bf16 [N][K], as gl_op_linear takes it); conv = 1,
 * the 3x3 conv of the NHWC sources x0 [B][H][W][C0] and x1 [..][C1] (x1 NULL, C1 = 0: one source) with stride, ups, pad_lo as in
 * gl_op_conv3x3, w: fp32 OIHW [N][C0 + C1][3][3], packed as there (M and K follow from the geometry and are not read). The epilogue:
 *   v = acc + bias[n] + bias2[(m / rows_per_b) * bias2_ld + n];  v = act(v)   (GL_ACT_*)
 *   mode 0, row-major [..][ldo] bf16 (out_f32: fp32): row r = (m / remap_in) * remap_out + m % remap_in + remap_off when remap_in > 0,
 *           else m; out[r] = res ? res[r * ldres ..] + (gate ? *gate : 1) * v : v   (gate: a device scalar)
 *   mode 3, fp32 [M / rows_per_b][n_real][rows_per_b]: the channels n < n_real alone
 * rows_per_b >= 1 always. What the launcher's validation refuses comes back as its error; this entry itself only looks at struct_size,
 * null pointers, the mode and the conv geometry it computes M and K from: every size and stride is the caller's to get right. */
#define GL_ACT_NONE 0
#define GL_ACT_SILU 1
#define GL_ACT_GELU 3
#define GL_ACT_QUICK_GELU 4
typedef struct gl_gemm_epilogue_args {
    unsigned struct_size;   /* sizeof(gl_gemm_epilogue_args) */
    int conv;
    int M, N, K;
    const void* x0;
    const void* x1;
    int C0, C1, B, H, W, stride, ups, pad_lo;
    const void* w;
    const float* bias;
    const float* bias2;
    int bias2_ld, rows_per_b;
    const void* res;
    int ldres;
    const float* gate;
    int act, out_f32, mode, n_real;
    int remap_in, remap_out, remap_off;
    void* out;
    int ldo;
} gl_gemm_epilogue_args;
int gl_op_gemm_epilogue(gl_ctx* ctx, const gl_gemm_epilogue_args* args, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
