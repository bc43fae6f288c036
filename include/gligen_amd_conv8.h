/* gligen_amd_conv8.h -- run conv8_kernel of libgligen_amd.so (the 3x3 / stride 1 / pad 1 convolution of 8 x 8 images that stages every
 * image once per 64-channel chunk, gligen_amd/csrc/gemm_conv8.hip) by name on the caller's buffers, with a given column tile and K
 * split, whatever the launcher would route; ask the router what it does with a problem; and set the family's developer knobs
 * (GL_CONV8, GL_CONV8_BN, GL_CONV8_SPLITS of tools/README.md) as a call. For tests (tests/test_conv8_gpu.py, tests/test_conv8_cpu.py)
 * -- the engine does not go through these entries. Conventions as in gligen_amd.h. The knobs are process-wide: set them before
 * launching, not while other threads launch. */
#ifndef GLIGEN_AMD_CONV8_H
#define GLIGEN_AMD_CONV8_H
#include <stddef.h>

#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One 3x3 convolution of the NHWC sources x0 [B][H][W][C0] and x1 [..][C1] (bf16; x1 NULL, C1 = 0: one source) to N channels:
 *   v = sum + bias[n] + bias2[(m / rows_per_b) * bias2_ld + n];  v = act(v)   (0 none, 1 SiLU);   m = (b H + y) W + x
 *   out[m * ldo + n] = res ? res[m * ldres + n] + v : v            bf16, or fp32 when out_f32
 * w: fp32 OIHW [N][C0 + C1][3][3], packed as gl_op_conv3x3 packs it. bias, bias2, res may be NULL; rows_per_b >= 1.
 * gl_conv8_routed reads the geometry, the epilogue's pointers (as flags) and act / out_f32 only; gl_op_conv8x8 also
 *   bn        column tile, 64 or 80, dividing N
 *   splits    K split in whole 64-channel chunks, 1 .. (C0 + C1) / 64, every part with at least one chunk (3 chunks: 1, 2, 3; 4: 1, 2, 4)
 *   grid_cap  resident workgroups (0: 256)
 *   slabs     fp32 [splits][B H W][N], the caller's, for splits > 1 (slab_bytes: its size); a split launch runs the reduce pass
 *             (splitk_reduce_kernel) that applies the epilogue, an unsplit one applies it in the kernel and touches no slab. */
typedef struct gl_conv8_args {
    unsigned struct_size;   /* sizeof(gl_conv8_args) */
    const void* x0;
    const void* x1;
    int C0, C1, B, H, W, N, stride, ups, pad_lo;
    const void* w;
    const float* bias;
    const float* bias2;
    int bias2_ld, rows_per_b;
    const void* res;
    int ldres;
    int act, out_f32;
    void* out;
    int ldo;
    int bn, splits, grid_cap;
    float* slabs;
    size_t slab_bytes;
} gl_conv8_args;

/* Would the launcher's router hand this conv to conv8_kernel (1) or leave it where it was (0)? Host code only: no context, nothing is
 * dereferenced. < 0: a bad argument. */
int gl_conv8_routed(const gl_conv8_args* args);

/* conv8_kernel on the caller's buffers. GL_ERR_UNSUPPORTED for a problem the kernel has no form for (images other than 8 x 8, stride,
 * upsample, channels that are no multiple of 64); GL_ERR_ARG for a tile / split / cap / slab size that does not fit the problem. */
int gl_op_conv8x8(gl_ctx* ctx, const gl_conv8_args* args, gl_stream s);

/* on: 1 the engine's eligible convs run on conv8_kernel (default), 0 never -- the launches are then those of gemm_u_kernel. bn, splits:
 * the routed launches' column tile (64 | 80) and K split, 0 = the shipped choice / the model. gl_gemm_force_clear
 * (gligen_amd_gemm_plans.h) puts all three back too. */
int gl_conv8_force_knobs(int on, int bn, int splits);

#ifdef __cplusplus
}
#endif
#endif
