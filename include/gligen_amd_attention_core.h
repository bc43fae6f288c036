/* gligen_amd_attention_core.h -- run ONE attention kernel of libgligen_amd.so on the caller's q, k and v^T buffers. gl_op_attention and
 * the engine always put projection GEMMs in front of the kernel and let attn_launch pick it; this entry exists so that every
 * instantiation in the binary is held to a float64 reference by itself, on exact bf16 operands, at the token-count edges and with
 * realistic contents in the padding (tests/test_attention_core_gpu.py) -- the engine does not go through it. No kernel is added for
 * it: the selector calls the launch helpers attn_launch calls. Conventions as in gligen_amd.h.
 *
 * Operation: o[b][i][h d + c] = sum_j softmax_j(d^-0.5 q_i . k_j) v_j[c] over the Nk real keys, per sample b and head h, bf16 in and out.
 *
 * Buffers (layout->d, dp, dpv, tq_pad, tk_pad, vt_perm32 as gl_op_attention_project reports them; tq and tk are not read here;
 * tq_pad % 128 == 0 >= Nq, tk_pad % 64 == 0 >= Nk; dp = 48 / 80 / 160 and dpv = 64 (48 with vt_perm32) / 96 / 160 for d = 40 / 80 / 160):
 *   q  [B H][tq_pad][dp]                    row-major
 *   k  [B H][tk_pad / 64][dp / 8][64][8]    key-tile layout: element (t, c) at (t / 64, c / 8, t % 64, c % 8)
 *   vt [B H][dpv][tk_pad]                   inside every group of 16 tokens (32 with vt_perm32) the quads of 4 tokens are stored in
 *                                           the order 0 2 1 3 (0 2 4 6 1 3 5 7)
 *   o  [B][o_rows_per_b][ldo]               head h of token i at o[(b o_rows_per_b + i) ldo + h d ...]; ldo % 4 == 0, 8-byte aligned
 *
 * The contract of the kernels, region by region (lines of gligen_amd/csrc/attention.hip; "1" attn_kernel, "2" attn2_kernel,
 * "3" attn3_kernel). nt = ceil(Nk / 64) key tiles are read, so with tk_pad = 64 nt every element of k and vt is loaded.
 *
 *   MUST HOLD A VALUE
 *   vt row d, columns [0, Nk) = 1.0 where dpv > d     the softmax denominator is row d of O^T = V^T P^T (1: 272-284, 2: 609-620,
 *                                                     3: 1032-1044; attn_vt_ones_launch 1104-1116). At d = 160 (dpv == d) there is
 *                                                     no such row: the denominator is a VALU sum (241-244, 286).
 *   k column 40 at d = 40 = 1.0 for 2 and 3            1 overwrites it with 1.0 on the way to LDS (143), so there any FINITE value serves;
 *     (1: any finite value)                            2 and 3 copy the tile by DMA (407-415, 736-744) and multiply q column 40 = -m
 *                                                     by it (432-434, 558-559; 763-765, 829-830, 951-952): must be 1.0 for keys < Nk.
 *   q columns [d, dp) of rows < Nq, k columns          multiplied into the scores as they are (173-176, 476-482, 847-853): q column c
 *     (d, dp) at d = 40 (41..47)                       times k column c. The product relies on their product being 0; this entry's
 *                                                     tests write 0 into both. (q column 40 itself is NOT read: 99, 433, 764
 *                                                     overwrite it.) dp == d at d = 80 and 160: no such columns.
 *   vt rows (d, dpv)                                   accumulated into O^T rows that are never stored (296, 628, 1051) and never
 *                                                     read back: FINITE is all they need (a NaN there stays in its own row).
 *
 *   READ, BUT WITHOUT EFFECT ON ROWS < Nq (must be finite: the kernels promise nothing for NaN / Inf)
 *   q rows [Nq, tq_pad)                                loaded by the lanes of those rows (93, 427, 758; the 8-wave kernel clamps rows
 *                                                     >= tq_pad to row tq_pad - 1: 393); softmax state is per lane = per query row
 *                                                     (190-245, 530-575, 919-963), wave-wide votes (200, 226, 542, 564, 808, 941, 957)
 *                                                     only decide whether a rescale by exactly 1.0 runs; nothing is stored (289, 621,
 *                                                     1046). At d = 40 kernel 3 a row whose denominator leaves (0, 1e30) makes its
 *                                                     workgroup run again with the exact maximum (997-1029): other bits may then
 *                                                     differ by rounding, which is why such rows must be of the real rows' kind.
 *   k rows and vt columns [Nk, tk_pad)                 their scores are computed and then replaced by -1e30 before anything reads
 *                                                     them (181-189, 518-529, 907-918): exp2 gives exactly 0 and 0 * v is exactly 0
 *                                                     for finite v (in the ones row too). Nothing else guards them.
 *
 *   NEVER READ OR WRITTEN
 *   o rows >= Nq of every sample, o columns outside [0, H d)   (289-301, 621-634, 1046-1056: stores of 4 elements at column h d + c, c < d)
 *   o is never read.
 */
#ifndef GLIGEN_AMD_ATTENTION_CORE_H
#define GLIGEN_AMD_ATTENTION_CORE_H
#include "gligen_amd.h"
#include "gligen_amd_gemm_plans.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kernel: which kernel runs.
 *   GL_ATTN_CORE_AUTO   what attn_launch picks for (d, Nk, vt_perm32) -- the product's choice, GL_ATTN_V2 included
 *   GL_ATTN_CORE_V1     attn_kernel: d = 40, 80, 160, any Nk; vt_perm32 = 0
 *   GL_ATTN_CORE_V2_W4  attn2_kernel with 4 waves, GL_ATTN_CORE_V2_W8 with 8 (256-row query blocks): d = 40, vt_perm32 = 0, Nk > 128
 *   GL_ATTN_CORE_V3     attn3_kernel: d = 40 (dpv = 48) and 80, vt_perm32 = 1, Nk > 128
 * A named kernel that has no instantiation for (d, vt_perm32, dpv), or a pipelined kernel asked for with Nk <= 128 (the product never
 * sends it there), answers GL_ERR_UNSUPPORTED (5) and launches nothing. The regime counters of gl_attn_regime_counters count here
 * as they do in gl_op_attention. */
enum { GL_ATTN_CORE_AUTO = 0, GL_ATTN_CORE_V1 = 1, GL_ATTN_CORE_V2_W4 = 2, GL_ATTN_CORE_V2_W8 = 3, GL_ATTN_CORE_V3 = 4 };

int gl_op_attention_core(gl_ctx* ctx, const void* q, const void* k, const void* vt, const gl_attn_proj_layout* layout, int B, int H, int Nq,
                         int Nk, void* o, int ldo, int o_rows_per_b, int kernel, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
