/* gligen_amd_vae.h -- the attention of the autoencoder's AttnBlock in libgligen_amd.so: which form a context runs, and the operator by
 * itself. Conventions as in gligen_amd.h. */
#ifndef GLIGEN_AMD_VAE_H
#define GLIGEN_AMD_VAE_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* AttnBlock (reference model.py:177-202) is one head over the h * w tokens of the latent grid with the whole channel count C as its
 * head dimension: o = softmax(q k^T C^-0.5) v. Two forms compute it:
 *   matrix  per image a GEMM into an fp32 score matrix [T][T], a row softmax into a bf16 matrix [T][T] and a second GEMM: 6 T^2 bytes
 *           of the context's arena per image (100 MB at T = 4096, 1.6 GB at 16384);
 *   flash   vae_attn_flash_kernel, C = 256 or 512: online softmax over 64-key tiles, nothing that grows with T^2.
 * mode: GL_VAE_ATTN_AUTO (default) = the matrix form up to 4096 tokens -- every launch and every bit of a decode or encode at that size
 * stay what they were -- and the flash form above that, and also below wherever C is 256 or 512 and the score matrices do not fit what
 * is left of the arena; GL_VAE_ATTN_MATRIX = always the matrix form (never replaced: a size that does not fit fails with the arena's
 * message); GL_VAE_ATTN_FLASH = always the flash form, GL_ERR_UNSUPPORTED naming C where the kernel has no instantiation. Per context
 * (a fork starts with its parent's mode); takes effect with the next gl_vae_decode / gl_vae_encode. */
enum { GL_VAE_ATTN_AUTO = 0, GL_VAE_ATTN_MATRIX = 1, GL_VAE_ATTN_FLASH = 2 };
int gl_vae_set_attention(gl_ctx* ctx, int mode);

/* The operator on the caller's device buffers: q, k, v and out are bf16 rows [B][T][C] (v row-major at this boundary; the call
 * transposes it into the context's arena, 2 B T C bytes), 16-byte aligned, T and C multiples of 64. mode as above, for this call only
 * (the context's mode is neither read nor changed). out[b][t][:] = softmax_t'(q[b][t] . k[b][t'] C^-0.5) v[b][t'][:], fp32
 * accumulation, P and out rounded to bf16. */
int gl_op_vae_attention(gl_ctx* ctx, const void* q, const void* k, const void* v, int B, int T, int C, int mode, void* out, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
