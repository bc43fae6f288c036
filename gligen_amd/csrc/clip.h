// CLIP towers. Text (transformers CLIPTextModel, the reference's FrozenCLIPEmbedder: ldm/modules/encoders/modules.py:144-173): the
// kernels around the bf16 GEMMs -- embedding gather, residual add + LayerNorm on the fp32 residual stream, causal attention at
// head dim 64, EOS-row pooling. The layer schedule is Engine::clip_text_encode (engine_clip.hip).
#pragma once
#include "common.h"

namespace gl {

constexpr int kClipMaxTokens = 96;   // clip_attn_kernel keeps a whole head (three 32-token tiles) in LDS
constexpr int kClipHeadDim = 64;
constexpr int kClipLongMaxTokens = 288; // clip_attn_long_kernel: K and V^T of a head in 77 KB of LDS, two workgroups per CU (ViT-L/14: 257)
constexpr int kClipMaxWidth = 2048;  // clip_add_ln_kernel: one wave per row, at most 8 float4 per lane

// h[row][:] = token_embedding[ids[row]] + position_embedding[row % T] (fp32). An id outside [0, vocab) reads row 0 / vocab - 1
// instead and is counted in *bad (device counter, may be null).
int clip_embed_launch(const int32_t* ids, const float* tok, const float* pos, float* h, int rows, int T, int width, int vocab, unsigned* bad,
                      hipStream_t stream);
// h += delta (delta may be null), then y = LayerNorm(h; gamma, beta): bf16 rows (ybf, the next GEMM's operand) or fp32 rows (yf32)
int clip_add_ln_launch(float* h, const float* delta, const float* gamma, const float* beta, float eps, bf16* ybf, float* yf32, int rows, int width,
                       hipStream_t stream);
// o[s][t][h * 64 ..] = softmax(q k^T / 8 (+ causal mask)) v per (sequence, head); qkv [S * T][3 * heads * 64] bf16 rows = [q | k | v]
// T <= kClipMaxTokens: clip_attn_kernel; kClipMaxTokens < T <= kClipLongMaxTokens, not causal: clip_attn_long_kernel
int clip_attn_launch(const bf16* qkv, bf16* o, int S, int T, int heads, int causal, hipStream_t stream);
// pooled[s][:] = x[s * T + clamp(eos[s], 0, T - 1)][:]
int clip_pool_launch(const float* x, const int32_t* eos, float* pooled, int S, int T, int width, hipStream_t stream);

// ---- vision tower (transformers CLIPVisionModelWithProjection: the image features of reference gligen_inference.py:104-128)
// bf16 patch rows [S * (image_size / patch)^2][Kpad] of fp32 NCHW pixel_values, column (c, ky, kx), zero behind 3 * patch^2
int clip_patch_rows_launch(const float* pixel_values, bf16* out, int S, int image_size, int patch, int Kpad, hipStream_t stream);
// h[s][0] = class_embedding + pos[0], h[s][1 + i] = patch[s * (T - 1) + i] + pos[1 + i] (fp32)
int clip_vision_embed_launch(const float* patch, const float* cls, const float* pos, float* h, int S, int T, int width, hipStream_t stream);
// y[row] = LayerNorm(x[row * in_stride ..] (+ delta, same stride)): fp32 and / or bf16 rows out_stride apart; yf32 may be x (in place)
int clip_ln_rows_launch(const float* x, const float* delta, int64_t in_stride, const float* gamma, const float* beta, float eps, float* yf32, bf16* ybf,
                        int64_t out_stride, int rows, int width, hipStream_t stream);
// out = a + b over n fp32 elements (n % 4 == 0)
int clip_add_launch(const float* a, const float* b, float* out, int64_t n, hipStream_t stream);

}  // namespace gl
