// Single-head flash attention of the VAE's AttnBlock (reference model.py:177-202) at head dimension 256 and 512: no buffer grows with
// the square of the token count. The score-matrix form it stands beside is Engine::vae_attn_matrix (engine_vae.hip).
#pragma once
#include "common.h"

namespace gl {

constexpr int kVaeAttnKeyTile = 64;   // keys per tile of the online softmax; T must be a multiple

inline bool vae_attn_flash_supports(int C) { return C == 256 || C == 512; }

// o[b][t][:] = softmax(q_b k_b^T C^-0.5) v_b (+ vbias): q, k, o bf16 rows [B][T][C], vt = v^T bf16 [B][C][T], vbias fp32 [C] or null
// (added behind the product: the rows of the softmax sum to 1). T % 64 == 0, C in {256, 512}, every pointer 16-byte aligned.
int vae_attn_flash_launch(const bf16* q, const bf16* k, const bf16* vt, const float* vbias, bf16* o, int B, int T, int C, hipStream_t stream);
// vt[b][c][t] = v[b][t][c] (bf16; T % 64 == 0, C % 64 == 0)
int vae_attn_transpose_launch(const bf16* v, bf16* vt, int B, int T, int C, hipStream_t stream);

}  // namespace gl
