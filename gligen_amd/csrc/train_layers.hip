// The UNet's layer kinds in training, for gfx950: forward + backward of a BasicTransformerBlock with a gatedSA / gatedSA2 / gatedCA fuser,
// of the SpatialTransformer around it, of a ResBlock and of the resampling convs, each also as a slice entry point under the
// reference's loss (train.h).
//
// Reference: ldm/modules/attention.py:333-338 (BasicTransformerBlock._forward), :236-244 (GatedSelfAttentionDense.forward),
// :127-186 (CrossAttention / SelfAttention), :37-64 (GEGLU / FeedForward); trainer.py:353-371 (run_one_step: mse_loss(model_output,
// noise)), :217-245 (what is trainable: fuser.*, position_net, downsample_net), :375-392 (loss.backward(); opt.step()).
// Gradients are produced for the fuser.* parameters only (weight gradients of the frozen SD layers are never formed --
// trainer.py:217-245 leaves them out of the optimizer), for the block's input and for the grounding tokens, so the step chains into
// position_net and the blocks in front of this one. Held to gradients of the reference's own autograd (tests/golden/).
#include "train_impl.h"

#include "train_fusers.h"

namespace gl {

using namespace train;

namespace {

// out[b][p][c] = a[b][p][c] + e[b][c]   (h + emb_out[..., None, None], openaimodel.py:230)
__global__ void add_per_sample_kernel(const float* __restrict__ a, const float* __restrict__ e, int HW, int Cc, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = a[i] + e[(i / ((size_t)HW * Cc)) * Cc + i % Cc];
}
// Downsample backward: z [B][H][W][C] = dy [B][H/2][W/2][C] at the even positions, zeros elsewhere (the transposed stride-2 conv is
// the stride-1 conv of this with the flipped filter). Upsample backward: dx [B][H][W][C] = 2 x 2 block sums of du [B][2H][2W][C]
// (the adjoint of nearest-neighbour doubling).
__global__ void zero_insert2_kernel(const float* __restrict__ dy, int H, int W, int Cc, size_t n, float* __restrict__ z) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Cc), xw = (int)((i / Cc) % W), yh = (int)((i / ((size_t)Cc * W)) % H);
    const size_t b = i / ((size_t)Cc * W * H);
    z[i] = ((xw | yh) & 1) ? 0.f : dy[((b * (H / 2) + yh / 2) * (W / 2) + xw / 2) * Cc + c];
}
__global__ void sum2x2_kernel(const float* __restrict__ du, int H, int W, int Cc, size_t n, float* __restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Cc), xw = (int)((i / Cc) % W), yh = (int)((i / ((size_t)Cc * W)) % H);
    const size_t b = i / ((size_t)Cc * W * H);
    const float* p = du + ((b * 2 * H + 2 * yh) * 2 * W + 2 * xw) * Cc + c;
    dx[i] = (p[0] + p[Cc]) + (p[(size_t)2 * W * Cc] + p[(size_t)2 * W * Cc + Cc]);
}

}  // namespace

// The frame of the four slice entry points: forward (writes y [n]), loss = mse_loss(y, target) and its gradient g, backward
// (g -> dL/dx [n_dx], returned), dx copied out
template <class Fwd, class Bwd>
static int with_mse_loss(Arena& ar, float* ws, size_t ws_bytes, hipStream_t s, const float* y, const float* target, size_t n, float* loss, float* dx, size_t n_dx,
                  Fwd&& forward, Bwd&& backward) {
    try {
        Ctx c{ar, ws, ws_bytes, s};
        forward(c);
        float* g = c.mse_loss(y, target, n, loss);
        const float* gx = backward(c, g);
        c.hip(hipMemcpyAsync(dx, gx, n_dx * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
        c.hip(hipGetLastError(), "training slice kernel launch");
    } catch (const GlError& e) {
        return set_error(e.code, "%s", e.what());
    }
    return GL_OK;
}

// y = BasicTransformerBlock(x, context, objs) (attention.py:333-338), everything the backward needs kept in the arena
static BlockSaved block_forward(const Ctx& c, const TrainBlockDims& d, const float* const* P, const float* x, const float* objs, const float* context, float* y) {
    const int B = d.B, N = d.N, Ng = d.Ng, C = d.C, H = d.heads, D = C / H, T = N + Ng, M = B * N, MT = B * T, MC = B * d.ctx_T, KD = d.ctx_dim;
    const size_t nx = (size_t)M * C;
    BlockSaved S;
    // x1 = attn1(norm1(x)) + x
    S.n1 = c.ln_fwd(x, M, C, P[TP_NORM1_W], P[TP_NORM1_B]);
    S.q1 = c.lin_fwd(S.n1.y, M, C, P[TP_A1_Q], nullptr, C);
    S.k1 = c.lin_fwd(S.n1.y, M, C, P[TP_A1_K], nullptr, C);
    S.v1 = c.lin_fwd(S.n1.y, M, C, P[TP_A1_V], nullptr, C);
    if (c.lora) {       // the adapters of the frozen SD Linears (train_lora.hip): each adds its low-rank term to the product in place
        lora_fwd(c, P[TP_A1_Q], S.n1.y, M, C, C, S.q1);
        lora_fwd(c, P[TP_A1_K], S.n1.y, M, C, C, S.k1);
        lora_fwd(c, P[TP_A1_V], S.n1.y, M, C, C, S.v1);
    }
    S.a1 = c.attn_fwd(D, S.q1, S.k1, S.v1, B, H, N, N);
    float* o1 = c.lin_fwd(S.a1.o, M, C, P[TP_A1_O], P[TP_A1_OB], C);
    if (c.lora) lora_fwd(c, P[TP_A1_O], S.a1.o, M, C, C, o1);
    float* x1 = c.gated_add(x, o1, nullptr, 1.f, nx);
    if (d.fuser_kind == 2) {
        // fuser (gatedCA, attention.py:207-212): x2 = x1 + scale tanh(alpha_attn) attn(norm1(x1), objs, objs): no fuser.linear, to_k / to_v read objs
        S.nf1 = c.ln_fwd(x1, M, C, P[TP_F_N1_W], P[TP_F_N1_B]);
        S.qf = c.lin_fwd(S.nf1.y, M, C, P[TP_F_Q], nullptr, C);
        S.kf = c.lin_fwd(objs, B * Ng, KD, P[TP_F_K], nullptr, C);
        S.vf = c.lin_fwd(objs, B * Ng, KD, P[TP_F_V], nullptr, C);
        S.af = c.attn_fwd(D, S.qf, S.kf, S.vf, B, H, N, Ng);
        S.af_vis = S.af.o;
        S.of = c.lin_fwd(S.af_vis, M, C, P[TP_F_O], P[TP_F_OB], C);
    } else {
        // fuser (gatedSA, attention.py:236-244): x2 = x1 + scale tanh(alpha_attn) attn(norm1([x1 ; linear(objs)]))[:, :N]
        float* ol = c.lin_fwd(objs, B * Ng, KD, P[TP_F_LIN_W], P[TP_F_LIN_B], C);
        float* cat = c.f32((size_t)MT * C);
        c.put_rows(cat, B, T, 0, x1, N, C);
        c.put_rows(cat, B, T, N, ol, Ng, C);
        S.nf1 = c.ln_fwd(cat, MT, C, P[TP_F_N1_W], P[TP_F_N1_B]);
        if (d.fuser_kind == 0) {
            S.qf = c.lin_fwd(S.nf1.y, MT, C, P[TP_F_Q], nullptr, C);
            S.kf = c.lin_fwd(S.nf1.y, MT, C, P[TP_F_K], nullptr, C);
            S.vf = c.lin_fwd(S.nf1.y, MT, C, P[TP_F_V], nullptr, C);
            S.af = c.attn_fwd(D, S.qf, S.kf, S.vf, B, H, T, T);
            S.af_vis = c.slice_rows(S.af.o, B, T, 0, N, C);
            S.of = c.lin_fwd(S.af_vis, M, C, P[TP_F_O], P[TP_F_OB], C);
        } else {
            // gatedSA2 (attention.py:272-297): [:, N:] keeps the grounding tokens' outputs only, so only those Ng rows are queries; their
            // projected outputs, an sg x sg grid, are resized to the sv x sv visual grid (bicubic) and that is the gated residual
            const int sg = isqrt_exact(Ng), sv = isqrt_exact(N);
            S.nf1_tail = c.slice_rows(S.nf1.y, B, T, N, Ng, C);
            S.qf = c.lin_fwd(S.nf1_tail, B * Ng, C, P[TP_F_Q], nullptr, C);
            S.kf = c.lin_fwd(S.nf1.y, MT, C, P[TP_F_K], nullptr, C);
            S.vf = c.lin_fwd(S.nf1.y, MT, C, P[TP_F_V], nullptr, C);
            S.af = c.attn_fwd(D, S.qf, S.kf, S.vf, B, H, Ng, T);
            S.af_vis = S.af.o;
            float* og = c.lin_fwd(S.af_vis, B * Ng, C, P[TP_F_O], P[TP_F_OB], C);
            S.of = c.f32(nx);
            c.ck(grid_resize_fwd_launch(og, B, sg, sv, C, S.of, c.s));
        }
    }
    float* x2 = c.gated_add(x1, S.of, P[TP_F_ALPHA_ATTN], d.fuser_scale, nx);
    //        x3 = x2 + scale tanh(alpha_dense) ff(norm2(x2))
    S.nf2 = c.ln_fwd(x2, M, C, P[TP_F_N2_W], P[TP_F_N2_B]);
    S.uf = c.lin_fwd(S.nf2.y, M, C, P[TP_F_FF1_W], P[TP_F_FF1_B], 8 * C);
    S.hf = c.geglu_fwd(S.uf, M, 4 * C);
    S.ff_f = c.lin_fwd(S.hf, M, 4 * C, P[TP_F_FF2_W], P[TP_F_FF2_B], C);
    float* x3 = c.gated_add(x2, S.ff_f, P[TP_F_ALPHA_DENSE], d.fuser_scale, nx);
    // x4 = attn2(norm2(x3), context) + x3
    S.n2 = c.ln_fwd(x3, M, C, P[TP_NORM2_W], P[TP_NORM2_B]);
    S.q2 = c.lin_fwd(S.n2.y, M, C, P[TP_A2_Q], nullptr, C);
    S.k2 = c.lin_fwd(context, MC, KD, P[TP_A2_K], nullptr, C);
    S.v2 = c.lin_fwd(context, MC, KD, P[TP_A2_V], nullptr, C);
    if (c.lora) {
        lora_fwd(c, P[TP_A2_Q], S.n2.y, M, C, C, S.q2);
        lora_fwd(c, P[TP_A2_K], context, MC, KD, C, S.k2);
        lora_fwd(c, P[TP_A2_V], context, MC, KD, C, S.v2);
    }
    S.a2 = c.attn_fwd(D, S.q2, S.k2, S.v2, B, H, N, d.ctx_T);
    float* o2 = c.lin_fwd(S.a2.o, M, C, P[TP_A2_O], P[TP_A2_OB], C);
    if (c.lora) lora_fwd(c, P[TP_A2_O], S.a2.o, M, C, C, o2);
    float* x4 = c.gated_add(x3, o2, nullptr, 1.f, nx);
    // y = ff(norm3(x4)) + x4
    S.n3 = c.ln_fwd(x4, M, C, P[TP_NORM3_W], P[TP_NORM3_B]);
    S.u3 = c.lin_fwd(S.n3.y, M, C, P[TP_FF1_W], P[TP_FF1_B], 8 * C);
    if (c.lora) lora_fwd(c, P[TP_FF1_W], S.n3.y, M, C, 8 * C, S.u3);
    float* h3 = c.geglu_fwd(S.u3, M, 4 * C);
    float* ff3 = c.lin_fwd(h3, M, 4 * C, P[TP_FF2_W], P[TP_FF2_B], C);
    if (c.lora) lora_fwd(c, P[TP_FF2_W], h3, M, 4 * C, C, ff3);
    c.gated_add(x4, ff3, nullptr, 1.f, nx, y);
    return S;
}

// g: dL/dy on entry, dL/dx on return (the running gradient of the residual stream). dobjs and G[slot] (fuser.* only) are written.
static void block_backward(const Ctx& c, const TrainBlockDims& d, const float* const* P, const BlockSaved& S, const float* objs, float* g, float* dobjs, float* const* G,
                           const float* context = nullptr) {
    hipStream_t s = c.s;
    const int B = d.B, N = d.N, Ng = d.Ng, C = d.C, H = d.heads, D = C / H, T = N + Ng, M = B * N, MT = B * T, KD = d.ctx_dim;
    const size_t nx = (size_t)M * C;
    {   // y = x4 + ff(norm3(x4)): frozen weights, data gradients only
        float* g_h3 = c.lin_dgrad(g, M, C, P[TP_FF2_W], 4 * C);
        if (lora_find(c, P[TP_FF2_W])) lora_bwd(c, P[TP_FF2_W], g, c.geglu_fwd(S.u3, M, 4 * C), M, 4 * C, C, g_h3);     // (ff.net.2's input is not kept)
        float* g_u3 = c.geglu_bwd(g_h3, S.u3, M, 4 * C);
        float* g_n3 = c.lin_dgrad(g_u3, M, 8 * C, P[TP_FF1_W], C);
        if (c.lora) lora_bwd(c, P[TP_FF1_W], g_u3, S.n3.y, M, C, 8 * C, g_n3);
        c.ln_bwd(g_n3, S.n3, P[TP_NORM3_W], M, C, g, true, nullptr, nullptr);
    }
    {   // x4 = x3 + attn2(norm2(x3), context): the context comes from the frozen text encoder, no dK / dV
        float* g_a2 = c.lin_dgrad(g, M, C, P[TP_A2_O], C);
        if (c.lora) lora_bwd(c, P[TP_A2_O], g, S.a2.o, M, C, C, g_a2);
        float* g_q2 = c.f32(nx);
        // adapters on to_k / to_v need dK / dV for their own gradients (weight gradients only: the context still has none)
        const bool kv = lora_find(c, P[TP_A2_K]) || lora_find(c, P[TP_A2_V]);
        const int MC = B * d.ctx_T;
        float* g_k2 = kv ? c.f32((size_t)MC * C) : nullptr;
        float* g_v2 = kv ? c.f32((size_t)MC * C) : nullptr;
        c.attn_bwd(D, S.q2, S.k2, S.v2, S.a2, g_a2, B, H, N, d.ctx_T, g_q2, g_k2, g_v2);
        if (kv) {
            lora_bwd(c, P[TP_A2_K], g_k2, context, MC, KD, C, nullptr);
            lora_bwd(c, P[TP_A2_V], g_v2, context, MC, KD, C, nullptr);
        }
        float* g_n2 = c.lin_dgrad(g_q2, M, C, P[TP_A2_Q], C);
        if (c.lora) lora_bwd(c, P[TP_A2_Q], g_q2, S.n2.y, M, C, C, g_n2);
        c.ln_bwd(g_n2, S.n2, P[TP_NORM2_W], M, C, g, true, nullptr, nullptr);
    }
    {   // x3 = x2 + g_d ff(norm2(x2)), g_d = scale tanh(alpha_dense): the fuser's feed-forward, TRAINABLE
        if (G[TP_F_ALPHA_DENSE]) c.dot_reduce(g, S.ff_f, nx, P[TP_F_ALPHA_DENSE], d.fuser_scale, 0, G[TP_F_ALPHA_DENSE]);
        float* g_ff = c.gated_scale(g, P[TP_F_ALPHA_DENSE], d.fuser_scale, nx);
        c.lin_wgrad(g_ff, S.hf, M, C, 4 * C, G[TP_F_FF2_W], G[TP_F_FF2_B]);
        float* g_hf = c.lin_dgrad(g_ff, M, C, P[TP_F_FF2_W], 4 * C);
        float* g_uf = c.geglu_bwd(g_hf, S.uf, M, 4 * C);
        c.lin_wgrad(g_uf, S.nf2.y, M, 8 * C, C, G[TP_F_FF1_W], G[TP_F_FF1_B]);
        float* g_nf2 = c.lin_dgrad(g_uf, M, 8 * C, P[TP_F_FF1_W], C);
        c.ln_bwd(g_nf2, S.nf2, P[TP_F_N2_W], M, C, g, true, G[TP_F_N2_W], G[TP_F_N2_B]);
    }
    if (d.fuser_kind == 2) {   // x2 = x1 + g_a attn(norm1(x1), objs, objs): the gatedCA fuser's attention, TRAINABLE; keys and values from the raw tokens
        if (G[TP_F_ALPHA_ATTN]) c.dot_reduce(g, S.of, nx, P[TP_F_ALPHA_ATTN], d.fuser_scale, 0, G[TP_F_ALPHA_ATTN]);
        float* g_of = c.gated_scale(g, P[TP_F_ALPHA_ATTN], d.fuser_scale, nx);
        c.lin_wgrad(g_of, S.af_vis, M, C, C, G[TP_F_O], G[TP_F_OB]);
        float* g_af = c.lin_dgrad(g_of, M, C, P[TP_F_O], C);
        float* g_qf = c.f32(nx);
        float* g_kf = c.f32((size_t)B * Ng * C);
        float* g_vf = c.f32((size_t)B * Ng * C);
        c.attn_bwd(D, S.qf, S.kf, S.vf, S.af, g_af, B, H, N, Ng, g_qf, g_kf, g_vf);
        c.lin_wgrad(g_qf, S.nf1.y, M, C, C, G[TP_F_Q], nullptr);
        c.lin_wgrad(g_kf, objs, B * Ng, C, KD, G[TP_F_K], nullptr);
        c.lin_wgrad(g_vf, objs, B * Ng, C, KD, G[TP_F_V], nullptr);
        float* g_objs = c.lin_dgrad(g_kf, B * Ng, C, P[TP_F_K], KD);
        c.add(g_objs, c.lin_dgrad(g_vf, B * Ng, C, P[TP_F_V], KD), (size_t)B * Ng * KD);
        c.hip(hipMemcpyAsync(dobjs, g_objs, (size_t)B * Ng * KD * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
        float* g_nf1 = c.lin_dgrad(g_qf, M, C, P[TP_F_Q], C);
        c.ln_bwd(g_nf1, S.nf1, P[TP_F_N1_W], M, C, g, true, G[TP_F_N1_W], G[TP_F_N1_B]);
    } else {   // x2 = x1 + g_a attn(norm1([x1 ; linear(objs)]))[:, :N] (gatedSA2: resize(...[:, N:])): the fuser's attention, TRAINABLE
        if (G[TP_F_ALPHA_ATTN]) c.dot_reduce(g, S.of, nx, P[TP_F_ALPHA_ATTN], d.fuser_scale, 0, G[TP_F_ALPHA_ATTN]);
        float* g_of = c.gated_scale(g, P[TP_F_ALPHA_ATTN], d.fuser_scale, nx);
        float* g_nf1 = nullptr;     // dL/d norm1([x1 ; linear(objs)]) [MT][C]
        if (d.fuser_kind == 0) {
            c.lin_wgrad(g_of, S.af_vis, M, C, C, G[TP_F_O], G[TP_F_OB]);
            float* g_af_vis = c.lin_dgrad(g_of, M, C, P[TP_F_O], C);
            float* g_af = c.f32((size_t)MT * C);      // the grounding-token rows of the attention output are dropped by [:, :N]: zero gradient
            c.hip(hipMemsetAsync(g_af, 0, (size_t)MT * C * 4, s), "hipMemsetAsync");
            c.put_rows(g_af, B, T, 0, g_af_vis, N, C);
            float* g_qf = c.f32((size_t)MT * C);
            float* g_kf = c.f32((size_t)MT * C);
            float* g_vf = c.f32((size_t)MT * C);
            c.attn_bwd(D, S.qf, S.kf, S.vf, S.af, g_af, B, H, T, T, g_qf, g_kf, g_vf);
            c.lin_wgrad(g_qf, S.nf1.y, MT, C, C, G[TP_F_Q], nullptr);
            c.lin_wgrad(g_kf, S.nf1.y, MT, C, C, G[TP_F_K], nullptr);
            c.lin_wgrad(g_vf, S.nf1.y, MT, C, C, G[TP_F_V], nullptr);
            g_nf1 = c.lin_dgrad(g_qf, MT, C, P[TP_F_Q], C);
            c.add(g_nf1, c.lin_dgrad(g_kf, MT, C, P[TP_F_K], C), (size_t)MT * C);
            c.add(g_nf1, c.lin_dgrad(g_vf, MT, C, P[TP_F_V], C), (size_t)MT * C);
        } else {
            // the visual rows of the attention output are dropped by [:, N:]: only the Ng grounding rows are queries and carry gradient
            const int sg = isqrt_exact(Ng), sv = isqrt_exact(N), MG = B * Ng;
            float* g_og = c.f32((size_t)MG * C);
            c.ck(grid_resize_bwd_launch(g_of, B, sg, sv, C, g_og, s));
            c.lin_wgrad(g_og, S.af_vis, MG, C, C, G[TP_F_O], G[TP_F_OB]);
            float* g_af = c.lin_dgrad(g_og, MG, C, P[TP_F_O], C);
            float* g_qf = c.f32((size_t)MG * C);
            float* g_kf = c.f32((size_t)MT * C);
            float* g_vf = c.f32((size_t)MT * C);
            c.attn_bwd(D, S.qf, S.kf, S.vf, S.af, g_af, B, H, Ng, T, g_qf, g_kf, g_vf);
            c.lin_wgrad(g_qf, S.nf1_tail, MG, C, C, G[TP_F_Q], nullptr);
            c.lin_wgrad(g_kf, S.nf1.y, MT, C, C, G[TP_F_K], nullptr);
            c.lin_wgrad(g_vf, S.nf1.y, MT, C, C, G[TP_F_V], nullptr);
            g_nf1 = c.lin_dgrad(g_kf, MT, C, P[TP_F_K], C);
            c.add(g_nf1, c.lin_dgrad(g_vf, MT, C, P[TP_F_V], C), (size_t)MT * C);
            float* g_tail = c.slice_rows(g_nf1, B, T, N, Ng, C);      // to_q read rows [N, T) only
            c.add(g_tail, c.lin_dgrad(g_qf, MG, C, P[TP_F_Q], C), (size_t)MG * C);
            c.put_rows(g_nf1, B, T, N, g_tail, Ng, C);
        }
        float* g_cat = c.f32((size_t)MT * C);
        c.ln_bwd(g_nf1, S.nf1, P[TP_F_N1_W], MT, C, g_cat, false, G[TP_F_N1_W], G[TP_F_N1_B]);
        c.add(g, c.slice_rows(g_cat, B, T, 0, N, C), nx);
        float* g_ol = c.slice_rows(g_cat, B, T, N, Ng, C);
        c.lin_wgrad(g_ol, objs, B * Ng, C, KD, G[TP_F_LIN_W], G[TP_F_LIN_B]);
        float* g_objs = c.lin_dgrad(g_ol, B * Ng, C, P[TP_F_LIN_W], KD);
        c.hip(hipMemcpyAsync(dobjs, g_objs, (size_t)B * Ng * KD * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
    }
    {   // x1 = x + attn1(norm1(x)): frozen
        float* g_a1 = c.lin_dgrad(g, M, C, P[TP_A1_O], C);
        if (c.lora) lora_bwd(c, P[TP_A1_O], g, S.a1.o, M, C, C, g_a1);
        float* g_q1 = c.f32(nx);
        float* g_k1 = c.f32(nx);
        float* g_v1 = c.f32(nx);
        c.attn_bwd(D, S.q1, S.k1, S.v1, S.a1, g_a1, B, H, N, N, g_q1, g_k1, g_v1);
        float* g_n1 = c.lin_dgrad(g_q1, M, C, P[TP_A1_Q], C);
        c.add(g_n1, c.lin_dgrad(g_k1, M, C, P[TP_A1_K], C), nx);
        c.add(g_n1, c.lin_dgrad(g_v1, M, C, P[TP_A1_V], C), nx);
        if (c.lora) {
            lora_bwd(c, P[TP_A1_Q], g_q1, S.n1.y, M, C, C, g_n1);
            lora_bwd(c, P[TP_A1_K], g_k1, S.n1.y, M, C, C, g_n1);
            lora_bwd(c, P[TP_A1_V], g_v1, S.n1.y, M, C, C, g_n1);
        }
        c.ln_bwd(g_n1, S.n1, P[TP_NORM1_W], M, C, g, true, nullptr, nullptr);
    }
}

// G (optional): the gradient slots, checked against the kind's key set
static void block_check(const TrainBlockDims& d, const float* const* P, float* const* G = nullptr) {
    if (d.C % 64 || d.ctx_dim % 64 || d.C % d.heads || d.B < 1 || d.N < 1 || d.Ng < 1) throw GlError(GL_ERR_ARG, "block_train_step: C and ctx_dim must be multiples of 64");
    if (d.fuser_kind < 0 || d.fuser_kind > 2) throw GlError(GL_ERR_ARG, fmt("block_train_step: fuser_kind %d (0 gatedSA, 1 gatedSA2, 2 gatedCA)", d.fuser_kind));
    if (d.fuser_kind == 1 && !isqrt_exact(d.Ng))
        throw GlError(GL_ERR_ARG, fmt("block_train_step: gatedSA2 needs a square number of grounding tokens (attention.py:281-283); Ng = %d", d.Ng));
    if (d.fuser_kind == 1 && !isqrt_exact(d.N))
        throw GlError(GL_ERR_ARG, fmt("block_train_step: gatedSA2 needs a square grid of visual tokens (attention.py:280-282); N = %d", d.N));
    for (int i = 0; i < TP_COUNT; ++i) {
        const bool absent = d.fuser_kind == 2 && (i == TP_F_LIN_W || i == TP_F_LIN_B);      // GatedCrossAttentionDense has no linear
        if (absent && (P[i] || (G && G[i])))
            throw GlError(GL_ERR_ARG, fmt("block_train_step: a gatedCA fuser has no fuser.linear.%s (parameter slot %d must be null in params and grads)",
                                          i == TP_F_LIN_W ? "weight" : "bias", i));
        if (!absent && !P[i]) throw GlError(GL_ERR_ARG, fmt("block_train_step: parameter slot %d is null", i));
    }
}

int block_train_step(Arena& ar, float* ws, size_t ws_bytes, const TrainBlockDims& d, const float* const* P, const float* x, const float* objs,
                     const float* context, const float* target, float* y, float* loss, float* dx, float* dobjs, float* const* G, hipStream_t s) {
    const size_t nx = (size_t)d.B * d.N * d.C;
    BlockSaved S;
    return with_mse_loss(
        ar, ws, ws_bytes, s, y, target, nx, loss, dx, nx, [&](const Ctx& c) { block_check(d, P, G); S = block_forward(c, d, P, x, objs, context, y); },
        [&](const Ctx& c, float* g) { block_backward(c, d, P, S, objs, g, dobjs, G); return g; });
}

// SpatialTransformer.forward (attention.py:366-376) around one BasicTransformerBlock: x + proj_out(block(proj_in(norm(x)))), norm =
// GroupNorm(32, eps 1e-6) without activation, proj_in / proj_out 1 x 1 convs = Linears over pixel rows. norm / proj_* are SD layers
// (frozen); gradients: the block's fuser.* parameters, dx, dobjs. P / G: [norm.w, norm.b, proj_in.w, proj_in.b, <37 block slots>,
// proj_out.w, proj_out.b].
void train::st_check(const TrainBlockDims& d, const float* const* P, float* const* G) {
    for (int i = 0; i < ST_COUNT; ++i)
        if (!P[i] && (i < ST_BLOCK0 || i >= ST_BLOCK0 + TP_COUNT)) throw GlError(GL_ERR_ARG, fmt("st_train_step: parameter slot %d is null", i));
    block_check(d, P + ST_BLOCK0, G ? G + ST_BLOCK0 : nullptr);
}
STSaved train::st_forward(const Ctx& c, const TrainBlockDims& d, const float* const* P, const float* x, const float* objs, const float* context, float* y) {
    const int B = d.B, N = d.N, C = d.C, M = B * N;
    const size_t nx = (size_t)M * C;
    STSaved S;
    S.n0 = c.gn_silu_fwd(x, B, N, C, P[ST_NORM_W], P[ST_NORM_B], false, 1e-6f);
    float* t0 = c.lin_fwd(S.n0.a, M, C, P[ST_PIN_W], P[ST_PIN_B], C);
    if (c.lora) lora_fwd(c, P[ST_PIN_W], S.n0.a, M, C, C, t0);
    float* yb = c.f32(nx);
    S.blk = block_forward(c, d, P + ST_BLOCK0, t0, objs, context, yb);
    S.yb = yb;
    float* po = c.lin_fwd(yb, M, C, P[ST_POUT_W], P[ST_POUT_B], C);
    if (c.lora) lora_fwd(c, P[ST_POUT_W], yb, M, C, C, po);
    c.gated_add(x, po, nullptr, 1.f, nx, y);
    return S;
}
void train::st_backward(const Ctx& c, const TrainBlockDims& d, const float* const* P, const STSaved& S, const float* objs, float* g, float* dobjs, float* const* G,
                        const float* context) {
    const int B = d.B, N = d.N, C = d.C, M = B * N;
    if (c.lora && !context && (lora_find(c, P[ST_BLOCK0 + TP_A2_K]) || lora_find(c, P[ST_BLOCK0 + TP_A2_V])))
        throw GlError(GL_ERR_ARG, "st_backward: an adapter on attn2.to_k / to_v needs the context in the backward");
    float* g_b = c.lin_dgrad(g, M, C, P[ST_POUT_W], C);                              // through proj_out
    if (c.lora) lora_bwd(c, P[ST_POUT_W], g, S.yb, M, C, C, g_b);
    block_backward(c, d, P + ST_BLOCK0, S.blk, objs, g_b, dobjs, G + ST_BLOCK0, context);     // g_b: dL/d(block output) -> dL/d(block input)
    float* g_a = c.lin_dgrad(g_b, M, C, P[ST_PIN_W], C);                             // through proj_in
    if (c.lora) lora_bwd(c, P[ST_PIN_W], g_b, S.n0.a, M, C, C, g_a);
    c.gn_silu_bwd(g_a, S.n0, P[ST_NORM_W], P[ST_NORM_B], B, N, C, g, true, false);   // + the residual x_in: g already holds dL/dy
}

int st_train_step(Arena& ar, float* ws, size_t ws_bytes, const TrainBlockDims& d, const float* const* P, const float* x, const float* objs,
                  const float* context, const float* target, float* y, float* loss, float* dx, float* dobjs, float* const* G, hipStream_t s) {
    const size_t nx = (size_t)d.B * d.N * d.C;
    STSaved S;
    return with_mse_loss(
        ar, ws, ws_bytes, s, y, target, nx, loss, dx, nx, [&](const Ctx& c) { st_check(d, P); S = st_forward(c, d, P, x, objs, context, y); },
        [&](const Ctx& c, float* g) { st_backward(c, d, P, S, objs, g, dobjs, G); return g; });
}

// Forward + backward of one ResBlock (openaimodel.py:154-232, no up / down, no scale-shift norm) under mse_loss(y, target): every
// parameter of it is frozen in the reference's trainer (trainer.py:217-245), so what the training step needs from a ResBlock is the
// gradient w.r.t. its INPUT -- the path by which the loss reaches the fusers in front of it. Rows are pixels ([B][H*W][C], the
// layout of this library; the reference's NCHW is a permutation of it).
void train::res_check(const TrainResDims& d, const float* const* P) {
    if (d.Cin % 64 || d.Cout % 64 || d.emb_dim % 64 || d.B < 1 || d.H < 1 || d.W < 1)
        throw GlError(GL_ERR_ARG, "resblock_train_step: Cin, Cout and emb_dim must be multiples of 64");
    const bool skip_conv = d.Cin != d.Cout;
    for (int i = 0; i < RP_COUNT; ++i)
        if (!P[i] && !(i >= RP_SKIP_W && !skip_conv)) throw GlError(GL_ERR_ARG, fmt("resblock_train_step: parameter slot %d is null", i));
    if (!skip_conv && (P[RP_SKIP_W] || P[RP_SKIP_B])) throw GlError(GL_ERR_ARG, "resblock_train_step: skip_connection is nn.Identity when Cin == Cout");
}
// silu_emb: SiLU(emb) [B][emb_dim] (emb_layers.0, shared by every ResBlock of a step).  h = conv(silu(gn(x))) + emb_layers(emb);
// y = skip(x) + conv(silu(gn(h)))
ResSaved train::res_forward(const Ctx& c, const TrainResDims& d, const float* const* P, const float* x, const float* silu_emb, float* y) {
    const int B = d.B, HW = d.H * d.W, Cin = d.Cin, Cout = d.Cout, M = B * HW;
    const size_t ny = (size_t)M * Cout;
    ResSaved S;
    S.n1 = c.gn_silu_fwd(x, B, HW, Cin, P[RP_GN1_W], P[RP_GN1_B]);
    S.x = x;
    S.silu_emb = silu_emb;
    float* h1 = c.conv3(S.n1.a, B, d.H, d.W, P[RP_C1_W], P[RP_C1_B], Cin, Cout, false);
    float* eo = c.lin_fwd(silu_emb, B, d.emb_dim, P[RP_EMB_W], P[RP_EMB_B], Cout);
    if (c.lora) {       // adapters on the frozen convs and Linears of the ResBlock (train_lora_conv.hip, train_lora.hip): each adds its term in place
        lora_conv_fwd(c, P[RP_C1_W], S.n1.a, B, d.H, d.W, Cin, Cout, 0, h1);
        lora_fwd(c, P[RP_EMB_W], silu_emb, B, d.emb_dim, Cout, eo);
    }
    float* h2 = c.f32(ny);
    c.ew(add_per_sample_kernel, ny, h1, eo, HW, Cout, ny, h2);
    S.n2 = c.gn_silu_fwd(h2, B, HW, Cout, P[RP_GN2_W], P[RP_GN2_B]);
    float* h3 = c.conv3(S.n2.a, B, d.H, d.W, P[RP_C2_W], P[RP_C2_B], Cout, Cout, false);
    if (c.lora) lora_conv_fwd(c, P[RP_C2_W], S.n2.a, B, d.H, d.W, Cout, Cout, 0, h3);
    const float* sk = x;
    if (Cin != Cout) {      // the 1 x 1 conv is a Linear over pixel rows
        float* sp = c.lin_fwd(x, M, Cin, P[RP_SKIP_W], P[RP_SKIP_B], Cout);
        if (c.lora) lora_fwd(c, P[RP_SKIP_W], x, M, Cin, Cout, sp);
        sk = sp;
    }
    c.gated_add(sk, h3, nullptr, 1.f, ny, y);
    return S;
}
float* train::res_backward(const Ctx& c, const TrainResDims& d, const float* const* P, const ResSaved& S, float* g) {
    const int B = d.B, HW = d.H * d.W, Cin = d.Cin, Cout = d.Cout, M = B * HW;
    float* g_a2 = c.conv3(g, B, d.H, d.W, P[RP_C2_W], nullptr, Cout, Cout, true);
    if (c.lora) lora_conv_bwd(c, P[RP_C2_W], g, S.n2.a, B, d.H, d.W, Cout, Cout, 0, g_a2);
    float* g_h2 = c.f32((size_t)M * Cout);
    c.gn_silu_bwd(g_a2, S.n2, P[RP_GN2_W], P[RP_GN2_B], B, HW, Cout, g_h2, false);    // = dL/dh1 (the emb path has nothing trainable upstream)
    float* g_a1 = c.conv3(g_h2, B, d.H, d.W, P[RP_C1_W], nullptr, Cin, Cout, true);
    if (c.lora) {
        lora_conv_bwd(c, P[RP_C1_W], g_h2, S.n1.a, B, d.H, d.W, Cin, Cout, 0, g_a1);
        if (lora_find(c, P[RP_EMB_W])) {      // dL/d(emb_layers output) [B][Cout]: g_h2 summed over each sample's pixels; only the adapter's gradients are formed
            const size_t mk = c.ar.mark();
            float* g_eo = c.f32((size_t)B * Cout);
            lora_sample_colsum(c, g_h2, B, HW, Cout, g_eo);
            lora_bwd(c, P[RP_EMB_W], g_eo, S.silu_emb, B, d.emb_dim, Cout, nullptr);
            c.ar.release(mk);
        }
    }
    float* g_x = Cin != Cout ? c.lin_dgrad(g, M, Cout, P[RP_SKIP_W], Cin) : g;         // through the skip connection
    if (c.lora && Cin != Cout) lora_bwd(c, P[RP_SKIP_W], g, S.x, M, Cin, Cout, g_x);
    c.gn_silu_bwd(g_a1, S.n1, P[RP_GN1_W], P[RP_GN1_B], B, HW, Cin, g_x, true);
    return g_x;
}

int resblock_train_step(Arena& ar, float* ws, size_t ws_bytes, const TrainResDims& d, const float* const* P, const float* x, const float* emb,
                        const float* target, float* y, float* loss, float* dx, hipStream_t s) {
    const size_t rows = (size_t)d.B * d.H * d.W;
    ResSaved S;
    return with_mse_loss(
        ar, ws, ws_bytes, s, y, target, rows * d.Cout, loss, dx, rows * d.Cin,
        [&](const Ctx& c) { res_check(d, P); S = res_forward(c, d, P, x, c.silu(emb, (size_t)d.B * d.emb_dim), y); },
        [&](const Ctx& c, float* g) { return res_backward(c, d, P, S, g); });
}

// Downsample (mode 0: conv3x3 stride 2, openaimodel.py:99-124) / Upsample (mode 1: nearest 2x + conv3x3, openaimodel.py:64-96) of C
// channels; the conv is a frozen SD layer: forward, and the gradient w.r.t. the input.
float* train::resample_forward(const Ctx& c, int mode, int B, int H, int W, int C, const float* w_oihw, const float* bias, const float* x) {
    float* y = c.conv3(x, B, H, W, w_oihw, bias, C, C, false, mode ? 1 : 2, mode ? 1 : 0);
    if (c.lora) lora_conv_fwd(c, w_oihw, x, B, H, W, C, C, mode ? 2 : 1, y);
    return y;
}
float* train::resample_backward(const Ctx& c, int mode, int B, int H, int W, int C, const float* w_oihw, const float* g, const float* x) {
    const size_t nx = (size_t)B * H * W * C;
    float* dx;
    if (mode == 0) {
        float* z = c.f32(nx);
        c.ew(zero_insert2_kernel, nx, g, H, W, C, nx, z);
        dx = c.conv3(z, B, H, W, w_oihw, nullptr, C, C, true);
    } else {
        float* gu = c.conv3(g, B, 2 * H, 2 * W, w_oihw, nullptr, C, C, true);
        dx = c.f32(nx);
        c.ew(sum2x2_kernel, nx, gu, H, W, C, nx, dx);
    }
    // the adapter's data gradient gathers from g on the output grid itself (train_lora_conv.hip): no zero-inserted or enlarged copy
    if (c.lora && lora_find(c, w_oihw)) {
        if (!x) throw GlError(GL_ERR_STATE, "resample_backward: an adapter on the conv needs the layer's input");
        lora_conv_bwd(c, w_oihw, g, x, B, H, W, C, C, mode ? 2 : 1, dx);
    }
    return dx;
}

int resample_train_step(Arena& ar, float* ws, size_t ws_bytes, int mode, int B, int H, int W, int C, const float* w_oihw, const float* bias, const float* x,
                        const float* target, float* y, float* loss, float* dx, hipStream_t s) {
    const int Ho = mode ? 2 * H : H / 2, Wo = mode ? 2 * W : W / 2;
    const size_t ny = (size_t)B * Ho * Wo * C, nx = (size_t)B * H * W * C;
    return with_mse_loss(
        ar, ws, ws_bytes, s, y, target, ny, loss, dx, nx,
        [&](const Ctx& c) {
            if (C % 64 || (mode == 0 && ((H | W) & 1)) || B < 1 || mode < 0 || mode > 1) throw GlError(GL_ERR_ARG, "resample_train_step: C % 64, even H / W for mode 0");
            const float* yv = resample_forward(c, mode, B, H, W, C, w_oihw, bias, x);
            c.hip(hipMemcpyAsync(y, yv, ny * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
        },
        [&](const Ctx& c, float* g) { return resample_backward(c, mode, B, H, W, C, w_oihw, g); });
}

// Ctx::conv3 (geom 0) or resample_forward / resample_backward (geom 1 Downsample, 2 Upsample) by themselves (train.h): the arena
// results copied out
int train_prim_conv3(Arena& ar, float* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout, int geom, const float* x, const float* w_oihw,
                     const float* bias, const float* dy, float* y, float* dx, hipStream_t s) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return set_error(GL_ERR_ARG, "gl_op_train_conv3: B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W, Cin, Cout);
    if (geom < 0 || geom > 2) return set_error(GL_ERR_ARG, "gl_op_train_conv3: geom %d (0 stride 1, 1 Downsample, 2 Upsample)", geom);
    if (Cin % 64 || Cout % 64) return set_error(GL_ERR_ARG, "gl_op_train_conv3: Cin=%d, Cout=%d: multiples of 64 are needed", Cin, Cout);
    if (geom && Cin != Cout) return set_error(GL_ERR_ARG, "gl_op_train_conv3: a resampling layer keeps its channels (Cin=%d, Cout=%d)", Cin, Cout);
    if (geom == 1 && ((H | W) & 1)) return set_error(GL_ERR_ARG, "gl_op_train_conv3: Downsample takes even H and W (%d x %d)", H, W);
    try {
        Ctx c{ar, ws, ws_bytes, s};
        const int Ho = geom == 1 ? H / 2 : geom == 2 ? 2 * H : H, Wo = geom == 1 ? W / 2 : geom == 2 ? 2 * W : W;
        const float* yv = geom ? resample_forward(c, geom - 1, B, H, W, Cin, w_oihw, bias, x) : c.conv3(x, B, H, W, w_oihw, bias, Cin, Cout, false);
        c.hip(hipMemcpyAsync(y, yv, (size_t)B * Ho * Wo * Cout * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
        if (dy && dx) {
            const float* gx = geom ? resample_backward(c, geom - 1, B, H, W, Cin, w_oihw, dy) : c.conv3(dy, B, H, W, w_oihw, nullptr, Cin, Cout, true);
            c.hip(hipMemcpyAsync(dx, gx, (size_t)B * H * W * Cin * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
        }
        c.hip(hipGetLastError(), "training conv kernel launch");
    } catch (const GlError& e) {
        return set_error(e.code, "%s", e.what());
    }
    return GL_OK;
}

}  // namespace gl
