// The whole training iteration of the reference (trainer.py:353-392: model(input) -> mse_loss(model_output, noise) -> backward) for a
// UNetModel with any grounding tokenizer and fuser type (openaimodel.py:237-464), composed of the layer kinds of train_layers.hip:
//   objs = position_net(boxes, masks, positive_embeddings)          text_grounding_net.py:30-52      TRAINABLE
//   emb  = time_embed(timestep_embedding(t))                         openaimodel.py:436-437           frozen, no backward needed
//   input_blocks / middle_block / output_blocks (skip concats) / out openaimodel.py:452-464
// Gradients for every fuser.* parameter of every SpatialTransformer and for position_net.*; nothing else is trainable in the
// reference (trainer.py:217-245), and no input gradient is needed in front of the first fuser. All activations of the forward stay
// in the arena (no recomputation at this size; DESIGN.md section 9 has the checkpointing plan for the full model).
#include "train_impl.h"
#include "train_run.h"

#include <cstring>

namespace gl {

using namespace train;

namespace train {

const float* Names::w(const std::string& k) const {
    auto it = idx.find(k);
    if (it == idx.end() || !params[it->second]) throw GlError(GL_ERR_MISSING, "unet_train_step: missing parameter '" + k + "'");
    return params[it->second];
}
bool Names::has(const std::string& k) const { auto it = idx.find(k); return it != idx.end() && params[it->second]; }
float* Names::g(const std::string& k) const {
    auto it = idx.find(k);
    return it == idx.end() ? nullptr : grads[it->second];
}

}  // namespace train

namespace {

__global__ void timestep_embedding_kernel(const float* __restrict__ t, int dim, float* __restrict__ out) {   // util.py:160-180
    const int b = blockIdx.x, half = dim / 2;
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
        const float a = t[b] * __expf(-9.210340371976184f * (float)i / (float)half);   // ln(10000)
        out[(size_t)b * dim + i] = cosf(a);
        out[(size_t)b * dim + half + i] = sinf(a);
    }
}
// PositionNet input rows (text_grounding_net.py:33-48): [pe * m + (1 - m) * null_positive | fourier(boxes) * m + (1 - m) * null_position],
// fourier = for k in 0..7: sin(f_k x) (4 values), cos(f_k x) (4 values), f_k = 100^(k / 8)   (util.py:12-26)
// (emb_masks: the mask of the embedding half -- `masks` itself for the text tokenizer, text_masks / image_masks for text+image,
// text_image_grounding_net.py:57-59). Keypoint tokenizer (keypoint_grounding_net.py:34-58): pe null, the embedding of token t of a sample
// is person_emb[t / 17] + keypoint_emb[t % 17], coords = 2 (x, y). Columns [D + 16 ncoord, W) are zero padding up to the GEMM's K step.
__global__ void posnet_input_kernel_f32(const float* __restrict__ coords, int ncoord, const float* __restrict__ masks, const float* __restrict__ emb_masks,
                                        const float* __restrict__ pe, const float* __restrict__ person_emb, const float* __restrict__ keypoint_emb, int tokens,
                                        const float* __restrict__ null_pos_feat, const float* __restrict__ null_xyxy, int D, int W, float* __restrict__ out) {
    const int row = blockIdx.x, PD = 16 * ncoord;
    const int t = row % tokens;
    for (int c = threadIdx.x; c < W; c += blockDim.x) {
        float v, nul;
        if (c >= D + PD) { out[(size_t)row * W + c] = 0.f; continue; }
        const float m = c < D ? emb_masks[row] : masks[row];
        if (c < D) {
            v = pe ? pe[(size_t)row * D + c] : person_emb[(size_t)(t / 17) * D + c] + keypoint_emb[(size_t)(t % 17) * D + c];
            nul = null_pos_feat[c];
        } else {
            const int j = c - D, k = j / (2 * ncoord), r = j % (2 * ncoord);
            const float a = powf(100.f, (float)k / 8.f) * coords[(size_t)row * ncoord + (r % ncoord)];
            v = r < ncoord ? sinf(a) : cosf(a);
            nul = null_xyxy[j];
        }
        out[(size_t)row * W + c] = v * m + (1.f - m) * nul;
    }
}
// keypoint tokenizer tables: d person_emb[p][c] = sum_{b, k} m g[b][17 p + k][c] (by = 17, inner = 17), d keypoint_emb[k][c] = sum_{b, p} m g[b][17 p + k][c]
__global__ void table_grad_kernel(const float* __restrict__ g, const float* __restrict__ masks, int B, int tokens, int ld, int D, int person, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
    if (c >= D) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < tokens; ++t)
            if ((person ? t / 17 : t % 17) == e) s += masks[b * tokens + t] * g[((size_t)b * tokens + t) * ld + c];
    out[(size_t)e * D + c] = s;
}
__global__ void concat_kernel(const float* __restrict__ a, int C0, const float* __restrict__ b, int C1, size_t rows, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int C = C0 + C1;
    if (i >= rows * C) return;
    const size_t r = i / C;
    const int c = (int)(i % C);
    out[i] = c < C0 ? a[r * C0 + c] : b[r * C1 + (c - C0)];
}

// one grounding MLP (Linear, SiLU, Linear, SiLU, Linear) and what its backward needs
struct PosBranch { std::string lin, null_emb; const float* emb; const float* emb_mask; float *pcat, *l0, *a0, *l1, *a1, *out, *w0p; };
struct Act { float* p; int C, H, W; };
enum Kind { K_RES, K_ST, K_DOWN, K_UP, K_CAT };
struct UNetLayer {
    Kind kind;
    std::string prefix;
    int Cin, Cout, H, W, C0;                  // K_CAT: C0 = channels of h, Cin - C0 = channels of the skip; skip_idx = its producer
    int skip_idx;
    const float* x_in;                         // the layer's input (kept: with checkpointing the backward recomputes the forward from it)
    std::vector<const float*> P;
    std::vector<float*> G;
    ResSaved rs;
    STSaved ss;
};

// trainer.py:217-242: fuser.*, position_net.*, and for a model with a grounding downsampler downsample_net.* and the first conv's
// weight (input_conv_train, :189-194, 233; its bias stays frozen); an inpainting model's first conv has 5 more input channels and is
// trained the same way (:191-192)
void check_trainable_set(const TrainUNetCfg& cfg, int n_params, const char* const* names, float* const* grads, const TrainSpatialIn* spatial) {
    if (cfg.inpaint_mode && (cfg.grounding_kind == 3 || cfg.extra_channels))
        throw GlError(GL_ERR_UNSUPPORTED, "unet_train_step: inpaint_mode with a spatial-map tokenizer / downsampler channels is undefined in the reference (openaimodel.py:445-446)");
    const bool ds_model = cfg.grounding_kind == 3 && cfg.extra_channels > 0;
    const bool conv_in_train = ds_model || cfg.inpaint_mode;
    for (int i = 0; i < n_params; ++i)
        if (grads[i] && !(strstr(names[i], ".fuser.") || !strncmp(names[i], "position_net.", 13) || (ds_model && !strncmp(names[i], "downsample_net.", 15)) ||
                          (conv_in_train && !strcmp(names[i], "input_blocks.0.0.weight"))))
            throw GlError(GL_ERR_ARG, fmt("unet_train_step: a gradient was asked for '%s', which the reference keeps frozen", names[i]));
    if (cfg.grounding_kind == 3 && !spatial) throw GlError(GL_ERR_ARG, "unet_train_step: a spatial-map model needs its TrainSpatialIn");
    if (spatial && (spatial->map_cls || spatial->extra_cls) &&
        (!spatial->map_cls || !spatial->extra_cls || spatial->map || spatial->extra || !cfg.extra_channels))
        throw GlError(GL_ERR_ARG, "unet_train_step: a mixture of class maps and planes: the tokenizer's map and grounding_extra_input are both u8 class maps "
                                  "or both fp32 planes");
}

// The adapters of a step by the address of their base weight. An adapter is admitted by name: the frozen Linears of a
// SpatialTransformer outside its fuser (the fuser's own Linears train in full), and the frozen convs and Linears of a ResBlock, a
// Downsample and an output block's Upsample (train_lora_conv.hip: down is [r][Ci][3][3] on the 3 x 3 convs, the geometry follows from
// the site); everything check_trainable_set refuses stays refused.
LoraTable lora_table(const Names& nm, const TrainLoraAdapter* adapters, int n_adapters) {
    static const char* const k_sites[] = {".attn1.to_q.weight", ".attn1.to_k.weight", ".attn1.to_v.weight", ".attn1.to_out.0.weight",
                                          ".attn2.to_q.weight", ".attn2.to_k.weight", ".attn2.to_v.weight", ".attn2.to_out.0.weight",
                                          ".ff.net.0.proj.weight", ".ff.net.2.weight", ".proj_in.weight", ".proj_out.weight"};
    static const char* const k_res_sites[] = {".in_layers.2.weight", ".out_layers.3.weight", ".emb_layers.1.weight", ".skip_connection.weight"};
    LoraTable t;
    if (n_adapters < 0 || (n_adapters && !adapters)) throw GlError(GL_ERR_ARG, "unet_train_step: null adapter array");
    for (int i = 0; i < n_adapters; ++i) {
        const TrainLoraAdapter& a = adapters[i];
        if (!a.name || !a.down || !a.up) throw GlError(GL_ERR_ARG, fmt("unet_train_step: adapter %d has a null name, down or up", i));
        const std::string name = a.name;
        auto ends = [&](const char* sfx) {
            const size_t n = strlen(sfx);
            return name.size() > n && !name.compare(name.size() - n, n, sfx);
        };
        auto starts = [&](const char* pfx) { return !name.compare(0, strlen(pfx), pfx); };
        bool site = false;
        for (const char* sfx : k_sites) site = site || ends(sfx);
        const bool in_st = name.find(".transformer_blocks.0.") != std::string::npos || name.find(".proj_") != std::string::npos;
        bool conv_site = (ends(".op.weight") && starts("input_blocks.")) || (ends(".conv.weight") && starts("output_blocks."));
        for (const char* sfx : k_res_sites) conv_site = conv_site || (ends(sfx) && (starts("input_blocks.") || starts("middle_block.") || starts("output_blocks.")));
        conv_site = conv_site && name.find(".transformer_blocks.") == std::string::npos;
        if ((!(site && in_st) && !conv_site) || name.find(".fuser.") != std::string::npos)
            throw GlError(GL_ERR_ARG, "unet_train_step: an adapter was given for '" + name + "': adapters go on attn1 / attn2 to_q, to_k, to_v, to_out.0, "
                                      "ff.net.0.proj, ff.net.2 and proj_in / proj_out of a SpatialTransformer (the fuser's Linears train in full)");
        if (a.rank < 1 || a.rank > 128) throw GlError(GL_ERR_ARG, fmt("unet_train_step: adapter '%s' has rank %d (1 <= r <= 128)", a.name, a.rank));
        if (nm.g(name)) throw GlError(GL_ERR_ARG, "unet_train_step: '" + name + "' has an adapter and a gradient of its own");
        if (!t.emplace(nm.w(name), LoraAdapter{a.down, a.up, a.g_down, a.g_up, a.rank, a.scale}).second)
            throw GlError(GL_ERR_ARG, "unet_train_step: two adapters for '" + name + "'");
    }
    return t;
}

UNetStep step_dims(const Ctx& c, const Names& nm, const TrainUNetCfg& cfg, const TrainUNetIn& in, const TrainSpatialIn* spatial, const char* const* block_names) {
    UNetStep u{c, nm, cfg, in, spatial, block_names};
    u.B = in.B; u.H0 = in.H; u.W0 = in.W; u.mc = cfg.model_channels; u.ED = 4 * u.mc; u.KD = cfg.context_dim; u.Ng = in.Ng;
    if (u.mc % 64 || u.KD % 64 || cfg.gr_dim % 64 || u.B < 1) throw GlError(GL_ERR_ARG, "unet_train_step: model_channels / context_dim / grounding dim must be multiples of 64");
    u.GK = cfg.grounding_kind; u.NB = in.Ng_boxes; u.MRB = u.B * u.NB; u.NC = u.GK == 2 ? 2 : 4;
    u.PWr = u.GK == 3 ? kCnxDims[3] : cfg.gr_dim + 16 * u.NC; u.PW = round_up(u.PWr, 64); u.NBR = u.GK == 1 ? 2 : 1;
    if (u.Ng != u.NB * u.NBR || (u.GK == 2 && u.NB % 17)) throw GlError(GL_ERR_ARG, "unet_train_step: Ng must be the box count (text), twice it (text+image), 17 per person (keypoint)");
    u.MR = u.B * u.Ng;
    if (cfg.fuser_kind < 0 || cfg.fuser_kind > 2) throw GlError(GL_ERR_ARG, fmt("unet_train_step: fuser_kind %d (0 gatedSA, 1 gatedSA2, 2 gatedCA)", cfg.fuser_kind));
    if (cfg.fuser_kind == 1 && !isqrt_exact(u.Ng))
        throw GlError(GL_ERR_ARG, fmt("unet_train_step: gatedSA2 needs a square number of grounding tokens (attention.py:281-283); Ng = %d", u.Ng));
    if (cfg.fuser_kind == 1 && in.H != in.W)
        throw GlError(GL_ERR_ARG, fmt("unet_train_step: gatedSA2 needs a square latent (attention.py:280-282: square visual grids); H = %d, W = %d", in.H, in.W));
    u.null_pos = u.GK == 2 ? "position_net.null_xy_feature" : "position_net.null_position_feature";
    u.Cx = cfg.in_channels; u.Ce = u.GK == 3 ? cfg.extra_channels : 0; u.Ci = cfg.inpaint_mode ? u.Cx + 1 : 0; u.Cin0 = u.Cx + u.Ce + u.Ci;
    u.M0 = (size_t)u.B * u.H0 * u.W0;
    return u;
}

// ---- grounding tokens (trainable): one MLP over [embedding | fourier(coords)] rows for the text tokenizer (boxes, 4 coords) and the
// keypoint tokenizer (points, 2 coords; the embedding is person + keypoint table rows), two MLPs (text, image) whose tokens are
// concatenated along the token axis for text+image (text_grounding_net.py:30-52, text_image_grounding_net.py:41-70,
// keypoint_grounding_net.py:34-58)
// (spatial-map tokenizers, GK 3: the same MLP over the ConvNeXt features mixed with null_feature and pos_embedding, K = 768)
float* grounding_forward(const UNetStep& u, PosBranch pb[2], SpatialSaved& tok) {
    const Ctx& c = u.c;
    const Names& nm = u.nm;
    const TrainUNetIn& in = u.in;
    const int GK = u.GK, MRB = u.MRB, PW = u.PW;
    pb[0] = {GK == 1 ? "position_net.linears_text" : "position_net.linears",
             GK == 1 ? "position_net.null_text_feature" : GK == 2 ? "position_net.null_person_feature" : "position_net.null_positive_feature",
             GK == 2 ? nullptr : in.positive_embeddings, GK == 1 ? in.text_masks : in.masks, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    pb[1] = {"position_net.linears_image", "position_net.null_image_feature", in.image_embeddings, in.image_masks, nullptr, nullptr, nullptr, nullptr, nullptr,
             nullptr, nullptr};
    float* objs = u.NBR == 1 ? nullptr : c.f32((size_t)u.MR * u.KD);
    for (int r = 0; r < u.NBR; ++r) {
        PosBranch& p = pb[r];
        if (GK == 3) {
            tok = spatial_forward(c, nm, u.cfg, *u.spatial, u.B);
            if (tok.M != MRB) throw GlError(GL_ERR_ARG, "unet_train_step: Ng must be (tok_resize / 32)^2 for a spatial-map tokenizer");
            p.pcat = tok.mix;
        } else {
            if ((!p.emb && GK != 2) || !p.emb_mask) throw GlError(GL_ERR_ARG, "unet_train_step: null grounding input");
            p.pcat = c.f32((size_t)MRB * PW);
            hipLaunchKernelGGL(posnet_input_kernel_f32, dim3(MRB), dim3(256), 0, c.s, in.boxes, u.NC, in.masks, p.emb_mask, p.emb,
                               GK == 2 ? nm.w("position_net.person_embeddings") : nullptr, GK == 2 ? nm.w("position_net.keypoint_embeddings") : nullptr, u.NB,
                               nm.w(p.null_emb), nm.w(u.null_pos), u.cfg.gr_dim, PW, p.pcat);
        }
        const float* w0 = nm.w(p.lin + ".0.weight");
        if (PW != u.PWr) w0 = p.w0p = pad_cols(c, w0, 512, u.PWr, PW);     // (the keypoint tokenizer's first Linear has K = 800)
        p.l0 = c.lin_fwd(p.pcat, MRB, PW, w0, nm.w(p.lin + ".0.bias"), 512);
        p.a0 = c.silu(p.l0, (size_t)MRB * 512);
        p.l1 = c.lin_fwd(p.a0, MRB, 512, nm.w(p.lin + ".2.weight"), nm.w(p.lin + ".2.bias"), 512);
        p.a1 = c.silu(p.l1, (size_t)MRB * 512);
        p.out = c.lin_fwd(p.a1, MRB, 512, nm.w(p.lin + ".4.weight"), nm.w(p.lin + ".4.bias"), u.KD);
        if (u.NBR == 1) objs = p.out;
        else c.put_rows(objs, u.B, u.Ng, r * u.NB, p.out, u.NB, u.KD);      // objs = cat([objs_text, objs_image], dim = 1)
    }
    return objs;
}

// position_net backward (the learnable null embeddings: the position one is shared by the branches; the keypoint tokenizer's person /
// keypoint embedding tables; GK 3: token mix + ConvNeXt). g_objs: dL/d objs [B][Ng][KD]
void grounding_backward(const UNetStep& u, const PosBranch pb[2], const SpatialSaved& tok, const float* g_objs) {
    const Ctx& c = u.c;
    const Names& nm = u.nm;
    const int MRB = u.MRB, PW = u.PW, NB = u.NB, gr_dim = u.cfg.gr_dim;
    for (int r = 0; r < u.NBR; ++r) {
        const PosBranch& p = pb[r];
        const float* go = u.NBR == 1 ? g_objs : c.slice_rows(g_objs, u.B, u.Ng, r * NB, NB, u.KD);
        c.lin_wgrad(go, p.a1, MRB, u.KD, 512, nm.g(p.lin + ".4.weight"), nm.g(p.lin + ".4.bias"));
        float* g_a1 = c.lin_dgrad(go, MRB, u.KD, nm.w(p.lin + ".4.weight"), 512);
        float* g_l1 = silu_bwd(c, g_a1, p.l1, (size_t)MRB * 512);
        c.lin_wgrad(g_l1, p.a0, MRB, 512, 512, nm.g(p.lin + ".2.weight"), nm.g(p.lin + ".2.bias"));
        float* g_a0 = c.lin_dgrad(g_l1, MRB, 512, nm.w(p.lin + ".2.weight"), 512);
        float* g_l0 = silu_bwd(c, g_a0, p.l0, (size_t)MRB * 512);
        lin_wgrad_unpad(c, g_l0, p.pcat, MRB, 512, u.PWr, PW, nm.g(p.lin + ".0.weight"), nm.g(p.lin + ".0.bias"));
        float* g_cat = c.lin_dgrad(g_l0, MRB, 512, p.w0p ? p.w0p : nm.w(p.lin + ".0.weight"), PW);
        if (u.GK == 3) {
            spatial_backward(c, nm, u.cfg, *u.spatial, u.B, tok, g_cat);
            continue;
        }
        if (float* gp = nm.g(p.null_emb)) null_grad(c, g_cat, p.emb_mask, MRB, PW, 0, gr_dim, gp, false);
        if (float* gp = nm.g(u.null_pos)) null_grad(c, g_cat, u.in.masks, MRB, PW, gr_dim, 16 * u.NC, gp, r != 0);
        if (u.GK == 2) {
            if (float* gp = nm.g("position_net.person_embeddings"))
                hipLaunchKernelGGL(table_grad_kernel, dim3(cdiv(gr_dim, 256), NB / 17), dim3(256), 0, c.s, g_cat, u.in.masks, u.B, NB, PW, gr_dim, 1, gp);
            if (float* gp = nm.g("position_net.keypoint_embeddings"))
                hipLaunchKernelGGL(table_grad_kernel, dim3(cdiv(gr_dim, 256), 17), dim3(256), 0, c.s, g_cat, u.in.masks, u.B, NB, PW, gr_dim, 0, gp);
        }
    }
}

// time embedding (frozen): silu(emb) [B][ED] is what every ResBlock's emb_layers starts with
float* time_embedding(const UNetStep& u) {
    const Ctx& c = u.c;
    float* te = c.f32((size_t)u.B * u.mc);
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3(u.B), dim3(256), 0, c.s, u.in.timesteps, u.mc, te);
    float* e0 = c.lin_fwd(te, u.B, u.mc, u.nm.w("time_embed.0.weight"), u.nm.w("time_embed.0.bias"), u.ED);
    float* e0s = c.silu(e0, (size_t)u.B * u.ED);
    float* emb = c.lin_fwd(e0s, u.B, u.ED, u.nm.w("time_embed.2.weight"), u.nm.w("time_embed.2.bias"), u.ED);
    return c.silu(emb, (size_t)u.B * u.ED);
}

UNetLayer res_layer(const Names& nm, const std::string& p, int Cin, int Cout, int H, int W) {
    UNetLayer l{K_RES, p, Cin, Cout, H, W, 0, -1, nullptr, {}, {}, {}, {}};
    static const char* k[RP_COUNT] = {"in_layers.0.weight", "in_layers.0.bias", "in_layers.2.weight", "in_layers.2.bias", "emb_layers.1.weight",
                                      "emb_layers.1.bias", "out_layers.0.weight", "out_layers.0.bias", "out_layers.3.weight", "out_layers.3.bias",
                                      "skip_connection.weight", "skip_connection.bias"};
    for (int i = 0; i < RP_COUNT; ++i) l.P.push_back((i >= RP_SKIP_W && Cin == Cout) ? nullptr : nm.w(p + "." + k[i]));
    return l;
}
UNetLayer st_layer(const UNetStep& u, const std::string& p, int C, int H, int W) {
    const Names& nm = u.nm;
    UNetLayer l{K_ST, p, C, C, H, W, 0, -1, nullptr, {}, {}, {}, {}};
    l.P.resize(ST_COUNT);
    l.G.assign(ST_COUNT, nullptr);
    l.P[ST_NORM_W] = nm.w(p + ".norm.weight"); l.P[ST_NORM_B] = nm.w(p + ".norm.bias");
    l.P[ST_PIN_W] = nm.w(p + ".proj_in.weight"); l.P[ST_PIN_B] = nm.w(p + ".proj_in.bias");
    l.P[ST_POUT_W] = nm.w(p + ".proj_out.weight"); l.P[ST_POUT_B] = nm.w(p + ".proj_out.bias");
    for (int i = 0; i < TP_COUNT; ++i) {
        const std::string k = p + ".transformer_blocks.0." + u.block_names[i];
        if (u.cfg.fuser_kind == 2 && (i == TP_F_LIN_W || i == TP_F_LIN_B)) {      // GatedCrossAttentionDense has no linear: the slots stay null
            if (nm.has(k) || nm.g(k))
                throw GlError(GL_ERR_ARG, "unet_train_step: '" + k + "' in the state_dict of a gatedCA model, whose fusers have no linear (attention.py:190-201)");
            continue;
        }
        l.P[ST_BLOCK0 + i] = nm.w(k);
        l.G[ST_BLOCK0 + i] = nm.g(k);
    }
    return l;
}
// a resampling conv (K_DOWN / K_UP) of C channels
UNetLayer resample_layer(const Names& nm, Kind kind, const std::string& p, int C, int H, int W) {
    return UNetLayer{kind, p, C, C, H, W, 0, -1, nullptr, {nm.w(p + ".weight"), nm.w(p + ".bias")}, {}, {}, {}};
}
TrainBlockDims st_dims(const UNetStep& u, const UNetLayer& l) {
    return {u.B, l.H * l.W, u.Ng, l.Cout, u.cfg.num_heads, u.in.ctx_T, u.KD, u.in.fuser_scale, u.cfg.fuser_kind};
}
TrainResDims res_dims(const UNetStep& u, const UNetLayer& l) { return {u.B, l.H, l.W, l.Cin, l.Cout, u.ED}; }

// One layer's forward on the stream h; the layer, with what its backward needs, is appended to L.
// checkpointing: a block's output is allocated first, everything its forward keeps (activations, statistics, the bf16
// operand copies) is given back to the arena behind it; the backward recomputes the forward from x_in
void run(const UNetStep& u, const float* objs, const float* semb, Act& h, std::vector<UNetLayer>& L, UNetLayer l) {
    const Ctx& c = u.c;
    const size_t rows = (size_t)u.B * l.H * l.W;
    float* y = nullptr;
    l.x_in = h.p;
    if (l.kind == K_RES) {
        res_check(res_dims(u, l), l.P.data());
        y = c.f32(rows * l.Cout);
        const size_t mk = c.ar.mark();
        l.rs = res_forward(c, res_dims(u, l), l.P.data(), h.p, semb, y);
        if (u.in.checkpoint) c.ar.release(mk);
    } else if (l.kind == K_ST) {
        st_check(st_dims(u, l), l.P.data(), l.G.data());
        y = c.f32(rows * l.Cout);
        const size_t mk = c.ar.mark();
        l.ss = st_forward(c, st_dims(u, l), l.P.data(), h.p, objs, u.in.context, y);
        if (u.in.checkpoint) c.ar.release(mk);
    } else {
        const bool up = l.kind == K_UP;
        y = resample_forward(c, up, u.B, l.H, l.W, l.Cin, l.P[0], l.P[1], h.p);
        h.H = up ? l.H * 2 : l.H / 2; h.W = up ? l.W * 2 : l.W / 2;
    }
    h.p = y; h.C = l.Cout;
    L.push_back(std::move(l));
}

// input_blocks / middle_block / output_blocks (openaimodel.py:452-464), in forward order, from h0 = conv_in's output; returns the
// stream in front of `out`
Act build_and_run_layers(const UNetStep& u, const float* objs, const float* semb, float* h0, std::vector<UNetLayer>& L) {
    const Ctx& c = u.c;
    const Names& nm = u.nm;
    const TrainUNetCfg& cfg = u.cfg;
    const int mc = u.mc;
    auto in_attn = [&](int ds) { for (int i = 0; i < cfg.n_attn; ++i) if (cfg.attention_resolutions[i] == ds) return true; return false; };
    Act h{h0, mc, u.H0, u.W0};
    std::vector<Act> hs{h};
    std::vector<int> hs_layer{-1};          // which layer produced each skip (-1: conv_in)
    int ch = mc, ds = 1, n = 1;
    for (int level = 0; level < cfg.n_mult; ++level) {
        const int mult = cfg.channel_mult[level];
        for (int r = 0; r < cfg.num_res_blocks; ++r) {
            const std::string p = fmt("input_blocks.%d", n);
            run(u, objs, semb, h, L, res_layer(nm, p + ".0", ch, mult * mc, h.H, h.W));
            ch = mult * mc;
            if (in_attn(ds)) run(u, objs, semb, h, L, st_layer(u, p + ".1", ch, h.H, h.W));
            hs.push_back(h); hs_layer.push_back((int)L.size() - 1);
            ++n;
        }
        if (level != cfg.n_mult - 1) {
            run(u, objs, semb, h, L, resample_layer(nm, K_DOWN, fmt("input_blocks.%d.0.op", n), ch, h.H, h.W));
            hs.push_back(h); hs_layer.push_back((int)L.size() - 1);
            ds *= 2;
            ++n;
        }
    }
    run(u, objs, semb, h, L, res_layer(nm, "middle_block.0", ch, ch, h.H, h.W));
    run(u, objs, semb, h, L, st_layer(u, "middle_block.1", ch, h.H, h.W));
    run(u, objs, semb, h, L, res_layer(nm, "middle_block.2", ch, ch, h.H, h.W));
    n = 0;
    for (int level = cfg.n_mult - 1; level >= 0; --level) {
        const int mult = cfg.channel_mult[level];
        for (int i = 0; i <= cfg.num_res_blocks; ++i) {
            const Act sk = hs.back();
            const int sk_layer = hs_layer.back();
            hs.pop_back(); hs_layer.pop_back();
            if (sk.H != h.H || sk.W != h.W) throw GlError(GL_ERR_STATE, "unet_train_step: skip / stream size mismatch");
            {   // h = cat([h, hs.pop()], dim = 1)
                const size_t rows = (size_t)u.B * h.H * h.W;
                float* cat = c.f32(rows * (h.C + sk.C));
                c.ew(concat_kernel, rows * (h.C + sk.C), h.p, h.C, sk.p, sk.C, rows, cat);
                L.push_back(UNetLayer{K_CAT, "", h.C + sk.C, h.C + sk.C, h.H, h.W, h.C, sk_layer, nullptr, {}, {}, {}, {}});
                h.p = cat; h.C += sk.C;
            }
            const std::string p = fmt("output_blocks.%d", n);
            run(u, objs, semb, h, L, res_layer(nm, p + ".0", h.C, mc * mult, h.H, h.W));
            ch = mc * mult;
            int j = 1;
            if (in_attn(ds)) { run(u, objs, semb, h, L, st_layer(u, p + ".1", ch, h.H, h.W)); j = 2; }
            if (level && i == cfg.num_res_blocks) {
                run(u, objs, semb, h, L, resample_layer(nm, K_UP, p + fmt(".%d.conv", j), ch, h.H, h.W));
                ds /= 2;
            }
            ++n;
        }
    }
    return h;
}

// out = conv(silu(gn(h)))  (openaimodel.py:389-393), the loss and dL/d out
struct OutSaved { Ctx::GN on; float* gy; };
OutSaved out_forward_and_loss(const UNetStep& u, const Act& h, float* eps_out, float* loss) {
    const Ctx& c = u.c;
    OutSaved o;
    o.on = c.gn_silu_fwd(h.p, u.B, u.H0 * u.W0, u.mc, u.nm.w("out.0.weight"), u.nm.w("out.0.bias"));
    const int Co = u.cfg.out_channels;
    const size_t ny = u.M0 * Co;
    const float* y = conv3x3_direct(c, o.on.a, u.nm.w("out.2.weight"), u.nm.w("out.2.bias"), u.B, u.H0, u.W0, u.mc, Co);
    if (eps_out) c.hip(hipMemcpyAsync(eps_out, y, ny * 4, hipMemcpyDeviceToDevice, c.s), "hipMemcpyAsync");
    if (c.loss_w) {     // per-sample weights (gl_train_set_loss_weights): the weighted loss and its gradient, train_run.hip
        float* part = c.f32((size_t)u.B);
        o.gy = c.f32(ny);
        c.ck(weighted_mse(y, u.in.target, c.loss_w, u.B, ny / (size_t)u.B, part, o.gy, loss, c.s));
    } else {
        o.gy = c.mse_loss(y, u.in.target, ny, loss);
    }
    return o;
}
// -> dL/d(the stream in front of `out`). The out conv's dgrad: the same direct conv on the flipped / transposed weight
float* out_backward(const UNetStep& u, const OutSaved& o) {
    const Ctx& c = u.c;
    const float* wt = c.conv_dgrad_weight(u.nm.w("out.2.weight"), u.cfg.out_channels, u.mc);
    float* g_a = conv3x3_direct(c, o.gy, wt, nullptr, u.B, u.H0, u.W0, u.cfg.out_channels, u.mc);
    float* g = c.f32(u.M0 * u.mc);
    c.gn_silu_bwd(g_a, o.on, u.nm.w("out.0.weight"), u.nm.w("out.0.bias"), u.B, u.H0 * u.W0, u.mc, g, false);
    return g;
}

// The layers' backward, last to first. g: dL/d(the last layer's output). in_grad: a trainable first conv (or downsampler) needs
// dL/d(conv_in output): the loop then runs through the layers in front of the first fuser too and keeps conv_in's skip gradient
// (hs_layer -1, the last output block's concat), which is added to what it returns. g_objs [B][Ng][KD] accumulates dL/d objs.
// Event j of grad_events is recorded behind the j-th SpatialTransformer (module order); returns their number through n_st.
float* layers_backward(const UNetStep& u, std::vector<UNetLayer>& L, const float* objs, const float* semb, float* g, bool in_grad, float* g_objs,
                       hipEvent_t* grad_events, int n_grad_events, int& n_st) {
    const Ctx& c = u.c;
    const int B = u.B;
    const bool checkpoint = u.in.checkpoint;
    std::vector<float*> skip_grad(L.size(), nullptr);     // dL/d(output of layer i) arriving through a skip connection
    int first_st = -1;
    for (size_t i = 0; i < L.size(); ++i)
        if (L[i].kind == K_ST) { first_st = (int)i; break; }
    std::vector<int> st_ordinal(L.size(), -1);            // SpatialTransformer number in module order (input_blocks .. middle .. output_blocks)
    n_st = 0;
    for (size_t i = 0; i < L.size(); ++i)
        if (L[i].kind == K_ST) st_ordinal[i] = n_st++;
    int stop = in_grad ? 0 : first_st;
    if (c.lora)     // a ResBlock or resampling layer with an adapter in front of the first fuser: its backward has to run too
        for (int i = 0; i < stop; ++i) {
            const UNetLayer& l = L[i];
            bool adapted = false;
            if (l.kind == K_RES)
                for (int k : {(int)RP_C1_W, (int)RP_EMB_W, (int)RP_C2_W, (int)RP_SKIP_W}) adapted = adapted || lora_find(c, l.P[k]);
            else if (l.kind == K_DOWN || l.kind == K_UP)
                adapted = lora_find(c, l.P[0]) != nullptr;
            if (adapted) { stop = i; break; }
        }
    float* skip0 = nullptr;
    for (int i = (int)L.size() - 1; i >= 0 && i >= stop; --i) {
        UNetLayer& l = L[i];
        const size_t rows = (size_t)B * l.H * l.W;
        if (skip_grad[i]) {     // this layer's output also went into a skip connection (l.H, l.W are its INPUT size)
            const size_t out_rows = l.kind == K_DOWN ? rows / 4 : l.kind == K_UP ? rows * 4 : rows;
            c.add(g, skip_grad[i], out_rows * l.Cout);
        }
        if (l.kind == K_CAT) {
            float* gh = c.f32(rows * l.C0);
            split_cols(c, g, l.Cin, 0, l.C0, rows, gh, false);
            const int C1 = l.Cin - l.C0;
            if (in_grad || l.skip_idx >= stop) {   // (without in_grad a skip produced in front of the first layer that trains carries no gradient anybody needs)
                float* gs = c.f32(rows * C1);
                split_cols(c, g, l.Cin, l.C0, C1, rows, gs, false);
                if (l.skip_idx < 0) skip0 = gs;
                else skip_grad[l.skip_idx] = gs;
            }
            g = gh;
        } else if (l.kind == K_RES) {
            float* keep = (checkpoint && l.Cin != l.Cout) ? c.f32(rows * l.Cin) : nullptr;    // (allocated in front of the scope below)
            const size_t mk = c.ar.mark();
            if (checkpoint) l.rs = res_forward(c, res_dims(u, l), l.P.data(), l.x_in, semb, c.f32(rows * l.Cout));
            float* gx = res_backward(c, res_dims(u, l), l.P.data(), l.rs, g);       // (g itself, updated in place, when Cin == Cout)
            if (keep) {
                c.hip(hipMemcpyAsync(keep, gx, rows * l.Cin * 4, hipMemcpyDeviceToDevice, c.s), "hipMemcpyAsync");
                gx = keep;
            }
            if (checkpoint) c.ar.release(mk);
            g = gx;
        } else if (l.kind == K_ST) {
            float* d_o = c.f32((size_t)u.MR * u.KD);
            const size_t mk = c.ar.mark();
            if (checkpoint) l.ss = st_forward(c, st_dims(u, l), l.P.data(), l.x_in, objs, u.in.context, c.f32(rows * l.Cout));
            st_backward(c, st_dims(u, l), l.P.data(), l.ss, objs, g, d_o, l.G.data(), u.in.context);      // g in place
            c.add(g_objs, d_o, (size_t)u.MR * u.KD);
            if (checkpoint) c.ar.release(mk);
            // this block's fuser gradients are final: the caller's communication stream may pick them up (gl_train_wait_grads)
            // while the blocks in front of it are still in backward
            if (grad_events && st_ordinal[i] < n_grad_events) c.hip(hipEventRecord(grad_events[st_ordinal[i]], c.s), "hipEventRecord");
        } else {
            g = resample_backward(c, l.kind == K_UP, B, l.H, l.W, l.Cin, l.P[0], g, l.x_in);
        }
    }
    if (in_grad && skip0) c.add(g, skip0, u.M0 * u.mc);      // g = dL/d(conv_in output) through input_blocks.1, plus its skip
    return g;
}

}  // namespace

int unet_train_step(Arena& ar, float* ws, size_t ws_bytes, const TrainUNetCfg& cfg, const TrainUNetIn& in, int n_params, const char* const* names,
                    const float* const* params, float* const* grads, const char* const* block_names, float* eps_out, float* loss, hipStream_t s, hipEvent_t* grad_events, int n_grad_events,
                    TrainWeightCache* cache, const TrainSpatialIn* spatial, const TrainLoraAdapter* adapters, int n_adapters, const float* loss_weights) {
    try {
        Names nm;
        nm.params = params;
        nm.grads = grads;
        for (int i = 0; i < n_params; ++i) nm.idx[names[i]] = i;
        check_trainable_set(cfg, n_params, names, grads, spatial);
        Ctx c{ar, ws, ws_bytes, s};
        c.loss_w = loss_weights;
        std::unordered_set<const void*> frozen;
        if (cache) {
            for (int i = 0; i < n_params; ++i)
                if (params[i] && !grads[i]) frozen.insert(params[i]);
            c.wc = cache;
            c.frozen = &frozen;
        }
        // the adapter tensors are read as fp32 by their own kernels: nothing of them enters the operand cache
        const LoraTable lora = lora_table(nm, adapters, n_adapters);
        if (!lora.empty()) c.lora = &lora;
        const UNetStep u = step_dims(c, nm, cfg, in, spatial, block_names);
        // ---- forward; every layer remembers what its backward needs
        PosBranch pb[2];
        SpatialSaved tok;
        const float* objs = grounding_forward(u, pb, tok);
        const float* semb = time_embedding(u);
        DsSaved dsv;
        const float* xin = nullptr;
        float* h0 = conv_in_forward(u, dsv, xin);
        std::vector<UNetLayer> L;
        const Act h = build_and_run_layers(u, objs, semb, h0, L);
        const OutSaved out = out_forward_and_loss(u, h, eps_out, loss);
        // ---- backward
        float* g = out_backward(u, out);
        float* g_objs = c.f32((size_t)u.MR * u.KD);
        c.hip(hipMemsetAsync(g_objs, 0, (size_t)u.MR * u.KD * 4, s), "hipMemsetAsync");
        const bool in_grad = (u.Ce > 0 && (nm.g("input_blocks.0.0.weight") || downsampler_grads(nm))) || (u.Ci > 0 && nm.g("input_blocks.0.0.weight"));
        int n_st_layers = 0;
        g = layers_backward(u, L, objs, semb, g, in_grad, g_objs, grad_events, n_grad_events, n_st_layers);
        if (in_grad) conv_in_backward(c, nm, spatial, dsv, xin, u.B, u.H0, u.W0, u.Cx, u.Ce, u.Ci, u.mc, g);
        grounding_backward(u, pb, tok, g_objs);
        // position_net's gradients -- the last ones of the step -- are final
        if (grad_events && n_st_layers < n_grad_events) c.hip(hipEventRecord(grad_events[n_st_layers], s), "hipEventRecord");
        c.hip(hipGetLastError(), "training step kernel launch");
    } catch (const GlError& e) {
        return set_error(e.code, "%s", e.what());
    }
    return GL_OK;
}

}  // namespace gl
