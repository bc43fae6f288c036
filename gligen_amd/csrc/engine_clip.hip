// gligen_amd engine -- the CLIP text and vision towers
#include "engine_impl.h"
#include <algorithm>

namespace gl {

// ---------------------------------------------------------------- CLIP text tower
void Engine::configure_clip_text(const gl_clip_text_config& c) {
    if (c.vocab < 1 || c.layers < 1 || c.heads < 1 || c.width < 1 || c.intermediate < 1 || c.max_positions < 1 || !(c.ln_eps > 0.f))
        throw GlError(GL_ERR_ARG, fmt("clip text config: vocab %d, width %d, heads %d, layers %d, intermediate %d, max_positions %d, ln_eps %g must all be positive",
                                      c.vocab, c.width, c.heads, c.layers, c.intermediate, c.max_positions, c.ln_eps));
    if (c.width % c.heads || c.width / c.heads != kClipHeadDim)
        throw GlError(GL_ERR_UNSUPPORTED, fmt("clip text tower: head dim %d (width %d / %d heads) is not supported: clip_attn_kernel is built for head dim %d",
                                              c.width / c.heads, c.width, c.heads, kClipHeadDim));
    if (c.width > kClipMaxWidth) throw GlError(GL_ERR_UNSUPPORTED, fmt("clip text tower: width %d exceeds %d", c.width, kClipMaxWidth));
    if (c.intermediate % 64) throw GlError(GL_ERR_UNSUPPORTED, fmt("clip text tower: intermediate size %d is not a multiple of 64", c.intermediate));
    if (c.max_positions > kClipMaxTokens)
        throw GlError(GL_ERR_UNSUPPORTED, fmt("clip text tower: max_positions %d exceeds the %d tokens clip_attn_kernel holds", c.max_positions, kClipMaxTokens));
    clipt_.cfg = c;
    clipt_.present = true;
}

// the uploaded tensor `key` is [d0] (d1 = 0) or [d0][d1]
void Engine::clip_expect_shape(const std::string& key, int64_t d0, int64_t d1) const {
    const RawTensor& t = raw(key);
    const int64_t a = t.shape.empty() ? 0 : t.shape[0], b = t.shape.size() > 1 ? t.shape[1] : 0;
    if (a != d0 || (d1 && b != d1))
        throw GlError(GL_ERR_ARG, fmt("'%s' has shape [%lld, %lld], the configuration expects [%lld, %lld]", key.c_str(), (long long)a, (long long)b, (long long)d0, (long long)d1));
}

void Engine::build_clip_layers(const std::string& P, int n, int width, int intermediate, std::vector<ClipLayerW>& out) {
    struct { int width, intermediate; } c{width, intermediate};
    out.clear();
    for (int l = 0; l < n; ++l) {
        const std::string L = P + "encoder.layers." + std::to_string(l) + ".";
        ClipLayerW w;
        w.ln1 = norm(L + "layer_norm1");
        w.ln2 = norm(L + "layer_norm2");
        for (const char* n : {"q_proj", "k_proj", "v_proj", "out_proj"}) {
            clip_expect_shape(L + "self_attn." + n + ".weight", c.width, c.width);
            clip_expect_shape(L + "self_attn." + n + ".bias", c.width, 0);
        }
        clip_expect_shape(L + "mlp.fc1.weight", c.intermediate, c.width);
        clip_expect_shape(L + "mlp.fc2.weight", c.width, c.intermediate);
        if (w.ln1.C != c.width || w.ln2.C != c.width) throw GlError(GL_ERR_ARG, "'" + L + "layer_norm*' does not match the configured width");
        // [q_proj ; k_proj ; v_proj] rows: one GEMM writes the rows [q | k | v] that clip_attn_kernel slices per head
        w.qkv.w = cast_rows({L + "self_attn.q_proj.weight", L + "self_attn.k_proj.weight", L + "self_attn.v_proj.weight"});
        w.qkv.N = 3 * c.width;
        w.qkv.K = c.width;
        float* b3 = reinterpret_cast<float*>(persist((size_t)3 * c.width * sizeof(float), false));
        const char* names[3] = {"q_proj", "k_proj", "v_proj"};
        for (int i = 0; i < 3; ++i)
            HIPCK(hipMemcpy(b3 + (size_t)i * c.width, F(L + "self_attn." + names[i] + ".bias"), (size_t)c.width * sizeof(float), hipMemcpyDeviceToDevice));
        w.qkv.b = b3;
        w.out = linear(L + "self_attn.out_proj");
        w.fc1 = linear(L + "mlp.fc1");
        w.fc2 = linear(L + "mlp.fc2");
        out.push_back(w);
    }
}

// Weights under "text_encoder/" + the checkpoint's key (transformers 4.x layout: transformer.text_model.*)
void Engine::build_clip_text() {
    const gl_clip_text_config& c = clipt_.cfg;
    const std::string P = "text_encoder/transformer.text_model.";
    clip_expect_shape(P + "embeddings.token_embedding.weight", c.vocab, c.width);
    clip_expect_shape(P + "embeddings.position_embedding.weight", c.max_positions, c.width);
    clipt_.tok = FK(P + "embeddings.token_embedding.weight");
    clipt_.pos = FK(P + "embeddings.position_embedding.weight");
    build_clip_layers(P, c.layers, c.width, c.intermediate, clipt_.layers);
    clipt_.final_ln = norm(P + "final_layer_norm");
    if (clipt_.final_ln.C != c.width) throw GlError(GL_ERR_ARG, "'" + P + "final_layer_norm' does not match the configured width");
    clipt_.bad_ids = reinterpret_cast<unsigned*>(persist(sizeof(unsigned), true));
}

// Seven launches per layer. The residual stream stays in fp32 (torch's autocast, the yardstick of the parity tests, adds bf16 linear
// outputs into an fp32 residual): the out-projection and fc2 write fp32 rows (bias included) that the NEXT LayerNorm's launch adds
// into the stream before it normalises -- clip_add_ln_kernel reads and writes the stream once per sub-layer. That is why the
// LayerNorms are not folded into the GEMMs behind them here (gemm.h: the folded form takes its row statistics from the bf16 GEMM
// that produced the rows).
const float* Engine::clip_layers_run(const std::vector<ClipLayerW>& layers, const ClipStack& c, float* h, float* tmp, int S, int T, bool causal,
                                     hipStream_t s) {
    const int M = S * T, W = c.width, I = c.intermediate;
    const size_t Mp = (size_t)round_up(M, 256);   // (whole GEMM tiles of rows exist behind every operand)
    bf16* xn = arena_.get<bf16>(Mp * W);
    bf16* qkv = arena_.get<bf16>(Mp * 3 * W);
    bf16* ao = arena_.get<bf16>(Mp * W);
    bf16* f1 = arena_.get<bf16>(Mp * I);
    auto lin = [&](const bf16* x, const LinW& L, void* out, bool f32, int act) {
        Epilogue E = e_rows(out, L.N, L.b);
        E.out_f32 = f32 ? 1 : 0; E.act = act;
        gemm(a_rows(x, L.K), L.w, M, L.N, L.K, E, s);
    };
    const float* delta = nullptr;
    const char* attn_name = T <= kClipMaxTokens ? "clip_attn_kernel" : "clip_attn_long_kernel";
    for (const ClipLayerW& w : layers) {
        CK(clip_add_ln_launch(h, delta, w.ln1.g, w.ln1.b, c.ln_eps, xn, nullptr, M, W, s));
        lin(xn, w.qkv, qkv, false, ACT_NONE);
        {
            ProfScope ps(this, s, attn_name, 4.0 * S * c.heads * (double)T * T * kClipHeadDim, 0.0);
            CK(clip_attn_launch(qkv, ao, S, T, c.heads, causal ? 1 : 0, s));
        }
        lin(ao, w.out, tmp, true, ACT_NONE);
        CK(clip_add_ln_launch(h, tmp, w.ln2.g, w.ln2.b, c.ln_eps, xn, nullptr, M, W, s));
        lin(xn, w.fc1, f1, false, ACT_QUICK_GELU);
        lin(f1, w.fc2, tmp, true, ACT_NONE);
        delta = tmp;
        n_launches += 3;   // two add + LayerNorm launches, one attention (gemm() counts its own)
    }
    return delta;
}

void Engine::clip_text_encode(const int32_t* ids, const int32_t* eos_index, int S, int T, float* last_hidden, float* pooled, hipStream_t s) {
    if (!clipt_.present || !finalized_) throw GlError(GL_ERR_STATE, "clip text tower not configured / finalized");
    if (!ids || !last_hidden || (pooled && !eos_index)) throw GlError(GL_ERR_ARG, "clip_text_encode: null ids / output (pooled needs eos_index)");
    const gl_clip_text_config& c = clipt_.cfg;
    if (S < 1 || T < 1 || T > c.max_positions)
        throw GlError(GL_ERR_ARG, fmt("clip_text_encode: %d sequences of %d tokens (1 <= tokens <= max_positions %d)", S, T, c.max_positions));
    const int W = c.width;
    // activation bytes of one chunk of Sc sequences: fp32 stream + fp32 scratch + bf16 [LN | q,k,v | attention | fc1] rows, row count
    // rounded up to whole GEMM tiles, + the allocator's alignment
    auto need = [&](int Sc) { return (size_t)round_up(Sc * T, 256) * ((size_t)W * (4 + 4 + 2 + 6 + 2) + (size_t)c.intermediate * 2) + 8 * 256; };
    const size_t mk = arena_.mark();
    const size_t avail = arena_.capacity() - std::min(arena_.capacity(), (mk + 255) & ~size_t(255));
    int Sc = S;
    while (Sc > 1 && need(Sc) > avail) Sc = (Sc + 1) / 2;
    if (need(Sc) > avail) throw GlError(GL_ERR_STATE, fmt("clip_text_encode: the arena (%zu bytes free) does not hold one sequence (%zu bytes)", avail, need(1)));
    for (int s0 = 0; s0 < S; s0 += Sc) {
        const int n = std::min(Sc, S - s0), M = n * T;
        const size_t Mp = (size_t)round_up(M, 256);
        float* h = arena_.get<float>(Mp * W);
        float* tmp = arena_.get<float>(Mp * W);
        CK(clip_embed_launch(ids + (size_t)s0 * T, clipt_.tok, clipt_.pos, h, M, T, W, c.vocab, clipt_.bad_ids, s));
        const float* delta = clip_layers_run(clipt_.layers, ClipStack{c.width, c.heads, c.intermediate, c.ln_eps}, h, tmp, n, T, true, s);
        float* out = last_hidden + (size_t)s0 * T * W;
        CK(clip_add_ln_launch(h, delta, clipt_.final_ln.g, clipt_.final_ln.b, c.ln_eps, nullptr, out, M, W, s));
        n_launches += 2;
        if (pooled) {
            CK(clip_pool_launch(out, eos_index + s0, pooled + (size_t)s0 * W, n, T, W, s));
            ++n_launches;
        }
        arena_.release(mk);
    }
}

// ---------------------------------------------------------------- CLIP vision tower
void Engine::configure_clip_vision(const gl_clip_vision_config& c) {
    if (c.image_size < 1 || c.patch < 1 || c.layers < 1 || c.heads < 1 || c.width < 1 || c.intermediate < 1 || c.projection_dim < 1 || !(c.ln_eps > 0.f))
        throw GlError(GL_ERR_ARG, fmt("clip vision config: image_size %d, patch %d, width %d, heads %d, layers %d, intermediate %d, projection_dim %d, ln_eps %g must all be positive",
                                      c.image_size, c.patch, c.width, c.heads, c.layers, c.intermediate, c.projection_dim, c.ln_eps));
    if (c.width % c.heads || c.width / c.heads != kClipHeadDim)
        throw GlError(GL_ERR_UNSUPPORTED, fmt("clip vision tower: head dim %d (width %d / %d heads) is not supported: the attention kernels are built for head dim %d",
                                              c.width / c.heads, c.width, c.heads, kClipHeadDim));
    if (c.width > kClipMaxWidth) throw GlError(GL_ERR_UNSUPPORTED, fmt("clip vision tower: width %d exceeds %d", c.width, kClipMaxWidth));
    if (c.intermediate % 64) throw GlError(GL_ERR_UNSUPPORTED, fmt("clip vision tower: intermediate size %d is not a multiple of 64", c.intermediate));
    if (c.image_size % c.patch)
        throw GlError(GL_ERR_UNSUPPORTED, fmt("clip vision tower: image_size %d is not a multiple of the patch size %d", c.image_size, c.patch));
    const int64_t g = c.image_size / c.patch, tokens = g * g + 1;
    if (tokens > kClipLongMaxTokens)
        throw GlError(GL_ERR_UNSUPPORTED, fmt("clip vision tower: %lld tokens (image_size %d / patch %d) exceed the %d clip_attn_long_kernel holds", (long long)tokens,
                                              c.image_size, c.patch, kClipLongMaxTokens));
    clipv_.cfg = c;
    clipv_.present = true;
}

// Weights under "clip_vision/" + the transformers key (CLIPModel / CLIPVisionModelWithProjection: vision_model.*, visual_projection.weight)
void Engine::build_clip_vision() {
    const gl_clip_vision_config& c = clipv_.cfg;
    const std::string R = "clip_vision/", P = R + "vision_model.";
    const int tokens = clip_vision_tokens();
    auto expect = [&](const std::string& key, std::vector<int64_t> want) {
        const RawTensor& t = raw(key);
        if (t.shape != want) {
            auto str = [](const std::vector<int64_t>& v) { std::string o = "["; for (size_t i = 0; i < v.size(); ++i) o += (i ? ", " : "") + std::to_string(v[i]); return o + "]"; };
            throw GlError(GL_ERR_ARG, "'" + key + "' has shape " + str(t.shape) + ", the configuration expects " + str(want));
        }
    };
    expect(P + "embeddings.class_embedding", {c.width});
    expect(P + "embeddings.patch_embedding.weight", {c.width, 3, c.patch, c.patch});
    expect(P + "embeddings.position_embedding.weight", {tokens, c.width});
    expect(R + "visual_projection.weight", {c.projection_dim, c.width});
    clipv_.cls = FK(P + "embeddings.class_embedding");
    clipv_.pos = FK(P + "embeddings.position_embedding.weight");
    clipv_.patch = linear(P + "embeddings.patch_embedding", false);    // [width][3 p p], K zero-padded to a multiple of 64 (588 -> 640)
    clipv_.pre_ln = norm(P + "pre_layrnorm");                          // (sic: the transformers key)
    clipv_.post_ln = norm(P + "post_layernorm");
    if (clipv_.pre_ln.C != c.width) throw GlError(GL_ERR_ARG, "'" + P + "pre_layrnorm' does not match the configured width");
    if (clipv_.post_ln.C != c.width) throw GlError(GL_ERR_ARG, "'" + P + "post_layernorm' does not match the configured width");
    build_clip_layers(P, c.layers, c.width, c.intermediate, clipv_.layers);
    clipv_.proj = linear(R + "visual_projection", false);
}

void Engine::clip_vision_encode(const float* pixel_values, int S, float* last_hidden, float* pooled, float* image_embeds, hipStream_t s) {
    if (!clipv_.present || !finalized_) throw GlError(GL_ERR_STATE, "clip vision tower not configured / finalized");
    if (!pixel_values || (!last_hidden && !pooled && !image_embeds)) throw GlError(GL_ERR_ARG, "clip_vision_encode: null pixel_values / no output");
    if (S < 1) throw GlError(GL_ERR_ARG, fmt("clip_vision_encode: %d images", S));
    const gl_clip_vision_config& c = clipv_.cfg;
    const int W = c.width, T = clip_vision_tokens(), NP = T - 1, Kp = clipv_.patch.K, D = c.projection_dim;
    const ClipStack stack{c.width, c.heads, c.intermediate, c.ln_eps};
    // activation bytes of one chunk of Sc images: what clip_text_encode counts + the bf16 patch rows (the fp32 patch embeddings use
    // the scratch rows) + the bf16 pooled rows the projection reads, row counts rounded up to whole GEMM tiles
    auto need = [&](int Sc) {
        return (size_t)round_up(Sc * T, 256) * ((size_t)W * (4 + 4 + 2 + 6 + 2) + (size_t)c.intermediate * 2) + (size_t)round_up(Sc * NP, 256) * Kp * 2 +
               (size_t)round_up(Sc, 256) * W * 2 + 10 * 256;
    };
    const size_t mk = arena_.mark();
    const size_t avail = arena_.capacity() - std::min(arena_.capacity(), (mk + 255) & ~size_t(255));
    int Sc = S;
    while (Sc > 1 && need(Sc) > avail) Sc = (Sc + 1) / 2;
    if (need(Sc) > avail) throw GlError(GL_ERR_STATE, fmt("clip_vision_encode: the arena (%zu bytes free) does not hold one image (%zu bytes)", avail, need(1)));
    const size_t image_elems = (size_t)3 * c.image_size * c.image_size;
    // no K split in this tower's GEMMs: a row's sums are then the same whatever the number of images, so an image's feature does
    // not depend on the batch it came in (nor on the chunking above)
    struct NoSplit { NoSplit() { gemm_set_no_split(1); } ~NoSplit() { gemm_set_no_split(0); } } no_split;
    for (int s0 = 0; s0 < S; s0 += Sc) {
        const int n = std::min(Sc, S - s0), M = n * T;
        const size_t Mp = (size_t)round_up(M, 256);
        float* h = arena_.get<float>(Mp * W);
        float* tmp = arena_.get<float>(Mp * W);
        bf16* rows = arena_.get<bf16>((size_t)round_up(n * NP, 256) * Kp);
        bf16* pooled_bf = arena_.get<bf16>((size_t)round_up(n, 256) * W);
        CK(clip_patch_rows_launch(pixel_values + (size_t)s0 * image_elems, rows, n, c.image_size, c.patch, Kp, s));
        Epilogue E = e_rows(tmp, W);
        E.out_f32 = 1;
        gemm(a_rows(rows, Kp), clipv_.patch.w, n * NP, W, Kp, E, s);
        CK(clip_vision_embed_launch(tmp, clipv_.cls, clipv_.pos, h, n, T, W, s));
        CK(clip_ln_rows_launch(h, nullptr, W, clipv_.pre_ln.g, clipv_.pre_ln.b, c.ln_eps, h, nullptr, W, M, W, s));   // in place
        n_launches += 3;
        const float* delta = clip_layers_run(clipv_.layers, stack, h, tmp, n, T, false, s);
        if (last_hidden) {
            CK(clip_add_launch(h, delta, last_hidden + (size_t)s0 * T * W, (int64_t)M * W, s));
            ++n_launches;
        }
        if (pooled || image_embeds) {
            // post_layernorm of the class rows (h + delta)[s * T]: a row stride of T * width, no gather
            CK(clip_ln_rows_launch(h, delta, (int64_t)T * W, clipv_.post_ln.g, clipv_.post_ln.b, c.ln_eps, pooled ? pooled + (size_t)s0 * W : nullptr,
                                   image_embeds ? pooled_bf : nullptr, W, n, W, s));
            ++n_launches;
        }
        if (image_embeds) {
            E = e_rows(image_embeds + (size_t)s0 * D, D);
            E.out_f32 = 1;
            gemm(a_rows(pooled_bf, W), clipv_.proj.w, n, D, clipv_.proj.K, E, s);
        }
        arena_.release(mk);
    }
}

}  // namespace gl
