// gligen_amd engine -- AutoencoderKL: decoder and encoder
#include "engine_impl.h"
#include "tile.h"
#include <algorithm>
#include <cmath>

namespace gl {

void Engine::configure_vae(const gl_vae_config& c) {
    if (c.n_mult < 1 || c.n_mult > 8) throw GlError(GL_ERR_ARG, "bad vae config");
    vae_.cfg = c;
    vae_.dec.present = true;
}

// mid.block_1 -> mid.attn_1 -> mid.block_2 of either half (model.py:409-415, 500-506)
void Engine::build_vae_mid(VaeHalf& h, const std::string& p, int C) {
    h.mid1 = resw(p + ".block_1", C, C, false);
    h.mid2 = resw(p + ".block_2", C, C, false);
    h.attn.gn = norm(p + ".attn_1.norm");
    h.attn.q = conv1(p + ".attn_1.q");
    h.attn.k = conv1(p + ".attn_1.k");
    h.attn.v = conv1(p + ".attn_1.v");
    h.attn.proj = conv1(p + ".attn_1.proj_out");
}

void Engine::build_vae() {
    const gl_vae_config& c = vae_.cfg;
    const std::string V = "vae/";
    vae_.dec.quant_w = F(V + "post_quant_conv.weight");
    vae_.dec.quant_b = F(V + "post_quant_conv.bias");
    const int block_in0 = c.ch * c.ch_mult[c.n_mult - 1];
    vae_.dec.in_small = conv3_small(V + "decoder.conv_in", block_in0);
    build_vae_mid(vae_.dec, V + "decoder.mid", block_in0);
    vae_.dec.levels.assign(c.n_mult, VaeLevel{});
    int block_in = block_in0;
    for (int level = c.n_mult - 1; level >= 0; --level) {
        const int block_out = c.ch * c.ch_mult[level];
        for (int i = 0; i <= c.num_res_blocks; ++i) {
            vae_.dec.levels[level].blocks.push_back(resw(V + fmt("decoder.up.%d.block.%d", level, i), block_in, block_out, false));
            block_in = block_out;
        }
        if (level != 0) {
            vae_.dec.levels[level].has_resample = true;
            vae_.dec.levels[level].resample = conv3(V + fmt("decoder.up.%d.upsample.conv", level), 0, true);
        }
    }
    vae_.dec.norm_out = norm(V + "decoder.norm_out");
    vae_.dec.conv_out = conv3(V + "decoder.conv_out", 32);
}

// Encoder of AutoencoderKL (reference model.py:368-459)
void Engine::build_vae_encoder() {
    const gl_vae_config& c = vae_.cfg;
    const std::string V = "vae/";
    vae_.enc.in_small = conv3_small(V + "encoder.conv_in", c.ch);
    vae_.enc.levels.assign(c.n_mult, VaeLevel{});
    int block_in = c.ch;
    for (int level = 0; level < c.n_mult; ++level) {
        const int block_out = c.ch * c.ch_mult[level];
        for (int i = 0; i < c.num_res_blocks; ++i) {
            vae_.enc.levels[level].blocks.push_back(resw(V + fmt("encoder.down.%d.block.%d", level, i), block_in, block_out, false));
            block_in = block_out;
        }
        if (level != c.n_mult - 1) {
            vae_.enc.levels[level].has_resample = true;
            vae_.enc.levels[level].resample = conv3(V + fmt("encoder.down.%d.downsample.conv", level));
        }
    }
    build_vae_mid(vae_.enc, V + "encoder.mid", block_in);
    vae_.enc.norm_out = norm(V + "encoder.norm_out");
    vae_.enc.conv_out = conv3(V + "encoder.conv_out", 32);
    if (vae_.enc.conv_out.Cout != 2 * c.z_channels) throw GlError(GL_ERR_ARG, "encoder.conv_out must produce 2 * z_channels moments");
    const RawTensor& q = raw(V + "quant_conv.weight");
    if (q.shape[0] != 2 * c.z_channels || q.shape[1] != 2 * c.z_channels)
        throw GlError(GL_ERR_UNSUPPORTED, "quant_conv must map 2*z_channels -> 2*z_channels (embed_dim == z_channels)");
    vae_.enc.quant_w = F(V + "quant_conv.weight");
    vae_.enc.quant_b = F(V + "quant_conv.bias");
    vae_.enc.present = true;
}

// ---------------------------------------------------------------- VAE
void Engine::set_vae_attention(int mode) {
    if (mode < 0 || mode > 2) throw GlError(GL_ERR_ARG, fmt("vae attention mode %d: 0 = auto, 1 = score matrices, 2 = flash", mode));
    vae_attn_mode_ = mode;
}

// Does this attention run on vae_attn_flash_kernel? Mode 1 is never replaced; mode 2 refuses a head dimension the kernel lacks; auto keeps
// the score-matrix form -- its launches and its bits -- up to 4096 tokens unless its matrices no longer fit behind the vt_bytes of v^T
bool Engine::vae_attn_flash_for(int mode, int HW, int C, size_t vt_bytes) const {
    if (mode == 1) return false;
    const bool have = vae_attn_flash_supports(C);
    if (mode == 2) {
        if (!have) throw GlError(GL_ERR_UNSUPPORTED, fmt("vae attention: flash form asked for at C=%d channels (vae_attn_flash_kernel is built for 256 and 512)", C));
        return true;
    }
    if (!have) return false;
    if (HW > 4096) return true;
    const size_t need = vt_bytes + (size_t)HW * HW * 6 + 3 * 256, left = arena_.capacity() - arena_.mark();
    return need > left;
}

void Engine::vae_attn_matrix(const bf16* q, const bf16* k, const bf16* vT, const float* vbias, bf16* o, int HW, int C, hipStream_t s) {
    float* S = arena_.get<float>((size_t)HW * HW);
    {
        Epilogue E = e_rows(S, HW);
        E.out_f32 = 1;
        gemm(a_rows(q, C), k, HW, HW, C, E, s);
    }
    bf16* Pm = arena_.get<bf16>((size_t)HW * HW);
    CK(softmax_rows_launch(S, Pm, HW, HW, 1.f / std::sqrt((float)C), s));
    ++n_launches;
    gemm(a_rows(Pm, HW), vT, HW, C, HW, e_rows(o, C, vbias), s);
}

// AttnBlock.forward (model.py:177-202): single head over HW tokens, scale C^-0.5
bf16* Engine::vae_attn(const VaeAttnW& a, const bf16* x, int B, int HW, hipStream_t s) {
    const int C = a.gn.C, M = B * HW;
    if (HW % 64 != 0) throw GlError(GL_ERR_UNSUPPORTED, "VAE attention needs h*w to be a multiple of 64");
    bf16* out = arena_.get<bf16>((size_t)M * C);
    const size_t mk = arena_.mark();
    bf16* n = groupnorm(TRef{x, C, nullptr, 0}, B, HW, a.gn, 1e-6f, false, s);
    bf16* q = linear_rows(n, M, a.q, ACT_NONE, nullptr, nullptr, s);
    bf16* k = linear_rows(n, M, a.k, ACT_NONE, nullptr, nullptr, s);
    bf16* o = arena_.get<bf16>((size_t)M * C);
    // v^T [C][HW] = Wv n_b^T per image (bias folded into the P v product: rows of P sum to 1)
    if (vae_attn_flash_for(vae_attn_mode_, HW, C, (size_t)C * HW * sizeof(bf16))) {
        bf16* vT = arena_.get<bf16>((size_t)M * C);
        for (int b = 0; b < B; ++b) gemm(a_rows(a.v.w, C), n + (size_t)b * HW * C, C, HW, C, e_rows(vT + (size_t)b * HW * C, HW), s);
        ProfScope ps(this, s, "vae_attn_flash_kernel", 4.0 * B * HW * HW * C, 0.0);
        CK(vae_attn_flash_launch(q, k, vT, a.v.b, o, B, HW, C, s));
        ++n_launches;
    } else {
        for (int b = 0; b < B; ++b) {
            const size_t mb = arena_.mark();
            bf16* vT = arena_.get<bf16>((size_t)C * HW);
            gemm(a_rows(a.v.w, C), n + (size_t)b * HW * C, C, HW, C, e_rows(vT, HW), s);
            vae_attn_matrix(q + (size_t)b * HW * C, k + (size_t)b * HW * C, vT, a.v.b, o + (size_t)b * HW * C, HW, C, s);
            arena_.release(mb);
        }
    }
    gemm(a_rows(o, C), a.proj.w, M, C, C, e_rows_res(out, C, a.proj.b, x), s);
    arena_.release(mk);
    return out;
}

void Engine::op_vae_attention(const bf16* q, const bf16* k, const bf16* v, int B, int T, int C, int mode, bf16* o, hipStream_t s) {
    if (mode < 0 || mode > 2) throw GlError(GL_ERR_ARG, fmt("vae attention mode %d: 0 = auto, 1 = score matrices, 2 = flash", mode));
    if (B <= 0 || T <= 0 || T % 64 || C <= 0 || C % 64)
        throw GlError(GL_ERR_UNSUPPORTED, fmt("vae attention: B=%d T=%d C=%d (T and C positive multiples of 64)", B, T, C));
    const size_t mk = arena_.mark();
    struct Release {
        Arena& ar;
        size_t mk;
        ~Release() { ar.release(mk); }   // stream-ordered reuse, as every operator's workspace
    } release{arena_, mk};
    const bool flash = vae_attn_flash_for(mode, T, C, (size_t)B * T * C * sizeof(bf16));
    bf16* vT = arena_.get<bf16>((size_t)B * T * C);
    CK(vae_attn_transpose_launch(v, vT, B, T, C, s));
    ++n_launches;
    if (flash) {
        CK(vae_attn_flash_launch(q, k, vT, nullptr, o, B, T, C, s));
        ++n_launches;
        return;
    }
    const size_t img = (size_t)T * C;
    for (int b = 0; b < B; ++b) {
        const size_t mb = arena_.mark();
        vae_attn_matrix(q + b * img, k + b * img, vT + b * img, nullptr, o + b * img, T, C, s);
        arena_.release(mb);
    }
}

// AutoencoderKL.decode (autoencoder.py:40-44) -> Decoder.forward (model.py:535-568)
void Engine::vae_decode(int B, int h, int w, const float* z, float* out, hipStream_t s) {
    if (!vae_.dec.present || !finalized_) throw GlError(GL_ERR_STATE, "vae not finalized");
    arena_.reset();
    vae_decode_pass(B, h, w, z, out, s);
}

void Engine::vae_decode_pass(int B, int h, int w, const float* z, float* out, hipStream_t s) {
    const gl_vae_config& c = vae_.cfg;
    int H = h, W = w;
    int C = vae_.dec.in_small.Cout;
    Im2colParams P{};
    P.x0 = z; P.C0 = c.z_channels; P.B = B; P.H = H; P.W = W;
    P.pre_w = vae_.dec.quant_w; P.pre_b = vae_.dec.quant_b; P.pre_scale = 1.f / c.scale_factor;   // post_quant_conv and 1 / scale_factor ride in the gather
    bf16* cur = conv3x3_small(vae_.dec.in_small, P, 1, s);
    const float eps = 1e-6f;
    cur = resblock(vae_.dec.mid1, TRef{cur, C, nullptr, 0}, B, H, W, nullptr, 0, eps, s);
    cur = vae_attn(vae_.dec.attn, cur, B, H * W, s);
    cur = resblock(vae_.dec.mid2, TRef{cur, C, nullptr, 0}, B, H, W, nullptr, 0, eps, s);
    for (int level = c.n_mult - 1; level >= 0; --level) {
        for (const ResW& r : vae_.dec.levels[level].blocks) {
            cur = resblock(r, TRef{cur, C, nullptr, 0}, B, H, W, nullptr, 0, eps, s);
            C = r.Cout;
        }
        if (vae_.dec.levels[level].has_resample) {
            cur = conv3x3(TRef{cur, C, nullptr, 0}, B, H, W, vae_.dec.levels[level].resample, 1, 1, 1, nullptr, 0, nullptr, s);
            H *= 2;
            W *= 2;
        }
    }
    gn_silu_conv3x3_nchw(cur, C, B, H, W, vae_.dec.norm_out, eps, vae_.dec.conv_out, c.out_ch, out, s);
}

// AutoencoderKL.encode (autoencoder.py:34-38) -> Encoder.forward (model.py:434-459) -> quant_conv -> posterior sample
void Engine::vae_encode(int B, int H, int W, const float* img, const float* noise, float* z, hipStream_t s) {
    if (!vae_.enc.present || !finalized_) throw GlError(GL_ERR_STATE, "vae encoder weights were not uploaded / not finalized");
    const gl_vae_config& c = vae_.cfg;
    const int total_stride = 1 << (c.n_mult - 1);
    if (H % total_stride || W % total_stride) throw GlError(GL_ERR_ARG, "vae_encode: image size must be divisible by the encoder stride");
    arena_.reset();
    const float* moments = vae_encode_pass(B, H, W, img, nullptr, s);
    vae_posterior(moments, noise, z, B, (H / total_stride) * (W / total_stride), s);
}

void Engine::vae_posterior(const float* moments, const float* noise, float* z, int B, int HW, hipStream_t s) {
    const gl_vae_config& c = vae_.cfg;
    CK(vae_posterior_launch(moments, vae_.enc.quant_w, vae_.enc.quant_b, noise, z, B, c.z_channels, HW, c.scale_factor, s));
    ++n_launches;
}

float* Engine::vae_encode_pass(int B, int H, int W, const float* img, float* moments, hipStream_t s) {
    const gl_vae_config& c = vae_.cfg;
    int C = vae_.enc.in_small.Cout;
    Im2colParams P{};
    P.x0 = img; P.C0 = vae_.enc.in_small.Cin; P.B = B; P.H = H; P.W = W;
    P.pre_scale = 1.f;
    bf16* cur = conv3x3_small(vae_.enc.in_small, P, 1, s);
    const float eps = 1e-6f;
    for (int level = 0; level < c.n_mult; ++level) {
        for (const ResW& r : vae_.enc.levels[level].blocks) {
            cur = resblock(r, TRef{cur, C, nullptr, 0}, B, H, W, nullptr, 0, eps, s);
            C = r.Cout;
        }
        if (vae_.enc.levels[level].has_resample) {
            // Downsample: F.pad(x, (0,1,0,1)) + conv3x3 stride 2 padding 0 (model.py:72-76) = pad_lo 0 in the gather
            cur = conv3x3(TRef{cur, C, nullptr, 0}, B, H, W, vae_.enc.levels[level].resample, 2, 0, 0, nullptr, 0, nullptr, s);
            H /= 2;
            W /= 2;
        }
    }
    cur = resblock(vae_.enc.mid1, TRef{cur, C, nullptr, 0}, B, H, W, nullptr, 0, eps, s);
    cur = vae_attn(vae_.enc.attn, cur, B, H * W, s);
    cur = resblock(vae_.enc.mid2, TRef{cur, C, nullptr, 0}, B, H, W, nullptr, 0, eps, s);
    if (!moments) moments = arena_.get<float>((size_t)B * 2 * c.z_channels * H * W);
    gn_silu_conv3x3_nchw(cur, C, B, H, W, vae_.enc.norm_out, eps, vae_.enc.conv_out, 2 * c.z_channels, moments, s);
    return moments;
}

// ---------------------------------------------------------------- tiled passes (include/gligen_amd_tiling.h)
void Engine::vae_tile_plan_check(const gl_tile_plan& p, int h_in, int w_in, int f, bool decode, int tiles_per_pass, const char* who) const {
    if (p.struct_size != sizeof(gl_tile_plan))
        throw GlError(GL_ERR_ARG, fmt("%s: plan->struct_size is %u, this library's gl_tile_plan has %zu bytes", who, p.struct_size, sizeof(gl_tile_plan)));
    if (tiles_per_pass < 1) throw GlError(GL_ERR_ARG, fmt("%s: tiles_per_pass = %d (at least 1)", who, tiles_per_pass));
    if (p.ny < 1 || p.nx < 1 || p.th_in < 1 || p.tw_in < 1 || p.th_in > h_in || p.tw_in > w_in)
        throw GlError(GL_ERR_ARG, fmt("%s: %d x %d tiles of %d x %d on a %d x %d input", who, p.ny, p.nx, p.th_in, p.tw_in, h_in, w_in));
    const bool scaled = decode ? (p.th_out == p.th_in * f && p.tw_out == p.tw_in * f) : (p.th_in == p.th_out * f && p.tw_in == p.tw_out * f);
    if (!scaled)
        throw GlError(GL_ERR_ARG, fmt("%s: tile %d x %d -> %d x %d does not match the autoencoder's factor %d", who, p.th_in, p.tw_in, p.th_out, p.tw_out, f));
    if (p.ny == 1 && p.nx == 1) {
        if (p.th_in != h_in || p.tw_in != w_in) throw GlError(GL_ERR_ARG, fmt("%s: a single tile must be the whole %d x %d input", who, h_in, w_in));
        return;
    }
    const int th_lat = decode ? p.th_in : p.th_out, tw_lat = decode ? p.tw_in : p.tw_out;
    if ((th_lat * tw_lat) % 64) throw GlError(GL_ERR_UNSUPPORTED, fmt("%s: tile of %d x %d latent pixels: VAE attention needs th * tw to be a multiple of 64", who, th_lat, tw_lat));
    if (!p.windows || !p.oy || !p.ox || !p.wy || !p.wx) throw GlError(GL_ERR_ARG, fmt("%s: null plan table", who));
}

void Engine::vae_decode_tiled(int B, int h, int w, const float* z, float* out, const gl_tile_plan& p, int tiles_per_pass, hipStream_t s) {
    if (!vae_.dec.present || !finalized_) throw GlError(GL_ERR_STATE, "vae not finalized");
    const gl_vae_config& c = vae_.cfg;
    const int f = 1 << (c.n_mult - 1);
    vae_tile_plan_check(p, h, w, f, true, tiles_per_pass, "vae_decode_tiled");
    if (p.ny == 1 && p.nx == 1) return vae_decode(B, h, w, z, out, s);
    const int total = B * p.ny * p.nx;
    const TileBlendPlan bp{p.ny, p.nx, p.th_out, p.tw_out, p.oy, p.ox, p.wy, p.wx};
    for (int t0 = 0; t0 < total; t0 += tiles_per_pass) {
        const int n = std::min(tiles_per_pass, total - t0);
        arena_.reset();
        float* zt = arena_.get<float>((size_t)n * c.z_channels * p.th_in * p.tw_in);
        float* it = arena_.get<float>((size_t)n * c.out_ch * p.th_out * p.tw_out);
        CK(tile_gather_launch(z, B, c.z_channels, h, w, p.windows + 3 * (size_t)t0, n, zt, p.th_in, p.tw_in, s));
        ++n_launches;
        vae_decode_pass(n, p.th_in, p.tw_in, zt, it, s);
        CK(tile_blend_launch(it, t0, n, bp, out, B, c.out_ch, h * f, w * f, s));
        ++n_launches;
    }
}

void Engine::vae_encode_tiled(int B, int H, int W, const float* img, const float* noise, float* z, float* moments_out, const gl_tile_plan& p,
                              int tiles_per_pass, hipStream_t s) {
    if (!vae_.enc.present || !finalized_) throw GlError(GL_ERR_STATE, "vae encoder weights were not uploaded / not finalized");
    const gl_vae_config& c = vae_.cfg;
    const int f = 1 << (c.n_mult - 1);
    if (H % f || W % f) throw GlError(GL_ERR_ARG, "vae_encode: image size must be divisible by the encoder stride");
    vae_tile_plan_check(p, H, W, f, false, tiles_per_pass, "vae_encode_tiled");
    const int h = H / f, w = W / f, Cin = vae_.enc.in_small.Cin, Cm = 2 * c.z_channels;
    arena_.reset();
    if (p.ny == 1 && p.nx == 1) {                                 // the untiled call; its moments land where the caller wants them
        const float* m = vae_encode_pass(B, H, W, img, moments_out, s);
        return vae_posterior(m, noise, z, B, h * w, s);
    }
    float* moments = moments_out ? moments_out : arena_.get<float>((size_t)B * Cm * h * w);
    const size_t base = arena_.mark();                            // the passes' reset: everything above the blended moments
    const int total = B * p.ny * p.nx;
    const TileBlendPlan bp{p.ny, p.nx, p.th_out, p.tw_out, p.oy, p.ox, p.wy, p.wx};
    for (int t0 = 0; t0 < total; t0 += tiles_per_pass) {
        const int n = std::min(tiles_per_pass, total - t0);
        arena_.release(base);
        float* it = arena_.get<float>((size_t)n * Cin * p.th_in * p.tw_in);
        float* mt = arena_.get<float>((size_t)n * Cm * p.th_out * p.tw_out);
        CK(tile_gather_launch(img, B, Cin, H, W, p.windows + 3 * (size_t)t0, n, it, p.th_in, p.tw_in, s));
        ++n_launches;
        vae_encode_pass(n, p.th_in, p.tw_in, it, mt, s);
        CK(tile_blend_launch(mt, t0, n, bp, moments, B, Cm, h, w, s));
        ++n_launches;
    }
    vae_posterior(moments, noise, z, B, h * w, s);
}

}  // namespace gl
