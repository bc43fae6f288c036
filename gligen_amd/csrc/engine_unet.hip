// gligen_amd engine -- UNetModel.forward: weight packing of the UNet, the transformer block and its fuser variants, conditioning
#include "engine_impl.h"
#include <algorithm>
#include <cmath>

namespace gl {

void Engine::configure_unet(const gl_unet_config& c) {
    if (c.n_mult < 1 || c.n_mult > 8 || c.n_attn < 0 || c.n_attn > 8) throw GlError(GL_ERR_ARG, "bad unet config");
    if (c.model_channels % 64 != 0) throw GlError(GL_ERR_UNSUPPORTED, "model_channels must be a multiple of 64");
    if (c.fuser_kind < 0 || c.fuser_kind > 2) throw GlError(GL_ERR_ARG, "fuser_kind: 0 gatedSA, 1 gatedSA2, 2 gatedCA");
    if (c.extra_channels < 0 || c.extra_channels > 64) throw GlError(GL_ERR_ARG, "extra_channels out of range");
    // openaimodel.py:446-447 is a breakpoint() in the reference: no shipped model combines the two
    if (c.extra_channels && c.inpaint_mode) throw GlError(GL_ERR_UNSUPPORTED, "inpaint_mode with a grounding downsampler is undefined in the reference");
    unet_.cfg = c;
    unet_.present = true;
}

void Engine::build_unet() {
    const gl_unet_config& c = unet_.cfg;
    const int mc = c.model_channels;
    const std::string U = "unet/";
    auto in_attn = [&](int ds) {
        for (int i = 0; i < c.n_attn; ++i)
            if (c.attention_resolutions[i] == ds) return true;
        return false;
    };
    unet_.te0 = linear(U + "time_embed.0");
    unet_.te2 = linear(U + "time_embed.2");

    // first conv through the small-channel im2col path (K = 9*in_c padded to 64)
    {
        const int in_c = (int)raw(U + "input_blocks.0.0.weight").shape[1];
        const int expect = c.inpaint_mode ? 2 * c.in_channels + 1 : c.in_channels + c.extra_channels;
        if (in_c != expect) throw GlError(GL_ERR_ARG, fmt("first conv has %d input channels, config implies %d", in_c, expect));
        unet_.conv_in_small = conv3_small(U + "input_blocks.0.0", mc);
        float* bcopy = reinterpret_cast<float*>(persist(mc * sizeof(float), false));  // engine-owned: restorable
        HIPCK(hipMemcpy(bcopy, unet_.conv_in_small.b, mc * sizeof(float), hipMemcpyDeviceToDevice));
        unet_.conv_in_small.b = bcopy;
    }

    std::vector<std::string> emb_keys;
    std::vector<const float*> emb_bias;
    std::vector<int> emb_n;
    int emb_total = 0;
    auto add_res = [&](const std::string& p, int Cin, int Cout) {
        ResW r = resw(p, Cin, Cout, true);
        r.emb_off = emb_total;
        emb_keys.push_back(p + ".emb_layers.1.weight");
        emb_bias.push_back(F(p + ".emb_layers.1.bias"));
        emb_n.push_back(Cout);
        emb_total += Cout;
        unet_.res.push_back(r);
        return Layer{L_RES, (int)unet_.res.size() - 1};
    };
    auto add_st = [&](const std::string& p, int C) {
        STW t;
        t.C = C;
        t.d = C / c.num_heads;
        t.idx = (int)unet_.st.size();
        int dp, dpv;
        CK(attn_dims(t.d, &dp, &dpv));
        const std::string tb = p + ".transformer_blocks.0";
        t.gn = norm(p + ".norm");
        t.proj_in = conv1(p + ".proj_in");
        t.proj_out = conv1(p + ".proj_out");
        t.ln1 = norm(tb + ".norm1");
        t.ln2 = norm(tb + ".norm2");
        t.ln3 = norm(tb + ".norm3");
        // q, k and v^T of a self-attention come out of ONE GEMM over the LayerNorm'ed rows (EPI_QKV_HEADS) when the head
        // count / width allow it; GL_QKV_FUSED=0 keeps the two-launch form (q,k GEMM + operand-swapped v^T GEMM) for A/B runs
        const bool want_fused = !(dev_env("GL_QKV_FUSED") && atoi(dev_env("GL_QKV_FUSED")) == 0);
        const bool fuse_qkv = want_fused && gemm_supports_qkv() && (2 * C) % 128 == 0;
        // LayerNorms folded into the projections behind them (gemm.h Epilogue::ln_stats; GL_LN_FOLD=0: the LayerNorm kernels of
        // rounds 1-2): norm1 -> attn1 q,k,v; fuser.norm1 -> fuser q,k,v; fuser.norm2 -> fuser.ff; norm2 -> attn2.to_q; norm3 -> ff
        const bool fold = fuse_qkv && !(dev_env("GL_LN_FOLD") && atoi(dev_env("GL_LN_FOLD")) == 0);
        ln_fold_ = fold;
        ff_rows_ = !(dev_env("GL_FF_ROWS") && atoi(dev_env("GL_FF_ROWS")) == 0);   // row-local feed-forward kernel (ffn.hip) where it exists
        ff_chain_ = dev_env("GL_FF_CHAIN") ? atoi(dev_env("GL_FF_CHAIN")) : 3;
        fuser_hoist_ = !(dev_env("GL_FUSER_KV_HOIST") && atoi(dev_env("GL_FUSER_KV_HOIST")) == 0);
        qkv_rows_ = dev_env("GL_QKV_ROWS") ? atoi(dev_env("GL_QKV_ROWS")) : 1;
        // pre_key: weight of the C x C projection in front of this attention's LayerNorm (row-local form, ffn.h qkv_rows_kernel)
        auto self_attn_w = [&](const std::string& a, const NormW* ln, const std::string& pre_key) {
            SelfAttnW w;
            w.fused = fuse_qkv;
            if (fuse_qkv && ln) {
                const char* names[3] = {".to_q.weight", ".to_k.weight", ".to_v.weight"};
                bf16* dst = reinterpret_cast<bf16*>(persist((size_t)3 * C * C * sizeof(bf16), false));
                float* bias = reinterpret_cast<float*>(persist((size_t)3 * C * sizeof(float), false));
                float* cs = reinterpret_cast<float*>(persist((size_t)3 * C * sizeof(float), false));
                for (int i = 0; i < 3; ++i) {
                    const FoldTmp t = fold_ln(a + names[i], nullptr, *ln);
                    if (t.N != C || t.K != C) throw GlError(GL_ERR_ARG, "'" + a + "': q / k / v projections must be C x C");
                    CK(cast_f32_bf16_launch(t.w, dst + (size_t)i * C * C, (int64_t)C * C, 0));
                    HIPCK(hipMemcpy(bias + (size_t)i * C, t.b, C * sizeof(float), hipMemcpyDeviceToDevice));
                }
                CK(rowsum_bf16_launch(dst, cs, 3 * C, C, 0));
                w.wqk = dst; w.b = bias; w.csum = cs; w.folded = true;
                if (qkv_rows_ && !pre_key.empty() && t.d == 40 && qkv_rows_stream_bytes(C, true, 3)) {
                    void* st = persist(qkv_rows_stream_bytes(C, true, 3), false);
                    CK(qkv_rows_pack_launch(raw(pre_key).p, dst, 3, st, C, 0));
                    w.rows_stream = st;
                }
            } else if (fuse_qkv) {
                w.wqk = cast_rows({a + ".to_q.weight", a + ".to_k.weight", a + ".to_v.weight"});
            } else {
                w.wqk = cast_rows({a + ".to_q.weight", a + ".to_k.weight"});
                w.wv = cast_rows({a + ".to_v.weight"});
            }
            return w;
        };
        t.a1 = self_attn_w(tb + ".attn1", fold ? &t.ln1 : nullptr, p + ".proj_in.weight");
        t.a1.out = linear(tb + ".attn1.to_out.0");
        FoldTmp qfold;
        if (fold) {
            const FoldTmp q = fold_ln(tb + ".attn2.to_q.weight", nullptr, t.ln2);
            qfold = q;
            bf16* dst = reinterpret_cast<bf16*>(persist((size_t)q.N * q.K * sizeof(bf16), false));
            float* bias = reinterpret_cast<float*>(persist((size_t)q.N * sizeof(float), false));
            float* cs = reinterpret_cast<float*>(persist((size_t)q.N * sizeof(float), false));
            CK(cast_f32_bf16_launch(q.w, dst, (int64_t)q.N * q.K, 0));
            HIPCK(hipMemcpy(bias, q.b, q.N * sizeof(float), hipMemcpyDeviceToDevice));
            CK(rowsum_bf16_launch(dst, cs, q.N, q.K, 0));
            t.a2.q.w = dst; t.a2.q.b = bias; t.a2.q.N = q.N; t.a2.q.K = q.K;
            t.a2.q_csum = cs; t.a2.folded = true;
        } else {
            t.a2.q = linear(tb + ".attn2.to_q", false);
        }
        t.a2.wk = cast_rows({tb + ".attn2.to_k.weight"});
        t.a2.wv = cast_rows({tb + ".attn2.to_v.weight"});
        t.a2.ctx_dim = (int)raw(tb + ".attn2.to_k.weight").shape[1];
        t.a2.out = linear(tb + ".attn2.to_out.0");
        t.ff = ffw(tb + ".ff", C, fold ? &t.ln3 : nullptr, ff_chain_ >= 1 ? tb + ".attn2.to_out.0.weight" : "", ff_chain_ >= 1 ? p + ".proj_out.weight" : "");
        if (has(tb + ".fuser.linear.weight") != (c.fuser_kind != 2))
            throw GlError(GL_ERR_ARG, "fuser weights do not match fuser_kind (gatedSA has fuser.linear, gatedCA does not)");
        t.fn1 = norm(tb + ".fuser.norm1");
        t.fn2 = norm(tb + ".fuser.norm2");
        if (c.fuser_kind != 2) {  // gatedSA and gatedSA2 hold the same parameters
            t.flin = linear(tb + ".fuser.linear");
            t.fa = self_attn_w(tb + ".fuser.attn", fold ? &t.fn1 : nullptr, tb + ".attn1.to_out.0.weight");
            t.fa.out = linear(tb + ".fuser.attn.to_out.0");
        } else {  // gatedCA: CrossAttention(query_dim, key_dim = value_dim = grounding-token dim) -- attention.py:194
            t.fca.q = linear(tb + ".fuser.attn.to_q", false);
            t.fca.wk = cast_rows({tb + ".fuser.attn.to_k.weight"});
            t.fca.wv = cast_rows({tb + ".fuser.attn.to_v.weight"});
            t.fca.ctx_dim = (int)raw(tb + ".fuser.attn.to_k.weight").shape[1];
            if (t.fca.ctx_dim != c.gr_out_dim || (int)raw(tb + ".fuser.attn.to_v.weight").shape[1] != c.gr_out_dim)
                throw GlError(GL_ERR_ARG, "gatedCA: fuser.attn key / value dim must equal the grounding-token dim");
            t.fca.out = linear(tb + ".fuser.attn.to_out.0");
        }
        const bool chain_q = ff_chain_ >= 3 && c.fuser_kind == 0 && fold && t.d == 40 && qfold.N == C && qfold.K == C;
        t.fff = ffw(tb + ".fuser.ff", C, fold ? &t.fn2 : nullptr, (ff_chain_ >= 2 && c.fuser_kind == 0) ? tb + ".fuser.attn.to_out.0.weight" : "", "",
                    chain_q ? qfold.w : nullptr, chain_q ? qfold.b : nullptr);
        raw(tb + ".fuser.alpha_attn");
        raw(tb + ".fuser.alpha_dense");
        unet_.st.push_back(t);
        return Layer{L_ST, t.idx};
    };

    std::vector<std::string> st_prefix;  // for alpha pointer table
    unet_.in_blocks.clear();
    unet_.in_blocks.push_back(UNetBlock{{Layer{L_CONV_IN, 0}}});
    std::vector<int> chans{mc};
    int ch = mc, ds = 1, n = 1;
    for (int level = 0; level < c.n_mult; ++level) {
        const int mult = c.channel_mult[level];
        for (int r = 0; r < c.num_res_blocks; ++r) {
            UNetBlock b;
            const std::string p = U + fmt("input_blocks.%d", n);
            b.layers.push_back(add_res(p + ".0", ch, mult * mc));
            ch = mult * mc;
            if (in_attn(ds)) {
                b.layers.push_back(add_st(p + ".1", ch));
                st_prefix.push_back(p + ".1");
            }
            unet_.in_blocks.push_back(b);
            chans.push_back(ch);
            ++n;
        }
        if (level != c.n_mult - 1) {
            unet_.updown.push_back(conv3(U + fmt("input_blocks.%d.0.op", n)));
            unet_.in_blocks.push_back(UNetBlock{{Layer{L_DOWN, (int)unet_.updown.size() - 1}}});
            chans.push_back(ch);
            ds *= 2;
            ++n;
        }
    }
    unet_.mid_block.layers.clear();
    unet_.mid_block.layers.push_back(add_res(U + "middle_block.0", ch, ch));
    unet_.mid_block.layers.push_back(add_st(U + "middle_block.1", ch));
    st_prefix.push_back(U + "middle_block.1");
    unet_.mid_block.layers.push_back(add_res(U + "middle_block.2", ch, ch));

    unet_.out_blocks.clear();
    n = 0;
    for (int level = c.n_mult - 1; level >= 0; --level) {
        const int mult = c.channel_mult[level];
        for (int i = 0; i <= c.num_res_blocks; ++i) {
            const int ich = chans.back();
            chans.pop_back();
            UNetBlock b;
            const std::string p = U + fmt("output_blocks.%d", n);
            b.layers.push_back(add_res(p + ".0", ch + ich, mc * mult));
            ch = mc * mult;
            int j = 1;
            if (in_attn(ds)) {
                b.layers.push_back(add_st(p + ".1", ch));
                st_prefix.push_back(p + ".1");
                j = 2;
            }
            if (level && i == c.num_res_blocks) {
                unet_.updown.push_back(conv3(p + fmt(".%d.conv", j), 0, true));
                b.layers.push_back(Layer{L_UP, (int)unet_.updown.size() - 1});
                ds /= 2;
            }
            unet_.out_blocks.push_back(b);
            ++n;
        }
    }
    unet_.out_norm = norm(U + "out.0");
    unet_.out_conv = conv3(U + "out.2", 32);
    if (unet_.out_conv.Cout != c.out_channels) throw GlError(GL_ERR_ARG, "out conv channels do not match out_channels");

    // all emb_layers in one GEMM
    unet_.embcat.w = cast_rows(emb_keys);
    unet_.embcat.K = 4 * mc;
    unet_.embcat.N = emb_total;
    {
        float* b = reinterpret_cast<float*>(persist(emb_total * sizeof(float), false));
        int off = 0;
        for (size_t i = 0; i < emb_bias.size(); ++i) {
            HIPCK(hipMemcpy(b + off, emb_bias[i], emb_n[i] * sizeof(float), hipMemcpyDeviceToDevice));
            off += emb_n[i];
        }
        unet_.embcat.b = b;
    }

    // fuser gates
    {
        std::vector<const float*> ptrs;
        for (auto& p : st_prefix) {
            ptrs.push_back(F(p + ".transformer_blocks.0.fuser.alpha_attn"));
            ptrs.push_back(F(p + ".transformer_blocks.0.fuser.alpha_dense"));
        }
        void* d = persist(ptrs.size() * sizeof(float*), false);
        HIPCK(hipMemcpy(d, ptrs.data(), ptrs.size() * sizeof(float*), hipMemcpyHostToDevice));
        unet_.alpha_ptrs = reinterpret_cast<const float* const*>(d);
        gates_ = reinterpret_cast<float*>(persist(ptrs.size() * sizeof(float), true));
        fuser_scale_ = reinterpret_cast<float*>(persist(unet_.st.size() * sizeof(float), true));   // one scale per fuser
        CK(fill_f32_launch(fuser_scale_, 1.f, (int)unet_.st.size(), 0));
    }

    // grounding tokenizer (position_net)
    unet_.gkind = c.grounding_kind;
    const std::string PN = U + "position_net.";
    if (unet_.gkind == 0) {
        for (int i = 0; i < 3; ++i) unet_.pn[0][i] = linear(PN + fmt("linears.%d", 2 * i));
        unet_.pn_null_feat[0] = F(PN + "null_positive_feature");
        unet_.pn_null_pos = F(PN + "null_position_feature");
    } else if (unet_.gkind == 1) {
        for (int i = 0; i < 3; ++i) {
            unet_.pn[0][i] = linear(PN + fmt("linears_text.%d", 2 * i));
            unet_.pn[1][i] = linear(PN + fmt("linears_image.%d", 2 * i));
        }
        unet_.pn_null_feat[0] = F(PN + "null_text_feature");
        unet_.pn_null_feat[1] = F(PN + "null_image_feature");
        unet_.pn_null_pos = F(PN + "null_position_feature");
    } else if (unet_.gkind == 2) {
        for (int i = 0; i < 3; ++i) unet_.pn[0][i] = linear(PN + fmt("linears.%d", 2 * i));
        unet_.pn_null_feat[0] = F(PN + "null_person_feature");
        unet_.pn_null_pos = F(PN + "null_xy_feature");
        // person_embeddings[p] + keypoint_embeddings[j] (keypoint_grounding_net.py:39-42)
        const RawTensor& pe = raw(PN + "person_embeddings");
        const RawTensor& ke = raw(PN + "keypoint_embeddings");
        const int P = (int)pe.shape[0], D = (int)pe.shape[1];
        std::vector<float> hp(pe.numel), hk(ke.numel), tab((size_t)P * 17 * D);
        HIPCK(hipMemcpy(hp.data(), pe.p, pe.numel * sizeof(float), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(hk.data(), ke.p, ke.numel * sizeof(float), hipMemcpyDeviceToHost));
        for (int p = 0; p < P; ++p)
            for (int j = 0; j < 17; ++j)
                for (int k = 0; k < D; ++k) tab[((size_t)p * 17 + j) * D + k] = hp[(size_t)p * D + k] + hk[(size_t)j * D + k];
        float* d = reinterpret_cast<float*>(persist(tab.size() * sizeof(float), false));
        HIPCK(hipMemcpy(d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
        unet_.kp_table = d;
    } else if (unet_.gkind == 3) {
        // spatial-map modalities (canny / hed / depth / normal / sem _grounding_net.py): tokens arrive through
        // gl_grounding.tokens; they are the output of gl_op_spatial_tokens (the ConvNeXt tokenizer below, built when its
        // weights were uploaded) or were computed elsewhere
        if (has(PN + "convnext_tiny_backbone.downsample_layers.0.0.weight")) build_convnext(PN);
    } else {
        throw GlError(GL_ERR_UNSUPPORTED, "grounding_kind must be 0 (text), 1 (text+image), 2 (keypoint) or 3 (precomputed tokens)");
    }
}

// SelfAttention.forward (attention.py:167-186) on LayerNorm'ed rows ln [B][T][C] (T % 64 == 0,
// rows >= Nk are zero), queries = first Nq rows, keys/values = first Nk rows.
void Engine::fuser_kv_fill(const STW& t, int B, int HW, hipStream_t s) {
    const int Ng = cond_.Ng, C = t.C, d = t.d, H = C / d;
    const int Ng64 = round_up(Ng, 64), Tf = HW + Ng64;
    int dp, dpv;
    CK(attn_dims(d, &dp, &dpv));
    const int vt_layout = attn_vt_layout(d, HW + Ng, &dpv);
    AttnBufs& bufs = attn_bufs(B, H, d, Tf, Tf, dpv, t.idx + 1);
    const size_t mk = arena_.mark();
    // LayerNorm of the grounding-token rows alone (per row: what the [x ; objs] pass computed for them), no affine: gamma / beta live in
    // the folded q,k,v weights; rows Ng .. Ng64 - 1 of every sample are zero and land behind the last key
    bf16* lno = arena_.get<bf16>((size_t)B * Ng64 * C);
    {
        LNParams P{};
        P.x = cond_.objs[t.idx]; P.B = B; P.N1 = Ng; P.N2 = 0; P.Tpad = Ng64; P.C = C; P.eps = 1e-5f; P.y = lno;
        CK(layernorm_launch(P, s));
    }
    Epilogue E = e_heads(EPI_QKV_HEADS, bufs.q, bufs.k, C, H, d, dp, Ng64, bufs.Tq_pad, bufs.Tk_pad);
    E.vt = bufs.vt; E.DPV = dpv; E.tok_off = HW; E.vt_perm32 = vt_layout;
    E.bias = t.fa.b;          // W beta of the folded LayerNorm
    // Its q rows land behind the last query, and the K / V^T rows Ng .. Ng64 - 1 hold the bias W beta, not zero: where they share a
    // query block or key tile with real rows the attention kernels load them, without effect on the real rows -- the query guard and the
    // `kv >= Nk` mask alone keep them out (include/gligen_amd_attention_core.h; tests/test_attention_core_gpu.py fills both places)
    CK(gemm_launch(a_rows(lno, C), t.fa.wqk, B * Ng64, 3 * C, C, E, ws_, ws_bytes_, s));
    arena_.release(mk);
    if (fuser_kv_.size() < unet_.st.size()) fuser_kv_.resize(unet_.st.size());
    fuser_kv_[t.idx] = FuserKV{cond_epoch_, B, HW};
}

bool Engine::qkv_rows_ok(const SelfAttnW& a, int B, int T, int Nk, int C, int d) const {
    if (!qkv_rows_ || !a.rows_stream || !a.fused || !a.folded || !qkv_rows_supported(B * T, C, d, T)) return false;
    int dpv = 0;
    return attn_vt_layout(d, Nk, &dpv) == 1;                     // the kernel writes V^T in the 32-token form of attn3_kernel only
}

void Engine::qkv_rows_project(const SelfAttnW& a, const bf16* x, int B, int T, int Nk, int C, int d, const LinW& pre, const bf16* pre_res, bf16* mid,
                              RowStats* mid_stats, int Tbuf, int slot, hipStream_t s, int Bin) {
    const int H = C / d, M = B * T;
    if (Bin < 0 || (Bin && B % Bin != 0)) throw GlError(GL_ERR_STATE, fmt("qkv_rows_project: %d input samples for a batch of %d", Bin, B));
    int dp, dpv;
    CK(attn_dims(d, &dp, &dpv));
    const int vt_layout = attn_vt_layout(d, Nk, &dpv);
    AttnBufs& bufs = attn_bufs(B, H, d, Tbuf ? Tbuf : T, Tbuf ? Tbuf : T, dpv, slot);
    QkvRowsParams P{};
    P.x = x; P.ldx = C; P.eps = 1e-5f; P.stream = a.rows_stream; P.M = M;
    P.in_period = (Bin && Bin != B) ? Bin * T : 0;
    P.pre = 1; P.pre_b = pre.b; P.pre_res = pre_res; P.ld_pre_res = C; P.mid_out = mid; P.ld_mid = C;
    if (mid_stats) {
        *mid_stats = RowStats{};
        if (ln_fold_) {
            mid_stats->ld = 1; mid_stats->nb = 1;
            mid_stats->p = arena_.get<float2>((size_t)M);
            P.stats_out = mid_stats->p;
        }
    }
    P.np = 3; P.bias = a.b; P.q = bufs.q; P.k = bufs.k; P.vt = bufs.vt;
    P.H = H; P.d = d; P.DP = dp; P.DPV = dpv; P.T = T; P.Tpad_q = bufs.Tq_pad; P.Tpad_k = bufs.Tk_pad; P.vt_perm32 = vt_layout;
    ProfScope ps(this, s, "qkv_rows_kernel<pre, 3>", 8.0 * M * (double)C * C, 0.0);
    CK(qkv_rows_launch(P, C, s));
    FILE* launch_log = launch_log_file();
    if (launch_log) {
        fprintf(launch_log, "qkv_rows_kernel<320, 40, true, 3>|%d|%d|%d|0|%.0f\n", M, 4 * C, C,
                (double)qkv_rows_stream_bytes(C, true, 3) + (pre_res ? 6.0 : 4.0) * M * C + 2.0 * M * H * (2.0 * dp + dpv));
        fflush(launch_log);
    }
    ++n_launches;
}

void Engine::self_attention(const SelfAttnW& a, const bf16* ln, int B, int T, int Nq, int Nk, int C, int d, bf16* o, hipStream_t s,
                            const RowStats* in_stats, int Tbuf, int slot, bool projected) {
    const int H = C / d;
    int dp, dpv;
    CK(attn_dims(d, &dp, &dpv));
    const int vt_layout = attn_vt_layout(d, Nk, &dpv);    // which V^T form the attention kernel for this (d, Nk) reads
    AttnBufs& bufs = attn_bufs(B, H, d, Tbuf ? Tbuf : T, Tbuf ? Tbuf : T, dpv, slot);
    if (in_stats && !(a.fused && a.folded)) throw GlError(GL_ERR_STATE, "self_attention: row statistics given to an unfolded projection");
    if (!projected) qkv_project_gemm(a, ln, B, T, Nk, C, d, s, in_stats, Tbuf, slot);
    attention(bufs.q, bufs.k, bufs.vt, o, B, H, d, Nq, Nk, bufs.Tq_pad, bufs.Tk_pad, vt_layout, s);
}

// q, k, v^T of a self-attention by GEMM: the fused EPI_QKV_HEADS launch (or the q,k GEMM + operand-swapped v^T GEMM)
void Engine::qkv_project_gemm(const SelfAttnW& a, const bf16* ln, int B, int T, int Nk, int C, int d, hipStream_t s, const RowStats* in_stats, int Tbuf, int slot) {
    const int H = C / d;
    int dp, dpv;
    CK(attn_dims(d, &dp, &dpv));
    const int vt_layout = attn_vt_layout(d, Nk, &dpv);
    AttnBufs& bufs = attn_bufs(B, H, d, Tbuf ? Tbuf : T, Tbuf ? Tbuf : T, dpv, slot);
    if (a.fused) {
        Epilogue E = e_heads(EPI_QKV_HEADS, bufs.q, bufs.k, C, H, d, dp, T, bufs.Tq_pad, bufs.Tk_pad);
        E.vt = bufs.vt; E.DPV = dpv; E.vt_perm32 = vt_layout;
        if (a.folded) E.bias = a.b;      // W beta of the folded LayerNorm (to_q / to_k / to_v have no bias of their own)
        if (in_stats) e_fold_ln(E, *in_stats, a.csum, C);   // `ln` holds the raw rows: (x - mean) * rstd happens in the epilogue
        gemm(a_rows(ln, C), a.wqk, B * T, 3 * C, C, E, s);
    } else {
        gemm(a_rows(ln, C), a.wqk, B * T, 2 * C, C, e_heads(EPI_QK_HEADS, bufs.q, bufs.k, C, H, d, dp, T, bufs.Tq_pad, bufs.Tk_pad), s);
        Epilogue E;
        epilogue_defaults(E);
        E.mode = EPI_VT_HEADS;
        E.out = bufs.vt; E.H = H; E.d = d; E.DPV = dpv; E.T = T; E.Tpad_k = bufs.Tk_pad; E.vt_perm32 = vt_layout;
        ProfScope ps(this, s, "gemm", 2.0 * C * (double)B * T * C, 0.0);
        CK(gemm_launch_t(a.wv, C, ln, B * T, C, E, s));
        if (profiling_) ps.rename(gemm_last_kernel_name());
        ++n_launches;
    }
}

bf16* Engine::feedforward_chain(const FFW& f, const bf16* x, int M, const LinW& pre, const bf16* pre_res, const float* pre_gate, const float* gate,
                                const LinW* post, const bf16* post_res, bf16* out, hipStream_t s, RowStats* out_stats, const ChainQ* cq) {
    const int C = f.C;
    if (!f.chain_stream || !ff_rows_supported(M, C) || (post != nullptr) != f.chain_post || (cq && (post || !f.chain_q_stream)))
        throw GlError(GL_ERR_STATE, "feedforward_chain: no chained stream of this shape");
    if (!out) out = arena_.get<bf16>((size_t)M * C);
    FFRowsParams P{};
    P.x = x; P.ldx = C; P.normalize = 1; P.eps = 1e-5f; P.stream = f.chain_stream; P.b2 = f.w2.b; P.gate = gate; P.out = out; P.ldo = C; P.M = M;
    P.pre = 1; P.pre_b = pre.b; P.pre_res = pre_res; P.ld_pre_res = C; P.pre_gate = pre_gate;
    P.mid_out = arena_.get<bf16>((size_t)M * C);     // (only written when the gate is too small for the residual to ride in the accumulator)
    P.ld_mid = C;
    if (post) { P.post = 1; P.post_b = post->b; P.post_res = post_res; P.ld_post_res = C; }
    if (cq) { P.post = 2; P.stream = f.chain_q_stream; P.post_b = f.chain_q_bias; P.q = cq->q; P.qDP = cq->DP; P.qT = cq->T; P.qTpad = cq->Tpad; }
    if (out_stats) {
        *out_stats = RowStats{};
        if (ln_fold_) {
            out_stats->ld = 1; out_stats->nb = 1;
            out_stats->p = arena_.get<float2>((size_t)M);
            P.stats_out = out_stats->p; P.stats_ld = 1;
        }
    }
    ProfScope ps(this, s, post ? "ff_rows_kernel<pre, post>" : cq ? "ff_rows_kernel<pre, to_q>" : "ff_rows_kernel<pre>", (24.0 + ((post || cq) ? 4.0 : 2.0)) * M * (double)C * C, 0.0);
    CK(ff_rows_launch(P, C, s));
    FILE* launch_log = launch_log_file();
    if (launch_log) {
        fprintf(launch_log, "ff_rows_kernel<320, 0, true, %d>|%d|%d|%d|0|%.0f\n", post ? 1 : cq ? 2 : 0, M, C, 4 * C,
                (double)ff_chain_stream_bytes(C, true, post != nullptr || cq != nullptr) + (post ? 8.0 : 6.0) * M * C + (cq ? 2.0 * M * (C / 40) * cq->DP : 0.0));   // (the symbol as rocprofv3 prints it: pmc_summarize.py joins on it)
        fflush(launch_log);
    }
    ++n_launches;
    return out;
}

bool Engine::can_fold(const RowStats& st, int M, int C, int Nc, int mode, int act, bool aligned) {
    if (!st.nb || !aligned) return false;
    Epilogue E;
    epilogue_defaults(E);
    E.mode = mode; E.act = act; E.geglu16 = gemm_geglu_layout();
    return gemm_ln_fold_supported(a_rows(nullptr, C), M, Nc, C, E);
}

// LayerNorm + feed-forward (+ gated residual) behind a projection that produced rows_in (statistics st_in, if it wrote any)
bf16* Engine::ff_behind(const FFW& f, const NormW& nw, const bf16* rows_in, RowStats& st_in, int B, int HW, const float* gate, bool rows, hipStream_t s,
                        RowStats* out_stats) {
    const int M = B * HW, C = f.C;
    const bool fold = rows || (f.folded && can_fold(st_in, M, C, 8 * C, EPI_ROWMAJOR, ACT_GEGLU, round_up(HW, 64) == HW));
    const bf16* ln = fold ? rows_in : (f.folded ? layernorm_plain(rows_in, B, HW, C, false, s) : layernorm(rows_in, B, HW, C, nw, false, s));
    return feedforward(f, ln, M, rows_in, gate, s, (fold && !rows) ? &st_in : nullptr, out_stats, rows, rows);
}

bf16* Engine::fuser_ff_tail(const STW& t, const bf16* o, const bf16* t1, int B, int HW, bool rows, hipStream_t s, RowStats* st3, bool* q_done) {
    const int M = B * HW;
    const float* g_attn = gates_ + 2 * t.idx;
    if (q_done) *q_done = false;
    if (rows && t.fff.chain_stream && !t.fff.chain_post) {   // one row-local launch for the three
        if (q_done && t.fff.chain_q_stream && t.a2.folded && HW % 128 == 0) {
            // ... and attn2.to_q(norm2(.)) behind them: the cross-attention's q buffer is filled by the same launch
            int dp, dpv;
            CK(attn_dims(t.d, &dp, &dpv));
            AttnBufs& bufs = attn_bufs(B, t.C / t.d, t.d, HW, cond_.ctx_Tpad);
            const ChainQ cq{bufs.q, dp, HW, bufs.Tq_pad};
            *q_done = true;
            return feedforward_chain(t.fff, o, M, t.fa.out, t1, g_attn, g_attn + 1, nullptr, nullptr, nullptr, s, st3, &cq);
        }
        return feedforward_chain(t.fff, o, M, t.fa.out, t1, g_attn, g_attn + 1, nullptr, nullptr, nullptr, s, st3);
    }
    RowStats st2;
    bf16* t2 = linear_rows(o, M, t.fa.out, ACT_NONE, t1, g_attn, s, rows ? nullptr : &st2);
    return ff_behind(t.fff, t.fn2, t2, st2, B, HW, g_attn + 1, rows, s, st3);
}

void Engine::block_ff_tail(const STW& t, const bf16* o, const bf16* t3, const bf16* x, bf16* out, int B, int HW, bool rows, hipStream_t s) {
    const int M = B * HW, C = t.C;
    if (rows && t.ff.chain_stream && t.ff.chain_post) {   // attn2.to_out + residual, LayerNorm, ff + residual, proj_out + x_in: one row-local launch
        feedforward_chain(t.ff, o, M, t.a2.out, t3, nullptr, nullptr, &t.proj_out, x, out, s, nullptr);
        return;
    }
    RowStats st4;
    bf16* t4 = linear_rows(o, M, t.a2.out, ACT_NONE, t3, nullptr, s, rows ? nullptr : &st4);
    bf16* t5 = ff_behind(t.ff, t.ln3, t4, st4, B, HW, nullptr, rows, s, nullptr);
    gemm(a_rows(t5, C), t.proj_out.w, M, C, C, e_rows_res(out, C, t.proj_out.b, x), s);
}

bf16* Engine::feedforward(const FFW& f, const bf16* ln, int M, const bf16* res, const float* gate, hipStream_t s, const RowStats* in_stats,
                          RowStats* out_stats, bool raw_rows, bool use_rows) {
    const int C = f.C;
    if (use_rows) {
        if (!f.rows_stream || !ff_rows_supported(M, C)) throw GlError(GL_ERR_STATE, "feedforward: no row-local stream of this shape");
        // one launch: LayerNorm (where folded and the rows are raw) + GEGLU projection + FF-out + (gated) residual + row statistics
        bf16* out = arena_.get<bf16>((size_t)M * C);
        FFRowsParams P{};
        P.x = ln; P.ldx = C; P.normalize = (raw_rows || in_stats) ? 1 : 0; P.eps = 1e-5f;
        if (P.normalize && !f.folded) throw GlError(GL_ERR_STATE, "feedforward: raw rows given to an unfolded projection");
        P.stream = f.rows_stream; P.b2 = f.w2.b; P.res = res; P.ldres = C; P.gate = gate; P.out = out; P.ldo = C; P.M = M;
        if (out_stats) {
            *out_stats = RowStats{};
            if (ln_fold_) {
                out_stats->ld = 1; out_stats->nb = 1;
                out_stats->p = arena_.get<float2>((size_t)M);
                P.stats_out = out_stats->p; P.stats_ld = 1;
            }
        }
        ProfScope ps(this, s, "ff_rows_kernel", 24.0 * M * (double)C * C, 0.0);
        CK(ff_rows_launch(P, C, s));
        FILE* launch_log = launch_log_file();
        if (launch_log) {
            fprintf(launch_log, "ff_rows_kernel<320, 0, false, false>|%d|%d|%d|0|%.0f\n", M, C, 4 * C, (double)ff_stream_bytes(C) + (res ? 6.0 : 4.0) * M * C);
            fflush(launch_log);
        }
        ++n_launches;
        return out;
    }
    if (raw_rows && !in_stats) throw GlError(GL_ERR_STATE, "feedforward: raw rows without statistics outside the row-local kernel");
    bf16* hbuf = arena_.get<bf16>((size_t)M * 4 * C);
    Epilogue E = e_rows(hbuf, 4 * C, f.b1);
    E.act = ACT_GEGLU; E.geglu16 = f.geglu16;
    if (in_stats) {
        if (!f.folded) throw GlError(GL_ERR_STATE, "feedforward: row statistics given to an unfolded projection");
        e_fold_ln(E, *in_stats, f.csum1, C);
    }
    gemm(a_rows(ln, C), f.w1, M, 8 * C, C, E, s);
    return linear_rows(hbuf, M, f.w2, ACT_NONE, res, gate, s, out_stats);
}

// to_q of a cross-attention by GEMM into the head-layout q buffer shared by every attention of (Tp queries, Tk_pad keys) per sample;
// st: `ln` holds RAW rows, the LayerNorm folded into q is applied from these statistics (csum: the row sums of q.w)
AttnBufs& Engine::to_q_heads(const LinW& q, const bf16* ln, int B, int Tp, int C, int d, int Tk_pad, const RowStats* st, const float* csum, hipStream_t s) {
    const int heads = C / d;
    int dp, dpv;
    CK(attn_dims(d, &dp, &dpv));
    AttnBufs& bufs = attn_bufs(B, heads, d, Tp, Tk_pad);
    Epilogue E = e_heads(EPI_QK_HEADS, bufs.q, nullptr, C, heads, d, dp, Tp, bufs.Tq_pad, 0);
    E.bias = q.b;               // null unless a LayerNorm is folded in (to_q has no bias of its own)
    if (st) e_fold_ln(E, *st, csum, C);
    gemm(a_rows(ln, C), q.w, B * Tp, C, C, E, s);
    return bufs;
}

// attn2.to_q(norm2(rows)) (attention.py:336, 136): LayerNorm folded into the GEMM where the rows came with statistics, else ln_kernel
void Engine::cross_q_gemm(const STW& t, const bf16* rows, const RowStats& st, int B, int HW, hipStream_t s) {
    const int C = t.C, M = B * HW;
    const int Tp = round_up(HW, 64);
    const bool f3 = t.a2.folded && can_fold(st, M, C, C, EPI_QK_HEADS, ACT_NONE, Tp == HW);
    const bf16* ln = f3 ? rows : (t.a2.folded ? layernorm_plain(rows, B, HW, C, true, s) : layernorm(rows, B, HW, C, t.ln2, true, s));
    to_q_heads(t.a2.q, ln, B, Tp, C, t.d, cond_.ctx_Tpad, f3 ? &st : nullptr, t.a2.q_csum, s);
}

// the grounding tokens' keys / values of the fuser's attention are in block t's own K / V^T buffers for this prompt and shape
// (fuser_kv_fill): projected here at the first eager pass that needs them, never inside a capture
void Engine::ensure_fuser_kv(const STW& t, int B, int HW, hipStream_t s) {
    if (fuser_kv_.size() < unet_.st.size()) fuser_kv_.resize(unet_.st.size());
    const FuserKV& kv = fuser_kv_[t.idx];
    if (kv.epoch == cond_epoch_ && kv.B == B && kv.HW == HW) return;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap);
    if (cap != hipStreamCaptureStatusNone) throw GlError(GL_ERR_STATE, "fuser keys of this prompt / shape were not projected before the graph capture");
    fuser_kv_fill(t, B, HW, s);
    n_launches += 2;
}

// fuser.norm1 over [x ; objs] (attention.py:241, 289): HW visual rows + the block's Ng grounding-token rows per sample -> [B][Tf][C]
bf16* Engine::concat_layernorm(const STW& t, const bf16* x, int B, int HW, int Tf, hipStream_t s) {
    const int Ng = cond_.Ng, C = t.C;
    bf16* lnc = arena_.get<bf16>((size_t)B * Tf * C);
    LNParams P{};
    P.x = x; P.x2 = cond_.objs[t.idx]; P.B = B; P.N1 = HW; P.N2 = Ng; P.Tpad = Tf; P.C = C; P.eps = 1e-5f;
    P.gamma = t.fa.folded ? nullptr : t.fn1.g; P.beta = t.fa.folded ? nullptr : t.fn1.b; P.y = lnc;
    ProfScope ps(this, s, "ln_kernel", 0.0, 2.0 * B * (HW + Ng) * (double)C * 2);
    CK(layernorm_launch(P, s));
    ++n_launches;
    return lnc;
}

// SpatialTransformer.forward + BasicTransformerBlock._forward + GatedSelfAttentionDense.forward
// (attention.py:366-376, 333-338, 236-244)
bf16* Engine::transformer(const STW& t, const bf16* x, int B, int Bp, int H, int W, hipStream_t s) {
    const int HW = H * W, M = B * HW, C = t.C, d = t.d, heads = C / d;
    bf16* out = arena_.get<bf16>((size_t)M * C);
    const size_t mk = arena_.mark();
    if (cond_.Beff != B) throw GlError(GL_ERR_STATE, fmt("unet_forward batch %d != batch %d of the conditioning set by gl_unet_set_cond", B, cond_.Beff));
    if (Bp <= 0 || B % Bp != 0) throw GlError(GL_ERR_STATE, fmt("transformer: prefix batch %d does not divide batch %d", Bp, B));
    // Everything in front of attn1.to_out sees x alone: with Bp < B it runs on the first Bp samples (Mp rows), and what reads its
    // results (o, t0) at B samples reads sample b % Bp
    const bool shared = Bp < B;
    const int Mp = Bp * HW;

    bf16* n = groupnorm(TRef{x, C, nullptr, 0}, Bp, HW, t.gn, 1e-6f, false, s);
    // Folded LayerNorms (gemm.h Epilogue::ln_stats): every GEMM that writes the residual stream also writes its rows' partial
    // (sum, sum of squares); the projection behind the next LayerNorm then reads the RAW rows and normalises in its epilogue.
    // Where no statistics exist (split-K producer, the [x ; objs] concatenation, an epilogue without the fold) the rows go
    // through ln_kernel without affine -- gamma / beta live in the folded weights either way.
    const int Tp = round_up(HW, 64);
    const bool aligned = Tp == HW;
    auto normed = [&](const bf16* rows, const NormW& nw, bool folded, bool fuse, bool pad64) -> const bf16* {
        if (fuse) return rows;
        return folded ? layernorm_plain(rows, Bp, HW, C, pad64, s) : layernorm(rows, Bp, HW, C, nw, pad64, s);   // (norm1: the prefix batch)
    };
    RowStats st0, st1, st2, st3;
    // the row-local feed-forward kernel normalises its raw input rows itself: their producers need not write statistics
    const bool r2 = !fuser_off_ && ff_rows_for(t, 1, B, HW, s), r4 = ff_rows_for(t, 2, B, HW, s);
    // proj_in -> norm1 -> attn1's q,k,v^T: one row-local launch where that kernel exists and fills the chip (ffn.h qkv_rows_kernel)
    bf16* t0;
    const bf16* ln = nullptr;
    bf16* o = arena_.get<bf16>((size_t)M * C);         // (B samples: the later attentions write it whole)
    bool rq1;
    {
    // the prefix's GEMMs take the plans of their full-batch forms: the same bits as without sharing (gemm.h gemm_set_plan_batch_scale)
    PlanAsBatch plan_as(B / Bp);
    rq1 = aligned && qkv_rows_for(t, 0, Bp, HW, HW, s);
    if (rq1) {
        t0 = arena_.get<bf16>((size_t)Mp * C);
        qkv_rows_project(t.a1, n, Bp, HW, HW, C, d, t.proj_in, nullptr, t0, nullptr, 0, 0, s);
        self_attention(t.a1, nullptr, Bp, Tp, HW, HW, C, d, o, s, nullptr, 0, 0, true);
        if (shared) cfg_shared_prefix_note(1);
    } else {
        t0 = linear_rows(n, Mp, t.proj_in, ACT_NONE, nullptr, nullptr, s, &st0);
        // x = attn1(norm1(x)) + x
        const bool f1 = t.a1.folded && can_fold(st0, Mp, C, 3 * C, EPI_QKV_HEADS, ACT_NONE, aligned);
        ln = normed(t0, t.ln1, t.a1.folded, f1, true);
        self_attention(t.a1, ln, Bp, Tp, HW, HW, C, d, o, s, f1 ? &st0 : nullptr);
    }
    }
    const int Ng = cond_.Ng;
    // attn1.to_out + residual -> fuser.norm1 -> the fuser's q,k,v^T over the visual rows: the same launch shape
    const bool rq2 = !fuser_off_ && unet_.cfg.fuser_kind == 0 && fuser_hoist_ && aligned && cond_.Ng > 0 && qkv_rows_for(t, 1, B, HW, HW + Ng, s);
    if (shared && !rq2) {
        // every form but the row-local launch below reads o and t0 at B samples: one copy kernel each, then the code is the unshared one
        replicate(o, o + (size_t)Mp * C, (size_t)Mp * C, B / Bp - 1, s);
        bf16* t0b = arena_.get<bf16>((size_t)M * C);
        replicate(t0, t0b, (size_t)Mp * C, B / Bp, s);
        t0 = t0b;
    }
    bf16* t1 = rq2 ? arena_.get<bf16>((size_t)M * C) : linear_rows(o, M, t.a1.out, ACT_NONE, t0, nullptr, s, &st1);

    bf16* t3;
    bool q_done = false;
    if (fuser_off_) {
        t3 = t1;
        st3 = st1;
    } else if (unet_.cfg.fuser_kind == 0) {
        // fuser (gatedSA): x = x + scale*tanh(alpha_attn) * attn(norm1([x ; linear(objs)]))[:, :N]
        const int Tf = round_up(HW + Ng, 64);
        if (rq2) {
            ensure_fuser_kv(t, B, HW, s);
            // (shared prefix: o and t0 hold Bp samples, the launch reads row m % Mp of both and writes t1 and q, k, v^T for all B)
            qkv_rows_project(t.fa, o, B, HW, HW + Ng, C, d, t.a1.out, t0, t1, nullptr, Tf, t.idx + 1, s, shared ? Bp : 0);
            if (shared) cfg_shared_prefix_note(2);
            self_attention(t.fa, nullptr, B, HW, HW, HW + Ng, C, d, o, s, nullptr, Tf, t.idx + 1, true);
        } else if (fuser_hoist_ && t.fa.fused && t.fa.folded && aligned) {
            // the grounding tokens' keys / values are in this block's buffers since the prompt was set (fuser_kv_fill); only the visual
            // rows are projected, raw, with the statistics attn1.to_out wrote (or through the plain LayerNorm where it wrote none)
            ensure_fuser_kv(t, B, HW, s);
            const bool ff = can_fold(st1, M, C, 3 * C, EPI_QKV_HEADS, ACT_NONE, aligned);
            const bf16* rows = ff ? t1 : layernorm_plain(t1, B, HW, C, false, s);
            self_attention(t.fa, rows, B, HW, HW, HW + Ng, C, d, o, s, ff ? &st1 : nullptr, Tf, t.idx + 1);
        } else {
            self_attention(t.fa, concat_layernorm(t, t1, B, HW, Tf, s), B, Tf, HW, HW + Ng, C, d, o, s);
        }
        //    x = x + scale*tanh(alpha_dense) * ff(norm2(x))
        t3 = fuser_ff_tail(t, o, t1, B, HW, r2, s, &st3, &q_done);
    } else {
        bf16* t2;
        if (unet_.cfg.fuser_kind == 1) {
            // fuser (gatedSA2, attention.py:271-297): the attention outputs AT the grounding tokens (an sg x sg grid) are
            // projected, resized bicubically to the visual grid and added as the gated residual
            int sg = 0;
            while (sg * sg < Ng) ++sg;
            if (sg * sg != Ng || H != W) throw GlError(GL_ERR_ARG, fmt("gatedSA2 needs square token grids (visual %dx%d, %d grounding tokens)", H, W, Ng));
            const int Ta = HW + Ng;
            const int Tf = round_up(Ta, 64);
            bf16* lnc = concat_layernorm(t, t1, B, HW, Tf, s);
            bf16* oa = arena_.get<bf16>((size_t)B * Ta * C);
            self_attention(t.fa, lnc, B, Tf, Ta, Ta, C, d, oa, s);                 // every token is a query here
            bf16* pr = linear_rows(oa, B * Ta, t.fa.out, ACT_NONE, nullptr, nullptr, s);  // [B][HW + Ng][C]
            t2 = arena_.get<bf16>((size_t)M * C);
            CK(fuser_resize_launch(pr, t1, gates_ + 2 * t.idx, t2, B, Ta, HW, sg, H, C, s));
            ++n_launches;
        } else {
            // fuser (gatedCA, attention.py:207-212): x = x + scale*tanh(alpha_attn) * attn(norm1(x), objs, objs)
            ln = layernorm(t1, B, HW, C, t.fn1, true, s);
            const AttnBufs& bufs = to_q_heads(t.fca.q, ln, B, Tp, C, d, cond_.obj_Tpad, nullptr, nullptr, s);
            attention(bufs.q, cond_.obj_k[t.idx], cond_.obj_vt[t.idx], o, B, heads, d, HW, Ng, bufs.Tq_pad, cond_.obj_Tpad, 0, s);
            t2 = linear_rows(o, M, t.fca.out, ACT_NONE, t1, gates_ + 2 * t.idx, s, r2 ? nullptr : &st2);
        }
        //        x = x + scale*tanh(alpha_dense) * ff(norm2(x))
        t3 = ff_behind(t.fff, t.fn2, t2, st2, B, HW, gates_ + 2 * t.idx + 1, r2, s, &st3);
    }

    // x = attn2(norm2(x), context) + x
    if (!q_done) cross_q_gemm(t, t3, st3, B, HW, s);
    {
        const AttnBufs& bufs = attn_bufs(B, heads, d, Tp, cond_.ctx_Tpad);
        attention(bufs.q, cond_.ctx_k[t.idx], cond_.ctx_vt[t.idx], o, B, heads, d, HW, cond_.ctx_T, bufs.Tq_pad, cond_.ctx_Tpad, 0, s);
    }
    // x = attn2.to_out(.) + x;  x = ff(norm3(x)) + x;  proj_out + x_in
    block_ff_tail(t, o, t3, x, out, B, HW, r4, s);
    arena_.release(mk);
    return out;
}

// ---------------------------------------------------------------- conditioning
void Engine::set_fuser_scale(float v, hipStream_t s) {
    if (!unet_.present || !finalized_) throw GlError(GL_ERR_STATE, "unet not finalized");
    CK(fill_f32_launch(fuser_scale_, v, (int)unet_.st.size(), s));
    // set_alpha_scale(model, 0) (the tail of the reference's alpha schedules, gligen_inference.py:31-66): every gated residual is
    // x + 0 * f(x) = x, so the fuser's attention and feed-forward are not launched at all (gatedSA2 never gets here with 0: the
    // reference's set_alpha_scale does not reach it)
    fuser_off_ = v == 0.f;
}

// UNetModel.restore_first_conv_from_SD (openaimodel.py:400-413): overwrite the packed first-conv
// buffers in place, so captured graphs (which hold these addresses) pick the new weights up.
void Engine::restore_first_conv(const float* w, const float* b, hipStream_t s) {
    if (!unet_.present || !finalized_) throw GlError(GL_ERR_STATE, "unet not finalized");
    if (unet_.cfg.inpaint_mode) throw GlError(GL_ERR_STATE, "first conv of an inpainting model is not restorable");
    const int mc = unet_.cfg.model_channels;
    // a 4 + k channel GLIGEN first conv (grounding downsampler) becomes the 4-channel SD conv: the k extra input
    // channels get zero weights, which is what dropping the concat (openaimodel.py:442-444, first_conv_type "SD") computes
    CK(pack_conv_small_launch(w, const_cast<bf16*>(unet_.conv_in_small.w), mc, unet_.conv_in_small.Cin, unet_.conv_in_small.Kpad, s, unet_.cfg.in_channels));
    HIPCK(hipMemcpyAsync(const_cast<float*>(unet_.conv_in_small.b), b, mc * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void Engine::set_cond(int Beff, const float* context, int n_ctx, const gl_grounding& g, hipStream_t s) {
    if (!unet_.present || !finalized_) throw GlError(GL_ERR_STATE, "unet not finalized");
    if (Beff <= 0 || n_ctx <= 0 || g.n <= 0) throw GlError(GL_ERR_ARG, "set_cond: empty batch / context / grounding");
    if (unet_.cfg.fuser_kind == 1) {
        int sg = 0;
        while (sg * sg < (unet_.gkind == 1 ? 2 * g.n : g.n)) ++sg;
        if (sg * sg != (unet_.gkind == 1 ? 2 * g.n : g.n)) throw GlError(GL_ERR_ARG, "gatedSA2 needs a square number of grounding tokens");
    }
    const gl_unet_config& c = unet_.cfg;
    const int Ng = unet_.gkind == 1 ? 2 * g.n : g.n;
    const int ctx_Tpad = round_up(n_ctx, 64);
    const int heads = c.num_heads;
    const bool ca = c.fuser_kind == 2;
    const int obj_Tpad = round_up(Ng, 64);
    const int obj_stride = ca ? obj_Tpad : Ng;   // rows per sample of the grounding-token matrix (gatedCA pads to the key tile)
    if (cond_.Beff != Beff || cond_.Ng != Ng || cond_.ctx_Tpad != ctx_Tpad) {
        // captured graphs bake Nk (= HW + Ng), the conditioning buffers and the batch: a last run -- on whatever stream it was issued --
        // is over before they and the buffers go
        sampler_wait_idle();
        HIPCK(hipStreamSynchronize(s));
        sampler_release_graph();
        for (void* p : cond_.allocs) (void)hipFree(p);
        cond_ = Cond{};
        auto palloc = [&](size_t bytes) {
            void* p = nullptr;
            HIPCK(hipMalloc(&p, bytes));
            HIPCK(hipMemset(p, 0, bytes));
            cond_.allocs.push_back(p);
            return p;
        };
        for (const STW& t : unet_.st) {
            int dp, dpv;
            CK(attn_dims(t.d, &dp, &dpv));
            if (ca) {
                cond_.objs.push_back(nullptr);
                cond_.obj_k.push_back(reinterpret_cast<bf16*>(palloc((size_t)Beff * heads * obj_Tpad * dp * sizeof(bf16))));
                cond_.obj_vt.push_back(reinterpret_cast<bf16*>(palloc((size_t)Beff * heads * dpv * obj_Tpad * sizeof(bf16))));
                CK(attn_vt_ones_launch(cond_.obj_vt.back(), Beff * heads, t.d, obj_Tpad, 0));
                CK(attn_k_init_launch(cond_.obj_k.back(), Beff * heads, t.d, obj_Tpad, 0));
            } else {
                cond_.objs.push_back(reinterpret_cast<bf16*>(palloc((size_t)Beff * Ng * t.C * sizeof(bf16))));
            }
            cond_.ctx_k.push_back(reinterpret_cast<bf16*>(palloc((size_t)Beff * heads * ctx_Tpad * dp * sizeof(bf16))));
            cond_.ctx_vt.push_back(reinterpret_cast<bf16*>(palloc((size_t)Beff * heads * dpv * ctx_Tpad * sizeof(bf16))));
            CK(attn_vt_ones_launch(cond_.ctx_vt.back(), Beff * heads, t.d, ctx_Tpad, 0));
            CK(attn_k_init_launch(cond_.ctx_k.back(), Beff * heads, t.d, ctx_Tpad, 0));
        }
        cond_.tokens = reinterpret_cast<bf16*>(palloc((size_t)Beff * obj_stride * c.gr_out_dim * sizeof(bf16)));
        HIPCK(hipStreamSynchronize(0));
        cond_.Beff = Beff;
        cond_.Ng = Ng;
        cond_.ctx_Tpad = ctx_Tpad;
        cond_.obj_Tpad = obj_Tpad;
    }
    if (cond_.ctx_T != n_ctx && (smp_.exec[0] || smp_.exec[1])) {  // captured cross-attention launches bake Nk = ctx_T
        sampler_wait_idle();
        sampler_release_graph();
    }
    cond_.ctx_T = n_ctx;
    arena_.reset();

    // ---- grounding tokens: objs = position_net(**grounding_input)  -> [Beff][Ng][out_dim]
    const int out_dim = c.gr_out_dim;
    bf16* objs = arena_.get<bf16>((size_t)Beff * obj_stride * out_dim);
    if (ca) HIPCK(hipMemsetAsync(objs, 0, (size_t)Beff * obj_stride * out_dim * sizeof(bf16), s));  // key-tile padding rows
    const int rows = Beff * g.n;
    auto mlp = [&](int which, const PosNetIn& pin_in, int remap_off) {
        PosNetIn pin = pin_in;
        const int Kp = unet_.pn[which][0].K;
        pin.out = arena_.get<bf16>((size_t)rows * Kp);
        pin.ld_out = Kp;
        pin.rows = rows;
        CK(posnet_input_launch(pin, s));
        bf16* h1 = linear_rows(pin.out, rows, unet_.pn[which][0], ACT_SILU, nullptr, nullptr, s);
        bf16* h2 = linear_rows(h1, rows, unet_.pn[which][1], ACT_SILU, nullptr, nullptr, s);
        Epilogue E = e_rows(objs, out_dim, unet_.pn[which][2].b);
        E.remap_in = g.n; E.remap_out = obj_stride; E.remap_off = remap_off;
        gemm(a_rows(h2, unet_.pn[which][2].K), unet_.pn[which][2].w, rows, out_dim, unet_.pn[which][2].K, E, s);
    };
    PosNetIn pin{};
    pin.null_pos = unet_.pn_null_pos;
    pin.mask = g.masks;
    if (unet_.gkind == 0) {
        if (!g.boxes || !g.masks || !g.text_embeddings) throw GlError(GL_ERR_ARG, "text grounding needs boxes, masks, text_embeddings");
        pin.feat = g.text_embeddings; pin.pos = g.boxes; pin.F = c.gr_in_dim; pin.P = 4; pin.null_feat = unet_.pn_null_feat[0];
        mlp(0, pin, 0);
    } else if (unet_.gkind == 1) {
        if (!g.boxes || !g.masks || !g.text_masks || !g.image_masks || !g.text_embeddings || !g.image_embeddings)
            throw GlError(GL_ERR_ARG, "text+image grounding needs boxes, masks, text/image masks and embeddings");
        pin.pos = g.boxes; pin.F = c.gr_in_dim; pin.P = 4;
        pin.feat = g.text_embeddings; pin.fmask = g.text_masks; pin.null_feat = unet_.pn_null_feat[0];
        mlp(0, pin, 0);
        pin.feat = g.image_embeddings; pin.fmask = g.image_masks; pin.null_feat = unet_.pn_null_feat[1];
        mlp(1, pin, g.n);
    } else if (unet_.gkind == 3) {
        if (!g.tokens) throw GlError(GL_ERR_ARG, "grounding_kind 3 needs gl_grounding.tokens");
        CK(pad_rows_cast_launch(g.tokens, objs, Beff, g.n, obj_stride, out_dim, s));
    } else {
        if (!g.points || !g.masks) throw GlError(GL_ERR_ARG, "keypoint grounding needs points and masks");
        if (g.n != c.max_persons * 17) throw GlError(GL_ERR_ARG, "keypoint grounding: n must be max_persons*17");
        pin.feat = unet_.kp_table; pin.feat_mod = g.n; pin.pos = g.points; pin.F = out_dim; pin.P = 2; pin.null_feat = unet_.pn_null_feat[0];
        mlp(0, pin, 0);
    }

    ++cond_epoch_;
    cond_.obj_stride = obj_stride;
    HIPCK(hipMemcpyAsync(cond_.tokens, objs, (size_t)Beff * obj_stride * out_dim * sizeof(bf16), hipMemcpyDeviceToDevice, s));  // gl_unet_grounding_tokens

    // ---- per transformer: fuser.linear(objs), attn2.to_k / to_v (context)
    bf16* ctxb = arena_.get<bf16>((size_t)Beff * ctx_Tpad * c.context_dim);
    CK(pad_rows_cast_launch(context, ctxb, Beff, n_ctx, ctx_Tpad, c.context_dim, s));
    for (const STW& t : unet_.st) {
        int dp, dpv;
        CK(attn_dims(t.d, &dp, &dpv));
        // to_k / to_v of a cross-attention over `rows` [Beff][Tpad][ctx_dim]: K in the key-tile layout, V^T, as the attention kernel reads them
        auto kv = [&](const CrossAttnW& a, const bf16* rows, int Tpad, bf16* k, bf16* vt) {
            Epilogue E = e_heads(EPI_QK_HEADS, k, nullptr, t.C, heads, t.d, dp, Tpad, Tpad, 0);
            E.q_tiled = 1;
            gemm(a_rows(rows, a.ctx_dim), a.wk, Beff * Tpad, t.C, a.ctx_dim, E, s);
            Epilogue V;
            epilogue_defaults(V);
            V.mode = EPI_VT_HEADS;
            V.out = vt; V.H = heads; V.d = t.d; V.DPV = dpv; V.T = Tpad; V.Tpad_k = Tpad;
            CK(gemm_launch_t(a.wv, t.C, rows, Beff * Tpad, a.ctx_dim, V, s));
        };
        if (!ca) {
            gemm(a_rows(objs, t.flin.K), t.flin.w, Beff * Ng, t.C, t.flin.K, e_rows(cond_.objs[t.idx], t.C, t.flin.b), s);
        } else {  // gatedCA: fuser.attn.to_k / to_v of the grounding tokens, head layouts of the attention kernel
            kv(t.fca, objs, obj_Tpad, cond_.obj_k[t.idx], cond_.obj_vt[t.idx]);
        }
        kv(t.a2, ctxb, ctx_Tpad, cond_.ctx_k[t.idx], cond_.ctx_vt[t.idx]);
    }
    // A captured graph of these shapes may be replayed for this prompt without another eager pass: the blocks whose shape is known
    // from the previous prompt get the new grounding-token keys / values now
    if (!ca && fuser_hoist_ && c.fuser_kind == 0)
        for (const STW& t : unet_.st)
            if ((size_t)t.idx < fuser_kv_.size() && fuser_kv_[t.idx].HW && fuser_kv_[t.idx].B == Beff && t.fa.fused && t.fa.folded) fuser_kv_fill(t, Beff, fuser_kv_[t.idx].HW, s);
}

// the `scale` attributes of the fuser modules, one per transformer block in module order (they are plain Python attributes in
// the reference: set_alpha_scale writes the same value into all of them, anything else may write them individually)
void Engine::set_fuser_scales(const float* scales, int n, hipStream_t s) {
    if (!unet_.present || !finalized_) throw GlError(GL_ERR_STATE, "unet not finalized");
    if (n != (int)unet_.st.size()) throw GlError(GL_ERR_ARG, fmt("set_fuser_scales: %d values for %d fusers", n, (int)unet_.st.size()));
    HIPCK(hipMemcpyAsync(fuser_scale_, scales, n * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCK(hipStreamSynchronize(s));   // `scales` is the caller's host memory
    bool all_zero = true;
    for (int i = 0; i < n; ++i) all_zero = all_zero && scales[i] == 0.f;
    fuser_off_ = all_zero;
}

void Engine::grounding_tokens(float* out, hipStream_t s) {
    if (!cond_.tokens) throw GlError(GL_ERR_STATE, "no conditioning set");
    CK(bf16_rows_to_f32_launch(cond_.tokens, out, cond_.Beff, cond_.Ng, cond_.obj_stride, unet_.cfg.gr_out_dim, s));
}

// ---------------------------------------------------------------- UNetModel.forward (openaimodel.py:420-464)
// SiLU(time_embed(timestep_embedding(t))) through every ResBlock's emb_layers at once: fp32 [R][unet_.embcat.N] (out = nullptr: from the arena)
float* Engine::emb_rows(const int64_t* t_dev, int R, float* out, hipStream_t s) {
    const int mc = unet_.cfg.model_channels;
    bf16* temb = arena_.get<bf16>((size_t)R * mc);
    CK(timestep_embed_launch(t_dev, temb, R, mc, s));
    bf16* e1 = linear_rows(temb, R, unet_.te0, ACT_SILU, nullptr, nullptr, s);
    bf16* semb = linear_rows(e1, R, unet_.te2, ACT_SILU, nullptr, nullptr, s);
    if (!out) out = arena_.get<float>((size_t)R * unet_.embcat.N);
    Epilogue E = e_rows(out, unet_.embcat.N, unet_.embcat.b);
    E.out_f32 = 1;
    gemm(a_rows(semb, unet_.embcat.K), unet_.embcat.w, R, unet_.embcat.N, unet_.embcat.K, E, s);
    return out;
}

void Engine::emb_table_build(const int64_t* t_host, int R, hipStream_t s) {
    if ((int)emb_t_cache_.size() == R && std::equal(t_host, t_host + R, emb_t_cache_.begin())) return;   // the schedule of the last run
    if (R > emb_table_cap_) {
        const int cap = std::max(R, 64);
        emb_table_ = reinterpret_cast<float*>(persist((size_t)cap * unet_.embcat.N * sizeof(float), false));
        emb_t_dev_ = reinterpret_cast<int64_t*>(persist((size_t)cap * sizeof(int64_t), false));
        if (!emb_cur_) emb_cur_ = reinterpret_cast<float*>(persist((size_t)unet_.embcat.N * sizeof(float), true));
        emb_table_cap_ = cap;
    }
    HIPCK(hipMemcpyAsync(emb_t_dev_, t_host, (size_t)R * sizeof(int64_t), hipMemcpyHostToDevice, s));
    const size_t mk = arena_.mark();
    emb_rows(emb_t_dev_, R, emb_table_, s);
    arena_.release(mk);
    emb_t_cache_.assign(t_host, t_host + R);
}

void Engine::unet_forward(int Beff, int h, int w, const float* x, int xB, const int64_t* t, const float* extra,
                          int extraB, float* eps, hipStream_t s, const float* emb_row) {
    if (!unet_.present || !finalized_) throw GlError(GL_ERR_STATE, "unet not finalized");
    if (cond_.Beff != Beff) throw GlError(GL_ERR_STATE, fmt("unet_forward batch %d but conditioning was set for %d", Beff, cond_.Beff));
    const gl_unet_config& c = unet_.cfg;
    const int extra_C = c.inpaint_mode ? c.in_channels + 1 : c.extra_channels;
    if ((extra_C != 0) != (extra != nullptr))
        throw GlError(GL_ERR_ARG, "the extra first-conv input (inpainting_extra_input / downsampled grounding_extra_input) must be given iff the model has those channels");
    if (xB <= 0 || Beff % xB != 0) throw GlError(GL_ERR_ARG, "x batch must divide the effective batch");
    const int mc = c.model_channels;
    arena_.reset();

    // time embedding: emb = time_embed(timestep_embedding(t)); every ResBlock consumes SiLU(emb)
    const float* embout = emb_row;
    int emb_ld = 0;                   // (a precomputed row is every sample's)
    if (!emb_row) {
        embout = emb_rows(t, Beff, nullptr, s);
        emb_ld = unet_.embcat.N;
        ++n_launches;
    }
    CK(gates_launch(unet_.alpha_ptrs, fuser_scale_, gates_, 2 * (int)unet_.st.size(), s));
    ++n_launches;

    struct Act { bf16* p; int C, H, W; };
    std::vector<Act> hs;
    Act cur{nullptr, 0, h, w};

    // The guidance pair's shared prefix. With one time-embedding row for every sample and x (and the extra first-conv input) of xB
    // samples serving Beff = R xB, samples b and b % xB are bit-identical until the first layer that reads conditioning: the first
    // transformer's fuser / cross-attention. The layers between conv_in and that transformer, and the transformer's own head (its
    // GroupNorm, proj_in, norm1, attn1), run on the first xB samples only. conv_in stays at Beff: its output is hs[0], which the last
    // output block concatenates at Beff. Per-sample timesteps (emb_row == nullptr) never share: whether they are equal is not
    // known on the host.
    int Bp = Beff;
    if (emb_row && Beff / xB > 1 && cfg_shared_prefix()) {
        bool has_st = false;
        for (const UNetBlock& b : unet_.in_blocks)
            for (const Layer& L : b.layers) has_st = has_st || L.kind == L_ST;
        if (has_st) {
            Bp = xB;
            cfg_shared_prefix_note(0);
        }
    }
    bool in_prefix = Bp < Beff;      // until the first transformer has run

    // Bl: the batch the layer runs at. full (Bl < Beff): its result is needed at Beff -- a skip connection, or the transformer's
    // residual behind proj_out -- so it is written into a Beff-sample buffer and copied behind itself
    auto run_layer = [&](const Layer& L, const TRef& in, int Bl, bool full) {
        PlanAsBatch plan_as(L.kind == L_ST ? 1 : Beff / Bl);    // a prefix layer's GEMMs / convs: planned as at Beff, the same bits (the transformer scopes its own)
        auto out_for = [&](int HWo, int Co) { return full ? arena_.get<bf16>((size_t)Beff * HWo * Co) : nullptr; };
        auto fill = [&](bf16* o, int HWo, int Co) {
            if (full) replicate(o, o + (size_t)Bl * HWo * Co, (size_t)Bl * HWo * Co, Beff / Bl - 1, s);
        };
        switch (L.kind) {
            case L_CONV_IN: {
                if (extra && extraB != xB) throw GlError(GL_ERR_ARG, "extra first-conv input batch must equal x batch");
                Im2colParams P{};
                P.x0 = x; P.C0 = c.in_channels;
                P.x1 = extra; P.C1 = extra_C;
                P.B = xB; P.H = cur.H; P.W = cur.W;
                cur.p = conv3x3_small(unet_.conv_in_small, P, Beff / xB, s);   // sample b reads x[b % xB]: one im2col launch per replica group
                cur.C = mc;
                break;
            }
            case L_RES: {
                const ResW& r = unet_.res[L.idx];
                cur.p = resblock(r, in, Bl, cur.H, cur.W, embout, emb_ld, 1e-5f, s, out_for(cur.H * cur.W, r.Cout));
                cur.C = r.Cout;
                fill(cur.p, cur.H * cur.W, cur.C);
                break;
            }
            case L_ST: {
                if (in.p1) throw GlError(GL_ERR_STATE, "transformer over concatenated input");
                cur.p = transformer(unet_.st[L.idx], in.p0, Beff, Bl, cur.H, cur.W, s);   // (its input holds Beff samples either way)
                break;
            }
            case L_DOWN: {
                const int Ho = (cur.H + 2 - 3) / 2 + 1, Wo = (cur.W + 2 - 3) / 2 + 1;
                cur.p = conv3x3(in, Bl, cur.H, cur.W, unet_.updown[L.idx], 2, 0, 1, nullptr, 0, nullptr, s, out_for(Ho * Wo, unet_.updown[L.idx].Cout));
                cur.H = Ho;
                cur.W = Wo;
                fill(cur.p, Ho * Wo, unet_.updown[L.idx].Cout);
                break;
            }
            case L_UP: {
                cur.p = conv3x3(in, Beff, cur.H, cur.W, unet_.updown[L.idx], 1, 1, 1, nullptr, 0, nullptr, s);
                cur.H *= 2;
                cur.W *= 2;
                break;
            }
        }
    };

    for (const UNetBlock& b : unet_.in_blocks) {
        for (size_t i = 0; i < b.layers.size(); ++i) {
            const Layer& L = b.layers[i];
            const bool pre = in_prefix && L.kind != L_CONV_IN;
            const bool last = i + 1 == b.layers.size();
            run_layer(L, TRef{cur.p, cur.C, nullptr, 0}, pre ? Bp : Beff, pre && L.kind != L_ST && (last || b.layers[i + 1].kind == L_ST));
            if (L.kind == L_ST) in_prefix = false;
        }
        hs.push_back(cur);
    }
    for (const Layer& L : unet_.mid_block.layers) run_layer(L, TRef{cur.p, cur.C, nullptr, 0}, Beff, false);
    for (const UNetBlock& b : unet_.out_blocks) {
        Act sk = hs.back();
        hs.pop_back();
        if (sk.H != cur.H || sk.W != cur.W) throw GlError(GL_ERR_ARG, "latent size must be divisible by the UNet's total stride");
        bool first = true;
        for (const Layer& L : b.layers) {
            if (first) run_layer(L, TRef{cur.p, cur.C, sk.p, sk.C}, Beff, false);  // th.cat([h, hs.pop()], dim=1)
            else run_layer(L, TRef{cur.p, cur.C, nullptr, 0}, Beff, false);
            first = false;
        }
    }
    // out: GroupNorm32 -> SiLU -> conv3x3 -> NCHW fp32
    gn_silu_conv3x3_nchw(cur.p, cur.C, Beff, cur.H, cur.W, unet_.out_norm, 1e-5f, unet_.out_conv, c.out_channels, eps, s);
}

}  // namespace gl
