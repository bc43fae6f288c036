// gligen_amd engine -- the core every model shares: error state, arena, profiling, contexts (fork), weight upload and the
// weight-descriptor builders, finalize, and the primitive launch helpers (see engine.h, include/gligen_amd.h). The models
// themselves: engine_unet / _policy / _vae / _clip / _spatial / _sampler .hip.
#include "engine_impl.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstring>

namespace gl {

static thread_local char g_err[2048] = "";
int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
const char* last_error() { return g_err; }

// ---------------------------------------------------------------- Arena
void Arena::init(size_t bytes) {
    off_ = hw_ = 0;
    HIPCK(hipGetDevice(&dev_));
    int vmm = 0;
    const char* sw = dev_env("GL_ARENA_VMM");
    if (!(sw && atoi(sw) == 0) && hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, dev_) == hipSuccess && vmm) {
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = dev_;
        size_t gran = 0;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) == hipSuccess && gran) {
            const size_t want = (bytes + gran - 1) / gran * gran;
            void* p = nullptr;
            if (hipMemAddressReserve(&p, want, gran, nullptr, 0) == hipSuccess && p) {
                base_ = reinterpret_cast<char*>(p);
                cap_ = want;
                gran_ = gran;
                vmm_ = true;
                mapped_ = 0;
                return;
            }
        }
        (void)hipGetLastError();
    }
    HIPCK(hipMalloc(reinterpret_cast<void**>(&base_), bytes));
    cap_ = bytes;
}
void Arena::grow(size_t need) {
    // 64 MiB steps (a multiple of the granularity): a few dozen mappings for a 1 GB high-water mark, none once it is reached
    const size_t step = std::max(gran_, ((size_t(64) << 20) + gran_ - 1) / gran_ * gran_);
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev_;
    while (mapped_ < need) {
        const size_t chunk = std::min(step, cap_ - mapped_);
        hipMemGenericAllocationHandle_t h;
        HIPCK(hipMemCreate(&h, chunk, &prop, 0));
        hipError_t e = hipMemMap(base_ + mapped_, chunk, 0, h, 0);
        if (e != hipSuccess) {
            (void)hipMemRelease(h);
            throw GlError(GL_ERR_HIP, fmt("workspace arena: hipMemMap of %zu bytes failed: %s", chunk, hipGetErrorString(e)));
        }
        hipMemAccessDesc acc = {};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(base_ + mapped_, chunk, &acc, 1);
        if (e != hipSuccess) {
            (void)hipMemUnmap(base_ + mapped_, chunk);
            (void)hipMemRelease(h);
            throw GlError(GL_ERR_HIP, fmt("workspace arena: hipMemSetAccess failed: %s", hipGetErrorString(e)));
        }
        handles_.push_back(reinterpret_cast<void*>(h));
        mapped_ += chunk;
    }
}
void Arena::destroy() {
    if (vmm_) {
        const size_t step = handles_.empty() ? 0 : std::max(gran_, ((size_t(64) << 20) + gran_ - 1) / gran_ * gran_);
        size_t at = 0;
        for (void* h : handles_) {
            const size_t chunk = std::min(step, cap_ - at);
            (void)hipMemUnmap(base_ + at, chunk);
            (void)hipMemRelease(reinterpret_cast<hipMemGenericAllocationHandle_t>(h));
            at += chunk;
        }
        handles_.clear();
        if (base_) (void)hipMemAddressFree(base_, cap_);
        vmm_ = false;
        mapped_ = 0;
    } else if (base_) {
        (void)hipFree(base_);
    }
    base_ = nullptr;
}
void* Arena::alloc(size_t bytes) {
    size_t a = (off_ + 255) & ~size_t(255);
    if (a + bytes > cap_)
        throw GlError(GL_ERR_STATE, fmt("workspace arena exhausted: need %zu more bytes (capacity %zu); "
                                        "create the context with a larger arena", bytes, cap_));
    if (vmm_ && a + bytes > mapped_) grow(a + bytes);
    off_ = a + bytes;
    hw_ = std::max(hw_, off_);
    return base_ + a;
}

// ---------------------------------------------------------------- Engine basics
Engine::Engine(int device) : device_(device) {}

Engine::~Engine() {
    sampler_release_graph();
    for (hipEvent_t e : smp_.tev) (void)hipEventDestroy(e);
    if (smp_.ev_in) (void)hipEventDestroy(smp_.ev_in);
    if (smp_.ev_out) (void)hipEventDestroy(smp_.ev_out);
    if (smp_.ev_done) (void)hipEventDestroy(smp_.ev_done);
    if (smp_.stream) (void)hipStreamDestroy(smp_.stream);
    for (hipEvent_t e : train_events_)
        if (e) (void)hipEventDestroy(e);
    if (!parent_)
        for (auto& kv : raw_)
            if (kv.second.p) (void)hipFree(kv.second.p);
    train_cache_destroy(train_cache);
    for (void* p : owned_) (void)hipFree(p);
    for (void* p : cond_.allocs) (void)hipFree(p);
    arena_.destroy();
}

// ---------------------------------------------------------------- per-kernel profile
Engine::ProfScope::ProfScope(Engine* eng, hipStream_t st, const std::string& name, double flops, double bytes) : e(eng), s(st), idx(0) {
    if (!e->profiling_) return;
    auto get = [&]() {
        hipEvent_t ev;
        if (!e->prof_pool_.empty()) { ev = e->prof_pool_.back(); e->prof_pool_.pop_back(); }
        else if (hipEventCreate(&ev) != hipSuccess) throw GlError(GL_ERR_HIP, "hipEventCreate failed");
        return ev;
    };
    ProfEvt pe{name, flops, bytes, get(), get()};
    idx = e->prof_.size();
    e->prof_.push_back(pe);
    (void)hipEventRecord(pe.e0, s);
}
Engine::ProfScope::~ProfScope() {
    if (e->profiling_) (void)hipEventRecord(e->prof_[idx].e1, s);
}
hipEvent_t* Engine::train_events() {
    if (train_events_.empty()) {
        train_events_.resize(kTrainEvents, nullptr);
        for (auto& e : train_events_) HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return train_events_.data();
}

void Engine::profile_begin() {
    prof_.clear();
    profiling_ = true;
}
std::vector<Engine::ProfRec> Engine::profile_end(hipStream_t s) {
    profiling_ = false;
    HIPCK(hipStreamSynchronize(s));
    std::vector<ProfRec> out;
    for (auto& pe : prof_) {
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, pe.e0, pe.e1));
        prof_pool_.push_back(pe.e0);
        prof_pool_.push_back(pe.e1);
        auto it = std::find_if(out.begin(), out.end(), [&](const ProfRec& r) { return r.name == pe.name; });
        if (it == out.end()) { out.push_back(ProfRec{pe.name}); it = out.end() - 1; }
        it->calls += 1; it->ms += ms; it->flops += pe.flops; it->bytes += pe.bytes;
    }
    prof_.clear();
    std::sort(out.begin(), out.end(), [](const ProfRec& a, const ProfRec& b) { return a.ms > b.ms; });
    return out;
}

void Engine::init_workspace() {
    if (ws_) return;
    ws_bytes_ = size_t(256) << 20;  // fp32 split-K slabs
    ws_ = reinterpret_cast<float*>(persist(ws_bytes_, false));
}

void Engine::attn_regime_counters(int enable, unsigned* out) {
    HIPCK(hipDeviceSynchronize());      // every attention launch that counted has finished
    if (!attn_ctr_) attn_ctr_ = reinterpret_cast<unsigned*>(persist(ATTN_CTR_N * sizeof(unsigned), true));
    HIPCK(hipMemcpy(out, attn_ctr_, ATTN_CTR_N * sizeof(unsigned), hipMemcpyDeviceToHost));
    HIPCK(hipMemset(attn_ctr_, 0, ATTN_CTR_N * sizeof(unsigned)));
    attn_counting_ = enable != 0;
}

void* Engine::persist(size_t bytes, bool zero) {
    void* p = nullptr;
    HIPCK(hipMalloc(&p, std::max<size_t>(bytes, 256)));
    if (zero) HIPCK(hipMemset(p, 0, std::max<size_t>(bytes, 256)));
    owned_.push_back(p);
    persist_bytes_ += std::max<size_t>(bytes, 256);
    return p;
}

std::shared_ptr<Engine> Engine::fork(const std::shared_ptr<Engine>& parent, size_t arena_bytes) {
    if (!parent || !parent->finalized_) throw GlError(GL_ERR_STATE, "gl_ctx_fork: the parent context is not finalized");
    HIPCK(hipDeviceSynchronize());                     // (the first-conv copy below reads what the parent's streams may still be writing)
    std::shared_ptr<Engine> c(new Engine(*parent));    // every weight descriptor: plain pointers into the parent's allocations
    Engine& e = *c;
    e.parent_ = parent->parent_ ? parent->parent_ : parent;
    // ---- what a context owns itself
    e.owned_.clear();
    e.persist_bytes_ = 0;
    e.fold_tmps_.clear();
    e.arena_ = Arena{};
    e.ws_ = nullptr;
    e.ws_bytes_ = 0;
    e.cond_ = Cond{};
    e.attn_bufs_.clear();
    e.attn_ctr_ = nullptr;
    e.attn_counting_ = false;
    e.smp_ = Sampler{};
    e.train_events_.clear();
    e.fuser_kv_.clear();
    e.emb_table_ = nullptr; e.emb_cur_ = nullptr; e.emb_t_dev_ = nullptr; e.emb_table_cap_ = 0; e.emb_t_cache_.clear();
    e.train_events_recorded = false;
    e.profiling_ = false;
    e.prof_.clear();
    e.prof_pool_.clear();
    e.n_launches = 0;
    try {
        e.arena_.init(arena_bytes ? arena_bytes : parent->arena_.capacity());
        e.init_workspace();
        if (e.unet_.present) {
            const size_t n_st = e.unet_.st.size(), ng = 2 * n_st;
            e.gates_ = reinterpret_cast<float*>(e.persist(std::max<size_t>(ng, 1) * sizeof(float), true));
            e.fuser_scale_ = reinterpret_cast<float*>(e.persist(std::max<size_t>(n_st, 1) * sizeof(float), true));
            if (ng) HIPCK(hipMemcpy(e.gates_, parent->gates_, ng * sizeof(float), hipMemcpyDeviceToDevice));
            if (n_st) HIPCK(hipMemcpy(e.fuser_scale_, parent->fuser_scale_, n_st * sizeof(float), hipMemcpyDeviceToDevice));
            // the first conv is rewritten in place by gl_unet_restore_first_conv: a copy per context, in the parent's current state
            ConvW& c1 = e.unet_.conv_in_small;
            const int mc = e.unet_.cfg.model_channels;
            const size_t wb = (size_t)mc * c1.Kpad * sizeof(bf16);
            bf16* w = reinterpret_cast<bf16*>(e.persist(wb, false));
            float* b = reinterpret_cast<float*>(e.persist(mc * sizeof(float), false));
            HIPCK(hipMemcpy(w, c1.w, wb, hipMemcpyDeviceToDevice));
            HIPCK(hipMemcpy(b, c1.b, mc * sizeof(float), hipMemcpyDeviceToDevice));
            c1.w = w;
            c1.b = b;
        }
    } catch (...) {
        c.reset();
        throw;
    }
    return c;
}

void Engine::upload(const std::string& key, const void* src, int ndim, const int64_t* shape, bool is_device) {
    if (finalized_) throw GlError(GL_ERR_STATE, "weights cannot be uploaded after gl_finalize");
    RawTensor t;
    t.numel = 1;
    for (int i = 0; i < ndim; ++i) {
        t.shape.push_back(shape[i]);
        t.numel *= shape[i];
    }
    HIPCK(hipMalloc(reinterpret_cast<void**>(&t.p), std::max<int64_t>(t.numel, 4) * sizeof(float)));
    HIPCK(hipMemcpy(t.p, src, t.numel * sizeof(float), is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    auto it = raw_.find(key);
    if (it != raw_.end()) (void)hipFree(it->second.p);
    raw_[key] = t;
}

const RawTensor& Engine::raw(const std::string& key) const {
    auto it = raw_.find(key);
    if (it == raw_.end()) throw GlError(GL_ERR_MISSING, "missing weight '" + key + "'");
    return it->second;
}

// ---------------------------------------------------------------- weight packing
NormW Engine::norm(const std::string& p) {
    NormW n;
    n.g = F(p + ".weight");
    n.b = F(p + ".bias");
    n.C = (int)raw(p + ".weight").numel;
    return n;
}

const bf16* Engine::cast_rows(const std::vector<std::string>& keys) {
    int64_t total = 0;
    for (auto& k : keys) total += raw(k).numel;
    bf16* dst = reinterpret_cast<bf16*>(persist(total * sizeof(bf16), false));
    int64_t off = 0;
    for (auto& k : keys) {
        const RawTensor& t = raw(k);
        CK(cast_f32_bf16_launch(t.p, dst + off, t.numel, 0));
        off += t.numel;
    }
    return dst;
}

LinW Engine::linear(const std::string& p, bool bias) {
    LinW l;
    const RawTensor& w = raw(p + ".weight");
    l.N = (int)w.shape[0];
    l.K = (int)(w.numel / w.shape[0]);
    if (l.K % 64 != 0) {  // zero-pad K (keypoint PositionNet: 768 + 32 -> 832)
        int Kp = round_up(l.K, 64);
        bf16* dst = reinterpret_cast<bf16*>(persist((size_t)l.N * Kp * sizeof(bf16), false));
        CK(cast_pad_cols_launch(w.p, dst, l.N, l.K, Kp, 0));
        l.w = dst;
        l.K = Kp;
    } else {
        l.w = cast_rows({p + ".weight"});
    }
    l.b = bias ? F(p + ".bias") : nullptr;
    return l;
}

LinW Engine::conv1(const std::string& p) { return linear(p, true); }

bool Engine::upconv_phase_form(int Cin, int Cout) {
    static const bool on = !(dev_env("GL_UPCONV_PHASES") && atoi(dev_env("GL_UPCONV_PHASES")) == 0);
    return on && gemm_supports_qkv() /* (the v5 main loop) */ && Cin % 64 == 0 && Cout % 8 == 0;
}

ConvW Engine::conv3(const std::string& p, int Npad, bool up2x) {
    ConvW c;
    const RawTensor& w = raw(p + ".weight");
    if (w.shape.size() != 4 || w.shape[2] != 3 || w.shape[3] != 3) throw GlError(GL_ERR_ARG, "'" + p + ".weight' is not a 3x3 conv");
    c.Cout = (int)w.shape[0];
    c.Cin = (int)w.shape[1];
    c.Npad = Npad ? Npad : c.Cout;
    if (up2x && c.Npad == c.Cout && upconv_phase_form(c.Cin, c.Cout)) {
        bf16* dst = reinterpret_cast<bf16*>(persist((size_t)16 * c.Cout * c.Cin * sizeof(bf16), false));
        CK(pack_upconv_phases_launch(w.p, dst, c.Cout, c.Cin, c.Cout, 0));
        c.w4 = dst;
    } else {
        bf16* dst = reinterpret_cast<bf16*>(persist((size_t)c.Npad * 9 * c.Cin * sizeof(bf16), false));
        CK(pack_conv_weight_launch(w.p, dst, c.Cout, c.Cin, 3, 3, c.Npad, 0));
        c.w = dst;
    }
    if (c.Npad != c.Cout) {
        float* b = reinterpret_cast<float*>(persist(c.Npad * sizeof(float), true));
        HIPCK(hipMemcpy(b, F(p + ".bias"), c.Cout * sizeof(float), hipMemcpyDeviceToDevice));
        c.b = b;
    } else {
        c.b = F(p + ".bias");
    }
    return c;
}

// a conv3x3 over a few input channels, packed for the small im2col path (conv3x3_small): [Cout][9 * Cin padded to 64]
ConvW Engine::conv3_small(const std::string& p, int Cout) {
    ConvW c;
    const RawTensor& w = raw(p + ".weight");
    c.Cin = (int)w.shape[1];
    c.Cout = Cout;
    c.Kpad = round_up(9 * c.Cin, 64);
    bf16* dst = reinterpret_cast<bf16*>(persist((size_t)Cout * c.Kpad * sizeof(bf16), false));
    CK(pack_conv_small_launch(w.p, dst, Cout, c.Cin, c.Kpad, 0));
    c.w = dst;
    c.b = F(p + ".bias");
    return c;
}

Engine::FoldTmp Engine::fold_ln(const std::string& wkey, const float* bias, const NormW& n) {
    const RawTensor& w = raw(wkey);
    FoldTmp t;
    t.N = (int)w.shape[0];
    t.K = (int)(w.numel / w.shape[0]);
    if (n.C != t.K) throw GlError(GL_ERR_ARG, "'" + wkey + "': LayerNorm width does not match the projection's input width");
    HIPCK(hipMalloc(reinterpret_cast<void**>(&t.w), (size_t)t.N * t.K * sizeof(float)));
    HIPCK(hipMalloc(reinterpret_cast<void**>(&t.b), (size_t)t.N * sizeof(float)));
    fold_tmps_.push_back(t.w);
    fold_tmps_.push_back(t.b);
    CK(ln_fold_launch(w.p, bias, n.g, n.b, t.w, t.b, t.N, t.K, 0));
    return t;
}

FFW Engine::ffw(const std::string& p, int C, const NormW* fold, const std::string& pre_key, const std::string& post_key, const float* post_q_w,
                const float* post_q_b) {
    FFW f;
    f.C = C;
    const RawTensor& w = raw(p + ".net.0.proj.weight");
    const int C8 = (int)w.shape[0], K = (int)w.shape[1];
    if (C8 != 8 * C || K != C) throw GlError(GL_ERR_ARG, "'" + p + "' GEGLU projection has unexpected shape");
    bf16* wp = reinterpret_cast<bf16*>(persist((size_t)C8 * K * sizeof(bf16), false));
    float* bp = reinterpret_cast<float*>(persist(C8 * sizeof(float), false));
    f.geglu16 = gemm_geglu_layout();
    const float* wsrc = w.p;
    const float* bsrc = F(p + ".net.0.proj.bias");
    if (fold) {   // the LayerNorm in front of this feed-forward, folded into its GEGLU projection
        const FoldTmp t = fold_ln(p + ".net.0.proj.weight", bsrc, *fold);
        wsrc = t.w;
        bsrc = t.b;
    }
    CK(pack_geglu_launch(wsrc, bsrc, wp, bp, 4 * C, K, f.geglu16, 0));
    if (fold) {
        float* cs = reinterpret_cast<float*>(persist(C8 * sizeof(float), false));
        CK(rowsum_bf16_launch(wp, cs, C8, K, 0));
        f.csum1 = cs;
        f.folded = true;
    }
    f.w1 = wp;
    f.b1 = bp;
    f.w2 = linear(p + ".net.2");
    if (ff_rows_ && ff_stream_bytes(C)) {   // the row-local kernel's fragment stream of the same (folded) weights
        void* st = persist(ff_stream_bytes(C), false);
        CK(ff_pack_launch(wsrc, bsrc, raw(p + ".net.2.weight").p, st, C, 0));
        f.rows_stream = st;
        if (fold && !pre_key.empty()) {      // chained form: the projections around this feed-forward ride in the same stream
            const bool post = !post_key.empty();
            void* cs = persist(ff_chain_stream_bytes(C, true, post), false);
            CK(ff_chain_pack_launch(wsrc, bsrc, raw(p + ".net.2.weight").p, raw(pre_key).p, post ? raw(post_key).p : nullptr, cs, C, 0));
            f.chain_stream = cs;
            f.chain_post = post;
            if (!post && post_q_w && post_q_b && C == 320) {     // + the cross-attention's to_q behind the next LayerNorm (d = 40: C / 8 heads)
                void* cq = persist(ff_chain_stream_bytes(C, true, true), false);
                CK(ff_chain_pack_launch(wsrc, bsrc, raw(p + ".net.2.weight").p, raw(pre_key).p, post_q_w, cq, C, 0));
                float* qb = reinterpret_cast<float*>(persist((size_t)C * sizeof(float), false));
                HIPCK(hipMemcpy(qb, post_q_b, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice));
                f.chain_q_stream = cq;
                f.chain_q_bias = qb;
            }
        }
    }
    return f;
}

ResW Engine::resw(const std::string& p, int Cin, int Cout, bool unet) {
    ResW r;
    r.Cin = Cin;
    r.Cout = Cout;
    if (unet) {
        r.n1 = norm(p + ".in_layers.0");
        r.c1 = conv3(p + ".in_layers.2");
        r.n2 = norm(p + ".out_layers.0");
        r.c2 = conv3(p + ".out_layers.3");
        r.has_skip = has(p + ".skip_connection.weight");
        if (r.has_skip) r.skip = conv1(p + ".skip_connection");
    } else {
        r.n1 = norm(p + ".norm1");
        r.c1 = conv3(p + ".conv1");
        r.n2 = norm(p + ".norm2");
        r.c2 = conv3(p + ".conv2");
        r.has_skip = has(p + ".nin_shortcut.weight");
        if (r.has_skip) r.skip = conv1(p + ".nin_shortcut");
        if (has(p + ".conv_shortcut.weight")) throw GlError(GL_ERR_UNSUPPORTED, "'" + p + "': 3x3 conv_shortcut is not supported");
    }
    if (r.c1.Cin != Cin || r.c1.Cout != Cout || (Cin != Cout) != r.has_skip)
        throw GlError(GL_ERR_ARG, fmt("'%s': weights do not match the configured topology (%d -> %d)", p.c_str(), Cin, Cout));
    return r;
}

void Engine::finalize() {
    if (finalized_) throw GlError(GL_ERR_STATE, "gl_finalize called twice");
    HIPCK(hipSetDevice(device_));
    if (unet_.present) build_unet();
    if (vae_.dec.present) build_vae();
    if (vae_.dec.present && has("vae/encoder.conv_in.weight")) build_vae_encoder();
    if (clipt_.present) build_clip_text();
    if (clipv_.present) build_clip_vision();
    HIPCK(hipDeviceSynchronize());
    for (void* p : fold_tmps_) (void)hipFree(p);   // fp32 W * gamma / b + W beta temporaries of the folded LayerNorms
    fold_tmps_.clear();
    // matrices now live packed in bf16: drop their fp32 staging copies (vectors stay, they are used as is)
    for (auto it = raw_.begin(); it != raw_.end();) {
        if (it->second.shape.size() >= 2 && it->first.find("quant_conv") == std::string::npos && !keep_raw_.count(it->first)) {
            (void)hipFree(it->second.p);
            it = raw_.erase(it);
        } else {
            ++it;
        }
    }
    finalized_ = true;
}

// ---------------------------------------------------------------- execution helpers
// developer aid (GL_LAUNCH_LOG=file, tools/gpu_traffic.sh): one line per GEMM / conv / attention launch, in launch order
FILE* launch_log_file() {
    static FILE* f = dev_env("GL_LAUNCH_LOG") ? fopen(dev_env("GL_LAUNCH_LOG"), "w") : nullptr;
    return f;
}
AttnParams attn_params(const bf16* q, const bf16* k, const bf16* vt, bf16* o, int H, int d, int Nq, int Nk, int Tq_pad, int Tk_pad, int vt_layout) {
    AttnParams P{};
    P.q = q; P.k = k; P.vt = vt; P.o = o;
    P.H = H; P.d = d; P.Nq = Nq; P.Nk = Nk; P.Tq_pad = Tq_pad; P.Tk_pad = Tk_pad;
    P.ldo = H * d; P.o_rows_per_b = Nq; P.vt_layout = vt_layout;
    P.scale_log2e = (float)(1.4426950408889634 / std::sqrt((double)d));
    return P;
}

void Engine::attention(const bf16* q, const bf16* k, const bf16* vt, bf16* o, int B, int H, int d, int Nq, int Nk, int Tq_pad, int Tk_pad, int vt_layout,
                       hipStream_t s) {
    const AttnParams P = attn_params(q, k, vt, o, H, d, Nq, Nk, Tq_pad, Tk_pad, vt_layout);
    const char* sym = attn_kernel_name(d, Nk, vt_layout);
    {
        ProfScope ps(this, s, sym, 4.0 * B * H * (double)Nq * Nk * d, 0.0);
        CK(attn_launch(P, B, s));
        // attention launches in the launch log: symbol | Nq | Nk | d | mode 2 | algorithmic bytes (q, k, v read once, o written once, unpadded)
        if (FILE* f = launch_log_file()) {
            fprintf(f, "%s|%d|%d|%d|2|%.0f\n", sym, Nq, Nk, d, 2.0 * B * H * d * (2.0 * Nq + 2.0 * Nk));
            fflush(f);
        }
    }
    ++n_launches;
}

void Engine::gemm(const AOperand& A_in, const bf16* W, int M, int N, int K, const Epilogue& E, hipStream_t s) {
    ProfScope ps(this, s, "gemm", 2.0 * M * N * K, 0.0);
    AOperand A = A_in;
    // the stride-1 convs of the 8 x 8 level: conv8_kernel stages an image once per channel chunk (gemm.h A_CONV8; same weights)
    if (A.mode == A_CONV3 && gemm_conv8_supported(A, M, N, K, E)) A.mode = A_CONV8;
    CK(gemm_launch(A, W, M, N, K, E, ws_, ws_bytes_, s));
    if (profiling_) {
        static const bool by_shape = dev_env("GL_PROF_SHAPES") != nullptr;  // developer aid: one record per problem, not per symbol
        std::string nm = gemm_last_kernel_name();  // the symbol the tile selection actually launched
        if (by_shape) nm += fmt(" M%d N%d K%d", M, N, K);
        ps.rename(nm);
    }
    // developer aid (tools/gpu_traffic.sh): one line per GEMM / conv launch, in launch order, to join rocprofv3's per-dispatch
    // counter rows (which carry the kernel symbol but not the problem) with their shapes
    FILE* launch_log = launch_log_file();
    if (launch_log) {
        const double a_rows = A.mode != A_ROWS ? (double)(M / (A.Ho * A.Wo)) * A.Hin * A.Win : (double)M;
        const double out_b = E.mode == EPI_NCHW_F32 ? 4.0 * M * E.n_real : (E.act == ACT_GEGLU ? 1.0 : 2.0) * M * (double)N * (E.out_f32 ? 2 : 1);
        const double bytes = a_rows * (A.C0 + A.C1) * 2 + (double)N * K * 2 + out_b + (E.res ? 2.0 * M * N : 0.0);
        fprintf(launch_log, "%s|%d|%d|%d|%d|%.0f\n", gemm_last_kernel_name(), M, N, K, A.mode, bytes);
        fflush(launch_log);
    }
    {
        int tm, tn, sp;
        gemm_last_cfg(&tm, &tn, &sp);
        n_launches += sp > 1 ? 2 : 1;   // a split-K problem is followed by splitk_reduce_kernel
    }
}

bf16* Engine::linear_rows(const bf16* x, int M, const LinW& L, int act, const bf16* res, const float* gate, hipStream_t s, RowStats* stats) {
    bf16* out = arena_.get<bf16>((size_t)M * L.N);
    Epilogue E = e_rows_res(out, L.N, L.b, res);
    E.act = act;
    E.gate = gate;
    if (stats) {   // row statistics of the result, for the folded LayerNorm of the GEMM that reads it next
        *stats = RowStats{};
        if (ln_fold_ && L.N % 64 == 0) {
            stats->ld = L.N / 32;     // one slot per wave column block of the narrowest tile (64 x 64: 32 columns per wave)
            stats->p = arena_.get<float2>((size_t)M * stats->ld);
            E.stats_out = stats->p;
            E.stats_ld = stats->ld;
        }
    }
    gemm(a_rows(x, L.K), L.w, M, L.N, L.K, E, s);
    if (stats && stats->p) stats->nb = gemm_last_stats_nb();
    return out;
}

bf16* Engine::groupnorm(const TRef& x, int B, int HW, const NormW& n, float eps, bool silu, hipStream_t s) {
    const int C = x.C();
    if (n.C != C) throw GlError(GL_ERR_ARG, fmt("groupnorm: %d channels given to a norm with %d", C, n.C));
    bf16* y = arena_.get<bf16>((size_t)B * HW * C);
    GNParams P{};
    P.x0 = x.p0; P.C0 = x.C0; P.x1 = x.p1; P.C1 = x.C1;
    P.B = B; P.HW = HW; P.eps = eps; P.gamma = n.g; P.beta = n.b; P.y = y; P.silu = silu ? 1 : 0;
    P.partial = reinterpret_cast<float*>(arena_.alloc(gn_partial_bytes(B, HW)));
    ProfScope ps(this, s, HW <= 256 ? "gn_small_kernel" : "gn_stats_kernel + gn_apply_kernel", 0.0, 2.0 * B * HW * (double)C * 2);
    CK(groupnorm_launch(P, s));
    n_launches += HW <= 256 ? 1 : 2;   // gn_small_kernel, or gn_stats_kernel + gn_apply_kernel
    return y;
}

// GroupNorm32 -> SiLU -> conv3x3 (reference openaimodel.py:212-232 in_layers / out_layers; VAE model.py:118-141). Where the conv runs
// on conv_halo_kernel the GroupNorm keeps only its statistics pass (groupnorm_coef_launch) and the conv normalises + activates
// its input while staging it (AOperand::gn): the normalised copy is never written to HBM. Elsewhere: the two passes of rounds 1-5.
bf16* Engine::gn_silu_conv3x3(const TRef& x, int B, int H, int W, const NormW& n, float eps, const ConvW& c, const float* bias2, int bias2_ld,
                              const bf16* res, bf16* out, hipStream_t s) {
    if (x.C() != c.Cin || n.C != c.Cin) throw GlError(GL_ERR_ARG, fmt("gn_silu_conv3x3: %d channels into a norm of %d and a conv of %d", x.C(), n.C, c.Cin));
    const int HW = H * W, M = B * HW;
    if (!out) out = arena_.get<bf16>((size_t)M * c.Cout);
    AOperand A = a_conv3(x, H, W, H, W, 1, 0, 1);
    Epilogue E = e_rows_res(out, c.Cout, c.b, res);
    E.bias2 = bias2; E.bias2_ld = bias2_ld; E.rows_per_b = HW;
    if (gn_prologue_ && gemm_gn_prologue_supported(A, M, c.Cout, 9 * c.Cin, E)) {
        GNParams P{};
        P.x0 = x.p0; P.C0 = x.C0; P.x1 = x.p1; P.C1 = x.C1;
        P.B = B; P.HW = HW; P.eps = eps; P.gamma = n.g; P.beta = n.b; P.silu = 1;
        P.partial = reinterpret_cast<float*>(arena_.alloc(gn_partial_bytes(B, HW)));
        P.coef = reinterpret_cast<float*>(arena_.alloc(gn_coef_bytes(B, c.Cin)));
        {
            const int nl = groupnorm_coef_launches(HW, x.C0, x.C1);
            ProfScope ps(this, s, nl == 1 ? "gn_small_coef_kernel" : "gn_stats_kernel + gn_coef_kernel", 0.0, 1.0 * B * HW * (double)c.Cin * 2);
            CK(groupnorm_coef_launch(P, s));
            n_launches += nl;
        }
        A.gn = P.coef;
        gemm(A, c.w, M, c.Cout, 9 * c.Cin, E, s);
        ++n_prologue_convs;
        return out;
    }
    bf16* a = groupnorm(x, B, HW, n, eps, true, s);
    A.p0 = a; A.C0 = c.Cin; A.ld0 = c.Cin; A.p1 = nullptr; A.C1 = 0; A.ld1 = 0;
    gemm(A, c.w, M, c.Cout, 9 * c.Cin, E, s);
    return out;
}

bf16* Engine::layernorm(const bf16* x, int B, int N, int C, const NormW& n, bool pad64, hipStream_t s) {
    const int Tp = pad64 ? round_up(N, 64) : N;
    bf16* y = arena_.get<bf16>((size_t)B * Tp * C);
    LNParams P{};
    P.x = x; P.x2 = nullptr; P.B = B; P.N1 = N; P.N2 = 0; P.Tpad = Tp; P.C = C; P.eps = 1e-5f;
    P.gamma = n.g; P.beta = n.b; P.y = y;
    ProfScope ps(this, s, "ln_kernel", 0.0, 2.0 * B * N * (double)C * 2);
    CK(layernorm_launch(P, s));
    ++n_launches;
    return y;
}

bf16* Engine::layernorm_plain(const bf16* x, int B, int N, int C, bool pad64, hipStream_t s) {
    NormW none;
    none.C = C;
    return layernorm(x, B, N, C, none, pad64, s);
}

bf16* Engine::conv3x3(const TRef& x, int B, int Hin, int Win, const ConvW& c, int stride, int ups, int pad_lo,
                      const float* bias2, int bias2_ld, const bf16* res, hipStream_t s, bf16* out) {
    if (x.C() != c.Cin) throw GlError(GL_ERR_ARG, fmt("conv3x3: input has %d channels, weight expects %d", x.C(), c.Cin));
    if (c.w4) {
        // Upsample (reference openaimodel.py:54-82, VAE model.py:42-57) in phase form: four 2x2 convs on the source, 4/9 of the MACs.
        // A batch whose source tensor is beyond the kernel's 32-bit buffer offsets goes in pieces of whole images.
        if (stride != 1 || ups != 1 || pad_lo != 1 || bias2 || res) throw GlError(GL_ERR_ARG, "conv3x3: phase-form weights serve the plain upsample conv only");
        const int Mi = 4 * Hin * Win;
        if (!out) out = arena_.get<bf16>((size_t)B * Mi * c.Cout);
        auto ok = [&](int b) { return gemm_upconv_phases_supported(a_conv2up(x, Hin, Win), b * Mi, c.Cout, 4 * c.Cin, e_rows(out, c.Cout, c.b)); };
        int Bc = B;
        while (Bc > 1 && !ok(Bc)) Bc = (Bc + 1) / 2;
        if (!ok(Bc)) throw GlError(GL_ERR_UNSUPPORTED, fmt("conv3x3: no phase form for a %d x %d x %d -> %d upsample conv", Hin, Win, c.Cin, c.Cout));
        for (int b0 = 0; b0 < B; b0 += Bc) {
            const size_t px = (size_t)b0 * Hin * Win;
            const TRef xb{x.p0 + px * x.C0, x.C0, x.p1 ? x.p1 + px * x.C1 : nullptr, x.C1};
            gemm(a_conv2up(xb, Hin, Win), c.w4, std::min(Bc, B - b0) * Mi, c.Cout, 4 * c.Cin, e_rows(out + (size_t)b0 * Mi * c.Cout, c.Cout, c.b), s);
        }
        return out;
    }
    const int Hup = Hin << ups, Wup = Win << ups;
    const int Ho = stride == 1 ? Hup : (pad_lo ? (Hup + 2 - 3) / 2 + 1 : (Hup + 1 - 3) / 2 + 1);
    const int Wo = stride == 1 ? Wup : (pad_lo ? (Wup + 2 - 3) / 2 + 1 : (Wup + 1 - 3) / 2 + 1);
    const int M = B * Ho * Wo;
    if (!out) out = arena_.get<bf16>((size_t)M * c.Cout);
    Epilogue E = e_rows_res(out, c.Cout, c.b, res);
    E.bias2 = bias2; E.bias2_ld = bias2_ld; E.rows_per_b = Ho * Wo;
    gemm(a_conv3(x, Hin, Win, Ho, Wo, stride, ups, pad_lo), c.w, M, c.Cout, 9 * c.Cin, E, s);
    return out;
}

// ResBlock._forward (openaimodel.py:212-232) / VAE ResnetBlock.forward (model.py:118-141)
void Engine::replicate(const bf16* src, bf16* dst, size_t n, int reps, hipStream_t s) {
    ProfScope ps(this, s, "replicate_kernel", 0.0, (1.0 + reps) * n * 2);
    CK(replicate_launch(src, dst, n * sizeof(bf16), reps, s));
    ++n_launches;
}

bf16* Engine::resblock(const ResW& r, const TRef& x, int B, int H, int W, const float* embout, int emb_ld, float eps, hipStream_t s, bf16* out) {
    const int HW = H * W, M = B * HW;
    if (!out) out = arena_.get<bf16>((size_t)M * r.Cout);
    const size_t mk = arena_.mark();
    bf16* h = gn_silu_conv3x3(x, B, H, W, r.n1, eps, r.c1, embout ? embout + r.emb_off : nullptr, emb_ld, nullptr, nullptr, s);
    const bf16* sk;
    if (r.has_skip) {
        bf16* skb = arena_.get<bf16>((size_t)M * r.Cout);
        AOperand A{};
        A.p0 = x.p0; A.C0 = x.C0; A.ld0 = x.C0; A.p1 = x.p1; A.C1 = x.C1; A.ld1 = x.C1; A.mode = A_ROWS;
        gemm(A, r.skip.w, M, r.Cout, r.Cin, e_rows(skb, r.Cout, r.skip.b), s);
        sk = skb;
    } else {
        if (x.p1) throw GlError(GL_ERR_STATE, "identity skip over a concatenated input");
        sk = x.p0;
    }
    gn_silu_conv3x3(TRef{h, r.Cout, nullptr, 0}, B, H, W, r.n2, eps, r.c2, nullptr, 0, sk, out, s);
    arena_.release(mk);
    return out;
}

// A conv3x3 over a few input channels (the first conv of the UNet and of both VAE halves) as im2col + GEMM (K = 9 * Cin padded to 64).
// P: the source planes, batch and size of ONE im2col launch; `reps` launches fill consecutive row blocks (UNet: sample b reads
// x[b % xB], one launch per replica group)
bf16* Engine::conv3x3_small(const ConvW& c, Im2colParams P, int reps, hipStream_t s) {
    const size_t rows = (size_t)P.B * P.H * P.W;
    bf16* col = arena_.get<bf16>(reps * rows * c.Kpad);
    bf16* out = arena_.get<bf16>(reps * rows * c.Cout);
    P.Kpad = c.Kpad;
    for (int r = 0; r < reps; ++r) {
        P.out = col + r * rows * c.Kpad;
        CK(im2col_small_launch(P, s));
        ++n_launches;
    }
    gemm(a_rows(col, c.Kpad), c.w, (int)(reps * rows), c.Cout, c.Kpad, e_rows(out, c.Cout, c.b), s);
    return out;
}

// The last conv of the UNet and of both VAE halves: GroupNorm32 -> SiLU -> conv3x3 (Cout padded to c.Npad) -> NCHW fp32 [B][n_real][HW]
void Engine::gn_silu_conv3x3_nchw(const bf16* x, int C, int B, int H, int W, const NormW& n, float eps, const ConvW& c, int n_real, float* out, hipStream_t s) {
    const int HW = H * W;
    bf16* a = groupnorm(TRef{x, C, nullptr, 0}, B, HW, n, eps, true, s);
    Epilogue E;
    epilogue_defaults(E);
    E.mode = EPI_NCHW_F32; E.out = out; E.bias = c.b; E.rows_per_b = HW; E.n_real = n_real;
    gemm(a_conv3(TRef{a, C, nullptr, 0}, H, W, H, W, 1, 0, 1), c.w, B * HW, c.Npad, 9 * C, E, s);
}

AttnBufs& Engine::attn_bufs(int B, int H, int d, int Tq, int Tk, int dpv_layout, int slot) {
    const int Tq_pad = round_up(Tq, 128), Tk_pad = round_up(Tk, 64);
    int dp, dpv;
    CK(attn_dims(d, &dp, &dpv));
    if (dpv_layout) dpv = dpv_layout;      // (attn_vt_layout: the 16x16x32 P V kernel reads a 48-row V^T at d = 40)
    const AttnKey key{{B, H, d, Tq_pad, Tk_pad, dpv, slot}};    // every field in full (XOR-ed shifted fields let dpv = 64 vanish and 96 / 160 collide)
    auto it = attn_bufs_.find(key);
    if (it != attn_bufs_.end()) return it->second;
    AttnBufs b;
    b.Tq_pad = Tq_pad;
    b.Tk_pad = Tk_pad;
    b.q = reinterpret_cast<bf16*>(persist((size_t)B * H * Tq_pad * dp * sizeof(bf16), true));
    b.k = reinterpret_cast<bf16*>(persist((size_t)B * H * Tk_pad * dp * sizeof(bf16), true));
    b.vt = reinterpret_cast<bf16*>(persist((size_t)B * H * dpv * Tk_pad * sizeof(bf16), true));
    CK(attn_vt_ones_launch(b.vt, B * H, d, Tk_pad, 0, dpv));  // denominator row (attention.hip), once per buffer
    CK(attn_k_init_launch(b.k, B * H, d, Tk_pad, 0));     // d = 40: the stabiliser's multiplier column
    HIPCK(hipStreamSynchronize(0));
    return attn_bufs_.emplace(key, b).first->second;
}

}  // namespace gl
