// What the training path's translation units share and nobody else sees (train.h is the interface capi.hip and engine.h see):
//   train_ops.hip        the primitive kernels, the Ctx methods over them, the frozen-weight operand cache, AdamW
//   train_attention.hip  the VALU and MFMA attention kernels, Ctx::attn_fwd / attn_bwd
//   train_lora.hip       the low-rank products of LoRA adapters in training (fp32-input MFMA), lora_fwd / lora_bwd
//   train_lora_conv.hip  the low-rank products of an adapted 3 x 3 conv (the same MFMA over gathered neighbour rows)
//   train_layers.hip     block, SpatialTransformer, ResBlock, resample: *_check / *_forward / *_backward; the four slice entry points
//   train_spatial.hip    ConvNeXt tokenizer, GroundingDownsampler and the first conv of the spatial-map models
//   train_unet.hip       the whole iteration: grounding MLPs, time embedding, the layer list, unet_train_step
// Dependencies run downwards only: every unit uses train_ops, train_layers uses train_attention, train_unet uses train_layers and
// train_spatial. The build has no relocatable device code: a kernel is launched only from the unit that defines it, and what another
// unit needs from it is a host function declared here. Ctx::ew and the two member templates take the kernel / the builder from the
// calling unit; this header names no kernel.
#pragma once
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "arena.h"
#include "train.h"

namespace gl {

// operand copies of frozen parameters, kept across training steps (train.h); train_cache_* are in train_ops.hip
struct TrainWeightCache {
    struct Key {
        const void* p; int kind, a, b, c;
        bool operator<(const Key& o) const { return std::tie(p, kind, a, b, c) < std::tie(o.p, o.kind, o.a, o.b, o.c); }
    };
    std::map<Key, void*> m;
    size_t bytes = 0;
};

namespace train {

enum WeightForm { WF_ROWS = 1, WF_TRANSPOSED = 2, WF_CONV = 3, WF_CONV_DGRAD = 4 };

// An fp32 operand x of a matrix product as bf16: hi = bf16(x), lo = bf16(x - hi) (lo null: single-pass bf16, GL_TRAIN_BF16X1)
struct Split { bf16* hi; bf16* lo; };

// the side of a square grid of n tokens, 0 when n is not a square
inline int isqrt_exact(int n) {
    int r = (int)lround(sqrt((double)n));
    return r * r == n ? r : 0;
}

// erf GELU (F.gelu default): gelu(g) = g Phi(g), gelu'(g) = Phi(g) + g phi(g)
__device__ __forceinline__ float gelu_cdf(float g) { return 0.5f * (1.f + erff(g * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_pdf(float g) { return 0.3989422804014327f * __expf(-0.5f * g * g); }

// A LoRA adapter of one frozen Linear in training (train_lora.hip): y = x W^T + scale (x down^T) up^T, down [r][K], up [N][r], fp32;
// a null gradient pointer: that gradient is not formed. The table is keyed by the base weight's address.
struct LoraAdapter { const float* down; const float* up; float* g_down; float* g_up; int r; float scale; };
using LoraTable = std::unordered_map<const void*, LoraAdapter>;

// The arena, the stream and every primitive operation as a method. The methods are defined in train_ops.hip, attn_fwd / attn_bwd in
// train_attention.hip; their comments are with the definitions.
struct Ctx {
    Arena& ar;
    float* ws;
    size_t ws_bytes;
    hipStream_t s;
    TrainWeightCache* wc = nullptr;                            // null: every operand copy is built per product in the arena
    const std::unordered_set<const void*>* frozen = nullptr;   // parameter tensors the caller does not update (no gradient asked for)
    const LoraTable* lora = nullptr;                           // adapters in training; null: every launch is the unadapted step's
    const float* loss_w = nullptr;                             // per-sample loss weights [B] of the UNet step (train_run.hip); null: mse_loss

    void ck(int rc) const { if (rc != GL_OK) throw GlError(rc, gl::last_error()); }
    void hip(hipError_t e, const char* what) const { if (e != hipSuccess) throw GlError(GL_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
    float* f32(size_t n) const { return ar.get<float>(n); }
    static dim3 g1(size_t n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }
    // one thread per element, 256 per workgroup: every argument initialises a value of the kernel's own parameter type (no narrowing)
    template <class... P, class... A>
    void ew(void (*k)(P...), size_t n, A&&... a) const {
        hipLaunchKernelGGL(k, g1(n), dim3(256), 0, s, P{std::forward<A>(a)}...);
    }
    // ... into a new buffer of n_out floats, the kernel's last argument
    template <class... P, class... A>
    float* ew_new(void (*k)(P...), size_t n_out, size_t n, A&&... a) const {
        float* out = f32(n_out);
        ew(k, n, a..., out);
        return out;
    }
    struct LN { float* y; float* xhat; float* rstd; };
    struct GN { float* a; float* xhat; float* rstd; };
    struct Attn { float* o; float* lse; };

    // a bf16 operand copy of weight W: from the cache when W is frozen and a cache is attached (built on first use, on this stream), else
    // from the arena (released with the product's mark as before)
    template <class F>
    bf16* weight_operand(const float* W, WeightForm kind, int a, int b, size_t n_elems, F&& build) const {
        if (wc && frozen && frozen->count(W)) {
            const TrainWeightCache::Key key{W, kind, a, b, 0};
            auto it = wc->m.find(key);
            if (it != wc->m.end()) return reinterpret_cast<bf16*>(it->second);
            void* p = nullptr;
            hip(hipMalloc(&p, n_elems * sizeof(bf16)), "hipMalloc (training weight cache)");
            const size_t mk = ar.mark();
            build(reinterpret_cast<bf16*>(p));
            ar.release(mk);               // (fp32 temporaries of the build; stream order keeps their reuse safe)
            wc->m.emplace(key, p);
            wc->bytes += n_elems * sizeof(bf16);
            return reinterpret_cast<bf16*>(p);
        }
        bf16* d = ar.get<bf16>(n_elems);
        build(d);
        return d;
    }
    // out [M][N] fp32 = a w^T (+ bias) as hi.hi + lo.hi + hi.lo: one(a, w, bias, out) launches one bf16 product into an [M][N] fp32 buffer
    template <class F>
    void split_product(F&& one, const Split& a, const Split& w, int M, int N, const float* bias, float* out) const {
        one(a.hi, w.hi, bias, out);
        if (a.lo && w.lo) {
            const size_t mk = ar.mark();
            float* t1 = f32((size_t)M * N);
            float* t2 = f32((size_t)M * N);
            one(a.lo, w.hi, nullptr, t1);
            one(a.hi, w.lo, nullptr, t2);
            add3(out, t1, t2, (size_t)M * N);
            ar.release(mk);
        }
    }

    Split to_bf16(const float* src, size_t n) const;
    Split transposed(const float* src, int R, int Cc, int Rpad) const;
    void mm1(const bf16* a, const bf16* w, int M, int N, int K, const float* bias, float* out) const;
    void add3(float* dst, const float* a, const float* b, size_t n) const;
    void mm(const Split& a, const Split& w, int M, int N, int K, const float* bias, float* out) const;
    bf16* cat3_rows(const float* src, size_t R, int K, int side) const;
    bf16* cat3_transposed(const float* src, int R, int Cc, int Rpad, int side) const;
    bf16* cat3_rows_w(const float* W, int N, int K) const;
    bf16* cat3_transposed_w(const float* W, int N, int K) const;
    static bool split_precision();
    static bool one_launch();
    float* lin_fwd(const float* x, int M, int K, const float* W, const float* b, int N) const;
    float* lin_dgrad(const float* dy, int M, int N, const float* W, int K) const;
    void lin_wgrad(const float* dy, const float* x, int M, int N, int K, float* dW, float* db) const;
    float* conv_dgrad_weight(const float* w_oihw, int O, int I) const;
    float* conv3(const float* a, int B, int H, int W, const float* w_oihw, const float* bias, int Cin, int Cout, bool dgrad, int stride = 1, int ups = 0) const;
    LN ln_fwd(const float* x, int R, int Cc, const float* g, const float* b, float eps = 1e-5f) const;
    void ln_bwd(const float* dy, const LN& f, const float* g, int R, int Cc, float* dx, bool accumulate, float* dgamma, float* dbeta) const;
    GN gn_silu_fwd(const float* x, int B, int HW, int Cc, const float* g, const float* b, bool silu = true, float eps = 1e-5f) const;
    void gn_silu_bwd(const float* da, const GN& f, const float* g, const float* b, int B, int HW, int Cc, float* dx, bool accumulate, bool silu = true) const;
    void colsum(const float* a, const float* b, int R, int Cc, float* out) const;
    void dot_reduce(const float* a, const float* b, size_t n, const float* alpha, float scale, int mode, float* out) const;
    float* mse_loss(const float* y, const float* target, size_t n, float* loss) const;
    float* silu(const float* x, size_t n) const;
    float* geglu_fwd(const float* u, int R, int I) const;
    float* geglu_bwd(const float* dh, const float* u, int R, int I) const;
    float* gated_add(const float* a, const float* b, const float* alpha, float scale, size_t n, float* out = nullptr) const;
    float* gated_scale(const float* a, const float* alpha, float scale, size_t n) const;
    void add(float* dst, const float* src, size_t n) const;
    float* slice_rows(const float* src, int B, int stride_rows, int row0, int rows, int Cc) const;
    void put_rows(float* dst, int B, int stride_rows, int row0, const float* src, int rows, int Cc) const;
    Attn attn_fwd(int D, const float* q, const float* k, const float* v, int B, int H, int Nq, int Nk) const;
    void attn_bwd(int D, const float* q, const float* k, const float* v, const Attn& f, const float* dout, int B, int H, int Nq, int Nk, float* dq, float* dk,
                  float* dv) const;
};

// ---- train_ops.hip: the small kernels more than one other unit uses, each behind a function
float* pad_cols(const Ctx& c, const float* src, int R, int K, int Kp);
void split_cols(const Ctx& c, const float* src, int ld, int c0, int Cc, size_t rows, float* dst, bool accumulate);
float* lin_fwd_any(const Ctx& c, const float* x, int M, int K, const float* W, const float* b, int N);
float* lin_dgrad_any(const Ctx& c, const float* dy, int M, int N, const float* W, int K);
void lin_wgrad_unpad(const Ctx& c, const float* dy, const float* xp, int M, int N, int K, int Kp, float* dW, float* db);
float* silu_bwd(const Ctx& c, const float* dy, const float* x, size_t n);
void null_grad(const Ctx& c, const float* g, const float* masks, int R, int ld, int c0, int n, float* out, bool accumulate);
float* conv3x3_direct(const Ctx& c, const float* x, const float* w, const float* bias, int B, int H, int W, int Cin, int Cout);

// ---- train_lora.hip: the low-rank products on the fp32-input MFMA, and the adapter term of a Linear whose weight is in c.lora
// (no entry: nothing is launched)
void lora_check(const char* what, int M, int K, int N, int r);
int lora_wgrad_chunk_rows(int M);       // rows per partial sum of a weight gradient: a function of M alone
void lora_down(const Ctx& c, const float* X, int M, int K, const float* A, int r, bool a_kr, float* T);                      // T = X A^T, A [r][K] or [K][r]
void lora_up(const Ctx& c, const float* T, int M, int r, const float* Bm, int N, bool b_rn, float s, float* Y);              // Y += s T B, B [N][r] or [r][N]
void lora_wgrad(const Ctx& c, const float* T, const float* Z, int M, int r, int N, float s, bool transposed, float* G);      // G [r][N] (or ^T) = s T^T Z
const LoraAdapter* lora_find(const Ctx& c, const float* W);
void lora_fwd(const Ctx& c, const float* W, const float* x, int M, int K, int N, float* y);                                  // y += s (x down^T) up^T
// dx (optional) += s (dy up) down; the adapter's gradients g_down = s (dy up)^T x, g_up = s dy^T (x down^T)
void lora_bwd(const Ctx& c, const float* W, const float* dy, const float* x, int M, int K, int N, float* dx);

// ---- train_lora_conv.hip: the low-rank products of an adapted 3 x 3 conv over pixel rows [B H W][C], down [r][Ci][3][3] (OIHW), for
// the geometries of Ctx::conv3: geom 0 stride 1, 1 Downsample (output H/2 x W/2), 2 Upsample (output 2H x 2W); H, W: the input's
constexpr size_t kLoraConvWgradWs = (size_t)64 << 20;   // partial sums of all nine taps at once up to this many bytes, else tap by tap
void lora_conv_check(const char* what, int B, int H, int W, int Ci, int Co, int r, int geom);
size_t lora_conv_out_rows(int geom, int B, int H, int W);
int lora_conv_wgrad_taps(int n_chunks, int r, int Ci);  // taps per launch of the weight gradient: 9 or 1, a function of the shape alone
void lora_conv_down(const Ctx& c, const float* X, int B, int H, int W, int Ci, const float* down, int r, int geom, float* T);             // T [Mo][r] = im2col(X) down^T
void lora_conv_dgrad(const Ctx& c, const float* U, int B, int H, int W, int Ci, const float* down, int r, int geom, float s, float* dX);  // dX [Mi][Ci] += s (transposed conv of U)
void lora_conv_wgrad(const Ctx& c, const float* U, const float* X, int B, int H, int W, int Ci, int r, int geom, float s, float* G);      // G (OIHW) = s U^T im2col(X)
// the adapter term of a 3 x 3 conv whose weight is in c.lora (no entry: nothing is launched): y += s up(down(x)); dx (optional) += its
// data gradient, and the adapter's gradients g_down, g_up (t is recomputed, as lora_bwd does)
void lora_conv_fwd(const Ctx& c, const float* W, const float* x, int B, int H, int Wd, int Ci, int Co, int geom, float* y);
void lora_conv_bwd(const Ctx& c, const float* W, const float* dy, const float* x, int B, int H, int Wd, int Ci, int Co, int geom, float* dx);
// out [B][C] = the sum of g [B][HW][C] over the HW pixels of each sample, in a fixed order (the gradient of a ResBlock's emb_layers output)
void lora_sample_colsum(const Ctx& c, const float* g, int B, int HW, int C, float* out);

// ---- train_layers.hip: the UNet's layer kinds. *_forward keeps what the backward needs in the arena; *_backward takes g = dL/dy
// Everything the backward of a BasicTransformerBlock needs from its forward
struct BlockSaved {
    Ctx::LN n1, nf1, nf2, n2, n3;
    Ctx::Attn a1, af, a2;
    float *q1, *k1, *v1, *qf, *kf, *vf, *q2, *k2, *v2;
    float *af_vis, *of, *uf, *hf, *ff_f, *u3;     // af_vis: the rows fuser.attn.to_out read; of: what alpha_attn gates
    float* nf1_tail = nullptr;                    // gatedSA2: norm1's output at the grounding tokens, the rows to_q read
};
struct STSaved {
    Ctx::GN n0;
    BlockSaved blk;
    float* yb = nullptr;        // the block's output, proj_out's input (read by an adapter's backward)
};
struct ResSaved {
    Ctx::GN n1, n2;
    const float* x = nullptr;           // the block's input and SiLU(emb): read by the backward of adapters on skip_connection / emb_layers.1
    const float* silu_emb = nullptr;
};
void st_check(const TrainBlockDims& d, const float* const* P, float* const* G = nullptr);
STSaved st_forward(const Ctx& c, const TrainBlockDims& d, const float* const* P, const float* x, const float* objs, const float* context, float* y);
void st_backward(const Ctx& c, const TrainBlockDims& d, const float* const* P, const STSaved& S, const float* objs, float* g, float* dobjs, float* const* G,
                 const float* context = nullptr);      // context: read only by adapters on attn2.to_k / to_v
void res_check(const TrainResDims& d, const float* const* P);
ResSaved res_forward(const Ctx& c, const TrainResDims& d, const float* const* P, const float* x, const float* silu_emb, float* y);
float* res_backward(const Ctx& c, const TrainResDims& d, const float* const* P, const ResSaved& S, float* g);
float* resample_forward(const Ctx& c, int mode, int B, int H, int W, int C, const float* w_oihw, const float* bias, const float* x);
float* resample_backward(const Ctx& c, int mode, int B, int H, int W, int C, const float* w_oihw, const float* g,
                        const float* x = nullptr);        // x: the layer's input, read only by an adapter on the conv

// ---- train_unet.hip: the model's state_dict by name, and what the stages of a step share
struct Names {
    std::unordered_map<std::string, int> idx;
    const float* const* params;
    float* const* grads;
    const float* w(const std::string& k) const;
    bool has(const std::string& k) const;
    float* g(const std::string& k) const;
};
struct UNetStep {
    const Ctx& c; const Names& nm; const TrainUNetCfg& cfg; const TrainUNetIn& in; const TrainSpatialIn* spatial; const char* const* block_names;
    int B, H0, W0, mc, ED, KD, Ng;
    int GK, NB, MRB, NC;            // grounding kind, boxes per sample, B NB rows per MLP, coordinates per box
    int PWr, PW;                    // the MLPs' input width, and padded to the GEMM's 64-step
    int NBR, MR;                    // MLP branches (text+image: 2), B Ng rows of objs
    int Cx, Ce, Ci, Cin0;           // conv_in reads Cx latent + Ce downsampler channels, or + Ci = Cx + 1 inpainting channels
    size_t M0;                      // B H0 W0 pixel rows
    std::string null_pos;
};

// ---- train_spatial.hip: the spatial-map models (grounding_kind 3) and the first conv
constexpr int kCnxDims[4] = {96, 192, 384, 768};       // ConvNeXt-tiny (convnext.py:203-207)
struct CnxBlockSaved { std::string p; const float* x; Ctx::LN n; float *u, *a, *h2; };
struct CnxDownSaved { std::string p; Ctx::LN l; float* col; int C, Cn; };
struct SpatialSaved {
    int R = 0, Cuse = 0, H = 0, M = 0;          // H: the last stage's grid side; M = B H H rows (B T tokens)
    float *img = nullptr, *img3 = nullptr, *col0 = nullptr, *w0p = nullptr;
    Ctx::LN stem_ln{};
    CnxDownSaved down[3];
    std::vector<CnxBlockSaved> blocks[4];
    float* mix = nullptr;                         // the MLP's input rows [B T][768]
};
struct DsSaved { float *r = nullptr, *a1 = nullptr, *s1 = nullptr, *out = nullptr; };
SpatialSaved spatial_forward(const Ctx& c, const Names& nm, const TrainUNetCfg& cfg, const TrainSpatialIn& sp, int B);
void spatial_backward(const Ctx& c, const Names& nm, const TrainUNetCfg& cfg, const TrainSpatialIn& sp, int B, const SpatialSaved& t, const float* g_mix);
bool downsampler_grads(const Names& nm);
float* conv_in_forward(const UNetStep& u, DsSaved& dsv, const float*& xin);
void conv_in_backward(const Ctx& c, const Names& nm, const TrainSpatialIn* spatial, const DsSaved& dsv, const float* xin, int B, int H0, int W0, int Cx,
                      int Ce, int Ci, int mc, const float* g);

}  // namespace train

}  // namespace gl
