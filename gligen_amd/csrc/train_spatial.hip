// The spatial-map models of the training path for gfx950 (grounding_kind 3: canny / depth / normal / hed / sem_grounding_net.py +
// *_grounding_downsampler.py): the ConvNeXt-tiny tokenizer (convnext.py:36-50, 71-81, 108-112), the GroundingDownsampler and the
// 4 + k channel first conv, forward in fp32 with every activation kept, and their backward. Matrix products go through the
// three-pass helpers of Ctx (train_ops.hip); the kernels below are the rest. Every reduction is a fixed-order sum (Ctx::colsum, the
// GEMMs, dwconv7_wgrad_kernel): no float atomics.
#include "train_impl.h"

#include "classmap.h"
#include "convnext.h"
#include "misc.h"

namespace gl {

using namespace train;

namespace {

// y = x + gamma h (gamma null: 1)   (Block.forward, convnext.py:47-50: layer scale, then the residual)
__global__ void layer_scale_residual_kernel(const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ gamma, int Cc, size_t n,
                                            float* __restrict__ y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = x[i] + (gamma ? gamma[i % Cc] : 1.f) * h[i];
}
// out = g gamma (per column)
__global__ void scale_cols_kernel(const float* __restrict__ g, const float* __restrict__ gamma, int Cc, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = g[i] * gamma[i % Cc];
}
__global__ void gelu_fwd_kernel(const float* __restrict__ u, size_t n, float* __restrict__ a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = u[i] * gelu_cdf(u[i]);
}
__global__ void gelu_bwd_kernel(const float* __restrict__ da, const float* __restrict__ u, size_t n, float* __restrict__ du) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = u[i];
    du[i] = da[i] * (gelu_cdf(g) + g * gelu_pdf(g));
}
// depthwise 7 x 7 conv, pad 3, over pixel rows [B][H][W][C] (convnext.py:38): y = bias + sum_taps w x. flip = 1: the taps rotated by
// 180 degrees -- the data gradient of the same conv (bias null); accumulate: y +=
__global__ void dwconv7_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int H, int W, int Cc, size_t n,
                                   int flip, int accumulate, float* __restrict__ y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Cc), xw = (int)((i / Cc) % W), yh = (int)((i / ((size_t)Cc * W)) % H);
    const size_t b = i / ((size_t)Cc * W * H);
    const float* wc = w + (size_t)c * 49;
    float acc = bias ? bias[c] : 0.f;
    for (int ky = 0; ky < 7; ++ky) {
        const int yy = yh + ky - 3;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 7; ++kx) {
            const int xx = xw + kx - 3;
            if (xx < 0 || xx >= W) continue;
            const int t = ky * 7 + kx;
            acc = fmaf(x[((b * H + yy) * W + xx) * Cc + c], wc[flip ? 48 - t : t], acc);
        }
    }
    y[i] = accumulate ? y[i] + acc : acc;
}
// depthwise weight gradient dw[c][tap] = sum over (b, y, x) of g[b][y][x][c] x[b][y + ky - 3][x + kx - 3][c]: grid (C / 64, 49), 64 channels
// x 16 pixel lanes; each lane sums pixels ry, ry + 16, .. in order, the 16 partials are added in a fixed order
__global__ void __launch_bounds__(1024) dwconv7_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, int B, int H, int W, int Cc,
                                                             float* __restrict__ dw) {
    __shared__ float part[16][64];
    const int tx = threadIdx.x & 63, ry = threadIdx.x >> 6, c = blockIdx.x * 64 + tx, tap = blockIdx.y, ky = tap / 7, kx = tap % 7;
    const int P = B * H * W;
    float s = 0.f;
    if (c < Cc)
        for (int p = ry; p < P; p += 16) {
            const int xw = p % W, yh = (p / W) % H, b = p / (W * H);
            const int yy = yh + ky - 3, xx = xw + kx - 3;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            s = fmaf(g[(size_t)p * Cc + c], x[(((size_t)b * H + yy) * W + xx) * Cc + c], s);
        }
    part[ry][tx] = s;
    __syncthreads();
    if (ry == 0 && c < Cc) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += part[i][tx];
        dw[(size_t)c * 49 + tap] = t;
    }
}
// im2col of a k x k conv (stride, pad) over an image addressed by strides (NCHW or pixel rows): out [B Ho Wo][Kp], column c k^2 + ky k + kx
// (the OIHW order of the weight); zero for taps outside the image and for columns >= Cin k^2
__global__ void im2col_f32_kernel(const float* __restrict__ x, int Cin, int H, int W, size_t sb, size_t sc, size_t sy, size_t sx, int k, int stride, int pad,
                                  int Ho, int Wo, int Kp, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int col = (int)(i % Kp);
    const size_t m = i / Kp;
    const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho);
    const size_t b = m / ((size_t)Wo * Ho);
    float v = 0.f;
    if (col < Cin * k * k) {
        const int c = col / (k * k), t = col % (k * k);
        const int iy = oy * stride - pad + t / k, ix = ox * stride - pad + t % k;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[b * sb + (size_t)c * sc + (size_t)iy * sy + (size_t)ix * sx];
    }
    out[i] = v;
}
// the adjoint of a patchify (im2col with stride == k, no padding: a permutation): dx (addressed by strides) from dp [B Ho Wo][ldp]
__global__ void unpatchify_kernel(const float* __restrict__ dp, int ldp, int Cin, int H, int W, int k, size_t sb, size_t sc, size_t sy, size_t sx, size_t n,
                                  float* __restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Cin), xw = (int)((i / Cin) % W), yh = (int)((i / ((size_t)Cin * W)) % H);
    const size_t b = i / ((size_t)Cin * W * H);
    const int Ho = H / k, Wo = W / k;
    dx[b * sb + (size_t)c * sc + (size_t)yh * sy + (size_t)xw * sx] =
        dp[((b * Ho + yh / k) * Wo + xw / k) * ldp + (size_t)c * k * k + (yh % k) * k + xw % k];
}
// objs = feat m_b + null (1 - m_b) + pos   (canny_grounding_net.py:48-56), rows [B][T][C]
__global__ void token_mix_f32_kernel(const float* __restrict__ feat, const float* __restrict__ mask, const float* __restrict__ null_feat,
                                     const float* __restrict__ pos, int T, int Cc, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Cc), t = (int)((i / Cc) % T);
    const float m = mask[i / ((size_t)Cc * T)];
    out[i] = feat[i] * m + null_feat[c] * (1.f - m) + pos[(size_t)t * Cc + c];
}
// its backward: dfeat = g m_b; the per-row mask of null_grad_kernel; d pos[t][c] = sum_b g[b][t][c] (b in order)
__global__ void mask_rows_kernel(const float* __restrict__ g, const float* __restrict__ mask, int T, int Cc, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = g[i] * mask[i / ((size_t)T * Cc)];
}
__global__ void expand_mask_kernel(const float* __restrict__ mask, int T, int n, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = mask[i / T];
}
__global__ void sum_batch_kernel(const float* __restrict__ g, int B, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += g[(size_t)b * n + i];
    out[i] = s;
}
// h = cat([x, e], dim = 1) as pixel rows (openaimodel.py:442-444): x rows [B HW][C0], e NCHW [B][C1][HW] -> [B HW][C0 + C1]
__global__ void cat_rows_nchw_kernel(const float* __restrict__ x, int C0, const float* __restrict__ e, int C1, int HW, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int C = C0 + C1, c = (int)(i % C);
    const size_t r = i / C, p = r % HW, b = r / HW;
    out[i] = c < C0 ? x[r * C0 + c] : e[(b * C1 + (c - C0)) * HW + p];
}
// data gradient of Conv2d(k 4, stride 2, pad 1) (GroundingDownsampler layers.2): g pixel rows [B][Ho Wo][Cout] -> dx NCHW [B][Cin][H][W]
__global__ void conv4x4s2_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ w, int Cin, int Cout, int H, int W, size_t n,
                                       float* __restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ix = (int)(i % W), iy = (int)((i / W) % H), ci = (int)((i / ((size_t)W * H)) % Cin);
    const size_t b = i / ((size_t)W * H * Cin);
    const int Ho = H / 2, Wo = W / 2;
    float acc = 0.f;
    for (int ky = 0; ky < 4; ++ky) {
        const int ty = iy + 1 - ky;          // iy = 2 oy - 1 + ky
        if (ty < 0 || (ty & 1) || (ty >> 1) >= Ho) continue;
        for (int kx = 0; kx < 4; ++kx) {
            const int tx = ix + 1 - kx;
            if (tx < 0 || (tx & 1) || (tx >> 1) >= Wo) continue;
            const float* gp = g + ((b * Ho + (ty >> 1)) * Wo + (tx >> 1)) * Cout;
            for (int co = 0; co < Cout; ++co) acc = fmaf(gp[co], w[((size_t)co * Cin + ci) * 16 + ky * 4 + kx], acc);
        }
    }
    dx[i] = acc;
}

float* gelu_fwd(const Ctx& c, const float* u, size_t n) { return c.ew_new(gelu_fwd_kernel, n, n, u, n); }
float* gelu_bwd(const Ctx& c, const float* da, const float* u, size_t n) { return c.ew_new(gelu_bwd_kernel, n, n, da, u, n); }

struct Strides { size_t b, c, y, x; };
Strides nchw(int Cc, int H, int W) { return {(size_t)Cc * H * W, (size_t)H * W, (size_t)W, 1}; }
Strides pixel_rows(int Cc, int H, int W) { return {(size_t)H * W * Cc, 1, (size_t)W * Cc, (size_t)Cc}; }

float* im2col(const Ctx& c, const float* x, int B, int Cin, int H, int W, Strides st, int k, int stride, int pad, int Ho, int Wo, int Kp) {
    const size_t n = (size_t)B * Ho * Wo * Kp;
    float* d = c.f32(n);
    c.ew(im2col_f32_kernel, n, x, Cin, H, W, st.b, st.c, st.y, st.x, k, stride, pad, Ho, Wo, Kp, n, d);
    return d;
}
// the adjoint of a k x k patchify: dp [B (H/k) (W/k)][ldp] -> pixel rows [B][H W][Cin]
float* unpatchify(const Ctx& c, const float* dp, int ldp, int B, int Cin, int H, int W, int k) {
    const size_t n = (size_t)B * H * W * Cin;
    float* dx = c.f32(n);
    const Strides r = pixel_rows(Cin, H, W);
    c.ew(unpatchify_kernel, n, dp, ldp, Cin, H, W, k, r.b, r.c, r.y, r.x, n, dx);
    return dx;
}
// weight (OIHW) and bias gradient of a k x k conv as an im2col of its input + lin_wgrad: x addressed by strides, dy pixel rows [B Ho Wo][Cout]
void conv_wgrad(const Ctx& c, const float* x, int B, int Cin, int H, int W, Strides st, int k, int stride, int pad, int Ho, int Wo, const float* dy,
                int Cout, float* dW, float* db) {
    if (!dW && !db) return;
    const int K = Cin * k * k, Kp = round_up(K, 64), M = B * Ho * Wo;
    const size_t mk = c.ar.mark();
    const float* col = dW ? im2col(c, x, B, Cin, H, W, st, k, stride, pad, Ho, Wo, Kp) : nullptr;
    lin_wgrad_unpad(c, dy, col, M, Cout, K, Kp, dW, db);
    c.ar.release(mk);
}

// the same two gradients from the u8 class map that stands for the one-hot planes x (classmap.h): dy binned by the class under each tap
void class_wgrad(const Ctx& c, int kind, const uint8_t* cls, const float* dy, ClassDyStrides ds, int B, int H, int W, int n_classes, int Cout, int R, float* dW,
                 float* db) {
    if (!dW && !db) return;
    const size_t mk = c.ar.mark();
    size_t n = 0;
    c.ck(class_conv_wgrad_partial_floats(kind, B, H, W, n_classes, Cout, R, &n));
    c.ck(class_conv_wgrad_launch(kind, cls, dy, ds, c.f32(n), dW, db, B, H, W, n_classes, Cout, R, c.s));
    c.ar.release(mk);
}

const char* const kPN = "position_net.";
const char* const kBB = "position_net.convnext_tiny_backbone.";

}  // namespace

// PositionNet.forward up to the MLP (canny_grounding_net.py:38-56; sem: nearest resize + in_conv first, sem_grounding_net.py:40-49)
SpatialSaved train::spatial_forward(const Ctx& c, const Names& nm, const TrainUNetCfg& cfg, const TrainSpatialIn& sp, int B) {
    hipStream_t s = c.s;
    const std::string PN = kPN, BB = kBB;
    SpatialSaved t;
    const int R = cfg.tok_resize;
    t.R = R;
    t.Cuse = cfg.tok_in_dim ? cfg.tok_in_dim : 3;
    if (R < 32 || R % 32) throw GlError(GL_ERR_ARG, "unet_train_step: tok_resize must be a positive multiple of 32");
    if (sp.map_cls) {     // the class map: the nearest resize and in_conv are one gather (classmap.h), the resized planes never exist
        if (!cfg.tok_in_dim)
            throw GlError(GL_ERR_UNSUPPORTED, "unet_train_step: a class map was given to a tokenizer without in_dim (canny, hed, depth, normal read an image, not classes)");
        if (!sp.mask) throw GlError(GL_ERR_ARG, "unet_train_step: null mask");
        t.img3 = c.f32((size_t)B * 3 * R * R);
        c.ck(class_inconv_launch(sp.map_cls, nm.w(PN + "in_conv.weight"), nm.w(PN + "in_conv.bias"), t.img3, B, sp.Ht, sp.Wt, cfg.tok_in_dim, R, s));
    } else {
        if (!sp.map || !sp.mask || sp.Ct < t.Cuse) throw GlError(GL_ERR_ARG, fmt("unet_train_step: the tokenizer reads %d map channels", t.Cuse));
        t.img = c.f32((size_t)B * t.Cuse * R * R);
        c.ck(resize_f32_launch(sp.map, t.img, B, sp.Ct, t.Cuse, sp.Ht, sp.Wt, R, 1, s));      // F.interpolate(x, resize_input): nearest
        t.img3 = t.img;
    }
    if (cfg.tok_in_dim && !sp.map_cls) {
        t.img3 = c.f32((size_t)B * 3 * R * R);
        c.ck(conv3x3_f32_launch(t.img, nm.w(PN + "in_conv.weight"), nm.w(PN + "in_conv.bias"), t.img3, B, t.Cuse, 3, R, R, s));
    }
    // stem: Conv2d(3, 96, 4, 4) as patches [B (R/4)^2][48 -> 64] times the OIHW weight as rows, then LayerNorm (convnext.py:71-74)
    int H = R / 4, C = kCnxDims[0], M = B * H * H;
    t.col0 = im2col(c, t.img3, B, 3, R, R, nchw(3, R, R), 4, 4, 0, H, H, 64);
    t.w0p = pad_cols(c, nm.w(BB + "downsample_layers.0.0.weight"), C, 48, 64);
    float* x = c.lin_fwd(t.col0, M, 64, t.w0p, nm.w(BB + "downsample_layers.0.0.bias"), C);
    t.stem_ln = c.ln_fwd(x, M, C, nm.w(BB + "downsample_layers.0.1.weight"), nm.w(BB + "downsample_layers.0.1.bias"), 1e-6f);
    x = t.stem_ln.y;
    for (int st = 0; st < 4; ++st) {
        if (st > 0) {     // LayerNorm + Conv2d(C, C', 2, 2) (convnext.py:76-81)
            CnxDownSaved& d = t.down[st - 1];
            d.p = BB + fmt("downsample_layers.%d", st);
            d.C = C;
            d.Cn = kCnxDims[st];
            d.l = c.ln_fwd(x, M, C, nm.w(d.p + ".0.weight"), nm.w(d.p + ".0.bias"), 1e-6f);
            d.col = im2col(c, d.l.y, B, C, H, H, pixel_rows(C, H, H), 2, 2, 0, H / 2, H / 2, 4 * C);
            H /= 2;
            M /= 4;
            x = c.lin_fwd(d.col, M, 4 * C, nm.w(d.p + ".1.weight"), nm.w(d.p + ".1.bias"), d.Cn);
            C = d.Cn;
        }
        for (int j = 0; nm.has(BB + fmt("stages.%d.%d.dwconv.weight", st, j)); ++j) {      // Block.forward (convnext.py:36-50)
            CnxBlockSaved b;
            b.p = BB + fmt("stages.%d.%d", st, j);
            b.x = x;
            const size_t n = (size_t)M * C;
            float* dw = c.f32(n);
            c.ew(dwconv7_f32_kernel, n, x, nm.w(b.p + ".dwconv.weight"), nm.w(b.p + ".dwconv.bias"), H, H, C, n, 0, 0, dw);
            b.n = c.ln_fwd(dw, M, C, nm.w(b.p + ".norm.weight"), nm.w(b.p + ".norm.bias"), 1e-6f);
            b.u = lin_fwd_any(c, b.n.y, M, C, nm.w(b.p + ".pwconv1.weight"), nm.w(b.p + ".pwconv1.bias"), 4 * C);
            b.a = gelu_fwd(c, b.u, 4 * n);
            b.h2 = c.lin_fwd(b.a, M, 4 * C, nm.w(b.p + ".pwconv2.weight"), nm.w(b.p + ".pwconv2.bias"), C);
            float* y = c.f32(n);
            c.ew(layer_scale_residual_kernel, n, x, b.h2, nm.has(b.p + ".gamma") ? nm.w(b.p + ".gamma") : nullptr, C, n, y);
            x = y;
            t.blocks[st].push_back(b);
        }
        if (t.blocks[st].empty()) throw GlError(GL_ERR_MISSING, fmt("unet_train_step: ConvNeXt stage %d has no blocks", st));
    }
    t.H = H;
    t.M = M;
    t.mix = c.f32((size_t)M * C);
    c.ew(token_mix_f32_kernel, (size_t)M * C, x, sp.mask, nm.w(PN + "null_feature"), nm.w(PN + "pos_embedding"), H * H, C, (size_t)M * C, t.mix);
    return t;
}

// No gradient is formed for the map itself.
void train::spatial_backward(const Ctx& c, const Names& nm, const TrainUNetCfg& cfg, const TrainSpatialIn& sp, int B, const SpatialSaved& t, const float* g_mix) {
    hipStream_t s = c.s;
    const std::string PN = kPN, BB = kBB;
    int H = t.H, M = t.M, C = kCnxDims[3];
    const int T = H * H;
    if (float* gp = nm.g(PN + "pos_embedding")) c.ew(sum_batch_kernel, (size_t)T * C, g_mix, B, (size_t)T * C, gp);
    if (float* gp = nm.g(PN + "null_feature")) {
        float* mr = c.f32(M);
        c.ew(expand_mask_kernel, M, sp.mask, T, M, mr);
        null_grad(c, g_mix, mr, M, C, 0, C, gp, false);
    }
    float* g = c.f32((size_t)M * C);
    c.ew(mask_rows_kernel, (size_t)M * C, g_mix, sp.mask, T, C, (size_t)M * C, g);
    for (int st = 3; st >= 0; --st) {
        for (int j = (int)t.blocks[st].size() - 1; j >= 0; --j) {
            const CnxBlockSaved& b = t.blocks[st][j];
            const size_t n = (size_t)M * C;
            const float* gam = nm.has(b.p + ".gamma") ? nm.w(b.p + ".gamma") : nullptr;
            const float* gh2 = g;
            if (gam) {      // y = x + gamma h2: d gamma = sum_rows g h2, dh2 = g gamma
                if (float* gg = nm.g(b.p + ".gamma")) c.colsum(g, b.h2, M, C, gg);
                float* t2 = c.f32(n);
                c.ew(scale_cols_kernel, n, g, gam, C, n, t2);
                gh2 = t2;
            }
            c.lin_wgrad(gh2, b.a, M, C, 4 * C, nm.g(b.p + ".pwconv2.weight"), nm.g(b.p + ".pwconv2.bias"));
            float* ga = lin_dgrad_any(c, gh2, M, C, nm.w(b.p + ".pwconv2.weight"), 4 * C);
            float* gu = gelu_bwd(c, ga, b.u, 4 * n);
            c.lin_wgrad(gu, b.n.y, M, 4 * C, C, nm.g(b.p + ".pwconv1.weight"), nm.g(b.p + ".pwconv1.bias"));
            float* gn = c.lin_dgrad(gu, M, 4 * C, nm.w(b.p + ".pwconv1.weight"), C);
            float* gdw = c.f32(n);
            c.ln_bwd(gn, b.n, nm.w(b.p + ".norm.weight"), M, C, gdw, false, nm.g(b.p + ".norm.weight"), nm.g(b.p + ".norm.bias"));
            if (float* gw = nm.g(b.p + ".dwconv.weight"))
                hipLaunchKernelGGL(dwconv7_wgrad_kernel, dim3(cdiv(C, 64), 49), dim3(1024), 0, s, gdw, b.x, B, H, H, C, gw);
            if (float* gb = nm.g(b.p + ".dwconv.bias")) c.colsum(gdw, nullptr, M, C, gb);
            // the residual's gradient g + the depthwise conv's data gradient (the same conv with the taps rotated by 180 degrees)
            c.ew(dwconv7_f32_kernel, n, gdw, nm.w(b.p + ".dwconv.weight"), nullptr, H, H, C, n, 1, 1, g);
        }
        if (st > 0) {       // LayerNorm + 2 x 2 patch conv: wgrad / dgrad of the patch GEMM, un-patchify, LayerNorm backward
            const CnxDownSaved& d = t.down[st - 1];
            c.lin_wgrad(g, d.col, M, d.Cn, 4 * d.C, nm.g(d.p + ".1.weight"), nm.g(d.p + ".1.bias"));
            float* gcol = c.lin_dgrad(g, M, d.Cn, nm.w(d.p + ".1.weight"), 4 * d.C);
            H *= 2;
            M *= 4;
            C = d.C;
            float* gl = unpatchify(c, gcol, 4 * C, B, C, H, H, 2);
            float* gx = c.f32((size_t)M * C);
            c.ln_bwd(gl, d.l, nm.w(d.p + ".0.weight"), M, C, gx, false, nm.g(d.p + ".0.weight"), nm.g(d.p + ".0.bias"));
            g = gx;
        }
    }
    // stem: LayerNorm backward, then the patch GEMM's weight / bias gradient
    const std::string s0 = BB + "downsample_layers.0.";
    float* gs = c.f32((size_t)M * C);
    c.ln_bwd(g, t.stem_ln, nm.w(s0 + "1.weight"), M, C, gs, false, nm.g(s0 + "1.weight"), nm.g(s0 + "1.bias"));
    lin_wgrad_unpad(c, gs, t.col0, M, C, 48, 64, nm.g(s0 + "0.weight"), nm.g(s0 + "0.bias"));
    if (cfg.tok_in_dim && (nm.g(PN + "in_conv.weight") || nm.g(PN + "in_conv.bias"))) {
        // sem's in_conv (Conv2d(152, 3, 3, 1, 1), sem_grounding_net.py:21, 46): the stem's data gradient back to pixel rows [B R R][3],
        // then im2col + lin_wgrad over the resized class planes
        const int R = t.R;
        float* gcol = lin_dgrad_any(c, gs, M, C, t.w0p, 64);
        float* g3 = unpatchify(c, gcol, 64, B, 3, R, R, 4);
        const Strides r = pixel_rows(3, R, R);
        if (sp.map_cls)
            class_wgrad(c, kClassWgradInConv, sp.map_cls, g3, {r.b, r.c, r.y, r.x}, B, sp.Ht, sp.Wt, t.Cuse, 3, R, nm.g(PN + "in_conv.weight"), nm.g(PN + "in_conv.bias"));
        else
            conv_wgrad(c, t.img, B, t.Cuse, R, R, nchw(t.Cuse, R, R), 3, 1, 1, R, R, g3, 3, nm.g(PN + "in_conv.weight"), nm.g(PN + "in_conv.bias"));
    }
}

namespace {
// canny_grounding_downsampler.py:21-29; hed: the resize only; sem: nearest, 152 -> 16 -> 8. NCHW fp32
DsSaved downsampler_forward(const Ctx& c, const Names& nm, const TrainSpatialIn& sp, int B, int Ce, int H0, int W0) {
    DsSaved d;
    const int Rd = sp.ds_resize, ni = sp.ds_n_in, mid = sp.ds_mid;
    if (sp.extra_cls) {
        if (sp.ds_mode != 1) throw GlError(GL_ERR_UNSUPPORTED, "unet_train_step: a class map was given to a downsampler that is not nearest mode (a bicubic resize mixes classes)");
        if (!mid) throw GlError(GL_ERR_UNSUPPORTED, "unet_train_step: a class map was given to a downsampler without layers (its output would be the planes themselves)");
    }
    if ((!sp.extra && !sp.extra_cls) || ni < 1 || (!sp.extra_cls && sp.Ce < ni) || Rd < 4)
        throw GlError(GL_ERR_ARG, "unet_train_step: grounding_extra_input / downsampler constants");
    if (mid ? (Rd != 4 * H0 || Rd != 4 * W0) : (Rd != H0 || Rd != W0 || ni != Ce))
        throw GlError(GL_ERR_ARG, fmt("unet_train_step: the downsampler (resize %d) does not match the %d x %d latent", Rd, H0, W0));
    if (!sp.extra_cls) {
        d.r = c.f32((size_t)B * ni * Rd * Rd);
        c.ck(resize_f32_launch(sp.extra, d.r, B, sp.Ce, ni, sp.He, sp.We, Rd, sp.ds_mode == 1 ? 1 : 0, c.s));
    }
    d.out = d.r;
    if (mid) {
        const int Rh = Rd / 2;
        const size_t nh = (size_t)B * mid * Rh * Rh;
        d.a1 = c.f32(nh);           // the first conv's pre-activation: the SiLU backward reads it
        if (sp.extra_cls) {     // the gather form of these trainable weights is rebuilt every step: arena memory, never the frozen-weight cache
            float* gw = c.f32((size_t)ni * 16 * mid);
            c.ck(class_conv_weight_relayout_launch(nm.w("downsample_net.layers.0.weight"), gw, mid, ni, c.s));
            c.ck(class_conv4x4s2_launch(sp.extra_cls, gw, nm.w("downsample_net.layers.0.bias"), d.a1, B, sp.He, sp.We, ni, mid, Rd, 0, c.s));
        } else {
            c.ck(conv4x4s2_f32_launch(d.r, nm.w("downsample_net.layers.0.weight"), nm.w("downsample_net.layers.0.bias"), d.a1, B, ni, mid, Rd, Rd, 0, c.s));
        }
        d.s1 = c.silu(d.a1, nh);
        d.out = c.f32((size_t)B * Ce * H0 * W0);
        c.ck(conv4x4s2_f32_launch(d.s1, nm.w("downsample_net.layers.2.weight"), nm.w("downsample_net.layers.2.bias"), d.out, B, mid, Ce, Rh, Rh, 0, c.s));
    }
    return d;
}

}  // namespace

bool train::downsampler_grads(const Names& nm) {
    bool any = false;
    for (const char* k : {"downsample_net.layers.0.weight", "downsample_net.layers.0.bias", "downsample_net.layers.2.weight", "downsample_net.layers.2.bias"})
        any = any || nm.g(k);
    return any;
}

// The first conv and the GroundingDownsampler (trainer.py:189-194, 229-236)
// (an inpainting model: Ci = Cx + 1 channels of inpainting_extra_input behind the latent's, no downsampler, `spatial` null -- only
// the weight gradient applies: nothing trainable sits in front of the first conv)
void train::conv_in_backward(const Ctx& c, const Names& nm, const TrainSpatialIn* spatial, const DsSaved& dsv, const float* xin, int B, int H0, int W0, int Cx,
                      int Ce, int Ci, int mc, const float* g) {
    const int Cin0 = Cx + Ce + Ci;
    if (float* gw = nm.g("input_blocks.0.0.weight")) conv_wgrad(c, xin, B, Cin0, H0, W0, pixel_rows(Cin0, H0, W0), 3, 1, 1, H0, W0, g, mc, gw, nullptr);
    if (!spatial || !spatial->ds_mid || !downsampler_grads(nm)) return;
    const TrainSpatialIn& sp = *spatial;
    // the first conv's data gradient for the k downsampler channels only: rows Cx .. Cx + k of the flipped / transposed filter
    const float* wt = c.conv_dgrad_weight(nm.w("input_blocks.0.0.weight"), mc, Cin0);
    float* gds = conv3x3_direct(c, g, wt + (size_t)Cx * mc * 9, nullptr, B, H0, W0, mc, Ce);
    const int Rd = sp.ds_resize, Rh = Rd / 2, mid = sp.ds_mid, ni = sp.ds_n_in;
    conv_wgrad(c, dsv.s1, B, mid, Rh, Rh, nchw(mid, Rh, Rh), 4, 2, 1, H0, W0, gds, Ce, nm.g("downsample_net.layers.2.weight"), nm.g("downsample_net.layers.2.bias"));
    const size_t nh = (size_t)B * mid * Rh * Rh;
    float* gs1 = c.f32(nh);
    c.ew(conv4x4s2_dgrad_kernel, nh, gds, nm.w("downsample_net.layers.2.weight"), mid, Ce, Rh, Rh, nh, gs1);
    float* ga1 = silu_bwd(c, gs1, dsv.a1, nh);
    if (sp.extra_cls) {
        const Strides r = nchw(mid, Rh, Rh);
        class_wgrad(c, kClassWgradDown, sp.extra_cls, ga1, {r.b, r.c, r.y, r.x}, B, sp.He, sp.We, ni, mid, Rd, nm.g("downsample_net.layers.0.weight"),
                    nm.g("downsample_net.layers.0.bias"));
    } else {
        const float* ga1r = im2col(c, ga1, B, mid, Rh, Rh, nchw(mid, Rh, Rh), 1, 1, 0, Rh, Rh, mid);     // NCHW -> pixel rows
        conv_wgrad(c, dsv.r, B, ni, Rd, Rd, nchw(ni, Rd, Rd), 4, 2, 1, Rh, Rh, ga1r, mid, nm.g("downsample_net.layers.0.weight"), nm.g("downsample_net.layers.0.bias"));
    }
}

// conv_in: frozen for the discrete models (forward only); for a model with a grounding downsampler its input is
// cat(x, downsample_net(grounding_extra_input)) (openaimodel.py:442-444) and its weight is trainable; for an inpainting model in.x
// already holds cat(x, inpainting_extra_input) (:445-447), Cin0 = 2 Cx + 1 channels per row, and the weight is trainable too -- the
// direct conv reads the fp32 weight itself, so no operand copy of it can end up in the frozen-weight cache. xin: the rows it read
float* train::conv_in_forward(const UNetStep& u, DsSaved& dsv, const float*& xin) {
    const Ctx& c = u.c;
    xin = u.in.x;
    if (u.Ce) {
        dsv = downsampler_forward(c, u.nm, *u.spatial, u.B, u.Ce, u.H0, u.W0);
        float* cat0 = c.f32(u.M0 * u.Cin0);
        c.ew(cat_rows_nchw_kernel, u.M0 * u.Cin0, u.in.x, u.Cx, dsv.out, u.Ce, u.H0 * u.W0, u.M0 * u.Cin0, cat0);
        xin = cat0;
    }
    return conv3x3_direct(c, xin, u.nm.w("input_blocks.0.0.weight"), u.nm.w("input_blocks.0.0.bias"), u.B, u.H0, u.W0, u.Cin0, u.mc);
}

// The direct conv by itself (train.h): forward, the data gradient of the input channels [c0, c0 + n) as conv_in_backward and the last
// conv's backward form it, and the weight gradient by conv_wgrad as conv_in_backward calls it
int train_prim_conv_direct(Arena& ar, float* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout, int c0, int n, const float* x, const float* w_oihw,
                           const float* bias, const float* dy, float* y, float* dx, float* dW, hipStream_t s) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return set_error(GL_ERR_ARG, "gl_op_train_conv_direct: B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W, Cin, Cout);
    if (c0 < 0 || n < 1 || c0 + n > Cin) return set_error(GL_ERR_ARG, "gl_op_train_conv_direct: channels [%d, %d) of %d", c0, c0 + n, Cin);
    try {
        Ctx c{ar, ws, ws_bytes, s};
        const size_t rows = (size_t)B * H * W;
        c.hip(hipMemcpyAsync(y, conv3x3_direct(c, x, w_oihw, bias, B, H, W, Cin, Cout), rows * Cout * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
        if (dy && dx) {
            const float* wt = c.conv_dgrad_weight(w_oihw, Cout, Cin);
            c.hip(hipMemcpyAsync(dx, conv3x3_direct(c, dy, wt + (size_t)c0 * Cout * 9, nullptr, B, H, W, Cout, n), rows * n * 4, hipMemcpyDeviceToDevice, s),
                  "hipMemcpyAsync");
        }
        if (dy && dW) conv_wgrad(c, x, B, Cin, H, W, pixel_rows(Cin, H, W), 3, 1, 1, H, W, dy, Cout, dW, nullptr);
        c.hip(hipGetLastError(), "training direct conv kernel launch");
    } catch (const GlError& e) {
        return set_error(e.code, "%s", e.what());
    }
    return GL_OK;
}

}  // namespace gl
