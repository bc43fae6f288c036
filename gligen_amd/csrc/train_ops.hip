// The primitive operations of the training path for gfx950: the kernels every layer is composed of and the Ctx methods that launch
// them (train_impl.h) -- bf16 operand builders, the matrix products over gemm.hip's bf16 MFMA GEMM (mm1 / mm / lin_* / conv3),
// LayerNorm, GroupNorm + SiLU, column sums, the dot / MSE reductions, GEGLU, the tanh gates --, the frozen-weight operand cache, AdamW,
// and the small kernels more than one other unit uses, each behind a function.
//
// What runs where: every matrix product of the forward and of the backward (dgrad  dX = dY W,  wgrad  dW = dY^T X) goes through
// the bf16 MFMA GEMM of gemm.hip with fp32 output (operands are cast / transposed to bf16 by the kernels below; accumulation and
// everything else is fp32, as the reference trains in fp32). Every reduction is a fixed-order sum: no float atomics.
#include "train_impl.h"

#include "adamw_update.h"
#include "gemm.h"
#include "misc.h"

namespace gl {

using namespace train;

namespace {

// The training path's matrix products run on the bf16 MFMA kernels at fp32-like precision: an fp32 operand x is the pair
// (hi = bf16(x), lo = bf16(x - hi)) and a product A W^T is  hi_A hi_W^T + lo_A hi_W^T + hi_A lo_W^T  (three GEMMs with fp32 accumulation;
// the dropped lo lo term is 2^-16 relative). The reference trains in fp32 (trainer.py: no autocast); single-pass bf16 is ~2^-9 per
// operand element, which through the 40-odd layers of the full UNet's backward reached 8e-4 rel-MSE on the deepest gradient
// (developer switch GL_TRAIN_BF16X1=1: one pass).
__global__ void transpose_f32_bf16_kernel(const float* __restrict__ src, int R, int Cc, int ld, bf16* __restrict__ dst, bf16* __restrict__ dst_lo, int Rpad) {
    __shared__ float tile[32][33];
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + threadIdx.x;
        tile[i][threadIdx.x] = (r < R && c < Cc) ? src[(size_t)r * ld + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + threadIdx.x;
        if (c < Cc && r < Rpad) {
            const float v = tile[threadIdx.x][i];
            const bf16 h = f2bf(v);
            dst[(size_t)c * Rpad + r] = h;
            if (dst_lo) dst_lo[(size_t)c * Rpad + r] = f2bf(v - bf2f(h));
        }
    }
}
__global__ void split_bf16_kernel(const float* __restrict__ src, size_t n, bf16* __restrict__ hi, bf16* __restrict__ lo) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = src[i];
    const bf16 h = f2bf(v);
    hi[i] = h;
    lo[i] = f2bf(v - bf2f(h));
}
// res = src - float(bf16(src))   (the low half of a conv weight, packed like the high half by pack_conv_weight_launch)
__global__ void bf16_residual_kernel(const float* __restrict__ src, size_t n, float* __restrict__ res) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) res[i] = src[i] - bf2f(f2bf(src[i]));
}
// The three passes of a split-precision product as ONE contraction (round 5): x = hi + lo in bf16, and
//     a w^T  ~  a_hi w_hi^T + a_lo w_hi^T + a_hi w_lo^T  =  [a_hi | a_lo | a_hi] [w_hi | w_hi | w_lo]^T
// -- the k dimension tripled, one GEMM launch with one fp32 accumulator instead of three launches, two fp32 temporaries and an add
// pass. side 0 (activation): segments (hi, lo, hi); side 1 (weight): (hi, hi, lo). Rows [R][3 K], columns K' = seg * K + c.
__global__ void cat3_rows_kernel(const float* __restrict__ src, size_t n, int K, int side, bf16* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t r = i / K;
    const int c = (int)(i - r * K);
    const float v = src[i];
    const bf16 h = f2bf(v), l = f2bf(v - bf2f(h));
    bf16* row = dst + r * 3 * (size_t)K;
    row[c] = h;
    row[K + c] = side ? h : l;
    row[2 * (size_t)K + c] = side ? l : h;
}
// [R][Cc] fp32 -> [Cc][3 Rpad] (the transposed operand of dgrad / wgrad), zero behind row R
__global__ void cat3_transposed_kernel(const float* __restrict__ src, int R, int Cc, int ld, int side, bf16* __restrict__ dst, int Rpad) {
    __shared__ float tile[32][33];
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + threadIdx.x;
        tile[i][threadIdx.x] = (r < R && c < Cc) ? src[(size_t)r * ld + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + threadIdx.x;
        if (c < Cc && r < Rpad) {
            const float v = tile[threadIdx.x][i];
            const bf16 h = f2bf(v), l = f2bf(v - bf2f(h));
            bf16* row = dst + (size_t)c * 3 * Rpad;
            row[r] = h;
            row[Rpad + r] = side ? h : l;
            row[2 * (size_t)Rpad + r] = side ? l : h;
        }
    }
}
// conv activations [rows][C] fp32 -> [rows][2 C] = (hi | lo): the implicit-GEMM loader reads channels (hi | lo | hi) as a two-source
// concat of this buffer with its own first half
__global__ void cat2_rows_kernel(const float* __restrict__ src, size_t n, int C, bf16* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t r = i / C;
    const int c = (int)(i - r * C);
    const float v = src[i];
    const bf16 h = f2bf(v);
    dst[r * 2 * (size_t)C + c] = h;
    dst[r * 2 * (size_t)C + C + c] = f2bf(v - bf2f(h));
}
// conv weight OIHW fp32 [O][I][9] -> [O][3 I][9] fp32 = (w | w | w - bf16(w)) along I: packed to bf16 it is (hi | hi | lo)
__global__ void conv_w_cat3_kernel(const float* __restrict__ w, int O, int I, float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)O * I * 9) return;
    const int t = (int)(idx % 9), i = (int)((idx / 9) % I);
    const size_t o = idx / ((size_t)9 * I);
    const float v = w[idx];
    float* row = out + o * 3 * (size_t)I * 9;
    row[(size_t)i * 9 + t] = v;
    row[((size_t)I + i) * 9 + t] = v;
    row[((size_t)2 * I + i) * 9 + t] = v - bf2f(f2bf(v));
}
__global__ void add3_kernel(float* __restrict__ dst, const float* __restrict__ a, const float* __restrict__ b, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += a[i] + b[i];
}


// out[c] = sum_r a[r][c] (* b[r][c]): 64 columns x 16 row lanes per workgroup, each row lane sums rows ry, ry + 16, ... in order and the
// sixteen partial sums are combined in a fixed order -- deterministic, and 16 x the parallelism of one thread per column (which was
// 8.5 % of a training iteration: profiles/r4_final/train_kernel_stats.csv is the profile before this change)
__global__ void __launch_bounds__(1024) colsum_kernel(const float* __restrict__ a, const float* __restrict__ b, int R, int Cc, float* __restrict__ out) {
    __shared__ float part[16][64];
    const int tx = threadIdx.x & 63, ry = threadIdx.x >> 6, c = blockIdx.x * 64 + tx;
    float s = 0.f;
    if (c < Cc)
        for (int r = ry; r < R; r += 16) s += b ? a[(size_t)r * Cc + c] * b[(size_t)r * Cc + c] : a[(size_t)r * Cc + c];
    part[ry][tx] = s;
    __syncthreads();
    if (ry == 0 && c < Cc) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += part[i][tx];
        out[c] = t;
    }
}

// LayerNorm over C per row (nn.LayerNorm: eps 1e-5 in the fusers, 1e-6 in ConvNeXt, convnext.py:29, 75, 80): one wave per row
__global__ void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b, int R, int Cc,
                              float* __restrict__ y, float* __restrict__ xhat, float* __restrict__ rstd_out, float eps) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const float* xr = x + (size_t)row * Cc;
    // One pass (sum, sum of squares) while the row is well conditioned: E[x^2] - mean^2 loses mean^2 / var of the fp32 digits, nothing
    // to speak of while mean^2 <= var. Otherwise -- rows N(30, 1) were off by 1e-4 of xhat, a constant row got a wrong rstd -- the
    // statistics are taken again without cancellation, relative to the row's first element p (x - p is exact or rounded at the size of
    // the spread, not of the mean): the mean of x - p, then the sum of squared deviations from it. The choice is per row and the sums are
    // in a fixed order either way.
    float s = 0.f, ss = 0.f;
    for (int c = lane; c < Cc; c += 64) { const float v = xr[c]; s += v; ss += v * v; }
    s = wave_sum(s); ss = wave_sum(ss);
    float p = s / Cc, md = 0.f;                            // xhat = ((x - p) - md) rstd; one pass: p = mean
    float var = fmaxf(ss / Cc - p * p, 0.f);
    if (p * p > var) {
        p = xr[0];
        s = 0.f; ss = 0.f;
        for (int c = lane; c < Cc; c += 64) s += xr[c] - p;
        md = wave_sum(s) / Cc;                             // mean - p
        for (int c = lane; c < Cc; c += 64) { const float d = (xr[c] - p) - md; ss += d * d; }
        var = wave_sum(ss) / Cc;
    }
    const float rstd = rsqrtf(var + eps);
    for (int c = lane; c < Cc; c += 64) {
        const float h = ((xr[c] - p) - md) * rstd;
        xhat[(size_t)row * Cc + c] = h;
        y[(size_t)row * Cc + c] = h * g[c] + b[c];
    }
    if (lane == 0) rstd_out[row] = rstd;
}
// dx (+)= rstd (g - mean(g) - xhat mean(g xhat)),  g = dy gamma
__global__ void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ xhat, const float* __restrict__ rstd, const float* __restrict__ gam,
                              int R, int Cc, float* __restrict__ dx, int accumulate) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const float* dr = dy + (size_t)row * Cc;
    const float* hr = xhat + (size_t)row * Cc;
    float m1 = 0.f, m2 = 0.f;
    for (int c = lane; c < Cc; c += 64) { const float gv = dr[c] * gam[c]; m1 += gv; m2 += gv * hr[c]; }
    m1 = wave_sum(m1) / Cc; m2 = wave_sum(m2) / Cc;
    const float rs = rstd[row];
    for (int c = lane; c < Cc; c += 64) {
        const float v = rs * (dr[c] * gam[c] - m1 - hr[c] * m2);
        float* o = dx + (size_t)row * Cc + c;
        *o = accumulate ? *o + v : v;
    }
}

// GEGLU (attention.py:37-44): h = val * gelu(gate), u = [val | gate] of width 2 I (erf GELU, F.gelu default)
__global__ void geglu_fwd_kernel(const float* __restrict__ u, int R, int I, float* __restrict__ h) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)R * I) return;
    const size_t r = idx / I, c = idx % I;
    const float val = u[r * 2 * I + c], g = u[r * 2 * I + I + c];
    h[idx] = val * 0.5f * g * (1.f + erff(g * 0.70710678118654752440f));
}
__global__ void geglu_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ u, int R, int I, float* __restrict__ du) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)R * I) return;
    const size_t r = idx / I, c = idx % I;
    const float val = u[r * 2 * I + c], g = u[r * 2 * I + I + c], d = dh[idx];
    const float Phi = gelu_cdf(g);
    const float phi = gelu_pdf(g);
    du[r * 2 * I + c] = d * g * Phi;
    du[r * 2 * I + I + c] = d * val * (Phi + g * phi);
}

// out = a + gate * b, gate = scale * tanh(*alpha) (alpha null: gate 1)
__global__ void gated_add_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ alpha, float scale, size_t n,
                                 float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = alpha ? scale * tanhf(*alpha) : 1.f;
    out[i] = a[i] + g * b[i];
}
// out = gate * a
__global__ void gated_scale_kernel(const float* __restrict__ a, const float* __restrict__ alpha, float scale, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = scale * tanhf(*alpha) * a[i];
}
__global__ void add_inplace_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}
// out[0] = coef(alpha) * sum_i a[i] b[i]: one block, fixed order.  mode 0: coef = scale (1 - tanh^2 alpha) (the gate's derivative);
// mode 1: coef = 1 / n and out = mean((a - b)^2) (the loss)
__global__ void __launch_bounds__(1024) dot_reduce_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, const float* __restrict__ alpha,
                                                          float scale, int mode, float* __restrict__ out) {
    __shared__ float red[16];
    float s = 0.f;
    for (size_t i = threadIdx.x; i < n; i += 1024) s += mode ? (a[i] - b[i]) * (a[i] - b[i]) : a[i] * b[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 16; ++i) t += red[i];
        if (mode) out[0] = t / (float)n;
        else { const float th = tanhf(*alpha); out[0] = scale * (1.f - th * th) * t; }
    }
}
// the same reduction for long vectors (the tanh-gate gradients and the loss at the 64 x 64 level are 10^7-element dots: one block took
// 1.2 ms each, 4 % of an iteration): fixed chunks -> partial sums (one block per chunk) -> one wave adds the partials in order
__global__ void __launch_bounds__(1024) dot_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, size_t chunk, int mode,
                                                           float* __restrict__ partial) {
    __shared__ float red[16];
    const size_t lo = (size_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    float s = 0.f;
    for (size_t i = lo + threadIdx.x; i < hi; i += 1024) s += mode ? (a[i] - b[i]) * (a[i] - b[i]) : a[i] * b[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 16; ++i) t += red[i];
        partial[blockIdx.x] = t;
    }
}
__global__ void dot_final_kernel(const float* __restrict__ partial, int nb, size_t n, const float* __restrict__ alpha, float scale, int mode, float* __restrict__ out) {
    if (threadIdx.x != 0) return;
    float t = 0.f;
    for (int i = 0; i < nb; ++i) t += partial[i];
    if (mode) out[0] = t / (float)n;
    else { const float th = tanhf(*alpha); out[0] = scale * (1.f - th * th) * t; }
}
// dy = 2 (y - t) / n   (d mse_loss / dy)
__global__ void mse_grad_kernel(const float* __restrict__ y, const float* __restrict__ t, size_t n, float* __restrict__ dy) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dy[i] = 2.f * (y[i] - t[i]) / (float)n;
}

// torch.optim.AdamW (trainer.py:245, one step of opt.step()): decoupled weight decay, bias-corrected moments, in place
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                             float b1, float omb1, float b2, float omb2, float eps, float decay, float step_size, float bc2_sqrt) {
    // torch.optim.AdamW (_single_tensor_adamw): every scalar below is formed in double on the host, as torch forms them from Python
    // floats, and rounded to fp32 once (adamw_update.h: adamw_scalars); the update itself is adamw_update, which train_optim.hip's
    // fused AdamW + EMA kernel shares
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    (void)lr;
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_update(pi, g[i], mi, vi, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
}

// ---- ResBlock pieces (openaimodel.py:154-232): GroupNorm32 + SiLU over pixel rows [B][HW][C] (fp32), and their backward.
// One workgroup per (group, sample); the group's HW x cpg slab is read twice (statistics, then apply; twice more for an ill-conditioned slab), sums in a fixed order.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// xhat = (x - mean) * rstd per (sample, group); a = silu(xhat * gamma + beta)   (util.py:223-226 GroupNorm32, eps 1e-5; nn.SiLU)
__global__ void __launch_bounds__(256) gn_silu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gam, const float* __restrict__ bet, int HW, int Cc,
                                                          float* __restrict__ xhat, float* __restrict__ rstd_out, float* __restrict__ a, int silu, float eps) {
    __shared__ float red[4];
    const int g = blockIdx.x, b = blockIdx.y, cpg = Cc / 32, n = HW * cpg;
    const float* xb = x + (size_t)b * HW * Cc + g * cpg;
    // one pass while mean^2 <= var, else again relative to the slab's first element, mean first, then the squared deviations from it
    // (ln_fwd_kernel's comment); the choice is the same for every thread of the workgroup
    float s = 0.f, q = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { const float v = xb[(size_t)(i / cpg) * Cc + i % cpg]; s += v; q += v * v; }
    s = block_sum_256(s, red);
    q = block_sum_256(q, red);
    float p = s / n, md = 0.f;                             // xhat = ((x - p) - md) rstd; one pass: p = mean
    float var = fmaxf(q / n - p * p, 0.f);
    if (p * p > var) {
        p = xb[0];
        s = 0.f; q = 0.f;
        for (int i = threadIdx.x; i < n; i += 256) s += xb[(size_t)(i / cpg) * Cc + i % cpg] - p;
        md = block_sum_256(s, red) / n;                    // mean - p
        for (int i = threadIdx.x; i < n; i += 256) { const float d = (xb[(size_t)(i / cpg) * Cc + i % cpg] - p) - md; q += d * d; }
        var = block_sum_256(q, red) / n;
    }
    const float rstd = rsqrtf(var + eps);
    for (int i = threadIdx.x; i < n; i += 256) {
        const int c = g * cpg + i % cpg;
        const size_t o = ((size_t)b * HW + i / cpg) * Cc + c;
        const float h = ((x[o] - p) - md) * rstd, u = h * gam[c] + bet[c];
        xhat[o] = h;
        a[o] = silu ? u / (1.f + __expf(-u)) : u;
    }
    if (threadIdx.x == 0) rstd_out[b * 32 + g] = rstd;
}
// da (gradient w.r.t. a = silu(u), u = xhat gamma + beta)  ->  dx of the GroupNorm's input:
//   du = da sigma(u) (1 + u (1 - sigma(u))),  t = du gamma,  dx = rstd (t - mean_g(t) - xhat mean_g(t xhat))      (dx (+)= when accumulate)
__global__ void __launch_bounds__(256) gn_silu_bwd_kernel(const float* __restrict__ da, const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                          const float* __restrict__ gam, const float* __restrict__ bet, int HW, int Cc,
                                                          float* __restrict__ dx, int accumulate, int silu) {
    __shared__ float red[4];
    const int g = blockIdx.x, b = blockIdx.y, cpg = Cc / 32, n = HW * cpg;
    auto t_of = [&](int i, float& h) {
        const int c = g * cpg + i % cpg;
        const size_t o = ((size_t)b * HW + i / cpg) * Cc + c;
        h = xhat[o];
        if (!silu) return da[o] * gam[c];
        const float u = h * gam[c] + bet[c], sg = 1.f / (1.f + __expf(-u));
        return da[o] * sg * (1.f + u * (1.f - sg)) * gam[c];
    };
    float m1 = 0.f, m2 = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { float h; const float t = t_of(i, h); m1 += t; m2 += t * h; }
    m1 = block_sum_256(m1, red) / n;
    m2 = block_sum_256(m2, red) / n;
    const float rs = rstd[b * 32 + g];
    for (int i = threadIdx.x; i < n; i += 256) {
        float h;
        const float t = t_of(i, h);
        const size_t o = ((size_t)b * HW + i / cpg) * Cc + g * cpg + i % cpg;
        const float v = rs * (t - m1 - h * m2);
        dx[o] = accumulate ? dx[o] + v : v;
    }
}
__global__ void silu_kernel(const float* __restrict__ x, size_t n, float* __restrict__ y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = x[i] / (1.f + __expf(-x[i]));
}
// The weights of the data-gradient conv: dX = conv3x3(dY, W'), W'[i][o][ky][kx] = W[o][i][2 - ky][2 - kx] (stride 1, pad 1: the
// transposed convolution of a 3x3 / pad 1 conv is a 3x3 / pad 1 conv with the filter flipped and the channel roles exchanged)
__global__ void conv_dgrad_weight_kernel(const float* __restrict__ w, int O, int I, float* __restrict__ wt) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= O * I * 9) return;
    const int t = idx % 9, i = (idx / 9) % I, o = idx / (9 * I);
    wt[((size_t)i * O + o) * 9 + (8 - t)] = w[idx];
}
// dst [N][Kp] = src [N][K] zero-padded on the right
__global__ void pad_cols_kernel(const float* __restrict__ src, int K, int Kp, size_t n, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Kp);
    dst[i] = c < K ? src[(i / Kp) * K + c] : 0.f;
}
// out[c] = sum_rows (1 - m[row]) g[row][c0 + c]   (the gradient of a learnable null embedding)
__global__ void null_grad_kernel(const float* __restrict__ g, const float* __restrict__ masks, int R, int ld, int c0, int n, float* __restrict__ out,
                                 int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += (1.f - masks[r]) * g[(size_t)r * ld + c0 + c];
    out[c] = accumulate ? out[c] + s : s;
}
__global__ void silu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, size_t n, float* __restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float sg = 1.f / (1.f + __expf(-x[i]));
    dx[i] = dy[i] * sg * (1.f + x[i] * (1.f - sg));
}
// fp32 direct 3x3 conv, stride 1, pad 1, over pixel rows, for the two convs with 4 channels on one side (conv_in 4 -> C, out C -> 4):
// one thread per output element. w OIHW.
__global__ void conv3x3_direct_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int H, int W, int Cin,
                                      int Cout, size_t n, float* __restrict__ y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int co = (int)(i % Cout), xw = (int)((i / Cout) % W), yh = (int)((i / ((size_t)Cout * W)) % H);
    const size_t b = i / ((size_t)Cout * W * H);
    float acc = bias ? bias[co] : 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = yh + ky - 1;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = xw + kx - 1;
            if (xx < 0 || xx >= W) continue;
            const float* xp = x + ((b * H + yy) * W + xx) * Cin;
            const float* wp = w + (size_t)co * Cin * 9 + ky * 3 + kx;
            for (int ci = 0; ci < Cin; ++ci) acc = fmaf(xp[ci], wp[(size_t)ci * 9], acc);
        }
    }
    y[i] = acc;
}
// dst[r][c] (+)= src[r][c0 + c]
__global__ void split_kernel(const float* __restrict__ src, int ld, int c0, int Cc, size_t rows, float* __restrict__ dst, int accumulate) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * Cc) return;
    const size_t r = i / Cc;
    const int c = (int)(i % Cc);
    const float v = src[r * ld + c0 + c];
    dst[i] = accumulate ? dst[i] + v : v;
}

}  // namespace

// operand copies of frozen parameters, kept across training steps (train.h)
TrainWeightCache* train_cache_create() { return new TrainWeightCache(); }
void train_cache_destroy(TrainWeightCache* c) {
    if (!c) return;
    for (auto& kv : c->m) (void)hipFree(kv.second);
    delete c;
}
size_t train_cache_bytes(const TrainWeightCache* c) { return c ? c->bytes : 0; }

namespace train {

Split Ctx::to_bf16(const float* src, size_t n) const {
    Split d{ar.get<bf16>(n), nullptr};
    if (split_precision()) {
        d.lo = ar.get<bf16>(n);
        ew(split_bf16_kernel, n, src, n, d.hi, d.lo);
    } else {
        ck(cast_f32_bf16_launch(src, d.hi, (int64_t)n, s));
    }
    return d;
}
// [R][Cc] fp32 -> [Cc][Rpad] bf16, columns R..Rpad zero (Rpad: the contraction length of the GEMM that reads it, a multiple of 64)
Split Ctx::transposed(const float* src, int R, int Cc, int Rpad) const {
    Split d{ar.get<bf16>((size_t)Cc * Rpad), split_precision() ? ar.get<bf16>((size_t)Cc * Rpad) : nullptr};
    hipLaunchKernelGGL(transpose_f32_bf16_kernel, dim3(cdiv(Cc, 32), cdiv(Rpad, 32)), dim3(32, 8), 0, s, src, R, Cc, Cc, d.hi, d.lo, Rpad);
    return d;
}
void Ctx::mm1(const bf16* a, const bf16* w, int M, int N, int K, const float* bias, float* out) const {
    AOperand A;
    aoperand_rows(A, a, K, K);
    Epilogue E;
    epilogue_defaults(E);
    E.out = out; E.ldo = N; E.out_f32 = 1; E.bias = bias;
    ck(gemm_launch(A, w, M, N, K, E, ws, ws_bytes, s));
}
void Ctx::add3(float* dst, const float* a, const float* b, size_t n) const { ew(add3_kernel, n, dst, a, b, n); }
// out [M][N] fp32 = a [M][K] w[N][K]^T (+ bias)
void Ctx::mm(const Split& a, const Split& w, int M, int N, int K, const float* bias, float* out) const {
    split_product([&](const bf16* ap, const bf16* wp, const float* b, float* o) { mm1(ap, wp, M, N, K, b, o); }, a, w, M, N, bias, out);
}
// ---- one-launch split-precision products (cat3_* above); GL_TRAIN_3LAUNCH=1 (developer A/B) keeps the three-launch form
bf16* Ctx::cat3_rows(const float* src, size_t R, int K, int side) const {
    bf16* d = ar.get<bf16>(R * 3 * (size_t)K);
    ew(cat3_rows_kernel, R * (size_t)K, src, R * (size_t)K, K, side, d);
    return d;
}
bf16* Ctx::cat3_transposed(const float* src, int R, int Cc, int Rpad, int side) const {
    bf16* d = ar.get<bf16>((size_t)Cc * 3 * Rpad);
    hipLaunchKernelGGL(cat3_transposed_kernel, dim3(cdiv(Cc, 32), cdiv(Rpad, 32)), dim3(32, 8), 0, s, src, R, Cc, Cc, side, d, Rpad);
    return d;
}
// the weight side of a product (side = 1): cached for frozen parameters
bf16* Ctx::cat3_rows_w(const float* W, int N, int K) const {
    return weight_operand(W, WF_ROWS, N, K, (size_t)N * 3 * K, [&](bf16* d) { ew(cat3_rows_kernel, (size_t)N * K, W, (size_t)N * K, K, 1, d); });
}
bf16* Ctx::cat3_transposed_w(const float* W, int N, int K) const {
    return weight_operand(W, WF_TRANSPOSED, N, K, (size_t)K * 3 * N, [&](bf16* d) {
        hipLaunchKernelGGL(cat3_transposed_kernel, dim3(cdiv(K, 32), cdiv(N, 32)), dim3(32, 8), 0, s, W, N, K, K, 1, d, N);
    });
}

bool Ctx::split_precision() {
    static const bool one_pass = dev_env("GL_TRAIN_BF16X1") && atoi(dev_env("GL_TRAIN_BF16X1")) != 0;
    return !one_pass;
}
bool Ctx::one_launch() {
    static const bool three = dev_env("GL_TRAIN_3LAUNCH") && atoi(dev_env("GL_TRAIN_3LAUNCH")) != 0;
    return split_precision() && !three;
}
// y = x W^T + b
float* Ctx::lin_fwd(const float* x, int M, int K, const float* W, const float* b, int N) const {
    float* y = f32((size_t)M * N);
    const size_t mk = ar.mark();       // the bf16 operand copies live for this product only (stream order keeps their reuse safe)
    if (one_launch()) mm1(cat3_rows(x, M, K, 0), cat3_rows_w(W, N, K), M, N, 3 * K, b, y);
    else mm(to_bf16(x, (size_t)M * K), to_bf16(W, (size_t)N * K), M, N, K, b, y);
    ar.release(mk);
    return y;
}
// dgrad: dx [M][K] = dy [M][N] W [N][K]   (the GEMM's "weight" operand is W^T, contraction over N)
float* Ctx::lin_dgrad(const float* dy, int M, int N, const float* W, int K) const {
    float* dx = f32((size_t)M * K);
    const size_t mk = ar.mark();
    if (one_launch()) mm1(cat3_rows(dy, M, N, 0), cat3_transposed_w(W, N, K), M, K, 3 * N, nullptr, dx);
    else mm(to_bf16(dy, (size_t)M * N), transposed(W, N, K, N), M, K, N, nullptr, dx);
    ar.release(mk);
    return dx;
}
// wgrad: dW [N][K] = dy^T x (contraction over the M rows, zero-padded to a multiple of 64), db [N] = column sums of dy
void Ctx::lin_wgrad(const float* dy, const float* x, int M, int N, int K, float* dW, float* db) const {
    const int Mp = round_up(M, 64);
    const size_t mk = ar.mark();
    if (dW) {
        if (one_launch()) mm1(cat3_transposed(dy, M, N, Mp, 0), cat3_transposed(x, M, K, Mp, 1), N, K, 3 * Mp, nullptr, dW);
        else mm(transposed(dy, M, N, Mp), transposed(x, M, K, Mp), N, K, Mp, nullptr, dW);
    }
    ar.release(mk);
    if (db) colsum(dy, nullptr, M, N, db);
}

float* Ctx::conv_dgrad_weight(const float* w_oihw, int O, int I) const { return ew_new(conv_dgrad_weight_kernel, (size_t)I * O * 9, (size_t)I * O * 9, w_oihw, O, I); }
// The activations are cast to bf16 for the implicit-GEMM kernel of gemm_u.hip. One launch over 3 Ci input channels where the loader's
// 64-channel step allows it -- activations (hi | lo | hi) as a two-source concat of the (hi | lo) buffer with its own first half,
// weights (hi | hi | lo) along I (cached for frozen convs: flip / transpose for dgrad, split, pack -- once) --, else three launches
float* Ctx::conv3(const float* a, int B, int H, int W, const float* w_oihw, const float* bias, int Cin, int Cout, bool dgrad, int stride, int ups) const {
    const int Ho = stride == 2 ? H / 2 : H << ups, Wo = stride == 2 ? W / 2 : W << ups;
    const int Ci = dgrad ? Cout : Cin, Co = dgrad ? Cin : Cout, M = B * Ho * Wo;
    const size_t nw = (size_t)Co * 9 * Ci, na = (size_t)B * H * W * Ci;
    float* out = f32((size_t)M * Co);
    const size_t mk_ops = ar.mark();   // packed weights / bf16 activation copies: this product's, released behind it
    auto weight_source = [&] { return dgrad ? conv_dgrad_weight(w_oihw, Cout, Cin) : w_oihw; };
    // parts: how many Ci-wide channel groups are concatenated along K (3: ap is the (hi | lo) buffer)
    auto launch = [&](int parts, const bf16* ap, const bf16* wq, const float* bb, float* o) {
        AOperand A{};
        A.p0 = ap; A.C0 = Ci; A.ld0 = Ci; A.mode = A_CONV3;
        if (parts == 3) { A.C0 = 2 * Ci; A.ld0 = 2 * Ci; A.p1 = ap; A.C1 = Ci; A.ld1 = 2 * Ci; }
        A.Hin = H; A.Win = W; A.Ho = Ho; A.Wo = Wo; A.stride = stride; A.ups = ups; A.pad_lo = 1;
        Epilogue E;
        epilogue_defaults(E);
        E.out = o; E.ldo = Co; E.out_f32 = 1; E.bias = bb; E.rows_per_b = Ho * Wo;
        ck(gemm_launch(A, wq, M, Co, parts * 9 * Ci, E, ws, ws_bytes, s));
    };
    if (one_launch() && Ci % 64 == 0) {
        const bf16* wp3 = weight_operand(w_oihw, dgrad ? WF_CONV_DGRAD : WF_CONV, Cout, Cin, 3 * nw, [&](bf16* d) {
            const float* src = weight_source();
            float* w3 = f32(3 * nw);
            ew(conv_w_cat3_kernel, nw, src, Co, Ci, w3);
            ck(pack_conv_weight_launch(w3, d, Co, 3 * Ci, 3, 3, Co, s));
        });
        bf16* a2 = ar.get<bf16>(2 * na);
        ew(cat2_rows_kernel, na, a, na, Ci, a2);
        launch(3, a2, wp3, bias, out);
    } else {
        const float* wsrc = weight_source();
        Split wp{ar.get<bf16>(nw), nullptr};
        ck(pack_conv_weight_launch(wsrc, wp.hi, Co, Ci, 3, 3, Co, s));
        if (split_precision()) {
            float* wres = f32(nw);
            ew(bf16_residual_kernel, nw, wsrc, nw, wres);
            wp.lo = ar.get<bf16>(nw);
            ck(pack_conv_weight_launch(wres, wp.lo, Co, Ci, 3, 3, Co, s));
        }
        const Split av = to_bf16(a, na);
        split_product([&](const bf16* ap, const bf16* wq, const float* bb, float* o) { launch(1, ap, wq, bb, o); }, av, wp, M, Co, bias, out);
    }
    ar.release(mk_ops);
    return out;
}

Ctx::LN Ctx::ln_fwd(const float* x, int R, int Cc, const float* g, const float* b, float eps) const {
    LN r{f32((size_t)R * Cc), f32((size_t)R * Cc), f32(R)};
    hipLaunchKernelGGL(ln_fwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, x, g, b, R, Cc, r.y, r.xhat, r.rstd, eps);
    return r;
}
void Ctx::ln_bwd(const float* dy, const LN& f, const float* g, int R, int Cc, float* dx, bool accumulate, float* dgamma, float* dbeta) const {
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, dy, f.xhat, f.rstd, g, R, Cc, dx, accumulate ? 1 : 0);
    if (dgamma) colsum(dy, f.xhat, R, Cc, dgamma);
    if (dbeta) colsum(dy, nullptr, R, Cc, dbeta);
}
Ctx::GN Ctx::gn_silu_fwd(const float* x, int B, int HW, int Cc, const float* g, const float* b, bool silu, float eps) const {
    GN r{f32((size_t)B * HW * Cc), f32((size_t)B * HW * Cc), f32((size_t)B * 32)};
    hipLaunchKernelGGL(gn_silu_fwd_kernel, dim3(32, B), dim3(256), 0, s, x, g, b, HW, Cc, r.xhat, r.rstd, r.a, silu ? 1 : 0, eps);
    return r;
}
void Ctx::gn_silu_bwd(const float* da, const GN& f, const float* g, const float* b, int B, int HW, int Cc, float* dx, bool accumulate, bool silu) const {
    hipLaunchKernelGGL(gn_silu_bwd_kernel, dim3(32, B), dim3(256), 0, s, da, f.xhat, f.rstd, g, b, HW, Cc, dx, accumulate ? 1 : 0, silu ? 1 : 0);
}
void Ctx::colsum(const float* a, const float* b, int R, int Cc, float* out) const {
    hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(Cc, 64)), dim3(1024), 0, s, a, b, R, Cc, out);
}
void Ctx::dot_reduce(const float* a, const float* b, size_t n, const float* alpha, float scale, int mode, float* out) const {
    if (n <= ((size_t)1 << 18)) {
        hipLaunchKernelGGL(dot_reduce_kernel, dim3(1), dim3(1024), 0, s, a, b, n, alpha, scale, mode, out);
        return;
    }
    const size_t chunk = (size_t)1 << 16;
    const int nb = (int)((n + chunk - 1) / chunk);
    const size_t mk = ar.mark();
    float* partial = f32(nb);
    hipLaunchKernelGGL(dot_partial_kernel, dim3(nb), dim3(1024), 0, s, a, b, n, chunk, mode, partial);
    hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(64), 0, s, partial, nb, n, alpha, scale, mode, out);
    ar.release(mk);
}
float* Ctx::mse_loss(const float* y, const float* target, size_t n, float* loss) const {
    dot_reduce(y, target, n, nullptr, 1.f, 1, loss);
    return ew_new(mse_grad_kernel, n, n, y, target, n);
}

float* Ctx::silu(const float* x, size_t n) const { return ew_new(silu_kernel, n, n, x, n); }
float* Ctx::geglu_fwd(const float* u, int R, int I) const { return ew_new(geglu_fwd_kernel, (size_t)R * I, (size_t)R * I, u, R, I); }
float* Ctx::geglu_bwd(const float* dh, const float* u, int R, int I) const { return ew_new(geglu_bwd_kernel, (size_t)R * 2 * I, (size_t)R * I, dh, u, R, I); }
float* Ctx::gated_add(const float* a, const float* b, const float* alpha, float scale, size_t n, float* out) const {
    if (!out) out = f32(n);
    ew(gated_add_kernel, n, a, b, alpha, scale, n, out);
    return out;
}
float* Ctx::gated_scale(const float* a, const float* alpha, float scale, size_t n) const { return ew_new(gated_scale_kernel, n, n, a, alpha, scale, n); }
void Ctx::add(float* dst, const float* src, size_t n) const { ew(add_inplace_kernel, n, dst, src, n); }
float* Ctx::slice_rows(const float* src, int B, int stride_rows, int row0, int rows, int Cc) const {
    float* d = f32((size_t)B * rows * Cc);
    hip(hipMemcpy2DAsync(d, (size_t)rows * Cc * 4, src + (size_t)row0 * Cc, (size_t)stride_rows * Cc * 4, (size_t)rows * Cc * 4, B, hipMemcpyDeviceToDevice, s),
        "hipMemcpy2DAsync");
    return d;
}
void Ctx::put_rows(float* dst, int B, int stride_rows, int row0, const float* src, int rows, int Cc) const {
    hip(hipMemcpy2DAsync(dst + (size_t)row0 * Cc, (size_t)stride_rows * Cc * 4, src, (size_t)rows * Cc * 4, (size_t)rows * Cc * 4, B, hipMemcpyDeviceToDevice, s),
        "hipMemcpy2DAsync");
}

// dst [R][Kp] = src [R][K] zero-padded on the right; dst[r][c] (+)= src[r][c0 + c]
float* pad_cols(const Ctx& c, const float* src, int R, int K, int Kp) { return c.ew_new(pad_cols_kernel, (size_t)R * Kp, (size_t)R * Kp, src, K, Kp, (size_t)R * Kp); }
void split_cols(const Ctx& c, const float* src, int ld, int c0, int Cc, size_t rows, float* dst, bool accumulate) {
    c.ew(split_kernel, rows * Cc, src, ld, c0, Cc, rows, dst, accumulate ? 1 : 0);
}
// y = x W^T + b and dx = dy W for any contraction length: zero-padded to the GEMM's 64-step (ConvNeXt's first stage has C = 96)
float* lin_fwd_any(const Ctx& c, const float* x, int M, int K, const float* W, const float* b, int N) {
    if (K % 64 == 0) return c.lin_fwd(x, M, K, W, b, N);
    const int Kp = round_up(K, 64);
    const float* xp = pad_cols(c, x, M, K, Kp);
    return c.lin_fwd(xp, M, Kp, pad_cols(c, W, N, K, Kp), b, N);
}
float* lin_dgrad_any(const Ctx& c, const float* dy, int M, int N, const float* W, int K) {
    if (N % 64 == 0) return c.lin_dgrad(dy, M, N, W, K);
    const int Np = round_up(N, 64);
    float* Wp = c.f32((size_t)Np * K);
    c.hip(hipMemsetAsync(Wp + (size_t)N * K, 0, (size_t)(Np - N) * K * 4, c.s), "hipMemsetAsync");
    c.hip(hipMemcpyAsync(Wp, W, (size_t)N * K * 4, hipMemcpyDeviceToDevice, c.s), "hipMemcpyAsync");
    return c.lin_dgrad(pad_cols(c, dy, M, N, Np), M, Np, Wp, K);
}
// the weight gradient of a Linear that ran on operands padded to Kp columns (xp [M][Kp]): formed as [N][Kp], its first K columns copied out
void lin_wgrad_unpad(const Ctx& c, const float* dy, const float* xp, int M, int N, int K, int Kp, float* dW, float* db) {
    float* dWp = dW && Kp != K ? c.f32((size_t)N * Kp) : dW;
    c.lin_wgrad(dy, xp, M, N, Kp, dWp, db);
    if (dWp != dW) split_cols(c, dWp, Kp, 0, K, (size_t)N, dW, false);
}
float* silu_bwd(const Ctx& c, const float* dy, const float* x, size_t n) { return c.ew_new(silu_bwd_kernel, n, n, dy, x, n); }
void null_grad(const Ctx& c, const float* g, const float* masks, int R, int ld, int c0, int n, float* out, bool accumulate) {
    c.ew(null_grad_kernel, n, g, masks, R, ld, c0, n, out, accumulate ? 1 : 0);
}
float* conv3x3_direct(const Ctx& c, const float* x, const float* w, const float* bias, int B, int H, int W, int Cin, int Cout) {
    const size_t n = (size_t)B * H * W * Cout;
    return c.ew_new(conv3x3_direct_kernel, n, n, x, w, bias, H, W, Cin, Cout, n);
}

}  // namespace train

// ---- the primitives by themselves (train.h; include/gligen_amd_train_prims.h): what a Ctx method returns in the arena is copied to
// the caller; what a method writes through a pointer (ln_bwd's dx / dgamma / dbeta, gn_silu_bwd's dx, the weight gradient, the dot) is
// written where the caller points
namespace {
template <class F>
int run_prim(Arena& ar, float* ws, size_t ws_bytes, hipStream_t s, F&& body) {
    try {
        Ctx c{ar, ws, ws_bytes, s};
        body(c);
        c.hip(hipGetLastError(), "training primitive kernel launch");
    } catch (const GlError& e) {
        return set_error(e.code, "%s", e.what());
    }
    return GL_OK;
}
void copy_out(const Ctx& c, float* dst, const float* src, size_t n) {
    if (dst) c.hip(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, c.s), "hipMemcpyAsync");
}
}  // namespace

int train_prim_linear(Arena& ar, float* ws, size_t ws_bytes, int M, int N, int K, const float* x, const float* W, const float* b, const float* dy, float* y,
                      float* dx, float* dW, float* db, hipStream_t s) {
    if (M < 1 || N < 1 || K < 1) return set_error(GL_ERR_ARG, "gl_op_train_linear: M=%d N=%d K=%d", M, N, K);
    return run_prim(ar, ws, ws_bytes, s, [&](const Ctx& c) {
        if (y) copy_out(c, y, lin_fwd_any(c, x, M, K, W, b, N), (size_t)M * N);
        if (!dy) return;
        if (dx) copy_out(c, dx, lin_dgrad_any(c, dy, M, N, W, K), (size_t)M * K);
        const int Kp = round_up(K, 64);
        if (dW || db) lin_wgrad_unpad(c, dy, dW && Kp != K ? pad_cols(c, x, M, K, Kp) : x, M, N, K, Kp, dW, db);
    });
}

int train_prim_layernorm(Arena& ar, float* ws, size_t ws_bytes, int R, int C, float eps, const float* x, const float* g, const float* b, const float* dy,
                         int accumulate, float* y, float* xhat, float* rstd, float* dx, float* dgamma, float* dbeta, hipStream_t s) {
    if (R < 1 || C < 1) return set_error(GL_ERR_ARG, "gl_op_train_layernorm: R=%d C=%d", R, C);
    return run_prim(ar, ws, ws_bytes, s, [&](const Ctx& c) {
        const size_t n = (size_t)R * C;
        const Ctx::LN f = c.ln_fwd(x, R, C, g, b, eps);
        copy_out(c, y, f.y, n);
        copy_out(c, xhat, f.xhat, n);
        copy_out(c, rstd, f.rstd, (size_t)R);
        if (dy) c.ln_bwd(dy, f, g, R, C, dx ? dx : c.f32(n), dx && accumulate, dgamma, dbeta);
    });
}

int train_prim_groupnorm(Arena& ar, float* ws, size_t ws_bytes, int B, int HW, int C, int silu, float eps, const float* x, const float* g, const float* b,
                         const float* da, int accumulate, float* a, float* xhat, float* rstd, float* dx, hipStream_t s) {
    if (B < 1 || HW < 1 || C < 1) return set_error(GL_ERR_ARG, "gl_op_train_groupnorm: B=%d HW=%d C=%d", B, HW, C);
    if (C % 32) return set_error(GL_ERR_ARG, "gl_op_train_groupnorm: C=%d is no multiple of the 32 groups", C);
    return run_prim(ar, ws, ws_bytes, s, [&](const Ctx& c) {
        const size_t n = (size_t)B * HW * C;
        const Ctx::GN f = c.gn_silu_fwd(x, B, HW, C, g, b, silu != 0, eps);
        copy_out(c, a, f.a, n);
        copy_out(c, xhat, f.xhat, n);
        copy_out(c, rstd, f.rstd, (size_t)B * 32);
        if (da && dx) c.gn_silu_bwd(da, f, g, b, B, HW, C, dx, accumulate != 0, silu != 0);
    });
}

int train_prim_geglu(Arena& ar, float* ws, size_t ws_bytes, int R, int I, const float* u, const float* dh, float* h, float* du, hipStream_t s) {
    if (R < 1 || I < 1) return set_error(GL_ERR_ARG, "gl_op_train_geglu: R=%d I=%d", R, I);
    return run_prim(ar, ws, ws_bytes, s, [&](const Ctx& c) {
        if (h) copy_out(c, h, c.geglu_fwd(u, R, I), (size_t)R * I);
        if (dh && du) copy_out(c, du, c.geglu_bwd(dh, u, R, I), (size_t)R * 2 * I);
    });
}

int train_prim_dot(Arena& ar, float* ws, size_t ws_bytes, size_t n, const float* a, const float* b, const float* alpha, float scale, int mode, float* out,
                   hipStream_t s) {
    return run_prim(ar, ws, ws_bytes, s, [&](const Ctx& c) { c.dot_reduce(a, b, n, alpha, scale, mode, out); });
}

int adamw_step(float* p, const float* g, float* m, float* v, size_t n, double lr, double b1, double b2, double eps, double wd, int step, hipStream_t s) {
    if (step < 1) return set_error(GL_ERR_ARG, "adamw_step: step counts from 1");
    const AdamwScalars k = adamw_scalars(lr, b1, b2, eps, wd, step);
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, g, m, v, n, (float)lr, k.b1, k.omb1, k.b2, k.omb2, k.eps, k.decay,
                       k.step_size, k.bc2_sqrt);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
