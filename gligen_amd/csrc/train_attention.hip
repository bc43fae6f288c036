// Attention of the training path for gfx950 (reference ldm/modules/attention.py:127-186, CrossAttention / SelfAttention), fp32 in and
// out: forward with the row log-sum-exp saved, backward with the probabilities RECOMPUTED from q, k and that log-sum-exp -- nothing of
// size Nq x Nk is ever stored. Two kernel families -- VALU (every built head dim) and MFMA (32 / 40 / 64 / 80) --, the head-dim table
// of each, and Ctx::attn_fwd / attn_bwd (train_impl.h), which choose between them.
#include "train_impl.h"

#include <type_traits>

namespace gl {

using namespace train;

namespace {

// ---- attention on row-major q [B][Nq][H d], k / v [B][Nk][H d]. A (batch, head, query) -- or key, in attn_bwd_kv -- is owned by LPQ
// adjacent lanes, each holding a DC-wide chunk of the head dimension (d = DC * LPQ; DC <= 40 keeps a lane's q / accumulator chunks in
// registers: with one lane per query d = 160 spilled 320 floats per lane and was 3 ms per launch). Dot products over d are chunk sums
// combined across the LPQ lanes by xor shuffles.
template <int LPQ>
__device__ __forceinline__ float lpq_sum(float v) {
    if constexpr (LPQ >= 2) v += __shfl_xor(v, 1, 64);
    if constexpr (LPQ >= 4) v += __shfl_xor(v, 2, 64);
    return v;
}
template <int DC, int LPQ>
__global__ void attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int H, int Nq, int Nk, float scale,
                                float* __restrict__ o, float* __restrict__ lse) {
    constexpr int D = DC * LPQ;
    const int bh = blockIdx.y, b = bh / H, h = bh % H, gi = blockIdx.x * blockDim.x + threadIdx.x, part = gi % LPQ;
    const int i = min(gi / LPQ, Nq - 1);                  // (lanes past the end recompute the last query and do not store: the shuffles need them)
    const bool live = gi / LPQ < Nq;
    const int ld = H * D, c0 = h * D + part * DC;
    float qi[DC], acc[DC];
    const float* qp = q + ((size_t)b * Nq + i) * ld + c0;
#pragma unroll
    for (int c = 0; c < DC; ++c) { qi[c] = qp[c] * scale; acc[c] = 0.f; }
    float m = -1e30f, l = 0.f;
    for (int j = 0; j < Nk; ++j) {
        const float* kp = k + ((size_t)b * Nk + j) * ld + c0;
        const float* vp = v + ((size_t)b * Nk + j) * ld + c0;
        float sc = 0.f;
#pragma unroll
        for (int c = 0; c < DC; ++c) sc = fmaf(qi[c], kp[c], sc);
        sc = lpq_sum<LPQ>(sc);
        const float mn = fmaxf(m, sc), corr = __expf(m - mn), p = __expf(sc - mn);
        l = l * corr + p;
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[c] = fmaf(acc[c], corr, p * vp[c]);
        m = mn;
    }
    if (!live) return;
    float* op = o + ((size_t)b * Nq + i) * ld + c0;
    const float inv = 1.f / l;
#pragma unroll
    for (int c = 0; c < DC; ++c) op[c] = acc[c] * inv;
    if (part == 0) lse[(size_t)bh * Nq + i] = m + __logf(l);
}
// dq and the row terms delta_i = do_i . o_i; the probabilities are recomputed from q, k and the saved log-sum-exp
template <int DC, int LPQ>
__global__ void attn_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ o,
                                  const float* __restrict__ dout, const float* __restrict__ lse, int H, int Nq, int Nk, float scale,
                                  float* __restrict__ dq, float* __restrict__ delta) {
    constexpr int D = DC * LPQ;
    const int bh = blockIdx.y, b = bh / H, h = bh % H, gi = blockIdx.x * blockDim.x + threadIdx.x, part = gi % LPQ;
    const int i = min(gi / LPQ, Nq - 1);
    const bool live = gi / LPQ < Nq;
    const int ld = H * D;
    const size_t off = ((size_t)b * Nq + i) * ld + h * D + part * DC;
    float qi[DC], di[DC], acc[DC];
    float dl = 0.f;
#pragma unroll
    for (int c = 0; c < DC; ++c) { qi[c] = q[off + c] * scale; di[c] = dout[off + c]; dl = fmaf(di[c], o[off + c], dl); acc[c] = 0.f; }
    dl = lpq_sum<LPQ>(dl);
    const float L = lse[(size_t)bh * Nq + i];
    for (int j = 0; j < Nk; ++j) {
        const float* kp = k + ((size_t)b * Nk + j) * ld + h * D + part * DC;
        const float* vp = v + ((size_t)b * Nk + j) * ld + h * D + part * DC;
        float sc = 0.f, dp = 0.f;
#pragma unroll
        for (int c = 0; c < DC; ++c) { sc = fmaf(qi[c], kp[c], sc); dp = fmaf(di[c], vp[c], dp); }
        sc = lpq_sum<LPQ>(sc);
        dp = lpq_sum<LPQ>(dp);
        const float ds = __expf(sc - L) * (dp - dl);
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[c] = fmaf(ds, kp[c], acc[c]);
    }
    if (!live) return;
#pragma unroll
    for (int c = 0; c < DC; ++c) dq[off + c] = acc[c] * scale;
    if (part == 0) delta[(size_t)bh * Nq + i] = dl;
}
template <int DC, int LPQ>
__global__ void attn_bwd_kv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ dout,
                                   const float* __restrict__ lse, const float* __restrict__ delta, int H, int Nq, int Nk, float scale,
                                   float* __restrict__ dk, float* __restrict__ dv) {
    constexpr int D = DC * LPQ;
    const int bh = blockIdx.y, b = bh / H, h = bh % H, gj = blockIdx.x * blockDim.x + threadIdx.x, part = gj % LPQ;
    const int j = min(gj / LPQ, Nk - 1);
    const bool live = gj / LPQ < Nk;
    const int ld = H * D;
    const size_t off = ((size_t)b * Nk + j) * ld + h * D + part * DC;
    float kj[DC], vj[DC], ak[DC], av[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) { kj[c] = k[off + c]; vj[c] = v[off + c]; ak[c] = 0.f; av[c] = 0.f; }
    for (int i = 0; i < Nq; ++i) {
        const float* qp = q + ((size_t)b * Nq + i) * ld + h * D + part * DC;
        const float* dp_ = dout + ((size_t)b * Nq + i) * ld + h * D + part * DC;
        float sc = 0.f, dp = 0.f;
#pragma unroll
        for (int c = 0; c < DC; ++c) { sc = fmaf(qp[c], kj[c], sc); dp = fmaf(dp_[c], vj[c], dp); }
        sc = lpq_sum<LPQ>(sc);
        dp = lpq_sum<LPQ>(dp);
        const float p = __expf(sc * scale - lse[(size_t)bh * Nq + i]);
        const float ds = p * (dp - delta[(size_t)bh * Nq + i]);
#pragma unroll
        for (int c = 0; c < DC; ++c) { av[c] = fmaf(p, dp_[c], av[c]); ak[c] = fmaf(ds, qp[c], ak[c]); }
    }
    if (!live) return;
#pragma unroll
    for (int c = 0; c < DC; ++c) { dk[off + c] = ak[c] * scale; dv[off + c] = av[c]; }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same three attention passes on the matrix cores (round 5): flash-style, one wave per 32 queries (forward, dq) or 32 keys (dk, dv),
// every product as THREE bf16 MFMA passes over (hi, lo) splits of its fp32 operands (x = hi + lo; hi.hi + lo.hi + hi.lo with fp32
// accumulation, the same scheme as the training GEMMs: 2^-16 relative), softmax arithmetic in fp32 registers. A prep pass writes every
// operand once per call in the two forms the MFMA fragments read straight from memory (no LDS in these kernels: a wave's fragment is
// one 16-byte load per lane):
//   R  [bh][N_pad][DP]   token-major rows, head dim zero-padded to a multiple of 16        (operand with k-slots over the head dim)
//   T  [bh][DPO][N_pad]  transposed, tokens permuted inside groups of 16 as [0-3, 8-11, 4-7, 12-15] (k-slots over tokens: the B
//                        operand of those products comes straight out of 32x32 accumulator registers, attention.hip's S^T -> P^T trick)
// each as hi and lo bf16. v_mfma_f32_32x32x16_bf16 layouts: A lane L = row L & 31, k-slots 8 (L >> 5) .. + 7; B lane L = column L & 31,
// same k-slots; D lane L = column L & 31, register 4 j + e = row 8 j + 4 (L >> 5) + e.
// Head dims 32 / 40 / 64 / 80 (d = 160 -- the 16 x 16 level, 256 tokens -- stays on the VALU kernels above: 5 % of the attention time).
struct APrep {
    const bf16* r_hi; const bf16* r_lo; const bf16* t_hi; const bf16* t_lo;
    int Npad;
};
__device__ __forceinline__ int perm16_tok(int t) {
    const int g = (t >> 2) & 3;
    return (t & ~15) | ((((g & 1) << 1) | (g >> 1)) << 2) | (t & 3);
}
// x [B][N][H d] fp32 (times mul) -> R / T hi / lo for every (b, h); one thread per (bh, token, column)
__global__ void attn_prep_kernel(const float* __restrict__ x, int N, int H, int d, float mul, int Npad, int DP, int DPO, bf16* __restrict__ r_hi,
                                 bf16* __restrict__ r_lo, bf16* __restrict__ t_hi, bf16* __restrict__ t_lo, size_t total) {
    const int CW = DP > DPO ? DP : DPO;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % CW);
        const int t = (int)((idx / CW) % Npad);
        const int bh = (int)(idx / ((size_t)CW * Npad));
        const int b = bh / H, h = bh - b * H;
        const float v = (t < N && c < d) ? x[(((size_t)b * N + t) * H + h) * d + c] * mul : 0.f;
        const bf16 hi = f2bf(v);
        const bf16 lo = f2bf(v - bf2f(hi));
        if (c < DP) {
            const size_t o = ((size_t)bh * Npad + t) * DP + c;
            r_hi[o] = hi; r_lo[o] = lo;
        }
        if (c < DPO) {
            const size_t o = ((size_t)bh * DPO + c) * Npad + perm16_tok(t);
            t_hi[o] = hi; t_lo[o] = lo;
        }
    }
}
// lse_pad [bh][Npad] (+1e30 behind the last query: its probabilities vanish), delta_pad [bh][Npad] = do_i . o_i (0 behind the last query)
__global__ void attn_delta_kernel(const float* __restrict__ o, const float* __restrict__ dout, const float* __restrict__ lse, int N, int H, int d, int Npad,
                                  float* __restrict__ lse_pad, float* __restrict__ delta_pad, size_t total) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(idx % Npad);
        const int bh = (int)(idx / Npad);
        const int b = bh / H, h = bh - b * H;
        float dl = 0.f, L = 1e30f;
        if (t < N) {
            const size_t off = (((size_t)b * N + t) * H + h) * d;
            for (int c = 0; c < d; ++c) dl = fmaf(dout[off + c], o[off + c], dl);
            L = lse[(size_t)bh * N + t];
        }
        lse_pad[idx] = L;
        delta_pad[idx] = dl;
    }
}
__device__ __forceinline__ float tr_max_xor32(float x) {
    const unsigned u = __float_as_uint(x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ bf16x8 ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
// acc += (ah + al) (bh + bl) without the lo.lo term
__device__ __forceinline__ void mfma3(f32x16& acc, const bf16x8& ah, const bf16x8& al, const bf16x8& bh, const bf16x8& bl) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
}
// accumulator registers 8 kk .. 8 kk + 7 of a 32 x 32 tile -> (hi, lo) B operands of k-step kk (k-slots = the tile's rows, in the
// permuted order of the T layouts)
__device__ __forceinline__ void split8(const f32x16& v, int kk, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = kk ? v[8 + e] : v[e];
        hi[e] = f2bf(x);
        lo[e] = f2bf(x - bf2f(hi[e]));
    }
}

// forward: o = softmax(q' k^T) v (q' = q scale, folded by the prep pass), lse = log sum exp. grid (Nq_pad / 32, B H), one wave
template <int DP, int DPO>
__global__ void __launch_bounds__(64) attn_mfma_fwd_kernel(APrep Q, APrep K, APrep V, int H, int d, int Nq, int Nk, float* __restrict__ o, float* __restrict__ lse) {
    constexpr int KS = DP / 16, DT = DPO / 32;
    const int lane = threadIdx.x, lrow = lane & 31, half = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H, q0 = blockIdx.x * 32;
    bf16x8 qh[KS], ql[KS];
    {
        const size_t off = ((size_t)bh * Q.Npad + q0 + lrow) * DP + 8 * half;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { qh[ks] = ld8(Q.r_hi + off + 16 * ks); ql[ks] = ld8(Q.r_lo + off + 16 * ks); }
    }
    f32x16 ot[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[i][r] = 0.f;
    float m = -1e30f, l = 0.f;
    const bf16* krh = K.r_hi + ((size_t)bh * K.Npad + lrow) * DP + 8 * half;
    const bf16* krl = K.r_lo + ((size_t)bh * K.Npad + lrow) * DP + 8 * half;
    const bf16* vth = V.t_hi + ((size_t)bh * DPO + lrow) * V.Npad + 8 * half;
    const bf16* vtl = V.t_lo + ((size_t)bh * DPO + lrow) * V.Npad + 8 * half;
    for (int k0 = 0; k0 < Nk; k0 += 32) {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) mfma3(s, ld8(krh + (size_t)k0 * DP + 16 * ks), ld8(krl + (size_t)k0 * DP + 16 * ks), qh[ks], ql[ks]);
        float mx = -1e30f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (k0 + 8 * (r >> 2) + 4 * half + (r & 3) >= Nk) s[r] = -1e30f;
            mx = fmaxf(mx, s[r]);
        }
        mx = tr_max_xor32(mx);
        const float mn = fmaxf(m, mx), alpha = __expf(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = __expf(s[r] - mn); ps += s[r]; }
        l = l * alpha + ps;
        m = mn;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[i][r] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 ph, pl;
            split8(s, kk, ph, pl);
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                const size_t off = (size_t)32 * i * V.Npad + k0 + 16 * kk;
                mfma3(ot[i], ld8(vth + off), ld8(vtl + off), ph, pl);
            }
        }
    }
    const float lt = l + __shfl_xor(l, 32, 64);
    const int q = q0 + lrow;
    if (q >= Nq) return;
    const float inv = 1.f / lt;
    float* op = o + (((size_t)b * Nq + q) * H + h) * d;
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dd = 32 * i + 8 * j + 4 * half;
            if (dd < d) *reinterpret_cast<float4*>(op + dd) = make_float4(ot[i][4 * j] * inv, ot[i][4 * j + 1] * inv, ot[i][4 * j + 2] * inv, ot[i][4 * j + 3] * inv);
        }
    if (half == 0) lse[(size_t)bh * Nq + q] = m + __logf(lt);
}

// dq = scale (dS K), dS = P (dP - delta), P = exp(q' k^T - lse), dP = do v^T. grid (Nq_pad / 32, B H), one wave
template <int DP, int DPO>
__global__ void __launch_bounds__(64) attn_mfma_bwd_q_kernel(APrep Q, APrep K, APrep V, APrep DO, const float* __restrict__ lse_pad,
                                                              const float* __restrict__ delta_pad, int H, int d, int Nq, int Nk, float scale,
                                                              float* __restrict__ dq) {
    constexpr int KS = DP / 16, DT = DPO / 32;
    const int lane = threadIdx.x, lrow = lane & 31, half = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H, q0 = blockIdx.x * 32;
    bf16x8 qh[KS], ql[KS], gh[KS], gl_[KS];
    {
        const size_t off = ((size_t)bh * Q.Npad + q0 + lrow) * DP + 8 * half;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qh[ks] = ld8(Q.r_hi + off + 16 * ks); ql[ks] = ld8(Q.r_lo + off + 16 * ks);
            gh[ks] = ld8(DO.r_hi + off + 16 * ks); gl_[ks] = ld8(DO.r_lo + off + 16 * ks);
        }
    }
    const float L = lse_pad[(size_t)bh * Q.Npad + q0 + lrow], dl = delta_pad[(size_t)bh * Q.Npad + q0 + lrow];
    f32x16 acc[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const size_t rbase = ((size_t)bh * K.Npad + lrow) * DP + 8 * half;
    const size_t tbase = ((size_t)bh * DPO + lrow) * K.Npad + 8 * half;
    for (int k0 = 0; k0 < Nk; k0 += 32) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const size_t off = rbase + (size_t)k0 * DP + 16 * ks;
            mfma3(s, ld8(K.r_hi + off), ld8(K.r_lo + off), qh[ks], ql[ks]);
            mfma3(dp, ld8(V.r_hi + off), ld8(V.r_lo + off), gh[ks], gl_[ks]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool ok = k0 + 8 * (r >> 2) + 4 * half + (r & 3) < Nk;
            s[r] = ok ? __expf(s[r] - L) * (dp[r] - dl) : 0.f;       // dS
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 dh, dlo;
            split8(s, kk, dh, dlo);
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                const size_t off = tbase + (size_t)32 * i * K.Npad + k0 + 16 * kk;
                mfma3(acc[i], ld8(K.t_hi + off), ld8(K.t_lo + off), dh, dlo);
            }
        }
    }
    const int q = q0 + lrow;
    if (q >= Nq) return;
    float* op = dq + (((size_t)b * Nq + q) * H + h) * d;
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dd = 32 * i + 8 * j + 4 * half;
            if (dd < d) *reinterpret_cast<float4*>(op + dd) = make_float4(acc[i][4 * j] * scale, acc[i][4 * j + 1] * scale, acc[i][4 * j + 2] * scale, acc[i][4 * j + 3] * scale);
        }
}

// dk = dS^T q' (= scale dS^T q), dv = P^T do. grid (Nk_pad / 32, B H), one wave owns 32 keys and walks the queries
template <int DP, int DPO>
__global__ void __launch_bounds__(64) attn_mfma_bwd_kv_kernel(APrep Q, APrep K, APrep V, APrep DO, const float* __restrict__ lse_pad,
                                                               const float* __restrict__ delta_pad, int H, int d, int Nq, int Nk, float* __restrict__ dk,
                                                               float* __restrict__ dv) {
    constexpr int KS = DP / 16, DT = DPO / 32;
    const int lane = threadIdx.x, lrow = lane & 31, half = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H, kb0 = blockIdx.x * 32;
    bf16x8 kh[KS], kl[KS], vh[KS], vl[KS];
    {
        const size_t off = ((size_t)bh * K.Npad + kb0 + lrow) * DP + 8 * half;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kh[ks] = ld8(K.r_hi + off + 16 * ks); kl[ks] = ld8(K.r_lo + off + 16 * ks);
            vh[ks] = ld8(V.r_hi + off + 16 * ks); vl[ks] = ld8(V.r_lo + off + 16 * ks);
        }
    }
    f32x16 ak[DT], av[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { ak[i][r] = 0.f; av[i][r] = 0.f; }
    const size_t rbase = ((size_t)bh * Q.Npad + lrow) * DP + 8 * half;
    const size_t tbase = ((size_t)bh * DPO + lrow) * Q.Npad + 8 * half;
    const float* Lp = lse_pad + (size_t)bh * Q.Npad + 4 * half;
    const float* Dp = delta_pad + (size_t)bh * Q.Npad + 4 * half;
    const int nq_pad32 = (Nq + 31) & ~31;
    for (int q0 = 0; q0 < nq_pad32; q0 += 32) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const size_t off = rbase + (size_t)q0 * DP + 16 * ks;
            mfma3(s, ld8(Q.r_hi + off), ld8(Q.r_lo + off), kh[ks], kl[ks]);      // rows = queries, columns = this wave's keys
            mfma3(dp, ld8(DO.r_hi + off), ld8(DO.r_lo + off), vh[ks], vl[ks]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 L4 = *reinterpret_cast<const float4*>(Lp + q0 + 8 * j);
            const float4 D4 = *reinterpret_cast<const float4*>(Dp + q0 + 8 * j);
            const float Lr[4] = {L4.x, L4.y, L4.z, L4.w}, Dr[4] = {D4.x, D4.y, D4.z, D4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = __expf(s[4 * j + e] - Lr[e]);        // (queries behind the last one carry lse = 1e30: p = 0)
                s[4 * j + e] = p;
                dp[4 * j + e] = p * (dp[4 * j + e] - Dr[e]);          // dS
            }
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 ph, pl, dh, dlo;
            split8(s, kk, ph, pl);
            split8(dp, kk, dh, dlo);
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                const size_t off = tbase + (size_t)32 * i * Q.Npad + q0 + 16 * kk;
                mfma3(av[i], ld8(DO.t_hi + off), ld8(DO.t_lo + off), ph, pl);
                mfma3(ak[i], ld8(Q.t_hi + off), ld8(Q.t_lo + off), dh, dlo);
            }
        }
    }
    const int key = kb0 + lrow;
    if (key >= Nk) return;
    const size_t ob = (((size_t)b * Nk + key) * H + h) * d;
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dd = 32 * i + 8 * j + 4 * half;
            if (dd < d) {
                *reinterpret_cast<float4*>(dk + ob + dd) = make_float4(ak[i][4 * j], ak[i][4 * j + 1], ak[i][4 * j + 2], ak[i][4 * j + 3]);
                *reinterpret_cast<float4*>(dv + ob + dd) = make_float4(av[i][4 * j], av[i][4 * j + 1], av[i][4 * j + 2], av[i][4 * j + 3]);
            }
        }
}

// ---- the one dispatch table: which instantiation serves a head dim. f is called with the two template arguments as
// std::integral_constants; false: no instantiation
template <int V> using Int = std::integral_constant<int, V>;
template <class F>
bool with_valu_dims(int D, F&& f) {       // <DC, LPQ>, D = DC * LPQ
    switch (D) {
        case 32: f(Int<32>{}, Int<1>{}); return true;
        case 40: f(Int<40>{}, Int<1>{}); return true;
        case 64: f(Int<32>{}, Int<2>{}); return true;
        case 80: f(Int<40>{}, Int<2>{}); return true;
        case 160: f(Int<40>{}, Int<4>{}); return true;
        default: return false;
    }
}
template <class F>
void with_mfma_dims(int D, F&& f) {       // <DP, DPO> = D rounded up to 16 / 32; D is one of attn_on_mfma's
    switch (D) {
        case 32: f(Int<32>{}, Int<32>{}); break;
        case 40: f(Int<48>{}, Int<64>{}); break;
        case 64: f(Int<64>{}, Int<64>{}); break;
        default: f(Int<80>{}, Int<96>{}); break;
    }
}
// GL_TRAIN_ATTN_VALU=1 (developer A/B) keeps every head dim on the VALU kernels
bool attn_on_mfma(int D) {
    static const bool valu = dev_env("GL_TRAIN_ATTN_VALU") && atoi(dev_env("GL_TRAIN_ATTN_VALU")) != 0;
    return !valu && (D == 32 || D == 40 || D == 64 || D == 80);
}

// the prep pass over one operand (a function of this unit, not a Ctx method: APrep is a kernel parameter type and stays in this unit's
// unnamed namespace with the kernels)
APrep attn_prep(const Ctx& c, const float* x, int B, int N, int H, int D, float mul) {
    const int Npad = round_up(N, 64), DP = round_up(D, 16), DPO = round_up(D, 32);
    const size_t nr = (size_t)B * H * Npad * DP, nt = (size_t)B * H * DPO * Npad;
    bf16* rh = c.ar.get<bf16>(nr); bf16* rl = c.ar.get<bf16>(nr); bf16* th = c.ar.get<bf16>(nt); bf16* tl = c.ar.get<bf16>(nt);
    const size_t total = (size_t)B * H * Npad * std::max(DP, DPO);
    hipLaunchKernelGGL(attn_prep_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65535 * 16)), dim3(256), 0, c.s, x, N, H, D, mul, Npad, DP, DPO, rh, rl, th,
                       tl, total);
    return APrep{rh, rl, th, tl, Npad};
}

}  // namespace

namespace train {

// ---- attention on row-major q [B][Nq][H D], k / v [B][Nk][H D]; dk, dv null: dq only
Ctx::Attn Ctx::attn_fwd(int D, const float* q, const float* k, const float* v, int B, int H, int Nq, int Nk) const {
    const float sc = 1.f / sqrtf((float)D);
    if (attn_on_mfma(D)) {
        Attn a{f32((size_t)B * Nq * H * D), f32((size_t)B * H * Nq)};
        const size_t mk = ar.mark();
        const APrep Q = attn_prep(*this, q, B, Nq, H, D, sc), K = attn_prep(*this, k, B, Nk, H, D, 1.f), V = attn_prep(*this, v, B, Nk, H, D, 1.f);
        with_mfma_dims(D, [&](auto dp, auto dpo) {
            hipLaunchKernelGGL((attn_mfma_fwd_kernel<dp(), dpo()>), dim3(Q.Npad / 32, B * H), dim3(64), 0, s, Q, K, V, H, D, Nq, Nk, a.o, a.lse);
        });
        ar.release(mk);
        return a;
    }
    Attn a{};
    const bool built = with_valu_dims(D, [&](auto dc, auto lpq) {
        a = Attn{f32((size_t)B * Nq * H * D), f32((size_t)B * H * Nq)};
        hipLaunchKernelGGL((attn_fwd_kernel<dc(), lpq()>), dim3(cdiv(Nq * lpq(), 64), B * H), dim3(64), 0, s, q, k, v, H, Nq, Nk, sc, a.o, a.lse);
    });
    if (!built) throw GlError(GL_ERR_UNSUPPORTED, fmt("training slice: head dim %d (32, 40, 64, 80, 160 are built)", D));
    return a;
}

void Ctx::attn_bwd(int D, const float* q, const float* k, const float* v, const Attn& f, const float* dout, int B, int H, int Nq, int Nk, float* dq, float* dk,
                   float* dv) const {
    const float sc = 1.f / sqrtf((float)D);
    if (attn_on_mfma(D)) {
        const size_t mk = ar.mark();
        const APrep Q = attn_prep(*this, q, B, Nq, H, D, sc), K = attn_prep(*this, k, B, Nk, H, D, 1.f), V = attn_prep(*this, v, B, Nk, H, D, 1.f),
                    G = attn_prep(*this, dout, B, Nq, H, D, 1.f);
        float* lp = f32((size_t)B * H * Q.Npad);
        float* dp = f32((size_t)B * H * Q.Npad);
        const size_t total = (size_t)B * H * Q.Npad;
        ew(attn_delta_kernel, total, f.o, dout, f.lse, Nq, H, D, Q.Npad, lp, dp, total);
        with_mfma_dims(D, [&](auto dpad, auto dpo) {
            hipLaunchKernelGGL((attn_mfma_bwd_q_kernel<dpad(), dpo()>), dim3(Q.Npad / 32, B * H), dim3(64), 0, s, Q, K, V, G, lp, dp, H, D, Nq, Nk, sc, dq);
            if (dk && dv)
                hipLaunchKernelGGL((attn_mfma_bwd_kv_kernel<dpad(), dpo()>), dim3(K.Npad / 32, B * H), dim3(64), 0, s, Q, K, V, G, lp, dp, H, D, Nq, Nk, dk, dv);
        });
        ar.release(mk);
        return;
    }
    const bool built = with_valu_dims(D, [&](auto dc, auto lpq) {
        float* delta = f32((size_t)B * H * Nq);
        hipLaunchKernelGGL((attn_bwd_q_kernel<dc(), lpq()>), dim3(cdiv(Nq * lpq(), 64), B * H), dim3(64), 0, s, q, k, v, f.o, dout, f.lse, H, Nq, Nk, sc, dq, delta);
        if (dk && dv)
            hipLaunchKernelGGL((attn_bwd_kv_kernel<dc(), lpq()>), dim3(cdiv(Nk * lpq(), 64), B * H), dim3(64), 0, s, q, k, v, dout, f.lse, delta, H, Nq, Nk, sc, dk, dv);
    });
    if (!built) throw GlError(GL_ERR_UNSUPPORTED, "training slice: head dim");
}

}  // namespace train

// attn_fwd, then attn_bwd when dout is given (train.h). o and lse are the forward's arena buffers copied out; the backward writes dq,
// dk, dv where the caller points, as the step's own calls do.
int train_prim_attention(Arena& ar, float* ws, size_t ws_bytes, int B, int H, int D, int Nq, int Nk, const float* q, const float* k, const float* v,
                         const float* dout, float* o, float* lse, float* dq, float* dk, float* dv, hipStream_t s) {
    if (B < 1 || H < 1 || Nq < 1 || Nk < 1) return set_error(GL_ERR_ARG, "gl_op_train_attention: B=%d H=%d Nq=%d Nk=%d", B, H, Nq, Nk);
    if (!with_valu_dims(D, [](auto, auto) {})) return set_error(GL_ERR_ARG, "gl_op_train_attention: head dim %d (32, 40, 64, 80, 160 are built)", D);
    try {
        Ctx c{ar, ws, ws_bytes, s};
        const size_t nq = (size_t)B * Nq * H * D;
        const Ctx::Attn f = c.attn_fwd(D, q, k, v, B, H, Nq, Nk);
        c.hip(hipMemcpyAsync(o, f.o, nq * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
        c.hip(hipMemcpyAsync(lse, f.lse, (size_t)B * H * Nq * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
        if (dout) c.attn_bwd(D, q, k, v, f, dout, B, H, Nq, Nk, dq ? dq : c.f32(nq), dk, dv);
        c.hip(hipGetLastError(), "training attention kernel launch");
    } catch (const GlError& e) {
        return set_error(e.code, "%s", e.what());
    }
    return GL_OK;
}

}  // namespace gl
