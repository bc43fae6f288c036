// CLIP tower kernels for gfx950 (see clip.h). Work per text call is small (S <= ~32 sequences of <= 77 tokens, 13 GFLOP each at
// ViT-L/14 size): the aim is few, exact, spill-free launches. The projections run on the bf16 MFMA GEMM (gemm.h; kernel: gemm_u.hip).
#include "clip.h"

#include <math.h>

namespace gl {

// ---------------------------------------------------------------------------------------------------------------- embedding
__global__ __launch_bounds__(256) void clip_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                         float* __restrict__ h, int rows, int T, int w4, int vocab, unsigned* bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * w4) return;
    const int row = (int)(i / w4), c = (int)(i - (int64_t)row * w4);
    int id = ids[row];
    if (id < 0 || id >= vocab) {
        if (bad && c == 0) atomicAdd(bad, 1u);
        id = id < 0 ? 0 : vocab - 1;
    }
    const float4 a = reinterpret_cast<const float4*>(tok)[(size_t)id * w4 + c];
    const float4 b = reinterpret_cast<const float4*>(pos)[(size_t)(row % T) * w4 + c];
    reinterpret_cast<float4*>(h)[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

int clip_embed_launch(const int32_t* ids, const float* tok, const float* pos, float* h, int rows, int T, int width, int vocab, unsigned* bad,
                      hipStream_t stream) {
    if (rows <= 0 || T <= 0 || width <= 0 || width % 4 || vocab <= 0) return set_error(GL_ERR_ARG, "clip_embed: rows=%d T=%d width=%d vocab=%d", rows, T, width, vocab);
    const int64_t n = (int64_t)rows * (width / 4);
    hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, stream, ids, tok, pos, h, rows, T, width / 4, vocab, bad);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// ------------------------------------------------------------------------------------------- residual add + LayerNorm (fp32 stream)
// One wave per row; the row stays in registers between the add, the two statistics passes (mean, then centred variance) and the
// affine output, so the fp32 residual stream is read once and written once per sub-layer.
__global__ __launch_bounds__(256) void clip_add_ln_kernel(float* __restrict__ h, const float* __restrict__ delta, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, bf16* __restrict__ ybf, float* __restrict__ yf32,
                                                          int rows, int width) {
    constexpr int MAXV = kClipMaxWidth / 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* hr = h + (size_t)row * width;
    float4 v[MAXV];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < width) {
            v[i] = *reinterpret_cast<const float4*>(hr + c);
            if (delta) {
                const float4 d = *reinterpret_cast<const float4*>(delta + (size_t)row * width + c);
                v[i].x += d.x; v[i].y += d.y; v[i].z += d.z; v[i].w += d.w;
                *reinterpret_cast<float4*>(hr + c) = v[i];
            }
            sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
    }
    const float mean = wave_sum(sum) / (float)width;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < width) {
            const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
            sq += (a * a + b * b) + (cc * cc + d * d);
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)width + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < width) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c);
            const float4 b = *reinterpret_cast<const float4*>(beta + c);
            float y[4] = {(v[i].x - mean) * rstd * g.x + b.x, (v[i].y - mean) * rstd * g.y + b.y, (v[i].z - mean) * rstd * g.z + b.z,
                          (v[i].w - mean) * rstd * g.w + b.w};
            if (yf32) {
                *reinterpret_cast<float4*>(yf32 + (size_t)row * width + c) = make_float4(y[0], y[1], y[2], y[3]);
            } else {
                U2BF4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o.e[e] = f2bf(y[e]);
                *reinterpret_cast<uint2*>(ybf + (size_t)row * width + c) = o.u;
            }
        }
    }
}

int clip_add_ln_launch(float* h, const float* delta, const float* gamma, const float* beta, float eps, bf16* ybf, float* yf32, int rows, int width,
                       hipStream_t stream) {
    if (rows <= 0 || width <= 0 || width % 4 || width > kClipMaxWidth || !gamma || !beta || (!ybf == !yf32))
        return set_error(GL_ERR_ARG, "clip_add_ln: rows=%d width=%d (width %% 4 == 0, <= %d; one output)", rows, width, kClipMaxWidth);
    hipLaunchKernelGGL(clip_add_ln_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, h, delta, gamma, beta, eps, ybf, yf32, rows, width);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// ---------------------------------------------------------------------------------------------------------------- attention
// One workgroup per (sequence, head), one wave per 32-query tile (T <= 96: three waves). Q, K and V^T of the head are staged once in
// LDS (40 KB: two workgroups per CU); rows / keys beyond T are zeros. Both products run on v_mfma_f32_32x32x16_bf16 in the swapped
// form of attention.hip: S^T = K Q^T puts the query on the lane and the 32 keys of a tile in the 16 accumulator registers of the two
// lane halves, so the row maximum / sum are register reductions plus one exchange with lane ^ 32, and the bf16-packed accumulator
// IS the B operand of O^T += V^T P^T (k order inside a step: key 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3), which is how the V^T
// fragment is gathered). All (at most three) score tiles of a query tile are held at once: plain two-pass softmax in fp32, no
// rescaling. Keys above the diagonal and keys >= T are set to -inf BEFORE the row maximum (p = 0 exactly: rows at or before a
// position do not depend on what follows it); key tiles entirely above the diagonal are not computed.
constexpr int CA_LDQ = kClipHeadDim + 8;     // Q / K row stride in LDS (elements): 144 B, 16-byte fragment reads
constexpr int CA_LDV = kClipMaxTokens + 4;   // V^T row stride: 200 B, 8-byte fragment reads, rows 50 dwords apart

__global__ __launch_bounds__(192) void clip_attn_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o, int T, int H, int causal) {
    __shared__ __attribute__((aligned(16))) bf16 sQ[kClipMaxTokens * CA_LDQ];
    __shared__ __attribute__((aligned(16))) bf16 sK[kClipMaxTokens * CA_LDQ];
    __shared__ __attribute__((aligned(16))) bf16 sVt[kClipHeadDim * CA_LDV];
    const int s = blockIdx.x / H, h = blockIdx.x - s * H;
    const int W = H * kClipHeadDim, ld = 3 * W;
    const bf16* base = qkv + (size_t)s * T * ld + h * kClipHeadDim;
    for (int i = threadIdx.x; i < kClipMaxTokens * 8; i += 192) {
        const int t = i >> 3, c = i & 7;
        uint4 q = make_uint4(0, 0, 0, 0), k = q;
        U4BF8 v;
        v.u = q;
        if (t < T) {
            const bf16* p = base + (size_t)t * ld + c * 8;
            q = *reinterpret_cast<const uint4*>(p);
            k = *reinterpret_cast<const uint4*>(p + W);
            v.u = *reinterpret_cast<const uint4*>(p + 2 * W);
        }
        *reinterpret_cast<uint4*>(sQ + t * CA_LDQ + c * 8) = q;
        *reinterpret_cast<uint4*>(sK + t * CA_LDQ + c * 8) = k;
#pragma unroll
        for (int j = 0; j < 8; ++j) sVt[(c * 8 + j) * CA_LDV + t] = v.e[j];
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, hh = lane >> 5;
    const int q0 = wave * 32;
    if (q0 >= T) return;
    const int qi = q0 + r;
    const int nkt = causal ? wave + 1 : (T + 31) >> 5;

    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(sQ + qi * CA_LDQ + ks * 16 + hh * 8);

    // ---- S^T tiles: [32 keys][32 queries], masked, scaled into the exp2 domain
    const float scale = 0.125f * 1.4426950408889634f;   // 64^-0.5 * log2(e)
    f32x16 sc[3];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
        if (kt < nkt) {
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (kt * 32 + r) * CA_LDQ + ks * 16 + hh * 8);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int key = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                const bool ok = key < T && (!causal || key <= qi);
                acc[e] = ok ? acc[e] * scale : -INFINITY;
                m = fmaxf(m, acc[e]);
            }
            sc[kt] = acc;
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));   // key 0 is valid for every query: m is finite

    // ---- p = exp2(s - m), row sum in fp32; O^T[d][query] += V^T[d][key] P^T[key][query]
    f32x16 ot[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) ot[dt][e] = 0.f;
    float lsum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
        if (kt < nkt) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                bf16x8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = __builtin_amdgcn_exp2f(sc[kt][8 * st + j] - m);
                    lsum += p;
                    pf[j] = f2bf(p);
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const bf16* vp = sVt + (dt * 32 + r) * CA_LDV + kt * 32 + 16 * st + 4 * hh;
                    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vp);
                    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vp + 8);
                    const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                    ot[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, ot[dt], 0, 0, 0);
                }
            }
        }
    }
    lsum += __shfl_xor(lsum, 32, 64);
    if (qi >= T) return;
    const float inv = 1.f / lsum;
    bf16* orow = o + ((size_t)s * T + qi) * W + h * kClipHeadDim;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            U2BF4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov.e[e] = f2bf(ot[dt][4 * g + e] * inv);
            *reinterpret_cast<uint2*>(orow + dt * 32 + 8 * g + 4 * hh) = ov.u;
        }
}

// ------------------------------------------------------------------------------------------------ attention, 96 < T <= 288
// The vision tower's attention (ViT-L/14: 257 tokens, not causal). One workgroup of four waves per (sequence, head, block of 128
// queries), one wave per 32-query tile. K and V^T of the whole head are staged once in LDS at the padded strides of clip_attn_kernel
// (K rows 144 B apart: conflict-free 16-byte fragment reads; V^T rows 584 B = 146 dwords apart: 18 r mod 64 is even and distinct over
// 32 rows, conflict-free 8-byte reads): 41472 + 37376 = 78848 B, so TWO workgroups share the 160 KB of a CU -- which is why the cap is
// 288 tokens and not 320 (88 KB, one workgroup of four waves per CU). Q never enters LDS: the query sits on the lane, so each lane
// reads the four 16-byte fragments of its own row straight from the qkv rows. The products are clip_attn_kernel's (S^T = K Q^T, the
// bf16-packed score accumulator is the B operand of O^T += V^T P^T), but nine score tiles at once would be 144 accumulator registers,
// so each wave walks the 32-key tiles with an online softmax: running maximum m, running fp32 sum and O^T rescaled by
// exp2(m_old - m_new) per tile. Keys >= T are -inf before the maximum (p = 0 exactly; their K / V rows in LDS are zeros and are never
// read from memory); key 0 is valid for every query, so m is finite from the first tile on. Query rows >= T run on zeros and are not
// stored; a wave whose tile lies entirely behind T leaves after the barrier.
constexpr int CL_LDV = kClipLongMaxTokens + 4;   // V^T row stride (elements)
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void clip_attn_long_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o, int T, int H, int nqb) {
    __shared__ __attribute__((aligned(16))) bf16 sK[kClipLongMaxTokens * CA_LDQ];
    __shared__ __attribute__((aligned(16))) bf16 sVt[kClipHeadDim * CL_LDV];
    const int qb = blockIdx.x % nqb, sh = blockIdx.x / nqb;
    const int s = sh / H, h = sh - s * H;
    const int W = H * kClipHeadDim, ld = 3 * W;
    const bf16* base = qkv + (size_t)s * T * ld + h * kClipHeadDim;
    const int nkt = (T + 31) >> 5;
    // token pairs (2 tp, 2 tp + 1) x 16-byte chunks: K rows verbatim, V transposed as one dword (two tokens of one feature) per store
    for (int i = threadIdx.x; i < nkt * 16 * 8; i += 256) {
        const int tp = i >> 3, c = i & 7, t0 = 2 * tp;
        U4BF8 k0, k1, v0, v1;
        k0.u = k1.u = v0.u = v1.u = make_uint4(0, 0, 0, 0);
        if (t0 < T) {
            const bf16* p = base + (size_t)t0 * ld + c * 8;
            k0.u = *reinterpret_cast<const uint4*>(p + W);
            v0.u = *reinterpret_cast<const uint4*>(p + 2 * W);
            if (t0 + 1 < T) {
                k1.u = *reinterpret_cast<const uint4*>(p + ld + W);
                v1.u = *reinterpret_cast<const uint4*>(p + ld + 2 * W);
            }
        }
        *reinterpret_cast<uint4*>(sK + t0 * CA_LDQ + c * 8) = k0.u;
        *reinterpret_cast<uint4*>(sK + (t0 + 1) * CA_LDQ + c * 8) = k1.u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            bf16x2 pr;
            pr[0] = v0.e[j];
            pr[1] = v1.e[j];
            *reinterpret_cast<bf16x2*>(sVt + (c * 8 + j) * CL_LDV + t0) = pr;
        }
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, hh = lane >> 5;
    const int q0 = qb * 128 + wave * 32;
    if (q0 >= T) return;
    const int qi = q0 + r;

    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        U4BF8 q;
        q.u = make_uint4(0, 0, 0, 0);
        if (qi < T) q.u = *reinterpret_cast<const uint4*>(base + (size_t)qi * ld + ks * 16 + hh * 8);
        qf[ks] = q.v;
    }

    const float scale = 0.125f * 1.4426950408889634f;   // 64^-0.5 * log2(e)
    f32x16 ot[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) ot[dt][e] = 0.f;
    float m = -INFINITY, lsum = 0.f;
#pragma unroll 1
    for (int kt = 0; kt < nkt; ++kt) {
        // ---- S^T tile: [32 keys][32 queries], masked, scaled into the exp2 domain
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (kt * 32 + r) * CA_LDQ + ks * 16 + hh * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
        }
        float tm = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
            acc[e] = key < T ? acc[e] * scale : -INFINITY;
            tm = fmaxf(tm, acc[e]);
        }
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const float mn = fmaxf(m, tm);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);   // first tile: exp2(-inf) = 0 on a zero state
        m = mn;
        lsum *= alpha;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) ot[dt][e] *= alpha;
        // ---- p = exp2(s - m); O^T[d][query] += V^T[d][key] P^T[key][query]
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            bf16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = __builtin_amdgcn_exp2f(acc[8 * st + j] - m);
                lsum += p;
                pf[j] = f2bf(p);
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16* vp = sVt + (dt * 32 + r) * CL_LDV + kt * 32 + 16 * st + 4 * hh;
                const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vp);
                const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vp + 8);
                const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                ot[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, ot[dt], 0, 0, 0);
            }
        }
    }
    lsum += __shfl_xor(lsum, 32, 64);
    if (qi >= T) return;
    const float inv = 1.f / lsum;
    bf16* orow = o + ((size_t)s * T + qi) * W + h * kClipHeadDim;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            U2BF4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov.e[e] = f2bf(ot[dt][4 * g + e] * inv);
            *reinterpret_cast<uint2*>(orow + dt * 32 + 8 * g + 4 * hh) = ov.u;
        }
}

int clip_attn_launch(const bf16* qkv, bf16* o, int S, int T, int heads, int causal, hipStream_t stream) {
    if (S <= 0 || heads <= 0 || T <= 0) return set_error(GL_ERR_UNSUPPORTED, "clip_attn: S=%d heads=%d T=%d (all >= 1)", S, heads, T);
    if (T <= kClipMaxTokens) {
        hipLaunchKernelGGL(clip_attn_kernel, dim3(S * heads), dim3(192), 0, stream, qkv, o, T, heads, causal);
        GL_LAUNCH_CHECK();
        return GL_OK;
    }
    if (causal) return set_error(GL_ERR_UNSUPPORTED, "clip_attn: causal attention over T=%d tokens (causal needs T <= %d)", T, kClipMaxTokens);
    if (T > kClipLongMaxTokens) return set_error(GL_ERR_UNSUPPORTED, "clip_attn: T=%d tokens exceed the %d clip_attn_long_kernel holds", T, kClipLongMaxTokens);
    const int nqb = cdiv(T, 128);
    hipLaunchKernelGGL(clip_attn_long_kernel, dim3(S * heads * nqb), dim3(256), 0, stream, qkv, o, T, heads, nqb);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// ------------------------------------------------------------------------------------------------------- vision tower: embeddings
// Patch rows for the 14 x 14 stride-14 (p x p stride-p) convolution as a GEMM: out[s * G * G + py * G + px][(c, ky, kx)] =
// pixel_values[s][c][py * p + ky][px * p + kx], read from NCHW as it is, bf16, columns [3 p p, Kpad) zero.
__global__ __launch_bounds__(256) void clip_patch_rows_kernel(const float* __restrict__ px, bf16* __restrict__ out, int S, int HW, int p, int G, int Kpad) {
    const int pp = p * p, K = 3 * pp;
    const int64_t total = (int64_t)S * G * G * Kpad;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t row = idx / Kpad;
        const int k = (int)(idx - row * Kpad);
        float v = 0.f;
        if (k < K) {
            const int c = k / pp, rem = k - c * pp, ky = rem / p, kx = rem - ky * p;
            const int s = (int)(row / (G * G)), cell = (int)(row - (int64_t)s * G * G), py = cell / G, pxi = cell - py * G;
            v = px[(((size_t)s * 3 + c) * HW + (py * p + ky)) * HW + pxi * p + kx];
        }
        out[idx] = f2bf(v);
    }
}

int clip_patch_rows_launch(const float* pixel_values, bf16* out, int S, int image_size, int patch, int Kpad, hipStream_t stream) {
    if (S <= 0 || patch <= 0 || image_size <= 0 || image_size % patch || Kpad % 64 || Kpad < 3 * patch * patch)
        return set_error(GL_ERR_ARG, "clip_patch_rows: S=%d image_size=%d patch=%d Kpad=%d", S, image_size, patch, Kpad);
    const int G = image_size / patch;
    int64_t g = cdiv64((int64_t)S * G * G * Kpad, 256);
    if (g > 65535) g = 65535;
    hipLaunchKernelGGL(clip_patch_rows_kernel, dim3((unsigned)g), dim3(256), 0, stream, pixel_values, out, S, image_size, patch, G, Kpad);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// h[s][0] = class_embedding + pos[0]; h[s][1 + i] = patch[s * (T - 1) + i] + pos[1 + i] (fp32)
__global__ __launch_bounds__(256) void clip_vision_embed_kernel(const float* __restrict__ patch, const float* __restrict__ cls, const float* __restrict__ pos,
                                                                float* __restrict__ h, int rows, int T, int w4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * w4) return;
    const int row = (int)(i / w4), c = (int)(i - (int64_t)row * w4);
    const int s = row / T, t = row - s * T;
    const float4 a = t ? reinterpret_cast<const float4*>(patch)[((size_t)s * (T - 1) + (t - 1)) * w4 + c] : reinterpret_cast<const float4*>(cls)[c];
    const float4 b = reinterpret_cast<const float4*>(pos)[(size_t)t * w4 + c];
    reinterpret_cast<float4*>(h)[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

int clip_vision_embed_launch(const float* patch, const float* cls, const float* pos, float* h, int S, int T, int width, hipStream_t stream) {
    if (S <= 0 || T < 2 || width <= 0 || width % 4) return set_error(GL_ERR_ARG, "clip_vision_embed: S=%d T=%d width=%d", S, T, width);
    const int64_t n = (int64_t)S * T * (width / 4);
    hipLaunchKernelGGL(clip_vision_embed_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, stream, patch, cls, pos, h, S * T, T, width / 4);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// --------------------------------------------------------------------------------------- LayerNorm of strided rows (vision tower)
// clip_add_ln_kernel's row routine without the stream write-back and with row strides: y[row] = LayerNorm(x[row] (+ delta[row])).
// y may BE x (pre_layrnorm: the residual stream starts from the normalised rows, so the launch overwrites it -- each lane reads the
// elements it writes before it writes them, and no pointer here is __restrict__), and a stride of T * width picks the class-token
// rows for post_layernorm without a gather. Either or both outputs.
__global__ __launch_bounds__(256) void clip_ln_rows_kernel(const float* x, const float* delta, int64_t in_stride, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float* yf32, bf16* ybf, int64_t out_stride, int rows,
                                                           int width) {
    constexpr int MAXV = kClipMaxWidth / 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * in_stride;
    float4 v[MAXV];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < width) {
            v[i] = *reinterpret_cast<const float4*>(xr + c);
            if (delta) {
                const float4 d = *reinterpret_cast<const float4*>(delta + (size_t)row * in_stride + c);
                v[i].x += d.x; v[i].y += d.y; v[i].z += d.z; v[i].w += d.w;
            }
            sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
    }
    const float mean = wave_sum(sum) / (float)width;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < width) {
            const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
            sq += (a * a + b * b) + (cc * cc + d * d);
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)width + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < width) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c);
            const float4 b = *reinterpret_cast<const float4*>(beta + c);
            float y[4] = {(v[i].x - mean) * rstd * g.x + b.x, (v[i].y - mean) * rstd * g.y + b.y, (v[i].z - mean) * rstd * g.z + b.z,
                          (v[i].w - mean) * rstd * g.w + b.w};
            if (yf32) *reinterpret_cast<float4*>(yf32 + (size_t)row * out_stride + c) = make_float4(y[0], y[1], y[2], y[3]);
            if (ybf) {
                U2BF4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o.e[e] = f2bf(y[e]);
                *reinterpret_cast<uint2*>(ybf + (size_t)row * out_stride + c) = o.u;
            }
        }
    }
}

int clip_ln_rows_launch(const float* x, const float* delta, int64_t in_stride, const float* gamma, const float* beta, float eps, float* yf32, bf16* ybf,
                        int64_t out_stride, int rows, int width, hipStream_t stream) {
    if (rows <= 0 || width <= 0 || width % 4 || width > kClipMaxWidth || !x || !gamma || !beta || (!ybf && !yf32) || in_stride < width || out_stride < width ||
        in_stride % 4 || out_stride % 4)
        return set_error(GL_ERR_ARG, "clip_ln_rows: rows=%d width=%d strides %lld / %lld (width %% 4 == 0, <= %d; strides >= width, %% 4 == 0; an output)", rows,
                         width, (long long)in_stride, (long long)out_stride, kClipMaxWidth);
    hipLaunchKernelGGL(clip_ln_rows_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, x, delta, in_stride, gamma, beta, eps, yf32, ybf, out_stride, rows, width);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// out = a + b (fp32 rows; the vision tower's last_hidden_state = the stream + the last fc2 output, which no LayerNorm follows)
__global__ __launch_bounds__(256) void clip_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
    reinterpret_cast<float4*>(out)[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
}

int clip_add_launch(const float* a, const float* b, float* out, int64_t n, hipStream_t stream) {
    if (n <= 0 || n % 4 || !a || !b || !out) return set_error(GL_ERR_ARG, "clip_add: n=%lld (a positive multiple of 4)", (long long)n);
    hipLaunchKernelGGL(clip_add_kernel, dim3((unsigned)cdiv64(n / 4, 256)), dim3(256), 0, stream, a, b, out, n / 4);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// ---------------------------------------------------------------------------------------------------------------- pooling
__global__ __launch_bounds__(256) void clip_pool_kernel(const float* __restrict__ x, const int32_t* __restrict__ eos, float* __restrict__ pooled, int T, int w4) {
    const int s = blockIdx.x;
    int t = eos[s];
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    const float4* src = reinterpret_cast<const float4*>(x) + ((size_t)s * T + t) * w4;
    float4* dst = reinterpret_cast<float4*>(pooled) + (size_t)s * w4;
    for (int c = threadIdx.x; c < w4; c += 256) dst[c] = src[c];
}

int clip_pool_launch(const float* x, const int32_t* eos, float* pooled, int S, int T, int width, hipStream_t stream) {
    if (S <= 0 || T <= 0 || width <= 0 || width % 4) return set_error(GL_ERR_ARG, "clip_pool: S=%d T=%d width=%d", S, T, width);
    hipLaunchKernelGGL(clip_pool_kernel, dim3(S), dim3(256), 0, stream, x, eos, pooled, T, width / 4);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
