// gligen_amd -- flash attention of the VAE's single-head AttnBlock (C = 256 | 512), gfx950
#include "vae_attention.h"

#include <cmath>

namespace gl {

// ------------------------------------------------------------------------------------------------ vae_attn_flash_kernel
// One head whose dimension is the whole channel count: a 64-key tile of K alone is 64 KB at C = 512 and the O accumulator of 32
// queries is 512 x 32 fp32, so the head dimension -- not the queries -- is what the four waves of a workgroup divide. One workgroup
// per (image, block of 64 queries = two 32-query tiles); wave w owns channels [w C/4, (w + 1) C/4) of q, k, v^T and of the output:
//   1. partial S^T = K[:, slice] Q^T[slice, :] for the tile's two 32-key subtiles and both query tiles (4 x C/64 MFMAs), K fragments
//      straight from the rows, each used for both query tiles (every wave reads its own slice: nothing is shared between waves, so K
//      does not pass through LDS; what bounds the kernel is streaming K and V^T once per workgroup, hence two query tiles);
//   2. the four partial score tiles meet in LDS (4 x 16 fp32 per lane per wave, float4 stores, 64 KB, a barrier in front of the reads
//      and one behind them); every wave sums them in wave order, so all four hold the same bits of S^T, and runs the same online
//      softmax on them (128 exp2 per lane per tile, against 64 | 32 MFMAs: cheaper than a second LDS round trip for P);
//   3. O^T[slice] += V^T[slice] P^T with the bf16-packed score registers as the B operand (no LDS, no lane movement), each V^T
//      fragment used for both query tiles.
// Row rho of a score subtile is key pi(rho) = rho with bits 2 and 3 exchanged: the registers 8 s .. 8 s + 7 that lane half h packs into
// the B fragment of k-step s then hold keys 16 s + 8 h .. + 7, so the matching V^T fragment is ONE 16-byte load of consecutive keys.
// T % 64 == 0: no key is masked, no query tile is partial and m is finite from the first tile on. One workgroup per CU (64 KB of LDS,
// more than 256 registers: one wave per SIMD).
constexpr int kVaeAttnQueryTiles = 2;   // 32-query tiles per workgroup

template <int C>
__global__ __launch_bounds__(256) void vae_attn_flash_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ vt,
                                                             const float* __restrict__ vbias, bf16* __restrict__ o, int T) {
    constexpr int NQ = kVaeAttnQueryTiles;
    constexpr int CW = C / 4;     // channels per wave
    constexpr int KS = CW / 16;   // k-steps of the score product
    constexpr int CT = CW / 32;   // 32-channel tiles of O^T
    __shared__ f32x4 sS[4 * NQ * 8 * 64];   // [wave][query tile][subtile * 4 + reg / 4][lane]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, hh = lane >> 5;
    const int b = blockIdx.y, q0 = blockIdx.x * (32 * NQ);
    const size_t row0 = (size_t)b * T;

    bf16x8 qf[NQ][KS];
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
        const bf16* qp = q + (row0 + q0 + nq * 32 + r) * C + wave * CW + hh * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[nq][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
    }
    const int pr = (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1);
    const bf16* kp = k + (row0 + pr) * C + wave * CW + hh * 8;
    const bf16* vp = vt + ((size_t)b * C + wave * CW + r) * T + hh * 8;

    const float scale = (C == 256 ? 0.0625f : 0.044194173824159220f) * 1.4426950408889634f;   // C^-0.5 * log2(e)
    f32x16 ot[NQ][CT];
    float m[NQ], lsum[NQ];
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
        m[nq] = -INFINITY;
        lsum[nq] = 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int e = 0; e < 16; ++e) ot[nq][ct][e] = 0.f;
    }
    const int nkt = T >> 6;
#pragma unroll 1
    for (int kt = 0; kt < nkt; ++kt) {
        // ---- this wave's share of S^T: [2 x 32 keys][NQ x 32 queries] over its channel slice
        f32x16 acc[NQ][2];
#pragma unroll
        for (int st = 0; st < 2; ++st) {
#pragma unroll
            for (int nq = 0; nq < NQ; ++nq)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[nq][st][e] = 0.f;
            const bf16* kr = kp + (size_t)(kt * 64 + st * 32) * C;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kr + ks * 16);
#pragma unroll
                for (int nq = 0; nq < NQ; ++nq) acc[nq][st] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[nq][ks], acc[nq][st], 0, 0, 0);
            }
        }
        // ---- all four shares through LDS
        if (kt) __syncthreads();   // the previous tile's reads are done
#pragma unroll
        for (int nq = 0; nq < NQ; ++nq)
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[nq][g >> 2][4 * (g & 3) + e];
                sS[((wave * NQ + nq) * 8 + g) * 64 + lane] = v;
            }
        __syncthreads();
#pragma unroll
        for (int nq = 0; nq < NQ; ++nq) {
            float tm = -INFINITY;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                f32x4 v = sS[(nq * 8 + g) * 64 + lane];
#pragma unroll
                for (int w = 1; w < 4; ++w) v += sS[((w * NQ + nq) * 8 + g) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float sc = v[e] * scale;
                    acc[nq][g >> 2][4 * (g & 3) + e] = sc;
                    tm = fmaxf(tm, sc);
                }
            }
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            const float mn = fmaxf(m[nq], tm);
            const float alpha = __builtin_amdgcn_exp2f(m[nq] - mn);   // first tile: exp2(-inf) = 0 on a zero state
            m[nq] = mn;
            lsum[nq] *= alpha;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int e = 0; e < 16; ++e) ot[nq][ct][e] *= alpha;
        }
        // ---- p = exp2(s - m); O^T[channel][query] += V^T[channel][key] P^T[key][query]
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                bf16x8 pf[NQ];
#pragma unroll
                for (int nq = 0; nq < NQ; ++nq)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float p = __builtin_amdgcn_exp2f(acc[nq][st][8 * s2 + j] - m[nq]);
                        lsum[nq] += p;
                        pf[nq][j] = f2bf(p);
                    }
                const bf16* vk = vp + kt * 64 + st * 32 + s2 * 16;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vk + (size_t)ct * 32 * T);
#pragma unroll
                    for (int nq = 0; nq < NQ; ++nq) ot[nq][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[nq], ot[nq][ct], 0, 0, 0);
                }
            }
    }
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
        const float l = lsum[nq] + __shfl_xor(lsum[nq], 32, 64);
        const float inv = 1.f / l;
        bf16* orow = o + (row0 + q0 + nq * 32 + r) * C + wave * CW;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = ct * 32 + 8 * g + 4 * hh;
                f32x4 bias = {0.f, 0.f, 0.f, 0.f};
                if (vbias) bias = *reinterpret_cast<const f32x4*>(vbias + wave * CW + c);
                U2BF4 ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov.e[e] = f2bf(ot[nq][ct][4 * g + e] * inv + bias[e]);
                *reinterpret_cast<uint2*>(orow + c) = ov.u;
            }
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int vae_attn_flash_launch(const bf16* q, const bf16* k, const bf16* vt, const float* vbias, bf16* o, int B, int T, int C, hipStream_t stream) {
    if (!vae_attn_flash_supports(C)) return set_error(GL_ERR_UNSUPPORTED, "vae_attn_flash: C=%d channels (the kernel is built for 256 and 512)", C);
    if (B <= 0 || T <= 0 || T % kVaeAttnKeyTile) return set_error(GL_ERR_UNSUPPORTED, "vae_attn_flash: B=%d T=%d (T a positive multiple of 64)", B, T);
    if (B > 65535) return set_error(GL_ERR_UNSUPPORTED, "vae_attn_flash: B=%d images exceed the grid's 65535", B);
    if (!aligned16(q) || !aligned16(k) || !aligned16(vt) || !aligned16(o) || !aligned16(vbias))
        return set_error(GL_ERR_ARG, "vae_attn_flash: q, k, v^T, bias and out must be 16-byte aligned");
    const dim3 grid(T / (32 * kVaeAttnQueryTiles), B);
    if (C == 256) hipLaunchKernelGGL(vae_attn_flash_kernel<256>, grid, dim3(256), 0, stream, q, k, vt, vbias, o, T);
    else hipLaunchKernelGGL(vae_attn_flash_kernel<512>, grid, dim3(256), 0, stream, q, k, vt, vbias, o, T);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// ------------------------------------------------------------------------------------------------ v rows -> v^T
// 64 tokens x 64 channels per workgroup through LDS: 16-byte loads along the channels, 16-byte stores along the tokens.
__global__ __launch_bounds__(256) void vae_attn_transpose_kernel(const bf16* __restrict__ v, bf16* __restrict__ vt, int T, int C) {
    __shared__ __attribute__((aligned(16))) bf16 tile[64][72];   // rows 144 B apart
    const int t0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    for (int i = threadIdx.x; i < 512; i += 256) {
        const int t = i >> 3, ch = (i & 7) * 8;
        *reinterpret_cast<uint4*>(&tile[t][ch]) = *reinterpret_cast<const uint4*>(v + ((size_t)b * T + t0 + t) * C + c0 + ch);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 256) {
        const int c = i >> 3, tk = (i & 7) * 8;
        U4BF8 u;
#pragma unroll
        for (int j = 0; j < 8; ++j) u.e[j] = tile[tk + j][c];
        *reinterpret_cast<uint4*>(vt + ((size_t)b * C + c0 + c) * T + t0 + tk) = u.u;
    }
}

int vae_attn_transpose_launch(const bf16* v, bf16* vt, int B, int T, int C, hipStream_t stream) {
    if (B <= 0 || B > 65535 || T <= 0 || T % 64 || C <= 0 || C % 64 || C / 64 > 65535)
        return set_error(GL_ERR_UNSUPPORTED, "vae_attn_transpose: B=%d T=%d C=%d (T and C positive multiples of 64)", B, T, C);
    if (!aligned16(v) || !aligned16(vt)) return set_error(GL_ERR_ARG, "vae_attn_transpose: v and v^T must be 16-byte aligned");
    hipLaunchKernelGGL(vae_attn_transpose_kernel, dim3(T / 64, C / 64, B), dim3(256), 0, stream, v, vt, T, C);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
