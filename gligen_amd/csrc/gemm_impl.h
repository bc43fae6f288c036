// What the GEMM's translation units share and nobody else sees (gemm.h is the interface the engine sees, gemm_plan.h the planner's):
//   gemm_basic.hip  gemm_glds_kernel, gemm_p_kernel
//   gemm_u.hip      gemm_u_kernel
//   gemm_halo.hip   conv_halo_kernel
//   gemm_wide.hip   gemm_wide_kernel
//   gemm_conv8.hip  conv8_kernel
//   gemm.hip        execute() for a GemmPlan, splitk_reduce_kernel, the on-device tuner, gemm_launch
// Here: the epilogue and LDS-read helpers more than one unit inlines, the two LDS-DMA macros, the host-side Launch and the entry
// function of every kernel unit. The build has no relocatable device code: a kernel is launched only from the unit that defines it,
// so this header holds no __global__ function and no __device__ variable, and no unit includes another unit's kernels.
#pragma once
#include <type_traits>

#include "gemm_plan.h"

namespace gl {

// tokens are permuted inside groups of 16 so that the attention kernel's P^T fragment (taken
// straight from MFMA accumulators) lines up with one ds_read_b128 of V^T: [0-3,8-11,4-7,12-15].
// p32 (Epilogue::vt_perm32, attn3_kernel): groups of 32, quads in the order [0,2,4,6,1,3,5,7] -- the four 8-key k-slot groups of a
// v_mfma_f32_16x16x32 B operand assembled from a 32x32 S^T accumulator by v_permlane16_swap (attention.hip).
__device__ __forceinline__ int perm_tok4(int t0, int p32 = 0) {
    if (p32) {
        const int g = (t0 >> 2) & 7;
        return (t0 & ~31) | ((((g & 1) << 2) | (g >> 1)) << 2);
    }
    int g = (t0 >> 2) & 3;
    int gp = ((g & 1) << 1) | (g >> 1);
    return (t0 & ~15) | (gp << 2);
}

__device__ __forceinline__ void store_bf16x4(bf16* dst, const float v[4]) {
    U2BF4 o;
    o.e[0] = f2bf(v[0]);
    o.e[1] = f2bf(v[1]);
    o.e[2] = f2bf(v[2]);
    o.e[3] = f2bf(v[3]);
    *reinterpret_cast<uint2*>(dst) = o.u;
}

// m / E.rows_per_b through the multiplier gemm_launch prepared (round-up method: shift = ceil(log2 d), magic = floor(2^32 (2^shift - d) / d) + 1).
// A per-lane "/" by a kernel argument makes hipcc build the reciprocal in VGPRs in front of the K loop and keep it there.
__device__ __forceinline__ int div_rpb(const Epilogue& E, int m) {
    return (int)((__umulhi((unsigned)m, E.rpb_magic) + (unsigned)m) >> E.rpb_shift);
}

__device__ __forceinline__ void epi_finish4(const Epilogue& E, int m, int n0, float v[4]) {
    if (E.bias) {
        float4 b = *reinterpret_cast<const float4*>(E.bias + n0);
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
    if (E.bias2) {
        int bb = div_rpb(E, m);
        float4 b = *reinterpret_cast<const float4*>(E.bias2 + (size_t)bb * E.bias2_ld + n0);
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
    if (E.act == ACT_SILU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = silu_f(v[i]);
    } else if (E.act == ACT_GELU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = gelu_erf_f(v[i]);
    } else if (E.act == ACT_QUICK_GELU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = quick_gelu_f(v[i]);
    }
    switch (E.mode) {
        case EPI_ROWMAJOR: {
            if (E.remap_in) m = (m / E.remap_in) * E.remap_out + (m % E.remap_in) + E.remap_off;
            if (E.res) {
                U2BF4 r;
                r.u = *reinterpret_cast<const uint2*>(E.res + (size_t)m * E.ldres + n0);
                float g = E.gate ? *E.gate : 1.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = bf2f(r.e[i]) + g * v[i];
            }
            if (E.out_f32) {
                float4 o = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(E.out) + (size_t)m * E.ldo + n0) = o;
            } else {
                store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + n0, v);
            }
            break;
        }
        case EPI_QKV_HEADS:
        case EPI_QK_HEADS: {
            int which = n0 >= E.C;
            int c = n0 - which * E.C;
            int h = c / E.d;
            int dd = c - h * E.d;
            int b = m / E.T;
            int t = m - b * E.T + E.tok_off;
            int tp = which ? E.Tpad_k : E.Tpad_q;
            bf16* base = which ? E.k : E.q;
            const size_t off = (which || E.q_tiled) ? ktile_off((size_t)(b * E.H + h), tp, t, dd, E.DP) : ((size_t)(b * E.H + h) * tp + t) * E.DP + dd;
            store_bf16x4(base + off, v);
            break;
        }
        case EPI_VT_HEADS: {  // m = feature, n0 = first of 4 consecutive tokens
            int h = m / E.d;
            int dd = m - h * E.d;
            int b = n0 / E.T;
            int t0 = n0 - b * E.T + E.tok_off;
            bf16* base = reinterpret_cast<bf16*>(E.out);
            store_bf16x4(base + ((size_t)(b * E.H + h) * E.DPV + dd) * E.Tpad_k + perm_tok4(t0, E.vt_perm32), v);
            break;
        }
        case EPI_NCHW_F32: {
            int b = div_rpb(E, m);
            int pix = m - b * E.rows_per_b;
            float* o = reinterpret_cast<float*>(E.out);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (n0 + i < E.n_real) o[((size_t)b * E.n_real + n0 + i) * E.rows_per_b + pix] = v[i];
            break;
        }
    }
}

// Store half of epi_finish4 for epilogues that load bias / residual for ALL their fragments up front
// (v already holds bias and residual; for EPI_ROWMAJOR m is the remapped output row). A wave's vmcnt is one
// in-order counter for loads and stores, so a load issued after a store cannot be waited for without
// waiting for that store: an epilogue that alternates {load bias/residual, store} per fragment pays one
// memory round trip per fragment (measured: 18 of the 27 us of a 32768 x 320 x 320 GEMM).
// WITH_GELU = false: the conv instantiations (never followed by a GELU) keep the erf code out of their register allocation
template <bool WITH_GELU = true>
__device__ __forceinline__ void epi_store4(const Epilogue& E, int m, int n0, float v[4]) {
    if (E.act == ACT_SILU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = silu_f(v[i]);
    } else if (WITH_GELU && E.act == ACT_GELU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = gelu_erf_f(v[i]);
    } else if (WITH_GELU && E.act == ACT_QUICK_GELU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = quick_gelu_f(v[i]);
    }
    switch (E.mode) {
        case EPI_ROWMAJOR: {
            if (E.out_f32) {
                float4 o = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(E.out) + (size_t)m * E.ldo + n0) = o;
            } else {
                store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + n0, v);
            }
            break;
        }
        case EPI_QKV_HEADS:
        case EPI_QK_HEADS: {
            int which = n0 >= E.C;
            int c = n0 - which * E.C;
            int h = c / E.d;
            int dd = c - h * E.d;
            int b = m / E.T;
            int t = m - b * E.T + E.tok_off;
            int tp = which ? E.Tpad_k : E.Tpad_q;
            bf16* base = which ? E.k : E.q;
            const size_t off = (which || E.q_tiled) ? ktile_off((size_t)(b * E.H + h), tp, t, dd, E.DP) : ((size_t)(b * E.H + h) * tp + t) * E.DP + dd;
            store_bf16x4(base + off, v);
            break;
        }
        case EPI_VT_HEADS: {  // m = feature, n0 = first of 4 consecutive tokens
            int h = m / E.d;
            int dd = m - h * E.d;
            int b = n0 / E.T;
            int t0 = n0 - b * E.T + E.tok_off;
            bf16* base = reinterpret_cast<bf16*>(E.out);
            store_bf16x4(base + ((size_t)(b * E.H + h) * E.DPV + dd) * E.Tpad_k + perm_tok4(t0, E.vt_perm32), v);
            break;
        }
        case EPI_NCHW_F32: {
            int b = div_rpb(E, m);
            int pix = m - b * E.rows_per_b;
            float* o = reinterpret_cast<float*>(E.out);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (n0 + i < E.n_real) o[((size_t)b * E.n_real + n0 + i) * E.rows_per_b + pix] = v[i];
            break;
        }
    }
}

// GEGLU: weight/bias rows are pre-packed so that inside every 32-row tile the accumulator
// groups alternate value,gate,value,gate for the same 4 output features (see pack_geglu_rows).
__device__ __forceinline__ void epi_geglu4(const Epilogue& E, int m, int nv0, float val[4], float gate[4]) {
    if (E.bias) {
        float4 bv = *reinterpret_cast<const float4*>(E.bias + nv0);
        float4 bg = *reinterpret_cast<const float4*>(E.bias + nv0 + 8);
        val[0] += bv.x; val[1] += bv.y; val[2] += bv.z; val[3] += bv.w;
        gate[0] += bg.x; gate[1] += bg.y; gate[2] += bg.z; gate[3] += bg.w;
    }
    int j0 = (nv0 >> 5) * 16 + ((nv0 & 31) >> 4) * 8 + (nv0 & 7);
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = val[i] * gelu_erf_f(gate[i]);
    store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + j0, o);
}

// Accumulator -> memory for one wave: lane (frow, fhalf) holds output row m0 + 32 i and, per 32x32
// tile, four groups of 4 consecutive columns starting at n0 + 32 j + 8 q.
template <int TM, int TN>
__device__ __forceinline__ void gemm_epilogue(f32x16 (&acc)[TM][TN], const Epilogue& E, int M, int N, int m0, int n0w,
                                              float* __restrict__ ws) {
    const bool split = gridDim.z > 1;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + i * 32;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nb = n0w + j * 32;
            if (split) {
                float* dst = ws + ((size_t)blockIdx.z * M + m) * N;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int n0 = nb + 8 * q;
                    if (n0 < N)
                        *reinterpret_cast<float4*>(dst + n0) =
                            make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
                }
            } else if (E.act == ACT_GEGLU) {
#pragma unroll
                for (int qq = 0; qq < 2; ++qq) {
                    int nv0 = nb + 16 * qq;
                    if (nv0 < N) {
                        float val[4], gate[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            val[e] = acc[i][j][8 * qq + e];
                            gate[e] = acc[i][j][8 * qq + 4 + e];
                        }
                        epi_geglu4(E, m, nv0, val, gate);
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int n0 = nb + 8 * q;
                    if (n0 < N) {
                        float v[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * q + e];
                        epi_finish4(E, m, n0, v);
                    }
                }
            }
        }
    }
}

#define GL_GLDS16(gsrc, ldst)                                                                      \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc),       \
                                     (__attribute__((address_space(3))) void*)(ldst), 16, 0, 0)

// GEGLU epilogue for the 16x16-tile kernel: packed weight rows come in groups of 32 = 16 value
// features followed by the 16 matching gate features (pack_geglu layout 1), so accumulator tile
// 2g holds values and tile 2g+1 gates for the same (row, 4 features) in the same lane.
__device__ __forceinline__ void epi_geglu4_t16(const Epilogue& E, int m, int nv0, float val[4], float gate[4]) {
    if (E.bias) {
        float4 bv = *reinterpret_cast<const float4*>(E.bias + nv0);
        float4 bg = *reinterpret_cast<const float4*>(E.bias + nv0 + 16);
        val[0] += bv.x; val[1] += bv.y; val[2] += bv.z; val[3] += bv.w;
        gate[0] += bg.x; gate[1] += bg.y; gate[2] += bg.z; gate[3] += bg.w;
    }
    const int j0 = (nv0 >> 5) * 16 + (nv0 & 15);
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = val[i] * gelu_erf_f(gate[i]);
    store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + j0, o);
}

// LDS fragment reads in inline asm. hipcc cannot tell that a ds_read of one ring slot does not alias the LDS-DMA
// just issued into another, so with compiler-visible LDS loads it puts s_waitcnt vmcnt(0) in front of the first
// ds_read after every DMA issue: the "prefetch" is drained before the multiply it should run under (seen in the
// ISA, and in the ablation as DMA time + MFMA time adding up exactly). Asm reads are invisible to that pass; their
// completion is waited for by hand (counted lgkmcnt, LDS returns in order) and the consumers are pinned below the
// wait through "+v" operands (an MFMA is register-only, a "memory" clobber does not order it).
template <int OFF>
__device__ __forceinline__ void lds_rd16(bf16x8& d, unsigned addr) {
    // no "memory" clobber: an asm that "may touch memory" makes the waitcnt pass drain the pending DMA exactly like a
    // visible LDS load would; volatile keeps it ordered against the barrier, the DMA issues and the other asm statements
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
template <int N, int STRIDE, int I = 0>
__device__ __forceinline__ void lds_rd16_n(bf16x8 (&d)[N], unsigned addr) {
    if constexpr (I < N) {
        lds_rd16<I * STRIDE>(d[I], addr);
        lds_rd16_n<N, STRIDE, I + 1>(d, addr);
    }
}
// "this value has arrived": an empty asm that reads (and re-defines) a loaded value makes hipcc place the wait for it HERE, once,
// instead of in every guarded block that uses it later
__device__ __forceinline__ void epi_ready(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
template <int N>
__device__ __forceinline__ void pin_regs(bf16x8 (&d)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(d[i]));
}

#define GL_BLDS16(rsrc, ldst, voff, soff)                                                                   \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(ldst), 16, \
                                             (int)(voff), (int)(soff), 0, 0)

// (mean, rstd) of row m from the producer's partial sums (Epilogue::ln_stats), fixed summation order
__device__ __forceinline__ float2 ln_row_stats(const Epilogue& E, int m) {
    float s = 0.f, q = 0.f;
    for (int nb = 0; nb < E.ln_nb; ++nb) {
        const float2 v = E.ln_stats[(size_t)m * E.ln_ld + nb];
        s += v.x; q += v.y;
    }
    const float mean = s * E.ln_inv_c;
    const float var = fmaxf(q * E.ln_inv_c - mean * mean, 0.f);
    return make_float2(mean, rsqrtf(var + E.ln_eps));
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side. The arguments every GEMM kernel starts with, and the stream it runs on
struct Launch {
    const AOperand& A; const bf16* W; int M, N, K; const Epilogue& E; float* ws;
    hipStream_t stream;
    template <auto KFN, class... Tail> int run(dim3 grid, int block, size_t lds, const Tail&... tail) const {
        return launch_lds<KFN>(grid, dim3(block), lds, stream, A, W, M, N, K, E, ws, tail...);
    }
};

// One entry function per kernel unit: it owns the unit's instantiation table, i.e. launches the kernel instantiated for the plan's
// (family, tm, tn, amode, qkv, gn) with that instantiation's LDS size, or fails with gemm_unknown_tile()
int gemm_exec_basic(const Launch& l, const GemmPlan& p);   // GEMM_GLDS, GEMM_P
int gemm_exec_u(const Launch& l, const GemmPlan& p);
int gemm_exec_halo(const Launch& l, const GemmPlan& p);
int gemm_exec_wide(const Launch& l, const GemmPlan& p);
int gemm_exec_conv8(const Launch& l, const GemmPlan& p);
inline int gemm_unknown_tile() { return set_error(GL_ERR_UNSUPPORTED, "gemm: unknown tile candidate"); }

}  // namespace gl
