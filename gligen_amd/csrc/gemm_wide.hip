// gemm_wide_kernel: 256-row tiles for the long-K, wide-N row GEMMs. Its header comment below is the description of this unit.
#include "gemm_impl.h"

namespace gl {

// ---------------------------------------------------------------------------------------------------------------------------
// "Wide" GEMM (A_ROWS, round 2): the geometry of conv_halo_kernel (gemm_halo.hip) for plain row-major activations. 8 waves, ONE workgroup per CU,
// 256 x (TN*32) tile, two LDS stages of (256 + BN) x 128 B, one barrier per K tile:
//     vmcnt(0) -> barrier -> DMA of the next K tile into the other stage -> all fragment reads -> MFMAs
// (hipcc runs the second K step's MFMAs behind the next barrier, as in the halo kernel). Against gemm_u_kernel's 128-row tiles
// the weight tile is fetched once per 256 rows: 52 KB of LDS-DMA per 256x160x64 multiply instead of 72 KB. For the long-K,
// wide-N problems (FF-out, the GEGLU projections of the 32x32 / 16x16 levels); whole tiles only (M % 256 == 0, N % BN == 0).
// LDS ring depth of the wide kernel. 3 (two K tiles in flight, counted vmcnt wait) was built and measured: 3-5 % SLOWER than 2 on
// every GEGLU projection (profiles/r3/wide_ring_kbench.txt) -- the K loop is not waiting for the fabric, it is sharing the LDS
// port between 128 KB of fragment reads and 48 KB of DMA writes per tile next to 0.43 us of MFMAs. tools/build_variant.sh NAME
// -DGL_WIDE_NST=3 rebuilds that arm.
#ifndef GL_WIDE_NST
#define GL_WIDE_NST 2
#endif
template <int TN>
__global__ void __launch_bounds__(512, 1)
gemm_wide_kernel(AOperand A, const bf16* __restrict__ W, int M, int N, int K, Epilogue E, float* __restrict__ ws, WideDesc wd) {
    constexpr int TM = 4;
    constexpr int BM = 256;
    constexpr int BN = TN * 32;
    constexpr int XP = BM / 64;                 // activation DMA passes (64 rows each)
    constexpr int WP = (BN + 63) / 64;          // weight DMA passes; the last one is partial when BN % 64 != 0
    constexpr int WREM = BN % 64;
    constexpr int STAGE = (BM + BN) * 128;
    constexpr int NST = GL_WIDE_NST;            // LDS ring depth: NST - 1 K tiles in flight behind the one being multiplied

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1;
    const int wn = wave & 1;
    const int l15 = lane & 15;
    const int q = lane >> 4;
    const int r0 = t >> 3;                                          // row inside a DMA pass
    const unsigned chb = (((t & 7) ^ ((r0 >> 1) & 7)) * 16);        // byte offset of this lane's (swizzled) source chunk
    const int nk = K >> 6;

    const __amdgpu_buffer_rsrc_t ra0 = __builtin_amdgcn_make_buffer_rsrc((void*)A.p0, 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra1 = __builtin_amdgcn_make_buffer_rsrc((void*)(A.p1 ? A.p1 : A.p0), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, 0x80000000u, 0x00020000);

    const int foff0 = l15 * 128 + (((q) ^ (l15 >> 1)) << 4);
    const int foff1 = l15 * 128 + (((q + 4) ^ (l15 >> 1)) << 4);
    const int xrow0 = wm * TM * 16 * 128;
    const int wrow0 = BM * 128 + wn * TN * 16 * 128;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

    // ---- work item state
    int m0 = 0, c_tn = 0, c_z = 0;
    unsigned vx0 = 0, vx1 = 0, vw0 = 0;   // byte offsets of this lane's chunk of row (tile's first row + r0) in p0 / p1 / W; pass i adds 64 rows
    auto setup = [&](int item_) {
        int item = item_;
        if (wd.xcd) {
            // block b sits on XCD b % 8 and the grid is a multiple of 8, so item & 7 is this workgroup's XCD: give every XCD a
            // contiguous range of the (tile_m, tile_n) order -- the 32 workgroups of an XCD then walk the column tiles of the same
            // one or two 256-row stripes together and the stripe crosses the fabric once, not once per XCD
            const int q = wd.n_items >> 3, r = wd.n_items & 7, xcd = item & 7, idx = item >> 3;
            item = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        }
        const int tile = item / wd.splits;
        c_z = item - tile * wd.splits;
        const int tm = tile / wd.tiles_n;
        c_tn = tile - tm * wd.tiles_n;
        m0 = tm * BM;
        vx0 = (unsigned)((m0 + r0) * A.ld0) * 2u + chb;
        vx1 = (unsigned)((m0 + r0) * A.ld1) * 2u + chb;
        vw0 = (unsigned)((c_tn * BN + r0) * K) * 2u + chb;
    };
    auto issue = [&](int kt_, int st_) {     // K tile kt into stage st
        const int kt = __builtin_amdgcn_readfirstlane(kt_);
        const int st = __builtin_amdgcn_readfirstlane(st_);
        const int k0 = kt << 6;
        const bool first = k0 < A.C0;
        unsigned char* xs = smem + st * STAGE + wave * 1024;
        if (first) {
#pragma unroll
            for (int i = 0; i < XP; ++i) GL_BLDS16(ra0, xs + i * 64 * 128, vx0, k0 * 2 + i * 64 * A.ld0 * 2);
        } else {
#pragma unroll
            for (int i = 0; i < XP; ++i) GL_BLDS16(ra1, xs + i * 64 * 128, vx1, (k0 - A.C0) * 2 + i * 64 * A.ld1 * 2);
        }
        unsigned char* wsm = xs + BM * 128;
#pragma unroll
        for (int i = 0; i < WP; ++i) {
            if (WREM && i == WP - 1 && wave >= WREM / 8) continue;   // wave-uniform
            GL_BLDS16(rw, wsm + i * 64 * 128, vw0, k0 * 2 + i * 64 * K * 2);
        }
    };

    f32x4 acc[TM][TN];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // K step 1 of a tile is multiplied one tile late: its MFMAs go out right behind the next barrier and DMA issue, and the next
    // tile's fragment reads fly under them (the order hipcc finds by itself in the unrolled halo kernel; this loop is not unrolled)
    bf16x8 xb[TM], wb[TN];
    auto step1 = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j], xb[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto compute = [&](int stg, bool pending) {
        const unsigned st = lds0 + stg * STAGE;
        const unsigned ax0 = st + xrow0 + foff0, ax1 = st + xrow0 + foff1;
        const unsigned aw0 = st + wrow0 + foff0, aw1 = st + wrow0 + foff1;
        bf16x8 xa[TM], wa[TN];
        if (pending) step1();
        lds_rd16_n<TM, 2048>(xa, ax0);
        lds_rd16_n<TN, 2048>(wa, aw0);
        lds_rd16_n<TM, 2048>(xb, ax1);
        lds_rd16_n<TN, 2048>(wb, aw1);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(TM + TN));  // the k-step 0 fragments have returned
        pin_regs(xa);
        pin_regs(wa);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[j], xa[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);   // (keeps K step 0's MFMAs in front of the wait below: they only need the first TM + TN reads)
        // every fragment read of this stage has RETURNED before the wave reaches the next barrier: behind that barrier the stage is
        // overwritten by DMA, and K step 1's fragments are consumed (the asm reads are invisible to hipcc's own lgkmcnt tracking)
        asm volatile("s_waitcnt lgkmcnt(0)");
        pin_regs(xb);
        pin_regs(wb);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto finish = [&]() {   // the item's last K step 1
        asm volatile("s_waitcnt lgkmcnt(0)");
        pin_regs(xb);
        pin_regs(wb);
        __builtin_amdgcn_sched_barrier(0);
        step1();
    };

    // lst: (mean, rstd) of the item's 256 rows in LDS when the LayerNorm in front of this GEMM is folded into it (gemm.h)
    auto epilogue = [&](const float2* lst) {
        const int mrow = m0 + wm * TM * 16 + l15;
        const int ncol = c_tn * BN + wn * TN * 16 + q * 4;
        if (wd.splits > 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    *reinterpret_cast<float4*>(ws + ((size_t)c_z * M + m) * N + ncol + j * 16) =
                        make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            }
            return;
        }
        if constexpr (TN % 2 == 0) {
            if (E.act == ACT_GEGLU) {   // geglu16 weight layout: fragment 2 jj = 16 value features, 2 jj + 1 = their gates
                float4 bv[TN / 2], bg[TN / 2];
#pragma unroll
                for (int jj = 0; jj < TN / 2; ++jj) {
                    bv[jj] = bg[jj] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (E.bias) {
                        bv[jj] = *reinterpret_cast<const float4*>(E.bias + ncol + jj * 32);
                        bg[jj] = *reinterpret_cast<const float4*>(E.bias + ncol + jj * 32 + 16);
                    }
                }
                if (lst) {   // folded LayerNorm: acc <- rstd (acc - mean csum), in place, before bias and GEGLU
#pragma unroll
                    for (int jj = 0; jj < TN / 2; ++jj) {
                        const float4 cv = *reinterpret_cast<const float4*>(E.ln_csum + ncol + jj * 32);
                        const float4 cg = *reinterpret_cast<const float4*>(E.ln_csum + ncol + jj * 32 + 16);
#pragma unroll
                        for (int i = 0; i < TM; ++i) {
                            const float2 st = lst[wm * TM * 16 + i * 16 + l15];
                            acc[i][2 * jj][0] = st.y * (acc[i][2 * jj][0] - st.x * cv.x); acc[i][2 * jj][1] = st.y * (acc[i][2 * jj][1] - st.x * cv.y);
                            acc[i][2 * jj][2] = st.y * (acc[i][2 * jj][2] - st.x * cv.z); acc[i][2 * jj][3] = st.y * (acc[i][2 * jj][3] - st.x * cv.w);
                            acc[i][2 * jj + 1][0] = st.y * (acc[i][2 * jj + 1][0] - st.x * cg.x); acc[i][2 * jj + 1][1] = st.y * (acc[i][2 * jj + 1][1] - st.x * cg.y);
                            acc[i][2 * jj + 1][2] = st.y * (acc[i][2 * jj + 1][2] - st.x * cg.z); acc[i][2 * jj + 1][3] = st.y * (acc[i][2 * jj + 1][3] - st.x * cg.w);
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int m = mrow + i * 16;
#pragma unroll
                    for (int jj = 0; jj < TN / 2; ++jj) {
                        const int n0 = ncol + jj * 32;
                        const f32x2 r0 = geglu2(f32x2{acc[i][2 * jj][0] + bv[jj].x, acc[i][2 * jj][1] + bv[jj].y},
                                                f32x2{acc[i][2 * jj + 1][0] + bg[jj].x, acc[i][2 * jj + 1][1] + bg[jj].y});
                        const f32x2 r1 = geglu2(f32x2{acc[i][2 * jj][2] + bv[jj].z, acc[i][2 * jj][3] + bv[jj].w},
                                                f32x2{acc[i][2 * jj + 1][2] + bg[jj].z, acc[i][2 * jj + 1][3] + bg[jj].w});
                        float o[4] = {r0.x, r0.y, r1.x, r1.y};
                        const int j0 = (n0 >> 5) * 16 + (n0 & 15);
                        store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + j0, o);
                    }
                }
                return;
            }
        }
        float4 bj[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            bj[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (E.bias) bj[j] = *reinterpret_cast<const float4*>(E.bias + ncol + j * 16);
        }
        const float g = (E.res && E.gate) ? *E.gate : 1.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = mrow + i * 16;
            uint2 rs[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                rs[j] = make_uint2(0, 0);
                if (E.res) rs[j] = *reinterpret_cast<const uint2*>(E.res + (size_t)m * E.ldres + ncol + j * 16);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n0 = ncol + j * 16;
                float v[4] = {acc[i][j][0] + bj[j].x, acc[i][j][1] + bj[j].y, acc[i][j][2] + bj[j].z, acc[i][j][3] + bj[j].w};
                if (E.act == ACT_SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
                }
                if (E.res) {
                    U2BF4 r;
                    r.u = rs[j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = bf2f(r.e[e]) + g * v[e];
                }
                if (E.out_f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(E.out) + (size_t)m * E.ldo + n0) = make_float4(v[0], v[1], v[2], v[3]);
                else store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + n0, v);
            }
        }
    };

    // ---- persistent loop over work items
    int item = blockIdx.x;
    if (item >= wd.n_items) return;
    int stg = 0;
    int kt = 0, kt_end = 0;
    // folded LayerNorm: this thread's share of the partial sums of row t >> 1 of the item whose K loop starts (the loads fly under
    // it); the finished item's pair is handed to its epilogue before the next item's fetch overwrites it
    // (the loaded pairs stay in registers untouched until the epilogue: an add right behind the load would make hipcc wait for it there)
    constexpr int LNV = 5;
    float2 ln_v[LNV];
    float ln_s = 0.f, ln_q = 0.f;
    auto ring_next = [](int s_) { return NST == 2 ? s_ ^ 1 : (s_ == NST - 1 ? 0 : s_ + 1); };
    // DMA instructions one K tile costs this wave (the wait below leaves exactly one tile in flight)
    const bool w_short = WREM && wave >= WREM / 8;
    auto begin_item = [&](int it) {
        setup(it);
        kt = c_z * wd.kt_per_split;
        kt_end = min(nk, kt + wd.kt_per_split);
        issue(kt, stg);
        if (NST == 3 && kt + 1 < kt_end) issue(kt + 1, ring_next(stg));
        if (E.ln_stats) {
            const float2* src = E.ln_stats + (size_t)(m0 + (t >> 1)) * E.ln_ld;
            ln_s = ln_q = 0.f;
#pragma unroll
            for (int i = 0; i < LNV; ++i) {
                const int nb = (t & 1) + 2 * i;
                ln_v[i] = make_float2(0.f, 0.f);
                if (nb < E.ln_nb) ln_v[i] = src[nb];
            }
            for (int nb = (t & 1) + 2 * LNV; nb < E.ln_nb; nb += 2) {   // (more than 10 column blocks: C = 1280)
                const float2 v = src[nb];
                ln_s += v.x; ln_q += v.y;
            }
        }
    };
    begin_item(item);
    zero_acc();
    // one K tile: wait for it, barrier, send the tile NST - 1 ahead, multiply. An item's first tile is its own copy of the body
    // (first = true): it drains the counter through the builtin -- the previous item's epilogue stores sit in the same counter as
    // the DMA (loads and stores do not retire in order with each other), and hipcc then KNOWS that nothing is pending, the
    // statistics prefetch of begin_item included; behind an asm wait its scoreboard would carry those loads around the K loop and
    // drain in front of every register copy it places on the back edge. The other tiles leave the tile behind them in flight.
    int stg_done = 0;
    auto tile = [&](auto first_c) {
        constexpr bool first = decltype(first_c)::value;
        stg = __builtin_amdgcn_readfirstlane(stg);
        kt = __builtin_amdgcn_readfirstlane(kt);
        kt_end = __builtin_amdgcn_readfirstlane(kt_end);
        if (NST == 3 && !first && kt + 1 < kt_end) {
            if (w_short) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(XP + WP - 1) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(XP + WP) : "memory");
        } else {
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (NST == 3) { if (kt + 2 < kt_end) issue(kt + 2, ring_next(ring_next(stg))); }
        else if (kt + 1 < kt_end) issue(kt + 1, stg ^ 1);
        compute(stg, !first);
        stg_done = stg;
        stg = ring_next(stg);
        ++kt;
    };
    for (;;) {
        tile(std::true_type{});
        while (kt < kt_end) tile(std::false_type{});
        finish();
        // item done: start the next item's first tile (into the stage the last tile was not read from), then store
        const int done_m0 = m0, done_tn = c_tn, done_z = c_z;
        float done_s = ln_s, done_q = ln_q;
#pragma unroll
        for (int i = 0; i < LNV; ++i) { done_s += ln_v[i].x; done_q += ln_v[i].y; }
        item += gridDim.x;
        const bool more = item < wd.n_items;
        if (more) begin_item(item);
        {
            const int nm0 = m0, ntn = c_tn, nz = c_z;
            m0 = done_m0; c_tn = done_tn; c_z = done_z;
            const float2* lst = nullptr;
            if (E.ln_stats && wd.splits == 1) {
                // folded LayerNorm: (mean, rstd) of the finished item's 256 rows from the producer's partial sums, into the stage the
                // last K tile was read from (free until the DMA behind the next barrier); two threads per row, fixed summation order
                float2* l = reinterpret_cast<float2*>(smem + stg_done * STAGE);
                __builtin_amdgcn_s_barrier();          // every wave is done with that stage's fragments
                const int row = t >> 1, part = t & 1;
                float s = done_s, qq = done_q;
                s += __shfl_xor(s, 1, 64); qq += __shfl_xor(qq, 1, 64);
                if (part == 0) {
                    const float mean = s * E.ln_inv_c;
                    const float var = fmaxf(qq * E.ln_inv_c - mean * mean, 0.f);
                    l[row] = make_float2(mean, rsqrtf(var + E.ln_eps));
                }
                __syncthreads();
                lst = l;
            }
            epilogue(lst);
            m0 = nm0; c_tn = ntn; c_z = nz;
        }
        if (!more) break;
        zero_acc();
    }
}

namespace {
// (always more than 48 KiB of LDS: launch_lds sets the attribute at the first launch of each instantiation)
constexpr size_t wide_lds(int tn) { return GL_WIDE_NST * (256 + tn * 32) * 128; }
}  // namespace

int gemm_exec_wide(const Launch& l, const GemmPlan& p) {
    switch (p.gn * 100 + p.tm * 10 + p.tn) {
        case 85: return l.run<gemm_wide_kernel<5>>(p.grid, 512, wide_lds(5), p.wide);
        case 84: return l.run<gemm_wide_kernel<4>>(p.grid, 512, wide_lds(4), p.wide);
    }
    return gemm_unknown_tile();
}

}  // namespace gl
