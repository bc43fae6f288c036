// gemm_u_kernel ("v5", the default bf16 MFMA GEMM + implicit-GEMM 3x3 convolution for gfx950):
//
//   C[M][N] = A[M][K] * W[N][K]^T   (+ fused epilogue)
//
// persistent work-item loop, buffer-descriptor LDS-DMA loader, inline-asm fragment reads (lds_rd16, gemm_impl.h), load-first /
// LDS-staged epilogue, on-device autotuned tile / split-K / residency. v_mfma_f32_16x16x32_bf16, fp32 accumulate, both operands
// K-contiguous in LDS with 128-byte rows whose 16-byte chunks are XOR-swizzled by ((row >> 1) & 7): ds_read_b128 fragment reads
// and LDS-DMA writes are conflict free.
// Operand roles are exchanged w.r.t. the textbook mapping (MFMA "A" = weight rows, "B" = activation rows), so a lane owns
// ONE output row and groups of 4 CONSECUTIVE output columns: 8-byte bf16 stores, bias as float4, no transpose.
// The activation loader optionally performs the im2col gather of a 3x3 convolution over an NHWC tensor (stride 1|2,
// nearest-2x upsample of the source, channel concat of two sources, asymmetric padding), so convs never materialise
// im2col or concat / upsample copies in HBM. It also runs the upsample + conv pair as four 2x2 convs on the source, one per
// output phase (A_CONV2UP, gemm.h: 4/9 of the multiply-adds; the nine-tap upsample loader stays for the training forward).
// Split-K goes through an fp32 slab workspace + splitk_reduce_kernel (gemm.hip).
#include "gemm_impl.h"

namespace gl {

// ---------------------------------------------------------------------------------------------
// v5 (unified persistent kernel, variant 4): 4 waves (2 M x 2 N), (TM*32) x (TN*32) tile, two LDS stages, two to four workgroups
// per CU. (Rounds 1-2 carried an 8-wave / three-stage geometry and a four-stage ring at one workgroup per CU in the same code;
// both lost every A/B and every autotune, DESIGN.md section 4, and were taken out in round 3.)
// What changed against v3/v4 is the loader. PMC showed v3 spending ~300 VALU/SALU instructions per
// K tile per wave on 64-bit DMA source addresses against 20-40 MFMAs (SQ_ACTIVE_INST_ANY ~ the
// whole budget of a wave, MFMA pipe 28 % busy), so both operands are fetched with
// buffer_load_dwordx4 ... lds through wave-uniform buffer descriptors: the per-lane byte offset
// (row, swizzled 16-byte chunk) is computed once per work item (conv: once per filter tap), the
// K-tile offset rides in the SGPR soffset, and a DMA costs one s_mov m0 + one buffer_load. Rows
// outside M / N and conv padding taps use an offset beyond num_records, for which the hardware
// returns zeros.
// QKV (EPI_QKV_HEADS, A_ROWS only): its own instantiations, so that the other kernels' register allocation is untouched
template <int WMW, int TM, int TN, int AMODE, int NST, bool QKV = false>
__global__ void __launch_bounds__(WMW * 128, 2)
gemm_u_kernel(AOperand A, const bf16* __restrict__ W, int M, int N, int K, Epilogue E, float* __restrict__ ws, WorkDesc wd) {
    constexpr int NT = WMW * 128;               // threads
    constexpr int RPP = NT / 8;                 // tile rows per DMA pass (one 128-byte row per 8 lanes)
    constexpr int BM = WMW * TM * 16;
    constexpr int BN = TN * 32;
    constexpr int XP = BM / RPP;                // activation passes
    constexpr int WP = BN / RPP;                // weight passes
    constexpr int STAGE = (BM + BN) * 128;      // two stages: the two (to four) 4-wave workgroups of a CU hide each other's DMA latency
    constexpr unsigned SENT = 0x80000000u;      // >= num_records of every descriptor: reads as zeros
    // A_CONV2UP (gemm.h): the four output phases are four ranges of TPP row tiles; a tile's rows are phase-local (< MP), its slab rows
    // for split-K are phase-major (phase * MP + row) and only the final store knows the interleaved output row
    constexpr bool UP = AMODE == A_CONV2UP;
    constexpr int TAPW = UP ? 2 : 3;            // filter taps per row
    static_assert(WMW == 2 && NST == 2, "one geometry: 4 waves, two LDS stages (deeper rings and the 8-wave form lost every A/B, DESIGN.md section 4)");
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile/loader mismatch");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1;
    const int wn = wave & 1;
    const int r0 = t >> 3;                                          // row inside a DMA pass
    const unsigned chb = (((t & 7) ^ ((r0 >> 1) & 7)) * 16);        // byte offset of this lane's (swizzled) source chunk
    const int nk = K >> 6;
    const int Cin = A.C0 + A.C1;
    const int Hup = UP ? A.Hin : A.Hin << A.ups;   // (UP walks the source itself)
    const int Wup = UP ? A.Win : A.Win << A.ups;
    const int MP = UP ? M >> 2 : M;             // rows a tile's row index is checked against
    const int TPP = (MP + BM - 1) / BM;         // (UP) row tiles per phase

    const __amdgpu_buffer_rsrc_t ra0 = __builtin_amdgcn_make_buffer_rsrc((void*)A.p0, 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra1 = __builtin_amdgcn_make_buffer_rsrc((void*)(A.p1 ? A.p1 : A.p0), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, 0x80000000u, 0x00020000);

    auto decode = [&](int w, int& tm, int& tn, int& z) {
        const int xcd = w & 7, idx = w >> 3;
        int id = idx;
        if (wd.box < 0) {
            const int q = wd.n_items >> 3, r = wd.n_items & 7;
            id += xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        }
        const int tile = id / wd.rz;
        z = id - tile * wd.rz;
        tm = tile / wd.tiles_n;
        tn = tile - tm * wd.tiles_n;
        if (wd.box >= 0) {
            const int lgm = wd.box & 15, lgn = wd.box >> 4;
            z += (xcd >> (lgm + lgn)) * wd.rz;
            tn += ((xcd >> lgm) & ((1 << lgn) - 1)) * wd.tiles_n;
            tm += (xcd & ((1 << lgm) - 1)) * wd.rm;
        }
    };

    // ---- load cursor: (item, K tile) plus, for the conv gather, the filter tap and channel offset of that tile
    int l_item = blockIdx.x, l_kt = 0, l_kt_end = 0;
    int l_tap = 0, l_cc = 0;     // A_CONV3: k = l_tap * Cin + l_cc.   A_ROWS: l_cc = k
    int xm[XP], xy[XP], xx[XP];  // A_ROWS: xm = row or -1.  A_CONV3: xm = b * Hin, (xy, xx) = top-left tap (xy very negative: no row)
    unsigned va[XP], vw[WP];     // per-lane byte offsets into the current activation source / the weight matrix

    // byte offsets of this lane's activation chunks for the current (tap, source)
    auto a_offsets = [&]() {
        const bool first = l_cc < A.C0;
        const int ld = first ? A.ld0 : A.ld1;
        if constexpr (AMODE == A_ROWS) {
#pragma unroll
            for (int i = 0; i < XP; ++i) va[i] = xm[i] >= 0 ? (unsigned)(xm[i] * ld) * 2u + chb : SENT;
        } else {
            const int ky = l_tap / TAPW;
            const int kx = l_tap - ky * TAPW;
#pragma unroll
            for (int i = 0; i < XP; ++i) {
                const int iy = xy[i] + ky;
                const int ix = xx[i] + kx;
                const bool ok = iy >= 0 && iy < Hup && ix >= 0 && ix < Wup;
                const int pix = UP ? (xm[i] + iy) * A.Win + ix : (xm[i] + (iy >> A.ups)) * A.Win + (ix >> A.ups);
                va[i] = ok ? (unsigned)(pix * ld) * 2u + chb : SENT;
            }
        }
    };

    auto setup_load = [&](int item) {
        int tm, tn, z;
        decode(item, tm, tn, z);
        l_kt = z * wd.kt_per_split;
        l_kt_end = min(nk, l_kt + wd.kt_per_split);
        int ph = 0;                             // (UP) output phase 2 py + px of the tile; tm becomes its row tile inside the phase
        if constexpr (UP) { ph = tm / TPP; tm -= ph * TPP; }
#pragma unroll
        for (int i = 0; i < XP; ++i) {
            const int m = tm * BM + r0 + i * RPP;
            const bool ok = m < MP;
            if constexpr (AMODE == A_ROWS) {
                xm[i] = ok ? m : -1;
                xy[i] = xx[i] = 0;
            } else if constexpr (UP) {
                // phase row m = (b Hin + y) Win + x; top-left source tap (y - 1 + py, x - 1 + px)
                const int ox = m % A.Win;
                const int tmp = m / A.Win;
                const int oy = tmp % A.Hin;
                xm[i] = tmp - oy;               // b * Hin
                xy[i] = ok ? oy - 1 + (ph >> 1) : -(1 << 20);
                xx[i] = ox - 1 + (ph & 1);
            } else {
                const int ox = m % A.Wo;
                const int tmp = m / A.Wo;
                const int oy = tmp % A.Ho;
                xm[i] = (tmp / A.Ho) * A.Hin;
                xy[i] = ok ? oy * A.stride - A.pad_lo : -(1 << 20);
                xx[i] = ox * A.stride - A.pad_lo;
            }
        }
#pragma unroll
        for (int i = 0; i < WP; ++i) {
            const int n = tn * BN + r0 + i * RPP;
            vw[i] = (n < N) ? (unsigned)((UP ? ph * N + n : n) * K) * 2u + chb : SENT;   // (UP: the phase's folded filter, W = [4][N][K])
        }
        const int k0 = l_kt << 6;
        if constexpr (AMODE == A_ROWS) {
            l_tap = 0;
            l_cc = k0;
        } else {
            l_tap = k0 / Cin;
            l_cc = k0 - l_tap * Cin;
        }
        a_offsets();
    };

    // DMA of K tile l_kt into ring slot `slot`, then advance the cursor by one tile
    bool more = true;
    auto issue_next = [&](int slot_) {
        // the cursor is wave-uniform by construction; say so, or one value merged through a divergent
        // branch makes hipcc wrap every buffer_load in a waterfall loop (descriptor / soffset / m0 "divergent")
        const int slot = __builtin_amdgcn_readfirstlane(slot_);
        l_cc = __builtin_amdgcn_readfirstlane(l_cc);
        l_kt = __builtin_amdgcn_readfirstlane(l_kt);
        unsigned char* xs = smem + slot * STAGE + wave * 1024;
        unsigned char* wsm = xs + BM * 128;
        const bool first = l_cc < A.C0;
        const int soff = (first ? l_cc : l_cc - A.C0) * 2;
        if (first) {
#pragma unroll
            for (int i = 0; i < XP; ++i) GL_BLDS16(ra0, xs + i * RPP * 128, va[i], soff);
        } else {
#pragma unroll
            for (int i = 0; i < XP; ++i) GL_BLDS16(ra1, xs + i * RPP * 128, va[i], soff);
        }
        const int woff = l_kt << 7;
#pragma unroll
        for (int i = 0; i < WP; ++i) GL_BLDS16(rw, wsm + i * RPP * 128, vw[i], woff);
        // advance
        l_cc += 64;
        if (++l_kt >= l_kt_end) {
            l_item += gridDim.x;
            more = l_item < wd.n_items;
            if (more) setup_load(l_item);
        } else if constexpr (AMODE != A_ROWS) {
            if (l_cc == Cin) {
                l_cc = 0;
                ++l_tap;
                a_offsets();
            } else if (l_cc == A.C0) {
                a_offsets();
            }
        } else {
            if (A.C1 && l_cc == A.C0) a_offsets();
        }
    };

    f32x4 acc[TM][TN];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    zero_acc();

    // fragment addressing: lane reads row (16 t + l15), 16-byte chunk 4 s + (lane >> 4); rows start at
    // multiples of 16, so the swizzle term ((row >> 1) & 7) is the lane constant l15 >> 1
    const int l15 = lane & 15;
    const int foff0 = l15 * 128 + ((((lane >> 4)) ^ (l15 >> 1)) << 4);
    const int foff1 = l15 * 128 + ((((lane >> 4) + 4) ^ (l15 >> 1)) << 4);
    const int xrow0 = wm * TM * 16 * 128;
    const int wrow0 = BM * 128 + wn * TN * 16 * 128;

    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    // swapv (wave-uniform, EPI_QKV_HEADS items in the V third): MFMA operand roles exchanged -- lane (l15, q) then holds
    // feature l15 and tokens 4q .. 4q+3 of every 16x16 tile (the v^T store pattern) instead of token l15, features 4q .. 4q+3
    auto compute = [&](int slot, bool swapv) {
        const unsigned st = lds0 + slot * STAGE;
        const unsigned ax0 = st + xrow0 + foff0, ax1 = st + xrow0 + foff1;
        const unsigned aw0 = st + wrow0 + foff0, aw1 = st + wrow0 + foff1;
        bf16x8 xa[TM], wa[TN], xb[TM], wb[TN];
        lds_rd16_n<TM, 2048>(xa, ax0);
        lds_rd16_n<TN, 2048>(wa, aw0);
        lds_rd16_n<TM, 2048>(xb, ax1);
        lds_rd16_n<TN, 2048>(wb, aw1);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(TM + TN));  // the k-step 0 fragments have returned
        pin_regs(xa);
        pin_regs(wa);
        __builtin_amdgcn_sched_barrier(0);
        if (!QKV || !swapv) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[j], xa[i], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i], wa[j], acc[i][j], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)");
        pin_regs(xb);
        pin_regs(wb);
        __builtin_amdgcn_sched_barrier(0);
        if (!QKV || !swapv) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j], xb[i], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xb[i], wb[j], acc[i][j], 0, 0, 0);
        }
    };

    // Folded LayerNorm (gemm.h, Epilogue::ln_stats): (mean, rstd) of the item's BM rows from the producer's partial sums, into the
    // ring slot whose K tile was multiplied last. TPR threads per row add the partials in a fixed order.
    // ln_fetch (when the compute cursor enters an item: the loads fly under its K loop) + ln_prepare (in front of its epilogue)
    // (the loaded pairs stay in registers untouched until ln_prepare: an add right behind the load would make hipcc wait for it there)
    constexpr int LNV = 5;
    float2 ln_v[LNV];
    float ln_s = 0.f, ln_q = 0.f;
    auto ln_fetch = [&](int tm) {
        constexpr int TPR = NT / BM;
        const int row = t / TPR, part = t % TPR;
        const int m = tm * BM + row;
        ln_s = ln_q = 0.f;
#pragma unroll
        for (int i = 0; i < LNV; ++i) {
            const int nb = part + i * TPR;
            ln_v[i] = make_float2(0.f, 0.f);
            if (m < M && nb < E.ln_nb) ln_v[i] = E.ln_stats[(size_t)m * E.ln_ld + nb];
        }
        if (m < M)
            for (int nb = part + LNV * TPR; nb < E.ln_nb; nb += TPR) {   // (more than LNV * TPR column blocks: the 16x16 / 8x8 levels)
                const float2 v = E.ln_stats[(size_t)m * E.ln_ld + nb];
                ln_s += v.x; ln_q += v.y;
            }
    };
    auto ln_prepare = [&](int tm, int slot_done) -> const float2* {
        float2* lst = reinterpret_cast<float2*>(smem + slot_done * STAGE);
        constexpr int TPR = NT / BM;
        __builtin_amdgcn_s_barrier();          // every wave is done with the fragments of that slot
        const int row = t / TPR, part = t % TPR;
        float s = ln_s, q = ln_q;
#pragma unroll
        for (int i = 0; i < LNV; ++i) { s += ln_v[i].x; q += ln_v[i].y; }
#pragma unroll
        for (int o = 1; o < TPR; o <<= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
        if (part == 0) {
            const float mean = s * E.ln_inv_c;
            const float var = fmaxf(q * E.ln_inv_c - mean * mean, 0.f);
            lst[row] = make_float2(mean, rsqrtf(var + E.ln_eps));
        }
        __syncthreads();
        return lst;
    };

    // q / k scatter of a QKV item outside the V third (the EPI_QK_HEADS store, no residual forms; a bias only with the folded LayerNorm)
    // Both head-layout epilogues fetch every coefficient (bias, csum, row statistics) BEFORE their first store and make hipcc wait
    // for them right there (epi_ready): vmcnt counts stores too, so a coefficient load between stores -- or a wait the compiler
    // re-inserts in every guarded block because the guard's other path has not waited -- makes each store wait for the
    // acknowledgement of the one before it (28 of the 32 stores of an item did, round 3).
    auto epilogue_qk = [&](int tm, int tn, const float2* lst) {
        const int mrow = tm * BM + wm * TM * 16 + l15;
        const int ncol = tn * BN + wn * TN * 16 + (lane >> 4) * 4;
        float2 st[TM];
        int rb[TM], rt[TM];   // sample and token of this lane's row in each row block
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            st[i] = lst ? lst[wm * TM * 16 + i * 16 + l15] : make_float2(0.f, 1.f);
            const int m = mrow + i * 16;
            rb[i] = m / E.T;
            rt[i] = m - rb[i] * E.T + E.tok_off;
        }
        float4 cs[TN], bj[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n0 = ncol + j * 16;
            cs[j] = bj[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n0 < N) {
                if (lst) cs[j] = *reinterpret_cast<const float4*>(E.ln_csum + n0);
                if (E.bias) bj[j] = *reinterpret_cast<const float4*>(E.bias + n0);   // (W beta of a folded LayerNorm, with or without statistics)
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) { epi_ready(cs[j]); epi_ready(bj[j]); }
#pragma unroll
        for (int i = 0; i < TM; ++i) asm volatile("" : "+v"(st[i].x), "+v"(st[i].y));
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n0 = ncol + j * 16;
            if (n0 >= N) continue;
            const int which = n0 >= E.C;
            const int cc = n0 - which * E.C;
            const int h = cc / E.d;
            const int dd = cc - h * E.d;
            bf16* base = which ? E.k : E.q;
            const int tp = which ? E.Tpad_k : E.Tpad_q;
            const bool tiled = which || E.q_tiled;   // keys: key-tile layout (gemm.h ktile_off)
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if (mrow + i * 16 >= M) continue;
                const int b = rb[i], t = rt[i];
                float v[4] = {st[i].y * (acc[i][j][0] - st[i].x * cs[j].x) + bj[j].x, st[i].y * (acc[i][j][1] - st[i].x * cs[j].y) + bj[j].y,
                              st[i].y * (acc[i][j][2] - st[i].x * cs[j].z) + bj[j].z, st[i].y * (acc[i][j][3] - st[i].x * cs[j].w) + bj[j].w};
                const size_t off = tiled ? ktile_off((size_t)(b * E.H + h), tp, t, dd, E.DP) : ((size_t)(b * E.H + h) * tp + t) * E.DP + dd;
                store_bf16x4(base + off, v);
            }
            __builtin_amdgcn_sched_barrier(0);   // addresses just in time: hoisting all TM x TN of them costs registers (spills at 4 x 5)
        }
    };

    // v^T store of an operand-swapped item (EPI_QKV_HEADS): feature n = column, 4 consecutive tokens per lane
    auto epilogue_vt = [&](int tm, int tn, const float2* lst) {
        const int nfeat = tn * BN + wn * TN * 16 + l15;
        const int mtok = tm * BM + wm * TM * 16 + (lane >> 4) * 4;
        float csv[TN], bnv[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = nfeat + j * 16;
            csv[j] = (lst && n < N) ? E.ln_csum[n] : 0.f;
            bnv[j] = (E.bias && n < N) ? E.bias[n] : 0.f;
        }
        float4 s01[TM], s23[TM];   // (mean, rstd) of the lane's four tokens of each row block: rows (wm TM + i) 16 + 4 q .. + 3 of the item
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            s01[i] = make_float4(0.f, 1.f, 0.f, 1.f);
            s23[i] = s01[i];
            if (lst) {
                s01[i] = *reinterpret_cast<const float4*>(lst + wm * TM * 16 + i * 16 + (lane >> 4) * 4);
                s23[i] = *reinterpret_cast<const float4*>(lst + wm * TM * 16 + i * 16 + (lane >> 4) * 4 + 2);
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(csv[j]), "+v"(bnv[j]));
#pragma unroll
        for (int i = 0; i < TM; ++i) { epi_ready(s01[i]); epi_ready(s23[i]); }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = nfeat + j * 16;
            if (n >= N) continue;
            const int cfeat = n - 2 * E.C;
            const int h = cfeat / E.d;
            const int dd = cfeat - h * E.d;
            const float cs = csv[j], bn = bnv[j];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m0 = mtok + i * 16;
                if (m0 >= M) continue;
                const int b = m0 / E.T;
                const int t0 = m0 - b * E.T + E.tok_off;
                float v[4] = {s01[i].y * (acc[i][j][0] - s01[i].x * cs) + bn, s01[i].w * (acc[i][j][1] - s01[i].z * cs) + bn,
                              s23[i].y * (acc[i][j][2] - s23[i].x * cs) + bn, s23[i].w * (acc[i][j][3] - s23[i].z * cs) + bn};
                store_bf16x4(E.vt + ((size_t)(b * E.H + h) * E.DPV + dd) * E.Tpad_k + perm_tok4(t0, E.vt_perm32), v);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // Epilogue: every load (bias, time-embedding bias, residual, gate) of the wave's TM x TN fragments is issued
    // before the first store (see epi_store4).
    auto epilogue = [&](int tm, int tn, int z) {
        int slab0 = 0;                          // (UP) first slab row of the tile's phase
        if constexpr (UP) { const int ph = tm / TPP; tm -= ph * TPP; slab0 = ph * MP; }
        const int mrow = tm * BM + wm * TM * 16 + l15;
        const int ncol = tn * BN + wn * TN * 16 + (lane >> 4) * 4;
        if (wd.splits > 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
                if (m >= MP) continue;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n0 = ncol + j * 16;
                    if (n0 >= N) continue;
                    *reinterpret_cast<float4*>(ws + ((size_t)z * M + slab0 + m) * N + n0) =
                        make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                }
            }
            return;
        }
        if constexpr (UP) return;               // (unsplit A_CONV2UP items always leave through epilogue_staged: gemm_upconv_phases_supported)
        if (E.act == ACT_GEGLU) {
            if constexpr (TN % 2 == 0) {
                float4 bv[TN / 2], bg[TN / 2];
#pragma unroll
                for (int jj = 0; jj < TN / 2; ++jj) {
                    const int n0 = ncol + jj * 32;
                    bv[jj] = bg[jj] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (E.bias && n0 < N) {
                        bv[jj] = *reinterpret_cast<const float4*>(E.bias + n0);
                        bg[jj] = *reinterpret_cast<const float4*>(E.bias + n0 + 16);
                    }
                }
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int m = mrow + i * 16;
                    if (m >= M) continue;
#pragma unroll
                    for (int jj = 0; jj < TN / 2; ++jj) {
                        const int n0 = ncol + jj * 32;
                        if (n0 >= N) continue;
                        const float bvv[4] = {bv[jj].x, bv[jj].y, bv[jj].z, bv[jj].w};
                        const float bgg[4] = {bg[jj].x, bg[jj].y, bg[jj].z, bg[jj].w};
                        float o[4];
#pragma unroll
                        for (int e = 0; e < 4; e += 2) {
                            const f32x2 r = geglu2(f32x2{acc[i][2 * jj][e] + bvv[e], acc[i][2 * jj][e + 1] + bvv[e + 1]},
                                                   f32x2{acc[i][2 * jj + 1][e] + bgg[e], acc[i][2 * jj + 1][e + 1] + bgg[e + 1]});
                            o[e] = r.x;
                            o[e + 1] = r.y;
                        }
                        const int j0 = (n0 >> 5) * 16 + (n0 & 15);
                        store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + j0, o);
                    }
                }
            }
            return;
        }
        float4 bj[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n0 = ncol + j * 16;
            bj[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (E.bias && n0 < N) bj[j] = *reinterpret_cast<const float4*>(E.bias + n0);
        }
        int mo[TM];  // output row (EPI_ROWMAJOR row remap applied)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = mrow + i * 16;
            mo[i] = (AMODE == A_ROWS && E.mode == EPI_ROWMAJOR && E.remap_in) ? (m / E.remap_in) * E.remap_out + (m % E.remap_in) + E.remap_off : m;
        }
        if (AMODE == A_CONV3 && E.bias2) {  // + broadcast per-sample bias (ResBlock time embedding); never combined with a residual; convs only (gemm_route)
            float4 b2[TM][TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
                const int bb = div_rpb(E, m);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n0 = ncol + j * 16;
                    b2[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (m < M && n0 < N) b2[i][j] = *reinterpret_cast<const float4*>(E.bias2 + (size_t)bb * E.bias2_ld + n0);
                }
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
                if (m >= M) continue;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n0 = ncol + j * 16;
                    if (n0 >= N) continue;
                    float v[4] = {acc[i][j][0] + bj[j].x + b2[i][j].x, acc[i][j][1] + bj[j].y + b2[i][j].y,
                                  acc[i][j][2] + bj[j].z + b2[i][j].z, acc[i][j][3] + bj[j].w + b2[i][j].w};
                    epi_store4<AMODE == A_ROWS>(E, mo[i], n0, v);
                }
            }
        } else if (E.mode == EPI_ROWMAJOR && E.res) {
            // (the fallback of epilogue_staged: fp32 / NCHW outputs, GELU, ragged N. The 128 x 160 tile fetches the residual one row
            // block at a time -- all 20 pieces at once do not fit its registers)
            constexpr bool ROWWISE = TM == 4 && TN == 5;
            uint2 rs[TM][TN];
            const float g = (AMODE == A_ROWS && E.gate) ? *E.gate : 1.f;
            auto fetch_row = [&](int i) {
                const int m = mrow + i * 16;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n0 = ncol + j * 16;
                    rs[ROWWISE ? 0 : i][j] = make_uint2(0, 0);
                    if (m < M && n0 < N) rs[ROWWISE ? 0 : i][j] = *reinterpret_cast<const uint2*>(E.res + (size_t)mo[i] * E.ldres + n0);
                }
            };
            if constexpr (!ROWWISE) {
#pragma unroll
                for (int i = 0; i < TM; ++i) fetch_row(i);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
                if constexpr (ROWWISE) fetch_row(i);
                if (m >= M) continue;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n0 = ncol + j * 16;
                    if (n0 >= N) continue;
                    U2BF4 r;
                    r.u = rs[ROWWISE ? 0 : i][j];
                    float v[4] = {acc[i][j][0] + bj[j].x, acc[i][j][1] + bj[j].y, acc[i][j][2] + bj[j].z, acc[i][j][3] + bj[j].w};
                    if (E.act == ACT_SILU) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = bf2f(r.e[e]) + g * v[e];
                    if (E.out_f32) {
                        *reinterpret_cast<float4*>(reinterpret_cast<float*>(E.out) + (size_t)mo[i] * E.ldo + n0) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
                        store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)mo[i] * E.ldo + n0, v);
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
                if (m >= M) continue;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n0 = ncol + j * 16;
                    if (n0 >= N) continue;
                    float v[4] = {acc[i][j][0] + bj[j].x, acc[i][j][1] + bj[j].y, acc[i][j][2] + bj[j].z, acc[i][j][3] + bj[j].w};
                    epi_store4<AMODE == A_ROWS>(E, mo[i], n0, v);
                }
            }
        }
    };

    // Row-major bf16 outputs leave through LDS: a fragment-layout store writes 16 rows x 32 B per instruction (measured
    // 2.7 TB/s for the tile set of one 32768 x 320 output, tools/storebench.hip), whole-row pieces of 16 B per lane reach 3.9,
    // and the residual is read the same way. Each wave stages one 16-row fragment row of its sub-tile at a time, in fp32
    // (single rounding, as before), in a private piece of the ring slot whose K tile was multiplied last.
    constexpr int WCOLS = TN * 16;                 // columns of a wave's sub-tile
    constexpr int LPR = WCOLS / 8;                 // lanes per staged row (8 columns each)
    constexpr int RPI = 64 / LPR;                  // rows per read instruction
    constexpr int NRI = (16 + RPI - 1) / RPI;      // read instructions per 16-row fragment row
    constexpr int RS = WCOLS * 4 + 16;             // staged row stride (bytes): +16 keeps the b128 writes conflict-free
    constexpr int EPW = 16 * RS;                   // bytes per wave
    static_assert(WMW * 2 * (EPW + 16 * LPR * 8) <= STAGE, "epilogue staging (+ row-statistics scratch) does not fit one ring slot");
    auto epilogue_staged = [&](int tm, int tn, int slot_done) -> bool {
        if (wd.splits > 1 || E.mode != EPI_ROWMAJOR || E.out_f32 || (N & 7) || (E.act == ACT_GEGLU && (TN & 1)) || E.act == ACT_GELU || E.act == ACT_QUICK_GELU) return false;
        if (E.res && E.act == ACT_SILU) return false;   // (no caller combines them; the fragment-layout epilogue handles it)
        unsigned char* ep = smem + slot_done * STAGE + wave * EPW;
        if constexpr ((TN & 1) == 0) {
            // value / gate fragments alternate (16 columns each), so a wave's TN*16 accumulator columns become TN*8 output
            // columns: val * gelu(gate) is formed in the fragment layout and staged, then leaves as 16 B per lane
            if (E.act == ACT_GEGLU) {
                constexpr int OW = TN * 8;                 // output columns of the wave
                constexpr int LPG = OW / 8;                // lanes per staged row
                constexpr int RSG = OW * 4 + 16;
                if (E.res || E.bias2 || E.remap_in || ((N >> 1) & 7)) return false;
                const int mrow = tm * BM + wm * TM * 16;
                const int ncb = tn * BN + wn * WCOLS;      // first accumulator column (a multiple of 32)
                const int rr = lane / LPG, cc = lane - rr * LPG;
                const int ocol = (ncb >> 1) + cc * 8;
                __builtin_amdgcn_s_barrier();
                float4 bv[TN / 2], bg[TN / 2];
#pragma unroll
                for (int jj = 0; jj < TN / 2; ++jj) {
                    const int n0 = ncb + jj * 32 + (lane >> 4) * 4;
                    bv[jj] = bg[jj] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (E.bias && n0 < N) {
                        bv[jj] = *reinterpret_cast<const float4*>(E.bias + n0);
                        bg[jj] = *reinterpret_cast<const float4*>(E.bias + n0 + 16);
                    }
                }
#pragma unroll
                for (int i = 0; i < TM; ++i) {
#pragma unroll
                    for (int jj = 0; jj < TN / 2; ++jj) {
                        const f32x2 r0 = geglu2(f32x2{acc[i][2 * jj][0] + bv[jj].x, acc[i][2 * jj][1] + bv[jj].y},
                                                f32x2{acc[i][2 * jj + 1][0] + bg[jj].x, acc[i][2 * jj + 1][1] + bg[jj].y});
                        const f32x2 r1 = geglu2(f32x2{acc[i][2 * jj][2] + bv[jj].z, acc[i][2 * jj][3] + bv[jj].w},
                                                f32x2{acc[i][2 * jj + 1][2] + bg[jj].z, acc[i][2 * jj + 1][3] + bg[jj].w});
                        *reinterpret_cast<float4*>(ep + l15 * RSG + (jj * 16 + (lane >> 4) * 4) * 4) = make_float4(r0.x, r0.y, r1.x, r1.y);
                    }
                    const int m = mrow + i * 16 + rr;
                    if (rr < 16 && m < M && ocol < (N >> 1)) {
                        const float4 a = *reinterpret_cast<const float4*>(ep + rr * RSG + cc * 32);
                        const float4 b = *reinterpret_cast<const float4*>(ep + rr * RSG + cc * 32 + 16);
                        U4BF8 o;
                        o.e[0] = f2bf(a.x); o.e[1] = f2bf(a.y); o.e[2] = f2bf(a.z); o.e[3] = f2bf(a.w);
                        o.e[4] = f2bf(b.x); o.e[5] = f2bf(b.y); o.e[6] = f2bf(b.z); o.e[7] = f2bf(b.w);
                        *reinterpret_cast<uint4*>(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + ocol) = o.u;
                    }
                }
                return true;
            }
        }
        int up_py = 0, up_px = 0;                              // (UP) output phase of the tile; tm becomes its row tile inside the phase
        if constexpr (UP) { const int ph = tm / TPP; tm -= ph * TPP; up_py = ph >> 1; up_px = ph & 1; }
        const int mrow = tm * BM + wm * TM * 16;               // first row of the wave's sub-tile
        const int ncb = tn * BN + wn * WCOLS;                  // first column
        const int rr = lane / LPR, cc = lane - rr * LPR;       // read side: row inside a read instruction, 8-column group
        float2* scr = reinterpret_cast<float2*>(smem + slot_done * STAGE + WMW * 2 * EPW) + wave * 16 * LPR;   // row-statistics scratch (Epilogue::stats_out)
        const int ncol = ncb + cc * 8;
        const bool col_ok = rr < RPI && ncol < N;
        // every wave is done with the fragments of the last K tile before any wave overwrites the slot
        __builtin_amdgcn_s_barrier();
        // ---- loads first (one in-order vmcnt for loads and stores): bias, time-embedding bias, residual
        float4 bj[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n0 = ncb + j * 16 + (lane >> 4) * 4;
            bj[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (E.bias && n0 < N) bj[j] = *reinterpret_cast<const float4*>(E.bias + n0);
        }
        const float g = (AMODE == A_ROWS && E.gate) ? *E.gate : 1.f   /* (gate and row remap exist for row GEMMs only: gemm_launch rejects them on a conv) */;
        auto out_row = [&](int i, int k) {  // output row of read instruction k of fragment row i, or -1
            const int r = k * RPI + rr;
            const int m = mrow + i * 16 + r;
            if (!(col_ok && r < 16 && m < MP)) return -1;
            if constexpr (UP) {   // phase row (b Hin + y) Win + x -> output row (b 2 Hin + 2 y + py) 2 Win + 2 x + px (div_rpb divides by Win here)
                const int q = div_rpb(E, m);
                return ((2 * q + up_py) * E.up_win + (m - q * E.up_win)) * 2 + up_px;
            }
            return (AMODE == A_ROWS && E.remap_in) ? (m / E.remap_in) * E.remap_out + (m % E.remap_in) + E.remap_off : m;
        };
        // the residual is prefetched for two fragment rows at a time (register budget); the second pair's loads queue behind
        // the first pair's stores, one extra store round trip per work item instead of one per fragment
        // Two copies of the row loop, chosen by a uniform branch: with the residual its loads have no "or zeros" alternative, so
        // hipcc cannot fold the bf16 unpacking into the block that loads (which made it wait for every load right behind its issue:
        // 32 of the epilogue's loads in the round-2 form, one memory round trip each)
        constexpr int PF = (TM >= 2 && !(TM == 4 && TN == 5)) ? 2 : 1;   // (128 x 160: one row block at a time, the tile sits at the 256-register limit)
        auto rows = [&](auto res_c) {
        constexpr bool HAS_RES = decltype(res_c)::value;
        uint4 rs[PF][NRI];
        auto prefetch_res = [&](int i0) {
            if constexpr (!HAS_RES) return;
#pragma unroll
            for (int ii = 0; ii < PF; ++ii)
#pragma unroll
                for (int k = 0; k < NRI; ++k) {
                    // UNCONDITIONAL per lane (a lane without an output row reads the tensor's first 16 bytes and never uses them):
                    // behind a per-lane guard hipcc unpacks the bf16 pairs inside the guarded block, i.e. waits for every load
                    // right behind its issue -- the residual reads of an item then cost one memory round trip EACH
                    const int mo = out_row(i0 + ii, k);
                    rs[ii][k] = *reinterpret_cast<const uint4*>(E.res + (mo >= 0 ? (size_t)mo * E.ldres + ncol : (size_t)0));
                }
        };
        auto res_ready = [&]() {   // one wait for the pair in front of its first store block (see epi_ready)
            if constexpr (!HAS_RES) return;
#pragma unroll
            for (int ii = 0; ii < PF; ++ii)
#pragma unroll
                for (int k = 0; k < NRI; ++k) asm volatile("" : "+v"(rs[ii][k].x), "+v"(rs[ii][k].y), "+v"(rs[ii][k].z), "+v"(rs[ii][k].w));
        };
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            if (i % PF == 0) prefetch_res(i);
            // fragment layout -> LDS: lane (l15, q) holds row l15, columns 16 j + 4 q .. + 3
            const int mf = mrow + i * 16 + l15;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                float4 v = make_float4(acc[i][j][0] + bj[j].x, acc[i][j][1] + bj[j].y, acc[i][j][2] + bj[j].z, acc[i][j][3] + bj[j].w);
                if (AMODE == A_CONV3 && E.bias2) {
                    const int n0 = ncb + j * 16 + (lane >> 4) * 4;
                    if (mf < M && n0 < N) {
                        const float4 b2 = *reinterpret_cast<const float4*>(E.bias2 + (size_t)div_rpb(E, mf) * E.bias2_ld + n0);
                        v.x += b2.x; v.y += b2.y; v.z += b2.z; v.w += b2.w;
                    }
                }
                *reinterpret_cast<float4*>(ep + l15 * RS + (j * 16 + (lane >> 4) * 4) * 4) = v;
            }
            if (i % PF == 0) res_ready();
            // LDS -> whole-row pieces: 8 consecutive columns per lane
#pragma unroll
            for (int k = 0; k < NRI; ++k) {
                const int r = k * RPI + rr;
                const int mo = out_row(i, k);
                if (mo < 0) continue;
                const float4 a = *reinterpret_cast<const float4*>(ep + r * RS + cc * 32);
                const float4 b = *reinterpret_cast<const float4*>(ep + r * RS + cc * 32 + 16);
                float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                if constexpr (!HAS_RES) {
                    if (E.act == ACT_SILU) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = silu_f(v[e]);
                    }
                }
                U4BF8 o;
                if constexpr (HAS_RES) {
                    U4BF8 rv;
                    rv.u = rs[i % PF][k];
#pragma unroll
                    for (int e = 0; e < 8; ++e) o.e[e] = f2bf(bf2f(rv.e[e]) + g * v[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o.e[e] = f2bf(v[e]);
                }
                *reinterpret_cast<uint4*>(reinterpret_cast<bf16*>(E.out) + (size_t)mo * E.ldo + ncol) = o.u;
                if constexpr (AMODE == A_ROWS) {
                    if (E.stats_out) {   // this lane's 8 FINAL outputs of row r -> (sum, sum of squares), through the wave's scratch
                        float s8 = 0.f, q8 = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const float f = bf2f(o.e[e]); s8 += f; q8 += f * f; }
                        scr[r * LPR + cc] = make_float2(s8, q8);
                    }
                }
            }
            if constexpr (AMODE == A_ROWS) {
                if (E.stats_out) {
                    // lanes 0..15 add the LPR pieces of "their" row in a fixed order: the row's partial over this wave's column block
                    __builtin_amdgcn_wave_barrier();
                    const int m = mrow + i * 16 + lane;
                    if (lane < 16 && m < M && ncb < N) {     // (a wave whose column block lies beyond N has nothing to report)
                        float s = 0.f, q = 0.f;
#pragma unroll
                        for (int c = 0; c < LPR; ++c) { const float2 v2 = scr[lane * LPR + c]; s += v2.x; q += v2.y; }
                        const int mo2 = E.remap_in ? (m / E.remap_in) * E.remap_out + (m % E.remap_in) + E.remap_off : m;
                        E.stats_out[(size_t)mo2 * E.stats_ld + (tn * 2 + wn)] = make_float2(s, q);
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        };
        if (E.res) rows(std::true_type{});
        else rows(std::false_type{});
        return true;
    };

    if (l_item >= wd.n_items) return;
    setup_load(l_item);
    int c_item = l_item, c_tm, c_tn, c_z;
    decode(c_item, c_tm, c_tn, c_z);
    bool c_swap = QKV && c_tn * BN >= 2 * E.C;   // BN divides 2C (checked on the host): an item is all V or no V
    if constexpr (QKV) {
        if (E.ln_stats) ln_fetch(c_tm);
    }
    int c_left = l_kt_end - l_kt;
    int slot_c = 0;      // ring slot of the tile being multiplied; the next tile's DMA goes into the other one
    if (more) issue_next(slot_c);
    for (;;) {
        c_left = __builtin_amdgcn_readfirstlane(c_left);
        slot_c = __builtin_amdgcn_readfirstlane(slot_c);
        more = __builtin_amdgcn_readfirstlane((int)more) != 0;
        // vmcnt(0), unconditional and through the builtin so that hipcc KNOWS nothing is pending: behind an asm wait its scoreboard
        // carries the epilogue's bias / residual loads (whose destination VGPRs the fragments reuse) around the loop and it re-waits
        // vmcnt(0) in front of the first fragment register write, i.e. right after the next DMA issue
        __builtin_amdgcn_s_waitcnt(0x0F70);
        // tile c is in LDS for every wave after this barrier, and every wave has finished reading tile c-1
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (more) issue_next(slot_c ^ 1);
        compute(slot_c, c_swap);
        const int slot_done = slot_c;
        slot_c ^= 1;
        if (--c_left == 0) {
            if constexpr (QKV) {
                // folded LayerNorm (the head-layout epilogues, unsplit by construction): row statistics first
                const float2* lst = E.ln_stats ? ln_prepare(c_tm, slot_done) : nullptr;
                if (c_swap) epilogue_vt(c_tm, c_tn, lst);
                else epilogue_qk(c_tm, c_tn, lst);
            } else {
                if (!epilogue_staged(c_tm, c_tn, slot_done)) epilogue(c_tm, c_tn, c_z);
            }
            c_item += gridDim.x;
            if (c_item >= wd.n_items) break;
            zero_acc();
            decode(c_item, c_tm, c_tn, c_z);
            c_swap = QKV && c_tn * BN >= 2 * E.C;
            if constexpr (QKV) {
                if (E.ln_stats) ln_fetch(c_tm);
            }
            c_left = min(nk, (c_z + 1) * wd.kt_per_split) - c_z * wd.kt_per_split;
        }
    }
}

namespace {

template <int TM, int TN>
int exec_u(const Launch& l, const GemmPlan& p) {   // 2 x 2 waves (WMW = 2) on a 2-stage ring
    const size_t lds = 2 * (TM * 32 + TN * 32) * 128;
    if (p.qkv) {   // (no 128 x 160 tile for the head layouts: gemm_plan_tile refuses it)
        if constexpr (TM == 4 && TN == 5) return set_error(GL_ERR_UNSUPPORTED, "gemm: no 128x160 tile for EPI_QKV_HEADS");
        else return l.run<gemm_u_kernel<2, TM, TN, A_ROWS, 2, true>>(p.grid, 256, lds, p.work);
    }
    if (p.amode == A_ROWS) return l.run<gemm_u_kernel<2, TM, TN, A_ROWS, 2>>(p.grid, 256, lds, p.work);
    if (p.amode == A_CONV2UP) return l.run<gemm_u_kernel<2, TM, TN, A_CONV2UP, 2>>(p.grid, 256, lds, p.work);
    return l.run<gemm_u_kernel<2, TM, TN, A_CONV3, 2>>(p.grid, 256, lds, p.work);
}

}  // namespace

int gemm_exec_u(const Launch& l, const GemmPlan& p) {
    switch (p.gn * 100 + p.tm * 10 + p.tn) {
        case 45: return exec_u<4, 5>(l, p);
        case 44: return exec_u<4, 4>(l, p);
        case 25: return exec_u<2, 5>(l, p);
        case 24: return exec_u<2, 4>(l, p);
        case 22: return exec_u<2, 2>(l, p);
    }
    return gemm_unknown_tile();
}

}  // namespace gl
