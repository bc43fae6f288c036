// conv_halo_kernel: the stride-1 3x3 convolution that stages its input pixels once per 64-channel chunk, halo included, and walks
// the nine filter taps inside LDS. Its header comment below is the description of this unit.
#include "gemm_impl.h"

namespace gl {

// ---------------------------------------------------------------------------------------------------------------------------
// conv3x3 "halo" kernel (stride 1, pad 1, power-of-two images up to 64 wide): 8 waves, ONE workgroup per CU, a 256 x (TN*32)
// output tile = 256 consecutive pixels (whole image rows / whole small images) x BN output channels.
// The implicit-GEMM loader of gemm_u_kernel (gemm_u.hip) stages the activation operand once per FILTER TAP (128 rows x 128 B per K tile next to 160
// weight rows: 36 KB of LDS-DMA per 128x160x64 multiply, and the DMA path -- about 53 GB/s per CU -- bounds it). Here a
// 64-channel chunk of the tile's input pixels INCLUDING the one-pixel halo is staged once ((R+2) x (W+2) rows of 128 B,
// 324-400 rows for the shapes below) and the nine taps are walked inside LDS: the fragment read of tap (ky, kx) is the same
// read shifted by ky (W+2) + kx halo rows. Per 256x160x64 multiply the DMA then brings one 20 KB weight tile plus 1/9 of a
// halo: 2.5x fewer bytes per FLOP.
//   LDS: two halo buffers (448 rows each = 7 DMA passes of 64 rows) + two weight slots.
//   K order inside a work item: chunk major, taps inside (weights stay [O][tap][I]: the tap only moves the SGPR offset).
//   Per (chunk, tap):  vmcnt(0) -> barrier -> DMA of the next weight tile + ONE pass of the next chunk's halo (taps 0..6)
//                      -> fragment reads + 40 MFMAs per wave.
//   Split-K splits by chunks and goes through the same fp32 slabs + splitk_reduce_kernel (gemm.hip) as gemm_u_kernel.
// GN = true (round 6): GroupNorm-apply + SiLU as the conv's prologue (reference openaimodel.py:212-232: GroupNorm32 -> SiLU -> conv).
// The RAW tensor is staged; every lane then normalises, in LDS, exactly the 16-byte piece its own DMA wrote (pass p of the next
// chunk is issued with tap p, has landed behind tap p + 1's vmcnt(0) and is rewritten during tap p + 1: no extra barrier, the
// chunk is first read two or more barriers later), from the chunk's 64 x (a, c) coefficients that one more 512-byte DMA brings
// into LDS beside the halo. Padding pixels never pass through the transform and stay zero, as the reference pads the ACTIVATED
// tensor. An item's first chunk (all seven passes issued at once by begin_item) is rewritten in front of its first barrier.
template <int TN, int NW, bool GN = false>
__global__ void __launch_bounds__(NW * 64, 1)
conv_halo_kernel(AOperand A, const bf16* __restrict__ W, int M, int N, int K, Epilogue E, float* __restrict__ ws, HaloDesc hd) {
    constexpr int NT = NW * 64;
    constexpr int RPP = NT / 8;                 // rows per DMA pass (one 128-byte row per 8 lanes)
    constexpr int TM = 32 / NW;                 // 16-row fragments per wave: NW/2 waves along M, 2 along N
    constexpr int BM = 256;
    constexpr int BN = TN * 32;
    constexpr int HROWS = 448;
    constexpr int HPASS = HROWS / RPP;          // halo DMA passes
    constexpr int HPT = (HPASS + 6) / 7;        // halo passes issued with each of the taps 0..6
    constexpr int HBUF = HROWS * 128;           // bytes per halo buffer
    constexpr int WSLOT = BN * 128;
    constexpr int WP = (BN + RPP - 1) / RPP;    // weight DMA passes; the last one is partial when BN % RPP != 0
    constexpr int WREM = BN % RPP;
    constexpr unsigned SENT = 0x80000000u;
    constexpr int COEF0 = 2 * HBUF + 2 * WSLOT;  // GN: two 1 KiB coefficient slots behind the weight slots (a DMA writes 64 x 16 B)
    static_assert(HPASS * RPP == HROWS && HPT * 7 >= HPASS && WREM % 8 == 0, "loader geometry");
    static_assert(!GN || (HPT == 1 && HPASS == 7), "the prologue rewrites pass p of the next chunk during tap p + 1");

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
    // The halo buffer is read at nine different row shifts (the filter taps), so its swizzle has to stay conflict free under any
    // shift: chunk ^= row & 6 does (a lane group of ds_read_b128 mixes rows {0-3, 12-15} of one 16-byte column with rows {4-11} of the
    // next; the column's low bit then tells the two sets apart and row mod 8 separates the rows inside each, whatever the first row
    // is). With the (row >> 1) & 7 swizzle of the aligned tiles only shifts that are multiples of 4 rows are conflict free: PMC
    // showed 23-25 % of this kernel's LDS cycles as bank conflicts (profiles/r3_final/pmc_mfma_report.txt), on the port that bounds it.
    const unsigned chb_h = (((t & 7) ^ (r0 & 6)) * 16);                  // (halo rows of a DMA pass: h = pass * 64 + r0)
    const int Cin = A.C0 + A.C1;

    const int Wd = 1 << hd.lgW, Hd = 1 << hd.lgH;
    const int R = BM >> hd.lgW;                 // image rows per tile
    const int lgHB = min(hd.lgH, 8 - hd.lgW);   // rows per halo block: a tile is R / HB whole images, or HB = R rows of one
    const int HB = 1 << lgHB;
    const int W2 = Wd + 2;
    const int blkrows = (HB + 2) * W2;
    const int NH = (R >> lgHB) * blkrows;       // halo rows in use (<= 400)

    const __amdgpu_buffer_rsrc_t ra0 = __builtin_amdgcn_make_buffer_rsrc((void*)A.p0, 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra1 = __builtin_amdgcn_make_buffer_rsrc((void*)(A.p1 ? A.p1 : A.p0), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, 0x80000000u, 0x00020000);

    // ---- halo row h = pass * RPP + r0 of a tile  <->  source pixel (first pixel of the tile) + hrel, if it is a real pixel: not a
    // left / right padding column, not beyond NH, not above / below the image (whole-image blocks: always padding there; a block
    // of R rows inside an image: padding only when the tile starts at the top / ends at the bottom of its image).
    // Recomputed per DMA pass (one pass per tile in the steady state) with multiply-shift divisions -- ceil(2^22 / d) is exact for
    // h < 2^22 / d, i.e. for every h < 448 with d <= 400 (a 16-bit reciprocal is NOT: 395 * ceil(65536 / 396) >> 16 = 1) -- rather
    // than kept in seven registers that the 256-register budget does not have. tests/test_host_cpu.py restates this index math.
    const unsigned inv_w2 = ((1u << 22) + W2 - 1) / W2, inv_blk = ((1u << 22) + blkrows - 1) / blkrows;
    // fragment rows: pixel p of the tile sits at halo row hr (tap (0,0)); tap (ky, kx) adds ky * W2 + kx. A wave's TM * 16 pixels lie
    // inside one halo block (a block has >= 64 pixels), so fragment i is fragment 0 plus a wave-uniform number of halo rows:
    // 16 pixels further along the image row, wrapping into the next halo row(s) every Wd pixels
    int hr00;
    {
        const int p = wm * TM * 16 + l15;
        const int blk = p >> (lgHB + hd.lgW);
        const int yl = (p >> hd.lgW) & (HB - 1);
        const int x = p & (Wd - 1);
        hr00 = blk * blkrows + yl * W2 + x;
    }
    auto hr_delta = [&](int i) -> int {   // halo rows from fragment 0 to fragment i (scalar): the wave's first pixel is a multiple
        const int px = i * 16;            // of 64, so x + (px mod Wd) never carries into the next image row
        return (px >> hd.lgW) * W2 + (px & (Wd - 1));
    };
    const int foff0 = l15 * 128 + (((q) ^ (l15 >> 1)) << 4);
    const int foff1 = l15 * 128 + (((q + 4) ^ (l15 >> 1)) << 4);
    const int wrow0 = wn * TN * 16 * 128;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

    // ---- work item state
    int m0 = 0, c_tn = 0, c_z = 0;
    bool top_ok = false, bot_ok = false;
    unsigned vw0 = SENT;              // byte offset of this lane's chunk of weight row (tile's first row + r0); pass i adds i * RPP rows
    auto setup = [&](int item) {
        const int tile = item / hd.splits;
        c_z = item - tile * hd.splits;
        const int tm = tile / hd.tiles_n;
        c_tn = tile - tm * hd.tiles_n;
        m0 = tm * BM;
        const int y0 = (m0 >> hd.lgW) & (Hd - 1);
        top_ok = y0 != 0;
        bot_ok = y0 + HB != Hd;
        vw0 = (unsigned)((c_tn * BN + r0) * K) * 2u + chb;     // N % BN == 0 (host): every weight row of the tile exists
    };
    auto issue_halo = [&](int p, int cc_, int hb_) {     // pass p of the 64-channel chunk at channel cc into halo buffer hb
        const int cc = __builtin_amdgcn_readfirstlane(cc_);
        const int hb = __builtin_amdgcn_readfirstlane(hb_);
        const bool first = cc < A.C0;
        const unsigned ld2 = (unsigned)(first ? A.ld0 : A.ld1) * 2u;
        const int soff = (first ? cc : cc - A.C0) * 2;
        int h = p * RPP + r0;
        // GN: the row map really is recomputed per pass -- without this hipcc hoists the seven item-invariant (pixel, mask) pairs out of
        // the chunk loop, and with the prologue's registers on top of the accumulators they no longer fit (spills inside the K loop)
        if constexpr (GN) asm volatile("" : "+v"(h));
        const int blk = (int)(((unsigned)h * inv_blk) >> 22);
        const int rem = h - blk * blkrows;
        const int hy = (int)(((unsigned)rem * inv_w2) >> 22);
        const int hx = rem - hy * W2;
        const bool ok = h < NH && hx >= 1 && hx <= Wd && (hy != 0 || top_ok) && (hy != HB + 1 || bot_ok);
        const int hrel = ((blk << lgHB) + hy - 1) * Wd + hx - 1;
        const unsigned va = ok ? __umul24((unsigned)(m0 + hrel), ld2) + chb_h : SENT;
        unsigned char* dst = smem + hb * HBUF + (p * RPP + wave * 8) * 128;
        if (first) GL_BLDS16(ra0, dst, va, soff);
        else GL_BLDS16(ra1, dst, va, soff);
    };
    auto issue_w = [&](int tap, int cc_, int ws_) {      // weight tile of (tap, chunk) into weight slot ws
        const int cc = __builtin_amdgcn_readfirstlane(cc_);
        const int wsl = __builtin_amdgcn_readfirstlane(ws_);
        const int soff = (tap * Cin + cc) * 2;
        unsigned char* dst = smem + 2 * HBUF + wsl * WSLOT + wave * 1024;
#pragma unroll
        for (int i = 0; i < WP; ++i) {
            if (WREM && i == WP - 1 && wave >= WREM / 8) continue;   // wave-uniform
            GL_BLDS16(rw, dst + i * RPP * 128, vw0, soff + i * RPP * K * 2);
        }
    };

    // GN: the 64 x (a, c) coefficients of channel chunk cc of the tile's sample (a 256-pixel tile lies inside one image: H W >= 256,
    // checked on the host) into coefficient slot hb: 512 contiguous bytes, lanes 0..31 of wave 0 (the other lanes write zeros)
    auto issue_coef = [&](int cc_, int hb_) {
        if constexpr (GN) {
            if (wave == 0) {
                const int cc = __builtin_amdgcn_readfirstlane(cc_);
                const int hb = __builtin_amdgcn_readfirstlane(hb_);
                const int smp = m0 >> (hd.lgW + hd.lgH);
                // (flat-address DMA: a fourth buffer descriptor would cost four SGPRs this kernel does not have; lanes 32..63 fetch the
                // same 512 bytes again into the slot's unused upper half)
                // scalar base + 32-bit lane offset, the lane id taken from v_mbcnt on the spot: any lane constant that lives across the
                // tap loop for this one instruction is a register the loop does not have (it was spilled, and its reload drained the DMA)
                unsigned lo;
                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lo));
                lo = (lo & 31u) * 16u;
                GL_GLDS16(reinterpret_cast<const unsigned char*>(A.gn) + (size_t)(unsigned)((smp * Cin + cc) * 8) + lo, smem + COEF0 + hb * 1024);
            }
        }
    };
    // GN: rewrite the 16-byte piece this lane's DMA of pass p wrote into halo buffer hb (8 channels of halo row p RPP + r0) as
    // bf16(silu(x a + c)) -- the arithmetic of gn_apply_kernel (norm.hip), so the conv multiplies the very values the two-pass form
    // would have read back from HBM. Lanes whose halo row is padding hold zeros and skip. LDS accesses in asm: a compiler-visible
    // LDS access behind an LDS-DMA issue would drain vmcnt(0) (see lds_rd16).
    // pass = PC::value + prt: the compile-time part rides in the DS instructions' offset field (a per-pass address in a VGPR is
    // loop invariant, hipcc hoists all seven out of the chunk loop and spills them), prt is the run-time pass of the first-chunk loop.
    // Three steps so that the caller can put matrix work between them: xf_read (five LDS reads), xf_math (after the caller's lgkmcnt
    // wait; branch-free: lanes whose halo row is padding compute on their zeros and select zero -- MFMAs can then be interleaved), xf_write.
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    struct XF { f32x4 a0, a1, c0, c1; };
    struct XP1 { u32x4 v; unsigned addr; bool ok; };
    // rsh: 0 = the piece this lane's own DMA wrote (a row shift reaches another wave's piece: valid behind a barrier only)
    auto xf_piece = [&](auto PC, int prt, int hb, int rsh, XP1& x) {
        constexpr int PI = decltype(PC)::value;
        int h = (PI + prt) * RPP + r0 + rsh;
        asm volatile("" : "+v"(h));       // (recomputed per call, see issue_halo)
        const int blk = (int)(((unsigned)h * inv_blk) >> 22);
        const int rem = h - blk * blkrows;
        const int hy = (int)(((unsigned)rem * inv_w2) >> 22);
        const int hx = rem - hy * W2;
        x.ok = h < NH && hx >= 1 && hx <= Wd && (hy != 0 || top_ok) && (hy != HB + 1 || bot_ok);
        x.addr = lds0 + hb * HBUF + (prt * RPP + rsh) * 128 + t * 16;
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(x.v) : "v"(x.addr), "n"(PI * RPP * 128));
    };
    auto xf_coef = [&](int hb, XF& x) {
        const unsigned caddr = lds0 + COEF0 + hb * 1024 + (((t & 7) ^ (r0 & 6)) << 6);
        asm volatile("ds_read_b128 %0, %1" : "=v"(x.a0) : "v"(caddr));
        asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(x.c0) : "v"(caddr));
        asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(x.a1) : "v"(caddr));
        asm volatile("ds_read_b128 %0, %1 offset:48" : "=v"(x.c1) : "v"(caddr));
    };
    auto xf_wait = [&](XF& x, XP1& p) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(p.v), "+v"(x.a0), "+v"(x.a1), "+v"(x.c0), "+v"(x.c1)); };
    auto xf_math = [&](const XF& x, const XP1& p) -> u32x4 {
        const float a[8] = {x.a0[0], x.a0[1], x.a0[2], x.a0[3], x.a1[0], x.a1[1], x.a1[2], x.a1[3]};
        const float c[8] = {x.c0[0], x.c0[1], x.c0[2], x.c0[3], x.c1[0], x.c1[1], x.c1[2], x.c1[3]};
        union { u32x4 u; bf16 e[8]; } o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned w = p.v[i];
            const float x0 = __uint_as_float(w << 16), x1 = __uint_as_float(w & 0xffff0000u);
            o.e[2 * i] = f2bf(silu_f(fmaf(x0, a[2 * i], c[2 * i])));
            o.e[2 * i + 1] = f2bf(silu_f(fmaf(x1, a[2 * i + 1], c[2 * i + 1])));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) o.u[i] = p.ok ? o.u[i] : 0u;
        return o.u;
    };
    auto xf_write = [&](auto PC, const XP1& p, u32x4 o) {
        constexpr int PI = decltype(PC)::value;
        asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(p.addr), "v"(o), "n"(PI * RPP * 128));
    };

    f32x4 acc[TM][TN];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    };

    // One (chunk, tap) tile: all 2 x (TM + TN) fragment reads go out at once (every wave of the workgroup reads at the same time and
    // keeps the LDS port full), the MFMAs of K step 0 start when its fragments are in, and hipcc is left to schedule the rest: it
    // runs the MFMAs of K step 1 behind the NEXT tile's barrier and DMA issue. Hand-placed alternatives were all slower on
    // MI355X (profiles/r2_final/halo_schedules.txt): the two wave groups half a tile out of phase (each wave gets one
    // ds_read_b128 out per ~45 clocks, four waves cannot fill the port), activation fragments of the next tile read ahead with
    // the reads interleaved between the MFMA rows, and four 128x80 waves (one per SIMD: nothing to issue while one waits).
    auto compute = [&](int tapoff, int hb, int wsl) {
        const unsigned hbase = lds0 + hb * HBUF;
        const unsigned wbase = lds0 + 2 * HBUF + wsl * WSLOT + wrow0;
        unsigned ax0[TM], ax1[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const unsigned hr = (unsigned)(hr00 + hr_delta(i) + tapoff);
            ax0[i] = hbase + hr * 128u + (((unsigned)q ^ (hr & 6u)) << 4);
            ax1[i] = ax0[i] ^ 64u;    // k-step 1 = chunks 4..7: (q + 4) ^ s = (q ^ s) ^ 4
        }
        const unsigned aw0 = wbase + foff0, aw1 = wbase + foff1;
        bf16x8 xa[TM], wa[TN], xb[TM], wb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) lds_rd16<0>(xa[i], ax0[i]);
        lds_rd16_n<TN, 2048>(wa, aw0);
#pragma unroll
        for (int i = 0; i < TM; ++i) lds_rd16<0>(xb[i], ax1[i]);
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
        asm volatile("s_waitcnt lgkmcnt(0)");
        pin_regs(xb);
        pin_regs(wb);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j], xb[i], acc[i][j], 0, 0, 0);
    };

    // GN variant: the same tile with K step 1 deferred BY HAND (what hipcc does by itself above: its MFMAs sink behind the next barrier
    // down to the first inline asm). Written out because the prologue's arithmetic has to sit between those MFMAs: k1_mfma(lo, hi)
    // issues MFMAs lo..hi-1 of the pending K step 1 (fragments xbp / wbp stay in registers across the barrier).
    bf16x8 xbp[TM], wbp[TN];
    auto k1_mfma = [&](auto LO, auto HI) {
#pragma unroll
        for (int ij = decltype(LO)::value; ij < decltype(HI)::value; ++ij)
            acc[ij / TN][ij % TN] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wbp[ij % TN], xbp[ij / TN], acc[ij / TN][ij % TN], 0, 0, 0);
    };
    auto compute_k0 = [&](int tapoff, int hb, int wsl) {   // fragment reads of both K steps, K step 0's MFMAs; K step 1 stays pending
        const unsigned hbase = lds0 + hb * HBUF;
        const unsigned wbase = lds0 + 2 * HBUF + wsl * WSLOT + wrow0;
        unsigned ax0[TM], ax1[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const unsigned hr = (unsigned)(hr00 + hr_delta(i) + tapoff);
            ax0[i] = hbase + hr * 128u + (((unsigned)q ^ (hr & 6u)) << 4);
            ax1[i] = ax0[i] ^ 64u;
        }
        const unsigned aw0 = wbase + foff0, aw1 = wbase + foff1;
        bf16x8 xa[TM], wa[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) lds_rd16<0>(xa[i], ax0[i]);
        lds_rd16_n<TN, 2048>(wa, aw0);
#pragma unroll
        for (int i = 0; i < TM; ++i) lds_rd16<0>(xbp[i], ax1[i]);
        lds_rd16_n<TN, 2048>(wbp, aw1);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(TM + TN));
        pin_regs(xa);
        pin_regs(wa);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[j], xa[i], acc[i][j], 0, 0, 0);
        asm volatile("s_waitcnt lgkmcnt(0)");
        pin_regs(xbp);
        pin_regs(wbp);
        __builtin_amdgcn_sched_barrier(0);
    };

    auto store_row = [&](int m, int n0, float (&v)[4]) {   // EPI_ROWMAJOR only (checked on the host)
        if (E.act == ACT_SILU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
        }
        if (E.out_f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(E.out) + (size_t)m * E.ldo + n0) = make_float4(v[0], v[1], v[2], v[3]);
        else store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + n0, v);
    };
    auto epilogue = [&]() {
        const int mrow = m0 + wm * TM * 16 + l15;
        const int ncol = c_tn * BN + wn * TN * 16 + q * 4;
        if (hd.splits > 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n0 = ncol + j * 16;
                    *reinterpret_cast<float4*>(ws + ((size_t)c_z * M + m) * N + n0) =
                        make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                }
            }
            return;
        }
        float4 bj[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            bj[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (E.bias) bj[j] = *reinterpret_cast<const float4*>(E.bias + ncol + j * 16);
        }
        if (E.bias2) {  // + broadcast per-sample bias (ResBlock time embedding); never combined with a residual
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
                const float* b2p = E.bias2 + (size_t)div_rpb(E, m) * E.bias2_ld + ncol;
                float4 b2[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) b2[j] = *reinterpret_cast<const float4*>(b2p + j * 16);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    float v[4] = {acc[i][j][0] + bj[j].x + b2[j].x, acc[i][j][1] + bj[j].y + b2[j].y,
                                  acc[i][j][2] + bj[j].z + b2[j].z, acc[i][j][3] + bj[j].w + b2[j].w};
                    store_row(m, ncol + j * 16, v);
                }
            }
        } else if (E.res) {
            const float g = E.gate ? *E.gate : 1.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
                uint2 rs[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) rs[j] = *reinterpret_cast<const uint2*>(E.res + (size_t)m * E.ldres + ncol + j * 16);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n0 = ncol + j * 16;
                    U2BF4 r;
                    r.u = rs[j];
                    float v[4] = {acc[i][j][0] + bj[j].x, acc[i][j][1] + bj[j].y, acc[i][j][2] + bj[j].z, acc[i][j][3] + bj[j].w};
                    if (E.act == ACT_SILU) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = bf2f(r.e[e]) + g * v[e];
                    if (E.out_f32) {
                        *reinterpret_cast<float4*>(reinterpret_cast<float*>(E.out) + (size_t)m * E.ldo + n0) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
                        store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)m * E.ldo + n0, v);
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow + i * 16;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    float v[4] = {acc[i][j][0] + bj[j].x, acc[i][j][1] + bj[j].y, acc[i][j][2] + bj[j].z, acc[i][j][3] + bj[j].w};
                    store_row(m, ncol + j * 16, v);
                }
            }
        }
    };

    // ---- persistent loop over work items. Per (chunk, tap), one barrier:
    //   vmcnt(0) -> barrier -> DMA of the next weight tile (+ HPT passes of the next chunk's halo, taps 0..6) -> compute
    int item = blockIdx.x;
    if (item >= hd.n_items) return;
    int hb = 0, wsl = 0;              // halo buffer / weight slot of the tile about to be multiplied
    int cc = 0, cc_end = 0;
    auto begin_item = [&](int it) {   // prologue DMA of an item: the whole first halo + the first weight tile
        setup(it);
        cc = c_z * hd.chunks_per_split * 64;
        cc_end = min(Cin, cc + hd.chunks_per_split * 64);
#pragma unroll
        for (int p = 0; p < HPASS; ++p) issue_halo(p, cc, hb);
        issue_coef(cc, hb);
        issue_w(0, cc, wsl);
    };
    begin_item(item);
    zero_acc();
    for (;;) {
        hb = __builtin_amdgcn_readfirstlane(hb);
        wsl = __builtin_amdgcn_readfirstlane(wsl);
        cc = __builtin_amdgcn_readfirstlane(cc);
        cc_end = __builtin_amdgcn_readfirstlane(cc_end);
        const bool next_chunk = cc + 64 < cc_end;
        auto one_tap = [&](auto TC) {
            constexpr int tap = decltype(TC)::value;
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this tile's weights (tap 0: and the chunk's halo) have landed
            bool first_chunk = false;
            if constexpr (GN) {
                first_chunk = tap == 0 && cc == c_z * hd.chunks_per_split * 64;
                if (tap == 0 && first_chunk) {   // an item's first chunk (still raw): all seven pieces, before anyone reads them
                    __builtin_amdgcn_s_barrier();      // (the coefficients are wave 0's DMA: landed for everybody only behind a barrier)
                    XF x;
                    xf_coef(hb, x);
#pragma unroll 1
                    for (int p = 0; p < HPASS; ++p) {
                        XP1 pc;
                        xf_piece(std::integral_constant<int, 0>{}, p, hb, 0, pc);
                        xf_wait(x, pc);
                        xf_write(std::integral_constant<int, 0>{}, pc, xf_math(x, pc));
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)");
                }
            }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (tap < 8) issue_w(tap + 1, cc, wsl ^ 1);
            else if (next_chunk) issue_w(0, cc + 64, wsl ^ 1);
            if (tap < 7 && next_chunk) {
#pragma unroll
                for (int pp = 0; pp < HPT; ++pp)
                    if (tap * HPT + pp < HPASS) issue_halo(tap * HPT + pp, cc + 64, hb ^ 1);
                if (tap == 0) issue_coef(cc + 64, hb ^ 1);
            }
            if constexpr (GN) {
                constexpr int NMF = TM * TN, HALF = NMF / 2;
                using I0 = std::integral_constant<int, 0>;
                using IH = std::integral_constant<int, HALF>;
                using IN = std::integral_constant<int, NMF>;
                constexpr int PX = (tap >= 1 && tap <= HPASS) ? tap - 1 : -1;   // the pass whose piece is rewritten during this tap
                if (PX >= 0 && next_chunk) {
                    // the piece of pass tap - 1 (landed behind this tap's vmcnt(0)): its reads fly under the first half of the pending
                    // MFMAs, its arithmetic is interleaved with the second half
                    constexpr int PXC = PX >= 0 ? PX : 0;
                    XF x;
                    XP1 p1;
                    xf_piece(std::integral_constant<int, PXC>{}, 0, hb ^ 1, 0, p1);
                    xf_coef(hb ^ 1, x);
                    k1_mfma(I0{}, IH{});
                    xf_wait(x, p1);
                    const u32x4 o = xf_math(x, p1);
                    k1_mfma(IH{}, IN{});
#pragma unroll
                    for (int g = 0; g < NMF - HALF; ++g) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
                        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);   // eight VALU
                    }
                    xf_write(std::integral_constant<int, PXC>{}, p1, o);
                } else if (!first_chunk) {
                    k1_mfma(I0{}, IN{});
                }
                compute_k0((tap / 3) * W2 + tap % 3, hb, wsl);
            } else {
                compute((tap / 3) * W2 + tap % 3, hb, wsl);
            }
            wsl ^= 1;
        };
        one_tap(std::integral_constant<int, 0>{}); one_tap(std::integral_constant<int, 1>{}); one_tap(std::integral_constant<int, 2>{});
        one_tap(std::integral_constant<int, 3>{}); one_tap(std::integral_constant<int, 4>{}); one_tap(std::integral_constant<int, 5>{});
        one_tap(std::integral_constant<int, 6>{}); one_tap(std::integral_constant<int, 7>{}); one_tap(std::integral_constant<int, 8>{});
        cc += 64;
        hb ^= 1;
        if (cc < cc_end) continue;
        if constexpr (GN) k1_mfma(std::integral_constant<int, 0>{}, std::integral_constant<int, TM * TN>{});   // the item's last K step 1
        // item done: start the next item's DMA (into the halo buffer / weight slot not read by the last tile), then store
        const int done_m0 = m0, done_tn = c_tn, done_z = c_z;
        item += gridDim.x;
        const bool more = item < hd.n_items;
        if (more) begin_item(item);
        {   // the epilogue addresses the finished item
            const int nm0 = m0, ntn = c_tn, nz = c_z;
            m0 = done_m0; c_tn = done_tn; c_z = done_z;
            epilogue();
            m0 = nm0; c_tn = ntn; c_z = nz;
        }
        if (!more) break;
        zero_acc();
    }
}

namespace {
// (always more than 48 KiB of LDS: launch_lds sets the attribute at the first launch of each instantiation)
constexpr size_t halo_lds(int tn, bool gn) { return 2 * 7 * 64 * 128 + 2 * tn * 32 * 128 + (gn ? 2048 : 0); }
}  // namespace

int gemm_exec_halo(const Launch& l, const GemmPlan& p) {
    switch (p.gn * 100 + p.tm * 10 + p.tn) {
        case 185: return l.run<conv_halo_kernel<5, 8, true>>(p.grid, 512, halo_lds(5, true), p.halo);
        case 184: return l.run<conv_halo_kernel<4, 8, true>>(p.grid, 512, halo_lds(4, true), p.halo);
        case 85: return l.run<conv_halo_kernel<5, 8>>(p.grid, 512, halo_lds(5, false), p.halo);
        case 84: return l.run<conv_halo_kernel<4, 8>>(p.grid, 512, halo_lds(4, false), p.halo);
    }
    return gemm_unknown_tile();
}

}  // namespace gl
