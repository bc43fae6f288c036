// conv8_kernel: the stride-1 3x3 convolution of the deepest UNet level (8 x 8 images, 1280-2560 input channels), which stages each
// image once per 64-channel chunk and walks the nine filter taps inside LDS. Its header comment below is the description of this unit.
#include "gemm_impl.h"

namespace gl {

// ---------------------------------------------------------------------------------------------------------------------------
// At M = 512 (batch 8) the 256 x 160 tiles of conv_halo_kernel (gemm_halo.hip) are 16 tiles, and the 64 x 160 tiles of gemm_u_kernel
// (gemm_u.hip) re-stage 8/9-identical pixels for every tap: 47 FLOP per staged byte, and the operand path bounds the launch. Here a
// workgroup (8 waves, one per CU) owns FOUR samples = 256 output rows, a NARROW column tile (BN = 64 or 80) and a range of 64-channel
// chunks, so that 2 row groups x 20 (16) column tiles x 5-8 K splits fill the chip:
//   pixels   the 4 x 64 pixels of a chunk are staged once into a zero-framed image of 10 halo rows per image row; the bottom pad row of
//            a sample is the top pad row of the next (370 rows of 128 B). The frame is zeroed once per workgroup: DMA only ever
//            writes pixel rows. Tap (ky, kx) of pixel (y, x) is halo row (y + ky) 10 + x + kx of its sample: a shifted read.
//   weights  [O][tap][I] as packed for A_CONV3; a stage is the three taps of one filter row ky for the chunk (3 BN rows of 128 B),
//            two stage slots, streamed by LDS-DMA one stage ahead.
//   per stage (chunk, ky):  vmcnt(0) -> barrier -> DMA of the next stage's weights (ky = 0: and of the next chunk's pixels into the
//            other image buffer) -> 3 taps x 2 K steps of fragment reads + 2 x TNF MFMAs (16x16x32) per wave.
//   waves    8 along M: wave w multiplies rows [32 (w & 1), +32) of sample w >> 1 by all BN columns (2 x TNF accumulators).
//   swizzle  a fragment is 2 image rows x 8 pixels; halo rows of equal x in consecutive image rows are 10 apart, so the 16-byte chunk
//            index is XOR-ed with 2 ((X >> 1) & 3), X = halo column: under every tap shift the sixteen lanes of a ds_read_b128 group
//            cover the sixteen 16-byte slots of the 256-byte bank row once (the parity of X picks the half, four consecutive X pairs
//            the even / odd slots). Weight rows keep the (row >> 1) & 7 swizzle of the aligned tiles.
//   output   K split: fp32 slabs [z][M][N] for splitk_reduce_kernel (gemm.hip), which owns every epilogue; unsplit: epi_finish4.
//            Rows of samples beyond the batch (a partly empty last group) are staged as zeros and never stored.
// Every output element is one fp32 accumulation over (chunk, ky, kx, channel) in that order inside a split, whatever the grid, the
// group a sample falls in or the batch: a sample's bits depend on (BN, K split) alone. No atomics, no cross-workgroup waits.
template <int TNF>
__global__ void __launch_bounds__(512, 1)
conv8_kernel(AOperand A, const bf16* __restrict__ W, int M, int N, int K, Epilogue E, float* __restrict__ ws, Conv8Desc cd) {
    constexpr int BN = TNF * 16;
    constexpr int HSTR = 90;                    // halo rows per sample (9 image rows of 10: the lower pad row belongs to the next sample)
    constexpr int HROWS = 4 * HSTR + 10;
    constexpr int HBUF = HROWS * 128;           // bytes per image buffer
    constexpr int WROWS = 3 * BN;               // weight rows per stage: [kx][column]
    constexpr int WSLOT = WROWS * 128;
    constexpr int WP = (WROWS + 63) / 64;       // weight DMA passes of 64 rows; the last one is partial for BN = 80 (wave-uniform)
    constexpr unsigned SENT = 0x80000000u;
    static_assert(WROWS % 8 == 0 && BN % 8 == 0, "a wave's eight DMA rows share one kx");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15;
    const int q = lane >> 4;
    const int Cin = A.C0 + A.C1;
    const int nchunks = Cin >> 6;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

    const __amdgpu_buffer_rsrc_t ra0 = __builtin_amdgcn_make_buffer_rsrc((void*)A.p0, 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra1 = __builtin_amdgcn_make_buffer_rsrc((void*)(A.p1 ? A.p1 : A.p0), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, 0x80000000u, 0x00020000);

    // ---- the zero frame, once: both image buffers entirely (the DMA passes below rewrite the pixel rows only)
    for (int o = t * 16; o < 2 * HBUF; o += 512 * 16) *reinterpret_cast<uint4*>(smem + o) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    // ---- loader lane constants. Pixels: pass p = sample p of the group, wave = image row, lane >> 3 = x, lane & 7 = 16-byte slot
    const int px = lane >> 3;
    const unsigned chb_h = (unsigned)(((lane & 7) ^ ((((px + 1) >> 1) & 3) << 1)) * 16);
    // weights: row R = pass * 64 + (t >> 3) of the stage = (kx, column) = (R / BN, R % BN)
    int w_kx[WP], w_n[WP];
#pragma unroll
    for (int i = 0; i < WP; ++i) {
        const int R = i * 64 + (t >> 3);
        w_kx[i] = R / BN;
        w_n[i] = R - w_kx[i] * BN;
    }

    // ---- fragment lane constants: pixel (y, x) = (4 half + 2 i + (l15 >> 3), l15 & 7) of sample sm sits at halo row
    // sm 90 + (y + ky) 10 + x + kx for tap (ky, kx); the swizzle key follows the halo column x + kx
    const int sm = wave >> 1, half = wave & 1;
    unsigned afrag[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        const int X = (l15 & 7) + kx;
        const int hr = sm * HSTR + (half * 4 + (l15 >> 3)) * 10 + X;
        afrag[kx] = lds0 + (unsigned)(hr * 128 + ((q ^ (((X >> 1) & 3) << 1)) << 4));
    }
    const unsigned wfrag = lds0 + 2 * HBUF + (unsigned)(l15 * 128 + ((q ^ (l15 >> 1)) << 4));

    f32x4 acc[2][TNF];

    for (int item = blockIdx.x; item < cd.n_items; item += gridDim.x) {
        // ---- item -> (row group, column tile, K split). The row groups of one (column tile, split) read the same weights: they are
        // eight items apart, i.e. on the same XCD (workgroups go round the eight XCDs), and the second finds them in that L2
        const int n_u = cd.tiles_n * cd.splits;
        const int G = 8 * cd.tiles_m;
        const int g = item / G, rem = item - g * G;
        const int width = min(8, n_u - g * 8);
        const int tm = rem / width;
        const int u = g * 8 + (rem - tm * width);
        const int c_tn = u / cd.splits;
        const int c_z = u - c_tn * cd.splits;
        const int m0 = tm * 256;
        const int ch0 = c_z * cd.chunks_per_split;
        const int ch1 = min(nchunks, ch0 + cd.chunks_per_split);
        const int nstages = (ch1 - ch0) * 3;

        unsigned vw[WP];   // byte offset of this lane's 16 bytes of weight row (column, kx); the stage adds (3 ky Cin + channel) * 2
#pragma unroll
        for (int i = 0; i < WP; ++i)
            vw[i] = ((unsigned)(c_tn * BN + w_n[i]) * (unsigned)K + (unsigned)(w_kx[i] * Cin)) * 2u + (unsigned)(((t & 7) ^ ((w_n[i] >> 1) & 7)) * 16);

        auto issue_pixels = [&](int ch_, int hb_) {      // the four samples' chunk ch into image buffer hb
            const int ch = __builtin_amdgcn_readfirstlane(ch_);
            const int hb = __builtin_amdgcn_readfirstlane(hb_);
            const int cc = ch * 64;
            const bool first = cc < A.C0;
            const unsigned ld2 = (unsigned)(first ? A.ld0 : A.ld1) * 2u;
            const int soff = (first ? cc : cc - A.C0) * 2;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int m = m0 + p * 64 + (t >> 3);
                const unsigned va = m < M ? (unsigned)m * ld2 + chb_h : SENT;
                unsigned char* dst = smem + hb * HBUF + (p * HSTR + (wave + 1) * 10 + 1) * 128;
                if (first) GL_BLDS16(ra0, dst, va, soff);
                else GL_BLDS16(ra1, dst, va, soff);
            }
        };
        auto issue_w = [&](int st_, int wsl_) {          // stage st = 3 (chunk - ch0) + ky into weight slot wsl
            const int st = __builtin_amdgcn_readfirstlane(st_);
            const int wsl = __builtin_amdgcn_readfirstlane(wsl_);
            const int dch = st / 3, ky = st - dch * 3;
            const int soff = (ky * 3 * Cin + (ch0 + dch) * 64) * 2;
            unsigned char* dst = smem + 2 * HBUF + wsl * WSLOT + wave * 1024;
#pragma unroll
            for (int i = 0; i < WP; ++i) {
                if (i * 64 + wave * 8 >= WROWS) continue;   // wave-uniform (BN = 80: the last pass has 48 rows)
                GL_BLDS16(rw, dst + i * 64 * 128, vw[i], soff);
            }
        };

        // One tap of the stage: every fragment read of both K steps goes out at once, K step 0 multiplies when its fragments are in
        auto tap = [&](auto KX, unsigned aoff, unsigned woff) {
            constexpr int kx = decltype(KX)::value;
            const unsigned ax0 = afrag[kx] + aoff, ax1 = ax0 ^ 64u;          // K step 1 = slots 4..7: (q + 4) ^ key = (q ^ key) ^ 4
            const unsigned aw0 = wfrag + woff + kx * BN * 128, aw1 = aw0 ^ 64u;
            bf16x8 xa[2], wa[TNF], xb[2], wb[TNF];
            lds_rd16<0>(xa[0], ax0);
            lds_rd16<2560>(xa[1], ax0);       // fragment 1: two image rows = 20 halo rows further
            lds_rd16_n<TNF, 2048>(wa, aw0);
            lds_rd16<0>(xb[0], ax1);
            lds_rd16<2560>(xb[1], ax1);
            lds_rd16_n<TNF, 2048>(wb, aw1);
            asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 + TNF));
            pin_regs(xa);
            pin_regs(wa);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TNF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[j], xa[i], acc[i][j], 0, 0, 0);
            asm volatile("s_waitcnt lgkmcnt(0)");
            pin_regs(xb);
            pin_regs(wb);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TNF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j], xb[i], acc[i][j], 0, 0, 0);
        };

#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TNF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        // every wave has left the previous item's last stage (its fragment reads were waited for): buffer 0 and slot 0 are free
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        issue_pixels(ch0, 0);
        issue_w(0, 0);
        int st = 0;
#pragma unroll 1
        for (int dch = 0; dch < ch1 - ch0; ++dch) {
            const int hb = dch & 1;
#pragma unroll 1
            for (int ky = 0; ky < 3; ++ky, ++st) {
                const int wsl = st & 1;
                __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this stage's weights (ky = 0 of a first chunk: and its pixels) have landed
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                // behind the barrier nobody reads the other weight slot (stage st - 1) or the other image buffer (chunk dch - 1) any more
                if (st + 1 < nstages) issue_w(st + 1, wsl ^ 1);
                if (ky == 0 && ch0 + dch + 1 < ch1) issue_pixels(ch0 + dch + 1, hb ^ 1);
                const unsigned aoff = (unsigned)(hb * HBUF + ky * 1280), woff = (unsigned)(wsl * WSLOT);
                tap(std::integral_constant<int, 0>{}, aoff, woff);
                tap(std::integral_constant<int, 1>{}, aoff, woff);
                tap(std::integral_constant<int, 2>{}, aoff, woff);
            }
        }

        // ---- store: lane (l15, q) holds row l15 of fragment i and columns 4 q .. 4 q + 3 of column fragment j
        const int mrow = m0 + sm * 64 + half * 32 + l15;
        const int ncol = c_tn * BN + q * 4;
        if (m0 + sm * 64 < M) {   // (wave-uniform: a sample beyond the batch was multiplied as zeros)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = mrow + i * 16;
#pragma unroll
                for (int j = 0; j < TNF; ++j) {
                    const int n0 = ncol + j * 16;
                    if (cd.splits > 1) {
                        *reinterpret_cast<float4*>(ws + ((size_t)c_z * M + m) * N + n0) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                    } else {
                        float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                        epi_finish4(E, m, n0, v);
                    }
                }
            }
        }
    }
}

namespace {
// (always more than 48 KiB of LDS: launch_lds sets the attribute at the first launch of each instantiation)
constexpr size_t conv8_lds(int tnf) { return 2 * 370 * 128 + 2 * 3 * tnf * 16 * 128; }
}  // namespace

int gemm_exec_conv8(const Launch& l, const GemmPlan& p) {
    switch (p.tn) {   // (tn: the column tile in units of 16 here)
        case 4: return l.run<conv8_kernel<4>>(p.grid, 512, conv8_lds(4), p.conv8);
        case 5: return l.run<conv8_kernel<5>>(p.grid, 512, conv8_lds(5), p.conv8);
    }
    return gemm_unknown_tile();
}

}  // namespace gl
