// The low-rank part of an adapted 3 x 3 conv in training, for gfx950 (kohya's conv_dim / LoCon form): y = conv(x, W) + b + s up(down(x)),
// s = alpha / r, down [r][Ci][3][3] (OIHW, the base conv's kernel size, stride and padding), up [Co][r] (1 x 1). W stays frozen and
// goes through Ctx::conv3; this unit adds the adapter term and forms the adapter's gradients over fp32 pixel rows [B H W][C]:
//   forward         t [Mo][r] = im2col(x) down^T                  y  += s t up^T          (lora_up, train_lora.hip)
//   data gradient   u [Mo][r] = dy up (lora_down, a_kr)            dx += s sum_tap u[the pixels that read this one through tap] down[:, :, tap]
//   weight grads    g_down = s u^T im2col(x)   (OIHW)              g_up = s dy^T t        (lora_wgrad)
// Three geometries, the ones Ctx::conv3 knows: 0 stride 1 pad 1 (ResBlock convs), 1 stride 2 pad 1 (Downsample, output H/2 x W/2),
// 2 stride 1 on the nearest-2x enlarged grid (Upsample, output 2H x 2W: output (oy, ox) reads source ((oy + ky - 1) >> 1,
// (ox + kx - 1) >> 1), zero when oy + ky - 1 or ox + kx - 1 leaves the enlarged grid). im2col is never written: a lane owns a pixel
// and walks the taps, reading its neighbour's row through L2, zeros where a tap leaves the image (also where the neighbouring row in
// memory belongs to the next image of the batch).
// The products run on the exact-fp32 MFMA with the lane maps of train_lora.hip (lane l, i = l & 15, q = l >> 4: A[row i][k = q],
// B[k = q][col i], D[row 4 q + reg][col i]). No atomics: the weight gradient is partial sums over chunks of output rows whose size
// depends on the shape alone (lora_wgrad_chunk_rows), added in ascending order by a second launch that writes OIHW.
#include "train_impl.h"

namespace gl {

using namespace train;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kRows = 64;        // pixel rows a workgroup of four waves handles at a time: 16 per wave (down, dgrad), 64 per stage (wgrad)
constexpr int kKc = 64;          // input channels staged per step of the down product
constexpr int kNc = 64;          // output columns per step of the data gradient; the column strip of a weight-gradient workgroup

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// as train_lora.hip: ld % 32 == 16 puts four consecutive k rows on four different groups of 16 banks
__host__ __device__ constexpr int lds_ld(int nt) { return (nt * 16) | 16; }

// The conv's grids: the input H x W, the output Ho x Wo
struct Geo { int geom, H, W, Ho, Wo; };

// The row of x that output pixel (b, oy, ox) reads through tap (ky, kx); -1: zero padding
__device__ __forceinline__ long long src_row(const Geo& g, int b, int oy, int ox, int ky, int kx) {
    int iy = (g.geom == 1 ? 2 * oy : oy) + ky - 1, ix = (g.geom == 1 ? 2 * ox : ox) + kx - 1;
    const int up = g.geom == 2 ? 1 : 0;
    if (iy < 0 || iy >= (g.H << up) || ix < 0 || ix >= (g.W << up)) return -1;
    iy >>= up;
    ix >>= up;
    return ((long long)b * g.H + iy) * g.W + ix;
}

// The output row that reads input pixel (b, py, px) through tap (ky, kx); -1: none. Geometry 2 has four candidates per tap, one per
// position (sub >> 1, sub & 1) of the pixel's 2 x 2 copies on the enlarged grid; the others have one (sub 0).
__device__ __forceinline__ long long reader_row(const Geo& g, int b, int py, int px, int ky, int kx, int sub) {
    int oy, ox;
    if (g.geom == 2) {
        oy = 2 * py + (sub >> 1) + 1 - ky;
        ox = 2 * px + (sub & 1) + 1 - kx;
    } else {
        oy = py + 1 - ky;
        ox = px + 1 - kx;
        if (g.geom == 1) {
            if ((oy | ox) & 1) return -1;       // (a negative odd value has its low bit set too)
            oy >>= 1;
            ox >>= 1;
        }
    }
    if (oy < 0 || oy >= g.Ho || ox < 0 || ox >= g.Wo) return -1;
    return ((long long)b * g.Ho + oy) * g.Wo + ox;
}

// T [Mo][r] = im2col(X) down^T: X [B H W][Ci], down [r][Ci][3][3]. lora_down_kernel with the contraction over (tap, ci): a workgroup
// owns 64 output pixels and all r columns (NT tiles of 16, zero-padded in LDS), wave w pixels 16 w .. 16 w + 15. Per tap and step of
// 64 channels down[:, k0 .. k0 + 63, tap] is staged in LDS as [k][j], read from its OIHW place, and a lane reads
// X[its pixel's neighbour][k0 + 16 jj + 4 q .. + 3] (jj = 0..3) as four float4, zeros for an out-of-image tap. Even and odd
// instructions accumulate separately, as there.
template <int NT>
__global__ void __launch_bounds__(256) lora_conv_down_kernel(const float* __restrict__ X, const float* __restrict__ A, Geo g, int Mo, int Ci, int r,
                                                             float* __restrict__ T) {
    constexpr int LD = lds_ld(NT);
    __shared__ float As[kKc * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int row = blockIdx.x * kRows + wave * 16 + i;
    const bool row_ok = row < Mo;
    const int m = row_ok ? row : 0, ox = m % g.Wo, oy = (m / g.Wo) % g.Ho, b = m / (g.Wo * g.Ho);
    f32x4 acc[2][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[0][t] = acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < 9; ++tap) {
        const long long src = row_ok ? src_row(g, b, oy, ox, tap / 3, tap % 3) : -1;
        const float* xr = X + (src < 0 ? 0 : (size_t)src) * (size_t)Ci + 4 * q;
        for (int k0 = 0; k0 < Ci; k0 += kKc) {
            float4 xv[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) xv[jj] = src >= 0 ? *reinterpret_cast<const float4*>(xr + k0 + 16 * jj) : float4{0.f, 0.f, 0.f, 0.f};
            __syncthreads();        // the previous chunk has been read
            for (int e = tid; e < kKc * NT * 16; e += 256) {
                const int j = e / kKc, kk = e % kKc;
                As[kk * LD + j] = j < r ? A[((size_t)j * Ci + k0 + kk) * 9 + tap] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float a[4] = {xv[jj].x, xv[jj].y, xv[jj].z, xv[jj].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* bp = As + (16 * jj + 4 * q + e) * LD + i;
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[e & 1][t] = mfma4(a[e], bp[16 * t], acc[e & 1][t]);
                }
            }
        }
    }
    // D[row 4 q + reg][col i]
    const int row0 = blockIdx.x * kRows + wave * 16 + 4 * q;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = 16 * t + i;
        if (j >= r) continue;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
            if (row0 + gg < Mo) T[(size_t)(row0 + gg) * r + j] = acc[0][t][gg] + acc[1][t][gg];
    }
}

// dX [Mi][Ci] += s sum_tap U[reader(tap)] down[:, :, tap]: U [Mo][r], the gather form of the transposed conv -- every dX row collects
// from the U rows that read it, one read and one write of dX. lora_up_kernel with a tap loop inside the column step: a workgroup owns
// 64 input pixels and the columns [blockIdx.y * ncols, + ncols) in steps of 64. Per step and tap down[:, n0 .. n0 + 63, tap] is staged
// in LDS as [k][n] and a lane reads its reader's U fragments (contraction index 4 step + q, zero beyond r or without a reader); the
// four 16-column tiles are four accumulators that run through every tap (geometry 2: through the four readers of every tap).
template <int KS>       // contraction steps of 4: r <= 4 KS
__global__ void __launch_bounds__(256) lora_conv_dgrad_kernel(const float* __restrict__ U, const float* __restrict__ A, Geo g, int Mi, int Ci, int r, int ncols,
                                                              float s, float* __restrict__ dX) {
    constexpr int LD = lds_ld(kNc / 16), kUnroll = KS < 8 ? KS : 8;
    __shared__ float Bs[4 * KS * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int row = blockIdx.x * kRows + wave * 16 + i;
    const bool row_ok = row < Mi;
    const int m = row_ok ? row : 0, px = m % g.W, py = (m / g.W) % g.H, b = m / (g.W * g.H);
    const int n_sub = g.geom == 2 ? 4 : 1;
    const int row0 = blockIdx.x * kRows + wave * 16 + 4 * q;
    const int n_begin = blockIdx.y * ncols;
    for (int n0 = n_begin; n0 < n_begin + ncols; n0 += kNc) {
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int tap = 0; tap < 9; ++tap) {
            __syncthreads();        // the previous tap's chunk has been read
            for (int e = tid; e < 4 * KS * kNc; e += 256) {
                const int k = e / kNc, n = e % kNc;
                Bs[k * LD + n] = k < r ? A[((size_t)k * Ci + n0 + n) * 9 + tap] : 0.f;
            }
            __syncthreads();
            for (int sub = 0; sub < n_sub; ++sub) {
                const long long o = row_ok ? reader_row(g, b, py, px, tap / 3, tap % 3, sub) : -1;
                const float* up = U + (o < 0 ? 0 : (size_t)o) * r;
#pragma unroll kUnroll
                for (int st = 0; st < KS; ++st) {
                    const int k = 4 * st + q;
                    const float a = (o >= 0 && k < r) ? up[k] : 0.f;
                    const float* bp = Bs + k * LD + i;
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = mfma4(a, bp[16 * t], acc[t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg)
                if (row0 + gg < Mi) {
                    float* yp = dX + (size_t)(row0 + gg) * Ci + n0 + 16 * t + i;
                    *yp = fmaf(s, acc[t][gg], *yp);
                }
    }
}

// P[chunk][tap - tap0][r][Ci] = U[rows of the chunk]^T X[the rows those read through tap]: lora_wgrad_kernel with the rows of Z gathered.
// Workgroup (strip, chunk, tap): columns [64 strip, + 64) of X, 16 per wave, all r rows of the result. Per stage of 64 output rows
// the rows of U are staged in LDS as [m][j] (zero beyond the chunk and r) with the X row each of them reads (-1: padding, or beyond
// the chunk); a lane reads X[that row][its column]. Even and odd steps accumulate separately.
template <int NT>
__global__ void __launch_bounds__(256) lora_conv_wgrad_kernel(const float* __restrict__ U, const float* __restrict__ X, Geo g, int Mo, int Ci, int r,
                                                              int chunk_rows, int tap0, float* __restrict__ P) {
    constexpr int LD = lds_ld(NT);
    __shared__ float Ts[kRows * LD];
    __shared__ int src[kRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int col = blockIdx.x * kNc + wave * 16 + i;
    const int tap = tap0 + blockIdx.z;
    const int m_begin = blockIdx.y * chunk_rows;
    const int m_end = m_begin + chunk_rows < Mo ? m_begin + chunk_rows : Mo;
    f32x4 acc[2][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[0][t] = acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int m0 = m_begin; m0 < m_end; m0 += kRows) {
        __syncthreads();        // the previous stage has been read
        if (tid < kRows) {
            const int m = m0 + tid;
            src[tid] = m < m_end ? (int)src_row(g, m / (g.Wo * g.Ho), (m / g.Wo) % g.Ho, m % g.Wo, tap / 3, tap % 3) : -1;
        }
        for (int e = tid; e < kRows * NT * 16; e += 256) {
            const int mm = e / (NT * 16), j = e % (NT * 16);
            Ts[mm * LD + j] = (m0 + mm < m_end && j < r) ? U[(size_t)(m0 + mm) * r + j] : 0.f;
        }
        __syncthreads();
        float z[16];
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int sr = src[4 * st + q];
            z[st] = sr >= 0 ? X[(size_t)sr * Ci + col] : 0.f;
        }
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const float* ap = Ts + (4 * st + q) * LD + i;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[st & 1][t] = mfma4(ap[16 * t], z[st], acc[st & 1][t]);
        }
    }
    // D[row 4 q + reg][col i]: row = the result's j within tile t, col = this wave's column of X
    float* p = P + ((size_t)blockIdx.y * gridDim.z + blockIdx.z) * r * Ci;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const int j = 16 * t + 4 * q + gg;
            if (j < r) p[(size_t)j * Ci + col] = acc[0][t][gg] + acc[1][t][gg];
        }
}

// G[j][ci][tap0 + t] = s (P[0][t] + P[1][t] + ... in ascending order): the OIHW place of n_taps taps of g_down
__global__ void lora_conv_wgrad_reduce_kernel(const float* __restrict__ P, int n_chunks, int n_taps, int tap0, int r, int Ci, float s, float* __restrict__ G) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per = (size_t)r * Ci, n_out = per * n_taps;
    if (e >= n_out) return;
    float v = P[e];
    for (int c = 1; c < n_chunks; ++c) v += P[(size_t)c * n_out + e];
    G[(e % per) * 9 + tap0 + e / per] = s * v;
}

// out[b][c] = sum over the HW pixels of g[b][.][c]: workgroup (16 columns, sample b); row lane j adds rows j, j + 16, ... in ascending
// order, then lane 0 adds the sixteen partial sums in ascending order
__global__ void __launch_bounds__(256) lora_sample_colsum_kernel(const float* __restrict__ g, int HW, int C, float* __restrict__ out) {
    __shared__ float part[16][17];
    const int ci = threadIdx.x & 15, j = threadIdx.x >> 4, col = blockIdx.x * 16 + ci;
    const float* p = g + (size_t)blockIdx.y * HW * C + col;
    float v = 0.f;
    for (int m = j; m < HW; m += 16) v += p[(size_t)m * C];
    part[j][ci] = v;
    __syncthreads();
    if (j == 0) {
        float t = part[0][ci];
        for (int k = 1; k < 16; ++k) t += part[k][ci];
        out[(size_t)blockIdx.y * C + col] = t;
    }
}

int tiles_of(int r) { return r <= 16 ? 1 : r <= 32 ? 2 : r <= 64 ? 4 : 8; }

Geo geo_of(int geom, int H, int W) { return Geo{geom, H, W, geom == 1 ? H / 2 : geom == 2 ? 2 * H : H, geom == 1 ? W / 2 : geom == 2 ? 2 * W : W}; }

}  // namespace

namespace train {

size_t lora_conv_out_rows(int geom, int B, int H, int W) {
    const Geo g = geo_of(geom, H, W);
    return (size_t)B * g.Ho * g.Wo;
}

void lora_conv_check(const char* what, int B, int H, int W, int Ci, int Co, int r, int geom) {
    if (r < 1 || r > 128) throw GlError(GL_ERR_ARG, fmt("%s: rank %d (the low-rank kernels take 1 <= r <= 128)", what, r));
    if (Ci < 64 || Ci % 64 || Co < 64 || Co % 64) throw GlError(GL_ERR_ARG, fmt("%s: Ci = %d and Co = %d must be multiples of 64", what, Ci, Co));
    if (geom < 0 || geom > 2) throw GlError(GL_ERR_ARG, fmt("%s: geom %d (0 stride 1, 1 Downsample, 2 Upsample)", what, geom));
    if (B < 1 || H < 1 || W < 1) throw GlError(GL_ERR_ARG, fmt("%s: B = %d, H = %d, W = %d (each >= 1)", what, B, H, W));
    if (geom == 1 && ((H | W) & 1)) throw GlError(GL_ERR_ARG, fmt("%s: Downsample takes even H and W (%d x %d)", what, H, W));
    if ((size_t)B * H * W * (geom == 2 ? 4 : 1) > (size_t)1 << 30) throw GlError(GL_ERR_ARG, fmt("%s: %d x %d x %d pixels (at most 2^30 output rows)", what, B, H, W));
}

void lora_conv_down(const Ctx& c, const float* X, int B, int H, int W, int Ci, const float* down, int r, int geom, float* T) {
    if (reinterpret_cast<uintptr_t>(X) & 15) throw GlError(GL_ERR_ARG, "low-rank conv product: the pixel rows must be 16-byte aligned (rows are read as float4)");
    const Geo g = geo_of(geom, H, W);
    const int Mo = B * g.Ho * g.Wo;
    const dim3 grid(cdiv(Mo, kRows)), block(256);
    switch (tiles_of(r)) {
        case 1: hipLaunchKernelGGL(lora_conv_down_kernel<1>, grid, block, 0, c.s, X, down, g, Mo, Ci, r, T); break;
        case 2: hipLaunchKernelGGL(lora_conv_down_kernel<2>, grid, block, 0, c.s, X, down, g, Mo, Ci, r, T); break;
        case 4: hipLaunchKernelGGL(lora_conv_down_kernel<4>, grid, block, 0, c.s, X, down, g, Mo, Ci, r, T); break;
        default: hipLaunchKernelGGL(lora_conv_down_kernel<8>, grid, block, 0, c.s, X, down, g, Mo, Ci, r, T); break;
    }
}

void lora_conv_dgrad(const Ctx& c, const float* U, int B, int H, int W, int Ci, const float* down, int r, int geom, float s, float* dX) {
    const Geo g = geo_of(geom, H, W);
    const int Mi = B * H * W;
    // column splits as lora_up: a function of the shape alone
    const int row_blocks = cdiv(Mi, kRows), strips = Ci / kNc;
    int splits = 1;
    while (splits < strips && row_blocks * splits < 256 && strips % (splits * 2) == 0) splits *= 2;
    const int ncols = Ci / splits;
    const dim3 grid(row_blocks, splits), block(256);
    const int ks = cdiv(r, 4);
    if (ks <= 1) hipLaunchKernelGGL(lora_conv_dgrad_kernel<1>, grid, block, 0, c.s, U, down, g, Mi, Ci, r, ncols, s, dX);
    else if (ks <= 2) hipLaunchKernelGGL(lora_conv_dgrad_kernel<2>, grid, block, 0, c.s, U, down, g, Mi, Ci, r, ncols, s, dX);
    else if (ks <= 4) hipLaunchKernelGGL(lora_conv_dgrad_kernel<4>, grid, block, 0, c.s, U, down, g, Mi, Ci, r, ncols, s, dX);
    else if (ks <= 8) hipLaunchKernelGGL(lora_conv_dgrad_kernel<8>, grid, block, 0, c.s, U, down, g, Mi, Ci, r, ncols, s, dX);
    else if (ks <= 16) hipLaunchKernelGGL(lora_conv_dgrad_kernel<16>, grid, block, 0, c.s, U, down, g, Mi, Ci, r, ncols, s, dX);
    else hipLaunchKernelGGL(lora_conv_dgrad_kernel<32>, grid, block, 0, c.s, U, down, g, Mi, Ci, r, ncols, s, dX);
}

int lora_conv_wgrad_taps(int n_chunks, int r, int Ci) {
    return (size_t)9 * n_chunks * r * Ci * sizeof(float) <= kLoraConvWgradWs ? 9 : 1;
}

void lora_conv_wgrad(const Ctx& c, const float* U, const float* X, int B, int H, int W, int Ci, int r, int geom, float s, float* G) {
    const Geo g = geo_of(geom, H, W);
    const int Mo = B * g.Ho * g.Wo;
    const int chunk = lora_wgrad_chunk_rows(Mo), n_chunks = cdiv(Mo, chunk);
    // all nine taps in one launch when their partials fit kLoraConvWgradWs, else tap by tap: a tap's sums are the same either way
    const int n_taps = lora_conv_wgrad_taps(n_chunks, r, Ci);
    const size_t mk = c.ar.mark();
    float* P = c.f32((size_t)n_chunks * n_taps * r * Ci);
    const dim3 grid(Ci / kNc, n_chunks, n_taps), block(256);
    for (int tap0 = 0; tap0 < 9; tap0 += n_taps) {
        switch (tiles_of(r)) {
            case 1: hipLaunchKernelGGL(lora_conv_wgrad_kernel<1>, grid, block, 0, c.s, U, X, g, Mo, Ci, r, chunk, tap0, P); break;
            case 2: hipLaunchKernelGGL(lora_conv_wgrad_kernel<2>, grid, block, 0, c.s, U, X, g, Mo, Ci, r, chunk, tap0, P); break;
            case 4: hipLaunchKernelGGL(lora_conv_wgrad_kernel<4>, grid, block, 0, c.s, U, X, g, Mo, Ci, r, chunk, tap0, P); break;
            default: hipLaunchKernelGGL(lora_conv_wgrad_kernel<8>, grid, block, 0, c.s, U, X, g, Mo, Ci, r, chunk, tap0, P); break;
        }
        hipLaunchKernelGGL(lora_conv_wgrad_reduce_kernel, Ctx::g1((size_t)n_taps * r * Ci), dim3(256), 0, c.s, P, n_chunks, n_taps, tap0, r, Ci, s, G);
    }
    c.ar.release(mk);       // stream order keeps the reuse safe
}

void lora_sample_colsum(const Ctx& c, const float* g, int B, int HW, int C, float* out) {
    hipLaunchKernelGGL(lora_sample_colsum_kernel, dim3(C / 16, B), dim3(256), 0, c.s, g, HW, C, out);
}

void lora_conv_fwd(const Ctx& c, const float* W, const float* x, int B, int H, int Wd, int Ci, int Co, int geom, float* y) {
    const LoraAdapter* a = lora_find(c, W);
    if (!a) return;
    lora_conv_check("unet_train_step (conv adapter)", B, H, Wd, Ci, Co, a->r, geom);
    const int Mo = (int)lora_conv_out_rows(geom, B, H, Wd);
    const size_t mk = c.ar.mark();
    float* t = c.f32((size_t)Mo * a->r);
    lora_conv_down(c, x, B, H, Wd, Ci, a->down, a->r, geom, t);
    lora_up(c, t, Mo, a->r, a->up, Co, false, a->scale, y);
    c.ar.release(mk);
}

void lora_conv_bwd(const Ctx& c, const float* W, const float* dy, const float* x, int B, int H, int Wd, int Ci, int Co, int geom, float* dx) {
    const LoraAdapter* a = lora_find(c, W);
    if (!a) return;
    const int r = a->r, Mo = (int)lora_conv_out_rows(geom, B, H, Wd);
    const size_t mk = c.ar.mark();
    if (dx || a->g_down) {
        float* u = c.f32((size_t)Mo * r);
        lora_down(c, dy, Mo, Co, a->up, r, true, u);
        if (dx) lora_conv_dgrad(c, u, B, H, Wd, Ci, a->down, r, geom, a->scale, dx);
        if (a->g_down) lora_conv_wgrad(c, u, x, B, H, Wd, Ci, r, geom, a->scale, a->g_down);
    }
    if (a->g_up) {
        float* t = c.f32((size_t)Mo * r);
        lora_conv_down(c, x, B, H, Wd, Ci, a->down, r, geom, t);
        lora_wgrad(c, t, dy, Mo, r, Co, a->scale, true, a->g_up);
    }
    c.ar.release(mk);
}

}  // namespace train

// include/gligen_amd_train_lora_conv.h: the low-rank part of one adapted 3 x 3 conv by itself
int train_prim_lora_conv3(Arena& ar, float* ws, size_t ws_bytes, int B, int H, int W, int Ci, int Co, int r, float scale, int geom, const float* x,
                          const float* down, const float* up, const float* dy, float* t, float* y, float* u, float* dx, float* g_down, float* g_up,
                          hipStream_t s) {
    try {
        lora_conv_check("gl_op_lora_conv3", B, H, W, Ci, Co, r, geom);
        Ctx c{ar, ws, ws_bytes, s};
        const int Mo = (int)lora_conv_out_rows(geom, B, H, W);
        const size_t mk = ar.mark();
        float* tt = t ? t : c.f32((size_t)Mo * r);
        lora_conv_down(c, x, B, H, W, Ci, down, r, geom, tt);
        if (y) lora_up(c, tt, Mo, r, up, Co, false, scale, y);
        if (dy) {
            float* uu = u ? u : c.f32((size_t)Mo * r);
            lora_down(c, dy, Mo, Co, up, r, true, uu);
            if (dx) lora_conv_dgrad(c, uu, B, H, W, Ci, down, r, geom, scale, dx);
            if (g_down) lora_conv_wgrad(c, uu, x, B, H, W, Ci, r, geom, scale, g_down);
            if (g_up) lora_wgrad(c, tt, dy, Mo, r, Co, scale, true, g_up);
        }
        ar.release(mk);
        c.hip(hipGetLastError(), "low-rank conv kernel launch");
    } catch (const GlError& e) {
        return set_error(e.code, "%s", e.what());
    }
    return GL_OK;
}

}  // namespace gl
