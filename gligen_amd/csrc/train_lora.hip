// The low-rank part of an adapted Linear in training, for gfx950: y = x W^T + s (x down^T) up^T with s = alpha / r, down [r][K],
// up [N][r] (kohya's lora_down / lora_up). W stays frozen and goes through the step's own products (train_ops.hip); this unit adds
// the adapter term and forms the adapter's gradients:
//   forward         t = x down^T             y  += s t up^T
//   data gradient   u = dy up                dx += s u down
//   weight grads    g_down = s u^T x         g_up = (s t^T dy)^T
// The products are tall and skinny (M up to 16 384 rows against r <= 128), so they run on the exact-fp32 MFMA
// (v_mfma_f32_16x16x4_f32: one fp32 per lane per operand, the result a k-ordered fmaf chain) straight from the fp32 activations: no
// bf16 split, no operand copy, no padding outside registers and LDS.
// Lane maps of the 16x16x4 form (lane l, i = l & 15, q = l >> 4): A[row i][k = q], B[k = q][col i], D[row 4 q + reg][col i]. The
// instruction sums its four k in lane-group order, so any assignment of contraction indices to (instruction, q) is a valid product as
// long as A and B use the same one; the kernels below choose the assignment that lets a lane load 16 bytes at a time.
// No atomics: the weight gradients are partial sums over row chunks whose size depends on the shape alone, added in ascending order
// by a second launch, so two runs give the same bits.
#include "train_impl.h"

namespace gl {

using namespace train;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kRows = 64;        // rows of X / Y / Z a workgroup of four waves handles at a time: 16 per wave (down, up), 64 per stage (wgrad)
constexpr int kKc = 64;          // contraction columns staged per step of the down product
constexpr int kNc = 64;          // output columns per step of the up product; the column strip of a weight-gradient workgroup

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// The leading dimension of an LDS image [k][j] read as B[k = q][col i] (or A[row i][k = q]): 16 consecutive floats from each of four
// consecutive k rows. ld % 32 == 16 puts the four rows on four different groups of 16 banks.
__host__ __device__ constexpr int lds_ld(int nt) { return (nt * 16) | 16; }

// T [M][r] = X [M][K] A^T. a_kr 0: A is [r][K] (t = x down^T); 1: A is [K][r] (u = dy up, A = up [N][r] with K = N).
// A workgroup owns 64 rows and all r columns (NT tiles of 16, zero-padded in LDS); wave w owns rows 16 w .. 16 w + 15. Per step of 64
// contraction columns the chunk of A is staged in LDS as [k][j] and a lane reads X[row i][k0 + 16 jj + 4 q .. + 3] (jj = 0..3) as four
// float4: X is read once. Contraction index 16 jj + 4 q + e goes to instruction (jj, e) of lane group q; even and odd instructions
// accumulate separately (two independent chains per tile: the 16x16x4 form has a 40-cycle dependent latency, 32-cycle issue).
template <int NT>
__global__ void __launch_bounds__(256) lora_down_kernel(const float* __restrict__ X, const float* __restrict__ A, int M, int K, int r, int a_kr,
                                                        float* __restrict__ T) {
    constexpr int LD = lds_ld(NT);
    __shared__ float As[kKc * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const size_t row = (size_t)blockIdx.x * kRows + wave * 16 + i;
    const bool row_ok = row < (size_t)M;
    const float* xr = X + (row_ok ? row : 0) * (size_t)K + 4 * q;
    f32x4 acc[2][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[0][t] = acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += kKc) {
        float4 xv[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) xv[jj] = row_ok ? *reinterpret_cast<const float4*>(xr + k0 + 16 * jj) : float4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();        // the previous chunk has been read
        if (a_kr) {             // A[k][j]: j runs fastest in memory and in LDS
            for (int e = tid; e < kKc * NT * 16; e += 256) {
                const int kk = e / (NT * 16), j = e % (NT * 16);
                As[kk * LD + j] = j < r ? A[(size_t)(k0 + kk) * r + j] : 0.f;
            }
        } else {                // A[j][k]: k runs fastest in memory
            for (int e = tid; e < kKc * NT * 16; e += 256) {
                const int j = e / kKc, kk = e % kKc;
                As[kk * LD + j] = j < r ? A[(size_t)j * K + k0 + kk] : 0.f;
            }
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
    // D[row 4 q + reg][col i]
    const size_t row0 = (size_t)blockIdx.x * kRows + wave * 16 + 4 * q;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = 16 * t + i;
        if (j >= r) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (row0 + g < (size_t)M) T[(row0 + g) * r + j] = acc[0][t][g] + acc[1][t][g];
    }
}

// Y [M][N] += s T [M][r] B. b_rn 0: B is [N][r] (y += s t up^T); 1: B is [r][N] (dx += s u down, N = K).
// A workgroup owns 64 rows and the columns [blockIdx.y * ncols, + ncols) in steps of 64; wave w owns rows 16 w .. + 15 and keeps its
// T fragments (contraction index 4 step + q, zero beyond r) in registers for every step. A 64-column chunk of B is staged in LDS as
// [k][n]; the four 16-column tiles of a step are four independent accumulators. One read and one write of Y.
template <int KS>       // contraction steps of 4: r <= 4 KS
__global__ void __launch_bounds__(256) lora_up_kernel(const float* __restrict__ T, const float* __restrict__ Bm, int M, int N, int r, int b_rn, int ncols,
                                                      float s, float* __restrict__ Y) {
    constexpr int LD = lds_ld(kNc / 16);
    __shared__ float Bs[4 * KS * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const size_t row = (size_t)blockIdx.x * kRows + wave * 16 + i;
    float a[KS];
#pragma unroll
    for (int st = 0; st < KS; ++st) {
        const int k = 4 * st + q;
        a[st] = (row < (size_t)M && k < r) ? T[row * r + k] : 0.f;
    }
    const size_t row0 = (size_t)blockIdx.x * kRows + wave * 16 + 4 * q;
    const int n_begin = blockIdx.y * ncols;
    for (int n0 = n_begin; n0 < n_begin + ncols; n0 += kNc) {
        __syncthreads();
        if (b_rn) {             // B[k][n]: n runs fastest in memory and in LDS
            for (int e = tid; e < 4 * KS * kNc; e += 256) {
                const int k = e / kNc, n = e % kNc;
                Bs[k * LD + n] = k < r ? Bm[(size_t)k * N + n0 + n] : 0.f;
            }
        } else {                // B[n][k]: k runs fastest in memory
            for (int e = tid; e < 4 * KS * kNc; e += 256) {
                const int n = e / (4 * KS), k = e % (4 * KS);
                Bs[k * LD + n] = k < r ? Bm[(size_t)(n0 + n) * r + k] : 0.f;
            }
        }
        __syncthreads();
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < KS; ++st) {
            const float* bp = Bs + (4 * st + q) * LD + i;
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = mfma4(a[st], bp[16 * t], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (row0 + g < (size_t)M) {
                    float* yp = Y + (row0 + g) * (size_t)N + n0 + 16 * t + i;
                    *yp = fmaf(s, acc[t][g], *yp);
                }
    }
}

// P[chunk][r][N] = T[rows of the chunk]^T Z[rows of the chunk]: T [M][r], Z [M][N], the contraction runs over rows. Workgroup
// (strip, chunk): columns [64 strip, + 64) of Z, 16 per wave, all r rows of the result (NT tiles of 16). Per stage of 64 rows the
// rows of T are staged in LDS as [m][j] (zero beyond M and r) and read as A[row j][k = m]; a lane reads Z[m0 + 4 st + q][its column]
// (zero beyond M). Even and odd steps accumulate separately.
template <int NT>
__global__ void __launch_bounds__(256) lora_wgrad_kernel(const float* __restrict__ T, const float* __restrict__ Z, int M, int N, int r, int chunk_rows,
                                                         float* __restrict__ P) {
    constexpr int LD = lds_ld(NT);
    __shared__ float Ts[kRows * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int col = blockIdx.x * kNc + wave * 16 + i;
    const size_t m_begin = (size_t)blockIdx.y * chunk_rows;
    const size_t m_end = m_begin + chunk_rows < (size_t)M ? m_begin + chunk_rows : (size_t)M;
    f32x4 acc[2][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[0][t] = acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (size_t m0 = m_begin; m0 < m_end; m0 += kRows) {
        float z[16];
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const size_t m = m0 + 4 * st + q;
            z[st] = m < m_end ? Z[m * N + col] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < kRows * NT * 16; e += 256) {
            const int mm = e / (NT * 16), j = e % (NT * 16);
            Ts[mm * LD + j] = (m0 + mm < m_end && j < r) ? T[(m0 + mm) * r + j] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const float* ap = Ts + (4 * st + q) * LD + i;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[st & 1][t] = mfma4(ap[16 * t], z[st], acc[st & 1][t]);
        }
    }
    // D[row 4 q + reg][col i]: row = the result's j within tile t, col = this wave's column of Z
    float* p = P + (size_t)blockIdx.y * r * N;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int j = 16 * t + 4 * q + g;
            if (j < r) p[(size_t)j * N + col] = acc[0][t][g] + acc[1][t][g];
        }
}

// G = s (P[0] + P[1] + ... in ascending order): [r][N], or written transposed as [N][r]
__global__ void lora_wgrad_reduce_kernel(const float* __restrict__ P, int n_chunks, int r, int N, float s, int transposed, float* __restrict__ G) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n_out = (size_t)r * N;
    if (e >= n_out) return;
    float v = P[e];
    for (int c = 1; c < n_chunks; ++c) v += P[(size_t)c * n_out + e];
    const size_t j = e / N, n = e % N;
    G[transposed ? n * r + j : e] = s * v;
}

int tiles_of(int r) { return r <= 16 ? 1 : r <= 32 ? 2 : r <= 64 ? 4 : 8; }

}  // namespace

namespace train {

void lora_check(const char* what, int M, int K, int N, int r) {
    if (r < 1 || r > 128) throw GlError(GL_ERR_ARG, fmt("%s: rank %d (the low-rank kernels take 1 <= r <= 128)", what, r));
    if (K < 64 || K % 64 || N < 64 || N % 64) throw GlError(GL_ERR_ARG, fmt("%s: K = %d and N = %d must be multiples of 64", what, K, N));
    if (M < 1) throw GlError(GL_ERR_ARG, fmt("%s: M = %d rows (M >= 1)", what, M));
}

int lora_wgrad_chunk_rows(int M) {
    const int per = round_up(cdiv(M, 32), kRows);
    return per > 256 ? per : 256;
}

void lora_down(const Ctx& c, const float* X, int M, int K, const float* A, int r, bool a_kr, float* T) {
    if (reinterpret_cast<uintptr_t>(X) & 15) throw GlError(GL_ERR_ARG, "low-rank product: the row operand must be 16-byte aligned (rows are read as float4)");
    const dim3 grid(cdiv(M, kRows)), block(256);
    switch (tiles_of(r)) {
        case 1: hipLaunchKernelGGL(lora_down_kernel<1>, grid, block, 0, c.s, X, A, M, K, r, a_kr ? 1 : 0, T); break;
        case 2: hipLaunchKernelGGL(lora_down_kernel<2>, grid, block, 0, c.s, X, A, M, K, r, a_kr ? 1 : 0, T); break;
        case 4: hipLaunchKernelGGL(lora_down_kernel<4>, grid, block, 0, c.s, X, A, M, K, r, a_kr ? 1 : 0, T); break;
        default: hipLaunchKernelGGL(lora_down_kernel<8>, grid, block, 0, c.s, X, A, M, K, r, a_kr ? 1 : 0, T); break;
    }
}

void lora_up(const Ctx& c, const float* T, int M, int r, const float* Bm, int N, bool b_rn, float s, float* Y) {
    // column splits: enough workgroups to fill the device when there are few row blocks; a function of the shape alone
    const int row_blocks = cdiv(M, kRows), strips = N / kNc;
    int splits = 1;
    while (splits < strips && row_blocks * splits < 256 && strips % (splits * 2) == 0) splits *= 2;
    const int ncols = N / splits;
    const dim3 grid(row_blocks, splits), block(256);
    const int ks = cdiv(r, 4);
    const int brn = b_rn ? 1 : 0;
    if (ks <= 1) hipLaunchKernelGGL(lora_up_kernel<1>, grid, block, 0, c.s, T, Bm, M, N, r, brn, ncols, s, Y);
    else if (ks <= 2) hipLaunchKernelGGL(lora_up_kernel<2>, grid, block, 0, c.s, T, Bm, M, N, r, brn, ncols, s, Y);
    else if (ks <= 4) hipLaunchKernelGGL(lora_up_kernel<4>, grid, block, 0, c.s, T, Bm, M, N, r, brn, ncols, s, Y);
    else if (ks <= 8) hipLaunchKernelGGL(lora_up_kernel<8>, grid, block, 0, c.s, T, Bm, M, N, r, brn, ncols, s, Y);
    else if (ks <= 16) hipLaunchKernelGGL(lora_up_kernel<16>, grid, block, 0, c.s, T, Bm, M, N, r, brn, ncols, s, Y);
    else hipLaunchKernelGGL(lora_up_kernel<32>, grid, block, 0, c.s, T, Bm, M, N, r, brn, ncols, s, Y);
}

void lora_wgrad(const Ctx& c, const float* T, const float* Z, int M, int r, int N, float s, bool transposed, float* G) {
    const int chunk = lora_wgrad_chunk_rows(M), n_chunks = cdiv(M, chunk);
    const size_t mk = c.ar.mark();
    float* P = c.f32((size_t)n_chunks * r * N);
    const dim3 grid(N / kNc, n_chunks), block(256);
    switch (tiles_of(r)) {
        case 1: hipLaunchKernelGGL(lora_wgrad_kernel<1>, grid, block, 0, c.s, T, Z, M, N, r, chunk, P); break;
        case 2: hipLaunchKernelGGL(lora_wgrad_kernel<2>, grid, block, 0, c.s, T, Z, M, N, r, chunk, P); break;
        case 4: hipLaunchKernelGGL(lora_wgrad_kernel<4>, grid, block, 0, c.s, T, Z, M, N, r, chunk, P); break;
        default: hipLaunchKernelGGL(lora_wgrad_kernel<8>, grid, block, 0, c.s, T, Z, M, N, r, chunk, P); break;
    }
    hipLaunchKernelGGL(lora_wgrad_reduce_kernel, Ctx::g1((size_t)r * N), dim3(256), 0, c.s, P, n_chunks, r, N, s, transposed ? 1 : 0, G);
    c.ar.release(mk);       // stream order keeps the reuse safe
}

const LoraAdapter* lora_find(const Ctx& c, const float* W) {
    if (!c.lora) return nullptr;
    auto it = c.lora->find(W);
    return it == c.lora->end() ? nullptr : &it->second;
}

void lora_fwd(const Ctx& c, const float* W, const float* x, int M, int K, int N, float* y) {
    const LoraAdapter* a = lora_find(c, W);
    if (!a) return;
    lora_check("unet_train_step (adapter)", M, K, N, a->r);
    const size_t mk = c.ar.mark();
    float* t = c.f32((size_t)M * a->r);
    lora_down(c, x, M, K, a->down, a->r, false, t);
    lora_up(c, t, M, a->r, a->up, N, false, a->scale, y);
    c.ar.release(mk);
}

void lora_bwd(const Ctx& c, const float* W, const float* dy, const float* x, int M, int K, int N, float* dx) {
    const LoraAdapter* a = lora_find(c, W);
    if (!a) return;
    const int r = a->r;
    const size_t mk = c.ar.mark();
    if (dx || a->g_down) {
        float* u = c.f32((size_t)M * r);
        lora_down(c, dy, M, N, a->up, r, true, u);
        if (dx) lora_up(c, u, M, r, a->down, K, true, a->scale, dx);
        if (a->g_down) lora_wgrad(c, u, x, M, r, K, a->scale, false, a->g_down);
    }
    if (a->g_up) {
        float* t = c.f32((size_t)M * r);
        lora_down(c, x, M, K, a->down, r, false, t);
        lora_wgrad(c, t, dy, M, r, N, a->scale, true, a->g_up);
    }
    c.ar.release(mk);
}

}  // namespace train

// include/gligen_amd_train_lora.h: the low-rank part of one adapted Linear by itself
int train_prim_lora_linear(Arena& ar, float* ws, size_t ws_bytes, int M, int K, int N, int r, float scale, int down_kr, int up_rn, const float* x,
                           const float* down, const float* up, const float* dy, float* t, float* y, float* u, float* dx, float* g_down, float* g_up,
                           hipStream_t s) {
    try {
        lora_check("gl_op_lora_linear", M, K, N, r);
        Ctx c{ar, ws, ws_bytes, s};
        const size_t mk = ar.mark();
        float* tt = t ? t : c.f32((size_t)M * r);
        lora_down(c, x, M, K, down, r, down_kr != 0, tt);
        if (y) lora_up(c, tt, M, r, up, N, up_rn != 0, scale, y);
        if (dy) {
            float* uu = u ? u : c.f32((size_t)M * r);
            // u = dy up: up [N][r] is the [K][r] form of the small operand, up [r][N] the [r][K] form
            lora_down(c, dy, M, N, up, r, up_rn == 0, uu);
            // dx += s u down: down [r][K] is the [r][N] form, down [K][r] the [N][r] form
            if (dx) lora_up(c, uu, M, r, down, K, down_kr == 0, scale, dx);
            // g_down has down's layout, g_up has up's
            if (g_down) lora_wgrad(c, uu, x, M, r, K, scale, down_kr != 0, g_down);
            if (g_up) lora_wgrad(c, tt, dy, M, r, N, scale, up_rn == 0, g_up);
        }
        ar.release(mk);
        c.hip(hipGetLastError(), "low-rank kernel launch");
    } catch (const GlError& e) {
        return set_error(e.code, "%s", e.what());
    }
    return GL_OK;
}

}  // namespace gl
