// The merge of a LoRA adapter into a module's fp32 parameters (include/gligen_amd_lora.h): W [N][K] += scale * up [N][r] @ down [r][K]
// in place. Load-time work -- a rank-128 adapter over every UNet matrix is about 0.2 TFLOP of fp32 --, so this is a plain LDS-tiled
// fp32 kernel and not an MFMA one: the packed bf16 engine is rebuilt from the merged parameters afterwards, which costs far more.
// One workgroup per 32 x 128 tile of W; per chunk of 32 ranks the up panel [32][32] (transposed, padded) and the down panel
// [32][128] are staged in LDS (20.1 KiB); a thread owns the 4 x 4 elements (ty + 8 a, tx + 32 b): a wave's W traffic is whole 128-byte
// row segments, its LDS reads are conflict-free (down) or broadcasts (up).
// Every element of W is written by one thread, from one fp32 accumulator that takes the ranks in ascending order through fmaf and a
// last fmaf(scale, acc, W): the result does not depend on the grid or on launch order, and two calls give the same bits. Ranks, rows
// and columns beyond the edge are staged as zeros (fmaf(0, 0, acc) == acc) and never stored.
#include "lora.h"

namespace gl {

namespace {

constexpr int kTileN = 32, kTileK = 128, kChunk = 32;       // rows and columns of W per workgroup, ranks per staging chunk
constexpr int kUpPitch = kTileN + 1;                        // odd: the transposing stores of a wave spread over the banks

__global__ void __launch_bounds__(256) lora_merge_kernel(float* __restrict__ W, const float* __restrict__ up, const float* __restrict__ down,
                                                         int N, int K, int r, float scale, int tiles_k) {
    __shared__ float up_t[kChunk][kUpPitch];                // [rank][row]
    __shared__ float dn[kChunk][kTileK];                    // [rank][column]
    const int tile = blockIdx.x;
    const int n0 = (tile / tiles_k) * kTileN, k0 = (tile % tiles_k) * kTileK;
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;

    for (int i0 = 0; i0 < r; i0 += kChunk) {
        // up [n0 + row][i0 + col] -> up_t[col][row]: 1024 elements, lanes along the rank (contiguous in memory)
#pragma unroll
        for (int j = 0; j < kTileN * kChunk / 256; ++j) {
            const int e = t + 256 * j, row = e / kChunk, col = e % kChunk;
            const int n = n0 + row, i = i0 + col;
            up_t[col][row] = (n < N && i < r) ? up[(size_t)n * r + i] : 0.f;
        }
        // down [i0 + row][k0 + col] -> dn[row][col]: 4096 elements, lanes along the column
#pragma unroll
        for (int j = 0; j < kChunk * kTileK / 256; ++j) {
            const int e = t + 256 * j, row = e / kTileK, col = e % kTileK;
            const int i = i0 + row, k = k0 + col;
            dn[row][col] = (i < r && k < K) ? down[(size_t)i * K + k] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < kChunk; ++i) {
            float u[4], d[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) u[a] = up_t[i][ty + 8 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) d[b] = dn[i][tx + 32 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(u[a], d[b], acc[a][b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int n = n0 + ty + 8 * a;
        if (n >= N) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int k = k0 + tx + 32 * b;
            if (k < K) {
                float* w = W + (size_t)n * K + k;
                *w = fmaf(scale, acc[a][b], *w);
            }
        }
    }
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

int lora_merge_launch(float* W, const float* up, const float* down, int N, int K, int r, float scale, hipStream_t s, int* launched) {
    if (launched) *launched = 0;
    if (!W || !up || !down) return set_error(GL_ERR_ARG, "lora_merge: null W / up / down");
    if (N < 1 || K < 1 || r < 1) return set_error(GL_ERR_ARG, "lora_merge: N, K and r must be positive (N %d, K %d, r %d)", N, K, r);
    const size_t w_bytes = (size_t)N * K * sizeof(float), up_bytes = (size_t)N * r * sizeof(float), dn_bytes = (size_t)r * K * sizeof(float);
    if (overlaps(W, w_bytes, up, up_bytes)) return set_error(GL_ERR_ARG, "lora_merge: W overlaps up (the update is in place: the factors must lie elsewhere)");
    if (overlaps(W, w_bytes, down, dn_bytes)) return set_error(GL_ERR_ARG, "lora_merge: W overlaps down (the update is in place: the factors must lie elsewhere)");
    if (scale == 0.f) return GL_OK;                          // W + 0 * (up @ down): nothing is read or written, W keeps its bits
    const int64_t tiles_k = cdiv64(K, kTileK), tiles = tiles_k * cdiv64(N, kTileN);
    if (tiles > 0x7fffffff) return set_error(GL_ERR_UNSUPPORTED, "lora_merge: %d x %d has %lld tiles, more than one grid holds", N, K, (long long)tiles);
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, s, W, up, down, N, K, r, scale, (int)tiles_k);
    GL_LAUNCH_CHECK();
    if (launched) *launched = 1;
    return GL_OK;
}

}  // namespace gl
