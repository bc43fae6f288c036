// Tiled autoencoder passes (include/gligen_amd_tiling.h): tile_gather_kernel (K18) cuts fixed-size windows out of an fp32 NCHW tensor
// -- latent tiles for the decoder (C = 4), image tiles for the encoder (C = 3) --, tile_blend_kernel (K19) writes the weighted sum of
// the tiles that cover each output element. Both are bandwidth-bound copies with a little index arithmetic: one lane per group of four
// consecutive elements of a row, lanes along x, so a wave's loads and stores are contiguous row segments; where the row length, the
// tile width, the tile's x origin and the base pointers are all multiples of four elements (16 bytes) the group moves as one float4,
// otherwise element by element (odd widths, origins on a latent grid). Grid-stride with a capped grid, as the kernels of misc.hip.
#include "tile.h"

namespace gl {

namespace {

constexpr int kMaxBlocks = 4096;

inline int grid_for(int64_t n) {
    int64_t g = cdiv64(n, 256);
    return (int)(g > kMaxBlocks ? kMaxBlocks : g < 1 ? 1 : g);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// K18. vec: W % 4 == 0, TW % 4 == 0, src and dst 16-byte aligned (the launch checks); a window whose ox is no multiple of 4 still goes
// element by element. A window that does not lie inside src is skipped: nothing is read or written out of bounds whatever the list holds.
__global__ void __launch_bounds__(256) tile_gather_kernel(const float* __restrict__ src, int B, int C, int H, int W, const int* __restrict__ windows,
                                                          float* __restrict__ dst, int TH, int TW, int vec, size_t groups) {
    const int TW4 = (TW + 3) >> 2;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        const size_t row = g / (size_t)TW4;
        const int lx = (int)(g - row * (size_t)TW4) * 4;
        const size_t pl = row / (size_t)TH;                       // tile * C + c
        const int ly = (int)(row - pl * (size_t)TH);
        const size_t t = pl / (size_t)C;
        const int c = (int)(pl - t * (size_t)C);
        const int b = windows[3 * t], oy = windows[3 * t + 1], ox = windows[3 * t + 2];
        if (b < 0 || b >= B || oy < 0 || ox < 0 || oy > H - TH || ox > W - TW) continue;
        const float* in = src + (((size_t)b * C + c) * H + (oy + ly)) * (size_t)W + (ox + lx);
        float* out = dst + row * (size_t)TW + lx;
        if (vec && !(ox & 3)) {
            *reinterpret_cast<float4*>(out) = *reinterpret_cast<const float4*>(in);
        } else {
            const int nv = TW - lx < 4 ? TW - lx : 4;
            for (int j = 0; j < nv; ++j) out[j] = in[j];
        }
    }
}

// K19. One lane owns four consecutive elements of one output row and nobody else writes them: no atomics, no memset of out.
//
// ORDER OF OPERATIONS, per element, fixed so that splitting the tile list over several calls does not change a bit: the covering tiles
// are visited in ascending tile index (b, ty, tx); the weight is w = wy * wx (one rounded product); the FIRST covering tile of the
// whole list gives acc = w * v (one rounded product), every later one acc = fma(w, v, acc) (one rounding). The value is thus one
// left-to-right chain over all covering tiles. A call whose range starts in the middle of an element's chain (a tile of an earlier
// call, index < first, covers the element too) reads what out holds -- the chain so far, stored exactly, being fp32 -- and continues
// it with the same fma; it never forms a partial sum of its own. Tiles of later calls (index >= first + n) are ignored, an element
// that no tile of this call covers is neither read nor written. Contraction is off: the products above are the only ones fused.
// The grid covers the images b0 .. of the batch that own a tile of this call (the launch works that out from the tile indices).
__global__ void __launch_bounds__(256) tile_blend_kernel(const float* __restrict__ tiles, int first, int n, TileBlendPlan p, float* __restrict__ out,
                                                         int b0, int C, int H, int W, int vec, size_t groups) {
#pragma clang fp contract(off)
    const int W4 = (W + 3) >> 2;
    const int TH = p.TH, TW = p.TW;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        const size_t row = g / (size_t)W4 + (size_t)b0 * C * H;
        const int x0 = (int)(g % (size_t)W4) * 4;
        const size_t pl = row / (size_t)H;                        // b * C + c
        const int y = (int)(row - pl * (size_t)H);
        const int b = (int)(pl / (size_t)C);
        const int c = (int)(pl - (size_t)b * C);
        const int nv = W - x0 < 4 ? W - x0 : 4;
        float* o = out + row * (size_t)W + x0;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        bool has[4] = {false, false, false, false}, prev[4] = {false, false, false, false};
        for (int ty = 0; ty < p.ny; ++ty) {
            const int ly = y - p.oy[ty];
            if (ly < 0 || ly >= TH) continue;
            const float wy = p.wy[(size_t)ty * TH + ly];
            for (int tx = 0; tx < p.nx; ++tx) {
                const int ox = p.ox[tx];
                const int lx0 = x0 - ox;
                if (lx0 <= -4 || lx0 >= TW) continue;
                const int id = (b * p.ny + ty) * p.nx + tx;
                if (id >= first + n) continue;
                if (id < first) {
                    for (int j = 0; j < nv; ++j) prev[j] = prev[j] || (lx0 + j >= 0 && lx0 + j < TW);
                    continue;
                }
                const float* tv = tiles + (((size_t)(id - first) * C + c) * TH + ly) * (size_t)TW;
                const float* wxr = p.wx + (size_t)tx * TW;
                float v[4], wx[4];
                bool in[4];
                if (vec && !(ox & 3)) {                           // then lx0 % 4 == 0 and 0 <= lx0 <= TW - 4: the group is covered as one
                    const float4 v4 = *reinterpret_cast<const float4*>(tv + lx0), w4 = *reinterpret_cast<const float4*>(wxr + lx0);
                    v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
                    wx[0] = w4.x; wx[1] = w4.y; wx[2] = w4.z; wx[3] = w4.w;
                    in[0] = in[1] = in[2] = in[3] = true;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int lx = lx0 + j;
                        in[j] = j < nv && lx >= 0 && lx < TW;
                        v[j] = in[j] ? tv[lx] : 0.f;
                        wx[j] = in[j] ? wxr[lx] : 0.f;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!in[j]) continue;
                    const float w = __fmul_rn(wy, wx[j]);
                    if (has[j]) acc[j] = __fmaf_rn(w, v[j], acc[j]);
                    else acc[j] = prev[j] ? __fmaf_rn(w, v[j], o[j]) : __fmul_rn(w, v[j]);
                    has[j] = true;
                }
            }
        }
        if (vec && has[0] && has[1] && has[2] && has[3]) {
            *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (has[j]) o[j] = acc[j];
        }
    }
}

}  // namespace

int tile_gather_launch(const float* src, int B, int C, int H, int W, const int* windows, int n, float* dst, int TH, int TW, hipStream_t s) {
    if (!src || !windows || !dst) return set_error(GL_ERR_ARG, "tile_gather: null src / windows / dst");
    if (B < 1 || C < 1 || H < 1 || W < 1 || n < 1 || TH < 1 || TW < 1 || TH > H || TW > W)
        return set_error(GL_ERR_ARG, "tile_gather: B %d, C %d, %d x %d, %d tiles of %d x %d (all positive, the tile no larger than the tensor)", B, C, H, W, n, TH, TW);
    const int vec = !(W & 3) && !(TW & 3) && aligned16(src) && aligned16(dst);
    const size_t groups = (size_t)n * C * TH * ((TW + 3) >> 2);
    hipLaunchKernelGGL(tile_gather_kernel, dim3(grid_for((int64_t)groups)), dim3(256), 0, s, src, B, C, H, W, windows, dst, TH, TW, vec, groups);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int tile_blend_launch(const float* tiles, int first_tile, int n, const TileBlendPlan& p, float* out, int B, int C, int H, int W, hipStream_t s) {
    if (!tiles || !out || !p.oy || !p.ox || !p.wy || !p.wx) return set_error(GL_ERR_ARG, "tile_blend: null tiles / out / plan table");
    if (B < 1 || C < 1 || H < 1 || W < 1 || p.ny < 1 || p.nx < 1 || p.TH < 1 || p.TW < 1 || p.TH > H || p.TW > W)
        return set_error(GL_ERR_ARG, "tile_blend: B %d, C %d, %d x %d, %d x %d tiles of %d x %d (all positive, the tile no larger than the tensor)", B, C, H, W,
                         p.ny, p.nx, p.TH, p.TW);
    const int64_t all = (int64_t)B * p.ny * p.nx;
    if (all > INT32_MAX || first_tile < 0 || n < 1 || (int64_t)first_tile + n > all)
        return set_error(GL_ERR_ARG, "tile_blend: tiles %d .. %d of %lld", first_tile, first_tile + n, (long long)all);
    const int vec = !(W & 3) && !(p.TW & 3) && aligned16(tiles) && aligned16(out) && aligned16(p.wx);
    const int per_image = p.ny * p.nx, b0 = first_tile / per_image, b1 = (first_tile + n - 1) / per_image;
    const size_t groups = (size_t)(b1 - b0 + 1) * C * H * ((W + 3) >> 2);
    hipLaunchKernelGGL(tile_blend_kernel, dim3(grid_for((int64_t)groups)), dim3(256), 0, s, tiles, first_tile, n, p, out, b0, C, H, W, vec, groups);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
