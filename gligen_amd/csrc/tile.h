// Tiled autoencoder passes (K18, K19): cut windows out of an fp32 NCHW tensor, and blend fp32 NCHW tiles back into one tensor with
// separable weights that sum to 1 over the tiles covering an element. See tile.hip; entry points in include/gligen_amd_tiling.h.
#pragma once
#include "common.h"

namespace gl {

// dst [n][C][TH][TW] = src [B][C][H][W] windows: tile j is src[b_j, :, oy_j : oy_j + TH, ox_j : ox_j + TW], windows = device int32
// [n][3] rows (b, oy, ox). An exact copy. A row that names a window outside src is skipped by the kernel (its tile is not written).
int tile_gather_launch(const float* src, int B, int C, int H, int W, const int* windows, int n, float* dst, int TH, int TW, hipStream_t s);

// The geometry of a blend: ny x nx tiles of TH x TW output elements per image; tile (b, ty, tx) has the index (b ny + ty) nx + tx and
// sits at (oy[ty], ox[tx]). oy [ny], ox [nx] device int32; wy [ny][TH], wx [nx][TW] device fp32.
struct TileBlendPlan {
    int ny, nx, TH, TW;
    const int* oy;
    const int* ox;
    const float* wy;
    const float* wx;
};

// out [B][C][H][W] (+)= sum over the tiles first_tile <= t < first_tile + n that cover the element of wy wx tiles[t - first_tile].
// An element no such tile covers is not touched; one that a tile t < first_tile covers too continues from what out holds.
int tile_blend_launch(const float* tiles, int first_tile, int n, const TileBlendPlan& p, float* out, int B, int C, int H, int W, hipStream_t s);

}  // namespace gl
