/* gligen_amd_tiling.h -- tiled passes through the autoencoder in libgligen_amd.so: decode (encode) an image as overlapping tiles of
 * a fixed size, each an ordinary pass through the decoder (encoder), blended across their overlaps into the full tensor. The arena's
 * high-water mark then depends on the tile and on the tiles per pass, not on the image. NOT the untiled result: GroupNorm statistics
 * and the mid-block attention are those of each tile. Conventions as in gligen_amd.h. */
#ifndef GLIGEN_AMD_TILING_H
#define GLIGEN_AMD_TILING_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A plan: ny x nx tiles per image, every tile th_in x tw_in on the input grid and th_out x tw_out on the output grid (decode: latent
 * -> image, out = f in; encode: image -> latent, in = f out; f = 2^(n_mult - 1)). Tile (b, ty, tx) has the index (b ny + ty) nx + tx.
 * All tables are DEVICE memory and are read by the launches of the call, stream-ordered:
 *   windows  int32 [B ny nx][3]: (b, oy, ox) of each tile on the input grid, in index order;
 *   oy, ox   int32 [ny], [nx]: the origins on the output grid;
 *   wy, wx   fp32 [ny][th_out], [nx][tw_out]: the per-axis weights; at every coordinate the weights of the covering tiles sum to 1.
 * gligen_amd/vae_tiling.py builds one (tile_plan, weight_tables). ny == nx == 1 is the untiled pass: the tables are not read. */
typedef struct gl_tile_plan {
    unsigned struct_size;   /* sizeof(gl_tile_plan): a caller built against another layout is refused */
    int ny, nx;
    int th_in, tw_in, th_out, tw_out;
    const int* windows;
    const int* oy;
    const int* ox;
    const float* wy;
    const float* wx;
} gl_tile_plan;

/* gl_vae_decode over tiles: z fp32 [B][zc][h][w] -> img fp32 [B][out_ch][f h][f w]. Per pass up to tiles_per_pass tiles (of any
 * images of the batch) are gathered into the arena, decoded as one batch by the launches of gl_vae_decode, and blended into img; the
 * arena is reset per pass. Every element of img is written; img is never read before its first write (no memset needed). With one
 * tile per axis this IS gl_vae_decode: the same launches, the same bits. Refused by name: a plan whose tiles do not match (h, w) and
 * f, th_in * tw_in no multiple of 64 (the AttnBlock), tiles_per_pass < 1. */
int gl_vae_decode_tiled(gl_ctx* ctx, int B, int h, int w, const float* z, float* img, const gl_tile_plan* plan, int tiles_per_pass, gl_stream s);

/* gl_vae_encode over tiles: img fp32 [B][3][H][W], noise fp32 [B][zc][H/f][W/f] -> z. The tiles' raw moments (the encoder's output
 * [2 zc] channels, before quant_conv) are blended into one tensor [B][2 zc][H/f][W/f]; quant_conv (1 x 1, so blending before it is the
 * same), the clamp of logvar and the draw mean + std * noise run once, on the blended tensor. moments_out (may be NULL) receives the
 * blended moments; without it they live at the bottom of the arena for the call. Window origins are multiples of f. With one tile per
 * axis this IS gl_vae_encode; moments_out, if given, is where its moments are written. */
int gl_vae_encode_tiled(gl_ctx* ctx, int B, int H, int W, const float* img, const float* noise, float* z, float* moments_out,
                        const gl_tile_plan* plan, int tiles_per_pass, gl_stream s);

/* The operators alone. gl_op_tile_gather: dst fp32 [n][C][TH][TW] = the windows src[b, :, oy : oy + TH, ox : ox + TW] of src fp32
 * [B][C][H][W], windows device int32 [n][3] rows (b, oy, ox); an exact copy; a row naming a window outside src is skipped. */
int gl_op_tile_gather(gl_ctx* ctx, const float* src, int B, int C, int H, int W, const int* windows, int n, float* dst, int TH, int TW, gl_stream s);

/* gl_op_tile_blend: tiles fp32 [n][C][th_out][tw_out] are the tiles first_tile .. first_tile + n - 1 of the plan (windows is not
 * read). Each element of out fp32 [B][C][H][W] belongs to one thread, which visits the covering tiles in ascending index: w = wy * wx,
 * the first covering tile of the whole plan gives w * v, every later one fma(w, v, sum so far) -- one chain per element, in fp32. If
 * a tile before first_tile covers the element, the chain continues from what out holds; otherwise out is overwritten; an element no
 * tile of this call covers is not touched. No atomics, no memset. Splitting a plan's tiles over several calls, in ascending order,
 * therefore gives the bits of one call. */
int gl_op_tile_blend(gl_ctx* ctx, const float* tiles, int first_tile, int n, const gl_tile_plan* plan, float* out, int B, int C, int H, int W,
                     gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
