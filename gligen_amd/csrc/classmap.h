// Semantic maps as class indices. A u8 class map stands for its one-hot fp32 planes: nearest resize of one-hot planes is the one-hot
// of the nearest resize of the indices, and a convolution over one-hot planes is a sum of one weight per tap. The planes' kernels
// (resize_f32_kernel, conv3x3_f32_kernel, conv4x4s2_f32_kernel) start from the bias and add the products in (channel, ky, kx) order;
// a product with 0 leaves the sum as it is and a product with 1 adds the weight, so adding the taps' weights in ascending
// (class, tap) order gives the same bits. Plus Pillow's crop + nearest resize of such maps, byte for byte.
#pragma once
#include <vector>

#include "common.h"
#include "image.h"
#include "../../include/gligen_amd_maps.h"

namespace gl {

constexpr int kClassMapMaxSide = 16384;   // source, box and resized sides
constexpr int kClassMapMaxMaps = 1024;    // maps of one gl_op_class_map_resize call
constexpr int kClassMaxClasses = 256;     // a class is one u8

// Pillow's nearest index table of one axis (ImagingScaleAffine: accumulated in double), + box0. Host only; refuses sizes outside
// [1, kClassMapMaxSide] by name.
int class_map_index_table(int box0, int box_len, int out, int* idx);

// what the resize launch reads on the device: one map and where its tables start in the table array (ints)
struct ClassMapJob {
    const uint8_t* src;   // [H][W] u8, rows src_stride bytes apart
    int src_stride;
    int tx, ty;           // first entry of the [out_w] column table (16-byte aligned) and of the [out_h] row table
};
// the block that is copied to the device: jobs | tables
struct ClassMapPlan {
    std::vector<char> block;
    size_t tab_off = 0;
    int S = 0, out_w = 0, out_h = 0;
};
// Validates the call (gl_op_class_map_resize's arguments) and lays it out. Host only: touches no device.
int class_map_resize_plan(const gl_class_map_desc* maps, int S, int out_w, int out_h, const uint8_t* out, ClassMapPlan* plan);
// `work`: plan.block.size() bytes of device memory, 256-byte aligned, the caller's until `stream` has passed the launch. One
// host-to-device copy and one launch on `stream`; the device is never waited for.
int class_map_resize_run(ImageStage& stage, ClassMapPlan& plan, void* work, uint8_t* out, hipStream_t stream);

// F.interpolate(one_hot(cls), R, mode="nearest") + Conv2d(n_classes, 3, 3, 1, 1): cls u8 [B][H][W], w fp32 [3][n_classes][3][3]
// -> y fp32 [B][3][R][R]
int class_inconv_launch(const uint8_t* cls, const float* w, const float* bias, float* y, int B, int H, int W, int n_classes, int R, hipStream_t stream);
// w fp32 [c_out][n_classes][16] -> g fp32 [n_classes][16][c_out]: the weights one tap of one class adds, contiguous
int class_conv_weight_relayout_launch(const float* w, float* g, int c_out, int n_classes, hipStream_t stream);
// F.interpolate(one_hot(cls), R, mode="nearest") + Conv2d(n_classes, c_out, 4, 2, 1) (+ SiLU): g from the relayout
// -> y fp32 [B][c_out][R/2][R/2]; c_out a multiple of 4, R even
int class_conv4x4s2_launch(const uint8_t* cls, const float* g, const float* bias, float* y, int B, int H, int W, int n_classes, int c_out, int R, int silu,
                           hipStream_t stream);

// Weight and bias gradient of the two convs above, from the class map: with cls' the map seen through the nearest resize to R,
//   dW[o][c][ky][kx] = sum over (b, y, x) of [cls'(b, s y + ky - 1, s x + kx - 1) == c] dy[b][o][y][x],   db[o] = sum of dy[b][o][y][x]
// A tap in the padding or on a class >= n_classes adds nothing. kind: kClassWgradInConv (3 x 3, stride 1, c_out = 3) or kClassWgradDown
// (4 x 4, stride 2, c_out a multiple of 4, R even). dy: fp32, element (b, o, y, x) at the given strides (NCHW or pixel rows); dW fp32
// [c_out][n_classes][k][k] and db [c_out], either may be null. part: class_conv_wgrad_partial_floats floats of workspace. Two launches,
// no atomics: per-tile partials are added in tile order, so the result has the same bits every run.
constexpr int kClassWgradInConv = 0, kClassWgradDown = 1;
constexpr int kClassWgradMaxOut = 4096;
struct ClassDyStrides { size_t b, c, y, x; };
int class_conv_wgrad_partial_floats(int kind, int B, int H, int W, int n_classes, int c_out, int R, size_t* n);
int class_conv_wgrad_launch(int kind, const uint8_t* cls, const float* dy, ClassDyStrides ds, float* part, float* dW, float* db, int B, int H, int W, int n_classes,
                            int c_out, int R, hipStream_t stream);

}  // namespace gl
