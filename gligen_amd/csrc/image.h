// CLIP image front end: Pillow's 8-bit resampler (ImagingResample: separable, fixed-point coefficients, u8 between the passes), a
// crop box and the normalisation, bit for bit, for a batch of images of different sizes in two launches.
#pragma once
#include <memory>
#include <vector>

#include "common.h"
#include "../../include/gligen_amd_image.h"

namespace gl {

constexpr int kImageMaxSide = 16384;   // source and resized sides
constexpr int kImagePrecisionBits = 22;   // Pillow's PRECISION_BITS for 8-bit samples: 32 - 8 - 2

// One axis of the resampler: for each of `out` samples the first source sample, the number of taps and `ksize` fixed-point
// coefficients (those beyond the count are 0), as Pillow's precompute_coeffs + normalize_coeffs_8bpc leave them.
struct ResampleAxis {
    int ksize = 0;
    std::vector<int> bounds;   // [out][2]: first sample, count
    std::vector<int> kk;       // [out][ksize]
};
// filter: 0 bicubic (a = -0.5, support 2), 1 bilinear (support 1). Host only, computed in double; cached per (in, out, filter) -- the
// cache is emptied when it holds kImageAxisCacheEntries tables, a table lives as long as someone holds it. Sizes outside
// [1, kImageMaxSide] and other filters are refused by name.
constexpr size_t kImageAxisCacheEntries = 256;
int resample_axis(int in, int out, int filter, std::shared_ptr<const ResampleAxis>* axis);

// what one launch pair reads on the device: the descriptor of an image with its tables (device addresses)
struct ImageJob {
    const uint8_t* src;   // [H][W][3] u8, rows src_stride bytes apart
    uint8_t* mid;         // [nrows][mid_stride] u8: the horizontal pass of source rows row0 .. row0 + nrows, cropped columns only
    void* out;            // u8 [ch][cw][3], or fp32 plane 0 of this image's [3][ch][cw]
    const int* hx;        // [cwp] first source column of each cropped output column
    const int* hk;        // [hks][cwp] its coefficients, tap-major: lanes along x read consecutive words
    const int* vy;        // [ch] first source row of each cropped output row
    const int* vk;        // [ch][vks] its coefficients: one row per wave, read through the scalar cache
    int src_stride, W;
    int row0, nrows;
    int cw, ch, cwp, mid_stride;   // cwp = cw rounded up to 4 pixels, mid_stride = 3 cwp
    int hks, vks;
    int hblock0, vblock0, vbx;     // first workgroup of this image in either launch; workgroups along x in the vertical one
};

// Everything a call has decided on the host: the block that is copied to the device (jobs, look-up table, tables; the addresses in
// `jobs` are offsets until image_resample_run adds the workspace's base) and the size of the workspace (that block + intermediates).
struct ImagePlan {
    std::vector<char> block;
    size_t work_bytes = 0;
    size_t lut_off = 0;
    int S = 0, out_kind = 0, hblocks = 0, vblocks = 0;
};

// Pinned staging memory for the block, reused by the next call once its copy has left the host.
struct ImageStage {
    void* host = nullptr;
    size_t cap = 0;
    hipEvent_t copied = nullptr;
    bool pending = false;
    ~ImageStage();
};
// Copies `bytes` of host memory to `dst` on `stream` through the staging memory (grown as needed). Waits, on the host, only for the
// previous call's copy to have left the staging memory; the device is never waited for.
int image_stage_upload(ImageStage& stage, const void* block, size_t bytes, void* dst, hipStream_t stream);

// Validates the call (gl_op_image_resample's arguments) and lays it out. Host only: touches no device.
int image_resample_plan(const gl_image_desc* images, int S, int filter, int out_kind, const float* lut_host, void* out, ImagePlan* plan);
// `work`: plan.work_bytes of device memory, 256-byte aligned, the caller's until `stream` has passed the two launches. One
// host-to-device copy and two launches on `stream`; the device is never waited for.
int image_resample_run(ImageStage& stage, ImagePlan& plan, void* work, hipStream_t stream);

}  // namespace gl
