// Pillow's 8-bit resampler on the device (see image.h). The arithmetic is integer from the coefficient tables on: products of a
// u8 sample with a coefficient of at most 23 bits + sign, accumulated in int32 on top of the rounding half, shifted right
// arithmetically by 22 and clamped to 0..255 -- after the horizontal pass (the u8 intermediate is part of the result) and again
// after the vertical one. A pass over an axis that keeps its size is Pillow's "skipped pass": here a one-tap table whose
// coefficient is 2^22, which the same formula turns into a copy.
#include "image.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

namespace gl {

// ---------------------------------------------------------------- coefficient tables (host, double)
namespace {

// No fused multiply-add in these three functions: the tables are defined by separately rounded double operations, and one
// contraction moves an entry.
double bicubic_filter(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

double bilinear_filter(double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

void compute_axis(int in, int out, int filter, ResampleAxis& t) {
#pragma clang fp contract(off)
    const double filter_support = filter == 0 ? 2.0 : 1.0;
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support * fs;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    t.ksize = ksize;
    t.bounds.assign((size_t)out * 2, 0);
    t.kk.assign((size_t)out * ksize, 0);
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double arg = (x + xmin - center + 0.5) / fs;
            w[x] = filter == 0 ? bicubic_filter(arg) : bilinear_filter(arg);
            ww += w[x];
        }
        int* k = &t.kk[(size_t)xx * ksize];
        for (int x = 0; x < xmax; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << kImagePrecisionBits)) : (int)(0.5 + v * (1 << kImagePrecisionBits));
        }
        t.bounds[(size_t)xx * 2] = xmin;
        t.bounds[(size_t)xx * 2 + 1] = xmax;
    }
}

}  // namespace

int resample_axis(int in, int out, int filter, std::shared_ptr<const ResampleAxis>* axis) {
    if (filter != 0 && filter != 1) return set_error(GL_ERR_UNSUPPORTED, "image resample: filter %d; the resampler has bicubic (0) and bilinear (1)", filter);
    if (in < 1 || in > kImageMaxSide) return set_error(GL_ERR_UNSUPPORTED, "image resample: a source side of %d is outside the limit of 1 .. %d", in, kImageMaxSide);
    if (out < 1 || out > kImageMaxSide) return set_error(GL_ERR_UNSUPPORTED, "image resample: a resized side of %d is outside the limit of 1 .. %d", out, kImageMaxSide);
    static std::mutex mu;
    static std::map<std::tuple<int, int, int>, std::shared_ptr<const ResampleAxis>> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(std::make_tuple(in, out, filter));
    if (it == cache.end()) {
        if (cache.size() >= kImageAxisCacheEntries) cache.clear();   // a service that sees every image size once must not grow for ever
        auto t = std::make_shared<ResampleAxis>();
        compute_axis(in, out, filter, *t);
        it = cache.emplace(std::make_tuple(in, out, filter), std::move(t)).first;
    }
    *axis = it->second;
    return GL_OK;
}

// ---------------------------------------------------------------- kernels
namespace {

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> kImagePrecisionBits, 0), 255); }

__device__ __forceinline__ int job_of_block(const ImageJob* jobs, int S, bool vertical) {
    int i = 0;   // S is a handful of images: a wave-uniform scan
    while (i + 1 < S && (int)blockIdx.x >= (vertical ? jobs[i + 1].vblock0 : jobs[i + 1].hblock0)) ++i;
    return i;
}

// Horizontal pass. One thread makes 4 neighbouring output pixels of one source row (12 bytes, stored as three words); consecutive
// lanes take consecutive pixel quads, so the coefficient words (tap-major table) and the stores are contiguous along x and the
// source bytes of a wave are one stretch of the row. Columns beyond the crop's width (cwp - cw <= 3) repeat the last column.
__global__ __launch_bounds__(256) void image_resample_h_kernel(const ImageJob* __restrict__ jobs, int S) {
    const ImageJob& j = jobs[job_of_block(jobs, S, false)];
    const int nq = j.cwp >> 2;
    const int item = ((int)blockIdx.x - j.hblock0) * 256 + (int)threadIdx.x;   // nrows * nq <= 16384 * 4096
    if (item >= j.nrows * nq) return;
    const int r = item / nq, q = item - r * nq;
    const uint8_t* __restrict__ row = j.src + (size_t)(j.row0 + r) * j.src_stride;
    const int4 x0 = *reinterpret_cast<const int4*>(j.hx + 4 * q);
    const int xs[4] = {x0.x, x0.y, x0.z, x0.w};
    const int last = j.W - 1, cwp = j.cwp, hks = j.hks;
    int acc[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p][0] = acc[p][1] = acc[p][2] = 1 << (kImagePrecisionBits - 1);
    const int* __restrict__ kp = j.hk + 4 * q;
    for (int k = 0; k < hks; ++k, kp += cwp) {
        const int4 c4 = *reinterpret_cast<const int4*>(kp);
        const int c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint8_t* s = row + 3 * min(xs[p] + k, last);   // a tap beyond the count has coefficient 0: any valid sample will do
            acc[p][0] += (int)s[0] * c[p];
            acc[p][1] += (int)s[1] * c[p];
            acc[p][2] += (int)s[2] * c[p];
        }
    }
    uint32_t w[3] = {0, 0, 0};
#pragma unroll
    for (int b = 0; b < 12; ++b) w[b >> 2] |= (uint32_t)clip8(acc[b / 3][b % 3]) << (8 * (b & 3));
    uint32_t* o = reinterpret_cast<uint32_t*>(j.mid + (size_t)r * j.mid_stride) + 3 * q;
    o[0] = w[0];
    o[1] = w[1];
    o[2] = w[2];
}

// Vertical pass. A wave owns one output row (its coefficient row and bounds are wave-uniform: scalar loads), a lane 4 consecutive
// bytes of it; the rows of the intermediate are read as words along x. F32: each byte goes through the 3 x 256 table of its channel
// into the planar fp32 image; otherwise the bytes are the output row.
template <bool F32>
__global__ __launch_bounds__(256) void image_resample_v_kernel(const ImageJob* __restrict__ jobs, int S, const float* __restrict__ lut) {
    __shared__ float lut_s[F32 ? 768 : 1];
    if (F32) {
        for (int t = threadIdx.x; t < 768; t += 256) lut_s[t] = lut[t];
        __syncthreads();
    }
    const ImageJob& j = jobs[job_of_block(jobs, S, true)];
    const int lb = (int)blockIdx.x - j.vblock0;
    const int by = lb / j.vbx, bx = lb - by * j.vbx;
    const int y = by * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int q = bx * 64 + ((int)threadIdx.x & 63);
    if (y >= j.ch || q >= (j.mid_stride >> 2)) return;
    const int first = j.vy[y] - j.row0, last = j.nrows - 1, vks = j.vks;
    const int* __restrict__ kk = j.vk + (size_t)y * vks;
    const uint8_t* __restrict__ col = j.mid + 4 * q;
    const size_t stride = j.mid_stride;
    int acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = 1 << (kImagePrecisionBits - 1);
    for (int k = 0; k < vks; ++k) {
        const int c = kk[k];
        const uint32_t v = *reinterpret_cast<const uint32_t*>(col + (size_t)min(first + k, last) * stride);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] += (int)((v >> (8 * t)) & 255u) * c;
    }
    const int cw = j.cw, ch = j.ch;
    if (F32) {
        float* o = reinterpret_cast<float*>(j.out);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int b = 4 * q + t, x = b / 3, c = b - 3 * x;
            if (x < cw) o[((size_t)c * ch + y) * cw + x] = lut_s[c * 256 + clip8(acc[t])];
        }
    } else {
        uint8_t* o = reinterpret_cast<uint8_t*>(j.out) + (size_t)y * cw * 3 + 4 * q;
        const int left = cw * 3 - 4 * q;   // bytes of the row from this lane's first on (<= 0 in the padding)
        if (left >= 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            uint32_t w = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) w |= (uint32_t)clip8(acc[t]) << (8 * t);
            *reinterpret_cast<uint32_t*>(o) = w;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < left) o[t] = (uint8_t)clip8(acc[t]);
        }
    }
}

size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace

// ---------------------------------------------------------------- host
ImageStage::~ImageStage() {
    if (copied) (void)hipEventDestroy(copied);
    if (host) (void)hipHostFree(host);
}

int image_resample_plan(const gl_image_desc* images, int S, int filter, int out_kind, const float* lut_host, void* out, ImagePlan* plan) {
    if (!images || !out || !plan || S < 1) return set_error(GL_ERR_ARG, "image resample: null images / out, or no image");
    if (filter != 0 && filter != 1) return set_error(GL_ERR_UNSUPPORTED, "image resample: filter %d; the resampler has bicubic (0) and bilinear (1)", filter);
    if (out_kind != 0 && out_kind != 1) return set_error(GL_ERR_ARG, "image resample: out_kind %d; 0 = u8 [ch][cw][3] per image, 1 = fp32 [S][3][ch][cw]", out_kind);
    if (out_kind == 1 && !lut_host) return set_error(GL_ERR_ARG, "image resample: the fp32 output needs the 3 x 256 look-up table");
    struct Axes { std::shared_ptr<const ResampleAxis> h, v; };   // empty: the axis keeps its size (a copy)
    std::vector<Axes> axes(S);
    for (int i = 0; i < S; ++i) {
        const gl_image_desc& d = images[i];
        if (!d.pixels) return set_error(GL_ERR_ARG, "image resample: image %d has no pixels", i);
        if (d.width < 1 || d.height < 1 || d.width > kImageMaxSide || d.height > kImageMaxSide)
            return set_error(GL_ERR_UNSUPPORTED, "image resample: image %d is %d x %d; a source side is limited to 1 .. %d", i, d.width, d.height, kImageMaxSide);
        if (d.resized_w < 1 || d.resized_h < 1 || d.resized_w > kImageMaxSide || d.resized_h > kImageMaxSide)
            return set_error(GL_ERR_UNSUPPORTED, "image resample: image %d is resized to %d x %d; a resized side is limited to 1 .. %d", i, d.resized_w,
                             d.resized_h, kImageMaxSide);
        if (d.row_stride < 3 * d.width)
            return set_error(GL_ERR_ARG, "image resample: image %d has a row stride of %d bytes, less than its 3 x %d interleaved u8 channels", i, d.row_stride, d.width);
        if (d.crop_x < 0 || d.crop_y < 0 || d.crop_w < 1 || d.crop_h < 1 || d.crop_x > d.resized_w - d.crop_w || d.crop_y > d.resized_h - d.crop_h)
            return set_error(GL_ERR_ARG, "image resample: image %d: the crop box (%d, %d, %d x %d) does not lie inside the resized %d x %d", i, d.crop_x, d.crop_y,
                             d.crop_w, d.crop_h, d.resized_w, d.resized_h);
        if (out_kind == 1 && (d.crop_w != images[0].crop_w || d.crop_h != images[0].crop_h))
            return set_error(GL_ERR_ARG, "image resample: the fp32 output is one [S][3][ch][cw] tensor: image %d is cropped to %d x %d, image 0 to %d x %d", i,
                             d.crop_w, d.crop_h, images[0].crop_w, images[0].crop_h);
        if (d.width != d.resized_w) GL_TRY(resample_axis(d.width, d.resized_w, filter, &axes[i].h));
        if (d.height != d.resized_h) GL_TRY(resample_axis(d.height, d.resized_h, filter, &axes[i].v));
    }
    // layout of the block: jobs | look-up table | per image: hx, hk, vy, vk ; behind the block: per image the intermediate
    size_t off = up256((size_t)S * sizeof(ImageJob));
    plan->lut_off = off;
    if (out_kind == 1) off = up256(off + 768 * sizeof(float));
    std::vector<ImageJob> jobs(S);
    std::vector<size_t> tab(S);
    int hblocks = 0, vblocks = 0;
    for (int i = 0; i < S; ++i) {
        const gl_image_desc& d = images[i];
        ImageJob& j = jobs[i];
        j.cw = d.crop_w, j.ch = d.crop_h, j.cwp = round_up(d.crop_w, 4), j.mid_stride = 3 * j.cwp;
        j.hks = axes[i].h ? axes[i].h->ksize : 1;
        j.vks = axes[i].v ? axes[i].v->ksize : 1;
        tab[i] = off;
        off = up256(off + ((size_t)j.cwp * (1 + j.hks) + (size_t)j.ch * (1 + j.vks)) * sizeof(int));
    }
    const size_t block_bytes = off;
    plan->block.assign(block_bytes, 0);
    char* base = plan->block.data();
    if (out_kind == 1) memcpy(base + plan->lut_off, lut_host, 768 * sizeof(float));
    for (int i = 0; i < S; ++i) {
        const gl_image_desc& d = images[i];
        ImageJob& j = jobs[i];
        int* hx = reinterpret_cast<int*>(base + tab[i]);
        int* hk = hx + j.cwp;
        int* vy = hk + (size_t)j.hks * j.cwp;
        int* vk = vy + j.ch;
        for (int x = 0; x < j.cwp; ++x) {
            const int xx = d.crop_x + std::min(x, j.cw - 1);
            hx[x] = axes[i].h ? axes[i].h->bounds[(size_t)xx * 2] : xx;
            for (int k = 0; k < j.hks; ++k) hk[(size_t)k * j.cwp + x] = axes[i].h ? axes[i].h->kk[(size_t)xx * j.hks + k] : 1 << kImagePrecisionBits;
        }
        int lo = d.height, hi = 0;
        for (int y = 0; y < j.ch; ++y) {
            const int yy = d.crop_y + y;
            const int y0 = axes[i].v ? axes[i].v->bounds[(size_t)yy * 2] : yy;
            const int n = axes[i].v ? axes[i].v->bounds[(size_t)yy * 2 + 1] : 1;
            vy[y] = y0;
            for (int k = 0; k < j.vks; ++k) vk[(size_t)y * j.vks + k] = axes[i].v ? axes[i].v->kk[(size_t)yy * j.vks + k] : 1 << kImagePrecisionBits;
            lo = std::min(lo, y0), hi = std::max(hi, y0 + n);
        }
        j.row0 = lo, j.nrows = hi - lo;   // 1 <= nrows, row0 + nrows <= H: the rows the vertical pass of the cropped rows reads
        j.src = d.pixels, j.src_stride = d.row_stride, j.W = d.width;
        j.out = out_kind == 1 ? static_cast<void*>(static_cast<float*>(out) + (size_t)i * 3 * j.ch * j.cw) : static_cast<void* const*>(out)[i];
        if (!j.out) return set_error(GL_ERR_ARG, "image resample: image %d has no output pointer", i);
        // addresses inside the workspace: offsets for now
        j.hx = reinterpret_cast<const int*>(tab[i]);
        j.hk = reinterpret_cast<const int*>(tab[i] + (size_t)j.cwp * sizeof(int));
        j.vy = reinterpret_cast<const int*>(tab[i] + (size_t)j.cwp * (1 + j.hks) * sizeof(int));
        j.vk = reinterpret_cast<const int*>(tab[i] + ((size_t)j.cwp * (1 + j.hks) + j.ch) * sizeof(int));
        j.mid = reinterpret_cast<uint8_t*>(off);
        off = up256(off + (size_t)j.nrows * j.mid_stride);
        j.hblock0 = hblocks, j.vblock0 = vblocks;
        j.vbx = cdiv(j.mid_stride / 4, 64);
        hblocks += cdiv(j.nrows * (j.cwp / 4), 256);
        vblocks += j.vbx * cdiv(j.ch, 4);
    }
    memcpy(base, jobs.data(), (size_t)S * sizeof(ImageJob));
    plan->work_bytes = off;
    plan->S = S, plan->out_kind = out_kind, plan->hblocks = hblocks, plan->vblocks = vblocks;
    return GL_OK;
}

int image_stage_upload(ImageStage& stage, const void* block, size_t bytes, void* dst, hipStream_t stream) {
    if (!stage.copied) GL_HIP(hipEventCreateWithFlags(&stage.copied, hipEventDisableTiming));
    if (stage.pending) {   // the previous call's copy out of the staging memory (long over by now; never the kernels behind it)
        GL_HIP(hipEventSynchronize(stage.copied));
        stage.pending = false;
    }
    if (stage.cap < bytes) {
        if (stage.host) GL_HIP(hipHostFree(stage.host));
        stage.host = nullptr, stage.cap = 0;
        const size_t cap = std::max(bytes * 2, size_t(1) << 20);
        GL_HIP(hipHostMalloc(&stage.host, cap, hipHostMallocDefault));
        stage.cap = cap;
    }
    memcpy(stage.host, block, bytes);
    GL_HIP(hipMemcpyAsync(dst, stage.host, bytes, hipMemcpyHostToDevice, stream));
    GL_HIP(hipEventRecord(stage.copied, stream));
    stage.pending = true;
    return GL_OK;
}

int image_resample_run(ImageStage& stage, ImagePlan& plan, void* work, hipStream_t stream) {
    if (!work || (reinterpret_cast<uintptr_t>(work) & 255)) return set_error(GL_ERR_ARG, "image resample: the workspace must be 256-byte aligned");
    ImageJob* jobs = reinterpret_cast<ImageJob*>(plan.block.data());
    const uintptr_t b = reinterpret_cast<uintptr_t>(work);
    for (int i = 0; i < plan.S; ++i) {
        ImageJob& j = jobs[i];
        j.hx = reinterpret_cast<const int*>(b + reinterpret_cast<uintptr_t>(j.hx));
        j.hk = reinterpret_cast<const int*>(b + reinterpret_cast<uintptr_t>(j.hk));
        j.vy = reinterpret_cast<const int*>(b + reinterpret_cast<uintptr_t>(j.vy));
        j.vk = reinterpret_cast<const int*>(b + reinterpret_cast<uintptr_t>(j.vk));
        j.mid = reinterpret_cast<uint8_t*>(b + reinterpret_cast<uintptr_t>(j.mid));
    }
    GL_TRY(image_stage_upload(stage, plan.block.data(), plan.block.size(), work, stream));
    plan.block.clear();   // the addresses are in: a plan runs once
    const ImageJob* djobs = static_cast<const ImageJob*>(work);
    const float* dlut = reinterpret_cast<const float*>(static_cast<const char*>(work) + plan.lut_off);
    hipLaunchKernelGGL(image_resample_h_kernel, dim3(plan.hblocks), dim3(256), 0, stream, djobs, plan.S);
    GL_LAUNCH_CHECK();
    if (plan.out_kind == 1)
        hipLaunchKernelGGL(image_resample_v_kernel<true>, dim3(plan.vblocks), dim3(256), 0, stream, djobs, plan.S, dlut);
    else
        hipLaunchKernelGGL(image_resample_v_kernel<false>, dim3(plan.vblocks), dim3(256), 0, stream, djobs, plan.S, dlut);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
