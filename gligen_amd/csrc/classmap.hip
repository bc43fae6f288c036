// Semantic maps as class indices (see classmap.h): Pillow's crop + nearest resize of u8 class maps, and the two convolutions that
// read one-hot planes -- the tokenizer's in_conv and the downsampler's first conv -- as gathers of one weight per tap, fused with
// the nearest resize in front of them. Once per prompt: plain latency-bound kernels, a thread per output pixel. For training, the
// weight gradients of the same two convs as sums of dy binned by the class under each tap, in a fixed order.
#include "classmap.h"

#include <algorithm>
#include <cstring>

namespace gl {

// ---------------------------------------------------------------- index table (host, double)
namespace {

// Sequential accumulation in double, as ImagingScaleAffine builds xintab / yintab: no fused multiply-add, no closed form.
void nearest_axis(int box0, int box_len, int out, int* idx) {
#pragma clang fp contract(off)
    const double a = (double)box_len / out;
    double xo = a * 0.5;
    for (int x = 0; x < out; ++x) {
        idx[x] = box0 + std::min((int)xo, box_len - 1);   // (Pillow skips a sample outside the image; the sum never gets there)
        xo += a;
    }
}

size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace

int class_map_index_table(int box0, int box_len, int out, int* idx) {
    if (!idx) return set_error(GL_ERR_ARG, "class map index table: null table");
    if (box_len < 1 || box_len > kClassMapMaxSide || box0 < 0 || box0 > kClassMapMaxSide - box_len)
        return set_error(GL_ERR_UNSUPPORTED, "class map index table: a box of %d samples from %d on is outside the limit of 1 .. %d samples inside 0 .. %d", box_len,
                         box0, kClassMapMaxSide, kClassMapMaxSide);
    if (out < 1 || out > kClassMapMaxSide) return set_error(GL_ERR_UNSUPPORTED, "class map index table: a resized side of %d is outside the limit of 1 .. %d", out, kClassMapMaxSide);
    nearest_axis(box0, box_len, out, idx);
    return GL_OK;
}

// ---------------------------------------------------------------- kernels
namespace {

constexpr int kNoKey = 1 << 30;   // a tap in the padding or without a class: sorted behind every (class, tap) and skipped

// Odd-even transposition sort of N keys in registers: every index is a constant once unrolled.
template <int N>
__device__ __forceinline__ void sort_keys(int (&k)[N]) {
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int i = r & 1; i + 1 < N; i += 2) {
            const int lo = min(k[i], k[i + 1]), hi = max(k[i], k[i + 1]);
            k[i] = lo;
            k[i + 1] = hi;
        }
    }
}

// resize_f32_kernel's nearest source index of resized coordinate o, as it stands there; -1 in the conv's zero padding
__device__ __forceinline__ int nearest_src(int o, int R, float scale, int n) {
    if (o < 0 || o >= R) return -1;
    return min((int)floorf(o * scale), n - 1);
}

// One thread makes 4 neighbouring output bytes of one row (one word where the rows allow it); blockIdx.y is the map.
__global__ __launch_bounds__(256) void class_map_resize_kernel(const ClassMapJob* __restrict__ jobs, const int* __restrict__ tab, uint8_t* __restrict__ out,
                                                               int out_w, int out_h) {
    const ClassMapJob j = jobs[blockIdx.y];
    const int* __restrict__ tx = tab + j.tx;
    const int* __restrict__ ty = tab + j.ty;
    uint8_t* __restrict__ o = out + (size_t)blockIdx.y * out_h * out_w;
    const int nq = (out_w + 3) >> 2;
    const int total = out_h * nq;   // <= 16384 * 4096
    const bool words = (out_w & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < total; i += (int)gridDim.x * 256) {
        const int y = i / nq, x0 = 4 * (i - y * nq);
        const uint8_t* __restrict__ row = j.src + (size_t)ty[y] * j.src_stride;
        uint8_t* orow = o + (size_t)y * out_w + x0;
        if (words) {
            const int4 t = *reinterpret_cast<const int4*>(tx + x0);
            *reinterpret_cast<uint32_t*>(orow) = (uint32_t)row[t.x] | (uint32_t)row[t.y] << 8 | (uint32_t)row[t.z] << 16 | (uint32_t)row[t.w] << 24;
        } else {
            for (int e = 0; e < 4 && x0 + e < out_w; ++e) orow[e] = row[tx[x0 + e]];
        }
    }
}

// One thread per output pixel, all 3 channels; the weights lie in LDS as [class][tap][3].
__global__ __launch_bounds__(256) void class_inconv_kernel(const uint8_t* __restrict__ cls, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ y, int B, int H, int W, int n_classes, int R) {
    extern __shared__ float wl[];
    const int per = n_classes * 9;
    for (int i = threadIdx.x; i < 3 * per; i += 256) {
        const int o = i / per;
        wl[(i - o * per) * 3 + o] = w[i];
    }
    __syncthreads();
    const float sy = (float)H / (float)R, sx = (float)W / (float)R;
    const float b0 = bias[0], b1 = bias[1], b2 = bias[2];
    const int64_t total = (int64_t)B * R * R;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % R);
        const int oy = (int)((i / R) % R);
        const int b = (int)(i / ((int64_t)R * R));
        const uint8_t* __restrict__ src = cls + (size_t)b * H * W;
        int ix[3], iy[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            ix[t] = nearest_src(ox + t - 1, R, sx, W);
            iy[t] = nearest_src(oy + t - 1, R, sy, H);
        }
        int key[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                int k = kNoKey;
                if (iy[ky] >= 0 && ix[kx] >= 0) {
                    const int c = src[(size_t)iy[ky] * W + ix[kx]];
                    if (c < n_classes) k = c * 9 + ky * 3 + kx;
                }
                key[ky * 3 + kx] = k;
            }
        }
        sort_keys<9>(key);
        float a0 = b0, a1 = b1, a2 = b2;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (key[t] != kNoKey) {
                const float* p = wl + key[t] * 3;
                a0 += p[0];
                a1 += p[1];
                a2 += p[2];
            }
        }
        float* yo = y + (size_t)b * 3 * R * R + (size_t)oy * R + ox;
        yo[0] = a0;
        yo[(size_t)R * R] = a1;
        yo[(size_t)2 * R * R] = a2;
    }
}

__global__ void class_conv_weight_relayout_kernel(const float* __restrict__ w, float* __restrict__ g, int c_out, int per) {
    const int total = c_out * per;
    for (int i = (int)blockIdx.x * blockDim.x + (int)threadIdx.x; i < total; i += (int)gridDim.x * blockDim.x) {
        const int o = i / per;
        g[(size_t)(i - o * per) * c_out + o] = w[i];
    }
}

// One thread per (output pixel, 4 output channels): the 16 taps' classes are read and sorted once, each adds one float4 of
// g [class][tap][c_out]. Pixels run along the lanes, so the 4 stores of a wave are contiguous rows of 4 planes.
__global__ __launch_bounds__(256) void class_conv4x4s2_kernel(const uint8_t* __restrict__ cls, const float* __restrict__ g, const float* __restrict__ bias,
                                                              float* __restrict__ y, int B, int H, int W, int n_classes, int c_out, int R, int silu) {
    const int Ro = R / 2, G = c_out / 4;
    const float sy = (float)H / (float)R, sx = (float)W / (float)R;
    const int64_t total = (int64_t)B * G * Ro * Ro;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % Ro);
        const int oy = (int)((i / Ro) % Ro);
        const int q = (int)((i / ((int64_t)Ro * Ro)) % G);
        const int b = (int)(i / ((int64_t)Ro * Ro * G));
        const uint8_t* __restrict__ src = cls + (size_t)b * H * W;
        int ix[4], iy[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            ix[t] = nearest_src(2 * ox - 1 + t, R, sx, W);
            iy[t] = nearest_src(2 * oy - 1 + t, R, sy, H);
        }
        int key[16];
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                int k = kNoKey;
                if (iy[ky] >= 0 && ix[kx] >= 0) {
                    const int c = src[(size_t)iy[ky] * W + ix[kx]];
                    if (c < n_classes) k = c * 16 + ky * 4 + kx;
                }
                key[ky * 4 + kx] = k;
            }
        }
        sort_keys<16>(key);
        float a0 = bias[4 * q], a1 = bias[4 * q + 1], a2 = bias[4 * q + 2], a3 = bias[4 * q + 3];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            if (key[t] != kNoKey) {
                const float4 p = *reinterpret_cast<const float4*>(g + (size_t)key[t] * c_out + 4 * q);
                a0 += p.x;
                a1 += p.y;
                a2 += p.z;
                a3 += p.w;
            }
        }
        if (silu) {   // conv4x4s2_f32_kernel's expression
            a0 = a0 / (1.f + __expf(-a0));
            a1 = a1 / (1.f + __expf(-a1));
            a2 = a2 / (1.f + __expf(-a2));
            a3 = a3 / (1.f + __expf(-a3));
        }
        const size_t plane = (size_t)Ro * Ro;
        float* yo = y + ((size_t)b * c_out + 4 * q) * plane + (size_t)oy * Ro + ox;
        yo[0] = a0;
        yo[plane] = a1;
        yo[2 * plane] = a2;
        yo[3 * plane] = a3;
    }
}

// ---- weight gradients of the two convs. dW[o][c][tap] is dy binned by the class under each tap, so nothing is multiplied by a zero
// plane: a workgroup stages one 16 x 16 tile of output pixels -- its dy values and the u16 class patch under it, 0xffff in the padding --
// and thread (tap, class lane) holds NB classes x CO channels of bins in registers. It walks the tile's pixels in ascending order, reads
// the class under its tap and adds dy to the bin of that class. A workgroup takes `tpb` consecutive tiles and writes one partial
// [bins][c_out] | bias [c_out]; class_conv_wgrad_reduce_kernel adds the partials in ascending order. No atomics: the same bits every run.
constexpr int kWgTile = 16;

template <int K, int S, int CO, int NB>
__global__ __launch_bounds__(256) void class_conv_wgrad_kernel(const uint8_t* __restrict__ cls, const float* __restrict__ dy, ClassDyStrides ds,
                                                               float* __restrict__ part, int H, int W, int n_classes, int c_out, int R, int Ro, int tiles_side,
                                                               int n_tiles, int tpb) {
    constexpr int T = K * K, CL = 256 / T, TS = kWgTile, PS = S * (TS - 1) + K;
    __shared__ uint16_t patch[PS * PS];
    __shared__ float dyl[TS * TS * CO];
    const int tid = threadIdx.x;
    const int tap = tid % T, cl = tid / T, ky = tap / K, kx = tap - ky * K;
    const int c0 = (int)blockIdx.y * (CL * NB) + cl;      // this thread's classes: c0 + j CL
    const int o0 = (int)blockIdx.z * CO;
    const float sy = (float)H / (float)R, sx = (float)W / (float)R;
    float acc[NB][CO], bacc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) {
        bacc[o] = 0.f;
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j][o] = 0.f;
    }
    const int t_end = min(n_tiles, ((int)blockIdx.x + 1) * tpb);
    for (int tile = (int)blockIdx.x * tpb; tile < t_end; ++tile) {
        const int b = tile / (tiles_side * tiles_side), tr = tile - b * tiles_side * tiles_side;
        const int y0 = (tr / tiles_side) * TS, x0 = (tr % tiles_side) * TS;
        const uint8_t* __restrict__ src = cls + (size_t)b * H * W;
        __syncthreads();      // the tile before has been read
        for (int i = tid; i < PS * PS; i += 256) {
            const int pr = i / PS, pc = i - pr * PS;
            const int iy = nearest_src(S * y0 - 1 + pr, R, sy, H), ix = nearest_src(S * x0 - 1 + pc, R, sx, W);
            patch[i] = (iy >= 0 && ix >= 0) ? (uint16_t)src[(size_t)iy * W + ix] : (uint16_t)0xffff;
        }
        for (int i = tid; i < TS * TS * CO; i += 256) {
            const int o = i / (TS * TS), p = i - o * (TS * TS);
            const int oy = y0 + p / TS, ox = x0 + p % TS;
            dyl[p * CO + o] = (oy < Ro && ox < Ro) ? dy[(size_t)b * ds.b + (size_t)(o0 + o) * ds.c + (size_t)oy * ds.y + (size_t)ox * ds.x] : 0.f;
        }
        __syncthreads();
        const int nh = min(TS, Ro - y0), nw = min(TS, Ro - x0);
        for (int py = 0; py < nh; ++py) {
            const uint16_t* __restrict__ prow = patch + (S * py + ky) * PS + kx;
            const float* __restrict__ drow = dyl + py * TS * CO;
            for (int px = 0; px < nw; ++px) {
                const int dc = (int)prow[S * px] - c0;
                float d[CO];
#pragma unroll
                for (int o = 0; o < CO; ++o) {
                    d[o] = drow[px * CO + o];
                    bacc[o] += d[o];
                }
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const float m = dc == j * CL ? 1.f : 0.f;      // 1 * d + acc is acc + d exactly
#pragma unroll
                    for (int o = 0; o < CO; ++o) acc[j][o] = fmaf(m, d[o], acc[j][o]);
                }
            }
        }
    }
    float* __restrict__ po = part + (size_t)blockIdx.x * ((size_t)n_classes * T + 1) * c_out;
    if (cl < CL) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int c = c0 + j * CL;
            if (c < n_classes) {
#pragma unroll
                for (int o = 0; o < CO; ++o) po[((size_t)c * T + tap) * c_out + o0 + o] = acc[j][o];
            }
        }
    }
    if (tid == 0 && blockIdx.y == 0) {
#pragma unroll
        for (int o = 0; o < CO; ++o) po[(size_t)n_classes * T * c_out + o0 + o] = bacc[o];
    }
}

// part [n_part][E + 1][c_out] (E = n_classes * taps; row E: the bias) -> dW [c_out][E] (OIHW), db [c_out]: partials added in ascending order
__global__ __launch_bounds__(256) void class_conv_wgrad_reduce_kernel(const float* __restrict__ part, int n_part, int E, int c_out, float* __restrict__ dW,
                                                                      float* __restrict__ db) {
    const int total = (E + 1) * c_out;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= total) return;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < n_part; ++k) s += part[(size_t)k * total + i];
    const int e = i / c_out, o = i - e * c_out;
    if (e < E) {
        if (dW) dW[(size_t)o * E + e] = s;
    } else if (db) {
        db[o] = s;
    }
}

inline int grid_for(int64_t n, int cap) {
    int64_t g = cdiv64(n, 256);
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

int check_map(const char* what, const void* cls, int B, int H, int W, int n_classes, int R) {
    if (!cls || B < 1) return set_error(GL_ERR_ARG, "%s: null class map, or no sample", what);
    if (H < 1 || W < 1 || H > kClassMapMaxSide || W > kClassMapMaxSide)
        return set_error(GL_ERR_UNSUPPORTED, "%s: the class map is %d x %d; a side is limited to 1 .. %d", what, W, H, kClassMapMaxSide);
    if (n_classes < 1 || n_classes > kClassMaxClasses)
        return set_error(GL_ERR_UNSUPPORTED, "%s: %d classes; a u8 class map holds 1 .. %d", what, n_classes, kClassMaxClasses);
    if (R < 2 || R > kClassMapMaxSide) return set_error(GL_ERR_UNSUPPORTED, "%s: a resized side of %d is outside the limit of 2 .. %d", what, R, kClassMapMaxSide);
    return GL_OK;
}

}  // namespace

// ---------------------------------------------------------------- host
int class_map_resize_plan(const gl_class_map_desc* maps, int S, int out_w, int out_h, const uint8_t* out, ClassMapPlan* plan) {
    if (!maps || !out || !plan || S < 1) return set_error(GL_ERR_ARG, "class map resize: null maps / out, or no map");
    if (S > kClassMapMaxMaps) return set_error(GL_ERR_UNSUPPORTED, "class map resize: %d maps; one call takes at most %d", S, kClassMapMaxMaps);
    if (out_w < 1 || out_h < 1 || out_w > kClassMapMaxSide || out_h > kClassMapMaxSide)
        return set_error(GL_ERR_UNSUPPORTED, "class map resize: resized to %d x %d; a resized side is limited to 1 .. %d", out_w, out_h, kClassMapMaxSide);
    for (int i = 0; i < S; ++i) {
        const gl_class_map_desc& d = maps[i];
        if (!d.pixels) return set_error(GL_ERR_ARG, "class map resize: map %d has no pixels", i);
        if (d.width < 1 || d.height < 1 || d.width > kClassMapMaxSide || d.height > kClassMapMaxSide)
            return set_error(GL_ERR_UNSUPPORTED, "class map resize: map %d is %d x %d; a source side is limited to 1 .. %d", i, d.width, d.height, kClassMapMaxSide);
        if (d.row_stride < d.width) return set_error(GL_ERR_ARG, "class map resize: map %d has a row stride of %d bytes, less than its width %d", i, d.row_stride, d.width);
        if (d.box_x < 0 || d.box_y < 0 || d.box_w < 1 || d.box_h < 1 || d.box_x > d.width - d.box_w || d.box_y > d.height - d.box_h)
            return set_error(GL_ERR_ARG, "class map resize: map %d: the box (%d, %d, %d x %d) does not lie inside the %d x %d map", i, d.box_x, d.box_y, d.box_w,
                             d.box_h, d.width, d.height);
    }
    const int wp = round_up(out_w, 4);   // a column table starts on 16 bytes: one thread reads 4 entries at once
    plan->tab_off = up256((size_t)S * sizeof(ClassMapJob));
    plan->block.assign(plan->tab_off + (size_t)S * (wp + round_up(out_h, 4)) * sizeof(int), 0);
    ClassMapJob* jobs = reinterpret_cast<ClassMapJob*>(plan->block.data());
    int* tab = reinterpret_cast<int*>(plan->block.data() + plan->tab_off);
    int off = 0;
    for (int i = 0; i < S; ++i) {
        const gl_class_map_desc& d = maps[i];
        jobs[i].src = d.pixels, jobs[i].src_stride = d.row_stride;
        jobs[i].tx = off;
        GL_TRY(class_map_index_table(d.box_x, d.box_w, out_w, tab + off));
        off += wp;
        jobs[i].ty = off;
        GL_TRY(class_map_index_table(d.box_y, d.box_h, out_h, tab + off));
        off += round_up(out_h, 4);
    }
    plan->S = S, plan->out_w = out_w, plan->out_h = out_h;
    return GL_OK;
}

int class_map_resize_run(ImageStage& stage, ClassMapPlan& plan, void* work, uint8_t* out, hipStream_t stream) {
    if (!work || (reinterpret_cast<uintptr_t>(work) & 255)) return set_error(GL_ERR_ARG, "class map resize: the workspace must be 256-byte aligned");
    GL_TRY(image_stage_upload(stage, plan.block.data(), plan.block.size(), work, stream));
    const ClassMapJob* djobs = static_cast<const ClassMapJob*>(work);
    const int* dtab = reinterpret_cast<const int*>(static_cast<const char*>(work) + plan.tab_off);
    const int gx = grid_for((int64_t)plan.out_h * cdiv(plan.out_w, 4), 1024);
    hipLaunchKernelGGL(class_map_resize_kernel, dim3(gx, plan.S), dim3(256), 0, stream, djobs, dtab, out, plan.out_w, plan.out_h);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int class_inconv_launch(const uint8_t* cls, const float* w, const float* bias, float* y, int B, int H, int W, int n_classes, int R, hipStream_t stream) {
    GL_TRY(check_map("class in_conv", cls, B, H, W, n_classes, R));
    if (!w || !bias || !y) return set_error(GL_ERR_ARG, "class in_conv: null weights / output");
    const size_t lds = (size_t)n_classes * 27 * sizeof(float);   // <= 27 KB
    // few, long-lived workgroups: each stages the whole weight once
    hipLaunchKernelGGL(class_inconv_kernel, dim3(grid_for((int64_t)B * R * R, 1024)), dim3(256), lds, stream, cls, w, bias, y, B, H, W, n_classes, R);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int class_conv_weight_relayout_launch(const float* w, float* g, int c_out, int n_classes, hipStream_t stream) {
    if (!w || !g || c_out < 1 || n_classes < 1 || n_classes > kClassMaxClasses) return set_error(GL_ERR_ARG, "class conv weight relayout: bad arguments");
    hipLaunchKernelGGL(class_conv_weight_relayout_kernel, dim3(grid_for((int64_t)c_out * n_classes * 16, 1024)), dim3(256), 0, stream, w, g, c_out, n_classes * 16);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int class_conv4x4s2_launch(const uint8_t* cls, const float* g, const float* bias, float* y, int B, int H, int W, int n_classes, int c_out, int R, int silu,
                           hipStream_t stream) {
    GL_TRY(check_map("class conv4x4s2", cls, B, H, W, n_classes, R));
    if (!g || !bias || !y) return set_error(GL_ERR_ARG, "class conv4x4s2: null weights / output");
    if (R & 1) return set_error(GL_ERR_ARG, "class conv4x4s2: odd input size %d", R);
    if (c_out < 4 || c_out % 4) return set_error(GL_ERR_UNSUPPORTED, "class conv4x4s2: %d output channels; a thread makes 4, so a multiple of 4 is needed", c_out);
    if (reinterpret_cast<uintptr_t>(g) & 15) return set_error(GL_ERR_ARG, "class conv4x4s2: the gather weights must be 16-byte aligned");
    hipLaunchKernelGGL(class_conv4x4s2_kernel, dim3(grid_for((int64_t)B * (c_out / 4) * (R / 2) * (R / 2), 8192)), dim3(256), 0, stream, cls, g, bias, y, B, H, W,
                       n_classes, c_out, R, silu);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

namespace {

struct WgradPlan { int Ro, tiles_side, n_tiles, tpb, n_part, T; };

int class_conv_wgrad_plan(int kind, const void* cls, int B, int H, int W, int n_classes, int c_out, int R, WgradPlan* p) {
    const char* what = kind == kClassWgradDown ? "class conv4x4s2 wgrad" : "class in_conv wgrad";
    if (kind != kClassWgradInConv && kind != kClassWgradDown) return set_error(GL_ERR_ARG, "class conv wgrad: kind %d; 0 (in_conv) or 1 (down) is built", kind);
    GL_TRY(check_map(what, cls, B, H, W, n_classes, R));
    if (kind == kClassWgradInConv && c_out != 3) return set_error(GL_ERR_UNSUPPORTED, "%s: %d output channels; in_conv has exactly 3", what, c_out);
    if (kind == kClassWgradDown && (c_out < 4 || c_out % 4 || c_out > kClassWgradMaxOut))
        return set_error(GL_ERR_UNSUPPORTED, "%s: %d output channels; a thread holds 4, so a multiple of 4 up to %d is needed", what, c_out, kClassWgradMaxOut);
    if (kind == kClassWgradDown && (R & 1)) return set_error(GL_ERR_ARG, "%s: odd input size %d", what, R);
    p->Ro = kind == kClassWgradDown ? R / 2 : R;
    p->T = kind == kClassWgradDown ? 16 : 9;
    p->tiles_side = cdiv(p->Ro, kWgTile);
    const int64_t n_tiles = (int64_t)B * p->tiles_side * p->tiles_side;
    if (n_tiles > (1 << 30)) return set_error(GL_ERR_UNSUPPORTED, "%s: %lld tiles of %d x %d output pixels; at most 2^30 are indexed", what, (long long)n_tiles, kWgTile, kWgTile);
    p->n_tiles = (int)n_tiles;
    p->tpb = cdiv(p->n_tiles, 512);      // a function of the shape alone: the summation order is fixed
    p->n_part = cdiv(p->n_tiles, p->tpb);
    return GL_OK;
}

}  // namespace

int class_conv_wgrad_partial_floats(int kind, int B, int H, int W, int n_classes, int c_out, int R, size_t* n) {
    WgradPlan p;
    if (!n) return set_error(GL_ERR_ARG, "class conv wgrad: null size");
    GL_TRY(class_conv_wgrad_plan(kind, n, B, H, W, n_classes, c_out, R, &p));
    *n = (size_t)p.n_part * ((size_t)n_classes * p.T + 1) * c_out;
    return GL_OK;
}

int class_conv_wgrad_launch(int kind, const uint8_t* cls, const float* dy, ClassDyStrides ds, float* part, float* dW, float* db, int B, int H, int W, int n_classes,
                            int c_out, int R, hipStream_t stream) {
    WgradPlan p;
    GL_TRY(class_conv_wgrad_plan(kind, cls, B, H, W, n_classes, c_out, R, &p));
    if (!dy || !part || (!dW && !db)) return set_error(GL_ERR_ARG, "class conv wgrad: null dy / partials, or neither gradient asked for");
    if (kind == kClassWgradInConv) {      // 28 class lanes x 6 classes per workgroup, the 3 output channels
        hipLaunchKernelGGL((class_conv_wgrad_kernel<3, 1, 3, 6>), dim3(p.n_part, cdiv(n_classes, 28 * 6), 1), dim3(256), 0, stream, cls, dy, ds, part, H, W, n_classes, c_out, R, p.Ro,
                           p.tiles_side, p.n_tiles, p.tpb);
    } else {                              // 16 class lanes x 6 classes per workgroup, 4 output channels
        hipLaunchKernelGGL((class_conv_wgrad_kernel<4, 2, 4, 6>), dim3(p.n_part, cdiv(n_classes, 16 * 6), c_out / 4), dim3(256), 0, stream, cls, dy, ds, part, H, W,
                           n_classes, c_out, R, p.Ro, p.tiles_side, p.n_tiles, p.tpb);
    }
    GL_LAUNCH_CHECK();
    const int E = n_classes * p.T;
    hipLaunchKernelGGL(class_conv_wgrad_reduce_kernel, dim3(cdiv((E + 1) * c_out, 256)), dim3(256), 0, stream, (const float*)part, p.n_part, E, c_out, dW, db);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
