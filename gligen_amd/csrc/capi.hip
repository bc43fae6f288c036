// extern "C" surface of libgligen_amd.so (see include/gligen_amd.h). Nothing throws across it.
#include "classmap.h"
#include "engine_impl.h"
#include "image.h"
#include "latent.h"
#include "lora.h"
#include "tile.h"
#include "train.h"
#include "train_fusers.h"
#include "../../include/gligen_amd_train_maps.h"
#include "../../include/gligen_amd_train_inputs.h"
#include "../../include/gligen_amd_train_fusers.h"
#include "../../include/gligen_amd_train_prims.h"
#include "../../include/gligen_amd_train_lora.h"
#include "../../include/gligen_amd_train_lora_conv.h"
#include "../../include/gligen_amd_trainer.h"
#include "../../include/gligen_amd_train_run.h"
#include "train_run.h"
#include "../../include/gligen_amd_sampler.h"
#include "../../include/gligen_amd_gemm_plans.h"
#include "../../include/gligen_amd_attention_core.h"
#include "../../include/gligen_amd_conv8.h"
#include "../../include/gligen_amd_ffn_rows.h"
#include "../../include/gligen_amd_norm.h"
#include "../../include/gligen_amd_vae.h"
#include "../../include/gligen_amd_latent.h"
#include "../../include/gligen_amd_lora.h"
#include "../../include/gligen_amd_tiling.h"
#include "gemm_plan.h"

#include <cstdlib>

#include <cmath>

using namespace gl;

struct gl_ctx {
    std::shared_ptr<Engine> holder;   // forks (gl_ctx_fork) keep the context whose weights they share alive
    Engine* eng;
    ImageStage image_stage;           // the pinned staging block of gl_op_image_resample and gl_op_class_map_resize
};

#define GL_API_BEGIN try {
#define GL_API_END                                       \
    }                                                    \
    catch (const gl::GlError& e) {                       \
        return gl::set_error(e.code, "%s", e.what());    \
    }                                                    \
    catch (const std::exception& e) {                    \
        return gl::set_error(GL_ERR_STATE, "%s", e.what()); \
    }                                                    \
    return GL_OK;

// every entry point runs on the context's own device, whatever the caller's current device is, and hands the caller's
// current device back on return (a process may hold engines on several GPUs next to torch's own notion of "current")
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
        else prev = -1;   // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
#define NEED(ctx)                                                         \
    if (!(ctx) || !(ctx)->eng) return gl::set_error(GL_ERR_ARG, "null context"); \
    DeviceGuard device_guard_((ctx)->eng->device());                      \
    if (!device_guard_.ok) return gl::set_error(GL_ERR_HIP, "hipSetDevice(%d) failed", (ctx)->eng->device());

static inline hipStream_t S(gl_stream s) { return reinterpret_cast<hipStream_t>(s); }
#define HIPCK_API(expr)                                                                           \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) throw GlError(GL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

extern "C" {

const char* gl_last_error(void) { return gl::last_error(); }

int gl_ctx_create(int device, size_t arena_bytes, gl_ctx** out) {
    if (!out) return gl::set_error(GL_ERR_ARG, "null out pointer");
    GL_API_BEGIN
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        throw GlError(GL_ERR_HIP, "no HIP device available: libgligen_amd has no CPU path");
    if (device < 0 || device >= ndev) throw GlError(GL_ERR_ARG, "device index out of range");
    if (hipSetDevice(device) != hipSuccess) throw GlError(GL_ERR_HIP, "hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) throw GlError(GL_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        throw GlError(GL_ERR_UNSUPPORTED, std::string("libgligen_amd is built for gfx950 (MI355X); device is ") + prop.gcnArchName);
    std::shared_ptr<Engine> eng(new Engine(device));
    eng->arena().init(arena_bytes ? arena_bytes : (size_t(8) << 30));
    eng->init_workspace();
    *out = new gl_ctx{eng, eng.get(), {}};
    GL_API_END
}

int gl_ctx_fork(gl_ctx* parent, size_t arena_bytes, gl_ctx** out) {
    NEED(parent);
    if (!out) return gl::set_error(GL_ERR_ARG, "null out pointer");
    GL_API_BEGIN
    std::shared_ptr<Engine> e = Engine::fork(parent->holder, arena_bytes);
    *out = new gl_ctx{e, e.get(), {}};
    GL_API_END
}

int gl_ctx_memory(gl_ctx* ctx, size_t* own_bytes, size_t* arena_bytes, int* is_fork) {
    NEED(ctx);
    GL_API_BEGIN
    if (own_bytes) *own_bytes = ctx->eng->weight_bytes();
    if (arena_bytes) *arena_bytes = ctx->eng->arena_bytes();
    if (is_fork) *is_fork = ctx->eng->is_fork() ? 1 : 0;
    GL_API_END
}

int gl_ctx_destroy(gl_ctx* ctx) {
    if (!ctx) return GL_OK;
    GL_API_BEGIN
    (void)hipDeviceSynchronize();
    delete ctx;      // the engine goes with its last holder: a parent outlives its forks
    GL_API_END
}

int gl_unet_configure(gl_ctx* ctx, const gl_unet_config* cfg) {
    NEED(ctx);
    if (!cfg) return gl::set_error(GL_ERR_ARG, "null config");
    GL_API_BEGIN
    ctx->eng->configure_unet(*cfg);
    GL_API_END
}

int gl_vae_configure(gl_ctx* ctx, const gl_vae_config* cfg) {
    NEED(ctx);
    if (!cfg) return gl::set_error(GL_ERR_ARG, "null config");
    GL_API_BEGIN
    ctx->eng->configure_vae(*cfg);
    GL_API_END
}

int gl_weight_upload(gl_ctx* ctx, const char* key, const void* data, int ndim, const int64_t* shape, int is_device) {
    NEED(ctx);
    if (!key || !data || ndim < 0 || (ndim > 0 && !shape)) return gl::set_error(GL_ERR_ARG, "bad weight upload arguments");
    GL_API_BEGIN
    ctx->eng->upload(key, data, ndim, shape, is_device != 0);
    GL_API_END
}

int gl_finalize(gl_ctx* ctx) {
    NEED(ctx);
    GL_API_BEGIN
    ctx->eng->finalize();
    GL_API_END
}

int gl_clip_text_configure(gl_ctx* ctx, const gl_clip_text_config* cfg) {
    NEED(ctx);
    if (!cfg) return gl::set_error(GL_ERR_ARG, "null config");
    GL_API_BEGIN
    ctx->eng->configure_clip_text(*cfg);
    GL_API_END
}

int gl_clip_text_encode(gl_ctx* ctx, const int32_t* ids, const int32_t* eos_index, int n_seq, int n_tok, float* last_hidden, float* pooled, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    ctx->eng->clip_text_encode(ids, eos_index, n_seq, n_tok, last_hidden, pooled, S(s));
    GL_API_END
}

int gl_clip_vision_configure(gl_ctx* ctx, const gl_clip_vision_config* cfg) {
    NEED(ctx);
    if (!cfg) return gl::set_error(GL_ERR_ARG, "null config");
    GL_API_BEGIN
    ctx->eng->configure_clip_vision(*cfg);
    GL_API_END
}

int gl_clip_vision_encode(gl_ctx* ctx, const float* pixel_values, int n_img, float* last_hidden, float* pooled, float* image_embeds, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    ctx->eng->clip_vision_encode(pixel_values, n_img, last_hidden, pooled, image_embeds, S(s));
    GL_API_END
}

int gl_op_clip_attention(gl_ctx* ctx, const void* qkv, void* out, int n_seq, int n_tok, int heads, int causal, gl_stream s) {
    NEED(ctx);
    if (!qkv || !out) return gl::set_error(GL_ERR_ARG, "null qkv/out");
    GL_API_BEGIN
    int r = clip_attn_launch((const bf16*)qkv, (bf16*)out, n_seq, n_tok, heads, causal, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

int gl_op_image_resample(gl_ctx* ctx, const gl_image_desc* images, int n_img, int filter, int out_kind, const float* lut_host, void* out, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    ImagePlan plan;
    GL_TRY(image_resample_plan(images, n_img, filter, out_kind, lut_host, out, &plan));
    gl::Arena& ar = ctx->eng->arena();
    const size_t mk = ar.mark();
    struct Release {
        gl::Arena& ar;
        size_t mk;
        ~Release() { ar.release(mk); }   // stream-ordered reuse, as every operator's workspace
    } release{ar, mk};
    void* work = ar.alloc(plan.work_bytes);
    GL_TRY(image_resample_run(ctx->image_stage, plan, work, S(s)));
    ctx->eng->n_launches += 2;
    GL_API_END
}

int gl_image_resample_coeffs(int in_size, int out_size, int filter, int* ksize, int* bounds, int bounds_cap, int* coeffs, int coeffs_cap) {
    if (!ksize) return gl::set_error(GL_ERR_ARG, "gl_image_resample_coeffs: null ksize");
    GL_API_BEGIN
    std::shared_ptr<const ResampleAxis> t;
    GL_TRY(resample_axis(in_size, out_size, filter, &t));
    *ksize = t->ksize;
    if (bounds) {
        if (bounds_cap < (int)t->bounds.size())
            return gl::set_error(GL_ERR_ARG, "gl_image_resample_coeffs: bounds holds %d ints, 2 * out_size = %d are needed", bounds_cap, (int)t->bounds.size());
        std::copy(t->bounds.begin(), t->bounds.end(), bounds);
    }
    if (coeffs) {
        if ((int64_t)coeffs_cap < (int64_t)t->kk.size())
            return gl::set_error(GL_ERR_ARG, "gl_image_resample_coeffs: coeffs holds %d ints, out_size * ksize = %zu are needed", coeffs_cap, t->kk.size());
        std::copy(t->kk.begin(), t->kk.end(), coeffs);
    }
    GL_API_END
}

int gl_unet_set_cond(gl_ctx* ctx, int Beff, const float* context, int n_ctx_tokens, const gl_grounding* g, gl_stream s) {
    NEED(ctx);
    if (!context || !g) return gl::set_error(GL_ERR_ARG, "null context/grounding");
    GL_API_BEGIN
    ctx->eng->set_cond(Beff, context, n_ctx_tokens, *g, S(s));
    GL_API_END
}

int gl_unet_set_fuser_scales(gl_ctx* ctx, const float* scales_host, int n, gl_stream s) {
    NEED(ctx);
    if (!scales_host) return gl::set_error(GL_ERR_ARG, "null scales");
    GL_API_BEGIN
    ctx->eng->set_fuser_scales(scales_host, n, S(s));
    GL_API_END
}

int gl_unet_grounding_tokens(gl_ctx* ctx, float* out, gl_stream s) {
    NEED(ctx);
    if (!out) return gl::set_error(GL_ERR_ARG, "null out pointer");
    GL_API_BEGIN
    ctx->eng->grounding_tokens(out, S(s));
    GL_API_END
}

int gl_op_spatial_tokens(gl_ctx* ctx, const float* image, int B, int C, int H, int W, const float* mask, float* tokens, gl_stream s) {
    NEED(ctx);
    if (!image || !mask || !tokens) return gl::set_error(GL_ERR_ARG, "null pointer");
    GL_API_BEGIN
    ctx->eng->spatial_tokens(B, image, C, H, W, mask, tokens, S(s));
    GL_API_END
}

int gl_op_grounding_downsample(gl_ctx* ctx, const float* img, int B, int Cimg, int H, int W, int n_in, int R, int mode,
                               const float* w1, const float* b1, int c_mid, const float* w2, const float* b2, int c_out,
                               float* out, gl_stream s) {
    NEED(ctx);
    if (!img || !out || B <= 0 || n_in <= 0 || n_in > Cimg || R <= 0) return gl::set_error(GL_ERR_ARG, "grounding_downsample: bad arguments");
    if (w1 && (!b1 || !w2 || !b2 || c_mid <= 0 || c_out <= 0 || R % 4)) return gl::set_error(GL_ERR_ARG, "grounding_downsample: bad conv arguments");
    GL_API_BEGIN
    if (!w1) {
        GL_TRY(gl::resize_f32_launch(img, out, B, Cimg, n_in, H, W, R, mode, S(s)));
    } else {
        gl::Arena& ar = ctx->eng->arena();
        const size_t mk = ar.mark();
        float* r = ar.get<float>((size_t)B * n_in * R * R);
        float* h1 = ar.get<float>((size_t)B * c_mid * (R / 2) * (R / 2));
        int rc = gl::resize_f32_launch(img, r, B, Cimg, n_in, H, W, R, mode, S(s));
        if (rc == GL_OK) rc = gl::conv4x4s2_f32_launch(r, w1, b1, h1, B, n_in, c_mid, R, R, 1, S(s));
        if (rc == GL_OK) rc = gl::conv4x4s2_f32_launch(h1, w2, b2, out, B, c_mid, c_out, R / 2, R / 2, 0, S(s));
        ar.release(mk);
        if (rc != GL_OK) return rc;
    }
    GL_API_END
}

// ---- include/gligen_amd_maps.h: semantic maps as class indices
int gl_op_class_map_resize(gl_ctx* ctx, const gl_class_map_desc* maps_host, int n_maps, int out_w, int out_h, uint8_t* out, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    ClassMapPlan plan;
    GL_TRY(class_map_resize_plan(maps_host, n_maps, out_w, out_h, out, &plan));
    gl::Arena& ar = ctx->eng->arena();
    const size_t mk = ar.mark();
    struct Release {
        gl::Arena& ar;
        size_t mk;
        ~Release() { ar.release(mk); }   // stream-ordered reuse, as every operator's workspace
    } release{ar, mk};
    void* work = ar.alloc(plan.block.size());
    GL_TRY(class_map_resize_run(ctx->image_stage, plan, work, out, S(s)));
    ++ctx->eng->n_launches;
    GL_API_END
}

int gl_class_map_index_table(int box0, int box_len, int out_size, int* idx_host, int cap) {
    if (!idx_host) return gl::set_error(GL_ERR_ARG, "gl_class_map_index_table: null table");
    if (out_size >= 1 && cap < out_size) return gl::set_error(GL_ERR_ARG, "gl_class_map_index_table: the table holds %d ints, out_size = %d are needed", cap, out_size);
    GL_API_BEGIN
    GL_TRY(class_map_index_table(box0, box_len, out_size, idx_host));
    GL_API_END
}

int gl_op_spatial_tokens_classes(gl_ctx* ctx, const uint8_t* cls, int B, int H, int W, const float* mask, float* tokens, gl_stream s) {
    NEED(ctx);
    if (!cls || !mask || !tokens) return gl::set_error(GL_ERR_ARG, "spatial_tokens_classes: null class map / mask / tokens");
    GL_API_BEGIN
    ctx->eng->spatial_tokens_classes(B, cls, H, W, mask, tokens, S(s));
    GL_API_END
}

int gl_op_grounding_downsample_classes(gl_ctx* ctx, const uint8_t* cls, int B, int H, int W, int n_classes, int R,
                                       const float* w1, const float* b1, int c_mid, const float* w2, const float* b2, int c_out,
                                       float* out, gl_stream s) {
    NEED(ctx);
    if (!cls || !out || !w1 || !b1 || !w2 || !b2) return gl::set_error(GL_ERR_ARG, "grounding_downsample_classes: null class map / weights / out");
    if (R <= 0 || R % 4) return gl::set_error(GL_ERR_ARG, "grounding_downsample_classes: resize_input %d; two stride-2 convs need a positive multiple of 4", R);
    if (c_out <= 0) return gl::set_error(GL_ERR_ARG, "grounding_downsample_classes: %d output channels", c_out);
    GL_API_BEGIN
    gl::Arena& ar = ctx->eng->arena();
    const size_t mk = ar.mark();
    int rc = GL_OK;
    if (n_classes < 1 || n_classes > kClassMaxClasses || c_mid < 4 || c_mid % 4 || B < 1)
        rc = gl::set_error(GL_ERR_UNSUPPORTED, "grounding_downsample_classes: %d samples, %d classes, %d middle channels; at least one sample, 1 .. %d classes and a multiple of 4 middle channels are needed",
                           B, n_classes, c_mid, kClassMaxClasses);
    if (rc == GL_OK) {
        float* g = ar.get<float>((size_t)n_classes * 16 * c_mid);
        float* h1 = ar.get<float>((size_t)B * c_mid * (R / 2) * (R / 2));
        rc = class_conv_weight_relayout_launch(w1, g, c_mid, n_classes, S(s));
        if (rc == GL_OK) rc = class_conv4x4s2_launch(cls, g, b1, h1, B, H, W, n_classes, c_mid, R, 1, S(s));
        if (rc == GL_OK) rc = gl::conv4x4s2_f32_launch(h1, w2, b2, out, B, c_mid, c_out, R / 2, R / 2, 0, S(s));
        if (rc == GL_OK) ctx->eng->n_launches += 3;
    }
    ar.release(mk);
    if (rc != GL_OK) return rc;
    GL_API_END
}

int gl_unet_set_fuser_scale(gl_ctx* ctx, float scale, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    ctx->eng->set_fuser_scale(scale, S(s));
    GL_API_END
}

int gl_unet_restore_first_conv(gl_ctx* ctx, const float* w, const float* b, gl_stream s) {
    NEED(ctx);
    if (!w || !b) return gl::set_error(GL_ERR_ARG, "null weights");
    GL_API_BEGIN
    ctx->eng->restore_first_conv(w, b, S(s));
    GL_API_END
}

int gl_unet_forward(gl_ctx* ctx, int Beff, int h, int w, const float* x, int xB, const int64_t* timesteps,
                    const float* inpaint_extra, int extraB, float* eps_out, gl_stream s) {
    NEED(ctx);
    if (!x || !timesteps || !eps_out || Beff <= 0 || h <= 0 || w <= 0) return gl::set_error(GL_ERR_ARG, "bad unet_forward arguments");
    GL_API_BEGIN
    ctx->eng->unet_forward(Beff, h, w, x, xB, timesteps, inpaint_extra, extraB, eps_out, S(s));
    GL_API_END
}

int gl_vae_decode(gl_ctx* ctx, int B, int h, int w, const float* z, float* img, gl_stream s) {
    NEED(ctx);
    if (!z || !img || B <= 0 || h <= 0 || w <= 0) return gl::set_error(GL_ERR_ARG, "bad vae_decode arguments");
    GL_API_BEGIN
    ctx->eng->vae_decode(B, h, w, z, img, S(s));
    GL_API_END
}

int gl_sample_plms(gl_ctx* ctx, const gl_plms_args* args, gl_stream s) {
    NEED(ctx);
    if (!args) return gl::set_error(GL_ERR_ARG, "null args");
    if (args->struct_size != sizeof(gl_plms_args))
        return gl::set_error(GL_ERR_ARG, "gl_sample_plms: args->struct_size is %u, this library's gl_plms_args has %zu bytes (set it to sizeof(gl_plms_args))",
                             args->struct_size, sizeof(gl_plms_args));
    GL_API_BEGIN
    ctx->eng->sample_plms(*args, S(s));
    GL_API_END
}

int gl_sample_solver(gl_ctx* ctx, const gl_solver_args* args, gl_stream s) {
    // the layout first: a caller built against another header is told so whatever else is wrong with the call
    if (!args) return gl::set_error(GL_ERR_ARG, "null args");
    if (args->struct_size != sizeof(gl_solver_args))
        return gl::set_error(GL_ERR_ARG, "gl_sample_solver: args->struct_size is %u, this library's gl_solver_args has %zu bytes (set it to sizeof(gl_solver_args))",
                             args->struct_size, sizeof(gl_solver_args));
    NEED(ctx);
    GL_API_BEGIN
    ctx->eng->sample_solver(*args, S(s));
    GL_API_END
}

int gl_op_solver_update(gl_ctx* ctx, const float* eps_pair, int has_uncond, float guidance, float a_t, const float* x, float* x_out,
                        float* d0_out, const float* d1, const float* d2, const float* z, float cx, float c0, float c1, float c2, float cn,
                        int64_t n, gl_stream s) {
    NEED(ctx);
    gl::SolverParams P{};
    P.eps_pair = eps_pair; P.has_uncond = has_uncond ? 1 : 0; P.guidance = guidance;
    P.d0_out = d0_out; P.d1 = d1; P.d2 = d2; P.z = z;
    P.cx = cx; P.c0 = c0; P.c1 = c1; P.c2 = c2; P.cn = cn;
    P.x = x; P.x_out = x_out; P.a_t = a_t; P.n = n;
    return gl::solver_update_launch(P, S(s));
}

int gl_sampler_timing(gl_ctx* ctx, float* avg_unet_eval_ms, float* first_eval_ms, int* n_evals) {
    NEED(ctx);
    if (!avg_unet_eval_ms || !first_eval_ms || !n_evals) return gl::set_error(GL_ERR_ARG, "null pointer");
    GL_API_BEGIN
    ctx->eng->sampler_timing(avg_unet_eval_ms, first_eval_ms, n_evals);
    GL_API_END
}

int gl_vae_encode(gl_ctx* ctx, int B, int H, int W, const float* img, const float* noise, float* z, gl_stream s) {
    NEED(ctx);
    if (!img || !noise || !z) return gl::set_error(GL_ERR_ARG, "null pointer");
    GL_API_BEGIN
    ctx->eng->vae_encode(B, H, W, img, noise, z, S(s));
    GL_API_END
}

int gl_unet_profile(gl_ctx* ctx, int Beff, int h, int w, const float* x, int xB, const int64_t* timesteps,
                    const float* inpaint_extra, int extraB, float* eps_out, gl_prof_rec* recs, int max_recs, int* n_recs,
                    gl_stream s) {
    NEED(ctx);
    if (!x || !timesteps || !eps_out || !recs || !n_recs || max_recs <= 0) return gl::set_error(GL_ERR_ARG, "null pointer");
    GL_API_BEGIN
    ctx->eng->profile_begin();
    std::vector<Engine::ProfRec> out;
    try {
        ctx->eng->unet_forward(Beff, h, w, x, xB, timesteps, inpaint_extra, extraB, eps_out, S(s));
    } catch (...) {
        (void)ctx->eng->profile_end(S(s));
        throw;
    }
    out = ctx->eng->profile_end(S(s));
    int n = 0;
    for (const auto& r : out) {
        if (n >= max_recs) break;
        gl_prof_rec& d = recs[n++];
        snprintf(d.name, sizeof d.name, "%s", r.name.c_str());
        d.calls = r.calls; d.ms = r.ms; d.flops = r.flops; d.bytes = r.bytes;
    }
    *n_recs = n;
    GL_API_END
}

int gl_to_uint8(const float* img, uint8_t* out, int B, int C, int HW, gl_stream s) {
    if (!img || !out) return gl::set_error(GL_ERR_ARG, "null pointer");
    // no context: the launch has to go to the device that holds the image, whatever the caller's current device is
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, img) != hipSuccess) {
        (void)hipGetLastError();
        return gl::set_error(GL_ERR_ARG, "gl_to_uint8: img is not a device pointer");
    }
    DeviceGuard guard(at.device);
    if (!guard.ok) return gl::set_error(GL_ERR_HIP, "hipSetDevice(%d) failed", at.device);
    return to_uint8_launch(img, out, B, C, HW, S(s));
}

int gl_arena_high_water(gl_ctx* ctx, size_t* bytes) {
    NEED(ctx);
    *bytes = ctx->eng->arena().high_water();
    return GL_OK;
}

int gl_launch_count(gl_ctx* ctx, int64_t* n) {
    NEED(ctx);
    *n = ctx->eng->n_launches;
    return GL_OK;
}

int gl_set_ff_rows_policy(int mode) { return gl::ff_rows_policy_set(mode); }

int gl_ff_rows_policy_report(char* buf, size_t cap) { return gl::ff_rows_policy_report(buf, cap); }

// ---- include/gligen_amd_sampler.h
int gl_set_cfg_shared_prefix(int on) { return gl::cfg_shared_prefix_set(on); }

// ---- include/gligen_amd_vae.h
int gl_vae_set_attention(gl_ctx* ctx, int mode) {
    NEED(ctx);
    GL_API_BEGIN
    ctx->eng->set_vae_attention(mode);
    GL_API_END
}

int gl_op_vae_attention(gl_ctx* ctx, const void* q, const void* k, const void* v, int B, int T, int C, int mode, void* out, gl_stream s) {
    NEED(ctx);
    if (!q || !k || !v || !out) return gl::set_error(GL_ERR_ARG, "gl_op_vae_attention: null pointer");
    GL_API_BEGIN
    if (((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out)) & 15) != 0)
        throw GlError(GL_ERR_ARG, "gl_op_vae_attention: q, k, v and out are 16-byte aligned");
    ctx->eng->op_vae_attention((const bf16*)q, (const bf16*)k, (const bf16*)v, B, T, C, mode, (bf16*)out, S(s));
    GL_API_END
}

// ---- include/gligen_amd_tiling.h
int gl_vae_decode_tiled(gl_ctx* ctx, int B, int h, int w, const float* z, float* img, const gl_tile_plan* plan, int tiles_per_pass, gl_stream s) {
    NEED(ctx);
    if (!z || !img || !plan || B <= 0 || h <= 0 || w <= 0) return gl::set_error(GL_ERR_ARG, "bad vae_decode_tiled arguments");
    GL_API_BEGIN
    ctx->eng->vae_decode_tiled(B, h, w, z, img, *plan, tiles_per_pass, S(s));
    GL_API_END
}

int gl_vae_encode_tiled(gl_ctx* ctx, int B, int H, int W, const float* img, const float* noise, float* z, float* moments_out,
                        const gl_tile_plan* plan, int tiles_per_pass, gl_stream s) {
    NEED(ctx);
    if (!img || !noise || !z || !plan || B <= 0 || H <= 0 || W <= 0) return gl::set_error(GL_ERR_ARG, "bad vae_encode_tiled arguments");
    GL_API_BEGIN
    ctx->eng->vae_encode_tiled(B, H, W, img, noise, z, moments_out, *plan, tiles_per_pass, S(s));
    GL_API_END
}

int gl_op_tile_gather(gl_ctx* ctx, const float* src, int B, int C, int H, int W, const int* windows, int n, float* dst, int TH, int TW, gl_stream s) {
    NEED(ctx);
    return gl::tile_gather_launch(src, B, C, H, W, windows, n, dst, TH, TW, S(s));
}

int gl_op_tile_blend(gl_ctx* ctx, const float* tiles, int first_tile, int n, const gl_tile_plan* plan, float* out, int B, int C, int H, int W,
                     gl_stream s) {
    NEED(ctx);
    if (!plan) return gl::set_error(GL_ERR_ARG, "gl_op_tile_blend: null plan");
    if (plan->struct_size != sizeof(gl_tile_plan))
        return gl::set_error(GL_ERR_ARG, "gl_op_tile_blend: plan->struct_size is %u, this library's gl_tile_plan has %zu bytes", plan->struct_size,
                             sizeof(gl_tile_plan));
    const gl::TileBlendPlan bp{plan->ny, plan->nx, plan->th_out, plan->tw_out, plan->oy, plan->ox, plan->wy, plan->wx};
    return gl::tile_blend_launch(tiles, first_tile, n, bp, out, B, C, H, W, S(s));
}

// ---- include/gligen_amd_gemm_plans.h
int gl_gemm_force_plan(int tm, int tn, int splits, int grid_cap) {
    bool tile = tm == 0 && tn == 0;
    for (int c = 0; c < kGemmTiles; ++c) tile |= kGemmTm[c] == tm && kGemmTn[c] == tn;
    if (!tile || splits < 0 || splits > 32 || grid_cap < 0)
        return gl::set_error(GL_ERR_ARG, "gl_gemm_force_plan: tile %dx%d / %d splits / cap %d (tiles 4x5 4x4 2x5 2x4 2x2 or 0x0, splits 0..32, cap >= 0)", tm, tn, splits, grid_cap);
    gemm_force_cfg(tm, tn, tm ? splits : 0);
    gemm_force_grid(grid_cap);
    return GL_OK;
}
int gl_gemm_force_knobs(int halo_splits, int wide_splits, int wide_xcd, int xcd_boxes, int halo, int wide) {
    if (halo_splits < 0 || wide_splits < 0 || wide_xcd < -1 || wide_xcd > 1 || xcd_boxes < 0 || xcd_boxes > 1 || halo < 0 || wide < 0 || wide > 2)
        return gl::set_error(GL_ERR_ARG, "gl_gemm_force_knobs: halo_splits %d, wide_splits %d, wide_xcd %d, xcd_boxes %d, halo %d, wide %d", halo_splits, wide_splits, wide_xcd, xcd_boxes, halo, wide);
    gemm_force_knobs(halo_splits, wide_splits, wide_xcd, xcd_boxes, halo, wide);
    return GL_OK;
}
int gl_gemm_force_clear(void) { gemm_force_clear(); return GL_OK; }
int gl_gemm_plan_log_clear(void) { gemm_plan_log_clear(); return GL_OK; }
int gl_gemm_plan_log(gl_gemm_plan_record* out, int max, int* n_written, int* n_launches) {
    if (!out || !n_written || !n_launches || max < 0) return gl::set_error(GL_ERR_ARG, "gl_gemm_plan_log: null pointer or negative max");
    GemmLogEntry e[kGemmLogSize];
    const int n = gemm_plan_log(e, std::min(max, (int)kGemmLogSize), n_launches);
    for (int i = 0; i < n; ++i) {
        const GemmPlan& p = e[i].plan;
        gl_gemm_plan_record& r = out[i];
        r = gl_gemm_plan_record{};
        snprintf(r.kernel, sizeof r.kernel, "%s", p.name);
        r.family = p.family; r.M = e[i].M; r.N = e[i].N; r.K = e[i].K;
        r.tm = p.tm; r.tn = p.tn; r.splits = p.splits; r.grid = p.grid;
        if (p.family == GEMM_HALO) { r.n_items = p.halo.n_items; r.units_per_split = p.halo.chunks_per_split; }
        else if (p.family == GEMM_CONV8) { r.n_items = p.conv8.n_items; r.units_per_split = p.conv8.chunks_per_split; }
        else if (p.family == GEMM_WIDE) { r.n_items = p.wide.n_items; r.units_per_split = p.wide.kt_per_split; r.xcd = p.wide.xcd; }
        else {
            r.n_items = p.work.n_items; r.units_per_split = p.work.kt_per_split;
            if (p.family != GEMM_GLDS) { r.box = p.work.box; r.rm = p.work.rm; r.rz = p.work.rz; }
        }
    }
    *n_written = n;
    return GL_OK;
}

int gl_box_calibrate(gl_ctx* ctx, gl_box_calibration* out, gl_stream s) {
    NEED(ctx);
    if (!out) return gl::set_error(GL_ERR_ARG, "gl_box_calibrate: null out pointer");
    GL_API_BEGIN
    Arena& ar = ctx->eng->arena();
    const size_t mk = ar.mark();
    const size_t bytes = size_t(1) << 30;   // 512 MiB -> 512 MiB: twice the Infinity Cache in each direction
    void* scratch = ar.alloc(bytes);
    HIPCK_API(hipMemsetAsync(scratch, 1, bytes, S(s)));
    float v[3] = {0.f, 0.f, 0.f};
    int rc = box_calibrate_launch(scratch, bytes, v, S(s));
    ar.release(mk);
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    out->hbm_copy_gbs = v[0];
    out->lds_dma_tbs = v[1];
    out->mfma_bf16_tflops = v[2];
    GL_API_END
}

int gl_mfma_calibrate(gl_ctx* ctx, int shape, int waves_per_simd, int n_acc, int zero_data, float target_ms, gl_mfma_calibration* out, gl_stream s) {
    NEED(ctx);
    if (!out) return gl::set_error(GL_ERR_ARG, "gl_mfma_calibrate: null out pointer");
    GL_API_BEGIN
    Arena& ar = ctx->eng->arena();
    const size_t mk = ar.mark();
    void* scratch = ar.alloc(4096);
    HIPCK_API(hipMemsetAsync(scratch, 0, 4096, S(s)));
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int rc = mfma_calibrate_launch(shape, waves_per_simd, n_acc, zero_data, target_ms, scratch, v, S(s));
    ar.release(mk);
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    out->tflops = v[0];
    out->sclk_mhz = v[1];
    out->ms = v[2];
    out->cycles_per_mfma = v[3];
    GL_API_END
}

// ------------------------------------------------------------------ single operators
int gl_op_linear(gl_ctx* ctx, const void* x, const void* w, const float* bias, const void* res, void* y,
                 int M, int N, int K, int act, int out_f32, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    Epilogue E = e_rows_res(y, N, bias, (const bf16*)res);
    E.out_f32 = out_f32; E.act = act;
    int r = gemm_launch(a_rows((const bf16*)x, K), (const bf16*)w, M, N, K, E, ctx->eng->splitk_ws(), ctx->eng->splitk_ws_bytes(), S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

int gl_op_geglu(gl_ctx* ctx, const void* x, const float* w_f32, const float* b_f32, void* y, int M, int inner, int K, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    Arena& ar = ctx->eng->arena();
    ar.reset();
    bf16* wp = ar.get<bf16>((size_t)2 * inner * K);
    float* bp = ar.get<float>((size_t)2 * inner);
    const int layout = gl::gemm_geglu_layout();
    int r = pack_geglu_launch(w_f32, b_f32, wp, bp, inner, K, layout, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    Epilogue E = e_rows(y, inner, bp);
    E.act = ACT_GEGLU; E.geglu16 = layout;
    r = gemm_launch(a_rows((const bf16*)x, K), wp, M, 2 * inner, K, E, ctx->eng->splitk_ws(), ctx->eng->splitk_ws_bytes(), S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

int gl_op_ln_linear(gl_ctx* ctx, const void* a, int M, int K0, const float* w0, const float* b0, const void* res, int C,
                    const float* gamma, const float* beta, const float* w1, const float* b1, int mode, int inner_or_heads, int T,
                    void* x_out, void* y_out, int* used_fold, gl_stream s) {
    NEED(ctx);
    if (!a || !w0 || !gamma || !beta || !w1 || !x_out || !y_out || !used_fold) return gl::set_error(GL_ERR_ARG, "gl_op_ln_linear: null pointer");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    Arena& ar = eng.arena();
    ar.reset();
    auto ck = [&](int rc) { if (rc != GL_OK) throw GlError(rc, gl::last_error()); };
    if (C % 64 || K0 % 64 || M <= 0) throw GlError(GL_ERR_ARG, "gl_op_ln_linear: C and K0 must be multiples of 64");
    const int N1 = mode == 0 ? 2 * inner_or_heads : C;
    // ---- producer: x = a W0^T + b0 (+ res), with the row statistics of x
    bf16* w0b = ar.get<bf16>((size_t)C * K0);
    ck(cast_f32_bf16_launch(w0, w0b, (int64_t)C * K0, S(s)));
    const int ld = C / 32;
    float2* stats = ar.get<float2>((size_t)M * ld);
    {
        Epilogue E = e_rows_res(x_out, C, b0, (const bf16*)res);
        E.stats_out = stats; E.stats_ld = ld;
        ck(gemm_launch(a_rows((const bf16*)a, K0), w0b, M, C, K0, E, eng.splitk_ws(), eng.splitk_ws_bytes(), S(s)));
    }
    const int nb = gemm_last_stats_nb();
    // ---- the consumer's folded weights: W1 * gamma, b1 + W1 beta, csum of the packed rows
    float* wf = ar.get<float>((size_t)N1 * C);
    float* bf = ar.get<float>((size_t)N1);
    ck(ln_fold_launch(w1, b1, gamma, beta, wf, bf, N1, C, S(s)));
    bf16* wp = ar.get<bf16>((size_t)N1 * C);
    float* bp = ar.get<float>((size_t)N1);
    float* cs = ar.get<float>((size_t)N1);
    AOperand A;
    Epilogue E;
    epilogue_defaults(E);
    if (mode == 0) {
        const int layout = gl::gemm_geglu_layout();
        ck(pack_geglu_launch(wf, bf, wp, bp, inner_or_heads, C, layout, S(s)));
        E.act = ACT_GEGLU; E.geglu16 = layout; E.out = y_out; E.ldo = inner_or_heads; E.bias = bp;
    } else {
        const int H = inner_or_heads, d = C / H;
        int dp, dpv;
        ck(attn_dims(d, &dp, &dpv));
        if (T <= 0 || M % T || T % 64) throw GlError(GL_ERR_ARG, "gl_op_ln_linear: mode 1 needs T (tokens per sample, a multiple of 64) dividing M");
        ck(cast_f32_bf16_launch(wf, wp, (int64_t)N1 * C, S(s)));
        HIPCK_API(hipMemcpyAsync(bp, bf, (size_t)N1 * sizeof(float), hipMemcpyDeviceToDevice, S(s)));
        E.mode = EPI_QK_HEADS; E.q = (bf16*)y_out; E.k = nullptr; E.C = C; E.H = H; E.d = d; E.DP = dp; E.T = T;
        E.Tpad_q = round_up(T, 128); E.bias = bp;
    }
    ck(rowsum_bf16_launch(wp, cs, N1, C, S(s)));
    aoperand_rows(A, (const bf16*)x_out, C, C);
    const bool fold = nb > 0 && gemm_ln_fold_supported(A, M, N1, C, E);
    *used_fold = fold ? 1 : 0;
    if (fold) {
        e_fold_ln(E, RowStats{stats, nb, ld}, cs, C);
    } else {   // the fallback the engine takes where no statistics exist: ln_kernel without affine, same folded weights
        bf16* xn = ar.get<bf16>((size_t)M * C);
        LNParams P{};
        P.x = (const bf16*)x_out; P.B = 1; P.N1 = M; P.N2 = 0; P.Tpad = M; P.C = C; P.eps = 1e-5f; P.y = xn;
        ck(layernorm_launch(P, S(s)));
        aoperand_rows(A, xn, C, C);
    }
    ck(gemm_launch(A, wp, M, N1, C, E, eng.splitk_ws(), eng.splitk_ws_bytes(), S(s)));
    GL_API_END
}

int gl_op_feedforward(gl_ctx* ctx, const void* x, int M, int C, const float* gamma, const float* beta, const float* w1, const float* b1,
                      const float* w2, const float* b2, const void* res, const float* gate, void* y, void* stats, int* used_rows,
                      gl_stream s) {
    NEED(ctx);
    if (!x || !w1 || !b1 || !w2 || !b2 || !y || !used_rows) return gl::set_error(GL_ERR_ARG, "gl_op_feedforward: null pointer");
    if ((gamma == nullptr) != (beta == nullptr)) return gl::set_error(GL_ERR_ARG, "gl_op_feedforward: gamma and beta come together");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    Arena& ar = eng.arena();
    ar.reset();
    auto ck = [&](int rc) { if (rc != GL_OK) throw GlError(rc, gl::last_error()); };
    if (C % 64 || M <= 0) throw GlError(GL_ERR_ARG, "gl_op_feedforward: C must be a multiple of 64");
    const float* w1e = w1;
    const float* b1e = b1;
    if (gamma) {   // LayerNorm folded into the projection: W1 * gamma, b1 + W1 beta
        float* wf = ar.get<float>((size_t)8 * C * C);
        float* bf = ar.get<float>((size_t)8 * C);
        ck(ln_fold_launch(w1, b1, gamma, beta, wf, bf, 8 * C, C, S(s)));
        w1e = wf; b1e = bf;
    }
    const bool rows = ff_rows_supported(M, C) && !(gl::dev_env("GL_FF_ROWS") && atoi(gl::dev_env("GL_FF_ROWS")) == 0);
    *used_rows = rows ? 1 : 0;
    // the per-row (sum, sum of squares) come out of the row-local kernel's epilogue; the two-GEMM form writes per-column-block partials
    // in the consumer's own layout (gemm.h Epilogue::stats_out), not this one: refuse rather than hand back zeros
    if (stats && !rows) throw GlError(GL_ERR_UNSUPPORTED, "gl_op_feedforward: row statistics are produced only by the row-local kernel (C = 320, M % 128 == 0)");
    if (rows) {
        void* st = ar.alloc(ff_stream_bytes(C));
        ck(ff_pack_launch(w1e, b1e, w2, st, C, S(s)));
        FFRowsParams P{};
        P.x = (const bf16*)x; P.ldx = C; P.normalize = gamma ? 1 : 0; P.eps = 1e-5f; P.stream = st; P.b2 = b2;
        P.res = (const bf16*)res; P.ldres = C; P.gate = gate; P.out = (bf16*)y; P.ldo = C; P.M = M;
        P.stats_out = (float2*)stats; P.stats_ld = 1;
        ck(ff_rows_launch(P, C, S(s)));
    } else {
        const bf16* in = (const bf16*)x;
        if (gamma) {
            bf16* xn = ar.get<bf16>((size_t)M * C);
            LNParams L{};
            L.x = in; L.B = 1; L.N1 = M; L.N2 = 0; L.Tpad = M; L.C = C; L.eps = 1e-5f; L.y = xn;
            ck(layernorm_launch(L, S(s)));
            in = xn;
        }
        const int layout = gl::gemm_geglu_layout();
        bf16* wp = ar.get<bf16>((size_t)8 * C * C);
        float* bp = ar.get<float>((size_t)8 * C);
        ck(pack_geglu_launch(w1e, b1e, wp, bp, 4 * C, C, layout, S(s)));
        bf16* w2b = ar.get<bf16>((size_t)C * 4 * C);
        ck(cast_f32_bf16_launch(w2, w2b, (int64_t)C * 4 * C, S(s)));
        bf16* hid = ar.get<bf16>((size_t)M * 4 * C);
        Epilogue E = e_rows(hid, 4 * C, bp);
        E.act = ACT_GEGLU; E.geglu16 = layout;
        ck(gemm_launch(a_rows(in, C), wp, M, 8 * C, C, E, eng.splitk_ws(), eng.splitk_ws_bytes(), S(s)));
        Epilogue E2 = e_rows_res(y, C, b2, (const bf16*)res);
        E2.gate = gate;
        ck(gemm_launch(a_rows(hid, 4 * C), w2b, M, C, 4 * C, E2, eng.splitk_ws(), eng.splitk_ws_bytes(), S(s)));
    }
    GL_API_END
}

int gl_op_ff_chain(gl_ctx* ctx, const void* x, int M, int C, const float* pre_w, const float* pre_b, const void* pre_res, const float* pre_gate,
                   const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2, const float* b2, const float* gate,
                   const float* post_w, const float* post_b, const void* post_res, void* y, gl_stream s) {
    NEED(ctx);
    if (!x || !pre_w || !pre_b || !pre_res || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !y) return gl::set_error(GL_ERR_ARG, "gl_op_ff_chain: null pointer");
    if (post_w && (!post_b || !post_res)) return gl::set_error(GL_ERR_ARG, "gl_op_ff_chain: the trailing projection needs its bias and residual");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    Arena& ar = eng.arena();
    ar.reset();
    auto ck = [&](int rc) { if (rc != GL_OK) throw GlError(rc, gl::last_error()); };
    if (!ff_rows_supported(M, C)) throw GlError(GL_ERR_UNSUPPORTED, "gl_op_ff_chain: no row-local kernel for this shape (C = 320, M % 128 == 0)");
    float* wf = ar.get<float>((size_t)8 * C * C);
    float* bf = ar.get<float>((size_t)8 * C);
    ck(ln_fold_launch(w1, b1, gamma, beta, wf, bf, 8 * C, C, S(s)));
    void* st = ar.alloc(ff_chain_stream_bytes(C, true, post_w != nullptr));
    ck(ff_chain_pack_launch(wf, bf, w2, pre_w, post_w, st, C, S(s)));
    FFRowsParams P{};
    P.x = (const bf16*)x; P.ldx = C; P.normalize = 1; P.eps = 1e-5f; P.stream = st; P.b2 = b2; P.gate = gate; P.out = (bf16*)y; P.ldo = C; P.M = M;
    P.pre = 1; P.pre_b = pre_b; P.pre_res = (const bf16*)pre_res; P.ld_pre_res = C; P.pre_gate = pre_gate;
    P.mid_out = ar.get<bf16>((size_t)M * C); P.ld_mid = C;
    if (post_w) { P.post = 1; P.post_b = post_b; P.post_res = (const bf16*)post_res; P.ld_post_res = C; }
    ck(ff_rows_launch(P, C, S(s)));
    GL_API_END
}

int gl_op_ff_chain_q(gl_ctx* ctx, const void* x, int B, int N, int C, const float* pre_w, const float* pre_b, const void* pre_res, const float* pre_gate,
                     const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2, const float* b2, const float* gate,
                     const float* gamma_q, const float* beta_q, const float* wq, void* y, void* q, gl_stream s) {
    NEED(ctx);
    if (!x || !pre_w || !pre_b || !pre_res || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !gamma_q || !beta_q || !wq || !y || !q)
        return gl::set_error(GL_ERR_ARG, "gl_op_ff_chain_q: null pointer");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    Arena& ar = eng.arena();
    ar.reset();
    auto ck = [&](int rc) { if (rc != GL_OK) throw GlError(rc, gl::last_error()); };
    const int M = B * N;
    if (!ff_rows_supported(M, C) || N % 128) throw GlError(GL_ERR_UNSUPPORTED, "gl_op_ff_chain_q: no row-local kernel for this shape (C = 320, N % 128 == 0)");
    float* wf = ar.get<float>((size_t)8 * C * C);
    float* bf = ar.get<float>((size_t)8 * C);
    ck(ln_fold_launch(w1, b1, gamma, beta, wf, bf, 8 * C, C, S(s)));
    float* wqf = ar.get<float>((size_t)C * C);
    float* bqf = ar.get<float>((size_t)C);
    ck(ln_fold_launch(wq, nullptr, gamma_q, beta_q, wqf, bqf, C, C, S(s)));
    void* st = ar.alloc(ff_chain_stream_bytes(C, true, true));
    ck(ff_chain_pack_launch(wf, bf, w2, pre_w, wqf, st, C, S(s)));
    FFRowsParams P{};
    P.x = (const bf16*)x; P.ldx = C; P.normalize = 1; P.eps = 1e-5f; P.stream = st; P.b2 = b2; P.gate = gate; P.out = (bf16*)y; P.ldo = C; P.M = M;
    P.pre = 1; P.pre_b = pre_b; P.pre_res = (const bf16*)pre_res; P.ld_pre_res = C; P.pre_gate = pre_gate;
    P.mid_out = ar.get<bf16>((size_t)M * C); P.ld_mid = C;
    P.post = 2; P.post_b = bqf; P.q = (bf16*)q; P.qDP = 48; P.qT = N; P.qTpad = N;
    ck(ff_rows_launch(P, C, S(s)));
    GL_API_END
}

int gl_op_adamw_step(gl_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                     double weight_decay, int step, gl_stream s) {
    NEED(ctx);
    if (!p || !g || !m || !v || n < 0) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_step: null pointer");
    return gl::adamw_step(p, g, m, v, (size_t)n, lr, beta1, beta2, eps, weight_decay, step, S(s));
}

int gl_op_adamw_ema_step(gl_ctx* ctx, float* p, const float* g, float* m, float* v, float* ema, int64_t n, double lr, double beta1, double beta2,
                         double eps, double weight_decay, double ema_rate, int step, gl_stream s) {
    NEED(ctx);
    if (!p || !g || !m || !v || !ema) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_ema_step: null pointer");
    if (n < 0) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_ema_step: n = %lld is negative", (long long)n);
    if (step < 1) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_ema_step: step = %d, steps count from 1", step);
    if (!(ema_rate >= 0.0 && ema_rate <= 1.0)) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_ema_step: ema_rate %g is outside [0, 1]", ema_rate);
    return gl::adamw_ema_step(p, g, m, v, ema, (size_t)n, lr, beta1, beta2, eps, weight_decay, ema_rate, step, S(s));
}

// ---- include/gligen_amd_train_run.h: accumulation, norm, clipping coefficient, clipped update, loss weights (train_run.hip)
static_assert(GL_GRAD_NORM_CHUNK == gl::kGradNormChunk && GL_GRAD_NORM_CHAIN == gl::kGradNormChain, "gligen_amd_train_run.h out of step with train_run.h");
static_assert(GL_GRAD_ACCUM_FIRST == gl::GRAD_ACCUM_FIRST && GL_GRAD_ACCUM_MIDDLE == gl::GRAD_ACCUM_MIDDLE && GL_GRAD_ACCUM_LAST == gl::GRAD_ACCUM_LAST,
              "gligen_amd_train_run.h out of step with train_run.h");

int gl_op_grad_accumulate(gl_ctx* ctx, float* acc, float* g, int64_t n, int mode, int k, gl_stream s) {
    NEED(ctx);
    if (!acc || !g) return gl::set_error(GL_ERR_ARG, "gl_op_grad_accumulate: null pointer");
    if (n < 0) return gl::set_error(GL_ERR_ARG, "gl_op_grad_accumulate: n = %lld is negative", (long long)n);
    if (k < 1) return gl::set_error(GL_ERR_ARG, "gl_op_grad_accumulate: k = %d micro-batches, at least 1", k);
    if (mode < GL_GRAD_ACCUM_FIRST || mode > GL_GRAD_ACCUM_LAST) return gl::set_error(GL_ERR_ARG, "gl_op_grad_accumulate: mode %d (0 first, 1 middle, 2 last)", mode);
    return gl::grad_accumulate(acc, g, (size_t)n, mode, k, S(s));
}

int64_t gl_grad_sqnorm_partials(int64_t n) { return n <= 0 ? 0 : (int64_t)gl::grad_sqnorm_partials((size_t)n); }

int gl_op_grad_sqnorm(gl_ctx* ctx, const float* g, int64_t n, float* partials, gl_stream s) {
    NEED(ctx);
    if (!g || !partials) return gl::set_error(GL_ERR_ARG, "gl_op_grad_sqnorm: null pointer");
    if (n < 0) return gl::set_error(GL_ERR_ARG, "gl_op_grad_sqnorm: n = %lld is negative", (long long)n);
    return gl::grad_sqnorm(g, (size_t)n, partials, S(s));
}

int gl_op_clip_coef(gl_ctx* ctx, const float* partials, int64_t count, float max_norm, float* out2, gl_stream s) {
    NEED(ctx);
    if (!out2 || (!partials && count != 0)) return gl::set_error(GL_ERR_ARG, "gl_op_clip_coef: null pointer");
    if (count < 0) return gl::set_error(GL_ERR_ARG, "gl_op_clip_coef: count = %lld is negative", (long long)count);
    if (!(max_norm > 0.f)) return gl::set_error(GL_ERR_ARG, "gl_op_clip_coef: max_norm %g is not > 0", (double)max_norm);
    return gl::clip_coef(partials, (size_t)count, max_norm, out2, S(s));
}

int gl_op_adamw_clip_step(gl_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                          double weight_decay, int step, const float* coef, gl_stream s) {
    NEED(ctx);
    if (!p || !g || !m || !v || !coef) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_clip_step: null pointer");
    if (n < 0) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_clip_step: n = %lld is negative", (long long)n);
    if (step < 1) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_clip_step: step = %d, steps count from 1", step);
    return gl::adamw_clip_step(p, g, m, v, nullptr, coef, (size_t)n, lr, beta1, beta2, eps, weight_decay, 0.0, step, S(s));
}

int gl_op_adamw_ema_clip_step(gl_ctx* ctx, float* p, const float* g, float* m, float* v, float* ema, int64_t n, double lr, double beta1, double beta2,
                              double eps, double weight_decay, double ema_rate, int step, const float* coef, gl_stream s) {
    NEED(ctx);
    if (!p || !g || !m || !v || !ema || !coef) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_ema_clip_step: null pointer");
    if (n < 0) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_ema_clip_step: n = %lld is negative", (long long)n);
    if (step < 1) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_ema_clip_step: step = %d, steps count from 1", step);
    if (!(ema_rate >= 0.0 && ema_rate <= 1.0)) return gl::set_error(GL_ERR_ARG, "gl_op_adamw_ema_clip_step: ema_rate %g is outside [0, 1]", ema_rate);
    return gl::adamw_clip_step(p, g, m, v, ema, coef, (size_t)n, lr, beta1, beta2, eps, weight_decay, ema_rate, step, S(s));
}

int gl_train_set_loss_weights(gl_ctx* ctx, const float* w, int B) {
    NEED(ctx);
    if (B < 0 || (!w && B != 0) || (w && B == 0)) return gl::set_error(GL_ERR_ARG, "gl_train_set_loss_weights: w [B] with B >= 1, or NULL and 0 to clear");
    ctx->eng->loss_weights = w;
    ctx->eng->loss_weights_B = B;
    return GL_OK;
}

static const char* const k_train_block_names[GL_TRAIN_BLOCK_PARAMS] = {
    "norm1.weight", "norm1.bias", "attn1.to_q.weight", "attn1.to_k.weight", "attn1.to_v.weight", "attn1.to_out.0.weight", "attn1.to_out.0.bias",
    "fuser.linear.weight", "fuser.linear.bias", "fuser.norm1.weight", "fuser.norm1.bias", "fuser.attn.to_q.weight", "fuser.attn.to_k.weight",
    "fuser.attn.to_v.weight", "fuser.attn.to_out.0.weight", "fuser.attn.to_out.0.bias", "fuser.norm2.weight", "fuser.norm2.bias",
    "fuser.ff.net.0.proj.weight", "fuser.ff.net.0.proj.bias", "fuser.ff.net.2.weight", "fuser.ff.net.2.bias", "fuser.alpha_attn", "fuser.alpha_dense",
    "norm2.weight", "norm2.bias", "attn2.to_q.weight", "attn2.to_k.weight", "attn2.to_v.weight", "attn2.to_out.0.weight", "attn2.to_out.0.bias",
    "norm3.weight", "norm3.bias", "ff.net.0.proj.weight", "ff.net.0.proj.bias", "ff.net.2.weight", "ff.net.2.bias"};
static_assert(GL_TRAIN_BLOCK_PARAMS == gl::TP_COUNT, "parameter table out of step with train.h");

const char* const* gl_train_block_param_names(void) { return k_train_block_names; }

int gl_op_block_train(gl_ctx* ctx, const gl_train_block_dims* dims, const float* const* params, const float* x, const float* objs,
                      const float* context, const float* target, float* y, float* loss, float* dx, float* dobjs, float* const* grads,
                      gl_stream s) {
    NEED(ctx);
    if (!dims || !params || !x || !objs || !context || !target || !y || !loss || !dx || !dobjs || !grads)
        return gl::set_error(GL_ERR_ARG, "gl_op_block_train: null pointer");
    for (int i = 0; i < GL_TRAIN_BLOCK_PARAMS; ++i)
        if (grads[i] && !(i >= gl::TP_F_LIN_W && i <= gl::TP_F_ALPHA_DENSE))
            return gl::set_error(GL_ERR_ARG, "gl_op_block_train: a gradient was asked for '%s', which the reference keeps frozen", k_train_block_names[i]);
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    gl::TrainBlockDims d{dims->B, dims->N, dims->Ng, dims->C, dims->heads, dims->ctx_T, dims->ctx_dim, dims->fuser_scale};
    int rc = gl::block_train_step(eng.arena(), eng.splitk_ws(), eng.splitk_ws_bytes(), d, params, x, objs, context, target, y, loss, dx, dobjs, grads, S(s));
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    GL_API_END
}

// ---- include/gligen_amd_train_fusers.h: the block slice by fuser kind, and the grid resize the gatedSA2 fuser is built on
int gl_op_block_train_fuser(gl_ctx* ctx, int fuser_kind, const gl_train_block_dims* dims, const float* const* params, const float* x, const float* objs,
                            const float* context, const float* target, float* y, float* loss, float* dx, float* dobjs, float* const* grads, gl_stream s) {
    NEED(ctx);
    if (!dims || !params || !x || !objs || !context || !target || !y || !loss || !dx || !dobjs || !grads)
        return gl::set_error(GL_ERR_ARG, "gl_op_block_train_fuser: null pointer");
    if (fuser_kind < 0 || fuser_kind > 2) return gl::set_error(GL_ERR_ARG, "gl_op_block_train_fuser: fuser_kind %d (0 gatedSA, 1 gatedSA2, 2 gatedCA)", fuser_kind);
    for (int i = 0; i < GL_TRAIN_BLOCK_PARAMS; ++i) {
        if (fuser_kind == 2 && (i == gl::TP_F_LIN_W || i == gl::TP_F_LIN_B) && (params[i] || grads[i]))
            return gl::set_error(GL_ERR_ARG, "gl_op_block_train_fuser: a gatedCA fuser has no '%s' (the slot is NULL in params and grads)", k_train_block_names[i]);
        if (grads[i] && !(i >= gl::TP_F_LIN_W && i <= gl::TP_F_ALPHA_DENSE))
            return gl::set_error(GL_ERR_ARG, "gl_op_block_train_fuser: a gradient was asked for '%s', which the reference keeps frozen", k_train_block_names[i]);
    }
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    gl::TrainBlockDims d{dims->B, dims->N, dims->Ng, dims->C, dims->heads, dims->ctx_T, dims->ctx_dim, dims->fuser_scale, fuser_kind};
    int rc = gl::block_train_step(eng.arena(), eng.splitk_ws(), eng.splitk_ws_bytes(), d, params, x, objs, context, target, y, loss, dx, dobjs, grads, S(s));
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    GL_API_END
}

int gl_op_grid_resize(gl_ctx* ctx, const float* src, int B, int sg, int sv, int C, float* dst, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    GL_TRY(gl::grid_resize_fwd_launch(src, B, sg, sv, C, dst, S(s)));
    ++ctx->eng->n_launches;
    GL_API_END
}

int gl_op_grid_resize_backward(gl_ctx* ctx, const float* g, int B, int sg, int sv, int C, float* dsrc, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    GL_TRY(gl::grid_resize_bwd_launch(g, B, sg, sv, C, dsrc, S(s)));
    ++ctx->eng->n_launches;
    GL_API_END
}

// ---- include/gligen_amd_latent.h: resize + q_sample in one launch, and the host table of its taps
int gl_op_latent_renoise(gl_ctx* ctx, const float* src, int B, int C, int h, int w, float* dst, int h2, int w2, int mode, float sa, float s1,
                         const float* noise, int noise_B, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    GL_TRY(gl::latent_renoise_launch(src, B, C, h, w, dst, h2, w2, mode, sa, s1, noise, noise_B, S(s)));
    ++ctx->eng->n_launches;
    GL_API_END
}

int gl_latent_resize_taps(int in_size, int out_size, int mode, int* first_index, float* weights) {
    int n_taps = 0;
    if (gl::latent_resize_taps(in_size, out_size, mode, first_index, weights, &n_taps) != GL_OK) return -1;
    return n_taps;
}

// ---- include/gligen_amd_lora.h: a LoRA adapter merged into fp32 parameters in place
int gl_op_lora_merge(gl_ctx* ctx, float* W, const float* up, const float* down, int N, int K, int r, float scale, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    int launched = 0;
    GL_TRY(gl::lora_merge_launch(W, up, down, N, K, r, scale, S(s), &launched));
    ctx->eng->n_launches += launched;
    GL_API_END
}

// ---- include/gligen_amd_train_prims.h: the training path's primitives one by one, over the arena and workspace the slices above use
#define TRAIN_PRIM(call)                                                        \
    GL_API_BEGIN                                                                \
    Engine& eng = *ctx->eng;                                                    \
    eng.arena().reset();                                                        \
    Arena& ar = eng.arena();                                                    \
    float* ws = eng.splitk_ws();                                                \
    const size_t ws_bytes = eng.splitk_ws_bytes();                              \
    const int rc = (call);                                                      \
    if (rc != GL_OK) throw GlError(rc, gl::last_error());                       \
    GL_API_END

int gl_op_train_attention(gl_ctx* ctx, int B, int H, int D, int Nq, int Nk, const float* q, const float* k, const float* v, const float* dout, float* o,
                          float* lse, float* dq, float* dk, float* dv, gl_stream s) {
    NEED(ctx);
    if (!q || !k || !v || !o || !lse) return gl::set_error(GL_ERR_ARG, "gl_op_train_attention: null pointer (q, k, v, o and lse are required)");
    if (!dk != !dv) return gl::set_error(GL_ERR_ARG, "gl_op_train_attention: dk and dv come together (both NULL: the dq-only call)");
    if (!dout && (dq || dk)) return gl::set_error(GL_ERR_ARG, "gl_op_train_attention: a gradient was asked for without dout");
    TRAIN_PRIM(gl::train_prim_attention(ar, ws, ws_bytes, B, H, D, Nq, Nk, q, k, v, dout, o, lse, dq, dk, dv, S(s)))
}

int gl_op_train_linear(gl_ctx* ctx, int M, int N, int K, const float* x, const float* W, const float* b, const float* dy, float* y, float* dx, float* dW,
                       float* db, gl_stream s) {
    NEED(ctx);
    if (!x || !W) return gl::set_error(GL_ERR_ARG, "gl_op_train_linear: null pointer (x and W are required)");
    if (!dy && (dx || dW || db)) return gl::set_error(GL_ERR_ARG, "gl_op_train_linear: a gradient was asked for without dy");
    TRAIN_PRIM(gl::train_prim_linear(ar, ws, ws_bytes, M, N, K, x, W, b, dy, y, dx, dW, db, S(s)))
}

int gl_op_train_layernorm(gl_ctx* ctx, int R, int C, float eps, const float* x, const float* g, const float* b, const float* dy, int accumulate, float* y,
                          float* xhat, float* rstd, float* dx, float* dgamma, float* dbeta, gl_stream s) {
    NEED(ctx);
    if (!x || !g || !b) return gl::set_error(GL_ERR_ARG, "gl_op_train_layernorm: null pointer (x, g and b are required)");
    if (!dy && (dx || dgamma || dbeta)) return gl::set_error(GL_ERR_ARG, "gl_op_train_layernorm: a gradient was asked for without dy");
    TRAIN_PRIM(gl::train_prim_layernorm(ar, ws, ws_bytes, R, C, eps, x, g, b, dy, accumulate, y, xhat, rstd, dx, dgamma, dbeta, S(s)))
}

int gl_op_train_groupnorm(gl_ctx* ctx, int B, int HW, int C, int silu, float eps, const float* x, const float* g, const float* b, const float* da,
                          int accumulate, float* a, float* xhat, float* rstd, float* dx, gl_stream s) {
    NEED(ctx);
    if (!x || !g || !b) return gl::set_error(GL_ERR_ARG, "gl_op_train_groupnorm: null pointer (x, g and b are required)");
    if (!da && dx) return gl::set_error(GL_ERR_ARG, "gl_op_train_groupnorm: dx was asked for without da");
    TRAIN_PRIM(gl::train_prim_groupnorm(ar, ws, ws_bytes, B, HW, C, silu, eps, x, g, b, da, accumulate, a, xhat, rstd, dx, S(s)))
}

int gl_op_train_geglu(gl_ctx* ctx, int R, int I, const float* u, const float* dh, float* h, float* du, gl_stream s) {
    NEED(ctx);
    if (!u) return gl::set_error(GL_ERR_ARG, "gl_op_train_geglu: null pointer (u is required)");
    if (!dh && du) return gl::set_error(GL_ERR_ARG, "gl_op_train_geglu: du was asked for without dh");
    TRAIN_PRIM(gl::train_prim_geglu(ar, ws, ws_bytes, R, I, u, dh, h, du, S(s)))
}

int gl_op_train_dot(gl_ctx* ctx, int64_t n, const float* a, const float* b, const float* alpha, float scale, int mode, float* out, gl_stream s) {
    NEED(ctx);
    if (!a || !b || !out || (mode == 0 && !alpha)) return gl::set_error(GL_ERR_ARG, "gl_op_train_dot: null pointer (a, b and out are required; alpha in mode 0)");
    if (n < 1 || mode < 0 || mode > 1) return gl::set_error(GL_ERR_ARG, "gl_op_train_dot: n = %lld, mode = %d (0 gate gradient, 1 mean squared difference)", (long long)n, mode);
    TRAIN_PRIM(gl::train_prim_dot(ar, ws, ws_bytes, (size_t)n, a, b, alpha, scale, mode, out, S(s)))
}

int gl_op_train_conv3(gl_ctx* ctx, int B, int H, int W, int Cin, int Cout, int geom, const float* x, const float* w_oihw, const float* bias, const float* dy,
                      float* y, float* dx, gl_stream s) {
    NEED(ctx);
    if (!x || !w_oihw || !y) return gl::set_error(GL_ERR_ARG, "gl_op_train_conv3: null pointer (x, w_oihw and y are required)");
    if (!dy && dx) return gl::set_error(GL_ERR_ARG, "gl_op_train_conv3: dx was asked for without dy");
    TRAIN_PRIM(gl::train_prim_conv3(ar, ws, ws_bytes, B, H, W, Cin, Cout, geom, x, w_oihw, bias, dy, y, dx, S(s)))
}

int gl_op_train_conv_direct(gl_ctx* ctx, int B, int H, int W, int Cin, int Cout, int c0, int n, const float* x, const float* w_oihw, const float* bias,
                            const float* dy, float* y, float* dx, float* dW, gl_stream s) {
    NEED(ctx);
    if (!x || !w_oihw || !y) return gl::set_error(GL_ERR_ARG, "gl_op_train_conv_direct: null pointer (x, w_oihw and y are required)");
    if (!dy && (dx || dW)) return gl::set_error(GL_ERR_ARG, "gl_op_train_conv_direct: a gradient was asked for without dy");
    TRAIN_PRIM(gl::train_prim_conv_direct(ar, ws, ws_bytes, B, H, W, Cin, Cout, c0, n, x, w_oihw, bias, dy, y, dx, dW, S(s)))
}
#undef TRAIN_PRIM

static_assert(GL_TRAIN_ST_PARAMS == gl::ST_COUNT, "parameter table out of step with train.h");
const char* const* gl_train_st_param_names(void) {
    static std::string store[GL_TRAIN_ST_PARAMS];
    static const char* names[GL_TRAIN_ST_PARAMS];
    static const bool once = [] {
        store[gl::ST_NORM_W] = "norm.weight"; store[gl::ST_NORM_B] = "norm.bias";
        store[gl::ST_PIN_W] = "proj_in.weight"; store[gl::ST_PIN_B] = "proj_in.bias";
        for (int i = 0; i < GL_TRAIN_BLOCK_PARAMS; ++i) store[gl::ST_BLOCK0 + i] = std::string("transformer_blocks.0.") + k_train_block_names[i];
        store[gl::ST_POUT_W] = "proj_out.weight"; store[gl::ST_POUT_B] = "proj_out.bias";
        for (int i = 0; i < GL_TRAIN_ST_PARAMS; ++i) names[i] = store[i].c_str();
        return true;
    }();
    (void)once;
    return names;
}

int gl_op_st_train(gl_ctx* ctx, const gl_train_block_dims* dims, const float* const* params, const float* x, const float* objs,
                   const float* context, const float* target, float* y, float* loss, float* dx, float* dobjs, float* const* grads, gl_stream s) {
    NEED(ctx);
    if (!dims || !params || !x || !objs || !context || !target || !y || !loss || !dx || !dobjs || !grads)
        return gl::set_error(GL_ERR_ARG, "gl_op_st_train: null pointer");
    for (int i = 0; i < GL_TRAIN_ST_PARAMS; ++i) {
        const int bi = i - gl::ST_BLOCK0;
        if (grads[i] && !(bi >= gl::TP_F_LIN_W && bi <= gl::TP_F_ALPHA_DENSE))
            return gl::set_error(GL_ERR_ARG, "gl_op_st_train: a gradient was asked for '%s', which the reference keeps frozen", gl_train_st_param_names()[i]);
    }
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    gl::TrainBlockDims d{dims->B, dims->N, dims->Ng, dims->C, dims->heads, dims->ctx_T, dims->ctx_dim, dims->fuser_scale};
    int rc = gl::st_train_step(eng.arena(), eng.splitk_ws(), eng.splitk_ws_bytes(), d, params, x, objs, context, target, y, loss, dx, dobjs, grads, S(s));
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    GL_API_END
}

static const char* const k_train_resblock_names[GL_TRAIN_RESBLOCK_PARAMS] = {
    "in_layers.0.weight", "in_layers.0.bias", "in_layers.2.weight", "in_layers.2.bias", "emb_layers.1.weight", "emb_layers.1.bias",
    "out_layers.0.weight", "out_layers.0.bias", "out_layers.3.weight", "out_layers.3.bias", "skip_connection.weight", "skip_connection.bias"};
static_assert(GL_TRAIN_RESBLOCK_PARAMS == gl::RP_COUNT, "parameter table out of step with train.h");

const char* const* gl_train_resblock_param_names(void) { return k_train_resblock_names; }

int gl_op_resblock_train(gl_ctx* ctx, const gl_train_resblock_dims* dims, const float* const* params, const float* x, const float* emb,
                         const float* target, float* y, float* loss, float* dx, gl_stream s) {
    NEED(ctx);
    if (!dims || !params || !x || !emb || !target || !y || !loss || !dx) return gl::set_error(GL_ERR_ARG, "gl_op_resblock_train: null pointer");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    gl::TrainResDims d{dims->B, dims->H, dims->W, dims->Cin, dims->Cout, dims->emb_dim};
    int rc = gl::resblock_train_step(eng.arena(), eng.splitk_ws(), eng.splitk_ws_bytes(), d, params, x, emb, target, y, loss, dx, S(s));
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    GL_API_END
}

int gl_op_resample_train(gl_ctx* ctx, int mode, int B, int H, int W, int C, const float* w_oihw, const float* bias, const float* x,
                         const float* target, float* y, float* loss, float* dx, gl_stream s) {
    NEED(ctx);
    if (!w_oihw || !x || !target || !y || !loss || !dx) return gl::set_error(GL_ERR_ARG, "gl_op_resample_train: null pointer");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    int rc = gl::resample_train_step(eng.arena(), eng.splitk_ws(), eng.splitk_ws_bytes(), mode, B, H, W, C, w_oihw, bias, x, target, y, loss, dx, S(s));
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    GL_API_END
}

// gl_train_set_loss_weights (include/gligen_amd_train_run.h): the weights belong to the next training step, which takes them here --
// before it checks anything, so that it clears them whether it succeeds or fails
static const float* take_loss_weights(gl_ctx* ctx, int* B) {
    Engine& eng = *ctx->eng;
    const float* w = eng.loss_weights;
    *B = eng.loss_weights_B;
    eng.loss_weights = nullptr;
    eng.loss_weights_B = 0;
    return w;
}

static void drop_loss_weights(gl_ctx* ctx) {      // (an entry point that fails in front of the shared step)
    int B;
    if (ctx && ctx->eng) take_loss_weights(ctx, &B);
}

// gl_unet_train_step and gl_unet_train_step_lora (include/gligen_amd_train_lora.h): the same iteration, with or without adapters
static int train_step_discrete(gl_ctx* ctx, const gl_unet_config* cfg, const gl_train_unet_in* in, int n_params, const char* const* names,
                               const float* const* params, float* const* grads, const gl::TrainLoraAdapter* adapters, int n_adapters, float* eps_out,
                               float* loss, gl_stream s) {
    NEED(ctx);
    int lw_B = 0;
    const float* lw = take_loss_weights(ctx, &lw_B);
    if (!cfg || !in || !names || !params || !grads || !loss || n_params <= 0) return gl::set_error(GL_ERR_ARG, "gl_unet_train_step: null pointer");
    if (lw && lw_B != in->B) return gl::set_error(GL_ERR_ARG, "gl_unet_train_step: %d loss weights were set, the step's batch is %d", lw_B, in->B);
    if (cfg->grounding_kind < 0 || cfg->grounding_kind > 2 || cfg->fuser_kind < 0 || cfg->fuser_kind > 2 || cfg->extra_channels)
        return gl::set_error(GL_ERR_UNSUPPORTED, "gl_unet_train_step: the training step is built for the text, text+image and keypoint tokenizers with gatedSA, gatedSA2 "
                                                 "or gatedCA fusers (fuser_kind 0 / 1 / 2), with or without inpaint_mode (no downsampler channels: inpaint_mode with "
                                                 "extra_channels is undefined in the reference)");
    if (cfg->grounding_kind == 1 && (!in->text_masks || !in->image_masks || !in->image_embeddings))
        return gl::set_error(GL_ERR_ARG, "gl_unet_train_step: the text+image tokenizer needs text_masks, image_masks and image_embeddings");
    if (!in->x || !in->timesteps || !in->context || !in->boxes || !in->masks || (!in->positive_embeddings && cfg->grounding_kind != 2) || !in->target)
        return gl::set_error(GL_ERR_ARG, "gl_unet_train_step: null input");
    if (cfg->gr_in_dim != cfg->gr_out_dim || cfg->gr_out_dim != cfg->context_dim)
        return gl::set_error(GL_ERR_UNSUPPORTED, "gl_unet_train_step: grounding in / out dim and context_dim are expected to be equal (768 in every shipped config)");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    gl::TrainUNetCfg c{};
    c.in_channels = cfg->in_channels; c.out_channels = cfg->out_channels; c.model_channels = cfg->model_channels; c.num_res_blocks = cfg->num_res_blocks;
    c.num_heads = cfg->num_heads; c.context_dim = cfg->context_dim; c.gr_dim = cfg->gr_in_dim; c.grounding_kind = cfg->grounding_kind; c.fuser_kind = cfg->fuser_kind; c.n_mult = cfg->n_mult; c.n_attn = cfg->n_attn;
    for (int i = 0; i < 8; ++i) { c.channel_mult[i] = cfg->channel_mult[i]; c.attention_resolutions[i] = cfg->attention_resolutions[i]; }
    c.inpaint_mode = cfg->inpaint_mode ? 1 : 0;       // in->x then holds 2 * in_channels + 1 channels per pixel row
    gl::TrainUNetIn u{in->B, in->H, in->W, in->ctx_T, cfg->grounding_kind == 1 ? 2 * in->Ng : in->Ng, in->Ng, in->x, in->timesteps, in->context, in->boxes,
                      in->masks, in->positive_embeddings, in->text_masks, in->image_masks, in->image_embeddings, in->target, in->fuser_scale, in->checkpoint};
    int rc = gl::unet_train_step(eng.arena(), eng.splitk_ws(), eng.splitk_ws_bytes(), c, u, n_params, names, params, grads, k_train_block_names, eps_out, loss, S(s),
                                 eng.train_events(), Engine::kTrainEvents, in->use_weight_cache ? eng.train_cache : nullptr, nullptr, adapters, n_adapters, lw);
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    eng.train_events_recorded = true;
    GL_API_END
}

int gl_unet_train_step(gl_ctx* ctx, const gl_unet_config* cfg, const gl_train_unet_in* in, int n_params, const char* const* names,
                       const float* const* params, float* const* grads, float* eps_out, float* loss, gl_stream s) {
    return train_step_discrete(ctx, cfg, in, n_params, names, params, grads, nullptr, 0, eps_out, loss, s);
}

// ---- include/gligen_amd_train_lora.h: the iteration with adapters, and the low-rank part of one adapted Linear by itself
int gl_unet_train_step_lora(gl_ctx* ctx, const gl_unet_config* cfg, const gl_train_unet_in* in, int n_params, const char* const* names,
                            const float* const* params, float* const* grads, const gl_lora_adapter* adapters, int n_adapters, float* eps_out,
                            float* loss, gl_stream s) {
    if (n_adapters < 0 || (n_adapters > 0 && !adapters)) {
        drop_loss_weights(ctx);
        return gl::set_error(GL_ERR_ARG, "gl_unet_train_step_lora: null adapter array");
    }
    std::vector<gl::TrainLoraAdapter> a((size_t)n_adapters);
    for (int i = 0; i < n_adapters; ++i)
        a[i] = {adapters[i].name, adapters[i].down, adapters[i].up, adapters[i].g_down, adapters[i].g_up, adapters[i].rank, adapters[i].scale};
    return train_step_discrete(ctx, cfg, in, n_params, names, params, grads, a.data(), n_adapters, eps_out, loss, s);
}

int gl_op_lora_linear(gl_ctx* ctx, int M, int K, int N, int rank, float scale, int down_kr, int up_rn, const float* x, const float* down,
                      const float* up, const float* dy, float* t, float* y, float* u, float* dx, float* g_down, float* g_up, gl_stream s) {
    NEED(ctx);
    if (!x || !down || !up) return gl::set_error(GL_ERR_ARG, "gl_op_lora_linear: null pointer (x, down and up are required)");
    if (!dy && (u || dx || g_down || g_up)) return gl::set_error(GL_ERR_ARG, "gl_op_lora_linear: a backward output was asked for without dy");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy)) & 15) return gl::set_error(GL_ERR_ARG, "gl_op_lora_linear: x and dy are 16-byte aligned");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    const int rc = gl::train_prim_lora_linear(eng.arena(), eng.splitk_ws(), eng.splitk_ws_bytes(), M, K, N, rank, scale, down_kr, up_rn, x, down, up, dy, t, y,
                                              u, dx, g_down, g_up, S(s));
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    GL_API_END
}

int gl_lora_wgrad_chunk_rows(int M) { return M < 1 ? 0 : gl::train::lora_wgrad_chunk_rows(M); }

// ---- include/gligen_amd_train_lora_conv.h: the low-rank part of one adapted 3 x 3 conv by itself
int gl_op_lora_conv3(gl_ctx* ctx, int B, int H, int W, int Ci, int Co, int rank, float scale, int geom, const float* x, const float* down,
                     const float* up, const float* dy, float* t, float* y, float* u, float* dx, float* g_down, float* g_up, gl_stream s) {
    NEED(ctx);
    if (!x || !down || !up) return gl::set_error(GL_ERR_ARG, "gl_op_lora_conv3: null pointer (x, down and up are required)");
    if (!dy && (u || dx || g_down || g_up)) return gl::set_error(GL_ERR_ARG, "gl_op_lora_conv3: a backward output was asked for without dy");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy)) & 15) return gl::set_error(GL_ERR_ARG, "gl_op_lora_conv3: x and dy are 16-byte aligned");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    const int rc = gl::train_prim_lora_conv3(eng.arena(), eng.splitk_ws(), eng.splitk_ws_bytes(), B, H, W, Ci, Co, rank, scale, geom, x, down, up, dy, t, y, u,
                                             dx, g_down, g_up, S(s));
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    GL_API_END
}

// gl_unet_train_step_spatial and gl_unet_train_step_spatial_classes: `spi` holds the planes or the class maps
static int train_step_spatial(const char* what, gl_ctx* ctx, const gl_unet_config* cfg, const gl_train_unet_in* in, const gl::TrainSpatialIn& spi, int n_params,
                              const char* const* names, const float* const* params, float* const* grads, float* eps_out, float* loss, gl_stream s) {
    NEED(ctx);
    int lw_B = 0;
    const float* lw = take_loss_weights(ctx, &lw_B);
    if (!cfg || !in || !names || !params || !grads || !loss || n_params <= 0) return gl::set_error(GL_ERR_ARG, "%s: null pointer", what);
    if (lw && lw_B != in->B) return gl::set_error(GL_ERR_ARG, "%s: %d loss weights were set, the step's batch is %d", what, lw_B, in->B);
    if (cfg->inpaint_mode)
        return gl::set_error(GL_ERR_UNSUPPORTED, "%s: inpaint_mode with a spatial-map tokenizer is undefined in the reference (openaimodel.py:445-446); "
                                                 "gl_unet_train_step trains the inpainting models", what);
    if (cfg->grounding_kind != 3 || cfg->fuser_kind < 0 || cfg->fuser_kind > 2)
        return gl::set_error(GL_ERR_UNSUPPORTED, "%s: built for a spatial-map tokenizer (grounding_kind 3) with gatedSA, gatedSA2 or gatedCA fusers (fuser_kind 0 / 1 / 2)", what);
    if (cfg->tok_resize < 32 || cfg->tok_resize % 32 || cfg->extra_channels < 0)
        return gl::set_error(GL_ERR_ARG, "%s: tok_resize must be a positive multiple of 32", what);
    if (in->boxes || in->masks || in->positive_embeddings || in->text_masks || in->image_masks || in->image_embeddings)
        return gl::set_error(GL_ERR_ARG, "%s: the box / embedding inputs of gl_train_unet_in are NULL for a spatial-map model", what);
    const bool has_map = spi.map || spi.map_cls, has_extra = spi.extra || spi.extra_cls;
    if (!in->x || !in->timesteps || !in->context || !in->target || !has_map || !spi.mask || ((cfg->extra_channels > 0) != has_extra))
        return gl::set_error(GL_ERR_ARG, "%s: null input (grounding_extra_input is given iff extra_channels > 0)", what);
    const int Ng = (cfg->tok_resize / 32) * (cfg->tok_resize / 32);
    if (in->Ng != Ng) return gl::set_error(GL_ERR_ARG, "%s: Ng = %d, the tokenizer makes (tok_resize / 32)^2 = %d tokens", what, in->Ng, Ng);
    if (cfg->gr_out_dim != cfg->context_dim)
        return gl::set_error(GL_ERR_UNSUPPORTED, "%s: grounding out dim and context_dim are expected to be equal (768 in every shipped config)", what);
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    gl::TrainUNetCfg c{};
    c.in_channels = cfg->in_channels; c.out_channels = cfg->out_channels; c.model_channels = cfg->model_channels; c.num_res_blocks = cfg->num_res_blocks;
    c.num_heads = cfg->num_heads; c.context_dim = cfg->context_dim; c.gr_dim = 768; c.grounding_kind = 3; c.fuser_kind = cfg->fuser_kind; c.n_mult = cfg->n_mult; c.n_attn = cfg->n_attn;
    for (int i = 0; i < 8; ++i) { c.channel_mult[i] = cfg->channel_mult[i]; c.attention_resolutions[i] = cfg->attention_resolutions[i]; }
    c.extra_channels = cfg->extra_channels; c.tok_resize = cfg->tok_resize; c.tok_in_dim = cfg->tok_in_dim;
    gl::TrainUNetIn u{in->B, in->H, in->W, in->ctx_T, Ng, Ng, in->x, in->timesteps, in->context, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      in->target, in->fuser_scale, in->checkpoint};
    int rc = gl::unet_train_step(eng.arena(), eng.splitk_ws(), eng.splitk_ws_bytes(), c, u, n_params, names, params, grads, k_train_block_names, eps_out, loss, S(s),
                                 eng.train_events(), Engine::kTrainEvents, in->use_weight_cache ? eng.train_cache : nullptr, &spi, nullptr, 0, lw);
    if (rc != GL_OK) throw GlError(rc, gl::last_error());
    eng.train_events_recorded = true;
    GL_API_END
}

int gl_unet_train_step_spatial(gl_ctx* ctx, const gl_unet_config* cfg, const gl_train_unet_in* in, const gl_train_spatial_in* sp, int n_params,
                               const char* const* names, const float* const* params, float* const* grads, float* eps_out, float* loss, gl_stream s) {
    if (!sp) {
        drop_loss_weights(ctx);
        return gl::set_error(GL_ERR_ARG, "gl_unet_train_step_spatial: null pointer");
    }
    gl::TrainSpatialIn spi{sp->map, sp->map_channels, sp->map_h, sp->map_w, sp->mask, sp->extra, sp->extra_in_channels, sp->extra_h, sp->extra_w,
                           sp->ds_resize, sp->ds_mode, sp->ds_n_in, sp->ds_mid};
    return train_step_spatial("gl_unet_train_step_spatial", ctx, cfg, in, spi, n_params, names, params, grads, eps_out, loss, s);
}

// ---- include/gligen_amd_train_maps.h: the same iteration from u8 class maps, and its weight-gradient operator
int gl_unet_train_step_spatial_classes(gl_ctx* ctx, const gl_unet_config* cfg, const gl_train_unet_in* in, const gl_train_spatial_classes_in* sp,
                                       int n_params, const char* const* names, const float* const* params, float* const* grads, float* eps_out,
                                       float* loss, gl_stream s) {
    if (!sp || !sp->map || !sp->extra) drop_loss_weights(ctx);
    if (!sp) return gl::set_error(GL_ERR_ARG, "gl_unet_train_step_spatial_classes: null pointer");
    if (!sp->map || !sp->extra)
        return gl::set_error(GL_ERR_ARG, "gl_unet_train_step_spatial_classes: the tokenizer's map and grounding_extra_input are both u8 class maps here; one is NULL");
    gl::TrainSpatialIn spi{nullptr, 0, sp->map_h, sp->map_w, sp->mask, nullptr, 0, sp->extra_h, sp->extra_w, sp->ds_resize, sp->ds_mode, sp->ds_n_in, sp->ds_mid};
    spi.map_cls = sp->map;
    spi.extra_cls = sp->extra;
    return train_step_spatial("gl_unet_train_step_spatial_classes", ctx, cfg, in, spi, n_params, names, params, grads, eps_out, loss, s);
}

// ---- include/gligen_amd_train_inputs.h: the input stage of a training iteration, one launch
int gl_train_step_inputs(gl_ctx* ctx, const gl_train_step_inputs_args* args, gl_stream s) {
    NEED(ctx);
    if (!args) return gl::set_error(GL_ERR_ARG, "gl_train_step_inputs: null args");
    if (args->struct_size != sizeof(gl_train_step_inputs_args))
        return gl::set_error(GL_ERR_ARG, "gl_train_step_inputs: args->struct_size is %u, this library's gl_train_step_inputs_args has %zu bytes (set it to "
                                         "sizeof(gl_train_step_inputs_args))", args->struct_size, sizeof(gl_train_step_inputs_args));
    GL_API_BEGIN
    gl::TrainStepInputs a{args->B, args->C, args->H, args->W, args->n_t, args->n_boxes, args->inpaint ? 1 : 0, args->z, args->noise, args->timesteps,
                          args->sqrt_alphas_cumprod, args->sqrt_one_minus_alphas_cumprod, args->boxes, args->mask, args->x_rows, args->target_rows, args->t_float};
    GL_TRY(gl::train_step_inputs_launch(a, S(s)));
    ++ctx->eng->n_launches;
    GL_API_END
}

int gl_op_class_conv_wgrad(gl_ctx* ctx, int kind, const uint8_t* cls, int B, int H, int W, int n_classes, int R, const float* dy, int c_out,
                           float* dW, float* db, gl_stream s) {
    NEED(ctx);
    if (!cls || !dy || (!dW && !db)) return gl::set_error(GL_ERR_ARG, "gl_op_class_conv_wgrad: null class map / dy, or neither gradient asked for");
    GL_API_BEGIN
    size_t n = 0;
    GL_TRY(class_conv_wgrad_partial_floats(kind, B, H, W, n_classes, c_out, R, &n));
    gl::Arena& ar = ctx->eng->arena();
    const size_t mk = ar.mark();
    float* part = ar.get<float>(n);
    const size_t Ro = kind == kClassWgradDown ? R / 2 : R;
    const int rc = class_conv_wgrad_launch(kind, cls, dy, {(size_t)c_out * Ro * Ro, Ro * Ro, Ro, 1}, part, dW, db, B, H, W, n_classes, c_out, R, S(s));
    ar.release(mk);      // stream-ordered reuse, as every operator's workspace
    if (rc != GL_OK) return rc;
    ctx->eng->n_launches += 2;
    GL_API_END
}

int gl_train_weight_cache(gl_ctx* ctx, int enable, size_t* bytes) {
    NEED(ctx);
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    if (enable && !eng.train_cache) eng.train_cache = gl::train_cache_create();
    if (!enable && eng.train_cache) {
        HIPCK_API(hipDeviceSynchronize());    // (a step that reads the copies may still be in flight)
        gl::train_cache_destroy(eng.train_cache);
        eng.train_cache = nullptr;
    }
    if (bytes) *bytes = gl::train_cache_bytes(eng.train_cache);
    GL_API_END
}

int gl_train_wait_grads(gl_ctx* ctx, int index, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    if (index < 0 || index >= Engine::kTrainEvents) throw GlError(GL_ERR_ARG, "gl_train_wait_grads: milestone index out of range");
    if (!eng.train_events_recorded) throw GlError(GL_ERR_STATE, "gl_train_wait_grads: no gl_unet_train_step has run on this context");
    HIPCK_API(hipStreamWaitEvent(S(s), eng.train_events()[index], 0));
    GL_API_END
}

int gl_op_conv3x3(gl_ctx* ctx, const void* x0, int C0, const void* x1, int C1, int B, int H, int W,
                  const float* w_oihw, const float* bias, int Cout, int stride, int ups, int pad_lo,
                  const void* res, void* y, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    Arena& ar = ctx->eng->arena();
    ar.reset();
    const int Cin = C0 + C1;
    if (stride == 1 && ups == 1 && pad_lo == 1 && !res && Engine::upconv_phase_form(Cin, Cout)) {   // the engine's Upsample: phase form
        ConvW c;
        c.Cin = Cin; c.Cout = Cout; c.Npad = Cout; c.b = bias;
        bf16* w4 = ar.get<bf16>((size_t)16 * Cout * Cin);
        const int rp = pack_upconv_phases_launch(w_oihw, w4, Cout, Cin, Cout, S(s));
        if (rp != GL_OK) throw GlError(rp, gl::last_error());
        c.w4 = w4;
        ctx->eng->conv3x3(TRef{(const bf16*)x0, C0, (const bf16*)x1, C1}, B, H, W, c, 1, 1, 1, nullptr, 0, nullptr, S(s), (bf16*)y);
        return GL_OK;
    }
    bf16* wp = ar.get<bf16>((size_t)Cout * 9 * Cin);
    int r = pack_conv_weight_launch(w_oihw, wp, Cout, Cin, 3, 3, Cout, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    const int Hup = H << ups, Wup = W << ups;
    const int Ho = stride == 1 ? Hup : (pad_lo ? (Hup + 2 - 3) / 2 + 1 : (Hup + 1 - 3) / 2 + 1);
    const int Wo = stride == 1 ? Wup : (pad_lo ? (Wup + 2 - 3) / 2 + 1 : (Wup + 1 - 3) / 2 + 1);
    AOperand A{};
    A.p0 = (const bf16*)x0; A.C0 = C0; A.ld0 = C0; A.p1 = (const bf16*)x1; A.C1 = C1; A.ld1 = C1;
    A.mode = A_CONV3; A.Hin = H; A.Win = W; A.Ho = Ho; A.Wo = Wo; A.stride = stride; A.ups = ups; A.pad_lo = pad_lo;
    Epilogue E;
    epilogue_defaults(E);
    E.out = y; E.ldo = Cout; E.bias = bias; E.res = (const bf16*)res; E.ldres = Cout; E.rows_per_b = Ho * Wo;
    r = gemm_launch(A, wp, B * Ho * Wo, Cout, 9 * Cin, E, ctx->eng->splitk_ws(), ctx->eng->splitk_ws_bytes(), S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

int gl_op_gn_silu_conv3x3(gl_ctx* ctx, const void* x0, int C0, const void* x1, int C1, int B, int H, int W, const float* gamma, const float* beta,
                          float eps, const float* w_oihw, const float* bias, int Cout, const float* bias2, const void* res, void* y, int mode,
                          int* used_prologue, gl_stream s) {
    NEED(ctx);
    if (!x0 || !gamma || !beta || !w_oihw || !y || !used_prologue) return gl::set_error(GL_ERR_ARG, "gl_op_gn_silu_conv3x3: null pointer");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    Arena& ar = eng.arena();
    ar.reset();
    const int Cin = C0 + C1;
    bf16* wp = ar.get<bf16>((size_t)Cout * 9 * Cin);
    int r = pack_conv_weight_launch(w_oihw, wp, Cout, Cin, 3, 3, Cout, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    NormW n;
    n.g = gamma; n.b = beta; n.C = Cin;
    ConvW c;
    c.w = wp; c.b = bias; c.Cin = Cin; c.Cout = Cout;
    const bool saved = eng.gn_prologue_;
    if (mode >= 0) eng.gn_prologue_ = mode != 0;
    const int64_t n0 = eng.n_prologue_convs;
    try {
        eng.gn_silu_conv3x3(TRef{(const bf16*)x0, C0, (const bf16*)x1, C1}, B, H, W, n, eps, c, bias2, Cout, (const bf16*)res, (bf16*)y, S(s));
    } catch (...) {
        eng.gn_prologue_ = saved;
        throw;
    }
    eng.gn_prologue_ = saved;
    *used_prologue = eng.n_prologue_convs > n0 ? 1 : 0;
    if (mode == 1 && !*used_prologue) throw GlError(GL_ERR_UNSUPPORTED, "gl_op_gn_silu_conv3x3: this shape has no GroupNorm prologue (conv_halo_kernel, H W % 256 == 0)");
    GL_API_END
}

static bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what gl_op_groupnorm and gl_op_groupnorm_coef refuse before anything is allocated or launched: the kernels read x0, x1 and y in
// 16-byte pieces and gamma / beta as float4
static int groupnorm_args(const char* who, const void* x0, int C0, const void* x1, int C1, int B, int HW, const float* gamma, const float* beta,
                          const void* out) {
    if (!x0 || !gamma || !beta || !out || (C1 > 0 && !x1)) return gl::set_error(GL_ERR_ARG, "%s: null pointer", who);
    if (C0 < 0 || C1 < 0 || B < 1 || B > 65535 || HW < 1) return gl::set_error(GL_ERR_ARG, "%s: C0=%d C1=%d B=%d HW=%d", who, C0, C1, B, HW);
    if (!aligned_to(x0, 16) || (C1 > 0 && !aligned_to(x1, 16)) || !aligned_to(gamma, 16) || !aligned_to(beta, 16) || !aligned_to(out, 16))
        return gl::set_error(GL_ERR_ARG, "%s: x0, x1, gamma, beta and the output must be 16-byte aligned", who);
    return GL_OK;
}

int gl_op_groupnorm(gl_ctx* ctx, const void* x0, int C0, const void* x1, int C1, int B, int HW,
                    const float* gamma, const float* beta, float eps, int silu, void* y, gl_stream s) {
    NEED(ctx);
    if (int rc = groupnorm_args("gl_op_groupnorm", x0, C0, x1, C1, B, HW, gamma, beta, y)) return rc;
    GL_API_BEGIN
    Arena& ar = ctx->eng->arena();
    ar.reset();
    GNParams P{};
    P.x0 = (const bf16*)x0; P.C0 = C0; P.x1 = (const bf16*)x1; P.C1 = C1; P.B = B; P.HW = HW; P.eps = eps;
    P.gamma = gamma; P.beta = beta; P.y = (bf16*)y; P.silu = silu;
    P.partial = reinterpret_cast<float*>(ar.alloc(gn_partial_bytes(B, HW)));
    int r = groupnorm_launch(P, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

// include/gligen_amd_norm.h: the statistics-only GroupNorm into the caller's coefficient buffer
int gl_op_groupnorm_coef(gl_ctx* ctx, const void* x0, int C0, const void* x1, int C1, int B, int HW, const float* gamma, const float* beta,
                         float eps, float* coef, int* launches, gl_stream s) {
    NEED(ctx);
    if (!coef) return gl::set_error(GL_ERR_ARG, "gl_op_groupnorm_coef: no coefficient buffer");
    if (int rc = groupnorm_args("gl_op_groupnorm_coef", x0, C0, x1, C1, B, HW, gamma, beta, coef)) return rc;
    GL_API_BEGIN
    Arena& ar = ctx->eng->arena();
    ar.reset();
    GNParams P{};
    P.x0 = (const bf16*)x0; P.C0 = C0; P.x1 = (const bf16*)x1; P.C1 = C1; P.B = B; P.HW = HW; P.eps = eps;
    P.gamma = gamma; P.beta = beta; P.coef = coef;
    P.partial = reinterpret_cast<float*>(ar.alloc(gn_partial_bytes(B, HW)));
    int r = groupnorm_coef_launch(P, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    if (launches) *launches = groupnorm_coef_launches(HW, C0, C1);
    GL_API_END
}

int gl_op_layernorm(gl_ctx* ctx, const void* x, const void* x2, int B, int N1, int N2, int Tpad, int C,
                    const float* gamma, const float* beta, float eps, void* y, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    LNParams P{};
    P.x = (const bf16*)x; P.x2 = (const bf16*)x2; P.B = B; P.N1 = N1; P.N2 = N2; P.Tpad = Tpad; P.C = C; P.eps = eps;
    P.gamma = gamma; P.beta = beta; P.y = (bf16*)y;
    int r = layernorm_launch(P, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

// include/gligen_amd_norm.h: ln_kernel with every field of LNParams the caller's (row strides, the no-affine form)
int gl_op_layernorm_rows(gl_ctx* ctx, const gl_layernorm_rows_args* a, gl_stream s) {
    NEED(ctx);
    if (!a) return gl::set_error(GL_ERR_ARG, "gl_op_layernorm_rows: null args");
    if (a->struct_size != sizeof(gl_layernorm_rows_args))
        return gl::set_error(GL_ERR_ARG, "gl_op_layernorm_rows: args->struct_size is %u, this library's gl_layernorm_rows_args has %zu bytes",
                             a->struct_size, sizeof(gl_layernorm_rows_args));
    if (a->B < 1 || a->N1 < 0 || a->N2 < 0 || a->Tpad < 1 || a->C < 8)
        return gl::set_error(GL_ERR_ARG, "gl_op_layernorm_rows: B=%d N1=%d N2=%d Tpad=%d C=%d", a->B, a->N1, a->N2, a->Tpad, a->C);
    if (!a->y || (a->N1 > 0 && !a->x) || (a->N2 > 0 && !a->x2)) return gl::set_error(GL_ERR_ARG, "gl_op_layernorm_rows: null pointer");
    if ((a->gamma == nullptr) != (a->beta == nullptr)) return gl::set_error(GL_ERR_ARG, "gl_op_layernorm_rows: gamma and beta come together");
    if (!aligned_to(a->x, 16) || !aligned_to(a->x2, 16) || !aligned_to(a->y, 16) || !aligned_to(a->gamma, 16) || !aligned_to(a->beta, 16))
        return gl::set_error(GL_ERR_ARG, "gl_op_layernorm_rows: x, x2, y, gamma and beta must be 16-byte aligned");
    GL_API_BEGIN
    LNParams P{};
    P.x = (const bf16*)a->x; P.x2 = (const bf16*)a->x2; P.B = a->B; P.N1 = a->N1; P.N2 = a->N2; P.Tpad = a->Tpad; P.C = a->C; P.eps = a->eps;
    P.gamma = a->gamma; P.beta = a->beta; P.y = (bf16*)a->y; P.ldx = a->ldx; P.ldy = a->ldy;
    int r = layernorm_launch(P, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

// The projections of gl_op_attention into the head-layout buffers q, k, vt (one fused EPI_QKV_HEADS launch for self-attention, else
// q scatter, k scatter into the key-tile layout and v^T): shared by gl_op_attention and gl_op_attention_project.
static void attention_project(Engine& eng, const void* xq, const void* xkv, int B, int Nq, int Nk, int C, int Ck, int H, const float* wq,
                              const float* wk, const float* wv, bf16* q, bf16* k, bf16* vt, int Tq_pad, int Tk_pad, int dp, int dpv, int vt_layout,
                              hipStream_t s) {
    Arena& ar = eng.arena();
    const int d = C / H, Tq = round_up(Nq, 64), Tk = round_up(Nk, 64);
    bf16* wqb = ar.get<bf16>((size_t)C * C);
    bf16* wkb = ar.get<bf16>((size_t)C * Ck);
    bf16* wvb = ar.get<bf16>((size_t)C * Ck);
    bf16* xqp = ar.get<bf16>((size_t)B * Tq * C);
    bf16* xkp = ar.get<bf16>((size_t)B * Tk * Ck);
    auto ck = [&](int rc) { if (rc != GL_OK) throw GlError(rc, gl::last_error()); };
    ck(cast_f32_bf16_launch(wq, wqb, (int64_t)C * C, s));
    ck(cast_f32_bf16_launch(wk, wkb, (int64_t)C * Ck, s));
    ck(cast_f32_bf16_launch(wv, wvb, (int64_t)C * Ck, s));
    ck(pad_rows_bf16_launch((const bf16*)xq, xqp, B, Nq, Tq, C, s));
    ck(pad_rows_bf16_launch((const bf16*)xkv, xkp, B, Nk, Tk, Ck, s));
    // self-attention (same rows for q, k, v): the engine's fused projection, one EPI_QKV_HEADS GEMM (GL_QKV_FUSED=0: off)
    const bool fused = xq == xkv && C == Ck && Nq == Nk && gemm_supports_qkv() && (2 * C) % 128 == 0 &&
                       !(dev_env("GL_QKV_FUSED") && atoi(dev_env("GL_QKV_FUSED")) == 0);
    if (fused) {
        bf16* wqkv = ar.get<bf16>((size_t)3 * C * C);
        ck(cast_f32_bf16_launch(wq, wqkv, (int64_t)C * C, s));
        ck(cast_f32_bf16_launch(wk, wqkv + (size_t)C * C, (int64_t)C * C, s));
        ck(cast_f32_bf16_launch(wv, wqkv + (size_t)2 * C * C, (int64_t)C * C, s));
        Epilogue E = e_heads(EPI_QKV_HEADS, q, k, C, H, d, dp, Tq, Tq_pad, Tk_pad);
        E.vt = vt; E.DPV = dpv; E.vt_perm32 = vt_layout;
        ck(gemm_launch(a_rows(xqp, C), wqkv, B * Tq, 3 * C, C, E, nullptr, 0, s));
    } else {
        ck(gemm_launch(a_rows(xqp, C), wqb, B * Tq, C, C, e_heads(EPI_QK_HEADS, q, nullptr, C, H, d, dp, Tq, Tq_pad, 0), eng.splitk_ws(),
                       eng.splitk_ws_bytes(), s));
        {
            Epilogue E = e_heads(EPI_QK_HEADS, k, nullptr, C, H, d, dp, Tk, Tk_pad, 0);
            E.q_tiled = 1;
            ck(gemm_launch(a_rows(xkp, Ck), wkb, B * Tk, C, Ck, E, eng.splitk_ws(), eng.splitk_ws_bytes(), s));
        }
        {
            Epilogue E;
            epilogue_defaults(E);
            E.mode = EPI_VT_HEADS; E.out = vt; E.H = H; E.d = d; E.DPV = dpv; E.T = Tk; E.Tpad_k = Tk_pad; E.vt_perm32 = vt_layout;
            ck(gemm_launch_t(wvb, C, xkp, B * Tk, Ck, E, s));
        }
    }
}

int gl_op_attention(gl_ctx* ctx, const void* xq, const void* xkv, int B, int Nq, int Nk, int C, int Ck, int H,
                    const float* wq, const float* wk, const float* wv, void* o, gl_stream s) {
    NEED(ctx);
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    eng.arena().reset();
    if (C % H != 0) throw GlError(GL_ERR_ARG, "C must be divisible by H");
    const int d = C / H;
    int dp, dpv;
    int r = attn_dims(d, &dp, &dpv);
    if (r != GL_OK) throw GlError(r, gl::last_error());
    const int Tq = round_up(Nq, 64), Tk = round_up(Nk, 64);
    const int vt_layout = attn_vt_layout(d, Nk, &dpv);
    AttnBufs& bufs = eng.attn_bufs(B, H, d, Tq, Tk, dpv);
    attention_project(eng, xq, xkv, B, Nq, Nk, C, Ck, H, wq, wk, wv, bufs.q, bufs.k, bufs.vt, bufs.Tq_pad, bufs.Tk_pad, dp, dpv, vt_layout, S(s));
    AttnParams P = attn_params(bufs.q, bufs.k, bufs.vt, (bf16*)o, H, d, Nq, Nk, bufs.Tq_pad, bufs.Tk_pad, vt_layout);
    P.counters = eng.attn_counters();     // nullptr unless gl_attn_regime_counters switched counting on
    r = attn_launch(P, B, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

// include/gligen_amd_gemm_plans.h: the same projections into the caller's buffers
int gl_op_attention_project(gl_ctx* ctx, const void* xq, const void* xkv, int B, int Nq, int Nk, int C, int Ck, int H, const float* wq,
                            const float* wk, const float* wv, void* q, void* k, void* vt, gl_attn_proj_layout* layout, gl_stream s) {
    NEED(ctx);
    if (!layout) return gl::set_error(GL_ERR_ARG, "gl_op_attention_project: null layout");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    if (H <= 0 || C % H != 0) throw GlError(GL_ERR_ARG, "C must be divisible by H");
    const int d = C / H;
    int dp, dpv;
    int r = attn_dims(d, &dp, &dpv);
    if (r != GL_OK) throw GlError(r, gl::last_error());
    const int vt_layout = attn_vt_layout(d, Nk, &dpv);
    *layout = gl_attn_proj_layout{d, dp, dpv, round_up(Nq, 64), round_up(Nk, 64), round_up(round_up(Nq, 64), 128), round_up(Nk, 64), vt_layout};
    if (!q && !k && !vt) return GL_OK;
    if (!xq || !xkv || !wq || !wk || !wv || !q || !k || !vt) throw GlError(GL_ERR_ARG, "gl_op_attention_project: null pointer");
    eng.arena().reset();
    attention_project(eng, xq, xkv, B, Nq, Nk, C, Ck, H, wq, wk, wv, (bf16*)q, (bf16*)k, (bf16*)vt, layout->tq_pad, layout->tk_pad, dp, dpv, vt_layout, S(s));
    GL_API_END
}

// include/gligen_amd_gemm_plans.h: the second token range of existing q, k, v^T buffers (the launch of Engine::fuser_kv_fill)
int gl_op_attention_project_range(gl_ctx* ctx, const void* x, int B, int Tr, int tok_off, int C, int H, const float* wq, const float* wk,
                                  const float* wv, const float* bias, void* q, void* k, void* vt, const gl_attn_proj_layout* layout, gl_stream s) {
    NEED(ctx);
    if (!x || !wq || !wk || !wv || !q || !k || !vt || !layout) return gl::set_error(GL_ERR_ARG, "gl_op_attention_project_range: null pointer");
    if (B < 1 || Tr < 64 || Tr % 64 || tok_off < 0 || tok_off % 64 || H <= 0 || C % H != 0 || layout->d != C / H)
        return gl::set_error(GL_ERR_ARG, "gl_op_attention_project_range: B=%d Tr=%d tok_off=%d C=%d H=%d d=%d (Tr, tok_off multiples of 64, d = C / H)", B, Tr, tok_off, C, H, layout->d);
    if (tok_off + Tr > layout->tq_pad || tok_off + Tr > layout->tk_pad)
        return gl::set_error(GL_ERR_ARG, "gl_op_attention_project_range: tokens [%d, %d) do not fit tq_pad=%d / tk_pad=%d", tok_off, tok_off + Tr, layout->tq_pad, layout->tk_pad);
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    int dp, dpv;
    int r = attn_dims(layout->d, &dp, &dpv);
    if (r != GL_OK) throw GlError(r, gl::last_error());
    if (dp != layout->dp || layout->dpv < layout->d) throw GlError(GL_ERR_ARG, "gl_op_attention_project_range: layout->dp / dpv are not this head size's");
    Arena& ar = eng.arena();
    ar.reset();
    auto ck = [&](int rc) { if (rc != GL_OK) throw GlError(rc, gl::last_error()); };
    bf16* wqkv = ar.get<bf16>((size_t)3 * C * C);
    ck(cast_f32_bf16_launch(wq, wqkv, (int64_t)C * C, S(s)));
    ck(cast_f32_bf16_launch(wk, wqkv + (size_t)C * C, (int64_t)C * C, S(s)));
    ck(cast_f32_bf16_launch(wv, wqkv + (size_t)2 * C * C, (int64_t)C * C, S(s)));
    Epilogue E = e_heads(EPI_QKV_HEADS, (bf16*)q, (bf16*)k, C, H, layout->d, dp, Tr, layout->tq_pad, layout->tk_pad);
    E.vt = (bf16*)vt; E.DPV = layout->dpv; E.tok_off = tok_off; E.vt_perm32 = layout->vt_perm32;
    E.bias = bias;
    ck(gemm_launch(a_rows((const bf16*)x, C), wqkv, B * Tr, 3 * C, C, E, eng.splitk_ws(), eng.splitk_ws_bytes(), S(s)));
    GL_API_END
}

// include/gligen_amd_gemm_plans.h: one gemm_launch with the epilogue the caller describes
int gl_op_gemm_epilogue(gl_ctx* ctx, const gl_gemm_epilogue_args* a, gl_stream s) {
    NEED(ctx);
    if (!a) return gl::set_error(GL_ERR_ARG, "gl_op_gemm_epilogue: null args");
    if (a->struct_size != sizeof(gl_gemm_epilogue_args))
        return gl::set_error(GL_ERR_ARG, "gl_op_gemm_epilogue: args->struct_size is %u, this library's gl_gemm_epilogue_args has %zu bytes", a->struct_size,
                             sizeof(gl_gemm_epilogue_args));
    if (!a->x0 || !a->w || !a->out || (a->C1 && !a->x1)) return gl::set_error(GL_ERR_ARG, "gl_op_gemm_epilogue: null pointer (x0, w, out; x1 when C1 > 0)");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    Arena& ar = eng.arena();
    ar.reset();
    AOperand A{};
    const bf16* w = (const bf16*)a->w;
    int M = a->M, K = a->K;
    if (a->conv) {
        const int Cin = a->C0 + a->C1;
        if (a->N < 1 || Cin < 1 || a->B < 1 || a->H < 1 || a->W < 1 || a->ups < 0 || a->ups > 1 || (a->stride != 1 && a->stride != 2))
            throw GlError(GL_ERR_ARG, "gl_op_gemm_epilogue: conv geometry");
        bf16* wp = ar.get<bf16>((size_t)a->N * 9 * Cin);
        int r = pack_conv_weight_launch((const float*)a->w, wp, a->N, Cin, 3, 3, a->N, S(s));
        if (r != GL_OK) throw GlError(r, gl::last_error());
        w = wp;
        const int Hup = a->H << a->ups, Wup = a->W << a->ups;
        const int Ho = a->stride == 1 ? Hup : (a->pad_lo ? (Hup + 2 - 3) / 2 + 1 : (Hup + 1 - 3) / 2 + 1);
        const int Wo = a->stride == 1 ? Wup : (a->pad_lo ? (Wup + 2 - 3) / 2 + 1 : (Wup + 1 - 3) / 2 + 1);
        A.p0 = (const bf16*)a->x0; A.C0 = a->C0; A.ld0 = a->C0; A.p1 = (const bf16*)a->x1; A.C1 = a->C1; A.ld1 = a->C1;
        A.mode = A_CONV3; A.Hin = a->H; A.Win = a->W; A.Ho = Ho; A.Wo = Wo; A.stride = a->stride; A.ups = a->ups; A.pad_lo = a->pad_lo;
        M = a->B * Ho * Wo; K = 9 * Cin;
    } else {
        A = a_rows((const bf16*)a->x0, K);
    }
    if (a->mode != EPI_ROWMAJOR && a->mode != EPI_NCHW_F32) throw GlError(GL_ERR_ARG, "gl_op_gemm_epilogue: mode is 0 (row-major) or 3 (NCHW fp32)");
    Epilogue E;
    epilogue_defaults(E);
    E.mode = a->mode; E.act = a->act; E.out = a->out; E.ldo = a->ldo; E.out_f32 = a->out_f32;
    E.bias = a->bias; E.bias2 = a->bias2; E.bias2_ld = a->bias2_ld; E.rows_per_b = a->rows_per_b;
    E.res = (const bf16*)a->res; E.ldres = a->ldres; E.gate = a->gate;
    E.n_real = a->n_real;
    E.remap_in = a->remap_in; E.remap_out = a->remap_out; E.remap_off = a->remap_off;
    int r = gemm_launch(A, w, M, a->N, K, E, eng.splitk_ws(), eng.splitk_ws_bytes(), S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

// ---- include/gligen_amd_conv8.h: conv8_kernel by name, the router's answer, the family's knobs
static bool conv8_describe(const gl_conv8_args* a, AOperand& A, Epilogue& E, int& M, int& K) {
    if (a->C0 < 1 || a->C1 < 0 || a->B < 1 || a->H < 1 || a->W < 1 || a->N < 1 || a->ups < 0 || a->ups > 1 || (a->stride != 1 && a->stride != 2) ||
        a->rows_per_b < 1)
        return false;
    const int Cin = a->C0 + a->C1;
    const int Hup = a->H << a->ups, Wup = a->W << a->ups;
    const int Ho = a->stride == 1 ? Hup : (a->pad_lo ? (Hup + 2 - 3) / 2 + 1 : (Hup + 1 - 3) / 2 + 1);
    const int Wo = a->stride == 1 ? Wup : (a->pad_lo ? (Wup + 2 - 3) / 2 + 1 : (Wup + 1 - 3) / 2 + 1);
    A = AOperand{};
    A.p0 = (const bf16*)a->x0; A.C0 = a->C0; A.ld0 = a->C0; A.p1 = (const bf16*)a->x1; A.C1 = a->C1; A.ld1 = a->C1;
    A.mode = A_CONV3; A.Hin = a->H; A.Win = a->W; A.Ho = Ho; A.Wo = Wo; A.stride = a->stride; A.ups = a->ups; A.pad_lo = a->pad_lo;
    M = a->B * Ho * Wo; K = 9 * Cin;
    epilogue_defaults(E);
    E.act = a->act; E.out = a->out; E.ldo = a->ldo; E.out_f32 = a->out_f32;
    E.bias = a->bias; E.bias2 = a->bias2; E.bias2_ld = a->bias2_ld; E.rows_per_b = a->rows_per_b;
    E.res = (const bf16*)a->res; E.ldres = a->ldres;
    return true;
}
int gl_conv8_routed(const gl_conv8_args* a) {
    if (!a || a->struct_size != sizeof(gl_conv8_args)) { gl::set_error(GL_ERR_ARG, "gl_conv8_routed: null args or a struct_size that is not this library's"); return -1; }
    AOperand A;
    Epilogue E;
    int M, K;
    if (!conv8_describe(a, A, E, M, K)) { gl::set_error(GL_ERR_ARG, "gl_conv8_routed: conv geometry"); return -1; }
    return gemm_conv8_supported(A, M, a->N, K, E) ? 1 : 0;
}
int gl_conv8_force_knobs(int on, int bn, int splits) {
    if (on < 0 || on > 1 || (bn != 0 && bn != 64 && bn != 80) || splits < 0 || splits > 32)
        return gl::set_error(GL_ERR_ARG, "gl_conv8_force_knobs: on %d, bn %d, splits %d (0 | 1, 0 | 64 | 80, 0..32)", on, bn, splits);
    gemm_conv8_force_knobs(on, bn, splits);
    return GL_OK;
}
int gl_op_conv8x8(gl_ctx* ctx, const gl_conv8_args* a, gl_stream s) {
    NEED(ctx);
    if (!a) return gl::set_error(GL_ERR_ARG, "gl_op_conv8x8: null args");
    if (a->struct_size != sizeof(gl_conv8_args))
        return gl::set_error(GL_ERR_ARG, "gl_op_conv8x8: args->struct_size is %u, this library's gl_conv8_args has %zu bytes", a->struct_size, sizeof(gl_conv8_args));
    if (!a->x0 || !a->w || !a->out || (a->C1 && !a->x1) || (a->splits > 1 && !a->slabs))
        return gl::set_error(GL_ERR_ARG, "gl_op_conv8x8: null pointer (x0, w, out; x1 when C1 > 0; slabs when splits > 1)");
    GL_API_BEGIN
    AOperand A;
    Epilogue E;
    int M, K;
    if (!conv8_describe(a, A, E, M, K)) throw GlError(GL_ERR_ARG, "gl_op_conv8x8: conv geometry");
    Arena& ar = ctx->eng->arena();
    ar.reset();
    bf16* wp = ar.get<bf16>((size_t)a->N * K);
    int r = pack_conv_weight_launch((const float*)a->w, wp, a->N, a->C0 + a->C1, 3, 3, a->N, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    r = gemm_conv8_launch(A, wp, M, a->N, K, E, a->splits > 1 ? a->slabs : nullptr, a->splits > 1 ? a->slab_bytes : 0, a->bn, a->splits, a->grid_cap, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

// include/gligen_amd_attention_core.h: one attention kernel on the caller's q, k, v^T (no projection in front, no buffer of the engine's)
int gl_op_attention_core(gl_ctx* ctx, const void* q, const void* k, const void* vt, const gl_attn_proj_layout* layout, int B, int H, int Nq,
                         int Nk, void* o, int ldo, int o_rows_per_b, int kernel, gl_stream s) {
    NEED(ctx);
    if (!q || !k || !vt || !o || !layout) return gl::set_error(GL_ERR_ARG, "gl_op_attention_core: null pointer");
    GL_API_BEGIN
    const gl_attn_proj_layout& L = *layout;
    int dp, dpv;
    int r = attn_dims(L.d, &dp, &dpv);
    if (r != GL_OK) throw GlError(r, gl::last_error());
    if (B <= 0 || H <= 0 || L.dp != dp) throw GlError(GL_ERR_ARG, "gl_op_attention_core: B, H > 0 and dp = 48 / 80 / 160 for d = 40 / 80 / 160");
    if (ldo < H * L.d || ldo % 4 != 0 || o_rows_per_b < Nq || (reinterpret_cast<uintptr_t>(o) & 7) != 0)
        throw GlError(GL_ERR_ARG, "gl_op_attention_core: ldo >= H d, ldo % 4 == 0, o_rows_per_b >= Nq, o 8-byte aligned");
    if (((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(vt)) & 15) != 0)
        throw GlError(GL_ERR_ARG, "gl_op_attention_core: q, k and vt are 16-byte aligned");
    if (L.vt_perm32 != 0 && L.vt_perm32 != 1) throw GlError(GL_ERR_ARG, "gl_op_attention_core: vt_perm32 is 0 or 1");
    // (the selector checks dpv against the named instantiation; attn_launch's own choice follows vt_perm32 alone)
    if (kernel == ATTN_SEL_AUTO && L.dpv != (L.vt_perm32 && L.d == 40 ? 48 : dpv))
        throw GlError(GL_ERR_ARG, "gl_op_attention_core: dpv does not belong to (d, vt_perm32)");
    AttnParams P = attn_params((const bf16*)q, (const bf16*)k, (const bf16*)vt, (bf16*)o, H, L.d, Nq, Nk, L.tq_pad, L.tk_pad, L.vt_perm32);
    P.ldo = ldo;
    P.o_rows_per_b = o_rows_per_b;
    P.counters = ctx->eng->attn_counters();     // as gl_op_attention: nullptr unless gl_attn_regime_counters switched counting on
    r = attn_launch_select(P, B, L.dpv, kernel, S(s));
    if (r != GL_OK) throw GlError(r, gl::last_error());
    GL_API_END
}

int gl_attn_regime_counters(gl_ctx* ctx, int enable, unsigned* lazy_moves, unsigned* reruns) {
    NEED(ctx);
    if (!lazy_moves || !reruns) return gl::set_error(GL_ERR_ARG, "gl_attn_regime_counters: null pointer");
    GL_API_BEGIN
    unsigned c[ATTN_CTR_N];
    ctx->eng->attn_regime_counters(enable, c);
    *lazy_moves = c[ATTN_CTR_LAZY_MOVES];
    *reruns = c[ATTN_CTR_RERUNS];
    GL_API_END
}


int gl_op_proj_attention(gl_ctx* ctx, const void* x, int B, int N, int C, int H, const float* pre_w, const float* pre_b, const void* pre_res,
                         const float* gamma, const float* beta, const float* wq, const float* wk, const float* wv, int Nkv_extra,
                         void* mid, void* o, int* used_rows, gl_stream s) {
    NEED(ctx);
    if (!x || !pre_w || !pre_b || !gamma || !beta || !wq || !wk || !wv || !mid || !o || !used_rows)
        return gl::set_error(GL_ERR_ARG, "gl_op_proj_attention: null pointer");
    GL_API_BEGIN
    Engine& eng = *ctx->eng;
    Arena& ar = eng.arena();
    ar.reset();
    auto ck = [&](int rc) { if (rc != GL_OK) throw GlError(rc, gl::last_error()); };
    if (C % H != 0 || N % 64 != 0 || Nkv_extra != 0) throw GlError(GL_ERR_ARG, "gl_op_proj_attention: C % H == 0, N % 64 == 0");
    const int d = C / H, M = B * N;
    int dp, dpv;
    ck(attn_dims(d, &dp, &dpv));
    const int vt_layout = attn_vt_layout(d, N, &dpv);
    AttnBufs& bufs = eng.attn_bufs(B, H, d, N, N, dpv);
    // LayerNorm folded into the three projections: W gamma (bf16), bias W beta
    bf16* wqkv = ar.get<bf16>((size_t)3 * C * C);
    float* bias = ar.get<float>((size_t)3 * C);
    {
        float* wf = ar.get<float>((size_t)C * C);
        const float* ws[3] = {wq, wk, wv};
        for (int i = 0; i < 3; ++i) {
            ck(ln_fold_launch(ws[i], nullptr, gamma, beta, wf, bias + (size_t)i * C, C, C, S(s)));
            ck(cast_f32_bf16_launch(wf, wqkv + (size_t)i * C * C, (int64_t)C * C, S(s)));
        }
    }
    const bool want = *used_rows != 0;
    const bool rows = want && qkv_rows_supported(M, C, d, N) && vt_layout == 1;
    *used_rows = rows ? 1 : 0;
    if (rows) {
        void* st = ar.alloc(qkv_rows_stream_bytes(C, true, 3));
        ck(qkv_rows_pack_launch(pre_w, wqkv, 3, st, C, S(s)));
        QkvRowsParams P{};
        P.x = (const bf16*)x; P.ldx = C; P.eps = 1e-5f; P.stream = st; P.M = M;
        P.pre = 1; P.pre_b = pre_b; P.pre_res = (const bf16*)pre_res; P.ld_pre_res = C; P.mid_out = (bf16*)mid; P.ld_mid = C;
        P.np = 3; P.bias = bias; P.q = bufs.q; P.k = bufs.k; P.vt = bufs.vt;
        P.H = H; P.d = d; P.DP = dp; P.DPV = dpv; P.T = N; P.Tpad_q = bufs.Tq_pad; P.Tpad_k = bufs.Tk_pad; P.vt_perm32 = vt_layout;
        ck(qkv_rows_launch(P, C, S(s)));
    } else {
        // the form it replaces: projection GEMM (+ residual), LayerNorm kernel without affine, fused q,k,v^T GEMM
        bf16* pw = ar.get<bf16>((size_t)C * C);
        ck(cast_f32_bf16_launch(pre_w, pw, (int64_t)C * C, S(s)));
        {
            ck(gemm_launch(a_rows((const bf16*)x, C), pw, M, C, C, e_rows_res(mid, C, pre_b, (const bf16*)pre_res), eng.splitk_ws(), eng.splitk_ws_bytes(), S(s)));
        }
        bf16* xn = ar.get<bf16>((size_t)M * C);
        LNParams L{};
        L.x = (const bf16*)mid; L.B = 1; L.N1 = M; L.N2 = 0; L.Tpad = M; L.C = C; L.eps = 1e-5f; L.y = xn;
        ck(layernorm_launch(L, S(s)));
        Epilogue E = e_heads(EPI_QKV_HEADS, bufs.q, bufs.k, C, H, d, dp, N, bufs.Tq_pad, bufs.Tk_pad);
        E.vt = bufs.vt; E.DPV = dpv; E.vt_perm32 = vt_layout; E.bias = bias;
        ck(gemm_launch(a_rows(xn, C), wqkv, M, 3 * C, C, E, nullptr, 0, S(s)));
    }
    ck(attn_launch(attn_params(bufs.q, bufs.k, bufs.vt, (bf16*)o, H, d, N, N, bufs.Tq_pad, bufs.Tk_pad, vt_layout), B, S(s)));
    GL_API_END
}

// include/gligen_amd_ffn_rows.h: the row-local kernels on the caller's buffers, every field of their parameter blocks the caller's.
// Folding and packing as gl_op_feedforward / gl_op_ff_chain / gl_op_ff_chain_q / gl_op_proj_attention do them; no other kernel
// stands in where the row-local one refuses.

int gl_op_ff_rows(gl_ctx* ctx, const gl_ff_rows_args* a, gl_stream s) {
    NEED(ctx);
    if (!a) return gl::set_error(GL_ERR_ARG, "gl_op_ff_rows: null args");
    if (a->struct_size != sizeof(gl_ff_rows_args))
        return gl::set_error(GL_ERR_ARG, "gl_op_ff_rows: args->struct_size is %u, this library's gl_ff_rows_args has %zu bytes", a->struct_size,
                             sizeof(gl_ff_rows_args));
    if (!a->x || !a->w1 || !a->b1 || !a->w2 || !a->b2 || !a->out) return gl::set_error(GL_ERR_ARG, "gl_op_ff_rows: null pointer");
    if ((a->gamma == nullptr) != (a->beta == nullptr)) return gl::set_error(GL_ERR_ARG, "gl_op_ff_rows: gamma and beta come together");
    GL_API_BEGIN
    Arena& ar = ctx->eng->arena();
    ar.reset();
    auto ck = [&](int rc) { if (rc != GL_OK) throw GlError(rc, gl::last_error()); };
    const int M = a->M, C = a->C;
    if (!ff_rows_supported(M, C)) throw GlError(GL_ERR_UNSUPPORTED, "gl_op_ff_rows: no row-local kernel for this shape (C = 320, M % 128 == 0)");
    if (a->pre != 0 && a->pre != 1) throw GlError(GL_ERR_ARG, "gl_op_ff_rows: pre is 0 or 1");
    if (a->post < 0 || a->post > 2) throw GlError(GL_ERR_ARG, "gl_op_ff_rows: post is 0, 1 or 2");
    if (a->post && !a->pre) throw GlError(GL_ERR_UNSUPPORTED, "gl_op_ff_rows: a trailing projection is built only together with a leading one");
    if (a->gamma && !a->normalize) throw GlError(GL_ERR_ARG, "gl_op_ff_rows: a LayerNorm affine needs normalize = 1");
    if (a->ldx < C || a->ldo < C || !aligned_to(a->x, 16) || !aligned_to(a->out, 8))
        throw GlError(GL_ERR_ARG, "gl_op_ff_rows: ldx, ldo >= C; x 16-byte, out 8-byte aligned");
    if (!a->pre && a->res && (a->ldres < C || !aligned_to(a->res, 8))) throw GlError(GL_ERR_ARG, "gl_op_ff_rows: ldres >= C, res 8-byte aligned");
    if (a->stats_out && (a->stats_ld < 1 || !aligned_to(a->stats_out, 8))) throw GlError(GL_ERR_ARG, "gl_op_ff_rows: stats_ld >= 1, stats_out 8-byte aligned");
    if (a->pre && (!a->pre_w || !a->pre_b || !a->pre_res || !a->mid_out || a->ld_pre_res < C || a->ld_mid < C || !aligned_to(a->pre_res, 8) ||
                   !aligned_to(a->mid_out, 8)))
        throw GlError(GL_ERR_ARG, "gl_op_ff_rows: the leading projection needs its weights, bias, residual and mid_out (strides >= C, 8-byte aligned)");
    if (a->post == 1 && (!a->post_w || !a->post_b || !a->post_res || a->ld_post_res < C || !aligned_to(a->post_res, 8)))
        throw GlError(GL_ERR_ARG, "gl_op_ff_rows: the trailing projection needs its weights, bias and residual (stride >= C, 8-byte aligned)");
    if (a->post == 2 && (!a->post_w || !a->gamma_q || !a->beta_q || !a->q || a->qT <= 0 || M % a->qT || a->qT % 32 || a->qTpad < a->qT || a->qDP < 40 ||
                         a->qDP % 4 || !aligned_to(a->q, 8)))
        throw GlError(GL_ERR_ARG, "gl_op_ff_rows: the trailing to_q projection needs Wq, its LayerNorm affine, q and qT % 32 == 0 | M, qTpad >= qT, qDP >= 40, qDP % 4 == 0");
    const float* w1e = a->w1;
    const float* b1e = a->b1;
    if (a->gamma) {
        float* wf = ar.get<float>((size_t)8 * C * C);
        float* bf = ar.get<float>((size_t)8 * C);
        ck(ln_fold_launch(a->w1, a->b1, a->gamma, a->beta, wf, bf, 8 * C, C, S(s)));
        w1e = wf; b1e = bf;
    }
    const float* post_w = a->post ? a->post_w : nullptr;
    const float* post_b = a->post_b;
    if (a->post == 2) {
        float* wqf = ar.get<float>((size_t)C * C);
        float* bqf = ar.get<float>((size_t)C);
        ck(ln_fold_launch(a->post_w, nullptr, a->gamma_q, a->beta_q, wqf, bqf, C, C, S(s)));
        post_w = wqf; post_b = bqf;
    }
    void* st = ar.alloc(ff_chain_stream_bytes(C, a->pre != 0, a->post != 0));
    ck(ff_chain_pack_launch(w1e, b1e, a->w2, a->pre ? a->pre_w : nullptr, post_w, st, C, S(s)));
    FFRowsParams P{};
    P.x = (const bf16*)a->x; P.ldx = a->ldx; P.normalize = a->normalize ? 1 : 0; P.eps = a->eps; P.stream = st; P.b2 = a->b2;
    P.res = a->pre ? nullptr : (const bf16*)a->res; P.ldres = a->ldres; P.gate = a->gate; P.out = (bf16*)a->out; P.ldo = a->ldo; P.M = M;
    P.stats_out = (float2*)a->stats_out; P.stats_ld = a->stats_ld;
    P.pre = a->pre; P.post = a->post;
    if (a->pre) {
        P.pre_b = a->pre_b; P.pre_res = (const bf16*)a->pre_res; P.ld_pre_res = a->ld_pre_res; P.pre_gate = a->pre_gate;
        P.mid_out = (bf16*)a->mid_out; P.ld_mid = a->ld_mid;
    }
    if (a->post) P.post_b = post_b;
    if (a->post == 1) { P.post_res = (const bf16*)a->post_res; P.ld_post_res = a->ld_post_res; }
    if (a->post == 2) { P.q = (bf16*)a->q; P.qDP = a->qDP; P.qT = a->qT; P.qTpad = a->qTpad; }
    ck(ff_rows_launch(P, C, S(s)));
    GL_API_END
}

int gl_op_qkv_rows(gl_ctx* ctx, const gl_qkv_rows_args* a, gl_stream s) {
    NEED(ctx);
    if (!a) return gl::set_error(GL_ERR_ARG, "gl_op_qkv_rows: null args");
    if (a->struct_size != sizeof(gl_qkv_rows_args))
        return gl::set_error(GL_ERR_ARG, "gl_op_qkv_rows: args->struct_size is %u, this library's gl_qkv_rows_args has %zu bytes", a->struct_size,
                             sizeof(gl_qkv_rows_args));
    if (!a->x || !a->w || !a->q) return gl::set_error(GL_ERR_ARG, "gl_op_qkv_rows: null pointer");
    if ((a->gamma == nullptr) != (a->beta == nullptr)) return gl::set_error(GL_ERR_ARG, "gl_op_qkv_rows: gamma and beta come together");
    GL_API_BEGIN
    Arena& ar = ctx->eng->arena();
    ar.reset();
    auto ck = [&](int rc) { if (rc != GL_OK) throw GlError(rc, gl::last_error()); };
    const int M = a->M, C = a->C, H = a->H, np = a->np;
    if (H <= 0 || C % H) throw GlError(GL_ERR_ARG, "gl_op_qkv_rows: C % H == 0");
    const int d = C / H;
    if (!qkv_rows_supported(M, C, d, a->T)) throw GlError(GL_ERR_UNSUPPORTED, "gl_op_qkv_rows: no row-local kernel for this shape (C = 320, d = 40, T % 128 == 0 divides M)");
    if (np != 1 && np != 3) throw GlError(GL_ERR_ARG, "gl_op_qkv_rows: np must be 1 (q) or 3 (q, k, v^T)");
    if (a->pre != 0 && a->pre != 1) throw GlError(GL_ERR_ARG, "gl_op_qkv_rows: pre is 0 or 1");
    if (a->ldx < C || !aligned_to(a->x, 16) || !aligned_to(a->q, 8) || a->Tpad_q < a->T || a->DP < d || a->DP % 8)
        throw GlError(GL_ERR_ARG, "gl_op_qkv_rows: ldx >= C, x 16-byte and q 8-byte aligned, Tpad_q >= T, DP >= d, DP % 8 == 0");
    if (np == 3 && (!a->k || !a->vt || !aligned_to(a->k, 16) || !aligned_to(a->vt, 16) || a->Tpad_k < a->T || a->Tpad_k % 64 || a->DPV < d))
        throw GlError(GL_ERR_ARG, "gl_op_qkv_rows: k and vt 16-byte aligned, Tpad_k >= T, Tpad_k % 64 == 0, DPV >= d");
    if (a->pre && (!a->pre_w || !a->pre_b || !a->mid_out || a->ld_mid < C || !aligned_to(a->mid_out, 8) ||
                   (a->pre_res && (a->ld_pre_res < C || !aligned_to(a->pre_res, 8))) || (a->stats_out && !aligned_to(a->stats_out, 8))))
        throw GlError(GL_ERR_ARG, "gl_op_qkv_rows: the leading projection needs its weights, bias and mid_out (strides >= C, 8-byte aligned)");
    if (a->in_period < 0 || (a->in_period && (a->in_period % a->T || M % a->in_period)))
        throw GlError(GL_ERR_ARG, "gl_op_qkv_rows: the input period must be whole samples and divide M");
    const int N = np * C;
    bf16* wb = ar.get<bf16>((size_t)N * C);
    float* bias = ar.get<float>((size_t)N);
    if (a->gamma) {
        float* wf = ar.get<float>((size_t)N * C);
        ck(ln_fold_launch(a->w, a->bias, a->gamma, a->beta, wf, bias, N, C, S(s)));
        ck(cast_f32_bf16_launch(wf, wb, (int64_t)N * C, S(s)));
    } else {
        ck(cast_f32_bf16_launch(a->w, wb, (int64_t)N * C, S(s)));
        if (a->bias) HIPCK_API(hipMemcpyAsync(bias, a->bias, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, S(s)));
        else ck(fill_f32_launch(bias, 0.f, N, S(s)));
    }
    void* st = ar.alloc(qkv_rows_stream_bytes(C, a->pre != 0, np));
    ck(qkv_rows_pack_launch(a->pre ? a->pre_w : nullptr, wb, np, st, C, S(s)));
    QkvRowsParams P{};
    P.x = (const bf16*)a->x; P.ldx = a->ldx; P.normalize = a->normalize ? 1 : 0; P.eps = a->eps; P.stream = st; P.M = M;
    P.pre = a->pre;
    if (a->pre) {
        P.pre_b = a->pre_b; P.pre_res = (const bf16*)a->pre_res; P.ld_pre_res = a->ld_pre_res; P.mid_out = (bf16*)a->mid_out; P.ld_mid = a->ld_mid;
        P.stats_out = (float2*)a->stats_out;
    }
    P.np = np; P.bias = bias; P.q = (bf16*)a->q; P.k = (bf16*)a->k; P.vt = (bf16*)a->vt;
    P.H = H; P.d = d; P.DP = a->DP; P.DPV = a->DPV; P.T = a->T; P.Tpad_q = a->Tpad_q; P.Tpad_k = a->Tpad_k; P.vt_perm32 = 1; P.in_period = a->in_period;
    ck(qkv_rows_launch(P, C, S(s)));
    GL_API_END
}

}  // extern "C"
