// Training slice (second half): forward + backward of ONE BasicTransformerBlock with a gatedSA, gatedSA2 or
// gatedCA fuser (reference ldm/modules/attention.py:333-338, 236-244, 272-297, 207-212) under the reference's loss, with the gradients the reference's trainer
// asks for (trainer.py:217-245: the fuser.* parameters; the block input and the grounding tokens so that the step chains into
// position_net and the blocks in front). The implementation is five units behind train_impl.h: train_ops / train_attention /
// train_layers / train_spatial / train_unet .hip.
#pragma once
#include "common.h"

namespace gl {

struct TrainBlockDims {
    int B, N, Ng, C, heads, ctx_T, ctx_dim;
    float fuser_scale;      // GatedSelfAttentionDense.scale (attention.py:232)
    int fuser_kind = 0;     // 0 gatedSA, 1 gatedSA2 (N and Ng squares: the residual is the Ng tokens' attention output resized to the
                            // visual grid, train_fusers.h), 2 gatedCA (no fuser.linear: TP_F_LIN_W / _B null in params and grads; to_k /
                            // to_v are [C][ctx_dim] and read objs)
};

// Parameter slots: the reference state_dict of BasicTransformerBlock(fuser_type="gatedSA" / "gatedSA2"; "gatedCA" has no
// fuser.linear.*), fp32 device pointers
enum {
    TP_NORM1_W = 0, TP_NORM1_B, TP_A1_Q, TP_A1_K, TP_A1_V, TP_A1_O, TP_A1_OB,
    TP_F_LIN_W, TP_F_LIN_B, TP_F_N1_W, TP_F_N1_B, TP_F_Q, TP_F_K, TP_F_V, TP_F_O, TP_F_OB,
    TP_F_N2_W, TP_F_N2_B, TP_F_FF1_W, TP_F_FF1_B, TP_F_FF2_W, TP_F_FF2_B, TP_F_ALPHA_ATTN, TP_F_ALPHA_DENSE,
    TP_NORM2_W, TP_NORM2_B, TP_A2_Q, TP_A2_K, TP_A2_V, TP_A2_O, TP_A2_OB,
    TP_NORM3_W, TP_NORM3_B, TP_FF1_W, TP_FF1_B, TP_FF2_W, TP_FF2_B,
    TP_COUNT
};

class Arena;
// x [B][N][C], objs [B][Ng][ctx_dim], context [B][ctx_T][ctx_dim], target [B][N][C]: fp32 device. Outputs (fp32 device): y [B][N][C],
// loss[1] = mse_loss(y, target) (trainer.py:366), dx, dobjs, and grads[slot] for every non-null slot among the fuser's
// (TP_F_LIN_W .. TP_F_ALPHA_DENSE), each shaped like its parameter. bf16 GEMM operands, fp32 accumulation and fp32 elsewhere.
int block_train_step(Arena& ar, float* ws, size_t ws_bytes, const TrainBlockDims& d, const float* const* params, const float* x,
                     const float* objs, const float* context, const float* target, float* y, float* loss, float* dx, float* dobjs,
                     float* const* grads, hipStream_t s);

// SpatialTransformer (attention.py:340-376) with one BasicTransformerBlock: slots = [norm.weight, norm.bias, proj_in.weight, proj_in.bias,
// the block's TP_* slots, proj_out.weight, proj_out.bias]; d.N = H * W pixels, d.C = in_channels = heads * d_head
enum { ST_NORM_W = 0, ST_NORM_B, ST_PIN_W, ST_PIN_B, ST_BLOCK0, ST_POUT_W = ST_BLOCK0 + TP_COUNT, ST_POUT_B, ST_COUNT };
int st_train_step(Arena& ar, float* ws, size_t ws_bytes, const TrainBlockDims& d, const float* const* params, const float* x, const float* objs,
                  const float* context, const float* target, float* y, float* loss, float* dx, float* dobjs, float* const* grads, hipStream_t s);

// ---- ResBlock (openaimodel.py:154-232): the second block type of the UNet. Frozen in the reference's trainer, so its backward is the
// input gradient only. Parameter slots = its state_dict (skip_connection.* null when Cin == Cout: nn.Identity), fp32 device pointers
struct TrainResDims {
    int B, H, W, Cin, Cout, emb_dim;
};
enum {
    RP_GN1_W = 0, RP_GN1_B, RP_C1_W, RP_C1_B, RP_EMB_W, RP_EMB_B, RP_GN2_W, RP_GN2_B, RP_C2_W, RP_C2_B, RP_SKIP_W, RP_SKIP_B,
    RP_COUNT
};
// x [B][H*W][Cin], emb [B][emb_dim], target [B][H*W][Cout] fp32 device (pixel rows) -> y [B][H*W][Cout], loss[1] = mse_loss(y, target), dx
int resblock_train_step(Arena& ar, float* ws, size_t ws_bytes, const TrainResDims& d, const float* const* params, const float* x, const float* emb,
                        const float* target, float* y, float* loss, float* dx, hipStream_t s);

// Downsample (mode 0: conv3x3 stride 2) / Upsample (mode 1: nearest 2x + conv3x3) of C channels (openaimodel.py:64-124): forward, loss, dx.
// x [B][H*W][C], y / target [B][Ho*Wo][C] pixel rows
int resample_train_step(Arena& ar, float* ws, size_t ws_bytes, int mode, int B, int H, int W, int C, const float* w_oihw, const float* bias, const float* x,
                        const float* target, float* y, float* loss, float* dx, hipStream_t s);

// ---- the whole training iteration for a UNetModel (openaimodel.py:237-464): every grounding tokenizer, every fuser type
struct TrainUNetCfg {
    int in_channels, out_channels, model_channels, num_res_blocks, num_heads, context_dim, gr_dim;
    int grounding_kind;                 // 0 text, 1 text+image (two MLPs, tokens concatenated), 2 keypoint (points in `boxes`, 17 tokens per person),
                                        // 3 spatial map (ConvNeXt-tiny tokenizer; TrainSpatialIn)
    int n_mult, channel_mult[8], n_attn, attention_resolutions[8];
    int extra_channels;                 // grounding_kind 3: GroundingDownsampler output channels in front of the first conv (0: none)
    int tok_resize, tok_in_dim;         // grounding_kind 3: PositionNet resize_input; channels of a semantic map (sem: in_conv first), else 0
    int fuser_kind;                     // TrainBlockDims::fuser_kind of every block; 1 (gatedSA2) needs H == W and a square Ng
    int inpaint_mode;                   // grounding_kind 0 / 1 / 2: the first conv reads 2 * in_channels + 1 channels (openaimodel.py:299-302, 445-447)
};
// The spatial-map inputs of a training step (grounding_kind 3): the tokenizer's map and mask, grounding_extra_input and the
// GroundingDownsampler's constants (canny / depth / normal / sem / hed_grounding_downsampler.py)
struct TrainSpatialIn {
    const float* map;                   // [B][Ct][Ht][Wt]
    int Ct, Ht, Wt;
    const float* mask;                  // [B]
    const float* extra;                 // [B][Ce][He][We]; null iff extra_channels == 0
    int Ce, He, We;
    int ds_resize, ds_mode, ds_n_in, ds_mid;   // resize, 0 bicubic / 1 nearest, channels read, channels of the first conv (0: no layers)
    // A semantic-map model's inputs as u8 class maps (classmap.h) instead of one-hot planes: both set and map / extra null, or both
    // null. The class counts are tok_in_dim and ds_n_in; Ct and Ce are not read.
    const uint8_t* map_cls = nullptr;   // [B][Ht][Wt]
    const uint8_t* extra_cls = nullptr; // [B][He][We]
};
struct TrainUNetIn {
    int B, H, W, ctx_T, Ng;             // Ng: grounding tokens per sample = Ng_boxes (text) or 2 * Ng_boxes (text+image)
    int Ng_boxes;
    const float* x;                     // [B][H*W][in_channels] pixel rows: the noised latent; inpaint_mode: [B][H*W][2 * in_channels + 1], the
                                        // noised latent, z * mask, mask (inpainting_extra_input, trainer.py:343-344), concatenated by the caller
    const float* timesteps;             // [B]
    const float* context;               // [B][ctx_T][context_dim]
    const float* boxes;                 // [B][Ng_boxes][4]
    const float* masks;                 // [B][Ng_boxes]
    const float* positive_embeddings;   // [B][Ng_boxes][gr_dim]: the text embeddings
    const float* text_masks;            // text+image only: [B][Ng_boxes] each
    const float* image_masks;
    const float* image_embeddings;      // text+image only: [B][Ng_boxes][gr_dim]
    const float* target;                // [B][H*W][out_channels]: the noise
    float fuser_scale;
    int checkpoint;                     // 1: keep only every block's input and output; a block's backward recomputes its forward (same gradients, bit for bit)
};
// names / params / grads: the model's state_dict (fp32 device pointers; grads[i] non-null only for fuser.* and position_net.* entries:
// the reference's trainable set, trainer.py:217-245). block_names: the TP_* state_dict keys. eps_out (optional) [B][H*W][out_channels].
// cache (optional, round 6): the bf16 operand copies -- (hi | hi | lo) rows / transposes, packed conv weights and their dgrad forms -- of
// every parameter whose grads[i] is null are built once and reused by later calls: the caller promises that it only ever changes the
// parameters it asked gradients for (gligen_amd.train.TrainStep does; reference trainer.py:217-245 freezes everything else).
struct TrainWeightCache;
TrainWeightCache* train_cache_create();
void train_cache_destroy(TrainWeightCache* c);      // frees every cached copy
size_t train_cache_bytes(const TrainWeightCache* c);
// A LoRA adapter in training (include/gligen_amd_train_lora.h; train_lora.hip): `name` is the state_dict key of a frozen Linear's weight
// [N][K] -- attn1 / attn2 .to_q / to_k / to_v / to_out.0, ff.net.0.proj, ff.net.2 of a SpatialTransformer's block, or its proj_in /
// proj_out --, down [rank][K], up [N][rank] fp32 device; g_down / g_up shaped like them (null: not formed). The layer computes
// x W^T + scale (x down^T) up^T.
struct TrainLoraAdapter {
    const char* name;
    const float* down;
    const float* up;
    float* g_down;
    float* g_up;
    int rank;
    float scale;
};
int unet_train_step(Arena& ar, float* ws, size_t ws_bytes, const TrainUNetCfg& cfg, const TrainUNetIn& in, int n_params, const char* const* names,
                    const float* const* params, float* const* grads, const char* const* block_names, float* eps_out, float* loss, hipStream_t s,
                    hipEvent_t* grad_events = nullptr, int n_grad_events = 0, TrainWeightCache* cache = nullptr, const TrainSpatialIn* spatial = nullptr,
                    const TrainLoraAdapter* adapters = nullptr, int n_adapters = 0, const float* loss_weights = nullptr);
// loss_weights (optional) [B] fp32 device: loss = (1/n) sum_b w_b sum_i (y - target)^2 and its gradient, from train_run.hip
// (gl_train_set_loss_weights); null: mse_loss, every launch and every bit as before.
// adapters (optional): their gradients are final at the milestone of their SpatialTransformer, like that block's fuser gradients. With
// none, every launch and every bit is the unadapted step's.
// grad_events (optional): event j is recorded on `s` when the backward of the j-th SpatialTransformer (module order) has written its
// fuser gradients -- the backward runs from the last block to the first, so high j come early --, event [number of SpatialTransformers]
// when position_net's, downsample_net's and the first conv's (the last gradients of the step) are written.
// spatial: required for grounding_kind 3; the trainable set then also admits downsample_net.* and, with extra_channels > 0,
// input_blocks.0.0.weight (trainer.py:189-194, 233). An inpainting model (inpaint_mode, grounding_kind 0 / 1 / 2) admits that weight too.

// The step's input stage in one launch (include/gligen_amd_train_inputs.h, train_inputs.hip): q_sample, the box mask, z * mask and the
// concatenation as the pixel rows TrainUNetIn.x / .target point at. Device pointers; boxes xor mask when inpaint, neither otherwise.
struct TrainStepInputs {
    int B, C, H, W, n_t, n_boxes, inpaint;
    const float *z, *noise;             // [B][C][H][W]
    const int64_t* timesteps;           // [B]
    const float *sqrt_ac, *sqrt_1mac;   // [n_t]
    const float* boxes;                 // [B][n_boxes][4]
    const float* mask;                  // [B][H*W]
    float *x_rows, *target_rows, *t_float;
};
int train_step_inputs_launch(const TrainStepInputs& a, hipStream_t s);

// ---- The primitives by themselves (include/gligen_amd_train_prims.h; the argument lists are the entry points'): a Ctx over the arena
// as the slices above build it -- no weight cache --, the Ctx methods the step is composed of, results copied to the caller on `s`.
// train_prim_attention is in train_attention.hip, train_prim_conv3 in train_layers.hip (it reaches the resampling layers),
// train_prim_conv_direct in train_spatial.hip (next to conv_wgrad), the others in train_ops.hip.
int train_prim_attention(Arena& ar, float* ws, size_t ws_bytes, int B, int H, int D, int Nq, int Nk, const float* q, const float* k, const float* v,
                         const float* dout, float* o, float* lse, float* dq, float* dk, float* dv, hipStream_t s);
int train_prim_linear(Arena& ar, float* ws, size_t ws_bytes, int M, int N, int K, const float* x, const float* W, const float* b, const float* dy, float* y,
                      float* dx, float* dW, float* db, hipStream_t s);
int train_prim_layernorm(Arena& ar, float* ws, size_t ws_bytes, int R, int C, float eps, const float* x, const float* g, const float* b, const float* dy,
                         int accumulate, float* y, float* xhat, float* rstd, float* dx, float* dgamma, float* dbeta, hipStream_t s);
int train_prim_groupnorm(Arena& ar, float* ws, size_t ws_bytes, int B, int HW, int C, int silu, float eps, const float* x, const float* g, const float* b,
                         const float* da, int accumulate, float* a, float* xhat, float* rstd, float* dx, hipStream_t s);
int train_prim_geglu(Arena& ar, float* ws, size_t ws_bytes, int R, int I, const float* u, const float* dh, float* h, float* du, hipStream_t s);
int train_prim_dot(Arena& ar, float* ws, size_t ws_bytes, size_t n, const float* a, const float* b, const float* alpha, float scale, int mode, float* out,
                   hipStream_t s);
int train_prim_conv3(Arena& ar, float* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout, int geom, const float* x, const float* w_oihw,
                     const float* bias, const float* dy, float* y, float* dx, hipStream_t s);
int train_prim_conv_direct(Arena& ar, float* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout, int c0, int n, const float* x, const float* w_oihw,
                           const float* bias, const float* dy, float* y, float* dx, float* dW, hipStream_t s);

// The low-rank part of one adapted Linear by itself (include/gligen_amd_train_lora.h; train_lora.hip)
int train_prim_lora_linear(Arena& ar, float* ws, size_t ws_bytes, int M, int K, int N, int r, float scale, int down_kr, int up_rn, const float* x,
                           const float* down, const float* up, const float* dy, float* t, float* y, float* u, float* dx, float* g_down, float* g_up,
                           hipStream_t s);

// The low-rank part of one adapted 3 x 3 conv by itself (include/gligen_amd_train_lora_conv.h; train_lora_conv.hip)
int train_prim_lora_conv3(Arena& ar, float* ws, size_t ws_bytes, int B, int H, int W, int Ci, int Co, int r, float scale, int geom, const float* x,
                          const float* down, const float* up, const float* dy, float* t, float* y, float* u, float* dx, float* g_down, float* g_up,
                          hipStream_t s);

namespace train { int lora_wgrad_chunk_rows(int M); }      // rows per partial sum of its weight-gradient kernel

// One AdamW update of a flat fp32 parameter range, in place (torch.optim.AdamW semantics: trainer.py:245, :384 opt.step()); step = 1, 2, ...
int adamw_step(float* p, const float* g, float* m, float* v, size_t n, double lr, double b1, double b2, double eps, double wd, int step, hipStream_t s);
// The same update (the same bits for p, m, v) and ema = ema_rate * ema + (1 - ema_rate) * p_new in one pass (train_optim.hip; trainer.py:121-123, 388-391)
int adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, double lr, double b1, double b2, double eps, double wd, double ema_rate,
                   int step, hipStream_t s);

}  // namespace gl
