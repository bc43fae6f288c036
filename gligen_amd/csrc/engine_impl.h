// What the engine's translation units (engine*.hip) share and nobody else sees: the error macros, the launch log and the small
// constructors of the recurring GEMM operand / epilogue shapes.
#pragma once
#include "engine.h"

namespace gl {

#define CK(expr)                                              \
    do {                                                      \
        int _r = (expr);                                      \
        if (_r != GL_OK) throw GlError(_r, gl::last_error()); \
    } while (0)
#define HIPCK(expr)                                                                             \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            throw GlError(GL_ERR_HIP, std::string(#expr) + " -> " + hipGetErrorString(_e));     \
    } while (0)

// developer aid (GL_LAUNCH_LOG=file, tools/gpu_traffic.sh): one line per GEMM / conv / attention launch, in launch order
FILE* launch_log_file();

unsigned ff_rows_policy_epoch();   // bumped when the kernel-form policy's mode changes: captured graphs of another epoch are dropped

// counters of the guidance pair's shared prefix (tail of gl_ff_rows_policy_report): 0 = an evaluation shared its prefix, 1 = a row-local
// projection ran at the prefix batch, 2 = a row-local projection read prefix-batch rows through an input period
void cfg_shared_prefix_note(int what);

// RAII over gemm_set_plan_batch_scale: the launches in its scope run at 1 / scale of the batch they are planned for
struct PlanAsBatch {
    explicit PlanAsBatch(int scale) { gemm_set_plan_batch_scale(scale); }
    ~PlanAsBatch() { gemm_set_plan_batch_scale(1); }
};

// ---- the recurring GEMM operand / epilogue shapes: a call site states only what differs from these
inline AOperand a_rows(const bf16* x, int K) {
    AOperand A;
    aoperand_rows(A, x, K, K);
    return A;
}
// implicit im2col of the NHWC channel-concat x, 3x3 taps
inline AOperand a_conv3(const TRef& x, int Hin, int Win, int Ho, int Wo, int stride, int ups, int pad_lo) {
    AOperand A{};
    A.p0 = x.p0; A.C0 = x.C0; A.ld0 = x.C0;
    A.p1 = x.p1; A.C1 = x.C1; A.ld1 = x.C1;
    A.mode = A_CONV3;
    A.Hin = Hin; A.Win = Win; A.Ho = Ho; A.Wo = Wo; A.stride = stride; A.ups = ups; A.pad_lo = pad_lo;
    return A;
}
// nearest-2x upsample + 3x3 / pad 1 conv of the NHWC channel-concat x in phase form (gemm.h A_CONV2UP): M = 4 B Hin Win
inline AOperand a_conv2up(const TRef& x, int Hin, int Win) {
    AOperand A = a_conv3(x, Hin, Win, 2 * Hin, 2 * Win, 1, 0, 1);
    A.mode = A_CONV2UP;
    return A;
}
// row-major [M][ldo] (bf16 unless the caller sets out_f32) + bias
inline Epilogue e_rows(void* out, int ldo, const float* bias = nullptr) {
    Epilogue E;
    epilogue_defaults(E);
    E.out = out; E.ldo = ldo; E.bias = bias;
    return E;
}
// ... + residual [M][ldo]
inline Epilogue e_rows_res(void* out, int ldo, const float* bias, const bf16* res) {
    Epilogue E = e_rows(out, ldo, bias);
    E.res = res; E.ldres = ldo;
    return E;
}
// head layout: `mode` EPI_QK_HEADS (q, k) or EPI_QKV_HEADS (q, k, v^T), T tokens per sample
inline Epilogue e_heads(int mode, bf16* q, bf16* k, int C, int H, int d, int DP, int T, int Tpad_q, int Tpad_k) {
    Epilogue E;
    epilogue_defaults(E);
    E.mode = mode;
    E.q = q; E.k = k; E.C = C; E.H = H; E.d = d; E.DP = DP; E.T = T; E.Tpad_q = Tpad_q; E.Tpad_k = Tpad_k;
    return E;
}
// the LayerNorm in front of a folded projection, applied in its epilogue from the rows' statistics (gemm.h Epilogue::ln_stats)
inline void e_fold_ln(Epilogue& E, const RowStats& st, const float* csum, int C) {
    E.ln_stats = st.p; E.ln_nb = st.nb; E.ln_ld = st.ld; E.ln_csum = csum;
    E.ln_inv_c = 1.f / (float)C; E.ln_eps = 1e-5f;
}

}  // namespace gl
