// bf16 MFMA GEMM + implicit-GEMM 3x3 convolution for gfx950 (CDNA4, wave64).
//
//   C[M][N] = A[M][K] * W[N][K]^T   (+ fused epilogue)
//
// Replaces every nn.Linear / 1x1 conv / 3x3 conv the reference's UNet and VAE dispatch to
// cuBLAS / cuDNN (reference ldm/modules/diffusionmodules/openaimodel.py:116-232 ResBlock convs,
// ldm/modules/attention.py:37-64,102-186 projections and GEGLU, ldm/modules/diffusionmodules/
// model.py:82-141 VAE ResnetBlock).
//
// Six files behind one internal header (gemm_impl.h: the helpers the kernels share, Launch, the units' entry functions):
//   gemm_basic.hip  gemm_glds_kernel (N < 128, the independent reference of `kbench check`) and gemm_p_kernel (operands beyond 2 GiB)
//   gemm_u.hip      gemm_u_kernel, the default: GEMMs and 3x3 convs of every kind
//   gemm_halo.hip   conv_halo_kernel: stride-1 3x3 convs on power-of-two images, optionally with the GroupNorm + SiLU prologue
//   gemm_wide.hip   gemm_wide_kernel: long-K, wide-N row GEMMs (FF-out, GEGLU projections)
//   gemm_conv8.hip  conv8_kernel: the stride-1 3x3 convs of the 8 x 8 level, each image staged once per channel chunk (A_CONV8)
//   gemm.hip        this file: execute() for a GemmPlan, the split-K reduce, the on-device tuner's timing loop, gemm_launch
// Which kernel runs a problem (family, tile, K split, resident grid, item order) is decided in gemm_plan.h / gemm_plan.hip, host code
// without a HIP call.
#include "gemm_impl.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace gl {

void epilogue_defaults(Epilogue& E) {
    E = Epilogue{};
    E.mode = EPI_ROWMAJOR;
    E.act = ACT_NONE;
    E.rows_per_b = 1;
    E.rpb_magic = 1; E.rpb_shift = 0;
}

void aoperand_rows(AOperand& A, const bf16* p, int K, int ld) {
    A = AOperand{};
    A.p0 = p;
    A.C0 = K;
    A.ld0 = ld;
    A.mode = A_ROWS;
}

// Deterministic split-K reduction + epilogue: one thread per (row, group of 4 columns).
__global__ void __launch_bounds__(256)
splitk_reduce_kernel(const float* __restrict__ ws, int splits, int M, int N, Epilogue E) {
    const int groups = N >> 2;
    const int64_t total = (int64_t)M * groups;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        int m = (int)(idx / groups);
        int n0 = (int)(idx - (int64_t)m * groups) << 2;
        if (E.act == ACT_GEGLU && E.geglu16) {
            if (n0 & 16) continue;  // gate groups are consumed by their value group
            float val[4] = {0, 0, 0, 0}, gate[4] = {0, 0, 0, 0};
            for (int z = 0; z < splits; ++z) {
                const float* p = ws + ((size_t)z * M + m) * N + n0;
                float4 a = *reinterpret_cast<const float4*>(p);
                float4 b = *reinterpret_cast<const float4*>(p + 16);
                val[0] += a.x; val[1] += a.y; val[2] += a.z; val[3] += a.w;
                gate[0] += b.x; gate[1] += b.y; gate[2] += b.z; gate[3] += b.w;
            }
            epi_geglu4_t16(E, m, n0, val, gate);
        } else if (E.act == ACT_GEGLU) {
            if (n0 & 8) continue;  // gate groups are consumed by their value group
            float val[4] = {0, 0, 0, 0}, gate[4] = {0, 0, 0, 0};
            for (int z = 0; z < splits; ++z) {
                const float* p = ws + ((size_t)z * M + m) * N + n0;
                float4 a = *reinterpret_cast<const float4*>(p);
                float4 b = *reinterpret_cast<const float4*>(p + 8);
                val[0] += a.x; val[1] += a.y; val[2] += a.z; val[3] += a.w;
                gate[0] += b.x; gate[1] += b.y; gate[2] += b.z; gate[3] += b.w;
            }
            epi_geglu4(E, m, n0, val, gate);
        } else {
            // Row-major bf16 outputs (every split-K conv and projection of the UNet): bias, per-sample bias, residual and gate are
            // requested BEFORE the slabs, unconditionally (an absent operand reads the slab area and is never used -- behind
            // `if (E.res)` hipcc would unpack inside the branch and wait there); they arrive while the slabs are summed
            const bool fast = E.mode == EPI_ROWMAJOR && !E.out_f32 && !E.remap_in && E.act != ACT_GELU && E.act != ACT_QUICK_GELU && !E.ln_stats;
            // (no `if (fast)` around the loads either: a value that is "loaded or zero" is the pattern that gets waited for in place)
            const float4 pb = *reinterpret_cast<const float4*>((fast && E.bias) ? E.bias + n0 : ws);
            const float4 pb2 = *reinterpret_cast<const float4*>((fast && E.bias2) ? E.bias2 + (size_t)div_rpb(E, m) * E.bias2_ld + n0 : ws);
            const uint2 pr = *reinterpret_cast<const uint2*>((fast && E.res) ? reinterpret_cast<const void*>(E.res + (size_t)m * E.ldres + n0)
                                                                              : reinterpret_cast<const void*>(ws));
            const float pg = *((fast && E.res && E.gate) ? E.gate : ws);
            // slabs four at a time, all four loads in flight before the first add (a slab beyond `splits` re-reads the last one and
            // counts as zero): one load per loop trip is one L2 round trip per slab and thread, 8-16 of them in a row at the 8 x 8
            // level. Summation order stays z = 0 .. splits - 1.
            float v[4] = {0, 0, 0, 0};
            const float* p0 = ws + (size_t)m * N + n0;
            const size_t zs = (size_t)M * N;
            for (int z = 0; z < splits; z += 4) {
                float4 a[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const float4*>(p0 + (size_t)min(z + u, splits - 1) * zs);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = z + u < splits;
                    v[0] += ok ? a[u].x : 0.f; v[1] += ok ? a[u].y : 0.f; v[2] += ok ? a[u].z : 0.f; v[3] += ok ? a[u].w : 0.f;
                }
            }
            if (E.ln_stats) {   // folded LayerNorm (gemm.h): rstd (acc - mean csum); epi_finish4 adds the folded bias
                const float2 st = ln_row_stats(E, m);
                const float4 cs = *reinterpret_cast<const float4*>(E.ln_csum + n0);
                v[0] = st.y * (v[0] - st.x * cs.x); v[1] = st.y * (v[1] - st.x * cs.y);
                v[2] = st.y * (v[2] - st.x * cs.z); v[3] = st.y * (v[3] - st.x * cs.w);
            }
            if (fast) {
                if (E.bias) { v[0] += pb.x; v[1] += pb.y; v[2] += pb.z; v[3] += pb.w; }
                if (E.bias2) { v[0] += pb2.x; v[1] += pb2.y; v[2] += pb2.z; v[3] += pb2.w; }
                if (E.act == ACT_SILU) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = silu_f(v[i]);
                }
                if (E.res) {
                    U2BF4 r;
                    r.u = pr;
                    const float g = E.gate ? pg : 1.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = bf2f(r.e[i]) + g * v[i];
                }
                int mo = m;
                if (E.up_win) {   // A_CONV2UP: slab row = phase * (M / 4) + phase row; see epilogue_staged of gemm_u_kernel
                    const int mp = M >> 2, ph = m / mp, r = m - ph * mp, q = div_rpb(E, r);
                    mo = ((2 * q + (ph >> 1)) * E.up_win + (r - q * E.up_win)) * 2 + (ph & 1);
                }
                store_bf16x4(reinterpret_cast<bf16*>(E.out) + (size_t)mo * E.ldo + n0, v);
            } else {
                epi_finish4(E, m, n0, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side: gemm_plan.h decides what runs; here a GemmPlan is executed, and the on-device tuner times the planner's candidates.
static thread_local GemmPlan t_last = [] { GemmPlan p{}; strcpy(p.name, "gemm"); return p; }();   // per calling thread: one engine context per thread
int gemm_last_stats_nb() { return t_last.stats_nb; }
const char* gemm_last_kernel_name() { return t_last.name; }
void gemm_last_cfg(int* tm, int* tn, int* splits) { *tm = t_last.tm; *tn = t_last.tn; *splits = t_last.splits; }
// the plan log: a ring of the calling thread's last kGemmLogSize launches (ops such as gl_op_attention make several)
static thread_local GemmLogEntry t_log[kGemmLogSize];
static thread_local int t_log_n = 0;   // launches since the last clear
void gemm_plan_log_clear() { t_log_n = 0; }
int gemm_plan_log(GemmLogEntry* out, int max, int* launches) {
    if (launches) *launches = t_log_n;
    const int n = std::max(0, std::min(std::min(t_log_n, kGemmLogSize), max));
    for (int i = 0; i < n; ++i) out[i] = t_log[(t_log_n - n + i) % kGemmLogSize];
    return n;
}

namespace {

// Launch what the plan says on `stream`: the kernel of its instantiation (the family's unit knows them), then the split-K reduce.
int execute(const GemmPlan& p, const AOperand& A, const bf16* W, int M, int N, int K, const Epilogue& E_in, float* ws, hipStream_t stream) {
    Epilogue E = E_in;                                                                     // what the kernels see: no statistics pointer
    if ((p.family == GEMM_P || p.family == GEMM_U) && !p.stats_nb) E.stats_out = nullptr;  // unless this launch produces them (the staged epilogue writes whenever the pointer is set)
    const Launch l{A, W, M, N, K, E, ws, stream};
    switch (p.family) {
        case GEMM_GLDS:
        case GEMM_P: GL_TRY(gemm_exec_basic(l, p)); break;
        case GEMM_U: GL_TRY(gemm_exec_u(l, p)); break;
        case GEMM_HALO: GL_TRY(gemm_exec_halo(l, p)); break;
        case GEMM_WIDE: GL_TRY(gemm_exec_wide(l, p)); break;
        case GEMM_CONV8: GL_TRY(gemm_exec_conv8(l, p)); break;
        default: return gemm_unknown_tile();
    }
    if (p.splits > 1) {
        int64_t total = (int64_t)M * (N / 4);
        int blocks = (int)fmin((double)cdiv64(total, 256), 4096.0);
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, stream, ws, p.splits, M, N, E);
        GL_LAUNCH_CHECK();
    }
    return GL_OK;
}

// Autotuner: the first (eager, non-capturing) launch of every distinct problem the shipped table does not hold times the planner's
// tile / split / residency candidates on the device with the caller's own buffers; gemm_plan caches the winner. A launch only writes
// E.out (and the split-K workspace), and the engine never aliases E.out with an input, so re-running a launch is idempotent.
int tune(const bf16* W, float* ws, hipStream_t stream, const GemmProblem& pb, bool use_u, const char* key, const GemmCand& model, GemmCand* win, bool* cache) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream) (void)hipStreamIsCapturing(stream, &cap);
    if (cap != hipStreamCaptureStatusNone) return GL_OK;   // (the model's choice, not remembered)
    auto run = [&](const GemmCand& c, hipStream_t s) -> int {
        GemmPlan plan{};
        GL_TRY(gemm_plan_tile(pb, use_u, c, plan));
        return execute(plan, pb.A, W, pb.M, pb.N, pb.K, pb.E, ws, s);
    };
    // timing events live on the device that is current for this call (the context's device), for this tuning pass only
    GL_HIP(hipDeviceSynchronize());     // a quiet chip: work another execution context has in flight on its own stream must not share the timed launches
    hipEvent_t ev[2];
    GL_HIP(hipEventCreate(&ev[0]));
    GL_HIP(hipEventCreate(&ev[1]));
    struct EvGuard { hipEvent_t* e; ~EvGuard() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } ev_guard{ev};
    float win_ms = 1e30f;
    // GL_GEMM_TUNE_CORUN=1 (developer, tools/README.md): the candidates are timed as TWO streams running the same launches side by side
    const int tune_reps = gemm_knobs().tune_reps, corun = gemm_knobs().corun;
    hipStream_t s2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    struct CoGuard { hipStream_t& s; hipEvent_t &a, &b; ~CoGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); if (s) (void)hipStreamDestroy(s); } } co_guard{s2, ev_fork, ev_join};
    if (corun) {
        GL_HIP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        GL_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        GL_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    }
    for (const GemmCand& c : gemm_tune_candidates(pb, use_u)) {
        GL_TRY(run(c, stream));  // warm-up (also sets the kernel's LDS attribute outside the timed region)
        GL_HIP(hipEventRecord(ev[0], stream));
        if (corun) {
            GL_HIP(hipEventRecord(ev_fork, stream));
            GL_HIP(hipStreamWaitEvent(s2, ev_fork, 0));
            for (int r = 0; r < tune_reps; ++r) {
                GL_TRY(run(c, stream));
                GL_TRY(run(c, s2));
            }
            GL_HIP(hipEventRecord(ev_join, s2));
            GL_HIP(hipStreamWaitEvent(stream, ev_join, 0));
        } else
            for (int r = 0; r < tune_reps; ++r) GL_TRY(run(c, stream));
        GL_HIP(hipEventRecord(ev[1], stream));
        GL_HIP(hipEventSynchronize(ev[1]));
        float ms = 0.f;
        GL_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        if (ms < win_ms) { win_ms = ms; *win = c; }
    }
    *cache = true;
    if (gemm_knobs().tune_log)
        fprintf(stderr, "[gemm autotune] %s -> %dx%d / %d splits @%d (%.1f us; model said %dx%d / %d) cfg %d %d %d\n", key, kGemmTm[win->c] * 32,
                kGemmTn[win->c] * 32, win->sp, win->grid ? win->grid : 512, win_ms * 1e3f / tune_reps, kGemmTm[model.c] * 32, kGemmTn[model.c] * 32, model.sp,
                win->c, win->sp, win->grid);
    return GL_OK;
}

}  // namespace

int gemm_launch(const AOperand& A, const bf16* W, int M, int N, int K, const Epilogue& E_in, float* ws,
                size_t ws_bytes, hipStream_t stream) {
    t_last.stats_nb = 0;
    Epilogue E = E_in;
    GemmPlan plan;
    GL_TRY(gemm_plan(A, M, N, K, E, ws != nullptr, ws_bytes, plan, [&](auto&&... a) { return tune(W, ws, stream, a...); }));
    t_last = plan;
    t_log[t_log_n % kGemmLogSize] = GemmLogEntry{plan, M, N, K};
    t_log_n = t_log_n == INT_MAX ? kGemmLogSize : t_log_n + 1;   // (the ring position survives the wrap: kGemmLogSize divides 2^31)
    return execute(plan, A, W, M, N, K, E, ws, stream);
}

int gemm_conv8_launch(const AOperand& A_in, const bf16* W, int M, int N, int K, const Epilogue& E_in, float* ws, size_t ws_bytes, int bn, int splits,
                      int grid_cap, hipStream_t stream) {
    t_last.stats_nb = 0;
    AOperand A = A_in;
    A.mode = A_CONV8;
    Epilogue E = E_in;
    GemmPlan plan;
    GL_TRY(gemm_conv8_plan(A, M, N, K, E, ws != nullptr, ws_bytes, bn, splits, grid_cap, plan));
    t_last = plan;
    return execute(plan, A, W, M, N, K, E, ws, stream);
}

int gemm_launch_t(const bf16* Wrows, int Mw, const bf16* X, int Nx, int K, const Epilogue& E, hipStream_t stream) {
    AOperand A;
    aoperand_rows(A, Wrows, K, K);
    return gemm_launch(A, X, Mw, Nx, K, E, nullptr, 0, stream);
}

}  // namespace gl
