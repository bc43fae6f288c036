// kbench — per-shape micro-benchmark of the gligen_amd kernels (developer tool, not shipped in
// the library). Reads the launch inventory written by tools/shapes.py, runs every distinct shape on
// random bf16 data through the same launch functions the engine uses, times it with HIP events on
// the launch stream and prints µs, TFLOP/s / GB/s and the count-weighted total per forward.
//
//   kbench <shapes-file> [reps] [filter]
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "attention.h"
#include "ffn.h"
#include "gemm.h"
#include "misc.h"
#include "norm.h"

using namespace gl;
#ifdef GL_FFN_ABLATE
namespace gl { void ff_rows_set_ablation(int abl); }
#endif

static hipStream_t cur_s = nullptr;  // stream the recorded launch closures enqueue on (switched by the "seq" mode)

#define HC(expr)                                                                          \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            fprintf(stderr, "%s:%d %s -> %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            exit(2);                                                                      \
        }                                                                                 \
    } while (0)
#define GC(expr)                                                          \
    do {                                                                  \
        int _r = (expr);                                                  \
        if (_r != GL_OK) {                                                \
            fprintf(stderr, "%s:%d gl error %d: %s\n", __FILE__, __LINE__, _r, gl::last_error()); \
            exit(3);                                                      \
        }                                                                 \
    } while (0)

__global__ void fill_bf16_kernel(bf16* p, size_t n, uint32_t seed, float scale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t x = (uint32_t)i * 2654435761u + seed;
        x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
        p[i] = (bf16)(((float)(x & 0xffff) / 32768.f - 1.f) * scale);
    }
}
__global__ void fill_f32_kernel(float* p, size_t n, uint32_t seed, float scale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t x = (uint32_t)i * 2654435761u + seed;
        x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
        p[i] = ((float)(x & 0xffff) / 32768.f - 1.f) * scale;
    }
}

__global__ void checksum_kernel(const uint32_t* p, size_t n, unsigned long long* out) {
    unsigned long long acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        acc += (unsigned long long)p[i] * (2 * (i % 1000003) + 1);
    atomicAdd(out, acc);
}
static unsigned long long checksum(const void* p, size_t bytes, hipStream_t s) {
    static unsigned long long* d = nullptr;
    if (!d) HC(hipMalloc(&d, 8));
    HC(hipMemsetAsync(d, 0, 8, s));
    hipLaunchKernelGGL(checksum_kernel, dim3(4096), dim3(256), 0, s, (const uint32_t*)p, bytes / 4, d);
    unsigned long long h = 0;
    HC(hipMemcpyAsync(&h, d, 8, hipMemcpyDeviceToHost, s));
    HC(hipStreamSynchronize(s));
    return h;
}

__global__ void maxdiff_kernel(const bf16* a, const bf16* b, size_t n, unsigned* out) {
    float d = 0.f, m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float x = (float)a[i], y = (float)b[i];
        if (x != x || y != y) { d = 1e30f; continue; }
        d = fmaxf(d, fabsf(x - y));
        m = fmaxf(m, fabsf(y));
    }
    atomicMax(out, __float_as_uint(d));
    atomicMax(out + 1, __float_as_uint(m));
}
static void maxdiff(const bf16* a, const bf16* b, size_t n, hipStream_t s, float* d, float* m) {
    static unsigned* dev = nullptr;
    if (!dev) HC(hipMalloc(&dev, 8));
    HC(hipMemsetAsync(dev, 0, 8, s));
    hipLaunchKernelGGL(maxdiff_kernel, dim3(4096), dim3(256), 0, s, a, b, n, dev);
    unsigned h[2];
    HC(hipMemcpyAsync(h, dev, 8, hipMemcpyDeviceToHost, s));
    HC(hipStreamSynchronize(s));
    memcpy(d, &h[0], 4);
    memcpy(m, &h[1], 4);
}

static bf16* dev_bf16(size_t n, uint32_t seed, float scale = 1.f) {
    bf16* p;
    HC(hipMalloc(&p, n * sizeof(bf16) + 256));
    hipLaunchKernelGGL(fill_bf16_kernel, dim3(2048), dim3(256), 0, 0, p, n, seed, scale);
    return p;
}
static float* dev_f32(size_t n, uint32_t seed, float scale = 1.f) {
    float* p;
    HC(hipMalloc(&p, n * sizeof(float) + 256));
    hipLaunchKernelGGL(fill_f32_kernel, dim3(2048), dim3(256), 0, 0, p, n, seed, scale);
    return p;
}

template <class F>
static float time_us(F&& fn, int reps, hipStream_t s) {
    hipEvent_t e0, e1;
    HC(hipEventCreate(&e0));
    HC(hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) fn();
    HC(hipStreamSynchronize(s));
    HC(hipEventRecord(e0, s));
    for (int i = 0; i < reps; ++i) fn();
    HC(hipEventRecord(e1, s));
    HC(hipEventSynchronize(e1));
    float ms = 0;
    HC(hipEventElapsedTime(&ms, e0, e1));
    HC(hipEventDestroy(e0));
    HC(hipEventDestroy(e1));
    return ms * 1000.f / reps;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: kbench <shapes-file> [reps] [filter]\n");
        return 1;
    }
    const int reps = argc > 2 ? atoi(argv[2]) : 10;
    const char* filter = argc > 3 && strcmp(argv[3], "-") ? argv[3] : nullptr;
    // "check": run every gemm/conv shape with main-loop variant 0 and 1 and require bit-identical outputs
    const bool check = argc > 4 && !strcmp(argv[4], "check");
    // "sweep": time every persistent-kernel tile shape x K split x grid cap per gemm/conv shape, print the best
    const bool sweep = argc > 4 && !strcmp(argv[4], "sweep");
    int n_bad = 0;
    const int kb_batch = getenv("KB_B") ? atoi(getenv("KB_B")) : 8;  // samples behind the gemm rows (head-layout epilogues)
    // "seq": after the per-shape table, enqueue the whole list (count launches per shape, no host sync in between) on one
    // stream, then on two streams concurrently, and print the wall times
    const bool seq = argc > 4 && !strcmp(argv[4], "seq");
    std::vector<std::pair<std::function<void()>, int>> recorded;
    if (const char* kf = getenv("KB_FORCE")) {  // "tm,tn,splits" developer override for every gemm/conv shape it fits
        int a = 0, b = 0, c2 = 0;
        sscanf(kf, "%d,%d,%d", &a, &b, &c2);
        gemm_force_cfg(a, b, c2);
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 1; }
    hipStream_t s;
    HC(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    cur_s = s;

    const size_t ACT = (size_t)320 << 20;  // elements: covers 4*512*512*256 (VAE) and the GEGLU outputs
    bf16* a0 = dev_bf16(ACT, 1);
    bf16* a1 = dev_bf16(ACT, 2);
    bf16* a2 = dev_bf16(ACT, 3);
    bf16* w = dev_bf16((size_t)64 << 20, 4, 0.05f);
    float* bias = dev_f32(1 << 16, 5, 0.1f);
    float* gam = dev_f32(1 << 16, 6, 1.f);
    size_t ws_bytes = (size_t)256 << 20;
    float *ws, *ws2;
    HC(hipMalloc(&ws, ws_bytes));
    HC(hipMalloc(&ws2, ws_bytes));
    float* partial;
    HC(hipMalloc(&partial, 1 << 20));
    const size_t CMP = check ? ACT : 0;  // reference copies of the two output buffers
    bf16 *r1 = nullptr, *r2 = nullptr;
    if (check) {
        HC(hipMalloc(&r1, ACT * 2));
        HC(hipMalloc(&r2, ACT * 2));
    }
    HC(hipDeviceSynchronize());

    double tot_us[5] = {0, 0, 0, 0, 0}, tot_flop[5] = {0, 0, 0, 0, 0};
    const char* cat[5] = {"gemm", "conv", "attn", "gn", "ln"};
    char line[512];
    printf("%-58s %9s %9s %8s %5s\n", "shape", "us", "TF/s|GB/s", "tot_ms", "cnt");
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '#' || strlen(line) < 3) continue;
        if (filter && !strstr(line, filter)) continue;
        char kind[16];
        int v[12] = {0};
        int n = sscanf(line, "%15s %d %d %d %d %d %d %d %d %d %d", kind, v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9);
        (void)n;
        line[strcspn(line, "\n")] = 0;
        float us = 0;
        std::function<void()> relaunch;
        int gM = 0, gN = 0, gK = 0;
        double flop = 0, bytes = 0;
        int count = 1, c = 0;
        if (!strcmp(kind, "gemm")) {
            const int M = v[0], N = v[1], K = v[2], epi = v[3];
            count = v[4]; c = 0;
            flop = 2.0 * M * N * K;
            gM = M; gN = N; gK = K;
            Epilogue E;
            epilogue_defaults(E);
            AOperand A;
            if (epi == 3) {  // transposed launch: rows operand = weights [M][K], other = activations [N][K]
                const int C = M, H = 8, d = C / H, B = kb_batch, T = N / B;
                int dp, dpv;
                GC(attn_dims(d, &dp, &dpv));
                E.mode = EPI_VT_HEADS; E.out = a2; E.H = H; E.d = d; E.DPV = dpv; E.T = T; E.Tpad_k = T;
                relaunch = [=] { GC(gemm_launch_t(w, C, a0, N, K, E, cur_s)); };
                us = time_us(relaunch, reps, s);
            } else {
                aoperand_rows(A, a0, K, K);
                if (epi == 0) {
                    E.out = a2; E.ldo = N; E.bias = bias; E.res = a1; E.ldres = N;
                } else if (epi == 1) {
                    E.act = ACT_GEGLU; E.geglu16 = gemm_geglu_layout(); E.out = a2; E.ldo = N / 2; E.bias = bias;
                } else if (epi == 4) {   // fused q, k, v^T projection (N = 3C)
                    const int H = 8, B = kb_batch, T = M / B;
                    const int C = K, d = C / H;
                    int dp, dpv;
                    GC(attn_dims(d, &dp, &dpv));
                    bf16* vt = a2 + ((size_t)200 << 20);
                    E.mode = EPI_QKV_HEADS; E.q = a1; E.k = a2; E.vt = vt; E.C = C; E.H = H; E.d = d; E.DP = dp; E.DPV = dpv; E.T = T;
                    E.Tpad_q = round_up(T, 128); E.Tpad_k = T;
                } else {
                    const int H = 8, B = kb_batch, T = M / B;
                    const int C = K, d = C / H;
                    int dp, dpv;
                    GC(attn_dims(d, &dp, &dpv));
                    E.mode = EPI_QK_HEADS; E.q = a1; E.k = a2; E.C = C; E.H = H; E.d = d; E.DP = dp; E.T = T;
                    E.Tpad_q = round_up(T, 128); E.Tpad_k = T;
                }
                relaunch = [=] { GC(gemm_launch(A, w, M, N, K, E, cur_s == s ? ws : ws2, ws_bytes, cur_s)); };
                us = time_us(relaunch, reps, s);
            }
        } else if (!strcmp(kind, "ffn")) {
            // row-local feed-forward (ffn.hip) against the two-GEMM form it replaces: ffn M C normalize count
            const int M = v[0], C = v[1], norm = v[2];
            count = v[3]; c = 0;
            flop = 24.0 * M * (double)C * C;
            static float *fw1 = nullptr, *fb1, *fw2, *fb2, *fgate;
            static bf16 *wp1, *w2b, *hid, *xn;
            static float* bp1;
            static void* strm;
            if (!fw1) {
                fw1 = dev_f32((size_t)8 * 320 * 320, 11, 0.05f);
                fb1 = dev_f32(8 * 320, 12, 0.1f);
                fw2 = dev_f32((size_t)320 * 4 * 320, 13, 0.03f);
                fb2 = dev_f32(320, 14, 0.1f);
                fgate = dev_f32(4, 15, 0.7f);
                HC(hipMalloc(&wp1, (size_t)8 * 320 * 320 * 2));
                HC(hipMalloc(&bp1, 8 * 320 * 4));
                HC(hipMalloc(&w2b, (size_t)320 * 4 * 320 * 2));
                HC(hipMalloc(&strm, ff_stream_bytes(320)));
                HC(hipMalloc(&hid, (size_t)65536 * 4 * 320 * 2));
                HC(hipMalloc(&xn, (size_t)65536 * 320 * 2));
            }
            if (!ff_rows_supported(M, C) || M > 65536) { printf("ffn: unsupported %d %d\n", M, C); continue; }
            GC(pack_geglu_launch(fw1, fb1, wp1, bp1, 4 * C, C, gemm_geglu_layout(), s));
            GC(cast_f32_bf16_launch(fw2, w2b, (int64_t)C * 4 * C, s));
            GC(ff_pack_launch(fw1, fb1, fw2, strm, C, s));
            FFRowsParams P{};
            P.x = a0; P.ldx = C; P.normalize = norm; P.eps = 1e-5f; P.stream = strm; P.b2 = fb2; P.res = a1; P.ldres = C; P.gate = fgate;
            P.out = a2; P.ldo = C; P.M = M;
            float2* st = reinterpret_cast<float2*>(partial);
            if (M * 8 <= (1 << 20)) { P.stats_out = st; P.stats_ld = 1; }
            relaunch = [=] { GC(ff_rows_launch(P, C, cur_s)); };
            auto two_gemm = [=] {
                const bf16* in = a0;
                if (norm) {
                    LNParams L{};
                    L.x = a0; L.B = 1; L.N1 = M; L.N2 = 0; L.Tpad = M; L.C = C; L.eps = 1e-5f; L.y = xn;
                    GC(layernorm_launch(L, cur_s));
                    in = xn;
                }
                AOperand A;
                aoperand_rows(A, in, C, C);
                Epilogue E;
                epilogue_defaults(E);
                E.act = ACT_GEGLU; E.geglu16 = gemm_geglu_layout(); E.out = hid; E.ldo = 4 * C; E.bias = bp1;
                GC(gemm_launch(A, wp1, M, 8 * C, C, E, ws, ws_bytes, cur_s));
                AOperand A2;
                aoperand_rows(A2, hid, 4 * C, 4 * C);
                Epilogue E2;
                epilogue_defaults(E2);
                E2.out = r2 ? r2 : a2 + ((size_t)100 << 20); E2.ldo = C; E2.bias = fb2; E2.res = a1; E2.ldres = C; E2.gate = fgate;
                GC(gemm_launch(A2, w2b, M, C, 4 * C, E2, ws, ws_bytes, cur_s));
            };
            const float us_ref = time_us(two_gemm, reps, s);
#ifdef GL_FFN_ABLATE
            {
                static const int abls[] = {1, 2, 4, 8, 16, 24, 32, 3, 6, 7, 25, 31};
                for (int ab : abls) {
                    ff_rows_set_ablation(ab);
                    const float t_ab = time_us(relaunch, reps, s);
                    printf("  ablation %2d: %.1f us\n", ab, t_ab);
                }
                ff_rows_set_ablation(0);
            }
#endif
            us = time_us(relaunch, reps, s);
            {
                const bf16* ref = r2 ? r2 : a2 + ((size_t)100 << 20);
                float d, m;
                maxdiff(a2, ref, (size_t)M * C, s, &d, &m);
                {
                    float d1, m1, d2, m2;
                    maxdiff(a2, a2, (size_t)M * C, s, &d1, &m1);
                    maxdiff(ref, ref, (size_t)M * C, s, &d2, &m2);
                    if (d1 != 0.f || d2 != 0.f) printf("  NaN check: fused %s (max %g), reference %s (max %g)\n", d1 != 0.f ? "HAS NaN" : "clean", m1, d2 != 0.f ? "HAS NaN" : "clean", m2);
                    // first bad row of the fused output
                    if (d1 != 0.f) {
                        std::vector<bf16> hb((size_t)M * C);
                        HC(hipMemcpy(hb.data(), a2, hb.size() * 2, hipMemcpyDeviceToHost));
                        int nbad = 0, first = -1, last = -1;
                        for (int r = 0; r < M; ++r) {
                            bool bad = false;
                            for (int cc = 0; cc < C; ++cc) { float f = (float)hb[(size_t)r * C + cc]; if (f != f) bad = true; }
                            if (bad) { ++nbad; if (first < 0) first = r; last = r; }
                        }
                        printf("  rows with NaN: %d of %d (first %d, last %d)\n", nbad, M, first, last);
                        int hist[32] = {0};
                        for (int r = 0; r < M; ++r) { bool bad = false; for (int cc = 0; cc < C; ++cc) { float f = (float)hb[(size_t)r * C + cc]; if (f != f) bad = true; } if (bad) ++hist[r & 31]; }
                        printf("  NaN rows by row %% 32:"); for (int i = 0; i < 32; ++i) printf(" %d", hist[i]); printf("\n");
                        printf("  NaN columns of row %d:", first); for (int cc = 0; cc < C; ++cc) { float f = (float)hb[(size_t)first * C + cc]; if (f != f) printf(" %d", cc); } printf("\n");
                        int chist[320] = {0}; long tot = 0;
                        for (int r = 0; r < M; ++r) for (int cc = 0; cc < C; ++cc) { float f = (float)hb[(size_t)r * C + cc]; if (f != f) { ++chist[cc]; ++tot; } }
                        printf("  NaN elements total %ld; by column (nonzero):", tot); for (int cc = 0; cc < C; ++cc) if (chist[cc]) printf(" %d:%d", cc, chist[cc]); printf("\n");
                    }
                }
                const bool ok = d <= 0.03f * m + 1e-6f;
                if (!ok) ++n_bad;
                printf("FFN M%d C%d norm%d: fused %.1f us (%.0f TF/s) vs two GEMMs%s %.1f us; maxdiff %g of %g %s\n", M, C, norm, us, flop / us * 1e-6,
                       norm ? " + ln_kernel" : "", us_ref, d, m, ok ? "ok" : "MISMATCH");
            }
        } else if (!strcmp(kind, "ffnc")) {
            // chained row-local kernel (ffn.hip): ffnc M C post count -- leading projection + LayerNorm + feed-forward (+ trailing
            // projection) in one launch against the separate launches it replaces
            const int M = v[0], C = v[1], post = v[2];
            count = v[3]; c = 0;
            flop = (24.0 + 2.0 * (1 + post)) * M * (double)C * C;
            static float *fw1 = nullptr, *fb1, *fw2, *fb2, *fgate, *fpre, *fpost, *fbpre, *fbpost;
            static bf16 *wp1, *w2b, *hid, *xn, *preb, *postb, *tmid, *t3, *mid2;
            static float* bp1;
            static void* strm[2];
            if (!fw1) {
                fw1 = dev_f32((size_t)8 * 320 * 320, 21, 0.05f);
                fb1 = dev_f32(8 * 320, 22, 0.1f);
                fw2 = dev_f32((size_t)320 * 4 * 320, 23, 0.03f);
                fb2 = dev_f32(320, 24, 0.1f);
                fgate = dev_f32(4, 25, 0.7f);
                fpre = dev_f32((size_t)320 * 320, 26, 0.06f);
                fpost = dev_f32((size_t)320 * 320, 27, 0.06f);
                fbpre = dev_f32(320, 28, 0.1f);
                fbpost = dev_f32(320, 29, 0.1f);
                HC(hipMalloc(&wp1, (size_t)8 * 320 * 320 * 2));
                HC(hipMalloc(&bp1, 8 * 320 * 4));
                HC(hipMalloc(&w2b, (size_t)320 * 4 * 320 * 2));
                HC(hipMalloc(&preb, (size_t)320 * 320 * 2));
                HC(hipMalloc(&postb, (size_t)320 * 320 * 2));
                HC(hipMalloc(&strm[0], ff_chain_stream_bytes(320, true, false)));
                HC(hipMalloc(&strm[1], ff_chain_stream_bytes(320, true, true)));
                HC(hipMalloc(&hid, (size_t)65536 * 4 * 320 * 2));
                HC(hipMalloc(&xn, (size_t)65536 * 320 * 2));
                HC(hipMalloc(&tmid, (size_t)65536 * 320 * 2));
                HC(hipMalloc(&t3, (size_t)65536 * 320 * 2));
                HC(hipMalloc(&mid2, (size_t)65536 * 320 * 2));
            }
            if (!ff_rows_supported(M, C) || M > 65536) { printf("ffnc: unsupported %d %d\n", M, C); continue; }
            GC(pack_geglu_launch(fw1, fb1, wp1, bp1, 4 * C, C, gemm_geglu_layout(), s));
            GC(cast_f32_bf16_launch(fw2, w2b, (int64_t)C * 4 * C, s));
            GC(cast_f32_bf16_launch(fpre, preb, (int64_t)C * C, s));
            GC(cast_f32_bf16_launch(fpost, postb, (int64_t)C * C, s));
            GC(ff_chain_pack_launch(fw1, fb1, fw2, fpre, post ? fpost : nullptr, strm[post], C, s));
            bf16* xres = a1 + ((size_t)64 << 20);     // x_in of the trailing projection
            FFRowsParams P{};
            P.x = a0; P.ldx = C; P.normalize = 1; P.eps = 1e-5f; P.stream = strm[post]; P.b2 = fb2; P.gate = fgate; P.out = a2; P.ldo = C; P.M = M;
            P.pre = 1; P.pre_b = fbpre; P.pre_res = a1; P.ld_pre_res = C; P.pre_gate = fgate + 1; P.mid_out = mid2; P.ld_mid = C;
            P.post = post; P.post_b = fbpost; P.post_res = xres; P.ld_post_res = C;
            relaunch = [=] { GC(ff_rows_launch(P, C, cur_s)); };
            bf16* refout = a2 + ((size_t)100 << 20);
            auto separate = [=] {
                {   // t = res + g1 (x Wpre^T + bpre)
                    AOperand A;
                    aoperand_rows(A, a0, C, C);
                    Epilogue E;
                    epilogue_defaults(E);
                    E.out = tmid; E.ldo = C; E.bias = fbpre; E.res = a1; E.ldres = C; E.gate = fgate + 1;
                    GC(gemm_launch(A, preb, M, C, C, E, ws, ws_bytes, cur_s));
                }
                LNParams L{};
                L.x = tmid; L.B = 1; L.N1 = M; L.N2 = 0; L.Tpad = M; L.C = C; L.eps = 1e-5f; L.y = xn;
                GC(layernorm_launch(L, cur_s));
                AOperand A;
                aoperand_rows(A, xn, C, C);
                Epilogue E;
                epilogue_defaults(E);
                E.act = ACT_GEGLU; E.geglu16 = gemm_geglu_layout(); E.out = hid; E.ldo = 4 * C; E.bias = bp1;
                GC(gemm_launch(A, wp1, M, 8 * C, C, E, ws, ws_bytes, cur_s));
                AOperand A2;
                aoperand_rows(A2, hid, 4 * C, 4 * C);
                Epilogue E2;
                epilogue_defaults(E2);
                E2.out = post ? t3 : refout; E2.ldo = C; E2.bias = fb2; E2.res = tmid; E2.ldres = C; E2.gate = fgate;
                GC(gemm_launch(A2, w2b, M, C, 4 * C, E2, ws, ws_bytes, cur_s));
                if (post) {
                    AOperand A3;
                    aoperand_rows(A3, t3, C, C);
                    Epilogue E3;
                    epilogue_defaults(E3);
                    E3.out = refout; E3.ldo = C; E3.bias = fbpost; E3.res = xres; E3.ldres = C;
                    GC(gemm_launch(A3, postb, M, C, C, E3, ws, ws_bytes, cur_s));
                }
            };
            const float us_ref = time_us(separate, reps, s);
            us = time_us(relaunch, reps, s);
            {
                float d, m, d2, m2;
                maxdiff(a2, refout, (size_t)M * C, s, &d, &m);
                d2 = m2 = 0.f;     // (t is no longer written: the feed-forward's residual rides in its accumulator)
                const bool ok = d <= 0.03f * m + 1e-6f;
                if (!ok) ++n_bad;
                printf("FFNC M%d C%d post%d: one launch %.1f us (%.0f TF/s) vs %d separate launches %.1f us; maxdiff out %g of %g, mid %g of %g %s\n", M, C, post, us,
                       flop / us * 1e-6, 4 + post, us_ref, d, m, d2, m2, ok ? "ok" : "MISMATCH");
            }
        } else if (!strcmp(kind, "conv")) {
            const int B = v[0], H = v[1], W = v[2], C0 = v[3], C1 = v[4], Cout = v[5], stride = v[6], ups = v[7];
            count = v[8]; c = 1;
            const int Hup = H << ups, Wup = W << ups;
            const int Ho = stride == 1 ? Hup : (Hup + 2 - 3) / 2 + 1, Wo = stride == 1 ? Wup : (Wup + 2 - 3) / 2 + 1;
            const int M = B * Ho * Wo, K = 9 * (C0 + C1);
            flop = 2.0 * M * Cout * K;
            gM = M; gN = Cout; gK = K;
            AOperand A{};
            A.p0 = a0; A.C0 = C0; A.ld0 = C0; A.p1 = C1 ? a1 : nullptr; A.C1 = C1; A.ld1 = C1;
            A.mode = A_CONV3; A.Hin = H; A.Win = W; A.Ho = Ho; A.Wo = Wo; A.stride = stride; A.ups = ups; A.pad_lo = 1;
            Epilogue E;
            epilogue_defaults(E);
            E.out = a2; E.ldo = Cout; E.bias = bias; E.bias2 = gam; E.bias2_ld = Cout; E.rows_per_b = Ho * Wo;
            if (Cout == 32) { E.mode = EPI_NCHW_F32; E.n_real = 4; E.bias2 = nullptr; }
            relaunch = [=] { GC(gemm_launch(A, w, M, Cout, K, E, cur_s == s ? ws : ws2, ws_bytes, cur_s)); };
            if (stride == 1 && ups == 1 && !C1 && Cout != 32 && (size_t)C0 * Cout <= (size_t)1280 * 1280) {
                // The conv behind a nearest-2x Upsample (reference openaimodel.py:54-82; bias only, as the engine launches it), both forms
                // from one fp32 filter: the shape's own line is the nine-tap loader with the replication as a view, the UPCONV line
                // behind it the four 2x2 phase convs (gemm.h A_CONV2UP); outputs compared
                static float* wf = nullptr;
                static bf16 *w9 = nullptr, *w4 = nullptr;
                if (!wf) {
                    wf = dev_f32((size_t)9 * 1280 * 1280, 31, 0.02f);
                    HC(hipMalloc(&w9, (size_t)9 * 1280 * 1280 * 2));
                    HC(hipMalloc(&w4, (size_t)16 * 1280 * 1280 * 2));
                    HC(hipDeviceSynchronize());
                }
                GC(pack_conv_weight_launch(wf, w9, Cout, C0, 3, 3, Cout, s));
                GC(pack_upconv_phases_launch(wf, w4, Cout, C0, Cout, s));
                E.bias2 = nullptr;
                const bf16* w9c = w9;
                relaunch = [=] { GC(gemm_launch(A, w9c, M, Cout, K, E, cur_s == s ? ws : ws2, ws_bytes, cur_s)); };
                AOperand A4 = A;
                A4.mode = A_CONV2UP; A4.ups = 0;
                Epilogue E4 = E;
                E4.out = a1;
                if (gemm_upconv_phases_supported(A4, M, Cout, 4 * C0, E4)) {
                    const bf16* w4c = w4;
                    auto phases = [=] { GC(gemm_launch(A4, w4c, M, Cout, 4 * C0, E4, cur_s == s ? ws : ws2, ws_bytes, cur_s)); };
                    const float us4 = time_us(phases, reps, s);
                    int ptm, ptn, psp;
                    gemm_last_cfg(&ptm, &ptn, &psp);
                    us = time_us(relaunch, reps, s);
                    float d, m;
                    maxdiff(a2, a1, (size_t)M * Cout, s, &d, &m);
                    const bool ok = d <= 0.02f * m + 1e-6f;
                    if (!ok) ++n_bad;
                    printf("UPCONV %-51s %9.1f %9.1f  phase form %dx%d/%d (nine-tap FLOP rate; %.2fx of the nine-tap %.1f us) maxdiff %g of %g %s\n", line, us4,
                           flop / us4 * 1e-6, ptm * 32, ptn * 32, psp, us4 / us, us, d, m, ok ? "ok" : "MISMATCH");
                } else {
                    us = time_us(relaunch, reps, s);
                }
            } else if (gemm_conv8_supported(A, M, Cout, K, E)) {
                // The 8 x 8 level: the shape's own line is the launcher's choice for A_CONV3 (gemm_u_kernel), the CONV8 line behind it
                // conv8_kernel (gemm.h A_CONV8, what the engine launches) on the same weights, both with their reduce pass; outputs compared
                AOperand A8 = A;
                A8.mode = A_CONV8;
                Epilogue E8 = E;
                if (!C1) E8.out = a1;
                auto conv8 = [=] { GC(gemm_launch(A8, w, M, Cout, K, E8, cur_s == s ? ws : ws2, ws_bytes, cur_s)); };
                const float us8 = time_us(conv8, reps, s);
                int ptm, ptn, psp;
                gemm_last_cfg(&ptm, &ptn, &psp);
                us = time_us(relaunch, reps, s);
                float d = 0.f, m = 0.f;
                if (!C1) maxdiff(a2, a1, (size_t)M * Cout, s, &d, &m);
                const bool ok = d <= 0.02f * m + 1e-6f;
                if (!ok) ++n_bad;
                printf("CONV8  %-51s %9.1f %9.1f  conv8_kernel<%d>/%d (%.2fx of gemm_u_kernel's %.1f us) maxdiff %g of %g %s\n", line, us8, flop / us8 * 1e-6,
                       ptn * 16, psp, us8 / us, us, d, m, ok ? "ok" : "MISMATCH");
            } else {
                us = time_us(relaunch, reps, s);
            }
        } else if (!strcmp(kind, "gnconv")) {
            // GroupNorm32 -> SiLU -> conv3x3 (reference openaimodel.py:212-232): "gnconv B H W C0 C1 Cout count". Two forms on the same
            // buffers: GroupNorm + SiLU as its own pass (stats + apply) in front of the conv, and statistics + coefficients with the
            // apply inside the conv's loader (AOperand::gn); outputs compared bit for bit
            const int B = v[0], H = v[1], W = v[2], C0 = v[3], C1 = v[4], Cout = v[5];
            count = v[6]; c = 1;
            const int M = B * H * W, Cin = C0 + C1, K = 9 * Cin;
            flop = 2.0 * M * Cout * K;
            gM = M; gN = Cout; gK = K;
            bf16* y_norm = a2;                                 // normalised copy of the two-pass form
            bf16* out1 = a2 + ((size_t)96 << 20);
            bf16* out2 = a2 + ((size_t)160 << 20);
            float* coef = partial + (1 << 17);
            GNParams P{};
            P.x0 = a0; P.C0 = C0; P.x1 = C1 ? a1 : nullptr; P.C1 = C1; P.B = B; P.HW = H * W; P.eps = 1e-5f;
            P.gamma = gam; P.beta = bias; P.y = y_norm; P.silu = 1; P.partial = partial; P.coef = coef;
            AOperand A{};
            A.mode = A_CONV3; A.Hin = H; A.Win = W; A.Ho = H; A.Wo = W; A.stride = 1; A.ups = 0; A.pad_lo = 1;
            Epilogue E;
            epilogue_defaults(E);
            E.ldo = Cout; E.bias = bias; E.bias2 = gam; E.bias2_ld = Cout; E.rows_per_b = H * W;
            AOperand A1 = A, A2 = A;
            A1.p0 = y_norm; A1.C0 = Cin; A1.ld0 = Cin;
            A2.p0 = a0; A2.C0 = C0; A2.ld0 = C0; A2.p1 = C1 ? a1 : nullptr; A2.C1 = C1; A2.ld1 = C1; A2.gn = coef;
            Epilogue E1 = E, E2 = E;
            E1.out = out1; E2.out = out2;
            if (!gemm_gn_prologue_supported(A2, M, Cout, K, E2)) { printf("%-58s no GroupNorm prologue for this shape\n", line); continue; }
            auto two_pass = [=] { GC(groupnorm_launch(P, cur_s)); GC(gemm_launch(A1, w, M, Cout, K, E1, cur_s == s ? ws : ws2, ws_bytes, cur_s)); };
            auto gn_only = [=] { GC(groupnorm_launch(P, cur_s)); };
            auto conv_only = [=] { GC(gemm_launch(A1, w, M, Cout, K, E1, cur_s == s ? ws : ws2, ws_bytes, cur_s)); };
            auto coef_only = [=] { GC(groupnorm_coef_launch(P, cur_s)); };
            auto conv_pro = [=] { GC(gemm_launch(A2, w, M, Cout, K, E2, cur_s == s ? ws : ws2, ws_bytes, cur_s)); };
            relaunch = [=] { GC(groupnorm_coef_launch(P, cur_s)); GC(gemm_launch(A2, w, M, Cout, K, E2, cur_s == s ? ws : ws2, ws_bytes, cur_s)); };
            const float us2 = time_us(two_pass, reps, s);
            us = time_us(relaunch, reps, s);
            const float t_gn = time_us(gn_only, reps, s), t_cv = time_us(conv_only, reps, s), t_cf = time_us(coef_only, reps, s), t_cp = time_us(conv_pro, reps, s);
            float d, m;
            maxdiff(out1, out2, (size_t)M * Cout, s, &d, &m);
            // (H W <= 256: the separate pass is gn_small_kernel's (x - mean) rstd gamma + beta, the same value with another rounding)
            const bool exact = H * W > 256;
            const bool ok = exact ? d == 0.f : d <= 0.01f * m;
            if (!ok) ++n_bad;
            printf("GNCONV %-44s two passes %.1f us (gn %.1f + conv %.1f) | prologue %.1f us (stats %.1f + conv %.1f)  maxdiff %g of %g %s\n", line, us2, t_gn, t_cv,
                   us, t_cf, t_cp, d, m, !ok ? "MISMATCH" : d == 0.f ? "bit-equal" : "within a bf16 step");
        } else if (!strcmp(kind, "attn")) {
            const int B = v[0], H = v[1], d = v[2], Nq = v[3], Nk = v[4];
            count = v[5]; c = 2;
            flop = 4.0 * B * H * d * (double)Nq * Nk;
            int dp, dpv;
            GC(attn_dims(d, &dp, &dpv));
            AttnParams P{};
            P.vt_layout = attn_vt_layout(d, Nk, &dpv);
            P.q = a0; P.k = a1; P.vt = a2;
            bf16* o = a2 + ((size_t)200 << 20);
            P.o = o;
            P.H = H; P.d = d; P.Nq = Nq; P.Nk = Nk; P.Tq_pad = round_up(Nq, 128); P.Tk_pad = round_up(Nk, 64);
            P.ldo = H * d; P.o_rows_per_b = Nq;
            P.scale_log2e = 1.4426950408889634f / sqrtf((float)d);
            GC(attn_vt_ones_launch(a2, B * H, d, P.Tk_pad, s, dpv));
            GC(attn_k_init_launch(a1, B * H, d, P.Tk_pad, s));
            relaunch = [=] { GC(attn_launch(P, B, cur_s)); };
            us = time_us(relaunch, reps, s);
        } else if (!strcmp(kind, "gn")) {
            const int B = v[0], HW = v[1], C0 = v[2], C1 = v[3], silu = v[4];
            count = v[5]; c = 3;
            bytes = 2.0 * B * HW * (double)(C0 + C1) * 2;  // algorithmic: read once + write once
            GNParams P{};
            P.x0 = a0; P.C0 = C0; P.x1 = C1 ? a1 : nullptr; P.C1 = C1; P.B = B; P.HW = HW; P.eps = 1e-5f;
            P.gamma = gam; P.beta = bias; P.y = a2; P.silu = silu; P.partial = partial;
            relaunch = [=] { GC(groupnorm_launch(P, cur_s)); };
            us = time_us(relaunch, reps, s);
        } else if (!strcmp(kind, "ln")) {
            const int B = v[0], N1 = v[1], N2 = v[2], Tpad = v[3], C = v[4];
            count = v[5]; c = 4;
            bytes = 2.0 * B * (double)(N1 + N2) * C * 2;
            LNParams P{};
            P.x = a0; P.x2 = N2 ? a1 : nullptr; P.B = B; P.N1 = N1; P.N2 = N2; P.Tpad = Tpad; P.C = C; P.eps = 1e-5f;
            P.gamma = gam; P.beta = bias; P.y = a2;
            relaunch = [=] { GC(layernorm_launch(P, cur_s)); };
            us = time_us(relaunch, reps, s);
        } else {
            continue;
        }
        if (sweep && c <= 1) {
            static const int tms[7] = {4, 4, 2, 2, 8, 8, 2}, tns[7] = {5, 4, 5, 4, 5, 4, 2};
            static const int sps[8] = {1, 2, 3, 4, 6, 8, 12, 16};
            float best = 1e30f;
            int btm = 0, btn = 0, bsp = 0, bgrid = 0;
            std::string all;
            for (int gi = 0; gi < 3; ++gi)
                for (int ci = 0; ci < 7; ++ci)
                    for (int si = 0; si < 8; ++si) {
                        if (c == 0 && v[3] == 1 && (tns[ci] & 1)) continue;
                        if (tms[ci] >= 8 && gi) continue;  // the wide / deep kernels always run one workgroup per CU
                        const int grid = gi == 0 ? 512 : gi == 1 ? 768 : 1024;
                        if (gi == 1 && (tms[ci] >= 8 || tms[ci] * 32 + tns[ci] * 32 > 192)) continue;  // 3 blocks/CU only fit for <= 48 KB of LDS
                        if (gi == 2 && tms[ci] * 32 + tns[ci] * 32 > 128) continue;                     // 4 blocks/CU: the 64 x 64 tile
                        gemm_force_cfg(tms[ci], tns[ci], sps[si]);
                        gemm_force_grid(grid);
                        const int nk = gK / 64;
                        if (sps[si] > 1 && (nk / sps[si] < 2 || (size_t)sps[si] * gM * gN * 4 > ws_bytes)) continue;
                        if (gN < 128 && !(c == 0 && v[3] == 1)) continue;  // small N runs the non-persistent kernel
                        if (c == 0 && v[3] == 3 && sps[si] > 1) continue;       // transposed launch has no split-K workspace
                        int ctm2, ctn2, csp2;
                        relaunch();
                        gemm_last_cfg(&ctm2, &ctn2, &csp2);
                        if (csp2 != sps[si] || ctm2 != (tms[ci] > 8 ? tms[ci] - 8 : tms[ci]) || ctn2 != tns[ci]) continue;  // rounded split / override did not fit
                        float tus = time_us(relaunch, 5, s);
                        char buf[64];
                        snprintf(buf, sizeof buf, " %s%dx%d/%d@%d=%.1f", tms[ci] > 8 ? "D" : "", ctm2 * 32, tns[ci] * 32, csp2, grid, tus);
                        all += buf;
                        if (tus < best) { best = tus; btm = tms[ci]; btn = tns[ci]; bsp = csp2; bgrid = grid; }
                    }
            gemm_force_cfg(0, 0, 0);
            gemm_force_grid(0);
            if (best < 1e29f)
                printf("SWEEP %-52s auto %.1f us | best %.1f us %dx%d/%d@%d\n", line, us, best, btm * 32, btn * 32, bsp, bgrid);
            printf("      %s\n", all.c_str());
        }
        if (check && c <= 1 && !(c == 0 && (v[3] == 1 || v[3] == 4))) {   // (GEGLU packing and the fused QKV launch exist only in the selected variant)
            // the selected variant (persistent 16x16-tile kernels) against variant 1 (LDS-DMA 32x32-tile kernel): different
            // accumulation order, so compare with a tolerance of a few bf16 ulps of the largest output
            gemm_set_variant(1);
            relaunch();
            HC(hipMemcpyAsync(r1, a1, CMP * 2, hipMemcpyDeviceToDevice, s));
            HC(hipMemcpyAsync(r2, a2, CMP * 2, hipMemcpyDeviceToDevice, s));
            gemm_set_variant(-1);  // back to GL_GEMM_VARIANT / the default
            relaunch();
            float d1, m1, d2, m2;
            maxdiff(a1, r1, CMP, s, &d1, &m1);
            maxdiff(a2, r2, CMP, s, &d2, &m2);
            const bool ok = d1 <= 0.02f * m1 + 1e-6f && d2 <= 0.02f * m2 + 1e-6f;
            if (!ok) { ++n_bad; printf("MISMATCH v1 vs selected: %s  (maxdiff %g of %g ; %g of %g)\n", line, d1, m1, d2, m2); }
        }
        const double rate = flop > 0 ? flop / us * 1e-6 : bytes / us * 1e-3;
        int ctm = 0, ctn = 0, csp = 0;
        if (c <= 1) gemm_last_cfg(&ctm, &ctn, &csp);
        printf("%-58s %9.1f %9.1f %8.3f %5d  %dx%d/%d\n", line, us, rate, us * count * 1e-3, count, ctm * 32, ctn * 32, csp);
        if (seq && relaunch) recorded.emplace_back(relaunch, count);
        tot_us[c] += (double)us * count;
        tot_flop[c] += flop * count;
    }
    double all = 0, allf = 0;
    for (int i = 0; i < 5; ++i) {
        printf("TOTAL %-5s %9.3f ms", cat[i], tot_us[i] * 1e-3);
        if (tot_flop[i] > 0) printf("  %8.1f TF/s", tot_flop[i] / tot_us[i] * 1e-6);
        printf("\n");
        all += tot_us[i];
        allf += tot_flop[i];
    }
    if (seq) {
        hipStream_t s1;
        HC(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking));
        hipEvent_t e0, e1, e2;
        HC(hipEventCreate(&e0)); HC(hipEventCreate(&e1)); HC(hipEventCreate(&e2));
        auto enqueue_all = [&](hipStream_t st, size_t start = 0) {  // start: rotate the list so two streams are out of phase
            cur_s = st;
            for (size_t k = 0; k < recorded.size(); ++k) {
                auto& rc = recorded[(k + start) % recorded.size()];
                for (int i = 0; i < rc.second; ++i) rc.first();
            }
        };
        for (int rep = 0; rep < 3; ++rep) {
            HC(hipDeviceSynchronize());
            HC(hipEventRecord(e0, s));
            enqueue_all(s);
            HC(hipEventRecord(e1, s));
            HC(hipEventSynchronize(e1));
            float one = 0, two = 0;
            HC(hipEventElapsedTime(&one, e0, e1));
            HC(hipDeviceSynchronize());
            auto t0 = std::chrono::steady_clock::now();
            enqueue_all(s);
            enqueue_all(s1, recorded.size() / 3);
            HC(hipStreamSynchronize(s));
            HC(hipStreamSynchronize(s1));
            two = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            HC(hipDeviceSynchronize());
            t0 = std::chrono::steady_clock::now();
            enqueue_all(s);
            enqueue_all(s);
            HC(hipStreamSynchronize(s));
            const float twice = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            printf("SEQ one pass on one stream %.3f ms | two passes back to back %.3f ms | two passes on two streams %.3f ms\n", one, twice, two);
        }
        cur_s = s;
    }
    if (check) printf("CHECK v1~selected: %s (%d mismatching shapes)\n", n_bad ? "FAILED" : "ok", n_bad);
    printf("TOTAL all   %9.3f ms  %8.1f TF/s (sum of isolated kernels, back-to-back launches of each shape)\n", all * 1e-3,
           allf / all * 1e-6);
    return n_bad ? 4 : 0;
}
