// Stand-alone driver of the GEMM planner for tests/test_gemm_plan_cpu.py: links gemm_plan.hip only, makes no HIP call.
//   gemm_plan_main <knobs>   with <knobs> one of default | no_table | wide2 | variant1 | variant2 (set through GemmKnobs, autotune off)
// stdin: one problem per line, 41 integers in the order of kFields in the test (pointers as 0 / 1: they are never dereferenced).
// stdout, per problem: rc tm tn splits stats_nb grid box rm rz kt_per_split xcd chunks_per_split gn_supported ln_supported name
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../gligen_amd/csrc/gemm_plan.h"

namespace gl {
int set_error(int code, const char*, ...) { return code; }
}  // namespace gl

using namespace gl;

int main(int argc, char** argv) {
    const char* knobs = argc > 1 ? argv[1] : "default";
    GemmKnobs& kn = gemm_knobs();
    kn = GemmKnobs{};
    kn.autotune = 0;
    if (!strcmp(knobs, "no_table")) kn.no_table = true;
    else if (!strcmp(knobs, "wide2")) kn.wide = 2;
    else if (!strcmp(knobs, "variant1")) kn.variant = 1;
    else if (!strcmp(knobs, "variant2")) kn.variant = 2;
    else if (strcmp(knobs, "default")) { fprintf(stderr, "unknown knob set %s\n", knobs); return 2; }

    static float dummy[4];   // what a non-null pointer of a descriptor points to
    auto ptr = [&](int on) { return on ? (void*)dummy : nullptr; };
    int v[41];
    for (;;) {
        for (int i = 0; i < 41; ++i)
            if (scanf("%d", &v[i]) != 1) return i == 0 ? 0 : 3;
        int i = 0;
        const int M = v[i++], N = v[i++], K = v[i++];
        AOperand A{};
        A.p0 = (const bf16*)dummy;
        A.mode = v[i++]; A.C0 = v[i++]; A.C1 = v[i++]; A.ld0 = v[i++]; A.ld1 = v[i++];
        A.Hin = v[i++]; A.Win = v[i++]; A.Ho = v[i++]; A.Wo = v[i++]; A.stride = v[i++]; A.ups = v[i++]; A.pad_lo = v[i++];
        A.gn = (const float*)ptr(v[i++]);
        Epilogue E{};
        E.out = dummy;
        E.mode = v[i++]; E.act = v[i++]; E.out_f32 = v[i++];
        E.bias = (const float*)ptr(v[i++]); E.bias2 = (const float*)ptr(v[i++]); E.bias2_ld = v[i++]; E.rows_per_b = v[i++];
        E.res = (const bf16*)ptr(v[i++]); E.gate = (const float*)ptr(v[i++]);
        E.q = (bf16*)ptr(v[i++]); E.k = (bf16*)ptr(v[i++]); E.vt = (bf16*)ptr(v[i++]); E.C = v[i++]; E.T = v[i++];
        E.remap_in = v[i++]; E.geglu16 = v[i++];
        E.stats_out = (float2*)ptr(v[i++]); E.stats_ld = v[i++];
        E.ln_stats = (const float2*)ptr(v[i++]); E.ln_nb = v[i++]; E.ln_ld = v[i++]; E.ln_csum = (const float*)ptr(v[i++]);
        const int has_ws = v[i++];
        const size_t ws_bytes = (size_t)v[i++] << 10;   // (KiB in the descriptor)
        gemm_set_no_split(v[i++]);

        const int gn_ok = gemm_gn_prologue_supported(A, M, N, K, E), ln_ok = gemm_ln_fold_supported(A, M, N, K, E);
        GemmPlan p;
        const int rc = gemm_plan(A, M, N, K, E, has_ws != 0, ws_bytes, p);
        if (rc != GL_OK) {
            printf("%d 0 0 0 0 0 0 0 0 0 0 0 %d %d -\n", rc, gn_ok, ln_ok);
            continue;
        }
        const bool tiles = p.family == GEMM_P || p.family == GEMM_U;
        printf("0 %d %d %d %d %d %d %d %d %d %d %d %d %d %s\n", p.tm, p.tn, p.splits, p.stats_nb, p.grid, tiles ? p.work.box : 0,
               tiles ? p.work.rm : 0, tiles ? p.work.rz : 0, p.family == GEMM_HALO ? 0 : p.family == GEMM_WIDE ? p.wide.kt_per_split : p.work.kt_per_split, p.family == GEMM_WIDE ? p.wide.xcd : 0,
               p.family == GEMM_HALO ? p.halo.chunks_per_split : 0, gn_ok, ln_ok, p.name);
    }
}
