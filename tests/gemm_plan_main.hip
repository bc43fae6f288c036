// Stand-alone driver of the GEMM planner for tests/test_gemm_plan_cpu.py: links gemm_plan.hip only, makes no HIP call.
//   gemm_plan_main <knobs>   with <knobs> one of default | no_table | wide2 | variant1 | variant2 (set through GemmKnobs, autotune off)
// stdin: one problem per line, 41 integers in the order of kFields in the test (pointers as 0 / 1: they are never dereferenced).
// stdout, per problem: rc tm tn splits stats_nb grid box rm rz kt_per_split xcd chunks_per_split gn_supported ln_supported name
//   gemm_plan_main candidates [wide2] [halo<N>]   (GL_GEMM_WIDE=2, GL_CONV_HALO=N; tests/test_gemm_candidates_cpu.py) prints, per problem, every plan a launch of it can be given:
//     PLAN <the line above>                        the default choice (table, else model)
//     TUNE tm tn splits cap / TUNE_CORUN ..        gemm_tune_candidates without / what GL_GEMM_TUNE_CORUN=1 adds (p / u problems)
//     FORCED tm tn splits n_items box rm rz kt     every tile x split 1..32 that gemm_force_cfg is given exactly as asked (the model's
//                                                  search space and the 64 x 64 tile), as planned with the XCD boxes on
//     FIXED halo_splits wide_splits wide_xcd <the line above>   the fixed-tile families under their own knobs
//     END
//   gemm_plan_main rpb   stdin: values of rows_per_b; per value `d rpb_magic rpb_shift`, the divide-free m / d gemm_validate prepares
//                        for the epilogues' div_rpb (tests/test_gemm_epilogues_cpu.py)
//   gemm_plan_main force_clear   the forcing knobs after gemm_force_cfg / gemm_force_grid / gemm_force_knobs, and after gemm_force_clear
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gligen_amd/csrc/gemm_plan.h"

namespace gl {
int set_error(int code, const char*, ...) { return code; }
}  // namespace gl

using namespace gl;

int main(int argc, char** argv) {
    const char* knobs = argc > 1 ? argv[1] : "default";
    const bool list = !strcmp(knobs, "candidates");
    GemmKnobs& kn = gemm_knobs();
    kn = GemmKnobs{};
    kn.autotune = 0;
    if (!strcmp(knobs, "no_table")) kn.no_table = true;
    else if (!strcmp(knobs, "wide2")) kn.wide = 2;
    else if (!strcmp(knobs, "variant1")) kn.variant = 1;
    else if (!strcmp(knobs, "variant2")) kn.variant = 2;
    else if (!strcmp(knobs, "force_clear")) {   // gemm_force_clear puts back what the environment / the defaults say: prints the ten values
        gemm_force_cfg(2, 4, 3);
        gemm_force_grid(7);
        gemm_force_knobs(2, 3, 1, 0, 4, 2);
        printf("%d %d %d %d %d %d %d %d %d %d\n", kn.force_tm, kn.force_tn, kn.force_splits, kn.force_grid, kn.halo_splits, kn.wide_splits, kn.wide_xcd, kn.xcd_boxes, kn.halo, kn.wide);
        gemm_force_clear();
        printf("%d %d %d %d %d %d %d %d %d %d\n", kn.force_tm, kn.force_tn, kn.force_splits, kn.force_grid, kn.halo_splits, kn.wide_splits, kn.wide_xcd, kn.xcd_boxes, kn.halo, kn.wide);
        return 0;
    }
    else if (!strcmp(knobs, "rpb")) {   // stdin: divisors; per divisor `d rpb_magic rpb_shift` as gemm_validate fills them for rows_per_b = d
        for (int d; scanf("%d", &d) == 1;) {
            static float dummy[4];
            AOperand A{};
            A.p0 = (const bf16*)dummy; A.C0 = 64; A.ld0 = 64; A.mode = A_ROWS;
            Epilogue E{};
            E.out = dummy; E.rows_per_b = d;
            GemmPlan p;
            const int rc = gemm_plan(A, 64, 128, 64, E, false, 0, p);
            if (rc != GL_OK) { fprintf(stderr, "rows_per_b = %d: error %d\n", d, rc); return 3; }
            printf("%d %u %d\n", d, E.rpb_magic, E.rpb_shift);
        }
        return 0;
    }
    else if (list) {
        kn.no_table = true;   // (a table entry is one of the candidates)
        for (int i = 2; i < argc; ++i) {
            if (!strcmp(argv[i], "wide2")) kn.wide = 2;
            else if (!strncmp(argv[i], "halo", 4)) kn.halo = atoi(argv[i] + 4);
            else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        }
    }
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
        auto print_plan = [&](int rc) {
            if (rc != GL_OK) {
                printf("%d 0 0 0 0 0 0 0 0 0 0 0 %d %d -\n", rc, gn_ok, ln_ok);
                return;
            }
            const bool tiles = p.family == GEMM_P || p.family == GEMM_U;
            printf("0 %d %d %d %d %d %d %d %d %d %d %d %d %d %s\n", p.tm, p.tn, p.splits, p.stats_nb, p.grid, tiles ? p.work.box : 0,
                   tiles ? p.work.rm : 0, tiles ? p.work.rz : 0, p.family == GEMM_HALO ? 0 : p.family == GEMM_WIDE ? p.wide.kt_per_split : p.work.kt_per_split, p.family == GEMM_WIDE ? p.wide.xcd : 0,
                   p.family == GEMM_HALO ? p.halo.chunks_per_split : 0, gn_ok, ln_ok, p.name);
        };
        if (list) {
            int rc = gemm_plan(A, M, N, K, E, has_ws != 0, ws_bytes, p);
            printf("PLAN ");
            print_plan(rc);
            if (rc == GL_OK) {
                const int family = p.family;
                if (family == GEMM_P || family == GEMM_U) {
                    const GemmProblem pb{A, M, N, K, E, has_ws != 0, ws_bytes};
                    const std::vector<GemmCand> plain = gemm_tune_candidates(pb, family == GEMM_U);
                    kn.corun = 1;
                    const std::vector<GemmCand> co = gemm_tune_candidates(pb, family == GEMM_U);
                    kn.corun = 0;
                    for (const GemmCand& c : plain) printf("TUNE %d %d %d %d\n", kGemmTm[c.c], kGemmTn[c.c], c.sp, c.grid ? c.grid : 512);
                    for (const GemmCand& c : co) {
                        bool seen = false;
                        for (const GemmCand& d : plain) seen |= d.c == c.c && d.sp == c.sp && d.grid == c.grid;
                        if (!seen) printf("TUNE_CORUN %d %d %d %d\n", kGemmTm[c.c], kGemmTn[c.c], c.sp, c.grid ? c.grid : 512);
                    }
                }
                if (family != GEMM_GLDS)
                    for (int c = 0; c < kGemmTiles; ++c)
                        for (int sp = 1; sp <= 32; ++sp) {
                            gemm_force_cfg(kGemmTm[c], kGemmTn[c], sp);
                            GemmPlan f;
                            Epilogue Ef = E;
                            if (gemm_plan(A, M, N, K, Ef, has_ws != 0, ws_bytes, f) == GL_OK && (f.family == GEMM_P || f.family == GEMM_U) &&
                                f.tm == kGemmTm[c] && f.tn == kGemmTn[c] && f.splits == sp)
                                printf("FORCED %d %d %d %d %d %d %d %d\n", f.tm, f.tn, f.splits, f.work.n_items, f.work.box, f.work.rm, f.work.rz, f.work.kt_per_split);
                        }
                gemm_force_cfg(0, 0, 0);
                static const int kHaloSplits[] = {1, 2, 3, 64}, kWideSplits[] = {1, 2, 3, 5};
                for (int hs = 0; hs < (family == GEMM_HALO ? 4 : 0); ++hs) {
                    kn.halo_splits = kHaloSplits[hs];
                    printf("FIXED %d 0 -1 ", kn.halo_splits);
                    print_plan(gemm_plan(A, M, N, K, E, has_ws != 0, ws_bytes, p));
                }
                for (int ws = 0; ws < (family == GEMM_WIDE ? 8 : 0); ++ws) {
                    kn.wide_splits = kWideSplits[ws >> 1]; kn.wide_xcd = ws & 1;
                    printf("FIXED 0 %d %d ", kn.wide_splits, kn.wide_xcd);
                    print_plan(gemm_plan(A, M, N, K, E, has_ws != 0, ws_bytes, p));
                }
                if (family == GEMM_GLDS) { printf("FIXED 0 0 -1 "); print_plan(rc); }
                kn.halo_splits = kn.wide_splits = 0; kn.wide_xcd = -1;
            }
            printf("END\n");
            continue;
        }
        const int rc = gemm_plan(A, M, N, K, E, has_ws != 0, ws_bytes, p);
        print_plan(rc);
    }
}
