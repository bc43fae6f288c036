// Which kernel runs a GEMM / conv, with which tile, K split, resident grid and item order: pure functions of the problem descriptor
// (gemm_plan.hip: no kernel, no HIP call; tests/test_gemm_plan_cpu.py). gemm.hip executes a GemmPlan (through the
// entry function of the kernel unit that holds the plan's family, gemm_impl.h) and times the tuner's candidates.
#pragma once
#include <functional>
#include <vector>

#include "gemm.h"

namespace gl {

// ---- kernel descriptors (the planner fills them, the kernels read them: WorkDesc gemm_u.hip / gemm_basic.hip, HaloDesc gemm_halo.hip,
// WideDesc gemm_wide.hip, Conv8Desc gemm_conv8.hip)
struct WorkDesc {
    int tiles_n;
    int splits;
    int kt_per_split;
    int n_items;
    // XCD partition of the item space. box < 0: contiguous ranges of the linear (tm, tn, z) order. Otherwise the 8 XCDs
    // form a 2^lgm x 2^lgn x 2^lgz grid over (M tiles, N tiles, K splits), box = lgm | lgn << 4, and each owns an
    // rm x tiles_n x rz box (tiles_n = N tiles PER BOX then), so that an activation panel is fetched by 2^lgn L2s and a
    // weight panel by 2^lgm (the K axis duplicates nothing). rz = splits when box < 0.
    int box, rm, rz;
};
struct HaloDesc {
    int tiles_n, splits, chunks_per_split, n_items;
    int lgW, lgH;   // image width / height (powers of two)
};
struct WideDesc {
    int tiles_n, splits, kt_per_split, n_items;
    int xcd;   // 1: every XCD walks a contiguous range of the (tile_m, tile_n) order (see plan_wide)
};
struct Conv8Desc {
    int tiles_n, splits, chunks_per_split, n_items;
    int tiles_m;   // row groups of four samples (the last one may be partly empty)
};

// ---- every developer switch of the GEMM (meanings: tools/README.md), read once through dev_env; the gemm_set_* / gemm_force_*
// functions of gemm.h write into it. Process-wide: set them before launching, not while other threads launch.
struct GemmKnobs {
    int variant = 4;                              // GL_GEMM_VARIANT: 1 = gemm_glds_kernel only, 2 = gemm_p_kernel, 4 = v5 (u + halo + wide)
    int wide = 1, wide_splits = 0;                // GL_GEMM_WIDE (0 never, 1 GEGLU, 2 all eligible), GL_GEMM_WIDE_SPLITS (0 = automatic)
    int halo = 8, halo_splits = 0;                // GL_CONV_HALO (eligible convs with M >= 256 * halo; 0 never), GL_CONV_HALO_SPLITS
    int xcd_boxes = 1, wide_xcd = -1;             // GL_GEMM_XCD_BOXES, GL_WIDE_XCD (-1 = by column-tile count)
    int autotune = 1, tune_reps = 3, corun = 0;   // GL_GEMM_AUTOTUNE / gemm_set_autotune, GL_GEMM_TUNE_REPS, GL_GEMM_TUNE_CORUN
    bool no_table = false, tune_log = false;      // GL_GEMM_NO_TABLE, GL_GEMM_TUNE_LOG (set = on)
    int force_tm = 0, force_tn = 0, force_splits = 0, force_grid = 0;   // gemm_force_cfg / gemm_force_grid (kbench sweeps, gl_gemm_force_plan)
    int conv8 = 1, conv8_bn = 0, conv8_splits = 0;   // GL_CONV8 (0: A_CONV8 is never offered), GL_CONV8_BN (64 | 80; 0 = automatic), GL_CONV8_SPLITS
};
GemmKnobs& gemm_knobs();
// The knobs a test sets through include/gligen_amd_gemm_plans.h that otherwise only the environment reaches; gemm_force_clear puts
// them back to what the environment / the defaults say and drops gemm_force_cfg / gemm_force_grid.
void gemm_force_knobs(int halo_splits, int wide_splits, int wide_xcd, int xcd_boxes, int halo, int wide);
void gemm_force_clear();
// conv8_kernel's own knobs (include/gligen_amd_conv8.h); gemm_force_clear puts them back as well
void gemm_conv8_force_knobs(int on, int bn, int splits);

struct GemmProblem {
    const AOperand& A;
    int M, N, K;
    const Epilogue& E;
    bool has_ws; size_t ws_bytes;   // the split-K workspace the caller passed
};

enum GemmFamily { GEMM_GLDS, GEMM_P, GEMM_U, GEMM_HALO, GEMM_WIDE, GEMM_CONV8 };

// A tile / split / resident-grid choice of the p / u family: index into the candidate tiles, K split, grid cap (0 = 512)
struct GemmCand { int c, sp, grid; };
constexpr int kGemmTiles = 5;
extern const int kGemmTm[kGemmTiles], kGemmTn[kGemmTiles];   // in units of 32 rows / columns

// Everything a launch needs. The instantiation is (family, tm, tn, amode, qkv, gn); tm, tn in units of 32 (halo / wide: tm = 8;
// conv8: tm = 8 and tn in units of 16).
struct GemmPlan {
    int family;
    int tm, tn, amode;
    bool qkv, gn;         // gemm_u_kernel: the head-layout instantiation (QKV = true); conv_halo_kernel: GroupNorm prologue
    int splits;
    int grid;             // workgroups launched (glds: tiles, times `splits` in z)
    union { WorkDesc work; HaloDesc halo; WideDesc wide; Conv8Desc conv8; };
    int stats_nb;         // column blocks of row statistics this launch writes to Epilogue::stats_out (0: none)
    char name[96];
};

// ---- the plan log (gemm.hip): what gemm_launch executed on the calling thread since the last clear, newest kGemmLogSize kept
struct GemmLogEntry { GemmPlan plan; int M, N, K; };
constexpr int kGemmLogSize = 32;
void gemm_plan_log_clear();
int gemm_plan_log(GemmLogEntry* out, int max, int* launches);   // oldest first; returns the entries written, *launches = launches since the clear

// ---- the p / u family, for the tuner: what it times, and the plan of one candidate
std::vector<GemmCand> gemm_tune_candidates(const GemmProblem& pb, bool use_u);
int gemm_plan_tile(const GemmProblem& pb, bool use_u, const GemmCand& cand, GemmPlan& plan);

// The on-device tuner: called under the cache's lock for a problem without a forced or cached choice. *win = model on entry; sets *cache when *win was measured.
using GemmTuner = std::function<int(const GemmProblem& pb, bool use_u, const char* key, const GemmCand& model, GemmCand* win, bool* cache)>;

// gemm_validate -> gemm_route -> forced choice | shipped table and earlier winners | analytic model (| tuner) -> plan.
int gemm_plan(const AOperand& A, int M, int N, int K, Epilogue& E, bool has_ws, size_t ws_bytes, GemmPlan& plan, const GemmTuner& tuner = nullptr);

// conv8_kernel with exactly this column tile (64 | 80), K split and cap on resident workgroups (0: 256) for any problem the KERNEL can
// run (conv8_kernel_eligible: fewer channels than the router asks for included), whatever the router would do with it: the plan of
// gemm_conv8_launch (gemm.h). A split that leaves a part without a chunk, or slabs beyond the workspace, is an error here.
int gemm_conv8_plan(const AOperand& A, int M, int N, int K, Epilogue& E, bool has_ws, size_t ws_bytes, int bn, int splits, int grid_cap, GemmPlan& plan);

}  // namespace gl
