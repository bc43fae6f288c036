// Kernel selection of the GEMM / conv launcher (gemm_plan.h): host code only.
#include "gemm_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <mutex>
#include <string>
#include <unordered_map>

namespace gl {

// ---- developer switches: the one place that reads them
static GemmKnobs read_knobs() {
    static const struct { const char* env; int GemmKnobs::*knob; } kInt[] = {
        {"GL_GEMM_VARIANT", &GemmKnobs::variant}, {"GL_GEMM_WIDE", &GemmKnobs::wide}, {"GL_GEMM_WIDE_SPLITS", &GemmKnobs::wide_splits},
        {"GL_CONV_HALO", &GemmKnobs::halo}, {"GL_CONV_HALO_SPLITS", &GemmKnobs::halo_splits}, {"GL_GEMM_XCD_BOXES", &GemmKnobs::xcd_boxes},
        {"GL_WIDE_XCD", &GemmKnobs::wide_xcd}, {"GL_GEMM_AUTOTUNE", &GemmKnobs::autotune}, {"GL_GEMM_TUNE_REPS", &GemmKnobs::tune_reps},
        {"GL_GEMM_TUNE_CORUN", &GemmKnobs::corun}, {"GL_CONV8", &GemmKnobs::conv8}, {"GL_CONV8_BN", &GemmKnobs::conv8_bn},
        {"GL_CONV8_SPLITS", &GemmKnobs::conv8_splits}};
    GemmKnobs k;
    for (const auto& e : kInt)
        if (const char* v = dev_env(e.env)) k.*e.knob = atoi(v);
    k.tune_reps = std::max(1, k.tune_reps);
    k.no_table = dev_env("GL_GEMM_NO_TABLE") != nullptr;
    k.tune_log = dev_env("GL_GEMM_TUNE_LOG") != nullptr;
    return k;
}
GemmKnobs& gemm_knobs() {
    static GemmKnobs k = read_knobs();
    return k;
}
void gemm_set_variant(int v) { gemm_knobs().variant = v < 0 ? read_knobs().variant : v; }   // < 0: back to GL_GEMM_VARIANT / the default
void gemm_set_autotune(int on) { gemm_knobs().autotune = on < 0 ? read_knobs().autotune : on; }
void gemm_force_cfg(int tm, int tn, int splits) { gemm_knobs().force_tm = tm; gemm_knobs().force_tn = tn; gemm_knobs().force_splits = splits; }
void gemm_force_grid(int g) { gemm_knobs().force_grid = g; }
void gemm_force_knobs(int halo_splits, int wide_splits, int wide_xcd, int xcd_boxes, int halo, int wide) {
    GemmKnobs& k = gemm_knobs();
    k.halo_splits = halo_splits; k.wide_splits = wide_splits; k.wide_xcd = wide_xcd; k.xcd_boxes = xcd_boxes; k.halo = halo; k.wide = wide;
}
void gemm_conv8_force_knobs(int on, int bn, int splits) {
    GemmKnobs& k = gemm_knobs();
    k.conv8 = on; k.conv8_bn = bn; k.conv8_splits = splits;
}
void gemm_force_clear() {
    const GemmKnobs d = read_knobs();
    gemm_force_cfg(0, 0, 0);
    gemm_force_grid(0);
    gemm_force_knobs(d.halo_splits, d.wide_splits, d.wide_xcd, d.xcd_boxes, d.halo, d.wide);
    gemm_conv8_force_knobs(d.conv8, d.conv8_bn, d.conv8_splits);
}
static thread_local int t_no_split = 0;
void gemm_set_no_split(int on) { t_no_split = on; }
static thread_local int t_plan_scale = 1;
void gemm_set_plan_batch_scale(int scale) { t_plan_scale = scale > 1 ? scale : 1; }

// GEGLU weight-row packing the current main-loop variant expects (pack_geglu_launch layout argument)
int gemm_geglu_layout() { return gemm_knobs().variant >= 2 ? 1 : 0; }
bool gemm_supports_qkv() { return gemm_knobs().variant == 4; }   // the v5 family (gemm_route: GEMM_U / GEMM_HALO / GEMM_WIDE)

// ---- routing
// v5 addresses both operands through 32-bit buffer offsets: every operand must be < 2 GiB. The rows of the activation tensor: M for
// row operands and for same-size stride-1 convs (M = B Ho Wo), the source pixels for strided / upsampling convs.
static size_t a_rows(const AOperand& A, int M) {
    return A.mode != A_ROWS && A.Ho * A.Wo > 0 ? (size_t)(M / (A.Ho * A.Wo)) * A.Hin * A.Win : (size_t)M;
}
// row tiles of `bm` rows: A_CONV2UP tiles each of its four phases on its own
static int row_tiles(const AOperand& A, int M, int bm) { return A.mode == A_CONV2UP ? 4 * cdiv(M / 4, bm) : cdiv(M, bm); }
static bool fits_buffer_offsets(const AOperand& A, int M, int N, int K) {
    return a_rows(A, M) * (size_t)std::max(A.ld0, A.ld1) * 2 < 0x7fff0000ull && (size_t)N * K * 2 * (A.mode == A_CONV2UP ? 4 : 1) < 0x7fff0000ull;
}

static inline int ilog2_exact(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
}
// The halo kernel's problems: 3x3, stride 1, pad 1, power-of-two images up to 64 wide whose 256-pixel tiles are whole rows of one
// image or whole images, plain row-major epilogue (bias, per-sample bias, residual, SiLU, fp32 slabs for split-K).
static bool halo_eligible(const AOperand& A, int M, int N, int K, const Epilogue& E) {
    if (A.mode != A_CONV3 || A.stride != 1 || A.ups || A.pad_lo != 1 || A.Ho != A.Hin || A.Wo != A.Win) return false;
    const int lgW = ilog2_exact(A.Win), lgH = ilog2_exact(A.Hin);
    if (lgW < 3 || lgW > 6 || lgH < 0 || M % 256) return false;
    const int R = 256 >> lgW, HB = std::min(A.Hin, R);
    if ((R / HB) * (HB + 2) * (A.Win + 2) > 448) return false;
    if (A.C0 % 64 || A.C1 % 64 || (N % 160 && N % 128)) return false;   // whole 160- or 128-wide tiles only
    if (E.mode != EPI_ROWMAJOR || E.remap_in || (E.act != ACT_NONE && E.act != ACT_SILU) || (E.bias2 && E.res)) return false;
    if (E.bias2 && (E.rows_per_b != A.Hin * A.Win)) return false;
    return fits_buffer_offsets(A, M, N, K);
}
// What conv8_kernel (gemm_conv8.hip) can run: 3x3, stride 1, pad 1 on 8 x 8 images, whole 64-channel chunks per source, whole 64- or
// 80-wide column tiles, a row-major epilogue (its unsplit form is epi_finish4, the split form splitk_reduce_kernel: bias, per-sample
// bias, residual, SiLU, bf16 or fp32 out). The mode may be A_CONV3 (a question) or A_CONV8 (a launch).
static bool conv8_kernel_eligible(const AOperand& A, int M, int N, int K, const Epilogue& E) {
    if ((A.mode != A_CONV3 && A.mode != A_CONV8) || A.stride != 1 || A.ups || A.pad_lo != 1 || A.gn) return false;
    if (A.Hin != 8 || A.Win != 8 || A.Ho != 8 || A.Wo != 8 || M <= 0 || M % 64) return false;
    if (A.C0 <= 0 || A.C0 % 64 || A.C1 % 64 || K != 9 * (A.C0 + A.C1) || (N % 64 && N % 80)) return false;
    if (E.mode != EPI_ROWMAJOR || E.remap_in || E.gate || (E.act != ACT_NONE && E.act != ACT_SILU) || E.ln_stats) return false;
    return fits_buffer_offsets(A, M, N, K);
}
// The router's answer (the caller switches A_CONV3 to A_CONV8 on a yes; GL_CONV8=0: never): the kernel's problems with at least ten
// chunks of input channels -- below that the K split that fills the chip leaves a workgroup one or two chunks, all prologue -- and
// what gemm_u_kernel's conv instantiations take otherwise (v5 main loop, no per-sample bias next to a residual, no forced tile)
bool gemm_conv8_supported(const AOperand& A, int M, int N, int K, const Epilogue& E) {
    const GemmKnobs& kn = gemm_knobs();
    if (!kn.conv8 || kn.variant != 4 || kn.force_tm || A.C0 + A.C1 < 640 || N < 128 || (E.bias2 && E.res)) return false;
    if (kn.conv8_bn && (kn.conv8_bn != 64 && kn.conv8_bn != 80)) return false;
    if (kn.conv8_bn && N % kn.conv8_bn) return false;
    return conv8_kernel_eligible(A, M, N, K, E);
}

// The wide kernel's problems: row-major activations, whole 256 x BN tiles, plain / residual / SiLU / GEGLU row-major epilogues.
static bool wide_eligible(const AOperand& A, int M, int N, int K, const Epilogue& E) {
    if (A.mode != A_ROWS || M % 256 || (N % 160 && N % 128)) return false;
    if (A.C1 && A.C0 % 64) return false;
    if (E.mode != EPI_ROWMAJOR || E.remap_in || E.bias2) return false;
    if (E.act == ACT_GEGLU) { if (N % 128 || !E.geglu16 || E.res || E.out_f32) return false; }
    else if (E.act != ACT_NONE && E.act != ACT_SILU) return false;
    return fits_buffer_offsets(A, M, N, K);
}

// The kernel family a (valid) problem goes to. honour_force = false: as if no gemm_force_cfg override were set.
static int gemm_route(const AOperand& A, int M, int N, int K, const Epilogue& E, bool honour_force = true) {
    const GemmKnobs& kn = gemm_knobs();
    if (A.mode == A_CONV8) return GEMM_CONV8;   // (gemm_validate has asked conv8_kernel_eligible)
    // the phase form of the upsample convs exists in gemm_u_kernel only, narrow outputs included (gemm_validate refuses every other family)
    if (A.mode == A_CONV2UP) return kn.variant == 4 && fits_buffer_offsets(A, M, N, K) ? GEMM_U : GEMM_P;
    // gemm_glds_kernel: narrow outputs, and everything under variant 1
    if (kn.variant < 2 || (N < 128 && E.act != ACT_GEGLU)) return GEMM_GLDS;
    // v5's epilogue has no bias2 + residual form, and the per-sample bias only in its conv instantiations
    const bool use_u = kn.variant == 4 && fits_buffer_offsets(A, M, N, K) && !(E.bias2 && (E.res || A.mode == A_ROWS));
    if (!use_u) return GEMM_P;
    const bool forced = honour_force && kn.force_tm;
    // eligible 3x3 convs with M >= 256 * GL_CONV_HALO (default 8; 0 = never) go to the halo kernel: at M = 512 (the 8 x 8 level) its
    // 16 tiles x deep split lose to the 64 x 160 tiles of gemm_u_kernel
    if (kn.halo && !forced && N >= 128 && halo_eligible(A, M, N, K, E) && M >= kn.halo * 256) return GEMM_HALO;
    // The wide kernel takes the GEGLU projections (GL_GEMM_WIDE=1, default): 0.78-0.82x the time of gemm_u_kernel's 128x128 tiles at the
    // 64x64 / 32x32 levels, even below. Everything else it is eligible for is slower there (narrow N: 256-row tiles leave CUs idle or
    // need a K split) or within 4 % (FF-out): GL_GEMM_WIDE=2 sends all of it for A/B runs, 0 none. (profiles/r2_final/wide_kbench.txt)
    if (kn.wide && !forced && (kn.wide >= 2 || E.act == ACT_GEGLU) && wide_eligible(A, M, N, K, E)) return GEMM_WIDE;
    return GEMM_U;
}

// AOperand::gn (GroupNorm-apply + SiLU inside the conv's loader) exists in conv_halo_kernel only, for tiles that lie inside one
// image (H W a multiple of 256: the tile's 256 pixels share one sample's coefficients)
bool gemm_gn_prologue_supported(const AOperand& A, int M, int N, int K, const Epilogue& E) {
    return K % 64 == 0 && gemm_route(A, M, N, K, E) == GEMM_HALO && (A.Hin * A.Win) % 256 == 0;
}

// A_CONV2UP: gemm_u_kernel with the staged row-major epilogue (or fp32 slabs + splitk_reduce_kernel): bias only, bf16 out
bool gemm_upconv_phases_supported(const AOperand& A, int M, int N, int K, const Epilogue& E) {
    if (A.mode != A_CONV2UP || M <= 0 || M != 4 * (M / (4 * A.Hin * A.Win)) * A.Hin * A.Win || A.Ho != 2 * A.Hin || A.Wo != 2 * A.Win) return false;
    if ((A.C0 + A.C1) % 64 || A.C0 % 64 || K != 4 * (A.C0 + A.C1) || N % 8 || A.gn) return false;
    if (E.mode != EPI_ROWMAJOR || E.act != ACT_NONE || E.out_f32 || E.bias2 || E.res || E.gate || E.remap_in || E.stats_out || E.ln_stats) return false;
    return gemm_route(A, M, N, K, E) == GEMM_U;
}

// Can a GEMM with this epilogue consume raw rows + row statistics instead of LayerNorm'ed rows (Epilogue::ln_stats)?
// The head-layout epilogues of gemm_u_kernel and the GEGLU epilogue of gemm_wide_kernel apply them. Looser than the launcher in two
// cases, kept as they are: a gemm_force_cfg override is not looked at (under one the launcher leaves the wide kernel), nor is a
// per-sample bias on a head-layout projection (the launcher sends that to gemm_p_kernel); gemm_plan_tile refuses both launches.
bool gemm_ln_fold_supported(const AOperand& A, int M, int N, int K, const Epilogue& E) {
    if (A.mode != A_ROWS || A.C1 || K % 64) return false;
    if (E.act == ACT_GEGLU) return E.mode == EPI_ROWMAJOR && gemm_route(A, M, N, K, E, false) == GEMM_WIDE;
    if (E.mode != EPI_QKV_HEADS && E.mode != EPI_QK_HEADS) return false;
    Epilogue Eh = E;
    Eh.bias2 = nullptr;
    return gemm_route(A, M, N, K, Eh, false) == GEMM_U;
}

// error code + message as set_error, GL_OK otherwise; fills E.rpb_magic / rpb_shift
static int gemm_validate(const AOperand& A, int M, int N, int K, Epilogue& E) {
    if (E.rows_per_b < 1) return set_error(GL_ERR_ARG, "gemm: rows_per_b=%d", E.rows_per_b);
    {   // divide-free m / rows_per_b for the epilogues (div_rpb)
        E.up_win = A.mode == A_CONV2UP ? A.Win : 0;
        const unsigned d = E.up_win ? (unsigned)E.up_win : (unsigned)E.rows_per_b;   // (A_CONV2UP has no per-sample bias: its epilogue divides by Win)
        int sh = 0;
        while ((1ull << sh) < d) ++sh;
        E.rpb_shift = sh;
        E.rpb_magic = (unsigned)((((1ull << sh) - d) << 32) / d + 1);
    }
    if (M <= 0 || N <= 0 || K <= 0) return set_error(GL_ERR_ARG, "gemm: empty problem M=%d N=%d K=%d", M, N, K);
    if (E.ln_stats && (!E.ln_csum || !E.bias || E.ln_nb < 1 || E.ln_ld < E.ln_nb || !gemm_ln_fold_supported(A, M, N, K, E)))
        return set_error(GL_ERR_UNSUPPORTED, "gemm: folded LayerNorm needs csum + folded bias + statistics, and an epilogue that applies them");
    if (K % 64 != 0) return set_error(GL_ERR_ARG, "gemm: K=%d must be a multiple of 64", K);
    if (N % 4 != 0) return set_error(GL_ERR_ARG, "gemm: N=%d must be a multiple of 4", N);
    if (A.gn && !gemm_gn_prologue_supported(A, M, N, K, E))
        return set_error(GL_ERR_UNSUPPORTED, "gemm: the GroupNorm prologue (AOperand::gn) exists in conv_halo_kernel only (3x3, stride 1, H W %% 256 == 0)");
    if (A.mode == A_CONV2UP) {
        if (!gemm_upconv_phases_supported(A, M, N, K, E))
            return set_error(GL_ERR_UNSUPPORTED, "conv3x3: no phase form of the upsample conv for this launch (gemm_u_kernel, bias-only bf16 epilogue, K = 4 Cin, N %% 8 == 0)");
    } else if (A.mode == A_CONV8) {
        if (!conv8_kernel_eligible(A, M, N, K, E))
            return set_error(GL_ERR_UNSUPPORTED, "conv3x3: A_CONV8 is the 3x3 / stride 1 / pad 1 conv of 8 x 8 images (channels %% 64, N %% 64 or 80, plain row-major epilogue)");
    } else if (A.mode == A_CONV3) {
        if ((A.C0 + A.C1) % 64 != 0 || A.C0 % 64 != 0 || K != 9 * (A.C0 + A.C1))
            return set_error(GL_ERR_ARG, "conv3x3: channels (%d,%d) must be multiples of 64 and K=9*Cin (K=%d)", A.C0, A.C1, K);
    } else {
        if (K != A.C0 + A.C1 || (A.C1 && A.C0 % 64 != 0))
            return set_error(GL_ERR_ARG, "gemm: K=%d does not match operand channels (%d,%d)", K, A.C0, A.C1);
    }
    if (A.mode != A_ROWS && (E.gate || E.remap_in))
        return set_error(GL_ERR_UNSUPPORTED, "conv3x3: the gated residual and the row remap are row-GEMM epilogues");
    if ((E.act == ACT_GELU || E.act == ACT_QUICK_GELU) && (E.res || E.bias2 || A.mode != A_ROWS))
        return set_error(GL_ERR_UNSUPPORTED, "gemm: the GELU / quick-GELU epilogues have no residual / broadcast-bias form");
    if (E.act == ACT_GEGLU && (N % 32 != 0 || E.mode != EPI_ROWMAJOR))
        return set_error(GL_ERR_ARG, "gemm: GEGLU epilogue needs packed N %% 32 == 0 (N=%d)", N);
    if (E.act == ACT_GEGLU && E.geglu16 != gemm_geglu_layout())
        return set_error(GL_ERR_STATE, "gemm: GEGLU weights were packed for a different main-loop variant");
    if (E.mode == EPI_QKV_HEADS) {
        if (A.mode != A_ROWS || A.C1) return set_error(GL_ERR_ARG, "gemm: EPI_QKV_HEADS takes a single row-major activation operand");
        if (!gemm_supports_qkv() || !fits_buffer_offsets(A, M, N, K) || N != 3 * E.C || (2 * E.C) % 128 || !E.vt || !E.q || !E.k || E.T % 64 || M % E.T)
            return set_error(GL_ERR_UNSUPPORTED, "gemm: EPI_QKV_HEADS needs the v5 main loop, N = 3C with 2C %% 128 == 0, tokens per sample %% 64 == 0");
    }
    return GL_OK;
}

// ---- the fixed-tile families
namespace {

struct Cfg { int bm, bn; float speed; };
const Cfg kCfgs[4] = {{128, 128, 1.0f}, {128, 64, 0.8f}, {64, 64, 0.55f}, {128, 32, 0.45f}};

const char* reduce_suffix(int splits) { return splits > 1 ? " + splitk_reduce_kernel" : ""; }
// K split of the 256-row kernels: `want`, else one work item per CU while a split keeps `min_units` K tiles / chunks; returns units per split
int split_units(const GemmProblem& pb, int want, int tiles, int units, int min_units, bool allowed, int& splits) {
    int sp = want;
    if (sp <= 0) {
        sp = 1;
        while (tiles * sp < 200 && units / (sp * 2) >= min_units) sp *= 2;
    }
    sp = std::max(1, std::min(sp, units));
    if (!pb.has_ws || !allowed) sp = 1;
    while (sp > 1 && (size_t)sp * pb.M * pb.N * sizeof(float) > pb.ws_bytes) --sp;
    const int per = cdiv(units, sp);
    splits = cdiv(units, per);
    return per;
}

// ph (here and below): the problem the CHOICES are made for -- pb itself, or pb with gemm_set_plan_batch_scale's row count. Tile and
// K split come from ph, every size of the launch (tiles, items, grid) from pb.
void plan_glds(const GemmProblem& pb, const GemmProblem& ph, GemmPlan& p) {
    const int M = ph.M, N = pb.N;
    // pick the tile: padding efficiency x relative tile speed x chip fill
    int best = 0;
    float best_score = -1.f;
    for (int c = 0; c < 4; ++c) {
        if (c == 3 && N > 32) continue;
        if (c != 3 && N <= 32) continue;
        const Cfg& cf = kCfgs[c];
        double tm = cdiv(M, cf.bm), tn = cdiv(N, cf.bn);
        double pad = ((double)M * N) / (tm * cf.bm * tn * cf.bn);
        double fill = fmin(1.0, tm * tn / 256.0);
        float score = (float)(pad * cf.speed * (0.35 + 0.65 * fill));
        if (score > best_score) { best_score = score; best = c; }
    }
    const Cfg& cf = kCfgs[best];
    snprintf(p.name, sizeof p.name, "gemm_glds_kernel<%dx%d, %d>", cf.bm, cf.bn, pb.A.mode);   // (the split is not named here)
    const int tiles_h = cdiv(M, cf.bm) * cdiv(N, cf.bn), tiles = cdiv(pb.M, cf.bm) * cdiv(N, cf.bn);
    const int nk = pb.K / 64;
    int splits = 1;
    if (pb.has_ws && !t_no_split && tiles_h < 256 && nk >= 8) {
        splits = std::min(std::min(cdiv(512, tiles_h), nk / 4), 16);
        while (splits > 1 && (size_t)splits * M * N * sizeof(float) > pb.ws_bytes) --splits;
    }
    const int kps = cdiv(nk, splits);
    p.splits = cdiv(nk, kps);
    p.tm = cf.bm / 32; p.tn = cf.bn / 32; p.grid = tiles;
    p.work = WorkDesc{cdiv(N, cf.bn), p.splits, kps, tiles, -1, 0, p.splits};
}

void plan_halo(const GemmProblem& pb, const GemmProblem& ph, GemmPlan& p) {
    const AOperand& A = pb.A;
    const int M = pb.M, N = pb.N, tn = N % 160 == 0 ? 5 : 4;
    HaloDesc& hd = p.halo;
    hd.lgW = ilog2_exact(A.Win); hd.lgH = ilog2_exact(A.Hin);
    hd.tiles_n = cdiv(N, tn * 32);
    const int tiles = (M / 256) * hd.tiles_n;
    hd.chunks_per_split = split_units(ph, gemm_knobs().halo_splits, (ph.M / 256) * hd.tiles_n, (A.C0 + A.C1) / 64, 2, true, hd.splits);
    hd.n_items = tiles * hd.splits;
    p.tm = 8; p.tn = tn; p.gn = A.gn != nullptr; p.splits = hd.splits;
    p.grid = std::min(hd.n_items, 256);
    snprintf(p.name, sizeof p.name, "conv_halo_kernel<%d, %d%s>%s", tn, 8, p.gn ? ", gn" : "", reduce_suffix(p.splits));
}

void plan_wide(const GemmProblem& pb, const GemmProblem& ph, GemmPlan& p) {
    const Epilogue& E = pb.E;
    const int M = pb.M, N = pb.N, tn = (E.act != ACT_GEGLU && N % 160 == 0) ? 5 : 4;
    WideDesc& wd = p.wide;
    wd.tiles_n = N / (tn * 32);
    const int tiles = (M / 256) * wd.tiles_n;
    wd.kt_per_split = split_units(ph, gemm_knobs().wide_splits, (ph.M / 256) * wd.tiles_n, pb.K / 64, 4, E.act != ACT_GEGLU, wd.splits);
    wd.n_items = tiles * wd.splits;
    // Item order against the 8 XCD L2s (profiles/r3/wide_ring_kbench.txt, per-problem fabric traffic in profiles/r3_final/).
    // Linear order with tiles_n a multiple of 8 is weight-stationary by accident: XCD x only ever sees the column tiles = x mod 8,
    // an eighth of the weight matrix stays in its L2 and the activations cross the fabric 8 times -- the cheaper side when the
    // weights are the larger operand (32x32 / 16x16 levels: 6.5 / 26 MB of weights against 10 / 5 MB of activations; contiguous
    // ranges measured 7-8 % slower there). At 64x64 (tiles_n = 20, 1.6 MB of weights, 21 MB of activations) linear order sends
    // every stripe to every XCD for nothing: contiguous ranges are 4-5 % faster.
    wd.xcd = gemm_knobs().wide_xcd >= 0 ? gemm_knobs().wide_xcd : (wd.tiles_n % 8 != 0 && wd.n_items >= 512);
    if (wd.n_items < 256 || std::min(wd.n_items, 256) % 8) wd.xcd = 0;
    p.tm = 8; p.tn = tn; p.splits = wd.splits;
    p.grid = std::min(wd.n_items, 256);
    snprintf(p.name, sizeof p.name, "gemm_wide_kernel<%d>%s", tn, reduce_suffix(p.splits));
}

// conv8_kernel: column tile (64 | 80) and K split in whole chunks. One work item per CU and launch: the items of a second round
// would start behind a full first one. In units of one chunk at a 64-wide tile, a launch costs
//   rounds x (chunks per split x BN / 64 + 1 for an item's prologue and store) + (split: 0.5 + 0.25 per slab for the reduce pass)
// and the cheapest (BN, split) is taken: for batch 8 that is four or five chunks per workgroup on 200-240 CUs. Measured choices for
// the benchmark's two shapes (profiles/conv8/) come first; GL_CONV8_BN / GL_CONV8_SPLITS (gemm_conv8_force_knobs) override both.
void plan_conv8_choice(const GemmProblem& ph, int& bn, int& splits) {
    const int N = ph.N, chunks = (ph.A.C0 + ph.A.C1) / 64, groups = cdiv(ph.M, 256);
    const GemmKnobs& kn = gemm_knobs();
    static const struct { int M, N, chunks, bn, sp; } kMeasured[] = {{512, 1280, 20, 64, 5}, {512, 1280, 40, 80, 8}};
    int want_bn = kn.conv8_bn, want_sp = kn.conv8_splits;
    if (!kn.no_table)
        for (const auto& e : kMeasured)
            if (e.M == ph.M && e.N == N && e.chunks == chunks) {
                if (!want_bn && !want_sp) { want_bn = e.bn; want_sp = e.sp; }
            }
    double best = 1e300;
    bn = 0; splits = 1;
    for (int b = 64; b <= 80; b += 16) {
        if (N % b || (want_bn && want_bn != b)) continue;
        const int tiles = groups * (N / b);
        for (int sp = 1; sp <= std::min(chunks, 32); ++sp) {
            const int per = cdiv(chunks, sp);
            if (cdiv(chunks, per) != sp) continue;                 // (not a split count of its own: the same launch as a smaller one)
            if (want_sp && sp != cdiv(chunks, cdiv(chunks, std::min(want_sp, chunks)))) continue;
            if (sp > 1 && (!ph.has_ws || (size_t)sp * ph.M * N * sizeof(float) > ph.ws_bytes)) continue;
            const double t = cdiv(tiles * sp, 256) * (per * b / 64.0 + 1.0) + (sp > 1 ? 0.5 + 0.25 * sp : 0.0);
            if (t < best) { best = t; bn = b; splits = sp; }
        }
    }
    if (!bn) { bn = N % 64 == 0 ? 64 : 80; splits = 1; }   // (a wanted split the workspace cannot hold: unsplit)
}
void plan_conv8_fill(const GemmProblem& pb, int bn, int splits, int grid_cap, GemmPlan& p) {
    const int chunks = (pb.A.C0 + pb.A.C1) / 64;
    Conv8Desc& cd = p.conv8;
    cd.tiles_m = cdiv(pb.M, 256);
    cd.tiles_n = pb.N / bn;
    cd.chunks_per_split = cdiv(chunks, splits);
    cd.splits = cdiv(chunks, cd.chunks_per_split);
    cd.n_items = cd.tiles_m * cd.tiles_n * cd.splits;
    p.family = GEMM_CONV8;
    p.tm = 8; p.tn = bn / 16; p.amode = A_CONV8; p.splits = cd.splits;
    p.grid = std::min(cd.n_items, grid_cap > 0 ? grid_cap : 256);
    snprintf(p.name, sizeof p.name, "conv8_kernel<%d>%s", bn, reduce_suffix(p.splits));
}

}  // namespace

// ---- the p / u family: tile shape + K split for the persistent kernels.
// candidates 0-3: 4 waves on a 2-stage ring, two (or three) workgroups per CU.
// Measured and dropped (twice: round 1 sweeps, round 2 on-device autotune over all 107 problems of the benchmark, 0 wins):
// the same tiles on a 4-stage ring (three K tiles in flight) with ONE workgroup per CU for the <= 256-item problems of the
// 16x16 / 8x8 UNet levels; and (round 1) an 8-wave 256-row tile on a 3-stage ring.
// candidate 4 (round 3): 64 x 64 tiles, 32 KB of LDS, up to four workgroups per CU -- for the M = 2048 / 512 problems of the
// 16x16 / 8x8 levels, whose 128 / 64-row tiles leave each CU one or two K-tile-deep latency chains (v5 kernel only)
const int kGemmTm[kGemmTiles] = {4, 4, 2, 2, 2}, kGemmTn[kGemmTiles] = {5, 4, 5, 4, 2};
static const int kSp[10] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};

// may tile c run with split sp? (normalises sp)
static bool feasible(const GemmProblem& pb, bool use_u, int c, int& sp) {
    const Epilogue& E = pb.E;
    const int tm = kGemmTm[c], tn = kGemmTn[c], nk = pb.K / 64;
    if (c == 4 && !use_u) return false;
    if (E.act == ACT_GEGLU && (tn & 1)) return false;
    if (E.mode == EPI_QKV_HEADS && (sp > 1 || (2 * E.C) % (tn * 32) || (tm == 4 && tn == 5))) return false;   // an item must not straddle the k | v boundary
    if (E.mode == EPI_QK_HEADS && E.ln_stats && (sp > 1 || (tm == 4 && tn == 5))) return false;                   // (same kernel family, no V third)
    if (sp > 1 && (t_no_split || !pb.has_ws || nk / sp < 2 || (size_t)sp * pb.M * pb.N * sizeof(float) > pb.ws_bytes)) return false;
    sp = cdiv(nk, cdiv(nk, sp));
    return true;
}

// The key of the tuned-plan cache; tools/make_tuned_table.py and gemm_tuned.inc carry the same string.
static void tuned_key(const GemmProblem& pb, bool use_u, char* key, size_t n) {
    const AOperand& A = pb.A; const Epilogue& E = pb.E;
    snprintf(key, n, "%d,%d,%d|%d,%d,%d,%d,%d,%d,%d|%d,%d,%d,%d,%d,%d|%d%s", pb.M, pb.N, pb.K, A.mode, A.C0, A.C1, A.stride, A.ups, A.Win,
             A.Hin, E.mode, E.act, E.res != nullptr, E.bias2 != nullptr, E.out_f32, E.gate != nullptr, (int)use_u,
             (E.mode == EPI_QK_HEADS && E.ln_stats) ? "|ln" : t_no_split ? "|ns" : "");   // (q-only projection behind a folded LayerNorm: another kernel family; "|ns": gemm_set_no_split)
}

// developer override (kbench sweeps): exactly this tile / split if it fits the problem
static bool forced_choice(const GemmProblem& pb, bool use_u, GemmCand& out) {
    const GemmKnobs& kn = gemm_knobs();
    const int want = kn.force_splits ? kn.force_splits : 1;   // no split given: unsplit
    // any split count that is its own normal form (nk = 10: 5 = cdiv(10, cdiv(10, 6)) is what the tuner's 6 runs as), not kSp alone
    if (!kn.force_tm || want < 1 || want > kSp[9]) return false;
    for (int c = 0; c < kGemmTiles; ++c) {
        int sp = want;
        if (kGemmTm[c] != kn.force_tm || kGemmTn[c] != kn.force_tn || !feasible(pb, use_u, c, sp) || sp != want) continue;
        out = GemmCand{c, sp, 0};
        return true;
    }
    return false;
}

// Analytic model (the capture-time / tuning-off choice for problems the table does not hold): minimise
//   (items per block) x (K tiles per item x cycles per K tile + fixed per-item cost) + split-K reduce pass
// over the tile shapes {128,64} x {160,128} and a few split counts.
static bool model_choice(const GemmProblem& pb, bool use_u, GemmCand& out) {
    const int M = pb.M, N = pb.N, nk = pb.K / 64;
    double best_t = 1e30;
    out = GemmCand{-1, 1, 0};
    for (int c = 0; c < 4; ++c) {   // (the analytic model was fitted without the 64 x 64 candidate: the autotuner alone may pick it)
        const int bm = kGemmTm[c] * 32, bn = kGemmTn[c] * 32;
        const int tiles = row_tiles(pb.A, M, bm) * cdiv(N, bn);
        for (int si = 0; si < 10; ++si) {
            int sp = kSp[si];
            if (!feasible(pb, use_u, c, sp)) continue;
            const int kps = cdiv(nk, sp);
            const int items = tiles * sp;
            const int per_block = cdiv(items, 512);
            // cycles per K tile of one block with two blocks per CU, fitted to kbench sweeps on MI355X
            double t_kt = 0.15 * bm * bn + 500.0;
            if (items <= 256) t_kt *= 0.75;
            const double t_item = kps * t_kt + (pb.E.act == ACT_GEGLU ? 9000.0 : 6000.0) * (bm * bn / 20480.0);
            double tt = per_block * t_item;
            if (sp > 1) tt += 6000.0 + (double)sp * M * N * 8.0 / 2000.0;  // fp32 slabs out and back + reduce launch
            if (tt < best_t) { best_t = tt; out.c = c; out.sp = sp; }
        }
    }
    return out.c >= 0;
}

// What the on-device tuner times: every feasible tile / split at two workgroups per CU and at the deeper residencies its LDS allows
std::vector<GemmCand> gemm_tune_candidates(const GemmProblem& pb, bool use_u) {
    const int M = pb.M, N = pb.N;
    const bool corun = gemm_knobs().corun;
    std::vector<GemmCand> out;
    for (int c = 0; c < kGemmTiles; ++c) {
        const int tiles = row_tiles(pb.A, M, kGemmTm[c] * 32) * cdiv(N, kGemmTn[c] * 32);
        if (c == 4 && ((size_t)M * N > ((size_t)1 << 23) || N % 64)) continue;   // small problems only (M N <= 8 M outputs: 2048 x 3840, 8192 x 640 ..)
        int last_sp = -1;
        for (int si = 0; si < 10; ++si) {
            int sp = kSp[si];
            if (!feasible(pb, use_u, c, sp) || sp == last_sp) continue;
            last_sp = sp;
            if (sp > 1 && tiles * sp > 4096) continue;      // splitting an already over-subscribed grid never paid
            for (int gi = 0; gi < (corun ? 5 : 3); ++gi) {
                const int grid = gi == 0 ? 0 : gi == 1 ? 768 : gi == 2 ? 1024 : gi == 3 ? 256 : 128;
                if (gi == 1 && (kGemmTm[c] * 32 + kGemmTn[c] * 32 > 192 || tiles * sp <= 512)) continue;  // 3 workgroups/CU need <= 48 KB LDS each
                if (gi == 2 && (kGemmTm[c] * 32 + kGemmTn[c] * 32 > 128 || tiles * sp <= 768)) continue;  // 4 workgroups/CU: the 64 x 64 tile (32 KB)
                if (gi == 3 && tiles * sp <= 256) continue;                                                // (co-run tuning) one workgroup per CU
                if (gi == 4 && tiles * sp <= 128) continue;                                                // (co-run tuning) half the CUs
                out.push_back(GemmCand{c, sp, grid});
            }
        }
    }
    return out;
}

int gemm_plan_tile(const GemmProblem& pb, bool use_u, const GemmCand& cand, GemmPlan& p) {
    const auto& [A, M, N, K, E, has_ws, ws_bytes] = pb;
    const int nk = K / 64;
    if (cand.c < 0 || cand.c >= (use_u ? kGemmTiles : 4)) return set_error(GL_ERR_UNSUPPORTED, "gemm: unknown tile candidate");
    const int tm = kGemmTm[cand.c], tn = kGemmTn[cand.c];
    WorkDesc& wd = p.work;
    wd.tiles_n = cdiv(N, tn * 32);
    wd.kt_per_split = cdiv(nk, cand.sp);
    wd.splits = cdiv(nk, wd.kt_per_split);
    wd.n_items = row_tiles(A, M, tm * 32) * wd.tiles_n * wd.splits;
    wd.box = -1; wd.rm = 0; wd.rz = wd.splits;
    if (use_u && gemm_knobs().xcd_boxes) {
        // fabric-side bytes ~ A_bytes * (#N bands) + W_bytes * (#M bands); only exact partitions (all boxes equal)
        const int tiles_m = row_tiles(A, M, tm * 32), tiles_n = wd.tiles_n;
        const double a_bytes = (double)a_rows(A, M) * (A.C0 + A.C1) * 2, w_bytes = (double)N * K * 2;
        double best = 1e300;
        for (int lgm = 3; lgm >= 0; --lgm)
            for (int lgn = 3 - lgm; lgn >= 0; --lgn) {
                const int lgz = 3 - lgm - lgn;
                if (tiles_m % (1 << lgm) || tiles_n % (1 << lgn) || wd.splits % (1 << lgz)) continue;
                const double cost = a_bytes * (1 << lgn) + w_bytes * (1 << lgm);
                if (cost < best) {
                    best = cost;
                    wd.box = lgm | lgn << 4;
                    wd.rm = tiles_m >> lgm; wd.tiles_n = tiles_n >> lgn; wd.rz = wd.splits >> lgz;
                }
            }
    }
    p.family = use_u ? GEMM_U : GEMM_P;
    p.tm = tm; p.tn = tn; p.amode = A.mode; p.splits = wd.splits;
    // q-only / q,k projections behind a folded LayerNorm run in the QKV instantiations too: these hold the statistics code
    p.qkv = use_u && (E.mode == EPI_QKV_HEADS || (E.mode == EPI_QK_HEADS && E.ln_stats));
    const int cap = cand.grid ? cand.grid : gemm_knobs().force_grid ? gemm_knobs().force_grid : 512;   // workgroups resident per launch: two per CU unless the tuner says otherwise
    p.grid = std::min(wd.n_items, cap);
    // row statistics for a folded LayerNorm downstream: only the staged row-major epilogue of gemm_u_kernel produces them
    // (one partial per row and wave column block of tn * 16 columns)
    p.stats_nb = (E.stats_out && use_u && wd.splits == 1 && A.mode == A_ROWS && E.mode == EPI_ROWMAJOR && !E.out_f32 && E.act != ACT_GEGLU &&
                  E.act != ACT_GELU && E.act != ACT_QUICK_GELU && !(E.res && E.act == ACT_SILU) /* (epilogue_staged does not take that combination) */ &&
                  N % (tn * 16) == 0 && N / (tn * 16) <= E.stats_ld)
                     ? N / (tn * 16) : 0;
    if (E.ln_stats && (!use_u || A.mode != A_ROWS || wd.splits > 1 || (tm == 4 && tn == 5) || (E.mode != EPI_QKV_HEADS && E.mode != EPI_QK_HEADS)))
        return set_error(GL_ERR_UNSUPPORTED, "gemm: the folded-LayerNorm epilogue exists for the head layouts of gemm_u_kernel and the GEGLU form of gemm_wide_kernel");
    // (the 128 x 160 tile is not built for QKV: with the second MFMA form it needs more than 256 registers)
    if (p.qkv && tm == 4 && tn == 5) return set_error(GL_ERR_UNSUPPORTED, "gemm: no 128x160 tile for EPI_QKV_HEADS");
    const char* red = reduce_suffix(p.splits);
    if (use_u && E.mode == EPI_QKV_HEADS) snprintf(p.name, sizeof p.name, "gemm_u_kernel<2, %d, %d, 0, 2, true>%s", tm, tn, red);
    else if (use_u) snprintf(p.name, sizeof p.name, "gemm_u_kernel<2, %d, %d, %d, 2, false>%s", tm, tn, A.mode, red);
    else snprintf(p.name, sizeof p.name, "gemm_p_kernel<%d, %d, %d>%s", tm, tn, A.mode, red);
    return GL_OK;
}

// ---- the tuned-plan cache: the shipped table plus what the on-device tuner found; process-wide, guarded by its mutex (ctypes
// drops the GIL during calls)
static std::unordered_map<std::string, GemmCand> g_tuned;
static std::mutex g_tune_mu;

static bool tuned_lookup(const char* key, bool use_u, GemmCand& out) {   // (caller holds g_tune_mu)
    if (g_tuned.empty() && use_u && !gemm_knobs().no_table) {
        // shipped choices for the problems of the benchmark configurations (generated by tools/make_tuned_table.py from an
        // autotune log taken on MI355X with 10 timed launches per candidate): deterministic kernel selection run to run
        static const struct { const char* key; int c, sp, grid; } kTable[] = {
#include "gemm_tuned.inc"
        };
        for (const auto& e : kTable) g_tuned.emplace(e.key, GemmCand{e.c, e.sp, e.grid});
    }
    const auto it = g_tuned.find(key);
    if (it != g_tuned.end()) out = it->second;
    return it != g_tuned.end();
}

int gemm_plan(const AOperand& A, int M, int N, int K, Epilogue& E, bool has_ws, size_t ws_bytes, GemmPlan& p, const GemmTuner& tuner) {
    GL_TRY(gemm_validate(A, M, N, K, E));
    const GemmProblem pb{A, M, N, K, E, has_ws, ws_bytes};
    // gemm_set_plan_batch_scale: family, tile and K split are those of the same problem with `scale` times the rows (what the tuned
    // table / an earlier tuning pass holds for it, else the model's choice; never timed here: the buffers hold M rows), so a row of
    // the result has the bits it has in the larger launch. Taken only where the larger problem's kernel family runs this one too.
    int Mh = (t_plan_scale > 1 && M <= 0x7fffffff / t_plan_scale) ? M * t_plan_scale : M;
    int family = gemm_route(A, Mh, N, K, E);
    if (Mh != M) {
        const int own = gemm_route(A, M, N, K, E);
        if (family != own && !(family == GEMM_HALO && halo_eligible(A, M, N, K, E)) && !(family == GEMM_WIDE && wide_eligible(A, M, N, K, E))) {
            Mh = M;
            family = own;
        }
    }
    const GemmProblem ph{A, Mh, N, K, E, has_ws, ws_bytes};
    p = GemmPlan{family, 0, 0, A.mode};
    if (p.family == GEMM_GLDS) { plan_glds(pb, ph, p); return GL_OK; }
    if (p.family == GEMM_HALO) { plan_halo(pb, ph, p); return GL_OK; }
    if (p.family == GEMM_WIDE) { plan_wide(pb, ph, p); return GL_OK; }
    if (p.family == GEMM_CONV8) {
        if (!gemm_conv8_supported(A, M, N, K, E)) return set_error(GL_ERR_UNSUPPORTED, "conv3x3: A_CONV8 without gemm_conv8_supported()");
        int bn, splits;
        plan_conv8_choice(ph, bn, splits);
        plan_conv8_fill(pb, bn, splits, gemm_knobs().force_grid, p);
        return GL_OK;
    }
    const bool use_u = p.family == GEMM_U;
    GemmCand pick;
    if (forced_choice(pb, use_u, pick)) return gemm_plan_tile(pb, use_u, pick, p);
    char key[160];
    tuned_key(ph, use_u, key, sizeof key);
    {
        std::lock_guard<std::mutex> lock(g_tune_mu);
        if (!tuned_lookup(key, use_u, pick)) {
            GemmCand model;
            if (!model_choice(ph, use_u, model)) return set_error(GL_ERR_ARG, "gemm: no tile configuration for M=%d N=%d K=%d", M, N, K);
            pick = model;
            if (tuner && gemm_knobs().autotune && Mh == M) {
                // the lock is held across the pass: two threads tuning at once would time each other's launches
                bool cache = false;
                GL_TRY(tuner(pb, use_u, key, model, &pick, &cache));
                if (cache) g_tuned[key] = pick;
            }
        }
    }
    return gemm_plan_tile(pb, use_u, pick, p);
}

int gemm_conv8_plan(const AOperand& A, int M, int N, int K, Epilogue& E, bool has_ws, size_t ws_bytes, int bn, int splits, int grid_cap, GemmPlan& p) {
    if (A.mode != A_CONV8) return set_error(GL_ERR_ARG, "gemm_conv8_plan: the operand is not A_CONV8");
    GL_TRY(gemm_validate(A, M, N, K, E));
    const int chunks = (A.C0 + A.C1) / 64;
    if ((bn != 64 && bn != 80) || N % bn || splits < 1 || splits > chunks || cdiv(chunks, cdiv(chunks, splits)) != splits || grid_cap < 0)
        return set_error(GL_ERR_ARG, "conv8: column tile %d / %d splits of %d chunks / cap %d (tile 64 | 80 dividing N, every part with a chunk, cap >= 0)", bn, splits, chunks, grid_cap);
    if (splits > 1 && (!has_ws || (size_t)splits * M * N * sizeof(float) > ws_bytes))
        return set_error(GL_ERR_ARG, "conv8: %d slabs of %d x %d do not fit the workspace", splits, M, N);
    const GemmProblem pb{A, M, N, K, E, has_ws, ws_bytes};
    p = GemmPlan{GEMM_CONV8, 0, 0, A.mode};
    plan_conv8_fill(pb, bn, splits, grid_cap, p);
    return GL_OK;
}

}  // namespace gl
