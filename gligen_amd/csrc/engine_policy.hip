// gligen_amd engine -- row-local kernel or GEMMs: the on-device kernel-form policy
#include "engine_impl.h"
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>

namespace gl {

// ---------------------------------------------------------------- row-local kernel or two GEMMs: decided by timing
// The row-local kernel (ffn.hip) wins where a launch fills the chip (one 128-row workgroup per CU: M = 32768) on a box whose
// fabric keeps up with its exposed row loads / stores, and loses elsewhere (M = 8192: 68 against 42 us for LayerNorm + two GEMMs;
// 1.65x slower on a slow-fabric box). So the engine does not dispatch on shape: at the first EAGER launch of a
// (feed-forward, chain form, M) it runs both forms on scratch rows with the block's real weights, times them with HIP events on the
// launch stream and keeps the faster for the life of the process (all contexts of a device share the table, so forks agree).
namespace ff_policy {
static std::mutex mu;
struct Entry { int rows; float us_rows, us_gemm; };
static std::map<uint64_t, Entry> table;
static std::atomic<int> mode{-1};          // -1 timed (default), 0 never the row-local kernel, 1 wherever it exists, 2 the static rule
static std::atomic<unsigned> epoch{1};     // bumped when the mode changes: captured graphs of another epoch are dropped
static uint64_t key(int dev, int which, int form, int C, int M) {
    return ((uint64_t)dev << 56) | ((uint64_t)which << 52) | ((uint64_t)form << 48) | ((uint64_t)C << 32) | (uint64_t)(unsigned)M;
}
// the rule for shapes that cannot be timed (first seen inside a stream capture): a launch of at least 7/8 of the chip's CUs
static bool static_rule(int M) { return M / 128 >= 224; }
static int current_mode() {
    static const bool env_once = [] {      // developer switch: GL_FF_POLICY=-1|0|1|2 presets the mode (PMC passes: no timing launches)
        if (const char* e = dev_env("GL_FF_POLICY")) mode.store(atoi(e));
        return true;
    }();
    (void)env_once;
    return mode.load();
}
}  // namespace ff_policy

int ff_rows_policy_set(int mode) {
    if (mode < -1 || mode > 2) return set_error(GL_ERR_ARG, "ff_rows policy %d (expected -1 timed, 0 never, 1 wherever supported, 2 static rule)", mode);
    if (ff_policy::mode.exchange(mode) != mode) ff_policy::epoch.fetch_add(1);
    return GL_OK;
}
unsigned ff_rows_policy_epoch() { return ff_policy::epoch.load(); }

// ---------------------------------------------------------------- the guidance pair's shared prefix (Engine::unet_forward)
namespace cfg_prefix {
static std::atomic<int> on{-1};            // -1: not decided yet (GL_CFG_SHARED_PREFIX, default on)
static int current() {
    int v = on.load();
    if (v < 0) {
        const char* e = dev_env("GL_CFG_SHARED_PREFIX");     // developer A/B: 0 = every layer at the full batch
        const int want = (e && atoi(e) == 0) ? 0 : 1;
        int expect = -1;
        on.compare_exchange_strong(expect, want);
        v = on.load();
    }
    return v;
}
// what the host issued in shared form so far (eager passes and captures, not graph replays): evaluations, row-local projections at the
// prefix batch, row-local projections that read prefix-batch rows through an input period
static std::atomic<long long> count[3];
}  // namespace cfg_prefix
bool cfg_shared_prefix() { return cfg_prefix::current() != 0; }
void cfg_shared_prefix_note(int what) { cfg_prefix::count[what].fetch_add(1); }
int cfg_shared_prefix_set(int on) {
    if (on != 0 && on != 1) return set_error(GL_ERR_ARG, "cfg shared prefix %d (expected 0 or 1)", on);
    if (cfg_prefix::current() != on) {
        cfg_prefix::on.store(on);
        ff_policy::epoch.fetch_add(1);      // captured sampler graphs hold the other form's launches
    }
    return GL_OK;
}
int ff_rows_policy_report(char* buf, size_t cap) {
    if (!buf || !cap) return set_error(GL_ERR_ARG, "ff_rows_policy_report: no buffer");
    std::lock_guard<std::mutex> lk(ff_policy::mu);
    size_t n = (size_t)snprintf(buf, cap, "mode=%d", ff_policy::mode.load());
    for (const auto& kv : ff_policy::table) {
        if (n + 96 + 128 >= cap) break;       // (room for the shared-prefix tail)
        const uint64_t k = kv.first;
        n += (size_t)snprintf(buf + n, cap - n, ";dev%d %s form%d C%d M%d -> %s (rows %.1f us, gemm %.1f us)", (int)(k >> 56),
                              ((k >> 52) & 15) == 1 ? "fuser.ff" : ((k >> 52) & 15) == 2 ? "ff" : ((k >> 52) & 15) == 3 ? "proj_in+attn1.qkv" : "attn1.to_out+fuser.qkv", (int)((k >> 48) & 15), (int)((k >> 32) & 0xffff), (int)(k & 0xffffffffu),
                              kv.second.rows ? "rows" : "gemm", kv.second.us_rows, kv.second.us_gemm);
    }
    if (n + 128 < cap)
        snprintf(buf + n, cap - n, ";cfg_shared_prefix=%d evals=%lld rows_at_prefix=%lld rows_periodic=%lld", cfg_prefix::current(),
                 cfg_prefix::count[0].load(), cfg_prefix::count[1].load(), cfg_prefix::count[2].load());
    return GL_OK;
}

// The decision for `key` (M rows of width C) between the form run(true, z) launches -- the row-local kernel -- and the one run(false, z)
// launches: by mode, else from the table, else (inside a capture) by the static rule, else by timing both. z: four scratch buffers
// of M x C bf16 from the arena, the first n_zero of them zeroed (no kernel on either path is data dependent); the block's real weights.
// name / form: what the GL_FF_POLICY_LOG line calls the pair (form < 0: none).
template <class Run>
bool Engine::timed_form(uint64_t key, int M, int C, int n_zero, const char* name, int form, hipStream_t s, Run&& run) {
    const int mode = ff_policy::current_mode();
    if (mode == 0) return false;
    if (mode == 1) return true;
    if (mode == 2) return ff_policy::static_rule(M);     // deterministic: the same kernel form -- hence the same output bits -- on every box, rank and run
    std::unique_lock<std::mutex> lk(ff_policy::mu);   // held across the timing pass: two contexts timing at once would time each other
    auto it = ff_policy::table.find(key);
    if (it != ff_policy::table.end()) return it->second.rows != 0;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap);
    if (cap != hipStreamCaptureStatusNone) {
        // a shape first met inside a capture cannot be timed: the static rule decides, and the decision is KEPT -- a later eager pass
        // must take the form the captured graph replays (the two forms differ in their last bits)
        const bool rows = ff_policy::static_rule(M);
        ff_policy::table[key] = ff_policy::Entry{rows ? 1 : 0, 0.f, 0.f};
        return rows;
    }

    // ---- time both forms on scratch rows. The device is drained first: another lane's batch in flight on its own stream
    // (gligen_inference.generate_stream starts lanes back to back) would otherwise share the chip with the timed launches and decide the table
    HIPCK(hipDeviceSynchronize());
    // whatever the timed launches throw, the context is left as it was found: arena mark, launch counter, profiling switch
    struct Restore {
        Engine* e; size_t mk; int64_t launches; bool prof;
        ~Restore() { e->arena_.release(mk); e->n_launches = launches; e->profiling_ = prof; }
    } restore{this, arena_.mark(), n_launches, profiling_};
    profiling_ = false;
    bf16* z[4];
    for (bf16*& p : z) p = arena_.get<bf16>((size_t)M * C);
    for (int i = 0; i < n_zero; ++i) HIPCK(hipMemsetAsync(z[i], 0, (size_t)M * C * sizeof(bf16), s));
    auto once = [&](bool rows) {
        const size_t m2 = arena_.mark();
        run(rows, z);
        arena_.release(m2);
    };
    hipEvent_t ev[2];
    HIPCK(hipEventCreate(&ev[0]));
    HIPCK(hipEventCreate(&ev[1]));
    struct EvGuard { hipEvent_t* e; ~EvGuard() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } guard{ev};
    float best[2] = {1e30f, 1e30f};
    constexpr int REPS = 4, ROUNDS = 3;
    for (int form_i = 0; form_i < 2; ++form_i) once(form_i == 1);    // warm-up: GEMM tile tuning, kernel attributes
    for (int r = 0; r < ROUNDS; ++r)
        for (int form_i = 0; form_i < 2; ++form_i) {                // alternate the two forms: a clock ramp hits both
            HIPCK(hipEventRecord(ev[0], s));
            for (int i = 0; i < REPS; ++i) once(form_i == 1);
            HIPCK(hipEventRecord(ev[1], s));
            HIPCK(hipEventSynchronize(ev[1]));
            float ms = 0.f;
            HIPCK(hipEventElapsedTime(&ms, ev[0], ev[1]));
            best[form_i] = std::min(best[form_i], ms * 1e3f / REPS);
        }
    const ff_policy::Entry e{best[1] < best[0] ? 1 : 0, best[1], best[0]};
    ff_policy::table[key] = e;
    static const bool log = dev_env("GL_FF_POLICY_LOG") != nullptr;
    if (log) {
        const std::string f = form < 0 ? "" : fmt(" form %d", form);
        fprintf(stderr, "[ff policy] %s%s C %d M %d: rows %.1f us, gemm %.1f us -> %s\n", name, f.c_str(), C, M, e.us_rows, e.us_gemm, e.rows ? "rows" : "gemm");
    }
    return e.rows != 0;
}

bool Engine::ff_rows_for(const STW& t, int which, int B, int HW, hipStream_t s) {
    if (which == 1 && unet_.cfg.fuser_kind != 0) which = 2;   // (gatedSA2 / gatedCA produce the fuser's rows differently: they follow the block's ff)
    const FFW& f = which == 1 ? t.fff : t.ff;
    const int M = B * HW, C = t.C;
    if (!f.folded || !f.rows_stream || !ff_rows_supported(M, C)) return false;
    const int form = f.chain_stream ? (f.chain_post ? 2 : 1) : 0;
    // z: the attention output, the residual in front, the block's input, the block's output
    return timed_form(ff_policy::key(device_, which, form, C, M), M, C, 3, which == 1 ? "fuser.ff" : "ff", form, s, [&](bool rows, bf16* const* z) {
        RowStats st;
        if (which == 1) {
            bool qd = false;
            bf16* t3z = fuser_ff_tail(t, z[0], z[1], B, HW, rows, s, &st, &qd);
            if (!qd && unet_.cfg.fuser_kind == 0 && t.fff.chain_q_stream) cross_q_gemm(t, t3z, st, B, HW, s);   // (the form that folds to_q in is timed against the form that launches it)
        } else block_ff_tail(t, z[0], z[1], z[2], z[3], B, HW, rows, s);
    });
}

// Row-local projection launch or GEMM + LayerNorm-folded q,k,v^T GEMM for attention `which` (0 = attn1 behind proj_in, 1 = fuser.attn
// behind attn1.to_out) of block t: the same policy as the row-local feed-forward (ff_policy: timed at the first eager launch per
// device and shape, gl_set_ff_rows_policy forces it) -- on a box whose fabric is slow the kernel's exposed row loads / stores lose
// what its fused launch wins (profiles/r6: 54 against 72 us on one box, 57 against 58 in the graph on another).
bool Engine::qkv_rows_for(const STW& t, int which, int B, int HW, int Nk, hipStream_t s) {
    const SelfAttnW& a = which ? t.fa : t.a1;
    const int M = B * HW, C = t.C, d = t.d;
    if (!qkv_rows_ok(a, B, HW, Nk, C, d)) return false;
    if (qkv_rows_ >= 2) return true;
    const LinW& pre = which ? t.a1.out : t.proj_in;
    const int Tf = which ? round_up(Nk, 64) : 0, slot = which ? t.idx + 1 : 0;
    // z: the projection's input, the residual in front, the residual stream behind it, the attention output
    return timed_form(ff_policy::key(device_, 3 + which, 0, C, M), M, C, 2, which ? "attn1.to_out+fuser.qkv" : "proj_in+attn1.qkv", -1, s, [&](bool rows, bf16* const* z) {
        if (rows) {
            qkv_rows_project(a, z[0], B, HW, Nk, C, d, pre, which ? z[1] : nullptr, z[2], nullptr, Tf, slot, s);
        } else {
            RowStats st;
            bf16* mid = linear_rows(z[0], M, pre, ACT_NONE, which ? z[1] : nullptr, nullptr, s, &st);
            const bool f = can_fold(st, M, C, 3 * C, EPI_QKV_HEADS, ACT_NONE, true);
            const bf16* ln = f ? mid : layernorm_plain(mid, B, HW, C, !which, s);
            qkv_project_gemm(a, ln, B, HW, Nk, C, d, s, f ? &st : nullptr, Tf, slot);
        }
        // ... and the attention that reads what was projected: the row-local launch leaves q / k / v^T (and the clocks) in another
        // state than the GEMM does, and the attention behind it was measured 4 us slower in situ -- time the pair, not the projection
        self_attention(a, nullptr, B, HW, HW, Nk, C, d, z[3], s, nullptr, Tf, slot, true);
    });
}

}  // namespace gl
