// gligen_amd engine -- the CFG + PLMS / DDIM sampling loop and its graph capture (plms.py:65-162)
#include "engine_impl.h"
#include <algorithm>

namespace gl {

// ---------------------------------------------------------------- PLMS sampler (plms.py:65-162)
// HIP-event time of the UNet evaluations of the last sample_plms call (on the engine's stream).
void Engine::sampler_timing(float* avg_ms, float* first_ms, int* n) {
    if (!smp_.ran || smp_.n_evals == 0) throw GlError(GL_ERR_STATE, "no sampling run to report");
    sampler_wait_idle();
    double sum = 0;
    int cnt = 0;
    float first = 0.f;
    for (int i = 0; i < smp_.n_evals; ++i) {
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, smp_.tev[2 * i], smp_.tev[2 * i + 1]));
        if (i == 0) first = ms;
        if (i >= 2 || smp_.n_evals <= 2) { sum += ms; ++cnt; }  // skip the eager warm-up eval and the capture
    }
    *avg_ms = cnt ? (float)(sum / cnt) : 0.f;
    *first_ms = first;
    *n = smp_.n_evals;
}

// The last sampling run has finished. The engine keeps no caller stream handle across calls (a C-API user may have destroyed the
// stream since): every run ends in an engine-owned event, and that is what later calls wait for.
void Engine::sampler_wait_idle() {
    if (smp_.ran && smp_.ev_done) HIPCK(hipEventSynchronize(smp_.ev_done));
}

void Engine::sampler_release_graph() {
    for (int i = 0; i < 2; ++i) {
        if (smp_.exec[i]) (void)hipGraphExecDestroy(smp_.exec[i]);
        if (smp_.graph[i]) (void)hipGraphDestroy(smp_.graph[i]);
        smp_.exec[i] = nullptr;
        smp_.graph[i] = nullptr;
        smp_.warm[i] = false;
    }
}

template <class Step>
void Engine::sampler_run(const SamplerLoopArgs& a, const char* who, hipStream_t caller, Step&& step) {
    if (!unet_.present || !finalized_) throw GlError(GL_ERR_STATE, "unet not finalized");
    // The loop runs on the CALLER's stream -- one stream per execution context: with a second, engine-owned stream per context the
    // lanes of a process are four streams on the chip's few hardware queues, and which lanes overlap depends on the order the streams
    // were first used (gligen_inference.py --repeat got none, bench.py 13 %, same library; tools/dbg_cli2.py). Only the legacy default
    // stream, which cannot be captured into a hipGraph, is replaced by an engine-owned non-blocking stream ordered after / before it
    // with events. GL_SAMPLER_OWN_STREAM=1 (developer A/B): always the engine-owned stream, the round 1-4 behaviour.
    static const bool own_env = dev_env("GL_SAMPLER_OWN_STREAM") && atoi(dev_env("GL_SAMPLER_OWN_STREAM")) != 0;
    const bool own = own_env || caller == nullptr;
    if (own && !smp_.stream) {
        HIPCK(hipStreamCreateWithFlags(&smp_.stream, hipStreamNonBlocking));
        HIPCK(hipEventCreateWithFlags(&smp_.ev_in, hipEventDisableTiming));
        HIPCK(hipEventCreateWithFlags(&smp_.ev_out, hipEventDisableTiming));
    }
    hipStream_t s = own ? smp_.stream : caller;
    if (own) {
        HIPCK(hipEventRecord(smp_.ev_in, caller));
        HIPCK(hipStreamWaitEvent(s, smp_.ev_in, 0));
    }
    if (!smp_.ev_done) HIPCK(hipEventCreateWithFlags(&smp_.ev_done, hipEventDisableTiming));
    // the sampler's buffers (x2, eps_pair, the eps history, the time-embedding row) are per context, not per stream: a run on another
    // caller stream than the last one is ordered behind that run's end
    if (smp_.ran && smp_.run_stream != s) HIPCK(hipStreamWaitEvent(s, smp_.ev_done, 0));
    struct DoneGuard {       // the run's end -- also when it ends in an exception: whatever was issued is what later calls wait for
        Engine* e; hipStream_t s;
        ~DoneGuard() { (void)hipEventRecord(e->smp_.ev_done, s); e->smp_.run_stream = s; e->smp_.ran = true; }
    } done_guard{this, s};
    const gl_unet_config& c = unet_.cfg;
    if (a.n_steps < 1 || !a.timesteps || !a.x) throw GlError(GL_ERR_ARG, fmt("%s: missing schedule or latent", who));
    if (a.mask && (!a.x0 || !a.noise || !a.sqrt_ac || !a.sqrt_1mac)) throw GlError(GL_ERR_ARG, fmt("%s: mask needs x0, noise and q_sample coefficients", who));
    const int maskB = a.mask_B ? a.mask_B : a.B, x0B = a.x0_B ? a.x0_B : a.B, noiseB = a.noise_B ? a.noise_B : a.B;
    if (a.mask && ((maskB != 1 && maskB != a.B) || (x0B != 1 && x0B != a.B) || (noiseB != 1 && noiseB != a.B)))
        throw GlError(GL_ERR_ARG, fmt("%s: mask / x0 / noise batch (%d, %d, %d) must be 1 or the latent batch %d", who, maskB, x0B, noiseB, a.B));
    const bool cfg = a.guidance_scale != 1.f;
    const int Beff = cfg ? 2 * a.B : a.B;
    if (cond_.Beff != Beff) throw GlError(GL_ERR_STATE, fmt("%s: conditioning batch is %d, need %d", who, cond_.Beff, Beff));
    const int Cl = c.in_channels;
    const int64_t n = (int64_t)a.B * Cl * a.h * a.w;
    if (smp_.B != a.B || smp_.h != a.h || smp_.w != a.w || smp_.extra != a.inpaint_extra || smp_.policy_epoch != ff_rows_policy_epoch()) {
        sampler_wait_idle();               // a graph exec still in flight on the PREVIOUS run's stream must not be destroyed
        HIPCK(hipStreamSynchronize(s));
        sampler_release_graph();
        smp_.policy_epoch = ff_rows_policy_epoch();
        if (smp_.B != a.B || smp_.h != a.h || smp_.w != a.w) {
            smp_.x2 = reinterpret_cast<float*>(persist(n * sizeof(float), false));
            smp_.eps_pair = reinterpret_cast<float*>(persist(2 * n * sizeof(float), false));
            for (int i = 0; i < 4; ++i) smp_.hist[i] = reinterpret_cast<float*>(persist(n * sizeof(float), false));
            smp_.x_tmp = reinterpret_cast<float*>(persist(n * sizeof(float), false));
            smp_.t_dev = reinterpret_cast<int64_t*>(persist(2 * a.B * sizeof(int64_t), false));
        }
        smp_.B = a.B; smp_.h = a.h; smp_.w = a.w; smp_.extra = a.inpaint_extra;
    }

    // every evaluation of the run shares one timestep over its samples, and the schedule is known: the time-embedding MLP and the
    // emb_layers GEMM of all steps in one batched pass; an evaluation copies its row (80 KB) instead of launching four tiny GEMM chains
    static const bool emb_table_on = !(dev_env("GL_EMB_TABLE") && atoi(dev_env("GL_EMB_TABLE")) == 0);    // developer A/B: 0 = per-evaluation time MLP
    if (emb_table_on) emb_table_build(a.timesteps, a.n_steps, s);
    int evals = 0;
    auto eval = [&](const float* xin, int64_t t, int row) {
        HIPCK(hipMemcpyAsync(smp_.x2, xin, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (emb_table_on) HIPCK(hipMemcpyAsync(emb_cur_, emb_table_ + (size_t)row * unet_.embcat.N, (size_t)unet_.embcat.N * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (!emb_table_on) CK(fill_i64_launch(smp_.t_dev, t, Beff, s));      // (with the table nothing on the device reads the timestep)
        while ((int)smp_.tev.size() < 2 * (evals + 1)) {
            hipEvent_t e;
            HIPCK(hipEventCreate(&e));
            smp_.tev.push_back(e);
        }
        HIPCK(hipEventRecord(smp_.tev[2 * evals], s));
        const int gi = fuser_off_ ? 1 : 0;
        // A variant is captured only after it has run EAGERLY once on this context with these shapes: that pass commits the arena up to
        // the variant's high-water mark (no hipMemMap inside a capture), tunes GEMM tiles and times the row-local / two-GEMM choice
        if (a.use_graph && evals >= 1 && smp_.warm[gi]) {
            if (!smp_.exec[gi]) {
                HIPCK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
                try {
                    unet_forward(Beff, a.h, a.w, smp_.x2, a.B, smp_.t_dev, a.inpaint_extra, a.B, smp_.eps_pair, s, emb_table_on ? emb_cur_ : nullptr);
                } catch (...) {
                    hipGraph_t g = nullptr;
                    (void)hipStreamEndCapture(s, &g);
                    if (g) (void)hipGraphDestroy(g);
                    throw;
                }
                HIPCK(hipStreamEndCapture(s, &smp_.graph[gi]));
                HIPCK(hipGraphInstantiate(&smp_.exec[gi], smp_.graph[gi], nullptr, nullptr, 0));
            }
            HIPCK(hipGraphLaunch(smp_.exec[gi], s));
        } else if (a.use_graph && smp_.exec[gi]) {
            HIPCK(hipGraphLaunch(smp_.exec[gi], s));
        } else {
            unet_forward(Beff, a.h, a.w, smp_.x2, a.B, smp_.t_dev, a.inpaint_extra, a.B, smp_.eps_pair, s, emb_table_on ? emb_cur_ : nullptr);
            smp_.warm[gi] = true;
        }
        HIPCK(hipEventRecord(smp_.tev[2 * evals + 1], s));
        ++evals;
        smp_.n_evals = evals;
    };

    // restore_first_conv_from_SD (plms.py:88-89): at the first step whose gate scale is 0. With a schedule that step is
    // derived here (a caller-supplied sd_conv_step must agree or be 0); without one the caller names it.
    int sd_step = -1;
    if (a.sd_conv_w && a.sd_conv_b) {
        if (a.fuser_scale) {
            for (int i = 0; i < a.n_steps && sd_step < 0; ++i)
                if (a.fuser_scale[i] == 0.f) sd_step = i;
            if (a.sd_conv_step > 0 && a.sd_conv_step != sd_step)
                throw GlError(GL_ERR_ARG, fmt("%s: sd_conv_step %d is not the first step with fuser_scale 0 (%d)", who, a.sd_conv_step, sd_step));
        } else {
            sd_step = a.sd_conv_step;
            if (sd_step >= a.n_steps) throw GlError(GL_ERR_ARG, fmt("%s: sd_conv_step beyond the last step", who));
        }
    }
    bool restored = false;
    for (int i = 0; i < a.n_steps; ++i) {
        if (a.fuser_scale) set_fuser_scale(a.fuser_scale[i], s);
        if (a.sd_conv_w && a.sd_conv_b && !restored && i == sd_step) {
            restore_first_conv(a.sd_conv_w, a.sd_conv_b, s);
            restored = true;
        }
        if (a.mask)
            CK(inpaint_blend_launch(a.x, a.x0, a.noise + (size_t)i * (n / a.B) * noiseB, a.mask, a.sqrt_ac[i], a.sqrt_1mac[i], a.B, Cl, a.h * a.w,
                                    x0B, noiseB, maskB, s));
        step(i, eval, n, cfg, s);
    }
    if (own) {
        HIPCK(hipEventRecord(smp_.ev_out, s));
        HIPCK(hipStreamWaitEvent(caller, smp_.ev_out, 0));
    }
}

template <class A>
static SamplerLoopArgs loop_args(const A& a) {
    return {a.B, a.h, a.w, a.n_steps, a.timesteps, a.fuser_scale, a.guidance_scale, a.x, a.inpaint_extra, a.mask, a.x0, a.noise,
            a.mask_B, a.x0_B, a.noise_B, a.sqrt_ac, a.sqrt_1mac, a.use_graph, a.sd_conv_w, a.sd_conv_b, a.sd_conv_step};
}

void Engine::sample_plms(const gl_plms_args& a, hipStream_t caller) {
    if (a.n_steps < 1 || !a.timesteps || !a.a_t || !a.a_prev || !a.x) throw GlError(GL_ERR_ARG, "sample_plms: missing schedule or latent");
    sampler_run(loop_args(a), "sample_plms", caller, [&](int i, auto& eval, int64_t n, bool cfg, hipStream_t s) {
        eval(a.x, a.timesteps[i], i);
        PlmsParams P{};
        P.eps_pair = smp_.eps_pair; P.has_uncond = cfg ? 1 : 0; P.guidance = a.guidance_scale;
        P.a_t = a.a_t[i]; P.a_prev = a.a_prev[i]; P.n = n;
        float* slot = smp_.hist[i & 3];
        if (a.ddim) {
            // DDIMSampler.p_sample_ddim, eta = 0 (ddim.py:111-134): same x_prev formula driven by e_t itself
            P.e_t_out = slot; P.c0 = 1.f; P.x = a.x; P.x_out = a.x;
            CK(plms_update_launch(P, s));
        } else if (i == 0) {
            // pseudo improved Euler (plms.py:143-149): x_prev from e_t, evaluate at t_next, average
            P.e_t_out = slot; P.c0 = 1.f; P.x = a.x; P.x_out = smp_.x_tmp;
            CK(plms_update_launch(P, s));
            eval(smp_.x_tmp, a.timesteps[std::min(1, a.n_steps - 1)], std::min(1, a.n_steps - 1));
            P.e_t_out = smp_.hist[1]; P.c0 = 0.5f; P.o1 = slot; P.c1 = 0.5f; P.x = a.x; P.x_out = a.x;
            CK(plms_update_launch(P, s));
        } else {
            P.e_t_out = slot; P.x = a.x; P.x_out = a.x;
            P.o1 = smp_.hist[(i - 1) & 3];
            if (i == 1) { P.c0 = 1.5f; P.c1 = -0.5f; }
            else if (i == 2) { P.o2 = smp_.hist[(i - 2) & 3]; P.c0 = 23.f / 12.f; P.c1 = -16.f / 12.f; P.c2 = 5.f / 12.f; }
            else {
                P.o2 = smp_.hist[(i - 2) & 3]; P.o3 = smp_.hist[(i - 3) & 3];
                P.c0 = 55.f / 24.f; P.c1 = -59.f / 24.f; P.c2 = 37.f / 24.f; P.c3 = -9.f / 24.f;
            }
            CK(plms_update_launch(P, s));
        }
    });
}

// ---------------------------------------------------------------- linear multistep solvers (DPM-Solver++ 1 / 2M, DDIM with eta > 0)
// One evaluation per step, then x <- cx x + c0 D0 + c1 D1 + c2 D2 + cn z with step i's host-computed coefficients; the data
// predictions rotate through smp_.hist. What the coefficients mean is the caller's business (ldm/models/diffusion/dpm_solver.py).
void Engine::sample_solver(const gl_solver_args& a, hipStream_t caller) {
    if (a.n_steps < 1 || !a.timesteps || !a.a_t || !a.x) throw GlError(GL_ERR_ARG, "sample_solver: missing schedule or latent");
    if (!a.cx || !a.c0 || !a.c1) throw GlError(GL_ERR_ARG, "sample_solver: cx, c0 and c1 are required (c2 and cn may be NULL)");
    if ((a.cn != nullptr) != (a.step_noise != nullptr))
        throw GlError(GL_ERR_ARG, fmt("sample_solver: cn is %s and step_noise is %s (the noise term needs both)", a.cn ? "given" : "NULL", a.step_noise ? "given" : "NULL"));
    for (int i = 0; i < a.n_steps; ++i) {
        if (!(a.a_t[i] > 0.f && a.a_t[i] <= 1.f)) throw GlError(GL_ERR_ARG, fmt("sample_solver: a_t[%d] = %g is outside (0, 1]", i, (double)a.a_t[i]));
        if (i < 1 && a.c1[i] != 0.f) throw GlError(GL_ERR_ARG, fmt("sample_solver: c1[%d] = %g, but step %d has no earlier data prediction", i, (double)a.c1[i], i));
        if (i < 2 && a.c2 && a.c2[i] != 0.f) throw GlError(GL_ERR_ARG, fmt("sample_solver: c2[%d] = %g, but step %d has no second earlier data prediction", i, (double)a.c2[i], i));
    }
    sampler_run(loop_args(a), "sample_solver", caller, [&](int i, auto& eval, int64_t n, bool cfg, hipStream_t s) {
        eval(a.x, a.timesteps[i], i);
        SolverParams P{};
        P.eps_pair = smp_.eps_pair; P.has_uncond = cfg ? 1 : 0; P.guidance = a.guidance_scale;
        P.a_t = a.a_t[i]; P.n = n;
        P.x = a.x; P.x_out = a.x; P.d0_out = smp_.hist[i & 3];
        P.cx = a.cx[i]; P.c0 = a.c0[i];
        // a zero coefficient is a term the launch does not load
        const bool h2 = a.c2 && a.c2[i] != 0.f, h1 = h2 || a.c1[i] != 0.f;
        if (h1) { P.d1 = smp_.hist[(i - 1) & 3]; P.c1 = a.c1[i]; }
        if (h2) { P.d2 = smp_.hist[(i - 2) & 3]; P.c2 = a.c2[i]; }
        if (a.cn && a.cn[i] != 0.f) { P.z = a.step_noise + (size_t)i * n; P.cn = a.cn[i]; }
        CK(solver_update_launch(P, s));
    });
}

}  // namespace gl
