/* gligen_amd_solver.h -- the linear multistep solver loop of libgligen_amd.so (DPM-Solver++ 1 / 2M, DDIM with eta > 0) and its update
 * kernel by itself. Conventions as in gligen_amd.h. */
#ifndef GLIGEN_AMD_SOLVER_H
#define GLIGEN_AMD_SOLVER_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One run of a linear multistep solver: one evaluation per step, then
 *     e = the guided noise prediction;  D0 = (x - sqrt(1 - a_t) e) / sqrt(a_t);  x <- cx x + c0 D0 + c1 D1 + c2 D2 + cn z
 * with step i's coefficients, D1 / D2 the data predictions of steps i - 1 / i - 2 and z the step's noise. DPM-Solver++ of order 1
 * (= DDIM with eta 0) and 2M, and DDIM with eta > 0 (reference ldm/models/diffusion/ddim.py:111-134), are such updates; the caller
 * computes the coefficients (ldm/models/diffusion/dpm_solver.py), the library knows none of the solvers. Every field gl_plms_args
 * also has means what it means there. */
typedef struct gl_solver_args {
    unsigned struct_size;        /* = sizeof(gl_solver_args), checked as gl_plms_args' */
    int B, h, w;
    int n_steps;
    const int64_t* timesteps;    /* host [n_steps]: the timestep each evaluation runs at */
    const float* a_t;            /* host [n_steps]: alphas_cumprod at that timestep, in (0, 1] */
    const float* cx;             /* host [n_steps] */
    const float* c0;             /* host [n_steps] */
    const float* c1;             /* host [n_steps]; c1[0] must be 0 (a zero coefficient is a term the step does not read) */
    const float* c2;             /* host [n_steps] or NULL; c2[0] and c2[1] must be 0 */
    const float* cn;             /* host [n_steps] or NULL */
    const float* step_noise;     /* device fp32 [n_steps][B][C][h][w]; required if and only if cn is given */
    const float* fuser_scale;
    float guidance_scale;
    float* x;                    /* device fp32 [B][C][h][w]: x_T in, x_0 out */
    const float* inpaint_extra;
    const float* mask;
    const float* x0;
    const float* noise;
    int mask_B, x0_B, noise_B;
    const float* sqrt_ac;
    const float* sqrt_1mac;
    int use_graph;
    const float* sd_conv_w;
    const float* sd_conv_b;
    int sd_conv_step;
} gl_solver_args;

/* The solver loop on the state gl_sample_plms uses (buffers, captured graphs): a run of one after the other at the same shape replays
 * the graph that exists. gl_sampler_timing reports it as well. A wrong struct_size, a missing array, a coefficient that names a data
 * prediction the step does not have, cn without step_noise (or the reverse) are refused with a message that names the value. */
int gl_sample_solver(gl_ctx* ctx, const gl_solver_args* args, gl_stream s);

/* One launch of the solver loop's update kernel (operator tests): every pointer device fp32; eps_pair [n] or, has_uncond,
 * [cond ; uncond] = [2][n]; d0_out [n] receives D0; d1, d2, z [n] or NULL (d2 needs d1); x_out may be x. */
int gl_op_solver_update(gl_ctx* ctx, const float* eps_pair, int has_uncond, float guidance, float a_t, const float* x, float* x_out,
                        float* d0_out, const float* d1, const float* d2, const float* z, float cx, float c0, float c1, float c2, float cn,
                        int64_t n, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
