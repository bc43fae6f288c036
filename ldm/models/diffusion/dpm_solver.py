"""DPM-Solver++ (2M) sampler with classifier-free guidance: the multistep data-prediction solver of Lu et al. 2022
(arXiv:2211.01095), 20-25 model evaluations where PLMS takes 51. Same constructor and in-place `input` semantics as
PLMSSampler / DDIMSampler.

Notation: abar = alphas_cumprod, alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log(alpha / sigma). A step goes from s (a_t) to
t (a_prev), h = lambda_t - lambda_s, and with D0 = (x - sigma_s e) / alpha_s the model's data prediction at s:

    order 1:   x_t = (sigma_t / sigma_s) x - alpha_t (e^{-h} - 1) D0                         (algebraically DDIM with eta = 0)
    order 2:   the same with D = (1 + 1/(2r)) D0 - (1/(2r)) D1,  r = (lambda_s - lambda_{s_prev}) / h,  D1 the previous step's D0

Step 0 is order 1; with lower_order_final and fewer than 10 steps so is the last one. Every such update is linear in (x, D0, D1), so
the device loop (Engine::sample_solver) is one hipGraph-replayed [cond ; uncond] evaluation per step plus one fused kernel that gets
step i's three numbers; dpm_solver_coefficients computes them here in float64. Any other `model` callable goes through
`_sample_generic`, the same loop on the host.

Two grids: "uniform" is make_ddim_timesteps' grid (what PLMS and DDIM use), "logsnr" the integer timesteps nearest to a grid uniform
in lambda, on which a second-order solver actually converges at second order (DESIGN.md §4 has the toy-problem figures).
"""
import numpy as np
import torch

from ldm.models.diffusion.plms import PLMSSampler, _np


def _lambda(abar):
    abar = np.asarray(abar, dtype=np.float64)
    return 0.5 * (np.log(abar) - np.log1p(-abar))


def dpm_solver_coefficients(a_t, a_prev, order=2, lower_order_final=True):
    """float64 [S, 3] = (cx, c0, c1) with x_prev = cx x + c0 D0 + c1 D1 for the steps a_t[i] -> a_prev[i] (alphas_cumprod at the
    evaluation and at its target, in sampling order). A pure function of the two arrays."""
    if order not in (1, 2):
        raise ValueError(f"DPM-Solver++: order {order!r} is not implemented (1 or 2)")
    a_t, a_prev = np.asarray(a_t, dtype=np.float64), np.asarray(a_prev, dtype=np.float64)
    if a_t.ndim != 1 or a_t.shape != a_prev.shape or len(a_t) < 1:
        raise ValueError(f"DPM-Solver++: a_t {a_t.shape} and a_prev {a_prev.shape} must be two equally long vectors")
    S = len(a_t)
    lam_s, lam_t = _lambda(a_t), _lambda(a_prev)
    h = lam_t - lam_s
    if not (h > 0).all():
        raise ValueError("DPM-Solver++: every step must go towards less noise (a_prev > a_t)")
    out = np.zeros((S, 3), dtype=np.float64)
    out[:, 0] = np.sqrt((1.0 - a_prev) / (1.0 - a_t))          # sigma_t / sigma_s
    phi = -np.sqrt(a_prev) * np.expm1(-h)                       # -alpha_t (e^{-h} - 1)
    out[:, 1] = phi
    for i in range(1, S):
        if order == 1 or (lower_order_final and S < 10 and i == S - 1):
            continue
        r = (lam_s[i] - lam_s[i - 1]) / h[i]
        out[i, 1] = phi[i] * (1.0 + 0.5 / r)
        out[i, 2] = -phi[i] * 0.5 / r
    return out


def ddim_eta_coefficients(a_t, a_prev, sigmas):
    """float64 [S, 4] = (cx, c0, c1 = 0, cn): the reference's p_sample_ddim (ddim.py:123-131)
    x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma^2) e_t + sigma z, with e_t = (x - sqrt(a_t) pred_x0) / sqrt(1 - a_t)."""
    a_t, a_prev, sigmas = (np.asarray(v, dtype=np.float64) for v in (a_t, a_prev, sigmas))
    k = np.sqrt(1.0 - a_prev - sigmas ** 2) / np.sqrt(1.0 - a_t)
    return np.stack([k, np.sqrt(a_prev) - k * np.sqrt(a_t), np.zeros_like(k), sigmas], axis=1)


def make_logsnr_timesteps(S, alphas_cumprod):
    """int64 [S + 1]: the integer timesteps nearest (in lambda) to S + 1 nodes uniform in lambda from the last timestep to timestep 0.
    The evaluations run at nodes 0 .. S-1, evaluation i stepping from abar[node_i] to abar[node_{i+1}]."""
    lam = _lambda(_np(alphas_cumprod))
    T = len(lam)
    if S < 1:
        raise ValueError(f"log-SNR grid: {S} steps")
    targets = np.linspace(lam[T - 1], lam[0], S + 1)
    nodes = np.abs(lam[None, :] - targets[:, None]).argmin(axis=1).astype(np.int64)
    if not (np.diff(nodes) < 0).all():
        smax = S
        while smax > 1:
            smax -= 1
            t = np.linspace(lam[T - 1], lam[0], smax + 1)
            if (np.diff(np.abs(lam[None, :] - t[:, None]).argmin(axis=1)) < 0).all():
                break
        raise ValueError(f"log-SNR grid: {S} steps put two nodes on one integer timestep of this {T}-step schedule "
                         f"(at most {smax} steps here; the SD schedule allows S <= 27)")
    return nodes


class DPMSolverSampler(PLMSSampler):
    multistep = True

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", order=2, lower_order_final=True, verbose=False):
        if order not in (1, 2):
            raise ValueError(f"DPMSolverSampler: order {order!r} is not implemented (1 or 2)")
        if ddim_discretize == "logsnr":
            nodes = make_logsnr_timesteps(ddim_num_steps, self.diffusion.alphas_cumprod)
            super().make_schedule(ddim_num_steps=1, verbose=False)       # the schedule buffers; its one-step grid is replaced below
            ac = _np(self.diffusion.alphas_cumprod)
            # in PLMSSampler's layout: ascending timesteps, index = S - i - 1 for sampling step i
            self.ddim_timesteps = nodes[:-1][::-1].copy()
            self.register_buffer("ddim_alphas", torch.as_tensor(ac[nodes[:-1]][::-1].copy()))
            self.register_buffer("ddim_alphas_prev", ac[nodes[1:]][::-1].copy())
            self.register_buffer("ddim_sigmas", torch.zeros(ddim_num_steps))
            self.register_buffer("ddim_sqrt_one_minus_alphas", np.sqrt(1.0 - ac[nodes[:-1]][::-1]))
        else:
            super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0.0, verbose=verbose)
        self.solver_order, self.lower_order_final = order, lower_order_final
        self._solver_arrays()

    def _solver_arrays(self):
        # sampling order (time descending)
        self.solver_a_t = _np(self.ddim_alphas).astype(np.float64)[::-1].copy()
        self.solver_a_prev = _np(self.ddim_alphas_prev).astype(np.float64)[::-1].copy()
        self.solver_coefs = dpm_solver_coefficients(self.solver_a_t, self.solver_a_prev, order=self.solver_order, lower_order_final=self.lower_order_final)

    def _cut_schedule(self, k):
        # the coefficients of the k steps that run, recomputed on them: the tail's first step has no previous data prediction and is
        # order 1, and lower_order_final is judged on k
        super()._cut_schedule(k)
        self._solver_arrays()

    @torch.no_grad()
    def sample(self, S, shape, input, uc=None, guidance_scale=1, mask=None, x0=None, *, x_init=None, strength=None, resize_mode="bicubic",
               **schedule_kwargs):
        self.make_schedule(ddim_num_steps=S, **schedule_kwargs)
        self._start_tail(shape, input, x_init, strength, resize_mode)
        return self.plms_sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0)

    # ---- device loop ---------------------------------------------------------------------
    def _sample_native(self, shape, input, uc, guidance_scale, mask, x0):
        # the only device-generator draws are q_sample's, one per step when inpainting: the update has no noise term
        img, time_range, cfg, scales, alphas, sd_conv, _, kwargs = self._native_setup(input, uc, guidance_scale, mask, x0, lambda i: 0)
        self.model.engine.sample_solver(img, time_range, self.solver_a_t, self.solver_coefs, scales, guidance_scale if cfg else 1.0, **kwargs)
        return self._native_finish(shape, input, img, time_range, alphas, sd_conv)

    # ---- the same loop on the host, for arbitrary model callables -------------------------------
    def _sample_generic(self, shape, input, uc, guidance_scale, mask, x0):
        b = shape[0]
        img = input["x"]
        time_range = np.flip(self.ddim_timesteps)
        S = len(time_range)
        alphas = self._gate_schedule(S) if self.alpha_generator_func is not None else None
        d_prev = None
        for i, step in enumerate(time_range):
            if alphas is not None:
                self.set_alpha_scale(self.model, alphas[i])
                if alphas[i] == 0:
                    self.model.restore_first_conv_from_SD()
            ts = torch.full((b,), int(step), device=self.device, dtype=torch.long)
            if mask is not None:
                assert x0 is not None
                img = self.diffusion.q_sample(x0, ts) * mask + (1.0 - mask) * img
                input["x"] = img
            x = input["x"].clone()
            input["timesteps"] = ts
            e = self.model(input)
            if uc is not None and guidance_scale != 1:
                e_u = self.model(dict(x=input["x"], timesteps=ts, context=uc, inpainting_extra_input=input["inpainting_extra_input"],
                                      grounding_extra_input=input["grounding_extra_input"]))
                e = e_u + guidance_scale * (e - e_u)
            a_t = float(self.solver_a_t[i])
            d0 = (x - float(np.sqrt(1.0 - a_t)) * e) / float(np.sqrt(a_t))
            cx, c0, c1 = (float(v) for v in self.solver_coefs[i])
            img = cx * x + c0 * d0
            if c1 != 0.0:
                img = img + c1 * d_prev
            input["x"] = img
            d_prev = d0
        return img
