"""DDIM sampler (eta = 0) with classifier-free guidance — drop-in for the reference's
ldm/models/diffusion/ddim.py (same constructor, make_schedule, sample / ddim_sampling signatures and
in-place updates of `input`); gligen_inference.py --no_plms selects it with 250 steps
(reference gligen_inference.py:385-387).

The reference only ever builds the schedule with its default ddim_eta = 0 (ddim.py:27,59-62), for which
sigma_t = 0 and p_sample_ddim (ddim.py:111-134) reduces to
    pred_x0 = (x - sqrt(1 - a_t) e_t) / sqrt(a_t);   x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev) e_t
i.e. the PLMS update with e' = e_t and no multistep history. The device loop is therefore the PLMS loop of
Engine::sample_plms with gl_plms_args.ddim = 1 (one hipGraph-replayed [cond ; uncond] evaluation per step + the
fused CFG / x_prev kernel); any other `model` callable goes through PLMSSampler._sample_generic with
multistep off.

StochasticDDIMSampler is the same sampler with the eta > 0 the reference's p_sample_ddim implements but its callers never
reach: x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma_t^2) e_t + sigma_t z. That update is linear in (x, pred_x0, z), so it
runs on the solver loop (Engine::sample_solver, ldm/models/diffusion/dpm_solver.py) with the reference's randn_like draws as z.
"""
import numpy as np
import torch

from ldm.models.diffusion.plms import PLMSSampler, _np


class DDIMSampler(PLMSSampler):
    multistep = False

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=False):
        if ddim_eta != 0:
            raise NotImplementedError("DDIMSampler: only ddim_eta = 0 (the value the reference uses) is implemented; "
                                      "StochasticDDIMSampler takes ddim_eta > 0")
        return super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0.0, verbose=verbose)

    @torch.no_grad()
    def ddim_sampling(self, shape, input, uc, guidance_scale=1, mask=None, x0=None):
        return self.plms_sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0)


class StochasticDDIMSampler(DDIMSampler):
    """DDIMSampler whose make_schedule accepts ddim_eta > 0 (ddim.py:111-134). `ddim_eta` set on the sampler is what
    sample(S, ...) builds its schedule with. With eta = 0 everything is DDIMSampler's, bit for bit."""
    ddim_eta = 0.0

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=None, verbose=False):
        eta = float(self.ddim_eta if ddim_eta is None else ddim_eta)
        if eta < 0:
            raise ValueError(f"StochasticDDIMSampler: ddim_eta = {eta} is negative")
        PLMSSampler.make_schedule(self, ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0.0, verbose=verbose)
        if eta != 0:
            # sigmas of make_ddim_sampling_parameters(eta=...) (reference util.py:72-83) over the grid just built
            from ldm.modules.diffusionmodules.util import make_ddim_sampling_parameters
            sigmas, _, _ = make_ddim_sampling_parameters(alphacums=self.diffusion.alphas_cumprod.cpu(), ddim_timesteps=self.ddim_timesteps,
                                                         eta=eta, verbose=verbose)
            self.register_buffer("ddim_sigmas", sigmas)

    def _stochastic(self):
        return bool((_np(self.ddim_sigmas) != 0).any())

    def _coefs(self):
        from ldm.models.diffusion.dpm_solver import ddim_eta_coefficients
        flip = lambda v: _np(v).astype(np.float64)[::-1].copy()                  # sampling order: index = S - i - 1
        a_t = flip(self.ddim_alphas)
        return a_t, ddim_eta_coefficients(a_t, flip(self.ddim_alphas_prev), flip(self.ddim_sigmas))

    def _sample_native(self, shape, input, uc, guidance_scale, mask, x0):
        if not self._stochastic():
            return super()._sample_native(shape, input, uc, guidance_scale, mask, x0)
        # the reference's draws in the reference's order (q_sample's when inpainting, then ddim.py:131's): equal seeds, equal noise
        img, time_range, cfg, scales, alphas, sd_conv, z, kwargs = self._native_setup(input, uc, guidance_scale, mask, x0, lambda i: 1)
        a_t, coefs = self._coefs()
        self.model.engine.sample_solver(img, time_range, a_t, coefs, scales, guidance_scale if cfg else 1.0, step_noise=torch.stack(z), **kwargs)
        return self._native_finish(shape, input, img, time_range, alphas, sd_conv)

    def _sample_generic(self, shape, input, uc, guidance_scale, mask, x0):
        if not self._stochastic():
            return super()._sample_generic(shape, input, uc, guidance_scale, mask, x0)
        b = shape[0]
        img = input["x"]
        time_range = np.flip(self.ddim_timesteps)
        S = len(time_range)
        alphas = self._gate_schedule(S) if self.alpha_generator_func is not None else None
        for i, step in enumerate(time_range):
            if alphas is not None:
                self.set_alpha_scale(self.model, alphas[i])
                if alphas[i] == 0:
                    self.model.restore_first_conv_from_SD()
            index = S - i - 1
            ts = torch.full((b,), int(step), device=self.device, dtype=torch.long)
            if mask is not None:
                assert x0 is not None
                img = self.diffusion.q_sample(x0, ts) * mask + (1.0 - mask) * img
                input["x"] = img
            x = input["x"]
            input["timesteps"] = ts
            e_t = self.model(input)
            if uc is not None and guidance_scale != 1:
                e_u = self.model(dict(x=x, timesteps=ts, context=uc, inpainting_extra_input=input["inpainting_extra_input"],
                                      grounding_extra_input=input["grounding_extra_input"]))
                e_t = e_u + guidance_scale * (e_t - e_u)
            a_t, a_prev, sigma = float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index]), float(self.ddim_sigmas[index])
            pred_x0 = (x - float(np.sqrt(1.0 - a_t)) * e_t) / float(np.sqrt(a_t))
            img = float(np.sqrt(a_prev)) * pred_x0 + float(np.sqrt(1.0 - a_prev - sigma ** 2)) * e_t + sigma * torch.randn_like(x)
            input["x"] = img
        return img
