"""PLMS sampler with classifier-free guidance — drop-in for the reference's
ldm/models/diffusion/plms.py (same constructor, make_schedule, sample signature and in-place
updates of `input`).

With the native UNetModel the whole loop runs on the device (Engine::sample_plms): the
[cond ; uncond] pair is one batched UNet evaluation captured in a hipGraph, followed by a fused
CFG + Adams-Bashforth + x_prev kernel (reference plms.py:116-158). Any other `model` callable
(e.g. a recording mock in host-logic tests) goes through `_sample_generic`, which restates the
reference loop around `model(input)` calls.
"""
import numpy as np
import torch

from ldm.modules.diffusionmodules.util import make_ddim_sampling_parameters, make_ddim_timesteps


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


class PLMSSampler(object):
    multistep = True  # False in ldm.models.diffusion.ddim.DDIMSampler: e' = e_t, one model evaluation per step

    def __init__(self, diffusion, model, schedule="linear", alpha_generator_func=None, set_alpha_scale=None):
        super().__init__()
        self.diffusion = diffusion
        self.model = model
        self.device = diffusion.betas.device
        self.ddpm_num_timesteps = diffusion.num_timesteps
        self.schedule = schedule
        self.alpha_generator_func = alpha_generator_func
        self.set_alpha_scale = set_alpha_scale
        self.use_graph = True

    def register_buffer(self, name, attr):
        if type(attr) == torch.Tensor:
            attr = attr.to(self.device)
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=False):
        if ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")
        self._tail = None   # a fresh schedule runs whole; sample(strength=...) cuts it (_cut_schedule)
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize, num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        ac = self.diffusion.alphas_cumprod
        assert ac.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        f32 = lambda x: x.clone().detach().to(torch.float32).to(self.device)
        self.register_buffer("betas", f32(self.diffusion.betas))
        self.register_buffer("alphas_cumprod", f32(ac))
        self.register_buffer("alphas_cumprod_prev", f32(self.diffusion.alphas_cumprod_prev))
        self.register_buffer("sqrt_alphas_cumprod", f32(np.sqrt(ac.cpu())))
        self.register_buffer("sqrt_one_minus_alphas_cumprod", f32(np.sqrt(1.0 - ac.cpu())))
        sigmas, alphas, alphas_prev = make_ddim_sampling_parameters(alphacums=ac.cpu(), ddim_timesteps=self.ddim_timesteps,
                                                                    eta=ddim_eta, verbose=verbose)
        self.register_buffer("ddim_sigmas", sigmas)
        self.register_buffer("ddim_alphas", alphas)
        self.register_buffer("ddim_alphas_prev", alphas_prev)
        self.register_buffer("ddim_sqrt_one_minus_alphas", np.sqrt(1.0 - alphas))

    @torch.no_grad()
    def sample(self, S, shape, input, uc=None, guidance_scale=1, mask=None, x0=None, *, x_init=None, strength=None, resize_mode="bicubic"):
        """x_init, strength: start from a given latent instead of pure noise (image-to-image, the second pass of a two-pass
        generation): the schedule is built as always, the last int(strength * n) of its n steps run (n = len(ddim_timesteps): the uniform
        grid of S = 6 has 7), from x_init resized to `shape` (resize_mode: nearest-exact, bilinear or bicubic) and noised to the first of
        them. strength=None: nothing changes."""
        self.make_schedule(ddim_num_steps=S)
        self._start_tail(shape, input, x_init, strength, resize_mode)
        return self.plms_sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0)

    # ---- partial sampling: the tail of the schedule from a given latent ---------------------------
    def _cut_schedule(self, k):
        """Keep the last k sampling steps of the schedule make_schedule built. Every per-step array is in ascending-timestep order
        (index = S - i - 1 for sampling step i), so the tail is its first k entries; what the loops derive from them (time_range, a_t,
        a_prev, sigmas, the inpainting sqrt tables, solver coefficients) follows. The gate schedule is cut from the full-length one
        (_gate_schedule), so gating follows the noise level, not the position in the shorter run."""
        S = len(self.ddim_timesteps)
        self._tail = (S, k)
        self.ddim_timesteps = self.ddim_timesteps[:k]
        for name in ("ddim_sigmas", "ddim_alphas", "ddim_alphas_prev", "ddim_sqrt_one_minus_alphas"):
            setattr(self, name, getattr(self, name)[:k])

    def _gate_schedule(self, S):
        """alpha_generator_func over the S steps about to run: of a tail, the last S values of the full schedule's."""
        tail = self.__dict__.get("_tail")
        if tail is None:
            return self.alpha_generator_func(S)
        full, k = tail
        assert k == S, "the schedule was cut to another length than the loop runs"
        return list(self.alpha_generator_func(full))[full - k:]

    def _start_tail(self, shape, input, x_init, strength, resize_mode):
        if x_init is None and strength is None:
            return
        who = type(self).__name__
        if strength is None:
            raise ValueError(f"{who}: x_init needs strength (the fraction of the schedule that runs from it, in (0, 1])")
        if x_init is None:
            raise ValueError(f"{who}: strength = {strength} needs x_init (the latent the tail of the schedule starts from)")
        strength = float(strength)
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"{who}: strength = {strength} is not in (0, 1]")
        S = len(self.ddim_timesteps)
        k = int(strength * S)
        if k == 0:
            raise ValueError(f"{who}: strength = {strength} of {S} steps leaves no step to run (int(strength * S) = 0)")
        if resize_mode not in ("nearest-exact", "bilinear", "bicubic"):
            raise ValueError(f"{who}: resize_mode {resize_mode!r}: nearest-exact, bilinear or bicubic")
        shape = tuple(int(v) for v in shape)
        if x_init.dim() != 4 or int(x_init.shape[1]) != shape[1] or int(x_init.shape[0]) not in (1, shape[0]):
            raise ValueError(f"{who}: x_init {tuple(x_init.shape)} is not [{shape[0]} or 1, {shape[1]}, h, w]")
        self._cut_schedule(k)
        t0 = int(self.ddim_timesteps[-1])          # the tail's first (largest) timestep
        # the noise: input["x"] when given (the role starting_noise has in a whole run), else one draw, before every other of the run
        noise = input["x"] if input["x"] is not None else torch.randn(shape, device=self.device)
        if tuple(noise.shape[1:]) != shape[1:] or int(noise.shape[0]) not in (1, shape[0]):
            raise ValueError(f"{who}: the starting noise {tuple(noise.shape)} does not fit a latent of {shape}")
        if int(x_init.shape[0]) != shape[0]:
            x_init = x_init.expand(shape[0], *x_init.shape[1:])
        if hasattr(self.model, "engine") and hasattr(self.model, "set_conditioning"):
            sa = float(self.diffusion.sqrt_alphas_cumprod[t0])
            s1 = float(self.diffusion.sqrt_one_minus_alphas_cumprod[t0])
            input["x"] = self.model.engine.latent_renoise(x_init, shape[2:], resize_mode, sa, s1, noise)
        else:
            # the same on the host, for arbitrary model callables: F.interpolate + q_sample, in the wider of the two dtypes
            import torch.nn.functional as F
            dtype = torch.promote_types(x_init.dtype, noise.dtype)
            x, noise = x_init.to(device=noise.device, dtype=dtype), noise.to(dtype)
            if tuple(x.shape[2:]) != shape[2:]:
                x = F.interpolate(x, size=shape[2:], mode=resize_mode, **({} if resize_mode == "nearest-exact" else dict(align_corners=False)))
            ts = torch.full((shape[0],), t0, device=noise.device, dtype=torch.long)
            input["x"] = self.diffusion.q_sample(x, ts, noise.expand(shape) if int(noise.shape[0]) != shape[0] else noise)

    @torch.no_grad()
    def plms_sampling(self, shape, input, uc=None, guidance_scale=1, mask=None, x0=None):
        if input["x"] is None:
            input["x"] = torch.randn(shape, device=self.device)
        if hasattr(self.model, "engine") and hasattr(self.model, "set_conditioning"):
            return self._sample_native(shape, input, uc, guidance_scale, mask, x0)
        return self._sample_generic(shape, input, uc, guidance_scale, mask, x0)

    # ---- device loop ---------------------------------------------------------------------
    def _native_setup(self, input, uc, guidance_scale, mask, x0, update_draws):
        """What a run on the device needs apart from its update rule (shared with DDIMSampler's eta > 0 path and DPMSolverSampler):
        conditioning, gate-scale schedule, the latent, the device-generator draws, the inpainting tensors, the SD first-conv swap and
        the channels in front of the first conv. update_draws(i) = how many randn_like(x) draws the reference's update makes at step i.
        Returns (img, time_range, cfg, scales, alphas, sd_conv, update_noise, engine keyword arguments)."""
        model = self.model
        time_range = np.flip(self.ddim_timesteps).copy()
        S = len(time_range)
        alphas = None
        if self.alpha_generator_func is not None:
            alphas = np.asarray(self._gate_schedule(S), dtype=np.float32)
        cfg = uc is not None and guidance_scale != 1
        context = input["context"]
        g = input.get("grounding_input")
        if g is None:
            g = model.grounding_tokenizer_input.get_null_input()
        if cfg:
            g_null = model.grounding_tokenizer_input.get_null_input()
            if model.engine.unet_cfg["grounding_kind"] == "tokens":  # spatial-map tokenizers: concatenate their outputs
                tok = lambda kw: model.position_net.tokens(engine=model.engine, **kw)
                g, g_null = {"tokens": tok(g)}, {"tokens": tok(g_null)}
            ctx2 = torch.cat([context, uc.to(context)], dim=0)
            g2 = {k: torch.cat([g[k], g_null[k].to(g[k])], dim=0) for k in g}
        else:
            ctx2, g2 = context, g
        model.set_conditioning(ctx2, g2)
        # The reference's set_alpha_scale matches GatedSelfAttentionDense / GatedCrossAttentionDense by exact type
        # (gligen_inference.py:24-28): a gatedSA2 model keeps scale = 1 on every step, whatever the alpha schedule says.
        # The schedule still decides when the SD first conv is swapped in (plms.py:88-89).
        scales = alphas
        if alphas is None or model.fuser_type == "gatedSA2":
            model.push_fuser_scales()   # whatever the modules carry (1 unless set by hand), possibly one value per fuser
            scales = None

        img = input["x"].to(device=model.engine.device, dtype=torch.float32).contiguous().clone()
        extra = {}
        # Device-generator draws, call for call as the reference makes them, so that equal seeds give equal noise:
        # per step one randn_like(x0) inside q_sample when inpainting (plms.py:96-99 -> ldm.py:19-22), then the
        # sigma_t * randn_like(x) of get_x_prev_and_pred_x0 (plms.py:138; sigma is 0, the draw still advances the
        # generator) -- twice on the first PLMS step (plms.py:144,159), once otherwise and for DDIM (ddim.py:131).
        noise = []
        update_noise = []
        if mask is not None:
            assert x0 is not None
            x0 = x0.to(device=img.device, dtype=torch.float32)
            mask = mask.to(device=img.device, dtype=torch.float32)
        for i in range(S):
            if mask is not None:
                noise.append(torch.randn_like(x0))
            for _ in range(update_draws(i)):
                update_noise.append(torch.randn_like(img))
        if mask is not None:
            if tuple(mask.shape[1:]) != (1, *img.shape[2:]) or tuple(x0.shape[1:]) != tuple(img.shape[1:]):
                raise ValueError(f"inpainting: mask {tuple(mask.shape)} / x0 {tuple(x0.shape)} do not match the latent {tuple(img.shape)}")
            extra = dict(mask=mask, x0=x0, noise=torch.stack(noise),
                         sqrt_ac=self.diffusion.sqrt_alphas_cumprod.cpu().numpy()[time_range],
                         sqrt_1mac=self.diffusion.sqrt_one_minus_alphas_cumprod.cpu().numpy()[time_range])
        gate_off = alphas is not None and bool((alphas == 0).any())
        if gate_off and not model.first_conv_restorable:
            model.restore_first_conv_from_SD()  # prints the reference's "not restorable" notice
        sd_conv = None
        if gate_off and model.first_conv_restorable and not model.__dict__.get("_first_conv_restored"):
            sd_conv = model.load_sd_first_conv()  # swapped in on the device at the first gated-off step
        restore_at = int(np.argmax(alphas == 0)) if sd_conv is not None else -1
        # channels concatenated to x in front of the first conv (reference openaimodel.py:442-447): the masked latent + mask
        # of an inpainting model, or the GroundingDownsampler output of a spatial-map model. The reference's uncond call
        # passes the same tensors (plms.py:118), so one [B] tensor serves both halves of the [cond ; uncond] evaluation; it
        # stays bound after the SD first conv is swapped in (the packed conv keeps its 4 + k layout, those weights are zero).
        if model.inpaint_mode:
            first_conv_extra = input.get("inpainting_extra_input")
            if first_conv_extra is None:
                raise ValueError("inpaint_mode model needs input['inpainting_extra_input']")
        else:
            first_conv_extra = model.first_conv_extra(input)
        kwargs = dict(inpaint_extra=first_conv_extra, use_graph=self.use_graph, sd_first_conv=sd_conv, restore_at=restore_at, **extra)
        return img, time_range, cfg, scales, alphas, sd_conv, update_noise, kwargs

    def _native_finish(self, shape, input, img, time_range, alphas, sd_conv):
        model = self.model
        if sd_conv is not None:
            model.restore_first_conv_from_SD()  # bring the module parameters in line with the engine
        if alphas is not None and self.set_alpha_scale is not None:
            self.set_alpha_scale(model, float(alphas[-1]))  # leave the modules as the reference loop does
        input["x"] = img
        input["timesteps"] = torch.full((shape[0],), int(time_range[-1]), device=img.device, dtype=torch.long)
        return img

    def _sample_native(self, shape, input, uc, guidance_scale, mask, x0):
        img, time_range, cfg, scales, alphas, sd_conv, _, kwargs = self._native_setup(
            input, uc, guidance_scale, mask, x0, lambda i: 2 if (i == 0 and self.multistep) else 1)
        a_t = _np(self.ddim_alphas).astype(np.float32)[::-1].copy()          # index = S - i - 1
        a_prev = _np(self.ddim_alphas_prev).astype(np.float32)[::-1].copy()
        self.model.engine.sample_plms(img, time_range, a_t, a_prev, scales, guidance_scale if cfg else 1.0, ddim=not self.multistep, **kwargs)
        return self._native_finish(shape, input, img, time_range, alphas, sd_conv)

    # ---- reference-shaped host loop for arbitrary model callables -------------------------------
    def _sample_generic(self, shape, input, uc, guidance_scale, mask, x0):
        b = shape[0]
        img = input["x"]
        time_range = np.flip(self.ddim_timesteps)
        S = len(time_range)
        alphas = self._gate_schedule(S) if self.alpha_generator_func is not None else None
        history = []

        def denoiser(inp):
            e = self.model(inp)
            if uc is not None and guidance_scale != 1:
                e_u = self.model(dict(x=inp["x"], timesteps=inp["timesteps"], context=uc,
                                      inpainting_extra_input=inp["inpainting_extra_input"],
                                      grounding_extra_input=inp["grounding_extra_input"]))
                e = e_u + guidance_scale * (e - e_u)
            return e

        def step_back(x, e, index):
            a_t, a_prev = float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index])  # noqa: E501
            pred_x0 = (x - float(np.sqrt(1.0 - a_t)) * e) / float(np.sqrt(a_t))
            return float(np.sqrt(a_prev)) * pred_x0 + float(np.sqrt(1.0 - a_prev)) * e

        for i, step in enumerate(time_range):
            if alphas is not None:
                self.set_alpha_scale(self.model, alphas[i])
                if alphas[i] == 0:
                    self.model.restore_first_conv_from_SD()
            index = S - i - 1
            ts = torch.full((b,), int(step), device=self.device, dtype=torch.long)
            ts_next = torch.full((b,), int(time_range[min(i + 1, S - 1)]), device=self.device, dtype=torch.long)
            if mask is not None:
                assert x0 is not None
                img = self.diffusion.q_sample(x0, ts) * mask + (1.0 - mask) * img
                input["x"] = img
            x = input["x"].clone()
            input["timesteps"] = ts
            e_t = denoiser(input)
            if not self.multistep:
                e_prime = e_t
            elif len(history) == 0:
                input["x"] = step_back(x, e_t, index)
                input["timesteps"] = ts_next
                e_prime = (e_t + denoiser(input)) / 2
            elif len(history) == 1:
                e_prime = (3 * e_t - history[-1]) / 2
            elif len(history) == 2:
                e_prime = (23 * e_t - 16 * history[-1] + 5 * history[-2]) / 12
            else:
                e_prime = (55 * e_t - 59 * history[-1] + 37 * history[-2] - 9 * history[-3]) / 24
            img = step_back(x, e_prime, index)
            input["x"] = img
            history = (history + [e_t])[-3:]
        return img
