"""A training run on MI355X: what the reference's Trainer (trainer.py:166-484) does between a data iterator and a checkpoint file,
around gligen_amd.train.TrainStep -- without its datasets, TensorBoard and image saving.

    Trainer(engine, config, model_state_dict, batches).start_training()

get_input (trainer.py:329-350: latent, context, timestep draw), run_one_step (q_sample / box mask / concatenation in one launch,
Engine.train_step_inputs; the grounding tensors through the config's grounding_tokenizer_input; TrainStep.step: forward, loss,
backward, gradient exchange, AdamW and -- with enable_ema -- the EMA in the same pass), the loop with the reference's save points,
checkpoints in the reference's own layout in both directions (model, opt = torch.optim.AdamW.state_dict(), scheduler = a LambdaLR's
state_dict(), iters, config_dict, ema, autoencoder / text_encoder / diffusion), resuming, and the in-training preview
(trainer.py:419-466). One key is added to the checkpoint, `rng` (the device generator's, torch's CPU generator's and Python's random
state), which the reference ignores and which makes a resumed run continue bit for bit.

    python -m gligen_amd.trainer --synthetic text --total_iters 20 --enable_ema true --output_dir out

runs on gligen_amd.synthetic weights and batches (no checkpoints or datasets exist offline), prints one line per logged iteration,
writes the checkpoints and, started again, continues from out/checkpoint_latest.pth.

With lora_rank in the config (--lora_rank, --lora_alpha, --lora_families, --lora_out) the run trains LoRA adapters over the frozen
model instead (gligen_amd.lora_train.LoraTrainStep; lora_train_base: and the reference's set with them): the checkpoint carries the
adapter tensors under `lora` next to their optimizer state, and lora_out is rewritten in kohya's format at every save point.

gradient_accumulation_steps K (--gradient_accumulation_steps), max_grad_norm (--max_grad_norm; 0: off) and min_snr_gamma
(--min_snr_gamma) are the usual switches of an SD-1.x trainer: an iteration draws K batches and takes one optimizer step on their mean
gradient (TrainStep's accumulate), clipped to a global norm, with the eps-prediction min-SNR weight of every sample's timestep on its
loss. total_iters, warmup_steps and save_every_iters count optimizer steps; checkpoints are written between groups only."""
from __future__ import annotations

import argparse
import os
import random
import shutil
import sys
from collections import deque
from typing import Callable, Dict, Iterator, Mapping, Optional, Union

import torch

from .train import TrainStep, add_input_channels, min_snr_weights, warmup_schedule

CKPT_KEYS = ("model", "text_encoder", "autoencoder", "diffusion", "opt", "scheduler", "iters", "config_dict")   # trainer.py:472-480 (+ "ema", "rng")
SPATIAL = ("canny", "hed", "depth", "normal", "sem")


def draw_timesteps(n: int, generator: torch.Generator, device, _t: Optional[torch.Tensor] = None) -> torch.Tensor:
    """trainer.py:335-337: t = (rand(n) * 1000).long(), and a 1000 (rand() rounds to 1.0 in fp32 products) becomes 999. _t: the
    uniform draw, given instead of drawn (tests)."""
    if _t is None:
        _t = torch.rand(n, generator=generator, device=device)
    t = (torch.pow(_t, 1) * 1000).long()
    return torch.where(t != 1000, t, torch.full_like(t, 999))


def scheduler_state_dict(base_lr: float, warmup_steps: int, total_iters: Optional[int], iters: int) -> dict:
    """The state_dict() of a real torch LambdaLR (what transformers' get_constant_ / get_cosine_schedule_with_warmup return,
    trainer.py:262-265) after `iters` calls of scheduler.step(): built over a stand-in optimizer and positioned directly, since the
    schedule is a closed form of the step count (last_epoch = iters, _step_count = iters + 1, _last_lr = [base_lr * lambda(iters)])."""
    factor = warmup_schedule(1.0, warmup_steps, total_iters)
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: factor(k + 1))
    sched.last_epoch = int(iters)
    sched._step_count = int(iters) + 1
    sched._last_lr = [base_lr * factor(int(iters) + 1)]
    return sched.state_dict()


def read_checkpoint(path: str) -> dict:
    """A checkpoint file of this Trainer or of the reference's (whose config_dict pickles omegaconf classes: read through
    gligen_inference.read_ckpt's stand-ins where omegaconf is not installed)."""
    try:
        return torch.load(path, map_location="cpu", weights_only=False)
    except (ImportError, AttributeError):
        from gligen_inference import read_ckpt
        return read_ckpt(path)


def _plugin(kind: str, what: str) -> dict:
    return dict(target=f"grounding_input.{kind}_grounding_{what}")


def _modality(target: str) -> str:
    """'text' / 'canny' / ... from a tokenizer target such as ldm.modules.diffusionmodules.canny_grounding_net.PositionNet"""
    mod = target.rsplit(".", 2)[-2]
    return mod[:-len("_grounding_net")] if mod.endswith("_grounding_net") else mod


class Trainer:
    """config: a plain mapping with the reference's names -- model (UNet kwargs, or {target, params}), base_learning_rate,
    weight_decay, warmup_steps, scheduler_type (constant | cosine), total_iters, enable_ema, ema_rate, inpaint_mode, save_every_iters,
    output_dir, ckpt (a first-stage checkpoint whose "model" is loaded over model_state_dict, trainer.py:211-213), optionally
    grounding_tokenizer_input / grounding_downsampler_input ({target}; derived from the tokenizer's modality when absent) and
    disable_inference_in_training, gradient_accumulation_steps (K, default 1: an iteration draws K batches), max_grad_norm (default
    and 0: no clipping), min_snr_gamma (default: uniform loss weights). model_state_dict: the starting weights in module order; a first conv narrower than the model's
    (inpaint_mode: 5 channels, a grounding downsampler: its out_dim) is zero-extended (trainer.py:189-193).
    batches: any iterator of dicts with the keys the reference's datasets produce (image or z, caption or context, the grounding
    tensors), or a callable n -> iterator, called with the number of batches already consumed (starting_iter * K), which lets a
    resumed run continue its data where it stopped.
    autoencoder / text_encoder: this package's AutoencoderKL / FrozenCLIPEmbedder on the device; without them the batch carries
    z / context. Every random draw of get_input comes from one torch.Generator on the device seeded seed + rank; the guidance drop
    (10 % of the iterations train on the null grounding input, openaimodel.py:428) from a random.Random(seed).
    resume: a checkpoint file; None resumes from output_dir/checkpoint_latest.pth when it exists (trainer.py:126-153, 291-304);
    False never resumes."""

    def __init__(self, engine, config: Mapping, model_state_dict: Mapping[str, torch.Tensor], batches: Union[Iterator, Callable[[int], Iterator]], *,
                 diffusion=None, autoencoder=None, text_encoder=None, seed: int = 123, resume: Union[None, bool, str] = None, rank: int = 0,
                 world: Optional[int] = None, bucket_mb: float = 128.0, checkpoint: bool = True, drop_prob: float = 0.1, overlap: bool = True,
                 log: Callable[[str], None] = print):
        from ldm.util import instantiate_from_config
        self.engine, self.config, self.rank, self.log = engine, dict(config), int(rank), log
        model = self.config["model"]
        cfg = dict(model["params"] if "params" in model and "target" in model else model)
        cfg["inpaint_mode"] = bool(self.config.get("inpaint_mode", cfg.get("inpaint_mode", False)))
        self.cfg = cfg
        dev = engine.device
        if diffusion is None:
            from ldm.models.diffusion.ldm import LatentDiffusion
            diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
        self.diffusion = diffusion.to(dev)
        self.schedule = {k: getattr(self.diffusion, k).detach().float().to(dev).contiguous() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}
        self.autoencoder, self.text_encoder = autoencoder, text_encoder

        sd = dict(model_state_dict)
        if self.config.get("ckpt") is not None:                       # trainer.py:211-213 (usually for inpainting training)
            sd.update(read_checkpoint(self.config["ckpt"])["model"])
        kind = _modality(cfg["grounding_tokenizer"]["target"]) if cfg.get("grounding_tokenizer") else "text"
        extra = 5 if cfg["inpaint_mode"] else 0
        if cfg.get("grounding_downsampler"):
            extra += int(instantiate_from_config(cfg["grounding_downsampler"]).out_dim)
        short = cfg["in_channels"] + extra - int(sd["input_blocks.0.0.weight"].shape[1])
        if short > 0:
            sd = add_input_channels(sd, short)

        self.base_lr, self.total_iters = float(self.config["base_learning_rate"]), int(self.config["total_iters"])
        self.warmup_steps = int(self.config.get("warmup_steps", 0))
        stype = self.config.get("scheduler_type", "constant")
        if stype not in ("constant", "cosine"):
            raise ValueError(f"scheduler_type {stype!r}: constant or cosine (trainer.py:262-267)")
        self.cosine_total = self.total_iters if stype == "cosine" else None
        self.enable_ema = bool(self.config.get("enable_ema", False))
        self.lora_rank = int(self.config.get("lora_rank") or 0)
        self.accumulate = int(self.config.get("gradient_accumulation_steps") or 1)
        if self.accumulate < 1:
            raise ValueError(f"gradient_accumulation_steps {self.accumulate}: at least 1")
        self.max_grad_norm = float(self.config.get("max_grad_norm") or 0.0) or None
        self.min_snr_gamma = float(self.config.get("min_snr_gamma") or 0.0) or None
        # (the checkpoint's config_dict carries the three keys: a resumed run is held to the same K)
        self.config.update(gradient_accumulation_steps=self.accumulate, max_grad_norm=self.max_grad_norm, min_snr_gamma=self.min_snr_gamma)
        run = dict(accumulate=self.accumulate, max_grad_norm=self.max_grad_norm)
        if self.lora_rank:
            from .lora_train import LoraSpec, LoraTrainStep
            if self.enable_ema:
                raise ValueError("Trainer: no EMA is kept of LoRA adapters (enable_ema with lora_rank)")
            conv_families = tuple(self.config.get("lora_conv_families") or ())
            families = self.config.get("lora_families")
            spec = LoraSpec(self.lora_rank, self.config.get("lora_alpha"), tuple(("attn",) if families is None else families), conv_families=conv_families,
                            conv_rank=self.config.get("lora_conv_rank"), conv_alpha=self.config.get("lora_conv_alpha"))
            self.ts = LoraTrainStep(engine, cfg, sd, spec, lr=warmup_schedule(self.base_lr, self.warmup_steps, self.cosine_total),
                                    weight_decay=float(self.config.get("weight_decay", 0.0)), bucket_mb=bucket_mb, world=world, checkpoint=checkpoint,
                                    drop_prob=drop_prob, rng=random.Random(seed), overlap=overlap, train_base=bool(self.config.get("lora_train_base", False)),
                                    seed=seed, **run)
        else:
            self.ts = TrainStep(engine, cfg, sd, lr=warmup_schedule(self.base_lr, self.warmup_steps, self.cosine_total),
                                weight_decay=float(self.config.get("weight_decay", 0.0)), bucket_mb=bucket_mb, world=world, checkpoint=checkpoint,
                                drop_prob=drop_prob, rng=random.Random(seed), overlap=overlap,
                                ema_rate=float(self.config.get("ema_rate", 0.9999)) if self.enable_ema else None, **run)
        # min(snr, gamma) / snr per timestep (eps-prediction), indexed with the batch's t in run_one_step
        self.snr_weights = min_snr_weights(self.diffusion.alphas_cumprod, self.min_snr_gamma, dev) if self.min_snr_gamma else None
        self._loss_sum = None
        self.generator = torch.Generator(device=dev).manual_seed(int(seed) + self.rank)
        self.grounding_tokenizer_input = instantiate_from_config(self.config.get("grounding_tokenizer_input") or _plugin(kind, "tokinzer_input.GroundingNetInput"))
        self.grounding_downsampler_input = None
        if self.config.get("grounding_downsampler_input") or cfg.get("grounding_downsampler"):
            self.grounding_downsampler_input = instantiate_from_config(self.config.get("grounding_downsampler_input") or
                                                                       _plugin(kind, "downsampler_input.GroundingDSInput"))
        self.output_dir = self.config.get("output_dir")
        self.save_every = int(self.config.get("save_every_iters", 5000))
        self.losses = deque(maxlen=16)          # the last iterations' losses, on the device (no host sync)
        self.iters = self.starting_iter = 0
        self._preview_model = None

        if resume is None and self.output_dir and os.path.exists(os.path.join(self.output_dir, "checkpoint_latest.pth")):
            resume = os.path.join(self.output_dir, "checkpoint_latest.pth")
        if resume:
            self.load(resume)
        self.batches = batches(self.starting_iter * self.accumulate) if (callable(batches) and not hasattr(batches, "__next__")) else batches

    # ---- one iteration ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def get_input(self, batch: Mapping) -> Dict[str, torch.Tensor]:
        """trainer.py:329-350 and the noise of :355: z, context, t, noise (and grounding_extra_input where the model has a grounding
        downsampler). The inpainting mask is not made here: run_one_step hands the boxes to Engine.train_step_inputs."""
        dev = self.engine.device
        z = self.autoencoder.encode(batch["image"].to(dev)) if self.autoencoder is not None else batch["z"]
        z = z.to(device=dev, dtype=torch.float32)
        context = self.text_encoder.encode(batch["caption"]) if self.text_encoder is not None else batch["context"]
        t = draw_timesteps(z.shape[0], self.generator, dev)
        noise = torch.randn(z.shape, generator=self.generator, device=dev, dtype=torch.float32)
        out = dict(z=z, context=context.to(device=dev, dtype=torch.float32), t=t, noise=noise)
        if self.grounding_downsampler_input is not None:
            out["grounding_extra_input"] = self.grounding_downsampler_input.prepare(batch)
        return out

    def run_one_step(self, batch: Mapping) -> torch.Tensor:
        """trainer.py:353-371 + 382-391: one micro-batch -- with gradient_accumulation_steps = 1 one iteration -- on `batch`. `iters`
        counts optimizer steps: it moves when the group is complete. Returns the loss as a device tensor (no host sync): this
        micro-batch's, and on the call that completes a group the mean over the group."""
        inp = self.get_input(batch)
        inpaint = self.cfg["inpaint_mode"]
        rows = self.engine.train_step_inputs(inp["z"], inp["noise"], inp["t"], self.schedule, boxes=batch["boxes"] if inpaint else None, inpaint=inpaint)
        step_batch = dict(self.grounding_tokenizer_input.prepare(batch), context=inp["context"], **rows)
        if "grounding_extra_input" in inp:
            step_batch["grounding_extra_input"] = inp["grounding_extra_input"]
        kw = dict(loss_weights=self.snr_weights[inp["t"]].contiguous()) if self.snr_weights is not None else {}
        loss, _ = self.ts.step(step_batch, **kw)
        if self.accumulate > 1:         # the mean of the group's losses, formed on the device
            self._loss_sum = loss if self._loss_sum is None else self._loss_sum + loss
            if not self.ts.at_boundary:
                return loss
            loss, self._loss_sum = self._loss_sum / self.accumulate, None
        self.iters += 1
        self.losses.append(loss)
        return loss

    def start_training(self) -> int:
        """trainer.py:375-404: iterations starting_iter .. total_iters - 1, each over gradient_accumulation_steps batches; save() at
        iteration 0, at every multiple of save_every_iters and at the end -- between groups, so that a resumed run is exact. The loss is read back (a host sync) only every 10th iteration, where the reference logs it. Returns the
        number of iterations done in total."""
        for it in range(self.starting_iter, self.total_iters):
            for _ in range(self.accumulate):
                loss = self.run_one_step(next(self.batches))
            assert self.iters == it + 1 and self.ts.at_boundary
            if self.rank == 0:
                if it % 10 == 0:
                    norm = f" grad_norm {float(self.ts.grad_norm):.4f}" if self.max_grad_norm else ""
                    self.log(f"iter {it + 1} loss {float(loss):.6f} lr {self.ts.lr_at(it + 1):.3e}{norm}")
                if it == 0 or it % self.save_every == 0 or it == self.total_iters - 1:
                    self.save()
                    if not self.config.get("disable_inference_in_training", True) and self.autoencoder is not None:
                        self.preview(next(self.batches))
        self.starting_iter = self.iters
        return self.iters

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------
    def state(self) -> dict:
        """The reference's checkpoint dict (trainer.py:472-482) at the current iteration, tensors on the CPU."""
        cpu = lambda sd: {k: v.detach().float().cpu() for k, v in sd.items()}
        if self.ts._comm is not None:
            torch.cuda.synchronize(self.engine.device)
        ckpt = dict(model=cpu(self.ts.state_dict()), opt=self.ts.torch_optimizer_state_dict(initial_lr=self.base_lr),
                    scheduler=scheduler_state_dict(self.base_lr, self.warmup_steps, self.cosine_total, self.iters), iters=int(self.iters),
                    config_dict=dict(self.config))
        for name, mod in (("text_encoder", self.text_encoder), ("autoencoder", self.autoencoder), ("diffusion", self.diffusion)):
            if mod is not None and hasattr(mod, "state_dict"):
                ckpt[name] = cpu(mod.state_dict())
        if self.enable_ema:
            ckpt["ema"] = cpu(self.ts.ema_state_dict())
        if self.lora_rank:
            ckpt["lora"] = cpu(self.ts.adapter_tensors())
        ckpt["rng"] = dict(device=self.generator.get_state().cpu(), python=self.ts.rng.getstate(), torch_cpu=torch.get_rng_state())
        return ckpt

    def save(self, path: Optional[str] = None) -> str:
        """checkpoint_<iters, 8 digits>.pth and checkpoint_latest.pth in `path` (default: config["output_dir"]); returns the latter."""
        path = path or self.output_dir
        if not path:
            raise ValueError("Trainer.save: no output_dir in the config and no path given")
        os.makedirs(path, exist_ok=True)
        ckpt = self.state()
        numbered = os.path.join(path, "checkpoint_" + str(self.iters).zfill(8) + ".pth")
        latest = os.path.join(path, "checkpoint_latest.pth")
        torch.save(ckpt, numbered + ".tmp")
        os.replace(numbered + ".tmp", numbered)
        # the same bytes under the second name: a hard link where the file system has them, else a copy; put in place by a rename, so
        # that a run killed while writing leaves the previous checkpoint_latest.pth whole
        if os.path.exists(latest + ".tmp"):
            os.remove(latest + ".tmp")
        try:
            os.link(numbered, latest + ".tmp")
        except OSError:
            shutil.copyfile(numbered, latest + ".tmp")
        os.replace(latest + ".tmp", latest)
        if self.lora_rank and self.config.get("lora_out"):
            out = self.config["lora_out"]
            self.ts.save_adapter(out + ".tmp", dtype=torch.float32 if self.config.get("lora_dtype", "fp16") == "fp32" else torch.float16)
            os.replace(out + ".tmp", out)
        return latest

    def load(self, path: str) -> None:
        """trainer.py:291-304: model, ema, opt and iters of a checkpoint written by save() or by the reference's trainer; `rng` when
        the file has it. The optimizer's step count becomes `iters`, which positions the LR schedule."""
        ckpt = read_checkpoint(path)
        saved_k = int((ckpt.get("config_dict") or {}).get("gradient_accumulation_steps") or 1)      # (a file without the key: K = 1)
        if saved_k != self.accumulate:
            raise ValueError(f"{path} was written with gradient_accumulation_steps = {saved_k}, this run has gradient_accumulation_steps = "
                             f"{self.accumulate}: iterations and the batch stream would no longer line up")
        if self.lora_rank:
            if "lora" not in ckpt:
                raise ValueError(f"{path} carries no adapters (`lora`): it was written by a run without lora_rank")
            saved = ckpt.get("config_dict") or {}
            for key in ("lora_conv_families", "lora_conv_rank", "lora_conv_alpha"):
                was, now = saved.get(key), self.config.get(key)
                was, now = (list(was or []), list(now or [])) if key == "lora_conv_families" else (was, now)
                if was != now:
                    raise ValueError(f"{path} was written with {key} = {was}, this run has {key} = {now}: the adapters would no longer be the same")
        self.ts.load_state_dict(ckpt["model"])
        if self.lora_rank:
            self.ts.load_adapter_tensors(ckpt["lora"])
        self.ts.load_torch_optimizer_state_dict(ckpt["opt"])
        if self.enable_ema:
            self.ts.load_ema_state_dict(ckpt["ema"])
        self.iters = self.starting_iter = int(ckpt["iters"])
        self.ts.steps = self.iters
        self._loss_sum = None           # (the loaders dropped an open group of micro-batches: its partial loss goes with it)
        rng = ckpt.get("rng")
        if rng:
            self.generator.set_state(rng["device"])
            self.ts.rng.setstate(rng["python"])
            torch.set_rng_state(rng["torch_cpu"])
        self.log(f"resumed from {path} at iteration {self.iters}")

    # ---- in-training inference -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def preview(self, batch: Mapping, steps: int = 50, guidance_scale: float = 5, use_ema: bool = False, x_T: Optional[torch.Tensor] = None,
                sampler: str = "plms", discretize: str = "uniform") -> torch.Tensor:
        """trainer.py:419-466: the current parameters (use_ema: the EMA ones) loaded into this package's inference UNetModel,
        PLMSSampler.sample from x_T (drawn when None), decoded; returns u8 [B, H, W, 3] on the device. Needs an autoencoder; the
        context and the unconditional context come from the text encoder, or from batch["context"] / batch["uc"] (zeros).
        sampler="dpmpp_2m": DPMSolverSampler on the `discretize` grid instead (20 steps do what 50 PLMS steps do)."""
        from ldm.models.diffusion.plms import PLMSSampler
        from ldm.modules.diffusionmodules.openaimodel import UNetModel
        if self.autoencoder is None:
            raise ValueError("Trainer.preview: no autoencoder was given, nothing can decode the samples")
        dev = self.engine.device
        if self.ts._comm is not None:
            torch.cuda.synchronize(dev)
        if self._preview_model is None:
            self._preview_model = UNetModel(**self.cfg).to(dev).eval()
        model = self._preview_model
        sd = self.ts.ema_state_dict() if use_ema else self.ts.state_dict()
        model.load_state_dict(sd, strict=True)
        model.grounding_tokenizer_input = self.grounding_tokenizer_input
        to = lambda v: v.to(dev) if torch.is_tensor(v) else v
        batch = {k: to(v) for k, v in batch.items()}
        if self.text_encoder is not None:
            context = self.text_encoder.encode(batch["caption"])
            uc = self.text_encoder.encode(len(batch["caption"]) * [""])
        else:
            context = batch["context"].float()
            uc = batch["uc"].float() if "uc" in batch else torch.zeros_like(context)
        B = int(context.shape[0])
        z = None
        if self.cfg["inpaint_mode"]:
            z = self.autoencoder.encode(batch["image"]) if "image" in batch else batch["z"].float()
        if x_T is not None:
            hw = int(x_T.shape[-1])
        elif z is not None or "z" in batch:
            hw = int((z if z is not None else batch["z"]).shape[-1])
        elif "image" in batch and hasattr(self.autoencoder, "ddconfig"):          # the latent of the batch's images
            hw = int(batch["image"].shape[-1]) // 2 ** (len(self.autoencoder.ddconfig["ch_mult"]) - 1)
        else:
            hw = int(self.cfg["image_size"])                                       # trainer.py:442: model.image_size
        inpainting_extra_input = None
        if self.cfg["inpaint_mode"]:
            rows = self.engine.train_step_inputs(z, torch.zeros_like(z), torch.zeros(B, dtype=torch.long, device=dev), self.schedule, boxes=batch["boxes"], inpaint=True)
            inpainting_extra_input = rows["x_rows"][..., self.cfg["in_channels"]:].permute(0, 3, 1, 2).contiguous()      # z * mask, mask
        grounding_extra_input = self.grounding_downsampler_input.prepare(batch) if self.grounding_downsampler_input is not None else None
        inp = dict(x=None if x_T is None else x_T.to(device=dev, dtype=torch.float32), timesteps=None, context=context, inpainting_extra_input=inpainting_extra_input,
                   grounding_extra_input=grounding_extra_input, grounding_input=self.grounding_tokenizer_input.prepare(batch))
        if sampler not in ("plms", "dpmpp_2m"):
            raise ValueError(f"Trainer.preview: sampler {sampler!r}: 'plms' or 'dpmpp_2m'")
        schedule_kwargs = {}
        if sampler == "dpmpp_2m":
            from ldm.models.diffusion.dpm_solver import DPMSolverSampler as PLMSSampler  # noqa: F811
            schedule_kwargs = dict(ddim_discretize=discretize)
        sampler = PLMSSampler(self.diffusion, model)
        samples = sampler.sample(S=steps, shape=(B, self.cfg["in_channels"], hw, hw), input=inp, uc=uc, guidance_scale=guidance_scale, **schedule_kwargs)
        images = torch.clamp(self.autoencoder.decode(samples), min=-1, max=1)
        return self.autoencoder.engine.to_uint8(images)


# ---- command line: a run on synthetic weights and batches ------------------------------------------------------------------------
def synthetic_config(kind: str, *, small: bool = False, latent: int = 64, inpaint: bool = False, fuser: str = "gatedSA") -> dict:
    """UNetModel kwargs of a synthetic run: the shipped topology (small: the two-level test UNet) with the `kind` tokenizer (text,
    text_image, keypoint, or a spatial-map modality with its grounding downsampler, as configs/cc3m_canny.yaml etc. pair them)."""
    from . import synthetic as syn
    cfg = dict(syn.UNET_CFG_SMALL if small else syn.UNET_CFG, fuser_type=fuser, inpaint_mode=bool(inpaint))
    if kind in SPATIAL:
        ds = dict(out_dim=1) if kind == "hed" else dict(resize_input=4 * latent, out_dim=8)
        tk = dict(resize_input=128 if small else 256, out_dim=768)
        if kind == "sem":
            ds["in_dim"], tk["in_dim"] = 152, 152
        cfg.update(grounding_downsampler=dict(target=f"ldm.modules.diffusionmodules.{kind}_grounding_downsampler.GroundingDownsampler", params=ds),
                   grounding_tokenizer=dict(target=f"ldm.modules.diffusionmodules.{kind}_grounding_net.PositionNet", params=tk))
    elif kind in syn.GROUNDING_TOKENIZERS:
        cfg["grounding_tokenizer"] = syn.GROUNDING_TOKENIZERS[kind]
    else:
        raise ValueError(f"--synthetic {kind}: one of {sorted(syn.GROUNDING_TOKENIZERS) + list(SPATIAL)}")
    return cfg


def synthetic_state_dict(cfg: Mapping, seed: int = 1234) -> Dict[str, torch.Tensor]:
    """Seeded weights for `cfg` in module order (gligen_amd.synthetic.seeded_state_dict over the model's own state_dict shapes)."""
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from . import synthetic as syn
    m = UNetModel(**cfg)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    del m
    return syn.seeded_state_dict(shapes, seed)


def synthetic_batches(kind: str, B: int, latent: int, *, start: int = 0, seed: int = 0, map_res: int = 256, n_valid: int = 3) -> Iterator[dict]:
    """An endless iterator of dataset-style batches drawn from gligen_amd.synthetic: batch i depends on (seed, i) alone, so a run
    resumed at iteration i sees the batches it would have seen. z [B, 4, latent, latent] and context [B, 77, 768] stand in for the
    image and the caption."""
    from . import synthetic as syn
    from .engine import SPATIAL_MAP_KEYS
    i = int(start)
    while True:
        s = seed * 1000003 + i
        batch = dict(z=syn.make_latent(B, 4, latent, latent, seed=s), context=syn.make_context(B, seed=s))
        if kind in SPATIAL:
            batch[SPATIAL_MAP_KEYS[kind]] = syn.make_spatial_map(kind, B, map_res, seed=s)
            batch["mask"] = torch.ones(B, 1)
        else:
            batch.update(syn.make_batch(kind, B, n_valid=n_valid, seed=s))
        yield batch
        i += 1


def _bool(v: str) -> bool:
    return str(v).lower() in ("1", "true", "yes", "y")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gligen_amd.trainer", description=__doc__.split("\n\n")[0])
    ap.add_argument("--synthetic", required=True, help="text | text_image | keypoint | canny | hed | depth | normal | sem")
    ap.add_argument("--inpaint", action="store_true", help="inpaint_mode: the 9-channel first conv, trained (discrete tokenizers)")
    ap.add_argument("--fuser", default="gatedSA", choices=["gatedSA", "gatedSA2", "gatedCA"])
    ap.add_argument("--small", action="store_true", help="the two-level test UNet instead of the shipped topology")
    ap.add_argument("--latent", type=int, default=64, help="latent height and width")
    ap.add_argument("--total_iters", type=int, default=20)
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--base_learning_rate", type=float, default=5e-5)
    ap.add_argument("--weight_decay", type=float, default=0.0)
    ap.add_argument("--warmup_steps", type=int, default=10000)
    ap.add_argument("--scheduler_type", default="constant", choices=["constant", "cosine"])
    ap.add_argument("--save_every_iters", type=int, default=5000)
    ap.add_argument("--enable_ema", type=_bool, default=False)
    ap.add_argument("--ema_rate", type=float, default=0.9999)
    ap.add_argument("--gradient_accumulation_steps", type=int, default=1, help="micro-batches per optimizer step (an iteration draws this many batches)")
    ap.add_argument("--max_grad_norm", type=float, default=0.0, help="clip the global gradient norm to this (0: off)")
    ap.add_argument("--min_snr_gamma", type=float, default=0.0, help="min-SNR-gamma loss weights, eps-prediction form (0: off; 5 is customary)")
    ap.add_argument("--lora_rank", type=int, default=0, help="train LoRA adapters of this rank over the frozen model instead of the reference's set")
    ap.add_argument("--lora_alpha", type=float, default=None, help="the adapters' alpha (default: the rank)")
    ap.add_argument("--lora_families", nargs="+", default=["attn"], choices=["attn", "ff", "proj"])
    ap.add_argument("--lora_conv_families", nargs="+", default=[], choices=["conv", "emb", "sample"],
                    help="also adapt ResBlock convs and skip_connection (conv), emb_layers.1 (emb), Downsample / Upsample convs (sample)")
    ap.add_argument("--lora_conv_rank", type=int, default=None, help="rank of the adapters on 3 x 3 convs (default: lora_rank)")
    ap.add_argument("--lora_conv_alpha", type=float, default=None, help="their alpha (default: lora_conv_rank)")
    ap.add_argument("--lora_out", default=None, help="the adapter in kohya's format (.safetensors), rewritten at every save point; default output_dir/lora.safetensors")
    ap.add_argument("--resume", action="store_true", help="continue from output_dir/checkpoint_latest.pth (also the default when that file exists)")
    ap.add_argument("--fresh", action="store_true", help="start from iteration 0 even if output_dir holds a checkpoint")
    ap.add_argument("--seed", type=int, default=123)
    ap.add_argument("--arena_gb", type=float, default=24.0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    from .build import build_native
    from .engine import Engine
    build_native()
    cfg = synthetic_config(a.synthetic, small=a.small, latent=a.latent, inpaint=a.inpaint, fuser=a.fuser)
    config = dict(model=cfg, base_learning_rate=a.base_learning_rate, weight_decay=a.weight_decay, warmup_steps=a.warmup_steps, scheduler_type=a.scheduler_type,
                  total_iters=a.total_iters, enable_ema=a.enable_ema, ema_rate=a.ema_rate, inpaint_mode=a.inpaint, save_every_iters=a.save_every_iters,
                  output_dir=a.output_dir, ckpt=None, batch_size=a.batch_size, seed=a.seed, disable_inference_in_training=True,
                  gradient_accumulation_steps=a.gradient_accumulation_steps, max_grad_norm=a.max_grad_norm or None, min_snr_gamma=a.min_snr_gamma or None)
    if a.lora_rank:
        config.update(lora_rank=a.lora_rank, lora_alpha=a.lora_alpha, lora_families=list(a.lora_families), lora_conv_families=list(a.lora_conv_families),
                      lora_conv_rank=a.lora_conv_rank, lora_conv_alpha=a.lora_conv_alpha,
                      lora_out=a.lora_out or os.path.join(a.output_dir, "lora.safetensors"))
    latest = os.path.join(a.output_dir, "checkpoint_latest.pth")
    if a.resume and not os.path.exists(latest):
        print(f"--resume: {latest} does not exist", file=sys.stderr)
        return 2
    engine = Engine(a.device, arena_gb=a.arena_gb)
    try:
        no_inpaint = dict(cfg, inpaint_mode=False)         # the starting weights have the 4-channel first conv; the Trainer extends it
        sd = synthetic_state_dict(no_inpaint if a.inpaint else cfg)
        batches = lambda start: synthetic_batches(a.synthetic, a.batch_size, a.latent, start=start, seed=a.seed, map_res=128 if a.small else 256)
        tr = Trainer(engine, config, sd, batches, seed=a.seed, resume=False if a.fresh else None)
        if tr.starting_iter >= a.total_iters:
            print("Training finished. Start exiting")
            return 0
        done = tr.start_training()
        torch.cuda.synchronize()
        print(f"Training finished at iteration {done}: {latest}")
    finally:
        engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
