"""Host side of one optimisation step of the reference's trainer on MI355X.

Reference: trainer.py:353-392 (run_one_step: model(input) on the noised latent, mse_loss(model_output, noise); loss.backward();
opt.step()), :217-245 (the trainable set: every fuser.* parameter and position_net; torch.optim.AdamW over it), :321-322 +
distributed.py:53-62 (DistributedDataParallel: gradients averaged over the ranks).

Everything numeric runs in the library: forward + backward in gl_unet_train_step, the update in gl_op_adamw_step. What lives here is
the bookkeeping the reference leaves to torch.optim / DDP: the trainable parameters and their gradients are views into a few flat
fp32 buffers (gligen_amd.dist.GradBuckets), so the backward writes the gradients where the collective reads them, one
reduce-scatter + all-gather pair per bucket goes over RCCL, and AdamW is one launch per bucket over the flat range.
The step is built for the three discrete grounding tokenizers and the five spatial-map ones with any of the reference's fuser types
(cfg["fuser_type"]: gatedSA, the default; gatedSA2, which needs a square number of grounding tokens and a square latent; gatedCA, whose
state_dict has no fuser.linear.*); the batch dict carries
boxes + masks + positive_embeddings (text), + text_embeddings / image_embeddings / text_masks / image_masks (text+image), points + masks
(keypoint), or the map under the reference's key (canny_edge, hed_edge, depth, normal, sem) + mask + grounding_extra_input.
An inpainting model (cfg["inpaint_mode"], discrete tokenizers; trainer.py:189-194, 339-344) trains its 9-channel first conv's weight
as well; its batch carries inpainting_extra_input [B, 5, H, W] next to x, or x_rows / target_rows from Engine.train_step_inputs.
With ema_rate the update is gl_op_adamw_ema_step: AdamW and the reference's EMA of the parameters (trainer.py:121-123, 390-391) in one
launch per bucket. The optimizer state travels in torch.optim.AdamW's own layout (torch_optimizer_state_dict), so a checkpoint crosses
to the reference's trainer and back; the loop, the checkpoint files and resuming are gligen_amd.trainer.Trainer."""
from __future__ import annotations

import math
import random
from typing import Callable, Dict, Mapping, Optional, Union

import torch
import torch.distributed as tdist

from .dist import GradBuckets

GROUNDING_KEYS = ("boxes", "masks", "positive_embeddings", "text_embeddings", "image_embeddings", "text_masks", "image_masks", "points",
                  # the spatial-map tokenizers' map and mask (grounding_input/*_grounding_tokinzer_input.py); grounding_extra_input, the
                  # GroundingDownsampler's input, is not part of the drop (openaimodel.py:428-429 replaces the tokenizer's input only).
                  # The bare "mask" is the spatial tokenizers' key alone: the discrete batches carry "masks", the inpainting mask
                  # never travels as a batch key (tests/test_train_spatial_cpu.py holds the discrete batches to that)
                  "canny_edge", "hed_edge", "depth", "normal", "sem", "mask")


def warmup_schedule(base_lr: float, warmup_steps: int, total_iters: Optional[int] = None) -> Callable[[int], float]:
    """The reference's LR schedules (trainer.py:262-267, transformers' get_constant_ / get_cosine_schedule_with_warmup):
    linear warm-up over `warmup_steps`, then constant -- or, with total_iters, half a cosine down to 0. step counts from 1
    (the optimiser step about to be taken), i.e. LambdaLR's epoch + 1 at the time opt.step() uses the rate."""
    def lr(step: int) -> float:
        k = step - 1                     # LambdaLR's epoch when this step's update is computed
        if k < warmup_steps:
            return base_lr * k / max(1, warmup_steps)
        if total_iters is None:
            return base_lr
        prog = (k - warmup_steps) / max(1, total_iters - warmup_steps)
        return base_lr * max(0.0, 0.5 * (1.0 + math.cos(math.pi * prog)))
    return lr


def min_snr_weights(alphas_cumprod, gamma: float, device=None) -> torch.Tensor:
    """Min-SNR-gamma loss weights for an eps-prediction model (Hang et al. 2023, "Efficient Diffusion Training via Min-SNR Weighting
    Strategy"; kohya's --min_snr_gamma): one weight per timestep, min(snr, gamma) / snr with snr = a / (1 - a) for a = alphas_cumprod[t],
    formed in float64 and stored as fp32 (on `device` when given). 1 exactly where snr <= gamma, below 1 at the low-noise timesteps.
    weights[t] for a batch's timesteps t are Engine.unet_train_step's / TrainStep.step's loss_weights."""
    if not float(gamma) > 0.0:
        raise ValueError(f"min_snr_weights: gamma {gamma!r} is not > 0")
    a = torch.as_tensor(alphas_cumprod).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    snr = a / (1.0 - a)
    w = (torch.clamp(snr, max=float(gamma)) / snr).to(torch.float32)
    return w if device is None else w.to(device).contiguous()


def null_grounding(batch: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """GroundingNetInput.get_null_input (grounding_input/*_tokinzer_input.py:30-45): every grounding tensor zeroed. A semantic map given
    as a torch.uint8 class map becomes 255 everywhere instead, the "no class" of grounding_input/_base.py: zeros would read as class 0
    in every pixel. grounding_extra_input is kept in either format."""
    null = lambda v: torch.full_like(v, 255) if v.dtype == torch.uint8 else torch.zeros_like(v)
    return {k: (null(v) if k in GROUNDING_KEYS else v) for k, v in batch.items()}


def has_grounding_downsampler(state_dict: Mapping[str, torch.Tensor], cfg: Optional[Mapping] = None) -> bool:
    """Whether the model feeds a GroundingDownsampler's output into its first conv (openaimodel.py:288-305): the config's
    `grounding_downsampler` when a config is given (TrainStep and Engine.unet_train_step pass it). Without a config it is a
    heuristic read off the state_dict: downsample_net.* weights, or a ConvNeXt tokenizer -- every spatial-map config the reference
    ships pairs its tokenizer with a downsampler (hed's has no parameters), but a custom config need not."""
    if cfg is not None:
        return bool(cfg.get("grounding_downsampler"))
    return any(k.startswith("downsample_net.") or k.startswith("position_net.convnext_tiny_backbone.") for k in state_dict)


def trainable_names(state_dict: Mapping[str, torch.Tensor], cfg: Optional[Mapping] = None):
    """trainer.py:217-245: 'transformer_blocks' + 'fuser' in the name, 'position_net', 'downsample_net', and the first conv's weight
    when additional channels come from a grounding downsampler or the config says inpaint_mode (trainer.py:189-194, 233:
    input_conv_train; the bias stays frozen). Without a config an inpainting model cannot be told from a state_dict whose first conv
    merely has nine input channels, and its first conv stays out of the set."""
    conv_train = has_grounding_downsampler(state_dict, cfg) or bool(cfg is not None and cfg.get("inpaint_mode"))
    return [k for k in state_dict if ".fuser." in k or k.startswith("position_net.") or k.startswith("downsample_net.")
            or (conv_train and k == "input_blocks.0.0.weight")]


def add_input_channels(state_dict: Mapping[str, torch.Tensor], n: int) -> Dict[str, torch.Tensor]:
    """A copy of `state_dict` whose first conv reads `n` more input channels, the new filter taps zero: what the reference does to an
    SD / GLIGEN checkpoint before it loads it into a model with a wider first conv (trainer.py:189-193; n = 5 for inpaint_mode: the
    masked latent's four channels and the mask). The existing channels keep their bits; the tensors of the input are not written."""
    if n < 0:
        raise ValueError("add_input_channels: n must be >= 0")
    out = dict(state_dict)
    w = state_dict["input_blocks.0.0.weight"]
    pad = torch.zeros((w.shape[0], int(n)) + tuple(w.shape[2:]), dtype=w.dtype, device=w.device)
    out["input_blocks.0.0.weight"] = torch.cat([w, pad], dim=1)
    return out


def _block_order(prefix: str):
    """Module order of a SpatialTransformer's path, whatever order the dict was iterated in: input_blocks.N (numeric N, so
    input_blocks.10 follows input_blocks.2), then middle_block.N, then output_blocks.N -- the order UNetModel.forward walks and
    gl_unet_train_step numbers the blocks in."""
    parts = prefix.split(".")
    stage = {"input_blocks": 0, "middle_block": 1, "output_blocks": 2}.get(parts[0])
    if stage is None:
        raise ValueError(f"trainable fuser outside input_blocks / middle_block / output_blocks: {prefix!r}")
    return (stage,) + tuple(int(p) if p.isdigit() else -1 for p in parts[1:])


def gradient_milestones(names):
    """For every trainable tensor the milestone of gl_unet_train_step behind which its gradient is final (gl_train_wait_grads): a fuser
    tensor's is the number of its SpatialTransformer in MODULE order (input_blocks .., middle_block, output_blocks .., by the numeric
    index in the path -- not the iteration order of the dict handed in: a re-sorted state_dict puts input_blocks.10 before
    input_blocks.2 and would point a bucket at the wrong event), every other tensor's (position_net, downsample_net, the first conv)
    is the number of SpatialTransformers -- the end of the backward. The backward walks the blocks from the last to the first, so milestone j is reached before milestone j - 1."""
    blocks = sorted({k.split(".transformer_blocks.")[0] for k in names if ".fuser." in k}, key=_block_order)
    index = {b: i for i, b in enumerate(blocks)}
    return {k: (index[k.split(".transformer_blocks.")[0]] if ".fuser." in k else len(blocks)) for k in names}


class TrainStep:
    """lr: a float, or a callable step -> rate (warmup_schedule: the reference's warm-up schedulers). drop_prob: the probability with
    which an iteration trains on the null grounding input (UNetModel.forward, openaimodel.py:428: 0.1 while training; 0 here by
    default so that a step is a pure function of its batch; null_grounding: zeros, or 255 = "no class" for a u8 class map, so class-map
    batches of the sem model drop the same way) -- drawn from `rng` (random.Random; seed it identically on every rank
    or not at all, as the reference does). With torch.distributed initialised, rank 0's trainable parameters are broadcast once at
    construction, as DistributedDataParallel does (trainer.py:321-322): replicas that start from different state_dicts would
    otherwise drift apart silently.

    overlap (default): the gradient exchange runs UNDER the backward, as DDP's does. The buckets are laid out in the order the
    gradients become final (last SpatialTransformer first, position_net last); after the training step has been enqueued, each
    bucket's reduce-scatter + all-gather and its AdamW update go to a communication stream that waits only for that bucket's
    milestone (gl_train_wait_grads), so bucket 0 is on the wire while the encoder blocks are still in backward; the compute stream
    joins the communication stream at the end of the step. overlap=False: backward, then every collective, then every update, on
    one stream (the round-4 schedule) -- the same numbers bit for bit (same kernels per bucket, same order inside a bucket).

    Arena: the engine's context must hold one block's recompute working set plus the saved block inputs -- 24 GB covers the shipped
    topology at batch 4 x 64 x 64 with checkpoint=True (bench.py / tools/train_bench.py create Engine(arena_gb=24)); the library
    raises 'arena exhausted' (GL_ERR_RUNTIME) rather than spilling when it does not.

    An inpainting model (cfg["inpaint_mode"]): step(batch) takes the reference's keys -- x (the noised latent) and
    inpainting_extra_input = cat(z * mask, mask) [B, 5, H, W] -- or x_rows [B, H, W, 9] / target_rows [B, H, W, 4] as
    Engine.train_step_inputs writes them (no permute copies; any model takes its rows that way); the first conv's weight is part of
    the trainable set and of the last bucket. The guidance drop leaves all three alone.

    The fuser type comes from cfg["fuser_type"] (Engine.unet_train_step): a gatedSA2 model has gatedSA's keys and buckets, a gatedCA model
    has no fuser.linear.* and its fuser.attn.to_k / to_v are [C, context_dim]; the trainable set is name-based and covers both.

    ema_rate (None: no average, the calls and buffers above and nothing else): the reference's EMA of the model (trainer.py:121-123,
    251-256, 390-391; --enable_ema, --ema_rate). One more flat buffer set `self.ema` in the bucket layout, initialised to the
    parameters (deepcopy(self.model)); every bucket update is then Engine.op_adamw_ema_step, AdamW and the average of the updated
    parameters in one pass on the stream the update ran on before: the same parameter bits, and the same EMA bits from both schedules.

    accumulate = K (1: the calls above and nothing else): step() is called once per MICRO-batch. Calls 1 .. K - 1 of a group run
    forward + backward and one Engine.op_grad_accumulate per bucket into one more bucket set `self.acc` (allocated only when K > 1) --
    no collective, as under DDP's no_sync, no update, `steps` does not move --; call K writes the mean (g_1 + .. + g_K) / K into the
    gradient buckets per bucket in front of that bucket's exchange, so the exchange and the update read what they read without
    accumulation. `steps`, the LR schedule and AdamW's bias correction count optimizer steps; the guidance drop is drawn per call;
    `micro` is the position in the group, `at_boundary` whether none is open; the loaders reset the group.

    max_grad_norm (None or 0: off): torch.nn.utils.clip_grad_norm_ over the whole trainable set, after the average over the ranks and
    the micro-batches. Behind bucket i's exchange, on its stream, Engine.op_grad_sqnorm writes that bucket's partial sums (the zero
    padding of a bucket included); behind the last bucket Engine.op_clip_coef forms (norm, coefficient) on the device and every bucket's
    update is Engine.op_adamw_clip_step / op_adamw_ema_clip_step, which reads the coefficient there: no host sync. Under overlap the
    exchanges and norm passes stay under the backward, the updates wait for the coefficient -- inherent to a global norm.
    `grad_norm` is the device tensor [1] with the norm before clipping, the same on every rank. The gradient buckets keep the
    UNCLIPPED average (torch scales .grad in place; nothing here reads it after the update).

    step(..., loss_weights=w): per-sample loss weights, fp32 [B] on the device (Engine.unet_train_step; min_snr_weights).

    Both schedules and the host-side one give the same bits with every combination of these, and two runs give the same bits.

    state_dict should be in module order (what UNetModel.state_dict() gives): the order of its trainable names is the parameter
    numbering of torch_optimizer_state_dict."""

    def __init__(self, engine, cfg: Mapping, state_dict: Mapping[str, torch.Tensor], lr: Union[float, Callable[[int], float]] = 5e-5,
                 weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, bucket_mb: float = 128.0, world: Optional[int] = None,
                 checkpoint: bool = True, drop_prob: float = 0.0, rng: Optional[random.Random] = None, broadcast: bool = True, overlap: bool = True,
                 cache_frozen: bool = True, exchange_even_alone: bool = False, ema_rate: Optional[float] = None, accumulate: int = 1,
                 max_grad_norm: Optional[float] = None):
        self.engine, self.cfg = engine, dict(cfg)
        # (a world of one rank issues no collective; True sends the buckets through the collectives anyway -- the one-GPU test of the
        # overlapped schedule with RCCL's kernels on the communication stream, tests/test_ops_gpu.py)
        self.exchange_even_alone = bool(exchange_even_alone)
        dev = engine.device
        self.lr = lr if callable(lr) else float(lr)
        self.wd, self.betas, self.eps = float(weight_decay), tuple(betas), float(eps)
        self.drop_prob, self.rng = float(drop_prob), rng or random.Random()
        self.checkpoint = bool(checkpoint)       # activation checkpointing per block (the reference: use_checkpoint=True in every shipped config)
        names = trainable_names(state_dict, self.cfg)
        self.param_order = list(names)      # torch.optim.AdamW's parameter numbering: the reference's named_parameters() order
        self.milestone = gradient_milestones(names)
        n_blocks = max(self.milestone.values(), default=0)
        # the engine numbers SpatialTransformers by walking the config; both counts must agree or bucket_ready waits on the wrong events
        n_st = getattr(engine, "count_spatial_transformers", None)
        if callable(n_st) and any(".fuser." in k for k in names) and n_st(self.cfg) != n_blocks:
            raise ValueError(f"TrainStep: {n_blocks} fuser blocks in the state_dict, {n_st(self.cfg)} SpatialTransformers in the config")
        # bucket order = the order in which gradients become final: blocks from the last to the first, position_net at the end
        names = sorted(names, key=lambda k: (self.milestone[k] == n_blocks, -self.milestone[k]))
        shapes = {k: tuple(state_dict[k].shape) for k in names}
        # parameters, gradients and the two AdamW moments share one bucket layout
        self.pbuf = GradBuckets(shapes, bucket_mb, world, device=dev)
        self.gbuf = GradBuckets(shapes, bucket_mb, world, device=dev)
        self.m = [torch.zeros_like(b) for b in self.pbuf.buckets]
        self.v = [torch.zeros_like(b) for b in self.pbuf.buckets]
        self.params: Dict[str, torch.Tensor] = {}
        for k, t in state_dict.items():
            t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            if k in shapes:
                self.pbuf.views[k].copy_(t)
                self.params[k] = self.pbuf.views[k]          # the model's trainable tensors ARE the flat buffers
            else:
                self.params[k] = t
        if broadcast and tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            for b in self.pbuf.buckets:            # the views alias the buckets: one collective per bucket moves every trainable tensor
                tdist.broadcast(b, src=0)
        if ema_rate is not None and not 0.0 <= float(ema_rate) <= 1.0:
            raise ValueError(f"TrainStep: ema_rate {ema_rate!r} is outside [0, 1]")
        self.ema_rate = None if ema_rate is None else float(ema_rate)
        self.ema = None if ema_rate is None else [b.clone() for b in self.pbuf.buckets]       # (after the broadcast: deepcopy(self.model))
        # a bucket may go out once the LAST of its gradients is written: its lowest block number -- or the end of the backward
        self.bucket_ready = []
        for items in self.gbuf.layout:
            ms = [self.milestone[n] for n, *_ in items]
            self.bucket_ready.append(n_blocks if n_blocks in ms else min(ms))
        self.overlap = bool(overlap) and hasattr(engine, "train_wait_grads")
        self._comm = torch.cuda.Stream(device=dev) if (self.overlap and torch.device(dev).type == "cuda") else None
        self.steps = 0
        # the bf16 operand copies of the frozen parameters are built once and kept on the device (gl_train_weight_cache): this step
        # changes nothing but the tensors it asks gradients for, and load_state_dict drops the copies
        self.cache_frozen = bool(cache_frozen) and hasattr(engine, "train_weight_cache")
        if self.cache_frozen:
            engine.train_weight_cache(False)       # (copies keyed by the addresses of another TrainStep's tensors must not outlive them)
            engine.train_weight_cache(True)
        self._init_run(accumulate, max_grad_norm)

    def lr_at(self, step: int) -> float:
        return float(self.lr(step)) if callable(self.lr) else self.lr

    def _init_run(self, accumulate: int, max_grad_norm: Optional[float]) -> None:
        """Gradient accumulation and norm clipping (the constructor's accumulate / max_grad_norm; LoraTrainStep shares it): the extra
        bucket set when K > 1, the partial sums of every bucket side by side and the (norm, coefficient) pair when clipping."""
        if int(accumulate) != accumulate or int(accumulate) < 1:
            raise ValueError(f"TrainStep: accumulate {accumulate!r} is not a number of micro-batches >= 1")
        self.accumulate = int(accumulate)
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"TrainStep: max_grad_norm {max_grad_norm!r} is negative or NaN (None or 0: no clipping)")
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else None
        self.micro = 0                      # micro-batches of the current group already summed
        self.acc = [torch.zeros_like(b) for b in self.gbuf.buckets] if self.accumulate > 1 else None
        self.grad_norm = None               # with clipping: the norm BEFORE clipping of the last optimizer step's gradient, a device tensor [1]
        if self.max_grad_norm is not None:
            counts = [self.engine.grad_sqnorm_partials(b.numel()) for b in self.gbuf.buckets]
            self._partials = torch.zeros(sum(counts), device=self.engine.device, dtype=torch.float32)
            ends = [sum(counts[:i + 1]) for i in range(len(counts))]
            self._partial_slices = [self._partials[e - c:e] for c, e in zip(counts, ends)]
            self._clip = torch.zeros(2, device=self.engine.device, dtype=torch.float32)
            self.grad_norm, self._coef = self._clip[0:1], self._clip[1:2]

    @property
    def at_boundary(self) -> bool:
        """No group of micro-batches is open: the last call of step() took an optimizer step (or none was made yet)."""
        return self.micro == 0

    def step(self, batch: Mapping[str, torch.Tensor], fuser_scale: float = 1.0, loss_weights: Optional[torch.Tensor] = None):
        """One micro-batch: forward, loss, backward; with accumulate = K the gradients of calls 1 .. K - 1 of a group are summed and
        nothing else happens; call K (every call when K = 1) averages them, exchanges the average over the ranks and takes the
        optimizer step, clipped to max_grad_norm when set. Returns (loss of this rank and micro-batch, eps)."""
        if self.drop_prob > 0.0 and self.rng.random() < self.drop_prob:      # random drop for guidance (openaimodel.py:428)
            batch = null_grounding(batch)
        loss, eps = self._forward_backward(batch, fuser_scale) if loss_weights is None else self._forward_backward(batch, fuser_scale, loss_weights)
        nb = len(self.gbuf.buckets)
        K = self.accumulate
        if K > 1:
            self.micro += 1
            if self.micro < K:      # inside a group: the sum alone, behind the backward -- no collective (DDP's no_sync), no update
                for i in range(nb):
                    self.engine.op_grad_accumulate(self.acc[i], self.gbuf.buckets[i], "first" if self.micro == 1 else "middle", K)
                return loss, eps
            self.micro = 0
        self.steps += 1
        lr = self.lr_at(self.steps)
        clip = self.max_grad_norm is not None
        kw = dict(lr=lr, betas=self.betas, eps=self.eps, weight_decay=self.wd)
        if clip:                    # the same updates on g * coef; coef stays on the device
            kw["coef"] = self._coef
        if self.ema is None:
            op = self.engine.op_adamw_clip_step if clip else self.engine.op_adamw_step
            upd = lambda i: op(self.pbuf.buckets[i], self.gbuf.buckets[i], self.m[i], self.v[i], self.steps, **kw)
        else:       # AdamW and the EMA of the updated parameters in one pass over the bucket
            op = self.engine.op_adamw_ema_clip_step if clip else self.engine.op_adamw_ema_step
            upd = lambda i: op(self.pbuf.buckets[i], self.gbuf.buckets[i], self.m[i], self.v[i], self.ema[i], self.steps, ema_rate=self.ema_rate, **kw)
        alone = self.exchange_even_alone

        def exchange(i):            # bucket i: the mean over the group into the gradient buffer, the mean over the ranks, its share of the norm
            if K > 1:
                self.engine.op_grad_accumulate(self.acc[i], self.gbuf.buckets[i], "last", K)
            self.gbuf.all_reduce_bucket(i, average=True, even_alone=alone)
            if clip:
                self.engine.op_grad_sqnorm(self.gbuf.buckets[i], self._partial_slices[i])

        def clipped_updates():      # a global norm: every update waits for the last bucket's share
            self.engine.op_clip_coef(self._partials, self.max_grad_norm, self._clip)
            for i in range(nb):
                upd(i)

        if not self.overlap:                        # backward, every collective, every update: one stream
            for i in range(nb):
                exchange(i)
            if clip:
                clipped_updates()
            else:
                for i in range(nb):
                    upd(i)
        elif self._comm is None:                    # (a host-side engine: the same per-bucket order without streams)
            for i in range(nb):
                self.engine.train_wait_grads(self.bucket_ready[i], None)
                exchange(i)
                if not clip:
                    upd(i)
            if clip:
                clipped_updates()
        else:
            main = torch.cuda.current_stream(self.engine.device)
            for i in range(nb):                     # bucket i: wait for its last gradient only, exchange, update -- all behind the backward
                self.engine.train_wait_grads(self.bucket_ready[i], self._comm)
                with torch.cuda.stream(self._comm):
                    exchange(i)
                    if not clip:
                        upd(i)
            if clip:                                # (the exchanges and the norm passes ran under the backward; the updates cannot)
                with torch.cuda.stream(self._comm):
                    clipped_updates()
            main.wait_stream(self._comm)            # the next forward reads the updated parameters
        return loss, eps

    def _forward_backward(self, batch, fuser_scale, loss_weights=None):
        """Forward, loss and backward into the gradient buckets: (loss, eps). (gligen_amd.lora_train.LoraTrainStep passes its adapters.)"""
        kw = dict(use_weight_cache=True) if self.cache_frozen else {}
        if loss_weights is not None:
            kw["loss_weights"] = loss_weights
        loss, eps, _ = self.engine.unet_train_step(self.cfg, self.params, batch, fuser_scale=fuser_scale, grads=self.gbuf.views, checkpoint=self.checkpoint, **kw)
        return loss, eps

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: v.clone() for k, v in self.params.items()}

    def optimizer_state_dict(self) -> Dict[str, object]:
        """What a resumed run needs beside the parameters (the reference's checkpoint carries opt, scheduler and iters,
        trainer.py:472-484): AdamW's two moments per trainable tensor and the step count (which also positions the LR schedule)."""
        m, v = {}, {}
        for items, mb, vb in zip(self.pbuf.layout, self.m, self.v):
            for name, off, n, shape in items:
                m[name] = mb[off:off + n].view(shape).clone()
                v[name] = vb[off:off + n].view(shape).clone()
        return {"steps": int(self.steps), "exp_avg": m, "exp_avg_sq": v}

    def load_optimizer_state_dict(self, state: Mapping[str, object]) -> None:
        for items, mb, vb in zip(self.pbuf.layout, self.m, self.v):
            for name, off, n, shape in items:
                mb[off:off + n].view(shape).copy_(state["exp_avg"][name])
                vb[off:off + n].view(shape).copy_(state["exp_avg_sq"][name])
        self.steps = int(state["steps"])
        self.micro = 0

    def _slices(self, bufs):
        """name -> the view of `bufs` (a buffer set in the bucket layout) that belongs to that trainable tensor."""
        return {name: b[off:off + n].view(shape) for items, b in zip(self.pbuf.layout, bufs) for name, off, n, shape in items}

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's ckpt["ema"] (trainer.py:481-482): a full state_dict in the order of the parameters; the trainable tensors
        come from the EMA buffers. Deviation from the reference: it averages the frozen tensors too, which never change, so their
        average is themselves up to the rounding jitter of rate * x + (1 - rate) * x; here the frozen tensors ARE the parameters."""
        if self.ema is None:
            raise ValueError("ema_state_dict: this TrainStep keeps no EMA (ema_rate=None)")
        ema = self._slices(self.ema)
        return {k: (ema[k] if k in ema else v).clone() for k, v in self.params.items()}

    def load_ema_state_dict(self, state_dict: Mapping[str, torch.Tensor]) -> None:
        """The inverse of ema_state_dict: the trainable tensors of `state_dict` into the EMA buffers (the frozen ones are not kept)."""
        if self.ema is None:
            raise ValueError("load_ema_state_dict: this TrainStep keeps no EMA (ema_rate=None)")
        for k, view in self._slices(self.ema).items():
            if k not in state_dict:
                raise ValueError(f"load_ema_state_dict: '{k}' is missing")
            if tuple(state_dict[k].shape) != tuple(view.shape):
                raise ValueError(f"load_ema_state_dict: '{k}' is {tuple(state_dict[k].shape)}, the model's is {tuple(view.shape)}")
            view.copy_(state_dict[k].to(device=view.device, dtype=torch.float32))

    def torch_optimizer_state_dict(self, initial_lr: Optional[float] = None) -> Dict[str, object]:
        """The optimizer in the layout of torch.optim.AdamW.state_dict(), the reference's ckpt["opt"] (trainer.py:245, 476):
        state[i] = {step, exp_avg, exp_avg_sq} (CPU tensors) and one param group with params = [0 .. n-1], where i numbers the
        trainable tensors in the order of the state_dict this step was built from (the reference's named_parameters() order). The
        keys and the type of `step` are read off a real torch.optim.AdamW over stand-in tensors, so they follow the installed
        torch. lr is the rate of the NEXT step (what a LambdaLR has left in the group after its scheduler.step()); initial_lr, when
        given, is added as the schedulers do. Before the first step `state` is empty, as torch's is."""
        n = len(self.param_order)
        stand = [torch.nn.Parameter(torch.zeros(1)) for _ in range(n)]
        opt = torch.optim.AdamW(stand, lr=self.lr_at(self.steps + 1), betas=self.betas, eps=self.eps, weight_decay=self.wd)
        if self.steps > 0:
            for q in stand:
                q.grad = torch.zeros(1)
            opt.step()          # materialises every state entry with this torch's keys
        out = opt.state_dict()
        m, v = self._slices(self.m), self._slices(self.v)
        for i, name in enumerate(self.param_order):
            st = out["state"].get(i)
            if st is None:
                continue
            extra = set(st) - {"step", "exp_avg", "exp_avg_sq"}
            if extra:
                raise RuntimeError(f"torch_optimizer_state_dict: this torch's AdamW keeps {sorted(extra)}, which the step does not have")
            st["step"] = torch.full_like(st["step"], self.steps) if torch.is_tensor(st["step"]) else int(self.steps)
            st["exp_avg"], st["exp_avg_sq"] = m[name].detach().cpu().clone(), v[name].detach().cpu().clone()
        if initial_lr is not None:
            out["param_groups"][0]["initial_lr"] = float(initial_lr)
        return out

    def load_torch_optimizer_state_dict(self, state: Mapping[str, object]) -> None:
        """The inverse: what torch.optim.AdamW.state_dict() of the reference's trainer, or torch_optimizer_state_dict, holds. As
        torch's load_state_dict does, the group's betas / eps / weight_decay replace this step's, and its lr when this step's rate is
        a constant (a schedule stays: `steps` positions it). A count or shape mismatch is a ValueError that names the tensor."""
        groups = state["param_groups"]
        ids = [i for g in groups for i in g["params"]]
        n = len(self.param_order)
        if len(ids) != n:
            odd = self.param_order[len(ids)] if len(ids) < n else f"parameter {n} of the saved optimizer"
            raise ValueError(f"load_torch_optimizer_state_dict: {len(ids)} parameters saved, {n} trainable tensors here (first without a partner: {odd})")
        saved = state["state"]
        m, v = self._slices(self.m), self._slices(self.v)
        steps = set()
        for name, i in zip(self.param_order, ids):
            st = saved.get(i)
            if st is None:          # torch keeps no entry for a parameter that never had a gradient
                m[name].zero_(); v[name].zero_()
                continue
            for key, dst in (("exp_avg", m[name]), ("exp_avg_sq", v[name])):
                if tuple(st[key].shape) != tuple(dst.shape):
                    raise ValueError(f"load_torch_optimizer_state_dict: {key} of parameter {i} is {tuple(st[key].shape)}, '{name}' is {tuple(dst.shape)}")
                dst.copy_(st[key].to(device=dst.device, dtype=torch.float32))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"load_torch_optimizer_state_dict: the parameters are at different steps {sorted(steps)}; this step keeps one count")
        self.steps = steps.pop() if steps else 0
        self.micro = 0
        g0 = groups[0]
        self.betas, self.eps, self.wd = tuple(float(b) for b in g0["betas"]), float(g0["eps"]), float(g0["weight_decay"])
        if not callable(self.lr):
            self.lr = float(g0["lr"])

    def load_state_dict(self, state_dict: Mapping[str, torch.Tensor]) -> None:
        """Parameters back into the flat buffers (trainable) / the frozen set, in place: the views the engine reads stay the same."""
        for k, t in state_dict.items():
            self.params[k].copy_(t.to(device=self.params[k].device, dtype=torch.float32))
        self.micro = 0                     # (an open group of micro-batches belonged to the parameters just replaced)
        if self.cache_frozen:              # frozen tensors may have changed under the cached operand copies
            self.engine.train_weight_cache(False)
            self.engine.train_weight_cache(True)
