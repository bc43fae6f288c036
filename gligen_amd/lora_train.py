"""Training LoRA adapters for a GLIGEN model on MI355X: the adapters' counterpart of gligen_amd.train.TrainStep.

An adapter sits on a frozen Linear of a SpatialTransformer -- attn1 / attn2 .to_q / .to_k / .to_v / .to_out.0 (family "attn"),
ff.net.0.proj / ff.net.2 (family "ff"), proj_in / proj_out (family "proj": 1 x 1 convs, run as Linears over pixel rows); the families
are the words gligen_amd.synthetic.LORA_FAMILIES and tools/make_synthetic_lora.py use -- and the layer computes
x W^T + (alpha / rank) (x down^T) up^T. down is initialised Kaiming-uniform and up zero, as kohya's networks/lora.py does, so the first
step's forward is the base model's. The fuser's own Linears train in full (TrainStep) and take no adapter.

Everything numeric runs in the library: forward + backward in gl_unet_train_step_lora (the low-rank products on the fp32-input MFMA,
csrc/train_lora.hip), the update in gl_op_adamw_step. The adapter tensors and their gradients are views into GradBuckets, laid out in
the order the gradients become final, exactly as TrainStep's; an adapter's gradients are final at the milestone of its
SpatialTransformer. What comes out is kohya's file format (adapter_state_dict / save_adapter), which `--lora` and
gligen_amd.lora.apply_loras consume.

The convolutional side (kohya's conv_dim / LoCon) comes in through LoraSpec's conv_families: "conv" (a ResBlock's in_layers.2,
out_layers.3 and skip_connection), "emb" (emb_layers.1) and "sample" (a Downsample's op, an Upsample's conv), meaning what
synthetic.LORA_FAMILIES means by them. A 3 x 3 site computes conv(x, W) + (conv_alpha / conv_rank) up(down(x)) with down
[conv_rank, Ci, 3, 3] of the base conv's stride and padding and up 1 x 1 (csrc/train_lora_conv.hip); skip_connection and emb_layers.1
are Linears and take rank / alpha. Their gradients are final at the last milestone of the step."""
from __future__ import annotations

import math
import random
import zlib
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Union

import torch
import torch.distributed as tdist

from . import lora
from .dist import GradBuckets
from .train import TrainStep, _block_order, trainable_names

FAMILY_SUFFIXES = {
    "attn": tuple(f".transformer_blocks.0.{a}.{p}.weight" for a in ("attn1", "attn2") for p in ("to_q", "to_k", "to_v", "to_out.0")),
    "ff": (".transformer_blocks.0.ff.net.0.proj.weight", ".transformer_blocks.0.ff.net.2.weight"),
    "proj": (".proj_in.weight", ".proj_out.weight"),
}
CONV_FAMILY_SUFFIXES = {
    "conv": (".in_layers.2.weight", ".out_layers.3.weight", ".skip_connection.weight"),
    "emb": (".emb_layers.1.weight",),
    "sample": (".op.weight", ".conv.weight"),
}
MAX_RANK = 128          # the low-rank kernels' limit
DOWN, UP = ".lora_down.weight", ".lora_up.weight"


class LoraSpec:
    """rank, alpha (None: rank, so that the scale alpha / rank is 1) and the families adapted; conv_families: the ResBlock and
    resampling sites (CONV_FAMILY_SUFFIXES), whose 3 x 3 convs take conv_rank (None: rank) and conv_alpha (None: conv_rank) while
    skip_connection and emb_layers.1 take rank / alpha. families may be empty when conv_families is not."""

    def __init__(self, rank: int, alpha: Optional[float] = None, families: Sequence[str] = ("attn",), *, conv_families: Sequence[str] = (),
                 conv_rank: Optional[int] = None, conv_alpha: Optional[float] = None):
        self.rank = int(rank)
        if not 1 <= self.rank <= MAX_RANK:
            raise ValueError(f"LoraSpec: rank {rank} (1 <= rank <= {MAX_RANK})")
        self.alpha = float(self.rank if alpha is None else alpha)
        self.families = tuple(families)
        self.conv_families = tuple(conv_families)
        bad = [f for f in self.families if f not in FAMILY_SUFFIXES]
        if bad or not (self.families or self.conv_families):
            raise ValueError(f"LoraSpec: families {bad or '()'}: some of {sorted(FAMILY_SUFFIXES)}")
        bad = [f for f in self.conv_families if f not in CONV_FAMILY_SUFFIXES]
        if bad:
            raise ValueError(f"LoraSpec: conv_families {bad}: some of {sorted(CONV_FAMILY_SUFFIXES)}")
        self.conv_rank = int(self.rank if conv_rank is None else conv_rank)
        if not 1 <= self.conv_rank <= MAX_RANK:
            raise ValueError(f"LoraSpec: conv_rank {conv_rank} (1 <= conv_rank <= {MAX_RANK})")
        self.conv_alpha = float(self.conv_rank if conv_alpha is None else conv_alpha)

    @property
    def scale(self) -> float:
        return self.alpha / self.rank

    @property
    def conv_scale(self) -> float:
        return self.conv_alpha / self.conv_rank

    def of_site(self, w) -> tuple:
        """(rank, alpha) of the adapter on weight w (anything with .shape): a 3 x 3 conv takes the conv pair."""
        return (self.conv_rank, self.conv_alpha) if _is_conv3(w) else (self.rank, self.alpha)

    def __repr__(self):
        conv = f", conv_families={self.conv_families}, conv_rank={self.conv_rank}, conv_alpha={self.conv_alpha:g}" if self.conv_families else ""
        return f"LoraSpec(rank={self.rank}, alpha={self.alpha:g}, families={self.families}{conv})"


def _is_conv3(w) -> bool:
    shape = tuple(int(s) for s in w.shape)
    return len(shape) == 4 and shape[2:] == (3, 3)


def st_prefixes(state_dict: Mapping[str, object]) -> List[str]:
    """The SpatialTransformers of a state_dict in module order: the numbering of gl_unet_train_step's gradient milestones."""
    return sorted({k.split(".transformer_blocks.")[0] for k in state_dict if ".transformer_blocks." in k}, key=_block_order)


def adapter_sites(state_dict: Mapping[str, object], spec: LoraSpec) -> List[str]:
    """The state_dict keys of the weights `spec` adapts, in the order of the state_dict."""
    sts = set(st_prefixes(state_dict))
    suffixes = tuple(s for f in spec.families for s in FAMILY_SUFFIXES[f])
    conv_suffixes = tuple(s for f in spec.conv_families for s in CONV_FAMILY_SUFFIXES[f])
    out = []
    for k in state_dict:
        if ".fuser." in k:
            continue
        if suffixes and k.endswith(suffixes):
            prefix = k.split(".transformer_blocks.")[0] if ".transformer_blocks." in k else k.rsplit(".", 2)[0]
            if prefix in sts:
                out.append(k)
        elif conv_suffixes and k.endswith(conv_suffixes) and ".transformer_blocks." not in k and k.startswith(("input_blocks.", "middle_block.", "output_blocks.")):
            out.append(k)
    return out


def _site_shape(w) -> tuple:
    """(N, K) of a Linear's [N, K] or a 1 x 1 conv's [N, K, 1, 1] weight, (Co, Ci) of a 3 x 3 conv's [Co, Ci, 3, 3]."""
    shape = tuple(int(s) for s in w.shape)
    if len(shape) not in (2, 4) or (any(s != 1 for s in shape[2:]) and shape[2:] != (3, 3)):
        raise ValueError(f"an adapted weight is [N, K], [N, K, 1, 1] or [Co, Ci, 3, 3]; got {shape}")
    return shape[0], shape[1]


def init_adapters(state_dict: Mapping[str, object], cfg: Optional[Mapping], spec: LoraSpec, seed: int = 0) -> Dict[str, torch.Tensor]:
    """`<module path>.lora_down.weight` [rank, K] and `.lora_up.weight` [N, rank] (fp32, CPU) for every site of `spec`, in module
    order: down Kaiming-uniform (a = sqrt(5): uniform in +-1 / sqrt(K)), up zero (kohya networks/lora.py); a 3 x 3 conv's down is
    [conv_rank, Ci, 3, 3] with fan-in 9 Ci, its up [Co, conv_rank]. Seeded per module, so a site's start does not depend on which other
    families are adapted. state_dict: tensors, or anything with .shape."""
    out: Dict[str, torch.Tensor] = {}
    for k in adapter_sites(state_dict, spec):
        N, K = _site_shape(state_dict[k])
        if K % 64 or N % 64:
            raise ValueError(f"init_adapters: '{k}' is [{N}, {K}]; the low-rank kernels take K and N that are multiples of 64")
        path = k[:-len(".weight")]
        gen = torch.Generator().manual_seed((zlib.crc32(path.encode()) ^ (int(seed) * 0x9E3779B1)) & 0x7FFFFFFF)
        conv3 = _is_conv3(state_dict[k])
        rank, _ = spec.of_site(state_dict[k])
        bound = 1.0 / math.sqrt(9 * K if conv3 else K)
        out[path + DOWN] = (torch.rand((rank, K, 3, 3) if conv3 else (rank, K), generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound
        out[path + UP] = torch.zeros((N, rank), dtype=torch.float32)
    if not out:
        raise ValueError(f"init_adapters: no weight of the families {spec.families + spec.conv_families} in this state_dict")
    return out


def kohya_state_dict(adapters: Mapping[str, torch.Tensor], state_dict: Mapping[str, object], alpha: float, dtype=torch.float32,
                     conv_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """Adapter tensors (init_adapters' keys) in kohya's form: lora_unet_<module path with underscores>.lora_down.weight /
    .lora_up.weight / .alpha; the factors of a conv (proj_in / proj_out, skip_connection) are 4-D with 1 x 1 tails; a 3 x 3 conv's
    down is saved as it is, its up with a (1, 1) tail and conv_alpha (None: alpha) as its .alpha."""
    out: Dict[str, torch.Tensor] = {}
    for key, down in adapters.items():
        if not key.endswith(DOWN):
            continue
        path = key[:-len(DOWN)]
        up = adapters[path + UP]
        w = state_dict[path + ".weight"]
        tail = (1, 1) if len(tuple(w.shape)) == 4 else ()
        conv3 = _is_conv3(w)
        name = lora.UNET_PREFIX + path.replace(".", "_")
        out[name + DOWN] = down.detach().reshape(tuple(down.shape) + (() if conv3 else tail)).to(dtype).cpu().contiguous()
        out[name + UP] = up.detach().reshape(tuple(up.shape) + tail).to(dtype).cpu().contiguous()
        out[name + ".alpha"] = torch.tensor(float(alpha if (conv_alpha is None or not conv3) else conv_alpha), dtype=dtype)
    return out


def adapter_milestones(names: Sequence[str], state_dict: Mapping[str, object]) -> Dict[str, int]:
    """The gradient milestone of every trainable tensor of a LoraTrainStep: an adapter tensor's and a fuser tensor's is the number of
    its SpatialTransformer in module order, every other tensor's (position_net, the first conv; the adapters of the conv families, on
    ResBlocks and resampling layers) the number of SpatialTransformers: the last milestone, recorded behind the whole backward."""
    sts = st_prefixes(state_dict)
    index = {p: i for i, p in enumerate(sts)}

    def of(k):
        if ".transformer_blocks." in k:
            return index[k.split(".transformer_blocks.")[0]]
        if k.endswith((DOWN, UP)):
            return index.get(k.rsplit(".", 3)[0], len(sts))       # <st>.proj_in.lora_down.weight; a conv-family site is in no SpatialTransformer
        return len(sts)
    return {k: of(k) for k in names}


class LoraTrainStep(TrainStep):
    """TrainStep over LoRA adapters: the same buckets, milestones, overlap schedule, AdamW launches and LR schedules, with
    `spec`'s adapters (or `adapters`: tensors under init_adapters' keys, e.g. of a checkpoint) as the trainable set. train_base=False
    (default) trains the adapters alone -- the fusers and position_net are frozen and, like every other base tensor, served from the
    frozen-weight operand cache --; True also trains the reference's set (train.trainable_names). The base state_dict is never
    changed by adapter-only training. No EMA of the adapters is kept."""

    def __init__(self, engine, cfg: Mapping, state_dict: Mapping[str, torch.Tensor], spec: LoraSpec, lr: Union[float, Callable[[int], float]] = 1e-4,
                 weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, bucket_mb: float = 128.0, world: Optional[int] = None,
                 checkpoint: bool = True, drop_prob: float = 0.0, rng: Optional[random.Random] = None, broadcast: bool = True, overlap: bool = True,
                 cache_frozen: bool = True, train_base: bool = False, seed: int = 0, adapters: Optional[Mapping[str, torch.Tensor]] = None,
                 accumulate: int = 1, max_grad_norm: Optional[float] = None):
        self.engine, self.cfg, self.spec = engine, dict(cfg), spec
        self.exchange_even_alone = False
        dev = engine.device
        self.lr = lr if callable(lr) else float(lr)
        self.wd, self.betas, self.eps = float(weight_decay), tuple(betas), float(eps)
        self.drop_prob, self.rng = float(drop_prob), rng or random.Random()
        self.checkpoint = bool(checkpoint)
        self.train_base = bool(train_base)
        start = init_adapters(state_dict, self.cfg, spec, seed) if adapters is None else {k: adapters[k] for k in init_adapters(state_dict, self.cfg, spec, seed)}
        self.sites = adapter_sites(state_dict, spec)
        self.base_names = trainable_names(state_dict, self.cfg) if self.train_base else []
        names = list(self.base_names) + list(start)
        self.param_order = list(names)
        self.milestone = adapter_milestones(names, state_dict)
        n_blocks = len(st_prefixes(state_dict))
        n_st = getattr(engine, "count_spatial_transformers", None)
        if callable(n_st) and n_st(self.cfg) != n_blocks:
            raise ValueError(f"LoraTrainStep: {n_blocks} SpatialTransformers in the state_dict, {n_st(self.cfg)} in the config")
        names = sorted(names, key=lambda k: (self.milestone[k] == n_blocks, -self.milestone[k]))
        shapes = {k: tuple(start[k].shape) if k in start else tuple(state_dict[k].shape) for k in names}
        self.pbuf = GradBuckets(shapes, bucket_mb, world, device=dev)
        self.gbuf = GradBuckets(shapes, bucket_mb, world, device=dev)
        self.m = [torch.zeros_like(b) for b in self.pbuf.buckets]
        self.v = [torch.zeros_like(b) for b in self.pbuf.buckets]
        self.params: Dict[str, torch.Tensor] = {}
        for k, t in state_dict.items():
            t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            if k in shapes:
                self.pbuf.views[k].copy_(t)
                self.params[k] = self.pbuf.views[k]
            else:
                self.params[k] = t
        for k, t in start.items():
            if tuple(t.shape) != shapes[k]:
                raise ValueError(f"LoraTrainStep: adapter tensor '{k}' is {tuple(t.shape)}, {spec} on this model gives {shapes[k]}")
            self.pbuf.views[k].copy_(t.to(device=dev, dtype=torch.float32))
        if broadcast and tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            for b in self.pbuf.buckets:
                tdist.broadcast(b, src=0)
        self.ema_rate, self.ema = None, None
        self.bucket_ready = []
        for items in self.gbuf.layout:
            ms = [self.milestone[n] for n, *_ in items]
            self.bucket_ready.append(n_blocks if n_blocks in ms else min(ms))
        self.overlap = bool(overlap) and hasattr(engine, "train_wait_grads")
        self._comm = torch.cuda.Stream(device=dev) if (self.overlap and torch.device(dev).type == "cuda") else None
        self.steps = 0
        self.cache_frozen = bool(cache_frozen) and hasattr(engine, "train_weight_cache")
        if self.cache_frozen:
            engine.train_weight_cache(False)
            engine.train_weight_cache(True)
        # what the engine takes: one entry per adapted weight, the tensors views into the parameter / gradient buckets
        self.adapters = []
        for w in self.sites:
            path = w[:-len(".weight")]
            self.adapters.append(dict(name=w, down=self.pbuf.views[path + DOWN], up=self.pbuf.views[path + UP], g_down=self.gbuf.views[path + DOWN],
                                      g_up=self.gbuf.views[path + UP], scale=spec.conv_scale if _is_conv3(state_dict[w]) else spec.scale))
        self._base_grads = {k: self.gbuf.views[k] for k in self.base_names}
        self._init_run(accumulate, max_grad_norm)     # gradient accumulation and norm clipping, as TrainStep's

    def _forward_backward(self, batch, fuser_scale, loss_weights=None):
        kw = dict(use_weight_cache=True) if self.cache_frozen else {}
        if loss_weights is not None:
            kw["loss_weights"] = loss_weights
        loss, eps, _, _ = self.engine.unet_train_step(self.cfg, self.params, batch, fuser_scale=fuser_scale, grads=self._base_grads, checkpoint=self.checkpoint,
                                                      adapters=self.adapters, **kw)
        return loss, eps

    # ---- the adapters
    def adapter_tensors(self) -> Dict[str, torch.Tensor]:
        """The adapter tensors under init_adapters' keys (clones, on the device), in module order."""
        return {k: self.pbuf.views[k].clone() for k in self.param_order if k.endswith((DOWN, UP))}

    def adapter_grads(self) -> Dict[str, torch.Tensor]:
        """The gradients the last step left in the buckets (after the exchange: the average over the ranks), by the same keys."""
        return {k: self.gbuf.views[k].clone() for k in self.param_order if k.endswith((DOWN, UP))}

    def load_adapter_tensors(self, tensors: Mapping[str, torch.Tensor]) -> None:
        for k in self.param_order:
            if not k.endswith((DOWN, UP)):
                continue
            if k not in tensors:
                raise ValueError(f"load_adapter_tensors: '{k}' is missing")
            if tuple(tensors[k].shape) != tuple(self.pbuf.views[k].shape):
                raise ValueError(f"load_adapter_tensors: '{k}' is {tuple(tensors[k].shape)}, this step's is {tuple(self.pbuf.views[k].shape)}")
            self.pbuf.views[k].copy_(tensors[k].to(device=self.pbuf.views[k].device, dtype=torch.float32))
        self.micro = 0          # (an open group of micro-batches belonged to the adapters just replaced)

    def adapter_state_dict(self, dtype=torch.float32) -> Dict[str, torch.Tensor]:
        """The adapter in kohya's form (CPU tensors): what gligen_amd.lora.parse_adapter / apply_loras and `--lora` read."""
        return kohya_state_dict(self.adapter_tensors(), self.params, self.spec.alpha, dtype, conv_alpha=self.spec.conv_alpha)

    def save_adapter(self, path, dtype=torch.float16) -> None:
        """The adapter as a .safetensors file (gligen_amd.lora.write_safetensors), fp16 as adapters are usually shared, or fp32."""
        if dtype not in (torch.float16, torch.float32):
            raise ValueError("save_adapter: dtype is torch.float16 or torch.float32")
        meta = dict(ss_network_dim=str(self.spec.rank), ss_network_alpha=f"{self.spec.alpha:g}", ss_network_module="networks.lora",
                    families=" ".join(self.spec.families), steps=str(self.steps))
        if self.spec.conv_families:
            meta.update(conv_families=" ".join(self.spec.conv_families), ss_network_args=f"conv_dim={self.spec.conv_rank} conv_alpha={self.spec.conv_alpha:g}")
        lora.write_safetensors(path, self.adapter_state_dict(dtype), metadata=meta)

    def ema_state_dict(self):
        raise ValueError("LoraTrainStep keeps no EMA")

    def load_ema_state_dict(self, state_dict):
        raise ValueError("LoraTrainStep keeps no EMA")
