"""LoRA adapters in kohya's format for the GLIGEN UNet and the CLIP text tower: read, resolve, merge on the device, stack, remove.

An adapter is merged into the modules' fp32 parameters in place (Engine.op_lora_merge = gl_op_lora_merge, on the weight-less scratch
engine of the device) and the packed bf16 engines are dropped, so the next call rebuilds them from the merged parameters: every packed
form (folded LayerNorms, GEGLU and row-local streams, phase convs), the execution lanes, the second-pass forks and the training weight
cache follow without any of them knowing about adapters. The originals of the touched tensors are kept on the host, so a second list of
adapters starts from them and remove_loras() gives them back bit for bit.

File format: `<module>.lora_down.weight` [r, K...], `<module>.lora_up.weight` [N, r(, 1, 1)] and an optional `<module>.alpha`; the
effective scale is user_scale * alpha / r (user_scale without alpha). The container is safetensors, read and written here (8-byte
little-endian header length, JSON header, raw little-endian data; F32, F16, BF16) -- the safetensors package is not needed --, or a
torch.load-able file, or a plain dict of tensors."""
from __future__ import annotations

import json
import os
import struct
import time
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch
from torch import nn


class LoraError(ValueError):
    """An adapter that is refused: the message names what and why. Nothing has been modified when it is raised."""


# ---- the safetensors container ---------------------------------------------------------------------------------------------------
SAFETENSORS_DTYPES = {"F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16}
_DTYPE_NAMES = {v: k for k, v in SAFETENSORS_DTYPES.items()}
_MAX_HEADER = 100 << 20       # the format's own limit on the JSON header


def write_safetensors(path, tensors: Mapping[str, torch.Tensor], metadata: Optional[Mapping[str, str]] = None) -> None:
    """Write `tensors` (F32, F16 or BF16; any shape, scalars included) as a safetensors file: tensors in name order, the header padded
    with spaces to a multiple of 8 bytes."""
    header, blobs, offset = {}, [], 0
    if metadata:
        header["__metadata__"] = {str(k): str(v) for k, v in metadata.items()}
    for name in sorted(tensors):
        t = tensors[name]
        if not torch.is_tensor(t) or t.dtype not in _DTYPE_NAMES:
            raise LoraError(f"write_safetensors: tensor {name!r} is {getattr(t, 'dtype', type(t).__name__)}; F32, F16 and BF16 are written")
        raw = t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        header[name] = {"dtype": _DTYPE_NAMES[t.dtype], "shape": [int(s) for s in t.shape], "data_offsets": [offset, offset + len(raw)]}
        blobs.append(raw)
        offset += len(raw)
    text = json.dumps(header, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(text)))
        f.write(text)
        for raw in blobs:
            f.write(raw)


def read_safetensors(path) -> Dict[str, torch.Tensor]:
    """The tensors of a safetensors file, on the host in their stored dtype. Refused by name: a file shorter than its header or its
    data says (truncated), a header that is not a JSON object, a dtype other than F32 / F16 / BF16, offsets that do not fit the shape."""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < 8:
        raise LoraError(f"{path}: truncated safetensors file ({len(blob)} bytes, the header length alone takes 8)")
    (n,) = struct.unpack("<Q", blob[:8])
    if n > _MAX_HEADER:
        raise LoraError(f"{path}: not a safetensors file (a header of {n} bytes)")
    if 8 + n > len(blob):
        raise LoraError(f"{path}: truncated safetensors file (the header has {n} bytes, {len(blob) - 8} follow its length)")
    try:
        header = json.loads(blob[8:8 + n].decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise LoraError(f"{path}: the safetensors header is not JSON ({e})") from None
    if not isinstance(header, dict):
        raise LoraError(f"{path}: the safetensors header is not a JSON object")
    data = memoryview(blob)[8 + n:]
    out = {}
    for name, info in header.items():
        if name == "__metadata__":
            continue
        try:
            dtype_name, shape, (lo, hi) = info["dtype"], [int(s) for s in info["shape"]], info["data_offsets"]
        except (KeyError, TypeError, ValueError):
            raise LoraError(f"{path}: tensor {name!r} has a malformed header entry {info!r}") from None
        if dtype_name not in SAFETENSORS_DTYPES:
            raise LoraError(f"{path}: tensor {name!r} has unknown dtype {dtype_name!r}; F32, F16 and BF16 are read")
        dtype = SAFETENSORS_DTYPES[dtype_name]
        numel = 1
        for s in shape:
            numel *= s
        if lo < 0 or hi < lo or hi - lo != numel * dtype.itemsize:
            raise LoraError(f"{path}: tensor {name!r} of shape {shape} and dtype {dtype_name} does not fit its data_offsets {[lo, hi]}")
        if hi > len(data):
            raise LoraError(f"{path}: truncated safetensors file (tensor {name!r} ends at byte {hi} of the data, {len(data)} are there)")
        if numel == 0:
            out[name] = torch.empty(shape, dtype=dtype)
        else:
            out[name] = torch.frombuffer(bytearray(data[lo:hi]), dtype=dtype).reshape(shape)
    return out


def _looks_like_safetensors(path) -> bool:
    with open(path, "rb") as f:
        head = f.read(9)
    if str(path).endswith(".safetensors"):
        return True
    return len(head) == 9 and struct.unpack("<Q", head[:8])[0] <= _MAX_HEADER and head[8:9] == b"{"


def load_adapter(source) -> Dict[str, torch.Tensor]:
    """An adapter's tensors by name: from a dict of tensors (taken as it is), a safetensors file or a torch.load-able file (a
    state dict, or a dict that holds one under "state_dict")."""
    if isinstance(source, Mapping):
        state = dict(source)
    else:
        path = os.fspath(source)
        if not os.path.isfile(path):
            raise LoraError(f"LoRA file {path!r} does not exist")
        if _looks_like_safetensors(path):
            state = read_safetensors(path)
        else:
            state = torch.load(path, map_location="cpu", weights_only=True)
            if isinstance(state, Mapping) and isinstance(state.get("state_dict"), Mapping):
                state = state["state_dict"]
            if not isinstance(state, Mapping):
                raise LoraError(f"{path}: holds a {type(state).__name__}, not a dict of tensors")
            state = dict(state)
    bad = [k for k, v in state.items() if not isinstance(k, str) or not torch.is_tensor(v)]
    if bad:
        raise LoraError(f"{_label(source)}: entries that are not named tensors: {bad[:10]}")
    return state


def _label(source) -> str:
    return f"<dict of {len(source)} tensors>" if isinstance(source, Mapping) else os.fspath(source)


# ---- kohya's format ------------------------------------------------------------------------------------------------------------
UNSUPPORTED_FORMS = {"hada_": "LoHa (Hadamard product) factors", "lokr_": "LoKr (Kronecker product) factors",
                     "lora_mid": "a Tucker / LoCon middle factor", "dora_scale": "DoRA magnitudes"}
FIRST_CONV_NAMES = ("lora_unet_conv_in", "lora_unet_input_blocks_0_0")
UNET_PREFIX, TE_PREFIX = "lora_unet_", "lora_te_"


class LoraEntry:
    """One `<module>.lora_down.weight` / `.lora_up.weight` (/ `.alpha`) group: down [r, K...], up [N, r(, 1, 1)], the stored alpha or
    None, and factor = alpha / r (1 without alpha), what the user's scale is multiplied by."""
    __slots__ = ("name", "down", "up", "alpha", "rank", "factor")

    def __init__(self, name, down, up, alpha):
        self.name, self.down, self.up, self.alpha = name, down, up, alpha
        self.rank = int(down.shape[0])
        self.factor = 1.0 if alpha is None else float(alpha) / self.rank

    @property
    def is_te(self):
        return self.name.startswith(TE_PREFIX)


def parse_adapter(state: Mapping[str, torch.Tensor], label: str = "adapter") -> List[LoraEntry]:
    """The pairs of an adapter in name order. Refused by name: LyCORIS forms that are not implemented, tensors that belong to no pair,
    a module with one half of its pair, factors whose ranks disagree, a file with no pair at all."""
    for key in state:
        for mark, what in UNSUPPORTED_FORMS.items():
            if mark in key:
                raise LoraError(f"{label}: tensor {key!r} holds {what}; only plain LoRA pairs (lora_down / lora_up / alpha) are implemented")
    groups: Dict[str, Dict[str, torch.Tensor]] = {}
    unknown = []
    for key, t in state.items():
        module, _, rest = key.partition(".")
        if rest in ("lora_down.weight", "lora_up.weight", "alpha"):
            groups.setdefault(module, {})[rest] = t
        else:
            unknown.append(key)
    if not any("lora_down.weight" in g and "lora_up.weight" in g for g in groups.values()):
        raise LoraError(f"{label}: no LoRA pair (<module>.lora_down.weight + <module>.lora_up.weight) among its {len(state)} tensors")
    if unknown:
        raise LoraError(f"{label}: tensors that belong to no LoRA pair: {sorted(unknown)[:10]}")
    entries = []
    for module in sorted(groups):
        g = groups[module]
        if "lora_down.weight" not in g or "lora_up.weight" not in g:
            raise LoraError(f"{label}: module {module!r} has {sorted(g)} but not both lora_down.weight and lora_up.weight")
        down, up = g["lora_down.weight"], g["lora_up.weight"]
        if down.dim() < 2 or up.dim() < 2 or int(down.shape[0]) < 1 or int(up.shape[1]) != int(down.shape[0]):
            raise LoraError(f"{label}: module {module!r}: lora_up {tuple(up.shape)} and lora_down {tuple(down.shape)} do not share a rank")
        alpha = None
        if "alpha" in g:
            if g["alpha"].numel() != 1:
                raise LoraError(f"{label}: module {module!r}: alpha has shape {tuple(g['alpha'].shape)}, a scalar is expected")
            alpha = float(g["alpha"].reshape(()).float())
        entries.append(LoraEntry(module, down, up, alpha))
    return entries


# ---- name tables, from the live modules ------------------------------------------------------------------------------------------
_RESNET_NAMES = {"in_layers.2": "conv1", "out_layers.3": "conv2", "emb_layers.1": "time_emb_proj", "skip_connection": "conv_shortcut"}


def _weight_modules(root: nn.Module, prefix: str = ""):
    """(path, module) of every nn.Linear / nn.Conv2d under root."""
    return [(prefix + p, m) for p, m in root.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d)) and p]


def unet_name_table(model) -> Dict[str, str]:
    """LoRA module name -> module path in the UNetModel, for every nn.Linear / nn.Conv2d it has: `lora_unet_` + the path with dots as
    underscores (fusers and position_net included), and the names kohya writes from the diffusers layout of the same network, derived
    from channel_mult, num_res_blocks and which blocks hold a transformer."""
    from ldm.modules.attention import SpatialTransformer
    from ldm.modules.diffusionmodules.openaimodel import Downsample, ResBlock, Upsample
    table: Dict[str, str] = {}

    def put(name, path):
        if table.setdefault(name, path) != path:
            raise LoraError(f"LoRA name {name!r} stands for both {table[name]!r} and {path!r} in this model")

    for path, _ in _weight_modules(model):
        put(UNET_PREFIX + path.replace(".", "_"), path)

    blocks: List[Tuple[str, str, nn.Module]] = []       # (diffusers block name, ldm path, module)
    n_levels, nrb = len(model.channel_mult), int(model.num_res_blocks)

    def members(alias, kind_index, path, block):
        """The ResBlock and (where the resolution has one) the SpatialTransformer of one TimestepEmbedSequential."""
        for idx, child in enumerate(block):
            if isinstance(child, ResBlock):
                blocks.append((alias.format("resnets", kind_index), f"{path}.{idx}", child))
            elif isinstance(child, SpatialTransformer):
                blocks.append((alias.format("attentions", kind_index), f"{path}.{idx}", child))

    for i in range(n_levels):
        for j in range(nrb):
            idx = 1 + (nrb + 1) * i + j
            members(f"down_blocks_{i}_{{}}_{{}}", j, f"input_blocks.{idx}", model.input_blocks[idx])
        if i != n_levels - 1:
            idx = 1 + (nrb + 1) * i + nrb
            if not isinstance(model.input_blocks[idx][0], Downsample):
                raise LoraError(f"input_blocks.{idx}.0 is not the downsampler of level {i}: this UNet does not have the layout the LoRA names assume")
            put(f"{UNET_PREFIX}down_blocks_{i}_downsamplers_0_conv", f"input_blocks.{idx}.0.op")
        for j in range(nrb + 1):
            idx = (nrb + 1) * i + j
            block = model.output_blocks[idx]
            members(f"up_blocks_{i}_{{}}_{{}}", j, f"output_blocks.{idx}", block)
            if j == nrb and i != n_levels - 1:
                last = len(block) - 1
                if not isinstance(block[last], Upsample):
                    raise LoraError(f"output_blocks.{idx}.{last} is not the upsampler of level {i}: this UNet does not have the layout the LoRA names assume")
                put(f"{UNET_PREFIX}up_blocks_{i}_upsamplers_0_conv", f"output_blocks.{idx}.{last}.conv")
    for idx, child in enumerate(model.middle_block):
        if isinstance(child, ResBlock):
            blocks.append((f"mid_block_resnets_{idx // 2}", f"middle_block.{idx}", child))
        elif isinstance(child, SpatialTransformer):
            blocks.append(("mid_block_attentions_0", f"middle_block.{idx}", child))
    for alias, path, block in blocks:
        for sub, _ in _weight_modules(block):
            inner = _RESNET_NAMES.get(sub, sub) if isinstance(block, ResBlock) else sub
            put(f"{UNET_PREFIX}{alias}_{inner.replace('.', '_')}", f"{path}.{sub}")
    put(UNET_PREFIX + "time_embedding_linear_1", "time_embed.0")
    put(UNET_PREFIX + "time_embedding_linear_2", "time_embed.2")
    put(UNET_PREFIX + "conv_out", "out.2")
    put(UNET_PREFIX + "conv_in", "input_blocks.0.0")
    return table


def te_name_table(text_encoder) -> Dict[str, str]:
    """LoRA module name -> module path in the FrozenCLIPEmbedder, for every nn.Linear of the installed CLIPTextModel. The names carry
    transformers 4.x's `text_model` level (lora_te_text_model_encoder_layers_n_...) whether or not the installed class has it."""
    tower = getattr(text_encoder.transformer, "text_model", None)
    root, prefix = (tower, "transformer.text_model.") if tower is not None else (text_encoder.transformer, "transformer.")
    table = {}
    for path, m in _weight_modules(root):
        if isinstance(m, nn.Linear):
            table[TE_PREFIX + "text_model_" + path.replace(".", "_")] = prefix + path
    return table


# ---- resolving an adapter against the modules ------------------------------------------------------------------------------------
def _fits(entry: LoraEntry, weight: torch.Tensor) -> bool:
    N, r = int(weight.shape[0]), entry.rank
    K = weight.numel() // N
    down, up = entry.down, entry.up
    if int(up.shape[0]) != N or up.numel() != N * r or down.numel() != r * K:
        return False
    if down.dim() == weight.dim() and tuple(down.shape[1:]) != tuple(weight.shape[1:]):
        return False
    return down.dim() in (2, weight.dim())


class _Plan:
    """What one adapter does: (root module, weight key in its state, parameter, entry, scale) per merge, and what was skipped."""

    def __init__(self, label, unet_scale, te_scale):
        self.label, self.unet_scale, self.te_scale = label, unet_scale, te_scale
        self.merges, self.skipped = [], []


def _normalise(adapters) -> List[Tuple[object, float, float]]:
    out = []
    for item in adapters or ():
        if isinstance(item, (str, os.PathLike, Mapping)):
            item = (item,)
        if not isinstance(item, (tuple, list)) or not 1 <= len(item) <= 3:
            raise LoraError(f"adapter {item!r}: give (source, scale) or (source, unet_scale, te_scale)")
        source = item[0]
        unet_scale = float(item[1]) if len(item) > 1 else 1.0
        te_scale = float(item[2]) if len(item) > 2 else unet_scale
        out.append((source, unet_scale, te_scale))
    return out


def parse_lora_spec(spec):
    """`PATH[:SCALE[:TE_SCALE]]` of the command line -> (path, unet_scale, te_scale); tuples pass through _normalise's rules."""
    if not isinstance(spec, str):
        return _normalise([spec])[0]
    parts = spec.split(":")
    scales = []
    while len(parts) > 1 and len(scales) < 2:
        try:
            scales.insert(0, float(parts[-1]))
        except ValueError:
            break
        parts.pop()
    path = ":".join(parts)
    if not path:
        raise LoraError(f"--lora {spec!r}: PATH[:SCALE[:TE_SCALE]] needs a path")
    return _normalise([(path, *scales)])[0]


def plan_loras(model, text_encoder, adapters) -> List[_Plan]:
    """Read, parse and resolve every adapter; nothing is modified. Raises LoraError for whatever is refused."""
    unet_table = unet_name_table(model)
    te_table = te_name_table(text_encoder) if text_encoder is not None else None
    unet_params = dict(model.named_parameters())
    te_params = dict(text_encoder.named_parameters()) if text_encoder is not None else {}
    first_conv = "input_blocks.0.0"
    plans = []
    for source, unet_scale, te_scale in _normalise(adapters):
        label = _label(source)
        plan = _Plan(label, unet_scale, te_scale)
        entries = parse_adapter(load_adapter(source), label)
        unresolved, misfits = [], []
        for e in entries:
            if e.is_te:
                if text_encoder is None:
                    if te_scale != 0.0:
                        raise LoraError(f"{label}: it has text-encoder entries ({e.name!r}, ...) and no text encoder was given; "
                                        "pass the text encoder, or a text-encoder scale of 0 to leave them out")
                    plan.skipped.append((e.name, "text-encoder entry, left out by a text-encoder scale of 0 (no text encoder given)"))
                    continue
                table, params, root, scale = te_table, te_params, text_encoder, te_scale
            elif e.name.startswith(UNET_PREFIX):
                table, params, root, scale = unet_table, unet_params, model, unet_scale
            else:
                unresolved.append(e.name)
                continue
            path = table.get(e.name)
            if path is None:
                unresolved.append(e.name)
                continue
            if root is model and (e.name in FIRST_CONV_NAMES or path == first_conv):
                plan.skipped.append((e.name, "the first conv is not adapted: the samplers swap it for SD's during gated-off steps, and it has "
                                             "4 + k or 9 input channels on some models"))
                continue
            weight = params[path + ".weight"]
            if not _fits(e, weight):
                misfits.append(f"{e.name}: lora_up {tuple(e.up.shape)} @ lora_down {tuple(e.down.shape)} does not fit {path}.weight {tuple(weight.shape)}")
                continue
            plan.merges.append((root, path + ".weight", weight, e, scale * e.factor))
        if unresolved:
            more = f" (and {len(unresolved) - 10} more)" if len(unresolved) > 10 else ""
            raise LoraError(f"{label}: module names that resolve to nothing in this model: {unresolved[:10]}{more}")
        if misfits:
            raise LoraError(f"{label}: shapes that do not fit their targets: " + "; ".join(misfits[:10]))
        plans.append(plan)
    return plans


# ---- applying, stacking, removing -----------------------------------------------------------------------------------------------
STASH = "_lora_stash"          # module.__dict__ key: {state key: the original tensor, on the host}
APPLIED = "_lora_applied"      # module.__dict__ key: what ensure_loras last applied


def _stash(module) -> Dict[str, torch.Tensor]:
    return module.__dict__.setdefault(STASH, {})


def forget_loras(module) -> None:
    """New weights arrived (load_state_dict): the stashed originals are not this module's any more."""
    module.__dict__.pop(STASH, None)
    module.__dict__.pop(APPLIED, None)


@torch.no_grad()
def _restore(module) -> int:
    stash = module.__dict__.get(STASH) or {}
    if stash:
        params = dict(module.named_parameters())
        for key, original in stash.items():
            params[key].copy_(original)
    return len(stash)


@torch.no_grad()
def apply_loras(model, text_encoder, adapters) -> dict:
    """Merge `adapters` -- a list of (source, scale) or (source, unet_scale, te_scale); source a file or a dict of tensors -- into the
    UNetModel's and the FrozenCLIPEmbedder's (None: no text encoder) parameters, in list order, starting from the original weights
    whatever was applied before; then drop both modules' engines. Everything is checked before anything is modified (LoraError).
    Returns dict(adapters=[dict(source, unet_scale, te_scale, unet=[paths], text_encoder=[paths])], skipped=[(source, name, why)],
    seconds=...)."""
    from . import runtime as _rt
    t0 = time.perf_counter()
    plans = plan_loras(model, text_encoder, adapters)
    for plan in plans:
        for _, key, weight, _, _ in plan.merges:
            if weight.dtype != torch.float32 or not weight.is_contiguous() or not weight.is_cuda:
                raise LoraError(f"{key} is {weight.dtype} on {weight.device}: adapters are merged into contiguous fp32 parameters on the HIP device")
    modules = [m for m in (model, text_encoder) if m is not None]
    for m in modules:
        _restore(m)
    report = dict(adapters=[], skipped=[])
    devices = set()
    for plan in plans:
        applied = dict(source=plan.label, unet_scale=plan.unet_scale, te_scale=plan.te_scale, unet=[], text_encoder=[])
        for root, key, weight, e, scale in plan.merges:
            applied["unet" if root is model else "text_encoder"].append(key[:-len(".weight")])
            if scale == 0.0:
                continue
            stash = _stash(root)
            if key not in stash:
                stash[key] = weight.detach().to("cpu", copy=True)
            dev = weight.device
            up = e.up.to(device=dev, dtype=torch.float32).reshape(e.up.shape[0], e.rank).contiguous()
            down = e.down.to(device=dev, dtype=torch.float32).reshape(e.rank, -1).contiguous()
            _rt.scratch_engine(dev).op_lora_merge(weight.data, up, down, scale)
            devices.add(dev)
        report["adapters"].append(applied)
        report["skipped"] += [(plan.label, name, why) for name, why in plan.skipped]
    for dev in devices:
        torch.cuda.synchronize(dev)
    for m in modules:
        m._drop_engine()
        m.__dict__.pop(APPLIED, None)
    report["seconds"] = time.perf_counter() - t0
    return report


@torch.no_grad()
def remove_loras(model, text_encoder=None) -> int:
    """Give every adapted parameter its original value back (torch.equal to before the first apply_loras), clear the stashes and drop
    the engines. Returns the number of tensors restored."""
    n = 0
    for m in (model, text_encoder):
        if m is None:
            continue
        restored = _restore(m)
        n += restored
        forget_loras(m)
        if restored:
            m._drop_engine()
    return n


def ensure_loras(model, text_encoder, adapters) -> Optional[dict]:
    """apply_loras unless this very list (same sources, same scales) is what the model carries already: run() calls it per prompt and
    the adapters are merged once per model load. Returns the report when something was applied."""
    spec = tuple((_label(s) if not isinstance(s, Mapping) else id(s), u, t) for s, u, t in _normalise(adapters))
    if model.__dict__.get(APPLIED) == spec:
        return None
    report = apply_loras(model, text_encoder, adapters)
    model.__dict__[APPLIED] = spec
    return report


def describe(report: dict) -> str:
    lines = []
    for a in report["adapters"]:
        lines.append(f"[gligen_amd] LoRA {a['source']}: {len(a['unet'])} UNet and {len(a['text_encoder'])} text-encoder modules "
                     f"(scale {a['unet_scale']:g} / {a['te_scale']:g})")
    for source, name, why in report["skipped"]:
        lines.append(f"[gligen_amd] LoRA {source}: skipped {name}: {why}")
    lines.append(f"[gligen_amd] LoRA merge took {report['seconds']:.3f} s; the engines are rebuilt on the next call")
    return "\n".join(lines)
