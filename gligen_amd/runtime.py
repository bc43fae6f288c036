"""Glue between the reference-shaped nn.Module containers (ldm.*) and the native engine."""
from __future__ import annotations

from typing import Dict, Mapping, Optional

import torch

from .engine import Engine


def tensor_fingerprint(t: Optional[torch.Tensor]):
    if t is None:
        return None
    return (t.data_ptr(), t._version, tuple(t.shape), t.dtype, str(t.device))


def mapping_fingerprint(m: Mapping[str, torch.Tensor]):
    return tuple((k, tensor_fingerprint(v)) for k, v in sorted(m.items()))


def module_device(module: torch.nn.Module) -> torch.device:
    p = next(module.parameters())
    if not p.is_cuda:
        raise RuntimeError(
            f"{type(module).__name__} is on {p.device}: the GLIGEN MI355X path only runs on a HIP device "
            "(call .to('cuda') as gligen_inference.load_ckpt does); there is no CPU implementation")
    return p.device


def grounding_kind_of(position_net) -> str:
    mod = type(position_net).__module__.rsplit(".", 1)[-1]
    kinds = {"text_grounding_net": "text", "text_image_grounding_net": "text_image", "keypoint_grounding_net": "keypoint",
             # spatial-map tokenizers (ConvNeXt backbone, once per prompt): the engine takes their output tokens
             "canny_grounding_net": "tokens", "hed_grounding_net": "tokens", "depth_grounding_net": "tokens",
             "normal_grounding_net": "tokens", "sem_grounding_net": "tokens"}
    if mod not in kinds:
        raise NotImplementedError(f"grounding tokenizer {type(position_net).__module__} is not implemented on MI355X")
    return kinds[mod]


_SCRATCH = {}


def scratch_engine(device) -> Engine:
    """A weight-less engine per device for stand-alone operator calls (GroundingDownsampler outside a UNetModel)."""
    dev = torch.device(device)
    key = dev.index or 0
    if key not in _SCRATCH:
        _SCRATCH[key] = Engine(dev, arena_gb=1.0)
    return _SCRATCH[key]


def build_unet_engine(model, arena_gb: float = 12.0) -> Engine:
    dev = module_device(model)
    eng = Engine(dev, arena_gb=arena_gb)
    kind = grounding_kind_of(model.position_net)
    pn = model.position_net
    eng.configure_unet(
        in_channels=model.in_channels, out_channels=model.out_channels, model_channels=model.model_channels,
        num_res_blocks=model.num_res_blocks, num_heads=model.num_heads, context_dim=model.context_dim,
        channel_mult=list(model.channel_mult), attention_resolutions=list(model.attention_resolutions),
        inpaint_mode=model.inpaint_mode, grounding_kind=kind,
        gr_in_dim=getattr(pn, "in_dim", None) or pn.out_dim, gr_out_dim=pn.out_dim,
        max_persons=getattr(pn, "max_persons_per_image", 0), fuser_type=model.fuser_type,
        extra_channels=model.additional_channel_from_downsampler if model.first_conv_type == "GLIGEN" else 0,
        tok_resize=getattr(pn, "resize_input", 0) if kind == "tokens" else 0,
        tok_in_dim=(getattr(pn, "in_dim", None) or 0) if kind == "tokens" else 0)
    # (the GroundingDownsampler runs through its own operator call with its weights passed along: gl_op_grounding_downsample)
    eng.upload("unet", {k: v for k, v in model.state_dict().items() if not k.startswith("downsample_net.")})
    eng.finalize()
    return eng


CLIP_TEXT_PREFIX = "transformer.text_model."


def clip_text_keys(layers: int):
    """The text tower's tensors under the key names GLIGEN checkpoints carry (transformers 4.x: 4 + 16 per layer)."""
    keys = [CLIP_TEXT_PREFIX + "embeddings.token_embedding.weight", CLIP_TEXT_PREFIX + "embeddings.position_embedding.weight"]
    for l in range(layers):
        p = f"{CLIP_TEXT_PREFIX}encoder.layers.{l}."
        for m in ("self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj", "layer_norm1", "mlp.fc1", "mlp.fc2", "layer_norm2"):
            keys += [p + m + ".weight", p + m + ".bias"]
    return keys + [CLIP_TEXT_PREFIX + "final_layer_norm.weight", CLIP_TEXT_PREFIX + "final_layer_norm.bias"]


def clip_text_upload_dict(state_dict: Mapping[str, torch.Tensor], layers: int) -> Dict[str, torch.Tensor]:
    """What the engine is given for a FrozenCLIPEmbedder state_dict in either key layout (transformers 4.x wraps the tower in
    `.text_model`, 5.x does not): the checkpoint's names, `position_ids` (a buffer of old versions) dropped, strictly -- a missing
    or an unknown tensor raises."""
    seen = {}
    for k, v in state_dict.items():
        if k.endswith("position_ids"):
            continue
        if k.startswith("transformer.") and not k.startswith(CLIP_TEXT_PREFIX):
            k = CLIP_TEXT_PREFIX + k[len("transformer."):]
        seen[k] = v
    want = clip_text_keys(layers)
    missing = [k for k in want if k not in seen]
    extra = sorted(set(seen) - set(want))
    if missing or extra:
        raise KeyError(f"text encoder state_dict does not match a {layers}-layer CLIP text tower: missing {missing[:4]}, unexpected {extra[:4]}")
    return {k: seen[k] for k in want}


def build_clip_text_engine(embedder, arena_gb: float = 0.25) -> Engine:
    """The native text tower of a FrozenCLIPEmbedder: its own engine with a small arena (32 sequences of 77 tokens need ~50 MB)."""
    dev = module_device(embedder)
    tower = getattr(embedder.transformer, "text_model", embedder.transformer)
    cfg = embedder.transformer.config
    eng = Engine(dev, arena_gb=arena_gb)
    try:
        eng.configure_clip_text(vocab=cfg.vocab_size, width=cfg.hidden_size, heads=cfg.num_attention_heads, layers=len(tower.encoder.layers),
                                intermediate=cfg.intermediate_size, max_positions=cfg.max_position_embeddings, ln_eps=cfg.layer_norm_eps)
        if cfg.hidden_act != "quick_gelu":
            raise NotImplementedError(f"CLIP text tower with hidden_act={cfg.hidden_act!r}: the native path implements quick_gelu")
        eng.upload("text_encoder", clip_text_upload_dict(embedder.state_dict(), len(tower.encoder.layers)))
        eng.finalize()
    except Exception:
        eng.close()
        raise
    return eng


CLIP_VISION_PREFIXES = ("vision_model.", "visual_projection.")


def clip_vision_keys(layers: int):
    """The vision tower's tensors and visual_projection under their transformers keys (8 + 16 per layer)."""
    v = "vision_model."
    keys = [v + "embeddings.class_embedding", v + "embeddings.patch_embedding.weight", v + "embeddings.position_embedding.weight",
            v + "pre_layrnorm.weight", v + "pre_layrnorm.bias"]
    for l in range(layers):
        p = f"{v}encoder.layers.{l}."
        for m in ("self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj", "layer_norm1", "mlp.fc1", "mlp.fc2", "layer_norm2"):
            keys += [p + m + ".weight", p + m + ".bias"]
    return keys + [v + "post_layernorm.weight", v + "post_layernorm.bias", "visual_projection.weight"]


def clip_vision_upload_dict(state_dict: Mapping[str, torch.Tensor], layers: int) -> Dict[str, torch.Tensor]:
    """What the engine is given for a CLIPModel state_dict (the text side -- text_model.*, text_projection.*, logit_scale -- is not
    the vision tower's and is ignored) or a CLIPVisionModelWithProjection one: `position_ids` dropped, strictly otherwise -- a missing
    or an unknown vision tensor raises."""
    seen = {k: v for k, v in state_dict.items() if k.startswith(CLIP_VISION_PREFIXES) and not k.endswith("position_ids")}
    other = sorted(k for k in state_dict if not k.startswith(CLIP_VISION_PREFIXES + ("text_model.", "text_projection.")) and k != "logit_scale")
    want = clip_vision_keys(layers)
    missing = [k for k in want if k not in seen]
    extra = sorted(set(seen) - set(want)) + other
    if missing or extra:
        raise KeyError(f"state_dict does not match a {layers}-layer CLIP vision tower with projection: missing {missing[:4]}, unexpected {extra[:4]}")
    return {k: seen[k] for k in want}


def clip_vision_arena_gb(images: int = 8, tokens: int = 257, width: int = 1024, intermediate: int = 4096, patch_k: int = 640) -> float:
    """The activation bytes Engine::clip_vision_encode needs for `images` at once (its need() formula), with 25 % on top: 8 images of
    ViT-L/14 are 2304 rows x 26.6 KB + patch rows = 64 MB -> 0.08."""
    up = lambda n: -(-n // 256) * 256
    need = up(images * tokens) * (width * 18 + intermediate * 2) + up(images * (tokens - 1)) * patch_k * 2 + up(images) * width * 2 + 10 * 256
    return 1.25 * need / 2 ** 30


def build_clip_vision_engine(clip_model, arena_gb: Optional[float] = None) -> Engine:
    """The native vision tower + visual_projection of a transformers CLIPModel or CLIPVisionModelWithProjection: its own engine, the
    arena sized for 8 images at once by default (more are encoded in chunks)."""
    dev = module_device(clip_model)
    cfg = getattr(clip_model.config, "vision_config", clip_model.config)
    layers = len(clip_model.vision_model.encoder.layers)
    projection_dim = int(clip_model.visual_projection.weight.shape[0])
    if cfg.hidden_act != "quick_gelu":
        raise NotImplementedError(f"CLIP vision tower with hidden_act={cfg.hidden_act!r}: the native path implements quick_gelu")
    if cfg.num_channels != 3:
        raise NotImplementedError(f"CLIP vision tower with num_channels={cfg.num_channels}: the native path reads 3-channel pixel_values")
    if arena_gb is None:
        kpad = -(-3 * cfg.patch_size ** 2 // 64) * 64
        tokens = (cfg.image_size // max(cfg.patch_size, 1)) ** 2 + 1
        arena_gb = max(clip_vision_arena_gb(8, tokens, cfg.hidden_size, cfg.intermediate_size, kpad), 0.03)
    eng = Engine(dev, arena_gb=arena_gb)
    try:
        eng.configure_clip_vision(image_size=cfg.image_size, patch=cfg.patch_size, width=cfg.hidden_size, heads=cfg.num_attention_heads, layers=layers,
                                  intermediate=cfg.intermediate_size, projection_dim=projection_dim, ln_eps=cfg.layer_norm_eps)
        eng.upload("clip_vision", clip_vision_upload_dict(clip_model.state_dict(), layers))
        eng.finalize()
    except Exception:
        eng.close()
        raise
    return eng


def clip_preprocess_settings(image_processor, image_size: Optional[int] = None) -> dict:
    """The arguments of Engine.clip_vision_preprocess read from a transformers CLIPImageProcessor: dict(size, crop, mean, std,
    filter). Supported: do_resize with size.shortest_edge, resample BICUBIC or BILINEAR, do_center_crop with a square crop_size (equal
    to the tower's image_size when that is given), do_rescale with rescale_factor 1 / 255, do_normalize with any mean and std.
    Anything else raises NotImplementedError naming the field. Host only."""
    ip = image_processor

    def refuse(field, what):
        raise NotImplementedError(f"native CLIP image preprocessing does not cover {field} {what}")

    def entry(d, k):
        return None if d is None else d.get(k) if isinstance(d, Mapping) else getattr(d, k, None)

    if not getattr(ip, "do_resize", False):
        refuse("do_resize", "= False (the images are resized to size.shortest_edge)")
    size = getattr(ip, "size", None)
    if entry(size, "shortest_edge") is None or any(entry(size, k) is not None for k in ("height", "width", "longest_edge", "max_height", "max_width")):
        refuse("size", f"= {size!r} (only shortest_edge is implemented)")
    resample = getattr(ip, "resample", None)
    filters = {3: "bicubic", 2: "bilinear"}       # PIL.Image.Resampling
    if resample is None or int(resample) not in filters:
        refuse("resample", f"= {resample!r} (BICUBIC and BILINEAR are implemented)")
    if not getattr(ip, "do_center_crop", False):
        refuse("do_center_crop", "= False (the tower reads a square centre crop)")
    crop = getattr(ip, "crop_size", None)
    ch, cw = entry(crop, "height"), entry(crop, "width")
    if ch is None or ch != cw or (image_size is not None and int(ch) != int(image_size)):
        refuse("crop_size", f"= {crop!r} (a square crop" + (f" of the tower's image_size {image_size})" if image_size is not None else ")"))
    if int(ch) > int(entry(size, "shortest_edge")):
        refuse("crop_size", f"= {crop!r} larger than size.shortest_edge = {entry(size, 'shortest_edge')} (the processor would pad)")
    if getattr(ip, "do_pad", None):
        refuse("do_pad", "= True")
    if not getattr(ip, "do_rescale", False):
        refuse("do_rescale", "= False (samples are scaled by 1 / 255)")
    if getattr(ip, "rescale_factor", None) != 1 / 255:
        refuse("rescale_factor", f"= {getattr(ip, 'rescale_factor', None)!r} (1 / 255 is implemented)")
    mean, std = getattr(ip, "image_mean", None), getattr(ip, "image_std", None)
    if not getattr(ip, "do_normalize", False):
        refuse("do_normalize", "= False")
    for name, v in (("image_mean", mean), ("image_std", std)):
        if not isinstance(v, (list, tuple)) or len(v) != 3 or (name == "image_std" and any(float(x) == 0 for x in v)):
            refuse(name, f"= {v!r} (three values, one per channel)")
    return dict(size=int(entry(size, "shortest_edge")), crop=int(ch), mean=tuple(float(x) for x in mean), std=tuple(float(x) for x in std),
                filter=filters[int(resample)])


def build_vae_engine(ae, arena_gb: float = 8.0) -> Engine:
    dev = module_device(ae)
    eng = Engine(dev, arena_gb=arena_gb)
    dd = ae.ddconfig
    eng.configure_vae(ch=dd["ch"], out_ch=dd["out_ch"], z_channels=dd["z_channels"], num_res_blocks=dd["num_res_blocks"],
                      embed_dim=ae.embed_dim, ch_mult=list(dd["ch_mult"]), scale_factor=ae.scale_factor)
    eng.upload("vae", ae.state_dict())  # decoder + post_quant_conv (decode), encoder + quant_conv (encode, inpainting)
    eng.finalize()
    return eng
