"""Python handle on the native engine (libgligen_amd.so): torch tensors in, torch tensors out.

torch is used only for device memory and the current HIP stream; every computation below is a
call through the C ABI. Nothing here falls back to torch ops.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib, vae_tiling
from ._lib import Grounding, PlmsArgs, SolverArgs, UNetConfig, VaeConfig, check

GROUNDING_KINDS = {"text": 0, "text_image": 1, "keypoint": 2, "tokens": 3}


def _stream(device=None) -> C.c_void_p:
    # the current stream OF THE ENGINE'S DEVICE: torch's current device may be another GPU of the same process
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


IMAGE_FILTERS = {"bicubic": 0, "bilinear": 1}      # gl_op_image_resample's filter argument


def clip_resize_size(width: int, height: int, shortest_edge: int):
    """(width, height) after CLIP's resize: the short side becomes `shortest_edge`, the long one int(shortest_edge * long / short)
    (transformers get_resize_output_image_size with default_to_square=False)."""
    short, long = (width, height) if width <= height else (height, width)
    new_long = int(shortest_edge * long / short)
    return (shortest_edge, new_long) if width <= height else (new_long, shortest_edge)


def normalise_lut(mean, std) -> np.ndarray:
    """[3, 256] float32: (float32(v) / float32(255) - float32(mean_c)) / float32(std_c), each operation rounded to float32 -- what
    rescale by 1 / 255 followed by normalize gives for a u8 sample v."""
    v = np.arange(256, dtype=np.float32)[None, :] / np.float32(255)
    return ((v - np.asarray(mean, dtype=np.float32)[:, None]) / np.asarray(std, dtype=np.float32)[:, None]).astype(np.float32)


SPATIAL_MAP_KEYS = dict(canny="canny_edge", hed="hed_edge", depth="depth", normal="normal", sem="sem")


def spatial_train_config(cfg: Mapping) -> Optional[dict]:
    """What the training step needs to know of a spatial-map model, from its UNetModel kwargs (None for the discrete tokenizers):
    the modality and the batch key of its map (the five *_grounding_net targets), the tokenizer's resize_input and semantic-map
    channels, and the GroundingDownsampler's resize / mode / channels -- read off the same classes the model is built from
    (ldm/modules/diffusionmodules/_spatial.py), so a config's `params` and the class defaults both apply."""
    import inspect
    from ldm.util import get_obj_from_str, instantiate_from_config
    tok = cfg.get("grounding_tokenizer") or {}
    mod = tok.get("target", "").rsplit(".", 2)
    modality = mod[-2][:-len("_grounding_net")] if len(mod) == 3 and mod[-2].endswith("_grounding_net") else None
    if modality not in SPATIAL_MAP_KEYS:
        return None
    defaults = {k: p.default for k, p in inspect.signature(get_obj_from_str(tok["target"]).__init__).parameters.items()}
    params = dict(tok.get("params") or {})
    out = dict(modality=modality, map_key=SPATIAL_MAP_KEYS[modality], tok_resize=int(params.get("resize_input", defaults["resize_input"])),
               tok_in_dim=int(params.get("in_dim", defaults.get("in_dim")) or 0), ds=None)
    if cfg.get("grounding_downsampler"):
        ds = instantiate_from_config(cfg["grounding_downsampler"])      # a few small convs: only its constants are read
        out["ds"] = dict(resize=int(ds.resize_input), mode={"bicubic": 0, "nearest": 1}[ds.mode], n_in=int(ds.n_in),
                         mid=int(ds.c_mid) if ds.has_layers else 0, out=int(ds.out_dim))
    return out


class TrainResDims(C.Structure):   # = gl_train_resblock_dims
    _fields_ = [(n, C.c_int) for n in ("B", "H", "W", "Cin", "Cout", "emb_dim")]


class TrainBlockDims(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("Ng", C.c_int), ("C", C.c_int), ("heads", C.c_int), ("ctx_T", C.c_int), ("ctx_dim", C.c_int),
                ("fuser_scale", C.c_float)]


class Engine:
    """One engine per device; owns packed bf16 weights, workspace arena and cached conditioning."""

    def __init__(self, device: int | torch.device | str = 0, arena_gb: float = 12.0):
        if not torch.cuda.is_available():
            raise _lib.GligenAmdError("no HIP device visible: gligen_amd needs an MI355X (gfx950) GPU")
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        self.device = torch.device("cuda", dev.index or 0)
        self.lib = _lib.load()
        self._ctx = C.c_void_p()
        torch.cuda.set_device(self.device)
        check(self.lib.gl_ctx_create(self.device.index, C.c_size_t(int(arena_gb * (1 << 30))), C.byref(self._ctx)))
        self.unet_cfg: Optional[dict] = None
        self.vae_cfg: Optional[dict] = None
        self.clip_cfg: Optional[dict] = None
        self.clip_vision_cfg: Optional[dict] = None
        self._keep: list = []
        self._vae_tiling = ("off", vae_tiling.DEFAULT_TILE, vae_tiling.DEFAULT_OVERLAP)
        self._vae_tiled_shapes: set = set()
        self._vae_plans: dict = {}

    def fork(self, arena_gb: Optional[float] = None) -> "Engine":
        """A second execution context on the same packed weights (gl_ctx_fork): its own arena, conditioning, gates, captured
        graphs and first-conv copy; everything gl_finalize packed is shared with -- and kept alive by -- this engine."""
        e = Engine.__new__(Engine)
        e.device, e.lib = self.device, self.lib
        e._ctx = C.c_void_p()
        e.unet_cfg, e.vae_cfg = self.unet_cfg, self.vae_cfg
        e._keep = []
        e._vae_tiling, e._vae_tiled_shapes, e._vae_plans = self._vae_tiling, set(), {}
        nbytes = 0 if arena_gb is None else int(arena_gb * (1 << 30))
        check(self.lib.gl_ctx_fork(self._ctx, C.c_size_t(nbytes), C.byref(e._ctx)))
        return e

    def memory(self) -> dict:
        """Device bytes this context allocated itself outside the arena (packed weights + slabs; a fork: slabs only), its
        arena reservation and the arena's high-water mark."""
        own, arena, fk, hw = C.c_size_t(0), C.c_size_t(0), C.c_int(0), C.c_size_t(0)
        check(self.lib.gl_ctx_memory(self._ctx, C.byref(own), C.byref(arena), C.byref(fk)))
        check(self.lib.gl_arena_high_water(self._ctx, C.byref(hw)))
        return dict(own_bytes=int(own.value), arena_bytes=int(arena.value), arena_high_water=int(hw.value), is_fork=bool(fk.value))

    def close(self) -> None:
        if self._ctx:
            check(self.lib.gl_ctx_destroy(self._ctx))
            self._ctx = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- configuration / weights -------------------------------------------------
    def configure_unet(self, *, in_channels, out_channels, model_channels, num_res_blocks, num_heads, context_dim,
                       channel_mult: Sequence[int], attention_resolutions: Sequence[int], inpaint_mode=False,
                       grounding_kind="text", gr_in_dim=768, gr_out_dim=768, max_persons=0, fuser_type="gatedSA",
                       extra_channels=0, tok_resize=0, tok_in_dim=0) -> None:
        cfg = UNetConfig()
        cfg.in_channels, cfg.out_channels, cfg.model_channels = in_channels, out_channels, model_channels
        cfg.num_res_blocks, cfg.num_heads, cfg.context_dim = num_res_blocks, num_heads, context_dim
        cfg.n_mult = len(channel_mult)
        for i, v in enumerate(channel_mult):
            cfg.channel_mult[i] = int(v)
        cfg.n_attn = len(attention_resolutions)
        for i, v in enumerate(attention_resolutions):
            cfg.attention_resolutions[i] = int(v)
        cfg.inpaint_mode = int(bool(inpaint_mode))
        cfg.grounding_kind = GROUNDING_KINDS[grounding_kind]
        cfg.gr_in_dim, cfg.gr_out_dim, cfg.max_persons = gr_in_dim, gr_out_dim, max_persons
        cfg.fuser_kind = _lib.fuser_kind(fuser_type)
        cfg.extra_channels = int(extra_channels)
        cfg.tok_resize, cfg.tok_in_dim = int(tok_resize), int(tok_in_dim)
        check(self.lib.gl_unet_configure(self._ctx, C.byref(cfg)))
        self.unet_cfg = dict(in_channels=in_channels, out_channels=out_channels, inpaint_mode=bool(inpaint_mode),
                             grounding_kind=grounding_kind, context_dim=context_dim, extra_channels=int(extra_channels),
                             gr_out_dim=gr_out_dim, tok_tokens=(int(tok_resize) // 32) ** 2)

    def configure_vae(self, *, ch, out_ch, z_channels, num_res_blocks, embed_dim, ch_mult: Sequence[int],
                      scale_factor: float) -> None:
        cfg = VaeConfig()
        cfg.ch, cfg.out_ch, cfg.z_channels, cfg.num_res_blocks, cfg.embed_dim = ch, out_ch, z_channels, num_res_blocks, embed_dim
        cfg.n_mult = len(ch_mult)
        for i, v in enumerate(ch_mult):
            cfg.ch_mult[i] = int(v)
        cfg.scale_factor = float(scale_factor)
        check(self.lib.gl_vae_configure(self._ctx, C.byref(cfg)))
        self.vae_cfg = dict(out_ch=out_ch, z_channels=z_channels, n_up=len(ch_mult) - 1)

    def configure_clip_text(self, *, vocab, width, heads, layers, intermediate, max_positions, ln_eps=1e-5) -> None:
        """The CLIP text tower (transformers CLIPTextConfig: vocab_size, hidden_size, num_attention_heads, num_hidden_layers,
        intermediate_size, max_position_embeddings, layer_norm_eps); weights go under the namespace 'text_encoder'."""
        cfg = _lib.ClipTextConfig()
        cfg.vocab, cfg.width, cfg.heads, cfg.layers = int(vocab), int(width), int(heads), int(layers)
        cfg.intermediate, cfg.max_positions, cfg.ln_eps = int(intermediate), int(max_positions), float(ln_eps)
        check(self.lib.gl_clip_text_configure(self._ctx, C.byref(cfg)))
        self.clip_cfg = dict(vocab=int(vocab), width=int(width), max_positions=int(max_positions))

    def clip_text_encode(self, ids: torch.Tensor, eos_index: torch.Tensor):
        """ids [S, T] integer token ids, eos_index [S] (the position HF pools) -> (last_hidden [S, T, width], pooled [S, width]), fp32."""
        if ids.dim() != 2 or eos_index.shape != (ids.shape[0],):
            raise ValueError("clip_text_encode: ids [S, T] and one eos index per sequence")
        S, T = int(ids.shape[0]), int(ids.shape[1])
        host = ids.detach().cpu()
        if S == 0 or int(host.min()) < 0 or int(host.max()) >= self.clip_cfg["vocab"]:
            raise ValueError(f"clip_text_encode: token ids must lie in [0, {self.clip_cfg['vocab']})")
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        eos = eos_index.to(device=self.device, dtype=torch.int32).contiguous()
        hidden = torch.empty((S, T, self.clip_cfg["width"]), device=self.device, dtype=torch.float32)
        pooled = torch.empty((S, self.clip_cfg["width"]), device=self.device, dtype=torch.float32)
        check(self.lib.gl_clip_text_encode(self._ctx, _ptr(ids), _ptr(eos), S, T, _ptr(hidden), _ptr(pooled), _stream(self.device)))
        return hidden, pooled

    def configure_clip_vision(self, *, image_size, patch, width, heads, layers, intermediate, projection_dim, ln_eps=1e-5) -> None:
        """The CLIP vision tower and visual_projection (transformers CLIPVisionConfig: image_size, patch_size, hidden_size,
        num_attention_heads, num_hidden_layers, intermediate_size, projection_dim, layer_norm_eps); weights go under the namespace
        'clip_vision'."""
        cfg = _lib.ClipVisionConfig()
        cfg.image_size, cfg.patch, cfg.width, cfg.heads, cfg.layers = int(image_size), int(patch), int(width), int(heads), int(layers)
        cfg.intermediate, cfg.projection_dim, cfg.ln_eps = int(intermediate), int(projection_dim), float(ln_eps)
        check(self.lib.gl_clip_vision_configure(self._ctx, C.byref(cfg)))
        self.clip_vision_cfg = dict(image_size=int(image_size), width=int(width), projection_dim=int(projection_dim),
                                    tokens=(int(image_size) // int(patch)) ** 2 + 1)

    def clip_vision_encode(self, pixel_values: torch.Tensor):
        """pixel_values [S, 3, image_size, image_size] (preprocessed) -> (last_hidden [S, T, width], pooled [S, width] after
        post_layernorm, image_embeds [S, projection_dim], not normalised), fp32."""
        c = self.clip_vision_cfg
        if c is None:
            raise _lib.GligenAmdError("clip_vision_encode: the CLIP vision tower is not configured")
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, c["image_size"], c["image_size"]) or pixel_values.shape[0] < 1:
            raise ValueError(f"clip_vision_encode: pixel_values {tuple(pixel_values.shape)}, expected [S >= 1, 3, {c['image_size']}, {c['image_size']}]")
        S = int(pixel_values.shape[0])
        px = pixel_values.to(device=self.device, dtype=torch.float32).contiguous()
        hidden = torch.empty((S, c["tokens"], c["width"]), device=self.device, dtype=torch.float32)
        pooled = torch.empty((S, c["width"]), device=self.device, dtype=torch.float32)
        embeds = torch.empty((S, c["projection_dim"]), device=self.device, dtype=torch.float32)
        check(self.lib.gl_clip_vision_encode(self._ctx, _ptr(px), S, _ptr(hidden), _ptr(pooled), _ptr(embeds), _stream(self.device)))
        return hidden, pooled, embeds

    def image_resample(self, images, sizes, crops=None, filter: str = "bicubic", lut=None):
        """PIL.Image.resize + crop of 8-bit RGB images, bit for bit, for a batch of different sizes in two launches
        (gl_op_image_resample). images: u8 [H, W, 3] tensors or arrays (host ones are uploaded; a device tensor may be a view with a
        row stride); sizes: (width, height) each image is resized to; crops: (x, y, width, height) inside the resized image, None = all
        of it. Returns the list of u8 [ch, cw, 3] device tensors, or, with lut (float32 [3, 256]: sample v of channel c becomes
        lut[c, v]; all crops equal), one float32 [S, 3, ch, cw] tensor."""
        if filter not in IMAGE_FILTERS:
            raise ValueError(f"image_resample: filter {filter!r}; the resampler has {', '.join(IMAGE_FILTERS)}")
        S = len(images)
        if S < 1 or len(sizes) != S or (crops is not None and len(crops) != S):
            raise ValueError("image_resample: one size (and one crop) per image, at least one image")
        descs = (_lib.ImageDesc * S)()
        keep = []
        for i, im in enumerate(images):
            t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError(f"image_resample: image {i} is {t.dtype} {tuple(t.shape)}; 3 interleaved u8 channels [H, W, 3] are read")
            t = t.to(self.device)
            if t.stride(2) != 1 or t.stride(1) != 3 or (t.shape[0] > 1 and t.stride(0) < 3 * t.shape[1]):
                t = t.contiguous()
            keep.append(t)
            w, h = (int(v) for v in sizes[i])
            x, y, cw, ch = (0, 0, w, h) if crops is None or crops[i] is None else (int(v) for v in crops[i])
            d = descs[i]
            d.pixels, d.width, d.height = t.data_ptr(), int(t.shape[1]), int(t.shape[0])
            d.row_stride = int(t.stride(0)) if t.shape[0] > 1 else 3 * int(t.shape[1])
            d.resized_w, d.resized_h, d.crop_x, d.crop_y, d.crop_w, d.crop_h = w, h, x, y, cw, ch
        if lut is None:
            outs = [torch.empty((max(d.crop_h, 0), max(d.crop_w, 0), 3), device=self.device, dtype=torch.uint8) for d in descs]
            out = (C.c_void_p * S)(*[o.data_ptr() for o in outs])
            check(self.lib.gl_op_image_resample(self._ctx, descs, S, IMAGE_FILTERS[filter], 0, None, out, _stream(self.device)))
            return outs
        table = np.ascontiguousarray(lut, dtype=np.float32)
        if table.shape != (3, 256):
            raise ValueError(f"image_resample: lut {table.shape}; one float32 row of 256 values per channel, [3, 256]")
        px = torch.empty((S, 3, max(descs[0].crop_h, 0), max(descs[0].crop_w, 0)), device=self.device, dtype=torch.float32)
        check(self.lib.gl_op_image_resample(self._ctx, descs, S, IMAGE_FILTERS[filter], 1, table.ctypes.data_as(C.POINTER(C.c_float)),
                                            _ptr(px), _stream(self.device)))
        return px

    def clip_vision_preprocess(self, images, size: int, crop: int, mean, std, filter: str = "bicubic") -> torch.Tensor:
        """transformers' CLIPImageProcessor on the device: resize the short side to `size` (clip_resize_size), centre crop `crop` x
        `crop`, (v / 255 - mean) / std. images: u8 [H, W, 3] tensors or arrays of any sizes -> pixel_values float32 [S, 3, crop, crop]
        on the device, the input of clip_vision_encode, bit for bit the processor's (Pillow backend)."""
        size, crop = int(size), int(crop)
        if crop > size:
            raise ValueError(f"clip_vision_preprocess: crop {crop} larger than the resized short side {size} (the processor would pad)")
        sizes = [clip_resize_size(int(im.shape[1]), int(im.shape[0]), size) for im in images]
        crops = [((w - crop) // 2, (h - crop) // 2, crop, crop) for w, h in sizes]
        return self.image_resample(images, sizes, crops, filter, normalise_lut(mean, std))

    def op_clip_attention(self, qkv: torch.Tensor, S: int, T: int, heads: int, causal: bool = False, out: Optional[torch.Tensor] = None):
        """The CLIP towers' attention launch: qkv bf16 [>= S * T, 3 * heads * 64] rows [q | k | v] -> bf16 [S * T, heads * 64] (written
        into `out` when given: rows >= S * T of it are left alone)."""
        if qkv.dtype != torch.bfloat16 or qkv.dim() != 2 or qkv.shape[1] != 3 * heads * 64 or qkv.shape[0] < S * T or not qkv.is_contiguous():
            raise ValueError("op_clip_attention: qkv must be contiguous bf16 [>= S * T, 3 * heads * 64]")
        if out is None:
            out = torch.empty((S * T, heads * 64), device=self.device, dtype=torch.bfloat16)
        elif out.dtype != torch.bfloat16 or out.dim() != 2 or out.shape[1] != heads * 64 or out.shape[0] < S * T or not out.is_contiguous():
            raise ValueError("op_clip_attention: out must be contiguous bf16 [>= S * T, heads * 64]")
        check(self.lib.gl_op_clip_attention(self._ctx, _ptr(qkv), _ptr(out), int(S), int(T), int(heads), int(bool(causal)), _stream(self.device)))
        return out

    def set_vae_attention(self, mode="auto") -> None:
        """gl_vae_set_attention: the form of the autoencoder's AttnBlock on this context. 'auto' (default): score matrices up to 4096
        tokens (6 T^2 bytes of arena per image), vae_attn_flash_kernel above that or where they do not fit; 'matrix'; 'flash'."""
        from ._lib import VAE_ATTN_MODES
        check(self.lib.gl_vae_set_attention(self._ctx, VAE_ATTN_MODES[mode] if isinstance(mode, str) else int(mode)))

    def vae_attention(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mode="auto") -> torch.Tensor:
        """softmax(q k^T C^-0.5) v on bf16 rows [B, T, C] (gl_op_vae_attention): one head whose dimension is C, T and C multiples of
        64; mode as set_vae_attention, for this call. Returns bf16 [B, T, C]."""
        from ._lib import VAE_ATTN_MODES
        for name, t in (("q", q), ("k", k), ("v", v)):
            if t.dtype != torch.bfloat16 or t.dim() != 3 or t.shape != q.shape or not t.is_contiguous() or t.device != q.device:
                raise ValueError(f"vae_attention: {name} must be contiguous bf16 [B, T, C] like q")
        B, T, Cn = q.shape
        out = torch.empty_like(q)
        check(self.lib.gl_op_vae_attention(self._ctx, _ptr(q), _ptr(k), _ptr(v), int(B), int(T), int(Cn),
                                           VAE_ATTN_MODES[mode] if isinstance(mode, str) else int(mode), _ptr(out), _stream(self.device)))
        return out

    def upload(self, namespace: str, state_dict: Mapping[str, torch.Tensor], prefix_filter: Optional[str] = None) -> int:
        """Upload fp32 parameters under '<namespace>/<reference state_dict key>'."""
        n = 0
        for key, t in state_dict.items():
            if prefix_filter is not None and not key.startswith(prefix_filter):
                continue
            t = t.detach().to(dtype=torch.float32).contiguous()
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
            check(self.lib.gl_weight_upload(self._ctx, f"{namespace}/{key}".encode(), C.c_void_p(t.data_ptr()),
                                            t.dim(), shape, int(t.is_cuda)))
            n += 1
        return n

    def finalize(self) -> None:
        check(self.lib.gl_finalize(self._ctx))

    # ---- denoising path ---------------------------------------------------------
    def set_cond(self, context: torch.Tensor, grounding: Mapping[str, torch.Tensor]) -> None:
        """context [Beff,T,768]; grounding = kwargs of the reference PositionNet.forward."""
        dev = self.device
        ctx = _f32(context, dev)
        kind = self.unet_cfg["grounding_kind"]
        g = Grounding()
        keep = [ctx]

        def put(name, field=None):
            t = _f32(grounding[name], dev)
            keep.append(t)
            setattr(g, field or name, t.data_ptr())
            return t

        if kind == "text":
            b = put("boxes"); put("masks"); put("positive_embeddings", "text_embeddings")
        elif kind == "text_image":
            b = put("boxes"); put("masks"); put("text_masks"); put("image_masks")
            put("text_embeddings"); put("image_embeddings")
        elif kind == "tokens":
            b = put("tokens")
        else:
            b = put("points"); put("masks")
        if b.shape[0] != ctx.shape[0]:
            raise ValueError("grounding batch does not match context batch")
        g.n = int(b.shape[1])
        check(self.lib.gl_unet_set_cond(self._ctx, int(ctx.shape[0]), _ptr(ctx), int(ctx.shape[1]), C.byref(g), _stream(self.device)))
        self._keep = keep
        self._cond_shape = (int(ctx.shape[0]), g.n * (2 if kind == "text_image" else 1))

    def grounding_tokens(self) -> torch.Tensor:
        """objs = position_net(**grounding_input) of the current conditioning, fp32 [Beff, Ng, out_dim]."""
        Beff, Ng = int(self._cond_shape[0]), int(self._cond_shape[1])
        out = torch.empty((Beff, Ng, self.unet_cfg["gr_out_dim"]), device=self.device, dtype=torch.float32)
        check(self.lib.gl_unet_grounding_tokens(self._ctx, _ptr(out), _stream(self.device)))
        return out

    def spatial_tokens(self, image: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """PositionNet.forward of the spatial-map tokenizers (ConvNeXt-tiny on the device): image [B,C,H,W], mask [B] or [B,1]
        -> grounding tokens fp32 [B, (resize_input/32)^2, out_dim]."""
        image = _f32(image, self.device)
        mask = _f32(mask.reshape(-1), self.device)
        B, Cc, H, W = image.shape
        if mask.shape[0] != B:
            raise ValueError("spatial_tokens: one mask value per image")
        out = torch.empty((B, self.unet_cfg["tok_tokens"], self.unet_cfg["gr_out_dim"]), device=self.device, dtype=torch.float32)
        check(self.lib.gl_op_spatial_tokens(self._ctx, _ptr(image), int(B), int(Cc), int(H), int(W), _ptr(mask), _ptr(out), _stream(self.device)))
        return out

    def grounding_downsample(self, img: torch.Tensor, n_in: int, resize: int, mode: str, convs) -> torch.Tensor:
        """GroundingDownsampler.forward: img [B,Cimg,H,W] -> [B,out,resize/4,resize/4] (convs = (w1,b1,w2,b2)) or, convs None,
        the resized first n_in channels [B,n_in,resize,resize]."""
        img = _f32(img, self.device)
        B, Cimg, H, W = img.shape
        m = {"bicubic": 0, "nearest": 1}[mode]
        if convs is None:
            out = torch.empty((B, n_in, resize, resize), device=self.device, dtype=torch.float32)
            check(self.lib.gl_op_grounding_downsample(self._ctx, _ptr(img), B, Cimg, H, W, n_in, resize, m, None, None, 0, None, None, 0,
                                                      _ptr(out), _stream(self.device)))
            return out
        w1, b1, w2, b2 = (_f32(t.detach(), self.device) for t in convs)
        out = torch.empty((B, w2.shape[0], resize // 4, resize // 4), device=self.device, dtype=torch.float32)
        check(self.lib.gl_op_grounding_downsample(self._ctx, _ptr(img), B, Cimg, H, W, n_in, resize, m, _ptr(w1), _ptr(b1), int(w1.shape[0]),
                                                  _ptr(w2), _ptr(b2), int(w2.shape[0]), _ptr(out), _stream(self.device)))
        return out

    # ---- semantic maps as class indices (include/gligen_amd_maps.h) ---------------
    def _class_map(self, cls: torch.Tensor, what: str) -> torch.Tensor:
        if cls.dtype != torch.uint8 or cls.dim() not in (3, 4) or (cls.dim() == 4 and cls.shape[1] != 1) or cls.numel() == 0:
            raise ValueError(f"{what}: the class map is {cls.dtype} {tuple(cls.shape)}; u8 [B, 1, H, W] or [B, H, W] is read")
        return cls.reshape(cls.shape[0], cls.shape[-2], cls.shape[-1]).to(self.device).contiguous()

    def class_map_resize(self, maps, size, boxes=None) -> torch.Tensor:
        """PIL.Image.crop(box).resize(size, Image.NEAREST) of single-channel u8 images of different sizes in one launch, byte for byte
        (gl_op_class_map_resize). maps: u8 [H, W] tensors or arrays (host ones are uploaded; a device tensor may be a view with a row
        stride); size: (width, height) of every result; boxes: (x, y, width, height) inside each map, None = all of it. Returns the
        u8 [S, height, width] device tensor."""
        S = len(maps)
        if S < 1 or (boxes is not None and len(boxes) != S):
            raise ValueError("class_map_resize: at least one map, and one box per map")
        w, h = (int(v) for v in size)
        descs = (_lib.ClassMapDesc * S)()
        keep = []
        for i, m in enumerate(maps):
            t = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m))
            if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError(f"class_map_resize: map {i} is {t.dtype} {tuple(t.shape)}; one u8 channel [H, W] is read")
            t = t.to(self.device)
            if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
                t = t.contiguous()
            keep.append(t)
            d = descs[i]
            d.pixels, d.width, d.height = t.data_ptr(), int(t.shape[1]), int(t.shape[0])
            d.row_stride = int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])
            d.box_x, d.box_y, d.box_w, d.box_h = (0, 0, d.width, d.height) if boxes is None or boxes[i] is None else (int(v) for v in boxes[i])
        out = torch.empty((S, max(h, 0), max(w, 0)), device=self.device, dtype=torch.uint8)
        check(self.lib.gl_op_class_map_resize(self._ctx, descs, S, w, h, _ptr(out), _stream(self.device)))
        return out

    def spatial_tokens_classes(self, cls: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """spatial_tokens of a semantic-map tokenizer from the class map u8 [B, 1, H, W] (a value >= in_dim: no class) instead of its
        in_dim one-hot planes: the same tokens, bit for bit (gl_op_spatial_tokens_classes)."""
        cls = self._class_map(cls, "spatial_tokens_classes")
        mask = _f32(mask.reshape(-1), self.device)
        B, H, W = cls.shape
        if mask.shape[0] != B:
            raise ValueError("spatial_tokens_classes: one mask value per map")
        out = torch.empty((B, self.unet_cfg["tok_tokens"], self.unet_cfg["gr_out_dim"]), device=self.device, dtype=torch.float32)
        check(self.lib.gl_op_spatial_tokens_classes(self._ctx, _ptr(cls), int(B), int(H), int(W), _ptr(mask), _ptr(out), _stream(self.device)))
        return out

    def grounding_downsample_classes(self, cls: torch.Tensor, n_classes: int, resize: int, convs) -> torch.Tensor:
        """grounding_downsample(one-hot planes of cls, n_classes, resize, "nearest", convs) from the class map u8 [B, 1, H, W] itself:
        -> [B, out, resize/4, resize/4], bit for bit (gl_op_grounding_downsample_classes)."""
        cls = self._class_map(cls, "grounding_downsample_classes")
        B, H, W = cls.shape
        w1, b1, w2, b2 = (_f32(t.detach(), self.device) for t in convs)
        if w1.shape[1] != n_classes:
            raise ValueError(f"grounding_downsample_classes: the first conv reads {w1.shape[1]} channels, the map has {n_classes} classes")
        out = torch.empty((B, w2.shape[0], resize // 4, resize // 4), device=self.device, dtype=torch.float32)
        check(self.lib.gl_op_grounding_downsample_classes(self._ctx, _ptr(cls), int(B), int(H), int(W), int(n_classes), int(resize), _ptr(w1), _ptr(b1),
                                                          int(w1.shape[0]), _ptr(w2), _ptr(b2), int(w2.shape[0]), _ptr(out), _stream(self.device)))
        return out

    def op_class_conv_wgrad(self, cls: torch.Tensor, dy: torch.Tensor, n_classes: int, R: int, kind: str):
        """Weight and bias gradient of a conv over F.interpolate(one_hot(cls), R, mode="nearest"), from the class map u8 [B, 1, H, W]
        itself (gl_op_class_conv_wgrad). kind "in_conv": Conv2d(n_classes, 3, 3, 1, 1), dy [B, 3, R, R]; "down": Conv2d(n_classes,
        c_out, 4, 2, 1), dy [B, c_out, R/2, R/2]. Returns (dW [c_out, n_classes, k, k], db [c_out]); the same bits on every call."""
        if kind not in ("in_conv", "down"):
            raise ValueError(f"op_class_conv_wgrad: kind {kind!r}; 'in_conv' or 'down' is built")
        cls = self._class_map(cls, "op_class_conv_wgrad")
        B, H, W = cls.shape
        dy = _f32(dy, self.device)
        Ro, k = (int(R) // 2, 4) if kind == "down" else (int(R), 3)
        if dy.dim() != 4 or dy.shape[0] != B or (int(R) > 0 and tuple(dy.shape[2:]) != (Ro, Ro)):
            raise ValueError(f"op_class_conv_wgrad: dy is {tuple(dy.shape)}; [{B}, c_out, {Ro}, {Ro}] is read")
        c_out = int(dy.shape[1])
        dW = torch.empty((c_out, max(int(n_classes), 0), k, k), device=self.device, dtype=torch.float32)
        db = torch.empty((c_out,), device=self.device, dtype=torch.float32)
        check(self.lib.gl_op_class_conv_wgrad(self._ctx, 1 if kind == "down" else 0, _ptr(cls), int(B), int(H), int(W), int(n_classes), int(R), _ptr(dy), c_out,
                                              _ptr(dW), _ptr(db), _stream(self.device)))
        return dW, db

    def set_fuser_scale(self, scale: float) -> None:
        check(self.lib.gl_unet_set_fuser_scale(self._ctx, C.c_float(float(scale)), _stream(self.device)))

    def set_fuser_scales(self, scales) -> None:
        """One gate multiplier per fuser module, in module order (for models whose fusers carry different `scale` values)."""
        arr = (C.c_float * len(scales))(*[float(v) for v in scales])
        check(self.lib.gl_unet_set_fuser_scales(self._ctx, arr, len(scales), _stream(self.device)))

    def restore_first_conv(self, weight: torch.Tensor, bias: torch.Tensor) -> None:
        w, b = _f32(weight, self.device), _f32(bias, self.device)
        check(self.lib.gl_unet_restore_first_conv(self._ctx, _ptr(w), _ptr(b), _stream(self.device)))
        self._keep_conv = (w, b)

    def unet_forward(self, x: torch.Tensor, timesteps: torch.Tensor, inpaint_extra: Optional[torch.Tensor] = None,
                     batch: Optional[int] = None) -> torch.Tensor:
        dev = self.device
        x = _f32(x, dev)
        t = timesteps.to(device=dev, dtype=torch.int64).contiguous()
        Beff = int(batch or t.shape[0])
        extra = None if inpaint_extra is None else _f32(inpaint_extra, dev)
        out = torch.empty((Beff, self.unet_cfg["out_channels"], x.shape[2], x.shape[3]), device=dev, dtype=torch.float32)
        check(self.lib.gl_unet_forward(self._ctx, Beff, int(x.shape[2]), int(x.shape[3]), _ptr(x), int(x.shape[0]), _ptr(t),
                                       _ptr(extra), 0 if extra is None else int(extra.shape[0]), _ptr(out), _stream(self.device)))
        return out

    def unet_profile(self, x: torch.Tensor, timesteps: torch.Tensor, inpaint_extra: Optional[torch.Tensor] = None,
                     batch: Optional[int] = None):
        """One eager UNet evaluation with HIP events around every GEMM / conv / attention / norm launch (on the launch
        stream); returns [dict(name, calls, ms, flops, bytes)] aggregated by kernel symbol, longest total time first."""
        dev = self.device
        x = _f32(x, dev)
        t = timesteps.to(device=dev, dtype=torch.int64).contiguous()
        Beff = int(batch or t.shape[0])
        extra = None if inpaint_extra is None else _f32(inpaint_extra, dev)
        out = torch.empty((Beff, self.unet_cfg["out_channels"], x.shape[2], x.shape[3]), device=dev, dtype=torch.float32)
        recs = (_lib.ProfRec * 512)()
        n = C.c_int(0)
        check(self.lib.gl_unet_profile(self._ctx, Beff, int(x.shape[2]), int(x.shape[3]), _ptr(x), int(x.shape[0]), _ptr(t),
                                       _ptr(extra), 0 if extra is None else int(extra.shape[0]), _ptr(out), recs, 512, C.byref(n),
                                       _stream(self.device)))
        return [dict(name=recs[i].name.decode(), calls=recs[i].calls, ms=recs[i].ms, flops=recs[i].flops, bytes=recs[i].bytes)
                for i in range(n.value)]

    def set_vae_tiling(self, mode="off", tile=vae_tiling.DEFAULT_TILE, overlap=vae_tiling.DEFAULT_OVERLAP) -> None:
        """The default of vae_decode / vae_encode on this context (a fork starts with its parent's): mode 'off' (the untiled pass),
        'on' (overlapping tiles blended by tile_blend_kernel; one tile per axis is the untiled pass itself) or 'auto' (untiled where
        it fits the arena, tiles where it does not); tile and overlap in latent pixels, an integer or (y, x). Tiles have their own
        GroupNorm statistics and attention: 'on' is not the untiled result."""
        vae_tiling.check_tiling(tile, overlap)
        self._vae_tiling = (vae_tiling.check_mode(mode), tile, overlap)

    def _vae_tiling_args(self, tiling, tile, overlap):
        mode, t0, o0 = self._vae_tiling
        mode = mode if tiling is None else vae_tiling.check_mode(tiling)
        tile, overlap = (t0 if tile is None else tile), (o0 if overlap is None else overlap)
        if mode != "off":
            vae_tiling.check_tiling(tile, overlap)
        return mode, tile, overlap

    def _vae_plan(self, kind: str, B: int, h: int, w: int, tile, overlap):
        """(Plan2D, gl_tile_plan with its device tables) of a decode ('dec') or encode ('enc') of B latents of h x w; kept per shape."""
        (th, tw), (ovy, ovx) = vae_tiling.check_tiling(tile, overlap)
        key = (kind, B, h, w, th, tw, ovy, ovx)
        hit = self._vae_plans.get(key)
        if hit is not None:
            return hit
        f = 2 ** self.vae_cfg["n_up"]
        p = vae_tiling.Plan2D(h, w, (th, tw), (ovy, ovx))
        s_in, s_out = (1, f) if kind == "dec" else (f, 1)
        wy, wx = p.tables(s_out)
        dev = self.device
        win = np.array([(b, oy * s_in, ox * s_in) for b in range(B) for oy in p.oy for ox in p.ox], dtype=np.int32)
        t = dict(windows=torch.from_numpy(win).to(dev), oy=torch.tensor([o * s_out for o in p.oy], dtype=torch.int32, device=dev),
                 ox=torch.tensor([o * s_out for o in p.ox], dtype=torch.int32, device=dev),
                 wy=torch.from_numpy(wy).contiguous().to(dev), wx=torch.from_numpy(wx).contiguous().to(dev))
        c = _lib.TilePlan(struct_size=C.sizeof(_lib.TilePlan), ny=p.ny, nx=p.nx, th_in=p.th * s_in, tw_in=p.tw * s_in, th_out=p.th * s_out,
                          tw_out=p.tw * s_out, **{k: v.data_ptr() for k, v in t.items()})
        if len(self._vae_plans) >= 16:
            self._vae_plans.pop(next(iter(self._vae_plans)))
        self._vae_plans[key] = (p, c, t)
        return self._vae_plans[key]

    def tile_gather(self, src: torch.Tensor, windows, th: int, tw: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gl_op_tile_gather: the windows (b, oy, ox) of size th x tw of src fp32 [B, C, H, W] as tiles [n, C, th, tw], an exact copy."""
        assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous()
        B, Cn, H, W = src.shape
        win = torch.as_tensor(np.asarray(windows, dtype=np.int32).reshape(-1, 3)).to(self.device)
        if out is None:
            out = torch.empty((win.shape[0], Cn, th, tw), device=self.device, dtype=torch.float32)
        assert out.is_contiguous() and tuple(out.shape) == (win.shape[0], Cn, th, tw)
        check(self.lib.gl_op_tile_gather(self._ctx, _ptr(src), int(B), int(Cn), int(H), int(W), _ptr(win), int(win.shape[0]), _ptr(out), int(th), int(tw),
                                         _stream(self.device)))
        return out

    def tile_blend(self, tiles: torch.Tensor, out: torch.Tensor, oy, ox, wy, wx, first_tile: int = 0) -> torch.Tensor:
        """gl_op_tile_blend: tiles fp32 [n, C, TH, TW] = the tiles first_tile .. first_tile + n - 1 (index (b ny + ty) nx + tx) of the plan
        with output-grid origins oy / ox and fp32 weight tables wy [ny, TH], wx [nx, TW], blended into out fp32 [B, C, H, W] in place."""
        assert tiles.is_cuda and tiles.dtype == torch.float32 and tiles.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32
        dev = self.device
        t = dict(oy=torch.as_tensor(np.asarray(oy, dtype=np.int32)).to(dev), ox=torch.as_tensor(np.asarray(ox, dtype=np.int32)).to(dev),
                 wy=torch.as_tensor(np.ascontiguousarray(wy, dtype=np.float32)).to(dev), wx=torch.as_tensor(np.ascontiguousarray(wx, dtype=np.float32)).to(dev))
        n, Cn, TH, TW = tiles.shape
        assert tuple(t["wy"].shape) == (len(oy), TH) and tuple(t["wx"].shape) == (len(ox), TW) and out.shape[1] == Cn
        c = _lib.TilePlan(struct_size=C.sizeof(_lib.TilePlan), ny=len(oy), nx=len(ox), th_in=TH, tw_in=TW, th_out=TH, tw_out=TW,
                          **{k: v.data_ptr() for k, v in t.items()})
        B, _, H, W = out.shape
        check(self.lib.gl_op_tile_blend(self._ctx, _ptr(tiles), int(first_tile), int(n), C.byref(c), _ptr(out), int(B), int(Cn), int(H), int(W),
                                        _stream(self.device)))
        torch.cuda.current_stream(dev).synchronize()          # the tables above are this call's own: they must outlive the launch
        return out

    def _vae_auto(self, key, untiled, tiled):
        """'auto': the untiled call where it fits the arena; where the arena refuses it, the tiled one -- and straight away from then on
        for that shape on this context. An exhausted arena leaves nothing behind: every pass starts by resetting it."""
        if key not in self._vae_tiled_shapes:
            try:
                return untiled()
            except _lib.GligenAmdError as e:
                if "workspace arena exhausted" not in str(e):
                    raise
            self._vae_tiled_shapes.add(key)
        return tiled()

    def vae_decode(self, z: torch.Tensor, tiling=None, tile=None, overlap=None, tiles_per_pass: Optional[int] = None) -> torch.Tensor:
        """AutoencoderKL.decode. tiling: None (this context's set_vae_tiling default), 'off', 'on' or 'auto'; tile / overlap in latent
        pixels; tiles_per_pass: how many tiles one pass decodes as a batch (default: eight 64 x 64 tiles' worth)."""
        dev = self.device
        z = _f32(z, dev)
        B, _, h, w = z.shape
        mode, tile, overlap = self._vae_tiling_args(tiling, tile, overlap)
        if mode == "auto":
            return self._vae_auto(("dec", B, h, w), lambda: self.vae_decode(z, "off"),
                                  lambda: self.vae_decode(z, "on", tile, overlap, tiles_per_pass))
        f = 2 ** self.vae_cfg["n_up"]
        out = torch.empty((B, self.vae_cfg["out_ch"], h * f, w * f), device=dev, dtype=torch.float32)
        if mode == "on":
            p, c, _ = self._vae_plan("dec", B, h, w, tile, overlap)
            if not p.single:
                n = int(tiles_per_pass) if tiles_per_pass is not None else max(1, (8 * 64 * 64) // (p.th * p.tw))
                check(self.lib.gl_vae_decode_tiled(self._ctx, int(B), int(h), int(w), _ptr(z), _ptr(out), C.byref(c), n, _stream(self.device)))
                return out
        # samples are independent: batches beyond 8 images at 64 x 64 go through in slices, so the arena (sized for the benchmark's
        # batch) bounds the activations whatever the caller's batch is
        n = max(1, (8 * 64 * 64) // (h * w))
        for i in range(0, B, n):
            m = min(n, B - i)
            check(self.lib.gl_vae_decode(self._ctx, int(m), int(h), int(w), _ptr(z[i:i + m]), _ptr(out[i:i + m]), _stream(self.device)))
        return out

    def vae_encode(self, img: torch.Tensor, noise: torch.Tensor, tiling=None, return_moments: bool = False, tile=None, overlap=None,
                   tiles_per_pass: Optional[int] = None):
        """AutoencoderKL.encode: img [B,3,H,W] in [-1,1], noise [B,zc,H/8,W/8] (the posterior's randn draw) -> latent. tiling, tile,
        overlap (latent pixels) and tiles_per_pass as in vae_decode; return_moments (tiled form only): (latent, the blended raw
        moments [B, 2 zc, H/f, W/f] the posterior was drawn from)."""
        dev = self.device
        img, noise = _f32(img, dev), _f32(noise, dev)
        B, _, H, W = img.shape
        mode, tile, overlap = self._vae_tiling_args(tiling, tile, overlap)
        if return_moments and mode == "off":
            raise ValueError("vae_encode: return_moments needs vae_tiling 'on' or 'auto' (only the tiled form hands out the moments)")
        f = 2 ** self.vae_cfg["n_up"]
        if mode == "auto":
            return self._vae_auto(("enc", B, H, W), lambda: self._vae_encode_untiled(img, noise, return_moments),
                                  lambda: self.vae_encode(img, noise, "on", return_moments, tile, overlap, tiles_per_pass))
        if mode == "on":
            if H % f or W % f:
                raise ValueError(f"vae_encode: image size {H} x {W} must be divisible by the encoder stride {f}")
            h, w = H // f, W // f
            p, c, _ = self._vae_plan("enc", B, h, w, tile, overlap)
            if not p.single:
                out = torch.empty_like(noise)
                moments = torch.empty((B, 2 * self.vae_cfg["z_channels"], h, w), device=dev, dtype=torch.float32) if return_moments else None
                # the analogue of vae_decode's rule, in image pixels: eight 512 x 512 tiles' worth per pass
                k = int(tiles_per_pass) if tiles_per_pass is not None else max(1, (8 * 512 * 512) // (p.th * p.tw * f * f))
                check(self.lib.gl_vae_encode_tiled(self._ctx, int(B), int(H), int(W), _ptr(img), _ptr(noise), _ptr(out), _ptr(moments),
                                                   C.byref(c), k, _stream(self.device)))
                return (out, moments) if return_moments else out
        return self._vae_encode_untiled(img, noise, return_moments)       # one tile per axis is the untiled pass itself

    def _vae_encode_untiled(self, img, noise, with_moments: bool):
        """The untiled encode in slices of the batch; with_moments: through gl_vae_encode_tiled's single-tile form, which is the same
        launches writing the moments where the caller can read them."""
        B, _, H, W = img.shape
        out = torch.empty_like(noise)
        n = max(1, (8 * 512 * 512) // (H * W))       # (slices of the batch, as in vae_decode)
        if not with_moments:
            for i in range(0, B, n):
                m = min(n, B - i)
                check(self.lib.gl_vae_encode(self._ctx, int(m), int(H), int(W), _ptr(img[i:i + m]), _ptr(noise[i:i + m]), _ptr(out[i:i + m]),
                                             _stream(self.device)))
            return out
        f = 2 ** self.vae_cfg["n_up"]
        moments = torch.empty((B, 2 * self.vae_cfg["z_channels"], H // f, W // f), device=self.device, dtype=torch.float32)
        one = _lib.TilePlan(struct_size=C.sizeof(_lib.TilePlan), ny=1, nx=1, th_in=H, tw_in=W, th_out=H // f, tw_out=W // f)
        for i in range(0, B, n):
            m = min(n, B - i)
            check(self.lib.gl_vae_encode_tiled(self._ctx, int(m), int(H), int(W), _ptr(img[i:i + m]), _ptr(noise[i:i + m]), _ptr(out[i:i + m]),
                                               _ptr(moments[i:i + m]), C.byref(one), 1, _stream(self.device)))
        return out, moments

    def _sampler_args(self, a, who, x, timesteps, fuser_scale, guidance_scale, inpaint_extra, mask, x0, noise, sqrt_ac, sqrt_1mac,
                      use_graph, sd_first_conv, restore_at):
        """The fields gl_plms_args and gl_solver_args share, written into `a`; returns what has to outlive the call."""
        dev = self.device
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        n = len(timesteps)
        ts = np.ascontiguousarray(timesteps, dtype=np.int64)
        a.struct_size = C.sizeof(type(a))
        a.B, a.h, a.w, a.n_steps = int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), n
        a.timesteps = ts.ctypes.data_as(C.POINTER(C.c_int64))
        keep = [ts]
        if fuser_scale is not None:
            fs = np.ascontiguousarray(fuser_scale, dtype=np.float32)
            a.fuser_scale = fs.ctypes.data_as(C.POINTER(C.c_float))
            keep.append(fs)
        a.guidance_scale = float(guidance_scale)
        a.x = x.data_ptr()
        if inpaint_extra is not None:
            inpaint_extra = _f32(inpaint_extra, dev); keep.append(inpaint_extra); a.inpaint_extra = inpaint_extra.data_ptr()
        if mask is not None:
            mask, x0, noise = _f32(mask, dev), _f32(x0, dev), _f32(noise, dev)
            B, Cl, h, w = x.shape
            if (mask.dim() != 4 or tuple(mask.shape[1:]) != (1, h, w) or x0.dim() != 4 or tuple(x0.shape[1:]) != (Cl, h, w)
                    or noise.dim() != 5 or noise.shape[0] != n or tuple(noise.shape[2:]) != (Cl, h, w)
                    or any(int(b) not in (1, B) for b in (mask.shape[0], x0.shape[0], noise.shape[1]))):
                raise ValueError(f"{who}: mask {tuple(mask.shape)}, x0 {tuple(x0.shape)}, noise {tuple(noise.shape)} do not fit "
                                 f"a latent {tuple(x.shape)} over {n} steps ([B|1,1,h,w], [B|1,C,h,w], [S,B|1,C,h,w])")
            sa = np.ascontiguousarray(sqrt_ac, dtype=np.float32); s1 = np.ascontiguousarray(sqrt_1mac, dtype=np.float32)
            keep += [mask, x0, noise, sa, s1]
            a.mask, a.x0, a.noise = mask.data_ptr(), x0.data_ptr(), noise.data_ptr()
            a.mask_B, a.x0_B, a.noise_B = int(mask.shape[0]), int(x0.shape[0]), int(noise.shape[1])
            a.sqrt_ac = sa.ctypes.data_as(C.POINTER(C.c_float)); a.sqrt_1mac = s1.ctypes.data_as(C.POINTER(C.c_float))
        a.use_graph = int(bool(use_graph))
        if sd_first_conv is not None:
            cw, cb = _f32(sd_first_conv[0], dev), _f32(sd_first_conv[1], dev)
            keep += [cw, cb]
            a.sd_conv_w, a.sd_conv_b = cw.data_ptr(), cb.data_ptr()
            if not 0 <= restore_at < n:
                raise ValueError(f"{who}: sd_first_conv needs restore_at = the step index it is swapped in at")
            a.sd_conv_step = int(restore_at)
        return keep

    def sample_plms(self, x: torch.Tensor, timesteps: np.ndarray, a_t: np.ndarray, a_prev: np.ndarray,
                    fuser_scale: Optional[np.ndarray], guidance_scale: float, *, inpaint_extra=None, mask=None, x0=None,
                    noise=None, sqrt_ac=None, sqrt_1mac=None, use_graph: bool = True, sd_first_conv=None,
                    restore_at: int = -1, ddim: bool = False) -> torch.Tensor:
        """In-place PLMS (or, ddim=True, eta-0 DDIM) loop on x (fp32 [B,C,h,w]); conditioning must already be set.
        Inpainting: mask [B|1,1,h,w], x0 [B|1,C,h,w], noise [S,B|1,C,h,w] (batch 1 broadcasts over the latent batch, as
        the reference's q_sample(x0, ts) * mask does). sd_first_conv = (weight, bias) swapped in before step restore_at."""
        a = PlmsArgs()
        keep = self._sampler_args(a, "sample_plms", x, timesteps, fuser_scale, guidance_scale, inpaint_extra, mask, x0, noise, sqrt_ac, sqrt_1mac,
                                  use_graph, sd_first_conv, restore_at)
        at = np.ascontiguousarray(a_t, dtype=np.float32)
        ap = np.ascontiguousarray(a_prev, dtype=np.float32)
        a.a_t = at.ctypes.data_as(C.POINTER(C.c_float))
        a.a_prev = ap.ctypes.data_as(C.POINTER(C.c_float))
        keep += [at, ap]
        a.ddim = int(bool(ddim))
        check(self.lib.gl_sample_plms(self._ctx, C.byref(a), _stream(self.device)))
        self._keep_plms = keep
        return x

    def sample_solver(self, x: torch.Tensor, timesteps: np.ndarray, a_t: np.ndarray, coefs: np.ndarray,
                      fuser_scale: Optional[np.ndarray], guidance_scale: float, *, step_noise=None, inpaint_extra=None, mask=None, x0=None,
                      noise=None, sqrt_ac=None, sqrt_1mac=None, use_graph: bool = True, sd_first_conv=None,
                      restore_at: int = -1) -> torch.Tensor:
        """In-place linear multistep solver loop on x (gl_sample_solver): per step one evaluation at timesteps[i], D0 = (x - sqrt(1 - a_t) e) /
        sqrt(a_t), then x <- cx x + c0 D0 + c1 D1 [+ c2 D2] [+ cn z]. coefs: [S, 3] = (cx, c0, c1) (what dpm_solver_coefficients returns),
        [S, 4] with cn behind them when step_noise [S, B, C, h, w] is given, or a dict with keys cx, c0, c1 and optionally c2, cn.
        The other arguments are sample_plms'."""
        a = SolverArgs()
        keep = self._sampler_args(a, "sample_solver", x, timesteps, fuser_scale, guidance_scale, inpaint_extra, mask, x0, noise, sqrt_ac, sqrt_1mac,
                                  use_graph, sd_first_conv, restore_at)
        n = len(timesteps)
        if isinstance(coefs, dict):
            cols = dict(coefs)
        else:
            cf = np.asarray(coefs, dtype=np.float64)
            if cf.ndim != 2 or cf.shape[0] != n or cf.shape[1] not in (3, 4):
                raise ValueError(f"sample_solver: coefs has shape {cf.shape}, need [{n}, 3] = (cx, c0, c1) or [{n}, 4] with cn")
            cols = dict(zip(("cx", "c0", "c1", "cn"), cf.T))
        unknown = set(cols) - {"cx", "c0", "c1", "c2", "cn"}
        if unknown or not {"cx", "c0", "c1"} <= set(cols):
            raise ValueError(f"sample_solver: coefs has the columns {sorted(cols)}, need cx, c0, c1 and optionally c2, cn")
        if ("cn" in cols) != (step_noise is not None):
            raise ValueError("sample_solver: the noise term needs both the cn column and step_noise")
        for name, col in list(cols.items()) + [("a_t", a_t)]:
            arr = np.ascontiguousarray(col, dtype=np.float32)
            if arr.shape != (n,):
                raise ValueError(f"sample_solver: {name} has shape {arr.shape}, need ({n},)")
            setattr(a, name, arr.ctypes.data_as(C.POINTER(C.c_float)))
            keep.append(arr)
        if step_noise is not None:
            step_noise = _f32(step_noise, self.device)
            if tuple(step_noise.shape) != (n, *x.shape):
                raise ValueError(f"sample_solver: step_noise {tuple(step_noise.shape)} is not [S, B, C, h, w] = {(n, *x.shape)}")
            keep.append(step_noise)
            a.step_noise = step_noise.data_ptr()
        check(self.lib.gl_sample_solver(self._ctx, C.byref(a), _stream(self.device)))
        self._keep_plms = keep
        return x

    def op_solver_update(self, eps, x, a_t, cx, c0, *, guidance=None, d1=None, c1=0.0, d2=None, c2=0.0, z=None, cn=0.0, out=None):
        """One solver_update_kernel launch (gl_op_solver_update): eps fp32 [n], or [2, n] = [cond ; uncond] with `guidance`; returns
        (x_out, D0). out: the tensor x_out is written to (x itself for an in-place update; a new one when None)."""
        dev = self.device
        n = x.numel()
        assert eps.is_cuda and eps.dtype == torch.float32 and x.dtype == torch.float32
        assert eps.numel() == (2 * n if guidance is not None else n)
        out = torch.empty_like(x) if out is None else out
        d0 = torch.empty_like(x)
        opt = lambda t: None if t is None else _ptr(t)
        check(self.lib.gl_op_solver_update(self._ctx, _ptr(eps), int(guidance is not None), float(guidance if guidance is not None else 1.0), float(a_t),
                                           _ptr(x), _ptr(out), _ptr(d0), opt(d1), opt(d2), opt(z), float(cx), float(c0), float(c1), float(c2), float(cn),
                                           int(n), _stream(dev)))
        return out, d0

    def latent_renoise(self, src: torch.Tensor, size, mode: str = "bicubic", sa: float = 1.0, s1: float = 0.0,
                       noise: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gl_op_latent_renoise: sa * resize(src [B,C,h,w]) + s1 * noise [B|1,C,h2,w2] in one launch, size = (h2, w2); the start point of
        a partial sampling (image-to-image, the second pass of a two-pass generation). mode: nearest-exact, bilinear or bicubic with
        torch's F.interpolate semantics (align_corners=False, no antialias). noise=None: the plain resize times sa. At equal sizes the
        result is diffusion.q_sample's, bit for bit. out: a contiguous fp32 tensor of the output's shape on this device to write into."""
        if mode not in _lib.LATENT_RESIZE_MODES:
            raise ValueError(f"latent_renoise: mode {mode!r}: one of {sorted(_lib.LATENT_RESIZE_MODES)}")
        dev = self.device
        src = _f32(src, dev)
        if src.dim() != 4:
            raise ValueError(f"latent_renoise: src has shape {tuple(src.shape)}, need [B, C, h, w]")
        B, Cc, h, w = (int(v) for v in src.shape)
        h2, w2 = (int(v) for v in size)
        if noise is not None:
            noise = _f32(noise, dev)
            if noise.dim() != 4 or tuple(noise.shape[1:]) != (Cc, h2, w2) or int(noise.shape[0]) not in (1, B):
                raise ValueError(f"latent_renoise: noise {tuple(noise.shape)} is not [{B} or 1, {Cc}, {h2}, {w2}]")
        if out is None:
            out = torch.empty((B, Cc, h2, w2), device=dev, dtype=torch.float32)
        elif (not out.is_cuda or out.device != dev or out.dtype != torch.float32 or not out.is_contiguous()
              or tuple(out.shape) != (B, Cc, h2, w2)):
            raise ValueError(f"latent_renoise: out must be a contiguous fp32 tensor of shape {(B, Cc, h2, w2)} on {dev}")
        check(self.lib.gl_op_latent_renoise(self._ctx, _ptr(src), B, Cc, h, w, _ptr(out), h2, w2, _lib.LATENT_RESIZE_MODES[mode], float(sa), float(s1),
                                            _ptr(noise), 0 if noise is None else int(noise.shape[0]), _stream(dev)))
        return out

    def op_lora_merge(self, W: torch.Tensor, up: torch.Tensor, down: torch.Tensor, scale: float) -> torch.Tensor:
        """gl_op_lora_merge: W [N, K...] += scale * up [N, r...] @ down [r, K...] in place, on the current stream. W, up and down are
        contiguous fp32 tensors on this engine's device (anything else raises: the update is in place, so nothing is converted or
        copied); the dimensions behind the first are flattened, which makes a conv pair (down [r, Cin, kh, kw], up [Cout, r, 1, 1])
        the same call. Returns W."""
        for name, t in (("W", W), ("up", up), ("down", down)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or t.device != self.device:
                what = f"{t.dtype}, {'contiguous' if t.is_contiguous() else 'not contiguous'}, on {t.device}" if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"op_lora_merge: {name} must be a contiguous fp32 tensor on {self.device} (it is {what})")
            if t.dim() < 2:
                raise ValueError(f"op_lora_merge: {name} has shape {tuple(t.shape)}, need at least two dimensions")
        N, r = int(W.shape[0]), int(down.shape[0])
        K = int(np.prod(W.shape[1:]))
        if int(up.shape[0]) != N or up.numel() != N * r or down.numel() != r * K:
            raise ValueError(f"op_lora_merge: up {tuple(up.shape)} @ down {tuple(down.shape)} does not give W {tuple(W.shape)}")
        check(self.lib.gl_op_lora_merge(self._ctx, _ptr(W), _ptr(up), _ptr(down), N, K, r, float(scale), _stream(self.device)))
        return W

    def sampler_timing(self):
        """(mean UNet-evaluation ms over graph replays, first eager evaluation ms, number of evaluations)."""
        a, f, n = C.c_float(), C.c_float(), C.c_int()
        check(self.lib.gl_sampler_timing(self._ctx, C.byref(a), C.byref(f), C.byref(n)))
        return float(a.value), float(f.value), int(n.value)

    def to_uint8(self, img: torch.Tensor) -> torch.Tensor:
        img = _f32(img, self.device)
        B, Cc, H, W = img.shape
        out = torch.empty((B, H, W, Cc), device=self.device, dtype=torch.uint8)
        check(self.lib.gl_to_uint8(_ptr(img), _ptr(out), int(B), int(Cc), int(H * W), _stream(self.device)))
        return out

    def arena_high_water(self) -> int:
        v = C.c_size_t()
        check(self.lib.gl_arena_high_water(self._ctx, C.byref(v)))
        return int(v.value)

    def launch_count(self) -> int:
        v = C.c_int64()
        check(self.lib.gl_launch_count(self._ctx, C.byref(v)))
        return int(v.value)

    def box_calibrate(self) -> dict:
        """What this box delivers (gl_box_calibrate): float4-copy GB/s beyond the Infinity Cache, global->LDS DMA TB/s from L2, sustained
        dense bf16 MFMA TFLOP/s with every SIMD issuing."""
        from ._lib import BoxCalibration
        c = BoxCalibration()
        check(self.lib.gl_box_calibrate(self._ctx, C.byref(c), _stream(self.device)))
        return {"hbm_copy_GBps": round(float(c.hbm_copy_gbs), 1), "lds_dma_TBps": round(float(c.lds_dma_tbs), 2),
                "mfma_bf16_TFLOPs": round(float(c.mfma_bf16_tflops), 1)}

    def mfma_calibrate(self, shape: int = 0, waves_per_simd: int = 2, n_acc: int = 4, zero_data: bool = False, target_ms: float = 25.0) -> dict:
        """gl_mfma_calibrate: back-to-back bf16 MFMA issue on every SIMD for target_ms, with the shader clock the kernel measured over
        its own loop. shape 0 = 32x32x16, 1 = 16x16x32."""
        from ._lib import MfmaCalibration
        c = MfmaCalibration()
        check(self.lib.gl_mfma_calibrate(self._ctx, int(shape), int(waves_per_simd), int(n_acc), int(bool(zero_data)), float(target_ms), C.byref(c),
                                         _stream(self.device)))
        return {"shape": "32x32x16" if shape == 0 else "16x16x32", "waves_per_simd": int(waves_per_simd), "accumulators": int(n_acc),
                "data": "zeros" if zero_data else "random", "TFLOPs": round(float(c.tflops), 1), "sclk_MHz": round(float(c.sclk_mhz), 1),
                "ms": round(float(c.ms), 2), "cycles_per_mfma": round(float(c.cycles_per_mfma), 2),
                "frac_of_2.5PF": round(float(c.tflops) / 2500.0, 3)}

    def mfma_calibration_table(self, target_ms: float = 25.0) -> list:
        """The matrix VERDICT round 5 asked for: both shapes x 1 / 2 waves per SIMD x 8 accumulators (+ the 4-accumulator form of
        gl_box_calibrate and an all-zeros run), each >= 20 ms."""
        rows = []
        for shape in (0, 1):
            for wps in (1, 2):
                rows.append(self.mfma_calibrate(shape, wps, 8, False, target_ms))
        rows.append(self.mfma_calibrate(0, 2, 4, False, target_ms))
        rows.append(self.mfma_calibrate(0, 2, 8, True, target_ms))
        return rows

    def set_ff_rows_policy(self, mode: int) -> None:
        """Row-local feed-forward kernel or two GEMMs at C = 320 (gl_set_ff_rows_policy): -1 = decided by on-device timing (default),
        0 = never, 1 = wherever the kernel exists, 2 = static rule (deterministic kernel choice: the same output bits on every box,
        rank and run -- the timed default may pick the other form, which differs in the last bits). Process-wide."""
        check(self.lib.gl_set_ff_rows_policy(int(mode)))

    def set_cfg_shared_prefix(self, on: bool) -> None:
        """gl_set_cfg_shared_prefix: run the layers in front of the first conditioning-dependent one once per [cond ; uncond]
        evaluation of the sampler (default) or at the full batch like the rest. Process-wide; captured graphs are dropped."""
        check(self.lib.gl_set_cfg_shared_prefix(int(bool(on))))

    # ---- one named GEMM plan at a time (include/gligen_amd_gemm_plans.h; process-wide forcing, per-thread log)
    def gemm_force_plan(self, tm=0, tn=0, splits=0, grid_cap=0) -> None:
        """gl_gemm_force_plan: tile (units of 32), K split and resident-grid cap of the p / u kernels. A choice that does not fit a
        problem is planned as usual: gemm_plan_log tells what ran."""
        check(self.lib.gl_gemm_force_plan(int(tm), int(tn), int(splits), int(grid_cap)))

    def gemm_force_knobs(self, halo_splits, wide_splits, wide_xcd, xcd_boxes, halo, wide) -> None:
        """gl_gemm_force_knobs; every knob is given (gemm_force_clear puts the library's own defaults back)."""
        check(self.lib.gl_gemm_force_knobs(int(halo_splits), int(wide_splits), int(wide_xcd), int(xcd_boxes), int(halo), int(wide)))

    def gemm_force_clear(self) -> None:
        check(self.lib.gl_gemm_force_clear())

    def gemm_plan_log_clear(self) -> None:
        check(self.lib.gl_gemm_plan_log_clear())

    def gemm_plan_log(self):
        """(records, launches): the calling thread's GEMM launches since gemm_plan_log_clear as dicts (the newest 32, in launch
        order), and how many there were."""
        from ._lib import GemmPlanRecord
        recs = (GemmPlanRecord * 32)()
        n, total = C.c_int(0), C.c_int(0)
        check(self.lib.gl_gemm_plan_log(recs, 32, C.byref(n), C.byref(total)))
        out = [{f: (getattr(r, f).decode() if f == "kernel" else getattr(r, f)) for f, _ in GemmPlanRecord._fields_} for r in recs[:n.value]]
        return out, total.value

    # ---- conv8_kernel by name (include/gligen_amd_conv8.h)
    def conv8_force_knobs(self, on=1, bn=0, splits=0) -> None:
        """gl_conv8_force_knobs: the 8 x 8 level's stride-1 convs on conv8_kernel or not, their column tile and K split (0: shipped / model)."""
        check(self.lib.gl_conv8_force_knobs(int(on), int(bn), int(splits)))

    def op_conv8x8(self, x0, w, out, bn, splits, *, x1=None, bias=None, bias2=None, rows_per_b=64, res=None, act=0, slabs=None, grid_cap=0,
                   B=None, ldo=None):
        """gl_op_conv8x8 on the caller's tensors: x0 [B][8][8][C0] (x1 [..][C1]) bf16, w fp32 OIHW [N][C0 + C1][3][3], out [B 64][ldo] bf16
        or fp32 (by its dtype; it may be a view into a larger guarded buffer), slabs fp32 with room for splits x B 64 x N values."""
        from ._lib import Conv8Args
        a = Conv8Args()
        a.struct_size = C.sizeof(Conv8Args)
        a.x0 = _ptr(x0); a.x1 = _ptr(x1)
        a.C0 = x0.shape[-1]; a.C1 = 0 if x1 is None else x1.shape[-1]
        a.B = x0.shape[0] if B is None else B
        a.H = a.W = 8; a.N = w.shape[0]; a.stride = 1; a.ups = 0; a.pad_lo = 1
        a.w = _ptr(w); a.bias = _ptr(bias); a.bias2 = _ptr(bias2); a.bias2_ld = a.N; a.rows_per_b = rows_per_b
        a.res = _ptr(res); a.ldres = a.N; a.act = act; a.out_f32 = int(out.dtype == torch.float32)
        a.out = _ptr(out); a.ldo = a.N if ldo is None else ldo
        a.bn = bn; a.splits = splits; a.grid_cap = grid_cap
        a.slabs = _ptr(slabs); a.slab_bytes = 0 if slabs is None else slabs.numel() * 4
        check(self.lib.gl_op_conv8x8(self._ctx, C.byref(a), _stream(self.device)))

    def ff_rows_policy_report(self) -> str:
        buf = C.create_string_buffer(4096)
        check(self.lib.gl_ff_rows_policy_report(buf, 4096))
        return buf.value.decode()

    # ---- single operators (parity tests / per-kernel profiling) -------------------
    def op_linear(self, x, w, bias=None, res=None, act=0, out_f32=False):
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty((M, N), device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
        check(self.lib.gl_op_linear(self._ctx, _ptr(x), _ptr(w), _ptr(bias), _ptr(res), _ptr(y), M, N, K, act, int(out_f32), _stream(self.device)))
        return y

    def op_geglu(self, x, w_f32, b_f32):
        M, K = x.shape
        inner = w_f32.shape[0] // 2
        y = torch.empty((M, inner), device=x.device, dtype=torch.bfloat16)
        check(self.lib.gl_op_geglu(self._ctx, _ptr(x), _ptr(w_f32), _ptr(b_f32), _ptr(y), M, inner, K, _stream(self.device)))
        return y

    def op_ln_linear(self, a, w0, b0, res, gamma, beta, w1, b1, mode, inner_or_heads, T=0):
        """Producer GEMM + folded-LayerNorm consumer GEMM (gl_op_ln_linear). Returns (x, y, used_fold)."""
        M, K0 = a.shape
        Cc = w0.shape[0]
        x = torch.empty((M, Cc), device=a.device, dtype=torch.bfloat16)
        if mode == 0:
            y = torch.empty((M, inner_or_heads), device=a.device, dtype=torch.bfloat16)
        else:
            d = Cc // inner_or_heads
            dp = {40: 48, 80: 80, 160: 160}[d]
            y = torch.zeros((M // T * inner_or_heads, ((T + 127) // 128) * 128, dp), device=a.device, dtype=torch.bfloat16)
        used = C.c_int(-1)
        check(self.lib.gl_op_ln_linear(self._ctx, _ptr(a), M, K0, _ptr(w0), _ptr(b0), _ptr(res), Cc, _ptr(gamma), _ptr(beta), _ptr(w1),
                                       _ptr(b1), int(mode), int(inner_or_heads), int(T), _ptr(x), _ptr(y), C.byref(used), _stream(self.device)))
        return x, y, int(used.value)

    def op_feedforward(self, x, w1, b1, w2, b2, gamma=None, beta=None, res=None, gate=None, want_stats=False):
        """LayerNorm + GEGLU projection + FF-out + (gated) residual (gl_op_feedforward). Returns (y, stats | None, used_rows)."""
        M, Cc = x.shape
        y = torch.empty((M, Cc), device=x.device, dtype=torch.bfloat16)
        stats = torch.zeros((M, 2), device=x.device, dtype=torch.float32) if want_stats else None
        used = C.c_int(-1)
        check(self.lib.gl_op_feedforward(self._ctx, _ptr(x), M, Cc, _ptr(gamma), _ptr(beta), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                                         _ptr(res), _ptr(gate), _ptr(y), _ptr(stats), C.byref(used), _stream(self.device)))
        return y, stats, int(used.value)

    def op_ff_chain(self, x, pre_w, pre_b, pre_res, gamma, beta, w1, b1, w2, b2, pre_gate=None, gate=None, post_w=None, post_b=None, post_res=None):
        """Leading projection + residual, LayerNorm, feed-forward + residual (, trailing projection + residual) in one row-local
        launch (gl_op_ff_chain)."""
        M, Cc = x.shape
        y = torch.empty((M, Cc), device=x.device, dtype=torch.bfloat16)
        check(self.lib.gl_op_ff_chain(self._ctx, _ptr(x), M, Cc, _ptr(pre_w), _ptr(pre_b), _ptr(pre_res), _ptr(pre_gate), _ptr(gamma), _ptr(beta),
                                      _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(gate), _ptr(post_w), _ptr(post_b), _ptr(post_res), _ptr(y),
                                      _stream(self.device)))
        return y

    def op_adamw_step(self, p, g, m, v, step, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """In-place AdamW update of a flat fp32 tensor (gl_op_adamw_step; torch.optim.AdamW semantics)."""
        for t in (p, g, m, v):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
        check(self.lib.gl_op_adamw_step(self._ctx, _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(lr), float(betas[0]), float(betas[1]),
                                        float(eps), float(weight_decay), int(step), _stream(self.device)))

    ADAMW_EMA_GRID = (16384, 256, 4)     # adamw_ema_kernel's grid cap, block size and elements per lane (train_optim.hip)

    def op_adamw_ema_step(self, p, g, m, v, ema, step, *, ema_rate, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """op_adamw_step's update of p, m, v (the same bits) and ema = ema_rate * ema + (1 - ema_rate) * p_new in the same pass
        (gl_op_adamw_ema_step; trainer.py:388-391: opt.step(), then update_ema). Flat fp32 tensors of one length; views at any 4-byte
        offset are taken (the kernel's scalar path)."""
        for t in (p, g, m, v, ema):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
        check(self.lib.gl_op_adamw_ema_step(self._ctx, _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), p.numel(), float(lr), float(betas[0]), float(betas[1]),
                                            float(eps), float(weight_decay), float(ema_rate), int(step), _stream(self.device)))

    # ---- include/gligen_amd_train_run.h: gradient accumulation, the global norm, the clipping coefficient, the clipped update
    GRAD_NORM_GRID = (16384, 64, 6, 4)   # grad_sqnorm_kernel (train_run.hip): elements per partial, squares per thread chain, wave levels, waves

    @staticmethod
    def _flat(*ts):
        for t in ts:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == ts[0].numel()

    def op_grad_accumulate(self, acc, g, mode: str, k: int):
        """One micro-batch of a gradient accumulation over flat fp32 tensors (gl_op_grad_accumulate). mode 'first': acc = g; 'middle':
        acc = acc + g; 'last': g = (acc + g) * fl(1 / k), acc left alone -- the mean of the k gradients lands in the gradient buffer."""
        self._flat(acc, g)
        check(self.lib.gl_op_grad_accumulate(self._ctx, _ptr(acc), _ptr(g), g.numel(), _lib.GRAD_ACCUM_MODES[mode], int(k), _stream(self.device)))

    def grad_sqnorm_partials(self, n: int) -> int:
        """The number of partial sums op_grad_sqnorm writes for n elements: ceil(n / GRAD_NORM_GRID[0]), a function of n alone."""
        return int(self.lib.gl_grad_sqnorm_partials(int(n)))

    def op_grad_sqnorm(self, g, partials=None):
        """The squared L2 norm of a flat fp32 tensor as fp32 partial sums in a fixed order (gl_op_grad_sqnorm), written to `partials`
        (grad_sqnorm_partials(g.numel()) floats; created when None) and returned."""
        self._flat(g)
        count = self.grad_sqnorm_partials(g.numel())
        if partials is None:
            partials = torch.empty(count, device=g.device, dtype=torch.float32)
        assert partials.is_cuda and partials.dtype == torch.float32 and partials.is_contiguous() and partials.numel() == count
        check(self.lib.gl_op_grad_sqnorm(self._ctx, _ptr(g), g.numel(), _ptr(partials), _stream(self.device)))
        return partials

    def op_clip_coef(self, partials, max_norm: float, out2=None):
        """out2 = (norm, min(1, max_norm / (norm + 1e-6))) from the partial sums of one or several ranges (gl_op_clip_coef): what
        torch.nn.utils.clip_grad_norm_ computes, left on the device. Returns out2 (fp32 [2])."""
        assert partials.is_cuda and partials.dtype == torch.float32 and partials.is_contiguous()
        if out2 is None:
            out2 = torch.empty(2, device=partials.device, dtype=torch.float32)
        assert out2.is_cuda and out2.dtype == torch.float32 and out2.is_contiguous() and out2.numel() == 2
        check(self.lib.gl_op_clip_coef(self._ctx, _ptr(partials), partials.numel(), float(max_norm), _ptr(out2), _stream(self.device)))
        return out2

    def op_adamw_clip_step(self, p, g, m, v, step, *, coef, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """op_adamw_step on g * coef (gl_op_adamw_clip_step): coef is a one-element fp32 device tensor (op_clip_coef's out2[1:2]) the
        kernel reads, so nothing waits for the host; g is not written."""
        self._flat(p, g, m, v)
        assert coef.is_cuda and coef.dtype == torch.float32 and coef.numel() == 1
        check(self.lib.gl_op_adamw_clip_step(self._ctx, _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(lr), float(betas[0]), float(betas[1]),
                                             float(eps), float(weight_decay), int(step), _ptr(coef), _stream(self.device)))

    def op_adamw_ema_clip_step(self, p, g, m, v, ema, step, *, ema_rate, coef, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """op_adamw_ema_step on g * coef (gl_op_adamw_ema_clip_step), coef as in op_adamw_clip_step."""
        self._flat(p, g, m, v, ema)
        assert coef.is_cuda and coef.dtype == torch.float32 and coef.numel() == 1
        check(self.lib.gl_op_adamw_ema_clip_step(self._ctx, _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), p.numel(), float(lr), float(betas[0]),
                                                 float(betas[1]), float(eps), float(weight_decay), float(ema_rate), int(step), _ptr(coef),
                                                 _stream(self.device)))

    @staticmethod
    def count_spatial_transformers(cfg: Mapping) -> int:
        """The number of SpatialTransformers of a UNetModel config, walked as gl_unet_train_step numbers them (openaimodel.py:307-383):
        one behind every ResBlock of the input and output paths whose level's downsampling rate is in attention_resolutions, and the
        middle block's. 16 for the shipped topology."""
        levels, nres, attn = len(cfg["channel_mult"]), int(cfg["num_res_blocks"]), {int(a) for a in cfg["attention_resolutions"]}
        n, ds = 0, 1
        for level in range(levels):
            n += nres * (ds in attn)
            if level != levels - 1:
                ds *= 2
        n += 1
        for level in reversed(range(levels)):
            n += (nres + 1) * (ds in attn)
            if level:
                ds //= 2
        return n

    def train_weight_cache(self, enable: bool = True) -> int:
        """Keep the bf16 operand copies of the frozen parameters across unet_train_step calls (gl_train_weight_cache); returns the bytes
        held. Only for callers that change nothing but the parameters they ask gradients for (TrainStep does); enable=False frees them."""
        n = C.c_size_t(0)
        check(self.lib.gl_train_weight_cache(self._ctx, 1 if enable else 0, C.byref(n)))
        return int(n.value)

    def unet_train_step(self, cfg: Mapping, state_dict: Mapping[str, torch.Tensor], batch: Mapping[str, torch.Tensor], fuser_scale: float = 1.0,
                        trainable=None, grads: Optional[Mapping[str, torch.Tensor]] = None, checkpoint: bool = False, use_weight_cache: bool = False,
                        *, loss_weights: Optional[torch.Tensor] = None, adapters=None):
        """One training iteration of the reference (trainer.py:353-392: model(input), mse_loss(model_output, noise), backward) on the
        device (gl_unet_train_step). cfg: UNetModel kwargs -- any tokenizer; cfg["fuser_type"] gatedSA (default), gatedSA2 (a square number
        of grounding tokens and H == W) or gatedCA (no fuser.linear.* keys) --; state_dict: the model's parameters (fp32, on this
        device: they are used in place); batch: x [B, 4, H, W] (noised latent), timesteps [B], context [B, 77, 768], boxes, masks,
        positive_embeddings (or, for the text+image tokenizer, text_embeddings, image_embeddings, text_masks, image_masks), target [B, 4, H, W] (the noise).
        A spatial-map model (cfg["grounding_tokenizer"] one of the five *_grounding_net targets; gl_unet_train_step_spatial) takes the map
        under the reference's key (canny_edge, hed_edge, depth, normal, sem), mask [B] and grounding_extra_input instead of the boxes.
        The sem model also trains from class maps: `sem` and `grounding_extra_input` both torch.uint8 [B, 1, H, W] or [B, H, W]
        (gl_unet_train_step_spatial_classes) give the loss, eps and gradients of their one-hot planes bit for bit, except in_conv's and
        downsample_net.layers.0's gradients, which are summed in another order; one u8 and one float input is a ValueError.
        An inpainting model (cfg["inpaint_mode"], discrete tokenizers; trainer.py:339-344) also takes inpainting_extra_input
        [B, 5, H, W] = cat(z * mask, mask), concatenated to x in front of the 9-channel first conv (openaimodel.py:445-447), and the
        gradient of input_blocks.0.0.weight is returned with the others. Instead of x / target (and inpainting_extra_input) any model
        takes x_rows [B, H, W, channels of the first conv] and target_rows [B, H, W, 4], the pixel rows train_step_inputs writes: the
        same bits, without the two permute copies.
        Returns (loss, eps [B, 4, H, W], grads) with grads over the reference's
        trainable set (train.trainable_names: trainer.py:189-245) or the `trainable` names given; `grads`: buffers to
        write into instead of fresh ones (every entry is overwritten); `checkpoint`: keep only block inputs / outputs and recompute each block's
        forward in its backward (the same gradients bit for bit, a fraction of the arena); `use_weight_cache`: keep / reuse the bf16
        operand copies of the tensors no gradient is asked for (train_weight_cache: only when those tensors never change).
        `adapters` (gl_unet_train_step_lora; discrete tokenizers): LoRA adapters in training, a sequence of mappings with name (the
        state_dict key of a frozen Linear's weight: gligen_amd.lora_train.adapter_sites), down [r, K], up [N, r], scale and optionally
        g_down / g_up, fp32 tensors on this device used in place; gradients that are not given are created. The layer computes
        x W^T + scale (x down^T) up^T. The adapters' gradients come back as a fourth value, {name: (g_down, g_up)}; `trainable=[]`
        trains the adapters alone.
        `loss_weights` (fp32 [B] on this device; gl_train_set_loss_weights, called right before the step, which clears them): the loss
        becomes (w[:, None, None, None] * (eps - target) ** 2).mean(), e.g. gligen_amd.train.min_snr_weights(...)[t]; None: mse_loss,
        the launches and bits of a step without weights."""
        dev = self.device
        c = UNetConfig()
        c.in_channels, c.out_channels, c.model_channels = cfg["in_channels"], cfg["out_channels"], cfg["model_channels"]
        c.num_res_blocks, c.num_heads, c.context_dim = cfg["num_res_blocks"], cfg["num_heads"], cfg["context_dim"]
        c.n_mult = len(cfg["channel_mult"])
        for i, v in enumerate(cfg["channel_mult"]):
            c.channel_mult[i] = int(v)
        c.n_attn = len(cfg["attention_resolutions"])
        for i, v in enumerate(cfg["attention_resolutions"]):
            c.attention_resolutions[i] = int(v)
        sp = spatial_train_config(cfg)          # a spatial-map tokenizer (canny / depth / normal / hed / sem_grounding_net.py)?
        if sp and adapters is not None:
            raise ValueError("unet_train_step: adapters are trained on the discrete-tokenizer models (text, text+image, keypoint)")
        ti = sp is None and "image_embeddings" in batch     # the text+image tokenizer (text_image_grounding_net.py)
        kp = sp is None and "points" in batch               # the keypoint tokenizer (keypoint_grounding_net.py); else the text tokenizer
        c.grounding_kind, c.fuser_kind = (3 if sp else 1 if ti else 2 if kp else 0), _lib.fuser_kind(cfg.get("fuser_type", "gatedSA"))
        c.max_persons = int(batch["points"].shape[1]) // 17 if kp else 0
        c.gr_in_dim = c.gr_out_dim = 768
        inpaint = bool(cfg.get("inpaint_mode"))
        c.inpaint_mode = int(inpaint)
        if sp:
            c.extra_channels = sp["ds"]["out"] if sp["ds"] else 0
            c.tok_resize, c.tok_in_dim = sp["tok_resize"], sp["tok_in_dim"]
        names = [k for k in state_dict.keys()]
        params = [_f32(state_dict[k], dev) for k in names]
        if trainable is None:
            from .train import trainable_names
            trainable = trainable_names(state_dict, cfg)
        if grads is None:
            grads = {k: torch.zeros_like(p) for k, p in zip(names, params) if k in set(trainable)}
        else:       # caller-owned gradient buffers (gligen_amd.dist.GradBuckets.views: the backward writes straight into the flat buckets)
            for k, gt in grads.items():
                assert gt.is_cuda and gt.dtype == torch.float32 and gt.is_contiguous() and tuple(gt.shape) == tuple(state_dict[k].shape), k
        if "x_rows" in batch:       # pixel rows as train_step_inputs writes them: used in place
            x_rows, target_rows = _f32(batch["x_rows"], dev), _f32(batch["target_rows"], dev)
            cin = c.in_channels * 2 + 1 if inpaint else c.in_channels
            if x_rows.dim() != 4 or target_rows.dim() != 4 or x_rows.shape[:3] != target_rows.shape[:3] or x_rows.shape[3] != cin \
                    or target_rows.shape[3] != c.out_channels:
                raise ValueError(f"unet_train_step: x_rows is [B, H, W, {cin}] and target_rows [B, H, W, {c.out_channels}] for this model; got "
                                 f"{tuple(x_rows.shape)} and {tuple(target_rows.shape)}")
            B, H, W = (int(v) for v in x_rows.shape[:3])
        else:
            x, target = batch["x"], batch["target"]
            B, Cx, H, W = x.shape
            rows = lambda t: _f32(t, dev).permute(0, 2, 3, 1).reshape(B, H * W, t.shape[1]).contiguous()
            if inpaint:             # the first conv reads cat(x, inpainting_extra_input) (openaimodel.py:445-447)
                if batch.get("inpainting_extra_input") is None:
                    raise ValueError("unet_train_step: an inpainting model's batch carries inpainting_extra_input [B, 5, H, W] (or x_rows)")
                x = torch.cat([_f32(x, dev), _f32(batch["inpainting_extra_input"], dev)], dim=1)
            x_rows, target_rows = rows(x), rows(target)
        n = len(names)
        narr = (C.c_char_p * n)(*[k.encode() for k in names])
        parr = (C.c_void_p * n)(*[p.data_ptr() for p in params])
        garr = (C.c_void_p * n)(*[(grads[k].data_ptr() if k in grads else None) for k in names])
        eps = torch.empty((B, H * W, c.out_channels), device=dev, dtype=torch.float32)
        loss = torch.zeros(1, device=dev, dtype=torch.float32)
        if loss_weights is not None:
            lw = loss_weights
            if not (torch.is_tensor(lw) and lw.is_cuda and lw.device == torch.device(dev) and lw.dtype == torch.float32 and lw.is_contiguous()
                    and tuple(lw.shape) == (B,)):
                raise ValueError(f"unet_train_step: loss_weights is a contiguous fp32 tensor of shape ({B},) on {dev}")
        # (set right before the step's own call: that call takes the weights and clears them, whatever it returns)
        weigh = (lambda: check(self.lib.gl_train_set_loss_weights(self._ctx, _ptr(loss_weights), B))) if loss_weights is not None else (lambda: None)
        if sp and (batch[sp["map_key"]].dtype == torch.uint8 or (sp["ds"] and batch["grounding_extra_input"].dtype == torch.uint8)):
            # the semantic-map model from u8 class maps (gl_unet_train_step_spatial_classes): both inputs are class maps
            if not sp["ds"]:
                raise ValueError("unet_train_step: a class map trains a model with a grounding downsampler; this config has none")
            cm = self._class_map(batch[sp["map_key"]], "unet_train_step")
            ce = self._class_map(batch["grounding_extra_input"], "unet_train_step")
            if cm.shape[0] != B or ce.shape[0] != B:
                raise ValueError(f"unet_train_step: the class maps hold {cm.shape[0]} and {ce.shape[0]} samples, x holds {B}")
            keep = dict(x=x_rows, t=_f32(batch["timesteps"], dev), ctx=_f32(batch["context"], dev), target=target_rows, mask=_f32(batch["mask"].reshape(-1), dev))
            if keep["mask"].shape[0] != B:
                raise ValueError("unet_train_step: one mask value per sample")
            ds = sp["ds"]
            u = _lib.TrainUNetIn(int(B), int(H), int(W), int(keep["ctx"].shape[1]), (sp["tok_resize"] // 32) ** 2, keep["x"].data_ptr(), keep["t"].data_ptr(),
                                 keep["ctx"].data_ptr(), None, None, None, keep["target"].data_ptr(), float(fuser_scale), None, None, None,
                                 int(bool(checkpoint)), int(bool(use_weight_cache)))
            s = _lib.TrainSpatialClassesIn(cm.data_ptr(), int(cm.shape[1]), int(cm.shape[2]), keep["mask"].data_ptr(), ce.data_ptr(), int(ce.shape[1]), int(ce.shape[2]),
                                           ds["resize"], ds["mode"], ds["n_in"], ds["mid"])
            weigh()
            check(self.lib.gl_unet_train_step_spatial_classes(self._ctx, C.byref(c), C.byref(u), C.byref(s), n, narr, parr, garr, _ptr(eps), _ptr(loss), _stream(dev)))
            return loss, eps.reshape(B, H, W, c.out_channels).permute(0, 3, 1, 2).contiguous(), grads
        if sp:      # batch: the map under the reference's key, mask, grounding_extra_input (gl_unet_train_step_spatial)
            keep = dict(x=x_rows, t=_f32(batch["timesteps"], dev), ctx=_f32(batch["context"], dev), target=target_rows,
                        map=_f32(batch[sp["map_key"]], dev), mask=_f32(batch["mask"].reshape(-1), dev))
            if keep["mask"].shape[0] != B:
                raise ValueError("unet_train_step: one mask value per sample")
            ds = sp["ds"]
            extra = _f32(batch["grounding_extra_input"], dev) if ds else None
            u = _lib.TrainUNetIn(int(B), int(H), int(W), int(keep["ctx"].shape[1]), (sp["tok_resize"] // 32) ** 2, keep["x"].data_ptr(), keep["t"].data_ptr(),
                                 keep["ctx"].data_ptr(), None, None, None, keep["target"].data_ptr(), float(fuser_scale), None, None, None,
                                 int(bool(checkpoint)), int(bool(use_weight_cache)))
            m = keep["map"]
            s = _lib.TrainSpatialIn(m.data_ptr(), int(m.shape[1]), int(m.shape[2]), int(m.shape[3]), keep["mask"].data_ptr(),
                                    extra.data_ptr() if ds else None, *((int(extra.shape[1]), int(extra.shape[2]), int(extra.shape[3])) if ds else (0, 0, 0)),
                                    ds["resize"] if ds else 0, ds["mode"] if ds else 0, ds["n_in"] if ds else 0, ds["mid"] if ds else 0)
            weigh()
            check(self.lib.gl_unet_train_step_spatial(self._ctx, C.byref(c), C.byref(u), C.byref(s), n, narr, parr, garr, _ptr(eps), _ptr(loss), _stream(dev)))
            return loss, eps.reshape(B, H, W, c.out_channels).permute(0, 3, 1, 2).contiguous(), grads
        keep = dict(x=x_rows, t=_f32(batch["timesteps"], dev), ctx=_f32(batch["context"], dev), boxes=_f32(batch["points" if kp else "boxes"], dev),
                    masks=_f32(batch["masks"], dev), pe=None if kp else _f32(batch["text_embeddings" if ti else "positive_embeddings"], dev), target=target_rows)
        if ti:
            keep.update(tm=_f32(batch["text_masks"], dev), im=_f32(batch["image_masks"], dev), ie=_f32(batch["image_embeddings"], dev))
        u = _lib.TrainUNetIn(int(B), int(H), int(W), int(keep["ctx"].shape[1]), int(keep["boxes"].shape[1]), keep["x"].data_ptr(), keep["t"].data_ptr(),
                             keep["ctx"].data_ptr(), keep["boxes"].data_ptr(), keep["masks"].data_ptr(), None if kp else keep["pe"].data_ptr(), keep["target"].data_ptr(),
                             float(fuser_scale), keep["tm"].data_ptr() if ti else None, keep["im"].data_ptr() if ti else None,
                             keep["ie"].data_ptr() if ti else None, int(bool(checkpoint)), int(bool(use_weight_cache)))
        if adapters is not None:
            aarr, agrads = self._lora_adapters(adapters, state_dict)
            weigh()
            check(self.lib.gl_unet_train_step_lora(self._ctx, C.byref(c), C.byref(u), n, narr, parr, garr, aarr, len(aarr), _ptr(eps), _ptr(loss), _stream(dev)))
            return loss, eps.reshape(B, H, W, c.out_channels).permute(0, 3, 1, 2).contiguous(), grads, agrads
        weigh()
        check(self.lib.gl_unet_train_step(self._ctx, C.byref(c), C.byref(u), n, narr, parr, garr, _ptr(eps), _ptr(loss), _stream(dev)))
        return loss, eps.reshape(B, H, W, c.out_channels).permute(0, 3, 1, 2).contiguous(), grads

    def _lora_adapters(self, adapters, state_dict):
        """The gl_lora_adapter array of unet_train_step's `adapters`, and {name: (g_down, g_up)}."""
        dev = torch.device(self.device)
        arr = (_lib.LoraAdapter * len(adapters))()
        agrads = {}
        for i, a in enumerate(adapters):
            name, down, up = a["name"], a["down"], a["up"]
            if name not in state_dict:
                raise ValueError(f"unet_train_step: adapter for '{name}', which is not in the state_dict")
            w = state_dict[name]
            N, r = int(w.shape[0]), int(down.shape[0])
            K = w.numel() // N
            g_down = a.get("g_down") if a.get("g_down") is not None else torch.zeros_like(down)
            g_up = a.get("g_up") if a.get("g_up") is not None else torch.zeros_like(up)
            dshape = (r, int(w.shape[1]), 3, 3) if (w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)) else (r, K)      # a 3 x 3 conv's down is OIHW
            for what, t, shape in (("down", down, dshape), ("up", up, (N, r)), ("g_down", g_down, dshape), ("g_up", g_up, (N, r))):
                if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
                    raise ValueError(f"unet_train_step: adapter '{name}': {what} is a contiguous fp32 tensor of shape {shape} on {self.device}; got "
                                     f"{tuple(t.shape)} {t.dtype} on {t.device}")
            arr[i] = _lib.LoraAdapter(name.encode(), down.data_ptr(), up.data_ptr(), g_down.data_ptr(), g_up.data_ptr(), r, float(a["scale"]))
            agrads[name] = (g_down, g_up)
        return arr, agrads

    def train_step_inputs(self, z: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor, schedule, *, boxes: Optional[torch.Tensor] = None,
                          mask: Optional[torch.Tensor] = None, inpaint: bool = False) -> Dict[str, torch.Tensor]:
        """What the reference's trainer computes between the VAE and the model (trainer.py:329-364), in one launch
        (gl_train_step_inputs), as the pixel rows unet_train_step takes: x_noisy = a[t] z + s[t] noise (q_sample, ldm.py:19-22, the bits
        torch gives on the CPU) and, with inpaint, z * mask and the mask behind it (trainer.py:342-344). z, noise [B, C, H, W];
        timesteps [B] integers; schedule: the diffusion's buffers, a mapping with sqrt_alphas_cumprod and sqrt_one_minus_alphas_cumprod
        (or that pair), best kept on this device. inpaint takes exactly one of boxes [B, Nb, 4] -- (x0, y0, x1, y1) fractions in
        [0, 1], the mask of draw_masks_from_boxes(boxes, H) without its random branches (H == W); anything else is a ValueError -- and
        mask [B, 1, H, W] / [B, H, W] / [B, H*W], e.g. the reference's random stroke masks, which are drawn on the host.
        Returns dict(x_rows [B, H, W, 2C + 1 or C], target_rows [B, H, W, C] = the noise, timesteps [B] float)."""
        dev = self.device
        if z.dim() != 4 or tuple(noise.shape) != tuple(z.shape) or timesteps.numel() != z.shape[0]:
            raise ValueError("train_step_inputs: z and noise are [B, C, H, W] of one shape, timesteps [B]")
        B, Cz, H, W = (int(v) for v in z.shape)
        if not inpaint and (boxes is not None or mask is not None):
            raise ValueError("train_step_inputs: boxes / mask are the inpainting model's inputs (inpaint=True)")
        if inpaint and (boxes is None) == (mask is None):
            raise ValueError("train_step_inputs: an inpainting step takes boxes or mask, exactly one of them")
        if boxes is not None:
            if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4 or boxes.shape[1] < 1:
                raise ValueError("train_step_inputs: boxes are [B, Nb, 4]")
            if H != W:
                raise ValueError(f"train_step_inputs: the mask drawn from boxes is square (inpaint_mask_func.py:22); the latent is {H} x {W}")
            if not bool(((boxes >= 0) & (boxes <= 1)).all()):
                raise ValueError("train_step_inputs: box coordinates are fractions in [0, 1]")
            boxes = _f32(boxes, dev)
        if mask is not None:
            if mask.numel() != B * H * W:
                raise ValueError(f"train_step_inputs: the mask holds {mask.numel()} values, B H W = {B * H * W}")
            mask = _f32(mask, dev).reshape(B, H * W)
        if isinstance(schedule, Mapping):
            sa, s1 = schedule["sqrt_alphas_cumprod"], schedule["sqrt_one_minus_alphas_cumprod"]
        else:
            sa, s1 = schedule
        sa, s1 = _f32(torch.as_tensor(sa), dev).reshape(-1), _f32(torch.as_tensor(s1), dev).reshape(-1)
        if sa.numel() != s1.numel() or sa.numel() < 1:
            raise ValueError("train_step_inputs: the two schedule tables have one length")
        zd, nd = _f32(z, dev), _f32(noise, dev)
        t = timesteps.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        x_rows = torch.empty((B, H, W, 2 * Cz + 1 if inpaint else Cz), device=dev, dtype=torch.float32)
        target_rows = torch.empty((B, H, W, Cz), device=dev, dtype=torch.float32)
        t_float = torch.empty(B, device=dev, dtype=torch.float32)
        a = _lib.TrainStepInputsArgs(C.sizeof(_lib.TrainStepInputsArgs), B, Cz, H, W, int(sa.numel()), int(boxes.shape[1]) if boxes is not None else 0,
                                     int(bool(inpaint)), zd.data_ptr(), nd.data_ptr(), t.data_ptr(), sa.data_ptr(), s1.data_ptr(),
                                     boxes.data_ptr() if boxes is not None else None, mask.data_ptr() if mask is not None else None,
                                     x_rows.data_ptr(), target_rows.data_ptr(), t_float.data_ptr())
        check(self.lib.gl_train_step_inputs(self._ctx, C.byref(a), _stream(dev)))
        return dict(x_rows=x_rows, target_rows=target_rows, timesteps=t_float)

    def train_wait_grads(self, index: int, stream=None) -> None:
        """Make `stream` (a torch.cuda.Stream; None: the current one) wait until the gradients of the index-th SpatialTransformer of the
        last unet_train_step -- or, index = number of SpatialTransformers, position_net's -- are written (gl_train_wait_grads)."""
        h = C.c_void_p(stream.cuda_stream) if stream is not None else _stream(self.device)
        check(self.lib.gl_train_wait_grads(self._ctx, int(index), h))

    def st_train_param_names(self):
        names = self.lib.gl_train_st_param_names()
        return [names[i].decode() for i in range(43)]

    def op_st_train(self, state_dict, x, objs, context, target, heads, fuser_scale=1.0):
        """Training slice (gl_op_st_train): forward + backward of one SpatialTransformer (GroupNorm, proj_in, one gatedSA
        BasicTransformerBlock, proj_out, residual) under mse_loss(y, target). x / target [B, C, H, W] as the reference passes them;
        state_dict: the module's reference state_dict. Returns (y, loss, dx, dobjs, grads) with grads keyed by the trainable
        (transformer_blocks.0.fuser.*) names."""
        dev = self.device
        names = self.st_train_param_names()
        params = [_f32(state_dict[n], dev) for n in names]
        B, Cc, H, W = x.shape
        rows = lambda t: _f32(t, dev).permute(0, 2, 3, 1).reshape(B, H * W, Cc).contiguous()
        xr, tr = rows(x), rows(target)
        objs, context = _f32(objs, dev), _f32(context, dev)
        dims = TrainBlockDims(int(B), int(H * W), int(objs.shape[1]), int(Cc), int(heads), int(context.shape[1]), int(context.shape[2]), float(fuser_scale))
        y, dx, dobjs = torch.empty_like(xr), torch.empty_like(xr), torch.empty_like(objs)
        loss = torch.zeros(1, device=dev, dtype=torch.float32)
        grads = {n: torch.zeros_like(p) for n, p in zip(names, params) if n.startswith("transformer_blocks.0.fuser.")}
        parr = (C.c_void_p * 43)(*[p.data_ptr() for p in params])
        garr = (C.c_void_p * 43)(*[(grads[n].data_ptr() if n in grads else None) for n in names])
        check(self.lib.gl_op_st_train(self._ctx, C.byref(dims), parr, _ptr(xr), _ptr(objs), _ptr(context), _ptr(tr), _ptr(y), _ptr(loss), _ptr(dx),
                                      _ptr(dobjs), garr, _stream(dev)))
        back = lambda t: t.reshape(B, H, W, Cc).permute(0, 3, 1, 2).contiguous()
        return back(y), loss, back(dx), dobjs, grads

    def op_resample_train(self, mode, weight, bias, x, target):
        """Training slice (gl_op_resample_train): Downsample (mode "down": conv3x3 stride 2) or Upsample (mode "up": nearest 2x +
        conv3x3) forward, mse_loss(y, target) and the input gradient. x [B, C, H, W], target [B, C, Ho, Wo] (reference layout)."""
        dev = self.device
        B, Cc, H, W = x.shape
        Ho, Wo = target.shape[2], target.shape[3]
        rows = lambda t: _f32(t, dev).permute(0, 2, 3, 1).reshape(B, -1, Cc).contiguous()
        xr, tr = rows(x), rows(target)
        y, dx = torch.empty_like(tr), torch.empty_like(xr)
        loss = torch.zeros(1, device=dev, dtype=torch.float32)
        w, b = _f32(weight, dev), _f32(bias, dev)
        check(self.lib.gl_op_resample_train(self._ctx, 0 if mode == "down" else 1, int(B), int(H), int(W), int(Cc), _ptr(w), _ptr(b), _ptr(xr), _ptr(tr),
                                            _ptr(y), _ptr(loss), _ptr(dx), _stream(dev)))
        return (y.reshape(B, Ho, Wo, Cc).permute(0, 3, 1, 2).contiguous(), loss, dx.reshape(B, H, W, Cc).permute(0, 3, 1, 2).contiguous())

    def resblock_train_param_names(self):
        names = self.lib.gl_train_resblock_param_names()
        return [names[i].decode() for i in range(12)]

    def op_resblock_train(self, state_dict, x, emb, target):
        """Training slice (gl_op_resblock_train): forward + backward of one ResBlock under mse_loss(y, target). x [B, Cin, H, W],
        emb [B, emb_dim], target [B, Cout, H, W] as the reference passes them (NCHW; the library's pixel-row layout is a permutation);
        state_dict: the block's reference state_dict. Returns (y [B, Cout, H, W], loss, dx [B, Cin, H, W])."""
        dev = self.device
        names = self.resblock_train_param_names()
        params = [(_f32(state_dict[n], dev) if n in state_dict else None) for n in names]
        B, Cin, H, W = x.shape
        Cout = target.shape[1]
        rows = lambda t: _f32(t, dev).permute(0, 2, 3, 1).reshape(t.shape[0], H * W, t.shape[1]).contiguous()
        xr, tr, e = rows(x), rows(target), _f32(emb, dev)
        dims = TrainResDims(int(B), int(H), int(W), int(Cin), int(Cout), int(e.shape[1]))
        y = torch.empty((B, H * W, Cout), device=dev, dtype=torch.float32)
        dx = torch.empty((B, H * W, Cin), device=dev, dtype=torch.float32)
        loss = torch.zeros(1, device=dev, dtype=torch.float32)
        parr = (C.c_void_p * 12)(*[(p.data_ptr() if p is not None else None) for p in params])
        check(self.lib.gl_op_resblock_train(self._ctx, C.byref(dims), parr, _ptr(xr), _ptr(e), _ptr(tr), _ptr(y), _ptr(loss), _ptr(dx),
                                            _stream(dev)))
        back = lambda t, Cc: t.reshape(B, H, W, Cc).permute(0, 3, 1, 2).contiguous()
        return back(y, Cout), loss, back(dx, Cin)

    def block_train_param_names(self):
        names = self.lib.gl_train_block_param_names()
        return [names[i].decode() for i in range(37)]

    def op_block_train(self, state_dict, x, objs, context, target, heads, fuser_scale=1.0, fuser_type=None):
        """Training slice (gl_op_block_train): forward + backward of one BasicTransformerBlock under mse_loss(y, target).
        state_dict: the block's reference state_dict (fp32). Returns (y, loss, dx, dobjs, grads) with grads a dict over the fuser.*
        parameter names. fuser_type "gatedSA" / "gatedSA2" / "gatedCA" goes through gl_op_block_train_fuser (gatedSA: the same
        launches and bits as the default entry); a gatedCA block's state_dict has no fuser.linear.* and one that has is refused."""
        dev = self.device
        names = self.block_train_param_names()
        if fuser_type is not None:
            kind = _lib.fuser_kind(fuser_type)
            absent = [n for n in names if n not in state_dict and kind == 2 and n.startswith("fuser.linear.")]
            params = [(None if n in absent else _f32(state_dict[n], dev)) for n in names]
            x, objs, context, target = (_f32(t, dev) for t in (x, objs, context, target))
            B, N, Cc = x.shape
            dims = TrainBlockDims(int(B), int(N), int(objs.shape[1]), int(Cc), int(heads), int(context.shape[1]), int(context.shape[2]), float(fuser_scale))
            y, dx, dobjs = torch.empty_like(x), torch.empty_like(x), torch.empty_like(objs)
            loss = torch.zeros(1, device=dev, dtype=torch.float32)
            grads = {n: torch.zeros_like(p) for n, p in zip(names, params) if n.startswith("fuser.") and p is not None}
            parr = (C.c_void_p * 37)(*[(p.data_ptr() if p is not None else None) for p in params])
            garr = (C.c_void_p * 37)(*[(grads[n].data_ptr() if n in grads else None) for n in names])
            check(self.lib.gl_op_block_train_fuser(self._ctx, kind, C.byref(dims), parr, _ptr(x), _ptr(objs), _ptr(context), _ptr(target), _ptr(y),
                                                   _ptr(loss), _ptr(dx), _ptr(dobjs), garr, _stream(self.device)))
            return y, loss, dx, dobjs, grads
        params = [_f32(state_dict[n], dev) for n in names]
        x, objs, context, target = (_f32(t, dev) for t in (x, objs, context, target))
        B, N, Cc = x.shape
        dims = TrainBlockDims(int(B), int(N), int(objs.shape[1]), int(Cc), int(heads), int(context.shape[1]), int(context.shape[2]), float(fuser_scale))
        y, dx, dobjs = torch.empty_like(x), torch.empty_like(x), torch.empty_like(objs)
        loss = torch.zeros(1, device=dev, dtype=torch.float32)
        grads = {n: torch.zeros_like(p) for n, p in zip(names, params) if n.startswith("fuser.")}
        parr = (C.c_void_p * 37)(*[p.data_ptr() for p in params])
        garr = (C.c_void_p * 37)(*[(grads[n].data_ptr() if n in grads else None) for n in names])
        check(self.lib.gl_op_block_train(self._ctx, C.byref(dims), parr, _ptr(x), _ptr(objs), _ptr(context), _ptr(target), _ptr(y), _ptr(loss),
                                         _ptr(dx), _ptr(dobjs), garr, _stream(self.device)))
        return y, loss, dx, dobjs, grads

    def op_grid_resize(self, src, sg, sv):
        """gl_op_grid_resize: src [B, sg*sg, C] fp32 rows -> [B, sv*sv, C], torch's bicubic (align_corners=False) of the square grid:
        the gatedSA2 fuser's residual on the training path."""
        src = _f32(src, self.device)
        B, n, Cc = src.shape
        if n != sg * sg:
            raise ValueError(f"op_grid_resize: src holds {n} tokens per sample, sg * sg = {sg * sg}")
        dst = torch.empty((B, sv * sv, Cc), device=self.device, dtype=torch.float32)
        check(self.lib.gl_op_grid_resize(self._ctx, _ptr(src), int(B), int(sg), int(sv), int(Cc), _ptr(dst), _stream(self.device)))
        return dst

    def op_grid_resize_backward(self, g, sg, sv):
        """gl_op_grid_resize_backward: g [B, sv*sv, C] -> [B, sg*sg, C], the exact transpose of op_grid_resize (a gather, no atomics:
        two calls give the same bits)."""
        g = _f32(g, self.device)
        B, n, Cc = g.shape
        if n != sv * sv:
            raise ValueError(f"op_grid_resize_backward: g holds {n} pixels per sample, sv * sv = {sv * sv}")
        dsrc = torch.empty((B, sg * sg, Cc), device=self.device, dtype=torch.float32)
        check(self.lib.gl_op_grid_resize_backward(self._ctx, _ptr(g), int(B), int(sg), int(sv), int(Cc), _ptr(dsrc), _stream(self.device)))
        return dsrc

    # ---- include/gligen_amd_train_prims.h: the training path's primitives one by one. Each returns a dict of fp32 tensors by output
    # name. out=None produces every output the inputs allow; out={name: tensor} produces those and writes them into the caller's tensors
    # (contiguous fp32 on the engine's device, views included), which is how a test puts guard zones round them.
    def _prim_outs(self, shapes, out, required=()):
        if out is None:
            return {k: torch.empty(shape, device=self.device, dtype=torch.float32) for k, shape in shapes.items()}
        for k, t in out.items():
            if k not in shapes:
                raise ValueError(f"no output {k!r} for these inputs (one of {sorted(shapes)})")
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shapes[k]) or t.device != torch.device(self.device):
                raise ValueError(f"output {k!r}: a contiguous fp32 tensor of shape {tuple(shapes[k])} on {self.device} is needed")
        missing = [k for k in required if k not in out]
        if missing:
            raise ValueError(f"outputs {missing} are required")
        return dict(out)

    def op_train_attention(self, q, k, v, heads, dout=None, out=None):
        """gl_op_train_attention: q [B, Nq, H D], k / v [B, Nk, H D] -> o, lse [B, H, Nq]; with dout also dq, dk, dv. out without
        dk / dv is the training step's dq-only call."""
        dev = self.device
        q, k, v = (_f32(t, dev) for t in (q, k, v))
        dout = None if dout is None else _f32(dout, dev)
        B, Nq, HD = q.shape
        Nk = k.shape[1]
        if HD % heads or k.shape != (B, Nk, HD) or v.shape != k.shape or (dout is not None and dout.shape != q.shape):
            raise ValueError("op_train_attention: q / dout [B, Nq, H D], k / v [B, Nk, H D]")
        shapes = {"o": q.shape, "lse": (B, heads, Nq)}
        if dout is not None:
            shapes.update(dq=q.shape, dk=k.shape, dv=k.shape)
        o = self._prim_outs(shapes, out, required=("o", "lse"))
        check(self.lib.gl_op_train_attention(self._ctx, int(B), int(heads), int(HD // heads), int(Nq), int(Nk), _ptr(q), _ptr(k), _ptr(v), _ptr(dout),
                                             *[_ptr(o.get(n)) for n in ("o", "lse", "dq", "dk", "dv")], _stream(dev)))
        return o

    def op_train_linear(self, x, W, b=None, dy=None, out=None):
        """gl_op_train_linear: x [M, K], W [N, K], b [N] -> y [M, N]; with dy [M, N] also dx, dW, db."""
        dev = self.device
        x, W = _f32(x, dev), _f32(W, dev)
        b, dy = (None if t is None else _f32(t, dev) for t in (b, dy))
        (M, K), N = x.shape, W.shape[0]
        if W.shape != (N, K) or (b is not None and b.shape != (N,)) or (dy is not None and dy.shape != (M, N)):
            raise ValueError("op_train_linear: x [M, K], W [N, K], b [N], dy [M, N]")
        shapes = {"y": (M, N)}
        if dy is not None:
            shapes.update(dx=(M, K), dW=(N, K), db=(N,))
        o = self._prim_outs(shapes, out)
        check(self.lib.gl_op_train_linear(self._ctx, int(M), int(N), int(K), _ptr(x), _ptr(W), _ptr(b), _ptr(dy),
                                          *[_ptr(o.get(n)) for n in ("y", "dx", "dW", "db")], _stream(dev)))
        return o

    def op_train_layernorm(self, x, g, b, eps=1e-5, dy=None, accumulate=False, out=None):
        """gl_op_train_layernorm: x [R, C] -> y, xhat, rstd [R]; with dy also dx (added to out["dx"] when accumulate), dgamma, dbeta."""
        dev = self.device
        x, g, b = (_f32(t, dev) for t in (x, g, b))
        dy = None if dy is None else _f32(dy, dev)
        R, Cc = x.shape
        if g.shape != (Cc,) or b.shape != (Cc,) or (dy is not None and dy.shape != x.shape):
            raise ValueError("op_train_layernorm: x / dy [R, C], g / b [C]")
        shapes = {"y": x.shape, "xhat": x.shape, "rstd": (R,)}
        if dy is not None:
            shapes.update(dx=x.shape, dgamma=(Cc,), dbeta=(Cc,))
        o = self._prim_outs(shapes, out, required=("dx",) if accumulate else ())
        if accumulate and out is None:
            raise ValueError("op_train_layernorm: accumulate adds to out['dx']")
        check(self.lib.gl_op_train_layernorm(self._ctx, int(R), int(Cc), C.c_float(eps), _ptr(x), _ptr(g), _ptr(b), _ptr(dy), 1 if accumulate else 0,
                                             *[_ptr(o.get(n)) for n in ("y", "xhat", "rstd", "dx", "dgamma", "dbeta")], _stream(dev)))
        return o

    def op_train_groupnorm(self, x, g, b, silu=True, eps=1e-5, da=None, accumulate=False, out=None):
        """gl_op_train_groupnorm: pixel rows x [B, HW, C], 32 groups -> a, xhat, rstd [B, 32]; with da also dx (added to out["dx"] when
        accumulate)."""
        dev = self.device
        x, g, b = (_f32(t, dev) for t in (x, g, b))
        da = None if da is None else _f32(da, dev)
        B, HW, Cc = x.shape
        if g.shape != (Cc,) or b.shape != (Cc,) or (da is not None and da.shape != x.shape):
            raise ValueError("op_train_groupnorm: x / da [B, HW, C], g / b [C]")
        shapes = {"a": x.shape, "xhat": x.shape, "rstd": (B, 32)}
        if da is not None:
            shapes.update(dx=x.shape)
        o = self._prim_outs(shapes, out, required=("dx",) if accumulate else ())
        if accumulate and out is None:
            raise ValueError("op_train_groupnorm: accumulate adds to out['dx']")
        check(self.lib.gl_op_train_groupnorm(self._ctx, int(B), int(HW), int(Cc), 1 if silu else 0, C.c_float(eps), _ptr(x), _ptr(g), _ptr(b), _ptr(da),
                                             1 if accumulate else 0, *[_ptr(o.get(n)) for n in ("a", "xhat", "rstd", "dx")], _stream(dev)))
        return o

    def op_train_geglu(self, u, dh=None, out=None):
        """gl_op_train_geglu: u [R, 2 I] = (val | gate) -> h [R, I]; with dh also du [R, 2 I]."""
        dev = self.device
        u = _f32(u, dev)
        dh = None if dh is None else _f32(dh, dev)
        R, I2 = u.shape
        if I2 % 2 or (dh is not None and dh.shape != (R, I2 // 2)):
            raise ValueError("op_train_geglu: u [R, 2 I], dh [R, I]")
        shapes = {"h": (R, I2 // 2)}
        if dh is not None:
            shapes.update(du=u.shape)
        o = self._prim_outs(shapes, out)
        check(self.lib.gl_op_train_geglu(self._ctx, int(R), int(I2 // 2), _ptr(u), _ptr(dh), _ptr(o.get("h")), _ptr(o.get("du")), _stream(dev)))
        return o

    def op_train_dot(self, a, b, mode, alpha=None, scale=1.0, out=None):
        """gl_op_train_dot: mode 0: scale (1 - tanh(alpha)^2) sum(a b); mode 1: mean((a - b)^2). Returns {"out": [1]}."""
        dev = self.device
        a, b = _f32(a, dev).reshape(-1), _f32(b, dev).reshape(-1)
        alpha = None if alpha is None else _f32(alpha, dev)
        if a.shape != b.shape:
            raise ValueError("op_train_dot: a and b hold the same number of elements")
        o = self._prim_outs({"out": (1,)}, out, required=("out",))
        check(self.lib.gl_op_train_dot(self._ctx, int(a.numel()), _ptr(a), _ptr(b), _ptr(alpha), C.c_float(scale), int(mode), _ptr(o["out"]), _stream(dev)))
        return o

    def op_train_conv3(self, x, w, bias=None, geom=0, dy=None, out=None):
        """gl_op_train_conv3: pixel rows x [B, H, W, Cin], w [Cout, Cin, 3, 3] -> y [B, Ho, Wo, Cout] (geom 0: stride 1; 1: Downsample,
        Ho = H / 2; 2: Upsample, Ho = 2 H); with dy (like y) also dx (like x)."""
        dev = self.device
        x, w = _f32(x, dev), _f32(w, dev)
        bias, dy = (None if t is None else _f32(t, dev) for t in (bias, dy))
        (B, H, W, Cin), Cout = x.shape, w.shape[0]
        ys = {0: (B, H, W, Cout), 1: (B, H // 2, W // 2, Cout), 2: (B, 2 * H, 2 * W, Cout)}.get(geom, (B, H, W, Cout))
        if w.shape != (Cout, Cin, 3, 3) or (bias is not None and bias.shape != (Cout,)) or (dy is not None and tuple(dy.shape) != ys):
            raise ValueError("op_train_conv3: x [B, H, W, Cin], w [Cout, Cin, 3, 3], bias [Cout], dy [B, Ho, Wo, Cout]")
        shapes = {"y": ys}
        if dy is not None:
            shapes.update(dx=x.shape)
        o = self._prim_outs(shapes, out, required=("y",))
        check(self.lib.gl_op_train_conv3(self._ctx, int(B), int(H), int(W), int(Cin), int(Cout), int(geom), _ptr(x), _ptr(w), _ptr(bias), _ptr(dy),
                                         _ptr(o["y"]), _ptr(o.get("dx")), _stream(dev)))
        return o

    def op_train_conv_direct(self, x, w, bias=None, c0=0, n=None, dy=None, out=None):
        """gl_op_train_conv_direct: pixel rows x [B, H, W, Cin], w [Cout, Cin, 3, 3] -> y [B, H, W, Cout]; with dy (like y) also dx
        [B, H, W, n], the gradient of the input channels [c0, c0 + n) (n None: all behind c0), and dW (like w)."""
        dev = self.device
        x, w = _f32(x, dev), _f32(w, dev)
        bias, dy = (None if t is None else _f32(t, dev) for t in (bias, dy))
        (B, H, W, Cin), Cout = x.shape, w.shape[0]
        n = Cin - c0 if n is None else n
        if w.shape != (Cout, Cin, 3, 3) or (bias is not None and bias.shape != (Cout,)) or (dy is not None and dy.shape != (B, H, W, Cout)):
            raise ValueError("op_train_conv_direct: x [B, H, W, Cin], w [Cout, Cin, 3, 3], bias [Cout], dy [B, H, W, Cout]")
        shapes = {"y": (B, H, W, Cout)}
        if dy is not None:
            shapes.update(dx=(B, H, W, n), dW=w.shape)
        o = self._prim_outs(shapes, out, required=("y",))
        check(self.lib.gl_op_train_conv_direct(self._ctx, int(B), int(H), int(W), int(Cin), int(Cout), int(c0), int(n), _ptr(x), _ptr(w), _ptr(bias),
                                               _ptr(dy), _ptr(o["y"]), _ptr(o.get("dx")), _ptr(o.get("dW")), _stream(dev)))
        return o

    # ---- include/gligen_amd_train_lora.h: the low-rank part of one adapted Linear by itself
    def op_lora_linear(self, x, down, up, scale=1.0, dy=None, down_kr=False, up_rn=False, out=None):
        """gl_op_lora_linear: x [M, K]; down [r, K] (down_kr: [K, r]); up [N, r] (up_rn: [r, N]). t [M, r] = x down^T and
        y [M, N] += scale t up^T; with dy [M, N] also u [M, r] = dy up, dx [M, K] += scale u down, g_down = scale u^T x and
        g_up = scale dy^T t in the layouts of down and up. y and dx are accumulated into: they come in through `out` (out=None starts
        them at zero)."""
        dev = self.device
        x, down, up = (_f32(t, dev) for t in (x, down, up))
        dy = None if dy is None else _f32(dy, dev)
        M, K = x.shape
        r = int(down.shape[1] if down_kr else down.shape[0])
        N = int(up.shape[1] if up_rn else up.shape[0])
        if tuple(down.shape) != ((K, r) if down_kr else (r, K)) or tuple(up.shape) != ((r, N) if up_rn else (N, r)) or (dy is not None and dy.shape != (M, N)):
            raise ValueError("op_lora_linear: x [M, K], down [r, K] (down_kr: [K, r]), up [N, r] (up_rn: [r, N]), dy [M, N]")
        shapes = {"t": (M, r), "y": (M, N)}
        if dy is not None:
            shapes.update(u=(M, r), dx=(M, K), g_down=tuple(down.shape), g_up=tuple(up.shape))
        if out is None:
            o = {k: torch.zeros(shape, device=dev, dtype=torch.float32) for k, shape in shapes.items()}
        else:
            o = self._prim_outs(shapes, out)
        check(self.lib.gl_op_lora_linear(self._ctx, int(M), int(K), int(N), r, C.c_float(scale), int(bool(down_kr)), int(bool(up_rn)), _ptr(x), _ptr(down),
                                         _ptr(up), _ptr(dy), *[_ptr(o.get(n)) for n in ("t", "y", "u", "dx", "g_down", "g_up")], _stream(dev)))
        return o

    # ---- include/gligen_amd_train_lora_conv.h: the low-rank part of one adapted 3 x 3 conv by itself
    def op_lora_conv3(self, x, down, up, scale=1.0, geom=0, dy=None, out=None):
        """gl_op_lora_conv3: pixel rows x [B, H, W, Ci]; down [r, Ci, 3, 3]; up [Co, r]; geom 0 stride 1 (output H x W), 1 Downsample
        (H/2 x W/2), 2 Upsample (2H x 2W). t [B, Ho, Wo, r] = im2col(x) down^T and y [B, Ho, Wo, Co] += scale t up^T; with dy (like y)
        also u [B, Ho, Wo, r] = dy up, dx (like x) += scale (transposed conv of u with down), g_down (like down) and g_up (like up).
        y and dx are accumulated into: they come in through `out` (out=None starts them at zero)."""
        dev = self.device
        x, down, up = (_f32(t, dev) for t in (x, down, up))
        dy = None if dy is None else _f32(dy, dev)
        if x.dim() != 4 or down.dim() != 4 or up.dim() != 2:
            raise ValueError("op_lora_conv3: x [B, H, W, Ci], down [r, Ci, 3, 3], up [Co, r]")
        (B, H, W, Ci), r, Co = x.shape, int(down.shape[0]), int(up.shape[0])
        Ho, Wo = (H // 2, W // 2) if geom == 1 else (2 * H, 2 * W) if geom == 2 else (H, W)
        if tuple(down.shape) != (r, Ci, 3, 3) or tuple(up.shape) != (Co, r) or (dy is not None and tuple(dy.shape) != (B, Ho, Wo, Co)):
            raise ValueError("op_lora_conv3: x [B, H, W, Ci], down [r, Ci, 3, 3], up [Co, r], dy [B, Ho, Wo, Co]")
        shapes = {"t": (B, Ho, Wo, r), "y": (B, Ho, Wo, Co)}
        if dy is not None:
            shapes.update(u=(B, Ho, Wo, r), dx=tuple(x.shape), g_down=tuple(down.shape), g_up=tuple(up.shape))
        if out is None:
            o = {k: torch.zeros(shape, device=dev, dtype=torch.float32) for k, shape in shapes.items()}
        else:
            o = self._prim_outs(shapes, out)
        check(self.lib.gl_op_lora_conv3(self._ctx, int(B), int(H), int(W), int(Ci), int(Co), r, C.c_float(scale), int(geom), _ptr(x), _ptr(down), _ptr(up),
                                        _ptr(dy), *[_ptr(o.get(n)) for n in ("t", "y", "u", "dx", "g_down", "g_up")], _stream(dev)))
        return o

    def lora_wgrad_chunk_rows(self, M: int) -> int:
        """Rows per partial sum of the low-rank weight-gradient kernel over M rows (gl_lora_wgrad_chunk_rows)."""
        return int(self.lib.gl_lora_wgrad_chunk_rows(int(M)))

    def op_conv3x3(self, x0, w_oihw, bias, x1=None, stride=1, ups=0, pad_lo=1, res=None):
        B, H, W, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[3]
        Cout = w_oihw.shape[0]
        Hup, Wup = H << ups, W << ups
        if stride == 1:
            Ho, Wo = Hup, Wup
        else:
            Ho = (Hup + (2 if pad_lo else 1) - 3) // 2 + 1
            Wo = (Wup + (2 if pad_lo else 1) - 3) // 2 + 1
        y = torch.empty((B, Ho, Wo, Cout), device=x0.device, dtype=torch.bfloat16)
        check(self.lib.gl_op_conv3x3(self._ctx, _ptr(x0), C0, _ptr(x1), C1, B, H, W, _ptr(w_oihw), _ptr(bias), Cout,
                                     stride, ups, pad_lo, _ptr(res), _ptr(y), _stream(self.device)))
        return y

    def op_gn_silu_conv3x3(self, x0, gamma, beta, eps, w_oihw, bias, x1=None, bias2=None, res=None, mode=-1):
        """GroupNorm32 -> SiLU -> conv3x3 (reference openaimodel.py:212-232). Returns (y, used_prologue)."""
        B, H, W, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[3]
        Cout = w_oihw.shape[0]
        y = torch.empty((B, H, W, Cout), device=x0.device, dtype=torch.bfloat16)
        used = C.c_int(0)
        check(self.lib.gl_op_gn_silu_conv3x3(self._ctx, _ptr(x0), C0, _ptr(x1), C1, B, H, W, _ptr(gamma), _ptr(beta), C.c_float(eps),
                                             _ptr(w_oihw), _ptr(bias), Cout, _ptr(bias2), _ptr(res), _ptr(y), int(mode), C.byref(used),
                                             _stream(self.device)))
        return y, bool(used.value)

    def op_groupnorm(self, x0, gamma, beta, eps, silu, x1=None):
        B, HW, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[2]
        y = torch.empty((B, HW, C0 + C1), device=x0.device, dtype=torch.bfloat16)
        check(self.lib.gl_op_groupnorm(self._ctx, _ptr(x0), C0, _ptr(x1), C1, B, HW, _ptr(gamma), _ptr(beta),
                                       C.c_float(eps), int(silu), _ptr(y), _stream(self.device)))
        return y

    def op_layernorm(self, x, gamma, beta, eps=1e-5, x2=None, Tpad=None):
        B, N1, Cc = x.shape
        N2 = 0 if x2 is None else x2.shape[1]
        Tpad = Tpad or (N1 + N2)
        y = torch.empty((B, Tpad, Cc), device=x.device, dtype=torch.bfloat16)
        check(self.lib.gl_op_layernorm(self._ctx, _ptr(x), _ptr(x2), B, N1, N2, Tpad, Cc, _ptr(gamma), _ptr(beta),
                                       C.c_float(eps), _ptr(y), _stream(self.device)))
        return y

    def op_ff_chain_q(self, x, pre_w, pre_b, pre_res, gamma, beta, w1, b1, w2, b2, gamma_q, beta_q, wq, pre_gate=None, gate=None):
        """The fuser's chained launch with attn2.to_q(norm2(.)) as its trailing projection (gl_op_ff_chain_q). x [B][N][320].
        Returns (y [B][N][C], q [B][8][N][40]) -- q decoded from the attention kernels' head layout."""
        B, N, Cc = x.shape
        y = torch.empty_like(x)
        qbuf = torch.zeros((B * 8, N, 48), device=x.device, dtype=torch.bfloat16)
        check(self.lib.gl_op_ff_chain_q(self._ctx, _ptr(x), B, N, Cc, _ptr(pre_w), _ptr(pre_b), _ptr(pre_res), _ptr(pre_gate), _ptr(gamma), _ptr(beta),
                                        _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(gate), _ptr(gamma_q), _ptr(beta_q), _ptr(wq), _ptr(y), _ptr(qbuf),
                                        _stream(self.device)))
        return y, qbuf.view(B, 8, N, 48)[..., :40]

    def op_proj_attention(self, x, pre_w, pre_b, pre_res, gamma, beta, wq, wk, wv, heads, rows=True):
        """mid = pre_res + x Wpre^T + pre_b; o = self-attention of LN(mid) without to_out (gl_op_proj_attention).
        Returns (mid, o, used_rows): used_rows = 1 when the row-local projection kernel ran."""
        B, N, Cc = x.shape
        mid = torch.empty_like(x)
        o = torch.empty_like(x)
        used = C.c_int(1 if rows else 0)
        check(self.lib.gl_op_proj_attention(self._ctx, _ptr(x), B, N, Cc, heads, _ptr(pre_w), _ptr(pre_b), _ptr(pre_res), _ptr(gamma), _ptr(beta),
                                            _ptr(wq), _ptr(wk), _ptr(wv), 0, _ptr(mid), _ptr(o), C.byref(used), _stream(self.device)))
        return mid, o, used.value

    def op_attention(self, xq, xkv, wq, wk, wv, heads):
        B, Nq, Cc = xq.shape
        _, Nk, Ck = xkv.shape
        o = torch.empty((B, Nq, Cc), device=xq.device, dtype=torch.bfloat16)
        check(self.lib.gl_op_attention(self._ctx, _ptr(xq), _ptr(xkv), B, Nq, Nk, Cc, Ck, heads, _ptr(wq), _ptr(wk), _ptr(wv),
                                       _ptr(o), _stream(self.device)))
        return o

    def op_attention_core(self, q, k, vt, layout, B, heads, Nq, Nk, o, ldo, o_rows_per_b, kernel="auto"):
        """One attention kernel on the caller's bf16 buffers (gl_op_attention_core; layouts and the buffer contract:
        include/gligen_amd_attention_core.h). layout: an AttnProjLayout (d, dp, dpv, tq_pad, tk_pad, vt_perm32); kernel: a key of
        _lib.ATTN_CORE_KERNELS. Writes rows < Nq, columns < heads * d of every sample of o [B][o_rows_per_b][ldo] and returns o; a
        kernel with no instantiation for the layout raises GligenAmdError('libgligen_amd error 5: ...')."""
        from ._lib import ATTN_CORE_KERNELS
        check(self.lib.gl_op_attention_core(self._ctx, _ptr(q), _ptr(k), _ptr(vt), C.byref(layout), B, heads, Nq, Nk, _ptr(o), ldo, o_rows_per_b,
                                            ATTN_CORE_KERNELS[kernel], _stream(self.device)))
        return o

    def op_ff_rows(self, **fields):
        """ff_rows_kernel on the caller's buffers (gl_op_ff_rows; include/gligen_amd_ffn_rows.h). fields: the members of gl_ff_rows_args
        by name -- tensors (or None) for the pointers, ints / floats for the rest; whatever is left out is 0 / null, eps 1e-5."""
        from ._lib import FFRowsArgs
        self._rows_call(self.lib.gl_op_ff_rows, FFRowsArgs, fields)

    def op_qkv_rows(self, **fields):
        """qkv_rows_kernel on the caller's buffers (gl_op_qkv_rows; include/gligen_amd_ffn_rows.h), fields as in op_ff_rows."""
        from ._lib import QkvRowsArgs
        self._rows_call(self.lib.gl_op_qkv_rows, QkvRowsArgs, fields)

    def op_groupnorm_coef(self, x0, C0, gamma, beta, eps, coef, x1=None, C1=0, B=None, HW=None):
        """The statistics-only GroupNorm on the caller's buffers (gl_op_groupnorm_coef; include/gligen_amd_norm.h): writes coef
        [B][(C0 + C1) / 8][16] floats and returns the number of kernel launches. x0 [B][HW][C0] (B, HW from its shape unless given)."""
        B, HW = (x0.shape[0] if B is None else B), (x0.shape[1] if HW is None else HW)
        launches = C.c_int(0)
        check(self.lib.gl_op_groupnorm_coef(self._ctx, _ptr(x0), C0, _ptr(x1), C1, B, HW, _ptr(gamma), _ptr(beta), C.c_float(eps), _ptr(coef),
                                            C.byref(launches), _stream(self.device)))
        return launches.value

    def op_layernorm_rows(self, **fields):
        """ln_kernel on the caller's buffers (gl_op_layernorm_rows; include/gligen_amd_norm.h), fields as in op_ff_rows: the members of
        gl_layernorm_rows_args by name (ldx, ldy, null gamma / beta and the caller's y among them)."""
        from ._lib import LayerNormRowsArgs
        self._rows_call(self.lib.gl_op_layernorm_rows, LayerNormRowsArgs, fields)

    def _rows_call(self, fn, struct, fields):
        names = {n for n, _ in struct._fields_}
        unknown = set(fields) - names
        if unknown or "struct_size" in fields:
            raise TypeError(f"{struct.__name__} has no field(s) {sorted(unknown | ({'struct_size'} & set(fields)))}")
        args = struct(struct_size=C.sizeof(struct), eps=1e-5)
        for name, ctype in struct._fields_:
            if name in fields and fields[name] is not None:
                setattr(args, name, fields[name].data_ptr() if ctype is C.c_void_p else fields[name])
        check(fn(self._ctx, C.byref(args), _stream(self.device)))

    def attn_regime_counters(self, enable):
        """(lazy_moves, reruns) counted by op_attention since the last call (gl_attn_regime_counters): the counts are reset, and
        counting is on afterwards iff `enable`. A test instrument: d = 40 only, 0 elsewhere."""
        lazy, reruns = C.c_uint(0), C.c_uint(0)
        check(self.lib.gl_attn_regime_counters(self._ctx, 1 if enable else 0, C.byref(lazy), C.byref(reruns)))
        return lazy.value, reruns.value
