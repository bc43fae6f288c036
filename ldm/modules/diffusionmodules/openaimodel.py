"""GLIGEN UNet (SD-1.4 UNet + one gated self-attention fuser per transformer block).

Drop-in for the reference's ldm/modules/diffusionmodules/openaimodel.py: same class names,
constructor kwargs (openaimodel.py:238-259), attributes, state_dict keys (966 tensors for the
shipped configs) and `forward(input: dict) -> eps` contract (openaimodel.py:420-464). The
sub-modules only hold parameters; `UNetModel.forward` hands the whole evaluation to the native
MI355X engine (gligen_amd/csrc/engine_unet.hip: Engine::unet_forward) — no torch operator runs.
"""
import torch
import torch.nn as nn

from gligen_amd import lora as _lora
from gligen_amd import runtime as _rt
from ldm.modules.attention import SpatialTransformer, _EngineOnly, _slots, zero_module
from ldm.modules.diffusionmodules.util import conv_nd, linear, normalization
from ldm.util import instantiate_from_config


class TimestepBlock(_EngineOnly):
    """Marker: layers that take the timestep embedding as second argument."""


class TimestepEmbedSequential(nn.Sequential, TimestepBlock):
    """Container whose children receive (x, emb), (x, context, objs) or (x) by kind
    (reference openaimodel.py:37-51); executed by the engine, block by block."""

    def forward(self, *args, **kwargs):
        return _EngineOnly.forward(self)


class Upsample(_EngineOnly):
    """nearest 2x then conv3x3 (reference openaimodel.py:54-82) — the upsample is folded into the
    conv's gather on the device."""

    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1):
        super().__init__()
        self.channels, self.out_channels, self.use_conv, self.dims = channels, out_channels or channels, use_conv, dims
        if not use_conv:
            raise NotImplementedError("conv_resample=False is not implemented")
        self.conv = conv_nd(dims, self.channels, self.out_channels, 3, padding=padding)


class Downsample(_EngineOnly):
    """conv3x3 stride 2 pad 1 (reference openaimodel.py:87-113)."""

    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1):
        super().__init__()
        self.channels, self.out_channels, self.use_conv, self.dims = channels, out_channels or channels, use_conv, dims
        if not use_conv:
            raise NotImplementedError("conv_resample=False is not implemented")
        self.op = conv_nd(dims, self.channels, self.out_channels, 3, stride=2, padding=padding)


class ResBlock(TimestepBlock):
    """GN-SiLU-conv, + Linear(SiLU(emb)), GN-SiLU-conv, + skip (reference openaimodel.py:116-232)."""

    def __init__(self, channels, emb_channels, dropout, out_channels=None, use_conv=False, use_scale_shift_norm=False,
                 dims=2, use_checkpoint=False, up=False, down=False):
        super().__init__()
        if use_scale_shift_norm or up or down or use_conv:
            raise NotImplementedError("scale-shift norm / resampling ResBlocks are not used by GLIGEN configs")
        self.channels, self.emb_channels, self.dropout = channels, emb_channels, dropout
        self.out_channels = out_channels or channels
        self.use_checkpoint = use_checkpoint
        self.in_layers = _slots(3, i0=normalization(channels), i2=conv_nd(dims, channels, self.out_channels, 3, padding=1))
        self.emb_layers = _slots(2, i1=linear(emb_channels, self.out_channels))
        self.out_layers = _slots(4, i0=normalization(self.out_channels),
                                 i3=zero_module(conv_nd(dims, self.out_channels, self.out_channels, 3, padding=1)))
        self.skip_connection = nn.Identity() if self.out_channels == channels else conv_nd(dims, channels, self.out_channels, 1)


class UNetModel(nn.Module):
    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, use_checkpoint=False, num_heads=8,
                 use_scale_shift_norm=False, transformer_depth=1, context_dim=None, fuser_type=None, inpaint_mode=False,
                 grounding_downsampler=None, grounding_tokenizer=None):
        super().__init__()
        assert fuser_type in ["gatedSA", "gatedSA2", "gatedCA"]
        self.image_size, self.in_channels, self.model_channels, self.out_channels = image_size, in_channels, model_channels, out_channels
        self.num_res_blocks, self.attention_resolutions, self.dropout = num_res_blocks, attention_resolutions, dropout
        self.channel_mult, self.conv_resample, self.use_checkpoint = channel_mult, conv_resample, use_checkpoint
        self.num_heads, self.context_dim, self.fuser_type, self.inpaint_mode = num_heads, context_dim, fuser_type, inpaint_mode
        self.grounding_tokenizer_input = None  # set externally (gligen_inference.py:348-349)
        # spatial-map modalities: the downsampled conditioning map enters as extra first-conv channels (reference
        # openaimodel.py:288-305); "GLIGEN" = the 4 + k channel conv is in place, "SD" = it was swapped for the SD one
        self.downsample_net = None
        self.additional_channel_from_downsampler = 0
        self.first_conv_type = "SD"
        self.first_conv_restorable = not inpaint_mode
        if grounding_downsampler is not None:
            if inpaint_mode:
                raise NotImplementedError("inpaint_mode with a grounding downsampler is a TODO breakpoint in the reference (openaimodel.py:446-447)")
            self.downsample_net = instantiate_from_config(grounding_downsampler)
            self.additional_channel_from_downsampler = self.downsample_net.out_dim
            self.first_conv_type = "GLIGEN"

        mc, ted = model_channels, model_channels * 4
        self.time_embed = _slots(3, i0=linear(mc, ted), i2=linear(ted, ted))
        # latent (| downsampled grounding map) | masked latent | mask
        in_c = in_channels * 2 + 1 if inpaint_mode else in_channels + self.additional_channel_from_downsampler
        self.input_blocks = nn.ModuleList([TimestepEmbedSequential(conv_nd(dims, in_c, mc, 3, padding=1))])

        def res(cin, cout):
            return ResBlock(cin, ted, dropout, out_channels=cout, dims=dims, use_checkpoint=use_checkpoint,
                            use_scale_shift_norm=use_scale_shift_norm)

        def st(ch):
            return SpatialTransformer(ch, key_dim=context_dim, value_dim=context_dim, n_heads=num_heads, d_head=ch // num_heads,
                                      depth=transformer_depth, fuser_type=fuser_type, use_checkpoint=use_checkpoint)

        skip_chans, ch, ds = [mc], mc, 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [res(ch, mult * mc)]
                ch = mult * mc
                if ds in attention_resolutions:
                    layers.append(st(ch))
                self.input_blocks.append(TimestepEmbedSequential(*layers))
                skip_chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(TimestepEmbedSequential(Downsample(ch, conv_resample, dims=dims, out_channels=ch)))
                skip_chans.append(ch)
                ds *= 2
        self.middle_block = TimestepEmbedSequential(res(ch, ch), st(ch), res(ch, ch))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                layers = [res(ch + skip_chans.pop(), mc * mult)]
                ch = mc * mult
                if ds in attention_resolutions:
                    layers.append(st(ch))
                if level and i == num_res_blocks:
                    layers.append(Upsample(ch, conv_resample, dims=dims, out_channels=ch))
                    ds //= 2
                self.output_blocks.append(TimestepEmbedSequential(*layers))
        self.out = _slots(3, i0=normalization(ch), i2=zero_module(conv_nd(dims, mc, out_channels, 3, padding=1)))
        self.position_net = instantiate_from_config(grounding_tokenizer)

        self._engine = None
        self._cond_key = None
        self._cond_held = None
        self._ds_cache = None

    # ---- engine lifecycle ---------------------------------------------------------------
    def _apply(self, fn, *a, **k):  # .to()/.cuda()/.float(): parameters move, the packed copy is stale
        self._drop_engine()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._drop_engine()
        _lora.forget_loras(self)  # new weights: the originals stashed under merged adapters are not this model's any more
        return super().load_state_dict(*a, **k)

    def _drop_engine(self):
        # the execution lanes forked from this engine (gligen_inference.generate_lanes) go first: they share its packed weights
        for lane in self.__dict__.pop("_lanes", None) or ():
            for m in lane[:2]:
                if m.__dict__.get("_engine") is not None:
                    m.__dict__["_engine"].close()
                    m.__dict__["_engine"] = None
        # and the second-pass contexts of two-pass generation (gligen_inference._hires_context)
        for m, _ in (self.__dict__.pop("_hires", None) or {}).values():
            if m.__dict__.get("_engine") is not None:
                m.__dict__["_engine"].close()
                m.__dict__["_engine"] = None
        eng = self.__dict__.get("_engine")
        if eng is not None:
            eng.close()
        self.__dict__["_engine"] = None
        self.__dict__["_cond_key"] = None
        self.__dict__["_cond_held"] = None
        self.__dict__["_ds_cache"] = None
        self.__dict__["_first_conv_restored"] = False

    @property
    def engine(self):
        """The native engine holding this model's packed bf16 weights (built on first use)."""
        if self._engine is None:
            self._engine = _rt.build_unet_engine(self)
            self._cond_key = None
        return self._engine

    def fuser_scales(self):
        """The fusers' `scale` attributes in module order (= the engine's transformer order)."""
        from ldm.modules.attention import GatedCrossAttentionDense, GatedSelfAttentionDense, GatedSelfAttentionDense2
        kinds = (GatedSelfAttentionDense, GatedSelfAttentionDense2, GatedCrossAttentionDense)
        return [float(m.scale) for m in self.modules() if type(m) in kinds]

    def fuser_scale(self):
        """The common gate multiplier of all fusers (what set_alpha_scale wrote); ValueError if they differ."""
        scales = set(self.fuser_scales())
        if len(scales) != 1:
            raise ValueError(f"the fusers carry different scales {sorted(scales)}: use fuser_scales()")
        return scales.pop()

    def push_fuser_scales(self):
        scales = self.fuser_scales()
        if len(set(scales)) == 1:
            self.engine.set_fuser_scale(scales[0])
        else:
            self.engine.set_fuser_scales(scales)

    def set_conditioning(self, context, grounding_input):
        """Step-invariant work (grounding tokens, fuser projections, text K/V), skipped when the very same tensors come
        back unmodified. The cache entry HOLDS the tensors it fingerprinted: an address / version match can then only mean
        "same live tensor, not written since" — a freed temporary whose block the allocator hands to the next prompt's
        same-shaped tensor can no longer pass for it."""
        key = (_rt.tensor_fingerprint(context), _rt.mapping_fingerprint(grounding_input))
        if key != self._cond_key:
            g = grounding_input
            if self.engine.unet_cfg["grounding_kind"] == "tokens" and "tokens" not in g:
                g = {"tokens": self.position_net.tokens(engine=self.engine, **g)}  # spatial-map tokenizer: once per prompt
            self.engine.set_cond(context, g)
            self.__dict__["_cond_key"] = key
            self.__dict__["_cond_held"] = (context, dict(grounding_input))

    def first_conv_extra(self, input):
        """The downsampled grounding map concatenated to x in front of the first conv (reference openaimodel.py:442-444):
        step-invariant, so computed once per distinct grounding_extra_input tensor. None for models without a downsampler.
        (After the SD first conv was swapped in the engine's weights for these channels are zero; the map still has to be
        bound because the packed first conv keeps its 4 + k layout.)"""
        if self.downsample_net is None or self.engine.unet_cfg.get("extra_channels", 0) == 0:
            return None
        g = input.get("grounding_extra_input")
        if g is None:
            raise ValueError("this model has a grounding downsampler: input['grounding_extra_input'] is required")
        key = _rt.tensor_fingerprint(g)
        if self._ds_cache is None or self._ds_cache[0] != key:
            self.__dict__["_ds_cache"] = (key, g, self.downsample_net(g, engine=self.engine))
        return self._ds_cache[2]

    # ---- reference API ------------------------------------------------------------------
    SD_FIRST_CONV_FILE = "SD_input_conv_weight_bias.pth"  # cwd-relative, as in the reference

    def load_sd_first_conv(self):
        """(weight, bias) of the original SD first conv (reference openaimodel.py:404)."""
        sd = torch.load(self.SD_FIRST_CONV_FILE)
        return sd["weight"], sd["bias"]

    def restore_first_conv_from_SD(self):
        """Swap the first conv for the original SD one (reference openaimodel.py:400-413, called by
        the samplers whenever the fuser gate is 0). The reference re-reads the file and rebuilds the
        module at every such step; here the weights are copied in place once (module parameters and
        the engine's packed copy), later calls are no-ops."""
        if not self.first_conv_restorable:
            print("First conv layer is not restorable and skipped this process, probably because this is an inpainting model?")
            return
        if self.__dict__.get("_first_conv_restored"):
            return
        w, b = self.load_sd_first_conv()
        conv = self.input_blocks[0][0]
        with torch.no_grad():
            if conv.weight.shape == w.shape:
                conv.weight.copy_(w.to(conv.weight))
                conv.bias.copy_(b.to(conv.bias))
            else:  # 4 + k channel GLIGEN conv: the reference builds a fresh 4-channel conv (openaimodel.py:407-409)
                new = conv_nd(2, self.in_channels, self.model_channels, 3, padding=1).to(conv.weight)
                new.weight.copy_(w.to(new.weight))
                new.bias.copy_(b.to(new.bias))
                self.GLIGEN_first_conv_state_dict = {k: v.clone() for k, v in conv.state_dict().items()}
                self.input_blocks[0]._modules["0"] = new  # not through _apply: the packed engine copy stays valid
                conv = new
        if self._engine is not None:
            # the engine zeroes the weights of the k downsampler channels: same result as dropping the concat
            self._engine.restore_first_conv(conv.weight, conv.bias)
        self.first_conv_type = "SD"
        self.__dict__["_first_conv_restored"] = True

    def restore_first_conv_from_GLIGEN(self):
        raise NotImplementedError("not implemented by the reference either (openaimodel.py:416-417)")

    @torch.no_grad()
    def forward(self, input):
        if self.training:
            raise NotImplementedError("the MI355X engine implements inference; call model.eval()")
        if "grounding_input" in input and input["grounding_input"] is not None:
            grounding_input = input["grounding_input"]
        else:  # guidance null case (reference openaimodel.py:422-426)
            grounding_input = self.grounding_tokenizer_input.get_null_input()
        eng = self.engine
        self.set_conditioning(input["context"], grounding_input)
        self.push_fuser_scales()
        extra = input.get("inpainting_extra_input") if self.inpaint_mode else self.first_conv_extra(input)
        if self.inpaint_mode and extra is None:
            raise ValueError("inpaint_mode model needs input['inpainting_extra_input']")
        x = input["x"]
        eps = eng.unet_forward(x, input["timesteps"], extra)
        return eps.to(x.dtype)
