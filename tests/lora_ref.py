"""References of the LoRA tests: the merge in float64 with its error bound, and the names an SD-1.x LoRA carries, generated from the
diffusers block layout alone (nothing of gligen_amd.lora is used here)."""
import torch

U = 2.0 ** -24          # the unit roundoff of fp32

# (N, K, r) of the operator test
OP_SHAPES = [(1, 1, 1), (5, 7, 3), (64, 64, 4), (65, 63, 1), (320, 768, 8), (320, 36, 4), (1280, 1280, 128), (2560, 320, 129), (33, 2880, 16)]


def merge64(W, up, down, scale):
    """W + scale * up @ down in float64 from the fp32 (or fp16 / bf16) values; up [N, r(, 1, 1)], down [r, K...]; the result has W's shape."""
    N, r = int(W.shape[0]), int(down.shape[0])
    return W.double() + float(scale) * (up.double().reshape(N, r) @ down.double().reshape(r, -1)).reshape(W.shape)


def merge_bound(W, up, down, scale):
    """Per element: 1.01 * 2^-24 * ((r + 2) |scale| sum_i |up_ni down_ik| + |ref|), both terms in float64. It holds for any order of
    summation: r rounded multiply-adds of the products (error <= gamma_r sum |up down|, gamma_r = r u / (1 - r u)), one rounded
    multiply-add of scale times the sum onto W (error <= u |result|); of the two spare units one covers a scale that is not an fp32
    number (it is rounded once on its way into the kernel), the other and the factor 1.01 the second-order terms."""
    N, r = int(W.shape[0]), int(down.shape[0])
    mag = (up.double().reshape(N, r).abs() @ down.double().reshape(r, -1).abs()).reshape(W.shape)
    return 1.01 * U * ((r + 2) * abs(float(scale)) * mag + merge64(W, up, down, scale).abs())


def op_case(N, K, r, w_mag, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) * w_mag
    up = torch.randn(N, r, generator=g)
    down = torch.randn(r, K, generator=g)
    return W, up, down


# ---- the names of an SD-1.x LoRA, from the diffusers layout ----------------------------------------------------------------------
SD14 = dict(block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, attention=(True, True, True, False), cross_attention_dim=768,
            in_channels=4, out_channels=4)
# the layout of synthetic.UNET_CFG_SMALL: channel_mult [1, 2], one ResBlock per level, attention on both levels
SMALL = dict(block_out_channels=(320, 640), layers_per_block=1, attention=(True, True), cross_attention_dim=768, in_channels=4, out_channels=4)

# pinned literally (LoRA name -> module path in the ldm-style UNetModel), on the SD-1.4 topology
PINNED = {
    "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q": "input_blocks.1.1.transformer_blocks.0.attn1.to_q",
    "lora_unet_down_blocks_2_downsamplers_0_conv": "input_blocks.9.0.op",
    "lora_unet_mid_block_attentions_0_proj_in": "middle_block.1.proj_in",
    "lora_unet_up_blocks_1_attentions_2_transformer_blocks_0_attn2_to_k": "output_blocks.5.1.transformer_blocks.0.attn2.to_k",
    "lora_unet_up_blocks_0_upsamplers_0_conv": "output_blocks.2.1.conv",
    "lora_unet_up_blocks_1_upsamplers_0_conv": "output_blocks.5.2.conv",
    "lora_unet_up_blocks_3_resnets_2_conv_shortcut": "output_blocks.11.0.skip_connection",
    "lora_unet_time_embedding_linear_2": "time_embed.2",
    # a fuser, through the module-path form
    "lora_unet_input_blocks_4_1_transformer_blocks_0_fuser_attn_to_v": "input_blocks.4.1.transformer_blocks.0.fuser.attn.to_v",
}
PINNED_TE = "lora_te_text_model_encoder_layers_11_mlp_fc2"      # -> encoder.layers.11.mlp.fc2 under the installed class's prefix


def _resnet(prefix, cin, cout, temb):
    out = {f"{prefix}_conv1": (cout, cin, 3, 3), f"{prefix}_conv2": (cout, cout, 3, 3), f"{prefix}_time_emb_proj": (cout, temb)}
    if cin != cout:
        out[f"{prefix}_conv_shortcut"] = (cout, cin, 1, 1)
    return out


def _transformer(prefix, c, cross):
    tb = f"{prefix}_transformer_blocks_0"
    out = {f"{prefix}_proj_in": (c, c, 1, 1), f"{prefix}_proj_out": (c, c, 1, 1)}
    for a, kv in (("attn1", c), ("attn2", cross)):
        out.update({f"{tb}_{a}_to_q": (c, c), f"{tb}_{a}_to_k": (c, kv), f"{tb}_{a}_to_v": (c, kv), f"{tb}_{a}_to_out_0": (c, c)})
    out.update({f"{tb}_ff_net_0_proj": (8 * c, c), f"{tb}_ff_net_2": (c, 4 * c)})
    return out


def diffusers_unet_targets(block_out_channels, layers_per_block, attention, cross_attention_dim, in_channels, out_channels):
    """{LoRA name: weight shape} of every Linear / Conv2d a kohya LoRA can address in diffusers' UNet2DConditionModel of this layout
    (CrossAttnDownBlock2D / DownBlock2D, UNetMidBlock2DCrossAttn, UpBlock2D / CrossAttnUpBlock2D), conv_in left out."""
    boc, n = list(block_out_channels), len(block_out_channels)
    temb = 4 * boc[0]
    t = {"time_embedding_linear_1": (temb, boc[0]), "time_embedding_linear_2": (temb, temb), "conv_out": (out_channels, boc[0], 3, 3)}
    ch = boc[0]
    for i, cout in enumerate(boc):
        for j in range(layers_per_block):
            t.update(_resnet(f"down_blocks_{i}_resnets_{j}", ch, cout, temb))
            ch = cout
            if attention[i]:
                t.update(_transformer(f"down_blocks_{i}_attentions_{j}", cout, cross_attention_dim))
        if i != n - 1:
            t[f"down_blocks_{i}_downsamplers_0_conv"] = (cout, cout, 3, 3)
    mid = boc[-1]
    t.update(_resnet("mid_block_resnets_0", mid, mid, temb))
    t.update(_resnet("mid_block_resnets_1", mid, mid, temb))
    t.update(_transformer("mid_block_attentions_0", mid, cross_attention_dim))
    rev = boc[::-1]
    prev = rev[0]
    for i, cout in enumerate(rev):
        cin = rev[min(i + 1, n - 1)]
        for j in range(layers_per_block + 1):
            skip = cin if j == layers_per_block else cout
            first = prev if j == 0 else cout
            t.update(_resnet(f"up_blocks_{i}_resnets_{j}", first + skip, cout, temb))
            if attention[n - 1 - i]:
                t.update(_transformer(f"up_blocks_{i}_attentions_{j}", cout, cross_attention_dim))
        if i != n - 1:
            t[f"up_blocks_{i}_upsamplers_0_conv"] = (cout, cout, 3, 3)
        prev = cout
    return {"lora_unet_" + k: v for k, v in t.items()}


def clip_text_targets(layers=12, width=768, intermediate=3072):
    """{LoRA name: weight shape} of the text tower's Linears as kohya names them."""
    t = {}
    for n in range(layers):
        p = f"lora_te_text_model_encoder_layers_{n}_"
        for m in ("q", "k", "v", "out"):
            t[f"{p}self_attn_{m}_proj"] = (width, width)
        t[p + "mlp_fc1"] = (intermediate, width)
        t[p + "mlp_fc2"] = (width, intermediate)
    return t
