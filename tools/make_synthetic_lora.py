"""Write a seeded LoRA adapter in kohya's format for one of the synthetic models (no real adapter exists offline).

    python tools/make_synthetic_lora.py out.safetensors [--kind text] [--small] [--rank 16] [--families attn ff] [--dtype fp16] [--seed 7]

The adapter addresses the modules of the chosen families (gligen_amd.synthetic.LORA_FAMILIES: attn, ff, proj, conv, emb, sample, time,
fuser, first_conv) under the names kohya writes for an SD-1.x UNet, so `gligen_inference.py --synthetic text --lora out.safetensors:0.8`
loads it. The model is only instantiated on the meta device: its shapes are all that is needed, no GPU and no weights.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    from gligen_amd import lora, synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("out", type=str, help="the file to write (.safetensors, or .pt for a torch file)")
    ap.add_argument("--kind", type=str, default="text", choices=sorted(syn.GROUNDING_TOKENIZERS))
    ap.add_argument("--small", action="store_true", help="the 2-level test UNet (UNET_CFG_SMALL) instead of the full-size one")
    ap.add_argument("--inpaint", action="store_true")
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--alpha", type=float, default=None, help="the stored alpha (default rank / 2)")
    ap.add_argument("--families", type=str, nargs="+", default=["attn", "ff"], choices=sorted(syn.LORA_FAMILIES))
    ap.add_argument("--dtype", type=str, default="fp16", choices=["fp16", "fp32", "bf16"])
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args(argv)
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    cfg = dict(syn.UNET_CFG_SMALL if args.small else syn.UNET_CFG, grounding_tokenizer=syn.GROUNDING_TOKENIZERS[args.kind], inpaint_mode=args.inpaint)
    with torch.device("meta"):
        model = UNetModel(**cfg)
    dtype = dict(fp16=torch.float16, fp32=torch.float32, bf16=torch.bfloat16)[args.dtype]
    adapter = syn.synthetic_lora(model, rank=args.rank, families=args.families, dtype=dtype, seed=args.seed, alpha=args.alpha)
    if args.out.endswith((".pt", ".pth")):
        torch.save(adapter, args.out)
    else:
        lora.write_safetensors(args.out, adapter, metadata=dict(ss_network_dim=args.rank, ss_network_module="networks.lora", synthetic_seed=args.seed))
    n = sum(1 for k in adapter if k.endswith(".lora_down.weight"))
    print(f"{args.out}: {n} modules of {args.families}, rank {args.rank}, {args.dtype}, {sum(t.numel() * t.element_size() for t in adapter.values()) / 2 ** 20:.1f} MiB")


if __name__ == "__main__":
    main()
