"""Generate the non-square goldens by RUNNING THE REFERENCE: its own AutoencoderKL and UNetModel, fp32 on the CPU, on the seeded
weights of gligen_amd/synthetic.py, at sizes that are not square:

    tests/golden/vae_small_24x40.npz          small VAE (f = 2): decode of a 24 x 40 latent (B = 2) -> img [2, 3, 48, 80], and encode of
                                              a seeded 48 x 80 image -> z [2, 4, 24, 40] with the posterior's recorded noise draw
    tests/golden/unet_small_text_16x24.npz    small text UNet: eps on a 16 x 24 latent, B = 2, the grounding batch of syn.make_batch

Weights are never stored (both sides regenerate them from the per-key seeds); only the reference's outputs and the one recorded
noise draw are. tests/test_vae_attention_cpu.py holds the CPU oracle (oracle/gligen_oracle.py, pinned at square sizes only by
tests/test_oracle_golden.py) to these files, which makes it the reference at non-square sizes for the GPU tests.

The reference's `ldm` / `grounding_input` packages collide by name with this repository's drop-in packages, so the tool takes the
repository off sys.path, puts the reference checkout first and loads gligen_amd/synthetic.py by file path (as oracle/make_golden.py
does). Run it from outside the repository, where a reference checkout exists:

    cd /tmp && python <repo>/tools/make_golden_sizes.py --reference <reference checkout>
"""
import argparse
import importlib.util
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAE_LATENT = (24, 40)
UNET_LATENT = (16, 24)
GINPUT_TEXT = "grounding_input.text_grounding_tokinzer_input.GroundingNetInput"


def _synthetic():
    spec = importlib.util.spec_from_file_location("gl_synthetic", os.path.join(REPO, "gligen_amd", "synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def vae_inputs(syn, torch):
    """The decode latent and the encode image of vae_small_24x40 (the tests rebuild them from here)."""
    h, w = VAE_LATENT
    f = 2 ** (len(syn.VAE_DDCONFIG_SMALL["ch_mult"]) - 1)
    z = syn.make_latent(2, 4, h, w, seed=13) * 0.18215 * 4
    x = torch.rand(2, 3, h * f, w * f, generator=torch.Generator().manual_seed(18)) * 2 - 1
    return z, x


def unet_inputs(syn, torch):
    """batch, x, context, timesteps of unet_small_text_16x24."""
    h, w = UNET_LATENT
    batch = syn.make_batch("text", 2, n_valid=3, seed=1)
    return batch, syn.make_latent(2, 4, h, w, seed=11), syn.make_context(2, seed=1), torch.tensor([981, 441], dtype=torch.long)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GLIGEN_REFERENCE"), help="checkout of the reference implementation (or $GLIGEN_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args(argv)
    if not args.reference or not os.path.isdir(os.path.join(args.reference, "ldm")):
        raise SystemExit("--reference: a directory with the reference's ldm package is needed")
    ref = os.path.abspath(args.reference)
    sys.path = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    import numpy as np
    import torch
    syn = _synthetic()
    from ldm.models.autoencoder import AutoencoderKL
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from ldm.util import instantiate_from_config
    assert sys.modules["ldm.util"].__file__.startswith(ref), "must import the reference's ldm package"

    # ---- small VAE, 24 x 40 latent
    dd = syn.VAE_DDCONFIG_SMALL
    ae = AutoencoderKL(ddconfig=dd, embed_dim=4, scale_factor=0.18215).eval()
    syn.fill_module_(ae, 4321)
    z, x = vae_inputs(syn, torch)
    draws, real_randn = [], torch.randn

    def rec_randn(*a, **k):
        t = real_randn(*a, generator=torch.Generator().manual_seed(99), **k)
        draws.append(t)
        return t

    with torch.no_grad():
        img = ae.decode(z)
        torch.randn = rec_randn
        try:
            zenc = ae.encode(x)
        finally:
            torch.randn = real_randn
    assert len(draws) == 1 and tuple(zenc.shape) == (2, 4) + VAE_LATENT and tuple(img.shape) == tuple(x.shape)
    meta = dict(ddconfig=dd, B=2, latent=list(VAE_LATENT), weight_seed=4321, torch=torch.__version__)
    np.savez_compressed(os.path.join(args.out, "vae_small_24x40.npz"), meta=json.dumps(meta), img=img.numpy(), z=zenc.numpy(), noise=draws[0].numpy())
    print(f"vae_small_24x40: img std {float(img.std()):.4f}, z std {float(zenc.std()):.4f}")

    # ---- small text UNet, 16 x 24 latent
    cfg = syn.UNET_CFG_SMALL
    model = UNetModel(**dict(cfg, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=False)).eval()
    syn.fill_module_(model, 1234)
    model.grounding_tokenizer_input = instantiate_from_config(dict(target=GINPUT_TEXT))
    batch, xl, ctx, t = unet_inputs(syn, torch)
    g = model.grounding_tokenizer_input.prepare(batch)
    inp = dict(x=xl, timesteps=t, context=ctx, grounding_input=g, inpainting_extra_input=None, grounding_extra_input=None)
    with torch.no_grad():
        eps = model(inp)
        eps_null = model({k: v for k, v in inp.items() if k != "grounding_input"})
    meta = dict(cfg=cfg, kind="text", B=2, latent=list(UNET_LATENT), n_valid=3, weight_seed=1234, torch=torch.__version__)
    np.savez_compressed(os.path.join(args.out, "unet_small_text_16x24.npz"), meta=json.dumps(meta), eps=eps.numpy(), eps_null=eps_null.numpy())
    print(f"unet_small_text_16x24: eps std {float(eps.std()):.4f}, cond-vs-null mse {float(((eps - eps_null) ** 2).mean()):.3e}")


if __name__ == "__main__":
    main()
