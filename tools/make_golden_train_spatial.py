"""Generate the spatial-map training goldens by RUNNING THE REFERENCE (read-only import, as oracle/make_golden.py does):

    tests/golden/unet_small_canny_train_step.npz   B 2, 16 x 16 latent, tokenizer resize 128, downsampler resize 64
    tests/golden/unet_small_hed_train_step.npz     B 1, 64 x 64 latent (the hed downsampler always goes to 64 x 64)
    tests/golden/unet_small_sem_train_step.npz     B 2, 16 x 16 latent

One training iteration of the reference's UNetModel with a ConvNeXt tokenizer and a GroundingDownsampler (configs/cc3m_canny.yaml
etc. on the small UNet): requires_grad exactly as trainer.py:189-245 sets it (every fuser.* parameter, position_net.* -- the whole
ConvNeXt backbone included --, downsample_net.*, and input_blocks.0.0.weight because additional_channel_from_downsampler > 0),
mse_loss(model_output, noise), loss.backward(). Stored: loss, eps, and per trainable tensor a strided sample of its gradient, its
scale and its L2 norm (oracle/make_golden.py:_grad_sample). Same config and weight seed as the unet_small_<modality> entries, so
golden_shapes("unet_small_<modality>") applies. Needs the reference checkout that oracle/make_golden.py reads (REF there); no test
imports this script:

    cd /tmp && python <repo>/tools/make_golden_train_spatial.py [--only canny hed sem]

At the same CPU thread count a re-run reproduces the committed files bit for bit.
"""
import argparse
import importlib.util
import json
import os
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gl_make_golden", os.path.join(REPO, "oracle", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)      # puts the reference first on sys.path and loads gligen_amd/synthetic.py by file path

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ldm.modules.diffusionmodules.openaimodel import UNetModel  # noqa: E402  (reference)
from ldm.util import instantiate_from_config  # noqa: E402

syn = mg.syn
SAMPLE = 1024          # gradient values stored per tensor: about 0.7 MB per file for the 306-312 trainable tensors
CASES = {"canny": dict(B=2, hw=16), "hed": dict(B=1, hw=64), "sem": dict(B=2, hw=16)}
DOWNSAMPLER = {"canny": dict(n_in=1, mode="bicubic"), "hed": dict(n_in=1, mode="bicubic"), "sem": dict(n_in=152, mode="nearest")}
RES, TOK_RESIZE = 128, 128


def spatial_cfg(modality, hw):
    """The config of oracle/make_golden.py:spatial_case (the unet_small_<modality> entries), without activation checkpointing."""
    ds_params = dict(out_dim=1) if modality == "hed" else dict(resize_input=4 * hw, out_dim=8)
    tk_params = dict(resize_input=TOK_RESIZE, out_dim=768)
    if modality == "sem":
        ds_params["in_dim"], tk_params["in_dim"] = 152, 152
    return dict(syn.UNET_CFG_SMALL, use_checkpoint=False,
                grounding_downsampler=dict(target=f"ldm.modules.diffusionmodules.{modality}_grounding_downsampler.GroundingDownsampler", params=ds_params),
                grounding_tokenizer=dict(target=f"ldm.modules.diffusionmodules.{modality}_grounding_net.PositionNet", params=tk_params))


def inputs(modality, B, hw):
    """The batch of a case from the seeded generators of gligen_amd.synthetic (the tests rebuild it the same way): the map, a mask
    that drops the second sample's map (its tokens are the null feature), the noised latent, timesteps, context and the noise."""
    img = syn.make_spatial_map(modality, B, RES, seed=3)
    mask = torch.ones(B, 1)
    if B > 1:
        mask[1] = 0.0
    return dict(img=img, mask=mask, x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441][:B], dtype=torch.long),
                context=syn.make_context(B, seed=6), target=syn.make_latent(B, 4, hw, hw, seed=7))


def train_case(modality):
    t0 = time.time()
    B, hw = CASES[modality]["B"], CASES[modality]["hw"]
    mg._timm_shim()
    cfg = spatial_cfg(modality, hw)
    real_hub = torch.hub.load_state_dict_from_url
    torch.hub.load_state_dict_from_url = lambda *a, **k: {"model": {}}   # pretrained=True would download ImageNet weights
    try:
        model = UNetModel(**cfg).eval()        # eval(): no 10 % guidance drop (openaimodel.py:428) -- the step is a function of its batch
    finally:
        torch.hub.load_state_dict_from_url = real_hub
    syn.fill_module_(model, 1234)
    gin = instantiate_from_config(dict(target=f"grounding_input.{modality}_grounding_tokinzer_input.GroundingNetInput"))
    dsin = instantiate_from_config(dict(target=f"grounding_input.{modality}_grounding_downsampler_input.GroundingDSInput"))
    d = inputs(modality, B, hw)
    batch = {mg.SPATIAL_KEYS[modality]: d["img"], "mask": d["mask"]}
    g, extra = gin.prepare(batch), dsin.prepare(batch)
    input_conv_train = model.additional_channel_from_downsampler > 0          # trainer.py:189-194
    trainable = []
    for k, p_ in model.named_parameters():                                     # trainer.py:217-242
        on = (("transformer_blocks" in k) and ("fuser" in k)) or "position_net" in k or "downsample_net" in k or \
             (input_conv_train and "input_blocks.0.0.weight" in k)
        p_.requires_grad_(on)
        if on:
            trainable.append(k)
    eps = model(dict(x=d["x"], timesteps=d["timesteps"], context=d["context"], grounding_input=g, inpainting_extra_input=None, grounding_extra_input=extra))
    loss = torch.nn.functional.mse_loss(eps, d["target"])
    loss.backward()
    out = dict(eps=eps.detach().numpy(), loss=np.float64(loss.item()))
    for k, p_ in model.named_parameters():
        if k in trainable:
            sub, sc, nrm = mg._grad_sample(p_.grad.numpy(), n=SAMPLE)
            out["grad." + k] = sub
            out["scale." + k] = np.float64(sc)
            out["norm." + k] = np.float64(nrm)
    meta = dict(cfg=cfg, modality=modality, B=B, hw=hw, res=RES, map_seed=3, latent_seed=6, context_seed=6, target_seed=7,
                mask=d["mask"].reshape(-1).tolist(), weight_seed=1234, n_trainable=len(trainable), sample=SAMPLE,
                downsampler=dict(DOWNSAMPLER[modality], resize=64 if modality == "hed" else 4 * hw))
    name = f"unet_small_{modality}_train_step"
    np.savez_compressed(os.path.join(mg.OUT, name + ".npz"), meta=json.dumps(meta), **out)
    print(f"{name}: loss {loss.item():.6f}, {len(trainable)} trainable tensors, "
          f"{sum(p.numel() for k, p in model.named_parameters() if k in trainable) / 1e6:.1f} M gradient values [{time.time() - t0:.1f}s]")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=list(CASES))
    for m in ap.parse_args().only:
        train_case(m)
