"""Generate the training goldens of the gatedSA2 and gatedCA fusers by RUNNING THE REFERENCE (read-only import, as
oracle/make_golden.py does):

    tests/golden/block_backward_gatedsa2.npz                 one BasicTransformerBlock, B 2, 16 x 16 tokens, C 320, 8 heads, Ng 16
    tests/golden/block_backward_gatedca.npz                  the same, Ng 30
    tests/golden/unet_small_gatedsa2_train_step.npz          text tokenizer, 16 box slots (a 4 x 4 grid)
    tests/golden/unet_small_gatedca_train_step.npz           text tokenizer, 30 box slots
    tests/golden/unet_small_canny_gatedsa2_train_step.npz    the inputs and config of unet_small_canny_train_step with
                                                             fuser_type="gatedSA2": resize 128 -> 4 x 4 tokens, resized to 16^2 and 8^2

The block files hold block_backward_gatedsa's case (oracle/make_golden.py:block_backward_case: the same seeds, draws and gates) with
the other fuser. That file's format stores every tensor whole (4.9 MB); a committed file stays under 1 MiB, so here y and dx are
stored as every STRIDE_ROWS-th token row (fp32), dobjs whole, and each fuser gradient as a strided sample (_grad_sample, n =
BLOCK_SAMPLE) with its scale and L2 norm -- the keys are block_backward_gatedsa's plus norm.*; the tests check full tensors against
autograd through the CPU oracle, which tests/test_train_fusers_cpu.py holds to these files. The three UNet files are one training
iteration each (oracle/make_golden.py:unet_backward_case, tools/make_golden_train_spatial.py:train_case with another fuser_type):
B 2, 16 x 16 latent, use_checkpoint=False, requires_grad as trainer.py:217-242 sets it, the 4096-sample gradient format with scale
and norm (1024 for the canny model's 310 tensors, as unet_small_canny_train_step). Needs the reference checkout that
oracle/make_golden.py reads (REF there); no test imports this script:

    cd /tmp && python <repo>/tools/make_golden_train_fusers.py [--only NAME ...]

At the same CPU thread count a re-run reproduces the committed files bit for bit.
"""
import argparse
import importlib.util
import json
import os
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mg = _by_path("gl_make_golden", os.path.join(REPO, "oracle", "make_golden.py"))   # puts the reference first on sys.path

import numpy as np  # noqa: E402
import torch  # noqa: E402

syn = mg.syn
BLOCK_SAMPLE, STRIDE_ROWS = 16384, 4
BLOCK_NG = {"gatedSA2": 16, "gatedCA": 30}
MAX_OBJS = {"gatedSA2": 16, "gatedCA": 30}


def _check_size(path):
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    return os.path.getsize(path)


def block_case(fuser_type, B=2, hw=16, C=320, heads=8, ctx_dim=768, ctx_T=77):
    from ldm.modules.attention import BasicTransformerBlock  # (reference)
    Ng = BLOCK_NG[fuser_type]
    name = "block_backward_" + fuser_type.lower()
    blk = BasicTransformerBlock(C, ctx_dim, ctx_dim, heads, C // heads, fuser_type, use_checkpoint=False)
    syn.fill_module_(blk, 77)
    with torch.no_grad():       # the gates start at tanh(0) = 0, where the fuser gets no gradient but alpha: open them
        blk.fuser.alpha_attn.fill_(0.6)
        blk.fuser.alpha_dense.fill_(-0.4)
    g = torch.Generator().manual_seed(4242)
    N = hw * hw
    x = torch.randn(B, N, C, generator=g).requires_grad_(True)
    objs = (torch.randn(B, Ng, ctx_dim, generator=g) * 0.5).requires_grad_(True)
    context = torch.randn(B, ctx_T, ctx_dim, generator=g)
    target = torch.randn(B, N, C, generator=g)
    for p_name, p_ in blk.named_parameters():
        p_.requires_grad_(p_name.startswith("fuser."))
    y = blk(x, context, objs)
    loss = torch.nn.functional.mse_loss(y, target)
    loss.backward()
    out = dict(y=y.detach().numpy()[:, ::STRIDE_ROWS].copy(), loss=np.float64(loss.item()), dx=x.grad.numpy()[:, ::STRIDE_ROWS].copy(),
               dobjs=objs.grad.numpy(), x_sum=np.float64(x.detach().double().sum().item()), target_sum=np.float64(target.double().sum().item()))
    n = 0
    for p_name, p_ in blk.named_parameters():
        if p_name.startswith("fuser."):
            sub, sc, nrm = mg._grad_sample(p_.grad.numpy(), n=BLOCK_SAMPLE)
            out["grad." + p_name], out["scale." + p_name], out["norm." + p_name] = sub, np.float64(sc), np.float64(nrm)
            n += 1
    out["meta"] = np.frombuffer(json.dumps(dict(B=B, hw=hw, Ng=Ng, C=C, heads=heads, ctx_dim=ctx_dim, ctx_T=ctx_T, seed=77, alpha_attn=0.6,
                                                alpha_dense=-0.4, fuser_type=fuser_type, sample=BLOCK_SAMPLE, stride_rows=STRIDE_ROWS)).encode(),
                                dtype=np.uint8)
    path = os.path.join(mg.OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: loss {loss.item():.6f}, |dx| {x.grad.abs().mean():.3e}, {n} fuser gradients, {_check_size(path)} bytes")


def _trainable(model, input_conv_train):
    names = []
    for k, p_ in model.named_parameters():                                    # trainer.py:217-242
        on = (("transformer_blocks" in k) and ("fuser" in k)) or "position_net" in k or "downsample_net" in k or \
             (input_conv_train and "input_blocks.0.0.weight" in k)
        p_.requires_grad_(on)
        if on:
            names.append(k)
    return names


def _store_grads(model, trainable, sample, out):
    for k, p_ in model.named_parameters():
        if k in trainable:
            sub, sc, nrm = mg._grad_sample(p_.grad.numpy(), n=sample)
            out["grad." + k], out["scale." + k], out["norm." + k] = sub, np.float64(sc), np.float64(nrm)


def unet_text_case(fuser_type, B=2, hw=16, n_valid=3):
    t0 = time.time()
    name = f"unet_small_{fuser_type.lower()}_train_step"
    cfg = dict(syn.UNET_CFG_SMALL, fuser_type=fuser_type, use_checkpoint=False)
    model = mg.build_unet(cfg, "text")          # eval(): no 10 % guidance drop (openaimodel.py:428)
    batch = syn.make_batch("text", B, n_valid=n_valid, seed=5, max_objs=MAX_OBJS[fuser_type])
    g = model.grounding_tokenizer_input.prepare(batch)
    x, ctx = syn.make_latent(B, 4, hw, hw, seed=6), syn.make_context(B, seed=6)
    t = torch.tensor([981, 441][:B], dtype=torch.long)
    target = syn.make_latent(B, 4, hw, hw, seed=7)
    trainable = _trainable(model, False)
    eps = model(dict(x=x, timesteps=t, context=ctx, grounding_input=g, inpainting_extra_input=None, grounding_extra_input=None))
    loss = torch.nn.functional.mse_loss(eps, target)
    loss.backward()
    out = dict(eps=eps.detach().numpy(), loss=np.float64(loss.item()))
    _store_grads(model, trainable, 4096, out)
    meta = dict(cfg=cfg, B=B, hw=hw, n_valid=n_valid, max_objs=MAX_OBJS[fuser_type], weight_seed=1234, n_trainable=len(trainable), sample=4096,
                kind="text")
    path = os.path.join(mg.OUT, name + ".npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print(f"{name}: loss {loss.item():.6f}, {len(trainable)} trainable tensors, {_check_size(path)} bytes [{time.time() - t0:.1f}s]")


def unet_canny_case():
    t0 = time.time()
    sp = _by_path("gl_make_golden_train_spatial", os.path.join(REPO, "tools", "make_golden_train_spatial.py"))
    from ldm.modules.diffusionmodules.openaimodel import UNetModel  # (reference)
    from ldm.util import instantiate_from_config
    modality, B, hw = "canny", 2, 16
    mg._timm_shim()
    cfg = dict(sp.spatial_cfg(modality, hw), fuser_type="gatedSA2")
    real_hub = torch.hub.load_state_dict_from_url
    torch.hub.load_state_dict_from_url = lambda *a, **k: {"model": {}}   # pretrained=True would look for ImageNet weights
    try:
        model = UNetModel(**cfg).eval()
    finally:
        torch.hub.load_state_dict_from_url = real_hub
    syn.fill_module_(model, 1234)
    gin = instantiate_from_config(dict(target=f"grounding_input.{modality}_grounding_tokinzer_input.GroundingNetInput"))
    dsin = instantiate_from_config(dict(target=f"grounding_input.{modality}_grounding_downsampler_input.GroundingDSInput"))
    d = sp.inputs(modality, B, hw)
    batch = {mg.SPATIAL_KEYS[modality]: d["img"], "mask": d["mask"]}
    g, extra = gin.prepare(batch), dsin.prepare(batch)
    trainable = _trainable(model, model.additional_channel_from_downsampler > 0)
    eps = model(dict(x=d["x"], timesteps=d["timesteps"], context=d["context"], grounding_input=g, inpainting_extra_input=None, grounding_extra_input=extra))
    loss = torch.nn.functional.mse_loss(eps, d["target"])
    loss.backward()
    out = dict(eps=eps.detach().numpy(), loss=np.float64(loss.item()))
    _store_grads(model, trainable, sp.SAMPLE, out)
    meta = dict(cfg=cfg, modality=modality, B=B, hw=hw, res=sp.RES, map_seed=3, latent_seed=6, context_seed=6, target_seed=7,
                mask=d["mask"].reshape(-1).tolist(), weight_seed=1234, n_trainable=len(trainable), sample=sp.SAMPLE,
                downsampler=dict(sp.DOWNSAMPLER[modality], resize=4 * hw))
    name = "unet_small_canny_gatedsa2_train_step"
    path = os.path.join(mg.OUT, name + ".npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print(f"{name}: loss {loss.item():.6f}, {len(trainable)} trainable tensors, {_check_size(path)} bytes [{time.time() - t0:.1f}s]")


CASES = {
    "block_backward_gatedsa2": lambda: block_case("gatedSA2"),
    "block_backward_gatedca": lambda: block_case("gatedCA"),
    "unet_small_gatedsa2_train_step": lambda: unet_text_case("gatedSA2"),
    "unet_small_gatedca_train_step": lambda: unet_text_case("gatedCA"),
    "unet_small_canny_gatedsa2_train_step": unet_canny_case,
}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=list(CASES))
    for case in ap.parse_args().only:
        CASES[case]()
