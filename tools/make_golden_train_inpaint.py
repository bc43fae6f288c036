"""Generate the inpainting training goldens by RUNNING THE REFERENCE (read-only import, as oracle/make_golden.py does):

    tests/golden/unet_small_inpaint_train_step.npz      text tokenizer
    tests/golden/unet_small_ti_inpaint_train_step.npz   text+image tokenizer

One training iteration of the reference's UNetModel with inpaint_mode=True (the 9-channel first conv, openaimodel.py:299-302,
445-447) on the small UNet, B 2, 16 x 16 latent, with the trainer's own input stage (trainer.py:329-364): x_noisy from the
diffusion's q_sample, the mask from draw_masks_from_boxes(boxes, 16), inpainting_extra_input = cat(z * mask, mask); requires_grad
exactly as trainer.py:217-242 sets it with input_conv_train = True (every fuser.* parameter, position_net.*, and
input_blocks.0.0.weight; its bias stays frozen), mse_loss(model_output, noise), loss.backward(), in eval() mode so that no guidance
drop happens. Some boxes of the seeded batch are overwritten BEFORE both uses, so that the grounding tokens and the mask see the
same boxes: one from 0.0 to 1.0 along x, two overlapping ones, one with x1 < x0; the zero padding boxes stay as they come.
Stored: loss, eps, x_noisy, mask, inpainting_extra_input, the boxes, and per trainable tensor a strided sample of its gradient,
its scale and its L2 norm (oracle/make_golden.py:_grad_sample). Same weight seed and shapes as the unet_small_inpaint entry
(text; the text+image model's are those of unet_small_text_image with the 9-channel first conv). Needs the reference checkout that
oracle/make_golden.py reads (REF there); no test imports this script:

    cd /tmp && python <repo>/tools/make_golden_train_inpaint.py [--only text text_image]

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

syn = mg.syn
SAMPLE = 4096          # gradient values stored per tensor, as the discrete training goldens: about 0.65 MB per file
NAMES = {"text": "unet_small_inpaint_train_step", "text_image": "unet_small_ti_inpaint_train_step"}
N_TRAINABLE = {"text": 128, "text_image": 135}       # the non-inpainting models' 127 / 134 and the first conv's weight
B, HW, N_VALID, TIMESTEPS = 2, 16, 3, [981, 441]
# (sample, box) -> (x0, y0, x1, y1)
BOXES = {(0, 0): (0.0, 0.25, 1.0, 0.5),              # from 0.0 to 1.0 along x: reaches both borders
         (0, 1): (0.1, 0.1, 0.5, 0.6), (0, 2): (0.3, 0.4, 0.8, 0.9),     # overlapping
         (1, 0): (0.7, 0.2, 0.3, 0.6)}               # x1 < x0: masks nothing


def train_case(kind):
    t0 = time.time()
    cfg = dict(syn.UNET_CFG_SMALL, use_checkpoint=False)
    model = mg.build_unet(cfg, kind, inpaint=True)        # eval(): no 10 % guidance drop (openaimodel.py:428)
    batch = syn.make_batch(kind, B, n_valid=N_VALID, seed=5)
    for (b, k), box in BOXES.items():
        batch["boxes"][b, k] = torch.tensor(box)
    g = model.grounding_tokenizer_input.prepare(batch)
    z = syn.make_latent(B, 4, HW, HW, seed=6)
    noise = syn.make_latent(B, 4, HW, HW, seed=7)
    t = torch.tensor(TIMESTEPS, dtype=torch.long)
    diffusion = mg.LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
    x_noisy = diffusion.q_sample(x_start=z, t=t, noise=noise)                 # trainer.py:356
    mask = mg.ref_draw_masks(batch["boxes"], HW)                              # trainer.py:342
    extra = torch.cat([z * mask, mask], dim=1)                                # trainer.py:343-344
    input_conv_train = True                                                   # trainer.py:191-194: inpaint_mode adds 5 channels
    trainable = []
    for k, p_ in model.named_parameters():                                    # trainer.py:217-242
        on = (("transformer_blocks" in k) and ("fuser" in k)) or "position_net" in k or "downsample_net" in k or \
             (input_conv_train and "input_blocks.0.0.weight" in k)
        p_.requires_grad_(on)
        if on:
            trainable.append(k)
    assert len(trainable) == N_TRAINABLE[kind], len(trainable)
    assert "input_blocks.0.0.weight" in trainable and "input_blocks.0.0.bias" not in trainable
    eps = model(dict(x=x_noisy, timesteps=t, context=syn.make_context(B, seed=6), grounding_input=g, inpainting_extra_input=extra,
                     grounding_extra_input=None))
    loss = torch.nn.functional.mse_loss(eps, noise)
    loss.backward()
    out = dict(eps=eps.detach().numpy(), loss=np.float64(loss.item()), x_noisy=x_noisy.numpy(), mask=mask.numpy(),
               inpainting_extra_input=extra.numpy(), boxes=batch["boxes"].numpy())
    for k, p_ in model.named_parameters():
        if k in trainable:
            sub, sc, nrm = mg._grad_sample(p_.grad.numpy(), n=SAMPLE)
            out["grad." + k] = sub
            out["scale." + k] = np.float64(sc)
            out["norm." + k] = np.float64(nrm)
    meta = dict(cfg=dict(cfg, grounding_tokenizer=syn.GROUNDING_TOKENIZERS[kind], inpaint_mode=True), kind=kind, B=B, hw=HW, n_valid=N_VALID,
                batch_seed=5, latent_seed=6, context_seed=6, target_seed=7, timesteps=TIMESTEPS, weight_seed=1234, n_trainable=len(trainable),
                sample=SAMPLE)
    path = os.path.join(mg.OUT, NAMES[kind] + ".npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(f"{NAMES[kind]}: loss {loss.item():.6f}, {len(trainable)} trainable tensors, mask zeros {int((mask == 0).sum())}, "
          f"{os.path.getsize(path)} bytes [{time.time() - t0:.1f}s]")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=list(NAMES))
    for kind in ap.parse_args().only:
        train_case(kind)
