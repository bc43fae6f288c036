"""Fingerprint of the training path: one line per case with a SHA-256 over loss, eps and every gradient tensor (sorted by name) of
gl_unet_train_step, and the arena's high-water mark. Two builds of the library that launch the same kernels on the same operands in
the same order print the same lines. Synthetic inputs, seeded weights, small UNet, B = 2, 16 x 16 latent: every tokenizer, the class-map inputs, an
inpainting model and the three fuser types.
   GL_DEV_SWITCHES=1 GL_GEMM_AUTOTUNE=0 PYTHONPATH=. python tools/train_outputs.py      (no timed tile choice: repeatable across processes)"""
import hashlib

import torch

from gligen_amd import synthetic as syn
from gligen_amd.engine import SPATIAL_MAP_KEYS, Engine
from gligen_amd.train import trainable_names

B, HW = 2, 16


def state_dict(cfg, dev):
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    m = UNetModel(**dict(cfg, inpaint_mode=bool(cfg.get("inpaint_mode"))))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    return {k: v.float().to(dev).contiguous() for k, v in syn.seeded_state_dict(shapes, 1234).items()}


def common():
    return dict(x=syn.make_latent(B, 4, HW, HW, seed=6), timesteps=torch.tensor([981., 441.]), context=syn.make_context(B, seed=6),
                target=syn.make_latent(B, 4, HW, HW, seed=7))


def discrete(kind, **kw):
    b = syn.make_batch(kind, B, n_valid=3, seed=5, **kw)
    batch = dict(common(), masks=b["masks"])
    if kind == "keypoint":
        batch["points"] = b["points"]
    elif kind == "text_image":
        batch.update(boxes=b["boxes"], text_embeddings=b["text_embeddings"], image_embeddings=b["image_embeddings"], text_masks=b["text_masks"],
                     image_masks=b["image_masks"])
    else:
        batch.update(boxes=b["boxes"], positive_embeddings=b["text_embeddings"])
    return dict(syn.UNET_CFG_SMALL, grounding_tokenizer=syn.GROUNDING_TOKENIZERS[kind]), batch


def inpaint():
    """The text model with inpaint_mode: inpainting_extra_input = cat(z * mask, mask), the mask 0 inside the boxes (trainer.py:339-344)."""
    cfg, batch = discrete("text")
    z, mask = syn.make_latent(B, 4, HW, HW, seed=8), torch.ones(B, 1, HW, HW)
    for b in range(B):
        for x0, y0, x1, y1 in (batch["boxes"][b] * HW).int().tolist():
            mask[b, :, y0:y1, x0:x1] = 0
    return dict(cfg, inpaint_mode=True), dict(batch, inpainting_extra_input=torch.cat([z * mask, mask], dim=1))


def fuser(fuser_type, cfg, batch):
    return dict(cfg, fuser_type=fuser_type), batch


def spatial(modality, class_maps=False):
    ds, tk = dict(resize_input=4 * HW, out_dim=8), dict(resize_input=64, out_dim=768)
    if modality == "sem":
        ds["in_dim"], tk["in_dim"] = 152, 152
    cfg = dict(syn.UNET_CFG_SMALL, grounding_downsampler=dict(target=f"ldm.modules.diffusionmodules.{modality}_grounding_downsampler.GroundingDownsampler", params=ds),
               grounding_tokenizer=dict(target=f"ldm.modules.diffusionmodules.{modality}_grounding_net.PositionNet", params=tk))
    img = syn.make_spatial_map(modality, B, 64, seed=3)
    if class_maps:
        img = img.argmax(1, keepdim=True).to(torch.uint8)
    return cfg, dict(common(), **{SPATIAL_MAP_KEYS[modality]: img, "mask": torch.ones(B, 1), "grounding_extra_input": img})


def case(name, cfg, batch, iterations=1, **kw):
    eng = Engine(0, arena_gb=24.0)          # a fresh arena per case: its high water is this case's
    sd = state_dict(cfg, eng.device)
    grads = {k: torch.zeros_like(sd[k]) for k in trainable_names(sd, cfg)}
    if kw.get("use_weight_cache"):
        eng.train_weight_cache(True)
    for _ in range(iterations):
        loss, eps, _ = eng.unet_train_step(cfg, sd, batch, grads=grads, **kw)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in [loss, eps] + [grads[k] for k in sorted(grads)]:
        h.update(t.detach().float().cpu().contiguous().numpy().tobytes())
    print(f"{name}: sha256 {h.hexdigest()} loss {float(loss):.9g} tensors {len(grads)} arena_high_water {eng.arena_high_water()}", flush=True)
    if kw.get("use_weight_cache"):
        eng.train_weight_cache(False)


if __name__ == "__main__":
    case("text", *discrete("text"))
    case("text, checkpoint", *discrete("text"), checkpoint=True)
    case("text, weight cache, 2 iterations", *discrete("text"), iterations=2, use_weight_cache=True)
    case("text+image", *discrete("text_image"))
    case("keypoint", *discrete("keypoint"))
    case("canny tokenizer + downsampler", *spatial("canny"))
    case("sem from planes", *spatial("sem"))
    case("sem from class maps", *spatial("sem", class_maps=True))
    case("text, inpaint_mode", *inpaint())
    case("gatedSA2", *fuser("gatedSA2", *discrete("text", max_objs=16)))           # a square Ng (and the square latent): 4 x 4 tokens
    case("gatedCA", *fuser("gatedCA", *discrete("text")))
    case("gatedSA2, canny tokenizer + downsampler", *fuser("gatedSA2", *spatial("canny")))      # Ng = (64 / 32)^2
