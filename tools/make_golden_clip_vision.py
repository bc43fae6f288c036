"""Generate the CLIP vision tower goldens. The reference reads its image features from transformers' CLIPModel (reference
gligen_inference.py:104-128); the vision side of that class is CLIPVisionModelWithProjection, so the golden is that class in fp32
on the CPU with seeded weights:

    tests/golden/clip_vision_small.npz    2 layers, width 256 / 4 heads, intermediate 512, patch 14 of 224: 257 tokens, 3 images,
                                          the whole last_hidden
    tests/golden/clip_vision_small50.npz  2 layers, width 128 / 2 heads, intermediate 256, patch 32 of 224: 50 tokens, 3 images
    tests/golden/clip_vision_full.npz     ViT-L/14 (24 layers, 1024 / 16 heads, 4096), 4 images; last_hidden rows ROWS only (the whole
                                          tensor is 1 MB per image)

Every floating tensor is gligen_amd.synthetic.seeded_tensor(key, shape, seed=778) under the transformers key (vision_model.*,
visual_projection.weight). The pixels come from a seeded CPU generator at CLIP-normalised scale (std 1.2), not from seeded_tensor.
Stored: pixel seed and shape (the pixels are regenerated, not stored), last_hidden, pooled = post_layernorm(last_hidden[:, 0]),
image_embeds (not normalised), feature = 28.7 * unit(image_embeds @ P) under the seeded 768 x 768 stand-in P of the reference's
projection_matrix, the YARDSTICKS autocast_rel_mse_{hidden,pooled,embeds,feature} (overall and per image) = relative MSE of the same
model under torch.autocast("cpu", torch.bfloat16) against its fp32 run, the pairwise relative squared distances of the images' final
features, and a JSON meta.

    PYTHONPATH=. python tools/make_golden_clip_vision.py
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gligen_amd import synthetic as syn  # noqa: E402

SEED, PIXEL_SEED, PIXEL_STD, PROJECTION = 778, 41, 1.2, 768
ROWS = [0, 1, 17, 128, 255, 256]
CASES = {"small": dict(layers=2, width=256, heads=4, intermediate=512, patch=14, image_size=224, images=3),
         "small50": dict(layers=2, width=128, heads=2, intermediate=256, patch=32, image_size=224, images=3),
         "full": dict(layers=24, width=1024, heads=16, intermediate=4096, patch=14, image_size=224, images=4, rows=ROWS)}


def vision_config(c, hidden_act="quick_gelu"):
    import transformers
    return transformers.CLIPVisionConfig(hidden_size=c["width"], intermediate_size=c["intermediate"], num_hidden_layers=c["layers"],
                                         num_attention_heads=c["heads"], image_size=c["image_size"], patch_size=c["patch"],
                                         projection_dim=PROJECTION, hidden_act=hidden_act)


def build_tower(c):
    """transformers' CLIPVisionModelWithProjection of one case with the seeded weights, fp32, eval."""
    import transformers
    model = transformers.CLIPVisionModelWithProjection(vision_config(c)).eval()
    new = {k: (syn.seeded_tensor(k, tuple(v.shape), seed=SEED) if v.is_floating_point() else v) for k, v in model.state_dict().items()}
    model.load_state_dict(new, strict=True)
    return model


def make_pixels(c):
    g = torch.Generator().manual_seed(PIXEL_SEED)
    return PIXEL_STD * torch.randn((c["images"], 3, c["image_size"], c["image_size"]), generator=g)


def projection_matrix():
    """A seeded stand-in of the reference's 768 x 768 `projection_matrix` file (tests/test_host_cpu.py draws it the same way)."""
    return torch.randn(PROJECTION, PROJECTION, generator=torch.Generator().manual_seed(5)) * 0.03


def final_feature(image_embeds, P):
    """gligen_inference.get_clip_feature's tail: project(x, P.T) = x @ P, unit norm x 28.7."""
    f = image_embeds.float() @ P
    return 28.7 * f / f.norm(dim=-1, keepdim=True)


def rel_mse(a, b):
    return float(((a.double() - b.double()) ** 2).mean() / (b.double() ** 2).mean())


def pairwise_rel_sq_dist(f):
    """d[i][j] = |f_i - f_j|^2 / |f_j|^2 = the relative MSE of answering image j with image i's feature."""
    f = f.double()
    return ((f[:, None] - f[None]) ** 2).sum(-1) / (f ** 2).sum(-1)[None]


def tower_outputs(model, pixels):
    out = model(pixel_values=pixels)
    hidden = out.last_hidden_state
    pooled = model.vision_model.post_layernorm(hidden[:, 0])
    return hidden.float(), pooled.float(), out.image_embeds.float()


@torch.no_grad()
def run_case(name):
    import transformers
    c = CASES[name]
    model = build_tower(c)
    pixels = make_pixels(c)
    P = projection_matrix()
    hidden, pooled, embeds = tower_outputs(model, pixels)
    feature = final_feature(embeds, P)
    with torch.autocast("cpu", torch.bfloat16):
        ah, ap, ae = tower_outputs(model, pixels)
    af = final_feature(ae, P)
    n = c["images"]
    rows = c.get("rows")
    out = dict(last_hidden=(hidden[:, rows] if rows else hidden).numpy(), pooled=pooled.numpy(), image_embeds=embeds.numpy(), feature=feature.numpy(),
               feature_pairwise_rel_sq_dist=pairwise_rel_sq_dist(feature).numpy())
    if rows:
        out["rows"] = np.array(rows)
        hidden, ah = hidden[:, rows], ah[:, rows]       # the yardstick of what is stored and compared
    for key, a, b in (("hidden", ah, hidden), ("pooled", ap, pooled), ("embeds", ae, embeds), ("feature", af, feature)):
        out["autocast_rel_mse_" + key] = np.float64(rel_mse(a, b))
        out["autocast_rel_mse_" + key + "_per_image"] = np.array([rel_mse(a[i], b[i]) for i in range(n)])
    out["meta"] = np.array(json.dumps(dict(seed=SEED, pixel_seed=PIXEL_SEED, pixel_std=PIXEL_STD, **{k: v for k, v in c.items()},
                                           tokens=(c["image_size"] // c["patch"]) ** 2 + 1, projection_dim=PROJECTION,
                                           transformers=transformers.__version__, torch=torch.__version__, threads=torch.get_num_threads())))
    return out


def load_case(name, golden_dir=None):
    golden_dir = golden_dir or os.path.join(REPO, "tests", "golden")
    return dict(np.load(os.path.join(golden_dir, f"clip_vision_{name}.npz")))


def main():
    gd = os.path.join(REPO, "tests", "golden")
    for name in CASES:
        out = run_case(name)
        d = out["feature_pairwise_rel_sq_dist"]
        print(name, "hidden std %.3f max %.2f" % (out["last_hidden"].std(), np.abs(out["last_hidden"]).max()),
              "autocast rel mse hidden %.3e pooled %.3e embeds %.3e feature %.3e" % tuple(float(out["autocast_rel_mse_" + k]) for k in ("hidden", "pooled", "embeds", "feature")),
              "min pairwise feature distance %.3e" % d[~np.eye(len(d), dtype=bool)].min())
        np.savez(os.path.join(gd, f"clip_vision_{name}.npz"), **out)


if __name__ == "__main__":
    main()
