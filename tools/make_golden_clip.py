"""Generate the CLIP text tower goldens. The reference's text encoder IS transformers.CLIPTextModel (reference
ldm/modules/encoders/modules.py:144-173), so the golden is that class in fp32 on the CPU with seeded weights:

    tests/golden/clip_text_small.npz     2 layers, intermediate 256, width 768 / 12 heads, 4 sequences of 1, 7, 30, 75 tokens
    tests/golden/clip_text_full.npz      12 layers, intermediate 3072 (ViT-L/14 text tower), 8 sequences of 1 .. 75 tokens
    tests/golden/clip_text_full_b.npz    last_hidden of sequences 4..7 of the full case (one file would exceed the 1 MiB per file
                                         kept under tests/golden/; tests/test_clip_*.py join the two)

Every floating tensor is gligen_amd.synthetic.seeded_tensor("transformer.text_model." + key, shape, seed=777): the transformers 4.x
key is the canonical one whatever version is installed. Stored: ids, last_hidden, pooled and the YARDSTICKS autocast_rel_mse_hidden /
autocast_rel_mse_pooled (overall and per sequence) = relative MSE of the same model under torch.autocast("cpu", torch.bfloat16)
against its fp32 run -- torch's own bf16 error on the reference, which the GPU parity bars are multiples of -- plus a JSON meta.

    PYTHONPATH=. python tools/make_golden_clip.py
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gligen_amd import synthetic as syn  # noqa: E402

SEED, BOS, EOS = 777, 49406, 49407
CASES = {"small": dict(layers=2, intermediate=256, lengths=[1, 7, 30, 75]),
         "full": dict(layers=12, intermediate=3072, lengths=[1, 2, 5, 9, 20, 40, 75, 75])}


def build_tower(layers, intermediate):
    """transformers' CLIPTextModel (width 768, 12 heads, 77 positions, quick_gelu) with the seeded weights, fp32, eval."""
    import transformers
    cfg = transformers.CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=intermediate, num_hidden_layers=layers,
                                      num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu")
    model = transformers.CLIPTextModel(cfg).eval()
    sd = model.state_dict()
    new = {}
    for k, v in sd.items():
        canon = k if k.startswith("text_model.") else "text_model." + k
        new[k] = syn.seeded_tensor("transformer." + canon, tuple(v.shape), seed=SEED) if v.is_floating_point() else v
    model.load_state_dict(new, strict=True)
    return model


def make_ids(lengths):
    g = torch.Generator().manual_seed(5)
    ids = torch.full((len(lengths), 77), EOS, dtype=torch.int64)
    ids[:, 0] = BOS
    for i, n in enumerate(lengths):
        ids[i, 1:1 + n] = torch.randint(0, BOS, (n,), generator=g)
    return ids


def rel_mse(a, b):
    return float(((a.double() - b.double()) ** 2).mean() / (b.double() ** 2).mean())


@torch.no_grad()
def run_case(name):
    c = CASES[name]
    model = build_tower(c["layers"], c["intermediate"])
    ids = make_ids(c["lengths"])
    ref = model(input_ids=ids)
    hidden, pooled = ref.last_hidden_state.float(), ref.pooler_output.float()
    with torch.autocast("cpu", torch.bfloat16):
        ac = model(input_ids=ids)
    ah, ap = ac.last_hidden_state.float(), ac.pooler_output.float()
    import transformers
    out = dict(ids=ids.numpy(), last_hidden=hidden.numpy(), pooled=pooled.numpy(),
               autocast_rel_mse_hidden=np.float64(rel_mse(ah, hidden)), autocast_rel_mse_pooled=np.float64(rel_mse(ap, pooled)),
               autocast_rel_mse_hidden_per_seq=np.array([rel_mse(ah[i], hidden[i]) for i in range(len(ids))]),
               autocast_rel_mse_pooled_per_seq=np.array([rel_mse(ap[i], pooled[i]) for i in range(len(ids))]),
               meta=np.array(json.dumps(dict(seed=SEED, layers=c["layers"], intermediate=c["intermediate"], lengths=c["lengths"],
                                             transformers=transformers.__version__, torch=torch.__version__, threads=torch.get_num_threads()))))
    return out


def load_case(name, golden_dir=None):
    """The arrays of one case (the full case's last_hidden joined from its two files)."""
    golden_dir = golden_dir or os.path.join(REPO, "tests", "golden")
    d = dict(np.load(os.path.join(golden_dir, f"clip_text_{name}.npz")))
    if "last_hidden_a" in d:
        b = np.load(os.path.join(golden_dir, f"clip_text_{name}_b.npz"))
        d["last_hidden"] = np.concatenate([d.pop("last_hidden_a"), b["last_hidden_b"]], axis=0)
    return d


def main():
    gd = os.path.join(REPO, "tests", "golden")
    for name in CASES:
        out = run_case(name)
        print(name, "hidden std %.3f max %.2f" % (out["last_hidden"].std(), np.abs(out["last_hidden"]).max()),
              "autocast rel mse hidden %.3e pooled %.3e" % (out["autocast_rel_mse_hidden"], out["autocast_rel_mse_pooled"]))
        if out["last_hidden"].nbytes > 900 * 1024:      # split so that no file exceeds 1 MiB
            h = out.pop("last_hidden")
            half = len(h) // 2
            out["last_hidden_a"] = h[:half]
            np.savez(os.path.join(gd, f"clip_text_{name}_b.npz"), last_hidden_b=h[half:])
        np.savez(os.path.join(gd, f"clip_text_{name}.npz"), **out)


if __name__ == "__main__":
    main()
