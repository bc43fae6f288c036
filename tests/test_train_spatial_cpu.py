"""The training step of the spatial-map models (ConvNeXt tokenizer, GroundingDownsampler, 4 + k channel first conv), host side and
pinning, no GPU: the reference's trainable set (trainer.py:189-245), the gradient milestones, the guidance drop, and the three
training goldens (tools/make_golden_train_spatial.py: the reference's loss.backward()) against autograd through the CPU oracle --
which makes the oracle the full-tensor checker of these models' gradients."""
import numpy as np
import pytest
import torch

from helpers import golden_shapes, load_golden, oracle_cfg
from gligen_amd import synthetic as syn
from gligen_amd.train import GROUNDING_KEYS, gradient_milestones, null_grounding, trainable_names

N_TRAINABLE = {"canny": 310, "hed": 306, "sem": 312}
MAP_KEYS = dict(canny="canny_edge", hed="hed_edge", depth="depth", normal="normal", sem="sem")


def spatial_batch(meta):
    """The batch of tools/make_golden_train_spatial.py:inputs, rebuilt from the same seeds: the tokenizer's map and mask, the
    downsampler's input (the same map: GroundingDSInput.prepare passes it through), latent, timesteps, context, noise."""
    B, hw = meta["B"], meta["hw"]
    img = syn.make_spatial_map(meta["modality"], B, meta["res"], seed=meta["map_seed"])
    return dict(img=img, mask=torch.tensor(meta["mask"], dtype=torch.float32).reshape(B, 1), extra=img,
                x=syn.make_latent(B, 4, hw, hw, seed=meta["latent_seed"]), timesteps=torch.tensor([981, 441][:B], dtype=torch.long),
                context=syn.make_context(B, seed=meta["context_seed"]), target=syn.make_latent(B, 4, hw, hw, seed=meta["target_seed"]))


def oracle_autograd(sd, meta, trainable, batch):
    """loss, eps and the full gradient of every `trainable` tensor by autograd through the CPU oracle (oracle/gligen_oracle.py)."""
    from oracle import gligen_oracle as orc
    tk = meta["cfg"]["grounding_tokenizer"]["params"]
    cfg = dict(oracle_cfg(meta["cfg"], "spatial"), tok_resize=tk["resize_input"], downsampler=meta["downsampler"])
    sdo = {k: v.detach().float().cpu().clone() for k, v in sd.items()}
    for k in trainable:
        sdo[k].requires_grad_(True)
    inp = dict(x=batch["x"], timesteps=batch["timesteps"].long(), context=batch["context"],
               grounding_input=dict(image=batch["img"], mask=batch["mask"]), grounding_extra_input=batch["extra"])
    eps = orc.unet_forward(sdo, cfg, inp)
    loss = torch.nn.functional.mse_loss(eps, batch["target"])
    loss.backward()
    return loss.detach(), eps.detach(), {k: sdo[k].grad for k in trainable}


def rel_mse(a, ref):
    a, ref = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(ref).float()
    return float(((a - ref) ** 2).mean() / (ref ** 2).mean().clamp_min(1e-30))


def golden_report(g, grads):
    """rel-MSE of every gradient on the golden's strided sample (the tanh gates held as ONE vector), and the norm ratios."""
    n = g["meta"]["sample"]
    gates = sorted(k for k in grads if k.endswith(".alpha_attn") or k.endswith(".alpha_dense"))
    report = {"<the gates>": rel_mse(torch.stack([grads[k].reshape(()).float().cpu() for k in gates]),
                                     np.array([float(g["grad." + k][0]) * float(g["scale." + k]) for k in gates], dtype=np.float32))}
    norms = {}
    for k, gt in grads.items():
        if k in gates:
            continue
        flat = gt.detach().float().cpu().reshape(-1)
        stride = max(1, flat.numel() // n)
        sub = flat[::stride][:n] if flat.numel() > n else flat
        report[k] = rel_mse(sub, torch.from_numpy(g["grad." + k].astype(np.float32)) * float(g["scale." + k]))
        nrm, ref_nrm = float(flat.double().norm()), float(g["norm." + k])
        norms[k] = 1.0 if nrm == ref_nrm == 0.0 else nrm / max(ref_nrm, 1e-30)     # (hed, B 1, mask 1: the null feature's gradient is 0)
    return report, norms


@pytest.mark.parametrize("modality", sorted(N_TRAINABLE))
def test_trainable_names_spatial(modality):
    """trainer.py:217-242 on a spatial model: fuser.*, position_net.* (the ConvNeXt backbone's 178 tensors among them), every
    downsample_net.* tensor, and the first conv's weight -- not its bias. From the config, or from the state_dict alone."""
    shapes = golden_shapes(f"unet_small_{modality}")
    cfg = load_golden(f"unet_small_{modality}_train_step")["meta"]["cfg"]
    for names in (trainable_names(shapes, cfg), trainable_names(shapes)):
        assert len(names) == N_TRAINABLE[modality]
        assert "input_blocks.0.0.weight" in names and "input_blocks.0.0.bias" not in names
        assert all(k in names for k in shapes if k.startswith("downsample_net."))
        assert sum(k.startswith("position_net.convnext_tiny_backbone.") for k in names) == 178
    # the discrete models keep the set they had (no downsampler: the first conv stays frozen)
    assert len(trainable_names(golden_shapes("unet_small_train_step"))) == 127
    assert "input_blocks.0.0.weight" not in trainable_names(golden_shapes("unet_small_inpaint"))


def test_gradient_milestones_spatial():
    """The tokenizer's, the downsampler's and the first conv's gradients are final at the end of the backward (milestone n_blocks)."""
    names = trainable_names(golden_shapes("unet_small_canny"))
    ms = gradient_milestones(names)
    n_blocks = max(ms.values())
    assert n_blocks == 7
    new = [k for k in names if k.startswith("downsample_net.") or k.startswith("position_net.") or k == "input_blocks.0.0.weight"]
    assert len(new) == 4 + 1 + 178 + 2 + 6          # downsampler, first conv, ConvNeXt, pos_embedding + null_feature, the MLP
    assert all(ms[k] == n_blocks for k in new)
    assert all(ms[k] < n_blocks for k in names if ".fuser." in k)


def test_null_grounding_spatial():
    """The 10 % guidance drop (openaimodel.py:428-429) replaces the tokenizer's input only: zero map, mask 0; grounding_extra_input
    and the rest of the batch stay."""
    B = 2
    for key in MAP_KEYS.values():
        assert key in GROUNDING_KEYS
    assert "mask" in GROUNDING_KEYS and "grounding_extra_input" not in GROUNDING_KEYS
    batch = dict(canny_edge=torch.rand(B, 3, 32, 32) + 0.1, mask=torch.ones(B, 1), grounding_extra_input=torch.rand(B, 3, 32, 32) + 0.1,
                 x=torch.randn(B, 4, 8, 8), timesteps=torch.tensor([981.0, 441.0]))
    nb = null_grounding(batch)
    assert torch.count_nonzero(nb["canny_edge"]) == 0 and torch.count_nonzero(nb["mask"]) == 0
    assert nb["canny_edge"].shape == batch["canny_edge"].shape
    for k in ("grounding_extra_input", "x", "timesteps"):
        assert torch.equal(nb[k], batch[k])
    # "mask" is the spatial tokenizers' key only: no discrete tokenizer's batch carries it (theirs is "masks")
    for kind in ("text", "text_image", "keypoint"):
        assert "mask" not in syn.make_batch(kind, B, n_valid=2, seed=5)


@pytest.mark.parametrize("modality", ["canny", "hed", "sem"])
def test_spatial_train_golden_vs_oracle_autograd(modality):
    """Autograd through the CPU oracle reproduces the reference's loss.backward() on the spatial training goldens: loss, eps and every
    stored gradient sample (the ConvNeXt backbone, pos_embedding, null_feature, the MLP, in_conv for sem, the downsampler, the first
    conv's weight, the fusers) and norm. This pins the oracle as the full-tensor checker of these models' gradients."""
    g = load_golden(f"unet_small_{modality}_train_step")
    meta = g["meta"]
    sd = syn.seeded_state_dict(golden_shapes(f"unet_small_{modality}"), meta["weight_seed"])
    names = trainable_names(sd, meta["cfg"])
    assert len(names) == meta["n_trainable"] == N_TRAINABLE[modality]
    assert sorted(names) == sorted(k[5:] for k in g if k.startswith("grad."))
    loss, eps, grads = oracle_autograd(sd, meta, names, spatial_batch(meta))
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < 1e-5
    assert rel_mse(eps, g["eps"]) < 1e-5
    report, norms = golden_report(g, grads)
    worst = max(report, key=report.get)
    print(modality, "oracle autograd vs reference: worst", worst, report[worst])
    assert not {k: v for k, v in report.items() if v >= 1e-5}
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), {k: v for k, v in norms.items() if abs(v - 1) >= 1e-3}


def test_ctypes_train_spatial_in_matches_the_c_header(tmp_path):
    """gl_train_spatial_in has the same size in include/gligen_amd.h (gcc, C99) and in its ctypes mirror (gligen_amd/_lib.py), and the
    new entry point is bound."""
    import ctypes as C
    import os
    import shutil
    import subprocess
    from helpers import ROOT
    from gligen_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gligen_amd.h"\nint main(void) {\n  printf("%zu\\n", sizeof(gl_train_spatial_in));\n  return 0;\n}\n')
    exe = tmp_path / "sz"
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == C.sizeof(_lib.TrainSpatialIn)
    assert "gl_unet_train_step_spatial" in _lib.SYMBOLS
