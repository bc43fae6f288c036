"""Training the inpainting models (inpaint_mode: 9-channel first conv; trainer.py:189-194, 339-344), host side and pinning, no GPU:
the trainable set with and without a config, add_input_channels, the entry point of include/gligen_amd_train_inputs.h (declared,
exported, bound, one struct layout in C and ctypes), the trainer's input stage restated in torch against the goldens
(tools/make_golden_train_inpaint.py: the reference's q_sample, draw_masks_from_boxes and loss.backward()), autograd through the CPU
oracle against the same goldens, and the ISA of the step-input kernel."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from helpers import ROOT, golden_shapes, grounding_kwargs, load_golden, oracle_cfg
from gligen_amd import synthetic as syn
from gligen_amd.train import add_input_channels, gradient_milestones, null_grounding, trainable_names
from test_train_spatial_cpu import golden_report, rel_mse

CASES = {"text": "unet_small_inpaint_train_step", "text_image": "unet_small_ti_inpaint_train_step"}
N_TRAINABLE = {"text": 128, "text_image": 135}
FIRST_CONV = "input_blocks.0.0.weight"


def inpaint_shapes(kind):
    """The state_dict shapes of the small inpainting model: the unet_small_inpaint entry (text), or the text+image model's with the
    9-channel first conv."""
    if kind == "text":
        return golden_shapes("unet_small_inpaint")
    return dict(golden_shapes("unet_small_text_image"), **{FIRST_CONV: [320, 9, 3, 3]})


def schedule():
    """The diffusion's q_sample tables (oracle/make_golden.py:misc_case: LatentDiffusion's buffers), fp32 [1000] each."""
    m = load_golden("misc")
    return dict(sqrt_alphas_cumprod=torch.from_numpy(m["diff_sqrt_alphas_cumprod"]),
                sqrt_one_minus_alphas_cumprod=torch.from_numpy(m["diff_sqrt_one_minus_alphas_cumprod"]))


def box_mask(boxes, size):
    """draw_masks_from_boxes(boxes, size) without its random branches (inpaint_mask_func.py:22-32), restated: the fp32 product
    box * size, int() of each coordinate, zeros in [y0:y1, x0:x1]. [B, 1, size, size]."""
    out = torch.ones(boxes.shape[0], 1, size, size)
    for b, bx in enumerate(boxes.float()):
        for box in bx:
            x0, y0, x1, y1 = (int(v) for v in box * size)
            out[b, 0, y0:y1, x0:x1] = 0
    return out


def restate_step_inputs(z, noise, t, sched, boxes=None, mask=None):
    """trainer.py:329-364 in torch on the CPU: (x_noisy, mask, inpainting_extra_input); mask and extra None without boxes / mask."""
    a = sched["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1)
    s = sched["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1)
    x_noisy = a * z + s * noise                                            # ldm.py:19-22
    if boxes is not None:
        mask = box_mask(boxes, z.shape[-1])
    if mask is None:
        return x_noisy, None, None
    mask = mask.reshape(z.shape[0], 1, z.shape[2], z.shape[3]).float()
    return x_noisy, mask, torch.cat([z * mask, mask], dim=1)


def golden_inputs(g):
    """The inputs of tools/make_golden_train_inpaint.py, rebuilt from the same seeds, with the golden's overwritten boxes."""
    meta = g["meta"]
    B, hw = meta["B"], meta["hw"]
    b = syn.make_batch(meta["kind"], B, n_valid=meta["n_valid"], seed=meta["batch_seed"])
    b["boxes"] = torch.from_numpy(g["boxes"]).clone()
    return dict(b=b, z=syn.make_latent(B, 4, hw, hw, seed=meta["latent_seed"]), noise=syn.make_latent(B, 4, hw, hw, seed=meta["target_seed"]),
                t=torch.tensor(meta["timesteps"], dtype=torch.long), context=syn.make_context(B, seed=meta["context_seed"]))


def reference_batch(g, d):
    """The batch of Engine.unet_train_step under the reference's keys, x_noisy and inpainting_extra_input from the golden."""
    b, kind = d["b"], g["meta"]["kind"]
    batch = dict(x=torch.from_numpy(g["x_noisy"]), inpainting_extra_input=torch.from_numpy(g["inpainting_extra_input"]), timesteps=d["t"].float(),
                 context=d["context"], boxes=b["boxes"], masks=b["masks"], target=d["noise"])
    if kind == "text_image":
        batch.update(text_embeddings=b["text_embeddings"], image_embeddings=b["image_embeddings"], text_masks=b["text_masks"], image_masks=b["image_masks"])
    else:
        batch["positive_embeddings"] = b["text_embeddings"]
    return batch


def oracle_autograd(sd, cfg, kind, trainable, d, x, extra):
    """loss, eps and the full gradient of every `trainable` tensor by autograd through the CPU oracle; x = the noised latent, extra =
    inpainting_extra_input (None: a model without the five extra channels)."""
    from oracle import gligen_oracle as orc
    sdo = {k: v.detach().float().cpu().clone() for k, v in sd.items()}
    for k in trainable:
        sdo[k].requires_grad_(True)
    inp = dict(x=x, timesteps=d["t"].long(), context=d["context"], grounding_input=grounding_kwargs(kind, d["b"]), inpainting_extra_input=extra)
    eps = orc.unet_forward(sdo, oracle_cfg(cfg, kind), inp)
    loss = torch.nn.functional.mse_loss(eps, d["noise"])
    loss.backward()
    return loss.detach(), eps.detach(), {k: sdo[k].grad for k in trainable}


def test_trainable_names_inpaint():
    """trainer.py:191-194, 233 with inpaint_mode: the first conv's weight joins fuser.* and position_net.*, its bias does not. Without
    a config the set is what it was (a 9-channel first conv alone does not say that it is trained)."""
    shapes = inpaint_shapes("text")
    cfg = load_golden(CASES["text"])["meta"]["cfg"]
    assert cfg["inpaint_mode"] is True
    names = trainable_names(shapes, cfg)
    assert len(names) == 128 and FIRST_CONV in names and "input_blocks.0.0.bias" not in names
    plain = trainable_names(shapes)
    assert len(plain) == 127 and FIRST_CONV not in plain and set(plain) == set(names) - {FIRST_CONV}
    assert trainable_names(shapes, dict(cfg, inpaint_mode=False)) == plain
    assert len(trainable_names(inpaint_shapes("text_image"), load_golden(CASES["text_image"])["meta"]["cfg"])) == 135
    ms = gradient_milestones(names)
    n_st = max(ms.values())
    assert n_st == 7 and ms[FIRST_CONV] == n_st and all(ms[k] < n_st for k in names if ".fuser." in k)


def test_null_grounding_keeps_the_inpainting_inputs():
    """The guidance drop replaces the grounding input only (openaimodel.py:428-429): inpainting_extra_input, x_rows and target_rows stay."""
    B = 2
    b = syn.make_batch("text", B, n_valid=2, seed=5)
    batch = dict(boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"], x=torch.randn(B, 4, 8, 8),
                 inpainting_extra_input=torch.rand(B, 5, 8, 8) + 0.1, x_rows=torch.rand(B, 8, 8, 9) + 0.1, target_rows=torch.rand(B, 8, 8, 4) + 0.1)
    nb = null_grounding(batch)
    for k in ("boxes", "masks", "positive_embeddings"):
        assert torch.count_nonzero(nb[k]) == 0
    for k in ("x", "inpainting_extra_input", "x_rows", "target_rows"):
        assert torch.equal(nb[k], batch[k]), k


def test_add_input_channels():
    """trainer.py:189-193: the first conv zero-extended by five input channels; the first four keep their bits."""
    sd = syn.seeded_state_dict(golden_shapes("unet_small_text"), 1234)
    w0 = sd[FIRST_CONV].clone()
    out = add_input_channels(sd, 5)
    assert tuple(out[FIRST_CONV].shape) == (320, 9, 3, 3)
    assert torch.equal(out[FIRST_CONV][:, :4], w0) and torch.count_nonzero(out[FIRST_CONV][:, 4:]) == 0
    assert torch.equal(sd[FIRST_CONV], w0) and tuple(sd[FIRST_CONV].shape) == (320, 4, 3, 3)          # the input is not written
    assert all(out[k] is sd[k] for k in sd if k != FIRST_CONV)
    assert {k: list(v.shape) for k, v in out.items()} == {k: list(v) for k, v in inpaint_shapes("text").items()}


def _declared(header):
    return set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_train_inputs_entry_point_is_declared_exported_and_bound():
    """include/gligen_amd_train_inputs.h declares exactly the names of TRAIN_INPUT_SYMBOLS, the built library exports them with the
    table's argument types, and the table shares no name with the other tables or headers."""
    from gligen_amd import _lib as table
    from gligen_amd.build import SOURCES, build_native
    assert "train_inputs.hip" in SOURCES
    build_native()
    lib = table.load()
    declared = _declared("gligen_amd_train_inputs.h")
    assert declared == set(table.TRAIN_INPUT_SYMBOLS) == {"gl_train_step_inputs"}
    raw = ctypes.CDLL(str(table.LIB_PATH))
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes == table.TRAIN_INPUT_SYMBOLS[name][1] and getattr(lib, name).restype == table.TRAIN_INPUT_SYMBOLS[name][0]
    assert not declared & (set(table.SYMBOLS) | set(table.IMAGE_SYMBOLS) | set(table.MAP_SYMBOLS) | set(table.TRAIN_MAP_SYMBOLS))
    for other in ("gligen_amd.h", "gligen_amd_image.h", "gligen_amd_maps.h", "gligen_amd_train_maps.h"):
        assert not declared & set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read())), other


def test_ctypes_train_step_inputs_args_matches_the_c_header(tmp_path):
    """A C99 file that includes only the new header compiles; gl_train_step_inputs_args has the same size and field offsets from gcc and
    from ctypes, and struct_size is its first field."""
    from gligen_amd import _lib
    fields = [n for n, _ in _lib.TrainStepInputsArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include "gligen_amd_train_inputs.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(gl_train_step_inputs_args));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(gl_train_step_inputs_args, {n}));\n' for n in fields) + "  return 0;\n}\n")
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.TrainStepInputsArgs) == 112
    assert out[1:] == [getattr(_lib.TrainStepInputsArgs, n).offset for n in fields] and fields[0] == "struct_size" and out[1] == 0


@pytest.mark.parametrize("kind", sorted(CASES))
def test_step_inputs_restated_in_torch_match_the_reference(kind):
    """a[t] * z + s[t] * noise, the box mask and the concatenation, restated in torch from the seeded inputs and the schedule of
    misc.npz, are the reference's q_sample / draw_masks_from_boxes / cat bit for bit -- which pins the restatement the device kernel is
    held to (tests/test_train_inpaint_gpu.py). The golden's boxes hold the cases: 0.0 to 1.0 along x, an overlap, x1 < x0, padding."""
    g = load_golden(CASES[kind])
    d = golden_inputs(g)
    boxes = d["b"]["boxes"]
    assert tuple(boxes[0, 0, [0, 2]].tolist()) == (0.0, 1.0) and float(boxes[1, 0, 2]) < float(boxes[1, 0, 0]) and torch.count_nonzero(boxes[:, 3:]) == 0
    x_noisy, mask, extra = restate_step_inputs(d["z"], d["noise"], d["t"], schedule(), boxes=boxes)
    assert torch.equal(x_noisy, torch.from_numpy(g["x_noisy"]))
    assert torch.equal(mask, torch.from_numpy(g["mask"]))
    assert torch.equal(extra, torch.from_numpy(g["inpainting_extra_input"]))
    m = mask[:, 0]
    assert torch.count_nonzero(m[0, 4:8, :]) == 0 and bool((m[0, 0] == 1).all())       # the 0.0 .. 1.0 box reaches both borders
    assert 0 < int((m[1] == 0).sum()) < int((m[0] == 0).sum())                         # sample 1: its x1 < x0 box masks nothing, the other two do


@pytest.mark.parametrize("kind", sorted(CASES))
def test_inpaint_train_golden_vs_oracle_autograd(kind):
    """Autograd through the CPU oracle (which concatenates inpainting_extra_input in front of the first conv) reproduces the
    reference's loss.backward() on the inpainting goldens: loss, eps, every sampled gradient -- the first conv's weight among them --
    and every norm, at the bars of the spatial goldens. This pins the oracle as the full-tensor checker of the first conv's gradient."""
    g = load_golden(CASES[kind])
    meta = g["meta"]
    sd = syn.seeded_state_dict(inpaint_shapes(kind), meta["weight_seed"])
    names = trainable_names(sd, meta["cfg"])
    assert len(names) == meta["n_trainable"] == N_TRAINABLE[kind]
    assert sorted(names) == sorted(k[5:] for k in g if k.startswith("grad."))
    d = golden_inputs(g)
    loss, eps, grads = oracle_autograd(sd, meta["cfg"], kind, names, d, torch.from_numpy(g["x_noisy"]), torch.from_numpy(g["inpainting_extra_input"]))
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < 1e-5
    assert rel_mse(eps, g["eps"]) < 1e-5
    report, norms = golden_report(g, grads)
    worst = max(report, key=report.get)
    print(kind, "oracle autograd vs reference: worst", worst, report[worst], "first conv", report[FIRST_CONV])
    assert not {k: v for k, v in report.items() if v >= 1e-5}
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), {k: v for k, v in norms.items() if abs(v - 1) >= 1e-3}


def test_step_input_kernel_isa(tmp_path):
    """train_inputs.hip cross-compiled for gfx950: the step-input kernel uses no scratch and spills nothing, and its two products and
    one sum are three separate instructions (no v_fma / v_mac contraction of a[t] z + s[t] noise)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "train_inputs.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--offload-device-only", "-S",
                        os.path.join(ROOT, "gligen_amd", "csrc", "train_inputs.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    entries = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])[1:]
    assert len(entries) == 1
    e = entries[0]
    name = re.search(r"\.name:\s*(\S+)", e).group(1)
    assert "train_step_inputs_kernel" in name
    val = lambda key: int(re.search(rf"\.{key}:\s*(\d+)", e).group(1))
    print("train_step_inputs_kernel: VGPRs", val("vgpr_count"), "SGPRs", val("sgpr_count"))
    assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0
    body = asm[asm.index(name + ":"):asm.index(".Lfunc_end", asm.index(name + ":"))]
    assert "scratch_" not in body
    assert not re.findall(r"\bv_(?:pk_)?(?:fma|fmac|mac)\w*_f32", body), "a[t] z + s[t] noise must stay two products and a sum"
