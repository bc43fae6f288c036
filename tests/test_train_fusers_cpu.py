"""Training the gatedSA2 and gatedCA fuser models, host side and pinning, no GPU: the entry points of
include/gligen_amd_train_fusers.h (declared, exported, bound), the ISA of the two grid-resize kernels, a float64 restatement of the
bicubic grid resize and its transpose (the tap table applied and transposed) held to torch's F.interpolate and its autograd -- it is
the reference of the operator tests in tests/test_train_fusers_gpu.py --, the trainable set on both key sets, and autograd through
the CPU oracle against the five goldens of tools/make_golden_train_fusers.py (the reference's loss.backward()), which makes the
oracle the full-tensor checker of these models' gradients."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from helpers import ROOT, block_backward_inputs, golden_shapes, grounding_kwargs, load_golden, oracle_cfg, _npz
from gligen_amd import synthetic as syn
from gligen_amd.train import trainable_names
from test_train_spatial_cpu import golden_report, rel_mse, spatial_batch
from test_train_spatial_cpu import oracle_autograd as spatial_oracle_autograd

# (sg, sv): upscales, identity, downscales, non-integer ratios, a one-token grid, the largest visual grid of the shipped models
RESIZE_PAIRS = [(4, 16), (4, 8), (4, 4), (4, 2), (3, 8), (1, 4), (8, 5), (8, 64)]
BLOCK_CASES = {"gatedSA2": "block_backward_gatedsa2", "gatedCA": "block_backward_gatedca"}
UNET_CASES = {"gatedsa2": "unet_small_gatedsa2_train_step", "gatedca": "unet_small_gatedca_train_step", "canny_gatedsa2": "unet_small_canny_gatedsa2_train_step"}
UNET_SHAPES = {"gatedsa2": "unet_small_gatedsa2", "gatedca": "unet_small_gatedca", "canny_gatedsa2": "unet_small_canny"}     # gatedSA2 has gatedSA's keys
N_TRAINABLE = {"gatedsa2": 127, "gatedca": 113, "canny_gatedsa2": 310}


# ---- the float64 restatement of the resize
def axis_tables(sg, sv):
    """One axis of torch's bicubic resize sg -> sv (align_corners=False: src = (dst + 0.5) sg / sv - 0.5, A = -0.75, taps clamped to the
    grid) as float64 [sv, sg] matrices: the weights (clamped taps that land on one source index summed), their absolute values summed,
    and the number of taps per entry."""
    A = -0.75
    W, Wabs, cnt = (torch.zeros(sv, sg, dtype=torch.float64) for _ in range(3))
    for o in range(sv):
        f = (o + 0.5) * sg / sv - 0.5
        fl = math.floor(f)
        t = f - fl
        a, b, c = t + 1.0, 1.0 - t, 2.0 - t
        w = [((A * a - 5 * A) * a + 8 * A) * a - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1, ((A + 2) * b - (A + 3)) * b * b + 1,
             ((A * c - 5 * A) * c + 8 * A) * c - 4 * A]
        for p in range(4):
            i = min(max(fl - 1 + p, 0), sg - 1)
            W[o, i] += w[p]
            Wabs[o, i] += abs(w[p])
            cnt[o, i] += 1
    return W, Wabs, cnt


def resize_matrices(sg, sv):
    """The whole operator on a square grid, [sv * sv, sg * sg] float64: weights, absolute weights (per tap), taps per entry."""
    W, Wabs, cnt = axis_tables(sg, sv)
    return torch.kron(W, W), torch.kron(Wabs, Wabs), torch.kron(cnt, cnt)


def resize_ref(t, sg, sv):
    """t [B, sg * sg, C] -> [B, sv * sv, C] in float64: the tap table applied."""
    return torch.einsum("os,bsc->boc", resize_matrices(sg, sv)[0], t.double())


def resize_adjoint_ref(g, sg, sv):
    """g [B, sv * sv, C] -> [B, sg * sg, C] in float64: the tap table transposed."""
    return torch.einsum("os,boc->bsc", resize_matrices(sg, sv)[0], g.double())


def resize_bounds(t, g, sg, sv):
    """The elementwise error bars of the fp32 operators on input t (forward) and g (adjoint): (n + 8) 2^-24 (|W| |v|), n the number
    of terms of that output's sum (16 forward; the taps that land on the source token, backward) and the 8 for the fp32 evaluation of
    the coordinate and the cubic polynomial."""
    _, Wabs, cnt = resize_matrices(sg, sv)
    fwd = (16 + 8) * 2.0 ** -24 * torch.einsum("os,bsc->boc", Wabs, t.double().abs())
    n_bwd = cnt.sum(dim=0)                                                  # [sg * sg]
    bwd = (n_bwd + 8).reshape(1, -1, 1) * 2.0 ** -24 * torch.einsum("os,boc->bsc", Wabs, g.double().abs())
    return fwd, bwd


@pytest.mark.parametrize("sg,sv", RESIZE_PAIRS)
def test_resize_restatement_is_torchs_bicubic_and_its_autograd(sg, sv):
    """The float64 tap table equals F.interpolate(mode="bicubic") on the grid, and its transpose equals that op's autograd."""
    gen = torch.Generator().manual_seed(100 * sg + sv)
    B, C = 2, 5
    t = torch.randn(B, sg * sg, C, generator=gen, dtype=torch.float64)
    g = torch.randn(B, sv * sv, C, generator=gen, dtype=torch.float64)
    x = t.permute(0, 2, 1).reshape(B, C, sg, sg).clone().requires_grad_(True)
    y = torch.nn.functional.interpolate(x, (sv, sv), mode="bicubic")
    y.backward(g.permute(0, 2, 1).reshape(B, C, sv, sv))
    ref = y.detach().reshape(B, C, sv * sv).permute(0, 2, 1)
    ref_adj = x.grad.reshape(B, C, sg * sg).permute(0, 2, 1)
    assert float((resize_ref(t, sg, sv) - ref).abs().max()) < 1e-12
    assert float((resize_adjoint_ref(g, sg, sv) - ref_adj).abs().max()) < 1e-12
    W, Wabs, cnt = axis_tables(sg, sv)
    assert float((W.sum(dim=1) - 1).abs().max()) < 1e-12 and int(cnt.sum()) == 4 * sv      # a partition of unity, four taps per destination
    if sg == sv:
        assert torch.equal(W, torch.eye(sg, dtype=torch.float64))


# ---- the C ABI
def _declared(header):
    return set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_train_fuser_entry_points_are_declared_exported_and_bound():
    """include/gligen_amd_train_fusers.h declares exactly the names of TRAIN_FUSER_SYMBOLS, the built library exports them with the
    table's argument types, and the table shares no name with the other tables or headers."""
    from gligen_amd import _lib as table
    from gligen_amd.build import SOURCES, build_native
    assert "train_fusers.hip" in SOURCES
    build_native()
    lib = table.load()
    declared = _declared("gligen_amd_train_fusers.h")
    assert declared == set(table.TRAIN_FUSER_SYMBOLS) == {"gl_op_block_train_fuser", "gl_op_grid_resize", "gl_op_grid_resize_backward"}
    raw = ctypes.CDLL(str(table.LIB_PATH))
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes == table.TRAIN_FUSER_SYMBOLS[name][1] and getattr(lib, name).restype == table.TRAIN_FUSER_SYMBOLS[name][0]
    others = (table.SYMBOLS, table.IMAGE_SYMBOLS, table.MAP_SYMBOLS, table.TRAIN_MAP_SYMBOLS, table.TRAIN_INPUT_SYMBOLS)
    assert not declared & set().union(*others)
    for other in ("gligen_amd.h", "gligen_amd_image.h", "gligen_amd_maps.h", "gligen_amd_train_maps.h", "gligen_amd_train_inputs.h"):
        assert not declared & set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read())), other
    # gl_op_block_train_fuser: gl_op_block_train's arguments with the kind in front of the dims
    assert table.TRAIN_FUSER_SYMBOLS["gl_op_block_train_fuser"][1] == [ctypes.c_void_p, ctypes.c_int] + table.SYMBOLS["gl_op_block_train"][1][1:]


def test_fuser_kind_mapping_is_one_function():
    from gligen_amd import _lib
    assert [_lib.fuser_kind(k) for k in ("gatedSA", "gatedSA2", "gatedCA", None)] == [0, 1, 2, 0]
    with pytest.raises(ValueError):
        _lib.fuser_kind("gatedXA")


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "gligen_amd_train_fusers.h"\nint main(void) { return sizeof(gl_train_block_dims) == 0; }\n')
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")], check=True)


def test_grid_resize_kernels_isa(tmp_path):
    """train_fusers.hip cross-compiled for gfx950: its two kernels use no scratch and spill nothing; the forward keeps no LDS, the
    backward's tables are dynamic LDS only; both stay at 8 waves per SIMD. Measured: forward 43 VGPRs, backward 46."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "train_fusers.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--offload-device-only", "-S",
                        os.path.join(ROOT, "gligen_amd", "csrc", "train_fusers.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    entries = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])[1:]
    names = [re.search(r"\.name:\s*(\S+)", e).group(1) for e in entries]
    assert len(entries) == 2 and sum("grid_resize_fwd_kernel" in n for n in names) == 1 and sum("grid_resize_bwd_kernel" in n for n in names) == 1, names
    for e, name in zip(entries, names):
        val = lambda key: int(re.search(rf"\.{key}:\s*(\d+)", e).group(1))
        print(name, "VGPRs", val("vgpr_count"), "SGPRs", val("sgpr_count"))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0
        assert val("group_segment_fixed_size") == 0
        assert val("vgpr_count") <= 64          # 8 waves per SIMD
        body = asm[asm.index(name + ":"):asm.index(".Lfunc_end", asm.index(name + ":"))]
        assert "scratch_" not in body
        assert "atomic" not in body             # the adjoint is a gather
        assert ("ds_" in body) == ("bwd" in name)


# ---- the trainable set
def test_trainable_names_on_both_key_sets():
    """trainer.py:217-242 is name-based: a gatedSA2 model has gatedSA's 127 trainable tensors, a gatedCA model has no fuser.linear.*
    (7 fusers x 2 fewer)."""
    sa2, ca = golden_shapes("unet_small_gatedsa2"), golden_shapes("unet_small_gatedca")
    assert sorted(sa2) == sorted(golden_shapes("unet_small_text"))
    assert len(trainable_names(sa2)) == 127 and len(trainable_names(ca)) == 113
    assert not [k for k in ca if ".fuser.linear." in k] and sum(".fuser.linear." in k for k in trainable_names(sa2)) == 14
    k = "input_blocks.1.1.transformer_blocks.0.fuser.attn.to_k.weight"
    assert list(sa2[k]) == [320, 320] and list(ca[k]) == [320, 768]


# ---- the goldens against autograd through the oracle
def block_state_dict(meta):
    from ldm.modules.attention import BasicTransformerBlock
    blk = BasicTransformerBlock(meta["C"], meta["ctx_dim"], meta["ctx_dim"], meta["heads"], meta["C"] // meta["heads"], meta["fuser_type"])
    sd = syn.seeded_state_dict({k: tuple(v.shape) for k, v in blk.state_dict().items()}, meta["seed"])
    sd["fuser.alpha_attn"] = torch.tensor(meta["alpha_attn"])
    sd["fuser.alpha_dense"] = torch.tensor(meta["alpha_dense"])
    return sd


def block_case(fuser_type):
    """(golden, meta, state_dict, (x, objs, context, target)) of a block golden; the inputs are block_backward_gatedsa's draws."""
    g, meta = _npz(BLOCK_CASES[fuser_type])
    assert meta["fuser_type"] == fuser_type
    inputs = block_backward_inputs(meta)
    assert abs(float(inputs[0].double().sum()) - float(g["x_sum"])) < 1e-6 and abs(float(inputs[3].double().sum()) - float(g["target_sum"])) < 1e-6
    return g, meta, block_state_dict(meta), inputs


def block_oracle_autograd(meta, sd, inputs):
    """y, loss, dx, dobjs and every fuser.* gradient in full, by autograd through the CPU oracle's transformer_block."""
    from oracle import gligen_oracle as orc
    x, objs, context, target = (t.clone() for t in inputs)
    x.requires_grad_(True)
    objs.requires_grad_(True)
    sdo = {"b." + k: v.detach().float().clone() for k, v in sd.items()}
    names = [k for k in sd if k.startswith("fuser.")]
    for k in names:
        sdo["b." + k].requires_grad_(True)
    y = orc.transformer_block(sdo, "b", x, context, objs, meta["heads"], 1.0, meta["fuser_type"])
    loss = torch.nn.functional.mse_loss(y, target)
    loss.backward()
    return y.detach(), loss.detach(), x.grad, objs.grad, {k: sdo["b." + k].grad for k in names}


def block_report(g, meta, y, loss, dx, dobjs, grads):
    """rel-MSE per stored tensor of a block golden (y and dx on every stride_rows-th token row, the gradients on their strided
    samples), the loss' relative error, and the gradients' norm ratios."""
    st, n = meta["stride_rows"], meta["sample"]
    report = {"y": rel_mse(y[:, ::st], g["y"]), "loss": abs(float(loss) - float(g["loss"])) / float(g["loss"]), "dx": rel_mse(dx[:, ::st], g["dx"]),
              "dobjs": rel_mse(dobjs, g["dobjs"])}
    names = sorted(k[5:] for k in g.files if k.startswith("grad."))
    assert names == sorted(grads.keys()) and len(names) == (15 if meta["fuser_type"] == "gatedCA" else 17)
    norms = {}
    for k in names:
        flat = grads[k].detach().float().cpu().reshape(-1)
        stride = max(1, flat.numel() // n)
        sub = flat[::stride][:n] if flat.numel() > n else flat
        report["grad." + k] = rel_mse(sub, torch.from_numpy(g["grad." + k].astype(np.float32)) * float(g["scale." + k]))
        norms[k] = float(flat.double().norm()) / max(float(g["norm." + k]), 1e-30)
    return report, norms


@pytest.mark.parametrize("fuser_type", sorted(BLOCK_CASES))
def test_block_golden_vs_oracle_autograd(fuser_type):
    g, meta, sd, inputs = block_case(fuser_type)
    report, norms = block_report(g, meta, *block_oracle_autograd(meta, sd, inputs))
    worst = max(report, key=report.get)
    print(fuser_type, "block: oracle autograd vs reference: worst", worst, report[worst])
    assert not {k: v for k, v in report.items() if v >= 1e-5}
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), {k: v for k, v in norms.items() if abs(v - 1) >= 1e-3}


def text_batch(meta):
    """The inputs of tools/make_golden_train_fusers.py:unet_text_case, rebuilt from the same seeds: (dataset batch, step batch)."""
    B, hw = meta["B"], meta["hw"]
    b = syn.make_batch("text", B, n_valid=meta["n_valid"], seed=5, max_objs=meta["max_objs"])
    batch = dict(x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441][:B]).float(), context=syn.make_context(B, seed=6),
                 boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"], target=syn.make_latent(B, 4, hw, hw, seed=7))
    return b, batch


def unet_oracle_autograd(case, meta, sd, trainable):
    """loss, eps and the full gradient of every `trainable` tensor of a UNet golden's step by autograd through the CPU oracle."""
    if case == "canny_gatedsa2":
        return spatial_oracle_autograd(sd, meta, trainable, spatial_batch(meta))
    from oracle import gligen_oracle as orc
    b, batch = text_batch(meta)
    sdo = {k: v.detach().float().cpu().clone() for k, v in sd.items()}
    for k in trainable:
        sdo[k].requires_grad_(True)
    eps = orc.unet_forward(sdo, oracle_cfg(meta["cfg"], "text"), dict(x=batch["x"], timesteps=batch["timesteps"].long(), context=batch["context"],
                                                                       grounding_input=grounding_kwargs("text", b)))
    loss = torch.nn.functional.mse_loss(eps, batch["target"])
    loss.backward()
    return loss.detach(), eps.detach(), {k: sdo[k].grad for k in trainable}


@pytest.mark.parametrize("case", sorted(UNET_CASES))
def test_unet_golden_vs_oracle_autograd(case):
    """Autograd through the CPU oracle (oracle/gligen_oracle.py with fuser_type) reproduces the reference's loss.backward(): loss, eps,
    every sampled gradient and every norm, at the bars of the other training goldens."""
    g = load_golden(UNET_CASES[case])
    meta = g["meta"]
    sd = syn.seeded_state_dict(golden_shapes(UNET_SHAPES[case]), meta["weight_seed"])
    names = trainable_names(sd, meta["cfg"])
    assert len(names) == meta["n_trainable"] == N_TRAINABLE[case]
    assert sorted(names) == sorted(k[5:] for k in g if k.startswith("grad."))
    loss, eps, grads = unet_oracle_autograd(case, meta, sd, names)
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < 1e-5
    assert rel_mse(eps, g["eps"]) < 1e-5
    report, norms = golden_report(g, grads)
    worst = max(report, key=report.get)
    print(case, "oracle autograd vs reference: worst", worst, report[worst])
    assert not {k: v for k, v in report.items() if v >= 1e-5}
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), {k: v for k, v in norms.items() if abs(v - 1) >= 1e-3}
