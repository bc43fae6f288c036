"""Training LoRA adapters, host side, no GPU: the float64 restatement of the adapted Linear (tests/lora_train_ref.py) against autograd
through the merged weight, init_adapters and the kohya form of an adapter against gligen_amd.lora's own parser and planner, the bucket
order and milestones of the adapter tensors, the ISA of csrc/train_lora.hip, and the entry points of
include/gligen_amd_train_lora.h (declared, exported, bound)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import lora_ref
import lora_train_ref as R
from helpers import ROOT, golden_shapes
from gligen_amd import lora, lora_train as lt, synthetic as syn

CONFIGS = {"unet_small_text": (syn.UNET_CFG_SMALL, 7), "unet_full_text": (syn.UNET_CFG, 16)}      # (config, SpatialTransformers)
PER_ST = {"attn": 8, "ff": 2, "proj": 2}


@pytest.mark.parametrize("M,K,N,r", [(5, 64, 128, 1), (77, 128, 64, 4), (33, 64, 64, 24)])
def test_restatement_is_autograd_through_the_merged_weight(M, K, N, r):
    """adapted_linear_ref (the formulas the kernels implement) equals autograd through W + s up down with the chain rule
    g_up = s dW down^T, g_down = s up^T dW, in float64 to 1e-12."""
    g = torch.Generator().manual_seed(M)
    x, dy, W = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g), torch.randn(N, K, generator=g)
    down, up = torch.randn(r, K, generator=g), torch.randn(N, r, generator=g)
    ref, auto = R.adapted_linear_ref(x, W, down, up, 1.75, dy), R.adapted_linear_autograd(x, W, down, up, 1.75, dy)
    for n in ("y", "dx", "g_down", "g_up"):
        assert ref[n].dtype == torch.float64 and ref[n].shape == auto[n].shape
        assert float((ref[n] - auto[n]).abs().max()) <= 1e-12 * max(1.0, float(auto[n].abs().max())), n
    dW = dy.double().T @ x.double()
    gd, gu = R.chain_rule(dW.reshape(N, K, 1, 1), down, up, 1.75)
    assert torch.allclose(gd, ref["g_down"], rtol=1e-12, atol=1e-12) and torch.allclose(gu, ref["g_up"], rtol=1e-12, atol=1e-12)


def test_case_lists_and_chunk_formula():
    """The cases the issue sets, and the restated row-chunk formula against the library's host function."""
    assert R.M_PLAIN == [1, 63, 154, 272] and R.M_CHUNK == [255, 256, 257, 529]
    assert R.KN == [(64, 64), (320, 320), (768, 320), (320, 2560), (1280, 320)] and R.RANKS == [1, 4, 24, 128]
    cases = [c for i in range(len(R.KN)) for c in R.kernel_cases(i)]
    assert len(cases) == 40 and {c[0] for c in cases} == set(R.M_ALL) and {(c[1], c[2]) for c in cases} == set(R.KN)
    for M in R.M_ALL:
        assert {c[3] for c in cases if c[0] == M} == set(R.RANKS) and {c[4:] for c in cases if c[0] == M} == set(R.ORIENTATIONS), M
    assert len(set(R.cross_cases())) == 16
    assert [R.wgrad_chunk_rows(m) for m in (1, 8192, 8193, 16384, 16385)] == [256, 256, 320, 512, 576]
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    lib = _lib.load()
    assert all(lib.gl_lora_wgrad_chunk_rows(m) == R.wgrad_chunk_rows(m) for m in list(range(1, 600)) + [8192, 8193, 16384, 16385, 1 << 20])
    x, dy, down, up, y0, dx0 = R.integer_case(154, 320, 320, 24)
    assert not torch.equal(down[:, :24], down[:, :24].T) and all(bool((t == t.round()).all()) for t in (x, dy, down, up, y0, dx0))


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("families", [("attn",), ("ff",), ("proj",), ("attn", "ff", "proj")], ids=lambda f: "+".join(f))
def test_init_adapters_names_and_shapes(name, families):
    """One down [r, K] / up [N, r] pair per Linear of the chosen families in every SpatialTransformer, none on a fuser; up == 0, down
    Kaiming-uniform (within 1 / sqrt(K), not degenerate); the same seed gives the same tensors, a site's start does not depend on
    the other families."""
    shapes = golden_shapes(name)
    sd = {k: torch.empty(v, device="meta") for k, v in shapes.items()}
    n_st = CONFIGS[name][1]
    spec = lt.LoraSpec(4, families=families)
    assert spec.alpha == 4.0 and spec.scale == 1.0
    sites = lt.adapter_sites(sd, spec)
    assert len(sites) == n_st * sum(PER_ST[f] for f in families) and len(lt.st_prefixes(sd)) == n_st
    assert not [k for k in sites if ".fuser." in k] and all(k in shapes for k in sites)
    a = lt.init_adapters(sd, CONFIGS[name][0], spec, seed=1)
    assert list(a) == [w[:-7] + s for w in sites for s in (lt.DOWN, lt.UP)]
    for w in sites:
        N, K = shapes[w][:2]
        down, up = a[w[:-7] + lt.DOWN], a[w[:-7] + lt.UP]
        assert tuple(down.shape) == (4, K) and tuple(up.shape) == (N, 4) and down.dtype == up.dtype == torch.float32
        assert int(torch.count_nonzero(up)) == 0
        assert float(down.abs().max()) <= K ** -0.5 and float(down.abs().max()) > 0.8 * K ** -0.5 and abs(float(down.mean())) < 0.2 * K ** -0.5
    b = lt.init_adapters(sd, None, spec, seed=1)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = lt.init_adapters(sd, None, lt.LoraSpec(4, families=families[:1]), seed=1)
    assert all(torch.equal(a[k], c[k]) for k in c)
    d = lt.init_adapters(sd, None, spec, seed=2)
    assert not any(torch.equal(a[k], d[k]) for k in a if k.endswith(lt.DOWN))


def test_spec_refusals():
    for bad in (0, 129, -1):
        with pytest.raises(ValueError, match="rank"):
            lt.LoraSpec(bad)
    with pytest.raises(ValueError, match="families"):
        lt.LoraSpec(4, families=("attn", "conv"))
    assert lt.LoraSpec(16, 8).scale == 0.5 and set(lt.FAMILY_SUFFIXES) == {"attn", "ff", "proj"} <= set(syn.LORA_FAMILIES)
    shapes = golden_shapes("unet_small_text")
    for fam, suffixes in lt.FAMILY_SUFFIXES.items():         # the same modules the synthetic adapters' families name
        sites = lt.adapter_sites(shapes_as_meta(shapes), lt.LoraSpec(4, families=(fam,)))
        want = [k for k in shapes if k.endswith(".weight") and syn.LORA_FAMILIES[fam](k[:-7])]
        assert sorted(sites) == sorted(want), fam


def shapes_as_meta(shapes):
    return {k: torch.empty(v, device="meta") for k, v in shapes.items()}


def test_kohya_form_resolves_on_the_product_model():
    """adapter_state_dict's form (kohya_state_dict) on the small product model: parse_adapter finds one pair per site with the alpha
    stored, plan_loras resolves every name (nothing unresolved, nothing skipped, every shape fits), conv factors are 4-D with 1 x 1
    tails, and the planned merge -- the planner's own weight, factors and scale -- is W + s up down within lora_ref's bound of the
    merge (the merge itself runs on the device: test_lora_train_gpu.py)."""
    from helpers import build_product_unet
    model = build_product_unet(syn.UNET_CFG_SMALL, "text")
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    spec = lt.LoraSpec(4, 2.0, ("attn", "ff", "proj"))
    g = torch.Generator().manual_seed(5)
    tensors = {k: torch.randn(v.shape, generator=g) * 0.05 for k, v in lt.init_adapters(sd, syn.UNET_CFG_SMALL, spec, 0).items()}
    for dtype in (torch.float32, torch.float16):
        ko = lt.kohya_state_dict(tensors, sd, spec.alpha, dtype)
        assert len(ko) == 3 * 84 and all(v.dtype == dtype for v in ko.values())
        assert all(k.startswith("lora_unet_") and "." not in k.split(".lora_")[0].split(".alpha")[0] for k in ko)
        entries = lora.parse_adapter(ko)
        assert len(entries) == 84 and all(e.alpha == 2.0 and e.rank == 4 and e.factor == 0.5 for e in entries)
        conv = [e for e in entries if "_proj_in" in e.name or "_proj_out" in e.name]
        assert len(conv) == 14 and all(e.down.dim() == 4 and tuple(e.down.shape[2:]) == (1, 1) and tuple(e.up.shape[2:]) == (1, 1) for e in conv)
        assert all(e.down.dim() == 2 for e in entries if e not in conv)
        (plan,) = lora.plan_loras(model, None, [(ko, 1.0)])
        assert len(plan.merges) == 84 and not plan.skipped
    worst = 0.0
    for _, key, weight, e, scale in plan.merges:          # (fp16 factors: the merge of what the file holds)
        path = key[:-len(".weight")]
        assert scale == spec.scale and torch.equal(e.down.reshape(4, -1).float(), tensors[path + lt.DOWN].half().float())
        N = weight.shape[0]
        got = (weight.detach().double() + scale * (e.up.double().reshape(N, 4) @ e.down.double().reshape(4, -1)).reshape(weight.shape)).float()
        want = lora_ref.merge64(sd[key], e.up, e.down, spec.scale)
        err = (got.double() - want).abs()
        bound = lora_ref.merge_bound(sd[key], e.up, e.down, spec.scale)
        assert bool((err <= bound).all()), key
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print("planned merges against W + s up down: worst error / bound", worst)


def test_bucket_order_and_milestones_follow_the_blocks():
    """An adapter tensor's milestone is the number of its SpatialTransformer in module order (output_blocks.10 after output_blocks.3),
    the same number its block's fuser tensors have in train.gradient_milestones; position_net's is the number of blocks; sorted as
    LoraTrainStep sorts them, the last block's tensors come first."""
    from gligen_amd.train import gradient_milestones, trainable_names
    shapes = golden_shapes("unet_full_text")
    spec = lt.LoraSpec(4, families=("attn", "ff", "proj"))
    names = list(lt.init_adapters(shapes_as_meta(shapes), None, spec, 0))
    base = trainable_names(shapes, syn.UNET_CFG)
    ms = lt.adapter_milestones(base + names, shapes)
    fuser = gradient_milestones(base)
    assert all(ms[k] == fuser[k] for k in base) and max(ms.values()) == 16
    sts = lt.st_prefixes(shapes)
    assert len(sts) == 16 and sts.index("input_blocks.2.1") < sts.index("input_blocks.8.1") < sts.index("middle_block.1") < sts.index("output_blocks.3.1") \
        < sts.index("output_blocks.10.1")
    for k in names:
        st = k.split(".transformer_blocks.")[0] if ".transformer_blocks." in k else k.rsplit(".", 3)[0]
        assert ms[k] == sts.index(st), k
    order = sorted(base + names, key=lambda k: (ms[k] == 16, -ms[k]))
    assert [ms[k] for k in order] == sorted((ms[k] for k in order), key=lambda m: (m == 16, -m))
    assert order[0].startswith("output_blocks.11.1.") and order[-1].startswith("position_net.")
    shuffled = dict(sorted(shapes.items()))           # a re-sorted state_dict gives the same numbering
    assert lt.adapter_milestones(names, shuffled) == {k: ms[k] for k in names}


# ---- the kernels' ISA
def test_train_lora_unit_isa(tmp_path):
    """train_lora.hip for gfx950, device only: every kernel has private_segment_fixed_size 0 and spills nothing, each of the three
    product kernels contains an f32-input MFMA and the reduce none, nothing is an atomic, and the unit is in the build."""
    from gligen_amd.build import SOURCES
    assert "train_lora.hip" in SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "train_lora.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--offload-device-only", "-S",
                        os.path.join(ROOT, "gligen_amd", "csrc", "train_lora.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", asm)
    families = {f: [k for k in kernels if f in k] for f in ("lora_down_kernel", "lora_up_kernel", "lora_wgrad_kernel", "lora_wgrad_reduce_kernel")}
    assert sum(len(v) for v in families.values()) == len(kernels) == 4 + 6 + 4 + 1, kernels
    for name in kernels:
        blk = asm[asm.index(".amdhsa_kernel " + name):]
        blk = blk[:blk.index(".end_amdhsa_kernel")]
        assert int(re.search(r"private_segment_fixed_size (\d+)", blk).group(1)) == 0, name
        meta = asm[asm.index(".name:           " + name):]
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0 and int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1)) == 0, name
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index("s_endpgm")]
        n_mfma = len(re.findall(r"v_mfma_f32_16x16x4_f32", body))
        assert (n_mfma == 0) if "reduce" in name else (n_mfma >= 2), (name, n_mfma)
        assert "atomic" not in body, name


# ---- the C ABI
def _declared(header):
    return set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_train_lora_entry_points_are_declared_exported_and_bound(tmp_path):
    """include/gligen_amd_train_lora.h declares exactly the names of TRAIN_LORA_SYMBOLS, the built library exports them with the
    table's argument types and counts, the table shares no name with another table or header, gl_lora_adapter has the size of its
    ctypes mirror, and the header compiles as C99."""
    from gligen_amd import _lib as table
    from gligen_amd.build import build_native
    build_native()
    lib = table.load()
    declared = _declared("gligen_amd_train_lora.h")
    assert declared == set(table.TRAIN_LORA_SYMBOLS) == {"gl_unet_train_step_lora", "gl_op_lora_linear", "gl_lora_wgrad_chunk_rows"}
    raw = ctypes.CDLL(str(table.LIB_PATH))
    text = open(os.path.join(ROOT, "include", "gligen_amd_train_lora.h")).read()
    for name, (res, args) in table.TRAIN_LORA_SYMBOLS.items():
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text).group(1)
        assert len(proto.split(",")) == len(args), name
    others = (table.SYMBOLS, table.TRAIN_PRIM_SYMBOLS, table.TRAINER_SYMBOLS, table.LORA_SYMBOLS, table.TRAIN_INPUT_SYMBOLS, table.TRAIN_FUSER_SYMBOLS)
    assert not declared & set().union(*others)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "gligen_amd_train_lora.h":
            assert not declared & set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read())), other
    src = tmp_path / "h.c"
    src.write_text('#include <stdio.h>\n#include "gligen_amd_train_lora.h"\nint main(void) { printf("%zu\\n", sizeof(gl_lora_adapter)); return 0; }\n')
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "h")], check=True)
    assert int(subprocess.run([str(tmp_path / "h")], capture_output=True, text=True, check=True).stdout) == ctypes.sizeof(table.LoraAdapter)
    capi = open(os.path.join(ROOT, "gligen_amd", "csrc", "capi.hip")).read()
    assert '#include "train_impl.h"' not in capi


def test_trainer_options_and_engine_signature():
    """The four trainer options parse, and Engine.unet_train_step / op_lora_linear / TrainStep keep their signatures."""
    import inspect
    from gligen_amd import trainer
    from gligen_amd.engine import Engine
    from gligen_amd.train import TrainStep
    src = inspect.getsource(trainer.main)
    assert all(f'"--{o}"' in src for o in ("lora_rank", "lora_alpha", "lora_families", "lora_out"))
    p = inspect.signature(Engine.unet_train_step).parameters
    assert list(p)[-1] == "adapters" and p["adapters"].default is None
    assert hasattr(Engine, "op_lora_linear") and issubclass(lt.LoraTrainStep, TrainStep)
    assert inspect.signature(lt.LoraTrainStep.__init__).parameters["train_base"].default is False
