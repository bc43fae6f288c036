"""LoRA adapters on 3 x 3 convs, host side, no GPU: the two float64 references of tests/lora_conv_ref.py against each other and
autograd, the mutation table of the gather form against the bounds the GPU tests use, the names, shapes and seeds of the conv
families (LoraSpec's conv_families, init_adapters, kohya_state_dict against gligen_amd.lora's own name table and parser), the ISA of
csrc/train_lora_conv.hip, and the entry point of include/gligen_amd_train_lora_conv.h (declared, exported, bound)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import lora_conv_ref as R
from helpers import ROOT, golden_shapes
from gligen_amd import lora, lora_train as lt, synthetic as syn

REF_CASES = [(0, 2, 1, 1, 64, 64, 4), (0, 2, 3, 5, 64, 128, 4), (0, 1, 5, 13, 128, 64, 24), (1, 2, 2, 2, 64, 64, 4), (1, 2, 6, 4, 64, 64, 1),
             (2, 2, 1, 1, 64, 64, 4), (2, 2, 3, 2, 128, 64, 4)]


@pytest.mark.parametrize("c", REF_CASES, ids=R.case_id)
def test_references_agree_with_autograd(c):
    """gather_ref (written out over the gather table: the formulas the kernels implement) equals conv_ref (F.conv2d on the NCHW
    permutation, geometry 2 after repeat_interleave x2, dx / g_down / g_up by torch.autograd) in float64 to 1e-12, for t, y, u, dx,
    g_down and g_up of all three geometries."""
    x, dy, down, up, y0, dx0 = R.gaussian_case(c)
    a, b = R.gather_ref(c, x, down, up, 1.75, dy, y0, dx0), R.conv_ref(c, x, down, up, 1.75, dy, y0, dx0)
    for n in R.NAMES:
        assert a[n].dtype == torch.float64 and a[n].shape == b[n].shape, n
        assert float((a[n] - b[n]).abs().max()) <= 1e-12 * max(1.0, float(b[n].abs().max())), n
    geom, B, H, W, Ci, Co, r = c
    if geom == 2:       # the issue's formula for the Upsample read
        idx = R.gather_table(geom, B, H, W)
        for m in range(idx.shape[0]):
            b_, oy, ox = m // (4 * H * W), (m // (2 * W)) % (2 * H), m % (2 * W)
            for tap in range(9):
                uy, ux = oy + tap // 3 - 1, ox + tap % 3 - 1
                want = (b_ * H + (uy >> 1)) * W + (ux >> 1) if (0 <= uy < 2 * H and 0 <= ux < 2 * W) else -1
                assert int(idx[m, tap]) == want


def test_case_lists_and_integer_inputs():
    """The cases the issue sets, and the exact-integer inputs: nine different taps, no (ky, kx) symmetry, every term sum below 2^24."""
    assert R.SHAPES[0] == [(1, 1), (2, 2), (3, 5), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (16, 17)]
    assert R.SHAPES[1] == [(2, 2), (6, 4), (16, 34)] and R.SHAPES[2] == [(1, 1), (3, 2), (8, 9)]
    assert [2 * h * w for h, w in R.SHAPES[0][3:6]] == [126, 128, 130] and [2 * h * w for h, w in R.SHAPES[0][6:]] == [510, 512, 544]
    assert (0, 1, 16, 17, 64, 64, 4) in R.shape_cases(0) and all(c[1] == 2 for c in R.shape_cases(1) + R.shape_cases(2))
    assert {(c[4], c[5]) for c in R.channel_cases()} == set(R.CHANNELS) == {(64, 64), (128, 64), (320, 320), (640, 320)}
    assert {(c[2], c[3]) for c in R.channel_cases()} == {(3, 5), (16, 17)}
    assert {(c[2], c[3], c[6]) for c in R.rank_cases() if c[0] == 0} == {(h, w, r) for h, w in R.SWEEP_IMAGES for r in (1, 4, 24, 128)}
    assert {c[0] for c in R.exact_cases()} == {0, 1, 2}
    for c in R.exact_cases():
        x, dy, down, up, y0, dx0 = R.integer_case(c)
        full = R.gather_ref(c, x, down, up, 0.5, dy, y0, dx0)
        assert all(bool((t == t.round()).all()) for t in (x, dy, down, up, y0, dx0))
        assert all(float(full["abs_" + n].max()) < 2 ** 24 for n in R.NAMES), c


# the mutations on a set of small cases; (mutation, case id, tensor) where the mutation provably changes nothing, so the mutated tensor
# has to be bit-equal: on a 1 x 1 image under stride 1 every tap but the centre reads padding, the flip keeps the centre where it is and
# so does exchanging ky and kx -- t, dx and g_down (zero off the centre tap) are what they were
MUTATION_CASES = [(0, 2, 1, 1, 64, 64, 4), (0, 2, 3, 5, 64, 64, 4), (1, 2, 2, 2, 64, 64, 4), (1, 2, 6, 4, 64, 64, 4), (2, 2, 1, 1, 64, 64, 4), (2, 2, 3, 2, 64, 64, 4)]
UNCHANGED = {("taps_flipped", "conv-B2-1x1-Ci64-Co64-r4", n) for n in ("t", "dx", "g_down")} | {("g_down_kykx", "conv-B2-1x1-Ci64-Co64-r4", "g_down")}


def test_mutations_exceed_the_bounds():
    """What the bounds of the GPU tests see, computed here on the CPU: each way of getting an adapted conv subtly wrong pushes every
    tensor it reaches over that tensor's elementwise bound by a factor of at least 16 on at least one case; the triples of UNCHANGED
    are bit-equal to the unmutated reference. Prints mutation, case, tensor, worst |difference| / bound."""
    best, seen = {}, set()
    for c in MUTATION_CASES:
        x, dy, down, up, y0, dx0 = R.gaussian_case(c)
        ref = R.gather_ref(c, x, down, up, 0.75, dy, y0, dx0)
        bound = R.bounds(c, ref)
        cid = R.case_id(c)
        for mut, (geoms, names) in R.MUTATIONS.items():
            if c[0] not in geoms:
                continue
            bad = R.gather_ref(c, x, down, up, 0.75, dy, y0, dx0, mut=mut)
            for n in names:
                ratio = float(((bad[n] - ref[n]).abs() / bound[n].clamp_min(1e-300)).max())
                print(f"[lora_conv mutations] {mut:22s} {cid:28s} {n:7s} x{ratio:.3g}")
                if (mut, cid, n) in UNCHANGED:
                    seen.add((mut, cid, n))
                    assert torch.equal(bad[n], ref[n]), (mut, cid, n)
                best[(mut, n)] = max(best.get((mut, n), 0.0), ratio)
    assert seen == UNCHANGED
    assert set(best) == {(m, n) for m, (_, names) in R.MUTATIONS.items() for n in names}
    weak = {k: v for k, v in best.items() if not v >= 16.0}
    assert not weak, weak


# ---- names, shapes, seeds
PER_FAMILY = {"conv": 21, "emb": 8, "sample": 2}        # unet_small_text: 8 ResBlocks (5 with a skip_connection), 1 Downsample, 1 Upsample


def shapes_as_meta(shapes):
    return {k: torch.empty(v, device="meta") for k, v in shapes.items()}


def test_conv_family_sites_names_and_shapes():
    """Every site of conv / emb / sample on the small product model's shapes is the module synthetic.LORA_FAMILIES names; 3 x 3 sites
    get down [conv_rank, Ci, 3, 3] (Kaiming-uniform with fan-in 9 Ci) and up [Co, conv_rank], skip_connection and emb_layers.1 get
    [rank, K] / [N, rank]; up is zero; a site's start does not depend on the other families; after kohya_state_dict every name
    resolves through lora.unet_name_table back to the same module, 3 x 3 downs are 4-D as they are, ups and 1 x 1 downs carry (1, 1)
    tails, and .alpha is the right one of the two alphas."""
    shapes = golden_shapes("unet_small_text")
    sd = shapes_as_meta(shapes)
    everything = lt.LoraSpec(4, 2.0, ("attn", "ff", "proj"), conv_families=("conv", "emb", "sample"), conv_rank=8, conv_alpha=2.0)
    full = lt.init_adapters(sd, None, everything, seed=1)
    for fam, n in PER_FAMILY.items():
        spec = lt.LoraSpec(4, 2.0, (), conv_families=(fam,), conv_rank=8, conv_alpha=2.0)
        sites = lt.adapter_sites(sd, spec)
        want = [k for k in shapes if k.endswith(".weight") and syn.LORA_FAMILIES[fam](k[:-7])]
        assert sorted(sites) == sorted(want) and len(sites) == n, fam
        a = lt.init_adapters(sd, None, spec, seed=1)
        assert list(a) == [w[:-7] + s for w in sites for s in (lt.DOWN, lt.UP)]
        for w in sites:
            down, up = a[w[:-7] + lt.DOWN], a[w[:-7] + lt.UP]
            Co, Ci = shapes[w][:2]
            if len(shapes[w]) == 4 and tuple(shapes[w][2:]) == (3, 3):
                assert tuple(down.shape) == (8, Ci, 3, 3) and tuple(up.shape) == (Co, 8) and spec.of_site(sd[w]) == (8, 2.0)
                lim = (9 * Ci) ** -0.5
            else:
                assert tuple(down.shape) == (4, Ci) and tuple(up.shape) == (Co, 4) and spec.of_site(sd[w]) == (4, 2.0)
                lim = Ci ** -0.5
            assert int(torch.count_nonzero(up)) == 0 and lim >= float(down.abs().max()) > 0.8 * lim and abs(float(down.mean())) < 0.2 * lim
            assert torch.equal(down, full[w[:-7] + lt.DOWN]), "a site's start does not depend on the other families"
        assert not any(torch.equal(a[k], v) for k, v in lt.init_adapters(sd, None, spec, seed=2).items() if k.endswith(lt.DOWN))
    assert len(full) == 2 * (7 * 12 + 31)
    from helpers import build_product_unet
    model = build_product_unet(syn.UNET_CFG_SMALL, "text")
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    table = lora.unet_name_table(model)
    g = torch.Generator().manual_seed(5)
    tensors = {k: torch.randn(v.shape, generator=g) * 0.05 for k, v in full.items()}
    ko = lt.kohya_state_dict(tensors, sd, everything.alpha, torch.float32, conv_alpha=0.5)
    assert len(ko) == 3 * (7 * 12 + 31)
    for k in lt.adapter_sites(sd, everything):
        path = k[:-7]
        name = lora.UNET_PREFIX + path.replace(".", "_")
        assert table[name] == path
        down, up, alpha = ko[name + lt.DOWN], ko[name + lt.UP], float(ko[name + ".alpha"])
        if len(shapes[k]) == 4 and tuple(shapes[k][2:]) == (3, 3):
            assert tuple(down.shape) == (8, shapes[k][1], 3, 3) and tuple(up.shape) == (shapes[k][0], 8, 1, 1) and alpha == 0.5
            assert torch.equal(down, tensors[path + lt.DOWN])
        elif len(shapes[k]) == 4:
            assert tuple(down.shape) == (4, shapes[k][1], 1, 1) and tuple(up.shape) == (shapes[k][0], 4, 1, 1) and alpha == 2.0
        else:
            assert tuple(down.shape) == (4, shapes[k][1]) and tuple(up.shape) == (shapes[k][0], 4) and alpha == 2.0
    entries = lora.parse_adapter(ko)
    assert len(entries) == 7 * 12 + 31 and {e.rank for e in entries} == {4, 8}
    (plan,) = lora.plan_loras(model, None, [(ko, 1.0)])
    assert sorted(key for _, key, *_ in plan.merges) == sorted(lt.adapter_sites(sd, everything)) and not plan.skipped
    assert all(scale == (0.5 / 8 if e.rank == 8 else 2.0 / 4) for *_, e, scale in plan.merges)
    ms = lt.adapter_milestones(list(full), shapes)
    assert max(ms.values()) == 7 and all(ms[k] == 7 for k in full if ".transformer_blocks." not in k and ".proj_" not in k)


def test_conv_spec_refusals_and_pins():
    """A bad conv_rank, an unknown conv_families word, channels that are no multiple of 64; the two pins of the Linear families hold."""
    for bad in (0, 129, -1):
        with pytest.raises(ValueError, match="conv_rank"):
            lt.LoraSpec(4, conv_families=("conv",), conv_rank=bad)
    with pytest.raises(ValueError, match="conv_families"):
        lt.LoraSpec(4, conv_families=("conv", "attn"))
    with pytest.raises(ValueError, match="families"):
        lt.LoraSpec(4, families=())
    with pytest.raises(ValueError, match="multiples of 64"):
        lt.init_adapters({"input_blocks.1.0.in_layers.2.weight": torch.empty(96, 64, 3, 3, device="meta")}, None, lt.LoraSpec(4, families=(), conv_families=("conv",)))
    with pytest.raises(ValueError, match="families"):
        lt.LoraSpec(4, families=("attn", "conv"))
    assert set(lt.FAMILY_SUFFIXES) == {"attn", "ff", "proj"} and set(lt.CONV_FAMILY_SUFFIXES) == {"conv", "emb", "sample"} <= set(syn.LORA_FAMILIES)
    s = lt.LoraSpec(16, 8, conv_families=("conv",))
    assert (s.conv_rank, s.conv_alpha, s.conv_scale, s.scale) == (16, 16.0, 1.0, 0.5)
    s = lt.LoraSpec(16, 8, conv_families=("conv",), conv_rank=4)
    assert (s.conv_rank, s.conv_alpha) == (4, 4.0) and lt.LoraSpec(4).conv_families == ()


def test_trainer_options_parse():
    import inspect
    from gligen_amd import trainer
    from gligen_amd.engine import Engine
    src = inspect.getsource(trainer.main)
    assert all(f'"--{o}"' in src for o in ("lora_conv_families", "lora_conv_rank", "lora_conv_alpha"))
    p = inspect.signature(Engine.op_lora_conv3).parameters
    assert list(p)[1:4] == ["x", "down", "up"] and p["geom"].default == 0


# ---- the kernels' ISA
def test_train_lora_conv_unit_isa(tmp_path):
    """train_lora_conv.hip for gfx950, device only: every kernel has private_segment_fixed_size 0 and spills nothing, each of the three
    product kernels contains an f32-input MFMA, the reduce and the per-sample column sum none, nothing is an atomic, and the unit is
    in the build."""
    from gligen_amd.build import SOURCES
    assert "train_lora_conv.hip" in SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "train_lora_conv.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--offload-device-only", "-S",
                        os.path.join(ROOT, "gligen_amd", "csrc", "train_lora_conv.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", asm)
    families = {f: [k for k in kernels if f in k] for f in ("lora_conv_down_kernel", "lora_conv_dgrad_kernel", "lora_conv_wgrad_kernel",
                                                            "lora_conv_wgrad_reduce_kernel", "lora_sample_colsum_kernel")}
    assert sum(len(v) for v in families.values()) == len(kernels) == 4 + 6 + 4 + 1 + 1, kernels
    for name in kernels:
        blk = asm[asm.index(".amdhsa_kernel " + name):]
        blk = blk[:blk.index(".end_amdhsa_kernel")]
        assert int(re.search(r"private_segment_fixed_size (\d+)", blk).group(1)) == 0, name
        meta = asm[asm.index(".name:           " + name):]
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0 and int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1)) == 0, name
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index("s_endpgm")]
        n_mfma = len(re.findall(r"v_mfma_f32_16x16x4_f32", body))
        assert (n_mfma == 0) if ("reduce" in name or "colsum" in name) else (n_mfma >= 2), (name, n_mfma)
        assert "atomic" not in body, name


# ---- the C ABI
def test_train_lora_conv_entry_point_is_declared_exported_and_bound(tmp_path):
    """include/gligen_amd_train_lora_conv.h declares exactly the names of TRAIN_LORA_CONV_SYMBOLS, the built library exports them with
    the table's argument types and counts, no other table or header has them, and the header compiles as C99."""
    from gligen_amd import _lib as table
    from gligen_amd.build import build_native
    build_native()
    lib = table.load()
    header = "gligen_amd_train_lora_conv.h"
    text = open(os.path.join(ROOT, "include", header)).read()
    declared = set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", text))
    assert declared == set(table.TRAIN_LORA_CONV_SYMBOLS) == {"gl_op_lora_conv3"}
    raw = ctypes.CDLL(str(table.LIB_PATH))
    for name, (res, args) in table.TRAIN_LORA_CONV_SYMBOLS.items():
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text).group(1)
        assert len(proto.split(",")) == len(args) == 20, name
    others = {k: v for k, v in vars(table).items() if k.endswith("SYMBOLS") and k != "TRAIN_LORA_CONV_SYMBOLS" and isinstance(v, dict)}
    assert len(others) >= 19 and not declared & set().union(*others.values())
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != header:
            assert not declared & set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read())), other
    src = tmp_path / "h.c"
    src.write_text('#include "gligen_amd_train_lora_conv.h"\nint main(void) { int (*f)(gl_ctx*, int, int, int, int, int, int, float, int, const float*, const float*, const float*, const float*, float*, float*, float*, float*, float*, float*, gl_stream) = gl_op_lora_conv3; return f != gl_op_lora_conv3; }\n')
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "h.o")], check=True)
    capi = open(os.path.join(ROOT, "gligen_amd", "csrc", "capi.hip")).read()
    assert '#include "train_impl.h"' not in capi
