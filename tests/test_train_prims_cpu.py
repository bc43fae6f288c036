"""The training path's primitives, host side, no GPU: the references of tests/train_prims_ref.py held to torch before the kernels
are held to them (test_train_prims_gpu.py) -- the hand-written float64 attention backward against torch.autograd, the split3 and
fp32 flavours against float64, the hand-written GroupNorm against F.group_norm --, the guard-zone helper against a write placed
outside, the summation-chain formulas, and the entry points of include/gligen_amd_train_prims.h (declared, exported, bound)."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import train_prims_ref as R
from helpers import ROOT


def close(a, b, tol):
    """max|a - b| within tol of the larger of 1 and max|b| (gradients that vanish in exact arithmetic are compared absolutely)."""
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("case", [R.AttnCase(40, 70, 75, 2, 2, None), R.AttnCase(160, 33, 31, 2, 2, None), R.AttnCase(32, 1, 1, 1, 3, None)]
                         + R.attention_regime_cases()[:4], ids=R.case_id)
def test_attention_reference_is_autograd(case):
    """attention_ref's hand-written backward (the formulas of train_attention.hip) equals torch.autograd of softmax(q k^T / sqrt(d)) v
    in float64 to 1e-12, regimes included."""
    q, k, v, dout = R.attention_inputs(case)
    ref, auto = R.attention_ref(q, k, v, dout, case.H), R.attention_autograd(q, k, v, dout, case.H)
    assert sorted(ref) == sorted(auto) == ["dk", "dq", "dv", "lse", "o"]
    for n in ref:
        assert ref[n].dtype == torch.float64 and ref[n].shape == auto[n].shape
        assert close(ref[n], auto[n], 1e-12), (n, float((ref[n] - auto[n]).abs().max()))


def test_flavours_stay_near_float64():
    """The split3 and fp32 flavours are within 1e-3 of float64 (the measure of the GPU tests) on every attention and Linear case, so a
    broken emulation cannot loosen a bound unseen; split3 is not fp32 in disguise (its error is above fp32's on the products); the
    gradients that vanish in exact arithmetic are the ones attention_zero_gradients names, and only those."""
    for c in R.attention_cases() + R.attention_regime_cases():
        q, k, v, dout = R.attention_inputs(c)
        ref = R.attention_ref(q, k, v, dout, c.H)
        zeros = R.attention_zero_gradients(c, q, k, dout, ref)
        assert {n: 64 * b for n, b in R.attention_zero_gradients(c, q, k, dout, ref, split=False).items()} == zeros      # 2^-22 against 2^-16
        assert set(zeros) == {n for n in ("dq", "dk") if float(ref[n].abs().max()) < 1e-9}, R.case_id(c)
        for flav in (R.attention_fp32, R.attention_split3):
            got = flav(q, k, v, dout, c.H)
            for n in ref:
                assert got[n].dtype == torch.float32
                if n in zeros:
                    assert float(got[n].abs().max()) <= zeros[n], (R.case_id(c), n)
                else:
                    assert R.rel_max(got[n], ref[n]) < 1e-3, (R.case_id(c), flav.__name__, n, R.rel_max(got[n], ref[n]))
    for M, K, N in R.LINEAR_SHAPES:
        x, W, b, dy = R.linear_inputs(M, K, N)
        ref, f32, s3 = R.linear_ref(x, W, b, dy), R.linear_fp32(x, W, b, dy), R.linear_split3(x, W, b, dy)
        for n in ref:
            assert R.rel_max(f32[n], ref[n]) < 1e-3 and R.rel_max(s3[n], ref[n]) < 1e-3, (M, K, N, n)
        assert all(R.rel_max(s3[n], ref[n]) > R.rel_max(f32[n], ref[n]) for n in ("y", "dx", "dW")), (M, K, N)


def test_split3_is_three_bf16_passes():
    """mm_split3 on operands that are bf16 values already is the exact product; on fp32 operands it misses exactly the lo.lo term."""
    gen = torch.Generator().manual_seed(5)
    a, b = torch.randn(7, 64, generator=gen), torch.randn(64, 5, generator=gen)
    ab, bb = a.bfloat16().float(), b.bfloat16().float()
    assert torch.equal(R.mm_split3(ab, bb), (ab.double() @ bb.double()).float())
    (ah, al), (bh, bl) = R.bf16_split(a), R.bf16_split(b)
    assert float((ah + al - a).abs().max()) <= 2.0 ** -16 * float(a.abs().max())
    full = (ah + al).double() @ (bh + bl).double()
    assert torch.equal(R.mm_split3(a, b), (full - al.double() @ bl.double()).float())


@functools.lru_cache(maxsize=None)
def conv3_data(c):
    """(inputs, float64 reference, split3 flavour) of a Conv3Case, computed once for the tests below."""
    inp = R.conv_inputs(c)
    return inp, R.conv3_ref(c, *inp), R.conv3_split3(c, *inp)


@functools.lru_cache(maxsize=None)
def direct_data(c):
    """(inputs, float64 reference with the absolute sums, split3 dW) of a DirectCase."""
    inp = R.conv_inputs(c)
    x, _, _, dy = inp
    return inp, R.direct_ref(c, *inp), R.wgrad_split3(R._nchw(dy), R._nchw(x))


def test_conv_references_are_autograd():
    """conv3_ref's hand-written gradients (flipped, channel-exchanged filter; zero insertion at the even positions; 2 x 2 block sums)
    and direct_ref's (the filter rows c0 .. c0 + n; dW = dy^T im2col(x) in OIHW order) equal torch.autograd through F.conv2d(stride) and
    F.interpolate(mode="nearest") in float64 to 1e-12, on every listed case."""
    for c in R.conv3_cases():
        inp, ref, _ = conv3_data(c)
        auto = R.conv3_autograd(c, *inp)
        for n in ("y", "dx"):
            assert ref[n].dtype == torch.float64 and ref[n].shape == auto[n].shape and ref[n].is_contiguous(), (c, n)
            assert close(ref[n], auto[n], 1e-12), (c, n, float((ref[n] - auto[n]).abs().max()))
        assert ref["dx"].shape == inp[0].shape and ref["y"].shape == inp[3].shape
    for c in R.direct_cases():
        inp, ref, _ = direct_data(c)
        auto = R.direct_autograd(c, *inp)
        for n in ("y", "dx", "dW"):
            assert ref[n].dtype == torch.float64 and ref[n].shape == auto[n].shape, (c, n)
            assert close(ref[n], auto[n], 1e-12), (c, n, float((ref[n] - auto[n]).abs().max()))
        assert ref["dW"].shape == inp[1].shape and ref["dx"].shape[-1] == c.n
        assert bool((ref["y_abs"] >= ref["y"].abs()).all()) and bool((ref["dx_abs"] >= ref["dx"].abs()).all())


def test_conv_split3_is_three_bf16_passes():
    """conv_split3 and wgrad_split3 on operands that are bf16 values already are the exact conv / weight gradient; on fp32 operands they
    miss exactly the lo.lo term; the flavours of every listed case stay within 1e-3 of float64, and the direct conv's worst-case chain bound stays
    below 1e-2 of the largest value (2881 roundings at 320 channels)."""
    gen = torch.Generator().manual_seed(11)
    a, w = torch.randn(2, 8, 5, 7, generator=gen), torch.randn(6, 8, 3, 3, generator=gen)
    dy = torch.randn(2, 6, 5, 7, generator=gen)
    ab, wb, dyb = (t.bfloat16().float() for t in (a, w, dy))
    for stride in (1, 2):
        assert torch.equal(R.conv_split3(ab, wb, stride), R.conv_f64(ab, wb, stride).float())
        (ah, al), (wh, wl) = R.bf16_split(a), R.bf16_split(w)
        full = R.conv_f64(ah.double() + al.double(), wh.double() + wl.double(), stride)
        assert torch.equal(R.conv_split3(a, w, stride), (full - R.conv_f64(al, wl, stride)).float())
    assert torch.equal(R.wgrad_split3(dyb, ab), R.wgrad_f64(dyb, ab).float())
    (dh, dl), (ah, al) = R.bf16_split(dy), R.bf16_split(a)
    full = R.wgrad_f64(dh.double() + dl.double(), ah.double() + al.double())
    assert float((R.wgrad_split3(dy, a).double() - (full - R.wgrad_f64(dl, al))).abs().max()) <= 2.0 ** -23 * float(full.abs().max())
    for c in R.conv3_cases():
        _, ref, s3 = conv3_data(c)
        for n in ("y", "dx"):
            assert s3[n].dtype == torch.float32 and 0 < R.rel_max(s3[n], ref[n]) < 1e-3, (c, n)
    for c in R.direct_cases():
        _, ref, dW3 = direct_data(c)
        assert 0 < R.rel_max(dW3, ref["dW"]) < 1e-3, c
        for n, bound in R.direct_bounds(c, ref).items():
            assert float(bound.max()) < 1e-2 * float(ref[n].abs().max()) and float(bound.min()) > 0, (c, n)


# mutation -> the tensors it reaches, per kind of case
CONV3_MUTATIONS = {"lo_hi_last_row": ("y", "dx"), "hi_lo_tap0": ("y", "dx"), "bf16x1": ("y", "dx"), "no_flip": ("dx",), "zero_insert_odd": ("dx",),
                   "sum2x2_missing": ("dx",)}
DW_MUTATIONS = ("lo_hi_last_row", "hi_lo_tap0", "bf16x1", "dW_taps_transposed")
# (mutation, case id, tensor) where the mutation provably changes nothing, so the mutated tensor has to equal the unmutated one:
#   at 1 x 1 every tap but the centre reads padding -- tap (0, 0) contributes nothing, its im2col columns are zero, the flip keeps the
#   centre where it is and so does exchanging ky and kx;
#   the single output of the 2 x 2 Downsample reads rows -1 .. 1: its tap (0, 0) is padding too
UNCHANGED = {("hi_lo_tap0", "g0-1x1x1-64-64", "y"), ("hi_lo_tap0", "g0-1x1x1-64-64", "dx"), ("no_flip", "g0-1x1x1-64-64", "dx"),
             ("hi_lo_tap0", "g1-1x2x2-64-64", "y"), ("hi_lo_tap0", "direct-1x1x1-64-4-c0n64", "dW"),
             ("dW_taps_transposed", "direct-1x1x1-64-4-c0n64", "dW")}


def test_conv_mutations_exceed_the_bounds():
    """What the bounds of the GPU tests see, computed here on the CPU: on every listed case, each way of getting the conv subtly wrong
    pushes every tensor it reaches over that tensor's bound -- the split-family bound 4 e3 for conv3's y and dx and for dW, the
    elementwise fp32-chain bound for the direct conv's y and dx. The only tensors let off are those of UNCHANGED, which have to be
    bit-equal to the unmutated flavour. Prints the table mutation, case, tensor, measure, bound."""
    seen = set()

    def judge(mut, cid, n, measure, bound, mutated, plain):
        print(f"[conv mutations] {mut:18s} {cid:26s} {n:3s} measure {measure:.3e}  bound {bound:.3e}  x{measure / bound:.1f}")
        if (mut, cid, n) in UNCHANGED:
            seen.add((mut, cid, n))
            assert torch.equal(mutated, plain), (mut, cid, n)
        else:
            assert measure > bound, (mut, cid, n, measure, bound)

    for c in R.conv3_cases():
        inp, ref, s3 = conv3_data(c)
        cid = R.conv_case_id(c)
        for mut, names in CONV3_MUTATIONS.items():
            if (mut == "zero_insert_odd" and c.geom != 1) or (mut == "sum2x2_missing" and c.geom != 2):
                continue
            bad = R.conv3_split3(c, *inp, mut=mut)
            for n in names:
                judge(mut, cid, n, R.rel_max(bad[n], ref[n]), R.split_family_bound(R.rel_max(s3[n], ref[n])), bad[n], s3[n])
    for c in R.direct_cases():
        (x, w, b, dy), ref, dW3 = direct_data(c)
        cid = R.conv_case_id(c)
        for mut in DW_MUTATIONS:
            bad = R.wgrad_split3(R._nchw(dy), R._nchw(x), mut)
            judge(mut, cid, "dW", R.rel_max(bad, ref["dW"]), R.split_family_bound(R.rel_max(dW3, ref["dW"])), bad, dW3)
        bad, bounds = R.direct_ref(c, x, w, b, dy, clamp=True), R.direct_bounds(c, ref)
        for n in ("y", "dx"):
            # the measure of an elementwise bound is the worst |error| / bound, against 1
            judge("clamp_border", cid, n, R._reduction_row(cid, n, bad[n], ref[n], bounds[n])[2], 1.0, bad[n], ref[n])
    assert seen == UNCHANGED


def test_norm_references_are_torchs():
    """The hand-written GroupNorm (pixel rows, groups of adjacent channels) equals F.group_norm + F.silu and their autograd in float64;
    layernorm_ref's xhat and rstd are those of F.layer_norm's output."""
    for B, HW, C in R.GN_SHAPES[1:]:
        x, g, b, da, dx0 = R.groupnorm_inputs(B, HW, C, 8)
        for silu in (False, True):
            ref = R.groupnorm_silu_ref(x, g, b, silu, 1e-5, da, dx0)
            xc = x.double().permute(0, 2, 1).contiguous().requires_grad_(True)
            u = F.group_norm(xc, 32, g.double(), b.double(), 1e-5)
            a = F.silu(u) if silu else u
            a.backward(da.double().permute(0, 2, 1))
            assert close(ref["a"], a.detach().permute(0, 2, 1), 1e-12)
            assert close(ref["dx"], xc.grad.permute(0, 2, 1) + dx0.double(), 1e-11)
            assert close(ref["xhat"] * g.double() + b.double(), u.detach().permute(0, 2, 1), 1e-12)
    x, g, b, da, _ = R.groupnorm_inputs(1, 1, 32, 30)
    one = R.groupnorm_silu_ref(x, g, b, True, 1e-5, da)          # a group of one value: xhat and dx are exactly 0
    assert not one["xhat"].any() and not one["dx"].any() and torch.equal(one["a"], F.silu(b.double()).reshape(1, 1, 32))
    x, g, b, dy, _ = R.layernorm_inputs(5, 96, 8)
    ref = R.layernorm_ref(x, g, b, 1e-6, dy)
    assert close(ref["xhat"] * g.double() + b.double(), ref["y"], 1e-13)
    assert close(ref["xhat"], (x.double() - x.double().mean(dim=-1, keepdim=True)) * ref["rstd"][:, None], 1e-12)
    assert not ref["xhat"][-1].any()                                # the constant row


def test_guard_zones_detect_a_write_outside():
    """Guarded reports a clean buffer as clean, and names a write one element in front of or behind the output, an element left
    unwritten and a non-finite result."""
    shapes = {"a": (3, 5), "b": (7,)}
    G = R.Guarded(shapes, "cpu")
    assert G.views["a"].shape == (3, 5) and G.views["a"].is_contiguous() and G.views["a"].data_ptr() % 16 == G.bufs["a"].data_ptr() % 16
    assert len(G.problems()) == 2 and all("not written" in p for p in G.problems())      # NaN everywhere before the call
    for v in G.views.values():
        v.fill_(1.0)
    assert G.problems() == []
    G.bufs["a"][R.GUARD + 15] = 2.0                                 # one element behind the last
    assert [p for p in G.problems() if p.startswith("a:") and "back guard" in p] and not [p for p in G.problems() if p.startswith("b:")]
    G = R.Guarded(shapes, "cpu")
    for v in G.views.values():
        v.fill_(1.0)
    G.bufs["b"][R.GUARD - 1] = float(torch.tensor(R.SENTINEL_BITS, dtype=torch.int32).view(torch.float32)) + 1.0   # the sentinel's neighbour value
    assert any(p.startswith("b:") and "front guard" in p for p in G.problems())
    G = R.Guarded(shapes, "cpu", init={"b": torch.arange(7.0)})
    assert torch.equal(G.views["b"], torch.arange(7.0))
    G.views["a"].fill_(0.0)
    G.views["a"][1, 2] = float("nan")
    assert any("1 of 15 elements were not written" in p for p in G.problems())
    G.views["a"][1, 2] = float("inf")
    assert any("not finite" in p for p in G.problems())


def test_measure_and_chains():
    """rel_max is an elementwise maximum (one wrong row of many is seen in full); an all-zero reference admits only zeros; the chain
    lengths are those of dot_reduce_kernel, the chunked path and colsum_kernel."""
    ref = torch.ones(4096, 8, dtype=torch.float64)
    got = ref.clone()
    got[17] *= 1.1
    assert abs(R.rel_max(got, ref) - 0.1) < 1e-12
    z = torch.zeros(3)
    assert R.rel_max(z, z) == 0.0 and R.rel_max(z + 1e-30, z) == float("inf")
    assert [R.dot_chain(n) for n in (1, 1024, 1025, 1 << 18)] == [23, 23, 24, 256 + 22]
    assert R.dot_chain((1 << 18) + 1) == 64 + 22 + 5 and R.dot_chain(R.DOT_SIZES[-1]) == 64 + 22 + 8
    assert [R.colsum_chain(r) for r in (1, 16, 17, 188)] == [17, 17, 18, 28]
    assert R.fp32_family_bound(0.0) == 2.0 ** -22 and R.fp32_family_bound(1e-6) == 8e-6 and R.split_family_bound(1e-5) == 4e-5


def test_case_lists():
    """The cases the issue sets: every head dim, both tile sizes crossed, B H <= 6, the regimes, the shapes of the other primitives."""
    cases = R.attention_cases()
    assert len(cases) == 2 * 9 + 3 * 3 + 1 and len(set(cases)) == len(cases)
    assert all(c.B * c.H <= 6 for c in cases) and {c.D for c in cases} == {32, 40, 64, 80, 160}
    assert {(c.Nq, c.Nk) for c in cases if c.D == 160} == set(R.ATTN_PAIRS) and (1, 3) in {(c.B, c.H) for c in cases}
    assert len(R.attention_cases(R.MFMA_DIMS)) == 19 and len(R.attention_regime_cases()) == 8
    assert (100, 96, 384) in R.LINEAR_SHAPES and (100, 384, 96) in R.LINEAR_SHAPES and len(R.LINEAR_SHAPES) == 7
    assert [C // 32 for _, _, C in R.GN_SHAPES] == [1, 2, 10, 3]
    assert R.DOT_SIZES == [1, 1023, 1025, 262144, 262145, 458759]
    # the convolutions: every form at the smallest shapes at which its path can still go wrong
    assert R.CONV3_SHAPES == [(2, 32, 32, 64, 128), (8, 16, 16, 128, 128), (1, 64, 64, 64, 128), (1, 12, 20, 192, 128), (3, 8, 8, 128, 320),
                              (2, 8, 8, 640, 320), (2, 2, 2, 128, 128), (1, 1, 1, 64, 64)]
    assert R.CONV3_DOWN_SHAPES == [(2, 16, 16, 128), (1, 12, 20, 64), (1, 2, 2, 64), (1, 64, 64, 64)]
    assert R.CONV3_UP_SHAPES == [(2, 8, 8, 128), (1, 6, 10, 64), (1, 1, 1, 64), (2, 16, 16, 128)]
    assert R.CONV_DIRECT_SHAPES == [(2, 8, 8, 320, 4, 0, 320), (1, 5, 7, 64, 4, 0, 64), (1, 1, 1, 64, 4, 0, 64), (2, 8, 8, 4, 320, 0, 4),
                                    (2, 8, 8, 9, 64, 0, 9), (1, 5, 7, 12, 64, 4, 8)]
    c3 = R.conv3_cases()
    assert len(c3) == 16 and [c.geom for c in c3] == [0] * 8 + [1] * 4 + [2] * 4 and all(c.Cin == c.Cout for c in c3 if c.geom)
    assert all(c.Cin % 64 == 0 and c.Cout % 64 == 0 for c in c3) and all(c.H % 2 == 0 and c.W % 2 == 0 for c in c3 if c.geom == 1)
    assert max(27 * c.Cin for c in c3) == 17280 and len({R.conv_case_id(c) for c in c3 + R.direct_cases()}) == 16 + 6
    assert all(" " not in R.conv_case_id(c) for c in c3 + R.direct_cases())
    assert R.CONV_FAMILIES == ("conv_halo_kernel", "gemm_u_kernel(conv)", "gemm_glds_kernel(conv)")
    assert R.gemm_kernel_family({"kernel": "gemm_u_kernel<2, 2, 5, 1, 2, false> + splitk_reduce_kernel"}) == "gemm_u_kernel(conv)"
    assert R.gemm_kernel_family({"kernel": "gemm_u_kernel<2, 4, 4, 0, 2, false>"}) == "gemm_u_kernel"
    assert R.gemm_kernel_family({"kernel": "gemm_glds_kernel<64x64, 1>"}) == "gemm_glds_kernel(conv)"
    assert R.gemm_kernel_family({"kernel": "conv_halo_kernel<4, 8> + splitk_reduce_kernel"}) == "conv_halo_kernel"


# ---- the C ABI
def _declared(header):
    return set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_train_prim_entry_points_are_declared_exported_and_bound():
    """include/gligen_amd_train_prims.h declares exactly the names of TRAIN_PRIM_SYMBOLS, the built library exports them with the table's
    argument types, and the table shares no name with the other tables or headers."""
    from gligen_amd import _lib as table
    from gligen_amd.build import build_native
    build_native()
    lib = table.load()
    declared = _declared("gligen_amd_train_prims.h")
    assert declared == set(table.TRAIN_PRIM_SYMBOLS) == {"gl_op_train_attention", "gl_op_train_linear", "gl_op_train_layernorm", "gl_op_train_groupnorm",
                                                         "gl_op_train_geglu", "gl_op_train_dot", "gl_op_train_conv3", "gl_op_train_conv_direct"}
    raw = ctypes.CDLL(str(table.LIB_PATH))
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes == table.TRAIN_PRIM_SYMBOLS[name][1] and getattr(lib, name).restype == table.TRAIN_PRIM_SYMBOLS[name][0]
    others = (table.SYMBOLS, table.IMAGE_SYMBOLS, table.MAP_SYMBOLS, table.TRAIN_MAP_SYMBOLS, table.TRAIN_INPUT_SYMBOLS, table.TRAIN_FUSER_SYMBOLS,
              table.TRAINER_SYMBOLS)
    assert not declared & set().union(*others)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "gligen_amd_train_prims.h":
            assert not declared & set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read())), other
    # the argument counts of the header's prototypes are the table's
    text = open(os.path.join(ROOT, "include", "gligen_amd_train_prims.h")).read()
    for name, (_, args) in table.TRAIN_PRIM_SYMBOLS.items():
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text).group(1)
        assert len(proto.split(",")) == len(args), name
    # capi.hip sees the training path through train.h only
    capi = open(os.path.join(ROOT, "gligen_amd", "csrc", "capi.hip")).read()
    assert '#include "train_impl.h"' not in capi


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "gligen_amd_train_prims.h"\nint main(void) { return sizeof(gl_stream) == 0; }\n')
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")], check=True)
