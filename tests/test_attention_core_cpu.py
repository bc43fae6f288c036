"""attention_core_ref by itself, without a GPU: the encoders against the decoder of the projection tests, the reference against
torch.softmax, the emulation of every kernel's rounding points against the derived bound on every case of the GPU grids, and the
conditions the case list promises (quiet rows; structured cases that are sensitive to one key too many and one key too few)."""
import os
import re

import pytest
import torch

import attention_core_ref as R
import gemm_candidates_ref as G

KERNEL_DIMS = [(kn, d) for kn, K in R.KERNELS.items() for d in K["dims"]]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    header = open(os.path.join(ROOT, "include", "gligen_amd_attention_core.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", code)) == set(_lib.ATTENTION_CORE_SYMBOLS) == {"gl_op_attention_core"}
    assert not set(_lib.ATTENTION_CORE_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.GEMM_PLAN_SYMBOLS))
    enum = dict((n, int(v)) for n, v in re.findall(r"GL_ATTN_CORE_([A-Z0-9_]+) = (\d)", code))
    assert enum == dict(AUTO=0, V1=1, V2_W4=2, V2_W8=3, V3=4)
    assert _lib.ATTN_CORE_KERNELS == {"auto": 0, "attn_kernel": 1, "attn2_kernel_w4": 2, "attn2_kernel_w8": 3, "attn3_kernel": 4}
    assert set(_lib.ATTN_CORE_KERNELS) == set(R.KERNELS) | {"auto"}
    lib = _lib.load()
    lay = R.layout(40, 1, 1, 0)
    import ctypes
    assert lib.gl_op_attention_core(None, None, None, None, ctypes.byref(lay), 1, 1, 1, 1, None, 40, 1, 0, None) == 2     # no context


@pytest.mark.parametrize("d,perm32", [(40, 0), (40, 1), (80, 0), (80, 1), (160, 0)])      # (no 32-token V^T form exists at d = 160)
def test_encoders_round_trip(d, perm32):
    """encode -> proj_region gives the logical tensors back, for both V^T forms and all head dims; what encode adds outside them is the
    header's MUST HOLD table and zeros."""
    Nq, Nk = 100, 77
    c = R.make_case(d, Nq, Nk, "random")
    lay = R.layout(d, Nq, Nk, perm32)
    q, k, vt = R.encode(lay, c.q, c.k, c.v, c.pad)
    full = dict(q=torch.cat([c.q, c.pad["q"]], 2), k=torch.cat([c.k, c.pad["k"]], 2), vt=torch.cat([c.v, c.pad["vt"]], 2))
    seen = {}
    for name, buf in (("q", q), ("k", k), ("vt", vt)):
        reg, val = G.proj_region(lay, R.B, R.H, name, buf)
        want = full[name].permute(0, 2, 1, 3).reshape(R.B, -1, R.H * d)
        assert torch.equal(val.double(), want), name
        rest = buf.clone()
        G.proj_region(lay, R.B, R.H, name, rest)[0][...] = 0
        seen[name] = rest
    # the rest of q is zero; of k: column 40 = 1.0 at d = 40 and zero; of vt: row d = 1.0 where dpv > d and zero
    assert not bool(seen["q"].any())
    k6 = seen["k"].view(R.B, R.H, lay.tk_pad // 64, lay.dp // 8, 64, 8)
    if d == 40:
        assert bool((k6[:, :, :, 5, :, 0] == 1).all())
        k6[:, :, :, 5, :, 0] = 0
    assert not bool(seen["k"].any())
    v4 = seen["vt"].view(R.B, R.H, lay.dpv, lay.tk_pad)
    if lay.dpv > d:
        assert bool((v4[:, :, d] == 1).all())
        v4[:, :, d] = 0
    assert not bool(seen["vt"].any())
    # the two V^T forms really differ (an identity permutation in either would pass the round trip of a symmetric decoder alone)
    i16, i32 = (R.index_map(R.layout(40, 64, 64, p), "vt")[0, 0, :32, 0] for p in (0, 1))
    assert i16.tolist()[:16] == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert i32.tolist() == [0, 1, 2, 3, 16, 17, 18, 19, 4, 5, 6, 7, 20, 21, 22, 23, 8, 9, 10, 11, 24, 25, 26, 27, 12, 13, 14, 15, 28, 29, 30, 31]


@pytest.mark.parametrize("d", [40, 80, 160])
def test_reference_is_softmax(d):
    for kind in R.KINDS:
        c = R.make_case(d, 33, 200, kind)
        want = torch.softmax((c.q @ c.k.transpose(-1, -2)) * d ** -0.5, -1) @ c.v
        got = R.reference(c.q, c.k, c.v)
        assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), kind
        o, bound = R.reference_and_bound(c.q, c.k, c.v, "attn_kernel")
        assert torch.equal(o, got) and bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
    one = R.make_case(d, 5, 1, "uniform")
    assert torch.equal(R.reference(one.q, one.k, one.v), one.v.expand(-1, -1, 5, -1))


def test_unsupported_table_covers_every_selector():
    t = R.unsupported_table()
    assert {(kn, d) for kn, d, p, nk, bad in t if not bad} == set(KERNEL_DIMS)
    for kn, d, p, nk, bad in t:
        K = R.KERNELS[kn]
        assert bad == (d not in K["dims"] or p != K["perm32"] or (K["pipelined"] and nk <= 128))
    assert any(bad for kn, d, p, nk, bad in t if kn == "attn3_kernel" and d == 40 and p == 1 and nk == 128)
    assert not any(bad for kn, d, p, nk, bad in t if kn == "attn3_kernel" and d == 40 and p == 1 and nk == 129)


@pytest.mark.parametrize("kernel,d", KERNEL_DIMS, ids=[f"{k}-d{d}" for k, d in KERNEL_DIMS])
def test_emulation_within_bound_and_case_conditions(kernel, d):
    """Every case of the kernel's GPU grid: the float64 emulation of its rounding points stays within the bound; every row is quiet
    (attn3_kernel's lazy stabiliser never moves); the structured cases see one key too many and one key too few at >= 100 x the bound.
    make_case draws the query rows of every Nq from one master block, so Nq = max(NQS) holds the rows of every grid point."""
    worst = 0.0
    for Nk in sorted({nk for _, nk in R.grid(kernel)}):
        Nq = max(R.NQS)
        for kind in R.KINDS:
            c = R.make_case(d, Nq, Nk, kind)
            o, bound = R.reference_and_bound(c.q, c.k, c.v, kernel)
            emu = R.emulate(c.q, c.k, c.v, kernel)
            ratio = float(((emu - o).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (kernel, d, Nk, kind, ratio)
            assert R.quiet_margin(c.q, c.k) < R.QUIET, (kernel, d, Nk, kind)
            # the filled padding: a padded key would beat every real score of every row, the padding query rows included
            if Nk % 64:
                qall = torch.cat([c.q, c.pad["q"]], 2)
                s_real = R.scores_log2(qall, c.k).max(-1).values
                s_pad = R.scores_log2(qall, c.pad["k"]).min(-1).values
                if kind == "uniform":
                    assert bool((s_pad[:, :, Nq:] > s_real[:, :, Nq:]).all())
                else:
                    assert bool((s_pad > s_real).all()), (kernel, d, Nk, kind)
            if kind in R.STRUCTURED:
                if Nk % 64:
                    assert float(((R.with_first_padded_key(c) - o).abs() / bound).max()) >= 100.0, (kernel, d, Nk, kind, "one key too many")
                if kind == "last" and Nk > 1:
                    assert float(((R.without_last_key(c) - o).abs() / bound).max()) >= 100.0, (kernel, d, Nk, kind, "one key too few")
            if kind == "uniform":
                assert float((o - c.v.mean(2, keepdim=True)).abs().max()) < 1e-14
    print(f"[attention_core] {kernel} d={d}: worst emulation / bound = {worst:.3f}")
    assert worst > 0.02, "the emulation rounds nowhere, or the bound is far from the rounding it describes"
