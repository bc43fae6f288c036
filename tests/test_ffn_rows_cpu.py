"""ffn_rows_ref by itself, without a GPU: the GELU fit of ffn.hip against float64 erfc, the fp32 emulation of the row-local kernels
against the derived bounds on every case of the GPU test, eight seeded defects the check has to reject, the cases against the
kernels' own preconditions, and the entry points' declaration."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import attention_core_ref as A
import ffn_rows_ref as R
import gemm_candidates_ref as G

ROOT = G.ROOT
BY_NAME = {c.name: c for c in R.CASES}


def test_entry_points_are_declared_exported_and_bound(tmp_path):
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    header = open(os.path.join(ROOT, "include", "gligen_amd_ffn_rows.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(gl_op_[a-z0-9_]+)\s*\(", code)) == set(_lib.FFN_ROWS_SYMBOLS) == {"gl_op_ff_rows", "gl_op_qkv_rows"}
    assert not set(_lib.FFN_ROWS_SYMBOLS) & set(_lib.SYMBOLS)
    # the structs: same fields in the same order, same size as the C compiler gives them
    for cname, st in (("gl_ff_rows_args", _lib.FFRowsArgs), ("gl_qkv_rows_args", _lib.QkvRowsArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, flags=re.S).group(1)
        names = [re.findall(r"[A-Za-z_0-9]+", piece)[-1] for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
        assert names == [n for n, _ in st._fields_], cname
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "gligen_amd_ffn_rows.h"\nint main(void) { printf("%zu %zu\\n", sizeof(gl_ff_rows_args), sizeof(gl_qkv_rows_args)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_lib.FFRowsArgs), ctypes.sizeof(_lib.QkvRowsArgs)]
    lib = _lib.load()
    assert lib.gl_op_ff_rows(None, None, None) == 2 and lib.gl_op_qkv_rows(None, None, None) == 2          # no context


def test_gelu_fit_holds_its_stated_error():
    """max(x, 0) - |x| 2^L(|x|) with the four constants of ffn.hip, evaluated in fp32 as geglu_step does, against x Phi(x) from float64
    erfc: within the 7.8e-5 the source states (and the bound uses) on a grid of step 2^-10 over [-12, 12] and far out; finite
    everywhere; exactly x and exactly 0 in the tails."""
    coef = R.gelu_fit_coefficients()
    assert len(coef) == 4 and all(v < 0 for v in coef), "all coefficients negative: h -> 0 for large |x|"
    x = torch.cat([torch.arange(-12 * 1024, 12 * 1024 + 1, dtype=torch.float32) / 1024, torch.tensor([-300.0, -40.0, -20.0, 20.0, 40.0, 300.0])])
    got = R.gelu_fit32(x, coef)
    assert bool(torch.isfinite(got).all())
    err = (got.double() - R.gelu64(x.double())).abs()
    worst = float(err.max())
    print(f"[ffn_rows] GELU fit: max |fit - x Phi(x)| = {worst:.3e} at x = {float(x[err.argmax()]):.4f}")
    assert worst <= R.GELU_FIT, worst
    far = torch.tensor([20.0, 40.0, 300.0])
    assert torch.equal(R.gelu_fit32(far, coef), far) and torch.equal(R.gelu_fit32(-far, coef), torch.zeros(3))
    # the sweep of the GPU test holds these points, as bf16 values
    g = R.sweep_gates()
    assert g.numel() == 4 * R.C and float(g.min()) == -300 and float(g.max()) == 300 and torch.equal(g, g.bfloat16().float())
    dense = g[(g >= -12) & (g <= 12)].sort().values
    assert float((dense[1:] - dense[:-1]).max()) <= 2.0 ** -4          # bf16 spacing at 8 .. 12 is 2^-4: the densest grid a bf16 bias can hold


def test_cases_meet_the_kernels_preconditions():
    for c in R.CASES:
        assert R.preconditions(c) == [], (c.name, R.preconditions(c))
        assert c.M <= 512
    # the transcription refuses what the source refuses
    c = BY_NAME["plain_M256_m0"]
    for k, v in (("M", 100), ("ldx", R.C + 4), ("ldo", R.C + 2)):
        bad = type(c)(**{**vars(c), k: v})
        assert R.preconditions(bad), k
    q = BY_NAME["period_T_M2T"]
    for k, v in (("T", 64), ("in_period", 64), ("in_period", 384), ("DP", 44), ("Tpad_k", 100), ("np", 2)):
        bad = type(q)(**{**vars(q), k: v})
        assert R.preconditions(bad), k
    # and the list holds what the issue names
    ff, qk = R.FF_CASES, R.QKV_CASES
    plain = [c for c in ff if not c.pre and not c.special]
    assert {(c.normalize, c.res, c.gate) for c in plain} >= {(n, r, g) for n in (0, 1) for r in (True, False) for g in (None, 0.37, 0.0, -0.6)}
    assert {c.mean for c in plain if c.normalize} == {0.0, 8.0, 32.0} and {c.ldx for c in plain} == {R.C, R.C + 8} and {c.stats for c in plain} == {True, False}
    assert {c.M for c in ff} == {128, 256, 384}
    chained = [c for c in ff if c.pre]
    for post in (0, 1, 2):
        assert {(c.pre_gate, c.gate) for c in chained if c.post == post} >= {(0.37, -0.6), (None, None), (0.5, 1e-30), (0.37, 1e-19)}
        assert {c.stats for c in chained if c.post == post} == {True, False}
    assert {(c.qTpad - c.qT, c.M // c.qT) for c in chained if c.post == 2} >= {(0, 1), (64, 1), (0, 2), (64, 2)}
    assert R.mid_written(BY_NAME["chain_pre_g0.5_1e-30"]) and not R.mid_written(BY_NAME["chain_pre_tiny_gate"])
    assert {(c.pre, c.pre_res) for c in qk} == {(1, True), (1, False), (0, False)} and {c.np for c in qk} == {1, 3}
    assert {(c.pre, c.normalize, c.np) for c in qk} == {(p, n, k) for p, n in ((1, 1), (0, 1), (0, 0)) for k in (1, 3)}
    assert {c.B for c in qk if not c.in_period} == {1, 2, 3} and {c.Tpad_k - c.T for c in qk} == {0, 64}
    assert {(c.in_period, c.M) for c in qk if c.in_period} == {(128, 256), (256, 512)}


def test_layout_index_is_the_kernels_addressing():
    """head_index against the address arithmetic of qkv_rows_kernel's stores (heads_qk, heads_vt) and gemm.h ktile_off, written out
    here element by element; and against attention_core_ref.index_map where the two describe the same buffer."""
    T, B = 128, 2
    for pad in (0, 64):
        lay = R.head_layout(T, T + pad, T + pad, 48, 48)
        b, t, f = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(R.C), indexing="ij")
        hd, dd = f // R.D, f % R.D
        tp = T + pad
        want = dict(q=((b * R.H + hd) * tp + t) * 48 + dd,
                    k=(b * R.H + hd) * tp * 48 + (t // 64) * 64 * 48 + (dd // 8) * 512 + (t % 64) * 8 + dd % 8,
                    vt=((b * R.H + hd) * 48 + dd) * tp + (t & ~31) + 16 * ((t >> 2) & 1) + 4 * ((t >> 3) & 3) + (t & 3))
        for name in ("q", "k", "vt"):
            assert torch.equal(R.head_index(lay, name, B, "cpu"), want[name].reshape(B * T, R.C)), (name, pad)
    lay = R.head_layout(T, T, T, 48, 48)
    for name in ("q", "k", "vt"):
        assert torch.equal(R.head_index(lay, name, B, "cpu").view(B, T, R.H, R.D).permute(0, 2, 1, 3), A.index_map(A.layout(40, T, T, 1), name, B, R.H)), name
    # heads_vt: register 4 j + e of the lane with half h is token tw + 8 j + 4 h + e, stored at tw + 16 h + 4 j + e
    for j in range(4):
        for h in range(2):
            for e in range(4):
                t = 8 * j + 4 * h + e
                assert (t & ~31) + 16 * ((t >> 2) & 1) + 4 * ((t >> 3) & 3) + (t & 3) == 16 * h + 4 * j + e


def _run(c, defect=None, tamper=None):
    ins = R.make_inputs(c, "cpu")
    outs = R.make_outputs(c, "cpu")
    R.store(outs, R.emulate(c, ins, defect))
    if tamper:
        tamper(outs)
    return R.verify(c, ins, outs)


@pytest.mark.parametrize("kind", ["ff", "qkv"])
def test_emulation_is_within_the_bounds_on_every_case(kind):
    lines, top = [], 0.0
    for c in (R.FF_CASES if kind == "ff" else R.QKV_CASES):
        worst = _run(c)
        lines.append(R.report_line(c, worst))
        top = max(top, max(r for r, _ in worst.values()))
    print("\n".join(lines))
    assert top > 0.02, "the emulation rounds nowhere, or the bounds are far from the rounding they describe"


def _plain(res):
    """The first plain case with zero-mean normalised rows, one workgroup, with / without a residual."""
    return next(c.name for c in R.FF_CASES if not c.pre and not c.special and c.normalize and c.mean == 0 and c.M == 128 and c.res == res)


DEFECTS = [("1 one chunk's FF-out contribution dropped from one element", _plain(False), "drop_chunk", "out"),
           ("2 two hidden features' W2 columns exchanged", _plain(False), "swap_w2_columns", "out"),
           ("3 the two half-waves' feature quads exchanged", _plain(True), "swap_half_waves", "out"),
           ("4 two tokens exchanged in K and V^T alike", "pre_res_B1", "swap_tokens", "k"),
           ("5 value and gate halves exchanged for one block", _plain(False), "swap_value_gate", "out"),
           ("6 output row m from input row m instead of m % in_period", "period_T_M2T", "no_period", "mid"),
           ("8 stats_out from the fp32 values instead of the stored bf16 ones", "stats_of_stored", "stats_of_fp32", "stats")]


@pytest.mark.parametrize("what,case,defect,output", DEFECTS, ids=[d[0].split()[0] for d in DEFECTS])
def test_seeded_defects_are_rejected(what, case, defect, output):
    c = BY_NAME[case]
    _run(c)
    with pytest.raises(AssertionError) as e:
        _run(c, defect)
    assert e.value.args[0][0] == case and e.value.args[0][1] == output and "err / bound" in e.value.args[0], (what, e.value.args)


def test_seeded_defect_7_one_padding_element_of_each_head_buffer():
    """q: a padding column [40, 48) and a padding row [T, Tpad_q); K: its column 40 .. 47 block and its extra key tile; V^T: a padding
    row and a column behind T; a stride gap of mid_out; a guard element."""
    c = BY_NAME["pre_res_B2"]
    assert c.Tpad_k == c.T + 64 and c.np == 3
    lay = R.head_layout(c.T, c.Tpad_q, c.Tpad_k, c.DP, c.DPV)
    q4 = lambda o: o["q"].payload.view(c.B * R.H, c.Tpad_q, c.DP)
    k6 = lambda o: o["k"].payload.view(c.B * R.H, c.Tpad_k // 64, c.DP // 8, 64, 8)
    v3 = lambda o: o["vt"].payload.view(c.B * R.H, c.DPV, c.Tpad_k)
    spots = [("q", lambda o: q4(o)[3, 5, 41:42]), ("q", lambda o: q4(o)[0, c.T, 0:1]), ("k", lambda o: k6(o)[2, 0, 5, 7, 0:1]), ("k", lambda o: k6(o)[15, 2, 0, 0, 0:1]),
             ("vt", lambda o: v3(o)[1, 40, 3:4]), ("vt", lambda o: v3(o)[9, 0, c.T:c.T + 1]), ("q", lambda o: o["q"].flat[0:1]), ("vt", lambda o: o["vt"].flat[-1:])]
    _run(c)
    for name, spot in spots:
        def tamper(outs, spot=spot):
            v = spot(outs)
            v.copy_((v.view(torch.int16) ^ 1).view(torch.bfloat16))      # one bit of one element
        with pytest.raises(AssertionError) as e:
            _run(c, tamper=tamper)
        assert e.value.args[0][:2] == (c.name, name) and "outside the written region" in e.value.args[0][2]
    cs = BY_NAME["pre_res_B3"]
    assert cs.ld_mid == R.C + 8

    def gap(outs):
        outs["mid"].payload.view(cs.M, cs.ld_mid)[7, R.C + 1] = 0.0
    with pytest.raises(AssertionError) as e:
        _run(cs, tamper=gap)
    assert e.value.args[0][:2] == (cs.name, "mid")
    # ff_rows with the residual in the accumulator must not touch mid_out at all
    cm = BY_NAME["chain_pre_g0.37_-0.6"]

    def mid(outs):
        outs["mid"].payload[11] = 1.0
    with pytest.raises(AssertionError) as e:
        _run(cm, tamper=mid)
    assert e.value.args[0][:2] == (cm.name, "mid")


def test_round_stage_and_statistics_terms():
    """round_stage bounds the difference of two roundings; the one-pass statistics term grows as the issue says (a multiple of
    u C (mean^2 + var)) and covers fp32 on rows 32 standard deviations from zero."""
    g = torch.Generator().manual_seed(5)
    v = torch.randn(20000, generator=g, dtype=torch.float64) * 3
    for e in (1e-7, 1e-4, 1e-2):
        d = (torch.rand(20000, generator=g, dtype=torch.float64) * 2 - 1) * e
        r, bound = R.round_stage(v, e)
        assert bool(((R.bf_round(v + d) - r).abs() <= bound).all())
        assert float((bound == 0).double().mean()) > (0.9 if e <= 1e-4 else 0.0)
    for mean in (0.0, 8.0, 32.0):
        x = ((torch.randn(64, R.C, generator=g) + mean) * 1.5).bfloat16()
        xh, e_x = R.ln_stage(x.double(), 0.0)
        assert bool(((R._ln32(x.float()).double() - xh).abs() <= e_x + 2.0 ** -8 * xh.abs()).all()), mean
        print(f"[ffn_rows] statistics term at mean {mean:g} sigma: max e_x = {float(e_x.max()):.2e}")
