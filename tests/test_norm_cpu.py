"""norm_ref by itself, without a GPU: the entry points' declaration, the case list against the kernels' preconditions and every path
and edge it has to reach (by the transcribed launch geometry), the sharpness of the bound from the reference alone, the fp32 twin of
the kernels within the bound on every case, and ten seeded faults the check has to reject."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import gemm_candidates_ref as G
import norm_ref as N

ROOT = G.ROOT
BY_NAME = {c.name: c for c in N.CASES}


def test_entry_points_are_declared_exported_and_bound(tmp_path):
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    header = open(os.path.join(ROOT, "include", "gligen_amd_norm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(gl_op_[a-z0-9_]+)\s*\(", code)) == set(_lib.NORM_SYMBOLS) == {"gl_op_groupnorm_coef", "gl_op_layernorm_rows"}
    assert not set(_lib.NORM_SYMBOLS) & set(_lib.SYMBOLS)
    body = re.search(r"typedef struct gl_layernorm_rows_args \{(.*?)\} gl_layernorm_rows_args;", code, flags=re.S).group(1)
    names = [re.findall(r"[A-Za-z_0-9]+", piece)[-1] for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    assert names == [n for n, _ in _lib.LayerNormRowsArgs._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "gligen_amd_norm.h"\nint main(void) { printf("%zu\\n", sizeof(gl_layernorm_rows_args)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout) == ctypes.sizeof(_lib.LayerNormRowsArgs)
    lib = _lib.load()
    assert lib.gl_op_groupnorm_coef(None, None, 0, None, 0, 0, 0, None, None, 0.0, None, None, None) == 2          # no context
    assert lib.gl_op_layernorm_rows(None, None, None) == 2


def test_cases_reach_every_path_and_edge():
    gn, ln = N.GN_CASES, N.LN_CASES
    geo = {c.name: N.gn_geometry(c.B, c.HW, c.C0 + c.C1) for c in gn}
    path = {c.name: N.gn_path(c.HW, c.C0, c.C1) for c in gn}
    for c in gn:
        assert N.gn_refusal(c.C0, c.C1) is None, c.name
        assert c.B * c.HW * (c.C0 + c.C1) * 2 < 100e6, (c.name, "a tensor above 100 MB")
        g = geo[c.name]
        if path[c.name] == "two_pass":          # the grids cover every pixel exactly once, and the block is launchable
            assert g.T <= 1024 and g.T >= 32 and (g.nsplit - g.empty - 1) * g.per < c.HW <= (g.nsplit - g.empty) * g.per
            assert g.aper % g.R == 0 and (g.agrid - 1) * g.aper < c.HW <= g.agrid * g.aper
    tp = [c for c in gn if path[c.name] == "two_pass"]
    sm = [c for c in gn if path[c.name] != "two_pass"]
    cpg = lambda c: (c.C0 + c.C1) // 32
    # the issue's table, by what each row reaches
    assert any(path[c.name] == "small256" and c.HW * cpg(c) // 4 < 64 for c in sm), "small256 with almost all threads idle"
    assert any(c.HW == 1 for c in sm)
    assert any(path[c.name] == "small256" and c.HW == 45 for c in sm) and any(path[c.name] == "small256" and c.HW == 180 and cpg(c) == 4 for c in sm)
    assert {c.C1 > 0 for c in sm if path[c.name] == "small1024"} == {True, False}
    assert any(c.C1 and c.C0 % cpg(c) for c in sm), "a small-form group that straddles the two sources"
    assert any(c.HW <= 256 and not c.C1 for c in tp) and any(c.HW <= 256 and c.C1 for c in tp), "two_pass at HW <= 256 because cpg % 4 != 0"
    assert any(c.HW == 257 for c in tp)
    assert {(720, 3), (2880, 6)} <= {(c.HW, geo[c.name].R) for c in tp}
    assert {6, 14} <= {cpg(c) for c in tp}, "groups that start at odd pairs inside an 8-channel chunk"
    assert any(geo[c.name].C8 >= 256 and geo[c.name].R == 1 and geo[c.name].empty > 0 for c in tp)
    e = geo["two_pass_empty_blocks"]
    assert (e.nsplit, e.per, e.empty) == (64, 9, 6) and 57 * 9 < 520 <= 58 * 9                     # blocks 58 .. 63
    assert any(geo[c.name].trips > 2048 // c.B and geo[c.name].atrips > 1 for c in tp), "several trips per apply block"
    assert any(geo[c.name].nsplit == 64 and geo[c.name].chain >= 512 for c in tp), "long per-thread chains"
    assert any(geo[c.name].per % geo[c.name].R for c in tp) and any(c.HW % geo[c.name].per for c in tp), "ragged ranges: clamped re-reads"
    assert {c.eps for c in gn} == {1e-5, 1e-6} and {c.silu for c in gn} == {0, 1} and {c.B for c in gn} >= {1, 2, 3}
    for form in ("small256", "small1024", "two_pass"):
        assert {c.silu for c in gn if path[c.name] == form} == {0, 1}, form
    for kind in ("offset", "outlier", "constant"):
        assert {path[c.name] == "two_pass" for c in gn if c.inp == kind} == {True, False}, kind
    assert any(c.C1 for c in tp) and any(c.C1 for c in sm), "poisoned two-source cases on both forms"
    assert any(c.C1 and c.C0 > c.C1 for c in gn), "a wrong row stride for source 1 reads past its end"
    # LayerNorm
    for c in ln:
        assert N.ln_refusal(c) is None, c.name
    assert {c.C for c in ln} >= {8, 96, 320, 512, 520, 768, 1280, 1536}
    assert any(c.C == 96 and c.ldy == 128 for c in ln) and any(c.C == 96 and c.ldy == 128 and c.Tpad > c.N1 + c.N2 for c in ln)
    assert {c.N2 > 0 for c in ln} == {True, False} and any(c.Tpad > c.N1 + c.N2 for c in ln) and any((c.B * c.Tpad) % 4 for c in ln)
    assert any(c.ldx > c.C and c.N2 for c in ln) and {c.affine for c in ln} == {True, False} and {c.inp for c in ln} == {"plain", "offset", "constant"}
    # the transcription refuses what the source refuses
    assert N.gn_refusal(100, 0) == 2 and N.gn_refusal(64, 0) == 5 and N.gn_refusal(124, 4) == 2 and N.gn_refusal(8256, 0) == 2 and N.gn_refusal(8192, 0) is None
    c = BY_NAME["c320_concat_pad"]
    for k, v in (("C", 324), ("C", 1544), ("Tpad", 45), ("ldx", 324), ("ldy", 312)):
        assert N.ln_refusal(type(c)(**{**vars(c), k: v})) == 2, (k, v)


SHARP = [c for c in N.CASES if c.inp not in ("offset", "outlier", "constant")]


@pytest.mark.parametrize("c", SHARP, ids=[c.name for c in SHARP])
def test_bound_is_sharp(c):
    """Beyond the final bf16 rounding the bound is at most a quarter of a bf16 ulp of the reference for 99 % of the elements: a
    condition on the reference and the bound alone, not a measurement."""
    share = N.sharp_share(c, N.make_inputs(c, "cpu"))
    print(f"[norm] {c.name}: bound <= ulp / 4 at {share:.4%} of the elements")
    assert share >= 0.99, (c.name, share)


def _run(c, defect=None, tamper=None):
    ins = N.make_inputs(c, "cpu")
    outs = N.make_outputs(c, "cpu")
    N.twin(c, ins, outs, defect)
    if tamper:
        tamper(outs)
    return N.verify(c, ins, outs)


@pytest.mark.parametrize("c", N.CASES, ids=[c.name for c in N.CASES])
def test_twin_is_within_the_bound(c):
    worst = _run(c)
    print(N.report_line(c, worst))
    if "fma_unsure" in worst:
        assert worst["fma_unsure"][0] <= 1e-3, (c.name, "the host cannot reproduce the fma at this share of the elements", worst["fma_unsure"][0])


def test_twin_rounds_somewhere():
    """The twin is an fp32 computation, not the reference again: on a long chain its statistics differ from float64's."""
    c = BY_NAME["two_pass_257"]
    worst = _run(c)
    assert worst["coef"][0] > 0, "the twin's coefficients equal the float64 reference to the last bit"


DEFECTS = [("the last pixel of a block's range dropped from the statistics", "two_pass_257", "drop_last_pixel"),
           ("a clamped re-read counted instead of zeroed", "two_pass_257", "count_reread"),
           ("hi and lo accumulators swapped at a chunk that straddles two groups", "two_pass_cpg10_64", "swap_hi_lo"),
           ("source 1 read with source 0's row stride", "two_pass_cpg30_cat_45", "src1_row_stride"),
           ("n = HW cpg from C0 in place of C", "two_pass_cpg30_cat_45", "n_from_C0"),
           ("an empty block's partial left unwritten", "two_pass_empty_blocks", "stale_empty_partial"),
           ("gamma read at c - C0 for source 1", "small_group_straddles_sources", "gamma_source_relative"),
           ("LayerNorm x2 read with ldx", "c520_ldx_concat", "x2_row_stride"),
           ("LayerNorm columns [C, ldy) of a pad row left unwritten", "c96_ldy128", "pad_row_tail_unwritten"),
           ("the coefficients' a and c halves swapped", "small_ragged_45", "swap_coef_halves")]


@pytest.mark.parametrize("what,case,defect", DEFECTS, ids=[d[2] for d in DEFECTS])
def test_seeded_faults_are_rejected(what, case, defect):
    c = BY_NAME[case]
    _run(c)
    with pytest.raises(AssertionError) as e:
        _run(c, defect)
    assert e.value.args[0][0] == case, (what, e.value.args)


def test_touched_guards_and_missing_zeros_are_rejected():
    c = BY_NAME["c96_ldy128"]

    def flip(sel):
        def tamper(outs):
            v = sel(outs)
            v.copy_((v.view(torch.int16) ^ 1).view(torch.bfloat16))      # one bit of one element
        return tamper
    for sel in (lambda o: o["y"].flat[0:1], lambda o: o["y"].flat[-1:], lambda o: o["y"].payload.view(-1, 128)[3, 96:97], lambda o: o["y"].payload.view(-1, 128)[46, 0:1]):
        with pytest.raises(AssertionError) as e:
            _run(c, tamper=flip(sel))
        assert e.value.args[0][:2] == (c.name, "y")
    g = BY_NAME["small_hw1"]
    for name in ("y", "coef"):
        def tamper(outs, name=name):
            outs[name].flat[N.GUARD - 1] = 0.0
        with pytest.raises(AssertionError) as e:
            _run(g, tamper=tamper)
        assert e.value.args[0][:2] == (g.name, name)
