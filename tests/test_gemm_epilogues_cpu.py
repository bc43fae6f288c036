"""What tests/test_gemm_epilogues_gpu.py runs and how it judges, held without a GPU.

The list of plans (tests/golden/gemm_epilogues.json) is what the planner of the day answers (tests/gemm_plan_main.hip built with the
address and undefined-behaviour sanitizers on the host code); the problems reach the kernels and branches they were chosen for; the
checker (gemm_epilogues_ref.check_output, the function the GPU child judges with) accepts the float64 reference rounded to the output
type at every problem and refuses each planted defect; the new entry points are declared, exported and bound; and the divide-free
m / rows_per_b that gemm_validate prepares for the epilogues' div_rpb is exact where the kernels use it."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gemm_candidates_ref as R
import gemm_epilogues_ref as E
from helpers import ROOT


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return R.build_planner(tmp_path_factory.mktemp("gemm_epilogues") / "gemm_plan_main")


def test_fixture_is_what_the_planner_says_today(planner):
    want = R.dump_fixture(R.fixture_payload(R.ask_planner(planner, E.PROBLEMS), E.PROBLEMS, E.PROVENANCE))
    have = open(E.FIXTURE).read()
    if want != have:
        a, b = json.loads(want), json.loads(have)
        diff = [pid for pid, i in a["problems"].items() if pid not in b["problems"] or a["answers"][i] != b["answers"][b["problems"][pid]]]
        pytest.fail(f"tests/golden/gemm_epilogues.json is stale (first differing: {diff[:5]}): python tests/gemm_epilogues_ref.py --write")
    assert os.path.getsize(E.FIXTURE) < 60_000


def _plans(p, f):
    """{(kernel name without the reduce, split)} over every launch of a problem."""
    out = {(x[-1].split(" + ")[0], x[6]) for x in f["fixed"]} | {(f["plan"][-1].split(" + ")[0], f["plan"][3])}
    amode = p["desc"].get("a_mode", 0)
    qkv = "true" if p["op"] == "range" else "false"
    return out | {(f"gemm_u_kernel<2, {tm}, {tn}, {amode}, 2, {qkv}>", sp) for tm, tn, sp, *_ in f["forced"]}


def test_the_list_reaches_the_edges():
    fx = E.load_fixture()
    assert set(fx) == {p["id"] for p in E.PROBLEMS} and {p["group"] for p in E.PROBLEMS} == set(E.GROUPS)
    assert not set(fx) & {p["id"] for p in R.PROBLEMS}
    by_epi, families = {}, set()
    for p in E.PROBLEMS:
        f, d = fx[p["id"]], p["desc"]
        assert f["plan"][0] == 0, p["id"]
        plans = _plans(p, f)
        families |= {re.sub(r"<2, \d, \d, (\d), 2, (\w+)>", r"<\1,\2>", n) if n.startswith("gemm_u") else n.split("<")[0] for n, _ in plans}
        epi = ("gn_" + p["args"]["extra"]) if p["op"] == "gnconv" else "nchw" if d.get("e_mode") == 3 else "heads" if p["op"] == "range" else \
            "bias2" if d.get("bias2") else p["args"]["epi"]
        by_epi.setdefault(epi, set()).update(plans)
    # conv_halo_kernel, gemm_u_kernel in its conv, row and head-layout instantiations, gemm_wide_kernel and gemm_glds_kernel
    assert families == {"conv_halo_kernel", "gemm_u_kernel<1,false>", "gemm_u_kernel<0,false>", "gemm_u_kernel<0,true>", "gemm_wide_kernel", "gemm_glds_kernel"}, families
    assert set(by_epi) == {"gate", "remap", "gelu", "quick_gelu", "bias2", "nchw", "heads", "gn_bias2", "gn_res"}
    # every epilogue unsplit and split: the kernel's own epilogue and the matching branch of splitk_reduce_kernel
    # (the head layouts are never split: gemm_plan.hip feasible())
    for epi, plans in by_epi.items():
        assert {sp > 1 for _, sp in plans} == ({False} if epi == "heads" else {True, False}), epi
    fam = lambda epi: {n.split("<")[0] for n, _ in by_epi[epi]}       # noqa: E731
    assert fam("gate") == {"gemm_u_kernel", "gemm_wide_kernel", "gemm_glds_kernel"}
    assert fam("bias2") == {"gemm_u_kernel", "conv_halo_kernel", "gemm_glds_kernel"}
    assert fam("nchw") == {"gemm_glds_kernel"} and fam("gn_bias2") == fam("gn_res") == {"conv_halo_kernel"}
    for fam_name in ("gemm_u_kernel", "gemm_wide_kernel", "gemm_glds_kernel"):
        assert {sp > 1 for n, sp in by_epi["gate"] if n.startswith(fam_name)} == {True, False}, fam_name
    for fam_name in ("gemm_u_kernel", "conv_halo_kernel"):
        assert {sp > 1 for n, sp in by_epi["bias2"] if n.startswith(fam_name)} == {True, False}, fam_name
    assert {n for n, _ in by_epi["gate"] if "glds" in n} == {f"gemm_glds_kernel<{t}, 0>" for t in ("128x128", "128x64", "64x64")}
    assert {n for n, _ in by_epi["nchw"]} == {"gemm_glds_kernel<128x32, 1>"}
    # the wide kernel's splits and item orders, the halo kernel's fixed splits (5 chunks as 2, 2, 1)
    assert {(x[1], x[2], x[6]) for x in fx["gate0.37_256x1280x1280"]["fixed"]} == {(s, o, s) for s in (1, 2, 3, 5) for o in (0, 1)}
    assert {(x[0], x[6], x[14]) for x in fx["b2conv_2x32x32_320+0to160"]["fixed"]} == {(1, 1, 5), (2, 2, 3), (3, 3, 2), (64, 5, 1)}
    assert {(x[0], x[6]) for x in fx["gnconv_2x32x32_128+64to160_bias2"]["fixed"]} == {(1, 1), (2, 2), (3, 3), (64, 3)}
    # rows_per_b below the rows of a tile (two samples in a 128-row tile) and not a power of two
    rpb = {p["desc"]["rows_per_b"]: p for p in E.PROBLEMS if p["desc"].get("bias2") and p["op"] == "conv"}
    assert 64 in rpb and any(tm * 32 > 64 for tm, *_ in fx[rpb[64]["id"]]["forced"])
    assert 240 in rpb and 240 & 239 and rpb[240]["desc"]["M"] % 128
    # the head layout's unsplit tiles (no 128 x 160 tile), both V^T forms, d = 40 and 80
    for p in E.PROBLEMS:
        if p["op"] == "range":
            assert {tuple(x[:3]) for x in fx[p["id"]]["forced"]} == {(4, 4, 1), (2, 5, 1), (2, 4, 1), (2, 2, 1)}, p["id"]
    lays = {(E.range_layout(p["args"]["C"], 8, p["args"]["tok_off"] + 64).d, E.range_layout(p["args"]["C"], 8, p["args"]["tok_off"] + 64).vt_perm32)
            for p in E.PROBLEMS if p["op"] == "range"}
    assert lays == {(40, 0), (40, 1), (80, 0), (80, 1)}


# ---------------------------------------------------------------------------------------------------------------- the checker
@pytest.fixture(scope="module")
def cases():
    """One case per problem on the CPU, made once and left unchanged (same inputs as on the device: the seeds are fixed)."""
    made = {}

    def get(pid):
        if pid not in made:
            made[pid] = E.make_case({p["id"]: p for p in E.PROBLEMS}[pid], "cpu")
        return made[pid]
    return get


def _verdict(before, after, want):
    out = []
    for name, (ref, bound, mask, exact) in want.items():
        out += E.check_output(after[name], before[name], ref, bound, mask, exact)[0]
    return out


@pytest.mark.parametrize("pid", [p["id"] for p in E.PROBLEMS])
def test_the_rounded_reference_passes(cases, pid):
    fx = E.load_fixture()[pid]
    splits = sorted({x[2] for x in fx["forced"]} | {x[6] for x in fx["fixed"]} | {fx["plan"][3]})
    for sp in (splits[0], splits[-1]):
        sims = E.simulate(cases(pid), sp)
        assert sims
        for before, after, want in sims:
            assert not _verdict(before, after, want), pid
            for ref, bound, mask, _ in want.values():
                assert bool(mask.any()) and bool((bound[mask] > 0).all()) and bool(torch.isfinite(bound).all())


def _planted(cases, pid, other_prob=None, edit=None, step=-1):
    """The verdict on an output that is right except for a defect: the simulation of `other_prob` (the same problem with one argument
    changed), or `edit(after)` applied to the correct one, judged against the unchanged problem."""
    before, after, want = E.simulate(cases(pid))[step]
    assert not _verdict(before, after, want)
    if other_prob is not None:
        after = E.simulate(E.make_case(other_prob, "cpu"))[step][1]
    else:
        after = {n: t.clone() for n, t in after.items()}
        edit(after)
    return _verdict(before, after, want)


def _prob(pid, **args):
    p = {q["id"]: q for q in E.PROBLEMS}[pid]
    return dict(p, args=dict(p["args"], **args))


def test_planted_bias2_of_the_neighbouring_sample(cases):
    pid = "b2conv_4x8x8_128+0to192"
    b2 = cases(pid)["parts"]["bias2"].view(4, -1)

    def edit(after):   # rows 112 .. 127 of every 128-row tile (the second of its two samples) take the first sample's bias
        y = after["out"].double().view(4, 64, -1)
        for b in (1, 3):
            y[b, 48:] += b2[b - 1] - b2[b]
        after["out"] = y.view(256, -1).bfloat16()
    assert any("err / bound" in f for f in _planted(cases, pid, edit=edit))


def test_planted_gate_treated_as_one(cases):
    for pid in ("gate0.37_100x320x640", "gate0.0_100x320x640", "gate0.37_100x64x1024"):
        found = _planted(cases, pid, other_prob=_prob(pid, gate=1.0))
        assert any("err / bound" in f for f in found), pid
    assert any("not the bits" in f for f in _planted(cases, "gate0.0_100x320x640", other_prob=_prob("gate0.0_100x320x640", gate=1.0)))


def test_planted_remap_offset_off_by_one_row(cases):
    pid = "remap_90x768x512_30to64"
    for step, offs in ((0, (1, 30)), (1, (0, 31))):
        found = _planted(cases, pid, other_prob=_prob(pid, offs=offs), step=step)
        assert any("outside the written range" in f for f in found) and any("err / bound" in f or "NaN" in f for f in found)

    def edit(after):   # the second launch also rewrites a row of the first range with the same values rounded differently
        after["out"][5] = (after["out"][5].float() * (1 + 2.0 ** -7)).bfloat16()
    assert any("outside the written range" in f for f in _planted(cases, pid, edit=edit, step=1))


def test_planted_channel_n_real_written(cases):
    pid = "nchw_2x16x16_128+0to3"

    def edit(after):   # channel 3 of sample 0 stored behind its three planes: on plane 0 of sample 1
        after["out"][1, 0, :] = 0.125
    assert _planted(cases, pid, edit=edit)
    # ... and of the last sample: behind the buffer, which the child's guard zones hold
    from gemm_candidates_ref import GUARD
    assert GUARD >= 64


def test_planted_tok_off_dropped(cases):
    pid = "range_3x64+64_C320"
    case = cases(pid)
    before, after, want = E.simulate(case)[-1]
    wrong = case["expect_at"](1, tok_off=0)
    bad = {n: torch.where(wrong[n][2], wrong[n][0].to(before[n].dtype), before[n]) for n in before}
    found = _verdict(before, bad, want)
    assert sum("outside the written range" in f for f in found) == 3 and sum("err / bound" in f for f in found) == 3, "q, k and v^T each"


def test_planted_gelu_in_place_of_quick_gelu(cases):
    for pid, other in (("quick_gelu_100x384x640", "gelu"), ("gelu_100x384x640", "quick_gelu")):
        assert any("err / bound" in f for f in _planted(cases, pid, other_prob=_prob(pid, epi=other)))


# ---------------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_are_declared_exported_and_bound():
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    header = open(os.path.join(ROOT, "include", "gligen_amd_gemm_plans.h")).read()
    declared = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", header))
    assert {"gl_op_gemm_epilogue", "gl_op_attention_project_range"} <= declared == set(_lib.GEMM_PLAN_SYMBOLS)
    public = open(os.path.join(ROOT, "include", "gligen_amd.h")).read()
    assert "gl_op_gemm_epilogue" not in public and "gl_op_attention_project_range" not in public
    lib = _lib.load()
    # the struct of the binding is the header's, field by field
    body = re.search(r"typedef struct gl_gemm_epilogue_args \{(.*?)\} gl_gemm_epilogue_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().lstrip("*").strip() for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?(unsigned|int|void\s*\*|float\s*\*)", "", decl.strip()).split(",")]
    assert names == [f for f, _ in _lib.GemmEpilogueArgs._fields_]
    # without a context nothing is launched: an error code and its message
    g = _lib.GemmEpilogueArgs()
    g.struct_size = ctypes.sizeof(g)
    assert lib.gl_op_gemm_epilogue(None, ctypes.byref(g), None) == 2 and b"null context" in lib.gl_last_error()
    lay = _lib.AttnProjLayout()
    assert lib.gl_op_attention_project_range(None, None, 1, 64, 64, 320, 8, None, None, None, None, None, None, None, ctypes.byref(lay), None) == 2


# ---------------------------------------------------------------------------------------------------------------- div_rpb
def test_div_rpb_of_the_host_code_is_exact(planner):
    """(umulhi(m, magic) + m) >> shift == m // d with the pair gemm_validate fills, around every multiple of d that is reached here:
    the first 2048 and the last 2048 below 2^31, the multiples next to every power of two, and 1024 more spread evenly."""
    ds = list(range(1, 4097)) + [16384, 65536]
    r = subprocess.run([str(planner), "rpb"], input="\n".join(map(str, ds)) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert [x[0] for x in rows] == ds
    top = 2 ** 31 - 1
    for d, magic, shift in rows:
        assert 0 < magic < 2 ** 32 and 0 <= shift <= 16 and (1 << shift) >= d > (1 << shift) // 2
        kmax = top // d
        ks = np.unique(np.concatenate([np.arange(0, min(2048, kmax) + 1), np.arange(max(kmax - 2048, 0), kmax + 1), np.linspace(0, kmax, 1024).astype(np.int64),
                                       *[np.array([(1 << e) // d, (1 << e) // d + 1]) for e in range(1, 32)]]))
        m = np.unique(np.concatenate([ks * d - 1, ks * d, ks * d + 1]))
        m = m[(m >= 0) & (m <= top)].astype(np.uint64)
        got = ((((m * np.uint64(magic)) >> np.uint64(32)) + m) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)      # (32-bit arithmetic, as the kernels')
        bad = np.nonzero(got != m // np.uint64(d))[0]
        assert bad.size == 0, f"rows_per_b = {d}: m = {int(m[bad[0]])} gives {int(got[bad[0]])}"
