"""The list of plans tests/test_gemm_candidates_gpu.py runs comes from the planner itself and cannot go stale (no GPU needed).

tests/gemm_plan_main.hip, mode `candidates`, is built with the address and undefined-behaviour sanitizers on the host code and asked
for every problem of tests/gemm_candidates_ref.py: its answer has to be tests/golden/gemm_candidates.json. The list has to reach the
edges it was chosen for, and the entry points of include/gligen_amd_gemm_plans.h have to be declared, exported, bound and strict."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import gemm_candidates_ref as R
from helpers import ROOT


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return R.build_planner(tmp_path_factory.mktemp("gemm_candidates") / "gemm_plan_main")


def test_fixture_is_what_the_planner_says_today(planner):
    want = R.dump_fixture(R.fixture_payload(R.ask_planner(planner)))
    have = open(R.FIXTURE).read()
    if want != have:
        a, b = json.loads(want), json.loads(have)
        diff = [pid for pid, i in a["problems"].items() if pid not in b["problems"] or a["answers"][i] != b["answers"][b["problems"][pid]]]
        pytest.fail(f"tests/golden/gemm_candidates.json is stale (first differing: {diff[:5]}): python tests/gemm_candidates_ref.py --write")
    assert os.path.getsize(R.FIXTURE) < 60_000


def test_the_list_reaches_the_edges():
    fx = R.load_fixture()
    assert set(fx) == {p["id"] for p in R.PROBLEMS}
    names = set()
    for p in R.PROBLEMS:
        f, d = fx[p["id"]], p["desc"]
        assert f["plan"][0] == 0, p["id"]
        names |= {f["plan"][-1].split(" + ")[0]} | {x[-1].split(" + ")[0] for x in f["fixed"]}
        forced = {tuple(x[:3]) for x in f["forced"]}
        assert {tuple(x[:3]) for x in f["tune"] + f["tune_corun"]} <= forced, f"{p['id']}: every candidate of the tuner can be forced"
        fam = f["plan"][-1].split("<")[0]
        if fam in ("gemm_u_kernel", "gemm_p_kernel"):
            assert f["tune"] and tuple(f["plan"][1:4]) in forced, p["id"]
        folded_geglu = d.get("act") == 2 and d.get("ln_stats")      # (that fold exists in gemm_wide_kernel only: no tile can be forced)
        assert (fam == "gemm_glds_kernel" or bool(folded_geglu)) == (not forced), p["id"]
        assert len(R.launches(p, f)) == 8 * len(forced) + 2 * sum(len({c[3] for c in f["tune"] + f["tune_corun"] if c[:3] == list(k)} - {512}) for k in forced) + len(f["fixed"]) + 1
        if d.get("act") == 2:
            assert all(tn % 2 == 0 for _, tn, _ in forced), "GEGLU: even tn only"
        if d["K"] == 128:
            assert all(sp == 1 for _, _, sp in forced), "nk = 2: no split"
    # all five families, gemm_glds_kernel's four tiles and its split rule, the phase form of the upsample conv
    assert {n.split("<")[0] for n in names} == {"gemm_glds_kernel", "gemm_u_kernel", "conv_halo_kernel", "gemm_wide_kernel"}
    assert {n for n in names if n.startswith("gemm_glds")} == {f"gemm_glds_kernel<{t}, 0>" for t in ("128x128", "128x64", "64x64", "128x32")} | {"gemm_glds_kernel<128x64, 1>"}
    assert {fx[p["id"]]["plan"][3] > 1 for p in R.PROBLEMS if p["desc"]["N"] < 128} == {True, False}
    assert any("gemm_u_kernel<2, 2, 4, 2, 2, false>" == fx[p["id"]]["plan"][-1] for p in R.PROBLEMS)
    # a last K split shorter than the others: nk = 10 as 4, 4, 2 and as 3, 3, 3, 1
    f = {tuple(x[:3]): x for x in fx["lin_100x320x640_plain"]["forced"]}
    assert f[(2, 4, 3)][7] == 4 and f[(2, 4, 4)][7] == 3 and f[(2, 4, 5)][7] == 2
    assert max(x[2] for x in fx["lin_333x960x1536_plain"]["forced"]) == 12 and max(x[2] for x in fx["lin_64x1280x4096_plain"]["forced"]) == 32
    # every way to spread the 8 XCDs over (M tiles, N tiles, K splits) -- the ten (lgm, lgn, lgz) with sum 3 -- and launches without boxes
    boxes = {(x[4] & 15, x[4] >> 4, x[2] // x[6]) for p in fx.values() for x in p["forced"] if x[4] >= 0}
    assert boxes == {(m, n, 1 << (3 - m - n)) for m in range(4) for n in range(4 - m)}, boxes
    assert {x[4] & 15 for x in fx["lin_1024x256x640_plain"]["forced"] if x[4] >= 0} == {1, 2, 3}
    assert any(x[4] < 0 for p in fx.values() for x in p["forced"])
    assert any(x[3] % 8 for p in fx.values() for x in p["forced"]), "n_items % 8 != 0"
    # the halo kernel's splits (5 chunks as 2, 2, 1) and the wide kernel's splits and item orders
    halo = {(x[0], x[6], x[14]) for x in fx["conv_2x32x32_320+0to160_s1u0p1"]["fixed"]}
    assert halo == {(1, 1, 5), (2, 2, 3), (3, 3, 2), (64, 5, 1)}, halo
    assert {(x[1], x[6]) for x in fx["lin_256x1280x1280_plain"]["fixed"]} == {(1, 1), (2, 2), (3, 3), (5, 5)}
    assert {(x[2], x[13]) for x in fx["lin_8192x1280x64_plain"]["fixed"]} == {(0, 0), (1, 1)}, "256 items: GL_WIDE_XCD decides the item order"
    probs = {p["id"]: p for p in R.PROBLEMS}
    # more items than the 256 workgroups of the halo and the wide kernel: their loops over items
    for pid in ("conv_8x32x32_320+0to320_s1u0p1", "lin_2048x1280x1280_plain"):
        d = probs[pid]["desc"]
        assert any(x[6] * (d["M"] // 256) * (d["N"] // (32 * x[5])) > 256 == x[8] for x in fx[pid]["fixed"]), pid
    # the pairs of the prefix test have candidates in common
    pairs = [p for p in R.PROBLEMS if "pair" in p]
    assert len(pairs) == 4 and all(len(R.pair_launches(p, fx[p["id"]], probs[p["pair"]], fx[p["pair"]])) >= 9 for p in pairs)


def test_force_clear_restores_the_defaults(planner):
    def run(**env):
        r = subprocess.run([str(planner), "force_clear"], capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        return [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    env = {k: "" for k in os.environ if k.startswith("GL_")}
    assert run(GL_DEV_SWITCHES="0", **{k: v for k, v in env.items() if k != "GL_DEV_SWITCHES"}) == [[2, 4, 3, 7, 2, 3, 1, 0, 4, 2], [0, 0, 0, 0, 0, 0, -1, 1, 8, 1]]
    got = run(GL_DEV_SWITCHES="1", GL_GEMM_XCD_BOXES="0", GL_CONV_HALO_SPLITS="3", GL_GEMM_WIDE="2")
    assert got[1] == [0, 0, 0, 0, 3, 0, -1, 0, 8, 2], "with GL_DEV_SWITCHES=1: back to what the environment says"


def test_entry_points_are_declared_exported_bound_and_strict():
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    header = open(os.path.join(ROOT, "include", "gligen_amd_gemm_plans.h")).read()
    declared = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.GEMM_PLAN_SYMBOLS) == {"gl_gemm_force_plan", "gl_gemm_force_knobs", "gl_gemm_force_clear", "gl_gemm_plan_log_clear", "gl_gemm_plan_log",
                                                           "gl_op_attention_project", "gl_op_attention_project_range", "gl_op_gemm_epilogue"}
    assert not declared & set(_lib.SYMBOLS)
    lib = _lib.load()
    fields = re.search(r"typedef struct gl_gemm_plan_record \{(.*?)\} gl_gemm_plan_record;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip().split("[")[0] for decl in fields.split(";") if decl.strip() for n in decl.replace("char", "").replace("int", "").split(",")]
    assert names == [f for f, _ in _lib.GemmPlanRecord._fields_] and ctypes.sizeof(_lib.GemmPlanRecord) == 96 + 4 * 14
    try:
        for bad in [(3, 3, 1, 0), (4, 5, 33, 0), (4, 5, -1, 0), (2, 2, 1, -1), (0, 4, 1, 0)]:
            assert lib.gl_gemm_force_plan(*bad) == 2 and b"gl_gemm_force_plan" in lib.gl_last_error(), bad
        for bad in [(-1, 0, -1, 1, 8, 1), (0, 0, 2, 1, 8, 1), (0, 0, -1, 2, 8, 1), (0, 0, -1, 1, -1, 1), (0, 0, -1, 1, 8, 3)]:
            assert lib.gl_gemm_force_knobs(*bad) == 2, bad
        for ok in [(4, 5, 1, 0), (4, 4, 32, 7), (2, 5, 0, 1024), (2, 4, 5, 3), (2, 2, 12, 1), (0, 0, 0, 128)]:
            assert lib.gl_gemm_force_plan(*ok) == 0, ok
        assert lib.gl_gemm_force_knobs(64, 5, 1, 0, 0, 2) == 0
        # the log of a thread that has launched nothing
        recs, n, total = (_lib.GemmPlanRecord * 32)(), ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.gl_gemm_plan_log_clear() == 0 and lib.gl_gemm_plan_log(recs, 32, ctypes.byref(n), ctypes.byref(total)) == 0
        assert (n.value, total.value) == (0, 0)
        assert lib.gl_gemm_plan_log(None, 32, ctypes.byref(n), ctypes.byref(total)) == 2
    finally:
        assert lib.gl_gemm_force_clear() == 0
