"""Every plan the GEMM planner can choose -- tile, K split, resident grid, XCD item order, and the fixed-tile families under
their own knobs -- run by itself on the device and held to float64 (tests/gemm_candidates_ref.py: the problems, the derived bounds;
tests/golden/gemm_candidates.json: the plans, from the planner itself).

The forcing (include/gligen_amd_gemm_plans.h) is process-wide and the `engine` fixture is shared, so each group of problems runs in
a fresh child (tests/gemm_candidates_child.py), one child at a time, each under its own time limit, with GL_DEV_SWITCHES=1,
GL_GEMM_AUTOTUNE=0 and without the shipped table (its entries are among the candidates). Asserted per group:
    * one REPORT per problem; the calls it counted as having run the plan asked for, and the distinct plans it compared with float64, are
      the numbers the fixture gives: a child that ran or verified less cannot pass;
    * no PROBLEM line: every plan was taken exactly as asked (tm, tn, splits, n_items, grid = min(n_items, cap), box / rm / rz, K tiles
      per split, kernel name for the fixed families), the guard zones keep their bits, no NaN is left, err <= bound element by element,
      a second run and every other grid cap / box setting / item order of the same (family, tile, split) give the same bits;
    * group `bits`: rows [0, M / 2) of an M-row launch equal the M / 2-row launch of the same candidate (what gemm_set_plan_batch_scale
      relies on for the guidance pair's shared prefix).
    * group `heads`: gl_op_ln_linear in both modes with a random LayerNorm affine, both launches of a call checked through the log: the
      producer (row statistics in its epilogue), then the q projection with the LayerNorm folded into the head-layout epilogue (the padding
      rows and columns of the q buffer stay untouched), or the GEGLU projection -- folded in gemm_wide_kernel at M = 256 under both item
      orders, behind the LayerNorm kernel at M = 100 / 300 under every even-tn tile and split.
    * group `proj`: gl_op_attention_project, the projections of gl_op_attention into guarded q, k and v^T buffers: the fused launch
      (never split, no 128 x 160 tile, the V third with exchanged operand roles) and, as cross-attention, the q scatter, the k scatter
      into the key-tile layout and the v^T projection, every record of the log checked; q, k and v^T element by element against float64,
      and what the layouts leave unwritten (padding rows and columns) keeps its bits.
Bit-equality across different tiles or splits is printed (distinct patterns per problem), not asserted.
If a child ends by a signal or at its time limit the remaining tests of the module skip: that is a finding to be read from the code,
not to be run again. profiles/gemm_candidates/ keeps the tables of one run."""
import os
import subprocess
import sys
import time

import pytest

import gemm_candidates_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TIME_LIMIT = 240
_dead = []      # the group whose child ended by a signal or at its time limit


def run_child(group):
    env = dict(os.environ, GL_DEV_SWITCHES="1", GL_GEMM_AUTOTUNE="0", GL_GEMM_NO_TABLE="1")
    for k in list(env):
        if k.startswith(("GL_GEMM_", "GL_CONV_HALO", "GL_WIDE_XCD", "GL_QKV_FUSED", "GL_UPCONV_PHASES")) and k not in ("GL_GEMM_AUTOTUNE", "GL_GEMM_NO_TABLE"):
            env.pop(k)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "gemm_candidates_child.py"), group], env=env, capture_output=True, text=True, timeout=TIME_LIMIT)
    except subprocess.TimeoutExpired as e:
        _dead.append(group)
        pytest.fail(f"group {group}: no end after {TIME_LIMIT} s\n{(e.stdout or b'')[-2000:]}")
    if r.returncode < 0:
        _dead.append(group)
    assert r.returncode == 0, f"group {group}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    reports, problems = {}, []
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "REPORT":
            assert w[1] not in reports, line
            reports[w[1]] = dict(launches=int(w[2]), keys=int(w[3]), worst=float(w[4]), worst_key=w[5], patterns=int(w[6]))
        elif w and w[0] == "PROBLEM":
            problems.append(line)
    print(f"[gemm candidates] group {group}: {len(reports)} problems, {sum(v['launches'] for v in reports.values())} launches ({time.time() - t0:.1f} s with start-up)")
    for pid, v in reports.items():
        print(f"[gemm candidates] {pid:48s} {v['launches']:5d} launches {v['keys']:3d} plans  worst err/bound {v['worst']:.3f} at {v['worst_key']:22s} {v['patterns']:3d} bit patterns")
    return reports, problems


def expected(group):
    """{problem: (calls of the operator, distinct plans)} from the fixture."""
    fx = R.load_fixture()
    probs = {p["id"]: p for p in R.PROBLEMS if p["group"] == group}
    plan = lambda e: (e["tm"], e["tn"], e["splits"])                                                      # noqa: E731
    out = {}
    for pid, p in probs.items():
        if p["op"] in ("part", "lnp") or (group == "bits" and "pair" not in p):
            continue
        if group == "bits":
            n = len(R.pair_launches(p, fx[pid], probs[p["pair"]], fx[p["pair"]]))
            out[pid] = (2 * n, n)
        elif p["op"] == "proj":
            ls = R.proj_launches(p, fx)
            part = (0, 0, 0) if len(p["parts"]) == 1 else (0, 1, 2)
            out[pid] = (len(ls), len({(i, plan(l["expect"][i])) for l in ls for i in part}) if len(p["parts"]) > 1 else 3 * len({plan(l["expect"][0]) for l in ls}))
        elif p["op"] in ("lnq", "lng"):
            ls = R.head_launches(p, fx[pid], fx[p["producer"]]) if p["op"] == "lnq" else R.lng_launches(p, fx)
            out[pid] = (len(ls), len({(plan(l["expect"][0]), plan(l["expect"][1])) for l in ls}))
        else:
            ls = R.launches(p, fx[pid])
            out[pid] = (len(ls), len({l["key"] for l in ls}))
    return out


@pytest.mark.parametrize("group", R.GROUPS)
def test_every_listed_plan(group):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    if _dead:
        pytest.skip(f"the child of group {_dead[0]} ended by a signal or at its time limit: nothing more is started")
    want = expected(group)
    assert want and min(min(v) for v in want.values()) > 0
    reports, problems = run_child(group)
    assert {k: (v["launches"], v["keys"]) for k, v in reports.items()} == want
    assert not problems, f"{len(problems)} findings; first: {problems[:5]}"
    assert all(v["worst"] <= 1.0 for v in reports.values())
