"""The epilogues of the model's own GEMM / conv launches that tests/test_gemm_candidates_gpu.py does not carry -- the per-sample bias
through div_rpb, the gated residual, the row remap, GELU and quick-GELU, EPI_NCHW_F32 with n_real < N, the second token range of the
head layouts with a bias, the GroupNorm prologue with bias2 / res -- each under every plan the planner can give its launch, in every
kernel family that implements it and behind splitk_reduce_kernel, element by element against float64 (tests/gemm_epilogues_ref.py:
the problems, the derived bounds, the checker; tests/golden/gemm_epilogues.json: the plans, from the planner itself).

As in test_gemm_candidates_gpu.py each group runs in a fresh child (tests/gemm_epilogues_child.py), one at a time, under its own
time limit, with GL_DEV_SWITCHES=1, GL_GEMM_AUTOTUNE=0 and without the shipped table. Asserted per group:
    * one REPORT per problem, with the launch and plan counts the fixture gives;
    * no PROBLEM line: every plan was taken exactly as asked, the guard zones keep their bits, no NaN is left, err <= bound element
      by element, a second run and every other grid cap / box setting / item order of the same (family, tile, split) give the same bits;
      gate = 0 leaves the residual bit for bit; rows outside the remapped ranges keep their sentinel and the first range's rows their
      bits after the second range's launch; nothing outside the n_real planes is written; the second token range matches float64 while
      every other element of q, k and v^T, the first range included, keeps the bits it had;
    * worst err / bound <= 1.
test_the_entries_refuse_instead_of_launching: null pointers, a struct of another size and what gemm_validate refuses are error codes.
If a child ends by a signal or at its time limit the remaining tests of the module skip: that is a finding to be read from the code,
not to be run again. profiles/gemm_epilogues/ keeps the tables of one run."""
import os
import subprocess
import sys
import time

import pytest

import gemm_epilogues_ref as E

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TIME_LIMIT = 240
_dead = []      # the group whose child ended by a signal or at its time limit


def run_child(group):
    env = dict(os.environ, GL_DEV_SWITCHES="1", GL_GEMM_AUTOTUNE="0", GL_GEMM_NO_TABLE="1")
    for k in list(env):
        if k.startswith(("GL_GEMM_", "GL_CONV_HALO", "GL_WIDE_XCD", "GL_QKV_FUSED", "GL_UPCONV_PHASES", "GL_ATTN_V2")) and k not in ("GL_GEMM_AUTOTUNE", "GL_GEMM_NO_TABLE"):
            env.pop(k)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "gemm_epilogues_child.py"), group], env=env, capture_output=True, text=True, timeout=TIME_LIMIT)
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
    print(f"[gemm epilogues] group {group}: {len(reports)} problems, {sum(v['launches'] for v in reports.values())} launches ({time.time() - t0:.1f} s with start-up)")
    for pid, v in reports.items():
        print(f"[gemm epilogues] {pid:40s} {v['launches']:5d} launches {v['keys']:3d} plans  worst err/bound {v['worst']:.3f} at {v['worst_key']:22s} {v['patterns']:3d} bit patterns")
    return reports, problems


def expected(group):
    """{problem: (launches, distinct plans)} from the fixture."""
    fx = E.load_fixture()
    out = {}
    for p in E.PROBLEMS:
        if p["group"] == group:
            ls = E.launches(p, fx[p["id"]])
            out[p["id"]] = (len(ls), len({l["key"] for l in ls}))
    return out


@pytest.mark.parametrize("group", E.GROUPS)
def test_every_epilogue_under_every_plan(group):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    if _dead:
        pytest.skip(f"the child of group {_dead[0]} ended by a signal or at its time limit: nothing more is started")
    want = expected(group)
    assert want and min(min(v) for v in want.values()) > 0
    reports, problems = run_child(group)
    assert {k: (v["launches"], v["keys"]) for k, v in reports.items()} == want
    per_problem = {pid: sum(1 for x in problems if x.split()[1] == pid) for pid in want}
    assert not problems, f"{len(problems)} findings {({k: v for k, v in per_problem.items() if v})}; first: {problems[:5]}"
    assert all(v["worst"] <= 1.0 for v in reports.values())


def test_the_entries_refuse_instead_of_launching(engine):
    """Null pointers, a struct of another size and the combinations gemm_validate refuses come back as error codes; the plan log stays empty."""
    import ctypes
    import torch
    from gligen_amd._lib import GL_ERR_UNSUPPORTED, AttnProjLayout, GemmEpilogueArgs
    from gligen_amd.engine import _ptr, _stream
    lib, ctx, dev, st = engine.lib, engine._ctx, engine.device, _stream(engine.device)
    M, N, K = 64, 128, 64
    x, w, out = (torch.zeros(s, dtype=torch.bfloat16, device=dev) for s in ((M, K), (N, K), (M, N)))
    w9 = torch.zeros((N, K, 3, 3), dtype=torch.float32, device=dev)
    gate = torch.ones(1, dtype=torch.float32, device=dev)

    def args(**kw):
        g = GemmEpilogueArgs()
        g.struct_size = ctypes.sizeof(GemmEpilogueArgs)
        g.M, g.N, g.K, g.x0, g.w, g.out, g.ldo, g.ldres, g.rows_per_b = M, N, K, _ptr(x), _ptr(w), _ptr(out), N, N, 1
        for k, v in kw.items():
            setattr(g, k, v)
        return g
    conv = dict(conv=1, w=_ptr(w9), C0=K, B=1, H=8, W=8, stride=1, pad_lo=1)
    engine.gemm_plan_log_clear()
    assert lib.gl_op_gemm_epilogue(ctx, None, st) == 2
    for code, kw in [(2, dict(struct_size=8)), (2, dict(x0=None)), (2, dict(w=None)), (2, dict(out=None)), (2, dict(C1=64)), (2, dict(rows_per_b=0)), (2, dict(K=100)),
                     (2, dict(mode=1)), (2, dict(mode=4)), (GL_ERR_UNSUPPORTED, dict(act=3, res=_ptr(out))), (GL_ERR_UNSUPPORTED, dict(act=4, bias2=_ptr(gate))),
                     (GL_ERR_UNSUPPORTED, dict(conv, res=_ptr(out), gate=_ptr(gate))), (GL_ERR_UNSUPPORTED, dict(conv, remap_in=8, remap_out=8)),
                     (GL_ERR_UNSUPPORTED, dict(conv, act=3)), (2, dict(conv, C0=32))]:
        assert lib.gl_op_gemm_epilogue(ctx, ctypes.byref(args(**kw)), st) == code and lib.gl_last_error(), kw
    lay = AttnProjLayout()
    C, H, T = 320, 8, 128
    assert lib.gl_op_attention_project(ctx, None, None, 1, T, T, C, C, H, None, None, None, None, None, None, ctypes.byref(lay), None) == 0
    xr = torch.zeros((64, C), dtype=torch.bfloat16, device=dev)
    wq = torch.zeros((C, C), dtype=torch.float32, device=dev)
    q, k, vt = (torch.zeros(H * n, dtype=torch.bfloat16, device=dev) for n in (lay.tq_pad * lay.dp, lay.tk_pad * lay.dp, lay.dpv * lay.tk_pad))
    good = dict(x=_ptr(xr), B=1, Tr=64, tok_off=64, C=C, H=H, wq=_ptr(wq), wk=_ptr(wq), wv=_ptr(wq), bias=None, q=_ptr(q), k=_ptr(k), vt=_ptr(vt), layout=ctypes.byref(lay))
    for kw in [dict(x=None), dict(wv=None), dict(q=None), dict(k=None), dict(vt=None), dict(layout=None), dict(Tr=32), dict(Tr=0), dict(tok_off=32), dict(tok_off=-64),
               dict(tok_off=128), dict(H=7), dict(H=4), dict(B=0)]:
        a = dict(good, **kw)
        assert lib.gl_op_attention_project_range(ctx, a["x"], a["B"], a["Tr"], a["tok_off"], a["C"], a["H"], a["wq"], a["wk"], a["wv"], a["bias"], a["q"], a["k"], a["vt"],
                                                 a["layout"], st) == 2, kw
    torch.cuda.synchronize()
    assert engine.gemm_plan_log()[1] == 0, "nothing was launched"
    assert bool((out == 0).all()) and bool((q == 0).all()) and bool((k == 0).all()) and bool((vt == 0).all())
