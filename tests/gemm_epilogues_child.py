"""Child process of test_gemm_epilogues_gpu.py (the forcing of include/gligen_amd_gemm_plans.h is process-wide): one group of
tests/gemm_epilogues_ref.py PROBLEMS, every launch tests/golden/gemm_epilogues.json lists for it.

A launch is the problem's steps in order (one call of the operator each: two for the row remap, whose second call writes the second
range of rows into the same buffer; two for the second token range, whose first call is gl_op_attention_project). Every buffer lies
between guard zones and starts as NaN (q, k, v^T: as 7). Per step the plan log has to show the plan that was asked for. The first
launch of a key (kernel family, tile, split) is held to float64 by gemm_epilogues_ref.check_output step by step -- inside the written
range err <= bound and no NaN, outside it the bits from before the call, gate = 0 the residual's own bits -- run a second time for the
same bits, and kept; every other launch of the key has to give its bits.
    REPORT <problem> <launches that ran the plan asked for, second runs not counted> <keys> <worst err/bound> <its key>
           <distinct bit patterns over the keys>
    DETAIL <problem> <key> <err/bound>
    PROBLEM <problem> <what>"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import torch  # noqa: E402

import gemm_epilogues_ref as E  # noqa: E402
from gemm_candidates_child import Out, apply, say, what  # noqa: E402
from gligen_amd.engine import Engine  # noqa: E402


def run_launch(eng, prob, case, l, outs, verify):
    """All steps of one launch. (what the plan log says against l["expect"], findings of check_output, worst err / bound)."""
    apply(eng, prob, l)
    for o in outs.values():
        o.reset()
    views = {n: o.view for n, o in outs.items()}
    bad, findings, worst = [], [], 0.0
    for i, step in enumerate(case["steps"]):
        before = {n: o.view.clone() for n, o in outs.items()} if verify and step["expect"] else None
        eng.gemm_plan_log_clear()
        E.run_step(eng, prob, case, step, views)
        if step["expect"] is None:
            continue
        recs, n = eng.gemm_plan_log()
        if n != 1:
            bad.append(f"step {i}: {n} GEMM launches instead of one")
            continue
        bad += [f"step {i} {k}: asked {v!r}, ran {recs[-1][k]!r}" for k, v in l["expect"].items() if recs[-1][k] != v]
        if "force" in l and recs[-1]["family"] not in (1, 2):
            bad.append(f"step {i}: family {recs[-1]['family']}")
        if before is not None and not bad:
            for name, (ref, bound, mask, exact) in step["expect"](l["expect"]["splits"]).items():
                f, ratio = E.check_output(outs[name].view, before[name], ref, bound, mask, exact)
                findings += [f"step {i} {name}: {x}" for x in f]
                worst = max(worst, ratio) if ratio == ratio else ratio
    return bad, findings, worst


def run_problem(eng, prob, fx):
    pid = prob["id"]
    case = E.make_case(prob, eng.device)
    outs = {n: Out(shape, dtype, eng.device, fill=fill) for n, (shape, dtype, fill) in case["bufs"].items()}
    bits = lambda: torch.cat([o.bits.view(torch.uint8) for o in outs.values()])      # noqa: E731
    first, worst, hashes, done = {}, (0.0, "-"), set(), 0
    for l in E.launches(prob, fx):
        key = l["key"]
        bad, findings, ratio = run_launch(eng, prob, case, l, outs, key not in first)
        if bad:
            say("PROBLEM", pid, what(l), "plan not taken:", "; ".join(bad))
            continue
        done += 1
        if key in first:
            if not torch.equal(bits(), first[key]):
                say("PROBLEM", pid, what(l), f"bits differ from the first launch of {key} (or a guard zone changed)")
            continue
        if not all(o.guards_ok() for o in outs.values()):
            say("PROBLEM", pid, what(l), "a guard zone changed")
        for f in findings:
            say("PROBLEM", pid, what(l), f)
        say("DETAIL", pid, key, repr(ratio))
        if worst[0] == worst[0] and not worst[0] >= ratio:      # (a NaN stays the worst)
            worst = (ratio, key)
        first[key] = bits().clone()
        hashes.add(hash(first[key].cpu().numpy().tobytes()))
        bad = run_launch(eng, prob, case, l, outs, False)[0]
        if bad or not torch.equal(bits(), first[key]):
            say("PROBLEM", pid, what(l), "a second run gives other bits")
    say("REPORT", pid, done, len(first), repr(worst[0]), worst[1], len(hashes))


if __name__ == "__main__":
    group = sys.argv[1]
    fixture = E.load_fixture()
    eng = Engine(0, arena_gb=1.0)
    t0 = time.time()
    probs = [p for p in E.PROBLEMS if p["group"] == group]
    if not probs:
        sys.exit(f"unknown group {group!r}")
    for p in probs:
        run_problem(eng, p, fixture[p["id"]])
    eng.gemm_force_clear()
    torch.cuda.synchronize()
    say("TIME", group, f"{time.time() - t0:.1f}")
    eng.close()
