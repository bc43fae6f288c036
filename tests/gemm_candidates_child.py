"""Child process of test_gemm_candidates_gpu.py (the forcing of include/gligen_amd_gemm_plans.h is process-wide): one group of
tests/gemm_candidates_ref.py PROBLEMS, every launch tests/golden/gemm_candidates.json lists for it.

Per launch: the plan log has to show the plan that was asked for; the output lies between guard zones and starts as NaN. The first
launch of a key (kernel family, tile, split) is compared with float64 element by element, run a second time for the same bits, and
kept; every other launch of the key -- other grid caps, XCD boxes on / off, the wide kernel's item orders -- has to give its bits.
    REPORT <problem> <calls of the operator that ran the plan asked for, second runs not counted> <keys> <worst err/bound> <its key>
           <distinct bit patterns over the keys>
    DETAIL <problem> <key> <err/bound> <max |err|>
    PROBLEM <problem> <what>
Group `heads`: gl_op_ln_linear, two launches per call (tests/gemm_candidates_ref.py head_launches).
Group `proj`: gl_op_attention_project, one fused launch or three (q, k, v^T) per call; each buffer is held to float64 by itself.
Group `bits`: rows [0, M / 2) of the M-row launch against the M / 2-row launch of the same candidate on the same rows.
    REPORT <pair> <launches> <candidates compared> 0 - 0"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import torch  # noqa: E402

import gemm_candidates_ref as R  # noqa: E402
from gligen_amd.engine import Engine  # noqa: E402

INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def say(*a):
    print(*a, flush=True)


class Out:
    """An output between two guard zones of fixed bits; reset() makes it NaN again."""

    def __init__(self, shape, dtype, dev, fill=float("nan")):
        self.fill = fill
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.empty(n + 2 * R.GUARD, dtype=dtype, device=dev)
        self.guard = (torch.arange(R.GUARD, device=dev) % 7 - 3).to(dtype)
        self.view = self.buf[R.GUARD:R.GUARD + n].view(shape)
        self.bits = self.buf.view(INT[dtype])

    def reset(self):
        self.buf[:R.GUARD] = self.guard
        self.buf[-R.GUARD:] = self.guard
        self.view.fill_(self.fill)

    def guards_ok(self):
        return torch.equal(self.buf[:R.GUARD], self.guard) and torch.equal(self.buf[-R.GUARD:], self.guard)


def apply(eng, prob, l):
    halo, wide = prob.get("halo", 8), prob.get("wide", 1)
    if "force" in l:
        eng.gemm_force_plan(*l["force"])
        eng.gemm_force_knobs(0, 0, -1, l["boxes"], halo, wide)
    else:
        hs, ws, wx = l.get("fixed", (0, 0, -1))
        eng.gemm_force_plan(0, 0, 0, 0)
        eng.gemm_force_knobs(hs, ws, wx, 1, halo, wide)


def launch(eng, prob, l, ins, out):
    """Run one launch into `out`; the list of what the plan log says against l["expect"] (empty: taken as asked)."""
    apply(eng, prob, l)
    out.reset()
    eng.gemm_plan_log_clear()
    R.run_op(eng, prob, ins, out.view)
    recs, n = eng.gemm_plan_log()
    if n != 1:
        return [f"{n} GEMM launches instead of one"]
    bad = [f"{k}: asked {v!r}, ran {recs[-1][k]!r}" for k, v in l["expect"].items() if recs[-1][k] != v]
    if "force" in l and recs[-1]["family"] not in (1, 2):
        bad.append(f"family {recs[-1]['family']}")
    return bad


def what(l):
    return f"force={l['force']} boxes={l['boxes']}" if "force" in l else f"fixed={l.get('fixed')} cap={l.get('cap', 512)}"


def run_problem(eng, prob, fx):
    pid = prob["id"]
    case = R.make_case(prob, eng.device)
    out = Out(case["shape"], case["dtype"], eng.device)
    first, worst, hashes, done = {}, (0.0, "-"), set(), 0
    ls = R.launches(prob, fx)
    weights = None
    for l in ls:
        bad = launch(eng, prob, l, case["ins"], out)
        if bad:
            say("PROBLEM", pid, what(l), "plan not taken:", "; ".join(bad))
            continue
        done += 1
        key = l["key"]
        if key in first:
            if not torch.equal(out.bits, first[key]):
                say("PROBLEM", pid, what(l), f"bits differ from the first launch of {key} (or a guard zone changed)")
            continue
        if not out.guards_ok():
            say("PROBLEM", pid, what(l), "a guard zone changed")
        ref, bound = case["ref"](l["expect"]["splits"])
        err = (out.view.double() - ref).abs()
        ratio = float((err / bound).max())
        if not ratio <= 1.0:       # (NaN included)
            say("PROBLEM", pid, what(l), f"err / bound = {ratio} ({int(torch.isnan(out.view).sum())} NaN left)")
        say("DETAIL", pid, key, repr(ratio), repr(float(err.max())))
        if not worst[0] >= ratio:
            worst = (ratio, key)
        first[key] = out.bits.clone()
        if weights is None:
            weights = torch.arange(1, out.bits.numel() + 1, device=eng.device, dtype=torch.int64) * 2654435761
        hashes.add(int((out.bits.long() * weights).sum()))
        bad = launch(eng, prob, l, case["ins"], out)
        if bad or not torch.equal(out.bits, first[key]):
            say("PROBLEM", pid, what(l), "a second run gives other bits")
    say("REPORT", pid, done, len(first), repr(worst[0]), worst[1], len(hashes))


def run_heads(eng, prob, fixture):
    """gl_op_ln_linear: x between guards against the producer's bound, then on the device's own x rows (R.lnq_ref / R.ln_fallback_ref):
    mode 1, the folded q projection, q [B H][Tpad][DP] prefilled with 7 -- token rows >= T and columns >= d keep the 7;
    mode 0, GEGLU(LN(x) W1^T + b1) [M][inner], folded in the wide kernel or, elsewhere, behind the LayerNorm kernel."""
    pid, a = prob["id"], prob["args"]
    M, C, N1, mode = a["M"], a["C"], a["N1"], a["mode"]
    case = R.make_lnq_case(prob, eng.device)
    wf, bf, e_b = case["folded"]
    x_out = Out((M, C), torch.bfloat16, eng.device)
    if mode:
        B, T, H = a["B"], a["T"], a["H"]
        d = C // H
        dp, tpad = {40: 48, 80: 80, 160: 160}[d], (T + 127) // 128 * 128
        y_out = Out((B * H, tpad, dp), torch.bfloat16, eng.device, fill=7.0)
        ls = R.head_launches(prob, fixture[pid], fixture[prob["producer"]])
    else:
        y_out = Out((M, N1 // 2), torch.bfloat16, eng.device)
        ls = R.lng_launches(prob, fixture)
    want_fold = 1 if mode or a["fold"] else 0
    first, worst, done = {}, (0.0, "-"), 0
    for l in ls:
        if "force" in l:
            eng.gemm_force_plan(*l["force"])
            eng.gemm_force_knobs(0, 0, -1, l["boxes"], 8, 1)
        else:
            eng.gemm_force_plan(0, 0, 0, l["cap"])
            eng.gemm_force_knobs(*l["fixed"], 1, 8, 1)
        x_out.reset()
        y_out.reset()
        eng.gemm_plan_log_clear()
        used = R.run_lnq(eng, prob, case["ins"], x_out.view, y_out.view)
        recs, n = eng.gemm_plan_log()
        bad = [f"{n} GEMM launches instead of two"] if n != 2 else \
            [f"{w} {k}: asked {v!r}, ran {r[k]!r}" for w, r, e in zip(("producer", "consumer"), recs, l["expect"]) for k, v in e.items() if r[k] != v]
        if used != want_fold:
            bad.append(f"used_fold = {used}")
        if bad:
            say("PROBLEM", pid, what(l), "plan not taken:", "; ".join(bad))
            continue
        done += 1
        both = torch.cat([x_out.bits, y_out.bits])
        ep, ec = l["expect"]
        key = "|".join(f"{e['tm']}x{e['tn']}/{e['splits']}" for e in (ep, ec))
        if key in first:
            if not torch.equal(both, first[key]):
                say("PROBLEM", pid, what(l), f"bits differ from the first launch of {key} (or a guard zone changed)")
            continue
        first[key] = both.clone()
        if not (x_out.guards_ok() and y_out.guards_ok()):
            say("PROBLEM", pid, what(l), "a guard zone changed")
        xr, xb = R._finish(case["acc"], (case["K0"] + 1 + (ep["splits"] if ep["splits"] > 1 else 0)) * R.U * case["S"], "res", case["res64"], False)
        rx = float(((x_out.view.double() - xr).abs() / xb).max())
        x64 = x_out.view.double()
        if mode:
            q = y_out.view.view(B, H, tpad, dp)
            if not (bool((q[:, :, T:, :] == 7).all()) and bool((q[:, :, :, d:] == 7).all())):
                say("PROBLEM", pid, what(l), "the padding of the q buffer was written")
            y = q[:, :, :T, :d].permute(0, 2, 1, 3).reshape(M, C).double()
            yr, yb = R.lnq_ref(x64, wf, bf, C, e_b=e_b)
        else:
            y = y_out.view.double()
            if a["fold"]:
                h, bh = R.lnq_ref(x64, wf, bf, C, e_b=e_b, round_out=False)
            else:
                h, bh = R.ln_fallback_ref(x64, wf, bf, e_b, C, splits=ec["splits"])
            yr, yb = R.geglu_finish(h, bh, N1 // 2)
        ry = float(((y - yr).abs() / yb).max())
        if not (rx <= 1.0 and ry <= 1.0):
            say("PROBLEM", pid, what(l), f"err / bound = {rx} (x), {ry} (y)")
        say("DETAIL", pid, key, repr(max(rx, ry)), repr(ry))
        if not worst[0] >= max(rx, ry):
            worst = (max(rx, ry), key)
    say("REPORT", pid, done, len(first), repr(worst[0]), worst[1], 0)


def run_proj(eng, prob, fixture):
    """gl_op_attention_project: q, k, v^T between guards and prefilled with 7. Per launch every part's log record; per buffer and plan the
    part took: what the layout says is written obeys the bound, everything else keeps the 7, the same plan gives the same bits."""
    pid, a = prob["id"], prob["args"]
    B, H = a["B"], a["H"]
    lay = R.proj_layout(eng, a)
    case = R.make_proj_case(prob, eng.device)
    outs = dict(q=Out((B * H * lay.tq_pad * lay.dp,), torch.bfloat16, eng.device, fill=7.0), k=Out((B * H * lay.tk_pad * lay.dp,), torch.bfloat16, eng.device, fill=7.0),
                vt=Out((B * H * lay.dpv * lay.tk_pad,), torch.bfloat16, eng.device, fill=7.0))
    part_of = dict(q=0, k=0, vt=0) if case["fused"] else dict(q=0, k=1, vt=2)
    first, worst, done = {}, (0.0, "-"), 0
    ls = R.proj_launches(prob, fixture)
    for l in ls:
        eng.gemm_force_plan(*l["force"])
        eng.gemm_force_knobs(0, 0, -1, l["boxes"], 8, 1)
        for o in outs.values():
            o.reset()
        eng.gemm_plan_log_clear()
        R.run_proj(eng, prob, case["ins"], outs["q"].view, outs["k"].view, outs["vt"].view)
        recs, n = eng.gemm_plan_log()
        bad = [f"{n} GEMM launches instead of {len(l['expect'])}"] if n != len(l["expect"]) else \
            [f"part {i} {k}: asked {v!r}, ran {r[k]!r}" for i, (r, e) in enumerate(zip(recs, l["expect"])) for k, v in e.items() if r[k] != v]
        if bad:
            say("PROBLEM", pid, what(l), "plan not taken:", "; ".join(bad))
            continue
        done += 1
        for name, o in outs.items():
            e = l["expect"][part_of[name]]
            key = f"{name}:{e['tm']}x{e['tn']}/{e['splits']}"
            if key in first:
                if not torch.equal(o.bits, first[key]):
                    say("PROBLEM", pid, what(l), f"bits differ from the first launch of {key} (or a guard zone or the padding changed)")
                continue
            first[key] = o.bits.clone()
            reg, val = R.proj_region(lay, B, H, name, o.view)
            ref, S, K = case["refs"][name]
            bound = (K + (e["splits"] if e["splits"] > 1 else 0)) * R.U * S + R.BF16_ULP * ref.abs()
            err = (val.double() - ref).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            rest = o.buf.clone()
            R.proj_region(lay, B, H, name, rest[R.GUARD:-R.GUARD])[0][...] = 7
            if not (o.guards_ok() and bool((rest[R.GUARD:-R.GUARD] == 7).all())):
                say("PROBLEM", pid, what(l), f"{key}: a guard zone or the padding of the buffer was written")
            if not ratio <= 1.0:
                say("PROBLEM", pid, what(l), f"{key}: err / bound = {ratio}")
            say("DETAIL", pid, key, repr(ratio), repr(float(err.max())))
            if not worst[0] >= ratio:
                worst = (ratio, key)
    say("REPORT", pid, done, len(first), repr(worst[0]), worst[1], 0)


def half_inputs(prob, ins):
    if prob["op"] == "linear":
        return dict(ins, x=ins["x"][:prob["args"]["M"] // 2].contiguous())
    return dict(ins, x0=ins["x0"][:prob["args"]["B"] // 2].contiguous())


def run_pair(eng, full, half, fxf, fxh):
    pid = full["id"]
    case, case_h = R.make_case(full, eng.device), R.make_case(half, eng.device)
    ins_h = half_inputs(full, case["ins"])
    out, out_h = Out(case["shape"], case["dtype"], eng.device), Out(case_h["shape"], case_h["dtype"], eng.device)
    n_rows = case_h["shape"][0]
    common, done = R.pair_launches(full, fxf, half, fxh), 0
    for key, lf, lh in common:
        bad = launch(eng, full, lf, case["ins"], out) + launch(eng, half, lh, ins_h, out_h)
        done += 0 if bad else 1
        if bad:
            say("PROBLEM", pid, key, "plan not taken:", "; ".join(bad))
        elif not (out.guards_ok() and out_h.guards_ok()) or bool(torch.isnan(out_h.view).any()):
            say("PROBLEM", pid, key, "a guard zone changed or a NaN is left")
        elif not torch.equal(out.view[:n_rows].contiguous().view(INT[case["dtype"]]), out_h.view.contiguous().view(INT[case["dtype"]])):
            say("PROBLEM", pid, key, f"rows [0, {n_rows}) of the full launch differ from the half launch")
    say("REPORT", pid, 2 * done, done, "0.0", "-", 0)


if __name__ == "__main__":
    group = sys.argv[1]
    fixture = R.load_fixture()
    eng = Engine(0, arena_gb=1.0)
    t0 = time.time()
    probs = {p["id"]: p for p in R.PROBLEMS if p["group"] == group}
    if not probs:
        sys.exit(f"unknown group {group!r}")
    for p in probs.values():
        if group == "proj":
            if "parts" in p:
                run_proj(eng, p, fixture)
        elif group == "heads":
            if p["op"] in ("lnq", "lng"):
                run_heads(eng, p, fixture)
        elif group != "bits":
            run_problem(eng, p, fixture[p["id"]])
        elif "pair" in p:
            run_pair(eng, p, probs[p["pair"]], fixture[p["id"]], fixture[p["pair"]])
    eng.gemm_force_clear()
    torch.cuda.synchronize()
    say("TIME", group, f"{time.time() - t0:.1f}")
    eng.close()
