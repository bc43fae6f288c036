"""Every plan the GEMM planner can give a launch, run one by one against float64 (tests/test_gemm_candidates_cpu.py and
tests/test_gemm_candidates_gpu.py with its child tests/gemm_candidates_child.py).

PROBLEMS names the launches: an operator of the C ABI with its sizes, and the descriptor the planner sees for it. Which plans a
problem can run with is NOT written here: tests/gemm_plan_main.hip (mode `candidates`) asks the planner, and the answer is kept as
tests/golden/gemm_candidates.json, which the CPU test holds to the planner of the day and the GPU test reads:
    plan        the default choice without the shipped table (model)
    tune        gemm_tune_candidates: [tm, tn, splits, cap]; tune_corun: what GL_GEMM_TUNE_CORUN=1 adds
    forced      every tile x split gemm_force_cfg is given exactly as asked, with n_items, box, rm, rz, K tiles per split (boxes on)
    fixed       the fixed-tile families (glds; halo with halo_splits 1, 2, 3, 64; wide with wide_splits 1, 2, 3, 5 x wide_xcd 0, 1)
launches() turns that into the list a child runs: each forced (tile, split) under the caps 512, 1, 3, 7 and every cap the tuner lists
for it, each with the XCD boxes on and off, then the fixed plans, then the default plan.

Bounds (derived, u = 2^-24; ref and S = sum_k |a_k| |w_k| in float64 on the bf16-rounded inputs):
    accumulator + bias      |acc - ref| <= L u (S + |bias|), L = K + 1 additions, + `splits` slab additions behind a K split
                            (the worst case of a length-L fp32 sum in any order; the MFMA's products of two bf16 are exact in fp32)
    SiLU                    y = v sigmoid(v), |dy/dv| <= 1.1; evaluated as v * rcp(1 + exp2(-v log2 e)): the argument carries 2 u |v| log2 e,
                            exp2 and rcp 1 ulp = 2 u each, the add and the multiply u each: (2 |v| + 6) u |y|
    residual                one more fp32 addition: u (|res| + |y|)
    GEGLU                   val gelu(gate), |gelu'| <= 1.13; gelu by Abramowitz & Stegun 7.1.26 (|erf error| <= 1.5e-7) in about 16 fp32
                            operations on values <= 1: |gelu error| <= |gate| / 2 (1.5e-7 + 16 u); product rule + 2 u |val gelu|
    bf16 output             + 2^-8 |ref| (one ulp of the output rounding); an fp32 output is the sum itself
    folded LayerNorm        lnq_ref
"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_candidates.json")
WS_KIB = 256 << 10          # the engine's split-K workspace (Engine::init_workspace)
SMALL_CAPS = (1, 3, 7)      # several items per workgroup at any size (the tuner's 512 only gets there on large problems)
U = 2.0 ** -24
BF16_ULP = 2.0 ** -8
GUARD = 64                  # elements in front of and behind every output

# one input line of gemm_plan_main (the order of tests/test_gemm_plan_cpu.py FIELDS)
FIELDS = [("M", 0), ("N", 0), ("K", 0),
          ("a_mode", 0), ("C0", 0), ("C1", 0), ("ld0", 0), ("ld1", 0), ("Hin", 0), ("Win", 0), ("Ho", 0), ("Wo", 0), ("stride", 0), ("ups", 0),
          ("pad_lo", 0), ("gn", 0),
          ("e_mode", 0), ("act", 0), ("out_f32", 0), ("bias", 1), ("bias2", 0), ("bias2_ld", 0), ("rows_per_b", 1), ("res", 0), ("gate", 0),
          ("q", 0), ("k", 0), ("vt", 0), ("C", 0), ("T", 0), ("remap_in", 0), ("geglu16", 0), ("stats_out", 0), ("stats_ld", 0),
          ("ln_stats", 0), ("ln_nb", 0), ("ln_ld", 0), ("ln_csum", 0),
          ("ws", 1), ("ws_kib", WS_KIB), ("no_split", 0)]
PLAN_FIELDS = ["rc", "tm", "tn", "splits", "stats_nb", "grid", "box", "rm", "rz", "kt_per_split", "xcd", "chunks_per_split", "gn_supported",
               "ln_supported", "name"]
EPILOGUES = {"plain": dict(), "res": dict(res=1), "silu": dict(act=1), "f32": dict(out_f32=1)}


def input_line(desc):
    unknown = set(desc) - {f for f, _ in FIELDS}
    assert not unknown, unknown
    return " ".join(str(desc.get(f, d)) for f, d in FIELDS)


# ---------------------------------------------------------------------------------------------------------------- the problems
def _linear(M, N, K, epi, group, tag="", **kw):
    e = EPILOGUES[epi]
    return dict(id=f"lin{tag}_{M}x{N}x{K}_{epi}", group=group, op="linear", args=dict(M=M, N=N, K=K, epi=epi),
                desc=dict(M=M, N=N, K=K, C0=K, ld0=K, **e), **kw)


def _geglu(M, inner, K, group):
    return dict(id=f"geglu_{M}x{inner}x{K}", group=group, op="geglu", args=dict(M=M, inner=inner, K=K),
                desc=dict(M=M, N=2 * inner, K=K, C0=K, ld0=K, act=2, geglu16=1))


def conv_out(H, W, stride, ups, pad_lo):
    Hup, Wup = H << ups, W << ups
    if stride == 1:
        return Hup, Wup
    return (Hup + (2 if pad_lo else 1) - 3) // 2 + 1, (Wup + (2 if pad_lo else 1) - 3) // 2 + 1


def _conv(B, H, W, C0, C1, Cout, group, stride=1, ups=0, pad_lo=1, res=0, tag="", **kw):
    Cin = C0 + C1
    phase = stride == 1 and ups == 1 and pad_lo == 1 and not res      # gl_op_conv3x3 runs the engine's Upsample in phase form
    Ho, Wo = conv_out(H, W, stride, ups, pad_lo)
    cid = f"conv{tag}_{B}x{H}x{W}_{C0}+{C1}to{Cout}_s{stride}u{ups}p{pad_lo}" + ("_res" if res else "")
    args = dict(B=B, H=H, W=W, C0=C0, C1=C1, Cout=Cout, stride=stride, ups=ups, pad_lo=pad_lo, res=res, phase=phase)
    if phase:
        desc = dict(M=4 * B * H * W, N=Cout, K=4 * Cin, a_mode=2, C0=C0, C1=C1, ld0=C0, ld1=C1, Hin=H, Win=W, Ho=2 * H, Wo=2 * W, stride=1, pad_lo=1)
    else:
        desc = dict(M=B * Ho * Wo, N=Cout, K=9 * Cin, a_mode=1, C0=C0, C1=C1, ld0=C0, ld1=C1, Hin=H, Win=W, Ho=Ho, Wo=Wo, stride=stride, ups=ups,
                    pad_lo=pad_lo, rows_per_b=Ho * Wo, res=res)
    return dict(id=cid, group=group, op="conv", args=args, desc=desc, **kw)


def _lnq(B, T, C, K0=320, heads=8):
    """gl_op_ln_linear mode 1: the producer x = a W0^T + b0 + res with the rows' partial sums (`lnp_`), then the q projection of the raw
    rows with the LayerNorm folded into its epilogue, in the attention kernels' q layout (`lnq_`: the head-layout instantiation)."""
    M, tag = B * T, f"{B}x{T}_C{C}"
    prod = dict(id=f"lnp_{tag}", group="heads", op="lnp", args=dict(M=M, N=C, K=K0, epi="res"),
                desc=dict(M=M, N=C, K=K0, C0=K0, ld0=K0, res=1, stats_out=1, stats_ld=C // 32))
    cons = dict(id=f"lnq_{tag}", group="heads", op="lnq", args=dict(B=B, T=T, M=M, C=C, N1=C, K0=K0, H=heads, mode=1), producer=prod["id"],
                desc=dict(M=M, N=C, K=C, C0=C, ld0=C, e_mode=1, q=1, C=C, T=T, ln_stats=1, ln_nb=1, ln_ld=C // 32, ln_csum=1))
    return [prod, cons]


def _proj(B, Nq, Nk, C, Ck, heads=8):
    """gl_op_attention_project. Self-attention (Nk = Nq, Ck = C): the fused q, k, v^T launch (EPI_QKV_HEADS: never split, no 128 x 160 tile,
    the V third with exchanged operand roles, no bias, no workspace), one part. Cross-attention: the q scatter, the k scatter into the
    key-tile layout (both with the workspace, so they split) and the v^T projection with exchanged roles (no workspace), three parts, each
    a fixture entry of its own. Tokens are padded to multiples of 64."""
    Tq, Tk = -(-Nq // 64) * 64, -(-Nk // 64) * 64
    tag = f"{B}x{Nq}x{Nk}_C{C}_Ck{Ck}"
    heads_ = dict(bias=0, C=C)
    if Nq == Nk and C == Ck:
        parts = [dict(id=f"qkv_{tag}", desc=dict(M=B * Tq, N=3 * C, K=C, C0=C, ld0=C, e_mode=4, q=1, k=1, vt=1, T=Tq, ws=0, ws_kib=0, **heads_))]
    else:
        parts = [dict(id=f"xq_{tag}", desc=dict(M=B * Tq, N=C, K=C, C0=C, ld0=C, e_mode=1, q=1, T=Tq, **heads_)),
                 dict(id=f"xk_{tag}", desc=dict(M=B * Tk, N=C, K=Ck, C0=Ck, ld0=Ck, e_mode=1, q=1, T=Tk, **heads_)),
                 dict(id=f"xv_{tag}", desc=dict(M=C, N=B * Tk, K=Ck, C0=Ck, ld0=Ck, e_mode=2, T=Tk, ws=0, ws_kib=0, bias=0))]
    for p in parts:
        p.update(group="proj", op="part", args={})
    return parts + [dict(id=f"proj_{tag}", group="proj", op="proj", args=dict(B=B, Nq=Nq, Nk=Nk, C=C, Ck=Ck, H=heads), parts=[p["id"] for p in parts],
                         desc=parts[0]["desc"])]


def _lng(M, C=320, inner=320, K0=320):
    """gl_op_ln_linear mode 0, GEGLU(LN(x) W1^T + b1): at M % 256 == 0 the fold lives in gemm_wide_kernel's GEGLU epilogue; elsewhere the
    operator runs the LayerNorm kernel and a plain GEGLU GEMM, which takes every forced even-tn tile and split."""
    fold = M % 256 == 0
    prod = dict(id=f"lngp_{M}_C{C}", group="heads", op="part", args={}, desc=dict(M=M, N=C, K=K0, C0=K0, ld0=K0, res=1, stats_out=1, stats_ld=C // 32))
    desc = dict(M=M, N=2 * inner, K=C, C0=C, ld0=C, act=2, geglu16=1)
    if fold:
        desc.update(ln_stats=1, ln_nb=1, ln_ld=C // 32, ln_csum=1)
    cons = dict(id=f"lngc_{M}_C{C}", group="heads", op="part", args={}, desc=desc)
    return [prod, cons, dict(id=f"lng_{M}_C{C}", group="heads", op="lng", args=dict(M=M, C=C, N1=2 * inner, K0=K0, mode=0, T=0, fold=fold),
                             parts=[prod["id"], cons["id"]], desc=desc)]


def _problems():
    out = []
    # row GEMMs: ragged M and N with uneven splits; nk = 24; nk = 64; nk = 2 (no split); 8 x 2 tiles of 128 x 128 (the box partitions)
    for M, N, K in [(100, 320, 640), (333, 960, 1536), (64, 1280, 4096), (512, 128, 128), (1024, 256, 640)]:
        out += [_linear(M, N, K, epi, "rows") for epi in EPILOGUES]
    # GEGLU: gemm_u_kernel (even tn only) at M = 100, 300, gemm_wide_kernel at M = 256
    out += [_geglu(M, 320, 640, "geglu_wide") for M in (100, 300, 256)]
    # gemm_wide_kernel with the other epilogues (wide = 2): its K split; 256 items for the XCD item order
    # (2048 rows: 64 tiles x 5 splits = 320 items on its 256 workgroups, the only way into its loop over items at a small size)
    for M, N, K in [(256, 1280, 1280), (8192, 1280, 64), (2048, 1280, 1280)]:
        out += [_linear(M, N, K, epi, "geglu_wide" if M == 256 else "wide_items", wide=2) for epi in EPILOGUES]
    # gemm_glds_kernel: N < 128, its four fixed tiles and its split rule (the 64 x 64 tile wins where 128 rows would be mostly padding: M = 40)
    for M in (100, 4096, 40):
        for N in (4, 32, 64, 96) if M != 40 else (64, 96):
            for K in (128, 1024):
                out += [_linear(M, N, K, epi, "glds") for epi in EPILOGUES]
    # convs: two sources; stride 1 / stride 2 with pad_lo 0 and 1 / nearest-2x upsample (with a residual: the nine-tap form); the phase form
    out += [_conv(2, 12, 20, 128, 64, 64, "conv"),
            _conv(2, 16, 16, 128, 0, 192, "conv"),
            _conv(2, 16, 16, 128, 0, 192, "conv", res=1),
            _conv(2, 16, 16, 128, 0, 192, "conv", stride=2, pad_lo=0),
            _conv(2, 16, 16, 128, 0, 192, "conv", stride=2, pad_lo=1),
            _conv(2, 16, 16, 128, 0, 192, "conv", ups=1, res=1),
            _conv(2, 8, 8, 64, 0, 128, "conv", ups=1),
            # conv_halo_kernel's shape: on gemm_u_kernel under every forced tile, on the halo kernel under its own splits (2 chunks of 64
            # channels; 5 chunks: 2, 2, 1 under halo_splits = 3), two sources and a residual
            _conv(2, 32, 32, 128, 0, 160, "conv_halo"),
            _conv(2, 32, 32, 320, 0, 160, "conv_halo"),
            _conv(2, 32, 32, 128, 64, 128, "conv_halo", res=1),
            # 64 tiles x 5 splits = 320 items on the halo kernel's 256 workgroups: its loop over items
            _conv(8, 32, 32, 320, 0, 320, "halo_items")]
    # the bits the guidance pair's shared prefix relies on: rows [0, M / 2) of the M-row launch against the M / 2-row launch
    for M in (512, 200):
        out += [_linear(M, 320, 640, "plain", "bits", tag="B", pair=f"linB_{M // 2}x320x640_plain"), _linear(M // 2, 320, 640, "plain", "bits", tag="B")]
    out += [_conv(2, 16, 16, 128, 0, 192, "bits", tag="B", pair="convB_1x16x16_128+0to192_s1u0p1"), _conv(1, 16, 16, 128, 0, 192, "bits", tag="B"),
            _conv(2, 32, 32, 320, 0, 160, "bits", tag="B", halo=4, pair="convB_1x32x32_320+0to160_s1u0p1"), _conv(1, 32, 32, 320, 0, 160, "bits", tag="B", halo=4)]
    # head layouts behind a folded LayerNorm: C = 320 (d = 40 in rows of 48) and 640, 64 tokens (in 128 rows) and 256, B = 1 and 3; C = 1280
    # has 20 / 40 partial sums per row, more than the consumer's threads hold in registers (the tail loop of its statistics fetch)
    for B, T, C in [(1, 64, 320), (3, 64, 320), (1, 256, 320), (3, 256, 320), (1, 64, 640), (3, 64, 640), (1, 256, 640), (3, 256, 640), (1, 64, 1280)]:
        out += _lnq(B, T, C)
    out += _lng(256) + _lng(100) + _lng(300)
    for C in (320, 640):
        out += [p for T in (64, 256) for B in (1, 3) for p in _proj(B, T, T, C, C)]
        out += _proj(1, 64, 77, C, 768) + _proj(3, 256, 30, C, 768)
    ids = [p["id"] for p in out]
    assert len(set(ids)) == len(ids), "problem ids are unique"
    return out


PROBLEMS = _problems()
GROUPS = ["rows", "geglu_wide", "wide_items", "glds", "conv", "conv_halo", "halo_items", "bits", "heads", "proj"]


# ---------------------------------------------------------------------------------------------------------------- the planner's answer
def build_planner(exe, sanitize=True):
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", *san, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "gligen_amd", "csrc", "gemm_plan.hip"), os.path.join(ROOT, "tests", "gemm_plan_main.hip"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _plan_fields(parts):
    return [int(x) for x in parts[:len(PLAN_FIELDS) - 1]] + [" ".join(parts[len(PLAN_FIELDS) - 1:])]


def ask_planner(exe, problems=None):
    """{id: {"plan", "tune", "tune_corun", "forced", "fixed"}} from gemm_plan_main candidates (one run per setting of the routing knobs)."""
    problems = PROBLEMS if problems is None else problems
    out = {}
    for wide, halo in sorted({(p.get("wide", 1), p.get("halo", 8)) for p in problems}):
        ps = [p for p in problems if (p.get("wide", 1), p.get("halo", 8)) == (wide, halo)]
        r = subprocess.run([str(exe), "candidates"] + (["wide2"] if wide == 2 else []) + ([f"halo{halo}"] if halo != 8 else []), input="\n".join(input_line(p["desc"]) for p in ps) + "\n",
                           capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
        blocks, cur = [], None
        for line in r.stdout.splitlines():
            w = line.split()
            if w[0] == "PLAN":
                cur = dict(plan=_plan_fields(w[1:]), tune=[], tune_corun=[], forced=[], fixed=[])
            elif w[0] in ("TUNE", "TUNE_CORUN", "FORCED"):
                cur[w[0].lower()].append([int(x) for x in w[1:]])
            elif w[0] == "FIXED":
                cur["fixed"].append([int(x) for x in w[1:4]] + _plan_fields(w[4:]))
            elif w[0] == "END":
                blocks.append(cur)
        assert len(blocks) == len(ps), (len(blocks), len(ps))
        out.update({p["id"]: b for p, b in zip(ps, blocks)})
    return out


def fixture_payload(answer, problems=None, provenance=None):
    """The file's form: each distinct answer once (the epilogues of a shape mostly share one), the tuner's caps behind the forced row of
    their (tile, split) -- so every tuner candidate is a forced one, or this raises -- and the problems as indices."""
    answers, index = [], {}
    for p in (PROBLEMS if problems is None else problems):
        a = answer[p["id"]]
        rows = {tuple(f[:3]): f + [[], []] for f in a["forced"]}
        for which, name in enumerate(("tune", "tune_corun")):
            for tm, tn, sp, cap in a[name]:
                rows[(tm, tn, sp)][8 + which].append(cap)
        c = {"plan": a["plan"], "forced": list(rows.values()), "fixed": a["fixed"]}
        if c not in answers:
            answers.append(c)
        index[p["id"]] = answers.index(c)
    return {"_provenance": provenance or "tests/gemm_plan_main.hip, mode `candidates`, over tests/gemm_candidates_ref.py PROBLEMS; regenerate with "
                                         "`python tests/gemm_candidates_ref.py --write` (tests/test_gemm_candidates_cpu.py holds it to the planner)",
            "plan_fields": PLAN_FIELDS, "forced_fields": ["tm", "tn", "splits", "n_items", "box", "rm", "rz", "kt_per_split", "tune_caps", "corun_caps"],
            "problems": index, "answers": answers}


def dump_fixture(payload):
    # one answer per line: small, and a planner change shows as the lines it touches
    head = {k: v for k, v in payload.items() if k != "answers"}
    lines = [json.dumps(head, separators=(",", ":"))[:-1] + ',"answers":[']
    lines += [json.dumps(a, separators=(",", ":")) + ("," if i + 1 < len(payload["answers"]) else "") for i, a in enumerate(payload["answers"])]
    return "\n".join(lines) + "\n]}\n"


def load_fixture(path=None):
    """{id: {"plan", "tune", "tune_corun", "forced", "fixed"}}, the file's form expanded again."""
    with open(path or FIXTURE) as f:
        data = json.load(f)
    out = {}
    for pid, i in data["problems"].items():
        a = data["answers"][i]
        out[pid] = dict(plan=a["plan"], fixed=a["fixed"], forced=[f[:8] for f in a["forced"]],
                        tune=[f[:3] + [cap] for f in a["forced"] for cap in f[8]], tune_corun=[f[:3] + [cap] for f in a["forced"] for cap in f[9]])
    return out


def launches(prob, fx):
    """The launches of one problem: dicts with `force` (tm, tn, splits, cap) or `fixed` (halo_splits, wide_splits, wide_xcd), `boxes`,
    `key` (launches with the same key must give the same bits) and `expect` (what the plan log has to say)."""
    out = []
    for tm, tn, sp, n_items, box, rm, rz, kt in fx["forced"]:
        caps = sorted({512, *SMALL_CAPS} | {c[3] for c in fx["tune"] + fx["tune_corun"] if c[:3] == [tm, tn, sp]})
        for cap in caps:
            for boxes in (1, 0):
                e = dict(tm=tm, tn=tn, splits=sp, n_items=n_items, grid=min(n_items, cap), units_per_split=kt)
                e.update(dict(box=box, rm=rm, rz=rz) if boxes else dict(box=-1, rm=0, rz=sp))
                out.append(dict(force=(tm, tn, sp, cap), boxes=boxes, key=f"{tm}x{tn}/{sp}", expect=e))
    for hs, ws, wx, *plan in fx["fixed"]:
        pl = dict(zip(PLAN_FIELDS, plan))
        e = dict(tm=pl["tm"], tn=pl["tn"], splits=pl["splits"], grid=pl["grid"], kernel=pl["name"], xcd=pl["xcd"],
                 units_per_split=pl["chunks_per_split"] if pl["name"].startswith("conv_halo") else pl["kt_per_split"])
        out.append(dict(fixed=(hs, ws, wx), boxes=1, key=f"{pl['name'].split('<')[0]}/{pl['splits']}", expect=e))
    pl = dict(zip(PLAN_FIELDS, fx["plan"]))
    e = dict(tm=pl["tm"], tn=pl["tn"], splits=pl["splits"], grid=pl["grid"], kernel=pl["name"])
    fam = pl["name"].split("<")[0]
    out.append(dict(boxes=1, key=f"{pl['tm']}x{pl['tn']}/{pl['splits']}" if fam in ("gemm_u_kernel", "gemm_p_kernel") else f"{fam}/{pl['splits']}", expect=e))
    return out


def pair_launches(full, fxf, half, fxh):
    """[(key, launch of the full problem, launch of the half problem)]: every candidate both have, boxes on at the default cap, and the
    fixed plans by their split."""
    def cands(prob, fx):
        c = {}
        for l in launches(prob, fx):
            if ("force" in l and l["boxes"] == 1 and l["force"][3] == 512) or "fixed" in l:
                c.setdefault(l["key"], l)
        return c
    cf, ch = cands(full, fxf), cands(half, fxh)
    return [(k, cf[k], ch[k]) for k in cf if k in ch]


def head_launches(cons, fxc, fxp):
    """gl_op_ln_linear under every unsplit tile: both of its launches take the forced tile where they can (the 128 x 160 tile has no
    head-layout form: the q projection is then planned as usual). `expect`: (producer, consumer)."""
    out = []
    unsplit_c = {tuple(x[:2]): x for x in fxc["forced"] if x[2] == 1}
    pl = dict(zip(PLAN_FIELDS, fxc["plan"]))
    for tm, tn, sp, n_items, box, rm, rz, kt in fxp["forced"]:
        if sp != 1:
            continue      # (a split producer emits no statistics: the operator then runs the LayerNorm kernel, another consumer launch)
        for cap in (512, *SMALL_CAPS):
            for boxes in (1, 0):
                ep = dict(tm=tm, tn=tn, splits=1, n_items=n_items, grid=min(n_items, cap), units_per_split=kt)
                ep.update(dict(box=box, rm=rm, rz=rz) if boxes else dict(box=-1, rm=0, rz=1))
                c = unsplit_c.get((tm, tn))
                if c:
                    ec = dict(tm=tm, tn=tn, splits=1, n_items=c[3], grid=min(c[3], cap), units_per_split=c[7])
                    ec.update(dict(box=c[4], rm=c[5], rz=c[6]) if boxes else dict(box=-1, rm=0, rz=1))
                else:
                    ec = dict(tm=pl["tm"], tn=pl["tn"], splits=pl["splits"])
                ec["kernel"] = f"gemm_u_kernel<2, {ec['tm']}, {ec['tn']}, 0, 2, false>"     # (the name's last argument says QKV only for EPI_QKV_HEADS)
                out.append(dict(force=(tm, tn, 1, cap), boxes=boxes, key=f"{tm}x{tn}/1", expect=(ep, ec)))
    return out


def proj_launches(prob, fx):
    """gl_op_attention_project under every (tile, split) any of its parts can be forced to, caps 512, 1, 3, 7, boxes on and off. `expect`:
    per part, the forced row where the part takes the choice, else its usual plan (tile, split and kernel; its grid follows the cap)."""
    parts = [fx[i] for i in prob["parts"]]
    names = [dict(zip(PLAN_FIELDS, f["plan"]))["name"].split("<")[1].split(">")[0].split(", ") for f in parts]
    out = []
    for tm, tn, sp in sorted({tuple(x[:3]) for f in parts for x in f["forced"]}):
        for cap in (512, *SMALL_CAPS):
            for boxes in (1, 0):
                es = []
                for f, nm in zip(parts, names):
                    row = {tuple(x[:3]): x for x in f["forced"]}.get((tm, tn, sp))
                    if row:
                        e = dict(tm=tm, tn=tn, splits=sp, n_items=row[3], grid=min(row[3], cap), units_per_split=row[7])
                        e.update(dict(box=row[4], rm=row[5], rz=row[6]) if boxes else dict(box=-1, rm=0, rz=sp))
                    else:
                        pl = dict(zip(PLAN_FIELDS, f["plan"]))
                        e = dict(tm=pl["tm"], tn=pl["tn"], splits=pl["splits"])
                    e["kernel"] = f"gemm_u_kernel<2, {e['tm']}, {e['tn']}, {nm[3]}, 2, {nm[5]}>" + (" + splitk_reduce_kernel" if e["splits"] > 1 else "")
                    es.append(e)
                out.append(dict(force=(tm, tn, sp, cap), boxes=boxes, expect=es))
    return out


def lng_launches(prob, fx):
    """Mode 0 of gl_op_ln_linear. Folded (wide kernel): no tile can be forced (a forced tile leaves the wide kernel, which alone has the
    fold), so the wide kernel's own knobs, with the producer under the caps 512 and 3. Else: proj_launches over (producer, consumer)."""
    if not prob["args"]["fold"]:
        return proj_launches(prob, fx)
    pp, out = dict(zip(PLAN_FIELDS, fx[prob["parts"][0]]["plan"])), []
    for hs, ws, wx, *plan in fx[prob["parts"][1]]["fixed"]:
        pl = dict(zip(PLAN_FIELDS, plan))
        for cap in (512, 3):
            out.append(dict(fixed=(hs, ws, wx), cap=cap, boxes=1,
                            expect=[dict(tm=pp["tm"], tn=pp["tn"], splits=pp["splits"], kernel=pp["name"]),
                                    dict(tm=pl["tm"], tn=pl["tn"], splits=pl["splits"], grid=pl["grid"], kernel=pl["name"], xcd=pl["xcd"], units_per_split=pl["kt_per_split"])]))
    return out


def make_proj_case(prob, dev):
    """Inputs, and per buffer (q, k, vt) the float64 projection of the zero-padded token rows as [B][T][C] with S = |x| |W|^T. No bias:
    |got - ref| <= (K + splits) u S + 2^-8 |ref|; a padded row is 0 exactly."""
    import torch
    a = prob["args"]
    B, Nq, Nk, C, Ck = a["B"], a["Nq"], a["Nk"], a["C"], a["Ck"]
    fused = len(prob["parts"]) == 1
    xq = _rnd((B, Nq, C), 1).bfloat16()
    xkv = xq if fused else _rnd((B, Nk, Ck), 5).bfloat16()
    wq, wk, wv = _rnd((C, C), 2, C ** -0.5).bfloat16().float(), _rnd((C, Ck), 3, Ck ** -0.5).bfloat16().float(), _rnd((C, Ck), 4, Ck ** -0.5).bfloat16().float()

    def ref(x, w, T):
        x64 = torch.nn.functional.pad(x.double(), (0, 0, 0, T - x.shape[1]))
        return (x64 @ w.double().t()).to(dev), (x64.abs() @ w.double().abs().t()).to(dev)
    Tq, Tk = -(-Nq // 64) * 64, -(-Nk // 64) * 64
    xq_d = xq.to(dev)
    ins = dict(xq=xq_d, xkv=xq_d if fused else xkv.to(dev), wq=wq.to(dev), wk=wk.to(dev), wv=wv.to(dev))
    return dict(ins=ins, fused=fused, refs=dict(q=ref(xq, wq, Tq) + (C,), k=ref(xkv, wk, Tk) + (Ck,), vt=ref(xkv, wv, Tk) + (Ck,)))


def proj_layout(eng, a):
    import ctypes
    from gligen_amd._lib import AttnProjLayout, check
    lay = AttnProjLayout()
    check(eng.lib.gl_op_attention_project(eng._ctx, None, None, a["B"], a["Nq"], a["Nk"], a["C"], a["Ck"], a["H"], None, None, None, None, None, None,
                                          ctypes.byref(lay), None))
    return lay


def run_proj(eng, prob, ins, q, k, vt):
    import ctypes
    from gligen_amd.engine import _ptr, _stream
    from gligen_amd._lib import AttnProjLayout, check
    a, lay = prob["args"], AttnProjLayout()
    check(eng.lib.gl_op_attention_project(eng._ctx, _ptr(ins["xq"]), _ptr(ins["xkv"]), a["B"], a["Nq"], a["Nk"], a["C"], a["Ck"], a["H"], _ptr(ins["wq"]),
                                          _ptr(ins["wk"]), _ptr(ins["wv"]), _ptr(q), _ptr(k), _ptr(vt), ctypes.byref(lay), _stream(eng.device)))


def proj_region(lay, B, H, name, buf):
    """(the part of a buffer the layout says is written, as a view into it; its values as [B][T][H d]), by the layouts of the header."""
    import torch
    d = lay.d
    if name == "q":
        reg = buf.view(B, H, lay.tq_pad, lay.dp)[:, :, :lay.tq, :d]
        val = reg
    elif name == "k":
        reg = buf.view(B, H, lay.tk_pad // 64, lay.dp // 8, 64, 8)[:, :, :lay.tk // 64, :d // 8]
        val = reg.permute(0, 1, 2, 4, 3, 5).reshape(B, H, lay.tk, d)
    else:
        reg = buf.view(B, H, lay.dpv, lay.tk_pad)[:, :, :d, :lay.tk]
        t = torch.arange(lay.tk, device=buf.device)
        g = (t >> 2) & (7 if lay.vt_perm32 else 3)
        pos = (t & ~31) | ((((g & 1) << 2) | (g >> 1)) << 2) | (t & 3) if lay.vt_perm32 else (t & ~15) | ((((g & 1) << 1) | (g >> 1)) << 2) | (t & 3)
        val = reg[..., pos].permute(0, 1, 3, 2)
    return reg, val.permute(0, 2, 1, 3).reshape(B, val.shape[2], H * d)


def geglu_finish(h, bh, inner):
    """val gelu(gate) of h = (val | gate) with bound bh, and its bound (module docstring), bf16 rounding included."""
    import torch
    val, gate, bv, bg = h[:, :inner], h[:, inner:], bh[:, :inner], bh[:, inner:]
    g = gate * 0.5 * (1 + torch.erf(gate * 2 ** -0.5))
    b_g = 1.13 * bg + 0.5 * gate.abs() * (1.5e-7 + 16 * U)
    y = val * g
    return y, g.abs() * bv + val.abs() * b_g + bv * b_g + 2 * U * y.abs() + BF16_ULP * y.abs()


def ln_fallback_ref(x64, w64, b1, e_b, C, splits=1, eps=1e-5):
    """The unfolded form: the LayerNorm kernel writes xn = bf16((x - mean) rstd) and a plain GEMM multiplies it. xn is off by one bf16 ulp
    plus the fp32 evaluation (mean, rstd as in lnq_ref; two more roundings); then a length-C fp32 sum with the bias (and the slabs of a K split)."""
    mean, sa, s2 = x64.mean(1), x64.abs().sum(1), (x64 * x64).sum(1)
    var = s2 / C - mean * mean
    r = ((var + eps) ** -0.5)[:, None]
    xh = (x64 - mean[:, None]) * r
    e_mean = (C + 2) * U * sa / C
    e_var = (C + 2) * U * s2 / C + 2 * mean.abs() * e_mean + e_mean ** 2 + 2 * U * (s2 / C + mean * mean)
    e_r = (0.505 * e_var / (var + eps) + 3 * U)[:, None]
    e_xn = BF16_ULP * xh.abs() + r * e_mean[:, None] * (1 + e_r) + xh.abs() * (e_r + 2 * U)
    wa = w64.abs().t()
    return xh @ w64.t() + b1, e_xn @ wa + (C + 1 + (splits if splits > 1 else 0)) * U * ((xh.abs() + e_xn) @ wa + b1.abs()) + e_b


def lnq_ref(x64, w64, b1, C, eps=1e-5, e_b=0.0, round_out=True):
    """y = rstd (x W^T - mean csum) + b1 in float64 on the producer's own bf16 rows x, and the bound of the kernel's fp32 evaluation:
    acc as every GEMM; csum a C-term fp32 sum; mean and E[x^2] C-term fp32 sums times the rounded 1 / C; var = E[x^2] - mean^2 with
    both products and the subtraction rounded; rsqrt(var + eps) moves by 0.505 of var's relative error (|d| < 0.01) plus the add and
    a 1-ulp rsqrt; then the product rule through rstd (acc - mean csum) + b1 and the bf16 rounding (round_out). w64 / b1 are the folded
    weights and bias of folded_affine, e_b the folded bias's own error."""
    s1, sa, s2 = x64.sum(1), x64.abs().sum(1), (x64 * x64).sum(1)
    mean = s1 / C
    var = s2 / C - mean * mean
    rstd = (var + eps) ** -0.5
    acc, S = x64 @ w64.t(), x64.abs() @ w64.abs().t()
    csum, ca = w64.sum(1), w64.abs().sum(1)
    m, r = mean[:, None], rstd[:, None]
    t = acc - m * csum
    y = r * t + b1
    e_acc, e_cs = C * U * S, C * U * ca
    e_mean = ((C + 2) * U * sa / C)[:, None]
    e_var = (C + 2) * U * s2 / C + 2 * mean.abs() * e_mean[:, 0] + e_mean[:, 0] ** 2 + 2 * U * (s2 / C + mean * mean)
    e_r = (0.505 * e_var / (var + eps) + 3 * U)[:, None]
    e_t = e_acc + m.abs() * e_cs + csum.abs() * e_mean + e_mean * e_cs + 2 * U * (acc.abs() + (m * csum).abs())
    return y, r * e_t * (1 + e_r) + (r * t).abs() * e_r + 2 * U * ((r * t).abs() + y.abs()) + e_b + (BF16_ULP * y.abs() if round_out else 0.0)


def folded_affine(w1, b1, gamma, beta, dev):
    """What the operator multiplies and adds: W' = bf16(fp32(W1 gamma)) (one fp32 product, one rounding: reproduced exactly) and
    b' = b1 + W1 beta, a C-term fp32 sum in some order: the float64 value and its error (C + 2) u (|b1| + |W1| |beta|)."""
    wf = (w1 * gamma).bfloat16().double()
    bf = b1.double() + w1.double() @ beta.double()
    e_b = (w1.shape[1] + 2) * U * (b1.double().abs() + w1.double().abs() @ beta.double().abs())
    return wf.to(dev), bf.to(dev), e_b.to(dev)


def make_lnq_case(prob, dev):
    """gl_op_ln_linear, both modes, with a random LayerNorm affine."""
    a = prob["args"]
    M, C, K0, N1 = a["M"], a["C"], a["K0"], a["N1"]
    t = _lin_tensors(M, C, K0)
    w1, b1 = _rnd((N1, C), 6, C ** -0.5).bfloat16().float(), _rnd((N1,), 7)
    gamma, beta = 1 + 0.2 * _rnd((C,), 8), 0.2 * _rnd((C,), 9)
    ins = dict(a=t["x"].to(dev), w0=t["w"].float().to(dev), b0=t["b"].to(dev), res=t["res"].to(dev), gamma=gamma.to(dev), beta=beta.to(dev),
               w1=w1.to(dev), b1=b1.to(dev))
    acc, S, res64 = t["acc"].to(dev), t["S"].to(dev), t["res"].double().to(dev)
    return dict(ins=ins, acc=acc, S=S, res64=res64, K0=K0, folded=folded_affine(w1, b1, gamma, beta, dev))


def run_lnq(eng, prob, ins, x_out, y_out):
    """gl_op_ln_linear into the two guarded outputs; returns used_fold."""
    import ctypes
    from gligen_amd.engine import _ptr, _stream
    from gligen_amd._lib import check
    a = prob["args"]
    used = ctypes.c_int(-1)
    check(eng.lib.gl_op_ln_linear(eng._ctx, _ptr(ins["a"]), a["M"], a["K0"], _ptr(ins["w0"]), _ptr(ins["b0"]), _ptr(ins["res"]), a["C"],
                                  _ptr(ins["gamma"]), _ptr(ins["beta"]), _ptr(ins["w1"]), _ptr(ins["b1"]), a["mode"], a["H"] if a["mode"] else a["N1"] // 2, a["T"], _ptr(x_out), _ptr(y_out),
                                  ctypes.byref(used), _stream(eng.device)))
    return used.value


# ---------------------------------------------------------------------------------------------------------------- tensors, references, bounds
def _rnd(shape, seed, scale=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _silu_bound(v, bv):
    import torch
    y = v * torch.sigmoid(v)
    return y, 1.1 * bv + (2 * v.abs() + 6) * U * y.abs()


def _finish(pre, b_pre, epi, res, out_f32):
    """Reference and bound of the row-major epilogues behind accumulator + bias `pre` (bound b_pre)."""
    y, b = pre, b_pre
    if epi == "silu":
        y, b = _silu_bound(pre, b_pre)
    if res is not None:
        b = b + U * (res.abs() + y.abs())
        y = y + res
    if not out_f32:
        b = b + BF16_ULP * y.abs()
    return y, b


_cache = {}


def _lin_tensors(M, N, K):
    import torch
    key = ("lin", M, N, K)
    if key not in _cache:
        _cache.clear()
        x, w = _rnd((M, K), 1).bfloat16(), _rnd((N, K), 2, K ** -0.5).bfloat16()
        b, res = _rnd((N,), 3), _rnd((M, N), 4).bfloat16()
        x64, w64 = x.double(), w.double()
        _cache[key] = dict(x=x, w=w, b=b, res=res, acc=x64 @ w64.t() + b.double(), S=x64.abs() @ w64.abs().t() + b.double().abs())
    return _cache[key]


def make_case(prob, dev):
    """Device inputs, and ref(splits) -> (float64 reference, elementwise bound) on the device, for one problem."""
    import torch
    import torch.nn.functional as F
    a, op = prob["args"], prob["op"]
    if op == "linear":
        t = _lin_tensors(a["M"], a["N"], a["K"])
        epi = a["epi"]
        res = t["res"] if epi == "res" else None
        f32 = epi == "f32"
        acc, S, K = t["acc"].to(dev), t["S"].to(dev), a["K"]
        res64 = None if res is None else res.double().to(dev)
        ins = dict(x=t["x"].to(dev), w=t["w"].to(dev), b=t["b"].to(dev), res=None if res is None else res.to(dev))
        shape, dtype = (a["M"], a["N"]), (torch.float32 if f32 else torch.bfloat16)

        def ref(splits):
            return _finish(acc, (K + 1 + (splits if splits > 1 else 0)) * U * S, epi, res64, f32)
    elif op == "geglu":
        M, inner, K = a["M"], a["inner"], a["K"]
        x, w, b = _rnd((M, K), 1).bfloat16(), _rnd((2 * inner, K), 2, K ** -0.5).bfloat16().float(), _rnd((2 * inner,), 3)
        x64, w64 = x.double(), w.double()
        h = (x64 @ w64.t() + b.double()).to(dev)
        S = (x64.abs() @ w64.abs().t() + b.double().abs()).to(dev)
        ins = dict(x=x.to(dev), w=w.to(dev), b=b.to(dev))
        shape, dtype = (M, inner), torch.bfloat16

        def ref(splits):
            return geglu_finish(h, (K + 1 + (splits if splits > 1 else 0)) * U * S, inner)
    else:
        B, H, W, C0, C1, Cout = a["B"], a["H"], a["W"], a["C0"], a["C1"], a["Cout"]
        Cin = C0 + C1
        x0 = _rnd((B, H, W, C0), 1).bfloat16()
        x1 = _rnd((B, H, W, C1), 2).bfloat16() if C1 else None
        if a["phase"]:
            # the phase form sums up to four taps into one weight before rounding it to bf16: multiples of 2^-9 below 2^-4 keep every
            # such sum exact in bf16 (8 significant bits), so the nine-tap float64 reference has the kernel's own weights
            g = torch.Generator().manual_seed(3)
            w = torch.randint(-31, 32, (Cout, Cin, 3, 3), generator=g).float() * 2.0 ** -9
        else:
            w = _rnd((Cout, Cin, 3, 3), 3, (9 * Cin) ** -0.5).bfloat16().float()
        b = _rnd((Cout,), 4)
        xin = (x0 if x1 is None else torch.cat([x0, x1], dim=-1)).double().permute(0, 3, 1, 2)
        if a["ups"]:
            xin = F.interpolate(xin, scale_factor=2, mode="nearest")

        def conv(x_, w_, b_):
            if a["stride"] == 2 and not a["pad_lo"]:
                return F.conv2d(F.pad(x_, (0, 1, 0, 1)), w_, b_, stride=2, padding=0)
            return F.conv2d(x_, w_, b_, stride=a["stride"], padding=1)
        acc = conv(xin, w.double(), b.double()).permute(0, 2, 3, 1).contiguous().to(dev)
        S = conv(xin.abs(), w.double().abs(), b.double().abs()).permute(0, 2, 3, 1).contiguous().to(dev)
        res = _rnd(tuple(acc.shape), 5).bfloat16() if a["res"] else None
        res64 = None if res is None else res.double().to(dev)
        ins = dict(x0=x0.to(dev), x1=None if x1 is None else x1.to(dev), w=w.to(dev), b=b.to(dev), res=None if res is None else res.to(dev))
        shape, dtype = tuple(acc.shape), torch.bfloat16
        K = 9 * Cin

        def ref(splits):
            return _finish(acc, (K + 1 + (splits if splits > 1 else 0)) * U * S, "plain", res64, False)
    return dict(ins=ins, shape=shape, dtype=dtype, ref=ref)


def run_op(eng, prob, ins, out):
    """One call of the problem's operator into `out` (a view between guard zones)."""
    from gligen_amd.engine import _ptr, _stream
    from gligen_amd._lib import check
    a, lib, ctx, st = prob["args"], eng.lib, eng._ctx, _stream(eng.device)
    if prob["op"] == "linear":
        check(lib.gl_op_linear(ctx, _ptr(ins["x"]), _ptr(ins["w"]), _ptr(ins["b"]), _ptr(ins["res"]), _ptr(out), a["M"], a["N"], a["K"],
                               1 if a["epi"] == "silu" else 0, 1 if a["epi"] == "f32" else 0, st))
    elif prob["op"] == "geglu":
        check(lib.gl_op_geglu(ctx, _ptr(ins["x"]), _ptr(ins["w"]), _ptr(ins["b"]), _ptr(out), a["M"], a["inner"], a["K"], st))
    else:
        check(lib.gl_op_conv3x3(ctx, _ptr(ins["x0"]), a["C0"], _ptr(ins["x1"]), a["C1"], a["B"], a["H"], a["W"], _ptr(ins["w"]), _ptr(ins["b"]), a["Cout"],
                                a["stride"], a["ups"], a["pad_lo"], _ptr(ins["res"]), _ptr(out), st))


if __name__ == "__main__":
    import sys
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        payload = fixture_payload(ask_planner(build_planner(os.path.join(d, "gemm_plan_main"), sanitize=False)))
    text = dump_fixture(payload)
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            f.write(text)
    print(f"{len(payload['problems'])} problems, {len(payload['answers'])} distinct answers, {len(text)} bytes")
