"""The epilogues the model's own launches use beyond those of tests/gemm_candidates_ref.py, each under every plan the planner can give
its launch, element by element against float64 (tests/test_gemm_epilogues_cpu.py, tests/test_gemm_epilogues_gpu.py with its child
tests/gemm_epilogues_child.py). The launches go through gl_op_gemm_epilogue / gl_op_attention_project_range
(include/gligen_amd_gemm_plans.h) and gl_op_gn_silu_conv3x3(mode = 1); which plans a problem can run with comes from the planner
(tests/gemm_plan_main.hip, mode `candidates`) and is kept as tests/golden/gemm_epilogues.json, exactly as in gemm_candidates_ref.py,
whose helpers (input_line, ask_planner, launches, load_fixture, ...) are used here.

A problem's case (make_case) is a list of steps, each one call of the operator; a step says, for every output buffer, what the call
has to leave there: (ref, bound, mask[, exact]) over the WHOLE buffer -- inside `mask` |got - ref| <= bound, outside it the bits the
buffer had before the call, and where `exact` is given those very bits. check_output is the one function that decides this; the child
applies it to the device's output and the CPU test to the rounded reference and to planted defects.

Bounds (derived; u = 2^-24, ref and S = sum_k |a_k| |w_k| in float64 on the bf16-rounded inputs, conventions of gemm_candidates_ref.py):
    accumulator + bias      e_v = L u (S + |bias|), L = K + 1 additions (+ `splits` slab additions behind a K split)
    per-sample bias2        one more addition: e_v = (K + 2 [+ splits]) u (S + |bias| + |bias2|)
    gated residual          y = res + g v with g the fp32 device scalar: the error of v scaled, the product and the sum rounded once each:
                            |g| e_v + 2 u (|res| + |g v|), then the output rounding; g = 0 gives res itself, bit for bit
    GELU                    |gelu'| <= 1.13; erf by Abramowitz & Stegun 7.1.26 (|erf error| <= 1.5e-7) in about 16 fp32 operations on values
                            <= 1: 1.13 e_v + |v| / 2 (1.5e-7 + 16 u)
    quick-GELU              v sigmoid(1.702 v) = silu(1.702 v) / 1.702: the SiLU bound of gemm_candidates_ref.py with its argument scaled,
                            (3.404 |v| + 6) u |y|, behind the slope 1.1 (the slope of silu(c v) / c is that of silu)
    NCHW fp32               the sum itself: e_v
    row remap, tok_off      only change addresses
    bf16 output             + 2^-8 |ref|
    GroupNorm prologue      the conv multiplies xn = bf16(silu(x a + c)) with the per-(sample, channel) coefficients of the coefficient
                            kernel: a, c and their bounds da, e_c from tests/norm_ref.py gn_expect; x a + c is one fused multiply-add:
                            |x| da + e_c + u |x a + c|, through the SiLU (slope 1.1 and its own terms), + 2^-8 |xn| for the rounding to
                            bf16 = e_xn; carried through |W| as ln_fallback_ref carries the LayerNorm's: sum |w| e_xn, plus the accumulation
                            terms above with S = sum |w| (|xn| + e_xn)
"""
import os
from types import SimpleNamespace

import gemm_candidates_ref as R
from gemm_candidates_ref import BF16_ULP, GUARD, U, _rnd  # noqa: F401

FIXTURE = os.path.join(R.ROOT, "tests", "golden", "gemm_epilogues.json")
GATES = (0.37, -0.6, 0.0)
ACTS = {"gelu": 3, "quick_gelu": 4}
EPI_NCHW_F32, EPI_QKV_HEADS = 3, 4
RANGE_TR = 64


# ---------------------------------------------------------------------------------------------------------------- the problems
def _gate(M, N, K, g, group, **kw):
    return dict(id=f"gate{g}_{M}x{N}x{K}", group=group, op="rows", args=dict(M=M, N=N, K=K, epi="gate", gate=g),
                desc=dict(M=M, N=N, K=K, C0=K, ld0=K, res=1, gate=1), **kw)


def _act(M, N, K, act, group):
    return dict(id=f"{act}_{M}x{N}x{K}", group=group, op="rows", args=dict(M=M, N=N, K=K, epi=act), desc=dict(M=M, N=N, K=K, C0=K, ld0=K, act=ACTS[act]))


def _remap(M, N, K, rin, rout, offs, group):
    return dict(id=f"remap_{M}x{N}x{K}_{rin}to{rout}", group=group, op="rows", args=dict(M=M, N=N, K=K, epi="remap", remap_in=rin, remap_out=rout, offs=offs),
                desc=dict(M=M, N=N, K=K, C0=K, ld0=K, remap_in=rin))


def _conv(B, H, W, C0, C1, N, group, n_real=0, **kw):
    """A stride-1 3x3 conv through gl_op_gemm_epilogue: with the per-sample bias [B][N + 4] (a leading dimension of its own), or as
    the model's last conv (N = 32 padded channels, EPI_NCHW_F32 with n_real of them real)."""
    K, HW = 9 * (C0 + C1), H * W
    desc = dict(M=B * HW, N=N, K=K, a_mode=1, C0=C0, C1=C1, ld0=C0, ld1=C1, Hin=H, Win=W, Ho=H, Wo=W, stride=1, pad_lo=1, rows_per_b=HW)
    desc.update(dict(e_mode=EPI_NCHW_F32) if n_real else dict(bias2=1, bias2_ld=N + 4))
    return dict(id=f"{'nchw' if n_real else 'b2conv'}_{B}x{H}x{W}_{C0}+{C1}to{n_real or N}", group=group, op="conv",
                args=dict(B=B, H=H, W=W, C0=C0, C1=C1, N=N, n_real=n_real), desc=desc, **kw)


def _gnconv(B, H, W, C0, C1, N, extra, group):
    """gl_op_gn_silu_conv3x3(mode = 1): the GroupNorm prologue of conv_halo_kernel with the per-sample bias or the residual."""
    K, HW = 9 * (C0 + C1), H * W
    desc = dict(M=B * HW, N=N, K=K, a_mode=1, C0=C0, C1=C1, ld0=C0, ld1=C1, Hin=H, Win=W, Ho=H, Wo=W, stride=1, pad_lo=1, gn=1, rows_per_b=HW)
    desc.update(dict(bias2=1, bias2_ld=N) if extra == "bias2" else dict(res=1))
    return dict(id=f"gnconv_{B}x{H}x{W}_{C0}+{C1}to{N}_{extra}", group=group, op="gnconv", args=dict(B=B, H=H, W=W, C0=C0, C1=C1, N=N, extra=extra), desc=desc)


def _range(B, tok_off, C, group, heads=8):
    M = B * RANGE_TR
    return dict(id=f"range_{B}x{tok_off}+{RANGE_TR}_C{C}", group=group, op="range", args=dict(B=B, tok_off=tok_off, Tr=RANGE_TR, C=C, H=heads),
                desc=dict(M=M, N=3 * C, K=C, C0=C, ld0=C, e_mode=EPI_QKV_HEADS, q=1, k=1, vt=1, C=C, T=RANGE_TR))


def _problems():
    out = []
    for M, N, K in [(100, 320, 640), (333, 960, 1536)]:
        out += [_gate(M, N, K, g, "epi_rows") for g in GATES]
    out += [_remap(90, 768, 512, 30, 64, (0, 30), "epi_rows")]
    for M, N, K in [(100, 384, 640), (333, 1024, 768)]:
        out += [_act(M, N, K, act, "epi_rows") for act in ACTS]
    out += [_gate(256, 1280, 1280, g, "epi_wide", wide=2) for g in GATES]
    # gemm_glds_kernel: its split rule (K = 1024) and no split (K = 128); M = 40 adds the 64 x 64 tile
    for M, N, K in [(100, 64, 1024), (100, 96, 128), (40, 64, 1024)]:
        out += [_gate(M, N, K, g, "epi_glds") for g in GATES]
    # rows_per_b = 64: a 128-row tile holds two samples; rows_per_b = 240, M = 720 ragged, two sources; N = 64: gemm_glds_kernel
    out += [_conv(4, 8, 8, 128, 0, 192, "epi_conv"), _conv(3, 12, 20, 128, 64, 160, "epi_conv"), _conv(3, 12, 20, 128, 0, 64, "epi_conv")]
    # conv_halo_kernel's shapes (a tile is 8 rows of one image; each tile another sample), also on gemm_u_kernel under every forced tile
    out += [_conv(2, 32, 32, 128, 0, 160, "epi_halo"), _conv(2, 32, 32, 320, 0, 160, "epi_halo"), _conv(8, 16, 16, 128, 0, 128, "epi_halo")]
    # 192 channels in 32 groups of 6: the groups 21 and 22 straddle the boundary between the two sources
    out += [_gnconv(2, 32, 32, 128, 64, 160, extra, "epi_halo") for extra in ("bias2", "res")]
    out += [_conv(2, 16, 16, 128, 0, 32, "epi_nchw", n_real=3), _conv(2, 12, 20, 320, 0, 32, "epi_nchw", n_real=4), _conv(1, 16, 16, 128, 0, 32, "epi_nchw", n_real=8)]
    # 256 row tiles: gemm_glds_kernel does not split, its own epilogue stores the planes (the model's last convs at full size)
    out += [_conv(2, 128, 128, 64, 0, 32, "epi_nchw", n_real=4)]
    out += [_range(B, off, C, "epi_heads") for C in (320, 640) for B in (1, 3) for off in (64, 256)]
    ids = [p["id"] for p in out]
    assert len(set(ids)) == len(ids), "problem ids are unique"
    return out


PROBLEMS = _problems()
GROUPS = ["epi_rows", "epi_wide", "epi_glds", "epi_conv", "epi_halo", "epi_nchw", "epi_heads"]
PROVENANCE = ("tests/gemm_plan_main.hip, mode `candidates`, over tests/gemm_epilogues_ref.py PROBLEMS; regenerate with "
              "`python tests/gemm_epilogues_ref.py --write` (tests/test_gemm_epilogues_cpu.py holds it to the planner)")


def load_fixture():
    return R.load_fixture(FIXTURE)


def launches(prob, fx):
    """As gemm_candidates_ref.launches; the head-layout launches name their instantiation."""
    ls = R.launches(prob, fx)
    if prob["op"] == "range":
        for l in ls:
            e = l["expect"]
            e["kernel"] = f"gemm_u_kernel<2, {e['tm']}, {e['tn']}, 0, 2, true>"
    return ls


# ---------------------------------------------------------------------------------------------------------------- the checker
def _bits(t):
    import torch
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def check_output(out, before, ref, bound, mask, exact=None):
    """(findings, worst err / bound). out, before: the buffer after and before the call; ref, bound (float64), mask (bool) of its shape."""
    import torch
    findings = []
    if bool(torch.isnan(out.double()[mask]).any()):
        findings.append(f"{int(torch.isnan(out.double()[mask]).sum())} NaN left")
    ratio = float(((out.double() - ref).abs() / bound.clamp_min(1e-300))[mask].max()) if bool(mask.any()) else 0.0
    if not ratio <= 1.0:
        findings.append(f"err / bound = {ratio}")
    changed = (_bits(out) != _bits(before)) & ~mask
    if bool(changed.any()):
        findings.append(f"{int(changed.sum())} elements outside the written range changed (first at flat index {int(changed.flatten().nonzero()[0])})")
    if exact is not None:
        where, values = exact
        off = (_bits(out) != _bits(values.to(out.dtype))) & where
        if bool(off.any()):
            findings.append(f"{int(off.sum())} elements are not the bits they have to be")
    return findings, ratio


# ---------------------------------------------------------------------------------------------------------------- cases
def _L(K, splits, extra=0):
    return (K + 1 + extra + (splits if splits > 1 else 0)) * U


def range_layout(C, H, T):
    """gl_attn_proj_layout of gl_op_attention_project for Nq = Nk = T (T % 64 == 0): the child holds it to the library's."""
    d = C // H
    perm = 1 if T > 128 and d in (40, 80) else 0
    return SimpleNamespace(d=d, dp={40: 48, 80: 80, 160: 160}[d], dpv=48 if perm and d == 40 else {40: 64, 80: 96, 160: 160}[d], tq=T, tk=T,
                           tq_pad=-(-T // 128) * 128, tk_pad=T, vt_perm32=perm)


def _rows_case(prob, dev):
    import torch
    a = prob["args"]
    M, N, K, epi = a["M"], a["N"], a["K"], a["epi"]
    t = R._lin_tensors(M, N, K)
    ins = dict(x=t["x"].to(dev), w=t["w"].to(dev), b=t["b"].to(dev))
    acc, S = t["acc"].to(dev), t["S"].to(dev)
    every = torch.ones((M, N), dtype=torch.bool, device=dev)
    if epi == "gate":
        g = float(torch.tensor(a["gate"], dtype=torch.float32))
        res = t["res"]
        res64 = res.double().to(dev)
        ins.update(res=res.to(dev), gate=torch.tensor([a["gate"]], dtype=torch.float32).to(dev))

        def expect(splits):
            gv = g * acc
            y = res64 + gv
            b = abs(g) * _L(K, splits) * S + 2 * U * (res64.abs() + gv.abs()) + BF16_ULP * y.abs()
            return dict(out=(y, b, every, (every, res64) if g == 0 else None))
        steps = [dict(call=dict(res="res", gate="gate"), expect=expect)]
        shape = (M, N)
    elif epi in ACTS:
        def expect(splits):
            e_v = _L(K, splits) * S
            if epi == "gelu":
                y = acc * 0.5 * (1 + torch.erf(acc * 2 ** -0.5))
                b = 1.13 * e_v + 0.5 * acc.abs() * (1.5e-7 + 16 * U)
            else:
                y = acc * torch.sigmoid(1.702 * acc)
                b = 1.1 * e_v + (3.404 * acc.abs() + 6) * U * y.abs()
            return dict(out=(y, b + BF16_ULP * y.abs(), every, None))
        steps = [dict(call=dict(act=ACTS[epi]), expect=expect)]
        shape = (M, N)
    else:
        rin, rout, nb = a["remap_in"], a["remap_out"], M // a["remap_in"]
        shape = (nb * rout, N)
        x2 = _rnd((M, K), 11).bfloat16()
        ins["x2"] = x2.to(dev)
        w64, b64 = t["w"].double(), t["b"].double()
        acc2, S2 = (x2.double() @ w64.t() + b64).to(dev), (x2.double().abs() @ w64.abs().t() + b64.abs()).to(dev)
        steps = []
        for off, xname, ac, s_ in zip(a["offs"], ("x", "x2"), (acc, acc2), (S, S2)):
            def expect(splits, off=off, ac=ac, s_=s_):
                rows = (torch.arange(M, device=dev) // rin) * rout + torch.arange(M, device=dev) % rin + off
                y, b, m = (torch.zeros(shape, dtype=torch.float64, device=dev), torch.zeros(shape, dtype=torch.float64, device=dev),
                           torch.zeros(shape, dtype=torch.bool, device=dev))
                y[rows], b[rows], m[rows] = ac, _L(K, splits) * s_ + BF16_ULP * ac.abs(), True
                return dict(out=(y, b, m, None))
            steps.append(dict(call=dict(x=xname, remap_in=rin, remap_out=rout, remap_off=off), expect=expect))
    return dict(ins=ins, bufs=dict(out=(shape, torch.bfloat16, float("nan"))), steps=steps)


def _conv_inputs(a, dev, gn=False):
    """x0, x1, w, b and, in float64 on the device, what the conv multiplies: xin [B][Cin][H][W]."""
    import torch
    B, H, W, C0, C1, N = a["B"], a["H"], a["W"], a["C0"], a["C1"], a["N"]
    Cin = C0 + C1
    x0 = _rnd((B, H, W, C0), 1).bfloat16()
    x1 = _rnd((B, H, W, C1), 2).bfloat16() if C1 else None
    w = _rnd((N, Cin, 3, 3), 3, (9 * Cin) ** -0.5).bfloat16().float()
    b = _rnd((N,), 4)
    ins = dict(x0=x0.to(dev), x1=None if x1 is None else x1.to(dev), w=w.to(dev), b=b.to(dev))
    x = (x0 if x1 is None else torch.cat([x0, x1], dim=-1)).double()
    return ins, x, w.double(), b.double()


def _conv64(x_nhwc, w, b):
    """3x3 / stride 1 / pad 1 in float64, NHWC in and out."""
    import torch.nn.functional as F
    return F.conv2d(x_nhwc.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1).contiguous()


def _conv_case(prob, dev):
    import torch
    a = prob["args"]
    B, H, W, N, n_real = a["B"], a["H"], a["W"], a["N"], a["n_real"]
    HW, K = H * W, 9 * (a["C0"] + a["C1"])
    ins, x, w64, b64 = _conv_inputs(a, dev)
    acc, S = _conv64(x, w64, b64).to(dev), _conv64(x.abs(), w64.abs(), b64.abs()).to(dev)
    if n_real:
        shape = (B, n_real, HW)
        y = acc.view(B, HW, N)[:, :, :n_real].permute(0, 2, 1).contiguous()
        s_ = S.view(B, HW, N)[:, :, :n_real].permute(0, 2, 1).contiguous()
        every = torch.ones(shape, dtype=torch.bool, device=dev)
        steps = [dict(call=dict(mode=EPI_NCHW_F32, n_real=n_real, rows_per_b=HW), expect=lambda splits: dict(out=(y, _L(K, splits) * s_, every, None)))]
        return dict(ins=ins, bufs=dict(out=(shape, torch.float32, float("nan"))), steps=steps)
    ld = N + 4
    bias2 = _rnd((B, ld), 6)
    ins["bias2"] = bias2.to(dev)
    b2 = bias2[:, :N].double().to(dev)[:, None, None, :]
    shape = (B * HW, N)
    every = torch.ones(shape, dtype=torch.bool, device=dev)

    def expect(splits):
        y = (acc + b2).view(shape)
        return dict(out=(y, _L(K, splits, 1) * (S + b2.abs()).view(shape) + BF16_ULP * y.abs(), every, None))
    return dict(ins=ins, bufs=dict(out=(shape, torch.bfloat16, float("nan"))), steps=[dict(call=dict(bias2="bias2", bias2_ld=ld, rows_per_b=HW), expect=expect)],
                parts=dict(bias2=b2, rows_per_b=HW))


def _gnconv_case(prob, dev):
    import torch
    import norm_ref as NR
    a = prob["args"]
    B, H, W, C0, C1, N = a["B"], a["H"], a["W"], a["C0"], a["C1"], a["N"]
    HW, C, K, eps = H * W, C0 + C1, 9 * (C0 + C1), 1e-5
    ins, x, w64, b64 = _conv_inputs(a, dev)
    gamma, beta = 1 + 0.2 * _rnd((C,), 8), 0.2 * _rnd((C,), 9)
    ins.update(gamma=gamma.to(dev), beta=beta.to(dev))
    c = SimpleNamespace(B=B, HW=HW, C0=C0, C1=C1, silu=True, eps=eps)
    x0c, x1c = x[..., :C0].reshape(B, HW, C0), x[..., C0:].reshape(B, HW, C1)
    _, _, (ca, da), (cc, e_c) = NR.gn_expect(c, dict(x0=x0c, x1=x1c, gamma=gamma, beta=beta))
    xr = x.view(B, HW, C)
    pre = xr * ca[:, None] + cc[:, None]
    e_pre = xr.abs() * da[:, None] + e_c[:, None] + U * pre.abs()
    xn, e_s = R._silu_bound(pre, e_pre)
    e_xn = (e_s + BF16_ULP * xn.abs()).view(B, H, W, C)
    xn = xn.view(B, H, W, C)
    zero = torch.zeros_like(b64)
    acc, carried = _conv64(xn, w64, b64).to(dev), _conv64(e_xn, w64.abs(), zero).to(dev)
    S = _conv64(xn.abs() + e_xn, w64.abs(), b64.abs()).to(dev)
    shape = (B * HW, N)
    every = torch.ones(shape, dtype=torch.bool, device=dev)
    if a["extra"] == "bias2":
        bias2 = _rnd((B, N), 6)
        ins["bias2"] = bias2.to(dev)
        b2 = bias2.double().to(dev)[:, None, None, :]

        def expect(splits):
            y = (acc + b2).view(shape)
            return dict(out=(y, (carried + _L(K, splits, 1) * (S + b2.abs())).view(shape) + BF16_ULP * y.abs(), every, None))
    else:
        res = _rnd((B * HW, N), 5).bfloat16()
        ins["res"] = res.to(dev)
        res64 = res.double().to(dev)

        def expect(splits):
            v = acc.view(shape)
            y = v + res64
            return dict(out=(y, (carried + _L(K, splits) * S).view(shape) + U * (res64.abs() + v.abs()) + BF16_ULP * y.abs(), every, None))
    return dict(ins=ins, bufs=dict(out=(shape, torch.bfloat16, float("nan"))), steps=[dict(call=dict(eps=eps), expect=expect)])


def range_positions(lay, B, H, dev):
    """Per buffer (q, k, vt): its element count and the flat index of every (b, token, feature) in it, [B][T][C], by the header's layouts."""
    import torch
    sizes = dict(q=B * H * lay.tq_pad * lay.dp, k=B * H * lay.tk_pad * lay.dp, vt=B * H * lay.dpv * lay.tk_pad)
    return {n: (sz, R.proj_region(lay, B, H, n, torch.arange(sz, device=dev))[1]) for n, sz in sizes.items()}


def _range_case(prob, dev):
    import torch
    a = prob["args"]
    B, off, Tr, C, H = a["B"], a["tok_off"], a["Tr"], a["C"], a["H"]
    T = off + Tr
    lay = range_layout(C, H, T)
    x_first, x = _rnd((B, T, C), 1).bfloat16(), _rnd((B, Tr, C), 5).bfloat16()
    ws = [_rnd((C, C), s, C ** -0.5).bfloat16().float() for s in (2, 3, 4)]
    bias = _rnd((3 * C,), 6)
    ins = dict(x_first=x_first.to(dev), x=x.to(dev), wq=ws[0].to(dev), wk=ws[1].to(dev), wv=ws[2].to(dev), bias=bias.to(dev))
    pos = range_positions(lay, B, H, dev)
    x64 = x.double()
    refs = {}
    for i, n in enumerate(("q", "k", "vt")):
        bi = bias[i * C:(i + 1) * C].double()
        refs[n] = ((x64 @ ws[i].double().t() + bi).to(dev), (x64.abs() @ ws[i].double().abs().t() + bi.abs()).to(dev))

    def expect(splits, tok_off=off):
        out = {}
        for n, (sz, p) in pos.items():
            sel = p[:, tok_off:tok_off + Tr].reshape(-1)
            y, b, m = torch.zeros(sz, dtype=torch.float64, device=dev), torch.zeros(sz, dtype=torch.float64, device=dev), torch.zeros(sz, dtype=torch.bool, device=dev)
            r, s_ = refs[n]
            y[sel], b[sel], m[sel] = r.reshape(-1), (_L(C, splits) * s_ + BF16_ULP * r.abs()).reshape(-1), True
            out[n] = (y, b, m, None)
        return out
    bufs = {n: ((sz,), torch.bfloat16, 7.0) for n, (sz, _) in pos.items()}
    return dict(ins=ins, bufs=bufs, steps=[dict(call=dict(first=True), expect=None), dict(call=dict(), expect=expect)], layout=lay, expect_at=expect)


def make_case(prob, dev):
    """ins, bufs {name: (shape, dtype, fill)} and steps [{call, expect(splits) -> {name: (ref, bound, mask, exact)} or None}]."""
    return {"rows": _rows_case, "conv": _conv_case, "gnconv": _gnconv_case, "range": _range_case}[prob["op"]](prob, dev)


def simulate(case, splits=1):
    """What a correct kernel leaves: per step that is held to a reference, ({name: before}, {name: after}) with the float64 reference
    rounded to the buffer's type inside the mask (CPU self-test of the checker)."""
    import torch
    state = {n: torch.full(shape, fill, dtype=dtype) for n, (shape, dtype, fill) in case["bufs"].items()}
    out = []
    for step in case["steps"]:
        if step["expect"] is None:
            continue
        want = step["expect"](splits)
        before = {n: t.clone() for n, t in state.items()}
        for n, (ref, _, mask, _) in want.items():
            state[n] = torch.where(mask, ref.to(state[n].dtype), state[n])
        out.append((before, {n: t.clone() for n, t in state.items()}, want))
    return out


# ---------------------------------------------------------------------------------------------------------------- running a step
def run_step(eng, prob, case, step, views):
    """One call of the problem's operator (the GPU child)."""
    import ctypes
    from gligen_amd._lib import AttnProjLayout, GemmEpilogueArgs, check
    from gligen_amd.engine import _ptr, _stream
    a, ins, call, lib, ctx, st = prob["args"], case["ins"], step["call"], eng.lib, eng._ctx, _stream(eng.device)
    if prob["op"] == "range":
        lay = AttnProjLayout()
        T = a["tok_off"] + a["Tr"]
        check(lib.gl_op_attention_project(ctx, None, None, a["B"], T, T, a["C"], a["C"], a["H"], None, None, None, None, None, None, ctypes.byref(lay), None))
        want = case["layout"]
        assert all(getattr(lay, f) == getattr(want, f) for f, _ in AttnProjLayout._fields_), "range_layout is not the library's layout"
        if call.get("first"):
            check(lib.gl_op_attention_project(ctx, _ptr(ins["x_first"]), _ptr(ins["x_first"]), a["B"], T, T, a["C"], a["C"], a["H"], _ptr(ins["wq"]), _ptr(ins["wk"]),
                                              _ptr(ins["wv"]), _ptr(views["q"]), _ptr(views["k"]), _ptr(views["vt"]), ctypes.byref(lay), st))
        else:
            check(lib.gl_op_attention_project_range(ctx, _ptr(ins["x"]), a["B"], a["Tr"], a["tok_off"], a["C"], a["H"], _ptr(ins["wq"]), _ptr(ins["wk"]), _ptr(ins["wv"]),
                                                    _ptr(ins["bias"]), _ptr(views["q"]), _ptr(views["k"]), _ptr(views["vt"]), ctypes.byref(lay), st))
        return
    if prob["op"] == "gnconv":
        used = ctypes.c_int(-1)
        check(lib.gl_op_gn_silu_conv3x3(ctx, _ptr(ins["x0"]), a["C0"], _ptr(ins["x1"]), a["C1"], a["B"], a["H"], a["W"], _ptr(ins["gamma"]), _ptr(ins["beta"]),
                                        ctypes.c_float(call["eps"]), _ptr(ins["w"]), _ptr(ins["b"]), a["N"], _ptr(ins.get("bias2")), _ptr(ins.get("res")), _ptr(views["out"]), 1,
                                        ctypes.byref(used), st))
        assert used.value == 1
        return
    g = GemmEpilogueArgs()
    g.struct_size = ctypes.sizeof(GemmEpilogueArgs)
    g.N, g.bias, g.rows_per_b, g.out = a["N"], _ptr(ins["b"]), call.get("rows_per_b", 1), _ptr(views["out"])
    g.ldo = g.ldres = a["N"]
    if prob["op"] == "conv":
        g.conv, g.x0, g.x1, g.w = 1, _ptr(ins["x0"]), _ptr(ins["x1"]), _ptr(ins["w"])
        g.C0, g.C1, g.B, g.H, g.W, g.stride, g.ups, g.pad_lo = a["C0"], a["C1"], a["B"], a["H"], a["W"], 1, 0, 1
    else:
        g.M, g.K, g.x0, g.w = a["M"], a["K"], _ptr(ins[call.get("x", "x")]), _ptr(ins["w"])
    for f in ("res", "gate", "bias2"):
        if f in call:
            setattr(g, f, _ptr(ins[call[f]]))
    for f in ("act", "mode", "n_real", "bias2_ld", "remap_in", "remap_out", "remap_off"):
        setattr(g, f, call.get(f, 0))
    check(lib.gl_op_gemm_epilogue(ctx, ctypes.byref(g), st))


if __name__ == "__main__":
    import sys
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        payload = R.fixture_payload(R.ask_planner(R.build_planner(os.path.join(d, "gemm_plan_main"), sanitize=False), PROBLEMS), PROBLEMS, PROVENANCE)
    text = R.dump_fixture(payload)
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            f.write(text)
    print(f"{len(payload['problems'])} problems, {len(payload['answers'])} distinct answers, {len(text)} bytes")
