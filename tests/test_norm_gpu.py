"""The normalisation kernels of norm.hip by themselves (gn_stats_kernel + gn_apply_kernel / gn_coef_kernel, gn_small_kernel and
gn_small_coef_kernel <256 | 1024>, ln_kernel), every output element against float64 and the derived bound of norm_ref, at the ragged
sizes the engine meets since any image size is accepted (HW = 45, 180, 720, 2880), at every switch between two kernels, with empty
statistics blocks, several trips per apply block and 576-addition chains.

Per case (norm_ref.CASES; test_norm_cpu.py holds the list to what it has to reach):
  * y of gl_op_groupnorm, the coefficients of gl_op_groupnorm_coef at their layout [c >> 3][16], y of gl_op_layernorm_rows: finite,
    |got - ref| <= bound per element -- bit-equal to the reference's bf16 wherever no rounding boundary is within the bound's reach --
    and within the project's bars as a whole (max |err| / max |ref| < 2.5e-2, mean |err| / mean |ref| < 1e-2);
  * on the two-launch path without SiLU, y is bit-equal to bf16(fma(x, a, c)) of the coefficient bits the device returned;
  * every output buffer is random finite data with GUARD elements in front and behind, which keep their bits; LayerNorm's pad rows
    and its columns [C, ldy) are zero to the bit;
  * a second run gives the same bits.
A sample's output inside a batch is bit-equal to that sample's alone; a refused call raises its documented code and writes nothing.
Measured on MI355X: profiles/norm/err_over_bound.txt."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import norm_ref as N
from gligen_amd._lib import GligenAmdError, check
from gligen_amd.engine import _ptr, _stream

pytestmark = pytest.mark.gpu


def groupnorm(engine, x0, C0, x1, C1, B, HW, gamma, beta, eps, silu, y):
    """gl_op_groupnorm from the binding itself: y is the caller's."""
    check(engine.lib.gl_op_groupnorm(engine._ctx, _ptr(x0), C0, _ptr(x1), C1, B, HW, _ptr(gamma), _ptr(beta), ctypes.c_float(eps), int(silu), _ptr(y),
                                     _stream(engine.device)))


def launch(engine, c, ins, outs):
    """(the number of launches gl_op_groupnorm_coef reports, or None)"""
    if c.kind == "ln":
        engine.op_layernorm_rows(**N.ln_fields(c, ins, outs))
        return None
    groupnorm(engine, *N.gn_call(c, ins, outs))
    return engine.op_groupnorm_coef(ins["x0"], c.C0, ins["gamma"], ins["beta"], c.eps, outs["coef"].payload, x1=ins["x1"], C1=c.C1, B=c.B, HW=c.HW)


def run_case(engine, c, ins=None):
    dev = engine.device
    ins = N.make_inputs(c, dev) if ins is None else ins
    outs = N.make_outputs(c, dev)
    n = launch(engine, c, ins, outs)
    torch.cuda.synchronize(dev)
    if c.kind == "gn":
        assert n == (2 if N.gn_path(c.HW, c.C0, c.C1) == "two_pass" else 1), (c.name, "launches", n)
    worst = N.verify(c, ins, outs)
    first = {k: b.flat.clone() for k, b in outs.items()}
    for b in outs.values():
        b.reset()
    launch(engine, c, ins, outs)
    for k, b in outs.items():
        assert torch.equal(b.flat.view(b.bits), first[k].view(b.bits)), (c.name, k, "two runs differ")
    print(N.report_line(c, worst))
    return ins, outs


@pytest.mark.parametrize("c", N.GN_CASES, ids=[c.name for c in N.GN_CASES])
def test_groupnorm_kernels(engine, c):
    ins, outs = run_case(engine, c)
    if c.inp == "constant" and N.gn_path(c.HW, c.C0, c.C1) != "two_pass" and not c.silu:
        # variance 0: x - mean is exactly 0 in the small form, so the group's output is bf16(beta)
        cpg = (c.C0 + c.C1) // 32
        y = outs["y"].get()[:, 5 * cpg: 6 * cpg]
        assert torch.equal(y, ins["beta"][5 * cpg: 6 * cpg].bfloat16().expand_as(y))


@pytest.mark.parametrize("c", N.LN_CASES, ids=[c.name for c in N.LN_CASES])
def test_layernorm_kernel(engine, c):
    run_case(engine, c)


@pytest.mark.parametrize("name", ["two_pass_cpg30_cat_45", "small_ragged_45"])
def test_a_sample_does_not_depend_on_its_batch(engine, name):
    """Statistics leaking across blockIdx.y would show: every sample alone gives the bits it gives inside the batch."""
    c = next(c for c in N.GN_CASES if c.name == name)
    assert c.B == 3
    dev = engine.device
    ins = N.make_inputs(c, dev)
    outs = N.make_outputs(c, dev)
    launch(engine, c, ins, outs)
    one = SimpleNamespace(**{**vars(c), "B": 1})
    for b in range(c.B):
        ins1 = dict(ins, x0=ins["x0"][b: b + 1], x1=None if ins["x1"] is None else ins["x1"][b: b + 1])
        outs1 = N.make_outputs(one, dev)
        launch(engine, one, ins1, outs1)
        assert outs1["y"].untouched() and outs1["coef"].untouched()
        assert torch.equal(outs1["y"].get().view(torch.int16), outs["y"].get()[b * c.HW: (b + 1) * c.HW].view(torch.int16)), (name, b, "y")
        assert torch.equal(outs1["coef"].get().view(torch.int32), outs["coef"].get()[b: b + 1].view(torch.int32)), (name, b, "coef")


def test_refusals_launch_nothing(engine):
    """What the kernels cannot run is an error (2: argument, 5: unsupported) before anything is launched: the outputs keep their fill."""
    dev = engine.device

    def kept(c, outs, what):
        torch.cuda.synchronize(dev)
        for k, b in outs.items():
            assert torch.equal(b.flat.view(b.bits), b.fill.view(b.bits)), (c.name, what, k, "a refused call wrote")

    def gn_refused(code, what, C0=None, C1=None, shift=None, coef_null=False):
        c = next(c for c in N.GN_CASES if c.name == "two_pass_cpg30_cat_45")
        ins, outs = N.make_inputs(c, dev), N.make_outputs(c, dev)
        a = dict(x0=ins["x0"], C0=c.C0 if C0 is None else C0, x1=ins["x1"], C1=c.C1 if C1 is None else C1, gamma=ins["gamma"], beta=ins["beta"],
                 y=outs["y"].payload, coef=outs["coef"].payload)
        if shift:
            a[shift] = a[shift].reshape(-1)[1:]                    # one element on: 2-byte (bf16) or 4-byte (fp32) aligned only
        if not coef_null and shift != "coef":
            with pytest.raises(GligenAmdError, match=f"libgligen_amd error {code}:"):
                groupnorm(engine, a["x0"], a["C0"], a["x1"], a["C1"], c.B, c.HW, a["gamma"], a["beta"], c.eps, c.silu, a["y"])
        if shift != "y":
            with pytest.raises(GligenAmdError, match=f"libgligen_amd error {code}:"):
                engine.op_groupnorm_coef(a["x0"], a["C0"], a["gamma"], a["beta"], c.eps, None if coef_null else a["coef"], x1=a["x1"], C1=a["C1"], B=c.B, HW=c.HW)
        kept(c, outs, what)

    for what, kw in (("C % 64", dict(C0=648)), ("C = 64 (cpg 2)", dict(C0=32, C1=32)), ("C1 > 0 with C0 % 8", dict(C0=636, C1=324)), ("C > 8192", dict(C0=8192, C1=64))):
        assert N.gn_refusal(kw.get("C0"), kw.get("C1", 320)) is not None
        gn_refused(N.gn_refusal(kw.get("C0"), kw.get("C1", 320)), what, **kw)
    assert N.gn_refusal(32, 32) == 5
    gn_refused(2, "no coefficient buffer", coef_null=True)
    for name in ("x0", "x1", "y", "gamma", "beta", "coef"):
        gn_refused(2, f"misaligned {name}", shift=name)

    def ln_refused(what, shift=None, **change):
        c = next(c for c in N.LN_CASES if c.name == "c520_ldx_concat")
        ins, outs = N.make_inputs(c, dev), N.make_outputs(c, dev)
        f = N.ln_fields(c, ins, outs)
        f.update(change)
        if shift:
            f[shift] = f[shift].reshape(-1)[1:] if f[shift].is_contiguous() else f[shift][0, 0, 1:]
        with pytest.raises(GligenAmdError, match="libgligen_amd error 2:"):
            engine.op_layernorm_rows(**f)
        kept(c, outs, what)

    ln_refused("C % 8", C=516)
    ln_refused("C > 1536", C=1544, ldx=1544)
    ln_refused("Tpad < N1 + N2", Tpad=12)
    ln_refused("ldx < C", ldx=512)
    ln_refused("ldx % 8", ldx=524)
    ln_refused("ldy < C", ldy=512)
    ln_refused("ldy % 8", ldy=524)
    ln_refused("no y", y=None)
    ln_refused("no x2", x2=None)
    ln_refused("gamma without beta", beta=None)
    for name in ("x", "x2", "y", "gamma", "beta"):
        ln_refused(f"misaligned {name}", shift=name)
