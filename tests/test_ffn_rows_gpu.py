"""The row-local kernels of ffn.hip by themselves (Engine.op_ff_rows / op_qkv_rows: ff_rows_kernel plain, <PRE>, <PRE, POST = 1>,
<PRE, POST = 2>; qkv_rows_kernel with PRE 0 / 1 and NP 1 / 3), every output element against float64 and the derived bound of
ffn_rows_ref, at M = 128 (one workgroup), 256 (the second workgroup's row base), 384 and 512.

Per case (ffn_rows_ref.CASES; test_ffn_rows_cpu.py holds the list to what it has to cover):
  * every output -- out, mid_out, stats_out, q, K, V^T, decoded from the kernels' layouts -- finite and |got - ref| <= bound per element,
    and within the project's bars as a whole (max |err| / max |ref| < 2.5e-2, mean |err| / mean |ref| < 1e-2);
  * every output buffer is random finite data with GUARD elements in front and behind: the stride gaps, q's padding columns and rows,
    K's extra key tile, V^T's padding rows and the columns behind T, mid_out where the residual rides in the accumulator, and the
    guards keep their bits;
  * a second run gives the same bits.
The input period: both halves of every output bit-equal, and equal to the launch without a period on the replicated rows.
Measured on MI355X: profiles/ffn_rows/err_over_bound.txt."""
from types import SimpleNamespace

import pytest
import torch

import ffn_rows_ref as R
from gligen_amd._lib import GligenAmdError

pytestmark = pytest.mark.gpu


def launch(engine, c, ins, outs):
    (engine.op_ff_rows if c.kind == "ff" else engine.op_qkv_rows)(**R.call_fields(c, ins, outs))


def run_case(engine, c, ins=None):
    dev = engine.device
    ins = R.make_inputs(c, dev) if ins is None else ins
    outs = R.make_outputs(c, dev)
    launch(engine, c, ins, outs)
    torch.cuda.synchronize(dev)
    worst = R.verify(c, ins, outs)
    first = {n: b.flat.clone() for n, b in outs.items()}
    for b in outs.values():
        b.reset()
    launch(engine, c, ins, outs)
    for n, b in outs.items():
        assert torch.equal(b.flat.view(b.bits), first[n].view(b.bits)), (c.name, n, "two runs differ")
    print(R.report_line(c, worst))
    return ins, outs


@pytest.mark.parametrize("c", R.FF_CASES, ids=[c.name for c in R.FF_CASES])
def test_ff_rows(engine, c):
    ins, outs = run_case(engine, c)
    if c.special and c.special[0] == "sweep":
        # every row sees the same gate pre-activations: the rows are copies, and the tails are exact (value 1: gelu(300) = 300, gelu(-300) = 0)
        y = outs["out"].get()
        assert torch.equal(y, y[:1].expand_as(y))
        k = c.special[1]
        g = R.sweep_gates().to(y.device)[4 * torch.arange(R.C, device=y.device) + k]
        far = g.abs() >= 20
        assert torch.equal(y[0][far].float(), g[far].clamp_min(0.0))
    if c.special and c.special[0] == "const":
        assert bool((outs["out"].get() == 1.0).all()) and torch.equal(outs["stats"].get(), torch.tensor([320.0, 320.0], device=engine.device).expand(c.M, 2))


@pytest.mark.parametrize("c", R.QKV_CASES, ids=[c.name for c in R.QKV_CASES])
def test_qkv_rows(engine, c):
    ins, outs = run_case(engine, c)
    if c.in_period:
        dev, p = engine.device, c.in_period
        for n, b in outs.items():
            v = b.get()
            assert torch.equal(v.view(c.M // p, p, -1), v[:p].expand(c.M // p, p, v.shape[1])), (c.name, n, "the periods differ")
        twin = SimpleNamespace(**{**vars(c), "in_period": 0})
        idx = torch.arange(c.M, device=dev) % p
        ins2 = dict(ins)
        ins2["x"] = R._strided_in(ins["x"][idx].cpu(), c.ldx, dev)
        if c.pre_res:
            ins2["pre_res"] = R._strided_in(ins["pre_res"][idx].cpu(), c.ld_pre_res, dev)
        outs2 = R.make_outputs(twin, dev)
        launch(engine, twin, ins2, outs2)
        for n, b in outs.items():
            assert torch.equal(b.flat.view(b.bits), outs2[n].flat.view(b.bits)), (c.name, n, "differs from the launch on the replicated rows")


def test_refusals_launch_nothing(engine):
    """A shape or form without a row-local kernel is an error (5: unsupported, 2: argument), never another kernel: the outputs keep their bits."""
    dev = engine.device
    by = {c.name: c for c in R.CASES}

    def refused(c, code, **change):
        ins, outs = R.make_inputs(c, dev), R.make_outputs(c, dev)
        f = R.call_fields(c, ins, outs)
        f.update(change)
        with pytest.raises(GligenAmdError, match=f"libgligen_amd error {code}:"):
            (engine.op_ff_rows if c.kind == "ff" else engine.op_qkv_rows)(**f)
        torch.cuda.synchronize(dev)
        for n, b in outs.items():
            assert torch.equal(b.flat.view(b.bits), b.fill.view(b.bits)), (c.name, change, n, "a refused call wrote")

    ff, chain, q2, qkv = by["plain_M256_m0"], by["chain_post1_g0.37_-0.6"], by["chain_post2_qpad"], by["pre_res_B2"]
    refused(ff, 5, M=100)
    refused(ff, 5, C=640)
    refused(ff, 2, ldx=R.C - 8)
    refused(ff, 2, ldo=R.C + 2)
    refused(chain, 5, pre=0)
    refused(chain, 2, post_res=None)
    refused(chain, 2, mid_out=None)
    refused(q2, 2, qTpad=q2.qT - 32)
    refused(q2, 2, qT=48)
    refused(q2, 2, qDP=36)
    refused(qkv, 5, T=64)
    refused(qkv, 5, M=qkv.M + 64)
    refused(qkv, 2, np=2)
    refused(qkv, 2, Tpad_k=qkv.T - 64)
    refused(qkv, 2, Tpad_k=qkv.T + 32)
    refused(qkv, 2, Tpad_q=qkv.T - 8)
    refused(qkv, 2, DP=44)
    refused(qkv, 2, in_period=64)
    refused(qkv, 2, vt=None)
