"""Every attention kernel in the binary by itself (Engine.op_attention_core), on exact bf16 q / k / v^T, at the token-count edges, with
realistic contents behind the last real token, against float64 and the derived per-element bound of attention_core_ref.

Per kernel and head dim one test runs the kernel's whole grid (attention_core_ref.grid: B = 2, H = 3; Nk around every tile edge and the
two-kernel switch at 128 / 129; Nq with a partly empty last query block of 128 and of 256 rows) x four data kinds (random, uniform,
last key dominant, key 0 dominant). Per point:
  * |got - ref| <= bound per element; the project's bars (max |y - ref| / max |ref| < 2.5e-2, mean |y - ref| / mean |ref| < 1e-2); all finite;
  * uniform data at Nk = 1: the output is v_0 bit for bit;
  * a second run gives the same bits (attn3_kernel at d = 40: the second run is the counting instantiation, and it counts (0, 0));
  * o sits in a guard pattern with ldo = H d + 8 and o_rows_per_b = Nq + 3: everything outside [b][0 .. Nq)[0 .. H d) keeps it;
  * with q rows [Nq, tq_pad) filled with fresh rows, K rows / V^T columns [Nk, tk_pad) with keys that would beat every real score
    and 4-sigma values -- what gatedSA's bias rows and reused buffers amount to -- rows < Nq come out bit-identical.
Selector 0 (attn_launch's own choice) runs the same grid per head dim at every Nk of both lists. The (selector, d, V^T form, Nk) table
of attention_core_ref.unsupported_table is asserted both ways. Buffers written by gl_op_attention_project tie selector 0 to
op_attention bit for bit; op_attention after a larger call on the same engine equals a fresh engine's.

Measured on MI355X: profiles/attention_core/err_over_bound.txt; the mutations this file catches: profiles/attention_core/mutations.txt."""
import pytest
import torch

import attention_core_ref as R
import gemm_candidates_ref as G
from gligen_amd._lib import GligenAmdError
from gligen_amd.engine import Engine

pytestmark = pytest.mark.gpu

MAX_BAR, MEAN_BAR = 2.5e-2, 1e-2
GUARD, PATTERN = 64, 7.0
KERNEL_DIMS = [(kn, d) for kn, K in R.KERNELS.items() for d in K["dims"]]


class Out:
    """o [B][Nq + 3][H d + 8] inside a flat buffer of PATTERN with GUARD elements in front and behind."""

    def __init__(self, Nq, d, dev, nh=R.H):
        self.Nq, self.C, self.rows, self.ldo, self.nh = Nq, nh * d, Nq + 3, nh * d + 8, nh
        self.flat = torch.full((2 * GUARD + R.B * self.rows * self.ldo,), PATTERN, dtype=torch.bfloat16, device=dev)
        self.o = self.flat[GUARD: GUARD + R.B * self.rows * self.ldo]
        self.view = self.o.view(R.B, self.rows, self.ldo)

    def result(self):
        """[B][H][Nq][d] of what was written; asserts that nothing else was."""
        got = self.view[:, :self.Nq, :self.C].clone()
        rest = self.flat.clone()
        rest[GUARD: GUARD + R.B * self.rows * self.ldo].view(R.B, self.rows, self.ldo)[:, :self.Nq, :self.C] = PATTERN
        assert bool((rest == PATTERN).all()), "the kernel wrote outside [b][0 .. Nq)[0 .. H d)"
        return got.view(R.B, self.Nq, self.nh, -1).permute(0, 2, 1, 3)


def run(engine, lay, bufs, Nq, Nk, selector, nh=R.H):
    out = Out(Nq, lay.d, bufs[0].device, nh)
    engine.op_attention_core(bufs[0], bufs[1], bufs[2], lay, R.B, nh, Nq, Nk, out.o, out.ldo, out.rows, selector)
    return out.result()


def perm32_of(engine, selector, d, Nk):
    """The V^T form the kernel reads; selector 0: the one the product's buffers have for (d, Nk)."""
    if selector != "auto":
        return R.KERNELS[selector]["perm32"]
    return G.proj_layout(engine, dict(B=R.B, Nq=64, Nk=Nk, C=R.H * d, Ck=R.H * d, H=R.H)).vt_perm32


def run_grid(engine, selector, bound_kernel_of, d, points):
    """The whole grid of one (selector, d). bound_kernel_of(Nk): the kernel whose bound applies. Returns the worst err / bound per kind."""
    dev = engine.device
    worst = {kind: 0.0 for kind in R.KINDS}
    counting = selector == "attn3_kernel" and d == 40
    for Nq, Nk in points:
        lay = R.layout(d, Nq, Nk, perm32_of(engine, selector, d, Nk))
        cases = [R.make_case(d, Nq, Nk, kind) for kind in R.KINDS]
        q, k, v = (torch.stack([getattr(c, n) for c in cases]).to(dev) for n in ("q", "k", "v"))       # [kind][B][H][N][d]
        ref, bound = R.reference_and_bound(q, k, v, bound_kernel_of(Nk))
        for i, (kind, c) in enumerate(zip(R.KINDS, cases)):
            what = (selector, d, Nq, Nk, kind)
            pad = {n: x.to(dev) for n, x in c.pad.items()}
            zero = R.encode(lay, q[i], k[i], v[i])
            got = run(engine, lay, zero, Nq, Nk, selector)
            g64 = got.double()
            assert bool(torch.isfinite(g64).all()), what
            err = (g64 - ref[i]).abs()
            ratio = float((err / bound[i]).max())
            worst[kind] = max(worst[kind], ratio)
            assert ratio <= 1.0, (what, "err / bound", ratio)
            assert float(err.max() / ref[i].abs().max()) < MAX_BAR and float(err.mean() / ref[i].abs().mean()) < MEAN_BAR, what
            if kind == "uniform" and Nk == 1:
                assert torch.equal(g64, v[i].expand(-1, -1, Nq, -1)), (what, "one key: the output is its value row")
            if counting:
                engine.attn_regime_counters(True)
            again = run(engine, lay, zero, Nq, Nk, selector)
            if counting:
                assert engine.attn_regime_counters(False) == (0, 0), (what, "a quiet case moved the lazy stabiliser")
            assert torch.equal(again, got), (what, "two runs differ")
            filled = R.encode(lay, q[i], k[i], v[i], pad)
            assert torch.equal(run(engine, lay, filled, Nq, Nk, selector), got), (what, "what lies behind the last real token changed rows < Nq")
    return worst


def report(selector, d, worst):
    print(f"[attention_core] {selector} d={d}: worst err / bound " + " ".join(f"{k}={x:.3f}" for k, x in worst.items()))


@pytest.mark.parametrize("kernel,d", KERNEL_DIMS, ids=[f"{k}-d{d}" for k, d in KERNEL_DIMS])
def test_kernel_grid(engine, kernel, d):
    report(kernel, d, run_grid(engine, kernel, lambda Nk: kernel, d, R.grid(kernel)))


def auto_kernel(d, Nk, perm32):
    """The kernel attn_launch runs for (d, Nk) and the buffer form the product gives it, for the bound that applies (the routing itself
    is attn_kernel_name's; with the default GL_ATTN_V2 the pipelined choice is attn3_kernel)."""
    return "attn3_kernel" if perm32 else "attn_kernel" if (Nk <= 128 or d != 40) else "attn2_kernel_w4"


@pytest.mark.parametrize("d", [40, 80, 160])
def test_auto_grid(engine, d):
    """Selector 0 at every (d, Nk) of both lists, in the buffer form the product uses there."""
    nks = sorted(set(R.NK_SHORT + R.NK_LONG))
    points = [(nq, nk) for nk in nks for nq in R.NQS]
    for nk in nks:          # the product's form: the 32-token V^T exactly where a pipelined kernel exists for the head dim
        assert perm32_of(engine, "auto", d, nk) == (1 if (nk > 128 and d in (40, 80)) else 0), (d, nk)
    report("auto", d, run_grid(engine, "auto", lambda Nk: auto_kernel(d, Nk, perm32_of(engine, "auto", d, Nk)), d, points))


def test_unsupported_table(engine):
    """Every (selector, d, V^T form, Nk): GL_ERR_UNSUPPORTED exactly where the table says, a finite answer within the bars elsewhere."""
    dev = engine.device
    n_bad = n_ok = 0
    for kernel, d, perm32, Nk, bad in R.unsupported_table():
        Nq = 33
        lay = R.layout(d, Nq, Nk, perm32)
        c = R.make_case(d, Nq, Nk, "random")
        bufs = R.encode(lay, c.q.to(dev), c.k.to(dev), c.v.to(dev))
        if bad:
            out = Out(Nq, d, dev)
            with pytest.raises(GligenAmdError, match="libgligen_amd error 5:"):
                engine.op_attention_core(bufs[0], bufs[1], bufs[2], lay, R.B, R.H, Nq, Nk, out.o, out.ldo, out.rows, kernel)
            assert bool((out.flat == PATTERN).all()), (kernel, d, perm32, Nk, "a refused call wrote")
            n_bad += 1
        else:
            got = run(engine, lay, bufs, Nq, Nk, kernel).double().cpu()
            ref = R.reference(c.q, c.k, c.v)
            assert float((got - ref).abs().max() / ref.abs().max()) < MAX_BAR, (kernel, d, perm32, Nk)
            n_ok += 1
    assert n_bad > 0 and n_ok > 0
    print(f"[attention_core] unsupported table: {n_bad} refused, {n_ok} ran")


PRODUCT_H = 8          # the projection GEMMs take C = H d in multiples of 64: the product's own head count (C = 320 / 640 / 1280)


def _product_inputs(d, Nq, Nk, self_attn, dev):
    C = PRODUCT_H * d
    g = torch.Generator().manual_seed(31 * d + Nq + Nk)
    xq = torch.randn(R.B, Nq, C, generator=g).bfloat16().to(dev)
    xkv = xq if self_attn else torch.randn(R.B, Nk, C, generator=g).bfloat16().to(dev)
    wq, wk, wv = (torch.randn(C, C, generator=g).mul(C ** -0.5).to(dev) for _ in range(3))
    return xq, xkv, wq, wk, wv


@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("Nq,Nk", [(200, 200), (100, 77)], ids=["self", "cross"])
def test_selector0_on_projected_buffers_is_op_attention(engine, d, Nq, Nk):
    """q, k, v^T written by gl_op_attention_project (the projections of op_attention) + selector 0 = op_attention, bit for bit."""
    dev = engine.device
    xq, xkv, wq, wk, wv = _product_inputs(d, Nq, Nk, Nq == Nk, dev)
    nh = PRODUCT_H
    a = dict(B=R.B, Nq=Nq, Nk=Nk, C=nh * d, Ck=nh * d, H=nh)
    lay = G.proj_layout(engine, a)
    sizes = R.buffer_sizes(lay, R.B, nh)
    q, k, vt = (torch.zeros(sizes[n], dtype=torch.bfloat16, device=dev) for n in ("q", "k", "vt"))
    R.init_required(lay, k, vt, R.B, nh)
    G.run_proj(engine, dict(args=a), dict(xq=xq, xkv=xkv, wq=wq, wk=wk, wv=wv), q, k, vt)
    got = run(engine, lay, (q, k, vt), Nq, Nk, "auto", nh)                              # [B][H][Nq][d]
    want = engine.op_attention(xq, xkv, wq, wk, wv, nh)                                 # [B][Nq][H d]
    assert torch.equal(got.permute(0, 2, 1, 3).reshape(R.B, Nq, nh * d), want)
    assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().max()) > 0


@pytest.mark.parametrize("d", [40, 160])
@pytest.mark.parametrize("first", [(128, 128), (128, 40)], ids=["after_128x128", "after_128x40"])
def test_history_of_the_engine_buffers(engine, d, first):
    """op_attention at (40, 40) after a larger call on the same engine equals a fresh engine's, bit for bit. After (128, 40) the call
    reuses the larger call's q / k / v^T buffers (the engine keys them by padded sizes: 128 query rows, 64 keys) and finds its q rows
    64 .. 127 in place; after (128, 128) the key count's padding differs (128 against 64), so that pair only shares the engine."""
    dev = engine.device
    big = _product_inputs(d, first[0], first[1], first[0] == first[1], dev)
    small = _product_inputs(d, 40, 40, True, dev)
    nh = PRODUCT_H
    engine.op_attention(*big, nh)
    got = engine.op_attention(*small, nh)
    fresh = Engine(0, arena_gb=1.0)
    try:
        want = fresh.op_attention(*small, nh)
    finally:
        fresh.close()
    assert torch.equal(got, want)
    ref = R.reference(*(x.double().view(R.B, 40, nh, d).permute(0, 2, 1, 3) for x in
                        ((small[0].float() @ small[2].bfloat16().float().t()), (small[1].float() @ small[3].bfloat16().float().t()),
                         (small[1].float() @ small[4].bfloat16().float().t()))))
    err = (got.double().view(R.B, 40, nh, d).permute(0, 2, 1, 3) - ref).abs()
    assert float(err.max() / ref.abs().max()) < MAX_BAR
