"""conv8_kernel (gligen_amd/csrc/gemm_conv8.hip) by name through gl_op_conv8x8 (include/gligen_amd_conv8.h): the 3x3 / stride 1 /
pad 1 convolution of 8 x 8 images, with every column tile, K split and epilogue forced, at the smallest shapes where it can go wrong:
    B in {1, 3, 4, 5}         a partly empty group of four samples, a full one, a full one plus a partly empty one
    (C0, C1)                  one, two and three 64-channel chunks, from one source and from two
    N                         one and three column tiles of 64 and of 80
    splits                    every K split the chunks allow (three chunks: 1, 2 = 2 + 1 uneven, 3)
    epilogue                  bias; + per-sample bias (rows_per_b = 64); + residual; SiLU
Every output element is held to a float64 convolution of the bf16 inputs with the derived bound of tests/gemm_candidates_ref.py: a
length-L fp32 sum, L = 9 (C0 + C1) + 2 additions (both biases) + one per slab behind a split, then SiLU / residual / one bf16 ulp.
The output and the slabs lie between guard zones whose bits must survive. The float64 reference is computed once per channel
configuration at B = 5, N = 240 and sliced: a smaller batch / narrower conv is a prefix of it."""
import functools

import pytest
import torch
import torch.nn.functional as F

import gemm_candidates_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = R.GUARD
BMAX, NMAX = 5, 240
CHANNELS = [(64, 0), (128, 0), (64, 64), (128, 64)]
EPILOGUES = ["bias", "bias2", "res", "silu"]


def splits_of(chunks):
    return sorted({-(-chunks // -(-chunks // s)) for s in range(1, chunks + 1)})     # the split counts that are their own normal form


def conv64(x, w):
    """float64 conv of x [B][8][8][C] with w [N][C][3][3] -> [B][8][8][N], on the CPU"""
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, stride=1, padding=1).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def tensors(C0, C1):
    Cin = C0 + C1
    x = R._rnd((BMAX, 8, 8, Cin), 11).bfloat16()
    w = R._rnd((NMAX, Cin, 3, 3), 12, (9 * Cin) ** -0.5).bfloat16().float()
    b, b2 = R._rnd((NMAX,), 13), R._rnd((BMAX, NMAX), 14)
    res = R._rnd((BMAX * 64, NMAX), 15).bfloat16()
    acc = conv64(x, w).reshape(BMAX * 64, NMAX)
    S = conv64(x.abs(), w.abs()).reshape(BMAX * 64, NMAX)
    d = dict(x0=x[..., :C0].contiguous(), x1=x[..., C0:].contiguous() if C1 else None, w=w, b=b, b2=b2, res=res, acc=acc, S=S)
    return {k: (None if v is None else v.to(DEV)) for k, v in d.items()}


def reference(t, B, N, K, epi, splits):
    """(float64 reference, elementwise bound) [B 64][N] on the device"""
    M = B * 64
    pre = t["acc"][:M, :N] + t["b"][:N].double()
    S = t["S"][:M, :N] + t["b"][:N].double().abs()
    if epi == "bias2":
        b2 = t["b2"][:B, :N].double().repeat_interleave(64, dim=0)
        pre, S = pre + b2, S + b2.abs()
    bound = (K + 2 + (splits if splits > 1 else 0)) * R.U * S
    return R._finish(pre, bound, "silu" if epi == "silu" else "plain", t["res"][:M, :N].double() if epi == "res" else None, False)


class Guarded:
    """A tensor of `n` elements between two guard zones of a fixed bit pattern."""
    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]

    def guards_intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        return bool((g == self.fill).all())


def launch(eng, t, B, N, bn, splits, epi, grid_cap=0, slabs=None, w=None, x0=None, x1=None):
    M = B * 64
    out = Guarded(M * N, torch.bfloat16, -7.0)
    out.view.fill_(3.0)
    sl = slabs
    if splits > 1 and sl is None:
        sl = Guarded(splits * M * N, torch.float32, -5.0)
    x0 = t["x0"] if x0 is None else x0
    x1 = t["x1"] if x1 is None else x1
    w = t["w"][:N].contiguous() if w is None else w
    eng.op_conv8x8(x0, w, out.view, bn, splits, x1=x1, bias=t["b"], bias2=t["b2"][:, :N].contiguous() if epi == "bias2" else None,
                   res=t["res"][:, :N].contiguous() if epi == "res" else None, act=1 if epi == "silu" else 0,
                   slabs=None if sl is None else sl.view, grid_cap=grid_cap, B=B)
    torch.cuda.synchronize()
    assert out.guards_intact(), "the output's guard zones were written"
    if sl is not None:
        assert sl.guards_intact(), "the slabs' guard zones were written"
    return out.view.reshape(M, N)


def worst_ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


def test_smallest_case(engine):
    """One sample, one chunk, one column tile, unsplit, bias: the first launch of the kernel."""
    t = tensors(64, 0)
    got = launch(engine, t, 1, 64, 64, 1, "bias")
    ref, bound = reference(t, 1, 64, 9 * 64, "bias", 1)
    r = worst_ratio(got, ref, bound)
    print(f"[conv8] smallest case: worst err / bound = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("bn", [64, 80])
@pytest.mark.parametrize("C0,C1", CHANNELS)
def test_every_tile_split_and_epilogue_against_float64(engine, C0, C1, bn):
    t = tensors(C0, C1)
    K = 9 * (C0 + C1)
    worst, n = 0.0, 0
    for B in (1, 3, 4, 5):
        for tiles in (1, 3):
            N = tiles * bn
            for splits in splits_of((C0 + C1) // 64):
                for epi in EPILOGUES:
                    got = launch(engine, t, B, N, bn, splits, epi)
                    ref, bound = reference(t, B, N, K, epi, splits)
                    r = worst_ratio(got, ref, bound)
                    assert r <= 1.0, (B, N, splits, epi, r)
                    worst, n = max(worst, r), n + 1
    print(f"[conv8] C0={C0} C1={C1} bn={bn}: {n} launches, worst err / bound = {worst:.3f}")


def test_fp32_output_unsplit_and_split(engine):
    """out_f32: the sum itself (no bf16 ulp in the bound), through the kernel's own epilogue and through the reduce pass."""
    t = tensors(128, 64)
    B, N, K = 3, 64, 9 * 192
    for splits in (1, 3):
        out = Guarded(B * 64 * N, torch.float32, -7.0)
        sl = Guarded(splits * B * 64 * N, torch.float32, -5.0) if splits > 1 else None
        engine.op_conv8x8(t["x0"], t["w"][:N].contiguous(), out.view, 64, splits, x1=t["x1"], bias=t["b"], slabs=None if sl is None else sl.view, B=B)
        torch.cuda.synchronize()
        assert out.guards_intact() and (sl is None or sl.guards_intact())
        pre = t["acc"][:B * 64, :N] + t["b"][:N].double()
        bound = (K + 2 + (splits if splits > 1 else 0)) * R.U * (t["S"][:B * 64, :N] + t["b"][:N].double().abs())
        assert worst_ratio(out.view.reshape(B * 64, N), pre, bound) <= 1.0, splits


def test_the_halo_is_zero_and_samples_do_not_bleed(engine):
    """(a) An input that is non-zero on the image border only: every tap that reaches over the edge must read zero, and the interior
    outputs see nothing but border pixels. (b) An input that is non-zero in sample 1 of a group of four only: samples 0, 2, 3 share
    pad rows with it in LDS and must come out as the bias alone, bit for bit."""
    t = tensors(64, 64)
    B, N, K = 4, 64, 9 * 128
    w = t["w"][:N].contiguous()
    x = torch.cat([t["x0"], t["x1"]], dim=-1)[:B].clone()
    border = torch.zeros(8, 8, dtype=torch.bool, device=DEV)
    border[0, :] = border[7, :] = border[:, 0] = border[:, 7] = True
    xb = x * border[None, :, :, None]
    xn = x.clone()
    xn[0] = 0; xn[2:] = 0
    for name, xin in (("border", xb), ("neighbour", xn)):
        for splits in (1, 2):
            got = launch(engine, t, B, N, 64, splits, "bias", w=w, x0=xin[..., :64].contiguous(), x1=xin[..., 64:].contiguous())
            acc = conv64(xin.cpu(), w.cpu()).reshape(B * 64, N).to(DEV)
            S = conv64(xin.cpu().abs(), w.cpu().abs()).reshape(B * 64, N).to(DEV)
            ref, bound = R._finish(acc + t["b"][:N].double(), (K + 2 + splits) * R.U * (S + t["b"][:N].double().abs()), "plain", None, False)
            assert worst_ratio(got, ref, bound) <= 1.0, (name, splits)
            if name == "neighbour":
                alone = t["b"][:N].bfloat16().expand(64, N)
                for smp in (0, 2, 3):
                    assert torch.equal(got[smp * 64:(smp + 1) * 64], alone), (smp, splits)


@pytest.mark.parametrize("tap", range(9))
def test_one_tap_at_a_time(engine, tap):
    """Weights that are non-zero in one filter tap only: the output is that tap's shifted 1x1 conv, so a wrong shift, a swapped
    (ky, kx) or a weight stage read under the wrong tap shows in every element."""
    t = tensors(64, 64)
    B, N, K = 3, 64, 9 * 128
    w = torch.zeros_like(t["w"][:N])
    w[:, :, tap // 3, tap % 3] = t["w"][:N, :, tap // 3, tap % 3]
    x = torch.cat([t["x0"], t["x1"]], dim=-1)[:B]
    acc = conv64(x.cpu(), w.cpu()).reshape(B * 64, N).to(DEV)
    S = conv64(x.cpu().abs(), w.cpu().abs()).reshape(B * 64, N).to(DEV)
    for splits in (1, 2):
        got = launch(engine, t, B, N, 64, splits, "bias", w=w.contiguous())
        ref, bound = R._finish(acc + t["b"][:N].double(), (K + 2 + splits) * R.U * (S + t["b"][:N].double().abs()), "plain", None, False)
        assert worst_ratio(got, ref, bound) <= 1.0, splits


@pytest.mark.parametrize("bn,splits", [(64, 1), (64, 2), (80, 3)])
def test_bits_do_not_depend_on_the_grid_cap_or_the_run(engine, bn, splits):
    """What the tuner relies on: for a fixed (column tile, split) the resident grid only changes which workgroup runs an item."""
    t = tensors(128, 64)
    B, N = 5, 3 * bn
    first = launch(engine, t, B, N, bn, splits, "bias2")
    for cap in (0, 1, 3, 7):
        assert torch.equal(launch(engine, t, B, N, bn, splits, "bias2", grid_cap=cap), first), cap


@pytest.mark.parametrize("B", [2, 4, 6])
@pytest.mark.parametrize("splits", [1, 3])
def test_the_first_half_of_a_batch_has_the_bits_of_the_half_batch(engine, B, splits):
    """What the guidance pair's shared prefix relies on: samples [0, B / 2) of a B-sample launch are the B / 2-sample launch, whatever
    group of four they share with the other half (B = 6: samples 0..2 sit in a full group there and in a partly empty one here)."""
    t = tensors(128, 64)
    x0 = torch.cat([t["x0"], t["x0"][:1]])      # six samples
    x1 = torch.cat([t["x1"], t["x1"][:1]])
    t6 = dict(t, b2=torch.cat([t["b2"], t["b2"][:1]]), res=torch.cat([t["res"], t["res"][:64]]))
    full = launch(engine, t6, B, 64, 64, splits, "bias2", x0=x0, x1=x1)
    half = launch(engine, t6, B // 2, 64, 64, splits, "bias2", x0=x0, x1=x1)
    assert torch.equal(full[:B // 2 * 64], half)


def test_what_the_entry_refuses(engine):
    from gligen_amd._lib import GligenAmdError
    t = tensors(64, 0)
    out = torch.zeros(64 * 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(GligenAmdError):      # a K split with more parts than chunks
        engine.op_conv8x8(t["x0"], t["w"][:64].contiguous(), out, 64, 2, bias=t["b"], slabs=torch.zeros(2 * 64 * 64, device=DEV), B=1)
    with pytest.raises(GligenAmdError):      # a column tile that does not divide N
        engine.op_conv8x8(t["x0"], t["w"][:64].contiguous(), out, 80, 1, bias=t["b"], B=1)
    t3 = tensors(128, 64)
    with pytest.raises(GligenAmdError):      # slabs smaller than splits x M x N
        engine.op_conv8x8(t3["x0"], t3["w"][:64].contiguous(), out, 64, 3, x1=t3["x1"], bias=t3["b"], slabs=torch.zeros(2 * 64 * 64, device=DEV), B=1)
