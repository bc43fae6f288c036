"""The normalisation kernels of gligen_amd/csrc/norm.hip by themselves (gl_op_groupnorm, gl_op_groupnorm_coef, gl_op_layernorm_rows): the
case list, the kernels' preconditions and launch geometry, guarded buffers, a float64 reference that follows the kernels' rounding
points, a derived per-element bound, and an fp32 emulation (the twin) that stands in for the kernels without a GPU.
tests/test_norm_cpu.py checks this module, tests/test_norm_gpu.py holds the kernels to it.

KERNEL FORMS (gn_path): small256 / small1024 -- gn_small_kernel<NT> and gn_small_coef_kernel<NT>, one workgroup of NT threads per
(sample, group), HW <= 256 and cpg % 4 == 0, NT = 1024 from HW cpg >= 8192; two_pass -- gn_stats_kernel + gn_apply_kernel (or
gn_coef_kernel) everywhere else. gn_geometry transcribes the two-pass launch: R pixel rows per block, nsplit statistics blocks of `per`
pixels (the last ones may be empty), the apply grid's nblk, per (rounded up to R) and trips per block.

ROUNDING POINTS the reference follows (u = 2^-24):
  statistics  float64 sums of the bf16 inputs; mean and rstd = (var + eps)^-1/2 rounded to fp32 as the kernels store them
  two_pass    a = rstd gamma, c = beta - mean a, y = fma(x, a, c); the reference evaluates (x - mean) a + beta in float64
  small       y = (x - mean) rstd gamma + beta
  LayerNorm   two passes over the row: mean, then the centred sum of squares, rsqrtf; y = (x - mean) rstd [gamma + beta]
  SiLU        y sigmoid(y) behind either form; bf16 at the end
BOUNDS, per element (ffn_rows_ref's statistics terms, with the chain lengths of the geometry; S1 = sum |x|, S2 = sum x^2 of a group):
  an fp32 sum whose every element passes through at most d additions is off by at most d u S; d = chain + 2 where
      two_pass  chain = 8 cdiv(per, R) (the thread's pixels, 8 channels each) + R (cdiv(cpg, 8) + 3) (the block's combine); the
                float64 combine of the nsplit partials is 2^-29 of that
      small     chain = cdiv(HW cpg / 4, NT) + 8 (the thread's pieces, the adds inside a piece, six butterfly steps)
  e_mean = (chain + 2) u S1 / n + 2 u |mean|  (the sum; the fp32 rounding of the kernel's mean against the reference's)
  e_var  = (chain + 3) u S2 / n + 2 |mean| e_mean + e_mean^2 + 2 u (S2 / n + mean^2)
  e_r    = sqrt((var + eps) / (max(var - e_var, 0) + eps)) - 1 + 5 u   (relative; the kernels clamp var at 0, so this is the worst
           case whatever e_var is: a constant group keeps a finite bound)
  two_pass    y' = (x - mean') a' + beta + the roundings of c and of the fma:
              |x - mean| da + e_mean (|a| + da) + 2 u (|beta| + |mean| |a|) + u |y|,  da = |a| (e_r + u)
              coefficients: a within da, c within e_mean (|a| + da) + |mean| da + 2 u (|beta| + |mean a|)
  small, LN   e_mean rstd |gamma| (1 + e_r) + |x - mean| rstd |gamma| (e_r + 4 u) + u |y|
              LayerNorm: e_mean = (chain + 1) u S1 / C + u |mean| with chain = 8 cdiv(C / 8, 64) + 6; the centred pass moves var by
              e_mean^2 + (chain + 4) u var, and rsqrtf is within 1 ulp (2 u)
  SiLU        gemm_candidates_ref._silu_bound: 1.1 e + (2 |v| + 6) u |silu(v)| -- exp2 and the reciprocal 1 ulp each -- and 2^-126
  bf16        ffn_rows_ref.round_stage on the value and its bound e: where no rounding boundary lies within e of the reference the
              kernel's bf16 has to EQUAL the reference's (bound 0); where one does, e + ulp / 2 against the unrounded value
Nothing is fitted to what the kernels return.

INPUT KINDS. plain: mean 0.5, sigma 2 (source 1: mean -1, sigma 1). offset: per-channel means up to 8, sigma 0.25. outlier: one
channel of group 7 at 100 x. constant: group 5 holds 1.5 everywhere (variance 0). Every source is dense (GNParams has no row stride)
and sits inside a flat buffer whose other elements hold 1e4 ("poison"): a read with the wrong row stride or past the end shows.
lift (the 576-addition chains of HW = 65536): gamma around 0.25, beta around 2, so that no output lies near zero, where the worst
case of such a chain -- an absolute error -- would exceed a quarter of the output's ulp at more than 1 % of the elements.
LayerNorm: x has row stride ldx with 1e4 in the gaps, x2 is dense.
"""
from types import SimpleNamespace

import torch

import ffn_rows_ref as F
import gemm_candidates_ref as G

U, BF16_ULP, GUARD = G.U, G.BF16_ULP, G.GUARD
MAX_BAR, MEAN_BAR = F.MAX_BAR, F.MEAN_BAR
IN_FILL = F.IN_FILL
MARGIN = 4096              # poisoned elements in front of and behind every input (a multiple of 8: the payload stays 16-byte aligned)
GN_UNR = 8
TINY = 2.0 ** -126
Buf, round_stage, _rnd = F.Buf, F.round_stage, F._rnd


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- preconditions, geometry
# transcribed once from norm.hip (gn_check, groupnorm_launch, groupnorm_coef_launch, layernorm_launch)
def gn_refusal(C0, C1):
    """The error code gn_check / groupnorm_launch answer with (2 argument, 5 unsupported), None where they launch."""
    C = C0 + C1
    if C % 64 or (C1 and C0 % 8):
        return 2
    cpg = C // 32
    if cpg < 4 or cpg & 1:
        return 5
    if C // 8 > 1024:
        return 2
    return None


def gn_path(HW, C0, C1):
    cpg = (C0 + C1) // 32
    if HW <= 256 and C0 % 4 == 0 and cpg % 4 == 0:
        return "small1024" if HW * cpg >= 8192 else "small256"
    return "two_pass"


def gn_geometry(B, HW, C):
    """The two-pass launch: statistics grid (nsplit, B) of T = C8 R threads, apply grid (agrid, B)."""
    C8, cpg = C // 8, C // 32
    R = 1 if C8 >= 256 else 256 // C8
    nsplit = max(1, min(64, cdiv(HW, R * GN_UNR)))
    per = cdiv(HW, nsplit)
    trips = cdiv(HW, R * GN_UNR)
    nblk = max(1, min(trips, max(1, 2048 // B)))
    aper = cdiv(cdiv(HW, nblk), R) * R
    return SimpleNamespace(C8=C8, cpg=cpg, R=R, T=C8 * R, nsplit=nsplit, per=per, empty=sum(1 for k in range(nsplit) if k * per >= HW), trips=trips,
                           nblk=nblk, aper=aper, agrid=cdiv(HW, aper), atrips=cdiv(aper, R * GN_UNR), chain=8 * cdiv(per, R) + R * (cdiv(cpg, 8) + 3))


def small_threads(path):
    return 1024 if path == "small1024" else 256


def gn_chain(c):
    """The longest chain of fp32 additions an input passes through on its way into the group's sum."""
    path = gn_path(c.HW, c.C0, c.C1)
    if path == "two_pass":
        return gn_geometry(c.B, c.HW, c.C0 + c.C1).chain
    return cdiv(c.HW * ((c.C0 + c.C1) // 32) // 4, small_threads(path)) + 8


def ln_refusal(c):
    if c.C % 8 or c.C > 1536:
        return 2
    if c.Tpad < c.N1 + c.N2:
        return 2
    if (c.ldx and (c.ldx < c.C or c.ldx % 8)) or (c.ldy and (c.ldy < c.C or c.ldy % 8)):
        return 2
    return None


def ln_chain(C):
    return 8 * cdiv(C // 8, 64) + 6


# ---------------------------------------------------------------------------------------------------------------- cases
def _gn(name, B, HW, C0, C1, silu, eps, inp="plain", lift=False):
    return SimpleNamespace(kind="gn", name=name, B=B, HW=HW, C0=C0, C1=C1, silu=silu, eps=eps, inp=inp, lift=lift)


GN_CASES = [
    _gn("small_idle_threads", 2, 4, 1280, 0, 1, 1e-5),
    _gn("small_hw1", 1, 1, 128, 0, 0, 1e-6),
    _gn("small_ragged_45", 3, 45, 640, 0, 1, 1e-5),
    _gn("small_cpg4_180", 2, 180, 128, 0, 0, 1e-6),
    _gn("small1024", 2, 256, 1280, 0, 1, 1e-5),
    _gn("small1024_cat", 1, 256, 1280, 1280, 0, 1e-6),
    _gn("small_group_straddles_sources", 2, 64, 1280, 640, 1, 1e-5),
    _gn("two_pass_cpg10_64", 2, 64, 320, 0, 0, 1e-5),
    _gn("two_pass_cpg30_cat_45", 3, 45, 640, 320, 1, 1e-5),
    _gn("two_pass_257", 1, 257, 128, 0, 0, 1e-6),
    _gn("two_pass_720_R3", 2, 720, 640, 0, 1, 1e-5),
    _gn("two_pass_2880_R6", 1, 2880, 320, 0, 0, 1e-5),
    _gn("two_pass_cpg6", 2, 300, 192, 0, 1, 1e-6),
    _gn("two_pass_cpg14", 1, 100, 448, 0, 0, 1e-5),
    _gn("two_pass_empty_blocks", 1, 520, 1280, 1280, 0, 1e-5),
    _gn("two_pass_apply_trips", 32, 513, 1088, 0, 1, 1e-5),
    _gn("two_pass_long_chains", 1, 65536, 128, 0, 1, 1e-6, lift=True),
    _gn("offset_small_45", 2, 45, 640, 0, 0, 1e-5, "offset"),
    _gn("offset_two_pass_720", 1, 720, 640, 0, 1, 1e-6, "offset"),
    _gn("offset_long_chains", 1, 65536, 128, 0, 0, 1e-5, "offset"),
    _gn("outlier_small_45", 2, 45, 640, 0, 1, 1e-5, "outlier"),
    _gn("outlier_two_pass_257", 1, 257, 128, 0, 0, 1e-5, "outlier"),
    _gn("constant_small_180", 1, 180, 128, 0, 0, 1e-5, "constant"),
    _gn("constant_two_pass_64", 2, 64, 320, 0, 1, 1e-6, "constant"),
    _gn("constant_two_pass_cat", 1, 300, 640, 320, 0, 1e-5, "constant"),
]


def _ln(name, B, N1, N2, Tpad, C, ldx=0, ldy=0, affine=True, inp="plain"):
    return SimpleNamespace(kind="ln", name=name, B=B, N1=N1, N2=N2, Tpad=Tpad, C=C, ldx=ldx, ldy=ldy, affine=affine, inp=inp, eps=1e-5)


LN_CASES = [
    _ln("c8", 2, 5, 0, 5, 8),
    _ln("c96_ldy128", 1, 45, 0, 47, 96, ldy=128),
    _ln("c96_ldy128_noaffine", 3, 9, 0, 9, 96, ldx=104, ldy=128, affine=False),
    _ln("c320_concat_pad", 3, 16, 30, 64, 320),
    _ln("c512_one_pass", 1, 7, 0, 7, 512),
    _ln("c520_ldx_concat", 2, 9, 4, 13, 520, ldx=528),
    _ln("c768_noaffine", 1, 10, 0, 10, 768, affine=False),
    _ln("c1280_concat", 1, 64, 13, 80, 1280),
    _ln("c1536_limit", 2, 3, 2, 6, 1536, ldx=1544, ldy=1544),
    _ln("c320_offset_rows", 1, 33, 0, 33, 320, inp="offset"),
    _ln("c320_constant_row", 1, 6, 0, 8, 320, inp="constant"),
]
CASES = GN_CASES + LN_CASES
assert len({c.name for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------- inputs and buffers
def _seed(c, k):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) * 64 + k) % (2 ** 31)


def _poisoned(t, dev):
    """(the flat buffer, t's values as a view of it): MARGIN elements of 1e4 in front and behind."""
    flat = torch.full((2 * MARGIN + t.numel(),), IN_FILL, dtype=t.dtype)
    flat[MARGIN: MARGIN + t.numel()] = t.reshape(-1)
    flat = flat.to(dev)
    return flat, flat[MARGIN: MARGIN + t.numel()].view(t.shape)


def make_inputs(c, dev):
    s = lambda k: _seed(c, k)
    if c.kind == "gn":
        C, cpg = c.C0 + c.C1, (c.C0 + c.C1) // 32
        if c.inp == "offset":
            x = _rnd((c.B, c.HW, C), s(1)) * 0.25 + (torch.rand(C, generator=torch.Generator().manual_seed(s(2))) * 16 - 8)
        else:
            x = _rnd((c.B, c.HW, C), s(1)) * 2 + 0.5
            if c.C1:
                x[..., c.C0:] = x[..., c.C0:] * 0.5 - 1.25
        if c.inp == "outlier":
            x[..., 7 * cpg + 1] *= 100
        if c.inp == "constant":
            x[..., 5 * cpg: 6 * cpg] = 1.5
        xb = x.bfloat16()
        gamma, beta = 1 + 0.3 * _rnd((C,), s(3)), 0.2 * _rnd((C,), s(4))
        if c.lift:
            gamma, beta = 0.25 * gamma, 2 + beta
        ins = dict(gamma=gamma.to(dev), beta=beta.to(dev), x1=None, flat1=None)
        ins["flat0"], ins["x0"] = _poisoned(xb[..., :c.C0].contiguous(), dev)
        if c.C1:
            ins["flat1"], ins["x1"] = _poisoned(xb[..., c.C0:].contiguous(), dev)
        return ins
    ldx = c.ldx or c.C
    x = _rnd((c.B, c.N1, c.C), s(1)) * 1.5 + 0.3
    if c.inp == "offset":
        x = (_rnd((c.B, c.N1, c.C), s(1)) + 8) * 1.5
    if c.inp == "constant":
        x[0, 2] = 1.5
    wide = torch.full((c.B, c.N1, ldx), IN_FILL)
    wide[..., :c.C] = x
    flat, view = _poisoned(wide.bfloat16(), dev)
    ins = dict(flat=flat, x=view[..., :c.C], x2=None, flat2=None, gamma=None, beta=None)
    if c.N2:
        ins["flat2"], ins["x2"] = _poisoned((_rnd((c.B, c.N2, c.C), s(2)) * 0.7 - 0.4).bfloat16(), dev)
    if c.affine:
        ins.update(gamma=(1 + 0.3 * _rnd((c.C,), s(3))).to(dev), beta=(0.2 * _rnd((c.C,), s(4))).to(dev))
    return ins


def make_outputs(c, dev):
    """{name: Buf}: random finite fill, GUARD elements around the payload; every element of every payload has to be written."""
    s = lambda k: _seed(c, 100 + k)
    if c.kind == "gn":
        C = c.C0 + c.C1
        return {"y": Buf(c.B * c.HW * C, torch.bfloat16, torch.arange(c.B * c.HW * C, device=dev).view(c.B * c.HW, C), s(1), dev),
                "coef": Buf(c.B * C * 2, torch.float32, torch.arange(c.B * C * 2, device=dev).view(c.B, C * 2), s(2), dev)}
    ldy = c.ldy or c.C
    return {"y": Buf(c.B * c.Tpad * ldy, torch.bfloat16, torch.arange(c.B * c.Tpad * ldy, device=dev).view(c.B * c.Tpad, ldy), s(1), dev)}


def gn_call(c, ins, outs):
    """The arguments of gl_op_groupnorm behind the context: (x0, C0, x1, C1, B, HW, gamma, beta, eps, silu, y)."""
    return (ins["x0"], c.C0, ins["x1"], c.C1, c.B, c.HW, ins["gamma"], ins["beta"], c.eps, c.silu, outs["y"].payload)


def ln_fields(c, ins, outs):
    """The fields of gl_layernorm_rows_args for Engine.op_layernorm_rows."""
    return dict(x=ins["x"], x2=ins["x2"], B=c.B, N1=c.N1, N2=c.N2, Tpad=c.Tpad, C=c.C, eps=c.eps, gamma=ins["gamma"], beta=ins["beta"], y=outs["y"].payload,
                ldx=c.ldx, ldy=c.ldy)


def coef_split(coef, B, C):
    """(a, c) [B][C] of the layout [B][C / 8][16]: a of 8 channels, then their c."""
    v = coef.reshape(B, C // 8, 2, 8)
    return v[:, :, 0].reshape(B, C), v[:, :, 1].reshape(B, C)


# ---------------------------------------------------------------------------------------------------------------- reference and bounds
def _f32(v):
    return v.float().double()


def _rel_rstd(var, e_var, eps):
    return ((var + eps) / ((var - e_var).clamp_min(0.0) + eps)).sqrt() - 1 + 5 * U


def gn_stats(c, x):
    """Per (sample, group), from x [B][HW][C] float64: mean and rstd as fp32 values, and the bounds e_mean (absolute), e_r (relative)."""
    C = c.C0 + c.C1
    cpg, n, chain = C // 32, c.HW * (C // 32), gn_chain(c)
    xg = x.view(c.B, c.HW, 32, cpg)
    s1, s2 = xg.abs().sum((1, 3)) / n, (xg * xg).sum((1, 3)) / n
    mean = xg.sum((1, 3)) / n
    var = (s2 - mean * mean).clamp_min(0.0)
    e_mean = (chain + 2) * U * s1
    e_var = (chain + 3) * U * s2 + 2 * mean.abs() * e_mean + e_mean ** 2 + 2 * U * (s2 + mean * mean)
    e_r = _rel_rstd(var, e_var, c.eps)
    per_channel = lambda v: v.repeat_interleave(cpg, 1)          # [B][32] -> [B][C]
    return per_channel(_f32(mean)), per_channel(_f32((var + c.eps) ** -0.5)), per_channel(e_mean + 2 * U * mean.abs()), per_channel(e_r)


def gn_expect(c, ins):
    """(y [B HW][C] before the bf16 rounding, its bound e_y; a, c [B][C] and their bounds), float64."""
    x = (ins["x0"] if ins["x1"] is None else torch.cat([ins["x0"], ins["x1"]], -1)).double()
    gm, bt = ins["gamma"].double(), ins["beta"].double()
    mean, rstd, e_mean, e_r = gn_stats(c, x)
    a = rstd * gm
    cc = bt - mean * a
    da = a.abs() * (e_r + U)
    e_c = e_mean * (a.abs() + da) + mean.abs() * da + 2 * U * (bt.abs() + (mean.abs() + e_mean) * (a.abs() + da))
    d = x - mean[:, None]
    y = d * a[:, None] + bt
    if gn_path(c.HW, c.C0, c.C1) == "two_pass":
        e = d.abs() * da[:, None] + (e_mean * (a.abs() + da) + 2 * U * (bt.abs() + (mean.abs() + e_mean) * (a.abs() + da)))[:, None]
    else:
        e = (e_mean * a.abs() * (1 + e_r + 4 * U))[:, None] + d.abs() * (a.abs() * (e_r + 4 * U))[:, None]
    e = e * (1 + U) + U * y.abs()
    if c.silu:
        y, e = G._silu_bound(y, e)
        e = e + TINY
    C = c.C0 + c.C1
    return y.view(-1, C), e.view(-1, C), (a, da + TINY), (cc, e_c + TINY)


def ln_rows(c, ins):
    """The real rows [B][N1 + N2][C] (float64) in output order."""
    x = ins["x"].double()
    return x if ins["x2"] is None else torch.cat([x, ins["x2"].double()], 1)


def ln_expect(c, ins):
    x = ln_rows(c, ins)
    chain = ln_chain(c.C)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    e_mean = (chain + 1) * U * x.abs().mean(-1, keepdim=True) + U * mean.abs()
    e_var = e_mean ** 2 + (chain + 4) * U * var + 2 * U * (var + c.eps)
    e_r = _rel_rstd(var, e_var, c.eps)
    rstd = (var + c.eps) ** -0.5
    gm = ins["gamma"].double() if c.affine else torch.ones((), dtype=torch.float64, device=x.device)
    bt = ins["beta"].double() if c.affine else torch.zeros((), dtype=torch.float64, device=x.device)
    y = d * rstd * gm + bt
    e = e_mean * rstd * gm.abs() * (1 + e_r + 4 * U) + d.abs() * rstd * gm.abs() * (e_r + 4 * U)
    return y, e * (1 + U) + U * y.abs()


def real_rows(c, dev):
    """Indices into [B Tpad] of the rows that hold data, in the order of ln_rows."""
    return (torch.arange(c.B, device=dev)[:, None] * c.Tpad + torch.arange(c.N1 + c.N2, device=dev)[None, :]).reshape(-1)


def bf16_ulp_of(v):
    _, ex = torch.frexp(v.abs().clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(v), ex - 8)


def sharp_share(c, ins):
    """The share of elements whose bound, beyond the final bf16 rounding, is at most a quarter of a bf16 ulp of the reference."""
    y, e = (gn_expect(c, ins)[:2] if c.kind == "gn" else ln_expect(c, ins))
    return float((e <= bf16_ulp_of(y) / 4).double().mean())


def fma_identity(x, a, cc):
    """bf16(fma(x, a, c)) on the host from fp32 coefficient bits: (the bf16 values, the mask of elements whose fp32 rounding the
    float64 evaluation cannot decide -- its sum sits on an fp32 rounding boundary to within float64's own rounding)."""
    p, c64 = x.double() * a.double(), cc.double() + torch.zeros_like(x, dtype=torch.float64)      # the product is exact (8 x 24 bits)
    t = p + c64
    bb = t - p
    inexact = ((p - (t - bb)) + (c64 - bb)) != 0          # TwoSum: where the float64 sum is exact (ties included) float32() decides
    t32 = t.float()
    resid = (t - t32.double()).abs()
    _, ex = torch.frexp(t32.double().abs().clamp_min(1e-300))
    half = torch.ldexp(torch.ones_like(t), ex - 25)        # half an fp32 ulp of t32 (a quarter, right under a power of two)
    tol = 2.0 ** -50 * t.abs()
    unsure = inexact & (((resid - half).abs() <= tol) | ((resid - half / 2).abs() <= tol))
    return t32.bfloat16(), unsure


def _check(c, name, got, ref, bound, worst):
    assert got.shape == ref.shape == bound.shape, (c.name, name)
    assert bool(torch.isfinite(got).all()), (c.name, name, "not finite")
    err = (got - ref).abs()
    ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), ratio)
    w = int(ratio.argmax())
    at = (w // ratio.shape[1], w % ratio.shape[1])
    worst[name] = (float(ratio.reshape(-1)[w]), at)
    assert worst[name][0] <= 1.0, (c.name, name, "err / bound", float(err[at] / bound[at].clamp_min(1e-300)), "at", at, "got", float(got[at]), "ref", float(ref[at]),
                                   "bound", float(bound[at]))


def _bars(c, name, got, ref):
    if float(ref.abs().max()) > 0:
        err = (got - ref).abs()
        bars = (float(err.max() / ref.abs().max()), float(err.mean() / ref.abs().mean()))
        assert bars[0] < MAX_BAR and bars[1] < MEAN_BAR, (c.name, name, "max |err| / max |ref|, mean |err| / mean |ref|", bars)


def verify(c, ins, outs):
    """Every output of the launches: nothing outside the payload touched, finite, err <= bound at every element, the zeros the
    kernel owes exactly zero, and (two_pass without SiLU) y bit-equal to bf16(fma(x, a, c)) of the returned coefficients. Returns
    {output: (worst err / bound, (row, column))}; raises AssertionError with the case, the output and the place."""
    for name, b in outs.items():
        assert b.untouched(), (c.name, name, "an element outside the written region changed")
    worst = {}
    if c.kind == "ln":
        got = outs["y"].get()
        dev, ldy = got.device, c.ldy or c.C
        rows = real_rows(c, dev)
        zero = torch.ones(got.shape, dtype=torch.bool, device=dev)
        zero[rows, :c.C] = False
        assert bool((got.view(torch.int16)[zero] == 0).all()), (c.name, "y", "a pad row or a column in [C, ldy) is not zero")
        y, e = ln_expect(c, ins)
        ref, bound = round_stage(y.view(-1, c.C), e.view(-1, c.C))
        g = got[rows, :c.C].double()
        _check(c, "y", g, ref, bound, worst)
        _bars(c, "y", g, ref)
        return worst
    C = c.C0 + c.C1
    y, e, (a, da), (cc, e_c) = gn_expect(c, ins)
    ref, bound = round_stage(y, e)
    got = outs["y"].get()
    _check(c, "y", got.double(), ref, bound, worst)
    _bars(c, "y", got.double(), ref)
    ga, gc = coef_split(outs["coef"].get(), c.B, C)
    _check(c, "coef", torch.cat([ga, gc], 1).double(), torch.cat([a, cc], 1), torch.cat([da, e_c], 1), worst)
    if gn_path(c.HW, c.C0, c.C1) == "two_pass" and not c.silu:
        x = ins["x0"] if ins["x1"] is None else torch.cat([ins["x0"], ins["x1"]], -1)
        want, unsure = fma_identity(x, ga[:, None], gc[:, None])
        same = want.view(-1, C).view(torch.int16) == got.view(torch.int16)
        unsure = unsure.view(-1, C)
        assert bool((same | unsure).all()), (c.name, "y", "not bf16(fma(x, a, c)) of the returned coefficients at", int((~(same | unsure)).nonzero()[0, 0]))
        worst["fma_unsure"] = (float(unsure.double().mean()), (0, 0))
    return worst


def report_line(c, worst):
    form = gn_path(c.HW, c.C0, c.C1) if c.kind == "gn" else "ln_kernel"
    return f"[norm] {c.name} ({form}): " + " ".join(f"{n}={r:.3g}@{at[0]},{at[1]}" for n, (r, at) in worst.items())


# ---------------------------------------------------------------------------------------------------------------- the twin
# fp32 emulations of the kernels: same thread ownership, same clamped re-reads, same partial layout, same fixed-order fp64 combine.
# defect: one of the seeded faults of test_norm_cpu.py, by name.
def _fma32(x, a, cc):
    return (x.double() * a.double() + cc.double()).float()


def _silu32(v):
    return v * (1.0 / (1.0 + torch.exp2(v * torch.tensor(-1.4426950408889634, dtype=torch.float32))))


def _wave_sum(v):
    """__shfl_xor butterfly over the last dim (64 lanes)."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def _gather_flat(flat, idx):
    return flat[idx.clamp(0, flat.numel() - 1)]


def twin_sources(c, ins, defect=None):
    """[B][HW][C] fp32 as the kernels address it: source 0 with row stride C0, source 1 with row stride C1."""
    x0 = ins["x0"].float()
    if not c.C1:
        return x0
    ld1 = c.C0 if defect == "src1_row_stride" else c.C1
    pix = torch.arange(c.B * c.HW)[:, None] * ld1
    x1 = _gather_flat(ins["flat1"], MARGIN + pix + torch.arange(c.C1)[None, :]).float().view(c.B, c.HW, c.C1)
    return torch.cat([x0, x1], -1)


def twin_stats(c, x, partial, defect=None):
    """gn_stats_kernel: fills partial [B][nsplit][32][2] (fp32) in place, block by block as the grid does."""
    g = gn_geometry(c.B, c.HW, c.C0 + c.C1)
    R, per, C8, cpg = g.R, g.per, g.C8, g.cpg
    J = 8 * cdiv(cdiv(per, R), 8)
    blk, ry, j = torch.arange(g.nsplit)[:, None, None], torch.arange(R)[None, :, None], torch.arange(J)[None, None, :]
    p0 = blk * per
    p1 = torch.clamp(p0 + per, max=c.HW)
    p = p0 + ry + j * R
    valid = p < p1
    slots = 8 * ((valid.sum(-1, keepdim=True) + 7) // 8)       # the thread's trips, GN_UNR pixels each
    reread = ~valid & (j < slots)                               # min(p + u R, p1 - 1): loaded, counted as zero
    count = valid & (p < p1 - 1) if defect == "drop_last_pixel" else valid | reread if defect == "count_reread" else valid
    pc = torch.minimum(p, p1 - 1).clamp_min(0)
    X = x[:, pc] * count[None, ..., None]                      # [B][nsplit][R][J][C]
    X = X.view(c.B, g.nsplit, R, J, C8, 8)
    ch = torch.arange(C8)[:, None] * 8 + 2 * (torch.arange(8)[None, :] // 2)
    hi = ch // cpg != (torch.arange(C8)[:, None] * 8) // cpg    # [C8][8]
    acc = torch.zeros(4, c.B, g.nsplit, R, C8)                  # s_lo, q_lo, s_hi, q_hi
    for jj in range(J):
        for e in range(8):
            f = X[:, :, :, jj, :, e]
            h = hi[:, e]
            acc[0] = torch.where(h, acc[0], acc[0] + f)
            acc[1] = torch.where(h, acc[1], acc[1] + f * f)
            acc[2] = torch.where(h, acc[2] + f, acc[2])
            acc[3] = torch.where(h, acc[3] + f * f, acc[3])
    if defect == "swap_hi_lo":
        cx = int((hi.any(1) & ~hi.all(1)).nonzero()[0])        # the first chunk that straddles two groups
        acc[:, :, :, :, cx] = acc[[2, 3, 0, 1]][:, :, :, :, cx]
    lo, hh = acc[:2].permute(1, 2, 3, 4, 0), acc[2:].permute(1, 2, 3, 4, 0)      # [B][nsplit][R][C8][2]
    for grp in range(32):
        cx_lo, cx_hi = (grp * cpg) // 8, ((grp + 1) * cpg - 1) // 8
        s = torch.zeros(c.B, g.nsplit, 2)
        for xx in range(max(0, cx_lo - 1), cx_hi + 1):
            gl_x = (xx * 8) // cpg
            for yy in range(R):
                if gl_x == grp:
                    s = s + lo[:, :, yy, xx]
                if gl_x + 1 == grp:
                    s = s + hh[:, :, yy, xx]
        written = torch.ones(g.nsplit, dtype=torch.bool)
        if defect == "stale_empty_partial":
            written = torch.arange(g.nsplit) * per < c.HW
        partial[:, written, grp] = s[:, written]


def twin_combine(partial, n, eps):
    """The fixed-order fp64 combine of gn_apply_kernel / gn_coef_kernel: (mean, rstd) [B][32] as fp32."""
    nsplit = partial.shape[1]
    red = []
    for part in range(4):
        s = torch.zeros(partial.shape[0], 32, 2, dtype=torch.float64)
        for i in range(16):
            if part + 4 * i < nsplit:
                s = s + partial[:, part + 4 * i].double()
        red.append(s)
    s = ((red[0] + red[1]) + red[2]) + red[3]
    return _finish_stats(s[..., 0], s[..., 1], n, eps)


def _finish_stats(s, q, n, eps):
    mean = s / n
    var = (q / n - mean * mean).clamp_min(0.0)
    return mean.float(), (1.0 / (var + eps).sqrt()).float()


def twin_small_stats(c, x, n, defect=None):
    """gn_small_kernel's statistics half: (mean, rstd) [B][32] as fp32."""
    C = c.C0 + c.C1
    cpg = C // 32
    hp, NT = cpg // 4, small_threads(gn_path(c.HW, c.C0, c.C1))
    n_q = c.HW * hp
    n_it = cdiv(n_q, NT)
    slab = torch.zeros(c.B, 32, n_it * NT, 4)
    slab[:, :, :n_q] = x.view(c.B, c.HW, 32, hp, 4).permute(0, 2, 1, 3, 4).reshape(c.B, 32, n_q, 4)
    slab = slab.view(c.B, 32, n_it, NT, 4)
    s, q = torch.zeros(c.B, 32, NT), torch.zeros(c.B, 32, NT)
    for it in range(n_it):
        a = slab[:, :, it]
        s = s + ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3]))
        q = q + ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + (a[..., 2] * a[..., 2] + a[..., 3] * a[..., 3]))
    s, q = _wave_sum(s.view(c.B, 32, NT // 64, 64))[..., 0].double(), _wave_sum(q.view(c.B, 32, NT // 64, 64))[..., 0].double()
    ss, qq = torch.zeros(c.B, 32, dtype=torch.float64), torch.zeros(c.B, 32, dtype=torch.float64)
    for w in range(NT // 64):
        ss, qq = ss + s[..., w], qq + q[..., w]
    return _finish_stats(ss, qq, n, c.eps)


def twin_gn(c, ins, defect=None):
    """gl_op_groupnorm and gl_op_groupnorm_coef in fp32: {"y": [B HW][C] bf16, "coef": [B][2 C] fp32}."""
    C = c.C0 + c.C1
    cpg = C // 32
    x = twin_sources(c, ins, defect)
    gm, bt = ins["gamma"].float(), ins["beta"].float()
    if defect == "gamma_source_relative" and c.C1:
        gm = torch.cat([gm[:c.C0], gm[:c.C1]])
    n = float(c.HW * ((c.C0 // 32) if defect == "n_from_C0" else cpg))
    two_pass = gn_path(c.HW, c.C0, c.C1) == "two_pass"
    if two_pass:
        g = gn_geometry(c.B, c.HW, C)
        partial = _rnd((c.B, g.nsplit, 32, 2), _seed(c, 50), 100.0)        # what the scratch holds before the launch
        twin_stats(c, x, partial, defect)
        mean, rstd = twin_combine(partial, n, c.eps)
    else:
        mean, rstd = twin_small_stats(c, x, n, defect)
    mean, rstd = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    a = rstd * gm
    cc = _fma32(-mean, a, bt.expand_as(a))
    if two_pass:
        y = _fma32(x, a[:, None], cc[:, None])
    else:
        y = (x - mean[:, None]) * rstd[:, None] * gm + bt
    if c.silu:
        y = _silu32(y)
    halves = (cc, a) if defect == "swap_coef_halves" else (a, cc)
    coef = torch.stack([h.view(c.B, C // 8, 8) for h in halves], 2).reshape(c.B, 2 * C)
    return {"y": y.bfloat16().view(-1, C), "coef": coef}


def twin_ln(c, ins, fill, defect=None):
    """ln_kernel in fp32, one wave per row: the whole payload [B Tpad][ldy] (fill: what it held before)."""
    ldx, ldy, C8 = c.ldx or c.C, c.ldy or c.C, c.C // 8
    out = fill.clone().view(c.B * c.Tpad, ldy)
    col = torch.arange(c.C)[None, :]
    r1 = torch.arange(c.B * c.N1)[:, None]
    rows = _gather_flat(ins["flat"], MARGIN + r1 * ldx + col).float().view(c.B, c.N1, c.C)
    if c.N2:
        r2 = torch.arange(c.B * c.N2)[:, None]
        x2 = _gather_flat(ins["flat2"], MARGIN + r2 * (ldx if defect == "x2_row_stride" else c.C) + col).float().view(c.B, c.N2, c.C)
        rows = torch.cat([rows, x2], 1)
    N = rows.shape[0] * rows.shape[1]
    V = torch.zeros(N, 192, 8)
    V[:, :C8] = rows.reshape(N, C8, 8)
    V = V.view(N, 3, 64, 8)                                   # chunk lane + 64 i sits in lane `lane`, pass i
    have = (torch.arange(3)[:, None] * 64 + torch.arange(64)[None, :] < C8)[None, :, :, None]
    s = torch.zeros(N, 64)
    for i in range(3):
        for e in range(8):
            s = s + V[:, i, :, e]
    mean = (_wave_sum(s)[:, :1] / c.C)[:, None, :, None]      # [N][1][1][1]
    D = torch.where(have, V - mean, torch.zeros(()))
    q = torch.zeros(N, 64)
    for i in range(3):
        for e in range(8):
            q = q + D[:, i, :, e] * D[:, i, :, e]
    rstd = torch.rsqrt(_wave_sum(q)[:, :1] / c.C + torch.tensor(c.eps, dtype=torch.float32))
    y = D.view(N, 192 * 8)[:, :c.C] * rstd
    if c.affine:
        y = y * ins["gamma"].float() + ins["beta"].float()
    real = real_rows(c, "cpu")
    pad = torch.ones(c.B * c.Tpad, dtype=torch.bool)
    pad[real] = False
    out[:, c.C:] = 0
    out[pad] = 0
    if defect == "pad_row_tail_unwritten":
        out[pad, c.C:] = fill.view(c.B * c.Tpad, ldy)[pad, c.C:]
    out[real, :c.C] = y.bfloat16()
    return out


def twin(c, ins, outs, defect=None):
    """The emulation's values into the buffers, as the launches would leave them."""
    for b in outs.values():
        b.reset()
    if c.kind == "gn":
        for name, v in twin_gn(c, ins, defect).items():
            outs[name].put(v)
    else:
        outs["y"].put(twin_ln(c, ins, outs["y"].fill[GUARD: GUARD + outs["y"].payload.numel()], defect))
