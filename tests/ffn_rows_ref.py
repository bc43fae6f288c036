"""The row-local kernels of gligen_amd/csrc/ffn.hip by themselves (gl_op_ff_rows, gl_op_qkv_rows): the case list, guarded buffers, a
float64 reference that follows the kernels' rounding points, a derived per-element bound, and an fp32 emulation that stands in for the
kernels without a GPU. tests/test_ffn_rows_cpu.py checks this module, tests/test_ffn_rows_gpu.py holds the kernels to it.

ROUNDING POINTS the reference follows (read from ffn.hip; u = 2^-24, fp32; bf16 keeps 8 significant bits):
  weights     bf16 of the fp32 weight, after the LayerNorm fold where there is one (W gamma: one fp32 product, reproduced exactly)
  b1          the GEGLU projection's bias rides as a 21st k-step: bf16 of the folded fp32 bias. Every other bias is added in fp32
  t           the leading projection's result, bf16 (the residual stream)
  xn          the normalised rows, bf16, before the projection
  hidden      val * gelu(gate), bf16, before FF-out
  y           bf16 before a trailing projection
Where the kernel hands an intermediate out (qkv_rows: mid_out; ff_rows: mid_out when |gate| <= 1e-20, `out` in front of the to_q
projection) the next stage's reference starts from the STORED values, so each stage is bounded by itself. Where it does not (t with
the residual in the accumulator, y in front of the proj_out projection, xn and the hidden tile always) the reference rounds its own
float64 value and the bound carries the difference:

  round_stage(v, e)   the kernel rounds v' with |v' - v| <= e, the reference rounds v. Both give the same bf16 unless a rounding
                      boundary (a midpoint of the bf16 grid; under a power of two it sits ulp / 4 below) lies within e of v. Where none
                      is in reach the reference goes on with bf16(v) and carries 0. Where one is, it goes on with v itself, unrounded,
                      and carries e + ulp / 2: the kernel's value is one rounding of v' away from v' (the ulp of the far end, which
                      may lie in the next binade); against the reference's own rounded value it would be a whole ulp. That is the
                      worst case, element by element, without charging an element a rounding it cannot have. Behind the LayerNorm
                      few elements are in reach (e is 1e-5 of the value); at the hidden tile most are (e carries the GELU fit and
                      the flips of xn, a third of an ulp), so there the term is the issue's "bf16 rounding of each hidden value
                      carried through |W2|": ulp(v) / 2 lies between 2^-9 |v| and 2^-8 |v|.
  What this costs: rows far from zero (mean 8, 32 standard deviations) put every xn within reach -- the statistics term is a good part
  of an ulp there -- and the worst case of 320 flips through |W1|, the GELU and |W2| is then larger than the output (err / bound of
  those cases is 1e-2 and below). The statistics of such rows are held per element by the ln_probe cases instead, where `out` IS xn.

BOUNDS, per element, as tests/gemm_candidates_ref.py derives them (S = sum |a| |w| in float64 on the rounded inputs):
  product     an operand off by da: da |W|^T; fp32 accumulation of K products and the bias in any order: (K + 2) u (S + |b|)
  statistics  one pass: mean = s / C, var = ss / C - mean^2 with s, ss length-C fp32 sums:
                  e_mean = (C + 2) u sum|x| / C
                  e_var  = (C + 2) u sum x^2 / C + 2 |mean| e_mean + e_mean^2 + 2 u (sum x^2 / C + mean^2)
              -- a multiple of u C (mean^2 + var), which is why a row far from zero loses its variance -- carried into rstd exactly:
                  e_r = (1 - e_var / (var + eps))^-1/2 - 1 + 3 u   (relative; the add and a 1-ulp rsqrt)
              xn = fma(x, rstd, -mean rstd): rstd (dx + e_mean) (1 + e_r) + |xh| e_r + 2 u rstd (|x| + |mean|) (the two terms cancel)
              An input off by dx moves mean by mean(dx) and var by 2 mean(|x - mean| dx) + mean(dx^2).
  GELU        the cubic exp2 fit: |fit(x) - x Phi(x)| <= GELU_FIT = 7.8e-5 for every x (the project's number: ffn.hip, tools/fit_gelu.py;
              test_ffn_rows_cpu.py holds the fp32 evaluation to it) in place of the Abramowitz-Stegun term; |gelu'| <= 1.13 carries the
              gate's own error; 4 u (|x| + 1) for the device's exp2 against the host's and the fma around it
  hidden      |g| e_val + |val| e_g + e_val e_g + 2 u |val g|, then round_stage, carried through |W2|
  residual    plain form: res + gate ff, three fp32 operations. Chained form with the residual in the accumulator: Y starts at
              t (1 / gate) and every one of the 4C + 2 accumulations rounds at the accumulator's magnitude |t / gate| + S, then
              gate (Y + b2): (4C + 8) u (|t| + |gate| (S + |b2|)) -- the issue's "two more roundings of |t|" and the accumulation's
              own, which are of the same size once t / gate dominates the sum (gate = 1e-19)
  output      bf16: 2^-8 |ref|
  row sums    stats_out against the float64 sum / sum of squares of the STORED bf16 outputs: (C + 2) u sum|v|, (C + 2) u sum v^2
Nothing is fitted to what the kernels return.

LAYOUTS. q [B H][Tpad_q][DP] row-major, K in key tiles (gemm.h ktile_off: element (t, c) at (t / 64, c / 8, t % 64, c % 8)), V^T
[B H][DPV][Tpad_k] with the quads of 4 tokens of every 32 in the order 0 2 4 6 1 3 5 7: decoded by gemm_candidates_ref.proj_region on a
buffer of its own offsets (what attention_core_ref.index_map does; its cache is keyed for tq == tq_pad only). Every output sits in a
flat buffer of random finite values with GUARD elements in front and behind; the index of the elements a launch may write is the
layout's written region -- everything else, the stride gaps, the padding rows and columns and the guards, has to keep its bits.
"""
from types import SimpleNamespace

import torch

import attention_core_ref as A
import gemm_candidates_ref as G
from gligen_amd._lib import AttnProjLayout

U = G.U
BF16_ULP = G.BF16_ULP
GUARD = G.GUARD
C = 320
H = 8
D = 40
EPS = 1e-5
GELU_FIT = 7.8e-5          # ffn.hip: "|gelu error| <= 7.8e-5 for every x"
GATE_MIN = 1e-20           # ffn.hip res_in_acc: at or below, t takes the way through mid_out
MAX_BAR, MEAN_BAR = 2.5e-2, 1e-2      # max |err| / max |ref|, mean |err| / mean |ref|: the project's bars for a bf16 output
IN_FILL = 1.0e4           # what the stride gaps of the inputs hold: a row read past its C columns shows


# ---------------------------------------------------------------------------------------------------------------- preconditions
# transcribed once from ffn.hip (ff_rows_supported, ff_rows_launch, qkv_rows_supported, qkv_rows_launch)
def ff_rows_supported(M, Cc):
    return Cc == 320 and M > 0 and M % 128 == 0


def qkv_rows_supported(M, Cc, d, T):
    return Cc == 320 and d == 40 and M > 0 and M % 128 == 0 and T > 0 and T % 128 == 0 and M % T == 0


def ff_preconditions(c):
    """The reasons ff_rows_launch would refuse the case (empty: accepted)."""
    bad = []
    if not ff_rows_supported(c.M, C):
        bad.append("shape")
    if c.ldx % 8 or c.ldo % 4 or (c.res and c.ldres % 4):
        bad.append("strides")
    if c.post and not c.pre:
        bad.append("post without pre")
    if c.post == 2 and (c.qT <= 0 or c.M % c.qT or c.qT % 32 or c.qDP < 40 or c.qDP % 4):
        bad.append("q geometry")
    if c.pre and (not c.normalize or c.ld_pre_res % 4 or c.ld_mid % 4):
        bad.append("pre")
    if c.post == 1 and c.ld_post_res % 4:
        bad.append("post stride")
    if c.post == 2 and c.qTpad < c.qT:
        bad.append("qTpad")           # (the entry point's own check: the kernel addresses token rows [0, qT) of qTpad)
    return bad


def qkv_preconditions(c):
    bad = []
    if not qkv_rows_supported(c.M, C, D, c.T):
        bad.append("shape")
    if c.np not in (1, 3):
        bad.append("np")
    if c.ldx % 8:
        bad.append("ldx")
    if c.np == 3 and c.Tpad_k % 32:
        bad.append("Tpad_k")
    if c.DP < D or c.DP % 8 or (c.np == 3 and c.DPV < D):
        bad.append("head geometry")
    if c.pre and (c.ld_mid % 4 or (c.pre_res and c.ld_pre_res % 4)):
        bad.append("pre strides")
    if c.in_period < 0 or (c.in_period and (c.in_period % c.T or c.M % c.in_period)):
        bad.append("in_period")
    if c.Tpad_q < c.T or (c.np == 3 and (c.Tpad_k < c.T or c.Tpad_k % 64)):
        bad.append("padded token counts")      # (the entry point's own check)
    return bad


# ---------------------------------------------------------------------------------------------------------------- cases
def _ff(name, M=128, normalize=1, affine=None, res=True, gate=None, stats=True, ld=C, mean=0.0, pre=0, post=0, pre_gate=None, qTpad_extra=0, qT=None,
        special=None, stats_ld=1):
    affine = bool(normalize) if affine is None else affine
    qT = (qT or M) if post == 2 else 0
    return SimpleNamespace(kind="ff", name=name, M=M, normalize=normalize, affine=affine, res=bool(res) and not pre, gate=gate, stats=stats, ldx=ld, ldo=ld,
                           ldres=ld, ld_pre_res=ld, ld_mid=ld, ld_post_res=ld, mean=mean, pre=pre, post=post, pre_gate=pre_gate, qDP=48 if post == 2 else 0,
                           qT=qT, qTpad=qT + qTpad_extra if post == 2 else 0, special=special, stats_ld=stats_ld)


def _ff_cases():
    out = []
    gates = (None, 0.37, 0.0, -0.6)
    i = 0
    # plain: normalize x res x gate in full; statistics, stride and the rows' mean spread over them so that every value meets every
    # normalize / res setting (mean only where the rows are normalised: elsewhere it is just a larger input)
    for normalize in (1, 0):
        for res in (True, False):
            for gi, gate in enumerate(gates):
                mean = (0.0, 8.0, 32.0)[(i + gi) % 3] if normalize else 0.0
                out.append(_ff(f"plain_n{normalize}_r{int(res)}_g{gate}_m{mean:g}", normalize=normalize, res=res, gate=gate, stats=(i + gi // 2) % 2 == 0,
                               ld=C + 8 if (i + gi) % 2 else C, mean=mean, stats_ld=2 if gi == 1 else 1))
                i += 1
    out += [_ff(f"plain_M256_m{mean:g}", M=256, gate=0.37, mean=mean, ld=C + 8) for mean in (0.0, 8.0, 32.0)]
    out += [_ff("plain_M384_noaffine", M=384, affine=False, gate=-0.6)]
    # the GELU per hidden feature: w1 = 0, value 1, gate pre-activations from b1, w2 selects hidden feature 4 c + k for output c
    out += [_ff(f"gelu_sweep{k}", normalize=0, res=False, stats=False, special=("sweep", k)) for k in range(4)]
    # the normalised rows themselves: value feature f = xn_f (w1 selects), gate pre-activation 256 (gelu = 256 exactly), w2 = 1 / 256 on
    # the diagonal: every product is exact, `out` holds the kernel's own bf16 xn, and the bound is the statistics term plus its rounding
    out += [_ff(f"ln_probe_m{mean:g}", normalize=1, affine=False, res=False, stats=False, mean=mean, special=("probe",)) for mean in (0.0, 8.0, 32.0)]
    # every output element 1 + 0.9 * 2^-9: stored as 1.0, so statistics of the fp32 values are off by 0.56 per row
    out += [_ff("stats_of_stored", normalize=1, res=False, special=("const",))]
    # chained
    forms = ((0, "pre"), (1, "post1"), (2, "post2"))
    for post, tag in forms:
        for pg, g in ((0.37, -0.6), (None, None), (0.5, 1e-30)):
            out.append(_ff(f"chain_{tag}_g{pg}_{g}", pre=1, post=post, pre_gate=pg, gate=g, ld=C + 8 if post == 1 else C))
        out.append(_ff(f"chain_{tag}_tiny_gate", pre=1, post=post, pre_gate=0.37, gate=1e-19))
        out.append(_ff(f"chain_{tag}_M256_nostats", M=256, pre=1, post=post, pre_gate=0.37, gate=-0.6, stats=False, ld=C + 8, qT=128))
    out += [_ff("chain_post2_qpad", pre=1, post=2, pre_gate=0.37, gate=-0.6, qTpad_extra=64),
            _ff("chain_post2_B2_qpad", M=256, pre=1, post=2, pre_gate=None, gate=0.37, qT=128, qTpad_extra=64, ld=C + 8),
            _ff("chain_post2_B2", M=256, pre=1, post=2, pre_gate=0.37, gate=None, qT=128)]
    return out


def _qkv(name, B=1, T=128, pre=1, pre_res=True, normalize=1, np_=3, pad=0, in_period=0, stats=True, ld=C, M=None, bias=True, affine=True):
    M = M or B * T
    return SimpleNamespace(kind="qkv", name=name, M=M, T=T, B=M // T, pre=pre, pre_res=bool(pre_res) and bool(pre), normalize=1 if pre else normalize, np=np_,
                           Tpad_q=T + pad, Tpad_k=T + pad, DP=48, DPV=48, in_period=in_period, stats=stats and bool(pre), ldx=ld, ld_pre_res=ld, ld_mid=ld,
                           bias=bias, affine=affine and (bool(pre) or bool(normalize)))


def _qkv_cases():
    out = []
    for B in (1, 2, 3):
        out += [_qkv(f"pre_res_B{B}", B=B, pad=64 if B == 2 else 0, ld=C + 8 if B == 3 else C),
                _qkv(f"pre_nores_B{B}", B=B, pre_res=False, pad=0 if B == 2 else 64, stats=B != 1, ld=C + 8 if B == 1 else C)]
    out += [_qkv("nopre_norm", pre=0, normalize=1, B=2, pad=64),
            _qkv("nopre_raw", pre=0, normalize=0, B=2, ld=C + 8, bias=False),
            _qkv("nopre_norm_B3", pre=0, normalize=1, B=3, affine=False),
            _qkv("np1_pre", np_=1, B=2, pad=64),
            _qkv("np1_pre_nores", np_=1, B=1, pre_res=False, ld=C + 8, stats=False),
            _qkv("np1_nopre_norm", np_=1, pre=0, normalize=1, B=2),
            _qkv("np1_nopre_raw", np_=1, pre=0, normalize=0, B=1, pad=64, ld=C + 8),
            # the guidance pair's shared prefix: output row m reads input row m % in_period
            _qkv("period_T_M2T", T=128, M=256, in_period=128, pad=64),
            _qkv("period_2T_M4T", T=128, M=512, in_period=256, ld=C + 8),
            _qkv("period_T_M2T_nopre", T=128, M=256, in_period=128, pre=0, normalize=1)]
    return out


FF_CASES = _ff_cases()
QKV_CASES = _qkv_cases()
CASES = FF_CASES + QKV_CASES
assert len({c.name for c in CASES}) == len(CASES)


def preconditions(c):
    return ff_preconditions(c) if c.kind == "ff" else qkv_preconditions(c)


# ---------------------------------------------------------------------------------------------------------------- inputs and buffers
def _rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _seed(c, k):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) * 64 + k) % (2 ** 31)


def _strided_in(t, ld, dev):
    """bf16 rows [M][C] as a view of stride ld into a buffer whose every other element is IN_FILL."""
    M = t.shape[0]
    flat = torch.full((2 * GUARD + M * ld,), IN_FILL, dtype=torch.bfloat16)
    flat[GUARD: GUARD + M * ld].view(M, ld)[:, :C] = t
    flat = flat.to(dev)
    return flat[GUARD: GUARD + M * ld].view(M, ld)[:, :C]


def sweep_gates():
    """The 4C gate pre-activations of the GELU sweep, as the bf16 values the kernel's bias step holds: dense over [-12, 12] and the
    tails +-20, +-40, +-300."""
    tails = torch.tensor([-300.0, -40.0, -20.0, 20.0, 40.0, 300.0, -12.0, 12.0])
    return torch.cat([torch.linspace(-12.0, 12.0, 4 * C - len(tails)), tails]).bfloat16().float()


def make_inputs(c, dev):
    """The case's tensors on dev: bf16 activations (strided views), fp32 parameters, gates as one-element tensors or None."""
    s = lambda k: _seed(c, k)
    ins = {}
    if c.kind == "ff":
        M = c.M
        x = _rnd((M, C), s(1)) * 1.5 + c.mean * 1.5 if not c.pre else _rnd((M, C), s(1))
        w1, b1 = _rnd((8 * C, C), s(2), C ** -0.5), 0.5 * _rnd((8 * C,), s(3))
        w2, b2 = _rnd((C, 4 * C), s(4), (4 * C) ** -0.5), 0.1 * _rnd((C,), s(5))
        if c.special and c.special[0] == "sweep":
            k = c.special[1]
            x = torch.ones(M, C)
            w1, b1 = torch.zeros(8 * C, C), torch.cat([torch.ones(4 * C), sweep_gates()])
            w2, b2 = torch.zeros(C, 4 * C), torch.zeros(C)
            w2[torch.arange(C), 4 * torch.arange(C) + k] = 1.0
        if c.special and c.special[0] == "probe":
            w1, b1 = torch.zeros(8 * C, C), torch.cat([torch.zeros(4 * C), torch.full((4 * C,), 256.0)])
            w1[torch.arange(C), torch.arange(C)] = 1.0
            w2, b2 = torch.zeros(C, 4 * C), torch.zeros(C)
            w2[torch.arange(C), torch.arange(C)] = 2.0 ** -8
        if c.special and c.special[0] == "const":
            w2, b2 = torch.zeros(C, 4 * C), torch.full((C,), 1.0 + 0.9 * 2.0 ** -9)
        ins.update(x=_strided_in(x.bfloat16(), c.ldx, dev), w1=w1.to(dev), b1=b1.to(dev), w2=w2.to(dev), b2=b2.to(dev))
        if c.affine:
            ins.update(gamma=(1 + 0.3 * _rnd((C,), s(6))).to(dev), beta=(0.2 * _rnd((C,), s(7))).to(dev))
        if c.res:
            ins["res"] = _strided_in(_rnd((M, C), s(8)).bfloat16(), c.ldres, dev)
        if c.gate is not None:
            ins["gate"] = torch.tensor([c.gate], dtype=torch.float32, device=dev)
        if c.pre:
            ins.update(pre_w=_rnd((C, C), s(9), C ** -0.5).to(dev), pre_b=(0.1 * _rnd((C,), s(10))).to(dev),
                       pre_res=_strided_in((_rnd((M, C), s(11)) * 1.3 + 0.2).bfloat16(), c.ld_pre_res, dev))
            if c.pre_gate is not None:
                ins["pre_gate"] = torch.tensor([c.pre_gate], dtype=torch.float32, device=dev)
        if c.post == 1:
            ins.update(post_w=_rnd((C, C), s(12), C ** -0.5).to(dev), post_b=(0.1 * _rnd((C,), s(13))).to(dev),
                       post_res=_strided_in(_rnd((M, C), s(14)).bfloat16(), c.ld_post_res, dev))
        if c.post == 2:
            ins.update(post_w=_rnd((C, C), s(12), C ** -0.5).to(dev), gamma_q=(1 + 0.3 * _rnd((C,), s(15))).to(dev), beta_q=(0.2 * _rnd((C,), s(16))).to(dev))
    else:
        rows = c.in_period or c.M
        ins["x"] = _strided_in(_rnd((rows, C), s(1)).bfloat16() if c.pre else (_rnd((rows, C), s(1)) * 1.3 + 0.2).bfloat16(), c.ldx, dev)
        if c.pre:
            ins.update(pre_w=_rnd((C, C), s(2), C ** -0.5).to(dev), pre_b=(0.1 * _rnd((C,), s(3))).to(dev))
            if c.pre_res:
                ins["pre_res"] = _strided_in((_rnd((rows, C), s(4)) * 1.3 + 0.2).bfloat16(), c.ld_pre_res, dev)
        if c.affine:
            ins.update(gamma=(1 + 0.3 * _rnd((C,), s(5))).to(dev), beta=(0.2 * _rnd((C,), s(6))).to(dev))
        ins["w"] = _rnd((c.np * C, C), s(7), 1.5 * C ** -0.5).to(dev)
        if c.bias:
            ins["bias"] = (0.1 * _rnd((c.np * C,), s(8))).to(dev)
    return ins


def head_layout(T, Tpad_q, Tpad_k, DP, DPV):
    return AttnProjLayout(d=D, dp=DP, dpv=DPV, tq=T, tk=T, tq_pad=Tpad_q, tk_pad=Tpad_k, vt_perm32=1)


def head_index(lay, name, B, dev):
    """Flat offset of logical element [b][token][h d + c] (tokens [0, T)) in buffer `name`."""
    offs = torch.arange(A.buffer_sizes(lay, B, H)[name], dtype=torch.int64, device=dev)
    return G.proj_region(lay, B, H, name, offs)[1].reshape(B * lay.tq, C)


class Buf:
    """One output: a flat buffer of random finite values, GUARD elements around the payload, and `index` [rows][cols], the flat
    offsets of the elements the launch may write (None: it may write nothing)."""

    def __init__(self, n, dtype, index, seed, dev):
        self.fill = (_rnd((n + 2 * GUARD,), seed) * 3).to(dtype).to(dev)
        self.flat = self.fill.clone()
        self.payload = self.flat[GUARD: GUARD + n]
        self.index = None if index is None else index + GUARD
        self.bits = torch.int16 if dtype == torch.bfloat16 else torch.int32

    def reset(self):
        self.flat.copy_(self.fill)

    def put(self, values):
        self.flat[self.index.reshape(-1)] = values.reshape(-1).to(self.flat.dtype)

    def get(self):
        return self.flat[self.index.reshape(-1)].view(self.index.shape)

    def untouched(self):
        """Everything outside `index` holds the bits it was filled with."""
        keep = torch.ones(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        if self.index is not None:
            keep[self.index.reshape(-1)] = False
        return torch.equal(self.flat.view(self.bits)[keep], self.fill.view(self.bits)[keep])


def _rows_index(M, ld, cols, dev):
    return torch.arange(M, device=dev)[:, None] * ld + torch.arange(cols, device=dev)[None, :]


def mid_written(c):
    """ff_rows writes mid_out only when the feed-forward's residual cannot ride in the accumulator."""
    return bool(c.pre) and c.gate is not None and abs(float(torch.tensor(c.gate, dtype=torch.float32))) <= GATE_MIN


def make_outputs(c, dev):
    """{name: Buf} of every buffer the launch is given to write."""
    s = lambda k: _seed(c, 100 + k)
    M, o = c.M, {}
    if c.kind == "ff":
        o["out"] = Buf(M * c.ldo, torch.bfloat16, _rows_index(M, c.ldo, C, dev), s(1), dev)
        if c.pre:
            o["mid"] = Buf(M * c.ld_mid, torch.bfloat16, _rows_index(M, c.ld_mid, C, dev) if mid_written(c) else None, s(2), dev)
        if c.stats:
            o["stats"] = Buf(M * 2 * c.stats_ld, torch.float32, _rows_index(M, 2 * c.stats_ld, 2, dev), s(3), dev)
        if c.post == 2:
            lay = head_layout(c.qT, c.qTpad, c.qTpad, c.qDP, 48)
            o["q"] = Buf(A.buffer_sizes(lay, M // c.qT, H)["q"], torch.bfloat16, head_index(lay, "q", M // c.qT, dev), s(4), dev)
    else:
        lay = head_layout(c.T, c.Tpad_q, c.Tpad_k, c.DP, c.DPV)
        sizes = A.buffer_sizes(lay, c.B, H)
        if c.pre:
            o["mid"] = Buf(M * c.ld_mid, torch.bfloat16, _rows_index(M, c.ld_mid, C, dev), s(2), dev)
        if c.stats:
            o["stats"] = Buf(M * 2, torch.float32, _rows_index(M, 2, 2, dev), s(3), dev)
        for i, name in enumerate(("q", "k", "vt")[:c.np]):
            o[name] = Buf(sizes[name], torch.bfloat16, head_index(lay, name, c.B, dev), s(4 + i), dev)
    return o


def call_fields(c, ins, outs):
    """The fields of gl_ff_rows_args / gl_qkv_rows_args for Engine.op_ff_rows / op_qkv_rows."""
    f = dict(M=c.M, C=C, x=ins["x"], ldx=c.ldx, normalize=c.normalize, gamma=ins.get("gamma"), beta=ins.get("beta"), pre=c.pre,
             pre_w=ins.get("pre_w"), pre_b=ins.get("pre_b"), pre_res=ins.get("pre_res"), ld_pre_res=c.ld_pre_res,
             mid_out=outs["mid"].payload if "mid" in outs else None, ld_mid=c.ld_mid, stats_out=outs["stats"].payload if "stats" in outs else None)
    if c.kind == "ff":
        f.update(w1=ins["w1"], b1=ins["b1"], w2=ins["w2"], b2=ins["b2"], res=ins.get("res"), ldres=c.ldres, gate=ins.get("gate"), out=outs["out"].payload,
                 ldo=c.ldo, stats_ld=c.stats_ld, post=c.post, pre_gate=ins.get("pre_gate"), post_w=ins.get("post_w"), post_b=ins.get("post_b"),
                 post_res=ins.get("post_res"), ld_post_res=c.ld_post_res, gamma_q=ins.get("gamma_q"), beta_q=ins.get("beta_q"),
                 q=outs["q"].payload if "q" in outs else None, qDP=c.qDP, qT=c.qT, qTpad=c.qTpad)
    else:
        f.update(H=H, np=c.np, w=ins["w"], bias=ins.get("bias"), q=outs["q"].payload, k=outs["k"].payload if "k" in outs else None,
                 vt=outs["vt"].payload if "vt" in outs else None, DP=c.DP, DPV=c.DPV, T=c.T, Tpad_q=c.Tpad_q, Tpad_k=c.Tpad_k, in_period=c.in_period)
    return f


# ---------------------------------------------------------------------------------------------------------------- reference and bounds
def bf_round(v):
    return v.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def round_stage(v, e):
    """(the operand the reference goes on with, the most bf16(v') can differ from it for any |v' - v| <= e) -- module docstring."""
    e = torch.as_tensor(e, dtype=torch.float64, device=v.device).expand_as(v)
    a = v.abs()
    _, ex = torch.frexp(a.clamp_min(1e-300))
    ulp = torch.ldexp(torch.ones_like(a), ex - 8)
    fr = a / ulp                                   # in [128, 256): the grid points of v's binade are the integers
    dist = torch.minimum(((fr - fr.floor()) - 0.5).abs(), fr - 128 + 0.25) * ulp     # (the midpoint below a power of two is ulp / 4 under it)
    # in reach: the kernel's bf16(v') against the UNROUNDED v is e and one rounding of v' (half an ulp of v', which may lie in the next
    # binade) -- half of what two independent roundings can differ by
    reach = dist <= e
    return torch.where(reach, v, bf_round(v)), torch.where(reach, e + torch.maximum(ulp, 2.0 ** -7 * (a + e)) / 2, torch.zeros_like(e))


def ln_stage(x, dx):
    """((x - mean) rstd in float64, the bound of the kernel's fp32 one-pass evaluation of it before the bf16 rounding); x exact up to dx."""
    dx = torch.as_tensor(dx, dtype=torch.float64, device=x.device).expand_as(x)
    sa, s2 = x.abs().sum(1), (x * x).sum(1)
    mean = x.mean(1)
    var = s2 / C - mean * mean
    rstd = (var + EPS) ** -0.5
    m, r = mean[:, None], rstd[:, None]
    xh = (x - m) * r
    e_mean = (C + 2) * U * sa / C + dx.mean(1)
    e_var = (C + 2) * U * s2 / C + 2 * mean.abs() * e_mean + e_mean ** 2 + 2 * U * (s2 / C + mean * mean) + 2 * ((x - m).abs() * dx).mean(1) + (dx * dx).mean(1)
    e_r = ((1 - (e_var / (var + EPS)).clamp_max(0.9)) ** -0.5 - 1 + 3 * U)[:, None]
    e_x = r * (dx + e_mean[:, None]) * (1 + e_r) + xh.abs() * e_r + 2 * U * r * (x.abs() + m.abs()) * (1 + e_r) + U * xh.abs()
    return xh, e_x


def matmul_stage(a, da, w, b, e_b, K):
    """(a W^T + b, its bound) for an operand off by da and a bias off by e_b."""
    wa = w.abs().t()
    S = (a.abs() + da) @ wa + b.abs()
    return a @ w.t() + b, da @ wa + (K + 2) * U * S + e_b


def gelu64(x):
    return 0.5 * x * torch.special.erfc(-x * 2 ** -0.5)


def hidden_stage(h, e_h):
    """val gelu(gate) of h = (val | gate), rounded to bf16 as the kernel's P^T operand, and what the kernel's can differ by."""
    n = h.shape[1] // 2
    val, gate, ev, eg = h[:, :n], h[:, n:], e_h[:, :n], e_h[:, n:]
    g = gelu64(gate)
    dg = 1.13 * eg + GELU_FIT + 4 * U * (gate.abs() + 1)
    hid = val * g
    return round_stage(hid, g.abs() * ev + val.abs() * dg + ev * dg + 2 * U * hid.abs())


def folded(w, b, gamma, beta, dev):
    """(bf16 weights, fp32 bias, the bias's error) as float64: through the LayerNorm fold where gamma is given."""
    if gamma is not None:
        return G.folded_affine(w.cpu(), b.cpu(), gamma.cpu(), beta.cpu(), dev)
    return w.bfloat16().double().to(dev), b.double().to(dev), torch.zeros_like(b, dtype=torch.float64, device=dev)


def stats_check(stored, got):
    """stats_out against the stored bf16 rows: [(got, ref, bound)] for the sum and the sum of squares."""
    v = stored.double()
    ref = torch.stack([v.sum(1), (v * v).sum(1)], 1)
    bound = (C + 2) * U * torch.stack([v.abs().sum(1), (v * v).sum(1)], 1) + 2.0 ** -100
    return got.double(), ref, bound


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def expect(c, ins, got):
    """{output: (got as float64, reference, bound)}, every one elementwise over the launch's written region. got: {name: what the
    buffers hold there} (Buf.get)."""
    dev = ins["x"].device
    x = ins["x"].double()
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    checks = {}
    if c.kind == "qkv":
        idx = torch.arange(c.M, device=dev) % (c.in_period or c.M)
        x = x[idx]
        if c.pre:
            pw = ins["pre_w"].bfloat16().double()
            pb = ins["pre_b"].double()
            res = ins["pre_res"].double()[idx] if c.pre_res else torch.zeros_like(x)
            t = x @ pw.t() + pb + res
            e_t = (C + 4) * U * (x.abs() @ pw.abs().t() + pb.abs() + res.abs())
            checks["mid"] = (got["mid"].double(), t, e_t + BF16_ULP * t.abs())
            if c.stats:
                checks["stats"] = stats_check(got["mid"], got["stats"])
            xn, dxn = round_stage(*ln_stage(got["mid"].double(), zero))
        elif c.normalize:
            xn, dxn = round_stage(*ln_stage(x, zero))
        else:
            xn, dxn = x, torch.zeros_like(x)
        bias = ins["bias"] if c.bias else torch.zeros(c.np * C, device=dev)
        wf, bfold, e_b = folded(ins["w"], bias, ins.get("gamma") if c.affine else None, ins.get("beta"), dev)
        r, e = matmul_stage(xn, dxn, wf, bfold, e_b, C)
        for i, name in enumerate(("q", "k", "vt")[:c.np]):
            ref = r[:, i * C: (i + 1) * C]
            checks[name] = (got[name].double(), ref, e[:, i * C: (i + 1) * C] + BF16_ULP * ref.abs())
        return checks
    rows, drows, t_r, dt = x, torch.zeros_like(x), None, None
    if c.pre:
        pw, pb, res = ins["pre_w"].bfloat16().double(), ins["pre_b"].double(), ins["pre_res"].double()
        pg = 1.0 if c.pre_gate is None else _f32(c.pre_gate)
        t = res + pg * (x @ pw.t() + pb)
        e_t = (C + 4) * U * (abs(pg) * (x.abs() @ pw.abs().t() + pb.abs()) + res.abs())
        if mid_written(c):
            checks["mid"] = (got["mid"].double(), t, e_t + BF16_ULP * t.abs())
            t_r, dt = got["mid"].double(), torch.zeros_like(t)
        else:
            t_r, dt = round_stage(t, e_t)
        rows, drows = t_r, dt
    if c.normalize:
        xn, dxn = round_stage(*ln_stage(rows, drows))
    else:
        xn, dxn = rows, drows
    wf, bfold, e_b = folded(ins["w1"], ins["b1"], ins.get("gamma") if c.affine else None, ins.get("beta"), dev)
    b1r, db1 = round_stage(bfold, e_b)
    hid, dhid = hidden_stage(*matmul_stage(xn, dxn, wf, b1r, db1, C))
    w2, b2 = ins["w2"].bfloat16().double(), ins["b2"].double()
    S2 = (hid.abs() + dhid) @ w2.abs().t() + b2.abs()
    ff = hid @ w2.t() + b2
    e_ff = dhid @ w2.abs().t() + (4 * C + 4) * U * S2
    if c.pre:
        g = 1.0 if c.gate is None else _f32(c.gate)
        y = t_r + g * ff
        if mid_written(c):
            e_y = abs(g) * e_ff + 3 * U * (t_r.abs() + abs(g) * ff.abs())
        else:
            e_y = dt + abs(g) * e_ff + (4 * C + 8) * U * (t_r.abs() + dt + abs(g) * S2)
    elif c.res:
        g = 1.0 if c.gate is None else _f32(c.gate)
        res = ins["res"].double()
        y = res + g * ff
        e_y = abs(g) * e_ff + 3 * U * (res.abs() + abs(g) * ff.abs())
    else:
        y, e_y = ff, e_ff                   # (without a residual the gate is not applied)
    if c.post == 1:
        y_r, dy = round_stage(y, e_y)
        o, e_o = matmul_stage(y_r, dy, ins["post_w"].bfloat16().double(), ins["post_b"].double(), zero, C)
        pres = ins["post_res"].double()
        ref = pres + o
        checks["out"] = (got["out"].double(), ref, e_o + 2 * U * (pres.abs() + o.abs()) + BF16_ULP * ref.abs())
    else:
        checks["out"] = (got["out"].double(), y, e_y + BF16_ULP * y.abs())
    if c.stats:
        checks["stats"] = stats_check(got["out"], got["stats"])
    if c.post == 2:
        xq, dxq = round_stage(*ln_stage(got["out"].double(), zero))
        wq, bq, e_bq = folded(ins["post_w"], torch.zeros(C, device=dev), ins["gamma_q"], ins["beta_q"], dev)
        q, e_q = matmul_stage(xq, dxq, wq, bq, e_bq, C)
        checks["q"] = (got["q"].double(), q, e_q + BF16_ULP * q.abs())
    return checks


def verify(c, ins, outs):
    """Every output of the launch: finite, err <= bound at every element, nothing outside the written region touched. Returns
    {output: (worst err / bound, (row, column) where)}; raises AssertionError with the case, the output and the place."""
    got = {}
    for name, b in outs.items():
        assert b.untouched(), (c.name, name, "an element outside the written region changed")
        if b.index is not None:
            got[name] = b.get()
            assert bool(torch.isfinite(got[name].float()).all()), (c.name, name, "not finite")
    worst = {}
    checks = expect(c, ins, got)
    assert set(checks) == {n for n, b in outs.items() if b.index is not None}, (c.name, sorted(checks), "an output is left out of the check")
    for name, (g, ref, bound) in checks.items():
        assert g.shape == ref.shape == bound.shape, (c.name, name)
        ratio = (g - ref).abs() / bound
        w = int(ratio.argmax())
        at = (w // ratio.shape[1], w % ratio.shape[1])
        worst[name] = (float(ratio.reshape(-1)[w]), at)
        assert worst[name][0] <= 1.0, (c.name, name, "err / bound", worst[name][0], "at", at, "got", float(g[at]), "ref", float(ref[at]), "bound", float(bound[at]))
        # the project's bars on top (tests/test_attention_core_gpu.py): where the worst case of the bound is wide -- rows far from zero
        # -- they still hold the output as a whole
        if name != "stats" and float(ref.abs().max()) > 0:
            err = (g - ref).abs()
            bars = (float(err.max() / ref.abs().max()), float(err.mean() / ref.abs().mean()))
            assert bars[0] < MAX_BAR and bars[1] < MEAN_BAR, (c.name, name, "max |err| / max |ref|, mean |err| / mean |ref|", bars)
    return worst


def report_line(c, worst):
    return f"[ffn_rows] {c.name}: " + " ".join(f"{n}={r:.3f}@{at[0]},{at[1]}" for n, (r, at) in worst.items())


# ---------------------------------------------------------------------------------------------------------------- the emulation
def gelu_fit_coefficients():
    """(C3, C2, C1, C0) of the cubic L in gelu(x) = max(x, 0) - |x| 2^L(|x|), read out of ffn.hip."""
    import os
    import re
    src = open(os.path.join(G.ROOT, "gligen_amd", "csrc", "ffn.hip")).read()
    return tuple(float(re.search(rf"#define FFR_GELU_C{i} (-?[0-9.eE+-]+)f", src).group(1)) for i in (3, 2, 1, 0))


def gelu_fit32(x, coef=None):
    """The kernel's GELU in fp32 (geglu_step J = 0 .. 4; every fmaf is one rounding: evaluated in float64 and rounded, which differs
    from a true fma only by double rounding)."""
    c3, c2, c1, c0 = (torch.tensor(v, dtype=torch.float32) for v in (coef or gelu_fit_coefficients()))
    fma = lambda a, b, c_: (a.double() * b.double() + c_.double()).float()
    a = x.abs()
    l = fma(a, c3, c2)
    l = fma(a, l, c1)
    l = fma(a, l, c0)
    return fma(-a, torch.exp2(l), x.clamp_min(0.0))


def _bf32(v):
    return v.bfloat16().float()


def _ln32(v):
    s, ss = v.sum(1, keepdim=True), (v * v).sum(1, keepdim=True)
    mean = s * (1.0 / C)
    var = (ss * (1.0 / C) - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + EPS)
    return _bf32(v * rstd - mean * rstd)


def _fold32(w, b, gamma, beta):
    if gamma is None:
        return _bf32(w), b
    return _bf32(w * gamma), b + w @ beta


def _stats32(v):
    return torch.stack([v.sum(1), (v * v).sum(1)], 1)


def emulate(c, ins, defect=None):
    """The launch in fp32 torch with the kernel's rounding points and its cubic GELU: {output: the values of its written region}.
    defect: one of the seeded mistakes of test_ffn_rows_cpu.py, by name."""
    f = lambda n: None if ins.get(n) is None else ins[n].float()
    x = f("x")
    out = {}
    if c.kind == "qkv":
        idx = torch.arange(c.M) % (c.in_period or c.M)
        xs = x[idx]
        res = f("pre_res")[idx] if c.pre_res else None
        if defect == "no_period":       # output row m from input row m: the rows behind the period are whatever lies there
            xs = torch.cat([x, x.roll(1, 0)] * (c.M // (2 * x.shape[0])))
        if c.pre:
            t = xs @ _bf32(f("pre_w")).t() + f("pre_b")
            t = _bf32(t + res if res is not None else t)
            out["mid"] = t
            if c.stats:
                out["stats"] = _stats32(t)
            xn = _ln32(t)
        else:
            xn = _ln32(xs) if c.normalize else xs
        bias = f("bias") if c.bias else torch.zeros(c.np * C)
        w, b = _fold32(f("w"), bias, f("gamma") if c.affine else None, f("beta"))
        r = _bf32(xn @ w.t() + b)
        for i, name in enumerate(("q", "k", "vt")[:c.np]):
            out[name] = r[:, i * C: (i + 1) * C].clone()
        if defect == "swap_tokens":
            for name in ("k", "vt"):
                out[name][[5, 70]] = out[name][[70, 5]]
        return out
    gate = 1.0 if c.gate is None else torch.tensor(c.gate, dtype=torch.float32)
    rows = x
    if c.pre:
        pg = 1.0 if c.pre_gate is None else torch.tensor(c.pre_gate, dtype=torch.float32)
        rows = _bf32(f("pre_res") + pg * (x @ _bf32(f("pre_w")).t() + f("pre_b")))
        if mid_written(c):
            out["mid"] = rows
    xn = _ln32(rows) if c.normalize else rows
    w1, b1 = _fold32(f("w1"), f("b1"), f("gamma") if c.affine else None, f("beta"))
    h = xn @ w1.t() + _bf32(b1)
    val, gt = h[:, :4 * C].clone(), h[:, 4 * C:].clone()
    if defect == "swap_value_gate":      # block (chunk 3, nb 1): 16 hidden features
        sl = slice(3 * 32 + 16, 3 * 32 + 32)
        val[:, sl], gt[:, sl] = h[:, 4 * C:][:, sl], h[:, :4 * C][:, sl]
    hid = _bf32(val * gelu_fit32(gt))
    w2 = _bf32(f("w2"))
    if defect == "swap_w2_columns":      # the k-slot order of the P^T operand: hidden features 8 jj + 4 h + e
        w2 = w2.clone()
        w2[:, [4, 8]] = w2[:, [8, 4]]
    acc = hid @ w2.t()
    if defect == "drop_chunk":           # the last chunk's contribution to one element of one row (a stale accumulator register),
        last = hid[:, 4 * C - 32:] @ w2[:, 4 * C - 32:].t()       # seeded in row 17 at the column where it is largest there
        col = int(last[17].abs().argmax())
        acc[17, col] -= last[17, col]
    ff = acc + f("b2")
    if c.pre:
        if mid_written(c):
            y = rows + gate * ff
        else:
            y = (rows * (1.0 / gate) + ff) * gate
    elif c.res:
        y = f("res") + gate * ff
    else:
        y = ff
    yb = _bf32(y)
    if defect == "swap_half_waves":      # lanes l and l ^ 32 hold the same row, features 8 j + 4 h + e: their quads exchanged in one row block
        yb = yb.clone()
        yb[32:64] = yb[32:64].view(32, C // 8, 2, 4).flip(2).reshape(32, C)
    if c.post == 1:
        o = _bf32(f("post_res") + (yb @ _bf32(f("post_w")).t() + f("post_b")))
    else:
        o = yb
    out["out"] = o
    if c.stats:
        out["stats"] = _stats32(y if defect == "stats_of_fp32" else o)
    if c.post == 2:
        wq, bq = _fold32(f("post_w"), torch.zeros(C), f("gamma_q"), f("beta_q"))
        out["q"] = _bf32(_ln32(yb) @ wq.t() + bq)
    return out


def store(outs, values):
    """The emulation's values into the buffers, as a launch would leave them."""
    for name, b in outs.items():
        b.reset()
        if b.index is not None:
            b.put(values[name])
