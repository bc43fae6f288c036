"""The attention kernels by themselves (gl_op_attention_core): encoders into the kernels' layouts, the float64 reference, a derived
per-element error bound, a float64 emulation of each kernel's rounding points, and the case list. No GPU is needed for any of it;
tests/test_attention_core_cpu.py checks this module, tests/test_attention_core_gpu.py holds the kernels to it.

Operation: o_i = sum_j w_ij v_j, w = softmax_j(c q_i . k_j), c = d^-0.5, on exact bf16 q, k, v (logical [B][H][N][d]).

ROUNDING POINTS, read from gligen_amd/csrc/attention.hip (u = 2^-8: bf16 keeps 8 significant bits, round to nearest; u32 = 2^-24: fp32). Scores are in log2
units: s_ij = c log2(e) q_i . k_j, p_ij = 2^(s_ij - m_i), A_ij = c log2(e) |q_i| . |k_j|.
  prescale   q~ = bf16(fp32(q) * fp32(c log2 e)) before the score product (98, 431, 762): every kernel at d = 40 and attn3_kernel at
             d = 80. Relative error u (+ u32 of the product, + u32 of the constant) per element: |dS_ij| <= (u + 4 u32) A_ij.
             attn_kernel at d = 80 / 160 multiplies the fp32 score by c log2 e instead (240): no bf16 rounding of q.
  stabiliser m_i. d = 40: a bf16 value (201, 543, 814, 942) that rides through the score MFMA as q column 40 times k column 40 = 1.0, so
             S - m comes out of one fp32 accumulation: exact in the operands, it only has to be CLOSE to the row maximum (moved when
             a tile exceeds it by 2^6; attn3_kernel: the first tile's maximum, then the lazy rule, which quiet rows never trigger).
             Otherwise an fp32 value subtracted in front of the exp2 (240, 488, 859). Each move multiplies every accumulator row of
             the query -- numerator rows and the denominator row alike -- by the same fp32 factor 2^-delta (209, 232, 551, 571, 823,
             936): the factor cancels in o, one fp32 rounding per row and move remains.
  scores     fp32 accumulation over dp (+ 1) terms in the matrix core, then at most two fp32 operations (the fma of 240, or `-= delta`
             / `- m_run`), then v_exp_f32 (about one ulp). In log2 units:
                 e32_ij = u32 ((dp + 8) A_ij + 8 (|s_ij| + max_j |s_ij| + 8)) + 2^-19
             -- generous by a small factor on purpose (it is 2^-11 of the bf16 terms); 2^-19 holds the exp2's own error and the up to
             nt <= 6 rescale roundings.
             e_s = e32 + (u + 4 u32) A_ij where q is prescaled, e32 elsewhere.
  P          p^_ij = bf16(p_ij 2^(+-e_s)) is the B operand of O^T += V^T P^T (248, 488, 859): relative error
                 eps_ij = 2^e_s - 1 + u 2^e_s.
  denominator  "ones" (dpv > d: d = 40, 80): row d of V^T is 1.0, so l_i = sum_j p^_ij comes out of the same MFMAs from the SAME
             bf16 p^ as the numerator (272-284, 609-620, 1032-1044). Because sum_j p_ij (v_j - o*_i) = 0,
                 o_i - o*_i = sum_j p_ij e_ij (v_j - o*_i) / sum_j p_ij (1 + e_ij),   |e_ij| <= eps_ij
                 |o_i - o*_i| <= sum_j w_ij eps_ij |v_j - o*_i| / (1 - sum_j w_ij eps_ij)                                   (E_ones)
             "valu" (dpv == d: d = 160): l_i sums the fp32 p before the bf16 rounding (241-244, 286), so the numerator's bf16
             rounding d_ij (|d_ij| <= u) does not cancel. With e'_ij the error of the fp32 p (|e'_ij| <= eps32_ij = 2^e_s - 1):
                 o_i - o*_i = (sum_j p_ij e'_ij (v_j - o*_i) + sum_j p_ij d_ij (1 + e'_ij) v_j) / sum_j p_ij (1 + e'_ij)
                 |o_i - o*_i| <= (sum_j w_ij eps32_ij |v_j - o*_i| + u sum_j w_ij (1 + eps32_ij) |v_j|) / (1 - sum_j w_ij eps32_ij)   (E_valu)
             -- the u term is NOT centred on o*: at d = 160 a row whose values share a large common part is allowed u times that part.
  accumulation  fp32 over the Nk keys (MFMA chains of 16 / 32 keys, the tile loop, the rescales), for a numerator row and for the
             denominator, then 1 / l and one product (288-299, 620-631, 1044-1054):
                 E_acc = 1.01 u32 (Nk + 2 nt + 8) (sum_j w_ij |v_j| + |o*_i|)
  store      bf16: u |o|.
  bound_i = (E + E_acc) (1 + u) + u |o*_i| + 2^-100   (the last term: p below fp32's normal range is flushed; it is 2^-126 of the row).
Nothing in it is fitted to what the kernels return. If a kernel misses it, the missing rounding point is to be found in the code.

THE EMULATION (`emulate`) runs the tile loop in float64 and rounds at exactly the bf16 points above (q~, the d = 40 stabiliser, P, the
denominator from the rounded or the unrounded p, the store), per kernel flavour; the fp32 points are left exact (they are the e32 and E_acc
terms). test_attention_core_cpu.py asserts emulation <= bound for every case.

DATA. Head-dim channel 0 is reserved (helpers.spike_attention_case does the same): every query row, the padding rows included, holds
Q_CH0 there and ordinary keys hold 0, so a key with g in channel 0 gains exactly Q_CH0 g c log2(e) log2 units against EVERY query.
  random     q, k, v ~ N(0, 1) (bf16)
  uniform    q = 0: every output is the mean of exactly Nk value rows (Nk = 1: v_0 bit for bit)
  last       the last real key carries DOMINANT_UNITS (= helpers.SPIKE_UNITS["quiet"]) log2 units: o is v_{Nk-1}; dropping it is seen
  first      key 0 carries them
The padding of the second run (`padding`): q rows [Nq, tq_pad) are fresh rows of the same distribution; K rows [Nk, tk_pad) are random
rows with PAD_UNITS log2 units in channel 0 -- above every real score of every row, the dominant key's included (asserted) -- and V^T
columns [Nk, tk_pad) are 4 N(0, 1): one such key let in replaces the output by its value row. (With q = 0 no key can score above
another; there the padded keys tie with the real ones and their values pull the mean.)"""
import math
from types import SimpleNamespace

import torch

import gemm_candidates_ref as G
import helpers
from gligen_amd._lib import AttnProjLayout

U = 2.0 ** -8
U32 = 2.0 ** -24
LOG2E = 1.4426950408889634
B, H = 2, 3
Q_CH0 = 4.0
DOMINANT_UNITS = helpers.SPIKE_UNITS["quiet"]
PAD_UNITS = 48.0
QUIET = helpers.SPIKE_BANDS["quiet"][1]
KINDS = ("random", "uniform", "last", "first")
STRUCTURED = ("last", "first")

DPS = {40: 48, 80: 80, 160: 160}
DPVS = {40: 64, 80: 96, 160: 160}
# selector -> the head dims it is instantiated for, the V^T token permutation it reads, rows per query block, pipelined (Nk > 128 only)
KERNELS = {
    "attn_kernel": dict(dims=(40, 80, 160), perm32=0, qblock=128, pipelined=False),
    "attn2_kernel_w4": dict(dims=(40,), perm32=0, qblock=128, pipelined=True),
    "attn2_kernel_w8": dict(dims=(40,), perm32=0, qblock=256, pipelined=True),
    "attn3_kernel": dict(dims=(40, 80), perm32=1, qblock=128, pipelined=True),
}
NK_SHORT = (1, 17, 63, 64, 65, 127, 128, 129, 200)
NK_LONG = (129, 191, 192, 193, 255, 256, 257, 327)
NQS = (1, 31, 33, 64, 100, 127, 128, 129, 257)
NQS_W8 = NQS + (255, 256)
MASTER_NQ = 384            # = the largest tq_pad of the grids


def grid(kernel):
    """(Nq, Nk) of one kernel's test."""
    nks = NK_LONG if KERNELS[kernel]["pipelined"] else NK_SHORT
    return [(nq, nk) for nk in nks for nq in (NQS_W8 if kernel == "attn2_kernel_w8" else NQS)]


def unsupported_table():
    """Every (selector, d, vt_perm32, Nk) of the grids' values, and whether gl_op_attention_core must answer GL_ERR_UNSUPPORTED."""
    out = []
    for kernel, K in KERNELS.items():
        for d in (40, 80, 160):
            for perm32 in (0, 1):
                if perm32 and d == 160:
                    continue                      # no such buffer form exists (GL_ERR_ARG territory, not a kernel question)
                for nk in sorted(set(NK_SHORT + NK_LONG)):
                    ok = d in K["dims"] and perm32 == K["perm32"] and (nk > 128 or not K["pipelined"])
                    out.append((kernel, d, perm32, nk, not ok))
    return out


def flavour(kernel, d):
    """Where a kernel rounds: prescale (q~ in bf16), stab: 'bf16_6' (bf16 stabiliser in the MFMA, moved past 2^6), 'bf16_first' (the first
    tile's maximum; quiet rows never move it again), 'fp32_6' (fp32, moved past 2^6), 'fp32_max' (the running maximum); denom."""
    if kernel == "attn_kernel":
        return dict(prescale=d == 40, stab="bf16_6" if d == 40 else "fp32_max", denom="valu" if d == 160 else "ones")
    if kernel in ("attn2_kernel_w4", "attn2_kernel_w8"):
        return dict(prescale=True, stab="bf16_6", denom="ones")
    return dict(prescale=True, stab="bf16_first" if d == 40 else "fp32_6", denom="ones")


def layout(d, Nq, Nk, perm32):
    """The buffers attn_launch's callers allocate for (d, Nq, Nk); tq = tq_pad and tk = tk_pad, so that gemm_candidates_ref.proj_region
    addresses every token row of them."""
    tq_pad, tk_pad = -(-Nq // 128) * 128, -(-Nk // 64) * 64
    return AttnProjLayout(d=d, dp=DPS[d], dpv=48 if (perm32 and d == 40) else DPVS[d], tq=tq_pad, tk=tk_pad, tq_pad=tq_pad, tk_pad=tk_pad,
                          vt_perm32=perm32)


def buffer_sizes(lay, nb=B, nh=H):
    return dict(q=nb * nh * lay.tq_pad * lay.dp, k=nb * nh * lay.tk_pad * lay.dp, vt=nb * nh * lay.dpv * lay.tk_pad)


_index_cache = {}


def index_map(lay, name, nb=B, nh=H, device="cpu"):
    """Flat offset in buffer `name` of logical element [b][h][token][c]: proj_region (the decoder of the three layouts, the V^T token
    permutation included) read backwards -- it is applied to a buffer that holds its own offsets."""
    key = (name, lay.d, lay.dp, lay.dpv, lay.tq_pad, lay.tk_pad, lay.vt_perm32, nb, nh, str(device))
    if key not in _index_cache:
        offs = torch.arange(buffer_sizes(lay, nb, nh)[name], dtype=torch.int64, device=device)
        _, val = G.proj_region(lay, nb, nh, name, offs)                   # [b][token][h d]
        _index_cache[key] = val.reshape(nb, val.shape[1], nh, lay.d).permute(0, 2, 1, 3).contiguous()
    return _index_cache[key]


def init_required(lay, k, vt, nb=B, nh=H):
    """The values the kernels need outside what the projections write (the header's MUST HOLD table): V^T row d = 1.0 where dpv > d,
    K column 40 = 1.0 at d = 40 -- for every token column, as attn_vt_ones_launch / attn_k_init_launch do."""
    if lay.dpv > lay.d:
        vt.view(nb, nh, lay.dpv, lay.tk_pad)[:, :, lay.d, :] = 1.0
    if lay.d == 40:
        k.view(nb, nh, lay.tk_pad // 64, lay.dp // 8, 64, 8)[:, :, :, 5, :, 0] = 1.0


def encode(lay, q, k, v, pad=None):
    """bf16 buffers (q, k, vt) of logical q [B][H][Nq][d], k, v [B][H][Nk][d]; rows behind the real ones from pad (q [..][tq_pad - Nq][d],
    k, v [..][tk_pad - Nk][d]) or zero. Head-dim padding is zero, the required ones are set."""
    nb, nh, Nq, d = q.shape
    Nk = k.shape[2]
    dev = q.device
    bufs = {}
    for name, x, T in (("q", q, lay.tq_pad), ("k", k, lay.tk_pad), ("vt", v, lay.tk_pad)):
        full = torch.zeros(nb, nh, T, d, dtype=torch.bfloat16, device=dev)
        full[:, :, :x.shape[2]] = x.to(torch.bfloat16)
        if pad is not None:
            full[:, :, x.shape[2]:] = pad[name].to(torch.bfloat16)
        buf = torch.zeros(buffer_sizes(lay, nb, nh)[name], dtype=torch.bfloat16, device=dev)
        buf[index_map(lay, name, nb, nh, dev).reshape(-1)] = full.reshape(-1)
        bufs[name] = buf
    init_required(lay, bufs["k"], bufs["vt"], nb, nh)
    return bufs["q"], bufs["k"], bufs["vt"]


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def _bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def ch0_gain(units, d):
    """The bf16 channel-0 value of a key that gains `units` log2 units against every query (and the units it really gains)."""
    c2 = d ** -0.5 * LOG2E
    g = float(_bf(torch.tensor(units / (Q_CH0 * c2), dtype=torch.float64)))
    return g, Q_CH0 * g * c2


def make_case(d, Nq, Nk, kind, seed=0):
    """Logical float64 q [B][H][Nq][d], k, v [B][H][Nk][d] of bf16 values, and the padding of the second run (see the module docstring).
    The draw depends on (d, Nk, kind) only: the query rows of every Nq are the first rows of one master block of MASTER_NQ rows, so
    the CPU test's pass over Nq = max(NQS) covers the rows of every grid point."""
    lay = layout(d, Nq, Nk, 0)
    assert lay.tq_pad <= MASTER_NQ
    g = torch.Generator().manual_seed(1000003 * d + 17 * Nk + 7 * KINDS.index(kind) + seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    q, k, v = rnd(B, H, MASTER_NQ, d)[:, :, :lay.tq_pad].clone(), rnd(B, H, lay.tk_pad, d), rnd(B, H, lay.tk_pad, d)
    q[..., 0] = Q_CH0
    k[..., 0] = 0
    v[:, :, Nk:] *= 4
    k[:, :, Nk:, 0] = ch0_gain(PAD_UNITS, d)[0]
    if kind == "uniform":
        q[:, :, :Nq] = 0
    elif kind == "last":
        k[:, :, Nk - 1, 0] = ch0_gain(DOMINANT_UNITS, d)[0]
    elif kind == "first":
        k[:, :, 0, 0] = ch0_gain(DOMINANT_UNITS, d)[0]
    q, k, v = _bf(q), _bf(k), _bf(v)
    return SimpleNamespace(d=d, Nq=Nq, Nk=Nk, kind=kind, q=q[:, :, :Nq], k=k[:, :, :Nk], v=v[:, :, :Nk],
                           pad=dict(q=q[:, :, Nq:], k=k[:, :, Nk:], vt=v[:, :, Nk:]))


# ---- reference and bound ------------------------------------------------------------------------------------------------------------
def scores_log2(q, k):
    return (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5 * LOG2E)


def reference(q, k, v):
    """softmax(d^-0.5 q k^T) v in float64, through exp2 of the log2-unit scores (held to torch.softmax by the CPU test)."""
    s = scores_log2(q, k)
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    return (p / p.sum(-1, keepdim=True)) @ v


def reference_and_bound(q, k, v, kernel):
    """(o*, the per-element bound of the module docstring for `kernel`), float64 [..][Nq][d]."""
    d, Nk = q.shape[-1], k.shape[-2]
    f = flavour(kernel, d)
    c2 = d ** -0.5 * LOG2E
    s = scores_log2(q, k)
    A = (q.abs() @ k.abs().transpose(-1, -2)) * c2
    smax = s.abs().max(-1, keepdim=True).values
    e_s = U32 * ((DPS[d] + 8) * A + 8 * (s.abs() + smax + 8)) + 2.0 ** -19
    if f["prescale"]:
        e_s = e_s + (U + 4 * U32) * A
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    w = p / p.sum(-1, keepdim=True)
    o = w @ v
    eps32 = torch.exp2(e_s) - 1
    eps = eps32 + U * torch.exp2(e_s)
    dev = (v.unsqueeze(-3) - o.unsqueeze(-2)).abs()                         # [..][Nq][Nk][d]: |v_j - o*_i|
    wav = w @ v.abs()
    if f["denom"] == "ones":
        we = w * eps
        E = (we.unsqueeze(-1) * dev).sum(-2) / (1 - we.sum(-1, keepdim=True))
    else:
        we = w * eps32
        E = ((we.unsqueeze(-1) * dev).sum(-2) + U * ((w * (1 + eps32)) @ v.abs())) / (1 - we.sum(-1, keepdim=True))
    nt = -(-Nk // 64)
    E_acc = 1.01 * U32 * (Nk + 2 * nt + 8) * (wav + o.abs())
    return o, (E + E_acc) * (1 + U) + U * o.abs() + 2.0 ** -100


def emulate(q, k, v, kernel):
    """The kernel's tile loop in float64, rounded at its bf16 points (module docstring). q, k, v float64 of bf16 values."""
    d, Nk = q.shape[-1], k.shape[-2]
    f = flavour(kernel, d)
    c32 = float(torch.tensor(LOG2E / math.sqrt(d), dtype=torch.float32))
    rb = lambda x: x.to(torch.float32).to(torch.bfloat16).to(torch.float64)
    qs = rb(q.to(torch.float32).to(torch.float64) * c32) if f["prescale"] else q
    S = qs @ k.transpose(-1, -2)                                             # prescaled: log2 units; else the raw q . k
    shape = q.shape[:-1]
    O = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    L = torch.zeros(shape + (1,), dtype=torch.float64, device=q.device)
    m = torch.zeros(shape + (1,), dtype=torch.float64, device=q.device) if f["stab"].startswith("bf16") else None
    for t in range(-(-Nk // 64)):
        st = S[..., 64 * t: min(64 * t + 64, Nk)]
        vt = v[..., 64 * t: min(64 * t + 64, Nk), :]
        if f["stab"].startswith("bf16"):
            mx = (st - m).max(-1, keepdim=True).values
            move = torch.ones_like(mx, dtype=torch.bool) if t == 0 else (mx > 6.0 if f["stab"] == "bf16_6" else torch.zeros_like(mx, dtype=torch.bool))
            m_new = torch.where(move, rb(m + mx), m)
            alpha = torch.exp2(m - m_new) if t > 0 else torch.ones_like(m)
            p32 = torch.exp2(st - m_new)
        elif f["stab"] == "fp32_6":
            mx = st.max(-1, keepdim=True).values
            m_new = mx if t == 0 else torch.where(mx - m > 6.0, mx, m)
            alpha = torch.exp2(m - m_new) if t > 0 else torch.ones_like(mx)
            p32 = torch.exp2(st - m_new)
        else:
            mx = st.max(-1, keepdim=True).values * c32
            m_new = mx if t == 0 else torch.maximum(m, mx)
            alpha = torch.exp2(m - m_new) if t > 0 else torch.ones_like(mx)
            p32 = torch.exp2(st * c32 - m_new)
        m = m_new
        pb = rb(p32)
        O = O * alpha + pb @ vt
        L = L * alpha + (p32 if f["denom"] == "valu" else pb).sum(-1, keepdim=True)
    return rb(O / L)


# ---- the case conditions ------------------------------------------------------------------------------------------------------------
def quiet_margin(q, k):
    """max over rows of (the row's largest score - the largest score of its first 64 keys), log2 units: what attn3_kernel's lazy
    stabiliser at d = 40 sees. Below helpers.SPIKE_BANDS['quiet'][1] no lazy move and no rerun can happen."""
    s = scores_log2(q, k)
    return float((s.max(-1).values - s[..., :64].max(-1).values).max())


def with_first_padded_key(case):
    """The float64 output had the mask let key Nk in (`kv > Nk`): the first padded key of the filled padding."""
    k = torch.cat([case.k, case.pad["k"][:, :, :1]], 2)
    v = torch.cat([case.v, case.pad["vt"][:, :, :1]], 2)
    return reference(case.q, k, v)


def without_last_key(case):
    return reference(case.q, case.k[:, :, :-1], case.v[:, :, :-1])
