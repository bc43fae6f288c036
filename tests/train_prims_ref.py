"""References, cases and the measuring code of the training path's primitive tests (test_train_prims_cpu.py holds the references to
torch on the CPU, test_train_prims_gpu.py and train_prims_child.py run the kernels against them through gligen_amd.engine's
op_train_* wrappers, include/gligen_amd_train_prims.h).

Every primitive has a float64 reference and an fp32 flavour (torch's own fp32 arithmetic; its norms are two-pass); the matrix
products have a third, split3, which forms every product as the kernels do: each fp32 operand x as hi = bf16(x), lo = bf16(x - hi),
the product as hi.hi + lo.hi + hi.lo (summed in float64 here, rounded to fp32 once). A kernel's error is measured per output tensor as
max|got - ref64| / max|ref64| and bounded by a multiple of the same measure of the flavour it belongs to, on that case's own inputs;
reductions get the elementwise bound of their summation tree. The convolutions: conv3 in its three geometries and the conv weight
gradient belong to the split family (three float64 convs of the bf16 halves), the fp32 direct conv gets the elementwise bound of its
sequential fmaf chain; their gradients are written out by hand from the kernels' comments and held to torch.autograd on the CPU. No
constant in this file was obtained by running a kernel."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24          # the unit roundoff of fp32
GUARD = 64                # floats of sentinel on each side of an output: 256 bytes keep the 16-byte alignment float4 stores need
SENTINEL_BITS = 0x4B3C614E   # 12345678.0f: finite, so a guard read by mistake does not look like the NaN prefill


# ---- the measure and the bounds
def rel_max(got, ref):
    """max|got - ref| / max|ref|; a reference that is exactly 0 everywhere admits only an exact 0 (0.0, else inf)."""
    d = float((got.double() - ref.double()).abs().max())
    m = float(ref.double().abs().max())
    if m == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / m


def fp32_family_bound(e32):
    """VALU attention, LayerNorm, GroupNorm, GEGLU: 8 times the fp32 flavour's own error (__expf, rsqrtf, erff at a few ulp and another
    summation order), and never below four ulp of the largest value."""
    return max(8.0 * e32, 2.0 ** -22)


def split_family_bound(e3):
    """MFMA attention and the Linear products: 4 times the split3 flavour's own error (accumulation order, the fp32 softmax arithmetic
    between the products)."""
    return 4.0 * e3


def dot_chain(n):
    """The longest chain of additions of Ctx::dot_reduce over n terms: a thread's strided sum, six shuffle steps, the sixteen wave
    sums -- and, above 2^18 terms, 64 Ki chunks of 64 terms per thread and the sum of the nb partials."""
    if n <= 1 << 18:
        return -(-n // 1024) + 6 + 16
    return 64 + 6 + 16 + -(-n // 65536)


def colsum_chain(R):
    """colsum_kernel: a row lane sums every sixteenth row, then the sixteen partial sums."""
    return -(-R // 16) + 16


def tree_bound(chain, abs_terms_sum):
    """|error| of an fp32 sum whose longest chain of additions is `chain`, one more rounding allowed for forming a term (a product: one
    rounding; the loss's (a - b)^2 takes two and a division follows its sum -- the chain lengths count a first addition to 0 and the
    additions of empty lanes, which are exact, and that slack covers them)."""
    return (chain + 1) * U24 * abs_terms_sum


# ---- guard zones
class Guarded:
    """Output tensors as views into larger buffers: GUARD floats of SENTINEL_BITS on each side, the view pre-filled with NaN (or with
    init[name], for an output the kernel adds to)."""

    def __init__(self, shapes, device, init=None):
        self.bufs, self.views = {}, {}
        for name, shape in shapes.items():
            n = int(math.prod(shape))
            buf = torch.empty(n + 2 * GUARD, device=device, dtype=torch.float32)
            buf.view(torch.int32).fill_(SENTINEL_BITS)
            view = buf[GUARD:GUARD + n].view(*shape)
            if init is not None and name in init:
                view.copy_(init[name])
            else:
                view.fill_(float("nan"))
            self.bufs[name], self.views[name] = buf, view

    def problems(self):
        """What went wrong, as a list of strings: a guard word that changed, a NaN left in an output."""
        out = []
        for name, buf in self.bufs.items():
            bits = buf.view(torch.int32)
            n = buf.numel() - 2 * GUARD
            for side, g in (("front", bits[:GUARD]), ("back", bits[GUARD + n:])):
                bad = (g != SENTINEL_BITS).nonzero().flatten()
                if bad.numel():
                    out.append(f"{name}: {bad.numel()} words of the {side} guard were overwritten (first at offset {int(bad[0])})")
            nans = int(torch.isnan(self.views[name]).sum())
            if nans:
                out.append(f"{name}: {nans} of {n} elements were not written (NaN left)")
            elif not bool(torch.isfinite(self.views[name]).all()):
                out.append(f"{name}: not finite")
        return out

    def cpu(self):
        return {k: v.detach().cpu().clone() for k, v in self.views.items()}


# ---- matrix products in the three flavours: mm(a, b) over the last two dims, a [.., m, k], b [.., k, n]
def bf16_split(x):
    hi = x.float().bfloat16().float()
    lo = (x.float() - hi).bfloat16().float()
    return hi, lo


def mm_split3(a, b):
    ah, al = (t.double() for t in bf16_split(a))
    bh, bl = (t.double() for t in bf16_split(b))
    return (ah @ bh + al @ bh + ah @ bl).float()


FLAVOURS = {"ref": (torch.float64, torch.matmul), "fp32": (torch.float32, torch.matmul), "split3": (torch.float32, mm_split3)}


# ---- attention (the formulas of train_attention.hip's header: the log-sum-exp saved, the probabilities recomputed from it)
def _heads(x, H):
    B, N, HD = x.shape
    return x.reshape(B, N, H, HD // H).permute(0, 2, 1, 3)


def _rows(x):
    B, H, N, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, H * D)


def _attention(q, k, v, dout, H, flavour):
    """q [B, Nq, H D], k / v [B, Nk, H D], dout like q or None -> dict o, lse [B, H, Nq] (, dq, dk, dv), written out by hand:
    s = (q scale) k^T, lse = log sum exp s, o = softmax(s) v; delta = rowsum(dout o), P = exp(s - lse), dP = dout v^T,
    dS = P (dP - delta), dq = scale dS k, dk = dS^T (q scale), dv = P^T dout. As the kernels, q is scaled before it enters a product
    (the prep pass splits q scale), and the forward's second product takes the unnormalised exp(s - rowmax) and divides afterwards."""
    dtype, mm = FLAVOURS[flavour]
    D = q.shape[-1] // H
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=dtype)
    qh, kh, vh = (_heads(t.to(dtype), H) for t in (q, k, v))
    qs = qh * scale
    s = mm(qs, kh.transpose(-1, -2))
    m = s.max(dim=-1, keepdim=True).values
    pt = torch.exp(s - m)
    l = pt.sum(dim=-1, keepdim=True)
    lse = m + torch.log(l)
    o = mm(pt, vh) / l
    out = {"o": _rows(o), "lse": lse.squeeze(-1)}
    if dout is not None:
        gh = _heads(dout.to(dtype), H)
        delta = (gh * o).sum(dim=-1, keepdim=True)
        dP = mm(gh, vh.transpose(-1, -2))
        P = torch.exp(s - lse)
        out["dq"] = _rows(mm(P * (dP - delta), kh) * scale)
        if flavour == "fp32":
            # the VALU dk / dv kernel recomputes the scores as (q k^T) scale and scales dk at the end; the MFMA one reads the scaled q
            P = torch.exp(mm(qh, kh.transpose(-1, -2)) * scale - lse)
            out["dk"] = _rows(mm((P * (dP - delta)).transpose(-1, -2), qh) * scale)
        else:
            out["dk"] = _rows(mm((P * (dP - delta)).transpose(-1, -2), qs))
        out["dv"] = _rows(mm(P.transpose(-1, -2), gh))
    return out


def attention_ref(q, k, v, dout, H):
    return _attention(q, k, v, dout, H, "ref")


def attention_fp32(q, k, v, dout, H):
    return _attention(q, k, v, dout, H, "fp32")


def attention_split3(q, k, v, dout, H):
    return _attention(q, k, v, dout, H, "split3")


def attention_autograd(q, k, v, dout, H):
    """torch.autograd of softmax(q k^T / sqrt(d)) v in float64: what attention_ref's hand-written backward is held to."""
    D = q.shape[-1] // H
    qh, kh, vh = (_heads(t.double(), H).clone().requires_grad_(True) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(D)
    o = torch.softmax(s, dim=-1) @ vh
    o.backward(_heads(dout.double(), H))
    return {"o": _rows(o.detach()), "lse": torch.logsumexp(s.detach(), dim=-1), "dq": _rows(qh.grad), "dk": _rows(kh.grad), "dv": _rows(vh.grad)}


# ---- Linear: y = x W^T + b, dx = dy W, dW = dy^T x, db = column sums of dy
def _linear(x, W, b, dy, flavour):
    dtype, mm = FLAVOURS[flavour]
    x, W, b, dy = (t.to(dtype) for t in (x, W, b, dy))
    return {"y": mm(x, W.t()) + b, "dx": mm(dy, W), "dW": mm(dy.t(), x), "db": dy.sum(dim=0)}


def linear_ref(x, W, b, dy):
    return _linear(x, W, b, dy, "ref")


def linear_fp32(x, W, b, dy):
    return _linear(x, W, b, dy, "fp32")


def linear_split3(x, W, b, dy):
    return _linear(x, W, b, dy, "split3")


# ---- LayerNorm, GroupNorm + SiLU, GEGLU: torch's ops and torch.autograd, in float64 (the reference) or float32 (the fp32 flavour)
def layernorm_ref(x, g, b, eps, dy, dx0=None, dtype=torch.float64):
    """-> y, xhat, rstd [R], dx (+ dx0), dgamma, dbeta."""
    x, g, b, dy = (t.to(dtype) for t in (x, g, b, dy))
    xr, gr, br = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    C = x.shape[-1]
    y = F.layer_norm(xr, (C,), gr, br, eps)
    y.backward(dy)
    dx = xr.grad if dx0 is None else xr.grad + dx0.to(dtype)
    return {"y": y.detach(), "xhat": F.layer_norm(x, (C,), None, None, eps), "rstd": torch.rsqrt(x.var(dim=-1, unbiased=False) + eps), "dx": dx,
            "dgamma": gr.grad, "dbeta": br.grad}


def layernorm_fp32(x, g, b, eps, dy, dx0=None):
    return layernorm_ref(x, g, b, eps, dy, dx0, dtype=torch.float32)


def groupnorm_silu_ref(x, g, b, silu, eps, da, dx0=None, dtype=torch.float64):
    """Pixel rows x [B, HW, C], 32 groups of adjacent channels -> a, xhat, rstd [B, 32], dx (+ dx0). Mean and two-pass variance by
    torch, written out because F.group_norm refuses a group of one value (B = HW = 1, C = 32); test_train_prims_cpu.py holds it to
    F.group_norm where that runs."""
    x, g, b, da = (t.to(dtype) for t in (x, g, b, da))
    B, HW, C = x.shape
    xr = x.clone().requires_grad_(True)
    xg = xr.reshape(B, HW, 32, C // 32)
    var, mean = torch.var_mean(xg, dim=(1, 3), unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    xhat = ((xg - mean) * rstd).reshape(B, HW, C)
    u = xhat * g + b
    a = F.silu(u) if silu else u
    a.backward(da)
    dx = xr.grad if dx0 is None else xr.grad + dx0.to(dtype)
    return {"a": a.detach(), "xhat": xhat.detach(), "rstd": rstd.detach().reshape(B, 32), "dx": dx}


def groupnorm_silu_fp32(x, g, b, silu, eps, da, dx0=None):
    return groupnorm_silu_ref(x, g, b, silu, eps, da, dx0, dtype=torch.float32)


def geglu_ref(u, dh, dtype=torch.float64):
    """u [R, 2 I] = (val | gate) -> h = val gelu(gate) (erf GELU), du."""
    ur = u.to(dtype).clone().requires_grad_(True)
    val, gate = ur.chunk(2, dim=-1)
    h = val * F.gelu(gate)
    h.backward(dh.to(dtype))
    return {"h": h.detach(), "du": ur.grad}


def geglu_fp32(u, dh):
    return geglu_ref(u, dh, dtype=torch.float32)


# ---- the convolutions. Tensors are pixel rows [B, H, W, C] outside and NCHW inside; w is OIHW [Cout, Cin, 3, 3]
Conv3Case = namedtuple("Conv3Case", "geom B H W Cin Cout")          # geom 0 stride 1, 1 Downsample (stride 2), 2 Upsample (nearest 2x + conv)
DirectCase = namedtuple("DirectCase", "B H W Cin Cout c0 n")         # dx for the input channels [c0, c0 + n)
SPLIT_MUTATIONS = ("lo_hi_last_row", "hi_lo_tap0", "bf16x1")         # what conv_split3 / wgrad_split3 can be told to get wrong


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _pixel_rows(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_f64(a, w, stride=1):
    """The 3x3 / pad 1 conv of a [B, C, H, W] with w OIHW in float64."""
    return F.conv2d(a.double(), w.double(), None, stride, 1)


def conv_split3(a, w, stride=1, mut=None):
    """The conv as Ctx::conv3 forms it: fp32 a and w as hi = bf16(.), lo = bf16(. - hi), three float64 convs hi.hi + lo.hi + hi.lo,
    rounded to fp32 once. mut (test_train_prims_cpu.py's mutations): lo_hi_last_row drops the lo_a hi_w pass on the last row of each
    output image, hi_lo_tap0 drops hi_a lo_w for the tap ky = kx = 0, bf16x1 keeps hi.hi alone."""
    assert a.dtype == torch.float32 and w.dtype == torch.float32 and mut in (None,) + SPLIT_MUTATIONS
    ah, al = (t.double() for t in bf16_split(a))
    wh, wl = (t.double() for t in bf16_split(w))
    cv = lambda p, q: F.conv2d(p, q, None, stride, 1)
    hh = cv(ah, wh)
    if mut == "bf16x1":
        return hh.float()
    lh, hl = cv(al, wh), cv(ah, wl)
    if mut == "lo_hi_last_row":
        lh[:, :, -1, :] = 0
    elif mut == "hi_lo_tap0":
        wl0 = torch.zeros_like(wl)
        wl0[:, :, 0, 0] = wl[:, :, 0, 0]
        hl = hl - cv(ah, wl0)
    return (hh + lh + hl).float()


def dgrad_weight(w, flip=True):
    """conv_dgrad_weight_kernel: W'[i][o][ky][kx] = W[o][i][2 - ky][2 - kx], the filter of the data-gradient conv."""
    return (w.flip(2, 3) if flip else w).transpose(0, 1).contiguous()


def _conv3(c, x, w, b, dy, cv, dtype, mut=None):
    """y and dx of a Conv3Case by the formulas of the kernels' comments, cv the conv of the flavour and dtype what it returns:
    geom 0  y = conv(x, w) + b,                  dx = conv(dy, W')
    geom 1  y = conv(x, w, stride 2) + b,        dx = conv(z, W'), z [H, W] = dy at the even positions, zeros elsewhere
    geom 2  y = conv(nearest2x(x), w) + b,       dx = the 2 x 2 block sums (p00 + p01) + (p10 + p11) of conv(dy, W') at [2H, 2W]
    mut: no_flip (W' without the flip), zero_insert_odd (dy at the odd positions), sum2x2_missing (p11 left out)."""
    xn, dyn = _nchw(x), _nchw(dy)
    a = xn.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) if c.geom == 2 else xn
    y = cv(a, w, 2 if c.geom == 1 else 1) + b.to(dtype).view(1, -1, 1, 1)
    wt = dgrad_weight(w, flip=mut != "no_flip")
    if c.geom == 0:
        dx = cv(dyn, wt)
    elif c.geom == 1:
        z = torch.zeros(c.B, c.Cin, c.H, c.W)
        o = 1 if mut == "zero_insert_odd" else 0
        z[:, :, o::2, o::2] = dyn
        dx = cv(z, wt)
    else:
        gu = cv(dyn, wt)
        p00, p01, p10, p11 = gu[:, :, 0::2, 0::2], gu[:, :, 0::2, 1::2], gu[:, :, 1::2, 0::2], gu[:, :, 1::2, 1::2]
        dx = (p00 + p01) + (p10 if mut == "sum2x2_missing" else p10 + p11)
    assert y.dtype == dtype and dx.dtype == dtype
    return {"y": _pixel_rows(y), "dx": _pixel_rows(dx)}


def conv3_ref(c, x, w, b, dy):
    return _conv3(c, x, w, b, dy, conv_f64, torch.float64)


def conv3_split3(c, x, w, b, dy, mut=None):
    """The split3 flavour of a Conv3Case: conv_split3, then the code's own fp32 composition (bias add, 2 x 2 sums). mut: one of
    SPLIT_MUTATIONS goes to every conv, the others to _conv3."""
    if mut in SPLIT_MUTATIONS:
        return _conv3(c, x, w, b, dy, lambda a, q, stride=1: conv_split3(a, q, stride, mut), torch.float32)
    return _conv3(c, x, w, b, dy, conv_split3, torch.float32, mut)


def conv3_autograd(c, x, w, b, dy):
    """torch.autograd through F.conv2d(stride) and F.interpolate(mode="nearest") in float64: what conv3_ref is held to."""
    xr = _nchw(x).double().clone().requires_grad_(True)
    a = F.interpolate(xr, scale_factor=2, mode="nearest") if c.geom == 2 else xr
    y = F.conv2d(a, w.double(), b.double(), 2 if c.geom == 1 else 1, 1)
    y.backward(_nchw(dy).double())
    return {"y": _pixel_rows(y.detach()), "dx": _pixel_rows(xr.grad)}


def _wgrad_terms(dyn, xn):
    """(dy [B, Cout, HW], col [B, 9 Cin, HW]): im2col_f32_kernel's columns c 9 + ky 3 + kx, zero for the taps outside the image."""
    return dyn.reshape(dyn.shape[0], dyn.shape[1], -1), F.unfold(xn, 3, padding=1)


def wgrad_f64(dyn, xn):
    """conv_wgrad: dW [Cout][Cin][3][3] = dy^T col, the sum over every pixel of every sample."""
    d, col = _wgrad_terms(dyn.double(), xn.double())
    return torch.einsum("bop,bkp->ok", d, col).reshape(dyn.shape[1], xn.shape[1], 3, 3)


def wgrad_split3(dyn, xn, mut=None):
    """lin_wgrad's three passes: dy is the activation side (hi, lo, hi), the im2col of x the weight side (hi, hi, lo). mut as
    conv_split3: the lo_dy hi_col pass without the pixels of each image's last row, hi_dy lo_col without the columns of tap 0, or hi.hi
    alone; dW_taps_transposed exchanges ky and kx in the result."""
    assert dyn.dtype == torch.float32 and xn.dtype == torch.float32
    (dh, col_h), (dl, col_l) = (_wgrad_terms(p.double(), q.double()) for p, q in zip(bf16_split(dyn), bf16_split(xn)))
    mm = lambda p, q: torch.einsum("bop,bkp->ok", p, q)
    out = mm(dh, col_h)
    if mut != "bf16x1":
        if mut == "lo_hi_last_row":
            dl = dl.clone()
            dl[:, :, -dyn.shape[3]:] = 0
        elif mut == "hi_lo_tap0":
            col_l = col_l.clone()
            col_l[:, 0::9] = 0
        out = out + mm(dl, col_h) + mm(dh, col_l)
    out = out.float().reshape(dyn.shape[1], xn.shape[1], 3, 3)
    return out.transpose(2, 3).contiguous() if mut == "dW_taps_transposed" else out


def direct_ref(c, x, w, b, dy, clamp=False):
    """conv3x3_direct's y, the data gradient of the channels [c0, c0 + n) (the direct conv of dy over rows c0 .. c0 + n of W') and dW,
    float64 -- and y_abs, dx_abs: the same sums over absolute values (+ |b|), what the fp32 chain's bound is made of. clamp (a
    mutation): the taps outside the image read the nearest pixel instead of 0."""
    def cv(a, q):
        if clamp:
            return F.conv2d(F.pad(a.double(), (1, 1, 1, 1), mode="replicate"), q.double())
        return conv_f64(a, q)
    xn, dyn = _nchw(x), _nchw(dy)
    wt = dgrad_weight(w)[c.c0:c.c0 + c.n]
    bb = b.double().view(1, -1, 1, 1)
    return {"y": _pixel_rows(cv(xn, w) + bb), "dx": _pixel_rows(cv(dyn, wt)), "dW": wgrad_f64(dyn, xn),
            "y_abs": _pixel_rows(conv_f64(xn.abs(), w.abs()) + bb.abs()), "dx_abs": _pixel_rows(conv_f64(dyn.abs(), wt.abs()))}


def direct_autograd(c, x, w, b, dy):
    xr, wr = _nchw(x).double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
    y = F.conv2d(xr, wr, b.double(), 1, 1)
    y.backward(_nchw(dy).double())
    return {"y": _pixel_rows(y.detach()), "dx": _pixel_rows(xr.grad[:, c.c0:c.c0 + c.n]), "dW": wr.grad}


def direct_bounds(c, ref):
    """conv3x3_direct_kernel is one sequential fp32 chain per output element: acc = b, then 9 Cin_eff fmaf in tap and channel order (fewer
    at the border). Each fmaf rounds once, so |err| <= 9 Cin_eff 2^-24 (sum |x||w| + |b|) to first order, elementwise; tree_bound allows one
    rounding more. Cin_eff is the contraction's channel count: Cin for y, Cout for dx."""
    return {"y": tree_bound(9 * c.Cin, ref["y_abs"]), "dx": tree_bound(9 * c.Cout, ref["dx_abs"])}


# ---- the cases
AttnCase = namedtuple("AttnCase", "D Nq Nk B H regime")
# both tile sizes (32, and the prep pass's 64) crossed on each side, Nk below one tile, a single query
ATTN_PAIRS = [(1, 1), (31, 33), (32, 32), (33, 31), (64, 64), (65, 30), (70, 75), (94, 94), (256, 77)]
ATTN_PAIRS_SHORT = [(33, 31), (65, 30), (70, 75)]
ATTN_REGIMES = ("scale4", "onehot", "uniform", "neg60")
MFMA_DIMS = (32, 40, 64, 80)


def attention_cases(dims=(32, 40, 64, 80, 160)):
    cases = []
    for D in dims:
        for Nq, Nk in (ATTN_PAIRS if D in (40, 160) else ATTN_PAIRS_SHORT):
            cases.append(AttnCase(D, Nq, Nk, 2, 2, None))
    if 40 in dims:
        cases.append(AttnCase(40, 70, 75, 1, 3, None))
    return cases


def attention_regime_cases():
    return [AttnCase(D, 70, 75, 2, 2, r) for D in (40, 160) for r in ATTN_REGIMES]


def case_id(c):
    if isinstance(c, AttnCase):
        return f"d{c.D}-q{c.Nq}-k{c.Nk}-b{c.B}-h{c.H}" + (f"-{c.regime}" if c.regime else "")
    return "-".join(str(v) for v in c)


def attention_inputs(c):
    """Seeded N(0, 1) q, k, v, dout [B, N, H D] fp32, reshaped by the case's regime:
    scale4   q and k times 4: logits of a few tens
    onehot   every query shares a component (q = n + 1.5 c), key j0 = 8 mean(q): its score is about 18 sqrt(D), one probability is
             about 1 and the others underflow
    uniform  all keys equal: uniform probabilities, dq = 0
    neg60    keys share a component (k = u + n / 4) and q -> q - c with c = 60 sqrt(D) u / |u|^2 per head: every score is near -60"""
    gen = torch.Generator().manual_seed(1000 * c.D + 10 * c.Nq + c.Nk + 7 * c.H + len(c.regime or ""))
    HD = c.H * c.D
    q, dout = (torch.randn(c.B, c.Nq, HD, generator=gen) for _ in range(2))
    k, v = (torch.randn(c.B, c.Nk, HD, generator=gen) for _ in range(2))
    if c.regime == "scale4":
        q, k = 4 * q, 4 * k
    elif c.regime == "onehot":
        q = q + 1.5 * torch.randn(c.B, 1, HD, generator=gen)
        k[:, c.Nk // 2] = 8 * q.mean(dim=1)
    elif c.regime == "uniform":
        k = k[:, :1].expand(-1, c.Nk, -1).contiguous()
    elif c.regime == "neg60":
        u = torch.randn(c.B, 1, HD, generator=gen)
        k = u + 0.25 * k
        norm2 = u.reshape(c.B, 1, c.H, c.D).pow(2).sum(dim=-1, keepdim=True)
        q = q - (60 * math.sqrt(c.D) * u.reshape(c.B, 1, c.H, c.D) / norm2).reshape(c.B, 1, HD)
    return q, k, v, dout


def attention_zero_gradients(c, q, k, dout, ref, split=True):
    """The gradients of a case that are 0 in exact arithmetic, {name: absolute bar}: dS sums to 0 over the keys, so dq = scale (dS k) is 0
    when all keys are equal (regime uniform, Nk = 1), and dS itself is 0 where one probability is 1 (Nk = 1; regime onehot, up to
    e^-100), which makes dk = dS^T (q scale) 0 as well. Their float64 reference is rounding noise (asserted here: below 1e-9 of the
    bar's scale), a relative measure means nothing, and the kernel's tensor is held absolutely to u max|dout| max|k| (dq) or
    u max|dout| max|q| (dk), the scale of a gradient with dS of order 1: u = 2^-16 for the split family (the dropped lo.lo term of its
    products), u = 2^-22 for the fp32 kernels (four ulp, the floor of fp32_family_bound)."""
    names = {"uniform": ("dq",), "onehot": ("dq", "dk")}.get(c.regime, ())
    if c.Nk == 1:
        names = ("dq", "dk")
    bars = {}
    for n in names:
        scale = float(dout.abs().max() * (k if n == "dq" else q).abs().max())
        assert float(ref[n].abs().max()) < 1e-9 * scale, (n, float(ref[n].abs().max()))
        bars[n] = (2.0 ** -16 if split else 2.0 ** -22) * scale
    return bars


# (M, K, N): the shipped models' products at a short row count (320 -> 320 and 768 -> 320 / 640), one tile plus one row, a single
# row, and the padded-K / padded-N forms of ConvNeXt's first stage. gemm_launch takes all of them (K a multiple of 64 after padding, N
# of 4).
LINEAR_SHAPES = [(188, 320, 320), (60, 768, 320), (154, 768, 640), (65, 64, 64), (1, 320, 320), (100, 96, 384), (100, 384, 96)]
LN_SHAPES = [(1, 320), (3, 96), (5, 1280), (188, 320), (4, 63), (4, 65)]
GN_SHAPES = [(1, 1, 32), (2, 16, 64), (1, 256, 320), (2, 64, 96)]        # channels per group 1, 2, 10, 3
OFFSETS = [0, 8, 30]
GEGLU_SHAPES = [(1, 1), (3, 255), (5, 257), (188, 1280)]
DOT_SIZES = [1, 1023, 1025, 1 << 18, (1 << 18) + 1, 3 * (1 << 16) + 7 + (1 << 18)]


# Ctx::conv3, stride 1 (B, H, W, Cin, Cout): the halo kernel with 8-row tiles of one image forward and the narrow-output family (N = 64)
# in dgrad; halo with one whole image per tile in both directions; the widest halo image; no power of two, H != W, M = 240 ragged against
# every tile; M = 192; the deep contraction K = 27 * 640; the 2 x 2 level; 1 x 1, where every tap but the centre is padding
CONV3_SHAPES = [(2, 32, 32, 64, 128), (8, 16, 16, 128, 128), (1, 64, 64, 64, 128), (1, 12, 20, 192, 128), (3, 8, 8, 128, 320), (2, 8, 8, 640, 320),
                (2, 2, 2, 128, 128), (1, 1, 1, 64, 64)]
CONV3_DOWN_SHAPES = [(2, 16, 16, 128), (1, 12, 20, 64), (1, 2, 2, 64), (1, 64, 64, 64)]        # (B, H, W, C) of the input
CONV3_UP_SHAPES = [(2, 8, 8, 128), (1, 6, 10, 64), (1, 1, 1, 64), (2, 16, 16, 128)]            # the last: a 32 x 32 dgrad at M = 2048, halo
# conv3x3_direct (B, H, W, Cin, Cout, c0, n): the last conv (C -> 4) three times, the first conv, the inpainting models' (K = 81, padded to
# 128 in conv_wgrad), the spatial-map models' downsampler slice
CONV_DIRECT_SHAPES = [(2, 8, 8, 320, 4, 0, 320), (1, 5, 7, 64, 4, 0, 64), (1, 1, 1, 64, 4, 0, 64), (2, 8, 8, 4, 320, 0, 4), (2, 8, 8, 9, 64, 0, 9),
                      (1, 5, 7, 12, 64, 4, 8)]
CONV_FAMILIES = ("conv_halo_kernel", "gemm_u_kernel(conv)", "gemm_glds_kernel(conv)")      # what the conv3 list as a whole has to run


def conv3_cases():
    return ([Conv3Case(0, *s) for s in CONV3_SHAPES] + [Conv3Case(1, *s, s[3]) for s in CONV3_DOWN_SHAPES]
            + [Conv3Case(2, *s, s[3]) for s in CONV3_UP_SHAPES])


def direct_cases():
    return [DirectCase(*s) for s in CONV_DIRECT_SHAPES]


def conv_case_id(c):
    if isinstance(c, Conv3Case):
        return f"g{c.geom}-{c.B}x{c.H}x{c.W}-{c.Cin}-{c.Cout}"
    return f"direct-{c.B}x{c.H}x{c.W}-{c.Cin}-{c.Cout}-c{c.c0}n{c.n}"


def conv_inputs(c):
    """Seeded x [B, H, W, Cin] N(0, 1), w N(0, 1) (9 Cin)^-1/2, a bias N(0, 1), dy (shaped like y) N(0, 1) drawn independently."""
    geom = getattr(c, "geom", 0)
    gen = torch.Generator().manual_seed(((c.B * 131 + c.H) * 131 + c.W) * 1009 + c.Cin * 17 + c.Cout * 3 + geom + 29 * getattr(c, "c0", 0))
    Ho, Wo = {0: (c.H, c.W), 1: (c.H // 2, c.W // 2), 2: (2 * c.H, 2 * c.W)}[geom]
    x = torch.randn(c.B, c.H, c.W, c.Cin, generator=gen)
    w = torch.randn(c.Cout, c.Cin, 3, 3, generator=gen) / math.sqrt(9 * c.Cin)
    return x, w, torch.randn(c.Cout, generator=gen), torch.randn(c.B, Ho, Wo, c.Cout, generator=gen)


def gemm_kernel_family(rec):
    """A gemm_plan_log record's kernel family, "(conv)" behind it when the instantiation is the implicit-GEMM 3x3 conv's (A_CONV3 = 1: the
    fourth template argument of gemm_u_kernel, the last of gemm_glds_kernel); the halo kernel is a conv by itself."""
    name = rec["kernel"]
    fam = name.split("<")[0]
    args = [a.strip() for a in name.split("<", 1)[1].split(">")[0].split(",")] if "<" in name else []
    conv = (fam == "gemm_u_kernel" and len(args) > 3 and args[3] == "1") or (fam == "gemm_glds_kernel" and args and args[-1] == "1")
    return fam + ("(conv)" if conv else "")


def linear_inputs(M, K, N):
    gen = torch.Generator().manual_seed(M * 1000003 + K * 1009 + N)
    return (torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / math.sqrt(K), torch.randn(N, generator=gen), torch.randn(M, N, generator=gen))


def layernorm_inputs(R, C, m):
    """x: N(0, 1) rows plus the offset m, the last row constant (variance 0) when there are at least three; g, b, dy, dx0 N(0, 1)."""
    gen = torch.Generator().manual_seed(R * 100003 + C * 101 + m)
    x = torch.randn(R, C, generator=gen) + m
    if R >= 3:
        x[-1] = m + 1.7
    g, b = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    return x, g, b, torch.randn(R, C, generator=gen), torch.randn(R, C, generator=gen)


def groupnorm_inputs(B, HW, C, m):
    gen = torch.Generator().manual_seed(B * 1000003 + HW * 1009 + C * 11 + m)
    x = torch.randn(B, HW, C, generator=gen) + m
    g, b = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    return x, g, b, torch.randn(B, HW, C, generator=gen), torch.randn(B, HW, C, generator=gen)


def geglu_inputs(R, I):
    """u = (val | gate) N(0, 1), the first gate column swept over [-12, 12] (more than one row), dh N(0, 1)."""
    gen = torch.Generator().manual_seed(R * 10007 + I)
    u = torch.randn(R, 2 * I, generator=gen)
    if R > 1:
        u[:, I] = torch.linspace(-12, 12, R)
    return u, torch.randn(R, I, generator=gen)


def dot_inputs(n):
    gen = torch.Generator().manual_seed(n)
    return torch.randn(n, generator=gen), torch.randn(n, generator=gen)


# ---- running a case on the device. Each run_* returns (rows, problems): rows = [(case, tensor, err, bound)], problems = strings
def _twice(call, shapes, init=None, device=None):
    """The call into guarded outputs, twice: (outputs on the CPU, problems) -- guards, NaN left, a second call that differs in a bit."""
    runs = []
    for _ in range(2):
        G = Guarded(shapes, device, init)
        call(G.views)
        torch.cuda.synchronize(device)
        runs.append(G)
    problems = runs[0].problems() + runs[1].problems()
    a, b = runs[0].cpu(), runs[1].cpu()
    problems += [f"{n}: the second call differs" for n in a if not torch.equal(a[n], b[n])]
    return a, problems


def _rows_of(cid, got, ref, flavour, bound_of, names):
    return [(cid, n, rel_max(got[n], ref[n]), bound_of(rel_max(flavour[n], ref[n]))) for n in names]


def run_attention(engine, c, valu=False):
    """valu: the process runs with GL_TRAIN_ATTN_VALU=1, every head dim is on the fp32 kernels."""
    q, k, v, dout = attention_inputs(c)
    ref = attention_ref(q, k, v, dout, c.H)
    split = c.D in MFMA_DIMS and not valu
    flav = (attention_split3 if split else attention_fp32)(q, k, v, dout, c.H)
    bound_of = split_family_bound if split else fp32_family_bound
    dev = engine.device
    shapes = {"o": q.shape, "lse": (c.B, c.H, c.Nq), "dq": q.shape, "dk": k.shape, "dv": k.shape}
    call = lambda out: engine.op_train_attention(q, k, v, c.H, dout=dout, out=out)
    got, problems = _twice(call, shapes, device=dev)
    dq_only, p2 = _twice(call, {n: shapes[n] for n in ("o", "lse", "dq")}, device=dev)
    problems += ["dq-only call: " + p for p in p2]
    problems += [f"{n}: the dq-only call differs from the full call" for n in dq_only if not torch.equal(dq_only[n], got[n])]
    cid = case_id(c)
    zeros = attention_zero_gradients(c, q, k, dout, ref, split)
    rows = _rows_of(cid, got, ref, flav, bound_of, ("o", "lse", "dq", "dk", "dv"))
    rows = [r for r in rows if r[1] not in zeros] + [(cid, n + "(abs)", float(got[n].abs().max()), bar) for n, bar in zeros.items()]
    return rows, [f"{cid} {p}" for p in problems]


def run_linear(engine, M, K, N):
    x, W, b, dy = linear_inputs(M, K, N)
    ref, flav = linear_ref(x, W, b, dy), linear_split3(x, W, b, dy)
    shapes = {"y": (M, N), "dx": (M, K), "dW": (N, K), "db": (N,)}
    got, problems = _twice(lambda out: engine.op_train_linear(x, W, b, dy, out=out), shapes, device=engine.device)
    cid = case_id((M, K, N))
    rows = _rows_of(cid, got, ref, flav, split_family_bound, ("y", "dx", "dW"))
    rows.append(_reduction_row(cid, "db", got["db"], ref["db"], tree_bound(colsum_chain(M), dy.double().abs().sum(dim=0))))
    return rows, [f"{cid} {p}" for p in problems]


def _reduction_row(cid, name, got, ref, bound):
    """A reduction's row: the worst element's |error| / bound against 1 (elementwise bound; an element whose bound is 0 must be exact)."""
    d = (got.double() - ref.double()).abs()
    ratio = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
    return (cid, name, float(ratio.max()), 1.0)


def run_layernorm(engine, R, C, m, eps, accumulate):
    x, g, b, dy, dx0 = layernorm_inputs(R, C, m)
    dx0 = dx0 if accumulate else None
    ref, flav = layernorm_ref(x, g, b, eps, dy, dx0), layernorm_fp32(x, g, b, eps, dy, dx0)
    shapes = {"y": (R, C), "xhat": (R, C), "rstd": (R,), "dx": (R, C), "dgamma": (C,), "dbeta": (C,)}
    call = lambda out: engine.op_train_layernorm(x, g, b, eps, dy=dy, accumulate=accumulate, out=out)
    got, problems = _twice(call, shapes, init={"dx": dx0} if accumulate else None, device=engine.device)
    cid = case_id((R, C, f"m{m}", f"eps{eps:g}", f"acc{int(accumulate)}"))
    rows = _rows_of(cid, got, ref, flav, fp32_family_bound, ("y", "xhat", "rstd", "dx"))
    # the two column sums are held to the float64 sums of the terms the kernel summed: dy, and dy times the xhat it was given
    terms = dy.double() * got["xhat"].double()
    rows.append(_reduction_row(cid, "dgamma", got["dgamma"], terms.sum(dim=0), tree_bound(colsum_chain(R), terms.abs().sum(dim=0))))
    rows.append(_reduction_row(cid, "dbeta", got["dbeta"], ref["dbeta"], tree_bound(colsum_chain(R), dy.double().abs().sum(dim=0))))
    return rows, [f"{cid} {p}" for p in problems]


def run_groupnorm(engine, B, HW, C, m, silu, accumulate, eps=1e-5):
    x, g, b, da, dx0 = groupnorm_inputs(B, HW, C, m)
    dx0 = dx0 if accumulate else None
    ref, flav = groupnorm_silu_ref(x, g, b, silu, eps, da, dx0), groupnorm_silu_fp32(x, g, b, silu, eps, da, dx0)
    shapes = {"a": x.shape, "xhat": x.shape, "rstd": (B, 32), "dx": x.shape}
    call = lambda out: engine.op_train_groupnorm(x, g, b, silu=silu, eps=eps, da=da, accumulate=accumulate, out=out)
    got, problems = _twice(call, shapes, init={"dx": dx0} if accumulate else None, device=engine.device)
    cid = case_id((B, HW, C, f"m{m}", f"silu{int(silu)}", f"acc{int(accumulate)}"))
    return _rows_of(cid, got, ref, flav, fp32_family_bound, ("a", "xhat", "rstd", "dx")), [f"{cid} {p}" for p in problems]


def run_geglu(engine, R, I):
    u, dh = geglu_inputs(R, I)
    ref, flav = geglu_ref(u, dh), geglu_fp32(u, dh)
    got, problems = _twice(lambda out: engine.op_train_geglu(u, dh=dh, out=out), {"h": (R, I), "du": (R, 2 * I)}, device=engine.device)
    cid = case_id((R, I))
    return _rows_of(cid, got, ref, flav, fp32_family_bound, ("h", "du")), [f"{cid} {p}" for p in problems]


def run_dot(engine, n, mode, alpha=0.3, scale=0.5):
    """mode 0: scale (1 - tanh(alpha)^2) sum a b; mode 1: mean((a - b)^2). The terms of the bound are the summed products times the
    coefficient."""
    a, b = dot_inputs(n)
    if mode == 0:
        alpha = float(torch.tensor(alpha, dtype=torch.float32))      # the value the kernel reads
        coef = scale * (1.0 - math.tanh(alpha) ** 2)
        terms = coef * a.double() * b.double()
    else:
        terms = (a.double() - b.double()) ** 2 / n
    al = torch.tensor([alpha]) if mode == 0 else None
    got, problems = _twice(lambda out: engine.op_train_dot(a, b, mode, alpha=al, scale=scale, out=out), {"out": (1,)}, device=engine.device)
    cid = case_id((n, f"mode{mode}"))
    row = _reduction_row(cid, "out", got["out"], terms.sum().reshape(1), tree_bound(dot_chain(n), terms.abs().sum().reshape(1)))
    return [row], [f"{cid} {p}" for p in problems]


def run_conv3(engine, c, kernels=None):
    """y and dx of gl_op_train_conv3 against conv3_ref, split-family bound. kernels (a dict): kernels[case id] = the kernel families of
    the GEMM plan log for the case's launches."""
    x, w, b, dy = conv_inputs(c)
    ref, flav = conv3_ref(c, x, w, b, dy), conv3_split3(c, x, w, b, dy)
    shapes = {"y": ref["y"].shape, "dx": x.shape}
    cid = conv_case_id(c)
    engine.gemm_plan_log_clear()
    got, problems = _twice(lambda out: engine.op_train_conv3(x, w, b, c.geom, dy=dy, out=out), shapes, device=engine.device)
    if kernels is not None:
        kernels[cid] = sorted({gemm_kernel_family(r) for r in engine.gemm_plan_log()[0]})
    return _rows_of(cid, got, ref, flav, split_family_bound, ("y", "dx")), [f"{cid} {p}" for p in problems]


def conv3_kernels(engine, c):
    """The kernel families one forward + backward of the case launches (no reference is computed)."""
    x, w, b, dy = conv_inputs(c)
    engine.gemm_plan_log_clear()
    engine.op_train_conv3(x, w, b, c.geom, dy=dy)
    return sorted({gemm_kernel_family(r) for r in engine.gemm_plan_log()[0]})


def run_conv_direct(engine, c):
    """y and dx of gl_op_train_conv_direct elementwise against the fp32 chain's bound (direct_bounds), dW in the split family."""
    x, w, b, dy = conv_inputs(c)
    ref = direct_ref(c, x, w, b, dy)
    bounds = direct_bounds(c, ref)
    dW3 = wgrad_split3(_nchw(dy), _nchw(x))
    shapes = {"y": ref["y"].shape, "dx": ref["dx"].shape, "dW": w.shape}
    call = lambda out: engine.op_train_conv_direct(x, w, b, c0=c.c0, n=c.n, dy=dy, out=out)
    got, problems = _twice(call, shapes, device=engine.device)
    cid = conv_case_id(c)
    rows = [_reduction_row(cid, n, got[n], ref[n], bounds[n]) for n in ("y", "dx")]
    rows.append((cid, "dW", rel_max(got["dW"], ref["dW"]), split_family_bound(rel_max(dW3, ref["dW"]))))
    return rows, [f"{cid} {p}" for p in problems]


def format_rows(rows):
    return [f"{cid:38s} {name:8s} err {err:.3e}  bound {bound:.3e}  err/bound {(err / bound if bound else (0.0 if err == 0 else math.inf)):.3f}"
            for cid, name, err, bound in rows]


def failures(rows):
    return [r for r in rows if not r[2] <= r[3]]
