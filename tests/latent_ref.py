"""References of the image-to-image / two-pass tests: the taps of gl_op_latent_renoise from their formulas in float64, the operator in
float64 (F.interpolate) and as an fp32 restatement in the kernel's order, its error bound, and float64 sampler loops (PLMS and DDIM
written from ldm/models/diffusion/plms.py and ddim.py; the 2M loop is tests/dpm_solver_ref.dpm_sample) that start from a float64
resize + q_sample and run the tail of a schedule. Nothing here imports the product's kernels, tables or samplers.

    nearest-exact: source index min(floor((2 o + 1) in / (2 out)), in - 1), in integers
    bilinear:      src = (o + 1/2) in / out - 1/2 clamped at 0; taps floor(src), floor(src) + 1 with weights 1 - t, t
    bicubic:       the same coordinate unclamped; taps floor(src) - 1 .. floor(src) + 2, cubic convolution with A = -0.75
    tap indices are clamped to [0, in - 1]
"""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

MODES = ("nearest-exact", "bilinear", "bicubic")
N_TAPS = {"nearest-exact": 1, "bilinear": 2, "bicubic": 4}

# (in, out) axis pairs of the tests. On these torch's nearest-exact (a float product, floor((o + 0.5) * float(in / out))) picks the index
# of the integer formula; it does not for 187 other pairs with in <= 64 (2 -> 41, for one), which is why the tests assert the agreement.
SIZE_PAIRS = ((8, 16), (8, 20), (12, 28), (16, 8), (5, 5), (7, 7), (1, 4), (16, 24), (24, 40), (3, 7), (2, 9), (16, 32), (64, 128))

# [B, C, h, w] -> (h2, w2) of the operator tests
OP_SHAPES = (((3, 4, 8, 8), (16, 16)), ((3, 4, 8, 12), (20, 28)), ((3, 4, 16, 16), (8, 8)), ((3, 4, 5, 7), (5, 7)), ((3, 4, 1, 1), (4, 4)),
             ((3, 4, 16, 24), (24, 40)), ((3, 4, 3, 2), (7, 9)), ((2, 3, 48, 80), (96, 160)))


def nearest_index(o, n_in, n_out):
    return min(((2 * o + 1) * n_in) // (2 * n_out), n_in - 1)


def axis_taps(n_in, n_out, mode):
    """(first_index int64 [n_out], weights float64 [n_out, 4]): tap p of output o reads clamp(first_index[o] + p, 0, n_in - 1). The
    coordinate is an exact rational; the weights are evaluated in float64 from it."""
    first = np.zeros(n_out, dtype=np.int64)
    w = np.zeros((n_out, 4), dtype=np.float64)
    for o in range(n_out):
        if mode == "nearest-exact":
            first[o], w[o, 0] = nearest_index(o, n_in, n_out), 1.0
            continue
        src = Fraction((2 * o + 1) * n_in - n_out, 2 * n_out)
        if mode == "bilinear":
            src = max(src, Fraction(0))
            i0 = math.floor(src)
            t = float(src - i0)
            first[o], w[o, :2] = i0, (1.0 - t, t)
        else:
            A = -0.75
            i0 = math.floor(src)
            t = float(src - i0)
            cc1 = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0                 # |x| <= 1
            cc2 = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A           # 1 < |x| < 2
            first[o], w[o] = i0 - 1, (cc2(t + 1.0), cc1(t), cc1(1.0 - t), cc2(2.0 - t))
    return first, w


def axis_matrix(n_in, n_out, mode, first=None, w=None, dtype=np.float64):
    """[n_out, n_in] with the taps' weights added on their clamped source indices; (first, w): other taps than axis_taps'."""
    if first is None:
        first, w = axis_taps(n_in, n_out, mode)
    m = np.zeros((n_out, n_in), dtype=dtype)
    for o in range(n_out):
        for p in range(N_TAPS[mode]):
            m[o, min(max(int(first[o]) + p, 0), n_in - 1)] += w[o, p]
    return m


def abs_axis_matrix(n_in, n_out, mode):
    first, w = axis_taps(n_in, n_out, mode)
    return axis_matrix(n_in, n_out, mode, first, np.abs(w))


def resize64(src, size, mode):
    """F.interpolate in float64, align_corners=False, no antialias."""
    kw = {} if mode == "nearest-exact" else dict(align_corners=False)
    return F.interpolate(src.double(), size=tuple(size), mode=mode, **kw)


def renoise64(src, size, mode, sa, s1, noise):
    out = resize64(src, size, mode) * float(sa)
    return out if noise is None else out + float(s1) * noise.double()


def renoise_bound(src, size, mode, sa, s1, noise):
    """(taps^2 + 8) 2^-24 (|sa| sum |w| |v| + |s1| |noise|), per element: the bar the fp32 grid resize is held to."""
    h, w = src.shape[2:]
    wy, wx = abs_axis_matrix(h, size[0], mode), abs_axis_matrix(w, size[1], mode)
    mag = torch.einsum("yh,bchw,xw->bcyx", torch.from_numpy(wy), src.double().abs(), torch.from_numpy(wx)) * abs(float(sa))
    if noise is not None:
        mag = mag + abs(float(s1)) * noise.double().abs()
    return (N_TAPS[mode] ** 2 + 8) * 2.0 ** -24 * mag


def renoise_fp32(src, size, mode, sa, s1, noise, taps_y, taps_x):
    """The kernel's arithmetic in numpy float32, in its order: per source row the horizontal taps ascending, then the rows ascending,
    then two rounded products and one rounded sum. taps_*: (first_index, weights float32 [n, 4]) of the two axes."""
    f32 = np.float32
    x = src.numpy().astype(f32)
    B, C, h, w = x.shape
    h2, w2 = size
    nt = N_TAPS[mode]
    (fy, wy), (fx, wx) = taps_y, taps_x
    ix = np.clip(np.asarray(fx)[:, None] + np.arange(nt)[None, :], 0, w - 1)          # [w2, nt]
    iy = np.clip(np.asarray(fy)[:, None] + np.arange(nt)[None, :], 0, h - 1)          # [h2, nt]
    if mode == "nearest-exact":
        acc = x[:, :, iy[:, 0]][:, :, :, ix[:, 0]]
    else:
        wx, wy = np.asarray(wx, dtype=f32), np.asarray(wy, dtype=f32)
        rows = None                                                                   # [B, C, h, w2]
        for q in range(nt):
            term = wx[None, None, None, :, q] * x[:, :, :, ix[:, q]]
            rows = term if rows is None else (rows + term).astype(f32)
        acc = None
        for p in range(nt):
            term = wy[None, None, :, p, None] * rows[:, :, iy[:, p], :]
            acc = term if acc is None else (acc + term).astype(f32)
    out = (f32(sa) * acc).astype(f32)
    if noise is not None:
        out = (out + (f32(s1) * np.broadcast_to(noise.numpy().astype(f32), out.shape)).astype(f32)).astype(f32)
    return torch.from_numpy(np.ascontiguousarray(out))


# ---- float64 sampler loops on the tail of a schedule ----------------------------------------------------------------------------------
def tail_grid(grid, k):
    """The last k steps of (timesteps, a_t, a_prev) in sampling order."""
    return tuple(np.asarray(v)[len(v) - k:].copy() for v in grid)


def start64(x_init, size, mode, sched, t0, noise):
    """float64 resize + q_sample to timestep t0 (ldm/models/diffusion/ldm.py q_sample)."""
    x = resize64(x_init, size, mode)
    if x.shape[0] != noise.shape[0]:
        x = x.expand(noise.shape[0], *x.shape[1:])
    return float(sched["sqrt_alphas_cumprod"][int(t0)]) * x + float(sched["sqrt_one_minus_alphas_cumprod"][int(t0)]) * noise.double()


def _guided(eps_fn, x, ts, scale, guidance_scale):
    e = eps_fn(x, ts, True, scale).double()
    if guidance_scale != 1:
        eu = eps_fn(x, ts, False, scale).double()
        e = eu + guidance_scale * (e - eu)
    return e


def plms_sample(eps_fn, x, grid, guidance_scale, alphas=None, on_gate_off=None, multistep=True):
    """plms.py:78-158 in float64 (multistep=False: ddim.py:111-134 with eta 0) over grid = (timesteps, a_t, a_prev) in sampling order:
    e' from the Adams-Bashforth history, two evaluations on the first step (the second at the next timestep), then
    pred_x0 = (x - sqrt(1 - a_t) e') / sqrt(a_t), x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev) e'."""
    timesteps, a_t, a_prev = grid
    S = len(timesteps)
    x = x.double()
    b = x.shape[0]
    hist = []

    def back(xx, e, i):
        at, ap = float(a_t[i]), float(a_prev[i])
        return math.sqrt(ap) * (xx - math.sqrt(1.0 - at) * e) / math.sqrt(at) + math.sqrt(1.0 - ap) * e
    for i, step in enumerate(timesteps):
        scale = 1.0 if alphas is None else float(alphas[i])
        if alphas is not None and alphas[i] == 0 and on_gate_off is not None:
            on_gate_off()
        ts = torch.full((b,), int(step), dtype=torch.long)
        e_t = _guided(eps_fn, x, ts, scale, guidance_scale)
        if not multistep:
            e_p = e_t
        elif len(hist) == 0:
            ts_next = torch.full((b,), int(timesteps[min(i + 1, S - 1)]), dtype=torch.long)
            e_p = (e_t + _guided(eps_fn, back(x, e_t, i), ts_next, scale, guidance_scale)) / 2
        elif len(hist) == 1:
            e_p = (3 * e_t - hist[-1]) / 2
        elif len(hist) == 2:
            e_p = (23 * e_t - 16 * hist[-1] + 5 * hist[-2]) / 12
        else:
            e_p = (55 * e_t - 59 * hist[-1] + 37 * hist[-2] - 9 * hist[-3]) / 24
        x = back(x, e_p, i)
        hist = (hist + [e_t])[-3:]
    return x
