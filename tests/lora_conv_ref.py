"""References, cases and the measuring code of the tests of LoRA adapters on 3 x 3 convs (test_lora_conv_cpu.py holds the float64
references to autograd and the mutation table; test_lora_conv_gpu.py runs the kernels of csrc/train_lora_conv.hip against them
through Engine.op_lora_conv3, include/gligen_amd_train_lora_conv.h).

The adapted conv: y = conv(x, W) + b + s up(down(x)), down [r, Ci, 3, 3] with the base conv's stride and padding, up [Co, r] (1 x 1),
s = alpha / r; this file is about the low-rank term alone. Activations are pixel rows [B, H, W, C]. Three geometries: 0 stride 1 pad 1,
1 stride 2 pad 1 (Downsample, H/2 x W/2 outputs), 2 stride 1 pad 1 after nearest 2x (Upsample, 2H x 2W outputs).

Two float64 references: conv_ref builds the term from F.conv2d on the NCHW permutation (geometry 2 after repeat_interleave) and takes
dx, g_down, g_up from autograd; gather_ref writes everything out over a table idx [Mo, 9] of the x row each output pixel reads
through each tap (-1: zero padding) -- the form the kernels have, and the form the mutations are made in.

Error bounds: every element of a kernel's output is a sum formed by a chain of fp32 additions; its bound is
train_prims_ref.tree_bound(chain, sum of |terms|) = (chain + 1) 2^-24 sum|terms|, the chain counted off csrc/train_lora_conv.hip and
csrc/train_lora.hip:
  lora_conv_down_kernel   t: two accumulators (even and odd instructions), each nine taps x Ci / 64 steps x 8 instructions x 4
                          contraction indices = 9 Ci / 2 fused multiply-adds, and their sum: 9 Ci / 2 + 1.
  lora_up_kernel          y += s t up^T: r fused multiply-adds (padding to a multiple of 4 adds exact zeros), fmaf(s, sum, y): r + 1.
  lora_down_kernel        u = dy up over Co: two accumulators of Co / 2 and their sum: Co / 2 + 1.
  lora_conv_dgrad_kernel  dx += s (...): one accumulator through nine taps (geometry 2: four readers per tap, 36 terms) of 4 ceil(r / 4)
                          fused multiply-adds each, then fmaf(s, sum, dx): 9 (36) * 4 ceil(r / 4) + 1.
  lora_conv_wgrad_kernel + its reduce   per chunk of `chunk` output rows two accumulators of chunk / 2 and their sum, the partials of
                          the chunks in ascending order, the product with s: chunk / 2 + 1 + (chunks - 1) + 1.
  lora_wgrad_kernel + its reduce        g_up: the same over the Mo output rows.
The products that read a kernel's own output (y and g_up read t; dx and g_down read u) are held to float64 on the t / u the kernel
produced, so each kernel is measured by itself; end to end (float64 all the way) a product's bound grows by what its operand's bound
lets through: |s| bound(t) |up|^T for y, and so on (end_to_end_bounds). No constant in this file was obtained by running a kernel."""
import math

import torch
import torch.nn.functional as F

import train_prims_ref as P
from lora_train_ref import wgrad_chunk_rows

GEOM_NAMES = {0: "conv", 1: "down", 2: "up"}

# ---- the cases the issue sets: (geom, B, H, W, Ci, Co, r)
SHAPES = {
    0: [(1, 1), (2, 2), (3, 5), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (16, 17)],
    1: [(2, 2), (6, 4), (16, 34)],
    2: [(1, 1), (3, 2), (8, 9)],
}
CHANNELS = [(64, 64), (128, 64), (320, 320), (640, 320)]
RANKS = [1, 4, 24, 128]
SWEEP_IMAGES = [(3, 5), (16, 17)]


def shape_cases(geom):
    """Every image of the geometry at B = 2, (Ci, Co) = (64, 64), rank 4; geometry 0 also B = 1 at 16 x 17."""
    cases = [(geom, 2, H, W, 64, 64, 4) for H, W in SHAPES[geom]]
    return cases + ([(0, 1, 16, 17, 64, 64, 4)] if geom == 0 else [])


def channel_cases():
    """Every (Ci, Co) on the 3 x 5 and 16 x 17 images, the rank walking through all of its values."""
    return [(0, 2, H, W, Ci, Co, RANKS[(i + j) % 4]) for j, (H, W) in enumerate(SWEEP_IMAGES) for i, (Ci, Co) in enumerate(CHANNELS)]


def rank_cases():
    """Every rank on the 3 x 5 and 16 x 17 images; the resampling geometries meet every rank tile count on their middle image."""
    cases = [(0, 2, H, W, 64, 64, r) for H, W in SWEEP_IMAGES for r in RANKS]
    return cases + [(1, 2, 6, 4, 64, 64, r) for r in (1, 24, 128)] + [(2, 2, 3, 2, 64, 64, r) for r in (1, 24, 128)]


def exact_cases():
    """Exact-integer cases: all three geometries, both sides of a 64-row workgroup, two contraction stages, two rank tiles."""
    return [(0, 2, 3, 5, 64, 64, 4), (0, 2, 5, 13, 128, 64, 24), (0, 1, 16, 17, 64, 128, 4), (1, 2, 2, 2, 64, 64, 4), (1, 2, 6, 4, 128, 64, 24),
            (1, 2, 16, 34, 64, 64, 4), (2, 2, 1, 1, 64, 64, 4), (2, 2, 3, 2, 128, 64, 24), (2, 2, 8, 9, 64, 64, 4)]


def case_id(c):
    geom, B, H, W, Ci, Co, r = c
    return f"{GEOM_NAMES[geom]}-B{B}-{H}x{W}-Ci{Ci}-Co{Co}-r{r}"


def out_hw(geom, H, W):
    return (H // 2, W // 2) if geom == 1 else (2 * H, 2 * W) if geom == 2 else (H, W)


# ---- the gather table, and the ways of getting it wrong
MUTATIONS = {   # mutation -> (geometries it exists in, tensors it reaches)
    "taps_flipped": ((0, 1, 2), ("t", "dx", "g_down")),
    "g_down_kykx": ((0, 1, 2), ("g_down",)),
    "border_clamped": ((0, 1, 2), ("t", "dx", "g_down")),
    "halo_across_images": ((0, 1, 2), ("t", "dx", "g_down")),
    "up_no_bounds_test": ((2,), ("t", "dx", "g_down")),
    "zero_insert_odd": ((1,), ("dx",)),
    "last_row_tap_dropped": ((0, 1, 2), ("t", "dx", "g_down")),
}


def gather_table(geom, B, H, W, mut=None):
    """idx [Mo, 9] int64: the row of x [B H W] that output pixel m reads through tap 3 ky + kx, -1 where it reads zero padding.
    mut (of the table): border_clamped -- the coordinate is clamped into the image; halo_across_images -- only the flat row index
    is tested, so the row above an image's first row is the previous image's last; up_no_bounds_test -- geometry 2's (o + k - 1) / 2
    rounds -1 to 0 as integer division does and only the upper edge is tested; last_row_tap_dropped -- the last output row loses its
    centre tap."""
    Ho, Wo = out_hw(geom, H, W)
    b, oy, ox = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    b, oy, ox = b.reshape(-1, 1), oy.reshape(-1, 1), ox.reshape(-1, 1)
    ky, kx = torch.arange(9).reshape(1, 9) // 3, torch.arange(9).reshape(1, 9) % 3
    st = 2 if geom == 1 else 1
    iy, ix = st * oy + ky - 1, st * ox + kx - 1
    Hh, Ww = (2 * H, 2 * W) if geom == 2 else (H, W)
    if mut == "border_clamped":
        iy, ix = iy.clamp(0, Hh - 1), ix.clamp(0, Ww - 1)
    if mut == "up_no_bounds_test":
        assert geom == 2
        ok = (iy <= Hh - 1) & (ix <= Ww - 1)
        iy, ix = iy.clamp_min(0), ix.clamp_min(0)        # trunc(-1 / 2) = 0
    elif mut == "halo_across_images":
        flat = b * Hh + iy
        ok = (flat >= 0) & (flat < B * Hh) & (ix >= 0) & (ix < Ww)
    else:
        ok = (iy >= 0) & (iy < Hh) & (ix >= 0) & (ix < Ww)
    if geom == 2:
        iy, ix = iy >> 1, ix >> 1
    idx = torch.where(ok, (b * H + iy) * W + ix, torch.full_like(iy, -1))
    if mut == "last_row_tap_dropped":
        idx[-1, 4] = -1
    return idx


def _cols(x2, idx):
    """im2col over the table: [Mo, 9, Ci], zeros where idx is -1."""
    return torch.where((idx >= 0).unsqueeze(-1), x2[idx.clamp_min(0)], torch.zeros((), dtype=x2.dtype))


def _scatter(contrib, idx, Mi):
    """sum over (m, tap) of contrib [Mo, 9, Ci] into the rows idx names: [Mi, Ci]."""
    out = torch.zeros(Mi, contrib.shape[-1], dtype=contrib.dtype)
    ok = idx >= 0
    return out.index_add_(0, idx[ok], contrib[ok])


def gather_ref(c, x, down, up, s, dy, y0, dx0, mut=None, t_from=None, u_from=None):
    """The six outputs in float64, written out over the gather table, plus the sum of |terms| of each (abs_*). t_from / u_from: the
    t / u the later products read (a kernel's own); default: the reference's. mut: one of MUTATIONS."""
    geom, B, H, W, Ci, Co, r = c
    x2, dy2, D9, U = x.double().reshape(-1, Ci), dy.double().reshape(-1, Co), down.double().reshape(r, Ci, 9), up.double()
    table_mut = mut if mut in ("border_clamped", "halo_across_images", "up_no_bounds_test", "last_row_tap_dropped") else None
    idx = gather_table(geom, B, H, W, table_mut)
    Dt = D9.flip(-1) if mut == "taps_flipped" else D9
    cols = _cols(x2, idx)
    t = torch.einsum("mtc,jct->mj", cols, Dt)
    u = dy2 @ U
    tt = t if t_from is None else t_from.double().reshape(-1, r)
    uu = u if u_from is None else u_from.double().reshape(-1, r)
    idx_dx = idx
    if mut == "zero_insert_odd":        # Downsample's u rows land on the odd positions of the H x W grid: every read moves by (1, 1)
        assert geom == 1
        Ho, Wo = out_hw(geom, H, W)
        b, oy, ox = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), indexing="ij")
        ky, kx = torch.arange(9).reshape(1, 9) // 3, torch.arange(9).reshape(1, 9) % 3
        iy, ix = 2 * oy.reshape(-1, 1) + 1 + ky - 1, 2 * ox.reshape(-1, 1) + 1 + kx - 1
        idx_dx = torch.where((iy < H) & (ix < W), (b.reshape(-1, 1) * H + iy) * W + ix, torch.full_like(iy, -1))
    Mi = B * H * W
    y = y0.double().reshape(-1, Co) + s * (tt @ U.T)
    dx = dx0.double().reshape(-1, Ci) + s * _scatter(torch.einsum("mj,jct->mtc", uu, Dt), idx_dx, Mi)
    g_down = s * torch.einsum("mj,mtc->jct", uu, cols)
    if mut == "taps_flipped":
        g_down = g_down.flip(-1)
    g_down = g_down.reshape(r, Ci, 3, 3)
    if mut == "g_down_kykx":
        g_down = g_down.transpose(2, 3).contiguous()
    g_up = s * (dy2.T @ tt)
    Ho, Wo = out_hw(geom, H, W)
    a = abs(s)
    return dict(
        t=t.reshape(B, Ho, Wo, r), y=y.reshape(B, Ho, Wo, Co), u=u.reshape(B, Ho, Wo, r), dx=dx.reshape(B, H, W, Ci), g_down=g_down, g_up=g_up,
        abs_t=torch.einsum("mtc,jct->mj", cols.abs(), Dt.abs()).reshape(B, Ho, Wo, r),
        abs_y=(y0.double().reshape(-1, Co).abs() + a * (tt.abs() @ U.abs().T)).reshape(B, Ho, Wo, Co),
        abs_u=(dy2.abs() @ U.abs()).reshape(B, Ho, Wo, r),
        abs_dx=(dx0.double().reshape(-1, Ci).abs() + a * _scatter(torch.einsum("mj,jct->mtc", uu.abs(), Dt.abs()), idx_dx, Mi)).reshape(B, H, W, Ci),
        abs_g_down=(a * torch.einsum("mj,mtc->jct", uu.abs(), cols.abs())).reshape(r, Ci, 3, 3), abs_g_up=a * (dy2.abs().T @ tt.abs()))


def conv_ref(c, x, down, up, s, dy, y0, dx0):
    """The same six through F.conv2d on the NCHW permutation (geometry 2: after repeat_interleave x2 of both axes) and autograd."""
    geom, B, H, W, Ci, Co, r = c
    xn = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    D, U = down.double().clone().requires_grad_(True), up.double().clone().requires_grad_(True)
    src = xn.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) if geom == 2 else xn
    t = F.conv2d(src, D, stride=2 if geom == 1 else 1, padding=1)                    # [B, r, Ho, Wo]
    term = s * F.conv2d(t, U.reshape(Co, r, 1, 1))
    term.backward(dy.double().permute(0, 3, 1, 2))
    rows = lambda v: v.detach().permute(0, 2, 3, 1).contiguous()
    return dict(t=rows(t), y=y0.double() + rows(term), u=dy.double() @ up.double(), dx=dx0.double() + rows(xn.grad), g_down=D.grad, g_up=U.grad)


# ---- bounds
def chains(c):
    geom, B, H, W, Ci, Co, r = c
    Ho, Wo = out_hw(geom, H, W)
    Mo = B * Ho * Wo
    chunk = wgrad_chunk_rows(Mo)
    wchain = chunk // 2 + 1 + (-(-Mo // chunk) - 1) + 1
    return dict(t=9 * Ci // 2 + 1, y=r + 1, u=Co // 2 + 1, dx=(36 if geom == 2 else 9) * 4 * -(-r // 4) + 1, g_down=wchain, g_up=wchain)


def bounds(c, ref):
    """Per-element bounds of the six outputs from a gather_ref result (its abs_* sums)."""
    return {n: P.tree_bound(L, ref["abs_" + n]) for n, L in chains(c).items()}


def end_to_end_bounds(c, ref, up, down, s, dy, x):
    """Bounds against float64 all the way: a product's own bound plus what the bound of the t / u it reads lets through."""
    geom, B, H, W, Ci, Co, r = c
    b = bounds(c, ref)
    a = abs(s)
    bt, bu = b["t"].reshape(-1, r), b["u"].reshape(-1, r)
    idx = gather_table(geom, B, H, W)
    D9 = down.double().reshape(r, Ci, 9).abs()
    cols = _cols(x.double().reshape(-1, Ci), idx).abs()
    return dict(
        t=b["t"], u=b["u"], y=b["y"] + (a * (bt @ up.double().abs().T)).reshape(b["y"].shape),
        dx=b["dx"] + (a * _scatter(torch.einsum("mj,jct->mtc", bu, D9), idx, B * H * W)).reshape(b["dx"].shape),
        g_down=b["g_down"] + (a * torch.einsum("mj,mtc->jct", bu, cols)).reshape(r, Ci, 3, 3),
        g_up=b["g_up"] + a * (dy.double().reshape(-1, Co).abs().T @ bt))


# ---- inputs
def gaussian_case(c, seed=0):
    geom, B, H, W, Ci, Co, r = c
    Ho, Wo = out_hw(geom, H, W)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * (B * H * W) + 31 * Ci + 17 * Co + 5 * r + geom)
    x, dy = torch.randn(B, H, W, Ci, generator=g), torch.randn(B, Ho, Wo, Co, generator=g)
    down, up = torch.randn(r, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5, torch.randn(Co, r, generator=g) * r ** -0.5
    return x, dy, down, up, torch.randn(B, Ho, Wo, Co, generator=g), torch.randn(B, H, W, Ci, generator=g)


def integer_case(c):
    """Small integers and a down whose nine taps all differ and are not symmetric in (ky, kx): every term sum of the six outputs stays
    below 2^24 (checked by the caller on the abs_* sums), so fp32 is exact in any order and a wrong lane map, tap order or OIHW write
    shows as a bit that differs."""
    geom, B, H, W, Ci, Co, r = c
    Ho, Wo = out_hw(geom, H, W)
    g = torch.Generator().manual_seed(B * H * W + Ci + Co + r + geom)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    x, dy = ri(-2, 2, B, H, W, Ci), ri(-2, 2, B, Ho, Wo, Co)
    j, ci = torch.arange(r).reshape(r, 1, 1, 1), torch.arange(Ci).reshape(1, Ci, 1, 1)
    ky, kx = torch.arange(3).reshape(1, 1, 3, 1), torch.arange(3).reshape(1, 1, 1, 3)
    down = (((3 * j + 5 * ci + (j * ci) % 3 + 3 * ky + kx) % 11) - 5).float()       # the tap moves the residue: nine different slices
    taps = down.reshape(r, Ci, 9)
    assert all(not torch.equal(taps[..., a], taps[..., b]) for a in range(9) for b in range(a)) and not torch.equal(down, down.transpose(2, 3))
    n = torch.arange(Co).reshape(Co, 1)
    up = (((2 * n + 7 * torch.arange(r).reshape(1, r) + n // 16) % 3) - 1).float()
    return x, dy, down, up, ri(-3, 3, B, Ho, Wo, Co), ri(-3, 3, B, H, W, Ci)


# ---- running a case on the device
NAMES = ("t", "y", "u", "dx", "g_down", "g_up")


def run_lora_conv3(engine, c, s=0.75, exact=False):
    """(rows, problems) as train_prims_ref's run_*: rows = [(case, tensor, worst error / bound, 1.0)], every product against float64
    on the device's own t / u, then (tensor + "(e2e)") against float64 all the way; with exact (integer inputs, s a power of two) a
    row's error is the number of elements that differ from float64 and its bound 0."""
    geom, B, H, W, Ci, Co, r = c
    x, dy, down, up, y0, dx0 = integer_case(c) if exact else gaussian_case(c)
    if exact:
        s = 0.5
    Ho, Wo = out_hw(geom, H, W)
    shapes = {"t": (B, Ho, Wo, r), "y": (B, Ho, Wo, Co), "u": (B, Ho, Wo, r), "dx": (B, H, W, Ci), "g_down": (r, Ci, 3, 3), "g_up": (Co, r)}
    call = lambda out: engine.op_lora_conv3(x, down, up, scale=s, geom=geom, dy=dy, out=out)
    got, problems = P._twice(call, shapes, init={"y": y0, "dx": dx0}, device=engine.device)
    cid = case_id(c) + ("-int" if exact else "")
    full = gather_ref(c, x, down, up, s, dy, y0, dx0)
    rows = []
    if exact:
        assert all(float(full["abs_" + n].max()) < 2 ** 24 for n in NAMES), cid
        rows = [(cid, n, float((got[n].double() != full[n]).sum()), 0.0) for n in NAMES]
    else:
        own = gather_ref(c, x, down, up, s, dy, y0, dx0, t_from=got["t"], u_from=got["u"])
        b_own, b_full = bounds(c, own), end_to_end_bounds(c, full, up, down, s, dy, x)
        rows = [P._reduction_row(cid, n, got[n], own[n], b_own[n]) for n in NAMES]
        rows += [P._reduction_row(cid, n + "(e2e)", got[n], full[n], b_full[n]) for n in ("y", "dx", "g_down", "g_up")]
    return rows, [f"{cid} {p}" for p in problems]
