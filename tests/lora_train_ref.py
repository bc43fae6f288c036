"""References, cases and the measuring code of the LoRA-training tests (test_lora_train_cpu.py holds the float64 restatement to
autograd; test_lora_train_gpu.py runs the kernels of csrc/train_lora.hip against it through Engine.op_lora_linear,
include/gligen_amd_train_lora.h, and the training step against autograd through the CPU oracle on the merged weights).

The adapted Linear: y = x W^T + s (x down^T) up^T, W [N, K], down [r, K], up [N, r], s = alpha / r. With dW = dy^T x the gradient
of the merged weight W + s up down, the chain rule gives g_up = s dW down^T and g_down = s up^T dW.

Error bounds: every element of a kernel's output is a sum formed by a chain of fp32 additions; its bound is
train_prims_ref.tree_bound(chain, sum of |terms|), chain being the kernel's longest addition chain, written down from the code of
csrc/train_lora.hip:
  lora_down_kernel    T = X A^T over a contraction of length L (K forward, N for u = dy up): two accumulators of L / 2 fused
                      multiply-adds each and their sum -- L / 2 + 1 <= L additions.
  lora_up_kernel      Y += s T B: r fused multiply-adds (the padding up to a multiple of 4 adds exact zeros), then fmaf(s, sum, y): r + 1.
  lora_wgrad_kernel + lora_wgrad_reduce_kernel   G = s T^T Z: per chunk of `chunk` rows two accumulators of chunk / 2 and their sum,
                      then the partials in ascending order and the product with s: chunk + partials covers it.
The products that read a kernel's own output (y reads t, dx and g_down read u, g_up reads t) are held to float64 on the t / u the
kernel produced, as the column sums of test_train_prims are: each kernel is then measured by itself. No constant in this file was
obtained by running a kernel."""
import math

import torch

import train_prims_ref as P

# ---- the cases the issue sets
M_PLAIN = [1, 63, 154, 272]
KN = [(64, 64), (320, 320), (768, 320), (320, 2560), (1280, 320)]
RANKS = [1, 4, 24, 128]
ORIENTATIONS = [(False, False), (False, True), (True, False), (True, True)]      # (down given as [K, r], up given as [r, N])
KROWS = 64              # rows a workgroup stages at a time (train_lora.hip: kRows)


def wgrad_chunk_rows(M):
    """train_lora.hip lora_wgrad_chunk_rows: at most 32 partial sums, chunks of whole 64-row stages, never below 256 rows."""
    per = -(-(-(-M // 32)) // KROWS) * KROWS
    return max(per, 256)


CHUNK = wgrad_chunk_rows(1)                                     # 256 for every M <= 8192
M_CHUNK = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17]         # one below, at, one above, 2x + 17 of the weight gradient's row chunk
assert all(wgrad_chunk_rows(m) == CHUNK for m in M_PLAIN + M_CHUNK)
M_ALL = M_PLAIN + M_CHUNK


def kernel_cases(kn_index):
    """Every M against one (K, N), the rank and the orientation pair walking through all of theirs; over the five (K, N) every M
    meets every rank and every orientation pair."""
    K, N = KN[kn_index]
    return [(M, K, N, RANKS[(i + kn_index) % 4], *ORIENTATIONS[(i // 4 + i + 3 * kn_index) % 4]) for i, M in enumerate(M_ALL)]


def cross_cases():
    """Every rank against every orientation pair at one shape with a ragged row edge."""
    return [(154, 320, 320, r, dkr, urn) for r in RANKS for dkr, urn in ORIENTATIONS]


# ---- float64
def adapted_linear_ref(x, W, down, up, s, dy):
    """Forward, dx, g_down, g_up of y = x W^T + s (x down^T) up^T in float64, written out (no autograd)."""
    x, W, down, up, dy = (t.double() for t in (x, W, down, up, dy))
    t = x @ down.T
    y = x @ W.T + s * (t @ up.T)
    u = dy @ up
    dx = dy @ W + s * (u @ down)
    return dict(t=t, y=y, u=u, dx=dx, g_down=s * (u.T @ x), g_up=s * (dy.T @ t))


def adapted_linear_autograd(x, W, down, up, s, dy):
    """The same through autograd on the merged weight W + s up down, the adapter gradients by the chain rule from dW."""
    x = x.double().clone().requires_grad_(True)
    Weff = (W.double() + s * (up.double() @ down.double())).requires_grad_(True)
    y = x @ Weff.T
    y.backward(dy.double())
    dW = Weff.grad
    return dict(y=y.detach(), dx=x.grad, g_up=s * (dW @ down.double().T), g_down=s * (up.double().T @ dW))


def chain_rule(dW, down, up, s):
    """(g_down, g_up) of an adapter from the gradient of the merged weight, float64; dW [N, K(, 1, 1)]."""
    dW = dW.double().reshape(dW.shape[0], -1)
    return s * (up.double().T @ dW), s * (dW @ down.double().T)


# ---- inputs
def gaussian_case(M, K, N, r, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * K + 17 * N + r)
    x, dy = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    down, up = torch.randn(r, K, generator=g) * K ** -0.5, torch.randn(N, r, generator=g) * r ** -0.5
    y0, dx0 = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    return x, dy, down, up, y0, dx0


def integer_case(M, K, N, r):
    """Small integers, an asymmetric small operand: every product and every sum of the six outputs is an integer below 2^24 (the
    largest, a weight gradient's, is at most M * 2 * 2 * max(K, N) * 2), so fp32 is exact in any order and a wrong lane map, a
    transposed write or a dropped row shows as a bit that differs."""
    assert M * 8 * max(K, N) < 2 ** 24 and r * 4 * max(K, N) * 2 < 2 ** 24
    g = torch.Generator().manual_seed(M + K + N + r)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    x, dy = ri(-2, 2, M, K), ri(-2, 2, M, N)
    jj, kk = torch.arange(r).reshape(r, 1), torch.arange(K).reshape(1, K)
    down = (((3 * jj + 5 * kk + (jj * kk) % 3) % 5) - 2).float()           # down[j][k] != down[k][j], no period of 16 or 4
    nn = torch.arange(N).reshape(N, 1)
    up = (((2 * nn + 7 * torch.arange(r).reshape(1, r) + nn // 16) % 3) - 1).float()
    return x, dy, down, up, ri(-3, 3, M, N), ri(-3, 3, M, K)


# ---- running a case on the device
def run_lora_linear(engine, M, K, N, r, down_kr, up_rn, s=0.75, exact=False):
    """(rows, problems) as train_prims_ref's run_*: rows = [(case, tensor, worst error / bound, 1.0)]; with exact (integer inputs, s a
    power of two) a row's error is the number of elements that differ from float64 and its bound 0."""
    x, dy, down, up, y0, dx0 = integer_case(M, K, N, r) if exact else gaussian_case(M, K, N, r)
    if exact:
        s = 0.5
    dn = down.T.contiguous() if down_kr else down
    upp = up.T.contiguous() if up_rn else up
    shapes = {"t": (M, r), "y": (M, N), "u": (M, r), "dx": (M, K), "g_down": tuple(dn.shape), "g_up": tuple(upp.shape)}
    call = lambda out: engine.op_lora_linear(x, dn, upp, scale=s, dy=dy, down_kr=down_kr, up_rn=up_rn, out=out)
    got, problems = P._twice(call, shapes, init={"y": y0, "dx": dx0}, device=engine.device)
    if down_kr:
        got["g_down"] = got["g_down"].T
    if up_rn:
        got["g_up"] = got["g_up"].T
    X, DY, D, U = x.double(), dy.double(), down.double(), up.double()
    tg, ug = got["t"].double(), got["u"].double()
    chunk = wgrad_chunk_rows(M)
    wchain = chunk + -(-M // chunk)
    ref = {
        "t": (X @ D.T, P.tree_bound(K, X.abs() @ D.abs().T)),
        "y": (y0.double() + s * (tg @ U.T), P.tree_bound(r + 1, y0.double().abs() + abs(s) * (tg.abs() @ U.abs().T))),
        "u": (DY @ U, P.tree_bound(N, DY.abs() @ U.abs())),
        "dx": (dx0.double() + s * (ug @ D), P.tree_bound(r + 1, dx0.double().abs() + abs(s) * (ug.abs() @ D.abs()))),
        "g_down": (s * (ug.T @ X), P.tree_bound(wchain, abs(s) * (ug.abs().T @ X.abs()))),
        "g_up": (s * (DY.T @ tg), P.tree_bound(wchain, abs(s) * (DY.abs().T @ tg.abs()))),
    }
    cid = f"M{M}-K{K}-N{N}-r{r}-d{int(down_kr)}u{int(up_rn)}" + ("-int" if exact else "")
    rows = []
    for name, (want, bound) in ref.items():
        if exact:
            rows.append((cid, name, float((got[name].double() != want).sum()), 0.0))
        else:
            rows.append(P._reduction_row(cid, name, got[name], want, bound))
    return rows, [f"{cid} {p}" for p in problems]


def rel_mse(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float(((a - ref) ** 2).mean() / (ref ** 2).mean().clamp_min(1e-300))
