"""Restatements and error bounds for the gradient unit of a training run (csrc/train_run.hip, include/gligen_amd_train_run.h): the
accumulation in torch fp32 in the kernel's operation order, the summation chain of grad_sqnorm_kernel emulated in fp32 and its error
bound derived from that chain, the clipping coefficient, the weighted loss in float64, min-SNR on the reference's schedule, and a
float64 AdamW that carries an elementwise bound of the fp32 op chain next to every value. Nothing here is fitted to what a kernel
returns: every bound is a sum of roundings counted off the code."""
import math

import torch

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
U64 = 2.0 ** -53
TINY = 2.0 ** -126          # a square below this may be flushed or lose bits: at most this much absolute error per term
N_LIST = [1, 3, 4, 5, 1027, 100003, 2 * 16384 * 256 * 4 + 7]      # the fused optimizer tests' list: tails, > 1 block, two grid-strides + 7
GRID = (16384, 64, 6, 4)    # grad_sqnorm_kernel: elements per partial, squares per thread chain, wave levels, waves (Engine.GRAD_NORM_GRID)
BLOCK = 256


def f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


# ---- accumulation
def accumulate_ref(gs):
    """first / middle / last over K gradients in torch fp32, the kernel's order: ((g1 + g2) + g3 ...) * fl(1 / K), every sum and the
    product rounded on its own (torch's fp32 ops are)."""
    K = len(gs)
    inv_k = torch.tensor(1.0 / K, dtype=torch.float32, device=gs[0].device)      # (float)(1.0 / K), formed in double
    acc = gs[0].clone()
    for g in gs[1:]:
        acc = acc + g
    return acc * inv_k


# ---- the norm
def partial_count(n, grid=GRID):
    return (n + grid[0] - 1) // grid[0]


def emulate_sqnorm_partials(g, grid=GRID):
    """grad_sqnorm_kernel's partial sums in torch fp32 on the CPU, operation by operation: thread t of the 256 owns the float4 groups
    t, t + 256, ... of its chunk and chains their squares x y z w in that order; a wave's 64 chains meet in a 6-level butterfly
    (lane ^ 32, ^ 16, ... ^ 1); the four wave sums are added in index order. Elements past n add nothing."""
    chunk, chain, depth, waves = grid
    assert chunk == BLOCK * chain and waves * 64 == BLOCK and 2 ** depth == 64
    g = g.detach().float().cpu().reshape(-1)
    count = partial_count(g.numel(), grid)
    x = torch.zeros(count * chunk, dtype=torch.float32)
    x[:g.numel()] = g
    x = x.view(count, chain // 4, BLOCK, 4)               # [chunk][j][thread][q]
    s = torch.zeros(count, BLOCK, dtype=torch.float32)
    for j in range(chain // 4):
        for q in range(4):
            v = x[:, j, :, q]
            s = s + v * v                                 # the square rounded, then the sum
    s = s.view(count, waves, 64)
    lane = torch.arange(64)
    off = 32
    while off >= 1:
        s = s + s[:, :, lane ^ off]
        off //= 2
    r = s[:, 0, 0]
    for w in range(1, waves):
        r = r + s[:, w, 0]
    return r


def sqnorm_sum_rel_bound(count, grid=GRID):
    """|S_hat - S| <= this * S for the sum of squares S (all terms >= 0, so every rounding acts on a partial sum <= S): a term meets
    the rounding of its square, at most chain - 1 roundings in its thread's chain (the first sum, 0 + q, is exact), `depth` in the wave
    butterfly and waves - 1 across the waves -- k = chain + depth + waves - 1 fp32 roundings, gamma_k = k u / (1 - k u) -- and then
    at most `count` double roundings in the sum of the partials (their conversion to double is exact)."""
    _, chain, depth, waves = grid
    k = chain + depth + waves - 1
    gk = k * U32 / (1.0 - k * U32)
    gd = count * U64 / (1.0 - count * U64)
    return (1.0 + gk) * (1.0 + gd) - 1.0


def norm_bound(norm64, n, grid=GRID, count=None):
    """|(float)sqrt(S_hat) - norm64| <= this. With S_hat = S (1 + theta), |theta| <= T: |sqrt(1 + theta) - 1| <= T / (2 - T); the
    double sqrt and the conversion to fp32 add one rounding each. Squares below 2^-126 contribute at most n 2^-126 to S absolutely,
    sqrt(n) 2^-63 to the norm (sqrt(S + e) - sqrt(S) <= sqrt(e))."""
    T = sqnorm_sum_rel_bound(partial_count(n, grid) if count is None else count, grid)     # (count: several ranges side by side)
    rel = (1.0 + T / (2.0 - T)) * (1.0 + U64) * (1.0 + U32) - 1.0
    return rel * norm64 + (1.0 + rel) * math.sqrt(n * TINY)


def coef_ref(norm64, max_norm):
    return min(1.0, max_norm / (norm64 + 1e-6))


def coef_bound(norm64, n, max_norm, grid=GRID, count=None):
    """|coef - min(1, max_norm / (norm64 + 1e-6))| <= this: the denominator fl(norm_hat + 1e-6f) carries the norm's error, the
    rounding of the constant 1e-6f (below u times the denominator) and the rounding of the sum; the quotient one more rounding --
    the norm's bound plus two fp32 roundings (and the constant's); min(1, .) does not expand a difference. max_norm is an fp32 number."""
    den = norm64 + 1e-6
    D = norm_bound(norm64, n, grid, count) / den + U32
    rel = (1.0 + U32) / ((1.0 - D) * (1.0 - U32)) - 1.0
    return rel * (max_norm / den)


# ---- the weighted loss
def weighted_loss_ref(eps, noise, w):
    """(loss, d loss / d eps) of (w[:, None, None, None] * (eps - noise) ** 2).mean() restated in float64."""
    e, t, w = eps.double(), noise.double(), w.double()
    d = e - t
    n = d.numel()
    wb = w.reshape(-1, *([1] * (d.dim() - 1)))
    return (wb * d * d).sum() / n, 2.0 * wb * d / n


def reference_alphas_cumprod():
    """The reference's schedule (ldm.py / ddpm.py: beta_schedule "linear", 0.00085 -> 0.012, 1000 steps: linear in sqrt(beta)), float64."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def min_snr_ref(ac, gamma):
    snr = ac.double() / (1.0 - ac.double())
    return torch.minimum(snr, torch.full_like(snr, gamma)) / snr


def oracle_autograd_weighted(sd, cfg, kind, trainable, d, x, extra, weights):
    """tests/test_train_inpaint_cpu.py's oracle_autograd with the weighted loss: one forward through the CPU oracle, then for every
    entry w of `weights` (a tensor [B], or None for mse_loss) the loss (w[:, None, None, None] * (eps - noise) ** 2).mean() and its
    gradient for every `trainable` tensor by autograd. Returns (eps, [(loss, grads), ...])."""
    from helpers import grounding_kwargs, oracle_cfg
    from oracle import gligen_oracle as orc
    sdo = {k: v.detach().float().cpu().clone() for k, v in sd.items()}
    for k in trainable:
        sdo[k].requires_grad_(True)
    inp = dict(x=x, timesteps=d["t"].long(), context=d["context"], grounding_input=grounding_kwargs(kind, d["b"]), inpainting_extra_input=extra)
    eps = orc.unet_forward(sdo, oracle_cfg(cfg, kind), inp)
    out = []
    for i, w in enumerate(weights):
        if w is None:
            loss = torch.nn.functional.mse_loss(eps, d["noise"])
        else:
            loss = (w.float().cpu()[:, None, None, None] * (eps - d["noise"]) ** 2).mean()
        gs = torch.autograd.grad(loss, [sdo[k] for k in trainable], retain_graph=i + 1 < len(weights))
        out.append((loss.detach(), dict(zip(trainable, gs))))
    return eps.detach(), out


# ---- AdamW in float64 with the elementwise bound of the fp32 op chain
def adamw_scalars32(lr, betas, eps, wd, step):
    """adamw_update.h: every scalar formed in double and rounded to fp32 once; returned as Python floats holding the fp32 values."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return dict(b1=f32(b1), omb1=f32(1.0 - b1), b2=f32(b2), omb2=f32(1.0 - b2), eps=f32(eps), decay=f32(1.0 - lr * wd), step_size=f32(lr / bc1),
                bc2_sqrt=f32(math.sqrt(bc2)))


class Adam64:
    """p, m, v in float64 from fp32 starting values, and next to each a tensor E* with |fp32 kernel's value - float64 value| <= E*,
    propagated through adamw_update's operations: every fp32 product, sum, sqrt and quotient adds u times the magnitude of its result
    (sqrtf and the division are correctly rounded on gfx950 without fast-math), and the errors of its operands pass through its
    derivative -- through sqrt as sqrt(v + Ev) - sqrt(max(v - Ev, 0)), which stays finite at v = 0. Where the bound of the denominator
    reaches the denominator itself the quotient's bound is infinite (counted in `unbounded`)."""

    def __init__(self, p):
        self.p = p.double().clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.Ep, self.Em, self.Ev = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.unbounded = 0

    def step(self, g, Eg, k):
        u = U32 * (1.0 + 2 * U32)
        g, ag = g.double(), g.double().abs()
        m_old, v_old = self.m, self.v
        m = k["b1"] * m_old + k["omb1"] * g
        Em = k["b1"] * self.Em + k["omb1"] * Eg + u * (k["b1"] * (m_old.abs() + self.Em) + k["omb1"] * (ag + Eg) + m.abs() + k["b1"] * self.Em + k["omb1"] * Eg)
        g2, Eg2 = g * g, 2 * ag * Eg + Eg * Eg
        v = k["b2"] * v_old + k["omb2"] * g2
        Ev = k["b2"] * self.Ev + k["omb2"] * Eg2 + u * (k["b2"] * (v_old + self.Ev) + 2 * k["omb2"] * (g2 + Eg2) + v + k["b2"] * self.Ev + k["omb2"] * Eg2)
        root = v.sqrt()
        Eroot = (v + Ev).sqrt() - (v - Ev).clamp_min(0.0).sqrt() + u * (root + Ev.sqrt())
        denom = root / k["bc2_sqrt"] + k["eps"]
        Ed = Eroot / k["bc2_sqrt"] + u * ((root + Eroot) / k["bc2_sqrt"] + denom + Eroot / k["bc2_sqrt"])
        q = m / denom
        room = denom - Ed
        bad = room <= 0
        self.unbounded += int(bad.sum())
        Eq = torch.where(bad, torch.full_like(q, float("inf")), (Em + q.abs() * Ed) / room.clamp_min(1e-300))
        Eq = Eq + u * (q.abs() + Eq)
        upd = k["step_size"] * q
        Eu = k["step_size"] * Eq + u * (upd.abs() + k["step_size"] * Eq)
        pd = self.p * k["decay"]
        Epd = k["decay"] * self.Ep + u * (pd.abs() + k["decay"] * self.Ep)
        p = pd - upd
        Ep = Epd + Eu + u * (p.abs() + Epd + Eu)
        self.p, self.m, self.v, self.Ep, self.Em, self.Ev = p, m, v, Ep, Em, Ev
