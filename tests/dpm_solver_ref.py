"""float64 restatements the DPM-Solver++ / stochastic-DDIM tests compare against. Nothing here imports the product's coefficient
function or grids: the loops are written from the formulas of the samplers' contract,

    alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log(alpha / sigma), step s -> t, h = lambda_t - lambda_s,
    D0 = (x - sigma_s e) / alpha_s
    order 1:  x_t = (sigma_t / sigma_s) x - alpha_t (e^{-h} - 1) D0
    order 2:  the same with D = (1 + 1/(2r)) D0 - (1/(2r)) D1,  r = (lambda_s - lambda_{s_prev}) / h
    step 0 is order 1; with lower_order_final and fewer than 10 steps so is the last one

and, for DDIM with eta > 0, from the reference's p_sample_ddim (ldm/models/diffusion/ddim.py:111-134). The loops drive an
eps_fn(x, t, cond, scale) callable, the protocol of oracle.gligen_oracle.plms_sample (tests/test_oracle_golden.py).

Also here: the Gaussian toy problem with its closed-form probability-flow solution, and toy_table(), which regenerates the table of
DESIGN.md §4 (python tests/dpm_solver_ref.py prints it).
"""
import math

import numpy as np
import torch


def lam(abar):
    abar = np.asarray(abar, dtype=np.float64)
    return 0.5 * (np.log(abar) - np.log1p(-abar))


def sd_alphas_cumprod(linear_start=0.00085, linear_end=0.012, timesteps=1000):
    betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


# --------------------------------------------------------------------------- grids: (timesteps, a_t, a_prev) in sampling order
def uniform_grid(S, ac):
    """make_ddim_timesteps('uniform') + make_ddim_sampling_parameters (reference util.py:55-83), flipped to sampling order."""
    T = len(ac)
    ts = np.arange(0, T, T // S) + 1
    a_t = ac[ts]
    a_prev = np.concatenate([[ac[0]], ac[ts[:-1]]])
    return ts[::-1].copy(), a_t[::-1].copy(), a_prev[::-1].copy()


def logsnr_nodes(S, ac):
    l = lam(ac)
    return np.array([int(np.argmin(np.abs(l - v))) for v in np.linspace(l[-1], l[0], S + 1)], dtype=np.int64)


def logsnr_grid(S, ac):
    nodes = logsnr_nodes(S, ac)
    return nodes[:-1].copy(), ac[nodes[:-1]], ac[nodes[1:]]


def continuous_logsnr_grid(S, lam_lo=-3.5, lam_hi=3.5):
    """abar at S + 1 nodes uniform in lambda: abar = sigmoid(2 lambda)."""
    a = 1.0 / (1.0 + np.exp(-2.0 * np.linspace(lam_lo, lam_hi, S + 1)))
    return a[:-1], a[1:]


# --------------------------------------------------------------------------- the solver step, from the formulas
def step_orders(S, order, lower_order_final):
    return [1 if (i == 0 or order == 1 or (lower_order_final and S < 10 and i == S - 1)) else 2 for i in range(S)]


def two_m_step(x, d0, d1, a_s, a_t, a_sprev, order):
    l_s, l_t = float(lam(a_s)), float(lam(a_t))
    h = l_t - l_s
    d = d0
    if order == 2:
        r = (l_s - float(lam(a_sprev))) / h
        d = (1.0 + 1.0 / (2.0 * r)) * d0 - (1.0 / (2.0 * r)) * d1
    return math.sqrt(1.0 - a_t) / math.sqrt(1.0 - a_s) * x - math.sqrt(a_t) * math.expm1(-h) * d


def _guided(eps_fn, x, ts, scale, guidance_scale):
    e = eps_fn(x, ts, True, scale)
    if guidance_scale != 1:
        eu = eps_fn(x, ts, False, scale)
        e = eu + guidance_scale * (e - eu)
    return e


def _blend(x, i, step, sched, mask, x0, noise):
    if mask is None:
        return x
    sa = float(sched["sqrt_alphas_cumprod"][int(step)])
    s1 = float(sched["sqrt_one_minus_alphas_cumprod"][int(step)])
    return (sa * x0.double() + s1 * noise[i].double()) * mask.double() + (1.0 - mask.double()) * x


def dpm_sample(eps_fn, x, grid, sched, guidance_scale, order=2, lower_order_final=True, alphas=None, mask=None, x0=None, noise=None,
               on_gate_off=None):
    """DPM-Solver++ (2M) in float64 around eps_fn. grid = (timesteps, a_t, a_prev) in sampling order; alphas / mask / x0 / noise /
    on_gate_off as oracle.gligen_oracle.plms_sample."""
    timesteps, a_t, a_prev = grid
    S = len(timesteps)
    orders = step_orders(S, order, lower_order_final)
    x = x.double()
    b = x.shape[0]
    d1 = None
    for i, step in enumerate(timesteps):
        scale = 1.0 if alphas is None else float(alphas[i])
        if alphas is not None and alphas[i] == 0 and on_gate_off is not None:
            on_gate_off()
        ts = torch.full((b,), int(step), dtype=torch.long)
        x = _blend(x, i, step, sched, mask, x0, noise)
        e = _guided(eps_fn, x, ts, scale, guidance_scale).double()
        d0 = (x - math.sqrt(1.0 - float(a_t[i])) * e) / math.sqrt(float(a_t[i]))
        x = two_m_step(x, d0, d1, float(a_t[i]), float(a_prev[i]), float(a_t[i - 1]) if i else None, orders[i])
        d1 = d0
    return x


def ddim_eta_sigmas(a_t, a_prev, eta):
    a_t, a_prev = np.asarray(a_t, dtype=np.float64), np.asarray(a_prev, dtype=np.float64)
    return eta * np.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev))                  # reference util.py:77


def ddim_eta_sample(eps_fn, x, grid, sigmas, z, sched, guidance_scale, alphas=None, mask=None, x0=None, noise=None, on_gate_off=None):
    """The reference's ddim_sampling + p_sample_ddim (ddim.py:65-134) in float64 with sigma_t = sigmas[i] and z[i] for its randn_like(x)."""
    timesteps, a_t, a_prev = grid
    x = x.double()
    b = x.shape[0]
    for i, step in enumerate(timesteps):
        scale = 1.0 if alphas is None else float(alphas[i])
        if alphas is not None and alphas[i] == 0 and on_gate_off is not None:
            on_gate_off()
        ts = torch.full((b,), int(step), dtype=torch.long)
        x = _blend(x, i, step, sched, mask, x0, noise)
        e = _guided(eps_fn, x, ts, scale, guidance_scale).double()
        at, ap, sg = float(a_t[i]), float(a_prev[i]), float(sigmas[i])
        pred_x0 = (x - math.sqrt(1.0 - at) * e) / math.sqrt(at)
        x = math.sqrt(ap) * pred_x0 + math.sqrt(1.0 - ap - sg ** 2) * e + sg * z[i].double()
    return x


# --------------------------------------------------------------------------- Gaussian toy problem
TOY_C2 = 0.25     # data ~ N(0, c^2 I)


def toy_eps(x, abar, c2=TOY_C2):
    """The exact noise prediction E[eps | x_t] for Gaussian data: x_t ~ N(0, abar c^2 + 1 - abar)."""
    return math.sqrt(1.0 - abar) * x / (abar * c2 + 1.0 - abar)


def toy_exact(x_T, abar_T, abar, c2=TOY_C2):
    """The probability-flow ODE's solution through x_T."""
    return x_T * math.sqrt(abar * c2 + 1.0 - abar) / math.sqrt(abar_T * c2 + 1.0 - abar_T)


def toy_x_T(n=4096, seed=0):
    return np.random.default_rng(seed).standard_normal(n)


def toy_rel_rms(step_fn, a_t, a_prev, x_T=None):
    """Relative RMS error, against the exact solution, of running x <- step_fn(i, x, e) over the grid with the exact noise prediction."""
    x_T = toy_x_T() if x_T is None else x_T
    x = x_T.copy()
    for i in range(len(a_t)):
        x = step_fn(i, x, toy_eps(x, float(a_t[i])))
    ref = toy_exact(x_T, float(a_t[0]), float(a_prev[-1]))
    return float(np.sqrt(np.mean((x - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def toy_error_ref(a_t, a_prev, order, lower_order_final=True):
    """toy_rel_rms of this module's own solver step (order 1 = DDIM with eta 0)."""
    S = len(a_t)
    orders = step_orders(S, order, lower_order_final)
    hist = {}

    def step(i, x, e):
        d0 = (x - math.sqrt(1.0 - a_t[i]) * e) / math.sqrt(a_t[i])
        hist[i] = d0
        return two_m_step(x, d0, hist.get(i - 1), float(a_t[i]), float(a_prev[i]), float(a_t[i - 1]) if i else None, orders[i])
    return toy_rel_rms(step, a_t, a_prev)


def toy_table():
    """The rows of DESIGN.md §4: (label, steps, relative RMS error) on the SD schedule, and the 32 -> 64 error ratios by order."""
    ac = sd_alphas_cumprod()
    rows = []
    for label, grid, S, order in (("DDIM, uniform timestep grid", uniform_grid, 50, 1), ("2M, uniform grid", uniform_grid, 20, 2),
                                  ("2M, integer timesteps nearest to a log-SNR-uniform grid", logsnr_grid, 20, 2),
                                  ("2M, integer timesteps nearest to a log-SNR-uniform grid", logsnr_grid, 10, 2)):
        _, a_t, a_prev = grid(S, ac)
        rows.append((label, S, toy_error_ref(a_t, a_prev, order)))
    ratios = {}
    for order in (1, 2):
        e32, e64 = (toy_error_ref(*continuous_logsnr_grid(S), order, lower_order_final=False) for S in (32, 64))
        ratios[order] = e32 / e64
    return rows, ratios


if __name__ == "__main__":
    rows, ratios = toy_table()
    for label, S, err in rows:
        print(f"| {label} | {S} | {err:.4f} |")
    for order, r in ratios.items():
        print(f"| order {order} | {r:.2f} |")
