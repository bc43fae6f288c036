"""DPM-Solver++ (2M) and stochastic DDIM on the host, no GPU: the coefficient function against DDIM and against the order it claims,
the log-SNR grid, the samplers' host loops against the float64 restatements of tests/dpm_solver_ref.py, and the C ABI of the solver loop."""
import ctypes as C
import math
import os
import shutil
import subprocess
from functools import partial

import numpy as np
import pytest
import torch

import dpm_solver_ref as ref
from helpers import ROOT
from gligen_amd import synthetic as syn
from ldm.models.diffusion.dpm_solver import DPMSolverSampler, dpm_solver_coefficients, make_logsnr_timesteps

AC = ref.sd_alphas_cumprod()


def _toy_error(a_t, a_prev, order, lower_order_final=True):
    """The toy problem solved with the PRODUCT's coefficients: x <- cx x + c0 D0 + c1 D1."""
    cf = dpm_solver_coefficients(a_t, a_prev, order=order, lower_order_final=lower_order_final)
    hist = {}

    def step(i, x, e):
        hist[i] = (x - math.sqrt(1.0 - a_t[i]) * e) / math.sqrt(a_t[i])
        return cf[i, 0] * x + cf[i, 1] * hist[i] + (cf[i, 2] * hist[i - 1] if i else 0.0)
    return ref.toy_rel_rms(step, a_t, a_prev)


@pytest.mark.parametrize("S", [4, 20, 50])
def test_order_one_is_ddim(S):
    _, a_t, a_prev = ref.uniform_grid(S, AC)
    cf = dpm_solver_coefficients(a_t, a_prev, order=1)
    assert cf.dtype == np.float64 and cf.shape == (len(a_t), 3) and not cf[:, 2].any()
    rng = np.random.default_rng(S)
    for i in range(len(a_t)):
        x, e = rng.standard_normal(64), rng.standard_normal(64)
        d0 = (x - math.sqrt(1.0 - a_t[i]) * e) / math.sqrt(a_t[i])
        ddim = math.sqrt(a_prev[i]) * d0 + math.sqrt(1.0 - a_prev[i]) * e
        got = cf[i, 0] * x + cf[i, 1] * d0
        assert np.abs(got - ddim).max() <= 1e-12 * np.abs(ddim).max(), (S, i)
    # the order-2 table: step 0 is order 1, and with fewer than 10 steps so is the last one
    cf2 = dpm_solver_coefficients(a_t, a_prev, order=2)
    assert cf2[0, 2] == 0 and np.array_equal(cf2[0], cf[0]) and (cf2[1:-1, 2] != 0).all()
    assert (cf2[-1, 2] == 0) == (len(a_t) < 10)
    assert dpm_solver_coefficients(a_t, a_prev, order=2, lower_order_final=False)[-1, 2] != 0
    for bad in (0, 3, "2"):
        with pytest.raises(ValueError, match="order"):
            dpm_solver_coefficients(a_t, a_prev, order=bad)


def test_convergence_order():
    ratio = {}
    for order in (1, 2):
        e32, e64 = (_toy_error(*ref.continuous_logsnr_grid(S), order, lower_order_final=False) for S in (32, 64))
        ratio[order] = e32 / e64
    print("error ratio 32 -> 64 steps:", ratio)
    assert 3.5 <= ratio[2] <= 4.5, ratio
    assert 1.8 <= ratio[1] <= 2.2, ratio
    # the restatement the GPU tests use as their reference has the same orders
    _, ratios = ref.toy_table()
    assert 3.5 <= ratios[2] <= 4.5 and 1.8 <= ratios[1] <= 2.2, ratios


def test_logsnr_grid():
    assert make_logsnr_timesteps(20, AC)[:4].tolist() == [999, 946, 888, 825]
    assert make_logsnr_timesteps(8, AC).tolist() == [999, 858, 681, 461, 233, 81, 20, 4, 0]
    for S in range(1, 28):
        nodes = make_logsnr_timesteps(S, AC)
        assert nodes.dtype == np.int64 and nodes.shape == (S + 1,) and nodes[0] == 999 and nodes[-1] == 0
        assert (np.diff(nodes) < 0).all(), S
        assert np.array_equal(nodes, ref.logsnr_nodes(S, AC))
    with pytest.raises(ValueError, match="27"):
        make_logsnr_timesteps(28, AC)
    _, a_t, a_prev = ref.logsnr_grid(20, AC)
    e_2m = _toy_error(a_t, a_prev, 2)
    _, a_t, a_prev = ref.uniform_grid(50, AC)
    e_ddim = _toy_error(a_t, a_prev, 1)
    print("toy problem: 2M logsnr S=20", e_2m, " DDIM uniform S=50", e_ddim)
    assert e_2m < e_ddim
    assert abs(e_2m - 0.0058) < 2e-4 and abs(e_ddim - 0.046) < 1e-3       # the figures of DESIGN.md §4


# ---- the samplers' host loops around a recording mock -------------------------------------------------------------------------------
class _Recorder(torch.nn.Module):
    """The tanh mock of tests/test_oracle_golden.py::test_plms_loop_against_reference_trace behind the model-callable protocol."""

    def __init__(self):
        super().__init__()
        from ldm.modules.attention import GatedSelfAttentionDense
        self.fuser = GatedSelfAttentionDense(8, 8, 1, 8)
        self.calls, self.restores = [], 0

    def restore_first_conv_from_SD(self):
        self.restores += 1

    def forward(self, inp):
        self.calls.append((int(inp["timesteps"][0]), "grounding_input" in inp, float(self.fuser.scale)))
        return _mock_eps(inp["x"], inp["timesteps"], "grounding_input" in inp)


def _mock_eps(x, t, cond):
    return torch.tanh(x) * (0.5 if cond else 0.3) + 0.01 * t.double().view(-1, 1, 1, 1) / 1000


def _diffusion():
    from ldm.models.diffusion.ldm import LatentDiffusion
    d = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
    sched = {k: getattr(d, k).numpy().astype(np.float64) for k in ("alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}
    return d, sched


def _replay(noise):
    """torch.randn_like that hands out noise[0], noise[1], ... in call order."""
    it = iter(noise)

    def fn(like, *a, **k):
        out = next(it).to(like)
        assert out.shape == like.shape
        return out
    return fn


def _rel_mse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).mean() / (b ** 2).mean())


def _inputs():
    x = syn.make_latent(2, 4, 8, 8, seed=5).double()
    inp = dict(x=x.clone(), timesteps=None, context=torch.zeros(2, 1, 1), grounding_input={}, inpainting_extra_input=None, grounding_extra_input=None)
    return x, inp


_LOOP_CASES = [pytest.param(S, grid, atype, False, id=f"S{S}-{grid}-{'alpha' if atype else 'noalpha'}")
               for S in (5, 10) for grid in ("uniform", "logsnr") for atype in (None, [0.3, 0.0, 0.7])] + \
              [pytest.param(5, "logsnr", [0.3, 0.0, 0.7], True, id="S5-logsnr-alpha-inpaint")]


@pytest.mark.parametrize("S,grid,atype,inpaint", _LOOP_CASES)
def test_dpm_solver_generic_loop(S, grid, atype, inpaint, monkeypatch):
    from gligen_inference import alpha_generator, set_alpha_scale
    diffusion, sched = _diffusion()
    mock = _Recorder()
    sampler = DPMSolverSampler(diffusion, mock, alpha_generator_func=partial(alpha_generator, type=atype), set_alpha_scale=set_alpha_scale)
    x, inp = _inputs()
    mask = x0 = noise = None
    if inpaint:
        g = torch.Generator().manual_seed(11)
        mask = (torch.rand(2, 1, 8, 8, generator=g) > 0.5).double()
        x0 = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
        noise = torch.randn(S, 2, 4, 8, 8, generator=g, dtype=torch.float64)
        monkeypatch.setattr(torch, "randn_like", _replay(noise))
    out = sampler.sample(S=S, shape=(2, 4, 8, 8), input=inp, uc=torch.ones(2, 1, 1), guidance_scale=7.5, mask=mask, x0=x0, ddim_discretize=grid)
    monkeypatch.undo()
    the_grid = (ref.uniform_grid if grid == "uniform" else ref.logsnr_grid)(S, sched["alphas_cumprod"])
    alphas = alpha_generator(S, atype)
    calls = []

    def eps_fn(xx, t, cond, scale):
        calls.append((int(t[0]), bool(cond), float(scale)))
        return _mock_eps(xx, t, cond)
    want = ref.dpm_sample(eps_fn, x, the_grid, sched, 7.5, alphas=alphas, mask=mask, x0=x0, noise=noise)
    assert mock.calls == calls == [(int(t), c, float(a)) for t, a in zip(the_grid[0], alphas) for c in (True, False)]
    assert mock.restores == sum(1 for a in alphas if a == 0)
    assert np.array_equal(np.flip(sampler.ddim_timesteps), the_grid[0])
    assert _rel_mse(out, want) < 1e-10
    assert inp["x"] is out and int(inp["timesteps"][0]) == int(the_grid[0][-1])
    # S = 5 takes the lower-order final step, S = 10 does not
    assert (sampler.solver_coefs[-1, 2] == 0) == (S < 10)


def test_dpm_solver_schedule_refusals():
    diffusion, _ = _diffusion()
    sampler = DPMSolverSampler(diffusion, _Recorder())
    with pytest.raises(ValueError, match="order"):
        sampler.make_schedule(10, order=3)
    with pytest.raises(ValueError, match="27"):
        sampler.make_schedule(28, ddim_discretize="logsnr")
    sampler.make_schedule(27, ddim_discretize="logsnr")
    assert len(sampler.ddim_timesteps) == 27 and sampler.solver_coefs.shape == (27, 3)


def test_ddim_eta(monkeypatch):
    """eta = 0.5 through StochasticDDIMSampler's host loop against the reference's p_sample_ddim in float64 with the same noise; eta = 0 is
    DDIMSampler's untouched branch, bit for bit. (DDIMSampler.make_schedule itself keeps refusing eta > 0: tests/test_host_cpu.py pins that.)"""
    from gligen_inference import alpha_generator, set_alpha_scale
    from ldm.models.diffusion.ddim import DDIMSampler, StochasticDDIMSampler
    diffusion, sched = _diffusion()
    S, atype = 10, [0.3, 0.0, 0.7]
    kw = dict(alpha_generator_func=partial(alpha_generator, type=atype), set_alpha_scale=set_alpha_scale)
    g = torch.Generator().manual_seed(12)
    z = torch.randn(S, 2, 4, 8, 8, generator=g, dtype=torch.float64)

    def run(cls, eta):
        mock = _Recorder()
        sampler = cls(diffusion, mock, **kw)
        if eta is not None:
            sampler.ddim_eta = eta
        x, inp = _inputs()
        monkeypatch.setattr(torch, "randn_like", _replay(z))
        out = sampler.sample(S=S, shape=(2, 4, 8, 8), input=inp, uc=torch.ones(2, 1, 1), guidance_scale=7.5)
        monkeypatch.undo()
        return x, out, mock, sampler

    x, out, mock, sampler = run(StochasticDDIMSampler, 0.5)
    grid = ref.uniform_grid(S, sched["alphas_cumprod"])
    sig = ref.ddim_eta_sigmas(grid[1], grid[2], 0.5)
    assert (sig > 0).all()
    np.testing.assert_allclose(np.asarray(sampler.ddim_sigmas, dtype=np.float64)[::-1], sig, rtol=1e-5)
    calls = []

    def eps_fn(xx, t, cond, scale):
        calls.append((int(t[0]), bool(cond), float(scale)))
        return _mock_eps(xx, t, cond)
    want = ref.ddim_eta_sample(eps_fn, x, grid, sig, z, sched, 7.5, alphas=alpha_generator(S, atype))
    assert mock.calls == calls
    assert _rel_mse(out, want) < 1e-10
    # the coefficient form the device loop gets is the same update
    from ldm.models.diffusion.dpm_solver import ddim_eta_coefficients
    cf = ddim_eta_coefficients(grid[1], grid[2], sig)
    rng = np.random.default_rng(3)
    for i in range(S):
        xx, e, zz = rng.standard_normal(16), rng.standard_normal(16), rng.standard_normal(16)
        d0 = (xx - math.sqrt(1 - grid[1][i]) * e) / math.sqrt(grid[1][i])
        direct = math.sqrt(grid[2][i]) * d0 + math.sqrt(1 - grid[2][i] - sig[i] ** 2) * e + sig[i] * zz
        assert np.abs(cf[i, 0] * xx + cf[i, 1] * d0 + cf[i, 3] * zz - direct).max() < 1e-12 * np.abs(direct).max()
    # eta = 0: the parent's branch
    _, base, _, _ = run(DDIMSampler, None)
    for eta in (None, 0.0):
        _, out0, _, s0 = run(StochasticDDIMSampler, eta)
        assert torch.equal(out0, base) and not s0._stochastic()
    assert not torch.equal(out, base)
    with pytest.raises(ValueError, match="negative"):
        StochasticDDIMSampler(diffusion, _Recorder()).make_schedule(10, ddim_eta=-0.1)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
PLMS_ARGS_SIZE = 168     # sizeof(gl_plms_args) before the solver loop existed: its layout is not this change's to touch


def test_solver_abi(tmp_path):
    from gligen_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gligen_amd_solver.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(gl_solver_args), sizeof(gl_plms_args));\n  return 0;\n}\n')
    exe = tmp_path / "sz"
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    solver, plms = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert solver == C.sizeof(_lib.SolverArgs)
    assert plms == C.sizeof(_lib.PlmsArgs) == PLMS_ARGS_SIZE
    plms_fields = [n for n, _ in _lib.PlmsArgs._fields_]
    solver_fields = [n for n, _ in _lib.SolverArgs._fields_]
    assert set(plms_fields) - set(solver_fields) == {"a_prev", "ddim"}
    assert set(solver_fields) - set(plms_fields) == {"cx", "c0", "c1", "c2", "cn", "step_noise"}
    from gligen_amd.build import build_native
    build_native()
    lib = _lib.load()
    import re
    declared = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "gligen_amd_solver.h")).read()))
    assert declared == set(_lib.SOLVER_SYMBOLS) == {"gl_sample_solver", "gl_op_solver_update"}
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes == _lib.SOLVER_SYMBOLS[name][1] and getattr(lib, name).restype == _lib.SOLVER_SYMBOLS[name][0]
    a = _lib.SolverArgs()
    a.struct_size = C.sizeof(_lib.SolverArgs) - 8
    assert lib.gl_sample_solver(None, C.byref(a), None) != 0
    msg = lib.gl_last_error().decode()
    assert str(C.sizeof(_lib.SolverArgs) - 8) in msg and str(C.sizeof(_lib.SolverArgs)) in msg and "gl_solver_args" in msg, msg
