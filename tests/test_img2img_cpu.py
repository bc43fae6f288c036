"""Image-to-image and two-pass generation on the host, no GPU: the tap table of gl_op_latent_renoise against its formulas, the C ABI of
include/gligen_amd_latent.h, an fp32 restatement of the kernel against float64, the ISA of latent.hip, and the samplers' partial
schedules (sample(x_init=, strength=)) through their host loops around a recording mock, against the float64 loops of tests/latent_ref.py
and tests/dpm_solver_ref.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dpm_solver_ref as dref
import latent_ref as ref
from helpers import ROOT
from gligen_amd import synthetic as syn


def _lib():
    from gligen_amd import _lib as table
    from gligen_amd.build import build_native
    build_native()
    return table.load(), table


def _taps(lib, table, n_in, n_out, mode):
    first = np.zeros(n_out, dtype=np.int32)
    w = np.full((n_out, 4), np.nan, dtype=np.float32)
    n = lib.gl_latent_resize_taps(n_in, n_out, table.LATENT_RESIZE_MODES[mode], first.ctypes.data_as(C.POINTER(C.c_int)),
                                  w.ctypes.data_as(C.POINTER(C.c_float)))
    assert n == ref.N_TAPS[mode], lib.gl_last_error()
    return first, w


# ---- the tap table ----------------------------------------------------------------------------------------------------------------
def test_torch_nearest_exact_is_the_integer_formula_on_the_test_pairs():
    """torch computes nearest-exact's index from a float scale; on the pairs the tests use it is the integer formula's (it is not on every
    pair: 2 -> 41 differs), so torch.equal against F.interpolate is a fair bar there."""
    for n_in, n_out in ref.SIZE_PAIRS:
        src = torch.arange(n_in, dtype=torch.float64).view(1, 1, 1, n_in)
        got = F.interpolate(src, size=(1, n_out), mode="nearest-exact").view(-1).long().tolist()
        assert got == [ref.nearest_index(o, n_in, n_out) for o in range(n_out)], (n_in, n_out)
    src = torch.arange(2, dtype=torch.float64).view(1, 1, 1, 2)
    assert F.interpolate(src, size=(1, 41), mode="nearest-exact").view(-1).long().tolist() != [ref.nearest_index(o, 2, 41) for o in range(41)]


@pytest.mark.parametrize("mode", ref.MODES)
def test_library_taps_equal_the_formulas(mode):
    """gl_latent_resize_taps against the formulas in float64: indices exactly, every weight to 4 ulp of itself (fp32)."""
    lib, table = _lib()
    worst = 0.0
    for n_in, n_out in ref.SIZE_PAIRS + ((2, 41), (41, 2), (1, 1)):
        first, w = _taps(lib, table, n_in, n_out, mode)
        want_first, want_w = ref.axis_taps(n_in, n_out, mode)
        assert np.array_equal(first, want_first), (n_in, n_out)
        if mode == "nearest-exact":
            assert first.tolist() == [ref.nearest_index(o, n_in, n_out) for o in range(n_out)]
        nt = ref.N_TAPS[mode]
        assert not w[:, nt:].any() and np.isfinite(w).all()
        ulp = np.spacing(np.abs(want_w[:, :nt]).astype(np.float32)).astype(np.float64)
        err = np.abs(w[:, :nt].astype(np.float64) - want_w[:, :nt]) / ulp
        worst = max(worst, float(err.max()))
        assert (err <= 4.0).all(), (n_in, n_out, float(err.max()))
        if n_in == n_out:       # the identity taps, exactly
            assert np.array_equal(w, np.tile(np.asarray({1: [1, 0, 0, 0], 2: [1, 0, 0, 0], 4: [0, 1, 0, 0]}[nt], dtype=np.float32), (n_out, 1)))
    print(f"[latent taps] {mode}: worst weight error {worst:.2f} ulp")
    # refusals: -1 and a message
    first, w = np.zeros(4, dtype=np.int32), np.zeros((4, 4), dtype=np.float32)
    ip, fp = first.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.gl_latent_resize_taps(4, 4, 7, ip, fp) == -1 and b"mode 7" in lib.gl_last_error()
    assert lib.gl_latent_resize_taps(0, 4, 2, ip, fp) == -1 and b"positive" in lib.gl_last_error()


def test_latent_entry_points_are_declared_exported_and_bound():
    lib, table = _lib()
    header = open(os.path.join(ROOT, "include", "gligen_amd_latent.h")).read()
    declared = set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", header))
    assert declared == set(table.LATENT_SYMBOLS) == {"gl_op_latent_renoise", "gl_latent_resize_taps"} and not declared & set(table.SYMBOLS)
    raw = C.CDLL(str(table.LIB_PATH))
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes == table.LATENT_SYMBOLS[name][1] and getattr(lib, name).restype == table.LATENT_SYMBOLS[name][0]
    for name, value in table.LATENT_RESIZE_MODES.items():
        assert re.search(r"#define GL_LATENT_" + name.upper().replace("-", "_") + r"\s+" + str(value) + r"\b", header), name
    # the header stands alone as C99
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c",
                    os.path.join(ROOT, "include", "gligen_amd_latent.h")], check=True)
    # a null context is refused before anything is launched
    assert lib.gl_op_latent_renoise(None, None, 1, 1, 1, 1, None, 1, 1, 2, 1.0, 0.0, None, 0, None) != 0


@pytest.mark.parametrize("mode", ref.MODES)
def test_fp32_restatement_against_float64(mode):
    """The kernel's arithmetic restated in numpy fp32 with the LIBRARY's taps, on the shapes of the GPU operator test, against float64
    F.interpolate * sa + s1 * noise: within (taps^2 + 8) 2^-24 (|sa| sum |w||v| + |s1||noise|) per element, and bit-equal to q_sample at
    equal sizes."""
    lib, table = _lib()
    from ldm.models.diffusion.ldm import LatentDiffusion
    diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
    worst = 0.0
    for n, (shape, size) in enumerate(ref.OP_SHAPES):
        g = torch.Generator().manual_seed(100 + n)
        src = torch.randn(shape, generator=g)
        t = 400 + 37 * n
        sa, s1 = float(diffusion.sqrt_alphas_cumprod[t]), float(diffusion.sqrt_one_minus_alphas_cumprod[t])
        taps_y, taps_x = _taps(lib, table, shape[2], size[0], mode), _taps(lib, table, shape[3], size[1], mode)
        for nb in (None, shape[0], 1):
            noise = None if nb is None else torch.randn((nb, shape[1]) + size, generator=g)
            got = ref.renoise_fp32(src, size, mode, sa, s1, noise, taps_y, taps_x)
            want = ref.renoise64(src, size, mode, sa, s1, noise)
            bound = ref.renoise_bound(src, size, mode, sa, s1, noise)
            err = (got.double() - want).abs()
            ok = err <= bound
            assert ok.all(), (shape, size, nb, float((err / bound)[~ok].max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            if tuple(shape[2:]) == size and noise is not None and nb == shape[0]:
                ts = torch.full((shape[0],), t, dtype=torch.long)
                assert torch.equal(got, diffusion.q_sample(src, ts, noise))
            if mode == "nearest-exact" and noise is None:
                assert torch.equal(ref.renoise_fp32(src, size, mode, 1.0, 0.0, None, taps_y, taps_x), F.interpolate(src, size=size, mode=mode))
    print(f"[latent restatement] {mode}: worst error / bound = {worst:.3f}")
    assert worst < 1.0


# ---- ISA ------------------------------------------------------------------------------------------------------------------------
def test_latent_kernels_use_no_scratch(tmp_path):
    from gligen_amd.build import EXTRA_FLAGS, SOURCES
    assert "latent.hip" in SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "latent.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *EXTRA_FLAGS.get("latent.hip", []), "-I", os.path.join(ROOT, "include"),
                        "--offload-device-only", "-S", os.path.join(ROOT, "gligen_amd", "csrc", "latent.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    kernels = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])[1:]
    names = [re.search(r"\.name:\s*(\S+)", e).group(1) for e in kernels]
    assert len(kernels) == 3 and all("latent_renoise_kernel" in n for n in names), names
    for e in kernels:
        val = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", e).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0
        assert val("max_flat_workgroup_size") == 256


# ---- the samplers' partial schedules through their host loops -------------------------------------------------------------------------
class _Recorder(torch.nn.Module):
    """The tanh mock of tests/test_dpm_solver_cpu.py behind the model-callable protocol; it keeps the first x it saw."""

    def __init__(self):
        super().__init__()
        from ldm.modules.attention import GatedSelfAttentionDense
        self.fuser = GatedSelfAttentionDense(8, 8, 1, 8)
        self.calls, self.restores, self.first_x = [], 0, None

    def restore_first_conv_from_SD(self):
        self.restores += 1

    def forward(self, inp):
        if self.first_x is None:
            self.first_x = inp["x"].clone()
        self.calls.append((int(inp["timesteps"][0]), "grounding_input" in inp, float(self.fuser.scale)))
        return _mock_eps(inp["x"], inp["timesteps"], "grounding_input" in inp)


def _mock_eps(x, t, cond):
    return torch.tanh(x) * (0.5 if cond else 0.3) + 0.01 * t.double().view(-1, 1, 1, 1) / 1000


def _diffusion():
    from ldm.models.diffusion.ldm import LatentDiffusion
    d = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
    sched = {k: getattr(d, k).numpy().astype(np.float64) for k in ("alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}
    return d, sched


def _rel_mse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).mean() / (b ** 2).mean())


def _sampler(name, diffusion, mock, atype):
    from gligen_inference import alpha_generator, set_alpha_scale
    from ldm.models.diffusion.ddim import DDIMSampler, StochasticDDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    cls = dict(plms=PLMSSampler, ddim=DDIMSampler, ddim_eta=StochasticDDIMSampler, dpmpp_2m=DPMSolverSampler)[name]
    s = cls(diffusion, mock, alpha_generator_func=partial(alpha_generator, type=atype), set_alpha_scale=set_alpha_scale)
    if name == "ddim_eta":
        s.ddim_eta = 0.5
    return s


def _draw_log(monkeypatch, scripted):
    """torch.randn / torch.randn_like that log their calls; randn_like hands out scripted[0], scripted[1], ..."""
    log, it, real = [], iter(scripted), torch.randn

    def randn(*a, **k):
        if "generator" not in k:
            log.append(("randn", tuple(a[0]) if len(a) == 1 and not isinstance(a[0], int) else tuple(a)))
        return real(*a, **k)

    def randn_like(like, *a, **k):
        log.append(("randn_like", tuple(like.shape)))
        return next(it).to(like)
    monkeypatch.setattr(torch, "randn", randn)
    monkeypatch.setattr(torch, "randn_like", randn_like)
    return log


_HOST_CASES = [("plms", 6, 0.5, "uniform"), ("ddim", 6, 0.5, "uniform"), ("ddim_eta", 6, 0.5, "uniform"), ("dpmpp_2m", 10, 0.6, "uniform"),
               ("dpmpp_2m", 10, 0.6, "logsnr"), ("dpmpp_2m", 5, 0.4, "uniform"), ("plms", 6, 1.0, "uniform"), ("dpmpp_2m", 5, 1.0, "logsnr")]


@pytest.mark.parametrize("atype", [[0.5, 0.0, 0.5], [1, 0, 0]], ids=["gate_off_tail", "gate_on"])
@pytest.mark.parametrize("name,S,strength,grid", _HOST_CASES, ids=[f"{n}-S{S}-{st}-{g}" for n, S, st, g in _HOST_CASES])
def test_tail_through_the_host_loops(name, S, strength, grid, atype, monkeypatch):
    """sample(x_init=, strength=) through _sample_generic: the visited timesteps are the schedule's tail (PLMS: with its second evaluation
    at the tail's first step), the gate values the tail of alpha_generator(S), the init draw the first of the run, the start
    q_sample(resize(x_init), tail[0], that draw), and the result the float64 loop's over the tail."""
    from gligen_inference import alpha_generator
    diffusion, sched = _diffusion()
    mock = _Recorder()
    sampler = _sampler(name, diffusion, mock, atype)
    B, shape = 2, (2, 4, 8, 12)
    g = torch.Generator().manual_seed(31)
    x_init = torch.randn(1, 4, 8, 8, generator=g, dtype=torch.float64)            # batch 1, another width: broadcast and resized
    z = torch.randn(S + 1, *shape, generator=g, dtype=torch.float64)              # the step noise of eta > 0
    torch.manual_seed(17)
    init_noise = torch.randn(shape)                                               # what the sampler will draw (the same global generator state)
    torch.manual_seed(17)
    log = _draw_log(monkeypatch, z)
    inp = dict(x=None, timesteps=None, context=torch.zeros(B, 1, 1), grounding_input={}, inpainting_extra_input=None, grounding_extra_input=None)
    kw = dict(ddim_discretize=grid) if name == "dpmpp_2m" else {}
    out = sampler.sample(S=S, shape=shape, input=inp, uc=torch.ones(B, 1, 1), guidance_scale=7.5, x_init=x_init, strength=strength,
                         resize_mode="bilinear", **kw)
    monkeypatch.undo()
    full = (dref.uniform_grid if grid == "uniform" else dref.logsnr_grid)(S, sched["alphas_cumprod"])
    n = len(full[0])                     # the schedule's length: make_ddim_timesteps' uniform grid of S = 6 has 7 steps
    assert n == (7 if S == 6 else S)
    k = int(strength * n)
    tail = ref.tail_grid(full, k)
    gates = alpha_generator(n, atype)[n - k:]
    assert len(gates) == k and np.array_equal(np.flip(sampler.ddim_timesteps), tail[0])
    # draws: the init draw first, then (eta > 0) one per step
    assert log[0] == ("randn", shape) and log[1:] == ([("randn_like", shape)] * k if name == "ddim_eta" else [])
    # the start point
    start = ref.start64(x_init, shape[2:], "bilinear", sched, tail[0][0], init_noise)
    assert _rel_mse(mock.first_x, start) < 1e-12
    if strength == 1.0:
        assert k == n and int(tail[0][0]) == int(full[0][0]) == max(int(t) for t in full[0])
    # evaluations
    calls = []

    def eps_fn(xx, t, cond, scale):
        calls.append((int(t[0]), bool(cond), float(scale)))
        return _mock_eps(xx, t, cond)
    if name == "dpmpp_2m":
        want = dref.dpm_sample(eps_fn, start, tail, sched, 7.5, alphas=gates)
        assert sampler.solver_coefs.shape == (k, 3) and sampler.solver_coefs[0, 2] == 0           # the tail's first step is order 1
        assert (sampler.solver_coefs[-1, 2] == 0) == (k < 10 or k == 1) and (k < 3 or sampler.solver_coefs[1, 2] != 0)
    elif name == "ddim_eta":
        sig = dref.ddim_eta_sigmas(full[1], full[2], 0.5)[n - k:]
        want = dref.ddim_eta_sample(eps_fn, start, tail, sig, z, sched, 7.5, alphas=gates)
    else:
        want = ref.plms_sample(eps_fn, start, tail, 7.5, alphas=gates, multistep=name == "plms")
    assert mock.calls == calls
    visited = [t for t, c, _ in mock.calls if c]
    extra = [int(tail[0][min(1, k - 1)])] if name == "plms" else []
    assert visited == [int(tail[0][0])] + extra + [int(t) for t in tail[0][1:]]
    assert [s for _, c, s in mock.calls if c] == [float(gates[0])] * (1 + len(extra)) + [float(a) for a in gates[1:]]
    assert mock.restores == sum(1 for a in gates if a == 0)
    if atype == [0.5, 0.0, 0.5]:
        assert gates == ([1] * int(0.5 * n) + [0] * (n - int(0.5 * n)))[n - k:]
        if S == 6 and strength < 1.0:
            assert gates[0] == 0, "3 of 7 steps: the tail starts inside the gated-off part"
        if S == 10 and strength < 1.0:
            assert gates[:2] == [1, 0], "6 of 10 steps: the gates go off at the tail's second step"
    assert _rel_mse(out, want) < 1e-10
    assert inp["x"] is out and int(inp["timesteps"][0]) == int(tail[0][-1])
    # the next plain run of the same sampler is whole again
    inp2 = dict(inp, x=torch.randn(shape, generator=g, dtype=torch.float64))
    n_before = len(mock.calls)
    sampler.sample(S=S, shape=shape, input=inp2, uc=None, guidance_scale=1, **kw)
    assert len(mock.calls) - n_before == n + (1 if name == "plms" else 0) and len(sampler.ddim_timesteps) == n


def test_strength_none_changes_nothing():
    diffusion, _ = _diffusion()
    outs = []
    for kw in ({}, dict(x_init=None, strength=None, resize_mode="nearest-exact")):
        mock = _Recorder()
        sampler = _sampler("dpmpp_2m", diffusion, mock, [0.3, 0.0, 0.7])
        x = syn.make_latent(2, 4, 8, 8, seed=5).double()
        inp = dict(x=x.clone(), timesteps=None, context=torch.zeros(2, 1, 1), grounding_input={}, inpainting_extra_input=None, grounding_extra_input=None)
        outs.append((sampler.sample(S=5, shape=(2, 4, 8, 8), input=inp, uc=torch.ones(2, 1, 1), guidance_scale=7.5, **kw), mock.calls))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


def test_given_noise_is_the_start_noise():
    """input["x"], when given, is the noise of the start point (the role starting_noise has in a whole run): nothing is drawn."""
    diffusion, sched = _diffusion()
    mock = _Recorder()
    sampler = _sampler("ddim", diffusion, mock, None)
    g = torch.Generator().manual_seed(3)
    x_init, noise = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64), torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    inp = dict(x=noise.clone(), timesteps=None, context=torch.zeros(2, 1, 1), grounding_input={}, inpainting_extra_input=None, grounding_extra_input=None)
    state = torch.get_rng_state()
    sampler.sample(S=4, shape=(2, 4, 8, 8), input=inp, x_init=x_init, strength=0.5)
    assert torch.equal(torch.get_rng_state(), state)
    t0 = int(dref.uniform_grid(4, sched["alphas_cumprod"])[0][2])
    assert mock.calls[0][0] == t0 and torch.equal(mock.first_x, diffusion.q_sample(x_init, torch.full((2,), t0), noise))


def test_sampler_refusals():
    diffusion, _ = _diffusion()
    x = torch.zeros(2, 4, 8, 8)
    inp = lambda: dict(x=None, timesteps=None, context=torch.zeros(2, 1, 1), grounding_input={}, inpainting_extra_input=None, grounding_extra_input=None)
    for name in ("plms", "ddim", "ddim_eta", "dpmpp_2m"):
        sampler = _sampler(name, diffusion, _Recorder(), None)
        run = lambda **kw: sampler.sample(S=10, shape=(2, 4, 8, 8), input=inp(), **kw)
        for bad in (0.0, -0.1, 1.01, float("nan")):
            with pytest.raises(ValueError, match=r"strength = .* is not in \(0, 1\]"):
                run(x_init=x, strength=bad)
        with pytest.raises(ValueError, match=r"leaves no step to run"):
            run(x_init=x, strength=0.05)
        with pytest.raises(ValueError, match="x_init needs strength"):
            run(x_init=x)
        with pytest.raises(ValueError, match="needs x_init"):
            run(strength=0.5)
        with pytest.raises(ValueError, match="resize_mode 'nearest'"):
            run(x_init=x, strength=0.5, resize_mode="nearest")
        with pytest.raises(ValueError, match="x_init .* is not"):
            run(x_init=torch.zeros(3, 4, 8, 8), strength=0.5)
        with pytest.raises(TypeError):
            sampler.sample(10, (2, 4, 8, 8), inp(), None, 1, None, None, x, 0.5)          # keyword-only
        assert not sampler.model.calls


def test_generate_refusals(monkeypatch):
    import gligen_inference as gi
    model = types.SimpleNamespace(image_size=8, channel_mult=[1, 2], in_channels=4, downsample_net=None)
    ae = types.SimpleNamespace(ddconfig={"ch_mult": [1, 2]})              # factor 2, total stride 2: sizes are multiples of 4, default 16 x 16
    ctx = torch.zeros(2, 1, 1)
    lat, img, mask = torch.zeros(2, 4, 8, 8), torch.zeros(2, 3, 16, 16), torch.ones(2, 1, 8, 8)
    gen = lambda **kw: gi.generate(model, ae, None, {}, ctx, ctx, **kw)
    with pytest.raises(ValueError, match="init_latent needs strength"):
        gen(init_latent=lat)
    with pytest.raises(ValueError, match="init_image needs strength"):
        gen(init_image=img)
    with pytest.raises(ValueError, match="needs init_image or init_latent"):
        gen(strength=0.5)
    with pytest.raises(ValueError, match="give one of them"):
        gen(init_latent=lat, init_image=img, strength=0.5)
    with pytest.raises(ValueError, match="hires = 12 x 16 is smaller"):
        gen(hires=(12, 16))
    with pytest.raises(ValueError, match="hires = 32 x 12 is smaller"):
        gen(hires=(32, 12))
    with pytest.raises(ValueError, match="hires = 16 x 16 is smaller"):
        gen(hires=(16, 16), height=32, width=16)
    with pytest.raises(ValueError, match="height = 18"):
        gen(hires=(18, 16))
    with pytest.raises(ValueError, match="hires_upscaler 'lanczos'"):
        gen(hires=(32, 32), hires_upscaler="lanczos")
    with pytest.raises(ValueError, match="hires with inpainting_mask"):
        gen(hires=(32, 32), inpainting_mask=mask, z0=lat)
    with pytest.raises(ValueError, match="init_image / init_latent with inpainting_mask"):
        gen(init_latent=lat, strength=0.5, inpainting_mask=mask, z0=lat)
    with pytest.raises(ValueError, match=r"init_image .* is not \[2 or 1, 3, H, W\]"):
        gen(init_image=torch.zeros(3, 3, 16, 16), strength=0.5)
    with pytest.raises(ValueError, match="hires through generate_lanes"):
        gi.generate_lanes(model, ae, None, {}, ctx, ctx, lanes=1, hires=(32, 32))
    with pytest.raises(ValueError, match="hires through generate_stream"):
        gi.generate_stream(model, ae, None, {}, ctx, ctx, [None], hires=(32, 32))
    assert sorted(gi.HIRES_UPSCALERS) == ["latent-bicubic", "latent-bilinear", "latent-nearest", "pixel-bicubic"]
    # run(): the config keys, before anything is loaded or sampled
    cfg = {"grounding_tokenizer_input": dict(target="grounding_input.text_grounding_tokinzer_input.GroundingNetInput")}
    models = (model, ae, None, None, cfg)
    base = dict(batch_size=2, guidance_scale=7.5, negative_prompt=None, no_plms=False, folder="unused")
    meta = dict(ckpt="synthetic_text", save_folder_name="x")
    with pytest.raises(ValueError, match="hires with --repeat"):
        gi.run(meta, dict(base, hires_height=32, repeat=2), models=models)
    with pytest.raises(ValueError, match="hires_height x hires_width = 32 x 8 is smaller"):
        gi.run(meta, dict(base, hires_height=32, hires_width=8), models=models)
    with pytest.raises(ValueError, match="init_image and strength go together"):
        gi.run(meta, dict(base, init_image="a.png"), models=models)
    with pytest.raises(ValueError, match="init_image and strength go together"):
        gi.run(meta, dict(base, strength=0.5), models=models)
    with pytest.raises(ValueError, match="hires with an inpainting entry"):
        gi.run(dict(meta, input_image="a.png"), dict(base, hires_width=32), models=models)
    # the command line carries the same names
    import argparse
    seen = {}
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", lambda self, argv=None: seen.setdefault("opts", {a.dest for a in self._actions}) and (_ for _ in ()).throw(SystemExit(0)))
    with pytest.raises(SystemExit):
        gi.main([])
    assert {"init_image", "strength", "hires_height", "hires_width", "hires_strength", "hires_steps", "hires_upscaler"} <= seen["opts"]
