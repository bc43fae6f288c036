"""Image-to-image and two-pass generation on a real MI355X: gl_op_latent_renoise by itself against float64, the samplers' partial
schedules on the device loops against float64 loops around the CPU oracle UNet, and generate() / run() with the new keywords against
the hand composition from the sampler classes, Engine.latent_renoise and the autoencoder. Small UNet and VAE, the latent size and batch
of the *_unet_small goldens."""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dpm_solver_ref as dref
import latent_ref as ref
from helpers import build_product_unet, build_product_vae, golden_shapes, grounding_kwargs, load_golden, mse, oracle_cfg
from gligen_amd import synthetic as syn

pytestmark = pytest.mark.gpu

PLMS_TOL = 2e-3        # relative MSE of the final latent: the bar of tests/test_path_gpu.py::test_plms_vs_reference
REPORT = {}


@pytest.fixture(autouse=True)
def _report(record_property):
    before = set(REPORT)
    yield
    for key in sorted(set(REPORT) - before):
        record_property(key, json.dumps(REPORT[key], sort_keys=True))
        print(f"[img2img] {key}: {json.dumps(REPORT[key], sort_keys=True)}")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _replay(noise):
    it = iter(noise)

    def fn(like, *a, **k):
        out = next(it).to(like)
        assert tuple(out.shape) == tuple(like.shape), (out.shape, like.shape)
        return out
    return fn


def _rel(a, b):
    b = b.float().cpu()
    return mse(a, b) / float(b.var())


def _diffusion(dev="cpu"):
    from ldm.models.diffusion.ldm import LatentDiffusion
    return LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).to(dev)


# ---- 1: the operator alone ----------------------------------------------------------------------------------------------------------
GUARD = 4096


def _guarded(dev, shape):
    """A NaN-filled buffer with the output in its middle: (buffer, the output view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev, dtype=torch.float32)
    return buf, buf[GUARD:GUARD + n].view(shape)


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("shape,size", ref.OP_SHAPES, ids=[f"{s[2]}x{s[3]}-{o[0]}x{o[1]}" for s, o in ref.OP_SHAPES])
def test_latent_renoise_against_float64(engine, shape, size, mode):
    """Noise none, of batch B and of batch 1. Per element |got - ref| <= (taps^2 + 8) 2^-24 (|sa| sum |w||v| + |s1||noise|): the bar the
    fp32 grid resize is held to. Equal sizes: torch.equal to diffusion.q_sample. nearest-exact with sa = 1 and no noise: torch.equal to
    F.interpolate. The output sits between NaN guard zones that stay untouched; a second call gives the same bits."""
    dev = engine.device
    diffusion = _diffusion()
    g = torch.Generator().manual_seed(sum(shape) + 7 * sum(size))
    src = torch.randn(shape, generator=g)
    t = 437
    sa, s1 = float(diffusion.sqrt_alphas_cumprod[t]), float(diffusion.sqrt_one_minus_alphas_cumprod[t])
    srcd = src.to(dev)
    worst = 0.0
    for nb in (None, shape[0], 1):
        noise = None if nb is None else torch.randn((nb, shape[1]) + size, generator=g)
        buf, out = _guarded(dev, (shape[0], shape[1]) + size)
        got = engine.latent_renoise(srcd, size, mode, sa, s1, None if noise is None else noise.to(dev), out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), "the kernel wrote outside its output"
        assert torch.equal(srcd.cpu(), src)
        got = got.cpu()
        want = ref.renoise64(src, size, mode, sa, s1, noise)
        bound = ref.renoise_bound(src, size, mode, sa, s1, noise)
        err = (got.double() - want).abs()
        frac = float((err[bound > 0] / bound[bound > 0]).max())
        worst = max(worst, frac)
        assert (err <= bound).all(), (nb, frac)
        again = engine.latent_renoise(srcd, size, mode, sa, s1, None if noise is None else noise.to(dev))
        assert torch.equal(again.cpu(), got)
        if tuple(shape[2:]) == size and noise is not None:
            ts = torch.full((shape[0],), t, dtype=torch.long)
            assert torch.equal(got, diffusion.q_sample(src, ts, noise.expand(got.shape)))
    if mode == "nearest-exact":
        assert torch.equal(engine.latent_renoise(srcd, size, mode).cpu(), F.interpolate(src, size=size, mode=mode))
    REPORT[f"op_{mode}_{shape[2]}x{shape[3]}_{size[0]}x{size[1]}"] = dict(worst_err_over_bound=worst)


def test_latent_renoise_refusals(engine):
    import ctypes as C
    from gligen_amd import GligenAmdError, _lib
    dev = engine.device
    x = torch.zeros(3, 4, 8, 8, device=dev)
    with pytest.raises(GligenAmdError, match="dst == src"):
        engine.latent_renoise(x, (8, 8), "bicubic", out=x)
    with pytest.raises(ValueError, match="mode 'nearest'"):
        engine.latent_renoise(x, (8, 8), "nearest")
    with pytest.raises(ValueError, match="noise"):
        engine.latent_renoise(x, (8, 8), noise=torch.zeros(2, 4, 8, 8, device=dev))
    y = torch.zeros(3, 4, 8, 8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda mode, nb: engine.lib.gl_op_latent_renoise(engine._ctx, p(x), 3, 4, 8, 8, p(y), 8, 8, mode, 1.0, 0.5, p(x), nb, None)
    for mode, nb, what in ((2, 2, "noise_B = 2"), (7, 3, "mode 7")):
        with pytest.raises(GligenAmdError, match=what):
            _lib.check(call(mode, nb))


# ---- the sampler cases ----------------------------------------------------------------------------------------------------------------
class _Case:
    """The fixture of the *_unet_small goldens (tests/test_dpm_solver_gpu.py): seeded small UNet, text grounding, guidance 7.5 against an
    unconditional context."""

    def __init__(self, dev, tmp_path, monkeypatch, alpha_type):
        meta = load_golden("ddim_unet_small")["meta"]
        self.dev, self.alpha_type = dev, alpha_type
        self.B, self.hw, self.n_valid = meta["B"], meta["hw"], meta["n_valid"]
        self.tmp_path, self.monkeypatch = tmp_path, monkeypatch
        torch.save(syn.sd_first_conv_state(), tmp_path / "SD_input_conv_weight_bias.pth")
        monkeypatch.chdir(tmp_path)
        self.diffusion = _diffusion(dev)
        self.batch = syn.make_batch("text", self.B, n_valid=self.n_valid, seed=1)
        self.ctx, self.uc = syn.make_context(self.B, seed=1), syn.make_context(self.B, seed=9)

    def model(self):
        return build_product_unet(syn.UNET_CFG_SMALL, "text", False, device=self.dev)

    def sampler(self, model, cls, use_graph=True, eta=None):
        from gligen_inference import alpha_generator, set_alpha_scale
        s = cls(self.diffusion, model, alpha_generator_func=partial(alpha_generator, type=self.alpha_type), set_alpha_scale=set_alpha_scale)
        s.use_graph = use_graph
        if eta is not None:
            s.ddim_eta = eta
        return s

    def input(self, model, x):
        gin = model.grounding_tokenizer_input.prepare(_to(self.batch, self.dev))
        return dict(x=None if x is None else x.to(self.dev), timesteps=None, context=self.ctx.to(self.dev), grounding_input=gin,
                    inpainting_extra_input=None, grounding_extra_input=None)

    def run(self, model, cls, S, shape, noise, x_init, strength, mode, use_graph=True, randn_like=None, eta=None, **schedule_kwargs):
        sampler = self.sampler(model, cls, use_graph, eta)
        if randn_like is not None:
            self.monkeypatch.setattr(torch, "randn_like", randn_like)
        out = sampler.sample(S=S, shape=shape, input=self.input(model, noise), uc=self.uc.to(self.dev), guidance_scale=7.5,
                             x_init=None if x_init is None else x_init.to(self.dev), strength=strength, resize_mode=mode, **schedule_kwargs)
        self.monkeypatch.undo()
        self.monkeypatch.chdir(self.tmp_path)
        return out.clone(), sampler

    def oracle(self):
        import oracle.gligen_oracle as orc
        sd = syn.seeded_state_dict(golden_shapes("unet_small_text"), 1234)
        gk = grounding_kwargs("text", self.batch)
        gnull = orc.null_grounding("text", gk)
        cfg = oracle_cfg(syn.UNET_CFG_SMALL, "text")

        def eps_fn(x, t, cond, scale):
            inp = dict(x=x.float(), timesteps=t, context=self.ctx if cond else self.uc, grounding_input=gk if cond else gnull, inpainting_extra_input=None)
            with torch.no_grad():
                return orc.unet_forward(sd, cfg, inp, fuser_scale=scale)

        def swap_in_sd_first_conv():
            sdc = syn.sd_first_conv_state()
            sd["input_blocks.0.0.weight"], sd["input_blocks.0.0.bias"] = sdc["weight"], sdc["bias"]
        sched = {k: v.astype(np.float64) for k, v in orc.make_schedule().items()}
        return eps_fn, swap_in_sd_first_conv, sched


GATE_OFF_TAIL = [0.5, 0.0, 0.5]      # the tails below start inside (or one step before) the gated-off part: the SD first conv goes in at once
HIRES_PX = (32, 48)                  # from the goldens' 32 x 32 pixels (latent 16 x 16) to a latent of 16 x 24


@pytest.fixture(scope="module", autouse=True)
def _warm_process(tmp_path_factory):
    """One untimed pass of everything compared bit for bit below, at both latent sizes: the engine tunes GEMM tiles and times its kernel
    forms at the first eager launch of a shape, process-wide, and the run that does the tuning differs from every later run of the
    process by bf16 rounding (tests/test_dpm_solver_gpu.py has the measurement)."""
    if not torch.cuda.is_available():
        yield
        return
    import gligen_inference as gi
    mp = pytest.MonkeyPatch()
    try:
        dev = torch.device("cuda:0")
        mp.setattr(gi, "device", dev)
        case = _Case(dev, tmp_path_factory.mktemp("warm"), mp, GATE_OFF_TAIL)
        model, ae = case.model(), build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
        for up in ("latent-bicubic", "pixel-bicubic"):
            _hires(case, model, ae, up, use_graph=False)
        model._drop_engine()
        ae._drop_engine()
    finally:
        mp.undo()
    yield


_TAILS = [
    # id, sampler, S, strength, schedule kwargs, eta, alpha_type, (h, w) of x_init, batch of x_init, (h, w) of the run
    ("plms", "plms", 6, 0.5, {}, None, GATE_OFF_TAIL, (16, 16), 2, (16, 16)),
    ("ddim", "ddim", 6, 0.5, {}, None, GATE_OFF_TAIL, (16, 16), 1, (16, 24)),
    ("ddim_eta", "ddim_eta", 6, 0.5, {}, 0.5, [1, 0, 0], (16, 16), 2, (16, 16)),
    ("2m_uniform", "2m", 10, 0.6, dict(ddim_discretize="uniform"), None, GATE_OFF_TAIL, (16, 16), 2, (16, 24)),
    ("2m_logsnr", "2m", 10, 0.6, dict(ddim_discretize="logsnr"), None, [1, 0, 0], (16, 16), 2, (16, 16)),
    ("2m_lower_order_final", "2m", 5, 0.4, dict(ddim_discretize="uniform"), None, GATE_OFF_TAIL, (16, 16), 2, (16, 16)),
    ("2m_strength_1", "2m", 5, 1.0, dict(ddim_discretize="logsnr"), None, [1, 0, 0], (16, 16), 2, (16, 24)),
]


@pytest.mark.parametrize("case_id,name,S,strength,skw,eta,atype,init_hw,init_b,run_hw", _TAILS, ids=[c[0] for c in _TAILS])
def test_tail_against_float64_loop(case_id, name, S, strength, skw, eta, atype, init_hw, init_b, run_hw, tmp_path, monkeypatch):
    """sample(x_init=, strength=) on the device loops against the float64 loop over the schedule's tail around the CPU oracle UNet, both
    started from the float64 resize + q_sample; eager and hipGraph runs agree bit for bit."""
    from gligen_inference import alpha_generator
    from ldm.models.diffusion.ddim import DDIMSampler, StochasticDDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    cls = {"plms": PLMSSampler, "ddim": DDIMSampler, "ddim_eta": StochasticDDIMSampler, "2m": DPMSolverSampler}[name]
    dev = _dev()
    case = _Case(dev, tmp_path, monkeypatch, atype)
    assert case.hw == 16 and case.B == 2
    shape = (case.B, 4) + run_hw
    g = torch.Generator().manual_seed(41)
    x_init = torch.randn((init_b, 4) + init_hw, generator=g)
    noise = torch.randn(shape, generator=g)
    z = torch.randn((S + 1,) + shape, generator=g)
    outs = []
    for use_graph in (False, True):
        model = case.model()
        out, sampler = case.run(model, cls, S, shape, noise, x_init, strength, "bicubic", use_graph, randn_like=_replay(z.to(dev)) if eta else None,
                                eta=eta, **skw)
        outs.append(out)
        n_evals = model.engine.sampler_timing()[2]
        restored = bool(model.__dict__.get("_first_conv_restored"))
        model._drop_engine()
    eps_fn, gate_off, sched = case.oracle()
    full = (dref.logsnr_grid if skw.get("ddim_discretize") == "logsnr" else dref.uniform_grid)(S, sched["alphas_cumprod"])
    n = len(full[0])
    k = int(strength * n)
    tail = ref.tail_grid(full, k)
    gates = alpha_generator(n, atype)[n - k:]
    assert np.array_equal(np.flip(sampler.ddim_timesteps), tail[0]) and n_evals == k + (1 if name == "plms" else 0)
    assert restored == (0 in gates)
    if strength == 1.0:
        assert k == n and int(tail[0][0]) == int(full[0][0])
    start = ref.start64(x_init, run_hw, "bicubic", sched, tail[0][0], noise)
    if name == "2m":
        want = dref.dpm_sample(eps_fn, start, tail, sched, 7.5, alphas=gates, on_gate_off=gate_off)
        assert sampler.solver_coefs[0, 2] == 0 and sampler.solver_coefs[-1, 2] == 0 and (k < 3 or sampler.solver_coefs[1, 2] != 0)
    elif name == "ddim_eta":
        sig = dref.ddim_eta_sigmas(full[1], full[2], eta)[n - k:]
        want = dref.ddim_eta_sample(eps_fn, start, tail, sig, z, sched, 7.5, alphas=gates, on_gate_off=gate_off)
    else:
        want = ref.plms_sample(eps_fn, start, tail, 7.5, alphas=gates, on_gate_off=gate_off, multistep=name == "plms")
    rel = _rel(outs[0], want)
    REPORT[f"tail_{case_id}"] = dict(x_rel_mse=rel, steps_run=k, of=n, first_gate=float(gates[0]))
    assert rel < PLMS_TOL, rel
    assert torch.equal(outs[0], outs[1]), "hipGraph replay must reproduce the eager launch sequence bit for bit"


# ---- generate() -----------------------------------------------------------------------------------------------------------------------
S1, S2, HIRES_STRENGTH = 5, 10, 0.6


def _gen_kwargs(case, **kw):
    # (build_product_unet keeps the full model's image_size: the goldens' 16 x 16 latent is asked for in pixels)
    return dict(dict(steps=S1, guidance_scale=7.5, alpha_type=case.alpha_type, sampler="dpmpp_2m", discretize="logsnr", height=2 * case.hw,
                     width=2 * case.hw), **kw)


def _hires(case, model, ae, upscaler, use_graph=True, seed=123):
    import gligen_inference as gi
    dev = case.dev
    torch.manual_seed(seed)
    x_T = syn.make_latent(case.B, 4, case.hw, case.hw, seed=6).to(dev)
    return gi.generate(model, ae, case.diffusion, _to(case.batch, dev), case.ctx.to(dev), case.uc.to(dev), starting_noise=x_T, use_graph=use_graph,
                       hires=HIRES_PX, hires_strength=HIRES_STRENGTH, hires_steps=S2, hires_upscaler=upscaler, **_gen_kwargs(case)).clone()


def _hires_by_hand(case, model, ae, upscaler, seed=123):
    """The same two passes from the sampler classes, Engine.latent_renoise and the autoencoder, both passes on `model`'s own context."""
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    dev = case.dev
    torch.manual_seed(seed)
    x_T = syn.make_latent(case.B, 4, case.hw, case.hw, seed=6).to(dev)
    lat, _ = case.run(model, DPMSolverSampler, S1, (case.B, 4, case.hw, case.hw), x_T, None, None, "bicubic", ddim_discretize="logsnr")
    h2, w2 = HIRES_PX[0] // 2, HIRES_PX[1] // 2
    mode = "bicubic"
    if upscaler == "pixel-bicubic":
        image = torch.clamp(ae.decode(lat), -1.0, 1.0)
        lat = ae.encode(model.engine.latent_renoise(image, HIRES_PX, "bicubic"))
    lat2, sampler = case.run(model, DPMSolverSampler, S2, (case.B, 4, h2, w2), None, lat, HIRES_STRENGTH, mode, ddim_discretize="logsnr")
    return ae.decode(lat2).clone(), len(sampler.ddim_timesteps)


@pytest.mark.parametrize("upscaler", ["latent-bicubic", "pixel-bicubic"])
def test_generate_hires_is_the_hand_composition(upscaler, tmp_path, monkeypatch):
    """generate(hires=...) against the two passes made by hand on another model with the same weights; the image has the second pass's
    size; from the second call on no context allocates or changes (Engine.memory() of the model's engine, its second-pass fork and the
    autoencoder's engine), and the fork ran the tail's evaluations only."""
    import gligen_inference as gi
    dev = _dev()
    monkeypatch.setattr(gi, "device", dev)
    case = _Case(dev, tmp_path, monkeypatch, [1, 0, 0])
    model, ae = case.model(), build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    outs, mems = [], []
    for _ in range(3):
        outs.append(_hires(case, model, ae, upscaler))
        fork = model.__dict__["_hires"][(case.B, HIRES_PX[0] // 2, HIRES_PX[1] // 2)][0]
        torch.cuda.synchronize()
        mems.append((model.engine.memory(), fork.engine.memory(), ae.engine.memory()))
    assert tuple(outs[0].shape) == (case.B, 3) + HIRES_PX and torch.isfinite(outs[0]).all()
    assert mems[1] == mems[2], "a context allocated between the second and the third call"
    assert mems[1][1]["is_fork"] and not mems[1][0]["is_fork"] and len(model.__dict__["_hires"]) == 1
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    k = int(HIRES_STRENGTH * S2)
    assert fork.engine.sampler_timing()[2] == k and model.engine.sampler_timing()[2] == S1
    other = case.model()
    by_hand, n2 = _hires_by_hand(case, other, ae, upscaler)
    assert n2 == k
    assert torch.equal(outs[1], by_hand)
    plain = gi.generate(model, ae, case.diffusion, _to(case.batch, dev), case.ctx.to(dev), case.uc.to(dev),
                        starting_noise=syn.make_latent(case.B, 4, case.hw, case.hw, seed=6).to(dev), **_gen_kwargs(case))
    assert tuple(plain.shape) == (case.B, 3, 2 * case.hw, 2 * case.hw)
    REPORT[f"hires_{upscaler}"] = dict(own_bytes_model=mems[2][0]["own_bytes"], own_bytes_fork=mems[2][1]["own_bytes"], evals_pass2=k)
    for m in (model, other, ae):
        m._drop_engine()


def test_hires_first_conv_state_across_the_contexts(tmp_path, monkeypatch):
    """alpha_type [0.3, 0, 0.7]: the first pass swaps the SD first conv in, the second pass's fork is made with it. Two calls on one model:
    the first is a fresh model's call, the second the call of a fresh model on which one plain generate() with that alpha_type ran first
    -- the pair of passes leaves the model as a plain call does --, bit for bit."""
    import gligen_inference as gi
    dev = _dev()
    monkeypatch.setattr(gi, "device", dev)
    case = _Case(dev, tmp_path, monkeypatch, [0.3, 0.0, 0.7])
    ae = build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    model = case.model()
    first = _hires(case, model, ae, "latent-bicubic")
    assert model.first_conv_type == "SD" and model.__dict__["_first_conv_restored"]
    fork, state = model.__dict__["_hires"][(case.B, HIRES_PX[0] // 2, HIRES_PX[1] // 2)]
    assert state == ("SD", True) and fork.__dict__["_first_conv_restored"]
    second = _hires(case, model, ae, "latent-bicubic")
    assert model.__dict__["_hires"][(case.B, HIRES_PX[0] // 2, HIRES_PX[1] // 2)][0] is fork, "the fork was rebuilt although the model's state did not change"
    scale_after = model.fuser_scales()
    model._drop_engine()
    fresh = case.model()
    assert torch.equal(first, _hires(case, fresh, ae, "latent-bicubic"))
    fresh._drop_engine()
    fresh = case.model()
    torch.manual_seed(5)
    gi.generate(fresh, ae, case.diffusion, _to(case.batch, dev), case.ctx.to(dev), case.uc.to(dev),
                starting_noise=syn.make_latent(case.B, 4, case.hw, case.hw, seed=6).to(dev), **_gen_kwargs(case))
    assert fresh.first_conv_type == "SD" and fresh.fuser_scales() == scale_after
    assert torch.equal(second, _hires(case, fresh, ae, "latent-bicubic"))
    assert not torch.equal(first, second)
    fresh._drop_engine()
    ae._drop_engine()


@pytest.mark.parametrize("image_batch", [2, 1])
def test_generate_init_image_is_encode_then_tail(image_batch, tmp_path, monkeypatch):
    """generate(init_image=, strength=) = autoencoder.encode, then the sampler's tail from that latent; a batch-1 image serves both samples."""
    import gligen_inference as gi
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    dev = _dev()
    monkeypatch.setattr(gi, "device", dev)
    case = _Case(dev, tmp_path, monkeypatch, [1, 0, 0])
    model, ae = case.model(), build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    image = (torch.rand(image_batch, 3, 2 * case.hw, 2 * case.hw, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(dev)
    x_T = syn.make_latent(case.B, 4, case.hw, case.hw, seed=6).to(dev)
    gen = lambda: gi.generate(model, ae, case.diffusion, _to(case.batch, dev), case.ctx.to(dev), case.uc.to(dev), starting_noise=x_T.clone(),
                              init_image=image, strength=0.6, **_gen_kwargs(case, steps=S2)).clone()
    torch.manual_seed(9)
    gen()                                                    # (tunes the shapes of this test)
    torch.manual_seed(9)
    got = gen()
    torch.manual_seed(9)
    lat0 = ae.encode(image)
    assert lat0.shape[0] == image_batch
    lat, sampler = case.run(model, DPMSolverSampler, S2, (case.B, 4, case.hw, case.hw), x_T.clone(), lat0, 0.6, "bicubic", ddim_discretize="logsnr")
    assert len(sampler.ddim_timesteps) == 6 and model.engine.sampler_timing()[2] == 6
    assert torch.equal(got, ae.decode(lat))
    # the start point itself: q_sample of the encoded image at the tail's first timestep with the given noise
    t0 = int(sampler.ddim_timesteps[-1])
    ts = torch.full((case.B,), t0, device=dev, dtype=torch.long)
    start = model.engine.latent_renoise(lat0.expand(case.B, -1, -1, -1), (case.hw, case.hw), "bicubic", float(case.diffusion.sqrt_alphas_cumprod[t0]),
                                        float(case.diffusion.sqrt_one_minus_alphas_cumprod[t0]), x_T)
    assert torch.equal(start, case.diffusion.q_sample(lat0.expand(case.B, -1, -1, -1), ts, x_T))
    model._drop_engine()
    ae._drop_engine()


def test_run_entry_hires_and_init_image(tmp_path, monkeypatch):
    """gligen_inference.run() from the config keys: hires_height / hires_width give images of that size, equal to generate() with the same
    seed; init_image + strength read the file through load_inpaint_image."""
    dev = _dev()
    import gligen_inference as gi
    from PIL import Image
    monkeypatch.setattr(gi, "device", dev)
    monkeypatch.chdir(tmp_path)
    B, hw = 2, 16
    cfg = gi.synthetic_config("text", image_size=hw)
    cfg["model"]["params"].update(syn.UNET_CFG_SMALL, image_size=hw, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"])
    cfg["autoencoder"]["params"]["ddconfig"] = syn.VAE_DDCONFIG_SMALL
    model = syn.fill_module_(gi.instantiate_from_config(cfg["model"]).eval(), 1234).to(dev)
    ae = syn.fill_module_(gi.instantiate_from_config(cfg["autoencoder"]).eval(), 4321).to(dev)
    diffusion = gi.instantiate_from_config(cfg["diffusion"]).to(dev)
    boxes, _ = syn.make_boxes(1, 2, seed=4)
    emb = syn.make_embeddings(1, 2, seed=4)[0, :2]
    meta = dict(ckpt="synthetic_text", prompt="x", save_folder_name="hires", locations=boxes[0, :2].tolist(), text_embeddings=list(emb),
                context=syn.make_context(B, seed=0), uc=syn.make_context(B, seed=1))
    args = dict(batch_size=B, guidance_scale=7.5, negative_prompt=None, no_plms=False, folder=str(tmp_path / "out"), steps=4, seed=3,
                sampler="dpmpp_2m", hires_height=HIRES_PX[0], hires_width=HIRES_PX[1], hires_steps=6, hires_strength=0.5, hires_upscaler="latent-bilinear")
    x_T = syn.make_latent(B, 4, hw, hw, seed=6).to(dev)
    samples = gi.run(meta, args, starting_noise=x_T.clone(), models=(model, ae, None, diffusion, cfg))
    assert sorted(os.listdir(tmp_path / "out" / "hires")) == ["0.png", "1.png"]
    assert tuple(samples.shape) == (B, 3) + HIRES_PX and torch.isfinite(samples).all()
    assert Image.open(tmp_path / "out" / "hires" / "1.png").size == (HIRES_PX[1], HIRES_PX[0])
    batch = gi.prepare_batch(meta, B)
    torch.cuda.manual_seed(3)
    direct = gi.generate(model, ae, diffusion, batch, meta["context"].to(dev), meta["uc"].to(dev), steps=4, guidance_scale=7.5, starting_noise=x_T.clone(),
                         sampler="dpmpp_2m", hires=HIRES_PX, hires_steps=6, hires_strength=0.5, hires_upscaler="latent-bilinear")
    assert torch.equal(direct, samples)
    assert model.__dict__["_hires"][(B, HIRES_PX[0] // 2, HIRES_PX[1] // 2)][0].engine.sampler_timing()[2] == 3
    # image-to-image from a file
    rgb = (torch.rand(40, 52, 3, generator=torch.Generator().manual_seed(2)) * 255).to(torch.uint8).numpy()
    Image.fromarray(rgb).save(tmp_path / "init.png")
    args2 = dict(batch_size=B, guidance_scale=7.5, negative_prompt=None, no_plms=False, folder=str(tmp_path / "out2"), steps=6, seed=3,
                 sampler="dpmpp_2m", init_image=str(tmp_path / "init.png"), strength=0.5)
    out2 = gi.run(meta, args2, starting_noise=x_T.clone(), models=(model, ae, None, diffusion, cfg))
    assert tuple(out2.shape) == (B, 3, 2 * hw, 2 * hw) and torch.isfinite(out2).all() and model.engine.sampler_timing()[2] == 3
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    image = gi.load_inpaint_image(str(tmp_path / "init.png"), size=(2 * hw, 2 * hw))
    assert tuple(image.shape) == (1, 3, 2 * hw, 2 * hw)
    model._drop_engine()
    ae._drop_engine()
