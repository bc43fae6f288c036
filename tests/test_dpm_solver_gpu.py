"""The solver loop on a real MI355X: solver_update_kernel by itself against float64, DPM-Solver++ (order 1 against the reference's own
DDIM goldens, 2M against the float64 loop of tests/dpm_solver_ref.py around the CPU oracle UNet), stochastic DDIM, the state the
samplers share, and gligen_inference.run() with the new sampler. Small UNet, the latent size and batch of the *_unet_small goldens."""
import json
import math
import os
from functools import partial

import numpy as np
import pytest
import torch

import dpm_solver_ref as ref
from helpers import build_product_unet, golden_shapes, grounding_kwargs, load_golden, mse, oracle_cfg, scripted_randn_like
from gligen_amd import synthetic as syn

pytestmark = pytest.mark.gpu

PLMS_TOL = 2e-3        # relative MSE of the final latent: the bar of tests/test_path_gpu.py::test_plms_vs_reference
ALPHA_TYPE = [0.3, 0.0, 0.7]
REPORT = {}


@pytest.fixture(autouse=True)
def _report(record_property):
    """What a test measured goes into pytest's report: a property of the test (--junitxml) and a line of its output (-s / -rP)."""
    before = set(REPORT)
    yield
    for key in sorted(set(REPORT) - before):
        record_property(key, json.dumps(REPORT[key], sort_keys=True))
        print(f"[dpm solver] {key}: {json.dumps(REPORT[key], sort_keys=True)}")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _replay(noise):
    """torch.randn_like that hands out noise[0], noise[1], ... in call order."""
    it = iter(noise)

    def fn(like, *a, **k):
        out = next(it).to(like)
        assert tuple(out.shape) == tuple(like.shape), (out.shape, like.shape)
        return out
    return fn


def _rel(a, b):
    b = torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).float().cpu()
    return mse(a, b) / float(b.var())


# ---- 1: the kernel alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guidance", [None, 7.5], ids=["noguidance", "g7.5"])
@pytest.mark.parametrize("n", [2 * 4 * 16 * 16, 1 * 4 * 7 * 9, 1 * 4 * 7 * 9 + 3, 3])
def test_solver_update_kernel(engine, n, guidance):
    """gl_op_solver_update against float64 over 0 / 1 / 2 history terms, with and without noise, in place and out of place. n: a
    multiple of 4 over several blocks (128-bit path), 252 (vector path, one block), 255 (vector path + scalar tail; with guidance the
    uncond half is then misaligned: scalar fallback) and 3 (scalar only). Per element
    |err| <= 4e-6 (|cx x| + (|c0| / alpha)(|x| + sigma (|e_u| + g (|e_c| + |e_u|))) + |c1 D1| + |c2 D2| + |cn z|): a dozen fp32 roundings of
    2^-24 each plus fp32 coefficients, margin about 5; the history slot holds D0 within the same bound."""
    dev = engine.device
    g = torch.Generator().manual_seed(n)
    rnd = lambda *s: torch.randn(*s, generator=g)
    # a 2M step of a 10-step run on the SD schedule (from the formulas, not the product's table), a third term and a noise term
    ts, a_ts, a_prevs = ref.uniform_grid(10, ref.sd_alphas_cumprod())
    i = 4
    a_t = float(a_ts[i])
    h = float(ref.lam(a_prevs[i]) - ref.lam(a_ts[i]))
    r = float(ref.lam(a_ts[i]) - ref.lam(a_ts[i - 1])) / h
    phi = -math.sqrt(a_prevs[i]) * math.expm1(-h)
    cx, c0, c1, c2, cn = math.sqrt((1 - a_prevs[i]) / (1 - a_t)), phi * (1 + 0.5 / r), -phi * 0.5 / r, 0.11, 0.37
    alpha, sigma = math.sqrt(a_t), math.sqrt(1 - a_t)
    worst = 0.0
    for nh in (0, 1, 2):
        for noise in (False, True):
            for inplace in (False, True):
                eps = rnd(2 if guidance is not None else 1, n)
                x, d1, d2, z = rnd(n), rnd(n), rnd(n), rnd(n)
                xd = x.to(dev)
                out, d0 = engine.op_solver_update(eps.to(dev).contiguous(), xd, a_t, cx, c0, guidance=guidance,
                                                  d1=d1.to(dev) if nh >= 1 else None, c1=c1 if nh >= 1 else 0.0,
                                                  d2=d2.to(dev) if nh >= 2 else None, c2=c2 if nh >= 2 else 0.0,
                                                  z=z.to(dev) if noise else None, cn=cn if noise else 0.0, out=xd if inplace else None)
                assert (out.data_ptr() == xd.data_ptr()) == inplace
                if not inplace:
                    assert torch.equal(xd.cpu(), x)
                X, E = x.double(), eps.double()
                if guidance is not None:
                    e = E[1] + guidance * (E[0] - E[1])
                    e_abs = E[1].abs() + guidance * (E[0].abs() + E[1].abs())
                else:
                    e, e_abs = E[0], E[0].abs()
                D0 = (X - sigma * e) / alpha
                want = cx * X + c0 * D0
                bound = (cx * X).abs() + (abs(c0) / alpha) * (X.abs() + sigma * e_abs)
                if nh >= 1:
                    want, bound = want + c1 * d1.double(), bound + (c1 * d1.double()).abs()
                if nh >= 2:
                    want, bound = want + c2 * d2.double(), bound + (c2 * d2.double()).abs()
                if noise:
                    want, bound = want + cn * z.double(), bound + (cn * z.double()).abs()
                bound = 4e-6 * bound
                err_x, err_d = (out.cpu().double() - want).abs(), (d0.cpu().double() - D0).abs()
                worst = max(worst, float((err_x / bound).max()), float((err_d / bound).max()))
                assert (err_x <= bound).all(), (nh, noise, inplace, float((err_x / bound).max()))
                assert (err_d <= bound).all(), (nh, noise, inplace, float((err_d / bound).max()))
    REPORT[f"kernel_n{n}_{'g' if guidance else 'nog'}"] = dict(worst_err_over_bound=worst)


def test_solver_update_kernel_refusals(engine):
    from gligen_amd import GligenAmdError
    dev = engine.device
    x, eps = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    with pytest.raises(GligenAmdError, match="d2 without d1"):
        engine.op_solver_update(eps, x, 0.5, 1.0, 1.0, d2=x.clone(), c2=1.0)
    with pytest.raises(GligenAmdError, match="a_t = 1.5"):
        engine.op_solver_update(eps, x, 1.5, 1.0, 1.0)


# ---- the sampler cases ----------------------------------------------------------------------------------------------------------------
class _Case:
    """The fixture of the *_unet_small goldens (tests/test_path_gpu.py::test_plms_vs_reference): seeded small UNet, text grounding, guidance
    7.5 against an unconditional context, optionally the inpainting model."""

    def __init__(self, dev, tmp_path, monkeypatch, inpaint=False, alpha_type=ALPHA_TYPE, x0_batch=None):
        from ldm.models.diffusion.ldm import LatentDiffusion
        from oracle.gligen_oracle import draw_masks_from_boxes
        g = load_golden("ddim_unet_small_inpaint" if inpaint else "ddim_unet_small")
        self.golden, meta = g, g["meta"]
        self.dev, self.inpaint, self.alpha_type = dev, inpaint, alpha_type
        self.B, self.hw, self.n_valid = meta["B"], meta["hw"], meta["n_valid"]
        self.tmp_path, self.monkeypatch = tmp_path, monkeypatch
        torch.save(syn.sd_first_conv_state(), tmp_path / "SD_input_conv_weight_bias.pth")
        monkeypatch.chdir(tmp_path)
        self.diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).to(dev)
        self.batch = syn.make_batch("text", self.B, n_valid=self.n_valid, seed=1)
        self.ctx, self.uc = syn.make_context(self.B, seed=1), syn.make_context(self.B, seed=9)
        self.x_T = syn.make_latent(self.B, 4, self.hw, self.hw, seed=6)
        self.mask = self.z0 = self.extra = None
        if inpaint:
            nb = x0_batch or self.B
            self.mask = draw_masks_from_boxes(self.batch["boxes"][:nb], self.hw)
            self.z0 = syn.make_latent(nb, 4, self.hw, self.hw, seed=2)
            self.extra = torch.cat([self.z0 * self.mask, self.mask], dim=1).expand(self.B, -1, -1, -1).contiguous()

    def model(self):
        return build_product_unet(syn.UNET_CFG_SMALL, "text", self.inpaint, device=self.dev)

    def run(self, model, cls, S, use_graph=True, randn_like=None, eta=None, **schedule_kwargs):
        """sampler.sample of `cls` on `model`; randn_like: the stand-in for torch.randn_like during the run."""
        from gligen_inference import alpha_generator, set_alpha_scale
        dev = self.dev
        gin = model.grounding_tokenizer_input.prepare(_to(self.batch, dev))
        sampler = cls(self.diffusion, model, alpha_generator_func=partial(alpha_generator, type=self.alpha_type), set_alpha_scale=set_alpha_scale)
        sampler.use_graph = use_graph
        if eta is not None:
            sampler.ddim_eta = eta
        to = lambda t: None if t is None else t.to(dev)
        inp = dict(x=self.x_T.to(dev), timesteps=None, context=self.ctx.to(dev), grounding_input=gin, inpainting_extra_input=to(self.extra),
                   grounding_extra_input=None)
        if randn_like is not None:
            self.monkeypatch.setattr(torch, "randn_like", randn_like)
        out = sampler.sample(S=S, shape=(self.B, 4, self.hw, self.hw), input=inp, uc=self.uc.to(dev), guidance_scale=7.5, mask=to(self.mask),
                             x0=to(self.z0), **schedule_kwargs)
        self.monkeypatch.undo()
        self.monkeypatch.chdir(self.tmp_path)
        return out.clone()

    def oracle(self):
        """(eps_fn, on_gate_off, sched) of the CPU oracle UNet with the same seeded weights."""
        import oracle.gligen_oracle as orc
        sd = syn.seeded_state_dict(golden_shapes("unet_small_inpaint" if self.inpaint else "unet_small_text"), 1234)
        gk = grounding_kwargs("text", self.batch)
        gnull = orc.null_grounding("text", gk)
        cfg = oracle_cfg(syn.UNET_CFG_SMALL, "text")

        def eps_fn(x, t, cond, scale):
            inp = dict(x=x.float(), timesteps=t, context=self.ctx if cond else self.uc, grounding_input=gk if cond else gnull,
                       inpainting_extra_input=self.extra)
            with torch.no_grad():
                return orc.unet_forward(sd, cfg, inp, fuser_scale=scale)

        def swap_in_sd_first_conv():
            if not self.inpaint:
                sdc = syn.sd_first_conv_state()
                sd["input_blocks.0.0.weight"], sd["input_blocks.0.0.bias"] = sdc["weight"], sdc["bias"]
        sched = {k: v.astype(np.float64) for k, v in orc.make_schedule().items()}
        return eps_fn, swap_in_sd_first_conv, sched


@pytest.fixture(scope="module", autouse=True)
def _warm_process(tmp_path_factory):
    """One untimed pass of the committed DDIM loop on each model before anything here compares runs bit for bit. The engine tunes GEMM
    tiles and times its kernel forms at the first eager launch of a shape, process-wide, and the run that does the tuning differs from
    every later run of the process by bf16 rounding (1e-3 of the latent's range; measured with the committed DDIM loop alone, first
    against second run of a fresh process). tests/test_path_gpu.py gets the same warm-up from the UNet tests in front of its sampler test."""
    if not torch.cuda.is_available():
        yield
        return
    from ldm.models.diffusion.ddim import DDIMSampler
    mp = pytest.MonkeyPatch()
    try:
        for inpaint in (False, True):
            case = _Case(torch.device("cuda:0"), tmp_path_factory.mktemp("warm"), mp, inpaint=inpaint)
            model = case.model()
            case.run(model, DDIMSampler, 5, use_graph=False, randn_like=_replay(torch.zeros(64, case.B, 4, case.hw, case.hw)) if inpaint else None)
            model._drop_engine()
    finally:
        mp.undo()
    yield


def test_order_one_against_ddim_goldens(tmp_path, monkeypatch):
    """DPM-Solver++ of order 1 on the uniform grid IS DDIM with eta 0: through gl_sample_solver against the reference's own DDIM goldens."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    dev = _dev()
    for inpaint in (False, True):
        name = "ddim_unet_small_inpaint" if inpaint else "ddim_unet_small"
        g = load_golden(name)
        case = _Case(dev, tmp_path, monkeypatch, inpaint=inpaint, alpha_type=g["meta"]["alpha_type"])
        S = g["meta"]["S"]
        noise = torch.from_numpy(g["noise"]).to(dev) if inpaint else None
        outs = []
        for use_graph in (False, True):
            model = case.model()
            outs.append(case.run(model, DPMSolverSampler, S, use_graph, randn_like=_replay(noise) if inpaint else None, order=1))
            model._drop_engine()
        model = case.model()
        ddim = case.run(model, DDIMSampler, S, randn_like=scripted_randn_like(noise, multistep=False) if inpaint else None)
        model._drop_engine()
        rel, rel_ddim = _rel(outs[0], g["x_out"]), _rel(outs[0], ddim)
        REPORT[f"order1_{name}"] = dict(x_rel_mse=rel, rel_mse_to_ddim_sampler=rel_ddim)
        assert rel < PLMS_TOL and rel_ddim < PLMS_TOL, REPORT[f"order1_{name}"]
        assert torch.equal(outs[0], outs[1]), "hipGraph replay must reproduce the eager launch sequence bit for bit"


_REFS = {}


def _reference_2m(case, S, grid):
    """The float64 2M loop around the CPU oracle UNet: computed once per (S, grid), shared, never modified."""
    key = (S, grid, case.inpaint)
    if key not in _REFS:
        from gligen_inference import alpha_generator
        eps_fn, gate_off, sched = case.oracle()
        the_grid = (ref.uniform_grid if grid == "uniform" else ref.logsnr_grid)(S, sched["alphas_cumprod"])
        _REFS[key] = ref.dpm_sample(eps_fn, case.x_T, the_grid, sched, 7.5, alphas=alpha_generator(S, case.alpha_type), on_gate_off=gate_off).float()
    return _REFS[key]


@pytest.mark.parametrize("grid", ["uniform", "logsnr"])
@pytest.mark.parametrize("S", [5, 10])
def test_2m_against_float64_loop(S, grid, tmp_path, monkeypatch):
    """S = 5 takes the lower-order final step, S = 10 does not; alpha schedule [0.3, 0, 0.7] with the SD first-conv swap."""
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    dev = _dev()
    case = _Case(dev, tmp_path, monkeypatch)
    outs = []
    for use_graph in (False, True):
        model = case.model()
        outs.append(case.run(model, DPMSolverSampler, S, use_graph, ddim_discretize=grid))
        model._drop_engine()
    rel = _rel(outs[0], _reference_2m(case, S, grid))
    REPORT[f"2m_S{S}_{grid}"] = dict(x_rel_mse=rel)
    assert rel < PLMS_TOL, rel
    assert torch.equal(outs[0], outs[1]), "hipGraph replay must reproduce the eager launch sequence bit for bit"


def test_2m_inpainting_broadcast(tmp_path, monkeypatch):
    """Mask and x0 of batch 1 broadcast over the latent batch, scripted q_sample noise of batch 1."""
    from gligen_inference import alpha_generator
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    dev = _dev()
    S = 5
    case = _Case(dev, tmp_path, monkeypatch, inpaint=True, x0_batch=1)
    assert case.B == 2 and case.mask.shape[0] == 1 and case.z0.shape[0] == 1
    noise = torch.randn(S, 1, 4, case.hw, case.hw, generator=torch.Generator().manual_seed(21))
    model = case.model()
    out = case.run(model, DPMSolverSampler, S, randn_like=_replay(noise.to(dev)), ddim_discretize="logsnr")
    model._drop_engine()
    eps_fn, gate_off, sched = case.oracle()
    want = ref.dpm_sample(eps_fn, case.x_T, ref.logsnr_grid(S, sched["alphas_cumprod"]), sched, 7.5, alphas=alpha_generator(S, case.alpha_type),
                          mask=case.mask, x0=case.z0, noise=noise, on_gate_off=gate_off)
    rel = _rel(out, want.float())
    REPORT["2m_inpaint_b1"] = dict(x_rel_mse=rel)
    assert rel < PLMS_TOL, rel


def test_samplers_share_state_without_leaking(tmp_path, monkeypatch):
    """PLMS, 2M, stochastic DDIM and 2M again on ONE model: both 2M results are a fresh model's bit for bit, and so is the PLMS result."""
    from ldm.models.diffusion.ddim import StochasticDDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    dev = _dev()
    case = _Case(dev, tmp_path, monkeypatch, alpha_type=None)       # (no first-conv swap: the model stays what a fresh one is)
    S = 5
    model = case.model()
    plms = case.run(model, PLMSSampler, S)
    first = case.run(model, DPMSolverSampler, S, ddim_discretize="logsnr")
    torch.manual_seed(5)
    eta = case.run(model, StochasticDDIMSampler, S, eta=0.5)
    second = case.run(model, DPMSolverSampler, S, ddim_discretize="logsnr")
    model._drop_engine()
    fresh = case.model()
    fresh_2m = case.run(fresh, DPMSolverSampler, S, ddim_discretize="logsnr")
    fresh._drop_engine()
    fresh = case.model()
    fresh_plms = case.run(fresh, PLMSSampler, S)
    fresh._drop_engine()
    assert torch.isfinite(eta).all() and not torch.equal(eta, first)
    assert torch.equal(first, second) and torch.equal(first, fresh_2m)
    assert torch.equal(plms, fresh_plms)


def test_ddim_eta_native(tmp_path, monkeypatch):
    """DDIM with eta = 0.5 on the device against the reference's p_sample_ddim in float64 around the oracle UNet, same scripted noise; with a
    seeded generator two runs are bit-identical."""
    from gligen_inference import alpha_generator
    from ldm.models.diffusion.ddim import StochasticDDIMSampler
    dev = _dev()
    case = _Case(dev, tmp_path, monkeypatch)
    S = 5
    z = torch.randn(S, case.B, 4, case.hw, case.hw, generator=torch.Generator().manual_seed(22))
    model = case.model()
    out = case.run(model, StochasticDDIMSampler, S, randn_like=_replay(z.to(dev)), eta=0.5)
    model._drop_engine()
    eps_fn, gate_off, sched = case.oracle()
    grid = ref.uniform_grid(S, sched["alphas_cumprod"])
    sig = ref.ddim_eta_sigmas(grid[1], grid[2], 0.5)
    want = ref.ddim_eta_sample(eps_fn, case.x_T, grid, sig, z, sched, 7.5, alphas=alpha_generator(len(grid[0]), case.alpha_type), on_gate_off=gate_off)
    rel = _rel(out, want.float())
    REPORT["ddim_eta0.5"] = dict(x_rel_mse=rel)
    assert rel < PLMS_TOL, rel
    seeded = []
    for _ in range(2):
        model = case.model()
        torch.manual_seed(77)
        seeded.append(case.run(model, StochasticDDIMSampler, S, eta=0.5))
        model._drop_engine()
    assert torch.equal(seeded[0], seeded[1]) and not torch.equal(seeded[0], out)


def test_run_entry_dpmpp_2m(tmp_path, monkeypatch):
    """gligen_inference.run() with sampler="dpmpp_2m" on the log-SNR grid: finite images, u8 files, bit-equal to generate() with the same
    seed; a config without the new keys runs PLMS, as it always did."""
    dev = _dev()
    import gligen_inference as gi
    from PIL import Image
    from ldm.models.diffusion.plms import PLMSSampler
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
    meta = dict(ckpt="synthetic_text", prompt="x", save_folder_name="dpm", locations=boxes[0, :2].tolist(), text_embeddings=list(emb),
                context=syn.make_context(B, seed=0), uc=syn.make_context(B, seed=1))
    args = dict(batch_size=B, guidance_scale=7.5, negative_prompt=None, no_plms=False, folder=str(tmp_path / "out"), steps=4,
                sampler="dpmpp_2m", discretize="logsnr")
    x_T = syn.make_latent(B, 4, hw, hw, seed=6).to(dev)
    samples = gi.run(meta, args, starting_noise=x_T.clone(), models=(model, ae, None, diffusion, cfg))
    assert sorted(os.listdir(tmp_path / "out" / "dpm")) == ["0.png", "1.png"]
    assert samples.shape == (B, 3, 2 * hw, 2 * hw) and torch.isfinite(samples).all()
    png = np.asarray(Image.open(tmp_path / "out" / "dpm" / "1.png"))
    expect = (torch.clamp(samples[1], -1, 1) * 0.5 + 0.5).cpu().numpy().transpose(1, 2, 0) * 255
    assert np.array_equal(png, expect.astype(np.uint8))
    batch = gi.prepare_batch(meta, B)
    direct = gi.generate(model, ae, diffusion, batch, meta["context"].to(dev), meta["uc"].to(dev), steps=4, guidance_scale=7.5,
                         starting_noise=x_T.clone(), sampler="dpmpp_2m", discretize="logsnr")
    assert torch.equal(direct, samples)
    # without the new keys: PLMS
    old = {k: v for k, v in args.items() if k not in ("sampler", "discretize")}
    old["folder"] = str(tmp_path / "out_plms")
    plms = gi.run(meta, old, starting_noise=x_T.clone(), models=(model, ae, None, diffusion, cfg))
    sampler = PLMSSampler(diffusion, model, alpha_generator_func=partial(gi.alpha_generator, type=None), set_alpha_scale=gi.set_alpha_scale)
    inp = dict(x=x_T.clone(), timesteps=None, context=meta["context"].to(dev), grounding_input=model.grounding_tokenizer_input.prepare(_to(batch, dev)),
               inpainting_extra_input=None, grounding_extra_input=None)
    latents = sampler.sample(S=4, shape=(B, 4, hw, hw), input=inp, uc=meta["uc"].to(dev), guidance_scale=7.5)
    assert torch.equal(plms, ae.decode(latents)) and not torch.equal(plms, samples)
    with pytest.raises(ValueError, match="logsnr"):
        gi.sampler_choice(None, False, "logsnr", 0.0)
    model._drop_engine()
    ae._drop_engine()
