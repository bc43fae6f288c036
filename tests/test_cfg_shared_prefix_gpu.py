"""The guidance pair's shared prefix (gl_set_cfg_shared_prefix, Engine::unet_forward) on a real MI355X.

Inside the sampler the [cond ; uncond] halves of an evaluation get the same latent, extra first-conv input and timestep, so the
layers in front of the first one that reads conditioning run once, at the latent batch. Every test samples with the switch off and
on in one process, with the kernel-form policy in a static mode (the same kernels in every run), and compares the final latents:

* against the committed reference golden where its shapes fit (B = 2), at the sampler tests' bar, and on-vs-off closer than
  off-vs-golden: the two forms differ by a reordered sum at most (another GEMM tile at the smaller M), a wrong sample index is O(1);
* against the off run elsewhere (xB = 1 and 3: odd, and more than one sample per half).

The prefix's GEMMs and convs are planned as their full-batch forms (gemm.h gemm_set_plan_batch_scale: the same kernel family, tile
and K split), so a prefix row has the bits it has without sharing. Measured on MI355X: on and off are bit-identical in every case
here (relative MSE 0.0), both forms sit 1.25e-4 / 1.47e-4 from the two goldens. Before that rule the tuner planned the smaller
problem on its own, the forms differed in last bits (9e-8 after one step), and the seeded random-weight fixtures amplified that to
the bf16-vs-fp32 level within three steps (on vs off 1.8e-4 .. 2.6e-4, above off-vs-golden): the checks below caught it.
"""
import functools
import os
import re
import tempfile
from functools import partial

import pytest
import torch

from helpers import build_product_unet, load_golden, mse, scripted_randn_like
from gligen_amd import synthetic as syn

pytestmark = pytest.mark.gpu

PLMS_TOL = 2e-3        # relative MSE of the final latent: the bar of tests/test_path_gpu.py::test_plms_vs_reference
EPS_MSE_TOL = 2e-4     # absolute MSE: the bar of tests/test_configs_gpu.py's [cond ; uncond] pair cases


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


@pytest.fixture()
def switches():
    """Policy mode and sharing are process-wide: whatever a test sets is put back."""
    yield []
    from gligen_amd import _lib
    lib = _lib.load()
    assert lib.gl_set_ff_rows_policy(-1) == 0 and lib.gl_set_cfg_shared_prefix(1) == 0


def _counters(eng):
    m = re.search(r"cfg_shared_prefix=(\d) evals=(\d+) rows_at_prefix=(\d+) rows_periodic=(\d+)", eng.ff_rows_policy_report())
    assert m, eng.ff_rows_policy_report()
    return tuple(int(v) for v in m.groups())


def _sample(model, B, hw, S, use_graph, dev, *, alpha_type=None, inpaint=False, noise=None, perm=None, seed_x=6):
    """One CFG sampling run of `model` as tests/test_path_gpu.py::test_plms_vs_reference issues it. perm: a permutation of the samples
    applied to the latent and to every conditioning tensor."""
    from gligen_inference import alpha_generator, set_alpha_scale
    from ldm.models.diffusion.ldm import LatentDiffusion
    from ldm.models.diffusion.plms import PLMSSampler
    from oracle.gligen_oracle import draw_masks_from_boxes
    diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).to(dev)
    batch = syn.make_batch("text", B, n_valid=3, seed=1)
    ctx, uc = syn.make_context(B, seed=1).to(dev), syn.make_context(B, seed=9).to(dev)
    x = syn.make_latent(B, 4, hw, hw, seed=seed_x).to(dev)          # a distinct latent per sample
    gin = model.grounding_tokenizer_input.prepare(_to(batch, dev))
    mask = z0 = extra = None
    if inpaint:
        mask = draw_masks_from_boxes(batch["boxes"], hw).to(dev)
        z0 = syn.make_latent(B, 4, hw, hw, seed=2).to(dev)
        extra = torch.cat([z0 * mask, mask], dim=1)
    if perm is not None:
        p = torch.as_tensor(perm, device=dev)
        x, ctx, uc = x[p], ctx[p], uc[p]
        gin = {k: (v[p] if torch.is_tensor(v) and v.shape[:1] == (B,) else v) for k, v in gin.items()}
    sampler = PLMSSampler(diffusion, model, alpha_generator_func=None if alpha_type is None else partial(alpha_generator, type=alpha_type),
                          set_alpha_scale=set_alpha_scale)
    sampler.use_graph = use_graph
    inp = dict(x=x, timesteps=None, context=ctx, grounding_input=gin, inpainting_extra_input=extra, grounding_extra_input=None)
    torch.manual_seed(11)               # the q_sample draws of an inpainting run: the same in every run
    with pytest.MonkeyPatch.context() as mp:
        if noise is not None:           # ... or the golden's recorded ones
            mp.setattr(torch, "randn_like", scripted_randn_like(noise.to(dev)))
        if 1000 % S:
            # the reference's uniform discretisation (util.py make_ddim_timesteps: range(0, 1000, 1000 // S) + 1) has S + 1 entries
            # when S does not divide 1000, the last one past the schedule: a 3-step run takes the first three (1, 334, 667)
            import ldm.models.diffusion.plms as plms_mod
            real = plms_mod.make_ddim_timesteps
            mp.setattr(plms_mod, "make_ddim_timesteps", lambda **k: real(**k)[:S])
        return sampler.sample(S=S, shape=(B, 4, hw, hw), input=inp, uc=uc, guidance_scale=7.5, mask=mask, x0=z0).clone()


def _rel(a, b):
    return mse(a, b) / float(b.float().var())


def _off_on_small(inpaint):
    """xB = 1 and 3, 3 PLMS steps, eager and graph, no golden of these shapes: on against off."""
    dev = _dev()
    model = build_product_unet(syn.UNET_CFG_SMALL, "text", inpaint, device=dev)
    eng = model.engine
    eng.set_ff_rows_policy(0)           # the row-local kernels off: the generic path, o and t0 replicated by the copy kernel
    figures = {}
    try:
        for B in (1, 3):
            for use_graph in (False, True):
                out = {}
                for on in (False, True):
                    eng.set_cfg_shared_prefix(on)
                    before = _counters(eng)
                    out[on] = _sample(model, B, 16, 3, use_graph, dev, inpaint=inpaint)
                    after = _counters(eng)
                    assert (after[1] > before[1]) == on, (before, after)          # evaluations that shared
                    assert after[2] == before[2] and after[3] == before[3]        # ... and never through the row-local kernel here
                figures[(B, use_graph)] = _rel(out[True], out[False])
                print("on vs off", B, use_graph, figures[(B, use_graph)])
    finally:
        model._drop_engine()
    for k, v in figures.items():
        assert v < PLMS_TOL, (k, v)


@functools.lru_cache(maxsize=None)
def _golden_runs(golden_name, inpaint):
    """The golden's own run (B = 2, its step count and alpha schedule: the fusers are gated off for the middle steps and the SD first
    conv is swapped in, so each run gets a fresh model), sharing off and on, eager and graph. Computed once, shared by the tests
    below: {use_graph: (off vs golden, on vs golden, on vs off)}."""
    dev = _dev()
    g = load_golden(golden_name)
    meta = g["meta"]
    noise = torch.from_numpy(g["noise"]) if inpaint else None
    ref = torch.from_numpy(g["x_out"])
    figures = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        torch.save(syn.sd_first_conv_state(), os.path.join(tmp, "SD_input_conv_weight_bias.pth"))   # restore_first_conv_from_SD reads the cwd
        os.chdir(tmp)
        try:
            for use_graph in (False, True):
                out = {}
                for on in (False, True):
                    model = build_product_unet(syn.UNET_CFG_SMALL, "text", inpaint, device=dev)
                    model.engine.set_ff_rows_policy(0)
                    model.engine.set_cfg_shared_prefix(on)
                    out[on] = _sample(model, meta["B"], meta["hw"], meta["S"], use_graph, dev, alpha_type=meta["alpha_type"], inpaint=inpaint, noise=noise)
                    model._drop_engine()
                figures[use_graph] = (_rel(out[False], ref), _rel(out[True], ref), _rel(out[True], out[False]))
                print("golden", golden_name, use_graph, "off", figures[use_graph][0], "on", figures[use_graph][1], "on vs off", figures[use_graph][2])
        finally:
            os.chdir(cwd)
    return figures


GOLDEN_CASES = [("plms_unet_small", False), ("plms_unet_small_inpaint", True)]


def test_generic_path_small_unet(switches):
    """The committed small text config, row-local kernels off, 3 PLMS steps with CFG, eager and graph, xB = 1 and 3, on against off;
    and the plms_unet_small golden's own run (B = 2, 5 steps, alpha schedule 0.6 / 0 / 0.4): both forms meet the sampler bar."""
    _off_on_small(False)
    for use_graph, (r_off, r_on, _) in _golden_runs(*GOLDEN_CASES[0]).items():
        assert r_off < PLMS_TOL and r_on < PLMS_TOL, (use_graph, r_off, r_on)


def test_inpainting_small_unet(switches):
    """The same on the 9-channel first conv: the masked latent + mask are one tensor for both halves."""
    _off_on_small(True)
    for use_graph, (r_off, r_on, _) in _golden_runs(*GOLDEN_CASES[1]).items():
        assert r_off < PLMS_TOL and r_on < PLMS_TOL, (use_graph, r_off, r_on)


@pytest.mark.parametrize("golden_name,inpaint", GOLDEN_CASES)
def test_on_vs_off_is_closer_than_off_vs_golden(golden_name, inpaint, switches):
    """The issue's second criterion on the golden runs: the relative MSE between the two forms is smaller than the off run's against
    the golden (measured: 0.0 against 1.25e-4 and 1.47e-4)."""
    for use_graph, (r_off, r_on, r_pair) in _golden_runs(golden_name, inpaint).items():
        assert r_pair < r_off, (use_graph, r_off, r_on, r_pair)


@pytest.fixture(scope="module")
def shipped_model():
    model = build_product_unet(syn.UNET_CFG, "text", False, device=_dev())
    yield model
    model._drop_engine()


@pytest.mark.parametrize("B", [1, 3])
def test_fast_path_shipped_topology(B, shipped_model, switches):
    """The shipped topology with the row-local kernels forced on, at the smallest latent qkv_rows_supported takes at both batches
    (16 x 16: T = 256 rows per sample, a multiple of 128; M = 256 B and 512 B), 2 PLMS steps. attn1's projection runs at the
    prefix batch and the fuser's projection reads its prefix-batch inputs through the input period: the counters say so.
    Measured on MI355X: bit-identical on vs off at both batches."""
    dev = _dev()
    eng = shipped_model.engine
    switches.append(eng)
    eng.set_ff_rows_policy(1)
    for use_graph in (False, True):
        out = {}
        for on in (False, True):
            eng.set_cfg_shared_prefix(on)
            before = _counters(eng)
            out[on] = _sample(shipped_model, B, 16, 2, use_graph, dev)
            after = _counters(eng)
            if on:
                assert after[0] == 1 and after[1] > before[1] and after[2] > before[2] and after[3] > before[3], (before, after)
            else:
                assert after[0] == 0 and after[1:] == before[1:], (before, after)
        d = mse(out[True], out[False])
        print("fast path on vs off", B, use_graph, d, _rel(out[True], out[False]))
        assert d < EPS_MSE_TOL, (B, use_graph, d)


def test_swapped_samples_swap_the_output_bit_for_bit(switches):
    """xB = 2 with sharing on: two latents, then the same two swapped together with their conditioning rows. Sample b of the
    full-batch layers reads prefix sample b % 2: any other index shows as a different output, not as rounding."""
    dev = _dev()
    model = build_product_unet(syn.UNET_CFG_SMALL, "text", False, device=dev)
    eng = model.engine
    switches.append(eng)
    try:
        for mode in (1, 0):             # the row-local launch with the input period, then the copy kernel
            eng.set_ff_rows_policy(mode)
            eng.set_cfg_shared_prefix(True)
            before = _counters(eng)
            a = _sample(model, 2, 16, 2, False, dev)
            b = _sample(model, 2, 16, 2, False, dev, perm=[1, 0])
            after = _counters(eng)
            assert after[1] > before[1] and (after[3] > before[3]) == (mode == 1), (mode, before, after)
            assert not torch.equal(a[0], a[1])
            assert torch.equal(a[0], b[1]) and torch.equal(a[1], b[0]), (mode, mse(a[0], b[1]), mse(a[1], b[0]))
    finally:
        model._drop_engine()


def test_gated_off_fusers_take_the_copy_path(switches, tmp_path, monkeypatch):
    """fuser_scale 0 for the later steps (alpha schedule 0.4 / 0 / 0.6) with the row-local kernels forced on: the first step's fuser
    projection reads through the input period, the gated-off steps have no such launch and replicate o and t0 instead."""
    dev = _dev()
    torch.save(syn.sd_first_conv_state(), tmp_path / "SD_input_conv_weight_bias.pth")
    monkeypatch.chdir(tmp_path)
    out = {}
    for on in (False, True):
        model = build_product_unet(syn.UNET_CFG_SMALL, "text", False, device=dev)
        eng = model.engine
        eng.set_ff_rows_policy(1)
        eng.set_cfg_shared_prefix(on)
        before = _counters(eng)
        out[on] = _sample(model, 3, 16, 4, True, dev, alpha_type=[0.4, 0.0, 0.6])
        after = _counters(eng)
        assert (after[1] > before[1]) == on and (after[3] > before[3]) == on, (before, after)
        model._drop_engine()
    r = _rel(out[True], out[False])
    print("gated off, on vs off", r)
    assert r < PLMS_TOL, r
