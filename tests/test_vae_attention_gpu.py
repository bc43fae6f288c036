"""The VAE's attention on a real MI355X: vae_attn_flash_kernel (single head, C = 256 | 512) beside the score-matrix form it replaces
above 4096 tokens, the mode switch (gl_vae_set_attention), and generate(height=, width=) at a non-square size.

Operator: float64 on the same bf16 values, an absolute bar derived from the kernels' rounding points and a relative bar against the
matrix form in the same run. In situ: both forms inside the small and the full autoencoder, against the reference's own output at a
non-square size (tests/golden/vae_small_24x40.npz, tools/make_golden_sizes.py) and against each other. End to end: the product's
generate() at 16 x 24 latents against a CPU loop around the oracle, which tests/test_vae_attention_cpu.py holds to the reference at
that size."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import ROOT, build_product_unet, build_product_vae, grounding_kwargs, load_golden, mse, oracle_cfg
from gligen_amd import synthetic as syn

pytestmark = pytest.mark.gpu

IMG_MSE_TOL = 2e-3      # tests/test_path_gpu.py: decoded image through ~30 bf16 layers
ENC_REL_TOL = 5e-3      # tests/test_path_gpu.py: test_vae_encode_vs_reference
EPS_MSE_TOL = 2e-4      # tests/test_path_gpu.py: one UNet evaluation
SAMPLER_TOL = 2e-3      # tests/test_path_gpu.py PLMS_TOL / tests/test_dpm_solver_gpu.py: relative MSE behind a sampling loop
REPORT = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    out = os.environ.get("GL_PARITY_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_report_vae_attention.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float(((a - b) ** 2).mean() / (b ** 2).mean())


# ---------------------------------------------------------------------------------------------------------------- operator
# The absolute bar (tests/test_clip_vision_gpu.py derives it for the same arithmetic). Both forms compute o = sum_j p^_j v_j / sum_j p_j
# with p^_j = bf16(p_j) (flash: of exp2(s_j - m); matrix: of the normalised p_j), fp32 sums, and store bf16(o). With u = 2^-9:
#   |sum_j p^_j v_j / sum p - o| <= u max_j |v_j|   (a convex combination of |v_j|, each weight off by <= u);  the final rounding adds
#   <= u |o| <= u max_j |v_j|;  the fp32 parts (C-term dot products, exp2, the running sum, one rescale per key tile) get u / 4.
U_BF16 = 2.0 ** -9
ABS_BAR = (2 + 0.25) * U_BF16
FLASH_VS_MATRIX = 1.5       # relative MSE of the flash form <= 1.5 x the matrix form's on the same inputs in the same run
OP_B = 2
OP_T = (64, 128, 192, 576)  # one key tile; two; an odd count; several (the running maximum and the LDS slots alternate)
OP_C = (256, 512)
OP_KINDS = ("flat", "dominant_last_tile", "rising_maxima")
_INPUTS, _REF, _OUT = {}, {}, {}


def _inputs(kind, T, C):
    """bf16 q, k, v [B][T][C], seeded. flat: scores of std ~0.06 around 0. dominant_last_tile: every query has one key in the LAST
    64-key tile whose score stands ~48 above the rest. rising_maxima: a shared direction makes every query's row maximum grow by
    ~0.125 sqrt(C) from one 64-key tile to the next, so the running maximum moves at every tile."""
    key = (kind, T, C)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * OP_KINDS.index(kind) + T + C)
        q = torch.randn((OP_B, T, C), generator=g) * 0.25
        k = torch.randn((OP_B, T, C), generator=g) * 0.25
        v = torch.randn((OP_B, T, C), generator=g)
        v[1] *= 3.0                                         # the two images differ in scale as well
        if kind == "dominant_last_tile":
            u = torch.randint(0, 2, (64, C), generator=g).float() * 2 - 1
            pick = torch.randint(0, 64, (OP_B, T), generator=g)
            k[:, T - 64:] = 4.0 * u
            q += u[pick] * (12.0 / C ** 0.5)
        elif kind == "rising_maxima":
            d = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
            q += 0.5 * d
            k += 0.25 * (torch.arange(T) // 64).float()[None, :, None] * d
        _INPUTS[key] = tuple(t.to(torch.bfloat16).contiguous() for t in (q, k, v))
    return _INPUTS[key]


def _reference(kind, T, C):
    key = (kind, T, C)
    if key not in _REF:
        q, k, v = (t.double() for t in _inputs(kind, T, C))
        s = q @ k.transpose(-1, -2) * C ** -0.5
        _REF[key] = (torch.softmax(s, dim=-1) @ v, v.abs().amax(dim=(1, 2)), s)
    return _REF[key]


@pytest.fixture(scope="module")
def op_engine():
    from gligen_amd.runtime import scratch_engine
    return scratch_engine(_dev())


def _run(eng, kind, T, C, mode):
    key = (kind, T, C, mode)
    if key not in _OUT:
        dev = _dev()
        q, k, v = (t.to(dev) for t in _inputs(kind, T, C))
        out = eng.vae_attention(q, k, v, mode=mode)
        torch.cuda.synchronize()
        _OUT[key] = out.cpu()
    return _OUT[key]


def test_the_input_kinds_are_what_they_claim():
    for C in OP_C:
        s = _reference("dominant_last_tile", 576, C)[2]
        top = s.argmax(dim=-1)
        assert bool((top >= 576 - 64).all()) and float((s.max(dim=-1).values - s[..., :512].max(dim=-1).values).min()) > 20
        s = _reference("rising_maxima", 576, C)[2]
        tile_max = s.reshape(OP_B, 576, 9, 64).amax(dim=-1)
        assert bool((tile_max[..., 1:] > tile_max[..., :-1] + 1.0).all())
        assert float(_reference("flat", 576, C)[2].abs().max()) < 1.0


@pytest.mark.parametrize("kind", OP_KINDS)
@pytest.mark.parametrize("T", OP_T)
@pytest.mark.parametrize("C", OP_C)
def test_operator_against_float64(C, T, kind, op_engine):
    ref, vmax, _ = _reference(kind, T, C)
    rec = {}
    for mode in ("matrix", "flash"):
        got = _run(op_engine, kind, T, C, mode).double()
        assert got.shape == ref.shape and bool(torch.isfinite(got).all())
        rec[mode] = dict(rel_mse=_rel(got, ref), max_abs_over_vmax=float(((got - ref).abs().amax(dim=(1, 2)) / vmax).max()))
    rec["abs_bar"], rec["rel_bar"] = ABS_BAR, FLASH_VS_MATRIX * rec["matrix"]["rel_mse"]
    REPORT[f"op_C{C}_T{T}_{kind}"] = rec
    print(json.dumps(rec))
    for mode in ("matrix", "flash"):
        assert rec[mode]["max_abs_over_vmax"] <= ABS_BAR, rec
    assert rec["flash"]["rel_mse"] <= rec["rel_bar"], rec


@pytest.mark.parametrize("mode", ["matrix", "flash"])
@pytest.mark.parametrize("C", OP_C)
def test_each_image_of_a_batch_gets_the_bits_it_gets_alone(C, mode, op_engine):
    dev = _dev()
    for T in (128, 576):
        both = _run(op_engine, "flat", T, C, mode)
        q, k, v = _inputs("flat", T, C)
        for b in range(OP_B):
            alone = op_engine.vae_attention(q[b:b + 1].to(dev), k[b:b + 1].to(dev), v[b:b + 1].to(dev), mode=mode).cpu()
            assert torch.equal(alone[0].view(torch.int16), both[b].view(torch.int16)), (C, T, b)


def test_auto_is_the_matrix_form_up_to_4096_tokens_and_modes_are_refused_by_name(op_engine):
    from gligen_amd import GligenAmdError
    dev = _dev()
    auto = op_engine.vae_attention(*(t.to(dev) for t in _inputs("flat", 576, 512)), mode="auto").cpu()
    assert torch.equal(auto.view(torch.int16), _run(op_engine, "flat", 576, 512, "matrix").view(torch.int16))
    x = torch.zeros((1, 64, 128), dtype=torch.bfloat16, device=dev)
    with pytest.raises(GligenAmdError, match="error 5.*C=128"):
        op_engine.vae_attention(x, x, x, mode="flash")
    assert op_engine.vae_attention(x, x, x, mode="matrix").shape == x.shape       # the matrix form takes any C % 64 == 0
    with pytest.raises(GligenAmdError, match="mode 3"):
        op_engine.vae_attention(x, x, x, mode=3)
    with pytest.raises(GligenAmdError, match="mode 7"):
        op_engine.set_vae_attention(7)
    y = torch.zeros((1, 96, 256), dtype=torch.bfloat16, device=dev)
    with pytest.raises(GligenAmdError, match="T=96"):
        op_engine.vae_attention(y, y, y, mode="flash")


# ---------------------------------------------------------------------------------------------------------------- full VAE
@pytest.fixture(scope="module")
def full_vae():
    ae = build_product_vae(syn.VAE_DDCONFIG, device=_dev())
    yield ae
    ae._drop_engine()


def _launches(eng, fn):
    a = eng.launch_count()
    out = fn()
    torch.cuda.synchronize()
    return out, eng.launch_count() - a


def test_flash_needs_no_buffer_that_grows_with_the_square_of_the_token_count(full_vae):
    """T = 4608, C = 512 on a fresh fork: the call may raise the arena's high-water mark by less than the bf16 P matrix ALONE would
    take (T^2 2 bytes = 42.5 MB); what it takes is v^T, 2 T C bytes = 4.7 MB."""
    dev = _dev()
    T, C = 4608, 512
    fork = full_vae.engine.fork(arena_gb=1.0)
    try:
        before = fork.memory()["arena_high_water"]
        g = torch.Generator().manual_seed(5)
        q, k, v = ((torch.randn((1, T, C), generator=g) * s).to(torch.bfloat16).to(dev) for s in (0.25, 0.25, 1.0))
        out = fork.vae_attention(q, k, v, mode="flash")
        torch.cuda.synchronize()
        rise = fork.memory()["arena_high_water"] - before
        REPORT["memory_T4608_C512"] = dict(rise_bytes=rise, p_matrix_bytes=T * T * 2)
        print(json.dumps(REPORT["memory_T4608_C512"]))
        assert 0 < rise < T * T * 2 and rise <= 2 * (2 * T * C), rise
        ref = torch.softmax(q[0].double() @ k[0].double().T * C ** -0.5, dim=-1) @ v[0].double()
        assert float((out[0].double() - ref).abs().max() / v.double().abs().max()) <= ABS_BAR
    finally:
        fork.close()


def test_full_vae_above_4096_tokens_takes_the_flash_kernel_and_agrees_with_the_matrix_form(full_vae):
    """A 72 x 64 latent (4608 tokens, 576 x 512 pixels). Under auto the per-image score GEMM, softmax and P v GEMM are one launch."""
    dev = _dev()
    eng = full_vae.engine
    z = (syn.make_latent(1, 4, 72, 64, seed=31) * 0.18215 * 4).to(dev)
    try:
        eng.set_vae_attention("matrix")
        full_vae.decode(z)                                   # (tunes the shapes of this size: launch counts are of tuned runs)
        img_m, n_m = _launches(eng, lambda: full_vae.decode(z))
        eng.set_vae_attention("auto")
        full_vae.decode(z)
        img_a, n_a = _launches(eng, lambda: full_vae.decode(z))
        eng.set_vae_attention("flash")
        img_f, n_f = _launches(eng, lambda: full_vae.decode(z))
    finally:
        eng.set_vae_attention("auto")
    REPORT["full_72x64"] = dict(launches_matrix=n_m, launches_auto=n_a, img_mse=mse(img_a, img_m), img_var=float(img_m.var()))
    print(json.dumps(REPORT["full_72x64"]))
    assert img_a.shape == (1, 3, 576, 512) and bool(torch.isfinite(img_a).all())
    assert n_a == n_f and 2 <= n_m - n_a <= 4, (n_m, n_a, n_f)      # S GEMM + softmax + P v GEMM (+ their split-K reductions) -> one kernel
    assert torch.equal(img_a, img_f)
    assert mse(img_a, img_m) < IMG_MSE_TOL, REPORT["full_72x64"]
    assert mse(img_a, img_m) < 1e-3 * float(img_m.var())            # (and relative to the image, not only to the absolute bar)


def test_full_vae_at_64x64_is_bit_for_bit_the_matrix_form_under_auto(full_vae):
    dev = _dev()
    eng = full_vae.engine
    z = (syn.make_latent(1, 4, 64, 64, seed=32) * 0.18215 * 4).to(dev)
    try:
        eng.set_vae_attention("matrix")
        full_vae.decode(z)
        img_m, n_m = _launches(eng, lambda: full_vae.decode(z))
        eng.set_vae_attention("auto")
        img_a, n_a = _launches(eng, lambda: full_vae.decode(z))
    finally:
        eng.set_vae_attention("auto")
    assert n_a == n_m and torch.equal(img_a, img_m)


# ---------------------------------------------------------------------------------------------------------------- small VAE, 24 x 40
def _mgs():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_sizes", os.path.join(ROOT, "tools", "make_golden_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_vae_at_24x40_against_the_reference_in_both_forms(monkeypatch):
    """960 tokens, C = 256. Decode and encode under the matrix form and under the flash form are the reference's (the bars of
    tests/test_path_gpu.py); auto at this size is the matrix form: the same bits from the same number of launches. Every form runs once
    untimed first (the run that tunes a shape's GEMM tiles differs from later ones by rounding)."""
    dev = _dev()
    g = load_golden("vae_small_24x40")
    ae = build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    eng = ae.engine
    z, x = _mgs().vae_inputs(syn, torch)
    noise = torch.from_numpy(g["noise"])
    monkeypatch.setattr(torch, "randn", lambda *a, **k: noise.clone())      # the one posterior draw, as recorded
    out, rec = {}, {}
    try:
        for mode in ("matrix", "flash", "auto"):
            eng.set_vae_attention(mode)
            ae.decode(z.to(dev)), ae.encode(x.to(dev))
            (img, zenc), n = _launches(eng, lambda: (ae.decode(z.to(dev)), ae.encode(x.to(dev))))
            out[mode] = (img.cpu(), zenc.cpu(), n)
            rec[mode] = dict(img_mse=mse(img, g["img"]), z_rel_mse=mse(zenc, g["z"]) / float(g["z"].var()), launches=n)
    finally:
        eng.set_vae_attention("auto")
        monkeypatch.undo()
        ae._drop_engine()
    REPORT["vae_small_24x40"] = rec
    print(json.dumps(rec))
    for mode in ("matrix", "flash", "auto"):
        assert out[mode][0].shape == (2, 3, 48, 80) and out[mode][1].shape == (2, 4, 24, 40)
        assert rec[mode]["img_mse"] < IMG_MSE_TOL and rec[mode]["z_rel_mse"] < ENC_REL_TOL, rec
    assert torch.equal(out["auto"][0], out["matrix"][0]) and torch.equal(out["auto"][1], out["matrix"][1]) and out["auto"][2] == out["matrix"][2]
    assert out["flash"][2] < out["matrix"][2] and not torch.equal(out["flash"][0], out["matrix"][0])


# ---------------------------------------------------------------------------------------------------------------- end to end, 16 x 24
E2E_H, E2E_W = 16, 24          # latent cells; the small VAE has factor 2: 32 x 48 pixels


def _oracle_parts(inpaint, batch, ctx, uc, extra):
    from oracle import gligen_oracle as orc
    from helpers import golden_shapes
    sd = syn.seeded_state_dict(golden_shapes("unet_small_inpaint" if inpaint else "unet_small_text"), 1234)
    gk = grounding_kwargs("text", batch)
    gnull = orc.null_grounding("text", gk)
    cfg = oracle_cfg(syn.UNET_CFG_SMALL, "text")

    def eps_fn(x, t, cond, scale):
        inp = dict(x=x.float(), timesteps=t, context=ctx if cond else uc, grounding_input=gk if cond else gnull, inpainting_extra_input=extra)
        with torch.no_grad():
            return orc.unet_forward(sd, cfg, inp, fuser_scale=scale)
    vsd = syn.seeded_state_dict(golden_shapes("vae_small"), 4321)
    dd = syn.VAE_DDCONFIG_SMALL
    vcfg = dict(ch_mult=dd["ch_mult"], num_res_blocks=dd["num_res_blocks"], scale_factor=0.18215)
    return orc, eps_fn, vsd, vcfg


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def test_generate_at_a_non_square_size_text_model():
    """Small text UNet + small VAE, 16 x 24 latent (32 x 48 pixels), B = 2, 4 PLMS steps, guidance 7.5 through generate(height=, width=):
    one evaluation against the reference's eps (unet_small_text_16x24), the final image against PLMS around the CPU oracle + its decode."""
    import gligen_inference as gi
    from ldm.models.diffusion.ldm import LatentDiffusion
    dev = _dev()
    mg = _mgs()
    g = load_golden("unet_small_text_16x24")
    model = build_product_unet(syn.UNET_CFG_SMALL, "text", device=dev)
    ae = build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    try:
        batch, x, ctx, t = mg.unet_inputs(syn, torch)
        gin = model.grounding_tokenizer_input.prepare(_to(batch, dev))
        eps = model(dict(x=x.to(dev), timesteps=t.to(dev), context=ctx.to(dev), grounding_input=gin, inpainting_extra_input=None, grounding_extra_input=None))
        rec = dict(eps_mse=mse(eps, g["eps"]))
        assert eps.shape == (2, 4, E2E_H, E2E_W) and rec["eps_mse"] < EPS_MSE_TOL, rec

        uc, x_T = syn.make_context(2, seed=9), syn.make_latent(2, 4, E2E_H, E2E_W, seed=6)
        diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).to(dev)
        img = gi.generate(model, ae, diffusion, _to(batch, dev), ctx.to(dev), uc.to(dev), steps=4, guidance_scale=7.5, starting_noise=x_T.to(dev),
                          height=2 * E2E_H, width=2 * E2E_W)
        orc, eps_fn, vsd, vcfg = _oracle_parts(False, batch, ctx, uc, None)
        lat = orc.plms_sample(eps_fn, x_T, 4, orc.make_schedule(), 7.5, alphas=orc.alpha_generator(4, None))
        with torch.no_grad():
            ref = orc.vae_decode(vsd, vcfg, lat)
        rec.update(img_rel_mse=mse(img, ref) / float(ref.var()), img_std=float(ref.std()))
        REPORT["e2e_text_16x24"] = rec
        print(json.dumps(rec))
        assert img.shape == (2, 3, 2 * E2E_H, 2 * E2E_W) and rec["img_rel_mse"] < SAMPLER_TOL, rec
        with pytest.raises(ValueError, match="multiple of 4 "):
            gi.generate(model, ae, diffusion, _to(batch, dev), ctx.to(dev), uc.to(dev), steps=4, height=34)
    finally:
        model._drop_engine()
        ae._drop_engine()


def test_generate_at_a_non_square_size_inpainting_model(monkeypatch):
    """The same size through the inpainting model: a rectangular mask from the boxes, z0 = encode of a 48 x 32 (width x height) image.
    z0 is held to the oracle's encode at the encode bar; the sampling loop (the device's z0, scripted q_sample draws) to PLMS around the
    oracle at the sampler bar, in the latent and in the decoded image."""
    import gligen_inference as gi
    from ldm.models.diffusion.ldm import LatentDiffusion
    from helpers import scripted_randn_like
    dev = _dev()
    model = build_product_unet(syn.UNET_CFG_SMALL, "text", True, device=dev)
    ae = build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    try:
        batch = syn.make_batch("text", 2, n_valid=3, seed=1)
        ctx, uc, x_T = syn.make_context(2, seed=1), syn.make_context(2, seed=9), syn.make_latent(2, 4, E2E_H, E2E_W, seed=6)
        mask = gi.draw_masks_from_boxes(batch["boxes"], (E2E_H, E2E_W))
        assert mask.shape == (2, 1, E2E_H, E2E_W) and 0 < float(mask.sum()) < mask.numel()
        image = torch.rand(1, 3, 2 * E2E_H, 2 * E2E_W, generator=torch.Generator().manual_seed(28)) * 2 - 1
        draw = torch.randn((1, 4, E2E_H, E2E_W), generator=torch.Generator().manual_seed(99))
        monkeypatch.setattr(torch, "randn", lambda *a, **k: draw.clone())
        z0 = ae.encode(image.to(dev))
        monkeypatch.undo()
        step_noise = torch.randn((4, 1, 4, E2E_H, E2E_W), generator=torch.Generator().manual_seed(77))
        extra = torch.cat([z0.cpu() * mask, mask], dim=1)
        orc, eps_fn, vsd, vcfg = _oracle_parts(True, batch, ctx, uc, extra)
        with torch.no_grad():
            z0_ref = orc.vae_encode(vsd, vcfg, image, draw)
        rec = dict(z0_rel_mse=mse(z0, z0_ref) / float(z0_ref.var()))
        assert z0.shape == (1, 4, E2E_H, E2E_W) and rec["z0_rel_mse"] < ENC_REL_TOL, rec

        diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).to(dev)
        monkeypatch.setattr(torch, "randn_like", scripted_randn_like(step_noise.to(dev)))
        img = gi.generate(model, ae, diffusion, _to(batch, dev), ctx.to(dev), uc.to(dev), steps=4, guidance_scale=7.5, starting_noise=x_T.to(dev),
                          inpainting_mask=mask.to(dev), z0=z0, height=2 * E2E_H, width=2 * E2E_W)
        monkeypatch.undo()
        lat = orc.plms_sample(eps_fn, x_T, 4, orc.make_schedule(), 7.5, alphas=orc.alpha_generator(4, None), mask=mask, x0=z0.cpu(), noise=step_noise)
        with torch.no_grad():
            ref = orc.vae_decode(vsd, vcfg, lat)
        rec.update(img_rel_mse=mse(img, ref) / float(ref.var()), img_std=float(ref.std()))
        REPORT["e2e_inpaint_16x24"] = rec
        print(json.dumps(rec))
        assert img.shape == (2, 3, 2 * E2E_H, 2 * E2E_W) and rec["img_rel_mse"] < SAMPLER_TOL, rec
    finally:
        monkeypatch.undo()
        model._drop_engine()
        ae._drop_engine()
