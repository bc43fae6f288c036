"""The training run on the device: the fused AdamW + EMA kernel (gl_op_adamw_ema_step) against gl_op_adamw_step bit for bit and
against the float64 EMA, TrainStep with an EMA in both schedules, the Trainer's resume (exact), its checkpoint crossing over to a
real torch.optim.AdamW and to the inference model, an inpainting and a canny model through the loop, and the in-training preview.
Everything runs on the small UNet of tests/golden/unet_small_train_2steps.npz: its config, B = 2, its 16 x 16 latent."""
import json
import os

import pytest
import torch

from helpers import GOLDEN, build_product_unet, build_product_vae, load_golden
from gligen_amd import synthetic as syn
from gligen_amd.train import TrainStep, trainable_names

pytestmark = pytest.mark.gpu

META = load_golden("unet_small_train_2steps")["meta"]
CFG = dict(META["cfg"], grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=False)
B, HW = META["B"], META["hw"]
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
GRID_CAP, BLOCK, PER_LANE = 16384, 256, 4          # adamw_ema_kernel's launch (train_optim.hip)
ABOVE_CAP = 2 * GRID_CAP * BLOCK * PER_LANE + 7   # two full grid-strides of the 16-byte path plus 7 elements
BOUND = 2.0 ** -22                                # |ema - ref| <= 2^-22 max(|ema_old|, |p_new|): three fp32 roundings of quantities bounded
                                                  # by that maximum, 2^-24 each, plus the rounding of 1 - rate


def fixture():
    return json.load(open(os.path.join(GOLDEN, "trainable_order.json")))


def guarded(src, off):
    """`src` [n] copied into the middle of a longer device tensor: (the whole tensor, its view of n elements `off` elements in)."""
    n = src.numel()
    whole = torch.full((off + n + 8,), 12345.0, device=src.device)
    whole[off:off + n] = src
    return whole, whole[off:off + n]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 100003, ABOVE_CAP])
def test_fused_kernel_gives_adamws_bits(engine, n):
    """p, m, v after op_adamw_ema_step are torch.equal to op_adamw_step on copies, over three steps with weight_decay = 0.01: with
    16-byte aligned tensors (the float4 path and its scalar tail), with every tensor a [1:] view of a longer one (a 4-byte offset:
    the scalar path), and with only `ema` misaligned. Elements in front of and past the n are untouched."""
    assert engine.ADAMW_EMA_GRID == (GRID_CAP, BLOCK, PER_LANE)
    dev = engine.device
    gen = torch.Generator(device=dev).manual_seed(n)
    rnd = lambda: torch.randn(n, generator=gen, device=dev)
    p0, m0, v0, e0 = rnd(), rnd() * 0.1, rnd().abs() * 0.01, rnd()
    grads = [rnd() for _ in range(3)]
    ref = [p0.clone(), m0.clone(), v0.clone()]
    layouts = {"aligned": (0, 0), "all at a 4-byte offset": (1, 1), "ema at a 4-byte offset": (0, 1)}
    runs = {k: [guarded(t, off_e if i == 3 else off) for i, t in enumerate((p0, m0, v0, e0))] for k, (off, off_e) in layouts.items()}
    for step, g in enumerate(grads, 1):
        engine.op_adamw_step(ref[0], g, ref[1], ref[2], step, **HYPER)
        for name, (off, _) in layouts.items():
            (_, p), (_, m), (_, v), (_, e) = runs[name]
            gw, gv = guarded(g, off)
            assert (p.data_ptr() % 16 != 0) == bool(off) and (e.data_ptr() % 16 != 0) == bool(layouts[name][1]) and gv.data_ptr() % 16 == 4 * off
            engine.op_adamw_ema_step(p, gv, m, v, e, step, ema_rate=0.9, **HYPER)
            assert torch.equal(gv, g)
            for got, want, what in ((p, ref[0], "p"), (m, ref[1], "m"), (v, ref[2], "v")):
                assert torch.equal(got, want), (name, what, step, int((got != want).sum()))
    for name, (off, off_e) in layouts.items():
        for i, (whole, view) in enumerate(runs[name]):
            o = off_e if i == 3 else off
            assert bool((whole[:o] == 12345.0).all()) and bool((whole[o + n:] == 12345.0).all()) and whole.numel() == o + n + 8, (name, i)
    # the EMA of the three layouts: the same bits (one arithmetic on the 16-byte and on the scalar path)
    assert torch.equal(runs["aligned"][3][1], runs["all at a 4-byte offset"][3][1]) and torch.equal(runs["aligned"][3][1], runs["ema at a 4-byte offset"][3][1])
    assert not torch.equal(runs["aligned"][3][1], e0)


@pytest.mark.parametrize("rate", [0.9999, 0.5, 0.0, 1.0])
def test_fused_kernel_ema_value(engine, rate):
    """ema = rate ema + (1 - rate) p_new against float64 on the fp32-rounded rate, |ema - ref| <= 2^-22 max(|ema_old|, |p_new|) element
    by element, on the 16-byte path with its tail and on the scalar path; rate 0 gives ema == p_new exactly, rate 1 leaves ema alone."""
    from gligen_amd import _lib
    dev = engine.device
    n = 100003
    gen = torch.Generator(device=dev).manual_seed(17)
    rnd = lambda: torch.randn(n, generator=gen, device=dev)
    p0, g, m0, v0, e0 = rnd(), rnd(), rnd() * 0.1, rnd().abs() * 0.01, rnd() * 3
    r = float(torch.tensor(rate, dtype=torch.float32))
    for off in (0, 1):
        (_, p), (_, gv), (_, m), (_, v), (_, e) = (guarded(t, off) for t in (p0, g, m0, v0, e0))
        engine.op_adamw_ema_step(p, gv, m, v, e, 1, ema_rate=rate, **HYPER)
        assert not torch.equal(p, p0)
        ref = r * e0.double() + (1.0 - r) * p.double()
        err = (e.double() - ref).abs()
        bound = BOUND * torch.maximum(e0.abs(), p.abs()).double()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"ema rate {rate} offset {off}: worst |ema - ref| / bound = {worst:.3f}")
        assert bool((err <= bound).all()), (rate, off, worst)
        if rate == 0.0:
            assert torch.equal(e, p)
        if rate == 1.0:
            assert torch.equal(e, e0)
    # refused by the library, by name
    (_, p), (_, gv), (_, m), (_, v), (_, e) = (guarded(t[:8], 0) for t in (p0, g, m0, v0, e0))
    for bad in (dict(ema_rate=1.5), dict(ema_rate=-0.1), dict(ema_rate=float("nan"))):
        with pytest.raises(_lib.GligenAmdError, match="ema_rate"):
            engine.op_adamw_ema_step(p, gv, m, v, e, 1, **dict(HYPER, **bad))
    with pytest.raises(_lib.GligenAmdError, match="step"):
        engine.op_adamw_ema_step(p, gv, m, v, e, 0, ema_rate=0.5, **HYPER)
    assert torch.equal(p, p0[:8]) and torch.equal(e, e0[:8])


def small_state_dict(cfg=CFG, seed=None):
    """Seeded weights of the small UNet in module order (the values of every other test of this model: the fill is per key)."""
    from gligen_amd.trainer import synthetic_state_dict
    return synthetic_state_dict(cfg, META["weight_seed"] if seed is None else seed)


def golden_batch():
    b = syn.make_batch("text", B, n_valid=META["n_valid"], seed=5)
    return dict(x=syn.make_latent(B, 4, HW, HW, seed=6), timesteps=torch.tensor([981, 441][:B]).float(), context=syn.make_context(B, seed=6),
                boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"], target=syn.make_latent(B, 4, HW, HW, seed=7))


def test_train_step_with_ema(engine):
    """Three steps at ema_rate = 0.5 on the golden batch: ema_state_dict() follows the float64 recurrence over the three parameter
    snapshots within three times the per-step bound for every trainable tensor, the frozen tensors are the parameters, the parameters
    are those of a run without an EMA bit for bit, and the one-stream schedule gives the same EMA bits."""
    sd, batch = small_state_dict(), golden_batch()
    names = trainable_names(sd, CFG)
    assert len(names) == 127

    def run(**kw):
        ts = TrainStep(engine, CFG, sd, lr=META["lr"], weight_decay=0.01, bucket_mb=32.0, world=1, **kw)
        snaps = []
        for _ in range(3):
            ts.step(batch)
            snaps.append({k: ts.params[k].clone() for k in names})
        torch.cuda.synchronize()
        return ts, snaps

    ts, snaps = run(ema_rate=0.5)
    assert len(ts.ema) == len(ts.pbuf.buckets) >= 4
    ema = ts.ema_state_dict()
    assert list(ema) == list(sd)
    worst = 0.0
    for k in sd:
        if k not in snaps[0]:
            assert torch.equal(ema[k], ts.params[k]) and torch.equal(ema[k].cpu(), sd[k]), k
            continue
        ref = sd[k].to(engine.device).double()
        scale = torch.zeros_like(ref)
        for s in snaps:
            scale = torch.maximum(scale, torch.maximum(ref.abs(), s[k].double().abs()))
            ref = 0.5 * ref + 0.5 * s[k].double()
        err = (ema[k].double() - ref).abs()
        bound = 3 * BOUND * scale
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (k, float(err.max()))
        assert not torch.equal(ema[k], snaps[-1][k]), k
    print("TrainStep EMA over three steps: worst |ema - float64 recurrence| / (3 x bound) =", round(worst, 4))
    plain, psnaps = run()
    assert plain.ema is None
    for a, b in zip(snaps, psnaps):
        assert all(torch.equal(a[k], b[k]) for k in a)
    one, osnaps = run(ema_rate=0.5, overlap=False)
    oema = one.ema_state_dict()
    assert all(torch.equal(ema[k], oema[k]) for k in ema), [k for k in ema if not torch.equal(ema[k], oema[k])][:5]
    assert all(torch.equal(snaps[-1][k], osnaps[-1][k]) for k in snaps[-1])
    # the inverse: the EMA into a fresh step's buffers
    ts.load_ema_state_dict({k: torch.zeros_like(v) for k, v in ema.items()})
    assert all(float(ts.ema_state_dict()[k].abs().sum()) == 0.0 for k in names)
    ts.load_ema_state_dict(ema)
    assert all(torch.equal(ts.ema_state_dict()[k], ema[k]) for k in ema)
    engine.train_weight_cache(False)


def run_config(out, **kw):
    return dict(dict(model=CFG, base_learning_rate=1e-3, weight_decay=0.01, warmup_steps=3, scheduler_type="constant", total_iters=4, enable_ema=True,
                     ema_rate=0.9, inpaint_mode=False, save_every_iters=1000, output_dir=str(out), ckpt=None), **kw)


def text_batches(start):
    from gligen_amd.trainer import synthetic_batches
    return synthetic_batches("text", B, HW, start=start, seed=3, n_valid=META["n_valid"])


def full_state(tr):
    """(parameters, EMA, both AdamW moments) of a Trainer, on the CPU."""
    torch.cuda.synchronize()
    cpu = lambda d: {k: v.detach().cpu() for k, v in d.items()}
    o = tr.ts.optimizer_state_dict()
    return dict(model=cpu(tr.ts.state_dict()), ema=cpu(tr.ts.ema_state_dict()), exp_avg=cpu(o["exp_avg"]), exp_avg_sq=cpu(o["exp_avg_sq"]))


@pytest.fixture(scope="module")
def runs(engine, tmp_path_factory):
    """The Trainer runs the resume and the cross-over test share (computed once, never written): A, four iterations in one go; B, two
    iterations and save(); C, a new Trainer(resume=file) on a fresh engine context, two more, with the third iteration's gradients
    and parameters kept; D, A's run from another seed."""
    from gligen_amd.engine import Engine
    from gligen_amd.trainer import Trainer, read_checkpoint
    out = tmp_path_factory.mktemp("trainer")
    sd = small_state_dict()
    quiet = lambda s: None
    r = {}
    a = Trainer(engine, run_config(out / "a"), sd, text_batches, seed=11, resume=False, log=quiet)
    for _ in range(4):
        a.run_one_step(next(a.batches))
    r["A"], r["A_losses"] = full_state(a), [float(l) for l in a.losses]
    del a
    b = Trainer(engine, run_config(out / "b"), sd, text_batches, seed=11, resume=False, log=quiet)
    for _ in range(2):
        b.run_one_step(next(b.batches))
    r["B_losses"] = [float(l) for l in b.losses]
    r["file"] = b.save()
    r["files"] = sorted(os.listdir(out / "b"))
    del b
    engine.train_weight_cache(False)
    r["ckpt"] = read_checkpoint(r["file"])
    fresh = Engine(0, arena_gb=6.0)
    try:
        c = Trainer(fresh, run_config(out / "elsewhere"), sd, text_batches, seed=999, resume=r["file"], log=quiet)
        r["C_start"] = (c.starting_iter, c.ts.steps)
        c.run_one_step(next(c.batches))
        torch.cuda.synchronize()
        r["grads3"] = {k: v.detach().cpu().clone() for k, v in c.ts.gbuf.views.items()}
        r["params3"] = {k: c.ts.params[k].detach().cpu().clone() for k in c.ts.gbuf.views}
        r["order"] = list(c.ts.param_order)
        c.run_one_step(next(c.batches))
        r["C"], r["C_losses"] = full_state(c), [float(l) for l in c.losses]
        del c
    finally:
        fresh.train_weight_cache(False)
        fresh.close()
    d = Trainer(engine, run_config(out / "d"), sd, text_batches, seed=12, resume=False, log=quiet)
    for _ in range(4):
        d.run_one_step(next(d.batches))
    r["D_losses"] = [float(l) for l in d.losses]
    del d
    engine.train_weight_cache(False)
    return r


def test_resume_is_exact(runs):
    """Four iterations in one go against two, save(), a new Trainer(resume=file) on a fresh engine context and two more: every
    parameter, every EMA tensor, both AdamW moments and the four losses are torch.equal -- the step has no float atomics, so anything
    less means something was not restored. The same seed gives the same four losses (the run in two pieces is one), another seed
    gives others."""
    assert runs["files"] == ["checkpoint_00000002.pth", "checkpoint_latest.pth"] and runs["C_start"] == (2, 2)
    assert len(runs["A_losses"]) == 4 and runs["B_losses"] + runs["C_losses"] == runs["A_losses"], (runs["A_losses"], runs["B_losses"], runs["C_losses"])
    for part in ("model", "ema", "exp_avg", "exp_avg_sq"):
        bad = [k for k in runs["A"][part] if not torch.equal(runs["A"][part][k], runs["C"][part][k])]
        assert not bad, (part, len(bad), bad[:5])
    assert len(runs["A"]["exp_avg"]) == 127 and len(runs["A"]["model"]) == 413
    assert all(l == l and abs(l) < 1e4 for l in runs["A_losses"] + runs["D_losses"])
    assert all(a != d for a, d in zip(runs["A_losses"], runs["D_losses"])), (runs["A_losses"], runs["D_losses"])
    moved = [k for k in runs["A"]["ema"] if k in runs["A"]["exp_avg"] and not torch.equal(runs["A"]["ema"][k], runs["A"]["model"][k])]
    assert len(moved) == 127                    # the EMA is an average, not a copy


def test_checkpoint_crosses_over(runs):
    """The file written after two iterations: the reference's keys; ckpt["opt"] loads into a real torch.optim.AdamW built on the CPU
    over ckpt["model"]'s trainable tensors in the fixture's order, and one further torch step from the Trainer's third-iteration
    gradients matches the Trainer's third iteration at rtol 1e-5, atol 1e-6; ckpt["model"] and ckpt["ema"] load with strict=True into
    the inference model."""
    ck = runs["ckpt"]
    assert set(ck) == {"model", "diffusion", "opt", "scheduler", "iters", "config_dict", "ema", "rng"} and ck["iters"] == 2
    order = fixture()["small_text"]["trainable"]
    assert runs["order"] == order and [k for k in ck["model"] if k in set(order)] == order
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in ck["model"].values())
    params = [ck["model"][k].clone().requires_grad_(True) for k in order]
    opt = torch.optim.AdamW(params, lr=123.0, weight_decay=0.5)         # (the saved group's hyper-parameters replace these)
    opt.load_state_dict(ck["opt"])
    g0 = opt.param_groups[0]
    assert g0["weight_decay"] == 0.01 and tuple(g0["betas"]) == (0.9, 0.999) and g0["lr"] == pytest.approx(1e-3 * 2 / 3)      # warm-up over 3: the third step's rate
    assert all(float(opt.state[p]["step"]) == 2 and opt.state[p]["exp_avg"].shape == p.shape for p in params)
    for p, k in zip(params, order):
        p.grad = runs["grads3"][k]
    opt.step()
    for p, k in zip(params, order):
        torch.testing.assert_close(p.detach(), runs["params3"][k], rtol=1e-5, atol=1e-6, msg=lambda m, k=k: f"{k}: {m}")
    assert any(not torch.equal(runs["params3"][k], ck["model"][k]) for k in order)
    assert ck["scheduler"]["last_epoch"] == 2 and ck["scheduler"]["_last_lr"] == [g0["lr"]]
    model = build_product_unet(CFG, "text")
    model.load_state_dict(ck["model"], strict=True)
    model.load_state_dict(ck["ema"], strict=True)


def test_inpainting_and_canny_models_through_the_loop(engine):
    """Two iterations of an inpainting model (the 4-channel starting weights zero-extended by five channels, boxes through
    train_step_inputs) and one of the small canny model: finite losses, every trainable tensor moves, and the first conv's weight
    sits in `opt` at the index the fixture gives it."""
    from gligen_amd.trainer import Trainer, synthetic_batches
    fx = fixture()
    def canny_batches(start):
        for b in synthetic_batches("canny", B, HW, start=start, seed=4, map_res=128):
            b["mask"][1] = 0.0              # the second sample's map is dropped: its tokens are the null feature, which then has a gradient
            yield b

    cases = [("small_text_inpaint", 2, dict(inpaint_mode=True), lambda s: synthetic_batches("text", B, HW, start=s, seed=4, n_valid=3)),
             ("small_canny", 1, dict(), canny_batches)]
    for entry, iters, extra, batches in cases:
        cfg = fx[entry]["cfg"]
        sd = small_state_dict(dict(cfg, inpaint_mode=False))
        assert sd["input_blocks.0.0.weight"].shape[1] == (4 if entry == "small_text_inpaint" else 12)
        tr = Trainer(engine, run_config("unused", model=cfg, enable_ema=False, total_iters=iters, warmup_steps=0, **extra), sd, batches, seed=5, resume=False, log=lambda s: None)
        before = {k: v.clone() for k, v in tr.ts.state_dict().items()}
        assert tuple(before["input_blocks.0.0.weight"].shape)[1] == (9 if entry == "small_text_inpaint" else 12)
        for _ in range(iters):
            tr.run_one_step(next(tr.batches))
        torch.cuda.synchronize()
        losses = [float(l) for l in tr.losses]
        assert len(losses) == iters and all(l == l and 0 < l < 1e4 for l in losses), (entry, losses)
        after = tr.ts.state_dict()
        order = fx[entry]["trainable"]
        assert tr.ts.param_order == order
        for k in before:
            assert torch.equal(before[k], after[k]) != (k in set(order)), (entry, k)
        i = order.index("input_blocks.0.0.weight")
        opt = tr.ts.torch_optimizer_state_dict()
        assert opt["param_groups"][0]["params"] == list(range(len(order)))
        assert tuple(opt["state"][i]["exp_avg"].shape) == tuple(after["input_blocks.0.0.weight"].shape) and float(opt["state"][i]["step"]) == iters
        assert float(opt["state"][i]["exp_avg"].abs().sum()) > 0
        if entry == "small_text_inpaint":
            assert i == 0 and all(torch.count_nonzero(after["input_blocks.0.0.weight"][:, c]) > 0 for c in range(4, 9))
        del tr
        engine.train_weight_cache(False)


def test_preview(engine):
    """With the small VAE and 4 PLMS steps, preview() after one training iteration on images returns u8 [B, f hw, f hw, 3] (f: the
    autoencoder's factor -- 2 for the small VAE's two levels, 8 for the shipped one), and the images equal what the inference model
    gives when loaded from the checkpoint's `model` dict with the same x_T."""
    from gligen_amd.trainer import Trainer
    from ldm.models.diffusion.plms import PLMSSampler
    dev = engine.device
    vae = build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    f = 2 ** (len(syn.VAE_DDCONFIG_SMALL["ch_mult"]) - 1)

    def batches(start):
        i = start
        while True:
            g = torch.Generator().manual_seed(40 + i)
            yield dict(image=torch.rand(B, 3, f * HW, f * HW, generator=g) * 2 - 1, context=syn.make_context(B, seed=i), **syn.make_batch("text", B, n_valid=3, seed=i))
            i += 1

    tr = Trainer(engine, run_config("unused", enable_ema=False, warmup_steps=0), small_state_dict(), batches, autoencoder=vae, seed=5, resume=False, log=lambda s: None)
    tr.run_one_step(next(tr.batches))
    batch = next(tr.batches)
    x_T = syn.make_latent(B, 4, HW, HW, seed=21)
    try:
        imgs = tr.preview(batch, steps=4, guidance_scale=5, x_T=x_T)
        assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == (B, f * HW, f * HW, 3) and imgs.is_cuda
        ck = tr.state()
        assert any(not torch.equal(ck["model"][k], v) for k, v in small_state_dict().items())       # (the iteration moved the parameters)
        assert "autoencoder" in ck and set(ck["autoencoder"]) == set(vae.state_dict())
        model = build_product_unet(CFG, "text", device=dev)
        model.load_state_dict({k: v.to(dev) for k, v in ck["model"].items()}, strict=True)
        try:
            to = lambda m: {k: v.to(dev) for k, v in m.items()}
            inp = dict(x=x_T.to(dev), timesteps=None, context=batch["context"].to(dev), inpainting_extra_input=None, grounding_extra_input=None,
                       grounding_input=model.grounding_tokenizer_input.prepare(to({k: v for k, v in batch.items() if k != "image"})))
            samples = PLMSSampler(tr.diffusion, model).sample(S=4, shape=(B, 4, HW, HW), input=inp, uc=torch.zeros_like(inp["context"]), guidance_scale=5)
            ref = vae.engine.to_uint8(torch.clamp(vae.decode(samples), min=-1, max=1))
        finally:
            model._drop_engine()
        assert torch.equal(imgs, ref), int((imgs != ref).sum())
        assert int(imgs.float().std()) > 0
    finally:
        if tr._preview_model is not None:
            tr._preview_model._drop_engine()
        vae._drop_engine()
        engine.train_weight_cache(False)
