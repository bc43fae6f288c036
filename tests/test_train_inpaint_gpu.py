"""Training the inpainting models on the device: gl_unet_train_step with inpaint_mode (the 9-channel first conv and its weight
gradient) against the reference's loss.backward() (tools/make_golden_train_inpaint.py) and autograd through the CPU oracle, and the
step-input kernel (gl_train_step_inputs: q_sample, box mask, z * mask, concatenation, one launch) against the torch restatement that
tests/test_train_inpaint_cpu.py holds to the reference bit for bit."""
import pytest
import torch

from helpers import golden_shapes, load_golden, oracle_cfg
from gligen_amd import synthetic as syn
from gligen_amd.train import add_input_channels, trainable_names
from test_train_inpaint_cpu import (CASES, FIRST_CONV, N_TRAINABLE, box_mask, golden_inputs, inpaint_shapes, oracle_autograd, reference_batch,
                                    restate_step_inputs, schedule)
from test_train_spatial_cpu import golden_report, rel_mse

pytestmark = pytest.mark.gpu

_STEP, _ROWS, _TWO = {}, {}, {}       # device results shared between the tests of this module (computed once, never written)


def seeded(shapes, seed, dev):
    return {k: v.float().to(dev).contiguous() for k, v in syn.seeded_state_dict(shapes, seed).items()}


def reference_step(engine, kind):
    """(golden, inputs, state_dict, batch, (loss, eps, grads)) of one training step on the reference-keyed batch of a golden."""
    if kind not in _STEP:
        g = load_golden(CASES[kind])
        d = golden_inputs(g)
        sd = seeded(inpaint_shapes(kind), g["meta"]["weight_seed"], engine.device)
        batch = reference_batch(g, d)
        _STEP[kind] = (g, d, sd, batch, engine.unet_train_step(g["meta"]["cfg"], sd, batch))
    return _STEP[kind]


def golden_rows(engine, kind):
    """train_step_inputs on a golden's inputs (boxes, inpaint): the rows of the second test's first case."""
    if kind not in _ROWS:
        g = load_golden(CASES[kind])
        d = golden_inputs(g)
        _ROWS[kind] = engine.train_step_inputs(d["z"], d["noise"], d["t"], schedule(), boxes=d["b"]["boxes"], inpaint=True)
    return _ROWS[kind]


def nchw(rows):
    return rows.permute(0, 3, 1, 2).contiguous().cpu()


@pytest.mark.parametrize("kind", sorted(CASES))
def test_inpaint_train_step_vs_reference(engine, kind):
    """One training iteration of an inpainting model (text, text+image tokenizer) against the reference's loss.backward(): loss, eps,
    every sampled gradient of the 128 / 135 trainable tensors (the gates as one vector) and every norm; the first conv's weight
    gradient in full against oracle autograd. Activation checkpointing gives the same bits; the first conv's bias cannot be asked
    for, and neither can the weight of a model without inpaint_mode."""
    from gligen_amd import _lib
    g, d, sd, batch, (loss, eps, grads) = reference_step(engine, kind)
    meta = g["meta"]
    cfg = meta["cfg"]
    assert len(grads) == meta["n_trainable"] == N_TRAINABLE[kind] and FIRST_CONV in grads
    report, norms = golden_report(g, grads)
    report["eps"] = rel_mse(eps, g["eps"])
    loss_err = abs(float(loss) - float(g["loss"])) / float(g["loss"])
    worst = max(report, key=report.get)
    wn = max(norms, key=lambda k: abs(norms[k] - 1))
    print(kind, "inpainting training step: loss", float(loss), "rel err", loss_err, "eps", report["eps"], "worst", worst, report[worst],
          "worst norm ratio", wn, norms[wn])
    assert loss_err < 1e-5 and report["eps"] < 1e-6, (loss_err, report["eps"])
    assert not {k: v for k, v in report.items() if v >= 1e-5}, {k: v for k, v in report.items() if v >= 1e-5}
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), {k: v for k, v in norms.items() if abs(v - 1) >= 1e-3}
    _, _, ref = oracle_autograd(sd, cfg, kind, [FIRST_CONV], d, batch["x"], batch["inpainting_extra_input"])
    full = rel_mse(grads[FIRST_CONV], ref[FIRST_CONV])
    print(kind, "first conv weight gradient in full vs oracle autograd:", full)
    assert full < 1e-5, full
    loss_c, eps_c, grads_c = engine.unet_train_step(cfg, sd, batch, checkpoint=True)
    assert torch.equal(loss_c, loss) and torch.equal(eps_c, eps)
    assert all(torch.equal(grads_c[k], grads[k]) for k in grads), [k for k in grads if not torch.equal(grads_c[k], grads[k])][:5]
    with pytest.raises(_lib.GligenAmdError):
        engine.unet_train_step(cfg, sd, batch, trainable=["input_blocks.0.0.bias"])
    if kind == "text":      # a discrete model without inpaint_mode: its first conv stays frozen
        gt = load_golden("unet_small_train_step")["meta"]
        sdt = seeded(golden_shapes("unet_small_text"), 1234, engine.device)
        plain = {k: v for k, v in batch.items() if k != "inpainting_extra_input"}
        with pytest.raises(_lib.GligenAmdError):
            engine.unet_train_step(gt["cfg"], sdt, plain, trainable=[FIRST_CONV])


def test_step_input_kernel(engine):
    """gl_train_step_inputs against the reference's own x_noisy / mask / inpainting_extra_input (the golden) and, at 3 x 64 x 64 with 30
    boxes per sample, against the torch restatement, bit for bit: timesteps 0 / 999 / 500, a whole-image box, a box below one pixel
    wide, overlapping boxes, a sample of padding boxes only. Then an explicit mask, a model without inpainting, the refusals, and one
    launch per call."""
    sched = schedule()
    g = load_golden(CASES["text"])
    d = golden_inputs(g)
    n0 = engine.launch_count()
    out = golden_rows(engine, "text")
    assert engine.launch_count() == n0 + 1
    assert tuple(out["x_rows"].shape) == (2, 16, 16, 9) and tuple(out["target_rows"].shape) == (2, 16, 16, 4)
    assert torch.equal(nchw(out["x_rows"]), torch.cat([torch.from_numpy(g["x_noisy"]), torch.from_numpy(g["inpainting_extra_input"])], dim=1))
    assert torch.equal(nchw(out["target_rows"]), d["noise"])
    assert out["timesteps"].dtype == torch.float32 and torch.equal(out["timesteps"].cpu(), d["t"].float())
    # ---- a case the golden does not cover
    B, hw, Nb = 3, 64, 30
    gen = torch.Generator().manual_seed(11)
    z, noise = torch.randn(B, 4, hw, hw, generator=gen), torch.randn(B, 4, hw, hw, generator=gen)
    t = torch.tensor([0, 999, 500], dtype=torch.long)
    lo, ext = torch.rand(B, Nb, 2, generator=gen) * 0.8, torch.rand(B, Nb, 2, generator=gen) * 0.2
    boxes = torch.cat([lo, (lo + ext).clamp(max=1.0)], dim=2)
    boxes[0, :, 2:] = (lo[0] + ext[0] * 0.4).clamp(max=1.0)                 # sample 0: small boxes, so that part of its mask stays 1
    boxes[0, 0] = torch.tensor([0.5, 0.5, 0.507, 0.8])                     # below one pixel wide: int(32.0) = int(32.448), masks nothing
    boxes[0, 1], boxes[0, 2] = torch.tensor([0.1, 0.1, 0.4, 0.4]), torch.tensor([0.3, 0.3, 0.6, 0.6])     # overlapping
    boxes[1, 5] = torch.tensor([0.0, 0.0, 1.0, 1.0])                       # the whole image
    boxes[2] = 0.0                                                          # padding boxes only
    x_noisy, mask, extra = restate_step_inputs(z, noise, t, sched, boxes=boxes)
    assert bool((mask[2] == 1).all()) and bool((mask[1] == 0).all()) and 0 < int((mask[0] == 0).sum()) < hw * hw
    lone = box_mask(boxes[:1, :1], hw)
    assert bool((lone == 1).all())                                          # (the sub-pixel box alone)
    out2 = engine.train_step_inputs(z, noise, t, sched, boxes=boxes, inpaint=True)
    assert torch.equal(nchw(out2["x_rows"]), torch.cat([x_noisy, extra], dim=1))
    assert torch.equal(nchw(out2["target_rows"]), noise) and torch.equal(out2["timesteps"].cpu(), t.float())
    # ---- an explicit mask: the box mask gives the boxes' result, a random 0 / 1 mask the restatement's
    out3 = engine.train_step_inputs(z, noise, t, sched, mask=mask, inpaint=True)
    assert all(torch.equal(out3[k], out2[k]) for k in out2)
    rmask = (torch.rand(B, 1, hw, hw, generator=gen) < 0.5).float()
    _, _, rextra = restate_step_inputs(z, noise, t, sched, mask=rmask)
    out4 = engine.train_step_inputs(z, noise, t, sched, mask=rmask.reshape(B, hw * hw), inpaint=True)
    assert torch.equal(nchw(out4["x_rows"]), torch.cat([x_noisy, rextra], dim=1))
    # ---- a model without inpainting: the noised latent's rows alone
    n1 = engine.launch_count()
    out5 = engine.train_step_inputs(z, noise, t, sched)
    assert engine.launch_count() == n1 + 1
    assert tuple(out5["x_rows"].shape) == (B, hw, hw, 4) and torch.equal(nchw(out5["x_rows"]), x_noisy) and torch.equal(nchw(out5["target_rows"]), noise)
    # ---- refused on the host
    for bad in (1.5, -0.1, float("nan")):
        bb = boxes.clone()
        bb[1, 3, 2] = bad
        with pytest.raises(ValueError):
            engine.train_step_inputs(z, noise, t, sched, boxes=bb, inpaint=True)
    with pytest.raises(ValueError):
        engine.train_step_inputs(z[:, :, :32], noise[:, :, :32], t, sched, boxes=boxes, inpaint=True)      # 32 x 64 with boxes
    with pytest.raises(ValueError):
        engine.train_step_inputs(z, noise, t, sched, boxes=boxes, mask=mask, inpaint=True)
    with pytest.raises(ValueError):
        engine.train_step_inputs(z, noise, t, sched, inpaint=True)
    assert tuple(engine.train_step_inputs(z[:, :, :32], noise[:, :, :32], t, sched, mask=mask[:, :, :32], inpaint=True)["x_rows"].shape) == (B, 32, hw, 9)


@pytest.mark.parametrize("kind", sorted(CASES))
def test_rows_in_same_bits(engine, kind):
    """unet_train_step fed the rows train_step_inputs wrote gives the bits of the reference-keyed batch; so does the non-inpainting
    unet_small_train_step fixture fed its rows instead of NCHW tensors."""
    g, d, sd, batch, (loss, eps, grads) = reference_step(engine, kind)
    rows = golden_rows(engine, kind)
    rb = {k: v for k, v in batch.items() if k not in ("x", "target", "inpainting_extra_input", "timesteps")}
    loss_r, eps_r, grads_r = engine.unet_train_step(g["meta"]["cfg"], sd, dict(rb, **rows))
    assert torch.equal(loss_r, loss) and torch.equal(eps_r, eps)
    assert sorted(grads_r) == sorted(grads) and all(torch.equal(grads_r[k], grads[k]) for k in grads)
    if kind == "text":
        meta = load_golden("unet_small_train_step")["meta"]
        B, hw = meta["B"], meta["hw"]
        sdt = seeded(golden_shapes("unet_small_train_step"), meta["weight_seed"], engine.device)
        b = syn.make_batch("text", B, n_valid=meta["n_valid"], seed=5)
        x, target = syn.make_latent(B, 4, hw, hw, seed=6), syn.make_latent(B, 4, hw, hw, seed=7)
        common = dict(timesteps=torch.tensor([981, 441][:B]).float(), context=syn.make_context(B, seed=6), boxes=b["boxes"], masks=b["masks"],
                      positive_embeddings=b["text_embeddings"])
        l0, e0, g0 = engine.unet_train_step(meta["cfg"], sdt, dict(common, x=x, target=target))
        l1, e1, g1 = engine.unet_train_step(meta["cfg"], sdt, dict(common, x_rows=x.permute(0, 2, 3, 1).contiguous(), target_rows=target.permute(0, 2, 3, 1).contiguous()))
        assert len(g0) == 127 and torch.equal(l0, l1) and torch.equal(e0, e1) and all(torch.equal(g0[k], g1[k]) for k in g0)
        with pytest.raises(ValueError):
            engine.unet_train_step(meta["cfg"], sdt, dict(common, **rows))          # nine channels into a four-channel model


def two_steps(engine):
    """TrainStep (world 1, lr 1e-3), two steps on the text golden's inpainting batch from the zero-extended unet_small_text weights."""
    if not _TWO:
        from gligen_amd.train import TrainStep
        g = load_golden(CASES["text"])
        d = golden_inputs(g)
        sd_cpu = add_input_channels(syn.seeded_state_dict(golden_shapes("unet_small_text"), g["meta"]["weight_seed"]), 5)
        ts = TrainStep(engine, g["meta"]["cfg"], sd_cpu, lr=1e-3, weight_decay=0.0, world=1)
        batch = reference_batch(g, d)
        losses = [float(ts.step(batch)[0]) for _ in range(2)]
        torch.cuda.synchronize()
        _TWO.update(g=g, d=d, sd_cpu=sd_cpu, batch=batch, losses=losses, after={k: v.cpu() for k, v in ts.state_dict().items()})
    return _TWO


def test_inpaint_two_optimizer_steps_from_a_zero_extended_conv(engine):
    """A training run that starts from a checkpoint without the five extra channels (add_input_channels, trainer.py:189-193): after two
    AdamW steps every frozen tensor keeps its bits (the first conv's bias among them), every trainable tensor has moved, the five
    new input channels of the first conv are non-zero, and both losses match oracle autograd + torch.optim.AdamW on the CPU."""
    r = two_steps(engine)
    g, d, sd_cpu, after = r["g"], r["d"], r["sd_cpu"], r["after"]
    cfg = g["meta"]["cfg"]
    names = set(trainable_names(sd_cpu, cfg))
    assert len(names) == 128 and FIRST_CONV in names and "input_blocks.0.0.bias" not in names
    for k, v in sd_cpu.items():
        assert torch.equal(after[k], v) != (k in names), k
    assert torch.count_nonzero(sd_cpu[FIRST_CONV][:, 4:]) == 0
    assert all(torch.count_nonzero(after[FIRST_CONV][:, c]) > 0 for c in range(4, 9))
    sdo = {k: v.clone() for k, v in sd_cpu.items()}
    params = [sdo[k].requires_grad_(True) for k in sd_cpu if k in names]
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.0)
    ref_losses = []
    for _ in range(2):
        opt.zero_grad()
        loss, _, grads = oracle_autograd({k: v.detach() for k, v in sdo.items()}, cfg, "text", sorted(names), d, r["batch"]["x"], r["batch"]["inpainting_extra_input"])
        ref_losses.append(float(loss))
        for k in names:
            sdo[k].grad = grads[k]
        opt.step()
    print("inpainting train steps: losses", r["losses"], "oracle + AdamW", ref_losses)
    for a, ref in zip(r["losses"], ref_losses):
        assert abs(a - ref) / ref < 1e-4, (r["losses"], ref_losses)


def test_trained_inpaint_weights_round_trip_to_inference(engine):
    """The state_dict after the two updates, loaded into a fresh inference model with inpaint_mode: eps of the bf16 inference path on
    the 9-channel input against the oracle's forward on the same updated weights, at the bar of the unet_small_inpaint parity test."""
    from oracle import gligen_oracle as orc
    from helpers import build_product_unet, grounding_kwargs, mse
    from test_path_gpu import EPS_MSE_TOL
    r = two_steps(engine)
    g, d, after, batch = r["g"], r["d"], r["after"], r["batch"]
    cfg = g["meta"]["cfg"]
    dev = engine.device
    model = build_product_unet(cfg, "text", inpaint=True, device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in after.items()}, strict=True)
    assert model.engine.unet_cfg["inpaint_mode"]
    to = lambda m: {k: v.to(dev) for k, v in m.items()}
    gin = model.grounding_tokenizer_input.prepare(to(d["b"]))
    eps = model(dict(x=batch["x"].to(dev), timesteps=d["t"].to(dev), context=d["context"].to(dev), grounding_input=gin,
                     inpainting_extra_input=batch["inpainting_extra_input"].to(dev), grounding_extra_input=None))
    eps_o = orc.unet_forward(after, oracle_cfg(cfg, "text"), dict(x=batch["x"], timesteps=d["t"], context=d["context"], grounding_input=grounding_kwargs("text", d["b"]),
                                                                  inpainting_extra_input=batch["inpainting_extra_input"]))
    err = mse(eps, eps_o)
    print("trained inpainting weights in the inference path: eps MSE", err)
    assert err < EPS_MSE_TOL, err


def test_inpaint_train_step_shipped_topology():
    """The shipped UNet (syn.UNET_CFG: 4 levels, 16 fusers) with inpaint_mode, B 1, 16 x 16 latent, checkpoint=True, on an engine of
    its own: loss, eps and the full gradient of the first conv's weight against oracle autograd."""
    from gligen_amd.engine import Engine
    shapes = dict(golden_shapes("unet_full_text"), **{FIRST_CONV: [320, 9, 3, 3]})
    cfg = dict(syn.UNET_CFG, use_checkpoint=False, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=True)
    B, hw = 1, 16
    b = syn.make_batch("text", B, n_valid=3, seed=5)
    d = dict(b=b, z=syn.make_latent(B, 4, hw, hw, seed=6), noise=syn.make_latent(B, 4, hw, hw, seed=7), t=torch.tensor([981], dtype=torch.long),
             context=syn.make_context(B, seed=6))
    x_noisy, mask, extra = restate_step_inputs(d["z"], d["noise"], d["t"], schedule(), boxes=b["boxes"])
    assert 0 < int((mask == 0).sum()) < hw * hw
    batch = dict(x=x_noisy, inpainting_extra_input=extra, timesteps=d["t"].float(), context=d["context"], boxes=b["boxes"], masks=b["masks"],
                 positive_embeddings=b["text_embeddings"], target=d["noise"])
    eng = Engine(0, arena_gb=40.0)
    try:
        sd = seeded(shapes, 1234, eng.device)
        loss, eps, grads = eng.unet_train_step(cfg, sd, batch, checkpoint=True)
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert len(grads) == len(trainable_names(shapes, cfg)) == 281
    loss_o, eps_o, ref = oracle_autograd({k: v.cpu() for k, v in sd.items()}, cfg, "text", [FIRST_CONV], d, x_noisy, extra)
    full = rel_mse(grads[FIRST_CONV], ref[FIRST_CONV])
    print("shipped topology, inpainting: loss", float(loss), "oracle", float(loss_o), "eps", rel_mse(eps, eps_o), "first conv full gradient", full)
    assert abs(float(loss) - float(loss_o)) / float(loss_o) < 1e-5
    assert rel_mse(eps, eps_o) < 1e-6
    assert full < 1e-5, full
