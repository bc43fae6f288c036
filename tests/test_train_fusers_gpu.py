"""Training the gatedSA2 and gatedCA fuser models on the device: the fp32 grid resize and its adjoint (gl_op_grid_resize /
gl_op_grid_resize_backward) against the float64 restatement that tests/test_train_fusers_cpu.py holds to torch's bicubic, the block
slice by fuser kind (gl_op_block_train_fuser) and the whole training step against the reference's loss.backward()
(tools/make_golden_train_fusers.py) and autograd through the CPU oracle, two AdamW steps of the gatedCA model, and the refusals."""
import pytest
import torch

from helpers import build_product_unet, golden_shapes, grounding_kwargs, load_golden, mse, oracle_cfg
from gligen_amd import synthetic as syn
from gligen_amd._lib import GligenAmdError
from gligen_amd.train import trainable_names
from test_train_fusers_cpu import (N_TRAINABLE, RESIZE_PAIRS, UNET_CASES, UNET_SHAPES, block_case, block_oracle_autograd, block_report, resize_adjoint_ref,
                                   resize_bounds, resize_ref, text_batch, unet_oracle_autograd)
from test_train_spatial_cpu import golden_report, rel_mse, spatial_batch
from test_train_spatial_gpu import device_batch

pytestmark = pytest.mark.gpu

_STEP = {}       # device results shared between the tests of this module (computed once, never written)
EPS_BAR = 1e-6   # the whole step's eps rel-MSE bar (test_inpaint_train_step_vs_reference)


def seeded(name, seed, dev):
    return {k: v.float().to(dev).contiguous() for k, v in syn.seeded_state_dict(golden_shapes(name), seed).items()}


# ---- 1. the resize operators
@pytest.mark.parametrize("sg,sv,C", [(sg, sv, 64) for sg, sv in RESIZE_PAIRS] + [(4, 16, 320)])
def test_grid_resize_forward_and_adjoint(engine, sg, sv, C):
    """gl_op_grid_resize and gl_op_grid_resize_backward against the float64 tap table, elementwise within (n + 8) 2^-24 (|W| |v|) (n the
    number of terms of that output's sum); <R t, g> = <t, R^T g> from the device outputs within the same bound; two runs give the same
    bits. The largest observed fraction of the bound is printed per case; measured on MI355X: 0.28 forward (8 -> 64), 0.46 backward
    (8 -> 5), the adjoint identity within 0.3 % of its bound."""
    gen = torch.Generator().manual_seed(1000 * sg + 10 * sv + C)
    B = 2
    t = torch.randn(B, sg * sg, C, generator=gen)
    g = torch.randn(B, sv * sv, C, generator=gen)
    y = engine.op_grid_resize(t, sg, sv)
    d = engine.op_grid_resize_backward(g, sg, sv)
    assert tuple(y.shape) == (B, sv * sv, C) and tuple(d.shape) == (B, sg * sg, C)
    assert torch.equal(engine.op_grid_resize(t, sg, sv), y) and torch.equal(engine.op_grid_resize_backward(g, sg, sv), d)
    y, d = y.double().cpu(), d.double().cpu()
    bf, bb = resize_bounds(t, g, sg, sv)
    ef, eb = (y - resize_ref(t, sg, sv)).abs(), (d - resize_adjoint_ref(g, sg, sv)).abs()
    frac_f, frac_b = float((ef / bf.clamp_min(1e-300)).max()), float((eb / bb.clamp_min(1e-300)).max())
    lhs, rhs = float((y * g.double()).sum()), float((t.double() * d).sum())
    bound_dot = float((bf * g.double().abs()).sum() + (bb * t.double().abs()).sum())
    print(f"grid resize {sg} -> {sv}, C {C}: largest error / bound forward {frac_f:.3f}, backward {frac_b:.3f}; adjoint identity {abs(lhs - rhs):.3e} of {bound_dot:.3e}")
    assert bool((ef <= bf).all()), frac_f
    assert bool((eb <= bb).all()), frac_b
    assert abs(lhs - rhs) <= bound_dot, (lhs, rhs, bound_dot)


# ---- 2. the block slice
@pytest.mark.parametrize("fuser_type", ["gatedSA2", "gatedCA"])
def test_fuser_block_backward_vs_reference(engine, fuser_type):
    """gl_op_block_train_fuser against the reference's autograd through one BasicTransformerBlock (block_backward_gatedsa's case with the
    other fuser), at that test's bars: loss < 1e-5, y < 1e-6, every tensor < 1e-5 on the golden's samples -- and in full against oracle
    autograd. For gatedCA this is where attn_bwd runs with Nq != Nk and dk, dv."""
    g, meta, sd, inputs = block_case(fuser_type)
    y, loss, dx, dobjs, grads = engine.op_block_train(sd, *inputs, meta["heads"], fuser_type=fuser_type)
    report, norms = block_report(g, meta, y, loss, dx, dobjs, grads)
    worst = max(report, key=report.get)
    print(fuser_type, "training slice: worst", worst, report[worst])
    assert report["loss"] < 1e-5 and report["y"] < 1e-6, report
    assert all(v < 1e-5 for v in report.values()), {k: v for k, v in report.items() if v >= 1e-5}
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), norms
    yo, _, dxo, dobjso, go = block_oracle_autograd(meta, sd, inputs)
    full = dict(y=rel_mse(y, yo), dx=rel_mse(dx, dxo), dobjs=rel_mse(dobjs, dobjso), **{k: rel_mse(grads[k], go[k]) for k in grads})
    worst = max(full, key=full.get)
    print(fuser_type, "training slice in full vs oracle autograd: worst", worst, full[worst])
    assert full["y"] < 1e-6 and all(v < 1e-5 for v in full.values()), {k: v for k, v in full.items() if v >= 1e-5}


def test_gatedsa_through_the_new_entry_is_the_old_entry(engine):
    """op_block_train(fuser_type="gatedSA") (gl_op_block_train_fuser, kind 0) gives the bits of gl_op_block_train."""
    from helpers import fuser_block_train_report
    _, case = fuser_block_train_report(engine)
    args = (case["sd"], case["x"], case["objs"], case["context"], case["target"], case["meta"]["heads"])
    old = engine.op_block_train(*args)
    new = engine.op_block_train(*args, fuser_type="gatedSA")
    for a, b in zip(old[:4], new[:4]):
        assert torch.equal(a, b)
    assert sorted(old[4]) == sorted(new[4]) and all(torch.equal(old[4][k], new[4][k]) for k in old[4])


# ---- 3. the whole step
def reference_step(engine, case):
    """(golden, state_dict, batch, (loss, eps, grads)) of one training step on a UNet golden's batch."""
    if case not in _STEP:
        g = load_golden(UNET_CASES[case])
        meta = g["meta"]
        sd = seeded(UNET_SHAPES[case], meta["weight_seed"], engine.device)
        batch = device_batch(meta, spatial_batch(meta)) if case == "canny_gatedsa2" else text_batch(meta)[1]
        _STEP[case] = (g, sd, batch, engine.unet_train_step(meta["cfg"], sd, batch))
    return _STEP[case]


def step_report(g, loss, eps, grads):
    report, norms = golden_report(g, grads)
    report["eps"] = rel_mse(eps, g["eps"])
    return report, norms, abs(float(loss) - float(g["loss"])) / float(g["loss"])


def assert_meets_golden(tag, g, loss, eps, grads):
    report, norms, loss_err = step_report(g, loss, eps, grads)
    worst = max(report, key=report.get)
    wn = max(norms, key=lambda k: abs(norms[k] - 1))
    print(tag, "training step: loss", float(loss), "rel err", loss_err, "eps", report["eps"], "worst", worst, report[worst], "worst norm ratio", wn, norms[wn])
    assert loss_err < 1e-5 and report["eps"] < EPS_BAR, (loss_err, report["eps"])
    assert not {k: v for k, v in report.items() if v >= 1e-5}, {k: v for k, v in report.items() if v >= 1e-5}
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), {k: v for k, v in norms.items() if abs(v - 1) >= 1e-3}


@pytest.mark.parametrize("case", sorted(UNET_CASES))
def test_fuser_train_step_vs_reference(engine, case):
    """One training iteration of a gatedSA2 / gatedCA model (text tokenizer; canny tokenizer + downsampler with gatedSA2) against the
    reference's loss.backward(): loss, eps, every sampled gradient (the gates as one vector) and every norm, at the bars of
    test_inpaint_train_step_vs_reference; one fuser.attn.to_k.weight, one fuser.linear.weight (gatedSA2) and the first position_net
    tensor in full against oracle autograd; checkpoint=True gives the same bits."""
    g, sd, batch, (loss, eps, grads) = reference_step(engine, case)
    meta = g["meta"]
    assert len(grads) == meta["n_trainable"] == N_TRAINABLE[case]
    assert_meets_golden(case, g, loss, eps, grads)
    full_keys = ["middle_block.1.transformer_blocks.0.fuser.attn.to_k.weight", next(k for k in sd if k.startswith("position_net."))]
    if case != "gatedca":
        full_keys.append("input_blocks.1.1.transformer_blocks.0.fuser.linear.weight")
    assert all(k in grads for k in full_keys)
    _, _, ref = unet_oracle_autograd(case, meta, sd, full_keys)
    full = {k: rel_mse(grads[k], ref[k]) for k in full_keys}
    print(case, "in full vs oracle autograd:", full)
    assert all(v < 1e-5 for v in full.values()), full
    loss_c, eps_c, grads_c = engine.unet_train_step(meta["cfg"], sd, batch, checkpoint=True)
    assert torch.equal(loss_c, loss) and torch.equal(eps_c, eps)
    assert all(torch.equal(grads_c[k], grads[k]) for k in grads), [k for k in grads if not torch.equal(grads_c[k], grads[k])][:5]


# ---- 4. the fuser type is honoured
def test_fuser_type_is_honoured(engine):
    """A gatedSA2 model has gatedSA's state_dict keys, so nothing but cfg["fuser_type"] tells the two apart: the gatedSA2 step meets its
    golden, and its eps differs from the same call with fuser_type="gatedSA" by more than 100 x the eps bar. The gatedCA step runs."""
    g, sd, batch, (loss, eps, grads) = reference_step(engine, "gatedsa2")
    cfg = g["meta"]["cfg"]
    assert cfg["fuser_type"] == "gatedSA2"
    assert_meets_golden("gatedsa2", g, loss, eps, grads)
    _, eps_sa, _ = engine.unet_train_step(dict(cfg, fuser_type="gatedSA"), sd, batch)
    apart = rel_mse(eps_sa, eps.cpu())
    print("gatedSA2 vs gatedSA on one state_dict: eps rel-MSE", apart)
    assert apart > 100 * EPS_BAR, apart
    loss_ca = reference_step(engine, "gatedca")[3][0]
    assert torch.isfinite(loss_ca).all()


# ---- 5. two optimiser steps
def test_gatedca_two_optimizer_steps_and_round_trip(engine):
    """TrainStep on the gatedCA model, two AdamW steps, against oracle autograd + torch.optim.AdamW on the CPU at the bars of
    test_train_two_optimizer_steps_vs_reference (losses 1e-4 relative, the update of two tensors 1e-3 rel-MSE); the updated weights in
    the bf16 inference engine then give the oracle's eps on them within the 2e-4 MSE bar."""
    from gligen_amd.train import TrainStep
    from oracle import gligen_oracle as orc
    from test_path_gpu import EPS_MSE_TOL
    g = load_golden(UNET_CASES["gatedca"])
    meta = g["meta"]
    cfg, lr = meta["cfg"], 1e-3
    sd_cpu = syn.seeded_state_dict(golden_shapes(UNET_SHAPES["gatedca"]), meta["weight_seed"])
    b, batch = text_batch(meta)
    ts = TrainStep(engine, cfg, sd_cpu, lr=lr, weight_decay=0.0, world=1)
    losses = [float(ts.step(batch)[0]) for _ in range(2)]
    torch.cuda.synchronize()
    after = {k: v.cpu() for k, v in ts.state_dict().items()}
    names = trainable_names(sd_cpu, cfg)
    assert len(names) == 113
    for k, v in sd_cpu.items():
        assert torch.equal(after[k], v) != (k in names), k
    sdo = {k: v.clone() for k, v in sd_cpu.items()}
    opt = torch.optim.AdamW([sdo[k].requires_grad_(True) for k in names], lr=lr, weight_decay=0.0)
    ref_losses = []
    for _ in range(2):
        opt.zero_grad()
        loss, _, grads = unet_oracle_autograd("gatedca", meta, {k: v.detach() for k, v in sdo.items()}, names)
        ref_losses.append(float(loss))
        for k in names:
            sdo[k].grad = grads[k]
        opt.step()
    print("gatedCA train steps: losses", losses, "oracle + AdamW", ref_losses)
    for a, ref in zip(losses, ref_losses):
        assert abs(a - ref) / ref < 1e-4, (losses, ref_losses)
    for key in ("input_blocks.1.1.transformer_blocks.0.fuser.attn.to_k.weight", "position_net.linears.4.weight"):
        rel = float(((after[key] - sdo[key].detach()) ** 2).mean() / ((sdo[key].detach() - sd_cpu[key]) ** 2).mean())
        print("gatedCA train steps:", key, "update rel-MSE", rel)
        assert rel < 1e-3, (key, rel)
    dev = engine.device
    model = build_product_unet(cfg, "text", device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in after.items()}, strict=True)
    gin = model.grounding_tokenizer_input.prepare({k: v.to(dev) for k, v in b.items()})
    eps = model(dict(x=batch["x"].to(dev), timesteps=batch["timesteps"].long().to(dev), context=batch["context"].to(dev), grounding_input=gin,
                     inpainting_extra_input=None, grounding_extra_input=None))
    eps_o = orc.unet_forward(after, oracle_cfg(cfg, "text"), dict(x=batch["x"], timesteps=batch["timesteps"].long(), context=batch["context"],
                                                                  grounding_input=grounding_kwargs("text", b)))
    err = mse(eps, eps_o)
    print("trained gatedCA weights in the inference path: eps MSE", err)
    assert err < EPS_MSE_TOL, err


# ---- 6. refusals
def test_fuser_refusals(engine):
    """gatedSA2 with 30 grounding tokens, a gatedCA model given a fuser.linear.weight, a gradient asked for a frozen key: each is a
    GligenAmdError that names the limit, and the engine works afterwards."""
    g, sd, batch, (loss, _, _) = reference_step(engine, "gatedsa2")
    cfg = g["meta"]["cfg"]
    meta30 = dict(g["meta"], max_objs=30)
    with pytest.raises(GligenAmdError, match="square number of grounding tokens"):
        engine.unet_train_step(cfg, sd, text_batch(meta30)[1])
    gb, mb, sdb, inputs = block_case("gatedSA2")
    x, objs, context, target = inputs
    with pytest.raises(GligenAmdError, match="square number of grounding tokens"):
        engine.op_block_train(sdb, x, torch.cat([objs, objs[:, :14]], dim=1), context, target, mb["heads"], fuser_type="gatedSA2")
    with pytest.raises(GligenAmdError, match="square grid of visual tokens"):
        engine.op_block_train(sdb, x[:, :250], objs, context, target[:, :250], mb["heads"], fuser_type="gatedSA2")
    gc, sdc, batchc, _ = reference_step(engine, "gatedca")
    key = "input_blocks.1.1.transformer_blocks.0.fuser.linear.weight"
    with pytest.raises(GligenAmdError, match="fuser.linear.weight"):
        engine.unet_train_step(gc["meta"]["cfg"], dict(sdc, **{key: sd[key]}), batchc, trainable=trainable_names(sdc, gc["meta"]["cfg"]))
    _, mc, sdbc, inputsc = block_case("gatedCA")
    with pytest.raises(GligenAmdError, match="fuser.linear.weight"):
        engine.op_block_train(dict(sdbc, **{"fuser.linear.weight": sdb["fuser.linear.weight"]}), *inputsc, mc["heads"], fuser_type="gatedCA")
    with pytest.raises(GligenAmdError, match="keeps frozen"):
        engine.unet_train_step(cfg, sd, batch, trainable=["out.2.weight"])
    with pytest.raises(GligenAmdError, match="keeps frozen"):
        engine.unet_train_step(gc["meta"]["cfg"], sdc, batchc, trainable=["middle_block.1.transformer_blocks.0.attn2.to_k.weight"])
    loss_again, _, _ = engine.unet_train_step(cfg, sd, batch)
    assert torch.equal(loss_again, loss)
