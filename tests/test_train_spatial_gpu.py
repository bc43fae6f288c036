"""The training step of the spatial-map models on the device (gl_unet_train_step_spatial): the ConvNeXt tokenizer, the
GroundingDownsampler and the 4 + k channel first conv, forward and backward, against the reference's loss.backward()
(tools/make_golden_train_spatial.py) and against autograd through the CPU oracle (held to those goldens by
tests/test_train_spatial_cpu.py)."""
import numpy as np
import pytest
import torch

from helpers import golden_shapes, load_golden
from gligen_amd import synthetic as syn
from gligen_amd.train import trainable_names
from test_train_spatial_cpu import MAP_KEYS, N_TRAINABLE, golden_report, oracle_autograd, rel_mse, spatial_batch

pytestmark = pytest.mark.gpu


def device_batch(meta, b):
    return {MAP_KEYS[meta["modality"]]: b["img"], "mask": b["mask"], "grounding_extra_input": b["extra"], "x": b["x"],
            "timesteps": b["timesteps"].float(), "context": b["context"], "target": b["target"]}


def seeded(name, seed, dev):
    return {k: v.float().to(dev).contiguous() for k, v in syn.seeded_state_dict(golden_shapes(name), seed).items()}


@pytest.mark.parametrize("modality", ["canny", "hed", "sem"])
def test_spatial_train_step_vs_reference(engine, modality):
    """One training iteration of a spatial-map model against the reference's loss.backward(): loss, eps, every sampled gradient of the
    310 / 306 / 312 trainable tensors (the ConvNeXt backbone, the tokenizer's MLP / pos_embedding / null_feature, sem's in_conv, the
    downsampler, the first conv's weight, the fusers; the tanh gates as one vector) and every norm. canny: every gradient tensor in full
    against oracle autograd. Then activation checkpointing gives the same bits, and frozen tensors cannot be asked for."""
    from gligen_amd import _lib
    g = load_golden(f"unet_small_{modality}_train_step")
    meta = g["meta"]
    cfg = meta["cfg"]
    sd = seeded(f"unet_small_{modality}", meta["weight_seed"], engine.device)
    b = spatial_batch(meta)
    batch = device_batch(meta, b)
    loss, eps, grads = engine.unet_train_step(cfg, sd, batch)
    assert len(grads) == meta["n_trainable"] == N_TRAINABLE[modality]
    report, norms = golden_report(g, grads)
    report["eps"] = rel_mse(eps, g["eps"])
    loss_err = abs(float(loss) - float(g["loss"])) / float(g["loss"])
    worst = max(report, key=report.get)
    wn = max(norms, key=lambda k: abs(norms[k] - 1))
    print(modality, "training step: loss", float(loss), "worst", worst, report[worst], "worst norm ratio", wn, norms[wn])
    assert loss_err < 1e-5 and report["eps"] < 1e-6, (loss_err, report["eps"])
    assert not {k: v for k, v in report.items() if v >= 1e-5}, {k: v for k, v in report.items() if v >= 1e-5}
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), {k: v for k, v in norms.items() if abs(v - 1) >= 1e-3}
    if modality == "canny":
        _, _, ref = oracle_autograd(sd, meta, list(grads), b)
        full = {k: rel_mse(grads[k], ref[k]) for k in grads if not (k.endswith(".alpha_attn") or k.endswith(".alpha_dense"))}
        gates = sorted(k for k in grads if k not in full)
        full["<the gates>"] = rel_mse(torch.stack([grads[k].reshape(()) for k in gates]), torch.stack([ref[k].reshape(()) for k in gates]))
        worst_full = max(full, key=full.get)
        print("canny: every gradient tensor in full vs oracle autograd: worst", worst_full, full[worst_full])
        assert full[worst_full] < 1e-5, {k: v for k, v in full.items() if v >= 1e-5}
    loss_c, eps_c, grads_c = engine.unet_train_step(cfg, sd, batch, checkpoint=True)
    assert torch.equal(loss_c, loss) and torch.equal(eps_c, eps)
    assert all(torch.equal(grads_c[k], grads[k]) for k in grads), [k for k in grads if not torch.equal(grads_c[k], grads[k])][:5]
    with pytest.raises(_lib.GligenAmdError):
        engine.unet_train_step(cfg, sd, batch, trainable=["input_blocks.0.0.bias"])
    with pytest.raises(_lib.GligenAmdError):
        engine.unet_train_step(cfg, sd, batch, trainable=["input_blocks.1.0.in_layers.2.weight"])


def test_spatial_null_tokenizer_input(engine):
    """The guidance drop's input (zero map, mask 0; grounding_extra_input kept): every ConvNeXt gradient is exactly 0, while
    pos_embedding, null_feature and the MLP get non-zero gradients that match oracle autograd."""
    meta = load_golden("unet_small_canny_train_step")["meta"]
    sd = seeded("unet_small_canny", meta["weight_seed"], engine.device)
    b = spatial_batch(meta)
    b = dict(b, img=torch.zeros_like(b["img"]), mask=torch.zeros_like(b["mask"]))
    _, _, grads = engine.unet_train_step(meta["cfg"], sd, device_batch(meta, b))
    cnx = [k for k in grads if k.startswith("position_net.convnext_tiny_backbone.")]
    assert len(cnx) == 178 and all(torch.count_nonzero(grads[k]) == 0 for k in cnx)
    tok = ["position_net.pos_embedding", "position_net.null_feature"] + [k for k in grads if k.startswith("position_net.linears.")]
    _, _, ref = oracle_autograd(sd, meta, tok, b)
    for k in tok:
        assert torch.count_nonzero(grads[k]) > 0, k
        assert rel_mse(grads[k], ref[k]) < 1e-5, (k, rel_mse(grads[k], ref[k]))


def test_spatial_train_step_two_updates(engine):
    """gligen_amd.train.TrainStep on canny (world 1, lr 1e-3, two steps): the frozen tensors (input_blocks.0.0.bias among them) keep
    their bits, every trainable tensor moves (the ConvNeXt and the downsampler included), and the two losses match oracle autograd +
    torch.optim.AdamW on the CPU."""
    from gligen_amd.train import TrainStep
    from test_train_spatial_cpu import oracle_autograd as oa
    meta = load_golden("unet_small_canny_train_step")["meta"]
    cfg = meta["cfg"]
    sd_cpu = syn.seeded_state_dict(golden_shapes("unet_small_canny"), meta["weight_seed"])
    b = spatial_batch(meta)
    ts = TrainStep(engine, cfg, sd_cpu, lr=1e-3, weight_decay=0.0, world=1)
    losses = [float(ts.step(device_batch(meta, b))[0]) for _ in range(2)]
    after = ts.state_dict()
    names = set(trainable_names(sd_cpu, cfg))
    assert "input_blocks.0.0.bias" not in names and len(names) == 310
    for k, v in sd_cpu.items():
        if k in names:
            assert not torch.equal(after[k].cpu(), v), k
        else:
            assert torch.equal(after[k].cpu(), v), k
    # the CPU reference: oracle autograd + torch.optim.AdamW over the same set
    sdo = {k: v.clone() for k, v in sd_cpu.items()}
    params = [sdo[k].requires_grad_(True) for k in sd_cpu if k in names]
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.0)
    ref_losses = []
    for _ in range(2):
        opt.zero_grad()
        loss, _, grads = oa({k: v.detach() for k, v in sdo.items()}, meta, sorted(names), b)
        ref_losses.append(float(loss))
        for k in names:
            sdo[k].grad = grads[k]
        opt.step()
    print("spatial train steps: losses", losses, "oracle + AdamW", ref_losses)
    for a, r in zip(losses, ref_losses):
        assert abs(a - r) / r < 1e-4, (losses, ref_losses)


def test_spatial_train_step_shipped_topology():
    """The shipped UNet (syn.UNET_CFG: 4 levels, 16 fusers) with the canny tokenizer at resize 256 (64 tokens) and downsampler, B 1,
    16 x 16 latent, checkpoint=True: loss, eps and the full gradient of every ConvNeXt, downsampler and first-conv tensor against
    oracle autograd."""
    from gligen_amd.engine import Engine
    small = golden_shapes("unet_small_canny")
    shapes = {k: v for k, v in golden_shapes("unet_full_text").items() if not k.startswith("position_net.")}
    shapes.update({k: v for k, v in small.items() if k.startswith("position_net.") or k.startswith("downsample_net.")})
    shapes["position_net.pos_embedding"] = [1, 64, 768]
    shapes["input_blocks.0.0.weight"] = [320, 12, 3, 3]
    cfg = dict(syn.UNET_CFG, use_checkpoint=False,
               grounding_downsampler=dict(target="ldm.modules.diffusionmodules.canny_grounding_downsampler.GroundingDownsampler",
                                          params=dict(resize_input=64, out_dim=8)),
               grounding_tokenizer=dict(target="ldm.modules.diffusionmodules.canny_grounding_net.PositionNet", params=dict(resize_input=256, out_dim=768)))
    meta = dict(modality="canny", B=1, hw=16, res=256, map_seed=3, latent_seed=6, context_seed=6, target_seed=7, mask=[1.0], cfg=cfg,
                downsampler=dict(n_in=1, mode="bicubic", resize=64))
    eng = Engine(0, arena_gb=40.0)
    try:
        sd = {k: v.float().to(eng.device).contiguous() for k, v in syn.seeded_state_dict(shapes, 1234).items()}
        b = spatial_batch(meta)
        loss, eps, grads = eng.unet_train_step(cfg, sd, device_batch(meta, b), checkpoint=True)
    finally:
        eng.close()
    assert len(grads) == len(trainable_names(shapes, cfg))
    check = [k for k in grads if k.startswith("position_net.convnext_tiny_backbone.") or k.startswith("downsample_net.") or k == "input_blocks.0.0.weight"]
    assert len(check) == 178 + 4 + 1
    loss_o, eps_o, ref = oracle_autograd({k: v.cpu() for k, v in sd.items()}, meta, check, b)
    assert abs(float(loss) - float(loss_o)) / float(loss_o) < 1e-5
    assert rel_mse(eps, eps_o) < 1e-6
    full = {k: rel_mse(grads[k], ref[k]) for k in check}
    worst = max(full, key=full.get)
    print("shipped topology, canny: worst full gradient", worst, full[worst])
    assert full[worst] < 1e-5, {k: v for k, v in full.items() if v >= 1e-5}
