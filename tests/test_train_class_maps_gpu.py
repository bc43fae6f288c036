"""Training the semantic-map model from u8 class maps on the device: the two weight-gradient kernels alone against float64 autograd
over the one-hot planes (gl_op_class_conv_wgrad), the whole iteration (gl_unet_train_step_spatial_classes) against the reference's
loss.backward() and, bit for bit where the summation order is the same, against the planes path on the same engine, TrainStep on
class-map batches, and the refusals."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden_shapes, load_golden
from gligen_amd import synthetic as syn
from gligen_amd.train import trainable_names
from test_train_spatial_cpu import N_TRAINABLE, golden_report, rel_mse, spatial_batch

pytestmark = pytest.mark.gpu

# the four tensors whose gradient the class path sums in another order than the planes path
REORDERED = ("position_net.in_conv.weight", "position_net.in_conv.bias", "downsample_net.layers.0.weight", "downsample_net.layers.0.bias")

# kind, source (H, W), R, B, n_classes, c_out. The last case is beyond the issue's table: more than 512 tiles, so a workgroup takes
# two tiles, the last workgroup one, and the tiles at the right and bottom edges are partial (392 = 24.5 tiles of 16).
KERNEL_CASES = [("in_conv", (37, 53), 24, 2, 152, 3), ("in_conv", (16, 16), 16, 1, 5, 3), ("in_conv", (96, 96), 96, 3, 152, 3),
                ("down", (40, 24), 32, 2, 152, 16), ("down", (8, 8), 8, 1, 7, 4), ("in_conv", (50, 70), 392, 1, 5, 3)]


def case_map(H, W, B, n_classes, seed):
    """Random classes 0 .. n_classes - 1 with both ends present, a block of 255 and a few 200s (no class when n_classes <= 200)."""
    cls = torch.randint(0, n_classes, (B, 1, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.uint8)
    cls[:, :, 0, 0], cls[:, :, 0, 1] = 0, n_classes - 1
    cls[:, :, H // 3:H // 3 + max(H // 4, 2), W // 2:W // 2 + max(W // 5, 2)] = 255
    cls[:, :, -2, 1::3] = 200
    cls[0, :, -1, -1], cls[-1, :, -1, 0] = 255, n_classes - 1
    return cls


@functools.lru_cache(maxsize=None)
def kernel_case(i):
    """The inputs of case i and the reference: one_hot -> F.interpolate(nearest, R) -> conv2d in float64 on the CPU, autograd for dW / db."""
    kind, (H, W), R, B, n, c_out = KERNEL_CASES[i]
    cls = case_map(H, W, B, n, 10 + i)
    idx = cls.long()
    planes = torch.zeros(B, n, H, W).scatter_(1, idx.clamp(max=n - 1), (idx < n).float())
    x = F.interpolate(planes, size=R, mode="nearest").double()
    k, stride = (4, 2) if kind == "down" else (3, 1)
    Ro = R // stride
    gen = torch.Generator().manual_seed(100 + i)
    dys = dict(ints=torch.randint(-2, 3, (B, c_out, Ro, Ro), generator=gen).float(), gauss=torch.randn(B, c_out, Ro, Ro, generator=gen))
    ref = {}
    for name, dy in dys.items():
        w = torch.zeros(c_out, n, k, k, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(c_out, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w, b, stride=stride, padding=1).backward(dy.double())
        ref[name] = (w.grad, b.grad)
    return cls, dys, ref


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(KERNEL_CASES)), ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}-to-{c[2]}" for c in KERNEL_CASES])
def test_class_conv_wgrad_vs_float64_autograd(engine, i):
    """Integer dy in -2 .. 2: every partial sum is an integer below 2^24, so dW and db equal the float64 reference exactly whatever the
    order. Gaussian dy: rel_mse < 1e-5, the bar of every training gradient. Two calls give equal bits."""
    kind, (H, W), R, B, n, c_out = KERNEL_CASES[i]
    cls, dys, ref = kernel_case(i)
    assert bool((cls == 255).any()) and bool((cls == 200).any())
    dW, db = engine.op_class_conv_wgrad(cls, dys["ints"], n, R, kind)
    assert tuple(dW.shape) == tuple(ref["ints"][0].shape) and tuple(db.shape) == (c_out,)
    assert torch.equal(dW.double().cpu(), ref["ints"][0]), float((dW.double().cpu() - ref["ints"][0]).abs().max())
    assert torch.equal(db.double().cpu(), ref["ints"][1])
    assert torch.count_nonzero(dW) > 0
    dWg, dbg = engine.op_class_conv_wgrad(cls, dys["gauss"], n, R, kind)
    ew, eb = rel_mse(dWg, ref["gauss"][0].float()), rel_mse(dbg, ref["gauss"][1].float())
    print(KERNEL_CASES[i], "gaussian dy: rel_mse dW", ew, "db", eb)
    assert ew < 1e-5 and eb < 1e-5, (ew, eb)
    dW2, db2 = engine.op_class_conv_wgrad(cls[:, 0], dys["gauss"], n, R, kind)       # [B, H, W], and the same bits again
    assert torch.equal(dW2, dWg) and torch.equal(db2, dbg)


def test_class_conv_wgrad_refusals(engine):
    """What the kernels do not take is refused with a message that names the limit."""
    from gligen_amd import _lib
    cls = case_map(8, 8, 1, 7, 3)
    with pytest.raises(_lib.GligenAmdError, match=r"resized side of 0 .*2 \.\. 16384"):
        engine.op_class_conv_wgrad(cls, torch.zeros(1, 3, 8, 8), 7, 0, "in_conv")
    with pytest.raises(_lib.GligenAmdError, match=r"6 output channels.*multiple of 4"):
        engine.op_class_conv_wgrad(cls, torch.zeros(1, 6, 4, 4), 7, 8, "down")
    with pytest.raises(_lib.GligenAmdError, match=r"257 classes.*1 \.\. 256"):
        engine.op_class_conv_wgrad(cls, torch.zeros(1, 3, 8, 8), 257, 8, "in_conv")
    with pytest.raises(_lib.GligenAmdError, match=r"4 output channels.*exactly 3"):
        engine.op_class_conv_wgrad(cls, torch.zeros(1, 4, 8, 8), 7, 8, "in_conv")
    with pytest.raises(_lib.GligenAmdError, match=r"odd input size 9"):
        engine.op_class_conv_wgrad(cls, torch.zeros(1, 4, 4, 4), 7, 9, "down")
    with pytest.raises(ValueError, match=r"the class map is torch.float32 .*u8 \[B, 1, H, W\] or \[B, H, W\] is read"):
        engine.op_class_conv_wgrad(cls.float(), torch.zeros(1, 3, 8, 8), 7, 8, "in_conv")
    with pytest.raises(ValueError, match="kind"):
        engine.op_class_conv_wgrad(cls, torch.zeros(1, 3, 8, 8), 7, 8, "up")
    dW, _ = engine.op_class_conv_wgrad(cls, torch.ones(1, 4, 4, 4), 7, 8, "down")   # the engine still works after the refusals
    assert torch.count_nonzero(dW) > 0


# ---- 2. the whole step --------------------------------------------------------------------------------------------------------------
def seeded(name, seed, dev):
    return {k: v.float().to(dev).contiguous() for k, v in syn.seeded_state_dict(golden_shapes(name), seed).items()}


def sem_batches(meta):
    """The golden's batch as planes and as class maps: the class map is argmax(1) of the planes, which are one-hot."""
    b = spatial_batch(meta)
    cls = b["img"].argmax(1, keepdim=True).to(torch.uint8)
    assert torch.equal(torch.zeros_like(b["img"]).scatter_(1, cls.long(), 1.0), b["img"])      # its one-hot planes are the golden's map
    rest = {"mask": b["mask"], "x": b["x"], "timesteps": b["timesteps"].float(), "context": b["context"], "target": b["target"]}
    return dict(rest, sem=b["img"], grounding_extra_input=b["extra"]), dict(rest, sem=cls, grounding_extra_input=cls.clone())


@pytest.fixture(scope="module")
def sem_steps(engine):
    """One iteration of the sem golden on the same engine, from planes and from class maps."""
    g = load_golden("unet_small_sem_train_step")
    meta = g["meta"]
    sd = seeded("unet_small_sem", meta["weight_seed"], engine.device)
    planes, classes = sem_batches(meta)
    return dict(g=g, meta=meta, sd=sd, planes_batch=planes, classes_batch=classes, planes=engine.unet_train_step(meta["cfg"], sd, planes),
                classes=engine.unet_train_step(meta["cfg"], sd, classes))


def test_class_train_step_vs_reference(sem_steps):
    """The assertions of test_spatial_train_step_vs_reference[sem] on the step fed from class maps."""
    g, meta = sem_steps["g"], sem_steps["meta"]
    loss, eps, grads = sem_steps["classes"]
    assert len(grads) == meta["n_trainable"] == N_TRAINABLE["sem"] == 312
    report, norms = golden_report(g, grads)
    report["eps"] = rel_mse(eps, g["eps"])
    loss_err = abs(float(loss) - float(g["loss"])) / float(g["loss"])
    worst = max(report, key=report.get)
    wn = max(norms, key=lambda k: abs(norms[k] - 1))
    print("sem from class maps: loss", float(loss), "worst", worst, report[worst], "worst norm ratio", wn, norms[wn],
          {k: report[k] for k in REORDERED})
    assert loss_err < 1e-5 and report["eps"] < 1e-6, (loss_err, report["eps"])
    assert not {k: v for k, v in report.items() if v >= 1e-5}, {k: v for k, v in report.items() if v >= 1e-5}
    assert all(abs(v - 1) < 1e-3 for v in norms.values()), {k: v for k, v in norms.items() if abs(v - 1) >= 1e-3}


def test_class_train_step_vs_planes(engine, sem_steps):
    """Against the planes path on the same engine: loss, eps and the 308 gradients that do not read the map are bit-identical, the four
    that do are the same sums in another order; checkpointing and the [B, H, W] form change no bit."""
    meta, sd = sem_steps["meta"], sem_steps["sd"]
    loss_p, eps_p, grads_p = sem_steps["planes"]
    loss, eps, grads = sem_steps["classes"]
    assert torch.equal(loss, loss_p) and torch.equal(eps, eps_p)
    same = [k for k in grads if k not in REORDERED]
    assert set(REORDERED) <= set(grads) and len(same) == 308
    assert all(torch.equal(grads[k], grads_p[k]) for k in same), [k for k in same if not torch.equal(grads[k], grads_p[k])][:5]
    for k in REORDERED:
        e = rel_mse(grads[k], grads_p[k].cpu())
        print(k, "classes vs planes rel_mse", e)
        assert torch.count_nonzero(grads[k]) > 0 and e < 1e-5, (k, e)
    loss_c, eps_c, grads_c = engine.unet_train_step(meta["cfg"], sd, sem_steps["classes_batch"], checkpoint=True)
    assert torch.equal(loss_c, loss) and torch.equal(eps_c, eps)
    assert all(torch.equal(grads_c[k], grads[k]) for k in grads), [k for k in grads if not torch.equal(grads_c[k], grads[k])][:5]
    b3 = dict(sem_steps["classes_batch"])
    b3["sem"], b3["grounding_extra_input"] = b3["sem"][:, 0], b3["grounding_extra_input"][:, 0]
    loss_3, eps_3, grads_3 = engine.unet_train_step(meta["cfg"], sd, b3)
    assert torch.equal(loss_3, loss) and torch.equal(eps_3, eps) and all(torch.equal(grads_3[k], grads[k]) for k in grads)


# ---- 3. TrainStep -------------------------------------------------------------------------------------------------------------------
def test_class_train_step_two_updates(engine):
    """gligen_amd.train.TrainStep on sem from class maps (world 1, lr 1e-3, two steps): frozen tensors keep their bits, every trainable
    tensor moves, both losses are within 1e-4 of the planes TrainStep's; a step with drop_prob = 1 (the map becomes 255, the mask 0)
    runs and leaves every ConvNeXt gradient exactly 0."""
    import random
    from gligen_amd.train import TrainStep
    meta = load_golden("unet_small_sem_train_step")["meta"]
    cfg = meta["cfg"]
    sd_cpu = syn.seeded_state_dict(golden_shapes("unet_small_sem"), meta["weight_seed"])
    planes, classes = sem_batches(meta)
    ts = TrainStep(engine, cfg, sd_cpu, lr=1e-3, weight_decay=0.0, world=1)
    ref_losses = [float(ts.step(planes)[0]) for _ in range(2)]
    ts = TrainStep(engine, cfg, sd_cpu, lr=1e-3, weight_decay=0.0, world=1)
    losses = [float(ts.step(classes)[0]) for _ in range(2)]
    after = ts.state_dict()
    names = set(trainable_names(sd_cpu, cfg))
    assert len(names) == 312 and "input_blocks.0.0.bias" not in names
    for k, v in sd_cpu.items():
        assert torch.equal(after[k].cpu(), v) != (k in names), k
    print("sem TrainStep: losses from class maps", losses, "from planes", ref_losses)
    assert losses[0] == ref_losses[0]
    for a, r in zip(losses, ref_losses):
        assert abs(a - r) / r < 1e-4, (losses, ref_losses)
    ts = TrainStep(engine, cfg, sd_cpu, lr=1e-3, weight_decay=0.0, world=1, drop_prob=1.0, rng=random.Random(0))
    loss, _ = ts.step(classes)
    assert np.isfinite(float(loss))
    cnx = [k for k in ts.gbuf.views if k.startswith("position_net.convnext_tiny_backbone.")]
    assert len(cnx) == 178 and all(torch.count_nonzero(ts.gbuf.views[k]) == 0 for k in cnx)
    assert torch.count_nonzero(ts.gbuf.views["position_net.null_feature"]) > 0
    assert torch.count_nonzero(ts.gbuf.views["downsample_net.layers.0.weight"]) > 0      # grounding_extra_input is not part of the drop


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_class_train_step_refusals(engine, sem_steps):
    from gligen_amd import _lib
    meta, sd, classes, planes = sem_steps["meta"], sem_steps["sd"], sem_steps["classes_batch"], sem_steps["planes_batch"]
    # a u8 map to a tokenizer without in_dim
    cmeta = load_golden("unet_small_canny_train_step")["meta"]
    csd = seeded("unet_small_canny", cmeta["weight_seed"], engine.device)
    cb = {k: v for k, v in classes.items() if k != "sem"}
    with pytest.raises(_lib.GligenAmdError, match="tokenizer without in_dim"):
        engine.unet_train_step(cmeta["cfg"], csd, dict(cb, canny_edge=classes["sem"]))
    # a mixture of class maps and planes, either way round
    with pytest.raises(ValueError, match=r"the class map is torch.float32 .*u8 \[B, 1, H, W\] or \[B, H, W\] is read"):
        engine.unet_train_step(meta["cfg"], sd, dict(classes, grounding_extra_input=planes["grounding_extra_input"]))
    with pytest.raises(ValueError, match=r"the class map is torch.float32 .*u8 \[B, 1, H, W\] or \[B, H, W\] is read"):
        engine.unet_train_step(meta["cfg"], sd, dict(planes, grounding_extra_input=classes["grounding_extra_input"]))
    # a map of another shape or batch
    with pytest.raises(ValueError, match=r"the class map is torch.uint8 .*u8 \[B, 1, H, W\] or \[B, H, W\] is read"):
        engine.unet_train_step(meta["cfg"], sd, dict(classes, sem=classes["sem"].repeat(1, 2, 1, 1)))
    with pytest.raises(ValueError, match="3 and 2 samples, x holds 2"):
        engine.unet_train_step(meta["cfg"], sd, dict(classes, sem=classes["sem"].repeat(2, 1, 1, 1)[:3]))
    loss, _, _ = engine.unet_train_step(meta["cfg"], sd, classes)          # and the engine still trains
    assert torch.equal(loss, sem_steps["classes"][0])
