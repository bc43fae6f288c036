"""Gradient accumulation, norm clipping and loss weights on the device (csrc/train_run.hip, include/gligen_amd_train_run.h): the
accumulate kernel against its fp32 restatement bit for bit, the norm and the coefficient against float64 within the bound derived from
the summation chain (tests/train_run_ref.py), the clipped updates against the unclipped ones on a scaled gradient bit for bit, the
weighted training step against autograd through the CPU oracle, TrainStep with accumulation and clipping against a float64 restatement
that carries the bound of the fp32 op chain, and the Trainer's resume through the command line. Flat tensors, or the small UNet of
tests/golden/unet_small_train_2steps.npz (B = 2, 16 x 16 latent)."""
import os
import subprocess
import sys

import pytest
import torch

import train_run_ref as R
from helpers import ROOT, golden_shapes, load_golden, rel_mse
from gligen_amd import synthetic as syn
from gligen_amd.train import TrainStep, min_snr_weights, trainable_names

pytestmark = pytest.mark.gpu

META = load_golden("unet_small_train_2steps")["meta"]
CFG = dict(META["cfg"], grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=False)
B, HW = META["B"], META["hw"]
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
N_LIST = R.N_LIST
_CASE = {}


def guarded(src, off):
    """`src` [n] copied into the middle of a longer device tensor: (the whole tensor, its view of n elements `off` elements in)."""
    n = src.numel()
    whole = torch.full((off + n + 8,), 12345.0, device=src.device)
    whole[off:off + n] = src
    return whole, whole[off:off + n]


def guards_ok(whole, off, n):
    return bool((whole[:off] == 12345.0).all()) and bool((whole[off + n:] == 12345.0).all()) and whole.numel() == off + n + 8


# ---- 1. accumulate
@pytest.mark.parametrize("n", N_LIST)
def test_accumulate_three_micro_batches(engine, n):
    """first, middle, last over K = 3 are torch.equal to ((g1 + g2) + g3) * fl(1/3) in torch fp32, with 16-byte aligned tensors and with
    every tensor at a 4-byte offset (the scalar path); `last` leaves acc alone ((g1 + g2)) and writes the gradient; elements in front
    of and behind the n are untouched."""
    dev = engine.device
    gen = torch.Generator(device=dev).manual_seed(n)
    gs = [torch.randn(n, generator=gen, device=dev) for _ in range(3)]
    want = R.accumulate_ref(gs)
    assert want.dtype == torch.float32 and not torch.equal(want, gs[2])
    for off in (0, 1):
        aw, acc = guarded(torch.full((n,), 777.0, device=dev), off)          # (first overwrites whatever acc held)
        views = [guarded(g, off) for g in gs]
        assert (acc.data_ptr() % 16 != 0) == bool(off)
        engine.op_grad_accumulate(acc, views[0][1], "first", 3)
        assert torch.equal(acc, gs[0]) and torch.equal(views[0][1], gs[0])
        engine.op_grad_accumulate(acc, views[1][1], "middle", 3)
        assert torch.equal(acc, gs[0] + gs[1]) and torch.equal(views[1][1], gs[1])
        engine.op_grad_accumulate(acc, views[2][1], "last", 3)
        assert torch.equal(views[2][1], want), (off, int((views[2][1] != want).sum()))
        assert torch.equal(acc, gs[0] + gs[1])
        assert guards_ok(aw, off, n) and all(guards_ok(w, off, n) for w, _ in views), off
    if n == 5:      # refused by the library, by name; n = 0 launches nothing
        from gligen_amd import _lib
        a, g = torch.zeros(5, device=dev), torch.ones(5, device=dev)
        with pytest.raises(_lib.GligenAmdError, match="k = 0"):
            engine.op_grad_accumulate(a, g, "last", 0)
        with pytest.raises(_lib.GligenAmdError, match="mode"):
            _lib.check(engine.lib.gl_op_grad_accumulate(engine._ctx, a.data_ptr(), g.data_ptr(), 5, 3, 2, None))
        with pytest.raises(_lib.GligenAmdError, match="negative"):
            _lib.check(engine.lib.gl_op_grad_accumulate(engine._ctx, a.data_ptr(), g.data_ptr(), -1, 0, 2, None))
        _lib.check(engine.lib.gl_op_grad_accumulate(engine._ctx, a.data_ptr(), g.data_ptr(), 0, 0, 2, None))
        assert float(a.abs().sum()) == 0.0 and float(g.sum()) == 5.0
        with pytest.raises(_lib.GligenAmdError, match="null"):          # (an empty torch tensor has no address)
            engine.op_grad_accumulate(a[:0], g[:0], "first", 2)


# ---- 2. norm and coefficient
def norm_data(n, dev):
    gen = torch.Generator(device=dev).manual_seed(31 + n % 9973)
    x = torch.randn(n, generator=gen, device=dev)
    spike = x.clone()
    spike[n // 2] = 1e6
    return {"normal": x, "zeros": torch.zeros(n, device=dev), "one element 1e6": spike}


def check_norm(engine, partials, norm64, n_total, what):
    """op_clip_coef over `partials` against float64: the norm within norm_bound, the coefficient for max_norm = fl(norm / 2) within
    coef_bound, exactly 1 for a max_norm above the norm."""
    count = partials.numel()
    bound = R.norm_bound(norm64, n_total, count=count)
    mx = R.f32(0.5 * norm64) if norm64 > 0 else 1.0
    out = engine.op_clip_coef(partials, mx)
    norm, coef = float(out[0]), float(out[1])
    cb = R.coef_bound(norm64, n_total, mx, count=count)
    print(f"{what}: norm {norm!r} float64 {norm64!r} |diff| / bound {abs(norm - norm64) / bound if bound else 0.0:.3f}; "
          f"coef {coef!r} |diff| / bound {abs(coef - R.coef_ref(norm64, mx)) / cb:.3f}")
    assert abs(norm - norm64) <= bound, (what, norm, norm64, bound)
    assert abs(coef - R.coef_ref(norm64, mx)) <= cb, (what, coef, R.coef_ref(norm64, mx), cb)
    if norm64 > 0:
        assert 0.49 < coef < 0.51
    above = engine.op_clip_coef(partials, R.f32(2.0 * norm64 + 1.0))
    assert float(above[1]) == 1.0 and float(above[0]) == norm
    return norm, coef


@pytest.mark.parametrize("n", N_LIST)
def test_norm_and_coefficient_vs_float64(engine, n):
    """Every data kind (N(0, 1); zeros; one element 1e6 among N(0, 1)), aligned and as a 4-byte-offset view: the count of partials is
    ceil(n / chunk); the norm and the coefficient stay within the bounds derived from the summation chain; zeros give norm 0 and
    coefficient 1 exactly; the offset view and a second run give the same bits; up to 100003 elements the partial sums are bit for bit
    the fp32 emulation of the chain; a NaN gives a NaN norm and coefficient."""
    dev = engine.device
    assert engine.GRAD_NORM_GRID == R.GRID
    count = R.partial_count(n)
    assert engine.grad_sqnorm_partials(n) == count
    for kind, x in norm_data(n, dev).items():
        norm64 = float(x.double().pow(2).sum().sqrt())
        partials = engine.op_grad_sqnorm(x)
        assert partials.numel() == count and x.data_ptr() % 16 == 0
        norm, coef = check_norm(engine, partials, norm64, n, f"n = {n} {kind}")
        if kind == "zeros":
            assert norm == 0.0 and coef == 1.0
        whole, view = guarded(x, 1)
        assert view.data_ptr() % 16 == 4
        pw, pv = guarded(torch.zeros(count, device=dev), 1)
        engine.op_grad_sqnorm(view, pv)
        assert torch.equal(pv, partials), (kind, "the 4-byte path sums in the same order")
        assert torch.equal(engine.op_grad_sqnorm(x), partials), (kind, "two runs")
        assert guards_ok(pw, 1, count) and torch.equal(view, x)
        if n <= 100003:
            assert torch.equal(partials.cpu(), R.emulate_sqnorm_partials(x)), kind
    bad = norm_data(n, dev)["normal"]
    bad[n // 3] = float("nan")
    out = engine.op_clip_coef(engine.op_grad_sqnorm(bad), 1.0)
    assert bool(torch.isnan(out).all()), out
    if n == 5:
        from gligen_amd import _lib
        p = torch.ones(3, device=dev)
        for mx in (0.0, -1.0, float("nan")):
            with pytest.raises(_lib.GligenAmdError, match="max_norm"):
                engine.op_clip_coef(p, mx)
        empty = engine.op_clip_coef(p[:0], 2.0)
        assert float(empty[0]) == 0.0 and float(empty[1]) == 1.0
        inf = engine.op_clip_coef(torch.tensor([float("inf")], device=dev), 2.0)        # torch: max_norm / inf = 0
        assert float(inf[0]) == float("inf") and float(inf[1]) == 0.0


def test_three_ragged_buckets_one_coefficient(engine):
    """Three ranges of ragged lengths, each into its slice of one partials tensor, one op_clip_coef over all of them: the global norm
    against float64 within the bound for the total."""
    dev = engine.device
    sizes = [1027, 100003, 16385]
    counts = [engine.grad_sqnorm_partials(n) for n in sizes]
    assert counts == [1, 7, 2]
    xs = [norm_data(n, dev)["normal"] * (i + 1) for i, n in enumerate(sizes)]
    partials = torch.full((sum(counts),), -1.0, device=dev)
    at = 0
    for x, c in zip(xs, counts):
        engine.op_grad_sqnorm(x, partials[at:at + c])
        at += c
    norm64 = float(sum(x.double().pow(2).sum() for x in xs).sqrt())
    check_norm(engine, partials, norm64, sum(sizes), "three ragged buckets")
    assert torch.equal(partials.cpu(), torch.cat([R.emulate_sqnorm_partials(x) for x in xs]))


# ---- 3. the clipped update
@pytest.mark.parametrize("n", N_LIST)
def test_clipped_update_gives_the_unclipped_bits_on_a_scaled_gradient(engine, n):
    """Three steps, weight_decay 0.01: p, m, v after op_adamw_clip_step are torch.equal to op_adamw_step on g * coef (the fp32 torch
    product on the device), coef read from a device tensor; op_adamw_ema_clip_step's p, m, v, ema are op_adamw_ema_step's; aligned
    and at a 4-byte offset; coef = 1.0 reproduces op_adamw_step on g; g is not written and the guards are untouched."""
    dev = engine.device
    gen = torch.Generator(device=dev).manual_seed(n + 1)
    rnd = lambda: torch.randn(n, generator=gen, device=dev)
    p0, m0, v0, e0 = rnd(), rnd() * 0.1, rnd().abs() * 0.01, rnd()
    grads = [rnd() for _ in range(3)]
    pair = torch.tensor([123.0, 0.37], device=dev)          # (norm, coefficient) as op_clip_coef leaves them
    for coef in (pair[1:2], torch.ones(1, device=dev)):
        ref = [t.clone() for t in (p0, m0, v0)]
        ref_e = [t.clone() for t in (p0, m0, v0, e0)]
        runs = {off: dict(plain=[guarded(t, off) for t in (p0, m0, v0)], ema=[guarded(t, off) for t in (p0, m0, v0, e0)]) for off in (0, 1)}
        for step, g in enumerate(grads, 1):
            scaled = g * coef
            if float(coef) == 1.0:
                assert torch.equal(scaled, g)
            engine.op_adamw_step(ref[0], scaled, ref[1], ref[2], step, **HYPER)
            engine.op_adamw_ema_step(ref_e[0], scaled, ref_e[1], ref_e[2], ref_e[3], step, ema_rate=0.9, **HYPER)
            for off in (0, 1):
                gw, gv = guarded(g, off)
                (_, p), (_, m), (_, v) = runs[off]["plain"]
                assert (p.data_ptr() % 16 != 0) == bool(off)
                engine.op_adamw_clip_step(p, gv, m, v, step, coef=coef, **HYPER)
                for got, want, what in ((p, ref[0], "p"), (m, ref[1], "m"), (v, ref[2], "v")):
                    assert torch.equal(got, want), (float(coef), off, what, step, int((got != want).sum()))
                (_, p), (_, m), (_, v), (_, e) = runs[off]["ema"]
                engine.op_adamw_ema_clip_step(p, gv, m, v, e, step, ema_rate=0.9, coef=coef, **HYPER)
                for got, want, what in ((p, ref_e[0], "p"), (m, ref_e[1], "m"), (v, ref_e[2], "v"), (e, ref_e[3], "ema")):
                    assert torch.equal(got, want), (float(coef), off, "ema run", what, step, int((got != want).sum()))
                assert torch.equal(gv, g) and guards_ok(gw, off, n)
        assert not torch.equal(ref[0], p0) and torch.equal(ref[0], ref_e[0])
        for off in (0, 1):
            assert all(guards_ok(w, off, n) for w, _ in runs[off]["plain"] + runs[off]["ema"])
    assert float(pair[0]) == 123.0 and float(pair[1]) == R.f32(0.37)
    if n == 5:
        from gligen_amd import _lib
        (_, p), (_, g), (_, m), (_, v), (_, e) = (guarded(t, 0) for t in (p0, grads[0], m0, v0, e0))
        with pytest.raises(_lib.GligenAmdError, match="step"):
            engine.op_adamw_clip_step(p, g, m, v, 0, coef=pair[1:2], **HYPER)
        with pytest.raises(_lib.GligenAmdError, match="ema_rate"):
            engine.op_adamw_ema_clip_step(p, g, m, v, e, 1, ema_rate=1.5, coef=pair[1:2], **HYPER)
        assert torch.equal(p, p0) and torch.equal(e, e0)


# ---- 4. the weighted training step
def case(engine):
    """The small text model (CPU and device), its batch, and the unweighted step's (loss, eps, grads)."""
    if not _CASE:
        assert (B, HW) == (2, 16)
        sd_cpu = syn.seeded_state_dict(golden_shapes("unet_small_train_step"), META["weight_seed"])
        sd = {k: v.float().to(engine.device).contiguous() for k, v in sd_cpu.items()}
        b = syn.make_batch("text", B, n_valid=META["n_valid"], seed=5)
        x, noise = syn.make_latent(B, 4, HW, HW, seed=6), syn.make_latent(B, 4, HW, HW, seed=7)
        d = dict(b=b, t=torch.tensor([981, 441][:B], dtype=torch.long), context=syn.make_context(B, seed=6), noise=noise)
        batch = dict(x=x, target=noise, timesteps=d["t"].float(), context=d["context"], boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"])
        _CASE.update(sd_cpu=sd_cpu, sd=sd, d=d, batch=batch, base=engine.unet_train_step(CFG, sd, batch))
    return _CASE


def held_to_oracle(what, got, oracle, bar=1e-5):
    """(loss, eps, grads) of the device against (loss, eps, grads) of the oracle: the relative error of the loss and the rel-MSE of eps
    and of every gradient; returns the report and whether all of it is under the bar of the training step everywhere else in tests/."""
    loss, eps, grads = got
    loss_o, eps_o, grads_o = oracle
    assert sorted(grads) == sorted(grads_o)
    report = {"loss": abs(float(loss) - float(loss_o)) / abs(float(loss_o)), "eps": rel_mse(eps, eps_o)}
    report.update({k: rel_mse(grads[k], grads_o[k]) for k in grads})
    worst = max(report, key=report.get)
    print(f"{what}: loss {float(loss)!r} oracle {float(loss_o)!r} rel err {report['loss']:.3g}; eps {report['eps']:.3g}; worst {worst} {report[worst]:.3g}; "
          f"best gradient {min(v for k, v in report.items() if k not in ('loss', 'eps')):.3g}")
    return report, all(v < bar for v in report.values())


def test_weighted_step_explicit_weights_vs_oracle(engine):
    """loss_weights = (0.125, 1.75): loss, eps and every trainable gradient against autograd through the CPU oracle under the weighted
    loss, rel-MSE < 1e-5; against the UNWEIGHTED oracle the loss (7 % off) and the gradients miss that bar -- every tensor of more than
    one element, and all of the scalar gates but at most two --, so the test sees the weights; a
    following call without weights returns the unweighted bits; a count of weights other than B is refused before anything runs and
    the refusal clears them."""
    from gligen_amd import _lib
    c = case(engine)
    dev = engine.device
    names = trainable_names(c["sd_cpu"], CFG)
    assert len(names) == 127
    w = torch.tensor([0.125, 1.75])
    got = engine.unet_train_step(CFG, c["sd"], c["batch"], loss_weights=w.to(dev))
    w2 = torch.tensor([1.75, 0.125])           # the same weights on the other samples (below)
    got2 = engine.unet_train_step(CFG, c["sd"], c["batch"], loss_weights=w2.to(dev))
    eps_o, ((loss_w, grads_w), (loss_u, grads_u), (loss_w2, grads_w2)) = R.oracle_autograd_weighted(c["sd_cpu"], CFG, "text", names, c["d"], c["batch"]["x"], None,
                                                                                                [w, None, w2])
    report, ok = held_to_oracle("explicit weights", got, (loss_w, eps_o, grads_w))
    assert ok, {k: v for k, v in report.items() if not v < 1e-5}
    report2, ok2 = held_to_oracle("the weights swapped", got2, (loss_w2, eps_o, grads_w2))
    assert ok2, {k: v for k, v in report2.items() if not v < 1e-5}
    wrong, _ = held_to_oracle("explicit weights vs the unweighted oracle", got, (loss_u, eps_o, grads_u))
    live = [k for k in names if float(grads_u[k].abs().max()) > 0]           # (a tensor no sample reaches has no gradient to weigh)
    assert len(live) > 120 and wrong["eps"] < 1e-5 and wrong["loss"] > 1e-2
    # w0 G0 + w1 G1 against G0 + G1: a tensor meets the unweighted gradient only where 0.875 G0 = 0.75 G1, which a scalar gate (one degree
    # of freedom) can come close to by chance; every tensor of more than one element misses the bar, and so do all gates but at most two
    missed = [k for k in live if wrong[k] > 1e-5]
    assert all(wrong[k] > 1e-5 for k in live if grads_u[k].numel() > 1), {k: wrong[k] for k in live if grads_u[k].numel() > 1 and not wrong[k] > 1e-5}
    assert len(missed) >= len(live) - 2, sorted(set(live) - set(missed))
    # with the weights swapped the coincidence would need 0.75 G0 = 0.875 G1 as well, i.e. G0 = G1 = 0: every live tensor, the gates
    # included, misses the unweighted oracle under at least one of the two weightings -- strictly, no exception
    wrong2, _ = held_to_oracle("the weights swapped vs the unweighted oracle", got2, (loss_u, eps_o, grads_u))
    assert wrong2["loss"] > 1e-2 and all(max(wrong[k], wrong2[k]) > 1e-5 for k in live), [k for k in live if not max(wrong[k], wrong2[k]) > 1e-5]
    assert torch.equal(got[1], c["base"][1])                      # (the weights touch the loss and what follows it, not the forward)
    # cleared: the next call is the unweighted step bit for bit
    loss, eps, grads = engine.unet_train_step(CFG, c["sd"], c["batch"])
    assert torch.equal(loss, c["base"][0]) and torch.equal(eps, c["base"][1]) and all(torch.equal(grads[k], c["base"][2][k]) for k in grads)
    assert not torch.equal(got[0], loss)
    # checkpointing and a second run give the weighted bits
    again = engine.unet_train_step(CFG, c["sd"], c["batch"], loss_weights=w.to(dev), checkpoint=True)
    assert torch.equal(again[0], got[0]) and all(torch.equal(again[2][k], got[2][k]) for k in names)
    with pytest.raises(ValueError, match="loss_weights"):
        engine.unet_train_step(CFG, c["sd"], c["batch"], loss_weights=torch.ones(3, device=dev))
    three = torch.ones(3, device=dev)
    _lib.check(engine.lib.gl_train_set_loss_weights(engine._ctx, three.data_ptr(), 3))
    with pytest.raises(_lib.GligenAmdError, match="loss weights"):
        engine.unet_train_step(CFG, c["sd"], c["batch"])
    loss, _, _ = engine.unet_train_step(CFG, c["sd"], c["batch"])
    assert torch.equal(loss, c["base"][0])


def test_weighted_step_min_snr(engine):
    """t = (20, 600), gamma = 5 through min_snr_weights on the reference's schedule: the first weight is below 0.2 and the second exactly
    1, so both branches occur; the step is held to the oracle under those weights."""
    c = case(engine)
    t = torch.tensor([20, 600])
    table = min_snr_weights(R.reference_alphas_cumprod(), 5.0)
    w = table[t]
    assert float(w[0]) < 0.2 and float(w[1]) == 1.0
    names = trainable_names(c["sd_cpu"], CFG)
    d = dict(c["d"], t=t)
    batch = dict(c["batch"], timesteps=t.float())
    got = engine.unet_train_step(CFG, c["sd"], batch, loss_weights=table.to(engine.device)[t.to(engine.device)].contiguous())
    eps_o, ((loss_w, grads_w), (loss_u, grads_u)) = R.oracle_autograd_weighted(c["sd_cpu"], CFG, "text", names, d, batch["x"], None, [w, None])
    report, ok = held_to_oracle("min-SNR weights", got, (loss_w, eps_o, grads_w))
    assert ok, {k: v for k, v in report.items() if not v < 1e-5}
    assert abs(float(got[0]) - float(loss_u)) / float(loss_u) > 1e-3


def test_weighted_step_lora(engine):
    """One LoRA case (rank 4, attention family, random up): loss, eps and every adapter gradient under loss_weights against the
    oracle on the merged weights + the chain rule, the bar of tests/test_lora_train_gpu.py; the call after it is unweighted."""
    import lora_train_ref as L
    from gligen_amd import lora_train as lt
    c = case(engine)
    dev = engine.device
    spec = lt.LoraSpec(4, 8.0, ("attn",))
    t = lt.init_adapters(c["sd_cpu"], CFG, spec, seed=3)
    g = torch.Generator().manual_seed(17)
    t = {k: (torch.randn(v.shape, generator=g) * 0.03 if k.endswith(lt.UP) else v) for k, v in t.items()}
    sites = lt.adapter_sites(c["sd_cpu"], spec)
    arr = lambda: [dict(name=s, down=t[s[:-7] + lt.DOWN].to(dev), up=t[s[:-7] + lt.UP].to(dev), scale=spec.scale) for s in sites]
    w = torch.tensor([0.125, 1.75])
    loss, eps, _, ag = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=arr(), trainable=[], loss_weights=w.to(dev))
    merged = dict(c["sd_cpu"])
    for s in sites:
        W = c["sd_cpu"][s]
        merged[s] = (W.double() + spec.scale * (t[s[:-7] + lt.UP].double() @ t[s[:-7] + lt.DOWN].double()).reshape(W.shape)).float()
    eps_o, ((loss_o, dW),) = R.oracle_autograd_weighted(merged, CFG, "text", sites, c["d"], c["batch"]["x"], None, [w])
    report = {"loss": abs(float(loss) - float(loss_o)) / float(loss_o), "eps": rel_mse(eps, eps_o)}
    for s in sites:
        gd_o, gu_o = L.chain_rule(dW[s], t[s[:-7] + lt.DOWN], t[s[:-7] + lt.UP], spec.scale)
        report[s + " g_down"], report[s + " g_up"] = rel_mse(ag[s][0], gd_o), rel_mse(ag[s][1], gu_o)
    worst = max(report, key=report.get)
    print("weighted LoRA step: loss", float(loss), "oracle", float(loss_o), "worst", worst, report[worst])
    assert not {k: v for k, v in report.items() if not v < 1e-5}, {k: v for k, v in report.items() if not v < 1e-5}
    plain = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=arr(), trainable=[])
    again = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=arr(), trainable=[])
    assert torch.equal(plain[0], again[0]) and not torch.equal(plain[0], loss)


def test_weighted_step_inpainting(engine):
    """One inpainting case (the 9-channel first conv, its weight trained): the set-and-clear route on a second entry point's inputs,
    held to the oracle under the weights."""
    from test_train_inpaint_cpu import CASES, golden_inputs, inpaint_shapes, reference_batch
    g = load_golden(CASES["text"])
    d = golden_inputs(g)
    cfg = g["meta"]["cfg"]
    sd_cpu = syn.seeded_state_dict(inpaint_shapes("text"), g["meta"]["weight_seed"])
    sd = {k: v.float().to(engine.device).contiguous() for k, v in sd_cpu.items()}
    batch = reference_batch(g, d)
    names = trainable_names(sd_cpu, cfg)
    assert len(names) == 128 and "input_blocks.0.0.weight" in names
    w = torch.tensor([1.75, 0.125])
    base = engine.unet_train_step(cfg, sd, batch)
    got = engine.unet_train_step(cfg, sd, batch, loss_weights=w.to(engine.device))
    eps_o, ((loss_o, grads_o),) = R.oracle_autograd_weighted(sd_cpu, cfg, "text", names, d, batch["x"], batch["inpainting_extra_input"], [w])
    report, ok = held_to_oracle("weighted inpainting step", got, (loss_o, eps_o, grads_o))
    assert ok, {k: v for k, v in report.items() if not v < 1e-5}
    after = engine.unet_train_step(cfg, sd, batch)
    assert torch.equal(after[0], base[0]) and not torch.equal(got[0], base[0]) and all(torch.equal(after[2][k], base[2][k]) for k in names)


# ---- 5. TrainStep end to end
def micro_batches():
    """Four batches of the small model: two optimizer steps of two micro-batches."""
    out = []
    for i in range(4):
        b = syn.make_batch("text", B, n_valid=META["n_valid"], seed=5 + i)
        out.append(dict(x=syn.make_latent(B, 4, HW, HW, seed=60 + i), timesteps=torch.tensor([981 - 100 * i, 441 + 50 * i][:B]).float(), context=syn.make_context(B, seed=6 + i),
                        boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"], target=syn.make_latent(B, 4, HW, HW, seed=70 + i)))
    return out


def test_train_step_accumulates_and_clips_vs_float64(engine):
    """K = 2, max_grad_norm = half the first norm, two optimizer steps. The float64 restatement is driven by the per-micro-batch
    gradients the engine itself returns on the same batches and parameters (grads=None): mean, norm, coefficient, AdamW, with the
    elementwise bound of the fp32 op chain carried along (train_run_ref.Adam64) -- every parameter stays inside it, and grad_norm
    inside the norm's bound. overlap=True and overlap=False are torch.equal; the gradient buckets keep the unclipped mean."""
    c = case(engine)
    dev = engine.device
    names = trainable_names(c["sd_cpu"], CFG)
    batches = micro_batches()
    lr, wd = float(META["lr"]), 0.01
    probe = [engine.unet_train_step(CFG, c["sd"], b, checkpoint=True)[2] for b in batches[:2]]
    first64 = float(sum(((probe[0][k].double() + probe[1][k].double()) / 2).pow(2).sum() for k in names).sqrt())
    mx = R.f32(0.5 * first64)
    assert mx > 0

    def run(**kw):
        ts = TrainStep(engine, CFG, c["sd_cpu"], lr=lr, weight_decay=wd, bucket_mb=32.0, world=1, accumulate=2, max_grad_norm=mx, **kw)
        micro, norms, coefs, means = [], [], [], []
        for step in range(2):
            pair = batches[2 * step:2 * step + 2]
            micro.append([{k: v.clone() for k, v in engine.unet_train_step(CFG, ts.params, b, checkpoint=True)[2].items()} for b in pair])
            assert ts.at_boundary
            ts.step(pair[0])
            assert ts.micro == 1 and not ts.at_boundary and ts.steps == step
            ts.step(pair[1])
            assert ts.at_boundary and ts.steps == step + 1
            torch.cuda.synchronize()
            norms.append(float(ts.grad_norm)); coefs.append(float(ts._coef)); means.append({k: v.clone() for k, v in ts.gbuf.views.items()})
        return ts, micro, norms, coefs, means

    ts, micro, norms, coefs, means = run()
    nb = len(ts.gbuf.buckets)
    assert nb >= 4 and len(ts.acc) == nb
    n_total, count = sum(b.numel() for b in ts.gbuf.buckets), ts._partials.numel()
    ref = {k: R.Adam64(c["sd_cpu"][k]) for k in names}
    u = R.U32
    for step in range(2):
        mean64 = {k: (micro[step][0][k].double().cpu() + micro[step][1][k].double().cpu()) / 2 for k in names}
        for k in names:       # the gradient buffer holds the unclipped fp32 mean (g1 + g2) * 0.5
            assert torch.equal(means[step][k], R.accumulate_ref([micro[step][0][k], micro[step][1][k]])), (step, k)
        norm64 = float(sum(v.pow(2).sum() for v in mean64.values()).sqrt())
        # the kernel sums the fp32 mean, every element within u of mean64: the norm moves by at most u norm64 on top of its own bound
        nbound = R.norm_bound(norm64, n_total, count=count) * (1 + u) + u * norm64
        print(f"step {step + 1}: grad_norm {norms[step]!r} float64 {norm64!r} |diff| / bound {abs(norms[step] - norm64) / nbound:.3f} coef {coefs[step]!r}")
        assert abs(norms[step] - norm64) <= nbound, (step, norms[step], norm64, nbound)
        coef64 = R.coef_ref(norm64, mx)
        cbound = R.coef_bound(norm64, n_total, mx, count=count) + 2 * u * coef64
        assert abs(coefs[step] - coef64) <= cbound and coefs[step] < 1.0
        if step == 0:
            assert abs(norm64 - first64) <= 1e-12 * first64 and 0.49 < coefs[0] < 0.51
        rel_g = (1 + u) * (1 + cbound / coef64) * (1 + u) - 1            # the mean's rounding, the coefficient's error, the product's rounding
        k32 = R.adamw_scalars32(lr, (0.9, 0.999), 1e-8, wd, step + 1)
        for k in names:
            gp = mean64[k] * coef64
            ref[k].step(gp, gp.abs() * rel_g, k32)
    worst, unbounded, total, moved = 0.0, 0, 0, 0
    for k in names:
        got = ts.params[k].double().cpu()
        err = (got - ref[k].p).abs()
        ok = err <= ref[k].Ep
        assert bool(ok.all()), (k, float(err.max()), float(ref[k].Ep[~ok].max()))
        finite = torch.isfinite(ref[k].Ep)
        # where the chain's bound is infinite the element is still held: over its first two steps AdamW moves a parameter by at most
        # 1.002 lr per step (|m_hat| / sqrt(v_hat) <= 1 at t = 1; at t = 2, m = 0.09 g1 + 0.1 g2 and v = 0.000999 g1^2 + 0.001 g2^2 give, by
        # Cauchy-Schwarz, sqrt(0.09^2 / 0.000999 + 0.1^2 / 0.001) sqrt(0.001999) / 0.19 = 1.0014) plus the decay lr wd |p|, in the kernel
        # and in float64 alike: both stay that close to the start
        p0 = c["sd_cpu"][k].double()
        reach = 2 * (1.002 * lr + lr * wd * (p0.abs() + 2.004 * lr)) * (1 + 8 * u)
        assert bool(((got - p0).abs() <= reach).all()) and bool((err[~finite] <= 2 * reach[~finite]).all()), k
        if bool(finite.any()):
            worst = max(worst, float((err[finite] / ref[k].Ep[finite].clamp_min(1e-300)).max()))
            assert float(ref[k].Ep[finite].max()) < 0.01 * lr + 16 * u * float(ref[k].p.abs().max()), k     # far below one update of ~lr: the bound can fail
        unbounded += ref[k].unbounded
        total += got.numel()
        moved += int((got != c["sd_cpu"][k].double()).sum())
    print(f"two clipped optimizer steps over K = 2: worst |p - float64| / bound {worst:.3f}; {unbounded} of {2 * total} quotients unbounded; {moved} of {total} moved")
    assert unbounded <= 0.001 * 2 * total and moved > 0.5 * total
    one = run(overlap=False)
    assert one[2] == norms and one[3] == coefs
    assert all(torch.equal(a, b) for a, b in zip(ts.pbuf.buckets, one[0].pbuf.buckets))
    assert all(torch.equal(a, b) for a, b in zip(ts.m + ts.v, one[0].m + one[0].v))
    ema = run(ema_rate=0.5)          # the fused clipped update + EMA: the same parameters
    assert all(torch.equal(a, b) for a, b in zip(ts.pbuf.buckets, ema[0].pbuf.buckets)) and not torch.equal(ema[0].ema[0], ema[0].pbuf.buckets[0])
    engine.train_weight_cache(False)


def test_lora_train_step_with_the_same_options(engine):
    """LoraTrainStep with accumulate = 2 and clipping runs; its first optimizer step moves no adapter element by more than lr, as AdamW
    bounds a first step (|m_hat / (sqrt(v_hat) + eps)| <= 1; 16 fp32 roundings allowed for the scalars and the operations of the
    update), and the norm is above max_grad_norm, so the step is clipped."""
    from gligen_amd import lora_train as lt
    c = case(engine)
    lr = 1e-3
    batches = micro_batches()
    ts = lt.LoraTrainStep(engine, CFG, c["sd_cpu"], lt.LoraSpec(4, 8.0, ("attn", "ff", "proj")), lr=lr, weight_decay=0.0, world=1, seed=3, accumulate=2, max_grad_norm=1e-4)
    start = {k: v.clone() for k, v in ts.adapter_tensors().items()}
    ts.step(batches[0])
    assert not ts.at_boundary and all(torch.equal(v, start[k]) for k, v in ts.adapter_tensors().items())
    ts.step(batches[1])
    torch.cuda.synchronize()
    after = ts.adapter_tensors()
    assert ts.at_boundary and ts.steps == 1 and float(ts.grad_norm) > 1e-4 and 0 < float(ts._coef) < 1
    step = max(float((after[k] - start[k]).abs().max()) for k in after)
    print("LoRA first clipped step: largest move", step, "lr", lr)
    assert 0 < step <= lr * (1 + 16 * R.U32)
    assert any(not torch.equal(after[k], start[k]) for k in after if k.endswith(lt.UP))
    engine.train_weight_cache(False)


_RCCL_ALONE = r"""
import os, socket, sys, torch
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import torch.distributed as dist
s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)
from gligen_amd.dist import GradBuckets
from gligen_amd.engine import Engine
from gligen_amd.train import TrainStep
import test_train_run_gpu as T
eng = Engine(0, arena_gb=6.0)
c = T.case(eng)
batches = T.micro_batches()
calls = []
real = GradBuckets.all_reduce_bucket
def counted(self, i, average=True, even_alone=False):
    n = real(self, i, average, even_alone)
    calls.append(n)
    return n
GradBuckets.all_reduce_bucket = counted
out = {}
probe = TrainStep(eng, T.CFG, c["sd_cpu"], lr=1e-3, bucket_mb=32.0, world=1, accumulate=2, max_grad_norm=1e30)
probe.step(batches[0]); probe.step(batches[1])
half = 0.5 * float(probe.grad_norm)            # clip to half the first norm
assert float(probe._coef) == 1.0 and half > 0
for name, kw in (("none", {}), ("rccl", dict(exchange_even_alone=True))):
    del calls[:]
    ts = TrainStep(eng, T.CFG, c["sd_cpu"], lr=1e-3, weight_decay=0.01, bucket_mb=32.0, world=1, accumulate=2, max_grad_norm=half, **kw)
    for b in batches:
        ts.step(b)
    torch.cuda.synchronize()
    nb = len(ts.gbuf.buckets)
    assert len(calls) == 2 * nb and sum(calls) == (0 if name == "none" else 2 * 2 * nb), (name, calls)      # exchanges at the two boundaries only
    out[name] = ([b.clone() for b in ts.pbuf.buckets], float(ts.grad_norm), float(ts._coef))
assert out["none"][1:] == out["rccl"][1:] and 0 < out["none"][2] < 1, (out["none"][1:], out["rccl"][1:])
assert all(torch.equal(a, b) for a, b in zip(out["none"][0], out["rccl"][0]))
eng.train_weight_cache(False)
eng.close()
dist.barrier(); dist.destroy_process_group()
print("accumulate + clip through rccl alone ok")
"""


def test_exchange_even_alone_gives_the_same_bits(tmp_path):
    """The RCCL world-of-one arm (tests/test_ops_gpu.py has it for the plain step) with accumulate = 2 and clipping: every bucket goes
    through reduce-scatter + all-gather at the two boundaries and nowhere else, and parameters, norm and coefficient are those of the
    run without an exchange, bit for bit."""
    script = tmp_path / "rccl_alone.py"
    script.write_text(_RCCL_ALONE)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "accumulate + clip through rccl alone ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- 6. the Trainer through its command line
def test_trainer_resumes_bit_for_bit_and_refuses_another_k(tmp_path):
    """python -m gligen_amd.trainer --small --latent 16 --batch_size 2 --gradient_accumulation_steps 2 --max_grad_norm 1.0 --min_snr_gamma 5
    (with an EMA, so the fused clipped update runs): four iterations in one run against two, a stop and two resumed -- parameters,
    EMA, both moments and the position of the random streams (which a batch stream out of step would have moved) are equal bit for
    bit; resuming with K = 3 is refused, naming the key."""
    from gligen_amd import trainer
    common = ["--synthetic", "text", "--small", "--latent", "16", "--batch_size", "2", "--gradient_accumulation_steps", "2", "--max_grad_norm", "1.0",
              "--min_snr_gamma", "5", "--enable_ema", "true", "--ema_rate", "0.9", "--warmup_steps", "2", "--base_learning_rate", "1e-3", "--weight_decay", "0.01",
              "--arena_gb", "4", "--seed", "5"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert trainer.main(common + ["--total_iters", "4", "--output_dir", a]) == 0
    assert trainer.main(common + ["--total_iters", "2", "--output_dir", b]) == 0
    two = trainer.read_checkpoint(os.path.join(b, "checkpoint_latest.pth"))
    assert two["iters"] == 2 and two["config_dict"]["gradient_accumulation_steps"] == 2 and two["config_dict"]["max_grad_norm"] == 1.0 \
        and two["config_dict"]["min_snr_gamma"] == 5.0
    assert trainer.main(common + ["--total_iters", "4", "--output_dir", b, "--resume"]) == 0
    one, res = trainer.read_checkpoint(os.path.join(a, "checkpoint_latest.pth")), trainer.read_checkpoint(os.path.join(b, "checkpoint_latest.pth"))
    assert one["iters"] == res["iters"] == 4 and float(one["opt"]["state"][0]["step"]) == 4
    for part in ("model", "ema"):
        bad = [k for k in one[part] if not torch.equal(one[part][k], res[part][k])]
        assert not bad, (part, len(bad), bad[:5])
    for i in one["opt"]["state"]:
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(one["opt"]["state"][i][key], res["opt"]["state"][i][key]), (i, key)
    assert len(one["opt"]["state"]) == 127
    assert torch.equal(one["rng"]["device"], res["rng"]["device"]) and one["rng"]["python"] == res["rng"]["python"]
    assert any(not torch.equal(two["model"][k], res["model"][k]) for k in two["model"]), "iterations three and four moved the model"
    other = list(common)
    other[other.index("--gradient_accumulation_steps") + 1] = "3"
    with pytest.raises(ValueError, match="gradient_accumulation_steps"):
        trainer.main(other + ["--total_iters", "6", "--output_dir", b, "--resume"])
