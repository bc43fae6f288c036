"""Training LoRA adapters on a real MI355X: the four kernels of csrc/train_lora.hip by themselves (gl_op_lora_linear) against float64,
element by element, behind guard zones; the training step with adapters (gl_unet_train_step_lora) against the unadapted step bit
for bit (up = 0) and against autograd through the CPU oracle on the merged weights; LoraTrainStep against the oracle +
torch.optim.AdamW; the saved adapter merged back into the inference model; the trainer's --lora_* options, stopped and resumed."""
import os
import subprocess
import sys

import pytest
import torch

import lora_train_ref as R
import train_prims_ref as P
from helpers import ROOT, golden_shapes, load_golden
from gligen_amd import synthetic as syn

pytestmark = pytest.mark.gpu


# ---- the kernels alone
def _report(rows, problems):
    print("\n".join(P.format_rows(rows)))
    assert not problems, problems
    bad = P.failures(rows)
    assert not bad, P.format_rows(bad)


@pytest.mark.parametrize("kn", range(len(R.KN)), ids=[f"K{k}-N{n}" for k, n in R.KN])
def test_lora_kernels_vs_float64(engine, kn):
    """t, y, u, dx, g_down, g_up of one adapted Linear's low-rank part at every M of the issue (1, 63, 154, 272 and one below, at, one
    above and 2x + 17 of the weight gradient's row chunk) against float64, every element within the bound of its addition chain;
    guard zones intact, nothing left unwritten, a second call the same bits."""
    rows, problems = [], []
    for M, K, N, r, dkr, urn in R.kernel_cases(kn):
        a, b = R.run_lora_linear(engine, M, K, N, r, dkr, urn)
        rows += a
        problems += b
    _report(rows, problems)


def test_lora_kernels_every_rank_and_orientation(engine):
    """Every rank (1, 4, 24, 128) against both layouts of both small operands."""
    rows, problems = [], []
    for case in R.cross_cases():
        a, b = R.run_lora_linear(engine, *case)
        rows += a
        problems += b
    _report(rows, problems)


def test_lora_kernels_operand_layout_exact(engine):
    """Exact-integer inputs with an asymmetric small operand: every output equals float64 bit for bit (a lane-map or transposed-write
    mistake cannot hide in a tolerance), for every rank tile count, both orientations and a ragged row edge on each side of the
    weight gradient's chunk."""
    rows, problems = [], []
    cases = [(154, 320, 320, r, dkr, urn) for r in R.RANKS for dkr, urn in R.ORIENTATIONS]
    cases += [(R.CHUNK + 1, 64, 64, 24, False, False), (2 * R.CHUNK + 17, 320, 2560, 4, True, True), (63, 1280, 320, 128, False, True),
              (1, 768, 320, 1, True, False), (272, 320, 2560, 128, False, False), (77 * 2, 768, 320, 24, False, False)]
    for case in cases:
        a, b = R.run_lora_linear(engine, *case, exact=True)
        rows += a
        problems += b
    print("\n".join(P.format_rows(rows)))
    assert not problems, problems
    assert all(err == 0.0 for _, _, err, _ in rows), [r for r in rows if r[2] != 0.0]


def test_lora_linear_limits_are_refused(engine):
    """rank outside 1..128, K or N that is no multiple of 64: each refused by a message that names it."""
    from gligen_amd._lib import GligenAmdError
    x, dy = torch.zeros(8, 64), torch.zeros(8, 64)
    with pytest.raises(GligenAmdError, match="rank 129"):
        engine.op_lora_linear(x, torch.zeros(129, 64), torch.zeros(64, 129), dy=dy)
    with pytest.raises(GligenAmdError, match="K = 96"):
        engine.op_lora_linear(torch.zeros(8, 96), torch.zeros(4, 96), torch.zeros(64, 4))
    with pytest.raises(GligenAmdError, match="N = 32"):
        engine.op_lora_linear(x, torch.zeros(4, 64), torch.zeros(32, 4))
    assert engine.lora_wgrad_chunk_rows(1) == R.CHUNK and all(engine.lora_wgrad_chunk_rows(m) == R.wgrad_chunk_rows(m) for m in (255, 8192, 8193, 16384, 100000))


# ---- the training step with adapters: the small two-level UNet, B = 2, 16 x 16 latent, text tokenizer
META = load_golden("unet_small_train_step")["meta"]
CFG, B, HW = META["cfg"], META["B"], META["hw"]
FAMILY_SETS = [("attn",), ("ff",), ("proj",), ("attn", "ff", "proj")]
RANK, ALPHA = 4, 8.0          # scale 2
_CASE, _STEPS, _TWO = {}, {}, {}      # computed once, shared, never written


def case(engine):
    """The state_dict (CPU and device), the batch and the unadapted step's (loss, eps, grads)."""
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


def adapters_for(engine, families, zero_up=False):
    """(spec, CPU tensors under init_adapters' keys, the engine's adapter list on the device)."""
    from gligen_amd import lora_train as lt
    c = case(engine)
    spec = lt.LoraSpec(RANK, ALPHA, families)
    t = lt.init_adapters(c["sd_cpu"], CFG, spec, seed=3)
    if not zero_up:
        g = torch.Generator().manual_seed(17)
        t = {k: (torch.randn(v.shape, generator=g) * 0.03 if k.endswith(lt.UP) else v) for k, v in t.items()}
    dev = engine.device
    arr = [dict(name=w, down=t[w[:-7] + lt.DOWN].to(dev), up=t[w[:-7] + lt.UP].to(dev), scale=spec.scale) for w in lt.adapter_sites(c["sd_cpu"], spec)]
    return spec, t, arr


def merged(sd_cpu, tensors, scale):
    """sd_cpu with W + scale up down (float64, rounded once) at every adapted weight."""
    from gligen_amd import lora_train as lt
    out = dict(sd_cpu)
    for k, down in tensors.items():
        if k.endswith(lt.DOWN):
            w = k[:-len(lt.DOWN)] + ".weight"
            W = sd_cpu[w]
            out[w] = (W.double() + scale * (tensors[k[:-len(lt.DOWN)] + lt.UP].double() @ down.double()).reshape(W.shape)).float()
    return out


def adapted_step(engine, families):
    if families not in _STEPS:
        c = case(engine)
        spec, t, arr = adapters_for(engine, families)
        _STEPS[families] = (spec, t, arr, engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=arr))
    return _STEPS[families]


def test_zero_up_adds_exact_zeros(engine):
    """With up = 0 (how training starts) loss, eps and every base gradient are torch.equal to the step without adapters; g_down is
    exactly zero and g_up is not. An empty adapter list is the unadapted step too."""
    c = case(engine)
    loss0, eps0, grads0 = c["base"]
    _, _, arr = adapters_for(engine, FAMILY_SETS[3], zero_up=True)
    loss, eps, grads, ag = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=arr)
    assert torch.equal(loss, loss0) and torch.equal(eps, eps0)
    assert sorted(grads) == sorted(grads0) and len(grads) == 127
    assert all(torch.equal(grads[k], grads0[k]) for k in grads0), [k for k in grads0 if not torch.equal(grads[k], grads0[k])][:5]
    assert len(ag) == 84 and all(int(torch.count_nonzero(gd)) == 0 for gd, _ in ag.values())
    assert all(bool(torch.isfinite(gu).all()) and int(torch.count_nonzero(gu)) > 0 for _, gu in ag.values())
    loss_e, eps_e, grads_e, ag_e = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=[])
    assert not ag_e and torch.equal(loss_e, loss0) and torch.equal(eps_e, eps0) and all(torch.equal(grads_e[k], grads0[k]) for k in grads0)


@pytest.mark.parametrize("families", FAMILY_SETS, ids=["attn", "ff", "proj", "all"])
def test_adapted_step_vs_oracle_autograd(engine, families):
    """Random up: loss, eps and every adapter gradient against autograd through the CPU oracle on W + s up down (the gradient of the
    merged weight, then the chain rule in float64), rel-MSE < 1e-5, the bar of the training step everywhere else."""
    from gligen_amd import lora_train as lt
    from test_train_inpaint_cpu import oracle_autograd
    c = case(engine)
    spec, t, arr, (loss, eps, grads, ag) = adapted_step(engine, families)
    sites = [a["name"] for a in arr]
    loss_o, eps_o, dW = oracle_autograd(merged(c["sd_cpu"], t, spec.scale), CFG, "text", sites, c["d"], c["batch"]["x"], None)
    assert not torch.equal(eps.cpu(), c["base"][1].cpu()), "the adapters change the output"
    loss_err = abs(float(loss) - float(loss_o)) / float(loss_o)
    report = {"eps": R.rel_mse(eps, eps_o)}
    for w in sites:
        gd_o, gu_o = R.chain_rule(dW[w], t[w[:-7] + lt.DOWN], t[w[:-7] + lt.UP], spec.scale)
        report[w + " g_down"], report[w + " g_up"] = R.rel_mse(ag[w][0], gd_o), R.rel_mse(ag[w][1], gu_o)
    worst = max(report, key=report.get)
    print(families, "adapted step: loss", float(loss), "oracle", float(loss_o), "rel err", loss_err, "eps", report["eps"], "worst", worst, report[worst])
    assert loss_err < 1e-5 and not {k: v for k, v in report.items() if not v < 1e-5}, (loss_err, {k: v for k, v in report.items() if not v < 1e-5})


def test_checkpoint_and_adapters_only_give_the_same_bits(engine):
    """checkpoint=True gives the bits of checkpoint=False; adapters alone (no base gradient asked for) give the adapter gradients of
    the step that also trains the reference's set, bit for bit; two runs give the same bits; the refusals name what they refuse."""
    from gligen_amd._lib import GligenAmdError
    c = case(engine)
    spec, t, arr, (loss, eps, grads, ag) = adapted_step(engine, FAMILY_SETS[3])
    same = lambda a, b: sorted(a) == sorted(b) and all(torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) for k in a)
    fresh = lambda: [dict(a) for a in arr]       # (no g_down / g_up: new gradient tensors per call)
    engine.train_weight_cache(True)        # (read only by the call that asks for it)
    for kw in (dict(checkpoint=True), dict(), dict(checkpoint=True, use_weight_cache=True)):
        loss_c, eps_c, grads_c, ag_c = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=fresh(), **kw)
        assert torch.equal(loss_c, loss) and torch.equal(eps_c, eps), kw
        assert all(torch.equal(grads_c[k], grads[k]) for k in grads) and same(ag_c, ag), kw
    loss_a, eps_a, grads_a, ag_a = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=fresh(), trainable=[])
    assert not grads_a and torch.equal(loss_a, loss) and torch.equal(eps_a, eps) and same(ag_a, ag)
    engine.train_weight_cache(False)
    site = arr[0]["name"]
    with pytest.raises(GligenAmdError, match="frozen"):          # an adapted weight takes no gradient of its own
        engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=fresh(), grads={site: torch.zeros_like(c["sd"][site])})
    fuser = next(k for k in c["sd"] if k.endswith(".fuser.attn.to_q.weight"))
    bad = dict(arr[0], name=fuser)
    with pytest.raises(GligenAmdError, match="fuser"):
        engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=[bad])
    with pytest.raises(GligenAmdError, match="frozen"):
        engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=fresh(), trainable=["out.2.weight"])


def two_steps(engine):
    """LoraTrainStep (adapters alone, all three families, world 1, lr 1e-3), two steps on the batch."""
    if not _TWO:
        from gligen_amd import lora_train as lt
        c = case(engine)
        spec = lt.LoraSpec(RANK, ALPHA, FAMILY_SETS[3])
        ts = lt.LoraTrainStep(engine, CFG, c["sd_cpu"], spec, lr=1e-3, weight_decay=0.0, world=1, seed=3)
        start = {k: v.cpu() for k, v in ts.adapter_tensors().items()}
        losses = [float(ts.step(c["batch"])[0]) for _ in range(2)]
        torch.cuda.synchronize()
        _TWO.update(ts=ts, spec=spec, start=start, losses=losses, after={k: v.cpu() for k, v in ts.adapter_tensors().items()},
                    base_after={k: v.cpu() for k, v in ts.state_dict().items()}, milestones=dict(ts.milestone), ready=list(ts.bucket_ready))
        engine.train_weight_cache(False)
    return _TWO


def test_two_lora_train_steps_vs_oracle_adamw(engine):
    """Two LoraTrainStep iterations from up = 0: the base model keeps its bits, the first loss is the base model's, up moves in the
    first step and down in the second (its first gradient is exactly zero), and both losses match oracle autograd on the merged
    weights + the chain rule + torch.optim.AdamW on the CPU under the inpainting two-step test's tolerance."""
    from gligen_amd import lora_train as lt
    from test_train_inpaint_cpu import oracle_autograd
    c, r = case(engine), two_steps(engine)
    spec, start, after = r["spec"], r["start"], r["after"]
    assert all(torch.equal(r["base_after"][k], v) for k, v in c["sd_cpu"].items())
    assert r["losses"][0] == float(c["base"][0])
    assert len(after) == 168 and all(not torch.equal(after[k], start[k]) for k in after)
    assert all(int(torch.count_nonzero(start[k])) == 0 for k in start if k.endswith(lt.UP))
    sites = lt.adapter_sites(c["sd_cpu"], spec)
    params = {k: v.clone().requires_grad_(True) for k, v in start.items()}
    opt = torch.optim.AdamW(list(params.values()), lr=1e-3, weight_decay=0.0)
    ref_losses = []
    for _ in range(2):
        opt.zero_grad()
        cur = {k: v.detach() for k, v in params.items()}
        loss, _, dW = oracle_autograd(merged(c["sd_cpu"], cur, spec.scale), CFG, "text", sites, c["d"], c["batch"]["x"], None)
        ref_losses.append(float(loss))
        for w in sites:
            gd, gu = R.chain_rule(dW[w], cur[w[:-7] + lt.DOWN], cur[w[:-7] + lt.UP], spec.scale)
            params[w[:-7] + lt.DOWN].grad, params[w[:-7] + lt.UP].grad = gd.float(), gu.float()
        opt.step()
    print("LoRA train steps: losses", r["losses"], "oracle + AdamW", ref_losses)
    for a, ref in zip(r["losses"], ref_losses):
        assert abs(a - ref) / ref < 1e-4, (r["losses"], ref_losses)
    # the buckets go out in the order the gradients become final: the last SpatialTransformer's first
    assert sorted(set(r["milestones"].values())) == list(range(7)) and r["ready"] == sorted(r["ready"], reverse=True)


def test_trained_adapter_round_trips_to_inference(engine, tmp_path):
    """The trained adapter saved in kohya's format, merged into the inference model by apply_loras: every adapted parameter is
    W + s up down within lora_ref's bound for the merge, and eps of the inference path matches the oracle's forward on the merged
    weights at the small-UNet parity bar."""
    import lora_ref
    from gligen_amd import lora, lora_train as lt
    from helpers import build_product_unet, grounding_kwargs, mse, oracle_cfg
    from oracle import gligen_oracle as orc
    from test_path_gpu import EPS_MSE_TOL
    c, r = case(engine), two_steps(engine)
    path = str(tmp_path / "trained.safetensors")
    r["ts"].save_adapter(path, dtype=torch.float32)
    dev = engine.device
    model = build_product_unet(CFG, "text", device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in c["sd_cpu"].items()}, strict=True)
    report = lora.apply_loras(model, None, [(path, 1.0)])
    assert len(report["adapters"][0]["unet"]) == 84 and not report["skipped"]
    got = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for w in lt.adapter_sites(c["sd_cpu"], r["spec"]):
        W, down, up = c["sd_cpu"][w], r["after"][w[:-7] + lt.DOWN], r["after"][w[:-7] + lt.UP]
        err = (got[w].double() - lora_ref.merge64(W, up, down, r["spec"].scale)).abs()
        assert bool((err <= lora_ref.merge_bound(W, up, down, r["spec"].scale)).all()), w
    d = c["d"]
    to = lambda m: {k: v.to(dev) for k, v in m.items()}
    gin = model.grounding_tokenizer_input.prepare(to(d["b"]))
    eps = model(dict(x=c["batch"]["x"].to(dev), timesteps=d["t"].to(dev), context=d["context"].to(dev), grounding_input=gin, inpainting_extra_input=None,
                     grounding_extra_input=None))
    eps_o = orc.unet_forward(merged(c["sd_cpu"], r["after"], r["spec"].scale), oracle_cfg(CFG, "text"),
                             dict(x=c["batch"]["x"], timesteps=d["t"], context=d["context"], grounding_input=grounding_kwargs("text", d["b"]), inpainting_extra_input=None))
    err = mse(eps, eps_o)
    model._drop_engine()
    print("trained adapter merged into the inference path: eps MSE", err)
    assert err < EPS_MSE_TOL, err


def test_trainer_lora_run_resumes_bit_for_bit(tmp_path):
    """python -m gligen_amd.trainer --synthetic text --small --latent 16 --lora_rank 4: three iterations in one go against two, a stop,
    and a resumed third: the adapter files are equal bit for bit, and the checkpoint carries the adapters and their optimizer state."""
    from gligen_amd import lora, trainer
    common = ["--synthetic", "text", "--small", "--latent", "16", "--lora_rank", "4", "--batch_size", "2", "--warmup_steps", "0", "--base_learning_rate", "1e-3",
              "--arena_gb", "4", "--seed", "5"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert trainer.main(common + ["--total_iters", "3", "--output_dir", a]) == 0
    assert trainer.main(common + ["--total_iters", "2", "--output_dir", b]) == 0
    two = lora.read_safetensors(os.path.join(b, "lora.safetensors"))
    assert trainer.main(common + ["--total_iters", "3", "--output_dir", b, "--resume"]) == 0
    one, resumed = lora.read_safetensors(os.path.join(a, "lora.safetensors")), lora.read_safetensors(os.path.join(b, "lora.safetensors"))
    assert sorted(one) == sorted(resumed) and len(one) == 3 * 56
    assert all(torch.equal(one[k], resumed[k]) for k in one), [k for k in one if not torch.equal(one[k], resumed[k])][:5]
    assert any(not torch.equal(two[k], resumed[k]) for k in two), "the third iteration moved the adapter"
    ck = trainer.read_checkpoint(os.path.join(b, "checkpoint_latest.pth"))
    assert ck["iters"] == 3 and len(ck["lora"]) == 2 * 56 and len(ck["opt"]["state"]) == 2 * 56
    assert len(lora.parse_adapter(resumed)) == 56
