"""LoRA adapters on 3 x 3 convs on a real MI355X: the kernels of csrc/train_lora_conv.hip by themselves (gl_op_lora_conv3, with the
lora_up / lora_down / lora_wgrad kernels of csrc/train_lora.hip it reuses) against float64, element by element, behind guard zones,
for the three geometries (stride 1, Downsample, Upsample), and the refusals by name; the training step with conv-family adapters
(conv, emb, sample) against the unadapted step bit for bit (up = 0) and against autograd through the CPU oracle on the merged
weights; LoraTrainStep against the oracle + torch.optim.AdamW; the saved adapter merged into the inference model and removed again;
the trainer's --lora_conv_* options, stopped and resumed.

Every test prints its figures; with GLIGEN_LORA_CONV_REPORT naming a directory the worst err / bound per tensor of each kernel test is
also appended to err_over_bound.txt there and the worst value of each step run to step_vs_oracle.txt (profiles/lora_conv/ keeps one
such run)."""
import os

import pytest
import torch

import lora_conv_ref as R
import train_prims_ref as P

pytestmark = pytest.mark.gpu


def _report(what, rows, problems):
    print("\n".join(P.format_rows(rows)))
    worst = {}
    for _, name, err, bound in rows:
        ratio = err / bound if bound else err
        worst[name] = max(worst.get(name, 0.0), ratio)
    line = f"{what:34s} " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items())
    print("[lora_conv worst err/bound]", line)
    out = os.environ.get("GLIGEN_LORA_CONV_REPORT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "err_over_bound.txt"), "a") as f:
            f.write(line + "\n")
    assert not problems, problems


def _run(engine, what, cases, exact=False):
    rows, problems = [], []
    for c in cases:
        a, b = R.run_lora_conv3(engine, c, exact=exact)
        rows += a
        problems += b
    _report(what, rows, problems)
    return rows


@pytest.mark.parametrize("geom", [0, 1, 2], ids=["conv", "down", "up"])
def test_lora_conv_kernels_every_image(engine, geom):
    """t, y, u, dx, g_down, g_up of one adapted conv's low-rank part on every image of the geometry (stride 1: 1 x 1, 2 x 2, 3 x 5 --
    two images inside one 64-row workgroup --, 63 / 64 / 65 rows per image, both sides of the weight gradient's 256-row chunk, B = 1;
    Downsample: one output pixel, 6 x 4, 16 x 34; Upsample: 1 x 1, 3 x 2, 8 x 9) against float64: every element within the bound of
    its addition chain, each product on the device's own t / u and end to end; guard zones intact, nothing left unwritten, a second
    call the same bits."""
    rows = _run(engine, f"images geom {geom}", R.shape_cases(geom))
    bad = P.failures(rows)
    assert not bad, P.format_rows(bad)


def test_lora_conv_kernels_every_channel_count(engine):
    """(Ci, Co) = (64, 64), (128, 64) (two contraction stages), (320, 320), (640, 320) on the 3 x 5 and 16 x 17 images."""
    rows = _run(engine, "channels", R.channel_cases())
    bad = P.failures(rows)
    assert not bad, P.format_rows(bad)


def test_lora_conv_kernels_every_rank(engine):
    """Rank 1, 4, 24, 128 (one, one, two and eight tiles of 16) on the 3 x 5 and 16 x 17 images, and on one image of each resampling
    geometry."""
    rows = _run(engine, "ranks", R.rank_cases())
    bad = P.failures(rows)
    assert not bad, P.format_rows(bad)


def test_lora_conv_kernels_exact_integers(engine):
    """Exact-integer inputs, a down whose nine taps all differ and are not symmetric: every output of all three geometries equals
    float64 bit for bit -- a lane map, a tap order or the OIHW write cannot hide in a tolerance."""
    rows = _run(engine, "exact integers (elements off)", R.exact_cases(), exact=True)
    assert all(err == 0.0 for _, _, err, _ in rows), [r for r in rows if r[2] != 0.0]


def test_lora_conv_limits_are_refused(engine):
    """rank 129, Ci 96, Co 32, an odd H under Downsample: each refused by a message that names it."""
    from gligen_amd._lib import GligenAmdError
    x = torch.zeros(2, 4, 4, 64)
    with pytest.raises(GligenAmdError, match="rank 129"):
        engine.op_lora_conv3(x, torch.zeros(129, 64, 3, 3), torch.zeros(64, 129))
    with pytest.raises(GligenAmdError, match="Ci = 96"):
        engine.op_lora_conv3(torch.zeros(2, 4, 4, 96), torch.zeros(4, 96, 3, 3), torch.zeros(64, 4))
    with pytest.raises(GligenAmdError, match="Co = 32"):
        engine.op_lora_conv3(x, torch.zeros(4, 64, 3, 3), torch.zeros(32, 4))
    with pytest.raises(GligenAmdError, match="even H and W .3 x 4"):
        engine.op_lora_conv3(torch.zeros(2, 3, 4, 64), torch.zeros(4, 64, 3, 3), torch.zeros(64, 4), geom=1)
    with pytest.raises(GligenAmdError, match="geom 3"):
        engine.op_lora_conv3(x, torch.zeros(4, 64, 3, 3), torch.zeros(64, 4), geom=3)


# ---- the training step with conv-family adapters: the small two-level UNet of test_lora_train_gpu.py (B = 2, 16 x 16 latent, text)
from test_lora_train_gpu import CFG, case      # noqa: E402  (the state_dict, the batch and the unadapted step: computed once, shared)

RANK, ALPHA, CONV_RANK, CONV_ALPHA = 4, 8.0, 8, 4.0        # scale 2 on the Linears, 0.5 on the 3 x 3 convs
RUNS = {"conv": ((), ("conv",)), "emb": ((), ("emb",)), "sample": ((), ("sample",)), "all": (("attn", "ff"), ("conv", "emb", "sample"))}
N_SITES = {"conv": 21, "emb": 8, "sample": 2, "all": 7 * 10 + 31}
_STEPS, _TWO = {}, {}


def spec_of(run):
    from gligen_amd import lora_train as lt
    families, conv_families = RUNS[run]
    return lt.LoraSpec(RANK, ALPHA, families, conv_families=conv_families, conv_rank=CONV_RANK, conv_alpha=CONV_ALPHA)


def adapters_for(engine, run, zero_up=False):
    """(spec, CPU tensors under init_adapters' keys, the engine's adapter list on the device)."""
    from gligen_amd import lora_train as lt
    c = case(engine)
    spec = spec_of(run)
    t = lt.init_adapters(c["sd_cpu"], CFG, spec, seed=3)
    if not zero_up:
        g = torch.Generator().manual_seed(17)
        t = {k: (torch.randn(v.shape, generator=g) * 0.03 if k.endswith(lt.UP) else v) for k, v in t.items()}
    dev = engine.device
    sites = lt.adapter_sites(c["sd_cpu"], spec)
    assert len(sites) == N_SITES[run]
    arr = [dict(name=w, down=t[w[:-7] + lt.DOWN].to(dev), up=t[w[:-7] + lt.UP].to(dev), scale=spec.of_site(c["sd_cpu"][w])[1] / spec.of_site(c["sd_cpu"][w])[0])
           for w in sites]
    return spec, t, arr


def merged(sd_cpu, tensors, arr):
    """sd_cpu with W + s (up @ down.reshape(r, -1)).reshape_as(W) (float64, rounded once) at every adapted weight."""
    from gligen_amd import lora_train as lt
    out = dict(sd_cpu)
    for a in arr:
        w, p = a["name"], a["name"][:-7]
        W, down, up = sd_cpu[w], tensors[p + lt.DOWN].double(), tensors[p + lt.UP].double()
        out[w] = (W.double() + a["scale"] * (up @ down.reshape(down.shape[0], -1)).reshape(W.shape)).float()
    return out


def chain_rule(dW, down, up, s):
    """(g_down, g_up) of an adapter from the gradient of the merged weight W + s (up @ down.reshape(r, -1)).reshape_as(W), float64."""
    dW2, d2 = dW.double().reshape(dW.shape[0], -1), down.double().reshape(down.shape[0], -1)
    return (s * (up.double().T @ dW2)).reshape(down.shape), s * (dW2 @ d2.T)


def adapted_step(engine, run):
    if run not in _STEPS:
        c = case(engine)
        spec, t, arr = adapters_for(engine, run)
        _STEPS[run] = (spec, t, arr, engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=arr))
    return _STEPS[run]


def _profile(name, line):
    out = os.environ.get("GLIGEN_LORA_CONV_REPORT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name), "a") as f:
            f.write(line + "\n")


def test_conv_zero_up_adds_exact_zeros(engine):
    """The small UNet holds every geometry: stride-1 convs at 16 x 16 (320 channels) and 8 x 8 (640), ResBlocks with Cin != Cout (a
    skip_connection; the output blocks' inputs are concatenations of 1280, 960 and 640 channels), one Downsample (320 channels,
    16 -> 8) and one Upsample (640 channels, 8 -> 16). With up = 0 on every adapter of conv + emb + sample + attn + ff (how training
    starts) loss, eps and every base gradient are torch.equal to the step without adapters, every g_down is exactly zero and every
    g_up is finite and not zero."""
    c = case(engine)
    loss0, eps0, grads0 = c["base"]
    _, _, arr = adapters_for(engine, "all", zero_up=True)
    loss, eps, grads, ag = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=arr)
    assert torch.equal(loss, loss0) and torch.equal(eps, eps0)
    assert sorted(grads) == sorted(grads0)
    assert all(torch.equal(grads[k], grads0[k]) for k in grads0), [k for k in grads0 if not torch.equal(grads[k], grads0[k])][:5]
    assert len(ag) == N_SITES["all"] and all(int(torch.count_nonzero(gd)) == 0 for gd, _ in ag.values())
    bad = [k for k, (_, gu) in ag.items() if not (bool(torch.isfinite(gu).all()) and int(torch.count_nonzero(gu)) > 0)]
    assert not bad, bad


@pytest.mark.parametrize("run", list(RUNS))
def test_conv_adapted_step_vs_oracle_autograd(engine, run):
    """Random up: loss, eps and every adapter gradient against autograd through the CPU oracle on
    W + s (up @ down.reshape(r, -1)).reshape_as(W) (the gradient of the merged weight, then the chain rule in float64), per family
    and all three with attn + ff; rel-MSE < 1e-5 per tensor, the bar of the training step everywhere else."""
    from gligen_amd import lora_train as lt
    from lora_train_ref import rel_mse
    from test_train_inpaint_cpu import oracle_autograd
    c = case(engine)
    spec, t, arr, (loss, eps, grads, ag) = adapted_step(engine, run)
    sites = [a["name"] for a in arr]
    loss_o, eps_o, dW = oracle_autograd(merged(c["sd_cpu"], t, arr), CFG, "text", sites, c["d"], c["batch"]["x"], None)
    assert not torch.equal(eps.cpu(), c["base"][1].cpu()), "the adapters change the output"
    loss_err = abs(float(loss) - float(loss_o)) / float(loss_o)
    report = {"eps": rel_mse(eps, eps_o)}
    for a in arr:
        w = a["name"]
        gd_o, gu_o = chain_rule(dW[w], t[w[:-7] + lt.DOWN], t[w[:-7] + lt.UP], a["scale"])
        assert ag[w][0].shape == gd_o.shape and ag[w][1].shape == gu_o.shape
        report[w + " g_down"], report[w + " g_up"] = rel_mse(ag[w][0], gd_o), rel_mse(ag[w][1], gu_o)
    worst = max(report, key=report.get)
    line = f"{run:7s} loss {float(loss):.9g} oracle {float(loss_o):.9g} rel err {loss_err:.3e}  eps rel-MSE {report['eps']:.3e}  worst {worst} {report[worst]:.3e}"
    print("[lora_conv step]", line)
    _profile("step_vs_oracle.txt", line)
    assert loss_err < 1e-5 and not {k: v for k, v in report.items() if not v < 1e-5}, (loss_err, {k: v for k, v in report.items() if not v < 1e-5})


def test_conv_checkpoint_cache_and_adapters_only_give_the_same_bits(engine):
    """checkpoint=True, the weight cache and a second run give the bits of the first; adapters alone (no base gradient asked for) give
    the same adapter gradients; what was refused before stays refused."""
    from gligen_amd._lib import GligenAmdError
    c = case(engine)
    spec, t, arr, (loss, eps, grads, ag) = adapted_step(engine, "all")
    same = lambda a, b: sorted(a) == sorted(b) and all(torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) for k in a)
    fresh = lambda: [dict(a) for a in arr]
    engine.train_weight_cache(True)
    for kw in (dict(checkpoint=True), dict(), dict(checkpoint=True, use_weight_cache=True)):
        loss_c, eps_c, grads_c, ag_c = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=fresh(), **kw)
        assert torch.equal(loss_c, loss) and torch.equal(eps_c, eps), kw
        assert all(torch.equal(grads_c[k], grads[k]) for k in grads) and same(ag_c, ag), kw
    loss_a, eps_a, grads_a, ag_a = engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=fresh(), trainable=[])
    assert not grads_a and torch.equal(loss_a, loss) and torch.equal(eps_a, eps) and same(ag_a, ag)
    engine.train_weight_cache(False)
    for name in ("input_blocks.0.0.weight", "out.2.weight", "time_embed.0.weight"):
        w = c["sd"][name]
        down = torch.zeros((4, w.shape[1], 3, 3) if w.dim() == 4 else (4, w.shape[1]), device=w.device)
        with pytest.raises(GligenAmdError, match="an adapter was given for"):
            engine.unet_train_step(CFG, c["sd"], c["batch"], adapters=[dict(name=name, down=down, up=torch.zeros(w.shape[0], 4, device=w.device), scale=1.0)])


def two_steps(engine):
    """LoraTrainStep (adapters alone, attn + ff + conv + emb + sample, world 1, lr 1e-3), two steps on the batch."""
    if not _TWO:
        from gligen_amd import lora_train as lt
        c = case(engine)
        spec = spec_of("all")
        ts = lt.LoraTrainStep(engine, CFG, c["sd_cpu"], spec, lr=1e-3, weight_decay=0.0, world=1, seed=3)
        start = {k: v.cpu() for k, v in ts.adapter_tensors().items()}
        losses = [float(ts.step(c["batch"])[0]) for _ in range(2)]
        torch.cuda.synchronize()
        _TWO.update(ts=ts, spec=spec, start=start, losses=losses, after={k: v.cpu() for k, v in ts.adapter_tensors().items()},
                    base_after={k: v.cpu() for k, v in ts.state_dict().items()}, milestones=dict(ts.milestone), adapters=[dict(name=a["name"], scale=a["scale"]) for a in ts.adapters])
        engine.train_weight_cache(False)
    return _TWO


def test_conv_two_lora_train_steps_vs_oracle_adamw(engine):
    """Two LoraTrainStep iterations from up = 0: the base model keeps its bits, the first loss is the base model's, every adapter
    tensor has moved after two steps, and both losses match oracle autograd on the merged weights + the chain rule +
    torch.optim.AdamW on the CPU under the existing two-step test's tolerance. The conv families' tensors sit at the last milestone."""
    from gligen_amd import lora_train as lt
    from test_train_inpaint_cpu import oracle_autograd
    c, r = case(engine), two_steps(engine)
    start, after, arr = r["start"], r["after"], r["adapters"]
    assert all(torch.equal(r["base_after"][k], v) for k, v in c["sd_cpu"].items())
    assert r["losses"][0] == float(c["base"][0])
    assert len(after) == 2 * N_SITES["all"] and all(not torch.equal(after[k], start[k]) for k in after)
    sites = [a["name"] for a in arr]
    params = {k: v.clone().requires_grad_(True) for k, v in start.items()}
    opt = torch.optim.AdamW(list(params.values()), lr=1e-3, weight_decay=0.0)
    ref_losses = []
    for _ in range(2):
        opt.zero_grad()
        cur = {k: v.detach() for k, v in params.items()}
        loss, _, dW = oracle_autograd(merged(c["sd_cpu"], cur, arr), CFG, "text", sites, c["d"], c["batch"]["x"], None)
        ref_losses.append(float(loss))
        for a in arr:
            w = a["name"]
            gd, gu = chain_rule(dW[w], cur[w[:-7] + lt.DOWN], cur[w[:-7] + lt.UP], a["scale"])
            params[w[:-7] + lt.DOWN].grad, params[w[:-7] + lt.UP].grad = gd.float(), gu.float()
        opt.step()
    print("conv LoRA train steps: losses", r["losses"], "oracle + AdamW", ref_losses)
    for a, ref in zip(r["losses"], ref_losses):
        assert abs(a - ref) / ref < 1e-4, (r["losses"], ref_losses)
    last = max(r["milestones"].values())
    assert last == 7 and all(m == last for k, m in r["milestones"].items() if ".transformer_blocks." not in k and ".proj_" not in k)


def test_conv_trained_adapter_round_trips_to_inference(engine, tmp_path):
    """The trained adapter saved in kohya's format (3 x 3 downs 4-D as they are, ups with a (1, 1) tail, .alpha per site), merged into
    the inference model by apply_loras unchanged: every adapted parameter is W + s up down within lora_ref's bound for the merge, eps
    of the inference path matches the oracle's forward on the merged weights at the small-UNet parity bar, and remove_loras restores
    every weight bit for bit."""
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
    assert len(report["adapters"][0]["unet"]) == N_SITES["all"] and not report["skipped"]
    got = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for a in r["adapters"]:
        w = a["name"]
        W, down, up = c["sd_cpu"][w], r["after"][w[:-7] + lt.DOWN], r["after"][w[:-7] + lt.UP]
        err = (got[w].double() - lora_ref.merge64(W, up, down, a["scale"])).abs()
        assert bool((err <= lora_ref.merge_bound(W, up, down, a["scale"])).all()), w
    d = c["d"]
    to = lambda m: {k: v.to(dev) for k, v in m.items()}
    gin = model.grounding_tokenizer_input.prepare(to(d["b"]))
    eps = model(dict(x=c["batch"]["x"].to(dev), timesteps=d["t"].to(dev), context=d["context"].to(dev), grounding_input=gin, inpainting_extra_input=None,
                     grounding_extra_input=None))
    eps_o = orc.unet_forward(merged(c["sd_cpu"], r["after"], r["adapters"]), oracle_cfg(CFG, "text"),
                             dict(x=c["batch"]["x"], timesteps=d["t"], context=d["context"], grounding_input=grounding_kwargs("text", d["b"]), inpainting_extra_input=None))
    err = mse(eps, eps_o)
    print("trained conv adapter merged into the inference path: eps MSE", err)
    lora.remove_loras(model)
    back = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    model._drop_engine()
    assert err < EPS_MSE_TOL, err
    assert all(torch.equal(back[k], v) for k, v in c["sd_cpu"].items()), [k for k, v in c["sd_cpu"].items() if not torch.equal(back[k], v)][:5]


def test_trainer_conv_lora_run_resumes_bit_for_bit(tmp_path):
    """python -m gligen_amd.trainer --synthetic text --small --latent 16 --lora_rank 4 --lora_conv_families conv emb sample
    --lora_conv_rank 4: three iterations in one go against two, a stop, and a resumed third: the adapter files are equal bit for bit;
    a resume with another --lora_conv_rank is refused."""
    from gligen_amd import lora, trainer
    common = ["--synthetic", "text", "--small", "--latent", "16", "--lora_rank", "4", "--lora_conv_families", "conv", "emb", "sample", "--batch_size", "2",
              "--warmup_steps", "0", "--base_learning_rate", "1e-3", "--arena_gb", "4", "--seed", "5"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert trainer.main(common + ["--lora_conv_rank", "4", "--total_iters", "3", "--output_dir", a]) == 0
    assert trainer.main(common + ["--lora_conv_rank", "4", "--total_iters", "2", "--output_dir", b]) == 0
    two = lora.read_safetensors(os.path.join(b, "lora.safetensors"))
    with pytest.raises(ValueError, match="lora_conv_rank"):
        trainer.main(common + ["--lora_conv_rank", "8", "--total_iters", "3", "--output_dir", b, "--resume"])
    assert trainer.main(common + ["--lora_conv_rank", "4", "--total_iters", "3", "--output_dir", b, "--resume"]) == 0
    one, resumed = lora.read_safetensors(os.path.join(a, "lora.safetensors")), lora.read_safetensors(os.path.join(b, "lora.safetensors"))
    n = 7 * 8 + 31
    assert sorted(one) == sorted(resumed) and len(one) == 3 * n
    assert all(torch.equal(one[k], resumed[k]) for k in one), [k for k in one if not torch.equal(one[k], resumed[k])][:5]
    assert any(not torch.equal(two[k], resumed[k]) for k in two), "the third iteration moved the adapter"
    ck = trainer.read_checkpoint(os.path.join(b, "checkpoint_latest.pth"))
    assert ck["iters"] == 3 and len(ck["lora"]) == 2 * n and ck["config_dict"]["lora_conv_families"] == ["conv", "emb", "sample"] and ck["config_dict"]["lora_conv_rank"] == 4
    entries = lora.parse_adapter(resumed)
    assert len(entries) == n and sum(e.down.dim() == 4 and tuple(e.down.shape[2:]) == (3, 3) for e in entries) == 18
