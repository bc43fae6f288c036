"""LoRA adapters on a real MI355X: gl_op_lora_merge by itself against float64 with a derived bound, apply_loras / remove_loras on the
small synthetic UNet and on a CLIP text tower (parameters against float64, outputs bit for bit against fresh modules that were handed
the merged weights), stacking, and the command line end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

import lora_ref as ref
from helpers import ROOT, build_product_unet, build_product_vae
from gligen_amd import lora
from gligen_amd import synthetic as syn

pytestmark = pytest.mark.gpu

FAMILIES = ("attn", "ff", "proj", "conv", "emb", "sample", "fuser")
REPORT = {}


@pytest.fixture(autouse=True)
def _report(record_property):
    before = set(REPORT)
    yield
    for key in sorted(set(REPORT) - before):
        record_property(key, json.dumps(REPORT[key], sort_keys=True))
        print(f"[lora] {key}: {json.dumps(REPORT[key], sort_keys=True)}")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _scratch(dev):
    from gligen_amd import runtime
    from gligen_amd.build import build_native
    build_native()
    return runtime.scratch_engine(dev)


def _check(got, W, up, down, scale, what):
    """got against the float64 merge within lora_ref.merge_bound, element by element; returns the worst error / bound."""
    want, bound = ref.merge64(W, up, down, scale), ref.merge_bound(W, up, down, scale)
    err = (got.detach().cpu().double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"[lora] {what}: worst error / bound = {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)
    return worst


# ---- the operator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w_mag", [1.0, 1e-3], ids=["w1", "w1e-3"])
@pytest.mark.parametrize("N,K,r", ref.OP_SHAPES, ids=[f"{n}x{k}r{r}" for n, k, r in ref.OP_SHAPES])
def test_merge_against_float64(N, K, r, w_mag):
    dev = _dev()
    eng = _scratch(dev)
    W, up, down = ref.op_case(N, K, r, w_mag, seed=N + 7 * K + 13 * r)
    if (N, K, r) == (320, 36, 4):          # a 3 x 3 conv from 4 channels: the same call with K = Cin kh kw
        W, up, down = W.reshape(320, 4, 3, 3), up.reshape(320, 4, 1, 1), down.reshape(4, 4, 3, 3)
    dW, dup, ddown = W.to(dev), up.to(dev), down.to(dev)
    worst = 0.0
    for scale in (0.75, -1.25):
        got = eng.op_lora_merge(dW.clone(), dup, ddown, scale)
        assert got.shape == W.shape
        worst = max(worst, _check(got, W, up, down, scale, f"{N}x{K} r{r} |W|~{w_mag:g} scale {scale}"))
        again = eng.op_lora_merge(dW.clone(), dup, ddown, scale)
        assert torch.equal(got, again), "two calls from the same start give the same bits"
        assert not torch.equal(got, dW)
    kept = eng.op_lora_merge(dW.clone(), dup, ddown, 0.0)
    assert torch.equal(kept.view(torch.int32), dW.view(torch.int32)), "scale == 0 leaves W bit for bit"
    assert torch.equal(dup, up.to(dev)) and torch.equal(ddown, down.to(dev))
    REPORT[f"merge_{N}x{K}r{r}_{w_mag:g}"] = dict(worst_err_over_bound=worst)


def test_merge_does_not_write_outside_w():
    """W in the middle of a larger buffer, odd sizes: the rows and columns beyond the tile edge are neither read into W nor written."""
    dev = _dev()
    eng = _scratch(dev)
    N, K, r = 37, 131, 5
    W, up, down = ref.op_case(N, K, r, 1.0, seed=3)
    buf = torch.full((N * K + 512,), 7.0, device=dev)
    view = buf[256:256 + N * K].view(N, K)
    view.copy_(W)
    eng.op_lora_merge(view, up.to(dev), down.to(dev), 0.5)
    _check(view, W, up, down, 0.5, "guarded")
    assert bool((buf[:256] == 7.0).all()) and bool((buf[256 + N * K:] == 7.0).all())


def test_merge_refusals():
    from gligen_amd._lib import GligenAmdError
    dev = _dev()
    eng = _scratch(dev)
    N, K, r = 8, 16, 4
    buf = torch.zeros(N * K + N * r + r * K, device=dev)
    W, up, down = buf[:N * K].view(N, K), buf[N * K:N * K + N * r].view(N, r), buf[N * K + N * r:].view(r, K)
    eng.op_lora_merge(W, up, down, 1.0)                                              # adjacent, not overlapping: fine
    with pytest.raises(GligenAmdError, match="lora_merge: W overlaps up"):
        eng.op_lora_merge(W, buf[N * K - 4:N * K - 4 + N * r].view(N, r), down, 1.0)
    with pytest.raises(GligenAmdError, match="lora_merge: W overlaps down"):
        eng.op_lora_merge(W, up, buf[4:4 + r * K].view(r, K), 1.0)
    with pytest.raises(GligenAmdError, match="lora_merge: W overlaps up"):
        eng.op_lora_merge(W, buf[:N * r].view(N, r), down, 0.0)                      # refused even when nothing would run
    p = lambda t: t.data_ptr()
    for sizes in ((0, K, r), (N, 0, r), (N, K, 0), (-1, K, r)):
        assert eng.lib.gl_op_lora_merge(eng._ctx, p(W), p(up), p(down), *sizes, 1.0, None) != 0
        assert b"lora_merge: N, K and r must be positive" in eng.lib.gl_last_error()
    assert eng.lib.gl_op_lora_merge(eng._ctx, None, p(up), p(down), N, K, r, 1.0, None) != 0 and b"null W" in eng.lib.gl_last_error()
    assert not buf.any()
    good = lambda: (torch.zeros(N, K, device=dev), torch.zeros(N, r, device=dev), torch.zeros(r, K, device=dev))
    for i, bad, what in ((0, lambda t: t.half(), "contiguous fp32"), (1, lambda t: t.double(), "contiguous fp32"), (2, lambda t: t.bfloat16(), "contiguous fp32"),
                         (0, lambda t: torch.zeros(K, N, device=dev).t(), "not contiguous"), (2, lambda t: torch.zeros(K, r, device=dev).t(), "not contiguous"),
                         (1, lambda t: t.cpu(), "on cpu"), (0, lambda t: t.reshape(-1), "at least two dimensions")):
        args = list(good())
        args[i] = bad(args[i])
        with pytest.raises(ValueError, match=what):
            eng.op_lora_merge(*args, 1.0)
    with pytest.raises(ValueError, match="does not give W"):
        eng.op_lora_merge(torch.zeros(N, K, device=dev), torch.zeros(N, r + 1, device=dev), torch.zeros(r, K, device=dev), 1.0)


# ---- the UNet ----------------------------------------------------------------------------------------------------------------------
def _inputs(model, dev, B=2, hw=16):
    batch = {k: v.to(dev) for k, v in syn.make_batch("text", B, n_valid=3, seed=0).items()}
    return dict(x=syn.make_latent(B, 4, hw, hw, seed=1).to(dev), timesteps=torch.tensor([981, 441][:B], device=dev),
                context=syn.make_context(B, seed=1).to(dev), grounding_input=model.grounding_tokenizer_input.prepare(batch),
                inpainting_extra_input=None, grounding_extra_input=None)


def _unet(dev):
    return build_product_unet(syn.UNET_CFG_SMALL, "text", device=dev)


def _fresh_with(state, dev):
    m = _unet(dev)
    m.load_state_dict(state)
    return m


@pytest.fixture(scope="module")
def unet_case():
    """One small UNet, two synthetic adapters, and what apply / remove leave behind: computed once, read by the tests below."""
    dev = _dev()
    _scratch(dev)
    model = _unet(dev)
    inp = _inputs(model, dev)
    A = syn.synthetic_lora(model, rank=4, families=FAMILIES, dtype=torch.float16, seed=7)
    Bd = syn.synthetic_lora(model, rank=3, families=("attn", "conv"), dtype=torch.float32, seed=8, alpha=3.0)
    original = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    e_before = model(inp).clone()
    engine_before = model.__dict__["_engine"]
    report = lora.apply_loras(model, None, [(A, 0.8)])
    applied = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    engine_gone = model.__dict__["_engine"] is None and engine_before._ctx.value is None
    e_after = model(inp).clone()
    fresh = _fresh_with(applied, dev)
    e_fresh = fresh(inp).clone()
    # [A] then [A, B] on the same model against [A, B] on a model that never carried an adapter
    lora.apply_loras(model, None, [(A, 0.8), (Bd, -0.5)])
    stacked = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    e_stacked = model(inp).clone()
    fresh.load_state_dict(original)
    lora.apply_loras(fresh, None, [(A, 0.8), (Bd, -0.5)])
    stacked_fresh = {k: v.detach().cpu().clone() for k, v in fresh.state_dict().items()}
    e_stacked_fresh = fresh(inp).clone()
    fresh._drop_engine()
    # scale 0
    lora.apply_loras(model, None, [(A, 0.0)])
    zeroed = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    e_zero = model(inp).clone()
    lora.apply_loras(model, None, [(A, 0.8)])
    n_removed = lora.remove_loras(model, None)
    removed = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    stash_gone = lora.STASH not in model.__dict__
    e_removed = model(inp).clone()
    model._drop_engine()
    return dict(A=A, B=Bd, report=report, original=original, applied=applied, stacked=stacked, stacked_fresh=stacked_fresh, zeroed=zeroed, removed=removed,
                e_before=e_before, e_after=e_after, e_fresh=e_fresh, e_stacked=e_stacked, e_stacked_fresh=e_stacked_fresh, e_zero=e_zero,
                e_removed=e_removed, engine_gone=engine_gone, n_removed=n_removed, stash_gone=stash_gone)


def _touched(adapter):
    """{parameter key: (up, down, alpha / r)} of a synthetic adapter on the small UNet. The name table is judged against lora_ref's
    diffusers walk on the host (test_lora_cpu.py); here the shapes of the diffusers names are checked once more."""
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    with torch.device("meta"):
        model = UNetModel(**dict(syn.UNET_CFG_SMALL, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"]))
    shapes = {k[:-len(".weight")]: tuple(v.shape) for k, v in model.state_dict().items() if k.endswith(".weight")}
    diffusers = ref.diffusers_unet_targets(**ref.SMALL)
    table = lora.unet_name_table(model)
    out = {}
    for name in sorted({k.split(".", 1)[0] for k in adapter}):
        path = table[name]
        if name in diffusers:
            assert shapes[path] == tuple(diffusers[name]), name
        else:
            assert ".fuser." in path and name == "lora_unet_" + path.replace(".", "_"), name
        alpha = adapter.get(name + ".alpha")
        down, up = adapter[name + ".lora_down.weight"], adapter[name + ".lora_up.weight"]
        out[path + ".weight"] = (up, down, 1.0 if alpha is None else float(alpha) / down.shape[0])
    return out


def test_apply_merges_the_touched_parameters_and_no_other(unet_case):
    c = unet_case
    touched = _touched(c["A"])
    assert len(touched) > 100 and any(".fuser." in k for k in touched) and any(k.endswith(".op.weight") for k in touched)
    assert any(".emb_layers.1." in k for k in touched) and any(".proj_in." in k for k in touched) and any(".in_layers.2." in k for k in touched)
    assert sorted(k[:-len(".weight")] for k in touched) == sorted(c["report"]["adapters"][0]["unet"])
    assert c["report"]["adapters"][0]["text_encoder"] == [] and c["report"]["skipped"] == [] and c["report"]["seconds"] > 0
    worst = 0.0
    for key, w0 in c["original"].items():
        if key in touched:
            up, down, factor = touched[key]
            worst = max(worst, _check(c["applied"][key], w0, up.float(), down.float(), 0.8 * factor, key))
            assert not torch.equal(c["applied"][key], w0)
        else:
            assert torch.equal(c["applied"][key], w0), key
    REPORT["unet_apply"] = dict(worst_err_over_bound=worst, tensors=len(touched))


def test_forward_follows_the_merged_parameters(unet_case):
    c = unet_case
    assert c["engine_gone"], "apply_loras dropped (and closed) the engine built before it"
    assert torch.isfinite(c["e_after"]).all() and not torch.equal(c["e_after"], c["e_before"]), "the stale engine is gone"
    assert torch.equal(c["e_after"], c["e_fresh"]), "the forward after apply_loras is that of a fresh model given the merged state dict"
    rel = float(((c["e_after"] - c["e_before"]).double() ** 2).mean() / (c["e_before"].double() ** 2).mean())
    REPORT["unet_forward"] = dict(rel_change=rel)
    assert rel > 1e-4, "an adapter of this size moves the output visibly"


def test_remove_restores_bit_for_bit(unet_case):
    c = unet_case
    assert c["n_removed"] == len(_touched(c["A"])) and c["stash_gone"]
    assert all(torch.equal(c["removed"][k], v) for k, v in c["original"].items())
    assert torch.equal(c["e_removed"], c["e_before"])


def test_stacking_starts_from_the_originals(unet_case):
    c = unet_case
    assert all(torch.equal(c["stacked"][k], v) for k, v in c["stacked_fresh"].items()), "[A] then [A, B] equals [A, B] on a fresh model"
    assert torch.equal(c["e_stacked"], c["e_stacked_fresh"])
    ta, tb = _touched(c["A"]), _touched(c["B"])
    assert set(tb) & set(ta) and not torch.equal(c["e_stacked"], c["e_after"])
    both = sorted(set(tb) & set(ta))
    for key in both[:8] + both[-8:]:       # the second merge starts from the first one's fp32 result (which the test above judges)
        _check(c["stacked"][key], c["applied"][key], tb[key][0], tb[key][1], -0.5 * tb[key][2], "stacked " + key)


def test_scale_zero_changes_nothing(unet_case):
    c = unet_case
    assert all(torch.equal(c["zeroed"][k].view(torch.int32), v.view(torch.int32)) for k, v in c["original"].items() if v.dtype == torch.float32)
    assert torch.equal(c["e_zero"], c["e_before"])


def test_apply_after_lanes_and_hires_contexts(monkeypatch):
    """With execution lanes and a second-pass fork alive, apply_loras leaves none of them behind and generate() runs on the merged
    weights: the images of a fresh model that was handed those weights."""
    dev = _dev()
    import gligen_inference as gi
    monkeypatch.setattr(gi, "device", dev)
    B, hw, S = 4, 16, 4
    model = _unet(dev)
    ae = build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    diffusion = gi.instantiate_from_config(gi.synthetic_config("text", image_size=hw)["diffusion"]).to(dev)
    batch = {k: v.to(dev) for k, v in syn.make_batch("text", B, n_valid=3, seed=0).items()}
    ctx, uc = syn.make_context(B, seed=1).to(dev), syn.make_context(B, seed=9).to(dev)
    x_T = syn.make_latent(B, 4, hw, hw, seed=6).to(dev)
    kw = dict(steps=S, guidance_scale=5.0, sampler="dpmpp_2m", height=2 * hw, width=2 * hw)      # (the small VAE has factor 2)
    gi.generate_lanes(model, ae, diffusion, batch, ctx, uc, lanes=2, starting_noise=x_T.clone(), **kw)
    gi.generate(model, ae, diffusion, batch, ctx, uc, starting_noise=x_T.clone(), hires=(32, 48), hires_steps=4, hires_strength=0.5, **kw)
    lanes, forks = model.__dict__["_lanes"], model.__dict__["_hires"]
    assert len(lanes) == 1 and len(forks) == 1
    held = [lanes[0][0], lanes[0][1]] + [m for m, _ in forks.values()]
    before = gi.generate(model, ae, diffusion, batch, ctx, uc, starting_noise=x_T.clone(), **kw).clone()
    A = syn.synthetic_lora(model, rank=4, families=("attn", "ff", "conv"), dtype=torch.float16, seed=7)
    lora.apply_loras(model, None, [(A, 0.8)])
    assert "_lanes" not in model.__dict__ and "_hires" not in model.__dict__ and model.__dict__["_engine"] is None
    assert all(m.__dict__["_engine"] is None for m in held), "every context that shared the old packed weights is closed"
    after = gi.generate(model, ae, diffusion, batch, ctx, uc, starting_noise=x_T.clone(), **kw).clone()
    split = gi.generate_lanes(model, ae, diffusion, batch, ctx, uc, lanes=2, starting_noise=x_T.clone(), **kw).clone()      # new lanes, new weights
    fresh = _fresh_with(model.state_dict(), dev)
    want = gi.generate(fresh, ae, diffusion, batch, ctx, uc, starting_noise=x_T.clone(), **kw)
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    assert torch.equal(after, want)
    assert float(((split - after).double() ** 2).mean() / after.double().var()) < 2e-3       # (the bar of the lanes tests: another tile choice per sub-batch)
    for m in (model, fresh, ae):
        m._drop_engine()


# ---- the text tower ------------------------------------------------------------------------------------------------------------------
def _embedder(dev, backend):
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_clip as mgc

    class Embedder(FrozenCLIPEmbedder):
        def __init__(self):
            nn.Module.__init__(self)
            c = mgc.CASES["small"]
            self.tokenizer, self.transformer, self.device, self.max_length = None, mgc.build_tower(c["layers"], c["intermediate"]), str(dev), 77
            self.backend, self._engine = backend, None
            self.freeze()

    return Embedder().to(dev), mgc.make_ids(mgc.CASES["small"]["lengths"])


@pytest.mark.parametrize("backend", ["hip", "hf"])
def test_text_tower(backend):
    dev = _dev()
    _scratch(dev)
    enc, ids = _embedder(dev, backend)
    model = _unet(dev)
    adapter = syn.synthetic_lora(model, enc, rank=4, families=("te", "attn"), dtype=torch.float16, seed=11, limit=24)
    te_names = sorted({k.split(".", 1)[0] for k in adapter if k.startswith("lora_te_")})
    assert len(te_names) == 12 and te_names == sorted(ref.clip_text_targets(2, 768, 256))
    original = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    h_before = enc.encode_ids(ids).clone()
    with pytest.raises(lora.LoraError, match="no text encoder was given"):
        lora.apply_loras(model, None, [(adapter, 1.0)])
    report = lora.apply_loras(model, enc, [(adapter, 1.0, 0.6)])
    assert len(report["adapters"][0]["text_encoder"]) == 12 and len(report["adapters"][0]["unet"]) == 24
    applied = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    linears = {"self_attn_q_proj": "self_attn.q_proj", "self_attn_k_proj": "self_attn.k_proj", "self_attn_v_proj": "self_attn.v_proj",
               "self_attn_out_proj": "self_attn.out_proj", "mlp_fc1": "mlp.fc1", "mlp_fc2": "mlp.fc2"}
    table = {f"lora_te_text_model_encoder_layers_{n}_{short}": next(k for k in original if k.endswith(f"encoder.layers.{n}.{path}.weight"))
             for n in range(2) for short, path in linears.items()}
    touched = set(table.values())
    assert sorted(table) == te_names
    assert len(touched) == 12
    for name, key in table.items():
        up, down, alpha = adapter[name + ".lora_up.weight"], adapter[name + ".lora_down.weight"], float(adapter[name + ".alpha"])
        _check(applied[key], original[key], up.float(), down.float(), 0.6 * alpha / 4, key)
    assert all(torch.equal(applied[k], v) for k, v in original.items() if k not in touched)
    h_after = enc.encode_ids(ids).clone()
    assert torch.isfinite(h_after).all() and not torch.equal(h_after, h_before)
    fresh, _ = _embedder(dev, backend)
    fresh.load_state_dict(enc.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), enc.state_dict().values()))
    if backend == "hip":
        assert enc.__dict__["_engine"] is not None, "the native engine was rebuilt from the merged parameters"
        assert torch.equal(fresh.encode_ids(ids), h_after), "the encoder after apply_loras is a fresh one loaded with the merged state dict"
    assert lora.remove_loras(model, enc) == 12 + 24
    assert all(torch.equal(v.cpu(), original[k]) for k, v in enc.state_dict().items())
    if backend == "hip":
        assert torch.equal(enc.encode_ids(ids), h_before)
    for m in (enc, fresh, model):
        m._drop_engine()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_command_line_end_to_end(tmp_path, monkeypatch, capsys):
    dev = _dev()
    import gligen_inference as gi
    from PIL import Image
    monkeypatch.setattr(gi, "device", dev)
    hw = 16

    def small_synthetic(kind="text", inpaint=False, **kw):       # the smallest synthetic size: the 2-level UNet and VAE of the goldens
        cfg = gi.synthetic_config(kind, inpaint, image_size=hw)
        cfg["model"]["params"].update(syn.UNET_CFG_SMALL, image_size=hw, grounding_tokenizer=syn.GROUNDING_TOKENIZERS[kind])
        cfg["autoencoder"]["params"]["ddconfig"] = syn.VAE_DDCONFIG_SMALL
        model = syn.fill_module_(gi.instantiate_from_config(cfg["model"]).eval(), 1234).to(dev)
        ae = syn.fill_module_(gi.instantiate_from_config(cfg["autoencoder"]).eval(), 4321).to(dev)
        return model, ae, gi.instantiate_from_config(cfg["diffusion"]).to(dev), cfg

    monkeypatch.setattr(gi, "load_synthetic", small_synthetic)
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    with torch.device("meta"):
        shape_model = UNetModel(**dict(syn.UNET_CFG_SMALL, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"]))
    path = tmp_path / "a.safetensors"
    lora.write_safetensors(path, syn.synthetic_lora(shape_model, rank=4, families=("attn", "ff", "first_conv"), dtype=torch.float16, seed=7))
    common = ["--synthetic", "text", "--batch_size", "2", "--steps", "4", "--sampler", "dpmpp_2m", "--seed", "1"]
    gi.main(common + ["--folder", str(tmp_path / "plain")])
    gi.main(common + ["--folder", str(tmp_path / "out"), "--lora", f"{path}:0.8"])
    text = capsys.readouterr().out
    assert "LoRA" in text and "70 UNet and 0 text-encoder modules (scale 0.8 / 0.8)" in text and "skipped lora_unet_conv_in" in text
    files = sorted(os.listdir(tmp_path / "out" / "synthetic_text"))
    assert files == ["0.png", "1.png"]
    a = torch.from_numpy(np.asarray(Image.open(tmp_path / "out" / "synthetic_text" / "0.png")).copy())
    b = torch.from_numpy(np.asarray(Image.open(tmp_path / "plain" / "synthetic_text" / "0.png")).copy())
    assert a.shape == b.shape == (32, 32, 3) and not torch.equal(a, b), "the adapter reached the images"
    # a name that resolves to nothing: the refusal's text, and no image
    bad = dict(lora.read_safetensors(path))
    bad.update({"lora_unet_down_blocks_9_attentions_0_proj_in." + k.split(".", 1)[1]: v for k, v in bad.items()
                if k.startswith("lora_unet_mid_block_attentions_0_transformer_blocks_0_attn1_to_q.")})
    lora.write_safetensors(tmp_path / "bad.safetensors", bad)
    with pytest.raises(SystemExit, match=r"--lora refused: .*resolve to nothing in this model: \['lora_unet_down_blocks_9_attentions_0_proj_in'\]"):
        gi.main(common + ["--folder", str(tmp_path / "bad"), "--lora", str(tmp_path / "bad.safetensors")])
    assert not os.path.exists(tmp_path / "bad")
