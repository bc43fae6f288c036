"""The native CLIP vision tower (Engine::clip_vision_encode, get_clip_feature(..., vision=engine), run() with native_clip on
image-grounded phrases) on the MI355X against the goldens of tools/make_golden_clip_vision.py: transformers'
CLIPVisionModelWithProjection in fp32 on the CPU. Tower and feature bars are 5 x the golden's own autocast yardstick (torch's bf16
error on the same model), read from the file; the operator bar is derived in test_attention_operator."""
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
_spec = importlib.util.spec_from_file_location("make_golden_clip_vision", os.path.join(ROOT, "tools", "make_golden_clip_vision.py"))
mgv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgv)

REPORT = {}
CAP = int(re.search(r"kClipLongMaxTokens\s*=\s*(\d+)", open(os.path.join(ROOT, "gligen_amd", "csrc", "clip.h")).read()).group(1))
SHORT = int(re.search(r"kClipMaxTokens\s*=\s*(\d+)", open(os.path.join(ROOT, "gligen_amd", "csrc", "clip.h")).read()).group(1))
E2E_IMG_TOL = 8.5e-4    # the project's end-to-end image budget (tests/test_configs_gpu.py, tests/test_clip_gpu.py)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float(((a - b) ** 2).mean() / (b ** 2).mean())


@pytest.fixture(scope="module")
def report():
    """The measured values: printed by each test, and kept as parity_report_clip_vision.json in $GL_PARITY_REPORT_DIR when set."""
    yield REPORT
    out = os.environ.get("GL_PARITY_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_report_clip_vision.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


# ---------------------------------------------------------------------------------------------------------------- operator
_QKV = {}


def _qkv(heads):
    """One seeded bf16 buffer [3][CAP][3 * heads * 64] per head count: every (S, T) case reads its first S sequences / T tokens, so
    the T = 96 run of the existing kernel and the runs of the new kernel see the same q, k, v rows."""
    if heads not in _QKV:
        g = torch.Generator().manual_seed(100 + heads)
        _QKV[heads] = torch.randn((3, CAP, 3 * heads * 64), generator=g).to(torch.bfloat16)
    return _QKV[heads]


def _attention_f64(qkv, heads, causal):
    """softmax(q k^T / 8 (+ causal mask)) v in float64 on the bf16 values: [S][T][heads * 64]; also max |v| per (sequence, head)."""
    S, T, _ = qkv.shape
    q, k, v = (x.double().reshape(S, T, heads, 64).permute(0, 2, 1, 3) for x in qkv.split(heads * 64, dim=-1))
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    o = torch.softmax(s, dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(S, T, heads * 64), v.abs().amax(dim=(-1, -2))


# The absolute bar. The kernels compute o = sum_j p^_j v_j / sum_j p_j with p^_j = bf16(p_j), the denominator summed in fp32 from the
# unrounded p_j, and store bf16(o). With u = 2^-9 (the unit roundoff of bf16, 8 significand bits, round to nearest):
#   |sum_j p^_j v_j / sum p - o| <= u sum_j p_j |v_j| / sum p <= u max_j |v_j|      (a convex combination of |v_j|, each weight off by <= u)
#   the final rounding adds <= u |o| <= u max_j |v_j|
# so |out - o| <= 2 u max|v|. The fp32 parts (64-term dot products, the exp2 unit, the running sum, one rescaling of the state per
# key tile in the online form: relative 2^-24 each, <= 9 tiles) perturb p_j by < 2^-15 relative: an allowance of u / 4 covers them
# with a margin of two orders of magnitude.
U_BF16 = 2.0 ** -9
ABS_BAR = (2 + 0.25) * U_BF16
# The relative bar of the new kernel: at most 1.5 x the relative MSE the EXISTING kernel shows at T = 96 on the same q, k, v rows
# (online rescaling adds at most one extra fp32 rounding per key tile; nine tiles must not add up to a different error class).
LONG_VS_SHORT = 1.5

OP_T = sorted({1, 31, 32, 33, 50, 96, 97, 128, 197, 256, 257, CAP})
OP_CASES = [(T, S, H, False) for T in OP_T for S in (1, 3) for H in (2, 16)] + [(T, S, H, True) for T in OP_T if T <= SHORT for S in (1, 3) for H in (2, 16)]


def _run_op(eng, dev, T, S, H, causal):
    qkv = _qkv(H)[:S, :T].contiguous()
    ref, vmax = _attention_f64(qkv, H, causal)
    out = torch.full((S * T + 5, H * 64), 777.0, dtype=torch.bfloat16, device=dev)        # five rows of padding behind the real ones
    eng.op_clip_attention(qkv.reshape(S * T, -1).to(dev), S, T, H, causal, out=out)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[S * T:] == 777.0).all()), "rows >= S * T of out were written"
    got = out[:S * T].double().reshape(S, T, H * 64)
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs().reshape(S, T, H, 64).amax(dim=(1, 3)) / vmax       # per (sequence, head), in units of max |v|
    return dict(rel_mse=_rel(got, ref), max_abs_over_vmax=float(err.max())), got


@pytest.fixture(scope="module")
def op_engine():
    from gligen_amd.runtime import scratch_engine
    return scratch_engine(_dev())


@pytest.fixture(scope="module")
def short_yardstick(op_engine):
    """Relative MSE of clip_attn_kernel (the existing one) at T = 96 on the shared rows, per (S, heads)."""
    dev = _dev()
    return {(S, H): _run_op(op_engine, dev, SHORT, S, H, False)[0]["rel_mse"] for S in (1, 3) for H in (2, 16)}


@pytest.mark.parametrize("T,S,H,causal", OP_CASES)
def test_attention_operator(T, S, H, causal, op_engine, short_yardstick, report):
    dev = _dev()
    rec, _ = _run_op(op_engine, dev, T, S, H, causal)
    rec.update(abs_bar=ABS_BAR, kernel="clip_attn_long_kernel" if T > SHORT else "clip_attn_kernel")
    if T > SHORT:
        rec.update(short_rel_mse_at_96=short_yardstick[(S, H)], rel_bar=LONG_VS_SHORT * short_yardstick[(S, H)])
    report[f"op_T{T}_S{S}_H{H}_{'causal' if causal else 'full'}"] = rec
    print(json.dumps(rec))
    assert rec["max_abs_over_vmax"] <= ABS_BAR, rec
    if T > SHORT:
        assert rec["rel_mse"] <= rec["rel_bar"], rec


@pytest.mark.parametrize("T", [t for t in OP_T if t not in (1, CAP)])
def test_attention_does_not_read_behind_the_last_key(T, op_engine):
    """A padded qkv buffer: other contents (huge values, NaN bit patterns) behind key T - 1 change no output bit."""
    dev = _dev()
    H, rows = 2, CAP + 32
    qkv = torch.zeros((rows, 3 * H * 64), dtype=torch.bfloat16)
    qkv[:T] = _qkv(H)[0, :T]
    a = op_engine.op_clip_attention(qkv.to(dev), 1, T, H, False).cpu()
    qkv[T:] = 3.0e38
    qkv[T + 1::2] = float("nan")
    b = op_engine.op_clip_attention(qkv.to(dev), 1, T, H, False).cpu()
    assert bool(torch.isfinite(a.float()).all()) and torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_attention_refuses_what_it_does_not_hold_by_name(op_engine):
    from gligen_amd import GligenAmdError
    dev = _dev()
    qkv = torch.zeros(((CAP + 1), 3 * 2 * 64), dtype=torch.bfloat16, device=dev)
    with pytest.raises(GligenAmdError, match=f"T={CAP + 1}"):
        op_engine.op_clip_attention(qkv, 1, CAP + 1, 2, False)
    with pytest.raises(GligenAmdError, match=f"causal.*T={SHORT + 1}"):
        op_engine.op_clip_attention(qkv, 1, SHORT + 1, 2, True)
    op_engine.op_clip_attention(qkv, 1, SHORT, 2, True)       # the text tower's route is open


# ---------------------------------------------------------------------------------------------------------------- tower
def _engine(name, dev):
    from gligen_amd.runtime import build_clip_vision_engine
    return build_clip_vision_engine(mgv.build_tower(mgv.CASES[name]).to(dev))


@pytest.mark.parametrize("name", ["small", "small50", "full"])
def test_tower_parity_with_hf_fp32(name, report):
    """last_hidden (the stored rows for `full`), pooled and image_embeds, overall and for EACH image separately, within 5 x the overall
    autocast yardstick of the golden; the final feature too. One image alone gives the bits it has in the batch; so does a second call."""
    dev = _dev()
    g = mgv.load_case(name)
    c = mgv.CASES[name]
    n = c["images"]
    eng = _engine(name, dev)
    pixels = mgv.make_pixels(c)
    l0 = eng.launch_count()
    hidden, pooled, embeds = eng.clip_vision_encode(pixels)
    launches = eng.launch_count() - l0
    tokens = (c["image_size"] // c["patch"]) ** 2 + 1
    assert hidden.shape == (n, tokens, c["width"]) and pooled.shape == (n, c["width"]) and embeds.shape == (n, mgv.PROJECTION)
    assert torch.isfinite(hidden).all() and torch.isfinite(pooled).all() and torch.isfinite(embeds).all()
    h = hidden[:, torch.as_tensor(g["rows"])] if "rows" in g else hidden
    feature = mgv.final_feature(embeds.cpu(), mgv.projection_matrix())
    got = dict(hidden=h, pooled=pooled, embeds=embeds, feature=feature)
    want = dict(hidden=g["last_hidden"], pooled=g["pooled"], embeds=g["image_embeds"], feature=g["feature"])
    rec = dict(launches=launches, images=n, tokens=tokens)
    for k in got:
        rec["bar_" + k] = 5 * float(g["autocast_rel_mse_" + k])
        rec[k] = _rel(got[k], want[k])
        rec[k + "_per_image"] = [_rel(got[k][i], want[k][i]) for i in range(n)]
        rec["autocast_" + k + "_per_image"] = g["autocast_rel_mse_" + k + "_per_image"].tolist()
    report["parity_" + name] = rec
    print(json.dumps(rec))
    for k in got:
        assert rec[k] <= rec["bar_" + k] and max(rec[k + "_per_image"]) <= rec["bar_" + k], (k, rec)
    # ---- rows are independent: image 0 alone, and a second call
    h1, p1, e1 = eng.clip_vision_encode(pixels[:1])
    assert torch.equal(h1[0], hidden[0]) and torch.equal(p1[0], pooled[0]) and torch.equal(e1[0], embeds[0])
    h2, p2, e2 = eng.clip_vision_encode(pixels)
    assert torch.equal(h2, hidden) and torch.equal(p2, pooled) and torch.equal(e2, embeds)
    eng.close()


def test_one_image_equals_row_0_of_four():
    """S = 1 against row 0 of S = 4, bit for bit, on the 257-token `small` tower (the golden has three images: a fourth is drawn)."""
    dev = _dev()
    c = mgv.CASES["small"]
    eng = _engine("small", dev)
    px = torch.cat([mgv.make_pixels(c), 1.2 * torch.randn((1, 3, 224, 224), generator=torch.Generator().manual_seed(3))])
    assert px.shape[0] == 4
    four, one = eng.clip_vision_encode(px), eng.clip_vision_encode(px[:1])
    for a, b in zip(one, four):
        assert torch.equal(a[0], b[0])
    assert not torch.equal(four[2][0], four[2][3])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- feature
def _native_clip_model(tmp_path):
    """A fabricated CLIPModel whose vision side the native path supports (hidden 128 / 2 heads of 64 / patch 32 / quick_gelu); the
    text side, the tokenizer and the processor are helpers._fabricated_clip's."""
    import transformers
    from helpers import _fabricated_clip
    model, processor, tok = _fabricated_clip(tmp_path)
    vcfg = transformers.CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=224,
                                         patch_size=32, projection_dim=768, hidden_act="quick_gelu")
    torch.manual_seed(1)
    native = transformers.CLIPModel(transformers.CLIPConfig(text_config=model.config.text_config.to_dict(), vision_config=vcfg.to_dict(),
                                                            projection_dim=768)).eval()
    return model, native, processor, tok


def _pngs(tmp_path, n):
    from PIL import Image
    paths = []
    for i in range(n):
        rs = np.random.RandomState(20 + i)
        base = rs.rand(6, 5, 3)                                   # a coarse pattern, upsampled: images that differ at every scale
        img = np.kron(base, np.ones((50, 48, 1))) * 0.8 + 0.2 * rs.rand(300, 240, 3)
        Image.fromarray((img * 255).astype(np.uint8)).save(tmp_path / f"ref{i}.png")
        paths.append(str(tmp_path / f"ref{i}.png"))
    return paths


def test_get_clip_feature_with_the_native_tower(tmp_path, monkeypatch, report):
    """get_clip_feature(..., is_image=True, vision=engine) on PNG files against the same function on the HF model in fp32 on the CPU.
    The bar is 5 x this model's own autocast yardstick: the relative MSE of the same function under torch.autocast("cpu", bfloat16)."""
    dev = _dev()
    import gligen_inference as gi
    from gligen_amd import GligenAmdError
    from gligen_amd.runtime import build_clip_vision_engine
    d16, native, processor, _ = _native_clip_model(tmp_path)
    monkeypatch.chdir(tmp_path)
    torch.save(mgv.projection_matrix(), tmp_path / "projection_matrix")
    paths = _pngs(tmp_path, 3)
    with pytest.raises(GligenAmdError, match="head dim 16"):       # helpers._fabricated_clip's vision tower stays refused by name
        build_clip_vision_engine(d16.to(dev))
    monkeypatch.setattr(gi, "device", "cpu")
    want = [gi.get_clip_feature(native, processor, p, is_image=True) for p in paths]
    with torch.autocast("cpu", torch.bfloat16):
        cast = [gi.get_clip_feature(native, processor, p, is_image=True).float() for p in paths]
    bar = 5 * _rel(torch.cat(cast), torch.cat(want))
    eng = build_clip_vision_engine(native.to(dev))
    monkeypatch.setattr(gi, "device", dev)
    native.forward = None                                          # the HF model is not called on this side
    got = [gi.get_clip_feature(native, processor, p, is_image=True, vision=eng) for p in paths]
    batched = gi.get_clip_image_features(native, processor, [paths[0], None, paths[1], paths[2]], eng)
    rec = dict(bar=bar, rel=[_rel(a, b) for a, b in zip(got, want)], norms=[float(a.norm()) for a in got],
               smallest_pairwise=min(_rel(want[i], want[j]) for i in range(3) for j in range(3) if i != j))
    report["get_clip_feature_native"] = rec
    print(json.dumps(rec))
    assert rec["smallest_pairwise"] >= 100 * bar, rec              # the files are distinct enough for the bar to test the pixels
    for a, b in zip(got, want):
        assert a.shape == b.shape == (1, 768) and a.device.type == "cuda" and abs(float(a.norm()) - 28.7) < 1e-3
    assert max(rec["rel"]) <= bar, rec
    assert batched[1] is None and all(torch.equal(batched[i], got[j]) for i, j in ((0, 0), (2, 1), (3, 2)))
    eng.close()


def test_other_towers_are_refused_by_name():
    dev = _dev()
    import transformers
    from gligen_amd import GligenAmdError
    from gligen_amd.runtime import build_clip_vision_engine

    def tower(**kw):
        base = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, image_size=224, patch_size=32, projection_dim=64,
                    hidden_act="quick_gelu")
        base.update(kw)
        return transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**base)).eval().to(dev)

    with pytest.raises(GligenAmdError, match="head dim 32"):
        build_clip_vision_engine(tower(num_attention_heads=4))
    with pytest.raises(GligenAmdError, match="image_size 230 is not a multiple of the patch size 32"):
        build_clip_vision_engine(tower(image_size=230))
    with pytest.raises(NotImplementedError, match="hidden_act='gelu'"):
        build_clip_vision_engine(tower(hidden_act="gelu"))
    with pytest.raises(GligenAmdError, match="577 tokens"):
        build_clip_vision_engine(tower(image_size=336, patch_size=14))
    with pytest.raises(GligenAmdError, match="intermediate size 200"):
        build_clip_vision_engine(tower(intermediate_size=200))


# ---------------------------------------------------------------------------------------------------------------- file to image
def test_file_to_image_with_image_grounded_phrases_without_hf_vision_compute(tmp_path, monkeypatch, report):
    """run(meta, args) with native_clip from a checkpoint FILE (the construction of test_file_to_image_without_torch_clip_compute) with
    the text_image tokenizer and a meta carrying `images`: one box with an image only, one with a phrase and an image. CLIPModel
    supplies weights and the processor; its vision forward (and its own) raise if they run. The images are compared with generate()
    fed the HF module's fp32 CPU features from the same weights."""
    dev = _dev()
    import transformers
    import gligen_inference as gi
    from gligen_amd import synthetic as syn
    from helpers import _fake_omegaconf_pickle, mse
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    monkeypatch.chdir(tmp_path)
    _, native, processor, tok = _native_clip_model(tmp_path)
    torch.save(mgv.projection_matrix(), tmp_path / "projection_matrix")
    paths = _pngs(tmp_path, 2)
    # ---- the reference features first: HF fp32 on the CPU
    monkeypatch.setattr(gi, "device", "cpu")
    img_feats = [gi.get_clip_feature(native, processor, p, is_image=True) for p in paths]
    monkeypatch.setattr(gi, "device", dev)
    native = native.to(dev)
    monkeypatch.setattr(gi, "_CLIP", {"model": native, "processor": processor})

    def no_forward(*a, **k):
        raise AssertionError("the HF CLIP model must not run: image features come from the native vision tower")

    monkeypatch.setattr(type(native.vision_model), "forward", no_forward)
    monkeypatch.setattr(type(native), "forward", no_forward)
    B, hw, steps, seed = 2, 16, 4, 5
    tcfg = transformers.CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=256, num_hidden_layers=2, num_attention_heads=12,
                                       max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=768, eos_token_id=tok.eos_token_id,
                                       bos_token_id=tok.bos_token_id, pad_token_id=tok.eos_token_id)
    monkeypatch.setattr(transformers.CLIPTokenizer, "from_pretrained", classmethod(lambda cls, *a, **k: tok))
    monkeypatch.setattr(transformers.CLIPTextModel, "from_pretrained", classmethod(lambda cls, *a, **k: transformers.CLIPTextModel(tcfg)))
    cfg = gi.synthetic_config("text_image", inpaint=False, image_size=hw)
    cfg["model"]["params"].update(syn.UNET_CFG_SMALL, image_size=hw, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text_image"])
    cfg["autoencoder"]["params"]["ddconfig"] = dict(syn.VAE_DDCONFIG_SMALL)
    cfg["text_encoder"] = dict(target="ldm.modules.encoders.modules.FrozenCLIPEmbedder")
    unet = syn.fill_module_(gi.instantiate_from_config(cfg["model"]).eval(), 1234)
    ae = syn.fill_module_(gi.instantiate_from_config(cfg["autoencoder"]).eval(), 4321)
    torch.manual_seed(7)
    enc = FrozenCLIPEmbedder(device="cpu")                      # the HF module, fp32, on the CPU: the reference side
    assert enc.tokenizer is tok and enc.backend == "hf"
    diffusion = gi.instantiate_from_config(cfg["diffusion"])
    path = tmp_path / "diffusion_pytorch_model.bin"
    te_sd = {("transformer.text_model." + k[len("transformer."):] if not k.startswith("transformer.text_model.") else k): v.cpu() for k, v in enc.state_dict().items()}
    _fake_omegaconf_pickle(path, dict(model=unet.state_dict(), autoencoder=ae.state_dict(), text_encoder=te_sd,
                                      diffusion=diffusion.state_dict(), iters=1, config={k: v for k, v in cfg.items()}))
    boxes, _ = syn.make_boxes(1, 2, seed=4)
    meta = dict(ckpt=str(path), prompt="a teddy bear sitting next to a bird", phrases=[None, "a bird"], images=[paths[0], paths[1]],
                locations=boxes[0, :2].tolist(), alpha_type=[0.5, 0.0, 0.5], save_folder_name="native_clip_images")
    args = dict(batch_size=B, guidance_scale=7.5, negative_prompt="blurry", no_plms=False, folder=str(tmp_path / "out"), steps=steps, seed=seed,
                native_clip=True)
    torch.save(syn.sd_first_conv_state(), tmp_path / "SD_input_conv_weight_bias.pth")
    samples = gi.run(dict(meta), dict(args))
    assert sorted(os.listdir(tmp_path / "out" / "native_clip_images")) == ["0.png", "1.png"]
    assert samples.shape == (B, 3, 2 * hw, 2 * hw) and torch.isfinite(samples).all()
    assert "vision" in gi._CLIP                                  # the engine is cached next to the model
    # ---- the reference side: HF fp32 on the CPU for everything CLIP, the same engine for the rest
    context, uc = enc.encode([meta["prompt"]] * B), enc.encode(["blurry"] * B)
    txt = enc.encode(["a bird"], return_pooler_output=True)[1]
    unet, ae, diffusion = unet.to(dev), ae.to(dev), diffusion.to(dev)
    unet.grounding_tokenizer_input = gi.instantiate_from_config(cfg["grounding_tokenizer_input"])
    batch = gi.prepare_batch(dict(meta, text_embeddings=[None, txt[0]], image_embeddings=[f for f in img_feats]), B)
    assert batch["image_masks"][0, :3].tolist() == [1, 1, 0] and batch["text_masks"][0, :3].tolist() == [0, 1, 0]
    assert float(batch["image_embeddings"][0, :2].abs().sum()) > 0
    x_T = torch.randn((B, 4, hw, hw), generator=torch.Generator().manual_seed(seed)).to(dev)
    ref = gi.generate(unet, ae, diffusion, batch, context.to(dev), uc.to(dev), steps=steps, guidance_scale=7.5, alpha_type=meta["alpha_type"],
                      starting_noise=x_T)
    rel = mse(ref, samples) / float(ref.float().var())
    # the image features matter to the picture: without them it is another picture by far more than the budget
    blind = gi.prepare_batch(dict(meta, text_embeddings=[None, txt[0]], image_embeddings=[None, None]), B)
    ref_blind = gi.generate(unet, ae, diffusion, blind, context.to(dev), uc.to(dev), steps=steps, guidance_scale=7.5, alpha_type=meta["alpha_type"],
                            starting_noise=x_T)
    rel_blind = mse(ref, ref_blind) / float(ref.float().var())
    report["file_to_image_native_clip_images"] = dict(rel_mse_images=rel, bar=E2E_IMG_TOL, rel_mse_without_image_features=rel_blind)
    print(json.dumps(report["file_to_image_native_clip_images"]))
    assert rel <= E2E_IMG_TOL, rel
    assert rel_blind > 10 * E2E_IMG_TOL, rel_blind
    gi._CLIP.pop("vision").close()
    unet._drop_engine()
    ae._drop_engine()
