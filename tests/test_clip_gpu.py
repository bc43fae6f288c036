"""The native CLIP text tower (Engine::clip_text_encode, FrozenCLIPEmbedder(backend="hip")) on the MI355X against the goldens of
tools/make_golden_clip.py: transformers' CLIPTextModel in fp32 on the CPU. Bars are 5 x the golden's own autocast yardstick
(torch's bf16 error on the same model), read from the file."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_clip", os.path.join(ROOT, "tools", "make_golden_clip.py"))
mgc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgc)

REPORT = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float(((a - b) ** 2).mean() / (b ** 2).mean())


def _embedder(name, dev, heads=12):
    """FrozenCLIPEmbedder(backend="hip") holding the golden's seeded tower."""
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    c = mgc.CASES[name]
    tower = mgc.build_tower(c["layers"], c["intermediate"])
    enc = FrozenCLIPEmbedder(device=str(dev), backend="hip")
    enc.transformer = tower
    return enc.to(dev)


@pytest.fixture(scope="module")
def report():
    """The measured values: printed by each test, and kept as parity_report_clip.json in $GL_PARITY_REPORT_DIR when that is set."""
    yield REPORT
    out = os.environ.get("GL_PARITY_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_report_clip.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


@pytest.mark.parametrize("name", ["small", "full"])
def test_parity_with_hf_fp32(name, report):
    """last_hidden and pooled, overall and for EACH sequence separately, within 5 x the overall autocast yardstick of the golden."""
    dev = _dev()
    g = mgc.load_case(name)
    enc = _embedder(name, dev)
    ids = torch.from_numpy(g["ids"])
    hidden, pooled = enc.encode_ids(ids, return_pooler_output=True)
    assert hidden.shape == g["last_hidden"].shape and pooled.shape == g["pooled"].shape
    assert torch.isfinite(hidden).all() and torch.isfinite(pooled).all()
    bar_h, bar_p = 5 * float(g["autocast_rel_mse_hidden"]), 5 * float(g["autocast_rel_mse_pooled"])
    rec = dict(bar_hidden=bar_h, bar_pooled=bar_p, hidden=_rel(hidden, g["last_hidden"]), pooled=_rel(pooled, g["pooled"]),
               hidden_per_seq=[_rel(hidden[i], g["last_hidden"][i]) for i in range(len(ids))],
               pooled_per_seq=[_rel(pooled[i], g["pooled"][i]) for i in range(len(ids))],
               autocast_hidden_per_seq=g["autocast_rel_mse_hidden_per_seq"].tolist(), autocast_pooled_per_seq=g["autocast_rel_mse_pooled_per_seq"].tolist(),
               launches=enc.engine.launch_count())
    report["parity_" + name] = rec
    print(json.dumps(rec))
    assert rec["hidden"] <= bar_h and rec["pooled"] <= bar_p, rec
    assert max(rec["hidden_per_seq"]) <= bar_h and max(rec["pooled_per_seq"]) <= bar_p, rec
    enc._drop_engine()


def test_the_mask_is_a_mask(report):
    """Other ids BEHIND each sequence's EOS leave every row at or before the EOS and the pooled row bit-identical; another id in
    front of it changes the pooled row."""
    dev = _dev()
    g = mgc.load_case("small")
    enc = _embedder("small", dev)
    ids = torch.from_numpy(g["ids"]).clone()
    lengths = json.loads(str(g["meta"]))["lengths"]
    h0, p0 = enc.encode_ids(ids, return_pooler_output=True)
    other = ids.clone()
    gen = torch.Generator().manual_seed(9)
    for i, n in enumerate(lengths):
        other[i, n + 2:] = torch.randint(0, 49406, (77 - n - 2,), generator=gen)     # EOS stays the row's largest id (legacy pooling rule)
    h1, p1 = enc.encode_ids(other, return_pooler_output=True)
    assert torch.equal(p0, p1)
    for i, n in enumerate(lengths):
        assert torch.equal(h0[i, :n + 2], h1[i, :n + 2]), i
        assert n + 2 == 77 or not torch.equal(h0[i, n + 2:], h1[i, n + 2:]), i
    front = ids.clone()
    front[:, 1] = (front[:, 1] + 1) % 49406
    _, p2 = enc.encode_ids(front, return_pooler_output=True)
    assert all(not torch.equal(p0[i], p2[i]) for i in range(len(ids)))
    enc._drop_engine()


def test_identical_rows_are_encoded_once_and_unpadded_phrase_pools_the_same_row(report):
    dev = _dev()
    from gligen_amd.engine import Engine
    g = mgc.load_case("small")
    enc = _embedder("small", dev)
    row = torch.from_numpy(g["ids"])[1:2]
    seen = []
    orig = Engine.clip_text_encode

    def spy(self, ids, eos):
        seen.append(tuple(ids.shape))
        return orig(self, ids, eos)

    Engine.clip_text_encode = spy
    try:
        h1, p1 = enc.encode_ids(row, return_pooler_output=True)
        h4, p4 = enc.encode_ids(row.repeat(4, 1), return_pooler_output=True)
    finally:
        Engine.clip_text_encode = orig
    assert seen == [(1, 77), (1, 77)]
    assert h4.shape == (4, 77, 768) and all(torch.equal(h4[i], h1[0]) and torch.equal(p4[i], p1[0]) for i in range(4))
    # the phrase alone, unpadded (BOS, 7 tokens, EOS), as get_clip_feature tokenizes it: same pooled row within the parity bar
    _, pu = enc.encode_ids(row[:, :9], return_pooler_output=True)
    rel = _rel(pu, p1)
    report["unpadded_vs_padded_pooled"] = rel
    assert rel <= 5 * float(g["autocast_rel_mse_pooled"]), rel
    enc._drop_engine()


E2E_IMG_TOL = 8.5e-4    # the project's end-to-end image budget (tests/test_configs_gpu.py)


def test_file_to_image_without_torch_clip_compute(tmp_path, monkeypatch, report):
    """run(meta, args) with native_clip from a checkpoint FILE in the reference's format (the construction of
    test_run_from_checkpoint_file, with a text tower of 2 layers / 12 heads of d = 64): prompt, negative prompt and phrase features
    come from the checkpoint's own tower on the HIP path -- CLIPModel (gi._clip) raises if it is touched. The images are compared
    with generate() fed the context, uc and phrase features of the HF module in fp32 on the CPU from the same weights."""
    dev = _dev()
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import transformers
    import gligen_inference as gi
    from gligen_amd import synthetic as syn
    from helpers import _fabricated_clip, _fake_omegaconf_pickle, mse
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    monkeypatch.setattr(gi, "device", dev)
    monkeypatch.chdir(tmp_path)

    def no_clip():
        raise AssertionError("CLIPModel must not be loaded: the phrase features come from the checkpoint's text tower")

    monkeypatch.setattr(gi, "_clip", no_clip)
    B, hw, steps, seed = 2, 16, 4, 5
    _, _, tok = _fabricated_clip(tmp_path)
    tcfg = transformers.CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=256, num_hidden_layers=2, num_attention_heads=12,
                                       max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=768, eos_token_id=tok.eos_token_id,
                                       bos_token_id=tok.bos_token_id, pad_token_id=tok.eos_token_id)
    monkeypatch.setattr(transformers.CLIPTokenizer, "from_pretrained", classmethod(lambda cls, *a, **k: tok))
    monkeypatch.setattr(transformers.CLIPTextModel, "from_pretrained", classmethod(lambda cls, *a, **k: transformers.CLIPTextModel(tcfg)))
    cfg = gi.synthetic_config("text", inpaint=False, image_size=hw)
    cfg["model"]["params"].update(syn.UNET_CFG_SMALL, image_size=hw, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"])
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
    meta = dict(ckpt=str(path), prompt="a teddy bear sitting next to a bird", phrases=["a teddy bear", "a bird"], locations=boxes[0, :2].tolist(),
                alpha_type=[0.5, 0.0, 0.5], save_folder_name="native_clip")
    args = dict(batch_size=B, guidance_scale=7.5, negative_prompt="blurry", no_plms=False, folder=str(tmp_path / "out"), steps=steps, seed=seed,
                native_clip=True)
    torch.save(syn.sd_first_conv_state(), tmp_path / "SD_input_conv_weight_bias.pth")
    samples = gi.run(dict(meta), dict(args))
    assert sorted(os.listdir(tmp_path / "out" / "native_clip")) == ["0.png", "1.png"]
    assert samples.shape == (B, 3, 2 * hw, 2 * hw) and torch.isfinite(samples).all()
    # ---- the reference side: HF fp32 on the CPU for everything CLIP, the same engine for the rest
    context, uc = enc.encode([meta["prompt"]] * B), enc.encode(["blurry"] * B)
    feats = enc.encode(meta["phrases"], return_pooler_output=True)[1]
    assert context.device.type == "cpu" and context.shape == (B, 77, 768) and not torch.equal(context, uc)
    unet, ae, diffusion = unet.to(dev), ae.to(dev), diffusion.to(dev)
    unet.grounding_tokenizer_input = gi.instantiate_from_config(cfg["grounding_tokenizer_input"])
    batch = gi.prepare_batch(dict(meta, text_embeddings=[f for f in feats]), B)
    assert float(batch["text_embeddings"][0, :2].abs().sum()) > 0
    x_T = torch.randn((B, 4, hw, hw), generator=torch.Generator().manual_seed(seed)).to(dev)
    ref = gi.generate(unet, ae, diffusion, batch, context.to(dev), uc.to(dev), steps=steps, guidance_scale=7.5, alpha_type=meta["alpha_type"],
                      starting_noise=x_T)
    rel = mse(ref, samples) / float(ref.float().var())
    report["file_to_image_native_clip"] = dict(rel_mse_images=rel, bar=E2E_IMG_TOL)
    print(json.dumps(report["file_to_image_native_clip"]))
    assert rel <= E2E_IMG_TOL, rel
    unet._drop_engine()
    ae._drop_engine()


def test_other_head_dims_are_refused_by_name():
    dev = _dev()
    import transformers
    from gligen_amd import GligenAmdError
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    enc = FrozenCLIPEmbedder(device=str(dev), backend="hip")
    enc.transformer = transformers.CLIPTextModel(transformers.CLIPTextConfig(
        vocab_size=49408, hidden_size=768, intermediate_size=256, num_hidden_layers=1, num_attention_heads=8, max_position_embeddings=77,
        hidden_act="quick_gelu")).eval()
    enc = enc.to(dev)
    with pytest.raises(GligenAmdError, match="head dim 96"):
        enc.encode_ids(torch.tensor([[49406, 5, 49407]]))
