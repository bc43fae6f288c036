"""The native CLIP vision tower without a GPU: C ABI, state-dict handling, goldens (and the condition that makes them a test of the
pixels), host wiring of get_clip_image_features / prepare_batch, and the ISA of clip_attn_long_kernel."""
import ctypes
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
_spec = importlib.util.spec_from_file_location("make_golden_clip_vision", os.path.join(ROOT, "tools", "make_golden_clip_vision.py"))
mgv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgv)


def test_clip_vision_entry_points_are_declared_exported_and_bound(tmp_path):
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    header = open(os.path.join(ROOT, "include", "gligen_amd.h")).read()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("gl_clip_vision_configure", "gl_clip_vision_encode", "gl_op_clip_attention"):
        assert re.search(r"\bint " + name + r"\s*\(", header) and hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS) == 59 == len(set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", header)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gligen_amd.h"\nint main(void) { printf("%zu\\n", sizeof(gl_clip_vision_config)); return 0; }\n')
    subprocess.run([shutil.which("gcc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout
    assert int(out) == ctypes.sizeof(_lib.ClipVisionConfig) == 32


def test_clip_model_and_vision_model_state_dicts_give_the_same_upload_dictionary():
    import transformers
    from gligen_amd.runtime import clip_vision_keys, clip_vision_upload_dict
    c = mgv.CASES["small50"]
    tower = mgv.build_tower(c)
    vsd = dict(tower.state_dict())
    full = transformers.CLIPModel(transformers.CLIPConfig(
        text_config=dict(hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1), vision_config=mgv.vision_config(c).to_dict(),
        projection_dim=mgv.PROJECTION)).eval()
    full.load_state_dict(vsd, strict=False)
    msd = dict(full.state_dict())
    assert any(k.startswith("text_model.") for k in msd) and "logit_scale" in msd and "text_projection.weight" in msd
    msd["vision_model.embeddings.position_ids"] = torch.arange(50)[None]       # a buffer of old transformers versions
    a, b = clip_vision_upload_dict(vsd, 2), clip_vision_upload_dict(msd, 2)
    assert list(a) == list(b) == clip_vision_keys(2) and len(a) == 8 + 16 * 2 and len(clip_vision_keys(24)) == 392
    assert all(torch.equal(a[k], b[k]) for k in a) and not any("position_ids" in k or k.startswith("text_") for k in a)
    missing = dict(vsd)
    del missing["vision_model.encoder.layers.1.mlp.fc2.bias"]
    with pytest.raises(KeyError, match="fc2.bias"):
        clip_vision_upload_dict(missing, 2)
    with pytest.raises(KeyError, match="pre_layrnorm.weight"):
        clip_vision_upload_dict({k: v for k, v in msd.items() if k != "vision_model.pre_layrnorm.weight"}, 2)
    with pytest.raises(KeyError, match="layers.2.mlp.fc1.weight"):
        clip_vision_upload_dict(dict(vsd, **{"vision_model.encoder.layers.2.mlp.fc1.weight": torch.zeros(1)}), 2)
    with pytest.raises(KeyError, match="something_else"):
        clip_vision_upload_dict(dict(vsd, something_else=torch.zeros(1)), 2)


def test_small_golden_is_the_hf_fp32_output():
    """Re-running transformers' CLIPVisionModelWithProjection in fp32 on the seeded weights and pixels reproduces the committed file
    (<= 1e-10 relative MSE, the fp32 reproducibility tolerance of the text golden), and the stored yardsticks are this model's."""
    g = mgv.load_case("small")
    out = mgv.run_case("small")
    rel = lambda a, b: float(((a.astype(np.float64) - b) ** 2).mean() / (b.astype(np.float64) ** 2).mean())
    assert g["last_hidden"].shape == (3, 257, 256) and g["pooled"].shape == (3, 256) and g["image_embeds"].shape == g["feature"].shape == (3, 768)
    for k in ("last_hidden", "pooled", "image_embeds", "feature"):
        assert rel(out[k], g[k]) <= 1e-10, k
    for k in ("hidden", "pooled", "embeds", "feature"):
        assert 0.5 < float(out["autocast_rel_mse_" + k]) / float(g["autocast_rel_mse_" + k]) < 2.0, k
    assert np.allclose(np.linalg.norm(g["feature"], axis=-1), 28.7, rtol=1e-5)
    assert json.loads(str(g["meta"]))["tokens"] == 257


@pytest.mark.parametrize("name", ["small", "small50", "full"])
def test_the_goldens_images_are_distinct(name):
    """The condition that makes the parity bars a test of the pixels: the smallest relative squared distance between two images' final
    features is >= 100 x the feature bar (5 x the autocast yardstick), so answering one image with another's feature -- or ignoring
    the pixels -- is at least 100 bars away."""
    g = mgv.load_case(name)
    n = mgv.CASES[name]["images"]
    d = g["feature_pairwise_rel_sq_dist"]
    f = g["feature"].astype(np.float64)
    again = ((f[:, None] - f[None]) ** 2).sum(-1) / (f ** 2).sum(-1)[None]
    assert d.shape == (n, n) and np.allclose(d, again, rtol=1e-6, atol=1e-12)
    smallest = float(d[~np.eye(n, dtype=bool)].min())
    bar = 5 * float(g["autocast_rel_mse_feature"])
    print(json.dumps(dict(case=name, smallest_pairwise=smallest, feature_bar=bar, ratio=smallest / bar)))
    assert smallest >= 100 * bar, (smallest, bar)
    for k in ("hidden", "pooled", "embeds", "feature"):
        assert 0 < float(g["autocast_rel_mse_" + k]) < 1e-3 and g["autocast_rel_mse_" + k + "_per_image"].shape == (n,)
    if name == "full":
        assert g["rows"].tolist() == [0, 1, 17, 128, 255, 256] and g["last_hidden"].shape == (4, 6, 1024)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"clip_vision_{name}.npz")) < 1 << 20


class _SpyVision:
    """Stands where the native engine stands: counts the calls, answers with features that depend on the pixels."""
    def __init__(self):
        self.calls = []

    def clip_vision_encode(self, pixel_values):
        self.calls.append(tuple(pixel_values.shape))
        S = pixel_values.shape[0]
        embeds = pixel_values.float().mean(dim=(1, 2, 3))[:, None] + torch.arange(768, dtype=torch.float32)[None] / 768
        return torch.zeros(S, 50, 64), torch.zeros(S, 64), embeds


def _pngs(tmp_path, n):
    from PIL import Image
    paths = []
    for i in range(n):
        Image.fromarray((np.random.RandomState(i).rand(40 + 7 * i, 60, 3) * 255).astype(np.uint8)).save(tmp_path / f"im{i}.png")
        paths.append(str(tmp_path / f"im{i}.png"))
    return paths


def test_image_features_are_one_batched_encode_and_prepare_batch_never_runs_the_hf_forward(tmp_path, monkeypatch):
    import gligen_inference as gi
    from helpers import _fabricated_clip
    model, processor, _ = _fabricated_clip(tmp_path)
    monkeypatch.setattr(gi, "device", "cpu")
    monkeypatch.chdir(tmp_path)
    P = torch.randn(768, 768, generator=torch.Generator().manual_seed(5)) * 0.03
    torch.save(P, tmp_path / "projection_matrix")
    paths = _pngs(tmp_path, 3)

    def no_forward(*a, **k):
        raise AssertionError("the HF model must not run: the images go through the native vision tower")

    monkeypatch.setattr(type(model), "forward", no_forward)
    monkeypatch.setattr(type(model.vision_model), "forward", no_forward)
    spy = _SpyVision()
    feats = gi.get_clip_image_features(model, processor, [paths[0], None, paths[1], paths[2], None], spy)
    assert spy.calls == [(3, 3, 224, 224)]
    assert [f is None for f in feats] == [False, True, False, False, True]
    for f in (feats[0], feats[2], feats[3]):
        assert f.shape == (1, 768) and abs(float(f.norm()) - 28.7) < 1e-3
    from PIL import Image
    pix = processor(images=[Image.open(paths[1]).convert("RGB")], return_tensors="pt")["pixel_values"]
    want = _SpyVision().clip_vision_encode(pix)[2] @ P
    assert torch.allclose(feats[2], want / want.norm() * 28.7, atol=1e-4)
    assert gi.get_clip_image_features(model, processor, [None, None], spy) == [None, None] and len(spy.calls) == 1
    one = gi.get_clip_feature(model, processor, paths[1], is_image=True, vision=spy)
    assert torch.allclose(one, feats[2], atol=1e-4) and spy.calls[-1] == (1, 3, 224, 224)
    assert gi.get_clip_feature(model, processor, None, is_image=True, vision=spy) is None

    # prepare_batch's native branch: phrases through the text encoder, images through the cached vision engine
    spy2 = _SpyVision()
    monkeypatch.setattr(gi, "_CLIP", {"model": model, "processor": processor, "vision": spy2})

    class Enc:
        def encode(self, text, return_pooler_output=False):
            return torch.zeros(len(text), 77, 768), torch.ones(len(text), 768)

    meta = dict(phrases=[None, "a bird", None], images=[paths[0], paths[2], None], locations=[[0, 0, .5, .5], [.1, .1, .2, .2], [.5, .5, 1, 1]])
    out = gi.prepare_batch(meta, 2, text_encoder=Enc())
    assert spy2.calls == [(2, 3, 224, 224)]
    assert out["image_masks"][0, :4].tolist() == [1, 1, 0, 0] and out["text_masks"][0, :4].tolist() == [0, 1, 0, 0]
    assert torch.allclose(out["image_embeddings"][1, 1], feats[3][0], atol=1e-4) and float(out["image_embeddings"][0, 2].abs().max()) == 0
    assert abs(float(out["image_embeddings"][0, 0].norm()) - 28.7) < 1e-3


def test_unsupported_towers_are_refused_by_name_before_the_device_is_needed(tmp_path):
    """hidden_act and num_channels are host-side refusals (module_device comes first on a machine without a GPU, so the checks are
    exercised on their own here through the configuration objects)."""
    from gligen_amd import runtime

    class FakeParam:
        is_cuda = True
        device = torch.device("cpu")

    def tower(**kw):
        import transformers
        cfg = mgv.vision_config(mgv.CASES["small50"], **{k: v for k, v in kw.items() if k == "hidden_act"})
        for k, v in kw.items():
            setattr(cfg, k, v)
        m = transformers.CLIPVisionModelWithProjection(cfg).eval()
        m.parameters = lambda: iter([FakeParam()])
        return m

    with pytest.raises(NotImplementedError, match="hidden_act='gelu'"):
        runtime.build_clip_vision_engine(tower(hidden_act="gelu"))
    with pytest.raises(NotImplementedError, match="num_channels=4"):
        runtime.build_clip_vision_engine(tower(num_channels=4))
    assert 0.05 < runtime.clip_vision_arena_gb() < 0.12


def test_clip_attn_long_kernel_isa(tmp_path):
    """clip_attn_long_kernel: both products on v_mfma_f32_32x32x16_bf16 (4 + 4 per key tile), no scratch, no spills, LDS small enough
    for two workgroups in the 160 KB of a CU, registers for at least the two waves per SIMD that makes."""
    from gligen_amd.build import EXTRA_FLAGS, SOURCES
    assert "clip.hip" in SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "clip.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *EXTRA_FLAGS.get("clip.hip", []), "-I", os.path.join(ROOT, "include"),
                        "--offload-device-only", "-S", os.path.join(ROOT, "gligen_amd", "csrc", "clip.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    name = re.search(r"^(_ZN2gl21clip_attn_long_kernel[^:\s]*):", asm, re.M).group(1)
    a = asm.index(name + ":")
    body = asm[a:asm.index(".Lfunc_end", a)]
    assert body.count("v_mfma_f32_32x32x16_bf16") >= 4 + 4 and "scratch_" not in body
    kernels = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])[1:]
    entry = next(e for e in kernels if re.search(r"\.name:\s*" + re.escape(name) + r"\s", e))
    val = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", entry).group(1))
    assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0
    assert val("group_segment_fixed_size") == 78848 and 2 * val("group_segment_fixed_size") <= 160 * 1024
    assert val("vgpr_count") <= 256 and val("max_flat_workgroup_size") == 256        # 2 waves per SIMD = two workgroups of four waves per CU
    for kern in kernels:      # the small kernels beside it
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", kern).group(1)) == 0
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", kern).group(1)) == 0
