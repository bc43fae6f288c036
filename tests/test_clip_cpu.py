"""The native CLIP text tower without a GPU: C ABI, goldens, key handling, EOS pooling rule, refusals and the ISA of clip.hip."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_clip", os.path.join(ROOT, "tools", "make_golden_clip.py"))
mgc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgc)


def test_clip_entry_points_are_declared_exported_and_bound(tmp_path):
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    header = open(os.path.join(ROOT, "include", "gligen_amd.h")).read()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("gl_clip_text_configure", "gl_clip_text_encode"):
        assert re.search(r"\bint " + name + r"\s*\(", header) and hasattr(lib, name) and name in _lib.SYMBOLS, name
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gligen_amd.h"\nint main(void) { printf("%zu\\n", sizeof(gl_clip_text_config)); return 0; }\n')
    subprocess.run([shutil.which("gcc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout
    assert int(out) == ctypes.sizeof(_lib.ClipTextConfig)


@pytest.mark.parametrize("name", ["small", "full"])
def test_goldens_are_hf_fp32_outputs(name):
    """Re-running transformers' CLIPTextModel in fp32 on the seeded weights reproduces the committed files (<= 1e-10 relative MSE:
    fp32 summation order across thread counts), and the stored yardsticks are those of this model."""
    g = mgc.load_case(name)
    out = mgc.run_case(name)
    rel = lambda a, b: float(((a.astype(np.float64) - b) ** 2).mean() / (b.astype(np.float64) ** 2).mean())
    assert np.array_equal(out["ids"], g["ids"])
    assert rel(out["last_hidden"], g["last_hidden"]) <= 1e-10 and rel(out["pooled"], g["pooled"]) <= 1e-10
    assert g["last_hidden"].shape == (len(g["ids"]), 77, 768)
    for k in ("autocast_rel_mse_hidden", "autocast_rel_mse_pooled"):
        assert 0.5 < float(out[k]) / float(g[k]) < 2.0, k
    # the pooled row is the EOS row
    lengths = mgc.CASES[name]["lengths"]
    for i, n in enumerate(lengths):
        assert np.array_equal(g["pooled"][i], g["last_hidden"][i, n + 1])


def test_both_key_layouts_give_the_same_upload_dictionary():
    from gligen_amd.runtime import clip_text_keys, clip_text_upload_dict
    tower = mgc.build_tower(2, 256)
    sd5 = {"transformer." + (k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in tower.state_dict().items()}
    sd4 = {"transformer.text_model." + k[len("transformer."):]: v for k, v in sd5.items()}
    sd4["transformer.text_model.embeddings.position_ids"] = torch.arange(77)[None]
    a, b = clip_text_upload_dict(sd4, 2), clip_text_upload_dict(sd5, 2)
    assert list(a) == list(b) == clip_text_keys(2) and len(a) == 4 + 16 * 2 and len(clip_text_keys(12)) == 196
    assert all(torch.equal(a[k], b[k]) for k in a) and not any("position_ids" in k for k in a)
    del sd5["transformer.encoder.layers.1.mlp.fc2.bias"]
    with pytest.raises(KeyError, match="fc2.bias"):
        clip_text_upload_dict(sd5, 2)


@pytest.mark.parametrize("eos_token_id", [2, 49407])
def test_eos_positions_is_where_hf_pools(eos_token_id):
    import transformers
    from ldm.modules.encoders.modules import eos_positions
    ids = torch.from_numpy(mgc.load_case("small")["ids"])
    last = torch.full((1, 77), 7, dtype=torch.int64)
    last[0, 0], last[0, 76] = 49406, 49407                       # a row whose EOS is the last position
    ids = torch.cat([ids, last])
    model = transformers.CLIPTextModel(transformers.CLIPTextConfig(
        vocab_size=49408, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1, max_position_embeddings=77,
        hidden_act="quick_gelu", eos_token_id=eos_token_id)).eval()
    with torch.no_grad():
        out = model(input_ids=ids)
    pos = eos_positions(ids, eos_token_id)
    assert pos.tolist() == [2, 8, 31, 76, 76]
    assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(len(ids)), pos])


def test_native_backend_never_falls_back():
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    with pytest.raises(ValueError):
        FrozenCLIPEmbedder(backend="bogus")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    enc = FrozenCLIPEmbedder(device="cpu", backend="hip")
    with pytest.raises(RuntimeError, match="HIP device|no HIP device"):
        enc.encode_ids(torch.tensor([[49406, 5, 49407]]))
    assert FrozenCLIPEmbedder(device="cpu").backend == "hf"


def test_prepare_batch_takes_phrase_features_from_the_text_encoder(monkeypatch):
    """prepare_batch(text_encoder=...): one batched encode of the phrases that are given, pooled rows as the text embeddings, and
    CLIPModel (gi._clip) is not touched when the meta has no images."""
    import gligen_inference as gi
    monkeypatch.setattr(gi, "device", "cpu")
    monkeypatch.setattr(gi, "_clip", lambda: (_ for _ in ()).throw(AssertionError("CLIPModel must not be loaded")))
    calls = []

    class Enc:
        def encode(self, text, return_pooler_output=False):
            calls.append(list(text))
            return torch.zeros(len(text), 77, 768), torch.arange(len(text), dtype=torch.float32)[:, None].expand(len(text), 768) + 1

    meta = dict(phrases=["a cat", None, "a dog"], locations=[[0, 0, .5, .5], [.1, .1, .2, .2], [.5, .5, 1, 1]])
    out = gi.prepare_batch(meta, 2, text_encoder=Enc())
    assert calls == [["a cat", "a dog"]]
    assert out["text_embeddings"].shape == (2, 30, 768) and out["text_masks"][0, :4].tolist() == [1, 0, 1, 0]
    assert out["text_embeddings"][1, 0, 0] == 1 and out["text_embeddings"][1, 2, 0] == 2 and float(out["image_masks"].sum()) == 0


def test_clip_attention_kernel_isa(tmp_path):
    """clip_attn_kernel: both products on v_mfma_f32_32x32x16_bf16, no scratch, no spills, LDS small enough for two workgroups per CU."""
    from gligen_amd.build import EXTRA_FLAGS, FLAGS, SOURCES
    assert "clip.hip" in SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "clip.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *EXTRA_FLAGS.get("clip.hip", []), "-I", os.path.join(ROOT, "include"),
                        "--offload-device-only", "-S", os.path.join(ROOT, "gligen_amd", "csrc", "clip.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    name = re.search(r"^(_ZN2gl16clip_attn_kernel[^:\s]*):", asm, re.M).group(1)
    a = asm.index(name + ":")
    body = asm[a:asm.index(".Lfunc_end", a)]
    assert body.count("v_mfma_f32_32x32x16_bf16") >= 4 + 2 and "scratch_" not in body
    entry = next(e for e in re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])[1:] if re.search(r"\.name:\s*" + re.escape(name) + r"\s", e))
    val = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", entry).group(1))
    assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0
    assert val("group_segment_fixed_size") <= 64 * 1024
    for kern in re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])[1:]:      # the small kernels beside it
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", kern).group(1)) == 0
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", kern).group(1)) == 0
