"""LoRA adapters on the host, no GPU: the safetensors container, the name tables on the SD-1.4 topology and on the small golden
config against the diffusers layout of tests/lora_ref.py, kohya's format and every refusal, the C ABI of include/gligen_amd_lora.h, and
the command line."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess

import pytest
import torch
from torch import nn

import lora_ref as ref
from helpers import ROOT
from gligen_amd import lora
from gligen_amd import synthetic as syn


def _unet(cfg, kind="text", inpaint=False):
    """The UNetModel of a config on the meta device: shapes and module paths, no weights."""
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    with torch.device("meta"):
        return UNetModel(**dict(cfg, grounding_tokenizer=syn.GROUNDING_TOKENIZERS[kind], inpaint_mode=inpaint)).eval()


class _Embedder(nn.Module):
    """A FrozenCLIPEmbedder as far as the name table and the merge are concerned: .transformer and _drop_engine()."""

    def __init__(self, layers=12, wrapped=False):
        super().__init__()
        import transformers
        cfg = transformers.CLIPTextConfig(vocab_size=64, hidden_size=32, intermediate_size=48, num_hidden_layers=layers, num_attention_heads=2,
                                          max_position_embeddings=77, projection_dim=32, bos_token_id=1, eos_token_id=2, pad_token_id=2)
        tower = transformers.CLIPTextModel(cfg)
        if wrapped != hasattr(tower, "text_model"):      # the other transformers layout: with / without the .text_model level
            inner = tower.text_model if hasattr(tower, "text_model") else tower
            tower = nn.Module()
            if wrapped:
                tower.text_model = inner
            else:
                tower.encoder, tower.embeddings, tower.final_layer_norm = inner.encoder, inner.embeddings, inner.final_layer_norm
        self.transformer = tower
        self.dropped = 0

    def _drop_engine(self):
        self.dropped += 1


# ---- the container ------------------------------------------------------------------------------------------------------------------
def _tensors():
    g = torch.Generator().manual_seed(0)
    return {"a.lora_down.weight": torch.randn(4, 7, generator=g), "a.lora_up.weight": torch.randn(5, 4, generator=g).half(),
            "b.conv": torch.randn(3, 2, 3, 3, generator=g).bfloat16(), "a.alpha": torch.tensor(2.0), "z.empty": torch.zeros(0, 3, dtype=torch.float16)}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def test_safetensors_round_trip_is_bit_exact(tmp_path):
    t = _tensors()
    t["nan"] = torch.tensor([float("nan"), -0.0, float("inf")])                 # payloads and signs survive: bytes, not values
    path = tmp_path / "t.safetensors"
    lora.write_safetensors(path, t, metadata={"ss_network_dim": 4})
    got = lora.read_safetensors(path)
    assert sorted(got) == sorted(t)
    for k in t:
        assert _same_bits(got[k], t[k]), k
    blob = path.read_bytes()
    (n,) = struct.unpack("<Q", blob[:8])
    header = json.loads(blob[8:8 + n])
    assert n % 8 == 0 and header["__metadata__"] == {"ss_network_dim": "4"} and header["a.alpha"] == {"dtype": "F32", "shape": [], "data_offsets": header["a.alpha"]["data_offsets"]}
    assert lora.load_adapter(str(path)).keys() == t.keys()                      # by extension
    other = tmp_path / "noext.bin"
    shutil.copy(path, other)
    assert lora.load_adapter(other).keys() == t.keys()                          # by its first bytes
    torch.save({"state_dict": {k: v for k, v in t.items()}}, tmp_path / "t.pt")
    assert all(_same_bits(v, t[k]) for k, v in lora.load_adapter(tmp_path / "t.pt").items())
    assert lora.load_adapter(t) == t                                            # a plain dict


def test_safetensors_against_the_package(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    t = {k: v for k, v in _tensors().items() if v.numel()}
    lora.write_safetensors(tmp_path / "ours.safetensors", t)
    theirs = st.load_file(str(tmp_path / "ours.safetensors"))
    assert sorted(theirs) == sorted(t) and all(_same_bits(theirs[k], t[k]) for k in t)
    st.save_file({k: v.contiguous() for k, v in t.items()}, str(tmp_path / "theirs.safetensors"), metadata={"x": "y"})
    ours = lora.read_safetensors(tmp_path / "theirs.safetensors")
    assert sorted(ours) == sorted(t) and all(_same_bits(ours[k], t[k]) for k in t)


def test_safetensors_refusals(tmp_path):
    path = tmp_path / "t.safetensors"
    lora.write_safetensors(path, _tensors())
    blob = path.read_bytes()
    for cut, what in ((4, "truncated"), (40, "truncated"), (len(blob) - 5, "truncated")):
        (tmp_path / "cut.safetensors").write_bytes(blob[:cut])
        with pytest.raises(lora.LoraError, match=what):
            lora.read_safetensors(tmp_path / "cut.safetensors")
    (n,) = struct.unpack("<Q", blob[:8])
    header = json.loads(blob[8:8 + n])
    header["a.alpha"]["dtype"] = "I64"
    text = json.dumps(header).encode()
    (tmp_path / "i64.safetensors").write_bytes(struct.pack("<Q", len(text)) + text + blob[8 + n:])
    with pytest.raises(lora.LoraError, match=r"'a.alpha' has unknown dtype 'I64'"):
        lora.read_safetensors(tmp_path / "i64.safetensors")
    header["a.alpha"]["dtype"] = "F16"
    text = json.dumps(header).encode()
    (tmp_path / "fit.safetensors").write_bytes(struct.pack("<Q", len(text)) + text + blob[8 + n:])
    with pytest.raises(lora.LoraError, match="does not fit its data_offsets"):
        lora.read_safetensors(tmp_path / "fit.safetensors")
    (tmp_path / "json.safetensors").write_bytes(struct.pack("<Q", 8) + b"not json")
    with pytest.raises(lora.LoraError, match="is not JSON"):
        lora.read_safetensors(tmp_path / "json.safetensors")
    with pytest.raises(lora.LoraError, match="F32, F16 and BF16 are written"):
        lora.write_safetensors(tmp_path / "x.safetensors", {"i": torch.zeros(2, dtype=torch.int64)})
    with pytest.raises(lora.LoraError, match="does not exist"):
        lora.load_adapter(tmp_path / "nothing.safetensors")
    # the safetensors package is not a dependency: gligen_amd/lora.py imports nothing of it
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "gligen_amd", "lora.py")).read())
    imported = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names} | {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert not any(m and m.split(".")[0] == "safetensors" for m in imported), imported


# ---- the name tables ----------------------------------------------------------------------------------------------------------------
def _check_targets(model, targets):
    table = lora.unet_name_table(model)
    params = dict(model.named_parameters())
    paths = {}
    for name, shape in targets.items():
        assert name in table, name
        w = params[table[name] + ".weight"]
        assert tuple(w.shape) == tuple(shape), (name, table[name], tuple(w.shape), shape)
        paths.setdefault(table[name], set()).add(name)
    # no two names reach one target with different shapes; every alias agrees with the module-path form
    for name, path in table.items():
        assert path + ".weight" in params, (name, path)
        assert table[lora.UNET_PREFIX + path.replace(".", "_")] == path
    by_path = {}
    for name, path in table.items():
        by_path.setdefault(path, []).append(name)
    for path, names in by_path.items():
        shapes = {tuple(targets[n]) for n in names if n in targets}
        assert len(shapes) <= 1, (path, names)
    # every diffusers name reaches a different module
    assert len({table[n] for n in targets}) == len(targets)
    return table, params


def test_name_table_on_the_sd14_topology():
    model = _unet(syn.UNET_CFG)
    targets = ref.diffusers_unet_targets(**ref.SD14)
    table, params = _check_targets(model, targets)
    for name, path in ref.PINNED.items():
        assert table[name] == path, (name, table.get(name))
    # every Linear / Conv2d of the SD-1.4 part of the network (no fuser, no position_net, not the first conv) carries a diffusers name
    covered = {table[n] for n in targets}
    sd_part = {p for p, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d)) and ".fuser." not in p
               and not p.startswith("position_net") and p != "input_blocks.0.0"}
    assert covered == sd_part
    assert table["lora_unet_conv_in"] == "input_blocks.0.0"
    assert table["lora_unet_position_net_linears_0"] == "position_net.linears.0"


def test_target_count_is_what_the_layout_says():
    """281 = 16 transformers x 12 + 22 resnets x 3 + 14 shortcuts + 3 downsamplers + 3 upsamplers + 2 time linears + conv_out, checked
    term by term so that a slip in lora_ref's walk cannot hide behind the same slip in the product's."""
    t = ref.diffusers_unet_targets(**ref.SD14)
    count = lambda pat: sum(1 for k in t if re.search(pat, k))
    assert count(r"_proj_in$") == 16 and count(r"attn[12]_to_(q|k|v|out_0)$") == 16 * 8 and count(r"ff_net_(0_proj|2)$") == 32
    assert count(r"resnets_\d_conv1$") == 22 and count(r"conv_shortcut$") == 2 + 12 and count(r"samplers_0_conv$") == 6
    assert count(r"_proj_out$") == 16 and count(r"time_emb_proj$") == 22 and count(r"resnets_\d_conv2$") == 22
    assert len(t) == 16 * 12 + 22 * 3 + 14 + 6 + 3 == 281


def test_name_table_on_the_small_config_and_other_kinds():
    model = _unet(syn.UNET_CFG_SMALL)
    targets = ref.diffusers_unet_targets(**ref.SMALL)
    table, _ = _check_targets(model, targets)
    assert table["lora_unet_down_blocks_0_downsamplers_0_conv"] == "input_blocks.2.0.op"
    assert table["lora_unet_up_blocks_0_upsamplers_0_conv"] == "output_blocks.1.2.conv"
    assert table["lora_unet_up_blocks_1_resnets_1_conv_shortcut"] == "output_blocks.3.0.skip_connection"
    assert "lora_unet_down_blocks_1_downsamplers_0_conv" not in table
    # an inpainting model and another tokenizer: the same SD part
    for kind, inpaint in (("text", True), ("keypoint", False), ("text_image", False)):
        _check_targets(_unet(syn.UNET_CFG_SMALL, kind, inpaint), targets)


@pytest.mark.parametrize("wrapped", [False, True], ids=["transformers5", "transformers4"])
def test_text_tower_names(wrapped):
    enc = _Embedder(layers=12, wrapped=wrapped)
    table = lora.te_name_table(enc)
    params = dict(enc.named_parameters())
    prefix = "transformer.text_model." if wrapped else "transformer."
    assert table[ref.PINNED_TE] == prefix + "encoder.layers.11.mlp.fc2"
    targets = ref.clip_text_targets(12, 32, 48)
    assert sorted(table) == sorted(targets)
    for name, shape in targets.items():
        assert tuple(params[table[name] + ".weight"].shape) == shape, name


# ---- parsing and resolving -----------------------------------------------------------------------------------------------------------
def _pair(N, K, r, alpha=None, dtype=torch.float32, conv=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    if conv:
        cin, kh = conv
        down, up = torch.randn(r, cin, kh, kh, generator=g), torch.randn(N, r, 1, 1, generator=g)
    else:
        down, up = torch.randn(r, K, generator=g), torch.randn(N, r, generator=g)
    out = {"lora_down.weight": down.to(dtype), "lora_up.weight": up.to(dtype)}
    if alpha is not None:
        out["alpha"] = torch.tensor(float(alpha), dtype=dtype)
    return out


def _named(**groups):
    return {f"{name}.{k}": v for name, g in groups.items() for k, v in g.items()}


Q = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q"          # [320, 320]
CONV = "lora_unet_down_blocks_0_resnets_0_conv1"                                    # [320, 320, 3, 3]
PROJ = "lora_unet_mid_block_attentions_0_proj_in"                                   # [640, 640, 1, 1] on the small config
TE = "lora_te_text_model_encoder_layers_1_mlp_fc1"                                  # [48, 32] in _Embedder


def test_parse_scales_and_shapes():
    state = _named(**{Q: _pair(320, 320, 8, alpha=4, dtype=torch.float16), CONV: _pair(320, None, 4, conv=(320, 3)), PROJ: _pair(640, 640, 2, alpha=2),
                      TE: _pair(48, 32, 2, alpha=1)})
    entries = {e.name: e for e in lora.parse_adapter(state)}
    assert entries[Q].rank == 8 and entries[Q].alpha == 4.0 and entries[Q].factor == 0.5 and entries[Q].down.dtype == torch.float16
    assert entries[CONV].alpha is None and entries[CONV].factor == 1.0 and entries[CONV].rank == 4
    assert entries[TE].is_te and not entries[Q].is_te
    model, enc = _unet(syn.UNET_CFG_SMALL), _Embedder(layers=2)
    (plan,) = lora.plan_loras(model, enc, [(state, 0.8, 0.25)])
    got = {key: (root, scale) for root, key, _, _, scale in plan.merges}
    assert got["input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight"] == (model, 0.8 * 4 / 8)
    assert got["input_blocks.1.0.in_layers.2.weight"] == (model, 0.8)
    assert got["middle_block.1.proj_in.weight"] == (model, 0.8)                       # a [N, r] @ [r, K] pair on a 1 x 1 conv
    assert next(v for k, v in got.items() if k.endswith("encoder.layers.1.mlp.fc1.weight")) == (enc, 0.25 * 1 / 2)
    assert not plan.skipped
    # (source, scale): the text tower takes the same scale; a bare source: 1
    assert [(u, t) for _, u, t in lora._normalise([(state, 0.5), state, (state, 1.0, 0.0)])] == [(0.5, 0.5), (1.0, 1.0), (1.0, 0.0)]
    assert lora.parse_lora_spec("a/b.safetensors:0.8") == ("a/b.safetensors", 0.8, 0.8)
    assert lora.parse_lora_spec("a/b.safetensors:0.8:0") == ("a/b.safetensors", 0.8, 0.0)
    assert lora.parse_lora_spec("C:/x/b.pt") == ("C:/x/b.pt", 1.0, 1.0)


def test_first_conv_is_skipped_and_reported():
    model = _unet(syn.UNET_CFG_SMALL, inpaint=True)        # 9 input channels: an SD adapter's conv_in would not even fit
    for name in ("lora_unet_conv_in", "lora_unet_input_blocks_0_0"):
        state = _named(**{name: _pair(320, None, 4, conv=(4, 3)), Q: _pair(320, 320, 2)})
        (plan,) = lora.plan_loras(model, None, [(state, 1.0)])
        assert [s[0] for s in plan.skipped] == [name] and "first conv" in plan.skipped[0][1]
        assert [key for _, key, *_ in plan.merges] == ["input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight"]


def test_refusals_fire_by_name_and_modify_nothing():
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    model = UNetModel(**dict(syn.UNET_CFG_SMALL, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"])).eval()     # real tensors, on the host
    enc = _Embedder(layers=2)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    good = _pair(320, 320, 2)
    cases = [
        (_named(**{Q: good, "lora_unet_down_blocks_7_nothing": good, **{f"lora_unet_bogus_{i}": good for i in range(12)}}),
         r"resolve to nothing in this model: \['lora_unet_bogus_0'.*\(and 3 more\)"),
        (_named(**{Q: good, "lora_xyz_thing": good}), r"resolve to nothing.*lora_xyz_thing"),
        (_named(**{Q: _pair(320, 321, 2)}), r"shapes that do not fit.*attn1_to_q: lora_up \(320, 2\) @ lora_down \(2, 321\) does not fit .*to_q.weight \(320, 320\)"),
        (_named(**{CONV: _pair(320, None, 2, conv=(320, 1))}), r"does not fit input_blocks.1.0.in_layers.2.weight \(320, 320, 3, 3\)"),
        (_named(**{Q: _pair(64, 320, 2)}), r"does not fit"),
        ({**_named(**{Q: good}), Q + ".hada_w1_a": torch.zeros(2, 2)}, r"hada_w1_a' holds LoHa"),
        ({**_named(**{Q: good}), Q + ".lokr_w1": torch.zeros(2, 2)}, r"holds LoKr"),
        ({**_named(**{Q: good}), Q + ".lora_mid.weight": torch.zeros(2, 2, 3, 3)}, r"holds a Tucker"),
        ({**_named(**{Q: good}), Q + ".dora_scale": torch.zeros(1, 320)}, r"holds DoRA"),
        ({"model.diffusion_model.out.2.weight": torch.zeros(4, 320, 3, 3)}, r"no LoRA pair"),
        ({Q + ".lora_down.weight": good["lora_down.weight"]}, r"no LoRA pair"),
        ({**_named(**{Q: good}), CONV + ".lora_up.weight": torch.zeros(320, 2)}, r"not both lora_down.weight and lora_up.weight"),
        ({**_named(**{Q: good}), Q + ".diff": torch.zeros(320, 320)}, r"belong to no LoRA pair"),
        (_named(**{Q: dict(good, **{"lora_up.weight": torch.zeros(320, 3)})}), r"do not share a rank"),
    ]
    for state, pattern in cases:
        with pytest.raises(lora.LoraError, match=pattern):
            lora.apply_loras(model, enc, [(_named(**{Q: good}), 1.0), (state, 1.0)])       # the good adapter in front is not merged either
    # text-encoder entries without a text encoder
    with_te = _named(**{Q: good, TE: _pair(48, 32, 2)})
    with pytest.raises(lora.LoraError, match="text-encoder entries .* and no text encoder was given"):
        lora.apply_loras(model, None, [(with_te, 1.0)])
    (plan,) = lora.plan_loras(model, None, [(with_te, 1.0, 0.0)])                          # ... unless its text-encoder scale is 0
    assert [s[0] for s in plan.skipped] == [TE] and len(plan.merges) == 1
    with pytest.raises(lora.LoraError, match=r"TE_SCALE\]\] needs a path"):
        lora.parse_lora_spec(":0.5")
    with pytest.raises(lora.LoraError, match=r"give \(source, scale\)"):
        lora.plan_loras(model, None, [(good, 1.0, 1.0, 1.0)])
    # parameters on the host are not merged into (there is no CPU path) -- and that, too, is said before anything is touched
    with pytest.raises(lora.LoraError, match="merged into contiguous fp32 parameters on the HIP device"):
        lora.apply_loras(model, None, [(_named(**{Q: good}), 1.0)])
    after = model.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items())
    assert lora.STASH not in model.__dict__ and enc.dropped == 0 and model.__dict__.get("_engine") is None


def test_load_state_dict_forgets_the_stash():
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    model = UNetModel(**dict(syn.UNET_CFG_SMALL, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"])).eval()
    model.__dict__[lora.STASH] = {"time_embed.0.weight": torch.zeros(1280, 320)}
    model.__dict__[lora.APPLIED] = ("x",)
    model.load_state_dict(model.state_dict())
    assert lora.STASH not in model.__dict__ and lora.APPLIED not in model.__dict__
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    import transformers

    class Small(FrozenCLIPEmbedder):
        def __init__(self):
            nn.Module.__init__(self)
            cfg = transformers.CLIPTextConfig(vocab_size=64, hidden_size=32, intermediate_size=48, num_hidden_layers=1, num_attention_heads=2,
                                              max_position_embeddings=77, projection_dim=32, bos_token_id=1, eos_token_id=2, pad_token_id=2)
            self.tokenizer, self.transformer, self.device, self.max_length = None, transformers.CLIPTextModel(cfg), "cpu", 77
            self.freeze()

    enc = Small()
    enc.__dict__[lora.STASH] = {"k": torch.zeros(1)}
    enc.load_state_dict(enc.state_dict())
    assert lora.STASH not in enc.__dict__


def test_synthetic_adapter_and_the_tool(tmp_path):
    model = _unet(syn.UNET_CFG_SMALL)
    families = ("attn", "ff", "proj", "conv", "emb", "sample", "fuser", "time", "first_conv")
    adapter = syn.synthetic_lora(model, rank=3, families=families, dtype=torch.float16, seed=5)
    again = syn.synthetic_lora(model, rank=3, families=families, dtype=torch.float16, seed=5)
    assert adapter.keys() == again.keys() and all(torch.equal(adapter[k], again[k]) for k in adapter)
    (plan,) = lora.plan_loras(model, None, [(adapter, 1.0)])
    touched = {key[:-len(".weight")] for _, key, *_ in plan.merges}
    every = {p for p, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d)) and not p.startswith("position_net") and p != "input_blocks.0.0"
             and not p.startswith("out.")}
    assert touched == every and [s[0] for s in plan.skipped] == ["lora_unet_conv_in"]
    assert all(scale == 0.5 for *_, scale in plan.merges)                           # alpha = rank / 2
    names = {k.split(".", 1)[0] for k in adapter}
    assert "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q" in names          # kohya's name where there is one
    assert "lora_unet_input_blocks_1_1_transformer_blocks_0_fuser_attn_to_q" in names               # the module path elsewhere
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_synthetic_lora", os.path.join(ROOT, "tools", "make_synthetic_lora.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "a.safetensors"
    tool.main([str(out), "--small", "--rank", "2", "--families", "attn", "--dtype", "bf16"])
    state = lora.load_adapter(out)
    assert all(v.dtype == torch.bfloat16 for v in state.values()) and len(lora.plan_loras(model, None, [(str(out), 1.0)])[0].merges) == 7 * 8       # 7 transformers


# ---- the C ABI and the command line ---------------------------------------------------------------------------------------------------
def test_lora_entry_point_is_declared_exported_and_bound():
    from gligen_amd import _lib as table
    from gligen_amd.build import SOURCES, build_native
    build_native()
    lib = table.load()
    assert "lora.hip" in SOURCES
    header = open(os.path.join(ROOT, "include", "gligen_amd_lora.h")).read()
    declared = set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", header))
    assert declared == set(table.LORA_SYMBOLS) == {"gl_op_lora_merge"} and not declared & set(table.SYMBOLS)
    raw = C.CDLL(str(table.LIB_PATH))
    assert hasattr(raw, "gl_op_lora_merge")
    assert lib.gl_op_lora_merge.argtypes == table.LORA_SYMBOLS["gl_op_lora_merge"][1] and lib.gl_op_lora_merge.restype == C.c_int
    assert table.LORA_SYMBOLS["gl_op_lora_merge"][1][7] is C.c_float               # scale travels as a float
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c",
                    os.path.join(ROOT, "include", "gligen_amd_lora.h")], check=True)
    assert lib.gl_op_lora_merge(None, None, None, None, 1, 1, 1, 1.0, None) != 0 and b"null context" in lib.gl_last_error()


def test_lora_kernel_uses_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "lora.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--offload-device-only", "-S",
                        os.path.join(ROOT, "gligen_amd", "csrc", "lora.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    kernels = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])[1:]
    assert len(kernels) == 1 and "lora_merge_kernel" in kernels[0]
    val = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", kernels[0]).group(1))
    assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0
    assert val("max_flat_workgroup_size") == 256 and val("group_segment_fixed_size") == 4 * (32 * 33 + 32 * 128)
    body = asm[asm.index("lora_merge_kernel"):]
    assert len(re.findall(r"\bv_(pk_)?fma(c|ak|mk)?_f32\b", body)) >= 16 and not re.search(r"\bv_mfma", body)      # fp32 FMAs, no matrix core


def test_command_line_and_run_carry_the_option(monkeypatch):
    import argparse
    import gligen_inference as gi
    seen = {}

    def parse(self, argv=None):
        seen["args"] = argparse.ArgumentParser.parse_known_args(self, argv)[0]
        raise SystemExit(0)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    with pytest.raises(SystemExit):
        gi.main(["--synthetic", "text", "--lora", "a.safetensors:0.8", "--lora", "b.pt:1:0"])
    assert seen["args"].loras == ["a.safetensors:0.8", "b.pt:1:0"]
    with pytest.raises(SystemExit):
        gi.main([])
    assert seen["args"].loras is None
    import inspect
    assert "loras" in inspect.signature(gi.load_ckpt).parameters and inspect.signature(gi.load_ckpt).parameters["loras"].default is None
    calls = []
    monkeypatch.setattr(lora, "apply_loras", lambda m, t, a: calls.append(a) or dict(adapters=[], skipped=[], seconds=0.0))
    model = _unet(syn.UNET_CFG_SMALL)
    assert gi.use_loras(model, None, None) is None and gi.use_loras(model, None, []) is None and not calls
    assert gi.use_loras(model, None, ["x.safetensors:0.5"]) is not None and calls == [[("x.safetensors", 0.5, 0.5)]]
    assert gi.use_loras(model, None, ["x.safetensors:0.5"]) is None and len(calls) == 1             # once per model load, not per prompt
    assert gi.use_loras(model, None, ["x.safetensors:0.6"]) is not None and len(calls) == 2         # another list is applied
