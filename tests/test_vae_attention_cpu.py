"""Any image size, without a GPU: the C ABI of include/gligen_amd_vae.h, the ISA of vae_attn_flash_kernel, the size validation of
generate() / run(), rectangular inpainting masks and crops, and the CPU oracle held to the REFERENCE's own output at non-square sizes
(tests/golden/vae_small_24x40.npz, unet_small_text_16x24.npz, made by tools/make_golden_sizes.py)."""
import ctypes
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from helpers import GINPUT, ROOT, golden_shapes, grounding_kwargs, load_golden, mse, oracle_cfg
from gligen_amd import synthetic as syn
from oracle import gligen_oracle as orc

_spec = importlib.util.spec_from_file_location("make_golden_sizes", os.path.join(ROOT, "tools", "make_golden_sizes.py"))
mgs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgs)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_vae_header_table_and_exports_agree():
    from gligen_amd import _lib
    from gligen_amd.build import SOURCES, build_native
    build_native()
    assert "vae_attention.hip" in SOURCES
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gligen_amd_vae.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.VAE_SYMBOLS) == {"gl_vae_set_attention", "gl_op_vae_attention"}
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SYMBOLS") and n != "VAE_SYMBOLS"]
    assert len(others) >= 12 and not any(declared & set(t) for t in others)
    # the declared parameter lists, type by type
    ctype = {"gl_ctx*": ctypes.c_void_p, "const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "gl_stream": ctypes.c_void_p, "int": ctypes.c_int}
    for name in declared:
        params = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", code).group(1).split(",")
        types = [ctype[re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*")] for p in params]
        res, args = _lib.VAE_SYMBOLS[name]
        assert res is ctypes.c_int and args == types, name
    enum = dict((n, int(v)) for n, v in re.findall(r"GL_VAE_ATTN_([A-Z]+) = (\d)", code))
    assert enum == dict(AUTO=0, MATRIX=1, FLASH=2) and _lib.VAE_ATTN_MODES == {"auto": 0, "matrix": 1, "flash": 2}
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    assert all(hasattr(raw, n) for n in declared)
    lib = _lib.load()
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.VAE_SYMBOLS[name][1]
    assert lib.gl_vae_set_attention(None, 0) == 2 and b"null context" in lib.gl_last_error()
    assert lib.gl_op_vae_attention(None, None, None, None, 1, 64, 256, 0, None, None) == 2


# ---------------------------------------------------------------------------------------------------------------- ISA
@pytest.fixture(scope="module")
def vae_attention_asm(tmp_path_factory):
    from gligen_amd.build import EXTRA_FLAGS
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path_factory.mktemp("isa") / "vae_attention.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *EXTRA_FLAGS.get("vae_attention.hip", []), "-I", os.path.join(ROOT, "include"),
                        "--offload-device-only", "-S", os.path.join(ROOT, "gligen_amd", "csrc", "vae_attention.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


@pytest.mark.parametrize("C", [256, 512])
def test_vae_attn_flash_kernel_isa(C, vae_attention_asm):
    """DESIGN.md section 3, row "VAE attn": four waves split the head dimension, two 32-query tiles per workgroup; per 64-key tile each
    wave issues 2 x 2 x C / 64 MFMAs for its share of S^T and 2 x C / 128 x 4 for its rows of O^T (64 at C = 512, 32 at C = 256), all
    v_mfma_f32_32x32x16_bf16; the loop is not unrolled, so the body holds exactly that many. One workgroup per CU: 64 KB of LDS, at most
    the 512 registers (VGPR + AGPR) of one wave per SIMD, no scratch, no spills; a barrier in front of the LDS reads and one behind."""
    asm = vae_attention_asm
    name = re.search(r"^(_ZN2gl21vae_attn_flash_kernelILi%d[^:\s]*):" % C, asm, re.M).group(1)
    a = asm.index(name + ":")
    body = asm[a:asm.index(".Lfunc_end", a)]
    nq = int(re.search(r"kVaeAttnQueryTiles\s*=\s*(\d+)", open(os.path.join(ROOT, "gligen_amd", "csrc", "vae_attention.hip")).read()).group(1))
    per_tile = nq * (2 * (C // 64) + (C // 128) * 4)
    assert nq == 2 and per_tile == {256: 32, 512: 64}[C]
    assert body.count("v_mfma_f32_32x32x16_bf16") == per_tile == len(re.findall(r"\bv_mfma_", body))
    assert "scratch_" not in body and body.count("s_barrier") == 2
    assert body.count("v_exp_f32") >= nq * (32 + 1)
    kernels = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])
    entry = next(e for e in kernels[1:] if re.search(r"\.name:\s*" + re.escape(name) + r"\s", e))
    val = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", entry).group(1))
    agpr = int(re.match(r"\s*(\d+)", entry).group(1))
    assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0
    assert val("group_segment_fixed_size") == 65536 <= 160 * 1024
    assert agpr <= val("vgpr_count") <= 512 and val("max_flat_workgroup_size") == 256       # .vgpr_count: the unified VGPR + AGPR total on gfx950
    for kern in kernels[1:]:       # the transpose kernel beside it
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", kern).group(1)) == 0
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", kern).group(1)) == 0


# ---------------------------------------------------------------------------------------------------------------- sizes
class _FakeSampler:
    """Stands where PLMSSampler stands: records the latent shape it is asked for."""
    seen = []

    def __init__(self, diffusion, model, **kw):
        pass

    def sample(self, S, shape, input, **kw):
        _FakeSampler.seen.append((tuple(shape), None if input["x"] is None else tuple(input["x"].shape)))
        return torch.zeros(shape)


class _FakeVae:
    ddconfig = dict(ch_mult=[1, 2, 4, 4])

    def decode(self, z):
        return torch.zeros(z.shape[0], 3, 8 * z.shape[2], 8 * z.shape[3])


class _FakeUNet:
    in_channels, image_size, channel_mult, downsample_net = 4, 64, [1, 2, 4, 4], None

    class _Tok:
        def prepare(self, batch):
            return {}
    grounding_tokenizer_input = _Tok()


def _generate(gi, **kw):
    _FakeSampler.seen.clear()
    ctx = torch.zeros(2, 77, 768)
    model = kw.pop("model", _FakeUNet())
    img = gi.generate(model, _FakeVae(), None, {}, ctx, ctx, steps=2, **kw)
    return img, _FakeSampler.seen[-1]


def test_generate_validates_height_and_width(monkeypatch):
    import gligen_inference as gi
    monkeypatch.setattr(gi, "PLMSSampler", _FakeSampler)
    img, (shape, _) = _generate(gi)
    assert shape == (2, 4, 64, 64) and img.shape == (2, 3, 512, 512)                    # height=None: exactly today's shapes
    img, (shape, _) = _generate(gi, height=768, width=512)
    assert shape == (2, 4, 96, 64) and img.shape == (2, 3, 768, 512)
    assert _generate(gi, width=1024)[1][0] == (2, 4, 64, 128)
    for bad in (dict(height=520), dict(width=96), dict(height=0), dict(height=512, width=-64)):
        with pytest.raises(ValueError, match="multiple of 64"):
            _generate(gi, **bad)
    with pytest.raises(ValueError, match=r"starting_noise.*\(2, 4, 64, 64\).*\(2, 4, 96, 64\)"):
        _generate(gi, height=768, starting_noise=torch.zeros(2, 4, 64, 64))
    with pytest.raises(ValueError, match="starting_noise"):
        _generate(gi, width=512, starting_noise=torch.zeros(2, 4, 96, 64))
    # without height / width a starting_noise keeps deciding the latent's size, as it always did (the small-latent tests rely on it)
    assert _generate(gi, starting_noise=torch.zeros(2, 4, 16, 16))[1] == ((2, 4, 64, 64), (2, 4, 16, 16))
    assert _generate(gi, height=768, starting_noise=torch.zeros(2, 4, 96, 64))[1] == ((2, 4, 96, 64), (2, 4, 96, 64))
    # the same checks in front of the lanes, before anything is split or forked
    ctx = torch.zeros(2, 77, 768)
    with pytest.raises(ValueError, match="multiple of 64"):
        gi.generate_lanes(_FakeUNet(), _FakeVae(), None, {}, ctx, ctx, lanes=2, height=100)
    with pytest.raises(ValueError, match="starting_noise"):
        gi.generate_stream(_FakeUNet(), _FakeVae(), None, {}, ctx, ctx, [torch.zeros(2, 4, 64, 64)], width=768)

    class Spatial(_FakeUNet):
        class downsample_net:
            resize_input = 256
    with pytest.raises(ValueError, match="resize_input = 256"):
        _generate(gi, model=Spatial(), height=768)
    assert _generate(gi, model=Spatial())[1][0] == (2, 4, 64, 64) and _generate(gi, model=Spatial(), height=512, width=512)[1][0] == (2, 4, 64, 64)
    small = type("V", (), dict(ddconfig=dict(ch_mult=[1, 2])))()
    m2 = type("M", (_FakeUNet,), dict(channel_mult=[1, 2], image_size=16))()
    assert gi.latent_hw(m2, small, 32, 48) == (16, 24) and gi.latent_hw(m2, small) == (16, 16)
    with pytest.raises(ValueError, match="multiple of 4 "):
        gi.latent_hw(m2, small, 34, 48)


def test_run_takes_height_and_width_from_its_config(monkeypatch, tmp_path):
    import gligen_inference as gi
    import gligen_amd.dist as gdist
    seen = []

    def fake_generate(model, autoencoder, diffusion, batch, context, uc, **kw):
        seen.append(dict(noise=None if kw["starting_noise"] is None else tuple(kw["starting_noise"].shape), height=kw["height"], width=kw["width"],
                         mask=None if kw.get("inpainting_mask") is None else kw["inpainting_mask"].clone()))
        return torch.zeros(context.shape[0], 3, 8, 8)

    monkeypatch.setattr(gi, "generate", fake_generate)
    monkeypatch.setattr(gi, "device", "cpu")
    monkeypatch.setattr(gi, "save_images", lambda *a, **k: None)
    monkeypatch.setattr(gdist, "barrier", lambda: None)
    monkeypatch.setenv("WORLD_SIZE", "1")
    meta = dict(ckpt="synthetic_text", prompt="p", save_folder_name="x", locations=[[0.1, 0.2, 0.5, 0.9]], text_embeddings=[torch.ones(768)],
                context=syn.make_context(3, seed=0), uc=syn.make_context(3, seed=1))
    cfg = dict(grounding_tokenizer_input=dict(target=GINPUT["text"]), inpaint_mode=True)
    args = dict(batch_size=3, guidance_scale=7.5, negative_prompt=None, no_plms=False, folder=str(tmp_path), seed=3)
    models = (_FakeUNet(), _FakeVae(), None, None, cfg)
    gi.run(meta, dict(args), models=models)
    assert seen[-1] == dict(noise=(3, 4, 64, 64), height=None, width=None, mask=None)
    gi.run(meta, dict(args, height=768, width=512), models=models)
    assert seen[-1]["noise"] == (3, 4, 96, 64) and (seen[-1]["height"], seen[-1]["width"]) == (768, 512)
    full = torch.randn((3, 4, 96, 64), generator=torch.Generator().manual_seed(3))
    for rank in range(2):                                   # the seeded x_T of a sharded run has the asked size, and so has an empty shard
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("RANK", str(rank))
        gi.run(meta, dict(args, height=768, width=512), models=models)
    assert seen[-1]["noise"] == (1, 4, 96, 64) and seen[-2]["noise"] == (2, 4, 96, 64) and full.shape[0] == 3
    monkeypatch.setenv("WORLD_SIZE", "8")
    monkeypatch.setenv("RANK", "7")
    assert gi.run(meta, dict(args, height=768, width=512), models=models).shape == (0, 3, 768, 512)
    assert gi.run(meta, dict(args), models=models).shape == (0, 3, 512, 512)
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    # inpainting follows the size: a rectangular mask from the boxes
    gi.run(dict(meta, input_image="unused", z0=torch.zeros(1, 4, 96, 64)), dict(args, height=768, width=512), models=models)
    m = seen[-1]["mask"]
    assert m.shape == (3, 1, 96, 64) and float(m[0, 0, int(0.2 * 96):int(0.9 * 96), int(0.1 * 64):int(0.5 * 64)].sum()) == 0 and float(m.sum()) > 0
    with pytest.raises(ValueError, match="native_inputs"):
        gi.run(meta, dict(args, height=768, native_inputs=True), models=models)
    with pytest.raises(ValueError, match="multiple of 64"):
        gi.run(meta, dict(args, width=500), models=models)
    # the two-lane split draws x_T at the asked size before it cuts the batch
    lanes_seen = []
    monkeypatch.setattr(gi, "SPLIT_BATCH_AT", 2)
    monkeypatch.setattr(gi, "generate_lanes", lambda *a, **k: lanes_seen.append((k["lanes"], tuple(k["starting_noise"].shape), k["height"], k["width"])) or torch.zeros(3, 3, 8, 8))
    gi.run(meta, dict(args, seed=None, height=576, width=640), models=models)
    assert lanes_seen == [(2, (3, 4, 72, 80), 576, 640)]


def test_command_line_has_height_and_width(monkeypatch):
    import gligen_inference as gi
    got = {}

    def fake_run(meta, config, starting_noise=None, models=None):
        got.update(height=config.height, width=config.width, z0=None if "z0" not in meta else tuple(meta["z0"].shape))

    class Vae(_FakeVae):
        def encode(self, x):
            return torch.zeros(x.shape[0], 4, x.shape[2] // 8, x.shape[3] // 8)
    monkeypatch.setattr(gi, "run", fake_run)
    monkeypatch.setattr(gi, "device", "cpu")
    monkeypatch.setattr(gi, "load_synthetic", lambda *a, **k: (_FakeUNet(), Vae(), None, {}))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    gi.main(["--synthetic", "text", "--height", "768", "--width", "640", "--inpaint"])
    assert got == dict(height=768, width=640, z0=(1, 4, 96, 80))
    gi.main(["--synthetic", "text"])
    assert got == dict(height=None, width=None, z0=None)


# ---------------------------------------------------------------------------------------------------------------- masks, crops
MASK64_SHA256 = "8685c8c4e814dc09513a85cf880ba9d45f01d34d11111e12c62950fb829fcfe5"      # of the parent commit's output (float32 [3, 1, 64, 64], sum 8331)


def test_draw_masks_from_boxes_keeps_its_square_form_and_takes_h_w():
    import gligen_inference as gi
    boxes, _ = syn.make_boxes(3, 8, seed=0)
    sq = gi.draw_masks_from_boxes(boxes, 64)
    assert sq.shape == (3, 1, 64, 64) and sq.dtype == torch.float32 and float(sq.sum()) == 8331.0
    assert hashlib.sha256(sq.numpy().tobytes()).hexdigest() == MASK64_SHA256
    assert torch.equal(sq, orc.draw_masks_from_boxes(boxes, 64)) and torch.equal(gi.draw_masks_from_boxes(boxes, (64, 64)), sq)
    for h, w in ((96, 64), (24, 16), (16, 24), (72, 80)):
        want = []
        for per_image in boxes:                     # inpaint_mask_func.py:16-41 with one size per axis
            m = torch.ones(h, w)
            for bx in per_image:
                x0, y0, x1, y1 = int(bx[0] * w), int(bx[1] * h), int(bx[2] * w), int(bx[3] * h)
                m[y0:y1, x0:x1] = 0
            want.append(m)
        got = gi.draw_masks_from_boxes(boxes, (h, w))
        assert got.shape == (3, 1, h, w) and torch.equal(got, torch.stack(want).unsqueeze(1)) and 0 < float(got.sum()) < got.numel()


def test_crop_and_resize_centre_crops_to_the_target_aspect(tmp_path, monkeypatch):
    import gligen_inference as gi
    from PIL import Image
    rng = np.random.RandomState(0)
    im = Image.fromarray((rng.rand(60, 100, 3) * 255).astype(np.uint8))
    assert np.array_equal(np.asarray(gi.crop_and_resize(im)), np.asarray(im.crop((20, 0, 80, 60)).resize((512, 512))))     # the square default
    out = gi.crop_and_resize(im, (64, 128))          # (width, height): taller than the source -> full height, middle 30 columns
    assert out.size == (64, 128) and np.array_equal(np.asarray(out), np.asarray(im.crop((35, 0, 65, 60)).resize((64, 128))))
    out = gi.crop_and_resize(im, (128, 64))          # wider than the source (2 : 1 against 5 : 3): full width, middle 50 rows
    assert np.array_equal(np.asarray(out), np.asarray(im.crop((0, 5, 100, 55)).resize((128, 64))))
    im.save(tmp_path / "a.png")
    monkeypatch.setattr(gi, "device", "cpu")
    t = gi.load_inpaint_image(str(tmp_path / "a.png"), size=(64, 128))
    assert t.shape == (1, 3, 128, 64) and float(t.min()) >= -1 and float(t.max()) <= 1
    assert torch.equal(t[0], gi._pil_to_unit_tensor(gi.crop_and_resize(im, (64, 128))))
    assert gi.load_inpaint_image(str(tmp_path / "a.png")).shape == (1, 3, 512, 512)
    with pytest.raises(ValueError, match="native_inputs"):
        gi.load_inpaint_image(str(tmp_path / "a.png"), native=True, size=(64, 128))


# ---------------------------------------------------------------------------------------------------------------- oracle vs reference
def test_oracle_vae_at_24x40_is_the_reference():
    g = load_golden("vae_small_24x40")
    dd = g["meta"]["ddconfig"]
    assert g["meta"]["latent"] == [24, 40] and g["img"].shape == (2, 3, 48, 80) and g["z"].shape == (2, 4, 24, 40)
    sd = syn.seeded_state_dict(golden_shapes("vae_small"), g["meta"]["weight_seed"])
    cfg = dict(ch_mult=dd["ch_mult"], num_res_blocks=dd["num_res_blocks"], scale_factor=0.18215)
    z, x = mgs.vae_inputs(syn, torch)
    with torch.no_grad():
        assert mse(orc.vae_decode(sd, cfg, z), g["img"]) < 1e-8                                                  # tests/test_oracle_golden.py: test_vae_decode
        zenc = orc.vae_encode(sd, cfg, x, torch.from_numpy(g["noise"]))
    assert mse(zenc, g["z"]) / float(g["z"].var()) < 1e-9                                                        # ... test_vae_encode
    assert g["img"].std() > 0.1 and g["z"].std() > 0.05
    for name in ("vae_small_24x40", "unet_small_text_16x24"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20


def test_oracle_unet_at_16x24_is_the_reference():
    g = load_golden("unet_small_text_16x24")
    meta = g["meta"]
    assert meta["latent"] == [16, 24] and g["eps"].shape == (2, 4, 16, 24)
    sd = syn.seeded_state_dict(golden_shapes("unet_small_text"), meta["weight_seed"])
    batch, x, ctx, t = mgs.unet_inputs(syn, torch)
    gk = grounding_kwargs("text", batch)
    cfg = oracle_cfg(meta["cfg"], "text")
    inp = dict(x=x, timesteps=t, context=ctx, grounding_input=gk, inpainting_extra_input=None)
    with torch.no_grad():
        assert mse(orc.unet_forward(sd, cfg, inp), g["eps"]) < 1e-9                                              # FP32_TOL of tests/test_oracle_golden.py
        assert mse(orc.unet_forward(sd, cfg, dict(inp, grounding_input=orc.null_grounding("text", gk))), g["eps_null"]) < 1e-9
    assert g["eps"].std() > 0.1 and mse(g["eps"], g["eps_null"]) > 1e-5
