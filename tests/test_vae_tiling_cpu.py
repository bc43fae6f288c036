"""Tiled autoencoder passes, no GPU: the tile plan's properties over an exhaustive small range, the weight tables, every refusal by
name, the config keys and command-line flags, and the C entry points of include/gligen_amd_tiling.h."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import vae_tiling_ref as ref
from helpers import GINPUT, ROOT
from gligen_amd import synthetic as syn
from gligen_amd import vae_tiling as vt

_CASES = [(T, ov, L) for T in (8, 16, 64) for ov in range(1, T // 2 + 1) for L in range(1, 4 * T + 4)]


def test_plan_properties():
    assert (64, 16, 113) in _CASES
    three = 0
    for T, ov, L in _CASES:
        o = vt.tile_plan(L, T, ov)
        assert o == ref.plan(L, T, ov), (L, T, ov)
        assert o[0] == 0
        if L <= T:
            assert o == [0]
            continue
        assert len(o) == -(-(L - ov) // (T - ov)) and o[-1] + T == L
        assert all(0 <= x and x + T <= L for x in o)
        assert all(b > a for a, b in zip(o, o[1:])), "origins strictly increasing"
        assert all(a + T - b >= ov for a, b in zip(o, o[1:])), "neighbours overlap by at least `overlap`"
        cover = np.zeros(L, dtype=int)
        for x in o:
            cover[x:x + T] += 1
        assert cover.min() >= 1
        three += int(cover.max() >= 3)
    assert vt.tile_plan(113, 64, 16) in ([0, 24, 49], [0, 25, 49])
    assert three > 0, "the range must contain plans where three tiles cover one coordinate"


@pytest.mark.parametrize("scale", [1, 2, 8])
def test_weight_tables(scale):
    cases = [c for c in _CASES if c[0] in (8, 16)] + [(64, ov, L) for ov in (1, 16, 32) for L in (64, 65, 113, 128, 200, 259)]
    if scale == 8:
        cases = cases[::7]
    for T, ov, L in cases:
        o = vt.tile_plan(L, T, ov)
        w = vt.weight_tables(L, T, ov, o, scale)
        w64 = ref.tables64(L, T, ov, o, scale)
        Te = min(T, L) * scale
        assert w.dtype == np.float32 and w.shape == (len(o), Te)
        assert np.array_equal(w, w64.astype(np.float32)), (L, T, ov)
        assert (w >= 0).all() and (w <= 1).all()
        total, cover = np.zeros(L * scale), np.zeros(L * scale, dtype=int)
        for t, x in enumerate(o):
            total[x * scale:x * scale + Te] += w[t].astype(np.float64)
            cover[x * scale:x * scale + Te] += 1
        assert np.abs(total - 1).max() <= 2.0 ** -22
        for t, x in enumerate(o):
            alone = cover[x * scale:x * scale + Te] == 1
            assert (w[t][alone] == 1).all(), "the weight is exactly 1 where one tile covers"
        # no ramp at the image borders: the first tile starts, and the last ends, at full weight among what covers the border
        assert w[0][0] == 1 and w[-1][-1] == 1
        if len(o) > 1:
            assert w[1][0] < 1 and w[1][0] > 0 and w[0][-1] < 1


def test_refusals_by_name():
    for tile in (0, 4, 12, 60, -8, (64, 20), 7.5, (8, 8, 8)):
        with pytest.raises(ValueError, match="vae_tile"):
            vt.check_tiling(tile, 1)
    for tile, ov in ((64, 0), (64, 33), (16, 9), ((64, 16), (16, 9)), (64, -1), (64, 1.5)):
        with pytest.raises(ValueError, match="vae_tile_overlap"):
            vt.check_tiling(tile, ov)
    assert vt.check_tiling() == ((64, 64), (16, 16)) and vt.check_tiling((16, 24), (8, 1)) == ((16, 24), (8, 1))
    for mode in ("yes", "ON", 1, True):
        with pytest.raises(ValueError, match="vae_tiling"):
            vt.check_mode(mode)
    assert [vt.check_mode(m) for m in (None, "off", "on", "auto")] == ["off", "off", "on", "auto"]
    with pytest.raises(ValueError, match="overlap"):
        vt.tile_plan(100, 16, 9)
    # the engine's methods refuse before anything reaches the library (no context is needed to get there)
    from gligen_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng._ctx = None
    eng.device, eng.vae_cfg = "cpu", dict(out_ch=3, z_channels=4, n_up=1)
    eng._vae_tiling, eng._vae_tiled_shapes, eng._vae_plans = ("off", 64, 16), set(), {}
    img, noise, z = torch.zeros(1, 3, 16, 16), torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError, match="return_moments"):
        eng.vae_encode(img, noise, return_moments=True)
    with pytest.raises(ValueError, match="return_moments"):
        eng.vae_encode(img, noise, tiling="off", return_moments=True)
    with pytest.raises(ValueError, match="vae_tile:"):
        eng.vae_decode(z, tiling="on", tile=12)
    with pytest.raises(ValueError, match="vae_tile_overlap"):
        eng.vae_encode(img, noise, tiling="auto", tile=8, overlap=5)
    with pytest.raises(ValueError, match="vae_tiling"):
        eng.vae_decode(z, tiling="maybe")
    with pytest.raises(ValueError, match="vae_tiling"):
        eng.set_vae_tiling("maybe")
    with pytest.raises(ValueError, match="vae_tile_overlap"):
        eng.set_vae_tiling("on", 16, 16)
    eng.set_vae_tiling("auto", (16, 32), 8)
    assert eng._vae_tiling == ("auto", (16, 32), 8)


class _FakeVae:
    ddconfig = dict(ch_mult=[1, 2, 4, 4])

    def __init__(self):
        self.calls = []

    def decode(self, z, **kw):
        self.calls.append(("decode", kw))
        return torch.zeros(z.shape[0], 3, 8 * z.shape[2], 8 * z.shape[3])

    def encode(self, x, **kw):
        self.calls.append(("encode", kw))
        return torch.zeros(x.shape[0], 4, x.shape[2] // 8, x.shape[3] // 8)


class _PlainVae(_FakeVae):                     # an autoencoder that knows nothing of tiling: "off" must not hand it a keyword
    def decode(self, z):
        return _FakeVae.decode(self, z)


class _FakeUNet:
    in_channels, image_size, channel_mult, downsample_net = 4, 64, [1, 2, 4, 4], None

    class _Tok:
        def prepare(self, batch):
            return {}
    grounding_tokenizer_input = _Tok()


class _FakeSampler:
    def __init__(self, *a, **k):
        pass

    def sample(self, S, shape, input, **kw):
        return torch.zeros(shape)


def test_generate_hands_the_setting_to_every_decode_and_encode(monkeypatch):
    import gligen_inference as gi
    monkeypatch.setattr(gi, "PLMSSampler", _FakeSampler)
    ctx = torch.zeros(2, 77, 768)
    ae = _FakeVae()
    want = dict(tiling="on", tile=32, overlap=8)
    gi.generate(_FakeUNet(), ae, None, {}, ctx, ctx, steps=2, vae_tiling="on", vae_tile=32, vae_tile_overlap=8,
                init_image=torch.zeros(1, 3, 512, 512), strength=0.5)
    assert ae.calls == [("encode", want), ("decode", want)]
    plain = _PlainVae()
    gi.generate(_FakeUNet(), plain, None, {}, ctx, ctx, steps=2)
    gi.generate(_FakeUNet(), plain, None, {}, ctx, ctx, steps=2, vae_tiling="off", vae_tile=32, vae_tile_overlap=8)
    assert plain.calls == [("decode", {}), ("decode", {})]
    for bad, name in ((dict(vae_tiling="tiles"), "vae_tiling"), (dict(vae_tiling="on", vae_tile=20), "vae_tile:"),
                      (dict(vae_tiling="auto", vae_tile_overlap=40), "vae_tile_overlap")):
        with pytest.raises(ValueError, match=name):
            gi.generate(_FakeUNet(), _FakeVae(), None, {}, ctx, ctx, steps=2, **bad)
    assert gi.vae_tiling_kwargs() == {} and gi.vae_tiling_kwargs(None) == {}
    assert gi.vae_tiling_kwargs("auto", (64, 32), 16) == dict(tiling="auto", tile=(64, 32), overlap=16)


def test_config_keys_reach_generate_and_the_command_line_has_the_flags(monkeypatch, tmp_path):
    import argparse
    import gligen_inference as gi
    import gligen_amd.dist as gdist
    seen = []
    monkeypatch.setattr(gi, "generate", lambda model, ae, diffusion, batch, context, uc, **kw: seen.append(kw) or torch.zeros(context.shape[0], 3, 8, 8))
    monkeypatch.setattr(gi, "device", "cpu")
    monkeypatch.setattr(gi, "save_images", lambda *a, **k: None)
    monkeypatch.setattr(gdist, "barrier", lambda: None)
    monkeypatch.setenv("WORLD_SIZE", "1")
    meta = dict(ckpt="synthetic_text", prompt="p", save_folder_name="x", locations=[[0.1, 0.2, 0.5, 0.9]], text_embeddings=[torch.ones(768)],
                context=syn.make_context(3, seed=0), uc=syn.make_context(3, seed=1))
    cfg = dict(grounding_tokenizer_input=dict(target=GINPUT["text"]))
    args = dict(batch_size=3, guidance_scale=7.5, negative_prompt=None, no_plms=False, folder=str(tmp_path), seed=3)
    models = (_FakeUNet(), _FakeVae(), None, None, cfg)
    gi.run(meta, dict(args), models=models)
    assert not {"vae_tiling", "vae_tile", "vae_tile_overlap"} & set(seen[-1]), "a config without the keys runs what it always ran"
    gi.run(meta, dict(args, vae_tiling="auto", vae_tile=32, vae_tile_overlap=4), models=models)
    assert (seen[-1]["vae_tiling"], seen[-1]["vae_tile"], seen[-1]["vae_tile_overlap"]) == ("auto", 32, 4)
    gi.run(meta, dict(args, vae_tiling="on"), models=models)
    assert seen[-1]["vae_tiling"] == "on" and "vae_tile" not in seen[-1]
    n = len(seen)
    for bad, name in ((dict(vae_tiling="always"), "vae_tiling"), (dict(vae_tiling="on", vae_tile=100), "vae_tile:"),
                      (dict(vae_tiling="on", vae_tile=16, vae_tile_overlap=9), "vae_tile_overlap")):
        with pytest.raises(ValueError, match=name):
            gi.run(meta, dict(args, **bad), models=models)
    assert len(seen) == n, "a refused setting must not reach the sampler"
    # the command line: the three flags, and a value outside off | on | auto is refused by the parser
    flags = {}
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args",
                        lambda self, argv=None: flags.update({a.dest: a for a in self._actions}) or (_ for _ in ()).throw(SystemExit(0)))
    with pytest.raises(SystemExit):
        gi.main([])
    assert {"vae_tiling", "vae_tile", "vae_tile_overlap"} <= set(flags)
    assert list(flags["vae_tiling"].choices) == ["off", "on", "auto"] and flags["vae_tiling"].default == "off"
    assert (flags["vae_tile"].default, flags["vae_tile_overlap"].default) == (64, 16)
    monkeypatch.undo()
    p = argparse.ArgumentParser()
    p.add_argument("--vae_tiling", choices=flags["vae_tiling"].choices)
    with pytest.raises(SystemExit):
        p.parse_args(["--vae_tiling", "maybe"])


def test_autoencoder_passes_the_setting_through():
    from ldm.models.autoencoder import AutoencoderKL
    ae = AutoencoderKL(ddconfig=syn.VAE_DDCONFIG_SMALL, embed_dim=4, scale_factor=0.18215).eval()
    calls = []
    fake = types.SimpleNamespace(vae_decode=lambda z, **kw: calls.append(kw) or torch.zeros(1, 3, 4, 4),
                                 vae_encode=lambda x, noise, **kw: calls.append(kw) or torch.zeros(1, 4, 2, 2), close=lambda: None)
    ae.__dict__["_engine"] = fake
    ae.decode(torch.zeros(1, 4, 2, 2))
    ae.decode(torch.zeros(1, 4, 2, 2), tiling="on", tile=16, overlap=4)
    ae.encode(torch.zeros(1, 3, 4, 4), tiling="auto")
    assert calls == [dict(tiling=None, tile=None, overlap=None), dict(tiling="on", tile=16, overlap=4), dict(tiling="auto", tile=None, overlap=None)]
    ae.__dict__["_engine"] = None


def test_tiling_entry_points_are_declared_exported_and_bound():
    from gligen_amd import _lib as table
    from gligen_amd.build import build_native
    build_native()
    header = open(os.path.join(ROOT, "include", "gligen_amd_tiling.h")).read()
    declared = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", header))
    names = {"gl_vae_decode_tiled", "gl_vae_encode_tiled", "gl_op_tile_gather", "gl_op_tile_blend"}
    assert declared == set(table.TILING_SYMBOLS) == names and not declared & set(table.SYMBOLS)
    lib = ctypes.CDLL(str(table.LIB_PATH))
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/gligen_amd_tiling.h but not exported"
    bound = table.load()
    for name in names:
        assert getattr(bound, name).argtypes == table.TILING_SYMBOLS[name][1]
    fields = re.search(r"typedef struct gl_tile_plan \{(.*?)\} gl_tile_plan;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    c_names = re.findall(r"([a-z_]+)\s*[,;]", fields)            # the declarators, in order
    assert c_names == [f[0] for f in table.TilePlan._fields_], c_names
    assert ctypes.sizeof(table.TilePlan) == 4 * 7 + 4 + 8 * 5      # 7 ints, padding to the pointers' alignment, 5 pointers
