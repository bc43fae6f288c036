"""Tiled autoencoder passes on a real MI355X: tile_gather_kernel and tile_blend_kernel by themselves (the blend against float64 with a
derived bound, bit for bit under any split into passes), the tiled decode and encode against the hand composition from untiled per-tile
calls, the single-tile case, the arena that the untiled pass exhausts and the tiled one does not ("auto" included), and generate()."""
import json
import math

import numpy as np
import pytest
import torch

import vae_tiling_ref as ref
from helpers import build_product_vae, mse
from gligen_amd import GligenAmdError
from gligen_amd import runtime as rt
from gligen_amd import synthetic as syn
from gligen_amd import vae_tiling as vt

pytestmark = pytest.mark.gpu

GUARD = 4096
REPORT = {}


@pytest.fixture(autouse=True)
def _report(record_property):
    before = set(REPORT)
    yield
    for key in sorted(set(REPORT) - before):
        record_property(key, json.dumps(REPORT[key], sort_keys=True))
        print(f"[vae_tiling] {key}: {json.dumps(REPORT[key], sort_keys=True)}")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _guarded(dev, shape):
    """A NaN-filled buffer with the output in its middle: (buffer, the output view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev, dtype=torch.float32)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _untouched(buf):
    torch.cuda.synchronize()
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


# ---- 1: the gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W,TH,TW", [(4, 24, 40, 16, 16), (3, 48, 80, 32, 32), (3, 21, 37, 8, 12), (4, 16, 24, 16, 24)])
def test_gather_is_an_exact_copy(engine, C, H, W, TH, TW):
    """Windows touching every border and corner, aligned and unaligned x origins, both images of the batch, a repeated window."""
    dev = engine.device
    B = 2
    src = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C * H + W)).to(dev)
    ys, xs = sorted({0, (H - TH) // 2, H - TH}), sorted({0, min(4, W - TW), (W - TW) // 2, max(W - TW - 1, 0), W - TW})
    windows = [(b, y, x) for b in range(B) for y in ys for x in xs] + [(1, 0, 0)]
    buf, out = _guarded(dev, (len(windows), C, TH, TW))
    got = engine.tile_gather(src, windows, TH, TW, out=out)
    assert _untouched(buf), "the kernel wrote outside its output"
    want = torch.stack([src[b, :, y:y + TH, x:x + TW] for b, y, x in windows])
    assert torch.equal(got, want)
    assert torch.equal(engine.tile_gather(src, windows, TH, TW), want)


# ---- 2: the blend alone -------------------------------------------------------------------------------------------------------------------
TH, TW = 16, 24
_SIZES = [(16, 24), (25, 37), (33, 51), (32, 48), (41, 75)]      # one tile; two per axis, odd width; more, odd width; all float4; odd, many
_OVERLAPS = [(1, 1), (8, 8), (8, 12)]                             # 1, 8 and T / 2 per axis


def _axis_cover(L, T, origins):
    c = np.zeros(L, dtype=int)
    for o in origins:
        c[o:o + T] += 1
    return int(c.max())


def test_blend_cases_reach_one_two_and_three_covering_tiles():
    covers_y = {_axis_cover(H, TH, vt.tile_plan(H, TH, ov[0])) for H, _ in _SIZES for ov in _OVERLAPS}
    covers_x = {_axis_cover(W, TW, vt.tile_plan(W, TW, ov[1])) for _, W in _SIZES for ov in _OVERLAPS}
    assert {1, 2, 3} <= covers_y and {1, 2, 3} <= covers_x


@pytest.mark.parametrize("ov", _OVERLAPS, ids=[f"ov{a}x{b}" for a, b in _OVERLAPS])
@pytest.mark.parametrize("H,W", _SIZES, ids=[f"{h}x{w}" for h, w in _SIZES])
def test_blend_against_float64(engine, H, W, ov):
    """gl_op_tile_blend against blend64 on the same fp32 tables: per element |got - ref| <= (n + 2) 2^-24 sum |wy wx v| (derivation:
    vae_tiling_ref.blend_bound). Guard zones untouched; a second call gives the same bits; passes of 1, 2 and all tiles give the bits of
    one call; tiles cut from one image blend back to it (partition of unity) within the bound."""
    dev = engine.device
    B = 2
    oy, ox = vt.tile_plan(H, TH, ov[0]), vt.tile_plan(W, TW, ov[1])
    wy, wx = vt.weight_tables(H, TH, ov[0], oy), vt.weight_tables(W, TW, ov[1], ox)
    n = B * len(oy) * len(ox)
    worst = 0.0
    for C in (3, 8):
        tiles = torch.randn(n, C, TH, TW, generator=torch.Generator().manual_seed(H * W + C))
        td = tiles.to(dev)
        want, mag, cnt = ref.blend64(tiles, B, H, W, oy, ox, wy, wx)
        bound = ref.blend_bound(mag, cnt)
        buf, out = _guarded(dev, (B, C, H, W))
        engine.tile_blend(td, out, oy, ox, wy, wx)
        assert _untouched(buf), "the kernel wrote outside its output"
        got = out.cpu()
        assert torch.isfinite(got).all(), "an element was left unwritten"
        err = (got.double() - want).abs()
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), float((err / bound).max())
        again = torch.full((B, C, H, W), float("nan"), device=dev)
        assert torch.equal(engine.tile_blend(td, again, oy, ox, wy, wx).cpu(), got)
        for step in (1, 2):
            split = torch.full((B, C, H, W), float("nan"), device=dev)
            for t0 in range(0, n, step):
                engine.tile_blend(td[t0:t0 + step].contiguous(), split, oy, ox, wy, wx, first_tile=t0)
            assert torch.equal(split.cpu(), got), f"passes of {step} tile(s) changed the bits"
        # partition of unity: the tiles of one image blend back to it
        image = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(7)).to(dev)
        cut = engine.tile_gather(image, [(b, y, x) for b in range(B) for y in oy for x in ox], TH, TW)
        back = engine.tile_blend(cut, torch.empty_like(image), oy, ox, wy, wx).cpu()
        _, mag1, _ = ref.blend64(cut.cpu(), B, H, W, oy, ox, wy, wx)
        # the fp32 weights sum to 1 within (ny + nx) 2^-25 <= (n + 1) 2^-25 (each entry is within 2^-25 of its float64 value and <= 1;
        # an axis that one tile covers has the weight 1 exactly)
        slack = ref.blend_bound(mag1, cnt) + (cnt.double() + 1) * 2.0 ** -25 * image.cpu().double().abs()
        assert ((back.double() - image.cpu().double()).abs() <= slack).all()
        single = cnt == 1
        assert torch.equal(back[:, :, single], image.cpu()[:, :, single]), "where one tile covers, the blend is a copy"
    REPORT[f"blend_{H}x{W}_ov{ov[0]}x{ov[1]}"] = dict(worst_fraction_of_bound=worst, tiles=n, max_cover=int(cnt.max()))


# ---- 3: the tiled decode against the hand composition -------------------------------------------------------------------------------------
def _decode_by_hand(ae, z, tile, overlap):
    """Per-tile untiled decodes, one call each, blended in float64 on the tables the engine uses."""
    B, _, h, w = z.shape
    f = 2 ** (len(ae.ddconfig["ch_mult"]) - 1)
    p = vt.Plan2D(h, w, tile, overlap)
    tiles = torch.cat([ae.decode(z[b:b + 1, :, y:y + p.th, x:x + p.tw].contiguous()).cpu() for b in range(B) for y in p.oy for x in p.ox])
    wy, wx = p.tables(f)
    out, mag, cnt = ref.blend64(tiles, B, h * f, w * f, [y * f for y in p.oy], [x * f for x in p.ox], wy, wx)
    return out, ref.blend_bound(mag, cnt), p


@pytest.mark.parametrize("name,dd,B,overlap,tiles", [("small", "VAE_DDCONFIG_SMALL", 2, 4, (2, 3)), ("full", "VAE_DDCONFIG", 1, 8, (2, 4))])
def test_tiled_decode_is_the_hand_composition(name, dd, B, overlap, tiles):
    """Latent 24 x 40, tile 16. tiles_per_pass = 1: every tile is decoded by the launches of the untiled batch-1 call, so the result is
    held to the blend's own bound. Default tiles_per_pass: the GEMM plans differ with the batch, mse < 1e-4 var as wherever else the batch
    changes them (tests/test_path_gpu.py)."""
    dev = _dev()
    ae = build_product_vae(getattr(syn, dd), device=dev)
    z = (syn.make_latent(B, 4, 24, 40, seed=31) * 0.18215 * 4).to(dev)
    kw = dict(tiling="on", tile=16, overlap=overlap)
    ae.engine.vae_decode(z, tiles_per_pass=1, **kw)                # (tunes the shapes compared below)
    ae.engine.vae_decode(z, **kw)
    _decode_by_hand(ae, z, 16, overlap)
    want, bound, p = _decode_by_hand(ae, z, 16, overlap)
    assert (p.ny, p.nx) == tiles
    one = ae.engine.vae_decode(z, tiles_per_pass=1, **kw).cpu()
    many = ae.engine.vae_decode(z, **kw).cpu()
    err = (one.double() - want).abs()
    frac = float((err / bound).max())
    rel = mse(many, want.float()) / float(want.var())
    REPORT[f"decode_{name}"] = dict(worst_fraction_of_bound_one_per_pass=frac, rel_mse_default_pass=rel, tiles=B * p.ny * p.nx)
    assert (err <= bound).all(), frac
    assert rel < 1e-4, rel
    assert torch.equal(ae.decode(z, **kw).cpu(), many), "AutoencoderKL.decode passes the setting through"
    untiled = ae.decode(z).cpu()
    REPORT[f"decode_{name}"]["rel_mse_tiled_vs_untiled"] = mse(many, untiled) / float(untiled.var())
    ae._drop_engine()


# ---- 4: one tile is the untiled pass ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dd", ["VAE_DDCONFIG_SMALL", "VAE_DDCONFIG"])
def test_single_tile_is_the_untiled_call(dd):
    dev = _dev()
    ae = build_product_vae(getattr(syn, dd), device=dev)
    eng = ae.engine
    f = 2 ** eng.vae_cfg["n_up"]
    z = (syn.make_latent(2, 4, 16, 8, seed=5) * 0.18215 * 4).to(dev)
    img = (torch.rand(2, 3, 16 * f, 8 * f, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(dev)
    noise = torch.randn(2, 4, 16, 8, generator=torch.Generator().manual_seed(9)).to(dev)
    eng.vae_decode(z), eng.vae_encode(img, noise)                 # (tunes)
    counts = []
    for kw in (dict(), dict(tiling="on", tile=16, overlap=8), dict(tiling="on", tile=(16, 8), overlap=(4, 2)), dict(tiling="auto", tile=16, overlap=8)):
        n0 = eng.launch_count()
        d = eng.vae_decode(z, **kw).clone()
        n1 = eng.launch_count()
        e = eng.vae_encode(img, noise, **kw).clone()
        n2 = eng.launch_count()
        counts.append((d, e, n1 - n0, n2 - n1))
    for d, e, nd, ne in counts[1:]:
        assert torch.equal(d, counts[0][0]) and torch.equal(e, counts[0][1])
        assert (nd, ne) == counts[0][2:], "one tile per axis must be the untiled launches"
    n0 = eng.launch_count()
    e, moments = eng.vae_encode(img, noise, tiling="on", tile=16, overlap=8, return_moments=True)
    assert eng.launch_count() - n0 == counts[0][3] and torch.equal(e, counts[0][1])
    assert tuple(moments.shape) == (2, 8, 16, 8) and torch.isfinite(moments).all()
    ae._drop_engine()


# ---- 5: the tiled encode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dd,B,overlap", [("small", "VAE_DDCONFIG_SMALL", 2, 4), ("full", "VAE_DDCONFIG", 1, 8)])
def test_tiled_encode(name, dd, B, overlap):
    """Latent 24 x 40 in tiles of 16 latent pixels (small: image 48 x 80, tile 32 px, overlap 8 px; full: image 192 x 320, tile 128 px,
    overlap 64 px). The blended moments against blend64 of the per-tile moments (single-tile calls, which
    test_single_tile_is_the_untiled_call ties to the untiled pass): mse < 1e-4 var. z against the posterior in float64 from the
    returned moments and the given noise: the tolerance of test_vae_encode_vs_reference."""
    dev = _dev()
    ae = build_product_vae(getattr(syn, dd), device=dev)
    eng = ae.engine
    f = 2 ** eng.vae_cfg["n_up"]
    h, w, T = 24, 40, 16
    img = (torch.rand(B, 3, h * f, w * f, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(dev)
    noise = torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(9)).to(dev)
    kw = dict(tiling="on", tile=T, overlap=overlap)
    eng.vae_encode(img, noise, **kw)                                # (tunes)
    z, moments = eng.vae_encode(img, noise, return_moments=True, **kw)
    assert torch.equal(z, eng.vae_encode(img, noise, **kw)) and tuple(moments.shape) == (B, 8, h, w)
    p = vt.Plan2D(h, w, T, overlap)
    tile_noise = torch.zeros(1, 4, T, T, device=dev)
    per_tile = []
    for b in range(B):
        for y in p.oy:
            for x in p.ox:
                win = img[b:b + 1, :, y * f:(y + T) * f, x * f:(x + T) * f].contiguous()
                per_tile.append(eng.vae_encode(win, tile_noise, return_moments=True, **kw)[1].cpu())
    wy, wx = p.tables(1)
    want, _, _ = ref.blend64(torch.cat(per_tile), B, h, w, p.oy, p.ox, wy, wx)
    rel_m = mse(moments, want.float()) / float(want.var())
    zref = ref.posterior64(moments, ae.quant_conv.weight.detach(), ae.quant_conv.bias.detach(), noise, ae.scale_factor)
    rel_z = mse(z, zref.float()) / float(zref.var())
    REPORT[f"encode_{name}"] = dict(moments_rel_mse=rel_m, z_rel_mse=rel_z, tiles=B * p.ny * p.nx)
    assert rel_m < 1e-4, rel_m
    assert rel_z < 5e-3, rel_z
    # one tile per pass: every tile goes through the launches of its single-tile call (recorded against the blend's bound, not asserted:
    # the bar this test is given is the relative mse above)
    one = eng.vae_encode(img, noise, tiles_per_pass=1, return_moments=True, **kw)[1].cpu()
    want1, mag, cnt = ref.blend64(torch.cat(per_tile), B, h, w, p.oy, p.ox, wy, wx)
    REPORT[f"encode_{name}"]["worst_fraction_of_bound_one_per_pass"] = float(((one.double() - want1).abs() / ref.blend_bound(mag, cnt)).max())
    ae._drop_engine()


# ---- 6: the arena the untiled pass exhausts --------------------------------------------------------------------------------------------------
def test_tiling_decodes_what_the_arena_refuses_and_auto_finds_out():
    """Small VAE (f = 2), flash attention on every context so that the arena holds activations only, batch 1, latent S = 96 x 96, tile
    16, overlap 4, 4 tiles per pass. Read at run time on a 2 GB context: U = high-water mark of the untiled decode, T = of the tiled
    one; the test asserts U >= 2 T and runs on a context of A = sqrt(U T) bytes. On an MI355X: U = 105 021 440, T = 11 862 016,
    A = 35 295 410 bytes (pure functions of the allocation sequence; the recorded property `arena_auto` carries them)."""
    dev = _dev()
    ae = build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    S, kw = 96, dict(tile=16, overlap=4, tiles_per_pass=4)
    z = (syn.make_latent(1, 4, S, S, seed=11) * 0.18215 * 4).to(dev)
    small = z[:, :, :24, :24].contiguous()

    def ctx(gb):
        e = rt.build_vae_engine(ae, arena_gb=gb)
        e.set_vae_attention("flash")
        return e
    e = ctx(2.0)
    untiled_big = e.vae_decode(z).clone()
    U = e.arena_high_water()
    e.close()
    e = ctx(2.0)
    e.vae_decode(z, tiling="on", **kw)                             # (tunes the tiles' shapes)
    tiled_big = e.vae_decode(z, tiling="on", **kw).clone()
    T = e.arena_high_water()
    e.vae_decode(small)                                            # (tunes the small shape before it is compared bit for bit)
    e.close()
    A = int(math.sqrt(float(U) * float(T)))
    REPORT["arena_auto"] = dict(U=U, T=T, A=A, S=S)
    assert U >= 2 * T, (U, T)
    e = ctx(A / float(1 << 30))
    before = e.vae_decode(small, tiling="auto", **kw).clone()      # fits: the untiled bits
    assert torch.equal(before, e.vae_decode(small)) and not torch.equal(before, e.vae_decode(small, tiling="on", **kw))
    with pytest.raises(GligenAmdError, match="workspace arena exhausted"):
        e.vae_decode(z)
    n0 = e.launch_count()
    on = e.vae_decode(z, tiling="on", **kw).clone()
    d_on = e.launch_count() - n0
    assert torch.isfinite(on).all() and tuple(on.shape) == (1, 3, 2 * S, 2 * S)
    assert torch.equal(on, tiled_big), "the arena's size must not change the tiled result"
    n0 = e.launch_count()
    auto1 = e.vae_decode(z, tiling="auto", **kw).clone()
    d_auto1 = e.launch_count() - n0
    n0 = e.launch_count()
    auto2 = e.vae_decode(z, tiling="auto", **kw).clone()
    d_auto2 = e.launch_count() - n0
    assert torch.equal(auto1, on) and torch.equal(auto2, on)
    assert d_auto1 > d_on and d_auto2 == d_on, "the second 'auto' call must go straight to the tiles"
    # the context is as usable as before the fallback: a size that fits still gives the untiled bits
    assert torch.equal(e.vae_decode(small, tiling="auto", **kw), before)
    assert e.arena_high_water() <= A
    REPORT["arena_auto"].update(launches_tiled=d_on, launches_first_auto=d_auto1, rel_mse_tiled_vs_untiled=mse(on, untiled_big) / float(untiled_big.var()))
    e.close()
    ae._drop_engine()


# ---- 7: through the public interface ----------------------------------------------------------------------------------------------------------
VT = dict(vae_tiling="on", vae_tile=8, vae_tile_overlap=4)         # the goldens' 16 x 16 latent: 3 x 3 tiles of 8 x 8
EKW = dict(tiling="on", tile=8, overlap=4)


def test_generate_with_tiling_is_sampling_then_the_tiled_decode(tmp_path, monkeypatch):
    import gligen_inference as gi
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from test_img2img_gpu import S1, _Case, _gen_kwargs, _to
    dev = _dev()
    monkeypatch.setattr(gi, "device", dev)
    case = _Case(dev, tmp_path, monkeypatch, [1, 0, 0])
    model, ae = case.model(), build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)
    x_T = syn.make_latent(case.B, 4, case.hw, case.hw, seed=6).to(dev)
    gen = lambda **kw: gi.generate(model, ae, case.diffusion, _to(case.batch, dev), case.ctx.to(dev), case.uc.to(dev), starting_noise=x_T.clone(),
                                   **_gen_kwargs(case), **kw).clone()
    gen(**VT), gen()                                               # (tunes)
    got, plain, off = gen(**VT), gen(), gen(vae_tiling="off", vae_tile=8, vae_tile_overlap=4)
    assert torch.equal(plain, off), "vae_tiling='off' must be the call without the keywords"
    assert not torch.equal(got, plain)
    lat, _ = case.run(model, DPMSolverSampler, S1, (case.B, 4, case.hw, case.hw), x_T.clone(), None, None, "bicubic", ddim_discretize="logsnr")
    assert torch.equal(got, ae.engine.vae_decode(lat, **EKW))
    assert torch.equal(plain, ae.engine.vae_decode(lat))
    REPORT["generate_tiled"] = dict(rel_mse_tiled_vs_untiled=mse(got, plain) / float(plain.var()))
    model._drop_engine()
    ae._drop_engine()


def test_generate_hires_pixel_bicubic_with_tiling_is_the_hand_composition(tmp_path, monkeypatch):
    """The pixel-bicubic round trip decodes, enlarges and encodes with the setting; from the second call on no context allocates."""
    import gligen_inference as gi
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from test_img2img_gpu import HIRES_PX, HIRES_STRENGTH, S1, S2, _Case, _gen_kwargs, _to
    dev = _dev()
    monkeypatch.setattr(gi, "device", dev)
    case = _Case(dev, tmp_path, monkeypatch, [1, 0, 0])
    model, ae = case.model(), build_product_vae(syn.VAE_DDCONFIG_SMALL, device=dev)

    def call():
        torch.manual_seed(123)
        x_T = syn.make_latent(case.B, 4, case.hw, case.hw, seed=6).to(dev)
        return gi.generate(model, ae, case.diffusion, _to(case.batch, dev), case.ctx.to(dev), case.uc.to(dev), starting_noise=x_T, hires=HIRES_PX,
                           hires_strength=HIRES_STRENGTH, hires_steps=S2, hires_upscaler="pixel-bicubic", **_gen_kwargs(case), **VT).clone()
    outs, mems = [], []
    for _ in range(3):
        outs.append(call())
        fork = model.__dict__["_hires"][(case.B, HIRES_PX[0] // 2, HIRES_PX[1] // 2)][0]
        torch.cuda.synchronize()
        mems.append((model.engine.memory(), fork.engine.memory(), ae.engine.memory()))
    assert mems[1] == mems[2], "a context allocated between the second and the third call"
    assert torch.equal(outs[1], outs[2]) and tuple(outs[1].shape) == (case.B, 3) + HIRES_PX
    other = case.model()
    torch.manual_seed(123)
    x_T = syn.make_latent(case.B, 4, case.hw, case.hw, seed=6).to(dev)
    lat, _ = case.run(other, DPMSolverSampler, S1, (case.B, 4, case.hw, case.hw), x_T, None, None, "bicubic", ddim_discretize="logsnr")
    image = torch.clamp(ae.decode(lat, **EKW), -1.0, 1.0)
    lat = ae.encode(other.engine.latent_renoise(image, HIRES_PX, "bicubic"), **EKW)
    lat2, _ = case.run(other, DPMSolverSampler, S2, (case.B, 4, HIRES_PX[0] // 2, HIRES_PX[1] // 2), None, lat, HIRES_STRENGTH, "bicubic", ddim_discretize="logsnr")
    assert torch.equal(outs[1], ae.decode(lat2, **EKW))
    for m in (model, other, ae):
        m._drop_engine()
