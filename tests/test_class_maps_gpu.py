"""Semantic maps as class indices on the device. A u8 class map stands for its 152 one-hot planes, so every result here is compared
bit for bit with what the planes give on the same engine (torch.equal, no tolerance), and next to that with what judged the planes
path before: Pillow for the resize, torch on the CPU for the downsampler, the reference's goldens for tokens and eps."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_class_maps_cpu as ref
from helpers import golden_shapes, load_golden, mse
from gligen_amd import synthetic as syn

pytestmark = pytest.mark.gpu

EPS_MSE_TOL = 2e-4     # absolute, on eps with std ~0.3: tests/test_configs_gpu.py's bar
N_CLASSES = 152


def planes_of(cls):
    """u8 [B,1,H,W] -> fp32 one-hot planes [B,152,H,W]; a value >= 152 (255: no class) becomes all-zero planes."""
    idx = cls.long()
    return torch.zeros(cls.shape[0], N_CLASSES, *cls.shape[2:], device=cls.device).scatter_(1, idx.clamp(max=N_CLASSES - 1), (idx < N_CLASSES).float())


def random_map(B, H, W, seed):
    """Per-pixel random classes with 0 and 151 present and a block of 255."""
    cls = torch.randint(0, N_CLASSES, (B, 1, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.uint8)
    cls[:, :, 0, 0], cls[:, :, 0, 1] = 0, N_CLASSES - 1
    cls[:, :, H // 3:H // 3 + max(H // 4, 3), W // 2:W // 2 + max(W // 5, 3)] = 255
    cls[0, :, -1, -1], cls[-1, :, -1, 0] = 255, N_CLASSES - 1         # the corners, where the padding meets "no class"
    return cls


# ---- 1. resize ---------------------------------------------------------------------------------------------------------------
def test_class_map_resize_is_pillow_byte_for_byte(engine):
    """The nine sizes in ONE call with prepare_batch_sem's centre-crop boxes to 512 x 512; then row-strided device views with off-centre
    boxes to 64 x 48, and to 61 x 47 (rows that are no whole words)."""
    assert ref.restatement_equals_pillow()
    maps = [ref.class_map(w, h, i) for i, (w, h) in enumerate(ref.SIZES)]
    boxes = [ref.centre_box(w, h) for w, h in ref.SIZES]
    n0 = engine.launch_count()
    out = engine.class_map_resize(maps, (512, 512), boxes)
    assert engine.launch_count() - n0 == 1
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(maps), 512, 512) and out.device.type == "cuda"
    got = out.cpu().numpy()
    for i, (w, h) in enumerate(ref.SIZES):
        bad = int((got[i] != ref.pillow_nearest(maps[i], boxes[i], 512, 512)).sum())
        print(f"{w}x{h} -> 512x512: {bad} bytes differ")
        assert bad == 0, (w, h, bad)
    views, arrays = [], []
    for i, (w, h) in enumerate([(97, 61), (640, 480), (333, 500)]):
        a = ref.class_map(w, h, 20 + i)
        wide = torch.zeros((h, w + 13), dtype=torch.uint8, device=engine.device)
        wide[:, 5:5 + w] = torch.from_numpy(a).to(engine.device)
        views.append(wide[:, 5:5 + w])
        arrays.append(a)
        assert views[-1].stride(0) == w + 13
    boxes = [(5, 7, 60, 40), (301, 11, 339, 469), (0, 499, 333, 1)]
    for size in ((64, 48), (61, 47)):
        got = engine.class_map_resize(views, size, boxes).cpu().numpy()
        for a, box, g in zip(arrays, boxes, got):
            assert np.array_equal(g, ref.pillow_nearest(a, box, *size)), (a.shape, box, size)
    assert np.array_equal(engine.class_map_resize([arrays[0]], (97, 61)).cpu().numpy()[0], arrays[0])      # no box: the whole map
    from gligen_amd._lib import GligenAmdError
    with pytest.raises(GligenAmdError, match="16384"):
        engine.class_map_resize([arrays[0]], (16385, 4))
    with pytest.raises(GligenAmdError, match="does not lie inside"):
        engine.class_map_resize([arrays[0]], (8, 8), [(90, 0, 8, 8)])


# ---- 2. downsampler ------------------------------------------------------------------------------------------------------------
def _downsamplers():
    from ldm.modules.diffusionmodules._spatial import SpatialDownsampler
    from ldm.modules.diffusionmodules.sem_grounding_downsampler import GroundingDownsampler

    class Nearest4(SpatialDownsampler):      # the base class's 4 middle channels (one channel group per pixel), sem's nearest resize
        mode = "nearest"
    return {"sem16": GroundingDownsampler, "base4": Nearest4}


@pytest.mark.parametrize("kind", ["sem16", "base4"])
@pytest.mark.parametrize("side", [50, 20])
def test_downsampler_from_classes_equals_planes(engine, kind, side):
    """SpatialDownsampler(resize_input=32, in_dim=152, out_dim=8) -- the semantic-map subclass (16 middle channels) and the base class's
    4 -- on a class map against the same module on its one-hot planes: the same bits; and both within 2e-5 of torch's fp32
    F.interpolate + convs on the CPU (fp32 on both sides: the bar of test_spatial_modality_vs_reference). 50 x 50 is scaled down by
    1.5625, 20 x 20 up."""
    dev = engine.device
    ds = syn.fill_module_(_downsamplers()[kind](resize_input=32, in_dim=N_CLASSES, out_dim=8).eval(), 77).to(dev)
    cls = random_map(2, side, side, seed=side).to(dev)
    planes = planes_of(cls)
    want = ds(planes, engine=engine)
    n0 = engine.launch_count()
    got = ds(cls, engine=engine)
    assert engine.launch_count() - n0 == 3
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 8, 8, 8) and torch.isfinite(got).all()
    assert torch.equal(got, want), float((got - want).abs().max())
    with torch.no_grad():
        cpu = ds.layers.cpu()(F.interpolate(planes.cpu(), 32, mode="nearest"))
    err = float((got.cpu() - cpu).abs().max())
    print(f"{kind} {side}x{side}: max abs err vs torch CPU {err:.3e}, std {float(cpu.std()):.3f}")
    assert err < 2e-5, err


def test_downsampler_refusals_name_the_limit(engine):
    from gligen_amd._lib import GligenAmdError
    from ldm.modules.diffusionmodules.canny_grounding_downsampler import GroundingDownsampler as Canny
    dev = engine.device
    cls = random_map(1, 20, 20, seed=1).to(dev)
    w1, b1, w2, b2 = torch.zeros(4, N_CLASSES, 4, 4), torch.zeros(4), torch.zeros(8, 4, 4, 4), torch.zeros(8)
    with pytest.raises(GligenAmdError, match="multiple of 4"):
        engine.grounding_downsample_classes(cls, N_CLASSES, 30, (w1, b1, w2, b2))
    with pytest.raises(GligenAmdError, match="multiple of 4"):
        engine.grounding_downsample_classes(cls, N_CLASSES, 32, (torch.zeros(6, N_CLASSES, 4, 4), torch.zeros(6), torch.zeros(8, 6, 4, 4), b2))
    with pytest.raises(ValueError, match="u8"):
        engine.grounding_downsample_classes(cls.float(), N_CLASSES, 32, (w1, b1, w2, b2))
    with pytest.raises(ValueError, match="uint8 class map"):
        Canny().to(dev)(cls, engine=engine)


# ---- 3. / 4. tokenizer and the whole modality ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sem_model():
    """The unet_small_sem model of the golden, its inputs, and the planes path's results on the same engine (computed once)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    from types import SimpleNamespace
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from ldm.util import instantiate_from_config
    g = load_golden("unet_small_sem")
    meta = g["meta"]
    model = syn.fill_module_(UNetModel(**meta["cfg"]).eval(), 1234).to(dev)
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == golden_shapes("unet_small_sem")
    B, hw = meta["B"], meta["hw"]
    planes = syn.make_spatial_map("sem", B, meta["res"], seed=1).to(dev)
    cls = planes.argmax(1, keepdim=True).to(torch.uint8)
    assert torch.equal(planes_of(cls), planes)
    new_input = lambda: instantiate_from_config(dict(target="grounding_input.sem_grounding_tokinzer_input.GroundingNetInput"))
    s = SimpleNamespace(g=g, meta=meta, model=model, dev=dev, planes=planes, cls=cls, mask=torch.ones(B, 1, device=dev), new_input=new_input,
                        x=syn.make_latent(B, 4, hw, hw, seed=1).to(dev), ctx=syn.make_context(B, seed=1).to(dev), t=torch.tensor([981, 441][:B], device=dev))
    yield s
    model._drop_engine()


def test_tokens_from_classes_equal_planes(sem_model):
    s = sem_model
    pn, eng = s.model.position_net, s.model.engine
    tok_planes = pn.tokens(engine=eng, sem=s.planes, mask=s.mask)
    tok = pn.tokens(engine=eng, sem=s.cls, mask=s.mask)
    assert tok.dtype == torch.float32 and tuple(tok.shape) == tuple(s.g["objs"].shape)
    assert torch.equal(tok, tok_planes), float((tok - tok_planes).abs().max())
    want = torch.from_numpy(s.g["objs"].astype(np.float32))
    rel = mse(tok, want) / float(want.var())
    print(f"tokens rel. MSE vs the reference {rel:.3e}")
    assert rel < 3e-4, rel
    # per-pixel random classes at a size that is no multiple of anything (100 -> 128: scaled up by 1.28), with a block of "no class"
    cls = random_map(2, 100, 100, seed=5).to(s.dev)
    assert torch.equal(pn.tokens(engine=eng, sem=cls, mask=s.mask), pn.tokens(engine=eng, sem=planes_of(cls), mask=s.mask))
    # 300 -> 128: scaled down, and a mask that mixes the null feature in
    cls = random_map(2, 300, 300, seed=6).to(s.dev)
    mask = torch.tensor([[1.0], [0.0]], device=s.dev)
    assert torch.equal(pn.tokens(engine=eng, sem=cls, mask=mask), pn.tokens(engine=eng, sem=planes_of(cls), mask=mask))
    # the null input of a class map: u8, all 255, and the tokens of the planes path's all-zero planes
    gin, gin_planes = s.new_input(), s.new_input()
    gin.prepare({"sem": s.cls, "mask": s.mask})
    gin_planes.prepare({"sem": s.planes, "mask": s.mask})
    null = gin.get_null_input()
    assert null["sem"].dtype == torch.uint8 and tuple(null["sem"].shape) == tuple(s.cls.shape) and bool((null["sem"] == 255).all())
    tok_null = pn.tokens(engine=eng, **null)
    assert torch.equal(tok_null, pn.tokens(engine=eng, **gin_planes.get_null_input()))
    want = torch.from_numpy(s.g["objs_null"].astype(np.float32))
    assert mse(tok_null, want) / float(want.var()) < 3e-4


def test_class_map_to_a_tokenizer_without_in_dim_is_refused():
    from ldm.modules.diffusionmodules.canny_grounding_net import PositionNet
    with pytest.raises(ValueError, match="canny_edge.*uint8 class map"):
        PositionNet(resize_input=64).tokens(engine=object(), canny_edge=torch.zeros(1, 1, 8, 8, dtype=torch.uint8), mask=torch.ones(1, 1))


def test_whole_modality_from_classes_equals_planes(sem_model):
    """model(inp) with the u8 map as grounding_input["sem"] and as grounding_extra_input: the eps of the planes run on the same model,
    bit for bit, cond and null, and both within the bar against the reference; the conditioning is computed once per distinct input."""
    s = sem_model
    model, eng = s.model, s.model.engine
    base = dict(x=s.x, timesteps=s.t, context=s.ctx, inpainting_extra_input=None)
    eps = {}
    for name, m in (("planes", s.planes), ("classes", s.cls)):
        gin = s.new_input()
        model.grounding_tokenizer_input = gin
        prepared = gin.prepare({"sem": m, "mask": s.mask})
        inp = dict(base, grounding_input=prepared, grounding_extra_input=m)
        n0 = eng.launch_count()
        cond = model(inp).clone()
        n1 = eng.launch_count()
        again = model(inp).clone()
        n2 = eng.launch_count()
        assert torch.equal(cond, again)
        assert 0 < n2 - n1 < n1 - n0, (name, n1 - n0, n2 - n1)          # the second call: the UNet alone
        null = model({k: v for k, v in inp.items() if k != "grounding_input"}).clone()
        eps[name] = (cond, null, n1 - n0, n2 - n1)
    assert eps["classes"][3] == eps["planes"][3]                        # the same UNet launches
    assert torch.equal(eps["classes"][0], eps["planes"][0]) and torch.equal(eps["classes"][1], eps["planes"][1])
    r = dict(eps=mse(eps["classes"][0], s.g["eps"]), eps_null=mse(eps["classes"][1], s.g["eps_null"]))
    print(r)
    assert r["eps"] < EPS_MSE_TOL and r["eps_null"] < EPS_MSE_TOL, r


# ---- 5. front end from files -----------------------------------------------------------------------------------------------------------
def test_native_inputs_from_files_equal_the_host_path(tmp_path, monkeypatch):
    from PIL import Image
    import gligen_inference as gi
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    for i, (w, h) in enumerate([(333, 500), (640, 480)]):
        Image.fromarray(ref.class_map(w, h, 30 + i)).save(tmp_path / f"sem{i}.png")
        Image.fromarray(np.random.RandomState(40 + i).randint(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / f"rgb{i}.png")
        sem, rgb = str(tmp_path / f"sem{i}.png"), str(tmp_path / f"rgb{i}.png")
        monkeypatch.setattr(gi, "device", "cpu")
        host_sem = gi.prepare_batch_sem(dict(sem=sem), 2)
        host_canny = gi.prepare_batch_canny(dict(canny_image=rgb), 2)
        host_z = gi.load_inpaint_image(rgb)
        monkeypatch.setattr(gi, "device", dev)
        got = gi.prepare_batch_sem(dict(sem=sem), 2, native=True)
        assert set(got) == {"sem", "mask"} and got["sem"].dtype == torch.uint8 and tuple(got["sem"].shape) == (2, 1, 512, 512) and got["sem"].is_cuda
        assert torch.equal(got["sem"].cpu()[:, 0].long(), host_sem["sem"].argmax(1)) and torch.equal(got["mask"].cpu(), host_sem["mask"])
        got = gi.prepare_batch_canny(dict(canny_image=rgb), 2, native=True)
        assert got["canny_edge"].dtype == torch.float32 and got["canny_edge"].is_cuda
        assert torch.equal(got["canny_edge"].cpu(), host_canny["canny_edge"]) and torch.equal(got["mask"].cpu(), host_canny["mask"])
        z = gi.load_inpaint_image(rgb, native=True)
        assert z.is_cuda and tuple(z.shape) == (1, 3, 512, 512) and torch.equal(z.cpu(), host_z)
    bad = ref.class_map(64, 64, 3)
    bad[5, 9] = 200
    Image.fromarray(bad).save(tmp_path / "bad.png")
    with pytest.raises(ValueError, match=r"\b200\b"):
        gi.prepare_batch_sem(dict(sem=str(tmp_path / "bad.png")), 2, native=True)
