"""The CLIP image front end on the device: Engine.image_resample against Pillow byte for byte, Engine.clip_vision_preprocess against
transformers' CLIPImageProcessor bit for bit (one mixed-size batch, two launches, batch invariance), image features that do not depend
on where the preprocessing ran, and refusals that name the limit."""
import numpy as np
import pytest
import torch

import test_image_front_end_cpu as ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_image_resample_is_pillow_byte_for_byte(engine, filt):
    """The ten resize cases in ONE call (different sizes, no crop): both edge clamps of the bounds, ksize 3 .. 61, skipped passes,
    the near-identity 4000 -> 3982 phase walk and both clip8 clamps; then a view with a row stride and a crop box inside the image."""
    assert ref.restatement_equals_pillow()
    images = [ref.image(W, H, case) for case, (W, H, w, h) in enumerate(ref.RESIZE_CASES)]
    n0 = engine.launch_count()
    outs = engine.image_resample(images, [(w, h) for W, H, w, h in ref.RESIZE_CASES], filter=filt)
    assert engine.launch_count() - n0 == 2
    for case, (W, H, w, h) in enumerate(ref.RESIZE_CASES):
        want = ref.pillow_resize(case, filt)
        got = outs[case].cpu().numpy()
        assert got.shape == want.shape == (h, w, 3)
        bad = int((got != want).sum())
        print(f"{filt} {W}x{H} -> {w}x{h}: {bad} of {want.size} bytes differ")
        assert bad == 0, (filt, W, H, w, h, bad)
    # a row stride larger than 3 W (and a base address that is no multiple of 4), crop boxes inside the resized image
    W, H, w, h = ref.RESIZE_CASES[0]
    wide = torch.zeros((H, W + 13, 3), dtype=torch.uint8, device=engine.device)
    wide[:, 5:5 + W] = torch.from_numpy(images[0]).to(engine.device)
    view = wide[:, 5:5 + W]
    assert view.stride(0) == 3 * (W + 13) and view.data_ptr() % 4 == 3
    boxes = [(37, 11, 201, 150), (0, 0, 7, 224), (291, 223, 7, 1)]
    outs = engine.image_resample([view] * 3, [(w, h)] * 3, boxes, filter=filt)
    want = ref.pillow_resize(0, filt)
    for (x, y, cw, ch), got in zip(boxes, outs):
        assert np.array_equal(got.cpu().numpy(), want[y:y + ch, x:x + cw]), (filt, x, y, cw, ch)


def test_clip_vision_preprocess_is_the_processor_bit_for_bit(engine):
    """Nine image sizes in ONE mixed-size call against transformers.CLIPImageProcessor(); the same images one at a time give the same
    bits; the batched call is two launches."""
    assert ref.restatement_equals_pillow()
    want, levels, want_levels = ref.processor_pixel_values()
    images = [ref.image(w, h, 100 + i) for i, (w, h) in enumerate(ref.CHAIN_SIZES)]
    kw = dict(size=224, crop=224, mean=ref.CLIP_MEAN, std=ref.CLIP_STD)
    n0 = engine.launch_count()
    got = engine.clip_vision_preprocess(images, **kw)
    assert engine.launch_count() - n0 == 2
    assert got.shape == (len(images), 3, 224, 224) and got.dtype == torch.float32 and got.device.type == "cuda"
    got = got.cpu().numpy()
    for i, (w, h) in enumerate(ref.CHAIN_SIZES):
        ref.assert_pixel_values_equal(got[i], want[i], f"{w}x{h}")
        assert np.array_equal(got[i], ref.clip_chain(images[i], **kw)[1]), (w, h)          # and the restatement exactly
        alone = engine.clip_vision_preprocess([torch.from_numpy(images[i])], **kw).cpu().numpy()
        assert np.array_equal(alone[0], got[i]), f"{w}x{h}: the bits depend on the batch"
    ref.assert_pixel_values_equal(engine.clip_vision_preprocess([levels], **kw).cpu().numpy()[0], want_levels, "all 256 levels")


def _native_clip_model(tmp_path):
    """A fabricated CLIPModel whose vision side the native tower supports (hidden 128 / 2 heads of 64 / patch 32 / quick_gelu) with
    helpers._fabricated_clip's processor: the construction of tests/test_clip_vision_gpu.py."""
    import transformers
    from helpers import _fabricated_clip
    model, processor, tok = _fabricated_clip(tmp_path)
    vcfg = transformers.CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=224,
                                         patch_size=32, projection_dim=768, hidden_act="quick_gelu")
    torch.manual_seed(1)
    native = transformers.CLIPModel(transformers.CLIPConfig(text_config=model.config.text_config.to_dict(), vision_config=vcfg.to_dict(),
                                                            projection_dim=768)).eval()
    return native, processor


def test_image_features_do_not_depend_on_where_the_preprocessing_ran(tmp_path, monkeypatch):
    """get_clip_image_features with preprocess="auto" (native: the processor is patched to raise) and with preprocess="processor"
    return torch.equal features for PNG files of three sizes: bit-equal pixel_values, a deterministic tower."""
    import gligen_inference as gi
    from PIL import Image
    from gligen_amd.runtime import build_clip_vision_engine
    assert ref.restatement_equals_pillow()
    native, processor = _native_clip_model(tmp_path)
    monkeypatch.chdir(tmp_path)
    torch.save(torch.randn(768, 768, generator=torch.Generator().manual_seed(5)) * 0.03, tmp_path / "projection_matrix")
    paths = []
    for i, (w, h) in enumerate([(240, 300), (640, 480), (97, 61)]):
        Image.fromarray(ref.image(w, h, 40 + i)).save(tmp_path / f"im{i}.png")
        paths.append(str(tmp_path / f"im{i}.png"))
    dev = torch.device("cuda", 0)
    monkeypatch.setattr(gi, "device", dev)
    eng = build_clip_vision_engine(native.to(dev))
    try:
        by_processor = gi.get_clip_image_features(native, processor, [paths[0], None, paths[1], paths[2]], eng, preprocess="processor")

        def no_processor(*a, **k):
            raise AssertionError("the processor must not run: the images are preprocessed on the device")

        monkeypatch.setattr(type(processor), "__call__", no_processor)
        monkeypatch.setattr(type(processor.image_processor), "__call__", no_processor)
        monkeypatch.setattr(type(processor.image_processor), "preprocess", no_processor)
        n0 = eng.launch_count()
        auto = gi.get_clip_image_features(native, processor, [paths[0], None, paths[1], paths[2]], eng)
        assert eng.launch_count() - n0 > 2
        one = gi.get_clip_feature(native, processor, paths[2], is_image=True, vision=eng, preprocess="native")
    finally:
        eng.close()
    assert auto[1] is None and by_processor[1] is None
    for i in (0, 2, 3):
        assert auto[i].shape == (1, 768) and auto[i].device.type == "cuda" and torch.equal(auto[i], by_processor[i]), i
    assert torch.equal(one, auto[3])
    assert not torch.equal(auto[0], auto[2]) and not torch.equal(auto[2], auto[3])


def test_limits_are_refused_by_name(engine):
    from gligen_amd import GligenAmdError
    small = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(GligenAmdError, match="16384"):
        engine.image_resample([np.zeros((8, 16385, 3), np.uint8)], [(224, 224)])
    with pytest.raises(GligenAmdError, match="16384"):
        engine.image_resample([np.zeros((16385, 8, 3), np.uint8)], [(224, 224)])
    with pytest.raises(GligenAmdError, match="16384"):
        engine.image_resample([small], [(16385, 8)])
    with pytest.raises(ValueError, match="bicubic, bilinear"):
        engine.image_resample([small], [(4, 4)], filter="lanczos")
    with pytest.raises(GligenAmdError, match="crop box"):
        engine.image_resample([small], [(4, 4)], [(1, 1, 4, 4)])
    with pytest.raises(ValueError, match="u8"):
        engine.image_resample([np.zeros((8, 8, 4), np.uint8)], [(4, 4)])
    with pytest.raises(ValueError, match="u8"):
        engine.image_resample([np.zeros((8, 8, 3), np.float32)], [(4, 4)])
    with pytest.raises(GligenAmdError, match="cropped to"):      # one fp32 tensor: all crops equal
        engine.image_resample([small, small], [(4, 4), (5, 5)], lut=np.zeros((3, 256), np.float32))
    # and the engine still works afterwards
    out = engine.image_resample([ref.image(8, 8, 0)], [(8, 8)])[0]
    assert np.array_equal(out.cpu().numpy(), ref.image(8, 8, 0))
