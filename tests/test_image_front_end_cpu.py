"""The CLIP image front end without a GPU: a numpy restatement of Pillow's 8-bit resampler (checked against the installed Pillow
before anything is compared with it), the library's coefficient tables, the whole chain against transformers' CLIPImageProcessor,
the settings reader, the host wiring of get_clip_image_features(..., preprocess=...) and the kernels' ISA facts."""
import ctypes
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the resampler, restated --------------------------------------------------------------------------------------------------
PRECISION_BITS = 22


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {"bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0)}


@functools.lru_cache(maxsize=None)
def coeffs(n_in, n_out, filt):
    """(ksize, bounds int32 [out, 2] = (first sample, count), coefficients int32 [out, ksize] in units of 2^-22), all in double."""
    f, filter_support = FILTERS[filt]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = filter_support * fs
    ksize = 2 * math.ceil(support) + 1
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def _one_pass(a, bounds, kk):
    """Along axis 1 of u8 [n, in, 3] -> u8 [n, out, 3]: clip8((2^21 + sum pixel * k) >> 22) (the sums stay below 2^31)."""
    out = np.empty((a.shape[0], len(bounds), 3), np.uint8)
    a = a.astype(np.int64)
    for xx, (xmin, xmax) in enumerate(bounds):
        acc = (a[:, xmin:xmin + xmax, :] * kk[xx, :xmax, None].astype(np.int64)).sum(1) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(a, w, h, filt):
    """PIL.Image.resize((w, h)) of u8 [H, W, 3]: horizontal pass first, u8 between the passes, a pass that keeps its size skipped."""
    H, W = a.shape[:2]
    if W != w:
        a = _one_pass(a, *coeffs(W, w, filt)[1:])
    if H != h:
        a = _one_pass(a.transpose(1, 0, 2), *coeffs(H, h, filt)[1:]).transpose(1, 0, 2)
    return np.ascontiguousarray(a)


def clip_size(w, h, s):
    short, long = min(w, h), max(w, h)
    new_long = int(s * long / short)
    return (s, new_long) if w <= h else (new_long, s)


def lut(mean, std):
    v = np.arange(256, dtype=np.float32)[None] / np.float32(255)
    return (v - np.asarray(mean, np.float32)[:, None]) / np.asarray(std, np.float32)[:, None]


def clip_chain(a, size, crop, mean, std, filt="bicubic"):
    """The u8 crop [crop, crop, 3] and pixel_values float32 [3, crop, crop] of one image."""
    w, h = clip_size(a.shape[1], a.shape[0], size)
    r = resize(a, w, h, filt)
    x, y = (w - crop) // 2, (h - crop) // 2
    u8 = r[y:y + crop, x:x + crop]
    t = lut(mean, std)
    return u8, np.stack([t[c][u8[..., c]] for c in range(3)])


# ---- the cases ------------------------------------------------------------------------------------------------------------------
RESIZE_CASES = [(640, 480, 298, 224), (333, 500, 224, 336), (224, 224, 224, 224), (100, 75, 298, 224), (517, 389, 512, 512),
                (2000, 1333, 336, 224), (31, 47, 224, 339), (225, 224, 225, 224), (4000, 225, 3982, 224), (1500, 40, 100, 40)]
CHAIN_SIZES = [(640, 480), (333, 500), (224, 224), (100, 75), (2000, 1333), (31, 47), (225, 224), (4000, 225), (223, 900)]
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def image(w, h, seed):
    """Seeded random u8 [h, w, 3]; odd widths carry full rows of 255 and of 0, so that both clamps of clip8 fire (bicubic overshoot)."""
    a = np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)
    if w % 2:
        a[::7] = 255
        a[3::11] = 0
    return a


@functools.lru_cache(maxsize=None)
def pillow_resize(case, filt):
    from PIL import Image
    W, H, w, h = RESIZE_CASES[case]
    return np.asarray(Image.fromarray(image(W, H, case)).resize((w, h), {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[filt]))


@functools.lru_cache(maxsize=None)
def restatement_equals_pillow():
    """Asserted first by every test that compares something with the restatement: a restatement that drifts from the installed
    Pillow fails here and cannot hide an error of the library."""
    import PIL
    for case, (W, H, w, h) in enumerate(RESIZE_CASES):
        for filt in FILTERS:
            got = resize(image(W, H, case), w, h, filt)
            bad = int((got != pillow_resize(case, filt)).sum())
            assert bad == 0, f"restatement != Pillow {PIL.__version__}: {W}x{H} -> {w}x{h} {filt}: {bad} bytes differ"
    return True


def test_restatement_is_pillow_byte_for_byte():
    assert restatement_equals_pillow()
    # the cases reach what they are there for: both edge clamps, ksize 5 .. 61, skipped passes, both clip8 clamps
    ks = {coeffs(a, b, f)[0] for W, H, w, h in RESIZE_CASES for a, b in ((W, w), (H, h)) if a != b for f in FILTERS}
    assert min(ks) == 3 and 5 in ks and max(ks) == 61
    _, b, _ = coeffs(4000, 3982, "bicubic")
    assert b[0, 0] == 0 and b[-1].sum() == 4000 and len(set((b[:, 0] - np.arange(3982)).tolist())) > 10       # the phase walks
    assert any(W == w for W, H, w, h in RESIZE_CASES) and any(H == h for W, H, w, h in RESIZE_CASES)
    out = pillow_resize(1, "bicubic")
    assert out.min() == 0 and out.max() == 255


# ---- the library's tables -------------------------------------------------------------------------------------------------------
def _lib():
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    return _lib.load()


def lib_coeffs(lib, n_in, n_out, filt):
    ks = ctypes.c_int(0)
    rc = lib.gl_image_resample_coeffs(n_in, n_out, filt, ctypes.byref(ks), None, 0, None, 0)
    assert rc == 0, lib.gl_last_error()
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.full((n_out, ks.value), -7, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    rc = lib.gl_image_resample_coeffs(n_in, n_out, filt, ctypes.byref(ks), bounds.ctypes.data_as(ip), bounds.size, kk.ctypes.data_as(ip), kk.size)
    assert rc == 0, lib.gl_last_error()
    return ks.value, bounds, kk


def test_image_entry_points_are_declared_exported_and_bound(tmp_path):
    """include/gligen_amd_image.h, the library's exports and the ctypes table agree; gl_image_desc has the size ctypes gives it."""
    lib = _lib()
    from gligen_amd import _lib as table
    header = open(os.path.join(ROOT, "include", "gligen_amd_image.h")).read()
    declared = set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", header))
    assert declared == set(table.IMAGE_SYMBOLS) == {"gl_op_image_resample", "gl_image_resample_coeffs"} and not declared & set(table.SYMBOLS)
    assert all(hasattr(lib, n) for n in declared)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gligen_amd_image.h"\nint main(void) { printf("%zu\\n", sizeof(gl_image_desc)); return 0; }\n')
    subprocess.run([shutil.which("gcc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout
    assert int(out) == ctypes.sizeof(table.ImageDesc) == 48


def test_library_tables_equal_the_restatement():
    assert restatement_equals_pillow()
    lib = _lib()
    axes = sorted({(a, b) for W, H, w, h in RESIZE_CASES for a, b in ((W, w), (H, h))})
    for n_in, n_out in axes:
        for code, filt in enumerate(("bicubic", "bilinear")):
            ks, bounds, kk = lib_coeffs(lib, n_in, n_out, code)
            want = coeffs(n_in, n_out, filt)
            assert ks == want[0] and np.array_equal(bounds, want[1]) and np.array_equal(kk, want[2]), (n_in, n_out, filt)
    # limits are refused by name, buffers that are too small are not written
    ks = ctypes.c_int(0)
    assert lib.gl_image_resample_coeffs(16385, 224, 0, ctypes.byref(ks), None, 0, None, 0) != 0 and b"16384" in lib.gl_last_error()
    assert lib.gl_image_resample_coeffs(640, 298, 2, ctypes.byref(ks), None, 0, None, 0) != 0 and b"bilinear" in lib.gl_last_error()
    small = np.zeros(4, np.int32)
    assert lib.gl_image_resample_coeffs(640, 298, 0, ctypes.byref(ks), small.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 4, None, 0) != 0
    assert not small.any()


# ---- the chain against the processor ------------------------------------------------------------------------------------------------
def assert_pixel_values_equal(got, want, what):
    """Bit equality; should a transformers release order its float operations differently, 1e-6 absolute: four float32 ulps at the
    largest magnitude (2.15) and 14 000 times less than the spacing of adjacent u8 levels (1.4e-2) -- one wrong byte still fails."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    import transformers
    worst = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what}: not bit-equal to transformers {transformers.__version__}'s processor, max abs difference {worst:.3e}")
    assert worst <= 1e-6, (what, worst)


@functools.lru_cache(maxsize=None)
def processor_pixel_values():
    """transformers.CLIPImageProcessor() on the CHAIN_SIZES images and on the 256-level image, computed once."""
    import transformers
    from PIL import Image
    proc = transformers.CLIPImageProcessor()
    imgs = [Image.fromarray(image(w, h, 100 + i)) for i, (w, h) in enumerate(CHAIN_SIZES)]
    out = proc(images=imgs, return_tensors="np")["pixel_values"]
    levels = np.repeat(np.arange(256, dtype=np.uint8), 196).reshape(224, 224, 1).repeat(3, 2)
    return out, levels, proc(images=[Image.fromarray(levels)], return_tensors="np")["pixel_values"][0]


def test_restated_chain_equals_clip_image_processor():
    assert restatement_equals_pillow()
    want, levels, want_levels = processor_pixel_values()
    for i, (w, h) in enumerate(CHAIN_SIZES):
        u8, px = clip_chain(image(w, h, 100 + i), 224, 224, CLIP_MEAN, CLIP_STD)
        assert_pixel_values_equal(px, want[i], f"{w}x{h}")
    u8, px = clip_chain(levels, 224, 224, CLIP_MEAN, CLIP_STD)
    assert np.array_equal(u8, levels) and len(np.unique(u8)) == 256
    assert_pixel_values_equal(px, want_levels, "all 256 levels")
    from gligen_amd.engine import clip_resize_size, normalise_lut
    assert np.array_equal(normalise_lut(CLIP_MEAN, CLIP_STD), lut(CLIP_MEAN, CLIP_STD))
    assert all(clip_resize_size(w, h, 224) == clip_size(w, h, 224) for w, h in CHAIN_SIZES) and clip_resize_size(4000, 225, 224) == (3982, 224)


# ---- settings reader and host wiring -------------------------------------------------------------------------------------------------
class _Processor:
    def __init__(self, image_processor):
        self.image_processor = image_processor
        self.calls = 0

    def __call__(self, images=None, **kw):
        self.calls += 1
        return self.image_processor(images=images, return_tensors="pt")


class _NativeVision:
    """Stands where the engine stands and offers the native front end; neither method may be reached by a refused call."""
    clip_vision_cfg = dict(image_size=224)

    def clip_vision_preprocess(self, *a, **k):
        raise AssertionError("the device must not be touched")

    clip_vision_encode = clip_vision_preprocess


def test_settings_reader_accepts_the_default_and_names_what_it_refuses(tmp_path):
    import transformers
    import gligen_inference as gi
    from gligen_amd.runtime import clip_preprocess_settings
    s = clip_preprocess_settings(transformers.CLIPImageProcessor(), 224)
    assert s == dict(size=224, crop=224, mean=CLIP_MEAN, std=CLIP_STD, filter="bicubic")
    assert clip_preprocess_settings(transformers.CLIPImageProcessor(resample=2, image_mean=[0.5, 0.4, 0.3]))["filter"] == "bilinear"
    from PIL import Image
    Image.fromarray(image(40, 30, 0)).save(tmp_path / "a.png")
    refused = [("do_center_crop", dict(do_center_crop=False)), ("resample", dict(resample=Image.LANCZOS)),
               ("size", dict(size=dict(height=224, width=224))), ("rescale_factor", dict(rescale_factor=1 / 256)),
               ("crop_size", dict(crop_size=dict(height=224, width=200))), ("do_normalize", dict(do_normalize=False))]
    for field, kw in refused:
        with pytest.raises(NotImplementedError, match=r"\b" + field + r"\b"):
            gi.get_clip_image_features(None, _Processor(transformers.CLIPImageProcessor(**kw)), [str(tmp_path / "a.png")], _NativeVision(), preprocess="native")
        with pytest.raises(NotImplementedError, match=r"\b" + field + r"\b"):
            gi.get_clip_feature(None, _Processor(transformers.CLIPImageProcessor(**kw)), str(tmp_path / "a.png"), is_image=True, vision=_NativeVision(),
                                preprocess="native")
    with pytest.raises(NotImplementedError, match="crop_size"):      # not the tower's image_size
        clip_preprocess_settings(transformers.CLIPImageProcessor(crop_size=dict(height=192, width=192)), 224)
    with pytest.raises(ValueError, match="preprocess"):
        gi.get_clip_image_features(None, None, [], _NativeVision(), preprocess="gpu")


class _PlainVision:
    """A stand-in without clip_vision_preprocess (as tests/test_clip_vision_cpu.py's spy and tools/clip_bench.py's stand-ins)."""
    def __init__(self):
        self.seen = []

    def clip_vision_encode(self, pixel_values):
        self.seen.append(pixel_values)
        return None, None, pixel_values.float().mean(dim=(1, 2, 3))[:, None] + torch.arange(768, dtype=torch.float32)[None] / 768


def test_auto_falls_back_to_the_processor_and_native_is_what_auto_uses(tmp_path, monkeypatch):
    import transformers
    import gligen_inference as gi
    from PIL import Image
    assert restatement_equals_pillow()
    monkeypatch.chdir(tmp_path)
    torch.save(torch.eye(768), tmp_path / "projection_matrix")
    a = image(97, 61, 3)
    Image.fromarray(a).save(tmp_path / "a.png")
    proc, plain = _Processor(transformers.CLIPImageProcessor()), _PlainVision()
    f_auto = gi.get_clip_image_features(None, proc, [str(tmp_path / "a.png")], plain)          # preprocess="auto" is the default
    assert proc.calls == 1 and len(plain.seen) == 1
    with pytest.raises(NotImplementedError, match="clip_vision_preprocess"):
        gi.get_clip_image_features(None, proc, [str(tmp_path / "a.png")], plain, preprocess="native")
    assert proc.calls == 1
    # unsupported settings: "auto" calls the processor as well, although the engine offers the native front end
    odd = _Processor(transformers.CLIPImageProcessor(resample=Image.LANCZOS))

    class Both(_PlainVision):
        clip_vision_cfg = dict(image_size=224)

        def clip_vision_preprocess(self, images, size, crop, mean, std, filter):
            self.native = (len(images), size, crop, filter)
            return torch.from_numpy(np.stack([clip_chain(im, size, crop, mean, std, filter)[1] for im in images]))

    both = Both()
    gi.get_clip_image_features(None, odd, [str(tmp_path / "a.png")], both)
    assert odd.calls == 1 and not hasattr(both, "native")
    # supported settings + an engine with the front end: the processor is not called, and the features are the same bits
    f_native = gi.get_clip_image_features(None, proc, [None, str(tmp_path / "a.png")], both)
    assert proc.calls == 1 and both.native == (1, 224, 224, "bicubic") and f_native[0] is None
    assert_pixel_values_equal(both.seen[-1].numpy(), plain.seen[0].numpy(), "native stand-in")
    assert torch.equal(f_native[1], f_auto[0])
    gi.get_clip_image_features(None, proc, [str(tmp_path / "a.png")], both, preprocess="processor")
    assert proc.calls == 2


# ---- ISA ------------------------------------------------------------------------------------------------------------------------
def test_image_kernels_use_no_scratch(tmp_path):
    from gligen_amd.build import EXTRA_FLAGS, SOURCES
    assert "image.hip" in SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "image.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *EXTRA_FLAGS.get("image.hip", []), "-I", os.path.join(ROOT, "include"),
                        "--offload-device-only", "-S", os.path.join(ROOT, "gligen_amd", "csrc", "image.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    kernels = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])[1:]
    names = [re.search(r"\.name:\s*(\S+)", e).group(1) for e in kernels]
    assert len(kernels) == 3 and sum("image_resample_h_kernel" in n for n in names) == 1 and sum("image_resample_v_kernel" in n for n in names) == 2, names
    for e in kernels:
        val = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", e).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0
        assert val("max_flat_workgroup_size") == 256 and val("vgpr_count") <= 64
