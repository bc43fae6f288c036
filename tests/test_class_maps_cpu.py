"""Semantic maps as class indices without a GPU: the header / exports / ctypes table of include/gligen_amd_maps.h, a numpy restatement
of Pillow's nearest index table (checked against the installed Pillow before anything is compared with it), the library's table,
the unchanged host paths of gligen_inference's batch builders, and the kernels' ISA facts."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (width, height) of the class maps; each is centre-cropped as prepare_batch_sem crops and resized to 512 x 512
SIZES = [(640, 480), (333, 500), (512, 512), (1024, 768), (37, 211), (4000, 3001), (2, 3), (683, 1025), (1500, 997)]


def centre_box(w, h):
    """(x, y, side, side): the square crop_and_resize / prepare_batch_sem cut (reference gligen_inference.py:189-193)."""
    c = min(w, h)
    return int(round((w - c) / 2.0)), int(round((h - c) / 2.0)), c, c


def index_table(box0, box_len, out):
    """Pillow's nearest path along one axis (ImagingScaleAffine): the source sample of each resized sample, accumulated in double."""
    a = box_len / out
    xo = a * 0.5
    t = np.empty(out, np.int32)
    for x in range(out):
        t[x] = box0 + int(xo)
        xo += a
    return t


def nearest(a, box, w, h):
    """PIL.Image.crop(box).resize((w, h), Image.NEAREST) of u8 [H, W], restated."""
    x, y, bw, bh = box
    return np.ascontiguousarray(a[index_table(y, bh, h)][:, index_table(x, bw, w)])


def class_map(w, h, seed, top=152):
    """Seeded per-pixel random classes 0 .. top - 1: neighbouring samples differ, so one wrong index shows."""
    return np.random.RandomState(seed).randint(0, top, (h, w), dtype=np.uint8)


def pillow_nearest(a, box, w, h):
    from PIL import Image
    x, y, bw, bh = box
    return np.asarray(Image.fromarray(a).crop((x, y, x + bw, y + bh)).resize((w, h), Image.NEAREST))


@functools.lru_cache(maxsize=None)
def restatement_equals_pillow():
    """Asserted first by every test that compares something with the restatement."""
    import PIL
    for i, (w, h) in enumerate(SIZES):
        a = class_map(w, h, i)
        bad = int((nearest(a, centre_box(w, h), 512, 512) != pillow_nearest(a, centre_box(w, h), 512, 512)).sum())
        assert bad == 0, f"restatement != Pillow {PIL.__version__}: {w}x{h} -> 512x512 nearest: {bad} bytes differ"
    a = class_map(97, 61, 50)          # off-centre box, unequal sides, both directions of scaling
    assert np.array_equal(nearest(a, (5, 7, 60, 40), 64, 48), pillow_nearest(a, (5, 7, 60, 40), 64, 48))
    assert np.array_equal(nearest(a, (30, 2, 11, 57), 48, 19), pillow_nearest(a, (30, 2, 11, 57), 48, 19))
    return True


def test_restatement_is_pillow_byte_for_byte():
    assert restatement_equals_pillow()
    # the cases reach both directions: up (2 -> 512), down by a ratio that is no integer (3001 -> 512), and a copy (512 -> 512)
    assert np.array_equal(index_table(0, 512, 512), np.arange(512)) and index_table(0, 2, 512).max() == 1 and index_table(0, 3001, 512)[-1] == 2998


def _lib():
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    return _lib.load()


def lib_table(lib, box0, box_len, out, cap=None):
    t = np.full(out if cap is None else cap, -7, np.int32)
    rc = lib.gl_class_map_index_table(box0, box_len, out, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), t.size)
    return rc, t


def test_map_entry_points_are_declared_exported_and_bound(tmp_path):
    """include/gligen_amd_maps.h, the library's exports and the ctypes table agree and share nothing with the other two headers;
    gl_class_map_desc has the size ctypes gives it."""
    lib = _lib()
    from gligen_amd import _lib as table
    header = open(os.path.join(ROOT, "include", "gligen_amd_maps.h")).read()
    declared = set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", header))
    assert declared == set(table.MAP_SYMBOLS) == {"gl_op_class_map_resize", "gl_class_map_index_table", "gl_op_spatial_tokens_classes",
                                                  "gl_op_grounding_downsample_classes"}
    assert not declared & set(table.SYMBOLS) and not declared & set(table.IMAGE_SYMBOLS)
    assert all(hasattr(lib, n) and getattr(lib, n).argtypes == table.MAP_SYMBOLS[n][1] for n in declared)
    for other in ("gligen_amd.h", "gligen_amd_image.h"):
        assert not declared & set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read())), other
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gligen_amd_maps.h"\nint main(void) { printf("%zu\\n", sizeof(gl_class_map_desc)); return 0; }\n')
    subprocess.run([shutil.which("gcc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout
    assert int(out) == ctypes.sizeof(table.ClassMapDesc) == 40


def test_library_index_table_equals_the_restatement():
    assert restatement_equals_pillow()
    lib = _lib()
    axes = sorted({(b0, bl, 512) for w, h in SIZES for b0, bl in (centre_box(w, h)[0::2], centre_box(w, h)[1::2])})
    axes += [(5, 60, 64), (7, 40, 48), (30, 11, 48), (2, 57, 19), (16383, 1, 7), (0, 16384, 16384)]      # off-centre boxes, the limits
    for box0, box_len, out in axes:
        rc, t = lib_table(lib, box0, box_len, out)
        assert rc == 0, lib.gl_last_error()
        assert np.array_equal(t, index_table(box0, box_len, out)), (box0, box_len, out)
        assert t.min() >= box0 and t.max() < box0 + box_len
    # limits are refused by name, a buffer that is too small is not written
    rc, t = lib_table(lib, 0, 16385, 512)
    assert rc != 0 and b"16384" in lib.gl_last_error() and (t == -7).all()
    rc, t = lib_table(lib, 1, 16384, 512)
    assert rc != 0 and b"16384" in lib.gl_last_error() and (t == -7).all()
    rc, t = lib_table(lib, 0, 640, 16385, cap=16385)
    assert rc != 0 and b"16384" in lib.gl_last_error() and (t == -7).all()
    rc, t = lib_table(lib, 0, 640, 0, cap=4)
    assert rc != 0 and (t == -7).all()
    rc, t = lib_table(lib, 0, 640, 512, cap=511)
    assert rc != 0 and b"512" in lib.gl_last_error() and (t == -7).all()
    assert lib.gl_class_map_index_table(0, 640, 512, None, 512) != 0


def test_host_batch_builders_are_unchanged(tmp_path, monkeypatch):
    """prepare_batch_sem / prepare_batch_canny without `native` return what they returned before the native inputs: the planes and the
    map computed here with Pillow and torch as the reference's prepare_batch_* compute them."""
    from PIL import Image
    import gligen_inference as gi
    monkeypatch.setattr(gi, "device", "cpu")
    assert restatement_equals_pillow()
    a = class_map(333, 500, 7)
    Image.fromarray(a).save(tmp_path / "sem.png")
    out = gi.prepare_batch_sem(dict(sem=str(tmp_path / "sem.png")), 2)
    assert set(out) == {"sem", "mask"} and out["sem"].dtype == torch.float32 and tuple(out["sem"].shape) == (2, 152, 512, 512)
    want = torch.from_numpy(nearest(a, centre_box(333, 500), 512, 512)).long()
    assert torch.equal(out["sem"][1].argmax(0), want) and torch.equal(out["sem"].sum(1), torch.ones(2, 512, 512))
    assert torch.equal(out["sem"][0], out["sem"][1]) and torch.equal(out["mask"], torch.ones(2, 1))
    rgb = np.random.RandomState(8).randint(0, 256, (480, 640, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "canny.png")
    out = gi.prepare_batch_canny(dict(canny_image=str(tmp_path / "canny.png")), 2)
    im = Image.open(tmp_path / "canny.png").convert("RGB").crop((80, 0, 560, 480)).resize((512, 512))
    want = (torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).float() / 255 - 0.5) / 0.5
    assert set(out) == {"canny_edge", "mask"} and torch.equal(out["canny_edge"], want.unsqueeze(0).repeat(2, 1, 1, 1)) and torch.equal(out["mask"], torch.ones(2, 1))
    # the table the native path hands to Engine.image_resample holds what the host expression makes of every u8 level
    levels = torch.arange(256, dtype=torch.uint8)
    assert np.array_equal(gi._unit_lut(), gi._pil_to_unit_tensor(levels.numpy()[None].repeat(3, 0).T.reshape(256, 1, 3)).reshape(3, 256).numpy())
    # a class value outside the 152 classes is refused by name before any device is touched
    bad = a.copy()
    bad[10, 10] = 200
    Image.fromarray(bad).save(tmp_path / "bad.png")
    with pytest.raises(ValueError, match=r"\b200\b"):
        gi.prepare_batch_sem(dict(sem=str(tmp_path / "bad.png")), 2, native=True)


def test_null_input_of_a_class_map_is_no_class():
    from grounding_input.sem_grounding_tokinzer_input import GroundingNetInput
    gin = GroundingNetInput()
    gin.prepare({"sem": torch.zeros(2, 1, 8, 8, dtype=torch.uint8), "mask": torch.ones(2, 1)})
    null = gin.get_null_input()
    assert null["sem"].dtype == torch.uint8 and tuple(null["sem"].shape) == (2, 1, 8, 8) and bool((null["sem"] == 255).all())
    assert null["mask"].dtype == torch.float32 and not null["mask"].any()
    gin.prepare({"sem": torch.ones(2, 152, 8, 8), "mask": torch.ones(2, 1)})          # the float case is as it was
    null = gin.get_null_input()
    assert null["sem"].dtype == torch.float32 and tuple(null["sem"].shape) == (2, 152, 8, 8) and not null["sem"].any() and not null["mask"].any()


def test_class_map_kernels_use_no_scratch(tmp_path):
    from gligen_amd.build import EXTRA_FLAGS, SOURCES
    assert "classmap.hip" in SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "classmap.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *EXTRA_FLAGS.get("classmap.hip", []), "-I", os.path.join(ROOT, "include"),
                        "--offload-device-only", "-S", os.path.join(ROOT, "gligen_amd", "csrc", "classmap.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    kernels = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])[1:]
    names = [re.search(r"\.name:\s*(\S+)", e).group(1) for e in kernels]
    for k in ("class_map_resize_kernel", "class_inconv_kernel", "class_conv4x4s2_kernel"):
        assert sum(k in n for n in names) == 1, (k, names)
    for e in kernels:
        val = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", e).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0, e[:300]
        assert val("vgpr_count") <= 64          # 8 waves per SIMD
