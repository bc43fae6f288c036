"""Training the semantic-map model from u8 class maps, host side, no GPU: the entry points of include/gligen_amd_train_maps.h are
declared, exported and bound; the new input struct has one size in C and in ctypes; the guidance drop of a class-map batch is
"no class" (255), not class 0."""
import ctypes
import os
import re
import shutil
import subprocess

import torch

from helpers import ROOT
from gligen_amd.train import null_grounding


def _declared(header):
    return set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_train_map_entry_points_are_declared_exported_and_bound():
    """Each maps header declares exactly the names of its ctypes table, the built library exports them with the table's argument
    types, and the tables share no name with one another or with the other headers."""
    from gligen_amd import _lib as table
    from gligen_amd.build import build_native
    build_native()
    lib = table.load()
    assert _declared("gligen_amd_maps.h") == set(table.MAP_SYMBOLS)
    declared = _declared("gligen_amd_train_maps.h")
    assert declared == set(table.TRAIN_MAP_SYMBOLS) == {"gl_unet_train_step_spatial_classes", "gl_op_class_conv_wgrad"}
    raw = ctypes.CDLL(str(table.LIB_PATH))
    for name in declared | set(table.MAP_SYMBOLS):
        assert hasattr(raw, name), f"{name} is declared but not exported"
    assert all(getattr(lib, n).argtypes == table.TRAIN_MAP_SYMBOLS[n][1] for n in declared)
    assert not declared & (set(table.SYMBOLS) | set(table.IMAGE_SYMBOLS) | set(table.MAP_SYMBOLS))
    for other in ("gligen_amd.h", "gligen_amd_image.h", "gligen_amd_maps.h"):
        assert not declared & set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read())), other
    # the planes entry point and its struct stay where they were
    assert "gl_unet_train_step_spatial" in table.SYMBOLS and "gl_unet_train_step_spatial" not in declared


def test_ctypes_train_spatial_classes_in_matches_the_c_header(tmp_path):
    """gl_train_spatial_classes_in: the same size from gcc (C99) and from ctypes, and the fields at the same offsets."""
    from gligen_amd import _lib
    fields = [n for n, _ in _lib.TrainSpatialClassesIn._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gligen_amd_train_maps.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(gl_train_spatial_classes_in));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(gl_train_spatial_classes_in, {n}));\n' for n in fields) + "  return 0;\n}\n")
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.TrainSpatialClassesIn) == 56
    assert out[1:] == [getattr(_lib.TrainSpatialClassesIn, n).offset for n in fields]


def test_null_grounding_of_a_class_map_is_no_class():
    """The guidance drop of a batch whose `sem` is a u8 class map: 255 in every pixel (zeros would be class 0 everywhere), mask 0,
    grounding_extra_input kept. A float batch is zeroed as before."""
    B = 2
    cls = torch.randint(0, 152, (B, 1, 16, 16), generator=torch.Generator().manual_seed(1)).to(torch.uint8)
    batch = dict(sem=cls, mask=torch.ones(B, 1), grounding_extra_input=cls.clone(), x=torch.randn(B, 4, 8, 8), timesteps=torch.tensor([981.0, 441.0]))
    nb = null_grounding(batch)
    assert nb["sem"].dtype == torch.uint8 and nb["sem"].shape == cls.shape and bool((nb["sem"] == 255).all())
    assert nb["mask"].dtype == torch.float32 and torch.count_nonzero(nb["mask"]) == 0
    for k in ("grounding_extra_input", "x", "timesteps"):
        assert torch.equal(nb[k], batch[k])
    assert torch.equal(batch["sem"], cls)                                   # the caller's batch is not written
    nb3 = null_grounding(dict(batch, sem=cls[:, 0]))                        # [B, H, W]
    assert nb3["sem"].dtype == torch.uint8 and tuple(nb3["sem"].shape) == (B, 16, 16) and bool((nb3["sem"] == 255).all())
    planes = dict(batch, sem=torch.rand(B, 152, 16, 16) + 0.1, grounding_extra_input=torch.rand(B, 152, 16, 16))
    nf = null_grounding(planes)
    assert nf["sem"].dtype == torch.float32 and torch.count_nonzero(nf["sem"]) == 0 and torch.count_nonzero(nf["mask"]) == 0
    assert torch.equal(nf["grounding_extra_input"], planes["grounding_extra_input"])
    assert "255" in null_grounding.__doc__                                  # the docstring says what a class map becomes
