"""Nearest-2x upsample + 3x3 conv as four 2x2 phase convs (gemm.h A_CONV2UP; reference openaimodel.py:54-82, VAE model.py:42-57).

After the replication, output pixel (2y + py, 2x + px) reads two source rows and two source columns, so the layer is four 2x2 convs on
the SOURCE whose filters are fixed sums of the 3x3 filter's taps: 4/9 of the multiply-adds. `engine.op_conv3x3(..., ups=1)` takes that
form; GL_UPCONV_PHASES=0 restores the nine-tap loader.

* exactness: small-integer data for which every folded weight, product and fp32 partial sum is exact in either form, so the output
  must be bit-equal to the fp32 reference rounded to bf16 -- indexing, padding and phase-mapping mistakes have no tolerance to hide behind;
* random data against the bf16-tap reference of tests/test_ops_gpu.py at that file's tolerance (the CPU model of the fold predicts 3.3e-3);
* both forms against each other (a subprocess runs the nine-tap form);
* the fold itself, in fp64 on the CPU, as an executable specification."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

TOL = 1.2e-2       # tests/test_ops_gpu.py: relative to the reference's max magnitude; bf16 output rounding alone is 2^-8 = 3.9e-3

# (B, H, W, C0, C1, Cout)
EXACT_SHAPES = [
    (3, 2, 3, 64, 0, 64),          # every tap of some pixel is padding; 18 rows per phase
    (2, 6, 10, 64, 0, 96),         # non-square, row and column tails in every phase
    (2, 8, 8, 64, 0, 128),         # the shape of test_ops_gpu.py::test_conv3x3's ups case
    (1, 64, 64, 128, 0, 128),      # many tiles per phase, K = 512: eight K tiles, the shallow end
    (8, 8, 8, 1280, 0, 1280),      # the workload's split-K site
    (2, 8, 8, 64, 64, 64),         # two sources
]
RANDOM_SHAPES = [EXACT_SHAPES[0], EXACT_SHAPES[1], EXACT_SHAPES[4]]


def rel_err(y, ref):
    y, ref = y.float(), ref.float()
    return ((y - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bf(t):
    return t.to(torch.bfloat16)


def conv_ref(x_nhwc, w, b):
    """nearest-2x upsample, then the 3x3 / pad 1 conv with every tap rounded to bf16 (tests/test_ops_gpu.py conv_ref, ups = 1)"""
    x = F.interpolate(x_nhwc.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    return F.conv2d(x, bf(w).float(), b, padding=1).permute(0, 2, 3, 1)


def random_case(shape):
    B, H, W, C0, C1, Cout = shape
    x = bf(rnd(B, H, W, C0 + C1, seed=1))
    w = rnd(Cout, C0 + C1, 3, 3, scale=(9 * (C0 + C1)) ** -0.5, seed=3)
    return x, w, rnd(Cout, seed=4)


def run_op(engine, shape, x, w, b):
    C0, C1 = shape[3], shape[4]
    xc = x.cuda()
    x0 = xc[..., :C0].contiguous()
    x1 = xc[..., C0:].contiguous() if C1 else None
    return engine.op_conv3x3(x0, w.cuda(), b.cuda(), x1=x1, ups=1).cpu()


# ---- the fold, as an executable specification (CPU)
# ROW_FOLD[py][a][ky] = 1 where filter row ky of output phase py reads source row (y - 1 + py + a); columns alike with px, kx
ROW_FOLD = torch.tensor([[[1, 0, 0], [0, 1, 1]],
                         [[1, 1, 0], [0, 0, 1]]], dtype=torch.float64)


def fold_filters(w):
    """[O][I][3][3] -> [py][px][O][I][a][b]: the four 2x2 filters"""
    return torch.einsum("pak,qbl,oikl->pqoiab", ROW_FOLD, ROW_FOLD, w.double())


def phase_form(x_nchw, w, b):
    """the layer as four 2x2 convs on the source: phase (py, px) reads source rows y - 1 + py, y + py and columns x - 1 + px, x + px"""
    Bn, _, H, W = x_nchw.shape
    w4 = fold_filters(w)
    y = torch.zeros(Bn, w.shape[0], 2 * H, 2 * W, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            xp = F.pad(x_nchw.double(), (1 - px, px, 1 - py, py))      # (left, right, top, bottom): zero padding carries over unchanged
            y[:, :, py::2, px::2] = F.conv2d(xp, w4[py, px], b.double())
    return y


@pytest.mark.parametrize("B,H,W", [(2, 3, 5), (1, 1, 1)])
def test_fold_is_exact_in_fp64(B, H, W):
    C, O = 3, 2
    x, w, b = rnd(B, C, H, W, seed=1).double(), rnd(O, C, 3, 3, seed=2).double(), rnd(O, seed=3).double()
    # data on a coarse binary grid: every sum of either form is then exact in fp64 and the two must agree to 0, not to an ulp
    x, w, b = (x * 64).round() / 64, (w * 64).round() / 64, (b * 64).round() / 64
    nine = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    assert torch.equal(phase_form(x, w, b), nine)


# ---- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upconv_exact(engine, shape):
    B, H, W, C0, C1, Cout = shape
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-2, 3, (B, H, W, C0 + C1), generator=g).to(torch.bfloat16)
    w = torch.randint(-1, 2, (Cout, C0 + C1, 3, 3), generator=g).float() * 2.0 ** -3
    b = torch.randint(-8, 9, (Cout,), generator=g).float() * 2.0 ** -3
    ref = F.conv2d(F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), w, b, padding=1).permute(0, 2, 3, 1)
    y = run_op(engine, shape, x, w, b)
    assert y.shape == ref.shape
    assert torch.equal(y, ref.to(torch.bfloat16)), f"max |diff| {(y.float() - ref).abs().max().item()}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upconv_random(engine, shape):
    x, w, b = random_case(shape)
    err = rel_err(run_op(engine, shape, x, w, b), conv_ref(x, w, b))
    print(f"phase form vs bf16-tap reference {shape}: {err:.3e}")
    assert err < TOL


_NINE_TAP_SNIPPET = r"""
import sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from gligen_amd.engine import Engine
import test_upconv_phases_gpu as t
eng = Engine(0, arena_gb=1.0)
torch.save([t.run_op(eng, s, *t.random_case(s)) for s in t.RANDOM_SHAPES], %r)
"""


@pytest.mark.gpu
def test_upconv_both_forms_agree(engine, tmp_path):
    """GL_UPCONV_PHASES=0 runs the nine-tap form (read once per process, hence the subprocess); the forms differ by rounding only."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "nine_tap.pt")
    env = dict(os.environ, GL_DEV_SWITCHES="1", GL_UPCONV_PHASES="0")
    r = subprocess.run([sys.executable, "-c", _NINE_TAP_SNIPPET % (os.path.dirname(here), here, out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for shape, nine in zip(RANDOM_SHAPES, torch.load(out)):
        err = rel_err(run_op(engine, shape, *random_case(shape)), nine)
        print(f"phase form vs nine-tap form {shape}: {err:.3e}")
        assert err < TOL
