"""Every softmax-stabiliser regime of the attention kernels at benchmark sizes, against a float64 reference.

attn3_kernel at d = 40 holds the only data-dependent control flow on the hot path: the stabiliser is the first tile's maximum, then
follows the running denominator two tiles late (the lazy move, at l > 2^40), and a workgroup whose denominator leaves (0, 1e30) or
goes non-finite runs all its tiles again with the exact per-tile maximum. The inputs come from helpers.spike_attention_case (a
rank-one bump in a reserved channel: chosen rows jump by a chosen number of log2 units at a chosen key, every other row is left
alone; tests/test_host_cpu.py checks from the float64 scores that each case sits in its regime's band), and the regime that ran is
read from the kernel's counters (Engine.attn_regime_counters), not inferred from the output.

Bars (those of test_ops_gpu.test_attention): max |y - ref| over all rows / max |ref| over the ordinary rows < 2.5e-2, mean |y - ref|
/ mean |ref| < 1e-2; per bumped row, max |y - ref| / the row's own max |ref| < 2.5e-2; every output finite; the same bits twice.

Counters at d = 40 (a workgroup is one (sample, head, 128-query block)):
  quiet data                                      lazy_moves == 0, reruns == 0
  lazy jump at a tile in 1 .. nt - 3              lazy_moves >= 1, reruns == 0
  any jump in tile 0                              reruns == 0 (the first tile's maximum absorbs it)
  lazy jump in the last two tiles                 reruns == 0
  finite-overshoot / overflow jump at a tile >= 1 reruns == the number of workgroups that hold such a row, exactly
d = 80 (no lazy path: the exact maximum every tile) and the other kernels: counters stay 0 / parity alone.

Measured on MI355X (100 tests, 11 s): tile 0 -> (lazy_moves, reruns) = (0, 0) for every size; a lazy jump in tiles 1 .. nt - 2 -> (1, 0)
(the drain iteration still sees tile nt - 2), in tile nt - 1 -> (0, 0); a hot jump -> (1, 1) up to tile nt - 2, (0, 1) in tile nt - 1;
staircase_50 (10, 0), staircase_150 (1, 1), common_minus_200 (0, 0), minus_200_on_tile0 (2, 2), four_regimes_one_block (3, 1),
four_regimes_spread (2, 2), the two-sample case (5, 4), quiet data (0, 0). Worst max_rel / mean_rel / row_rel: attn3 d = 40 4.8e-3 /
2.6e-3 / 5.3e-3 (overflow rows 3.4e-3), attn3 d = 80 4.7e-3 / 2.1e-3 / 3.1e-3, attn_kernel at 77 keys 4.9e-3 / 3.0e-3 / 3.1e-3, d = 160
4.3e-3 / 1.8e-3 / 3.1e-3, GL_ATTN_V2 = 0 / 1 / 2 4.8e-3 / 2.6e-3 / 2.6e-3 each.
Mutation check (scratch builds): with the rerun branch disabled every overshoot / overflow case of test_d40_grid at a tile >= 1 fails
(22), with test_d40_rerun_count_over_samples and the composites staircase_150, minus_200_on_tile0, four_regimes_one_block and
four_regimes_spread; without the `sc -= delta` of the lazy move every lazy case of test_d40_grid whose move runs fails (tile1, mid and
before_last_full at all three shapes that have them, last_full at 4126 keys: 8), with two_bumps_large_then_small, staircase_50 and
four_regimes_spread. No other d = 40 test of this file fails under either."""
import os
import subprocess
import sys
import time

import pytest
import torch

import helpers
from helpers import SPIKE_UNITS as U

pytestmark = pytest.mark.gpu

H = 8
MAX_BAR, MEAN_BAR, ROW_BAR = 2.5e-2, 1e-2, 2.5e-2
HOT = ("overshoot", "overflow")          # regimes that must send their workgroup through the rerun


def check_parity(m, what):
    print(f"[regimes] {what}: max_rel={m['max_rel']:.3e} mean_rel={m['mean_rel']:.3e} row_rel={m['row_rel']:.3e}")
    assert m["finite"], what
    assert m["max_rel"] < MAX_BAR, (what, m)
    assert m["mean_rel"] < MEAN_BAR, (what, m)
    assert m["row_rel"] < ROW_BAR, (what, m)


def run_counted(engine, case, what):
    """op_attention with the counters on, then once more with them off (the production instantiation): parity of the first, the same
    bits from the second. Returns (lazy_moves, reruns)."""
    engine.attn_regime_counters(True)
    y = engine.op_attention(case.xq, case.xkv, case.wq, case.wk, case.wv, case.H)
    lazy, reruns = engine.attn_regime_counters(False)
    y2 = engine.op_attention(case.xq, case.xkv, case.wq, case.wk, case.wv, case.H)
    assert engine.attn_regime_counters(False) == (0, 0)         # nothing counts while the switch is off
    print(f"[regimes] {what}: lazy_moves={lazy} reruns={reruns}")
    check_parity(helpers.spike_attention_metrics(case, y), what)
    assert torch.equal(y, y2), "two runs of the same case differ"
    return lazy, reruns


def hot_workgroups(entries):
    """entries: [(sample, head, rows, regime, tile)] -> the (sample, head, query block) triples that must rerun."""
    return {(b, h, r // 128) for b, h, rows, regime, tile in entries if regime in HOT and tile >= 1 for r in rows}


@pytest.mark.parametrize("name,shape,regime,pname,tile,bumps", [pytest.param(*g, id=g[0]) for g in helpers.spike_grid(40)])
def test_d40_grid(engine, name, shape, regime, pname, tile, bumps):
    B, Nq, Nk, C = shape
    nt = (Nk + 63) // 64
    case = helpers.spike_attention_case(B, Nq, Nk, C, H, bumps, device="cuda")
    lazy, reruns = run_counted(engine, case, f"{name} (tile {tile} of {nt})")
    if tile == 0:
        assert reruns == 0, (lazy, reruns)
    elif regime == "lazy":
        assert reruns == 0, (lazy, reruns)
        if tile <= nt - 3:
            assert lazy >= 1, (lazy, reruns)
    else:
        assert reruns == 1, (lazy, reruns)


@pytest.mark.parametrize("name,shape,regime,pname,tile,bumps", [pytest.param(*g, id=g[0]) for g in helpers.spike_grid(80)])
def test_d80_grid(engine, name, shape, regime, pname, tile, bumps):
    """attn3_kernel<80, 96, false, 4>: the stabiliser is subtracted in front of the exps and moves with the exact per-tile maximum --
    no lazy path, no rerun: the counters stay 0 and parity decides (the existing spike test stops at gain 6, ~55 units)."""
    B, Nq, Nk, C = shape
    case = helpers.spike_attention_case(B, Nq, Nk, C, H, bumps, device="cuda")
    lazy, reruns = run_counted(engine, case, name)
    assert (lazy, reruns) == (0, 0)


@pytest.mark.parametrize("Nk", [4096, 4126])
def test_d40_quiet(engine, Nk):
    """No bump, and a bump that stays below the lazy threshold: neither regime runs (64 and 65 tiles)."""
    for bumps in ((), [(0, 2, [5, 700, 4000], {40 * 64 + 7: U["quiet"]})]):
        case = helpers.spike_attention_case(1, 4096, Nk, 320, H, bumps, device="cuda")
        lazy, reruns = run_counted(engine, case, f"quiet-{Nk}-{len(bumps)}-bumps")
        assert (lazy, reruns) == (0, 0)


def test_d40_rerun_count_over_samples(engine):
    """(2, 1000, 4126): a ragged query count (the last block holds 104 real rows and 24 of padding) and two samples, overflow rows in
    sample 1 only -- first block, a middle block and the ragged last block of one head, one more block of another head. Exactly those
    four workgroups rerun: a padded query, or sample 0, that reran would show as a fifth."""
    entries = [(1, 3, [5, 300, 990], "overflow", 31), (1, 6, [600, 610], "overshoot", 50)]
    bumps = [(1, 3, [5, 300, 990], {31 * 64 + 20: U["overflow"]}), (1, 6, [600, 610], {50 * 64 + 9: U["overshoot"]})]
    case = helpers.spike_attention_case(2, 1000, 4126, 320, H, bumps, device="cuda")
    lazy, reruns = run_counted(engine, case, "samples")
    assert reruns == len(hot_workgroups(entries)) == 4, (lazy, reruns)


K = lambda tile, off=11: 64 * tile + off      # noqa: E731  (a key inside a tile)
# name -> (bumps, expected lazy_moves (None: not asserted; ">=1"; 0), expected reruns)
COMPOSITES = {
    # two jumps of clearly different size in one row, both orders: the later, smaller one is 30 units below the first
    "two_bumps_large_then_small": ([(0, 1, [200], {K(10): U["lazy"], K(20): U["lazy"] - 30})], ">=1", 0),
    "two_bumps_small_then_large": ([(0, 1, [200], {K(10): U["lazy"] - 30, K(20): U["lazy"]})], ">=1", 0),
    # ten consecutive tiles, each 50 units above the last (the first 60 above the row's ordinary scores): a move per step, no rerun
    "staircase_50": ([(0, 4, [1000], {K(20 + i): 60.0 + 50.0 * i for i in range(10)})], ">=1", 0),
    # steps of 150 units: no move can keep up
    "staircase_150": ([(0, 4, [1000], {K(20 + i): 150.0 * (i + 1) for i in range(10)})], None, 1),
    # -200 units on every key of the row: the reference does not change, the first tile's maximum must take it
    "common_minus_200": ([(0, 5, [77, 2000], {(0, 4126): -200.0})], 0, 0),
    # -200 units on tile 0 only: the row's own scores are the jump, at tile 1
    "minus_200_on_tile0": ([(0, 5, [77, 2000], {(0, 64): -200.0})], None, 2),
    # all four regimes in one 128-query block of one head, one wave each (a = 16, 8, 4, 1 on one key: 236 / 118 / 59 / 14.75 units)
    "four_regimes_one_block": ([(0, 2, [1283], {K(31): 236.0}), (0, 2, [1315], {K(31): 236.0}, 8.0),
                                (0, 2, [1347], {K(31): 236.0}, 4.0), (0, 2, [1379], {K(31): 236.0}, 1.0)], ">=1", 1),
    # all four regimes over different blocks and heads
    "four_regimes_spread": ([(0, 1, [200], {K(5): U["lazy"]}), (0, 2, [1500], {K(40): U["overshoot"]}),
                             (0, 5, [3000], {4111: U["overflow"]}), (0, 7, [4000], {K(3): U["quiet"]})], ">=1", 2),
}


@pytest.mark.parametrize("name", list(COMPOSITES))
def test_d40_composites(engine, name):
    bumps, want_lazy, want_reruns = COMPOSITES[name]
    case = helpers.spike_attention_case(1, 4096, 4126, 320, H, bumps, device="cuda")
    lazy, reruns = run_counted(engine, case, name)
    assert reruns == want_reruns, (lazy, reruns)
    if want_lazy == ">=1":
        assert lazy >= 1, (lazy, reruns)
    elif want_lazy == 0:
        assert lazy == 0, (lazy, reruns)
    if name == "staircase_50":
        assert lazy >= 8, (lazy, reruns)           # ten steps, each beyond 2^40 over the last: "many moves" (the last two tiles' may go unseen)
    if name == "common_minus_200":
        plain = helpers.spike_attention_case(1, 4096, 4126, 320, H, (), device="cuda")
        assert float((case.ref - plain.ref).abs().max()) < 1e-9      # a bump common to all keys of a row cancels in the softmax


# ---- the other attention kernels: no counters, parity alone, same bars ------------------------------------------------------------
def other_kernel_cases():
    out = []
    # attn_kernel<48, 64> (77 keys: tile 1 is keys 64..76) and attn_kernel<80, 96> on the default route
    for B, Nq, C in ((8, 4096, 320), (1, 100, 320), (2, 1024, 640)):
        for key in (70, 20):
            for regime in ("lazy", "overflow"):
                out.append((f"d{C // H}-{B}x{Nq}x77-key{key}-{regime}", (B, Nq, 77, C), [(B - 1, 3, [37], {key: U[regime]})]))
    # attn_kernel<160, 160>: 2 tiles (94 keys) and 5 tiles (286 keys): first, middle and the ragged last tile
    for Nq, Nk, keys in ((64, 94, (20, 80)), (256, 286, (20, 150, 270))):
        for key in keys:
            for regime in ("lazy", "overflow"):
                out.append((f"d160-2x{Nq}x{Nk}-key{key}-{regime}", (2, Nq, Nk, 1280), [(1, 3, [37], {key: U[regime]})]))
    return out


@pytest.mark.parametrize("name,shape,bumps", [pytest.param(*c, id=c[0]) for c in other_kernel_cases()])
def test_other_kernels(engine, name, shape, bumps):
    B, Nq, Nk, C = shape
    case = helpers.spike_attention_case(B, Nq, Nk, C, H, bumps, device="cuda")
    lazy, reruns = run_counted(engine, case, name)
    assert (lazy, reruns) == (0, 0)


_SWITCH_SNIPPET = r"""
import sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import helpers
from gligen_amd.engine import Engine
eng = Engine(0, arena_gb=2.0)
worst = dict(max_rel=0.0, mean_rel=0.0, row_rel=0.0)
finite, same, n = True, True, 0
for name, shape, regime, pname, tile, bumps in helpers.spike_grid(40):
    B, Nq, Nk, C = shape
    if Nk != 4126 or regime == "overshoot":
        continue
    case = helpers.spike_attention_case(B, Nq, Nk, C, 8, bumps, device="cuda")
    y = eng.op_attention(case.xq, case.xkv, case.wq, case.wk, case.wv, 8)
    same = same and torch.equal(y, eng.op_attention(case.xq, case.xkv, case.wq, case.wk, case.wv, 8))
    m = helpers.spike_attention_metrics(case, y)
    print("CASE", name, m, file=sys.stderr)
    finite = finite and m["finite"]
    for k in worst:
        worst[k] = max(worst[k], m[k])
    n += 1
print("WORST", n, int(finite), int(same), worst["max_rel"], worst["mean_rel"], worst["row_rel"])
"""


def test_d40_switched_kernels():
    """The d = 40 position grid at 4126 keys (lazy- and overflow-size bumps) through the kernels the developer switch GL_ATTN_V2 selects:
    0 = attn_kernel<48, 64> for every key count, 1 / 2 = attn2_kernel with 4 / 8 waves (the form the hoisted grounding-token K / V
    runs). The switch is read once per process: one child per value, each with its own time limit; a child that fails ends the test."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for mode in ("0", "1", "2"):
        env = dict(os.environ, GL_ATTN_V2=mode, GL_DEV_SWITCHES="1")
        t0 = time.time()
        r = subprocess.run([sys.executable, "-c", _SWITCH_SNIPPET % (root, os.path.join(root, "tests"))], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, f"GL_ATTN_V2={mode}: exit status {r.returncode}\n{r.stderr[-3000:]}"
        n, finite, same, max_rel, mean_rel, row_rel = r.stdout.strip().split("WORST")[-1].split()
        print(f"[regimes] GL_ATTN_V2={mode}: {n} cases, max_rel={max_rel} mean_rel={mean_rel} row_rel={row_rel} ({time.time() - t0:.1f} s)")
        assert int(n) == 12 and int(finite) == 1 and int(same) == 1, r.stdout
        assert float(max_rel) < MAX_BAR and float(mean_rel) < MEAN_BAR and float(row_rel) < ROW_BAR, r.stdout
