"""The GEMM planner (gligen_amd/csrc/gemm_plan.hip) picks, for every problem, the kernel, tile, K split, resident grid and item
order that the launcher picked before selection was separated from launching (no GPU needed: the planner is host code without a
HIP call).

tests/golden/gemm_plans.json holds problem descriptors and what the launcher of the commit before the split chose for them (see its
"_provenance"). The planner plus a small main (tests/gemm_plan_main.hip) is built into a stand-alone program, with the address and
undefined-behaviour sanitizers on the host code, run over every descriptor in every recorded knob setting, and each field has to
be equal: return code, tm, tn, splits, stats_nb, resident grid, box / rm / rz, K tiles per split, the wide kernel's XCD flag, the
halo kernel's chunks per split, the answers of gemm_gn_prologue_supported / gemm_ln_fold_supported and the kernel name."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "gemm_plans.json"

# one input line of gemm_plan_main: (field, value when the descriptor does not name it). Pointers are 0 / 1; ws_kib is in KiB.
FIELDS = [("M", 0), ("N", 0), ("K", 0),
          ("a_mode", 0), ("C0", 0), ("C1", 0), ("ld0", 0), ("ld1", 0), ("Hin", 0), ("Win", 0), ("Ho", 0), ("Wo", 0), ("stride", 0), ("ups", 0),
          ("pad_lo", 0), ("gn", 0),
          ("e_mode", 0), ("act", 0), ("out_f32", 0), ("bias", 1), ("bias2", 0), ("bias2_ld", 0), ("rows_per_b", 1), ("res", 0), ("gate", 0),
          ("q", 0), ("k", 0), ("vt", 0), ("C", 0), ("T", 0), ("remap_in", 0), ("geglu16", 0), ("stats_out", 0), ("stats_ld", 0),
          ("ln_stats", 0), ("ln_nb", 0), ("ln_ld", 0), ("ln_csum", 0),
          ("ws", 1), ("ws_kib", 1 << 20), ("no_split", 0)]
RESULT = ["rc", "tm", "tn", "splits", "stats_nb", "grid", "box", "rm", "rz", "kt_per_split", "xcd", "chunks_per_split", "gn_supported",
          "ln_supported", "name"]


def input_line(desc):
    unknown = set(desc) - {f for f, _ in FIELDS} - {"note"}
    assert not unknown, unknown
    return " ".join(str(desc.get(f, d)) for f, d in FIELDS)


def parse_output(text):
    rows = []
    for line in text.splitlines():
        parts = line.split(" ", len(RESULT) - 1)
        rows.append([int(x) for x in parts[:-1]] + [parts[-1]])
    return rows


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_main"
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"),
           str(ROOT / "gligen_amd" / "csrc" / "gemm_plan.hip"), str(ROOT / "tests" / "gemm_plan_main.hip"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def fixture():
    return json.loads(FIXTURE.read_text())


def test_fixture_covers_the_shipped_table_and_the_routing_boundaries(fixture):
    import re
    keys = re.findall(r'\{"([^"]+)"', (ROOT / "gligen_amd" / "csrc" / "gemm_tuned.inc").read_text())
    assert len(keys) > 300
    assert set(keys) <= set(fixture["table_keys"]), "every key of gemm_tuned.inc has its descriptor"
    assert set(fixture["knobs"]) == {"default", "no_table", "wide2", "variant1", "variant2"}
    names = {e[-1].split("<")[0] for p in fixture["problems"] for _, e in p["expect"]}
    assert {"gemm_glds_kernel", "gemm_p_kernel", "gemm_u_kernel", "conv_halo_kernel", "gemm_wide_kernel"} <= names
    assert FIXTURE.stat().st_size < 200_000


@pytest.mark.parametrize("knobs", ["default", "no_table", "wide2", "variant1", "variant2"])
def test_planner_reproduces_the_recorded_choices(planner, fixture, knobs):
    cases = [(p["desc"], e) for p in fixture["problems"] for ks, e in p["expect"] if knobs in ks]
    assert len(cases) >= (5 if knobs.startswith("variant") else 300)
    r = subprocess.run([str(planner), knobs], input="\n".join(input_line(d) for d, _ in cases) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert not r.stderr.strip(), r.stderr[-3000:]   # (sanitizer reports)
    got = parse_output(r.stdout)
    assert len(got) == len(cases)
    bad = [(d, dict(zip(RESULT, e)), dict(zip(RESULT, g))) for (d, e), g in zip(cases, got) if list(e) != g]
    assert not bad, f"{len(bad)} of {len(cases)} problems planned differently; first: {bad[0]}"
