"""conv8_kernel without a GPU: the entries of include/gligen_amd_conv8.h are declared, exported and bound; the router leaves every
8 x 8 problem of the planner fixtures (tests/golden/gemm_candidates.json, tests/golden/gemm_epilogues.json: 64 and 128 input channels)
where it was and takes the benchmark's two shapes; the knobs switch it off and gl_gemm_force_clear puts them back; and the kernel's
unit compiles for gfx950 without scratch, with a stage loop that waits for its DMA once, directly in front of its barrier."""
import ctypes
import os
import re
import shutil
import subprocess

import gemm_candidates_ref as R
import gemm_epilogues_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    return _lib, _lib.load()


def _args(mod, B=8, C0=1280, C1=0, N=1280, H=8, W=8, stride=1, ups=0, pad_lo=1, bias2=True, res=False, act=0, out_f32=0):
    a = mod.Conv8Args()
    a.struct_size = ctypes.sizeof(mod.Conv8Args)
    a.x0 = 1; a.x1 = 1 if C1 else None
    a.C0, a.C1, a.B, a.H, a.W, a.N, a.stride, a.ups, a.pad_lo = C0, C1, B, H, W, N, stride, ups, pad_lo
    a.w = 1; a.bias = 1; a.bias2 = 1 if bias2 else None; a.bias2_ld = N; a.rows_per_b = H * W
    a.res = 1 if res else None; a.ldres = N; a.act = act; a.out_f32 = out_f32; a.out = 1; a.ldo = N
    return a


def test_entries_are_declared_exported_and_bound():
    mod, lib = _lib()
    header = open(os.path.join(ROOT, "include", "gligen_amd_conv8.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", code)) == set(mod.CONV8_SYMBOLS) == {"gl_op_conv8x8", "gl_conv8_routed", "gl_conv8_force_knobs"}
    assert not set(mod.CONV8_SYMBOLS) & (set(mod.SYMBOLS) | set(mod.GEMM_PLAN_SYMBOLS) | set(mod.ATTENTION_CORE_SYMBOLS))
    fields = re.search(r"typedef struct gl_conv8_args \{(.*?)\} gl_conv8_args;", code, re.S).group(1)
    names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in mod.Conv8Args._fields_]
    a = _args(mod)
    assert lib.gl_op_conv8x8(None, ctypes.byref(a), None) == 2      # no context
    a.struct_size -= 4
    assert lib.gl_conv8_routed(ctypes.byref(a)) < 0
    assert lib.gl_conv8_force_knobs(1, 72, 0) == 2 and lib.gl_conv8_force_knobs(2, 0, 0) == 2


def test_router_refuses_the_fixture_problems_and_takes_the_benchmark_shapes():
    mod, lib = _lib()
    lib.gl_gemm_force_clear()
    seen = 0
    for p in list(R.PROBLEMS) + list(E.PROBLEMS):
        d = p.get("desc", {})
        if d.get("a_mode") not in (1, 2) or d.get("Hin") != 8 or d.get("Win") != 8:      # (2: an upsample conv in its phase form)
            continue
        seen += 1
        a = _args(mod, B=d["M"] // (d["Ho"] * d["Wo"]), C0=d["C0"], C1=d.get("C1", 0), N=d["N"], stride=d.get("stride", 1), ups=1 if d["a_mode"] == 2 else d.get("ups", 0),
                  pad_lo=d.get("pad_lo", 0), bias2=bool(d.get("bias2")), res=bool(d.get("res")), act=d.get("act", 0), out_f32=d.get("out_f32", 0))
        assert lib.gl_conv8_routed(ctypes.byref(a)) == 0, p["id"]
    assert seen >= 2
    bench = [dict(C0=1280, bias2=True), dict(C0=1280, bias2=False, res=True), dict(C0=2560, bias2=True), dict(C0=1280, C1=1280, bias2=True),
             dict(C0=1280, B=4), dict(C0=1280, B=3), dict(C0=640, B=16)]
    for kw in bench:
        assert lib.gl_conv8_routed(ctypes.byref(_args(mod, **kw))) == 1, kw
    # everything else at this level stays where it is
    others = [dict(C0=576), dict(H=16, W=16), dict(stride=2, H=16, W=16), dict(ups=1), dict(pad_lo=0), dict(N=1000), dict(C0=1280, C1=32),
              dict(bias2=True, res=True), dict(act=3), dict(N=64)]
    for kw in others:
        assert lib.gl_conv8_routed(ctypes.byref(_args(mod, **kw))) == 0, kw


def test_knobs_switch_the_family_off_and_force_clear_puts_them_back():
    mod, lib = _lib()
    a = _args(mod)
    try:
        assert lib.gl_conv8_force_knobs(0, 0, 0) == 0
        assert lib.gl_conv8_routed(ctypes.byref(a)) == 0
        assert lib.gl_conv8_force_knobs(1, 80, 4) == 0
        assert lib.gl_conv8_routed(ctypes.byref(a)) == 1
        assert lib.gl_conv8_routed(ctypes.byref(_args(mod, N=1216))) == 0      # 1216 = 19 x 64: no whole 80-wide tiles
    finally:
        lib.gl_gemm_force_clear()
    assert lib.gl_conv8_routed(ctypes.byref(_args(mod, N=1216))) == 1


def test_unit_compiles_for_gfx950_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "gemm_conv8.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--offload-device-only", "-S",
                        os.path.join(ROOT, "gligen_amd", "csrc", "gemm_conv8.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    meta = asm[asm.index("amdhsa.kernels:"):]
    entries = re.split(r"\n  - \.agpr_count:", meta)[1:]
    assert len(entries) == 2                                  # column tiles of 64 and 80
    for e in entries:
        name = re.search(r"\.name:\s*(\S+)", e).group(1)
        assert "conv8_kernel" in name
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", e).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", e).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_count:\s*(\d+)", e).group(1)) <= 256, name
        a = asm.index(name + ":")
        body = [l.strip() for l in asm[a:asm.index(".Lfunc_end", a)].split("\n")]
        assert not [l for l in body if l.startswith("scratch_")], name
        # the stage loop: the one barrier that has a vmcnt(0) directly in front of it; from there to the last MFMA of the stage the
        # weights of the next stage are issued by LDS-DMA and nothing waits for them
        tops = [i for i, l in enumerate(body) if l.startswith("s_barrier") and body[i - 1].replace(" ", "") == "s_waitcntvmcnt(0)"]
        assert len(tops) == 1, (name, len(tops))
        mf = [i for i, l in enumerate(body) if l.startswith("v_mfma_f32_16x16x32_bf16")]
        tnf = 5 if "ILi5E" in name else 4
        assert len(mf) == 3 * 2 * 2 * tnf, (name, len(mf))      # three taps x two K steps x 2 x TNF fragments
        dma = [l for l in body if l.startswith("buffer_load_dwordx4") and " lds" in l]
        assert len(dma) >= 2 * (3 + 4), (name, len(dma))      # prologue + loop: a weight stage (3 or 4 passes) and a chunk's four samples
        assert "v_readfirstlane" not in "\n".join(body[tops[0]:tops[0] + 60]), (name, "waterfall loops around the LDS-DMA?")
        waits = [l for l in body[min(mf):max(mf)] if l.startswith("s_waitcnt") and "vmcnt" in l]
        assert not waits, (name, waits)                       # the multiply of a stage runs under the DMA issued in front of it
