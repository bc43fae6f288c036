"""ISA regression check of the GEMM main loop (no GPU needed: hipcc cross-compiles gfx950).

The v5 GEMM prefetches K tiles by LDS-DMA and relies on NOTHING draining that DMA between its issue and the MFMAs
of the tile being multiplied. hipcc re-inserts `s_waitcnt vmcnt(0)` there at the slightest provocation (a
compiler-visible LDS load, an inline asm with a "memory" clobber, a conditional drain at the loop top), which is
invisible to every numerical test and costs 10-25 % of GEMM throughput. This test compiles the GEMM's units
(gemm_u.hip, gemm_halo.hip, gemm_wide.hip, gemm_basic.hip, gemm.hip) to gfx950 assembly and asserts, for every
gemm_u_kernel instantiation, that between the main loop's s_barrier and its last
MFMA the only vmcnt wait is the intended one directly in front of the barrier, that the DMA is not wrapped in
waterfall loops, and that nothing spills."""
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def gemm_asm(tmp_path_factory):
    """The assembly of the GEMM's translation units (gemm_impl.h: one per kernel family + the host unit with the split-K reduce),
    compiled side by side and concatenated: a kernel is defined in exactly one of them."""
    from gligen_amd.build import GEMM_UNITS
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    tmp = tmp_path_factory.mktemp("isa")

    def listing(unit):
        out = tmp / (unit + ".s")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", str(ROOT / "include"), "--offload-device-only", "-S",
               str(ROOT / "gligen_amd" / "csrc" / unit), "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return out.read_text()

    with ThreadPoolExecutor(max_workers=min(len(GEMM_UNITS), 8)) as ex:
        return "\n".join(ex.map(listing, GEMM_UNITS))


def _kernels(asm):
    for name in re.findall(r"^(_ZN2gl13gemm_u_kernelI[^:\s]*):", asm, re.M):
        a = asm.index(name + ":")
        b = asm.index(".Lfunc_end", a)
        yield name, asm[a:b].split("\n")


def test_gemm_main_loop_has_no_dma_drain(gemm_asm):
    seen = 0
    for name, body in _kernels(gemm_asm):
        seen += 1
        barrier = [i for i, l in enumerate(body) if "s_barrier" in l]
        mfma = [i for i, l in enumerate(body) if "v_mfma" in l]
        dma_i = [i for i, l in enumerate(body) if "buffer_load_dwordx4" in l and " lds" in l]
        reads = [i for i, l in enumerate(body) if "ds_read_b128" in l]
        assert barrier and mfma, name
        # the loop-top barrier is the one that is followed by the K-tile DMA issue before any other barrier (the epilogues
        # of the head-layout instantiations have barriers of their own, around the folded LayerNorm's row statistics, and
        # hipcc lays that code out between the loop top and the MFMAs)
        top = next(b for k, b in enumerate(barrier) if any(b < d < (barrier[k + 1] if k + 1 < len(barrier) else len(body)) for d in dma_i))
        issue = [d for d in dma_i if d > top and all(not (top < b < d) for b in barrier)]
        assert len(issue) >= 4, f"{name}: expected the K-tile DMA issue right behind the loop barrier, found {len(issue)}"   # (64 x 64 tile: 2 + 2 passes)
        head = body[top + 1:issue[-1]]
        # the multiply: the fragment reads in front of the first MFMA up to the last MFMA
        first_read = min(r for r in reads if 0 < mfma[0] - r < 300)
        mult = body[first_read:mfma[-1]]
        for what, seg in (("the loop barrier and the DMA issue", head), ("the fragment reads and the last MFMA", mult)):
            waits = [l.strip() for l in seg if "s_waitcnt" in l and "vmcnt" in l]
            assert not waits, f"{name}: vmcnt wait(s) between {what}: {waits[:4]}"
        # DMA must not be wrapped in waterfall loops (descriptor / soffset / m0 proven wave-uniform)
        text = "\n".join(head)
        assert len(re.findall(r"v_readfirstlane_b32", text)) <= 12, f"{name}: waterfall loops around the LDS-DMA?"
    assert seen >= 8


def test_gemm_kernels_do_not_spill(gemm_asm):
    """No kernel of the GEMM's units spills -- with one bounded exception: conv_halo_kernel<5, 8, GN = true> (256 registers, the GroupNorm
    prologue's operands on top of 80 accumulators + 72 fragment registers) parks a handful of lane constants (<= 6 dwords) of its EPILOGUE in
    scratch, once per work item; test_halo_kernel_gn_prologue_rides_under_the_deferred_mfmas pins that its tap loop has none."""
    meta = gemm_asm[gemm_asm.index("amdhsa.kernels:"):]
    entries = re.split(r"\n  - \.agpr_count:", meta)[1:]
    assert len(entries) > 20
    for e in entries:
        name = re.search(r"\.name:\s*(\S+)", e).group(1)
        spills = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", e).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", e).group(1))
        if name.startswith("_ZN2gl16conv_halo_kernelILi5ELi8ELb1E"):
            assert spills <= 6 and scratch <= 32, (name, spills, scratch)
        else:
            assert spills == 0 and scratch == 0, (name, spills, scratch)


def test_halo_kernel_keeps_its_cross_barrier_pipelining(gemm_asm):
    """conv_halo_kernel: hipcc runs the MFMAs of a tile's second K step BEHIND the next tile's barrier and DMA issue, in front of the
    next tile's fragment reads (which then fly under them). That order is worth ~20 % of the kernel (every
    variant that lost it -- run-time ablation switches, a branch chain in front of the barrier -- fell back to the speed of the
    implicit-GEMM kernel), and nothing in the source pins it: this test does. Also: no scratch, no spills."""
    names = [n for n in re.findall(r"^(_ZN2gl16conv_halo_kernel[^:\s]*):", gemm_asm, re.M) if "Lb0E" in n]   # (the GroupNorm-prologue variants: next test)
    assert len(names) == 2
    for name in names:
        a = gemm_asm.index(name + ":")
        body = gemm_asm[a:gemm_asm.index(".Lfunc_end", a)].split("\n")
        assert not [l for l in body if "scratch_" in l], name
        bars = [i for i, l in enumerate(body) if "s_barrier" in l]
        assert len(bars) == 9, (name, len(bars))          # one barrier per filter tap
        for k in range(1, 7):                                # taps 1..6 (the last two segments also hold the loop's back edge)
            seg = [l.strip() for l in body[bars[k]:bars[k + 1]]]
            first_read = next(i for i, l in enumerate(seg) if l.startswith("ds_read"))
            ahead = sum(1 for l in seg[:first_read] if l.startswith("v_mfma"))
            assert ahead >= 16, f"{name}: tap {k}: only {ahead} MFMAs in front of the fragment reads"
            dma = [i for i, l in enumerate(seg) if l.startswith("buffer_load") and "lds" in l]
            assert dma and dma[0] < first_read, f"{name}: tap {k}: the DMA must be issued before the fragment reads"


def test_halo_kernel_gn_prologue_rides_under_the_deferred_mfmas(gemm_asm):
    """conv_halo_kernel<.., GN = true> (GroupNorm-apply + SiLU inside the conv's loader): K step 1 of a tile is deferred by hand
    behind the next barrier, and the prologue's arithmetic on the piece of the next chunk's halo (8 exp2 + 8 rcp per lane and tap)
    sits BETWEEN those MFMAs -- a VALU-only block in front of them costs the kernel ~20 %. Pinned here: per steady-state tap one piece
    is read, rewritten and stored, at least half of the deferred MFMAs are interleaved with its transcendentals, the DMA goes out
    before the fragment reads, and nothing spills inside the tap loop."""
    names = [n for n in re.findall(r"^(_ZN2gl16conv_halo_kernel[^:\s]*):", gemm_asm, re.M) if "Lb1E" in n]
    assert len(names) == 2
    for name in names:
        a = gemm_asm.index(name + ":")
        body = gemm_asm[a:gemm_asm.index(".Lfunc_end", a)].split("\n")
        bars = [i for i, l in enumerate(body) if "s_barrier" in l]
        assert len(bars) == 10, (name, len(bars))         # the first-chunk barrier + one per filter tap
        for k in range(2, 8):                                # taps 1..6
            seg = [l.strip() for l in body[bars[k]:bars[k + 1]]]
            assert not [l for l in seg if l.startswith("scratch_")], f"{name}: tap {k - 1} spills"
            trans = [i for i, l in enumerate(seg) if l.startswith("v_exp_f32") or l.startswith("v_rcp_f32")]
            assert len(trans) == 16, f"{name}: tap {k - 1}: {len(trans)} transcendentals (one 8-channel piece = 8 exp2 + 8 rcp)"
            between = sum(1 for l in seg[trans[0]:trans[-1]] if l.startswith("v_mfma"))
            assert between >= 6, f"{name}: tap {k - 1}: only {between} MFMAs between the prologue's transcendentals"
            assert sum(1 for l in seg if l.startswith("ds_write_b128")) == 1, name
            first_frag = max(i for i, l in enumerate(seg) if l.startswith("ds_write_b128"))
            dma = [i for i, l in enumerate(seg) if l.startswith("buffer_load") and "lds" in l]
            assert dma and dma[-1] < first_frag, f"{name}: tap {k - 1}: the DMA must be issued before the prologue and the fragment reads"


def test_wide_gemm_waits_for_its_fragment_reads_before_the_barrier(gemm_asm):
    """gemm_wide_kernel multiplies K step 1 of a tile behind the NEXT barrier. Its fragment reads are inline asm (invisible to hipcc's
    lgkmcnt bookkeeping), so the source must wait lgkmcnt(0) itself before the wave reaches that barrier: behind it the LDS stage is
    overwritten by DMA and the fragments are consumed. Order inside the loop: barrier, DMA issue, deferred MFMAs, all fragment
    reads, lgkmcnt(TM+TN), K step 0's MFMAs, lgkmcnt(0). An item's first tile is its own copy of that body (nothing deferred yet)
    in front of the loop."""
    names = re.findall(r"^(_ZN2gl16gemm_wide_kernel[^:\s]*):", gemm_asm, re.M)
    assert len(names) == 2
    for name in names:
        a = gemm_asm.index(name + ":")
        body = [l.strip() for l in gemm_asm[a:gemm_asm.index(".Lfunc_end", a)].split("\n")]
        assert not [l for l in body if l.startswith("scratch_")], name
        bar = next(i for i, l in enumerate(body) if l.startswith("s_barrier"))
        ev = []
        for l in body[bar:]:
            if l.startswith("ds_read"): ev.append("r")
            elif l.startswith("v_mfma"): ev.append("M")
            elif l.startswith("buffer_load") and " lds" in l: ev.append("D")
            elif l.startswith("s_waitcnt") and "lgkmcnt(0)" in l: ev.append("W")
            elif l.startswith("s_waitcnt") and "lgkmcnt" in l: ev.append("w")
        seq = re.sub(r"(.)\1+", r"\1", "".join(ev))          # collapse runs
        assert seq.startswith("DrwMW" "DMrwMW"), f"{name}: first tile + loop order is {seq[:16]}"


@pytest.fixture(scope="module")
def attn_asm(tmp_path_factory):
    from gligen_amd.build import EXTRA_FLAGS
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path_factory.mktemp("isa") / "attention.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *EXTRA_FLAGS.get("attention.hip", []), "-I", str(ROOT / "include"),
           "--offload-device-only", "-S", str(ROOT / "gligen_amd" / "csrc" / "attention.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


def test_attention_d40_loop_is_lean(attn_asm):
    """The d = 40 attention kernel is bound by VALU + MFMA issue (they barely overlap on gfx950), so its 64-key loop must
    stay free of per-score work that the design removed: no v_fma in front of the exps (the stabiliser rides through the
    MFMA), no AGPR traffic (VGPR-destination MFMAs), no LDS bpermute for the row max, and <= 128 VGPRs (four waves per SIMD)."""
    name = re.search(r"^(_ZN2gl11attn_kernelILi48ELi64ELb1EE[^:\s]*):", attn_asm, re.M).group(1)
    a = attn_asm.index(name + ":")
    body = attn_asm[a:attn_asm.index(".Lfunc_end", a)]
    meta = attn_asm[attn_asm.index(".name:           " + name):]
    assert int(re.search(r"\.vgpr_count:\s*(\d+)", meta).group(1)) <= 128
    assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", meta).group(1)) == 0
    ops = [l.split()[0] for l in body.split("\n") if l.strip() and not l.strip().startswith((";", "."))]
    count = lambda op: sum(1 for o in ops if o.startswith(op))
    assert count("v_accvgpr") == 0
    assert count("ds_bpermute") <= 1 and count("v_permlane32_swap") >= 1   # one shuffle is left after the loop (denominator row)
    # peeled first tile + loop: 64 exps and 28 MFMAs, and only the handful of fmas of the rare paths
    assert count("v_mfma_f32_32x32x16_bf16") == 28
    assert 64 <= count("v_exp_f32") <= 70
    assert count("v_fma_f32") <= 8


def test_attn2_loop_is_pipelined_and_lean(attn_asm):
    """attn2_kernel (d = 40): the steady-state loop is two iterations (the score register sets swap roles), each with its 14
    MFMAs interleaved with the 32 exps / 16 packs of the previous tile -- the interleave is hipcc's, nothing in the source pins
    it but three sched_barriers, so it is pinned here -- one vmcnt wait + one barrier per iteration at the top, the K / V^T tiles
    by LDS-DMA (4 pieces per wave and iteration), no scratch, and a DMA issue that costs a handful of scalar instructions
    (the first version spent ~80 per iteration on wave-uniform branches around each piece)."""
    name = re.search(r"^(_ZN2gl12attn2_kernelILi48ELi64ELb1ELi4EE[^:\s]*):", attn_asm, re.M).group(1)
    a = attn_asm.index(name + ":")
    body = attn_asm[a:attn_asm.index(".Lfunc_end", a)].split("\n")
    meta = attn_asm[attn_asm.index(".name:           " + name):]
    assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", meta).group(1)) == 0
    head = next(i for i, l in enumerate(body) if "Inner Loop Header" in l)
    label = body[head].split(":")[0].strip()
    back = max(i for i, l in enumerate(body) if re.search(r"s_(c?branch\w*)\s+" + re.escape(label) + r"\s*$", l))
    loop = [l.strip() for l in body[head:back + 1] if l.strip() and not l.strip().startswith((";", "."))]
    ops = [l.split()[0] for l in loop]
    count = lambda op: sum(1 for o in ops if o.startswith(op))
    assert count("v_mfma_f32_32x32x16_bf16") == 28 and count("s_barrier") == 2
    assert count("buffer_load_dwordx4") == 8 and count("ds_read_b128") == 28
    assert count("global_load") == 0 and count("ds_write") == 0 and count("scratch_") == 0
    assert [l for l in loop if l.startswith("s_waitcnt") and "vmcnt" in l] == ["s_waitcnt vmcnt(0)"] * 2
    assert count("s_") - count("s_waitcnt") - count("s_nop") - count("s_barrier") <= 48, "the DMA issue / loop control grew scalar code again"
    # the interleave: in each iteration's hot path, between the first and the last MFMA, VALU work is spread between the MFMAs --
    # no run of more than 10 VALU instructions without an MFMA, no run of more than 3 MFMAs back to back
    first = next(i for i, o in enumerate(ops) if o.startswith("v_mfma"))
    last_first_iter = [i for i, o in enumerate(ops) if o.startswith("v_mfma")][13]
    run_v = run_m = worst_v = worst_m = 0
    for o in ops[first:last_first_iter + 1]:
        if o.startswith("v_mfma"):
            run_m += 1; run_v = 0
        elif o.startswith("v_"):
            run_v += 1; run_m = 0
        worst_v, worst_m = max(worst_v, run_v), max(worst_m, run_m)
    assert worst_v <= 10 and worst_m <= 3, (worst_v, worst_m)


def test_attn3_loop_puts_pv_on_16x16x32(attn_asm):
    """attn3_kernel (d = 40, round 5): attn2's pipeline with O^T += V^T P^T on v_mfma_f32_16x16x32_bf16. Per iteration of the
    steady-state loop (two per trip, the score sets swap roles): 6 MFMAs 32x32x16 for S^T, 12 MFMAs 16x16x32 for P V, the 8
    v_permlane16_swap that turn the 32x32 accumulators into the 16-query B operands, 6 + 6 fragment reads, K / V^T by LDS-DMA
    (at most 4 pieces per wave), one vmcnt wait + one barrier; no scratch, fewer registers than attn2 (O^T is 24, not 32)."""
    name = re.search(r"^(_ZN2gl12attn3_kernelILi48ELi48ELb1ELi4ELb0EE[^:\s]*):", attn_asm, re.M).group(1)
    a = attn_asm.index(name + ":")
    body = attn_asm[a:attn_asm.index(".Lfunc_end", a)].split("\n")
    meta = attn_asm[attn_asm.index(".name:           " + name):]
    assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.vgpr_count:\s*(\d+)", meta).group(1)) <= 256
    head = next(i for i, l in enumerate(body) if "Inner Loop Header" in l)
    label = body[head].split(":")[0].strip()
    back = max(i for i, l in enumerate(body) if re.search(r"s_(c?branch\w*)\s+" + re.escape(label) + r"\s*$", l))
    loop = [l.strip() for l in body[head:back + 1] if l.strip() and not l.strip().startswith((";", "."))]
    ops = [l.split()[0] for l in loop]
    count = lambda op: sum(1 for o in ops if o.startswith(op))
    assert count("v_mfma_f32_32x32x16_bf16") == 12 and count("v_mfma_f32_16x16x32_bf16") == 24 and count("s_barrier") == 2
    assert count("v_permlane16_swap") >= 16 and count("v_exp_f32") >= 64
    assert count("ds_read_b128") == 24 and count("buffer_load_dwordx4") <= 16
    assert count("global_load") == 0 and count("ds_write") == 0 and count("scratch_") == 0
    assert [l for l in loop if l.startswith("s_waitcnt") and "vmcnt" in l] == ["s_waitcnt vmcnt(0)"] * 2
    # the interleave of the first iteration: VALU work sits between the MFMAs
    mf = [i for i, o in enumerate(ops) if o.startswith("v_mfma")]
    run_v = run_m = worst_v = worst_m = 0
    for o in ops[mf[0]:mf[17] + 1]:
        if o.startswith("v_mfma"):
            run_m += 1; run_v = 0
        elif o.startswith("v_"):
            run_v += 1; run_m = 0
        worst_v, worst_m = max(worst_v, run_v), max(worst_m, run_m)
    assert worst_v <= 22 and worst_m <= 8, (worst_v, worst_m)   # (round 6: no row maximum between the six MFMAs of the second P V half any more)
    # d = 80 (attn3_kernel<80, 96, false, 4>, the LATE_V form): the steady-state loop fits 256 registers without scratch traffic
    # (the once-only first / last iterations may spill a few accumulator tuples across their merges: bounded here)
    name80 = re.search(r"^(_ZN2gl12attn3_kernelILi80ELi96ELb0ELi4ELb0EE[^:\s]*):", attn_asm, re.M).group(1)
    a = attn_asm.index(name80 + ":")
    body = attn_asm[a:attn_asm.index(".Lfunc_end", a)].split("\n")
    meta = attn_asm[attn_asm.index(".name:           " + name80):]
    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", meta).group(1)) <= 256
    head = next(i for i, l in enumerate(body) if "Inner Loop Header" in l)
    label = body[head].split(":")[0].strip()
    back = max(i for i, l in enumerate(body) if re.search(r"s_(c?branch\w*)\s+" + re.escape(label) + r"\s*$", l))
    ops = [l.strip().split()[0] for l in body[head:back + 1] if l.strip() and not l.strip().startswith((";", "."))]
    count = lambda op: sum(1 for o in ops if o.startswith(op))
    assert count("scratch_") == 0 and count("v_mfma_f32_32x32x16_bf16") == 20 and count("v_mfma_f32_16x16x32_bf16") == 48


@pytest.fixture(scope="module")
def norm_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path_factory.mktemp("isa") / "norm.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", str(ROOT / "include"), "--offload-device-only", "-S",
           str(ROOT / "gligen_amd" / "csrc" / "norm.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


def _wait_scan(asm, *filters):
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_waits", ROOT / "tools" / "isa_waits.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {name: (loads, imm, stores, after) for name, loads, imm, stores, after in mod.scan(None, filters, text=asm)}


def test_norm_kernels_keep_their_loads_in_flight(norm_asm):
    """GroupNorm is latency-bound unless every thread has several 16-byte loads in flight. Written as
    `x = 0; if (pixel in range) x = load`, hipcc folds the bf16 unpacking into the guarded block and waits for each load right
    behind its issue (seen in round 3: 7 of 8 loads in gn_stats_kernel, 22 in gn_apply_kernel incl. its 16 partial sums). The
    kernels now load unconditionally from a clamped address; this pins that no load is followed by vmcnt(0) within two
    instructions (tools/isa_waits.py)."""
    res = _wait_scan(norm_asm, "gn_stats_kernel", "gn_apply_kernel")   # (ln_kernel keeps its guards: one load per lane at C = 320,
    assert len(res) == 2                                                # where the guarded form measured 17 % faster)
    for name, (loads, imm, stores, after) in res.items():
        assert loads >= 8 and imm <= 1, (name, loads, imm)


def test_gemm_epilogues_wait_once_before_their_stores(gemm_asm):
    """vmcnt counts stores: a coefficient load between stores, or a wait hipcc re-inserts in every guarded block, makes each store
    wait for the acknowledgement of the one before it. The head-layout epilogues of the q,k,v^T projection (QKV instantiations)
    fetch everything first and force one wait (epi_ready): at most one vmcnt(0) behind a store; the row-GEMM instantiations keep
    no load that is waited for right behind its issue (the residual of the staged epilogue used to be: 32 of them)."""
    res = _wait_scan(gemm_asm, "gemm_u_kernel")
    qkv = {n: v for n, v in res.items() if "Lb1E" in n}
    rows = {n: v for n, v in res.items() if "ELi0ELi2ELb0E" in n}
    assert len(qkv) == 4 and len(rows) == 5
    for name, (loads, imm, stores, after) in qkv.items():
        assert stores >= 8 and after <= 1, (name, stores, after)
    for name, (loads, imm, stores, after) in rows.items():
        assert imm == 0, (name, loads, imm)


# ---- the row-local feed-forward kernel (ffn.hip): one wave per SIMD, the main loop a fixed asm-ordered stream. What is pinned here
# are the properties whose absence no numerical test on a lucky box shows (each was a real bug on the way):
@pytest.fixture(scope="module")
def ffn_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path_factory.mktemp("isa") / "ffn.s"
    from gligen_amd import build as glbuild       # the flags the shipped library is built with, so that what is pinned is what runs
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *glbuild.EXTRA_FLAGS["ffn.hip"], "-I", str(ROOT / "include"), "--offload-device-only", "-S",
           str(ROOT / "gligen_amd" / "csrc" / "ffn.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


def _ffn_kernels(asm):
    for name in re.findall(r"^(_ZN2gl12_GLOBAL__N_114ff_rows_kernelI[^:\s]*):", asm, re.M):
        a = asm.index(name + ":")
        b = asm.index(".end_amdhsa_kernel", a)
        meta = asm[a:b]
        body = [l.strip() for l in meta.split("\n") if l.strip() and not l.strip().startswith(";") and not l.strip().startswith(".")]
        yield name, meta, body


def _regs(tok):
    m = re.match(r"([av])\[(\d+):(\d+)\]", tok)
    if m:
        return m.group(1), set(range(int(m.group(2)), int(m.group(3)) + 1))
    m = re.match(r"([av])(\d+)$", tok)
    return (m.group(1), {int(m.group(2))}) if m else (None, set())


def test_ffn_kernels_fit_the_register_file_without_scratch(ffn_asm):
    names = [n for n, _, _ in _ffn_kernels(ffn_asm)]
    assert len(names) == 4, names          # plain, leading projection, leading + trailing projection, leading + trailing to_q (round 6)
    for name, meta, _ in _ffn_kernels(ffn_asm):
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta) or "scratch_" not in meta, name
        assert "scratch_load" not in meta and "scratch_store" not in meta, name
        nv = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
        assert nv <= 512, (name, nv)


def test_ffn_main_loop_is_the_stream_it_was_written_as(ffn_asm):
    """Two chunks per loop iteration: 124 MFMAs (32x32x16), one fragment read behind each, 32 DMA blocks, two barriers, and nothing
    else that could stall the lone wave of a SIMD: no accumulator moves, no packed fp32 (a wait state per dependent pair), no
    compiler-inserted vmcnt wait inside the stream (its counted waits do not see the asm DMAs)."""
    for name, meta, body in _ffn_kernels(ffn_asm):
        # the steady-state loop: a label and the backward branch to it with 124 MFMAs in between
        lines = [l.strip() for l in meta.split("\n") if l.strip() and not l.strip().startswith(";")]
        labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
        seg = None
        for i, l in enumerate(lines):
            m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)
            if m and labels.get(m.group(1), 1 << 30) < i:
                cand = [x for x in lines[labels[m.group(1)]:i] if not x.startswith(".")]
                if sum(1 for x in cand if x.startswith("v_mfma")) == 124:
                    seg = cand
        assert seg, name
        assert all("32x32x16_bf16" in x for x in seg if x.startswith("v_mfma")), name
        cnt = lambda p: sum(1 for l in seg if re.match(p, l))
        assert cnt(r"v_mfma") == 124, (name, cnt(r"v_mfma"))
        assert cnt(r"ds_read_b128") == 124, (name, cnt(r"ds_read_b128"))
        assert cnt(r"buffer_load_dwordx4 .* lds") == 32, (name, cnt(r"buffer_load_dwordx4 .* lds"))
        assert cnt(r"v_accvgpr_") == 0, (name, cnt(r"v_accvgpr_"))
        assert cnt(r"v_pk_") == 0, name
        assert cnt(r"v_exp_f32") == 32 and cnt(r"v_rcp_f32") == 0, name      # one transcendental per hidden feature (the exp2 form of erf-GELU)
        assert cnt(r"global_load|global_store") == 0, name
        waits = [l for l in seg if l.startswith("s_waitcnt") and "vmcnt" in l]
        assert all(w.replace(" ", "") == "s_waitcntvmcnt(0)" for w in waits) and len(waits) <= 3, (name, waits)
        # the GEGLU arithmetic of 32 hidden features per lane and chunk: 7 VALU each besides the exp (no canonicalising v_max in front
        # of max(x, 0): -fno-honor-nans in build.py)
        assert cnt(r"v_(fma|mul|max|add|sub|cvt_pk)_") <= 7 * 32 - 8, (name, cnt(r"v_(fma|mul|max|add|sub|cvt_pk)_"))
        assert len(seg) < 900, (name, len(seg))     # ~6 issue slots per 32-cycle MFMA


def test_ffn_accumulators_are_never_touched_next_to_their_mfmas(ffn_asm):
    """(1) No v_accvgpr_write lands within six instructions in front of an MFMA that reads that register (hipcc pads that hazard
    for its own MFMAs, not for an asm statement: the x fragments are pinned into the AGPR half before the stream starts).
    (2) No v_accvgpr_read of an accumulator tuple sits between that tuple's last MFMA and the settle nops (hipcc is free to hoist
    the epilogue's reads of a tuple right behind the ISSUE of its last MFMA unless every tuple is an operand of the settle statement)."""
    for name, _, body in _ffn_kernels(ffn_asm):
        acc = set()
        for l in body:
            if l.startswith("v_mfma"):
                c, r = _regs(l.split(None, 1)[1].split(",")[0].strip())
                if c == "a":
                    acc |= r
        nops = [i for i, l in enumerate(body) if l.startswith("s_nop 15")]
        for i, l in enumerate(body):
            if l.startswith("v_mfma"):
                srcs = set()
                for tok in l.split(None, 1)[1].split(",")[1:]:
                    c, r = _regs(tok.strip())
                    if c == "a":
                        srcs |= r
                for j in range(max(0, i - 6), i):
                    if body[j].startswith("v_accvgpr_write"):
                        c, r = _regs(body[j].split()[1].rstrip(","))
                        assert not (r & srcs), (name, body[j], l)
            if l.startswith("v_accvgpr_read"):
                c, r = _regs(l.split(",")[1].strip())
                if r & acc:
                    for j in range(i - 1, max(0, i - 40), -1):
                        if body[j].startswith("v_mfma"):
                            c2, r2 = _regs(body[j].split(None, 1)[1].split(",")[0].strip())
                            if c2 == "a" and (r & r2):
                                assert any(j < n < i for n in nops), (name, body[j], l)
                                break


def test_row_local_epilogues_issue_no_global_load_between_their_stores(ffn_asm):
    """Round 6: a global load inside an epilogue's per-feature-block loop makes hipcc wait vmcnt(0) in front of its use -- for every
    store issued before it, loads and stores share the counter: ten serialised round trips per epilogue (qkv_rows_kernel 65 -> 54 us,
    ff_rows_kernel<pre, post> 117 -> 112 us when they went). What is pinned: the q,k,v^T kernels have no scratch, every global load of
    theirs sits in front of the first MFMA, and every vmcnt wait in them is a full one (the asm stream's own: stage boundaries and the
    wait in front of an epilogue) -- hipcc found no load to wait for among the stores. In the feed-forward kernels no global load
    is followed by a global store before the next wait."""
    names = re.findall(r"^(_ZN2gl12_GLOBAL__N_115qkv_rows_kernelI[^:\s]*):", ffn_asm, re.M)
    assert len(names) == 4, names          # {leading projection or not} x {q,k,v^T or q only}
    for name in names:
        a = ffn_asm.index(name + ":")
        meta = ffn_asm[a:ffn_asm.index(".end_amdhsa_kernel", a)]
        body = [l.strip() for l in meta.split("\n") if l.strip() and not l.strip().startswith(";") and not l.strip().startswith(".")]
        assert "scratch_load" not in meta and "scratch_store" not in meta, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 512, name
        first_mfma = next(i for i, l in enumerate(body) if l.startswith("v_mfma"))
        loads = [i for i, l in enumerate(body) if l.startswith("global_load")]
        assert loads and max(loads) < first_mfma, (name, [body[i] for i in loads if i > first_mfma][:3])
        waits = [l.replace(" ", "") for l in body[first_mfma:] if l.startswith("s_waitcnt") and "vmcnt" in l]
        assert waits and all(w == "s_waitcntvmcnt(0)" for w in waits), (name, sorted(set(waits)))
        assert sum(1 for l in body if l.startswith("global_store")) >= 40, name
    for name, meta, body in _ffn_kernels(ffn_asm):
        pending_load = False
        for l in body:
            if l.startswith("global_load"):
                pending_load = True
            elif l.startswith("s_waitcnt") and "vmcnt" in l:
                pending_load = False
            elif l.startswith("global_store"):
                assert not pending_load, (name, "a store behind an unwaited load: the next use of that load waits for the store too")


def test_ffn_dma_statements_declare_what_they_clobber():
    """The LDS-DMA asm steps its cursors with s_add_u32: SCC has to be in the clobber list (without it hipcc kept the loop
    condition in SCC across the statement and the loop ran until the 32-bit stream offset overflowed)."""
    src = (ROOT / "gligen_amd" / "csrc" / "ffn.hip").read_text()
    stmts = re.findall(r'asm volatile\("(?:s_nop 4\\n\\t)?s_mov_b32 m0.*?;', src, re.S)
    assert len(stmts) == 2
    assert all('"scc"' in st for st in stmts)


TRAIN_UNITS = ["train_ops", "train_attention", "train_layers", "train_spatial", "train_unet"]


def test_training_attention_kernels_keep_their_chunks_in_registers(tmp_path):
    """train_attention.hip's fp32 attention kernels split a head dimension over 1 / 2 / 4 lanes in chunks of <= 40 so that a lane's q /
    accumulator chunks stay in registers (one lane per query at d = 160 spilled 320 floats and ran 3 ms per launch): the forward
    kernels use no scratch at all, the backward ones at most a few dozen dwords (they sit at the 128-register default bound).
    Across the five units of the training path (train_impl.h): 80 kernels, each defined in one unit only -- the build has no
    relocatable device code, so a kernel is launched from the unit that defines it."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

    def listing(unit):
        out = tmp_path / (unit + ".s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", str(ROOT / "include"), "--offload-device-only", "-S",
                            str(ROOT / "gligen_amd" / "csrc" / (unit + ".hip")), "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return out.read_text()

    with ThreadPoolExecutor(max_workers=len(TRAIN_UNITS)) as ex:
        listings = dict(zip(TRAIN_UNITS, ex.map(listing, TRAIN_UNITS)))
    seen = seen_reductions = 0
    owner = {}
    for unit, asm in listings.items():
        for m in re.finditer(r"\.amdhsa_kernel (\S+)", asm):
            blk = asm[m.start():asm.index(".end_amdhsa_kernel", m.start())]
            name = m.group(1)
            assert name not in owner, (name, owner[name], unit)
            owner[name] = unit
            scratch = int(re.search(r"private_segment_fixed_size (\d+)", blk).group(1))
            if "attn_fwd_kernel" in name:
                assert scratch == 0, (name, scratch)
                seen += 1
            elif "attn_bwd" in name:
                assert scratch <= 256, (name, scratch)
                seen += 1
            elif "colsum_kernel" in name or "gn_silu" in name:
                assert scratch == 0, (name, scratch)
                seen_reductions += 1
    assert seen == 15       # 5 head dims x (forward, backward-q, backward-kv)
    assert seen_reductions == 3     # colsum_kernel, gn_silu_fwd_kernel, gn_silu_bwd_kernel: a rename must not empty that branch
    assert len(owner) == 80, {u: sum(1 for v in owner.values() if v == u) for u in TRAIN_UNITS}
