"""The primitives of the training path on the device, one by one (include/gligen_amd_train_prims.h): the MFMA and VALU attention
kernels, the Linear products, LayerNorm, GroupNorm + SiLU, GEGLU and the dot / MSE reduction against the float64 references of
tests/train_prims_ref.py, which tests/test_train_prims_cpu.py holds to torch.

The measure is per output tensor max|got - ref64| / max|ref64| -- a maximum, so one wrong row of 4096 counts in full. Every output is
a view between two 64-float guard zones and starts as NaN: after the call the guards hold their bits and no NaN is left. A second call
gives the same bits. Every bound is computed at run time from the references on the case's own inputs:
    fp32 family (VALU attention, LayerNorm, GroupNorm, GEGLU)    err <= max(8 e32, 2^-22), e32 the measure of torch's fp32 arithmetic
    split family (MFMA attention, the Linear products, conv3 in
                  every geometry, the conv weight gradient)      err <= 4 e3, e3 the measure of the three-pass bf16 emulation
    reductions (dot, and the column sums db, dgamma, dbeta)      |err| <= (L + 1) 2^-24 sum|terms| per element, L the longest chain
    the direct conv (y, dx)                                      |err| <= (9 Cin_eff + 1) 2^-24 (sum|x||w| + |b|) per element
Each test prints err / bound of every tensor; profiles/train_prims/ keeps such tables."""
import os
import subprocess
import sys
import time

import pytest

import train_prims_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def check(rows, problems):
    for line in R.format_rows(rows):
        print("[train prims]", line)
    assert not problems, problems
    assert not R.failures(rows), R.format_rows(R.failures(rows))


@pytest.mark.parametrize("case", R.attention_cases(), ids=R.case_id)
def test_attention(engine, case):
    """o, lse, dq, dk, dv of Ctx::attn_fwd / attn_bwd, the full call and the dq-only call (dq bit-equal between the two). Head dims 32,
    40, 64, 80 run the MFMA kernels (split family), 160 the VALU kernels (fp32 family). Nk = 1 makes dq and dk vanish in exact
    arithmetic: train_prims_ref.attention_zero_gradients."""
    check(*R.run_attention(engine, case))


@pytest.mark.parametrize("case", R.attention_regime_cases(), ids=R.case_id)
def test_attention_regimes(engine, case):
    """Large logits, one probability of 1 with the rest underflowing, uniform probabilities, and scores near -60 against the -1e30
    start of the running maximum and the padded-key mask; everything stays finite."""
    check(*R.run_attention(engine, case))


@pytest.mark.parametrize("M,K,N", R.LINEAR_SHAPES)
def test_linear(engine, M, K, N):
    """y, dx, dW of lin_fwd_any / lin_dgrad_any / lin_wgrad_unpad in the default one-launch form (split family), db by colsum."""
    check(*R.run_linear(engine, M, K, N))


@pytest.mark.parametrize("m", R.OFFSETS)
@pytest.mark.parametrize("R_,C", R.LN_SHAPES)
def test_layernorm(engine, R_, C, m):
    """ln_fwd / ln_bwd on N(m, 1) rows and a constant row, eps 1e-5 and 1e-6, dx written and dx added to a random tensor."""
    rows, problems = [], []
    for eps in (1e-5, 1e-6):
        for accumulate in (False, True):
            r, p = R.run_layernorm(engine, R_, C, m, eps, accumulate)
            rows += r
            problems += p
    check(rows, problems)


@pytest.mark.parametrize("m", R.OFFSETS)
@pytest.mark.parametrize("B,HW,C", R.GN_SHAPES)
def test_groupnorm_silu(engine, B, HW, C, m):
    """gn_silu_fwd / gn_silu_bwd at 1, 2, 10 and 3 channels per group on N(m, 1) values, with and without SiLU, dx written and added."""
    rows, problems = [], []
    for silu in (True, False):
        for accumulate in (False, True):
            r, p = R.run_groupnorm(engine, B, HW, C, m, silu, accumulate)
            rows += r
            problems += p
    check(rows, problems)


@pytest.mark.parametrize("R_,I", R.GEGLU_SHAPES)
def test_geglu(engine, R_, I):
    check(*R.run_geglu(engine, R_, I))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", R.DOT_SIZES)
def test_dot(engine, n, mode):
    """Ctx::dot_reduce below, at and above the 2^18 threshold of its chunked path; mode 0 with alpha = 0.3."""
    check(*R.run_dot(engine, n, mode))


CONV3_KERNELS = {}      # case id -> kernel families of its launches, filled by test_conv3


@pytest.mark.parametrize("case", R.conv3_cases(), ids=R.conv_case_id)
def test_conv3(engine, case):
    """y and dx of Ctx::conv3 (geom 0), of Downsample (geom 1: stride 2 forward, zero insertion + the flipped stride-1 conv backward) and
    of Upsample (geom 2: nearest 2x + conv forward, the dgrad conv at 2H x 2W + 2 x 2 block sums backward) in the aliased two-source
    one-launch form, K = 27 Cin: split family. Prints the kernel families the GEMM plan log showed."""
    rows, problems = R.run_conv3(engine, case, CONV3_KERNELS)
    print("[train prims]", R.conv_case_id(case), "kernels:", ", ".join(CONV3_KERNELS[R.conv_case_id(case)]))
    check(rows, problems)


def test_conv3_kernel_families(engine):
    """The conv3 list as a whole runs conv_halo_kernel, the conv instantiation of gemm_u_kernel and gemm_glds_kernel, and nothing but the
    conv kernels: a routing change cannot quietly empty a path. Families only -- tile and split are the tuner's. A case test_conv3 has
    not run in this process is launched here (without a reference)."""
    seen = {}
    for c in R.conv3_cases():
        cid = R.conv_case_id(c)
        seen[cid] = CONV3_KERNELS.get(cid) or R.conv3_kernels(engine, c)
        print("[train prims]", cid, "kernels:", ", ".join(seen[cid]))
        assert seen[cid], cid
    families = set().union(*seen.values())
    assert families >= set(R.CONV_FAMILIES), families
    assert all(f.endswith("(conv)") or f == "conv_halo_kernel" for f in families), families
    assert "conv_halo_kernel" in seen["g0-2x32x32-64-128"] and "gemm_glds_kernel(conv)" in seen["g0-2x32x32-64-128"]      # forward; dgrad, N = 64
    assert "conv_halo_kernel" in seen["g2-2x16x16-128-128"] and "gemm_u_kernel(conv)" in seen["g2-2x16x16-128-128"]      # 32 x 32 dgrad; ups forward


@pytest.mark.parametrize("case", R.direct_cases(), ids=R.conv_case_id)
def test_conv_direct(engine, case):
    """conv3x3_direct's y and its data gradient for the channels [c0, c0 + n) elementwise against the fp32 chain's bound (err / bound
    against 1), dW of conv_wgrad (im2col + lin_wgrad_unpad) in the split family."""
    check(*R.run_conv_direct(engine, case))


def test_argument_errors(engine):
    """A null required pointer, dk without dv, a head dim the tables do not build and C % 32 != 0 are GL_ERR_ARG with a message; so
    are the convs' refusals: channels off the 64-step, a resampling layer that changes its channels, an odd Downsample, a geom outside
    0 .. 2, dx without dy, a channel range outside the input."""
    import ctypes as C
    import torch
    from gligen_amd._lib import GligenAmdError
    t = torch.zeros(2, 4, 96, device=engine.device)
    st = C.c_void_p(torch.cuda.current_stream(engine.device).cuda_stream)
    p, null = C.c_void_p(t.data_ptr()), C.c_void_p(0)
    lib, ctx = engine.lib, engine._ctx

    def refused(rc, word):
        assert rc == 2, rc                                            # GL_ERR_ARG
        assert word in lib.gl_last_error().decode(), lib.gl_last_error()

    refused(lib.gl_op_train_attention(ctx, 1, 1, 32, 4, 4, p, p, p, p, p, null, null, null, null, st), "required")
    refused(lib.gl_op_train_attention(ctx, 1, 1, 32, 4, 4, p, p, p, p, p, p, p, p, null, st), "dk and dv come together")
    refused(lib.gl_op_train_attention(ctx, 1, 1, 48, 4, 4, p, p, p, null, p, p, null, null, null, st), "head dim 48")
    refused(lib.gl_op_train_groupnorm(ctx, 1, 4, 48, 1, C.c_float(1e-5), p, p, p, null, 0, p, p, p, null, st), "32 groups")
    refused(lib.gl_op_train_linear(ctx, 4, 96, 96, null, p, null, null, p, null, null, null, st), "required")
    refused(lib.gl_op_train_dot(ctx, 4, p, p, null, C.c_float(1.0), 0, p, st), "alpha")
    with pytest.raises(GligenAmdError):
        engine.op_train_attention(t, t, t, 2)                         # 96 / 2 = 48 through the wrapper
    conv3 = lambda B, H, W, Ci, Co, geom, x=p, w=p, dy=null, y=p, dx=null: lib.gl_op_train_conv3(ctx, B, H, W, Ci, Co, geom, x, w, null, dy, y, dx, st)
    refused(conv3(1, 2, 2, 96, 64, 0), "multiples of 64")
    refused(conv3(1, 2, 2, 64, 96, 0), "multiples of 64")
    refused(conv3(1, 2, 2, 64, 128, 1), "keeps its channels")
    refused(conv3(1, 2, 2, 64, 128, 2), "keeps its channels")
    refused(conv3(1, 3, 2, 64, 64, 1), "even H and W")
    refused(conv3(1, 2, 3, 64, 64, 1), "even H and W")
    refused(conv3(1, 2, 2, 64, 64, 3), "geom 3")
    refused(conv3(1, 2, 2, 64, 64, -1), "geom -1")
    refused(conv3(1, 2, 2, 64, 64, 0, x=null), "required")
    refused(conv3(1, 2, 2, 64, 64, 0, w=null), "required")
    refused(conv3(1, 2, 2, 64, 64, 0, y=null), "required")
    refused(conv3(1, 2, 2, 64, 64, 0, dx=p), "without dy")
    direct = lambda c0, n, x=p, dy=null, y=p, dx=null, dW=null: lib.gl_op_train_conv_direct(ctx, 1, 2, 2, 4, 8, c0, n, x, p, null, dy, y, dx, dW, st)
    refused(direct(0, 4, x=null), "required")
    refused(direct(0, 4, y=null), "required")
    refused(direct(0, 4, dx=p), "without dy")
    refused(direct(0, 4, dW=p), "without dy")
    refused(direct(2, 3), "channels [2, 5) of 4")
    with pytest.raises(GligenAmdError):
        engine.op_train_conv3(torch.zeros(1, 3, 2, 64), torch.zeros(64, 64, 3, 3), geom=1)


# ---- the other code paths: GL_TRAIN_ATTN_VALU and GL_TRAIN_3LAUNCH are read once per process
CHILDREN = {
    # switch: (what the child runs, REPORT lines: tensors per case)
    "GL_TRAIN_ATTN_VALU": ("attention", 5 * len(R.attention_cases(R.MFMA_DIMS))),
    "GL_TRAIN_3LAUNCH": ("linear+conv3", 4 * len(R.LINEAR_SHAPES) + 2 * len(R.conv3_cases())),
}


def run_child(switch):
    what, n_reports = CHILDREN[switch]
    env = dict(os.environ, GL_DEV_SWITCHES="1", GL_GEMM_AUTOTUNE="0")
    for k in ("GL_TRAIN_3LAUNCH", "GL_TRAIN_ATTN_VALU", "GL_TRAIN_BF16X1"):
        env.pop(k, None)
    env[switch] = "1"
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "train_prims_child.py"), what], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"{switch}=1: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    rows, problems = [], []
    for line in r.stdout.splitlines():
        if line.startswith("REPORT "):
            _, cid, tensor, err, bound = line.split()
            rows.append((cid, tensor, float(err), float(bound)))
        elif line.startswith("PROBLEM "):
            problems.append(line)
    print(f"[train prims] {switch}=1: {len(rows)} tensors ({time.time() - t0:.1f} s)")
    for line in R.format_rows(rows):
        print(f"[train prims] {switch}=1", line)
    assert len(rows) == n_reports and len({r[:2] for r in rows}) == n_reports, (len(rows), n_reports)
    assert not problems, problems
    assert not R.failures(rows), R.format_rows(R.failures(rows))


def test_developer_switch_paths():
    """One fresh child per switch, each under its own time limit, the first failure ends the test: the attention list of head dims 32,
    40, 64, 80 on the VALU kernels (fp32 family), the Linear list and the conv3 list (every geom) in the three-launch form (split family,
    the same bound). The number of reports is
    asserted, so a child that ran less cannot pass."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    for switch in CHILDREN:
        run_child(switch)
