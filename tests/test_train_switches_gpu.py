"""The training path's developer switches (tools/README.md) select code no default run reaches on small shapes: GL_TRAIN_3LAUNCH the
three-launch split-precision products, GL_TRAIN_ATTN_VALU the fp32 VALU attention kernels for every head dim (d = 160 runs them by
default), GL_TRAIN_BF16X1 the one-pass bf16 products. Each is read once per process, so each gets a fresh child
(train_switches_child.py: the fuser block, the two ResBlocks, Downsample / Upsample against their goldens)."""
import os
import subprocess
import sys
import time

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def fp32_bar(case, tensor):
    """The bars of test_ops_gpu.py's test_fuser_block / test_resblock / test_resample _backward_vs_reference (the default path's)."""
    if tensor == "loss":
        return 1e-5
    if tensor == "y":
        return 1e-6
    return 1e-5 if case == "block" else 1e-6


# GL_TRAIN_BF16X1: per-tensor relative MSE of the one-pass products. ResBlocks' y / dx: the figures DESIGN.md section 9 records, held at
# the precision they are recorded with (a result must round to no more than the figure: 6.1e-6 admits anything below 6.15e-6 -- the
# parent's own 6.12e-6 is what was written down as 6.1e-6). Every other figure is twice what the commit in front of this test
# measured with this child: profiles/train_split/switches_parent.txt has the measurements. One-pass error moves with the tile's
# split-K choice, so the children run with GL_GEMM_AUTOTUNE=0: no timed tile choice, the same tiles on every box.
BF16X1_BARS = {
    ("block", "y"): 1.47e-05,
    ("block", "loss"): 1e-05,
    ("block", "dx"): 4.04e-05,
    ("block", "dobjs"): 7.91e-05,
    ("block", "grad.fuser.alpha_attn"): 4.95e-07,
    ("block", "grad.fuser.alpha_dense"): 1.92e-10,
    ("block", "grad.fuser.attn.to_k.weight"): 8.8e-05,
    ("block", "grad.fuser.attn.to_out.0.bias"): 1.25e-05,
    ("block", "grad.fuser.attn.to_out.0.weight"): 3.88e-05,
    ("block", "grad.fuser.attn.to_q.weight"): 8.97e-05,
    ("block", "grad.fuser.attn.to_v.weight"): 3.53e-05,
    ("block", "grad.fuser.ff.net.0.proj.bias"): 3.33e-05,
    ("block", "grad.fuser.ff.net.0.proj.weight"): 6.88e-05,
    ("block", "grad.fuser.ff.net.2.bias"): 1.24e-05,
    ("block", "grad.fuser.ff.net.2.weight"): 6.37e-05,
    ("block", "grad.fuser.linear.bias"): 2.83e-05,
    ("block", "grad.fuser.linear.weight"): 7.93e-05,
    ("block", "grad.fuser.norm1.bias"): 2.6e-05,
    ("block", "grad.fuser.norm1.weight"): 4.55e-05,
    ("block", "grad.fuser.norm2.bias"): 3.5e-05,
    ("block", "grad.fuser.norm2.weight"): 5.34e-06,
    ("resblock_backward_skipconv", "y"): 5.85e-06,  # 5.8e-6
    ("resblock_backward_skipconv", "loss"): 9.14e-05,
    ("resblock_backward_skipconv", "dx"): 6.15e-06,  # 6.1e-6
    ("resblock_backward_identity", "y"): 9.5e-07,  # 9e-7
    ("resblock_backward_identity", "loss"): 3.4e-06,
    ("resblock_backward_identity", "dx"): 1.45e-06,  # 1.4e-6
    ("resample_down", "y"): 1.13e-05,
    ("resample_down", "loss"): 4.49e-06,
    ("resample_down", "dx"): 1.54e-05,
    ("resample_up", "y"): 1.16e-05,
    ("resample_up", "loss"): 8.32e-05,
    ("resample_up", "dx"): 1.11e-05,
}


def run_child(switch):
    env = dict(os.environ, GL_DEV_SWITCHES="1", GL_GEMM_AUTOTUNE="0")
    for k in ("GL_TRAIN_3LAUNCH", "GL_TRAIN_ATTN_VALU", "GL_TRAIN_BF16X1"):
        env.pop(k, None)
    env[switch] = "1"
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "train_switches_child.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{switch}=1: exit status {r.returncode}\n{r.stderr[-3000:]}"
    rep = {}
    for line in r.stdout.splitlines():
        if line.startswith("REPORT "):
            _, case, tensor, value = line.split()
            rep[case, tensor] = float(value)
    worst = max(rep, key=rep.get)
    print(f"[train switches] {switch}=1: {len(rep)} tensors, worst {worst} {rep[worst]:.3g} ({time.time() - t0:.1f} s)")
    for k in sorted(rep):
        print(f"[train switches] {switch}=1 {k[0]} {k[1]} {rep[k]!r}")
    assert len(rep) == 21 + 4 * 3, sorted(rep)      # block: y, loss, dx, dobjs + 17 gradients; four slices with y, loss, dx
    return rep


@pytest.mark.gpu
def test_training_developer_switches():
    """One child per switch, each under its own time limit; the first failure ends the test.
    GL_TRAIN_3LAUNCH and GL_TRAIN_ATTN_VALU are fp32-level paths: the default path's bars.
    GL_TRAIN_BF16X1: BF16X1_BARS. Measured on the parent commit: worst tensor resblock_backward_skipconv loss 4.57e-05 (bound 9.14e-05); the ResBlocks' y / dx
    5.8e-06 / 6.12e-06 (skip conv) and 9.1e-07 / 1.41e-06 (identity) against DESIGN.md's 5.8e-6 / 6.1e-6 and 9e-7 / 1.4e-6."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    for switch in ("GL_TRAIN_3LAUNCH", "GL_TRAIN_ATTN_VALU"):
        rep = run_child(switch)
        bad = {k: v for k, v in rep.items() if not v < fp32_bar(*k)}
        assert not bad, (switch, bad)
    rep = run_child("GL_TRAIN_BF16X1")
    assert sorted(rep) == sorted(BF16X1_BARS)
    bad = {k: (v, BF16X1_BARS[k]) for k, v in rep.items() if not v <= BF16X1_BARS[k]}
    assert not bad, bad
