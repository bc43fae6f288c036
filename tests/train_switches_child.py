"""Child process of test_train_switches_gpu.py (the training path's developer switches are read once per process): the small training
slices of test_ops_gpu.py -- the fuser block, the two ResBlocks, Downsample / Upsample -- against their goldens through the same
helpers, one line `REPORT <case> <tensor> <value>` per compared tensor (relative MSE; `loss`: relative error)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from gligen_amd.engine import Engine  # noqa: E402
from helpers import fuser_block_train_report, resample_train_report, resblock_train_report  # noqa: E402


def report(case, values):
    for k, v in values.items():
        print("REPORT", case, k, repr(float(v)), flush=True)


if __name__ == "__main__":
    eng = Engine(0, arena_gb=6.0)
    report("block", fuser_block_train_report(eng)[0])
    for name in ("resblock_backward_skipconv", "resblock_backward_identity"):
        report(name, resblock_train_report(eng, name)[0])
    for mode in ("down", "up"):
        report("resample_" + mode, resample_train_report(eng, mode))
