"""Child process of test_train_prims_gpu.py (GL_TRAIN_ATTN_VALU and GL_TRAIN_3LAUNCH are read once per process): part of the case
list of tests/train_prims_ref.py on the code the switch selects, one line `REPORT <case> <tensor> <err> <bound>` per compared tensor
and one line `PROBLEM ...` per guard, NaN or determinism finding.
    attention   the attention list of head dims 32, 40, 64, 80 -- with GL_TRAIN_ATTN_VALU=1 on the VALU kernels, fp32-family bound
    linear      the Linear list -- with GL_TRAIN_3LAUNCH=1 in the three-launch form, split-family bound
    conv3       the conv3 list, every geom -- with GL_TRAIN_3LAUNCH=1 three single-source conv launches and an add pass, the same bound
Parts joined with + run one after the other in one process."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import train_prims_ref as R  # noqa: E402
from gligen_amd.engine import Engine  # noqa: E402


def report(rows, problems):
    for cid, tensor, err, bound in rows:
        print("REPORT", cid, tensor, repr(float(err)), repr(float(bound)), flush=True)
    for p in problems:
        print("PROBLEM", p, flush=True)


if __name__ == "__main__":
    parts = sys.argv[1].split("+")
    if set(parts) - {"attention", "linear", "conv3"}:
        sys.exit(f"unknown part in {sys.argv[1]!r}")
    eng = Engine(0, arena_gb=2.0)
    for what in parts:
        if what == "attention":
            valu = os.environ.get("GL_TRAIN_ATTN_VALU") == "1"
            for case in R.attention_cases(R.MFMA_DIMS):
                report(*R.run_attention(eng, case, valu=valu))
        elif what == "linear":
            for M, K, N in R.LINEAR_SHAPES:
                report(*R.run_linear(eng, M, K, N))
        else:
            for case in R.conv3_cases():
                report(*R.run_conv3(eng, case))
    eng.close()
