"""Gradient accumulation, norm clipping and min-SNR weights, host side and pinning, no GPU: the entry points of
include/gligen_amd_train_run.h (declared, exported, bound), the ISA of csrc/train_run.hip, TrainStep's schedule on a recording
stand-in engine, two gloo ranks against torch.optim.AdamW on the clipped mean gradient, the Trainer's iteration count / batch stream /
resume refusal, min_snr_weights against the float64 formula, and the consistency of tests/train_run_ref.py itself."""
import ctypes
import json
import os
import re
import shutil
import socket
import subprocess
import sys
import textwrap
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import train_run_ref as R
from helpers import ROOT
from gligen_amd import synthetic as syn
from gligen_amd.train import TrainStep, min_snr_weights, warmup_schedule

HEADER = "gligen_amd_train_run.h"
FUSER_W = "input_blocks.1.1.transformer_blocks.0.fuser.linear.weight"
FUSER_A = "input_blocks.1.1.transformer_blocks.0.fuser.alpha_attn"
PN_W = "position_net.linears.0.weight"
TINY_CFG = dict(in_channels=4, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=False)


def tiny_state_dict():
    g = torch.Generator().manual_seed(3)
    return {"input_blocks.0.0.weight": torch.randn(8, 4, 3, 3, generator=g), FUSER_A: torch.randn((), generator=g), FUSER_W: torch.randn(16, 8, generator=g),
            "out.2.weight": torch.randn(4, 4, generator=g), PN_W: torch.randn(12, 5, generator=g)}


# ---- 1. the header
def test_train_run_entry_points_are_declared_exported_and_bound():
    """include/gligen_amd_train_run.h declares exactly the names of TRAIN_RUN_SYMBOLS, the built library exports them with the table's
    types, and neither the header nor the table shares a name with another header or table."""
    from gligen_amd import _lib as table
    from gligen_amd.build import SOURCES, build_native
    assert "train_run.hip" in SOURCES
    build_native()
    lib = table.load()
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    declared = set(re.findall(r"^(?:int|int64_t) (gl_[a-z0-9_]+)\s*\(", text, flags=re.M))
    assert declared == set(table.TRAIN_RUN_SYMBOLS) == {"gl_op_grad_accumulate", "gl_grad_sqnorm_partials", "gl_op_grad_sqnorm", "gl_op_clip_coef",
                                                        "gl_op_adamw_clip_step", "gl_op_adamw_ema_clip_step", "gl_train_set_loss_weights"}
    raw = ctypes.CDLL(str(table.LIB_PATH))
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes == table.TRAIN_RUN_SYMBOLS[name][1] and getattr(lib, name).restype == table.TRAIN_RUN_SYMBOLS[name][0]
    others = {k: v for k, v in vars(table).items() if k.endswith("SYMBOLS") and k != "TRAIN_RUN_SYMBOLS" and isinstance(v, dict)}
    assert len(others) >= 18 and "TRAINER_SYMBOLS" in others and "SYMBOLS" in others
    assert not {k: declared & set(v) for k, v in others.items() if declared & set(v)}
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != HEADER:
            assert not declared & set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read())), other
    # and the other way round: nothing another header declares is named with a parenthesis here
    mentioned = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", text))
    assert mentioned == declared, mentioned - declared
    # the clipped updates take their unclipped entry point's arguments with `coef` in front of the stream
    a, b = table.SYMBOLS["gl_op_adamw_step"][1], table.TRAIN_RUN_SYMBOLS["gl_op_adamw_clip_step"][1]
    assert b == a[:-1] + [ctypes.c_void_p] + a[-1:]
    a, b = table.TRAINER_SYMBOLS["gl_op_adamw_ema_step"][1], table.TRAIN_RUN_SYMBOLS["gl_op_adamw_ema_clip_step"][1]
    assert b == a[:-1] + [ctypes.c_void_p] + a[-1:]
    # the host-only count, and the geometry the header states
    from gligen_amd.engine import Engine
    chunk = Engine.GRAD_NORM_GRID[0]
    assert Engine.GRAD_NORM_GRID == R.GRID and chunk == R.BLOCK * Engine.GRAD_NORM_GRID[1]
    assert re.search(r"#define GL_GRAD_NORM_CHUNK %d\b" % chunk, text) and re.search(r"#define GL_GRAD_NORM_CHAIN %d\b" % Engine.GRAD_NORM_GRID[1], text)
    for n, want in ((-5, 0), (0, 0), (1, 1), (chunk, 1), (chunk + 1, 2), (209_000_000, R.partial_count(209_000_000)), (2 ** 40 + 1, 2 ** 40 // chunk + 1)):
        assert lib.gl_grad_sqnorm_partials(n) == want, n


# ---- 2. the ISA
def test_train_run_unit_isa(tmp_path):
    """train_run.hip for gfx950, device only: no kernel name in common with the five units behind train_impl.h or with train_optim
    (the build has no relocatable device code); the clipped AdamW kernels use no scratch and no LDS, move their data with 16-byte
    loads and stores and have no v_pk_fma_f32, as adamw_ema_kernel is held; the accumulate and norm kernels, which promise one
    rounding per product and sum and have no division to expand, contain no fused multiply-add at all; no kernel of the unit
    contains an atomic."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    units = ["train_run", "train_optim", "train_ops", "train_attention", "train_layers", "train_spatial", "train_unet"]

    def listing(unit):
        out = tmp_path / (unit + ".s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--offload-device-only", "-S",
                            os.path.join(ROOT, "gligen_amd", "csrc", unit + ".hip"), "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return out.read_text()

    with ThreadPoolExecutor(max_workers=len(units)) as ex:
        asm = dict(zip(units, ex.map(listing, units)))
    kernels = {u: set(re.findall(r"\.amdhsa_kernel (\S+)", a)) for u, a in asm.items()}
    mine = kernels["train_run"]
    for want in ("grad_accum_kernel", "grad_sqnorm_kernel", "clip_coef_kernel", "adamw_clip_kernel", "weighted_mse_kernel"):
        assert any(want in k for k in mine), (want, mine)
    assert len([k for k in mine if "grad_accum_kernel" in k]) == 3 and len([k for k in mine if "adamw_clip_kernel" in k]) == 2
    for u in units[1:]:
        assert not mine & kernels[u], (u, mine & kernels[u])
    a = asm["train_run"]
    body = lambda name: a[a.index(name + ":"):a.index(".Lfunc_end", a.index(name + ":"))]
    for name in mine:
        assert "atomic" not in body(name), name
    clipped = sorted(k for k in mine if "adamw_clip_kernel" in k)
    for name in clipped:
        blk = a[a.index(".amdhsa_kernel " + name):a.index(".end_amdhsa_kernel", a.index(".amdhsa_kernel " + name))]
        assert int(re.search(r"private_segment_fixed_size (\d+)", blk).group(1)) == 0
        assert int(re.search(r"group_segment_fixed_size (\d+)", blk).group(1)) == 0
        b = body(name)
        assert "scratch_" not in b and "ds_" not in b
        assert "v_pk_fma_f32" not in b, name            # (v_fma_f32 itself belongs to the expansions of the division and sqrtf)
        assert "global_load_dwordx4" in b and "global_store_dwordx4" in b, name      # the vector path moves 16 bytes per lane and access
    for name in mine:
        if "grad_accum_kernel" in name or "grad_sqnorm_kernel" in name:
            assert "global_load_dwordx4" in body(name) and "v_pk_fma_f32" not in body(name) and not re.search(r"\bv_fma(c|ak|mk)?_f32\b", body(name)), name


# ---- 3. the schedule on a recording stand-in engine
class RecEngine:
    """Engine for TrainStep and the Trainer on the CPU that records every call in order and implements the new operators in torch
    fp32 in the kernels' operation order (tests/train_run_ref.py). strict: today's signatures only, as the stand-ins of
    tests/test_trainer_cpu.py, test_dist_cpu.py and test_host_cpu.py have them -- any new keyword is a TypeError."""
    device = torch.device("cpu")

    def __init__(self, grads_of=None):
        self.calls, self.n_steps = [], 0
        self.grads_of = grads_of or (lambda call, k, shape: torch.randn(shape, generator=torch.Generator().manual_seed(1000 * call + len(k))))

    def _fb(self, grads, extra):
        self.calls.append(("fb",) + extra)
        for k in sorted(grads):
            grads[k].copy_(self.grads_of(self.n_steps, k, grads[k].shape))
        self.n_steps += 1
        return torch.tensor([float(self.n_steps)]), torch.zeros(1), grads

    def unet_train_step(self, cfg, params, batch, fuser_scale=1.0, trainable=None, grads=None, checkpoint=False, loss_weights=None):
        return self._fb(grads, () if loss_weights is None else (("loss_weights", tuple(loss_weights.tolist())),))

    def train_wait_grads(self, index, stream=None):
        self.calls.append(("wait", index))

    def _adamw(self, p, g, m, v, step, lr, betas, eps, weight_decay):
        m.mul_(betas[0]).add_(g, alpha=1 - betas[0]); v.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
        p.mul_(1 - lr * weight_decay).addcdiv_(m / (1 - betas[0] ** step), (v / (1 - betas[1] ** step)).sqrt() + eps, value=-lr)

    def op_adamw_step(self, p, g, m, v, step, lr, betas, eps, weight_decay):
        self.calls.append(("adamw", p.data_ptr(), step, lr))
        self._adamw(p, g, m, v, step, lr, betas, eps, weight_decay)

    def op_adamw_ema_step(self, p, g, m, v, ema, step, *, ema_rate, lr, betas, eps, weight_decay):
        self.calls.append(("adamw_ema", p.data_ptr(), step, lr))
        self._adamw(p, g, m, v, step, lr, betas, eps, weight_decay)
        ema.mul_(ema_rate).add_(p, alpha=1 - ema_rate)

    # the new operators
    def op_grad_accumulate(self, acc, g, mode, k):
        self.calls.append(("accum", g.data_ptr(), mode, k))
        if mode == "first":
            acc.copy_(g)
        elif mode == "middle":
            acc.add_(g)
        else:
            g.copy_((acc + g) * torch.tensor(1.0 / k, dtype=torch.float32))

    def grad_sqnorm_partials(self, n):
        return R.partial_count(n)

    def op_grad_sqnorm(self, g, partials=None):
        self.calls.append(("sqnorm", g.data_ptr()))
        partials.copy_(R.emulate_sqnorm_partials(g))
        return partials

    def op_clip_coef(self, partials, max_norm, out2=None):
        self.calls.append(("coef", max_norm))
        norm = partials.double().sum().sqrt().float()
        c = torch.tensor(max_norm, dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32))
        out2[0], out2[1] = norm, torch.where(c > 1, torch.ones_like(c), c)
        return out2

    def op_adamw_clip_step(self, p, g, m, v, step, *, coef, lr, betas, eps, weight_decay):
        self.calls.append(("adamw_clip", p.data_ptr(), step, lr))
        assert coef.numel() == 1
        self._adamw(p, g * coef, m, v, step, lr, betas, eps, weight_decay)

    def op_adamw_ema_clip_step(self, p, g, m, v, ema, step, *, ema_rate, coef, lr, betas, eps, weight_decay):
        self.calls.append(("adamw_ema_clip", p.data_ptr(), step, lr))
        self._adamw(p, g * coef, m, v, step, lr, betas, eps, weight_decay)
        ema.mul_(ema_rate).add_(p, alpha=1 - ema_rate)

    def train_step_inputs(self, z, noise, timesteps, schedule, *, boxes=None, mask=None, inpaint=False):
        a = schedule["sqrt_alphas_cumprod"][timesteps].reshape(-1, 1, 1, 1)
        s = schedule["sqrt_one_minus_alphas_cumprod"][timesteps].reshape(-1, 1, 1, 1)
        self.last_t = timesteps.clone()
        return dict(x_rows=(a * z + s * noise).permute(0, 2, 3, 1).contiguous(), target_rows=noise.permute(0, 2, 3, 1).contiguous(), timesteps=timesteps.float())


class TodaysEngine(RecEngine):
    """The strict form: the signatures of the existing stand-ins and nothing else."""

    def unet_train_step(self, cfg, params, batch, fuser_scale=1.0, trainable=None, grads=None, checkpoint=False):
        return self._fb(grads, ())

    op_grad_accumulate = grad_sqnorm_partials = op_grad_sqnorm = op_clip_coef = op_adamw_clip_step = op_adamw_ema_clip_step = None


def recorded_step(eng, **kw):
    """A TrainStep over the tiny state_dict in several buckets whose exchanges land in the engine's call list."""
    ts = TrainStep(eng, {}, tiny_state_dict(), bucket_mb=1e-4, world=1, **kw)
    real = ts.gbuf.all_reduce_bucket

    def exchange(i, average=True, even_alone=False):
        eng.calls.append(("exchange", i))
        return real(i, average=average, even_alone=even_alone)

    ts.gbuf.all_reduce_bucket = exchange
    return ts


def test_schedule_defaults_are_todays_and_the_new_order():
    """With every option at its default the engine sees exactly today's calls with today's keywords (an engine that accepts nothing
    else runs), in all three schedules. accumulate = 3 with max_grad_norm = 1: calls one and two of a group are the backward and one
    accumulate per bucket -- no exchange, no update, `steps` and the rate do not move --; call three runs, per bucket, (wait,) last,
    exchange, sqnorm, then one coef, then the clipped updates. Both schedules give the same bits, and an open group is dropped by the
    loaders."""
    for overlap in (True, False):
        eng = TodaysEngine()
        ts = recorded_step(eng, lr=0.1, overlap=overlap)
        assert ts.accumulate == 1 and ts.max_grad_norm is None and ts.acc is None and ts.grad_norm is None and ts.at_boundary and ts.micro == 0
        nb = len(ts.gbuf.buckets)
        assert nb >= 2
        ts.step({}); ts.step({})
        p = [b.data_ptr() for b in ts.pbuf.buckets]
        one = lambda s: [("fb",)] + ([x for i in range(nb) for x in (("wait", ts.bucket_ready[i]), ("exchange", i), ("adamw", p[i], s, 0.1))] if overlap else
                                     [("exchange", i) for i in range(nb)] + [("adamw", p[i], s, 0.1) for i in range(nb)])
        assert eng.calls == one(1) + one(2) and ts.steps == 2 and ts.at_boundary
    with pytest.raises(ValueError, match="accumulate"):
        TrainStep(RecEngine(), {}, tiny_state_dict(), world=1, accumulate=0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        TrainStep(RecEngine(), {}, tiny_state_dict(), world=1, max_grad_norm=-1.0)
    assert TrainStep(RecEngine(), {}, tiny_state_dict(), world=1, max_grad_norm=0).max_grad_norm is None       # 0 also means off

    rates = []

    def lr(step):
        rates.append(step)
        return 0.1 * step

    final = {}
    for overlap in (True, False):
        eng = RecEngine()
        ts = recorded_step(eng, lr=lr, overlap=overlap, accumulate=3, max_grad_norm=1.0, weight_decay=0.01)
        nb = len(ts.gbuf.buckets)
        assert len(ts.acc) == nb and all(a.data_ptr() != g.data_ptr() and a.shape == g.shape for a, g in zip(ts.acc, ts.gbuf.buckets))
        g = [b.data_ptr() for b in ts.gbuf.buckets]
        p = [b.data_ptr() for b in ts.pbuf.buckets]
        want = []
        for group in (1, 2):
            del rates[:]
            for micro, mode in ((1, "first"), (2, "middle")):
                before = len(eng.calls)
                ts.step({})
                assert eng.calls[before:] == [("fb",)] + [("accum", g[i], mode, 3) for i in range(nb)]
                assert ts.micro == micro and not ts.at_boundary and ts.steps == group - 1 and rates == []
            before = len(eng.calls)
            ts.step({})
            per_bucket = lambda i: ([("wait", ts.bucket_ready[i])] if overlap else []) + [("accum", g[i], "last", 3), ("exchange", i), ("sqnorm", g[i])]
            want = [("fb",)] + [x for i in range(nb) for x in per_bucket(i)] + [("coef", 1.0)] + [("adamw_clip", p[i], group, 0.1 * group) for i in range(nb)]
            assert eng.calls[before:] == want
            assert ts.micro == 0 and ts.at_boundary and ts.steps == group and rates == [group]
        assert float(ts.grad_norm) > 1.0 and ts.grad_norm.data_ptr() == ts._clip.data_ptr() and 0 < float(ts._clip[1]) < 1
        final[overlap] = ts
        # an open group does not survive a load
        ts.step({})
        assert ts.micro == 1
        ts.load_state_dict(ts.state_dict())
        assert ts.micro == 0
        ts.step({})
        ts.load_optimizer_state_dict(ts.optimizer_state_dict())
        assert ts.micro == 0
        ts.step({})
        ts.load_torch_optimizer_state_dict(ts.torch_optimizer_state_dict())
        assert ts.micro == 0 and ts.steps == 2
    assert all(torch.equal(a, b) for a, b in zip(final[True].pbuf.buckets, final[False].pbuf.buckets))
    # the gradient buffer holds the unclipped mean of the group: ((g1 + g2) + g3) * fl(1/3)
    eng, ts = RecEngine(), None
    ts = recorded_step(eng, lr=0.1, accumulate=3, max_grad_norm=1.0)
    for _ in range(3):
        ts.step({})
    for k, view in ts.gbuf.views.items():
        assert torch.equal(view, R.accumulate_ref([eng.grads_of(c, k, view.shape) for c in range(3)])), k
    # an EMA takes the clipped fused update; loss weights reach the engine only when given
    eng = RecEngine()
    ts = recorded_step(eng, lr=0.1, max_grad_norm=1.0, ema_rate=0.5)
    ts.step({}, loss_weights=torch.tensor([0.25, 1.0]))
    assert eng.calls[0] == ("fb", ("loss_weights", (0.25, 1.0))) and [c[0] for c in eng.calls if c[0].startswith("adamw")] == ["adamw_ema_clip"] * len(ts.pbuf.buckets)
    lora_kw = __import__("inspect").signature(__import__("gligen_amd.lora_train", fromlist=["x"]).LoraTrainStep.__init__).parameters
    assert lora_kw["accumulate"].default == 1 and lora_kw["max_grad_norm"].default is None


# ---- 4. two gloo ranks
RANKS_WORKER = textwrap.dedent("""
    import os, sys, json
    sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
    import torch
    import torch.distributed as tdist
    import train_run_ref as R
    from test_train_run_cpu import RecEngine, tiny_state_dict
    from gligen_amd import dist as gdist
    from gligen_amd.train import TrainStep
    rank, local_rank, world = gdist.init_from_env(backend="gloo")
    n_coll = [0]
    real_all_reduce = tdist.all_reduce
    def counted(*a, **kw):
        n_coll[0] += 1
        return real_all_reduce(*a, **kw)
    tdist.all_reduce = counted

    def grads_of(r):       # other gradients on every rank and for every micro-batch
        return lambda call, k, shape: torch.randn(shape, generator=torch.Generator().manual_seed(100003 * r + 1000 * call + len(k)))

    class Eng(RecEngine):  # the clipped update through the real torch.optim.AdamW, on the bucket's own flat layout
        def op_adamw_clip_step(self, p, g, m, v, step, *, coef, lr, betas, eps, weight_decay):
            P = torch.nn.Parameter(p)                          # (shares p's memory)
            opt = torch.optim.AdamW([P], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
            if step > 1:
                opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=m, exp_avg_sq=v)
            P.grad = g * coef
            opt.step()
            if step == 1:
                m.copy_(opt.state[P]["exp_avg"]); v.copy_(opt.state[P]["exp_avg_sq"])

    HYPER = dict(lr=0.05, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
    K, MAXN = 2, 0.5
    eng = Eng(grads_of(rank))
    ts = TrainStep(eng, {{}}, tiny_state_dict(), bucket_mb=1e-4, world=world, accumulate=K, max_grad_norm=MAXN, **HYPER)
    nb = len(ts.gbuf.buckets)
    start = [b.clone() for b in ts.pbuf.buckets]
    norms = []
    for call in range(2 * K):
        ts.step({{}})
        if ts.at_boundary:
            norms.append(float(ts.grad_norm))
    clipped_coll = n_coll[0]
    # two plain steps issue as many collectives
    n_coll[0] = 0
    plain = TrainStep(Eng(grads_of(rank)), {{}}, tiny_state_dict(), bucket_mb=1e-4, world=world, **HYPER)
    plain.step({{}}); plain.step({{}})
    plain_coll = n_coll[0]

    # the reference, in one process: the mean gradient formed in the same fp32 order, its norm in the kernel's order, then
    # torch.optim.AdamW on the bucket-shaped parameters; beside it torch's own clip_grad_norm_ on the same mean
    def bucket_of(r, call, i):
        buf = torch.zeros_like(ts.gbuf.buckets[i])
        for name, off, n, shape in ts.gbuf.layout[i]:
            buf[off:off + n] = grads_of(r)(call, name, shape).reshape(-1)
        return buf
    ref = [torch.nn.Parameter(b.clone()) for b in start]
    opt = torch.optim.AdamW(ref, **HYPER)
    tref = [torch.nn.Parameter(b.clone()) for b in start]
    topt = torch.optim.AdamW(tref, **HYPER)
    ref_norms, torch_norms, coefs = [], [], []
    for step in range(2):
        mean = []
        for i in range(nb):
            per_rank = [R.accumulate_ref([bucket_of(r, step * K + c, i) for c in range(K)]) for r in range(world)]
            mean.append((per_rank[0] + per_rank[1]) / world)
        partials = torch.cat([R.emulate_sqnorm_partials(b) for b in mean])
        norm = partials.double().sum().sqrt().float()
        c = torch.tensor(MAXN, dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32))
        coef = torch.where(c > 1, torch.ones_like(c), c)
        ref_norms.append(float(norm)); coefs.append(float(coef))
        for q, b in zip(ref, mean):
            q.grad = b * coef
        opt.step()
        for q, b in zip(tref, mean):
            q.grad = b.clone()
        torch_norms.append(float(torch.nn.utils.clip_grad_norm_(tref, MAXN, norm_type=2, error_if_nonfinite=False)))
        topt.step()
    same = all(torch.equal(a, b.detach()) for a, b in zip(ts.pbuf.buckets, ref))
    near = max(float((a - b.detach()).abs().max()) for a, b in zip(ts.pbuf.buckets, tref))
    digest = [float(b.double().sum()) for b in ts.pbuf.buckets]
    print("RESULT " + json.dumps(dict(rank=rank, same=same, near=near, nb=nb, clipped_coll=clipped_coll, plain_coll=plain_coll, norms=norms, ref_norms=ref_norms,
                                      torch_norms=torch_norms, coefs=coefs, digest=digest, moved=not torch.equal(ts.pbuf.buckets[0], start[0]))))
    gdist.shutdown()
""")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_gloo_ranks_accumulate_and_clip(tmp_path):
    """Two ranks whose gradients differ per rank and per micro-batch, K = 2, max_grad_norm below the norm, two optimizer steps: both
    ranks hold bit for bit the parameters of torch.optim.AdamW on coef times the mean gradient, the mean formed in the same fp32 order
    ((g1 + g2) * 0.5 per rank, the sum over the ranks, / world) and the norm in the kernel's order; torch's own clip_grad_norm_ on that
    mean returns the same norm up to its summation order and leads to the same parameters up to that; the number of collectives is
    that of two plain steps, and grad_norm is the same on both ranks."""
    port = _free_port()
    script = tmp_path / "ranks_worker.py"
    script.write_text(RANKS_WORKER.format(root=ROOT))
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    res = {}
    for p in procs:
        out, err = p.communicate(timeout=180)
        assert p.returncode == 0, err[-3000:]
        r = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
        res[r["rank"]] = r
    for r in res.values():
        assert r["same"] and r["moved"] and r["nb"] >= 2, r
        assert r["clipped_coll"] == r["plain_coll"] == 2 * r["nb"], r
        assert r["norms"] == r["ref_norms"] and all(n > 0.5 for n in r["norms"]) and all(0 < c < 1 for c in r["coefs"]), r
        assert all(abs(a - b) <= 4 * R.U32 * b for a, b in zip(r["norms"], r["torch_norms"])), r       # < 300 terms: another order, a few ulp
        assert r["near"] < 1e-6, r
    assert res[0]["digest"] == res[1]["digest"] and res[0]["norms"] == res[1]["norms"]


# ---- the Trainer on the stand-in engine
def tiny_batches(start=0):
    i = start
    while True:
        g = torch.Generator().manual_seed(500 + i)
        yield dict(i=i, z=torch.randn(2, 4, 8, 8, generator=g), context=torch.randn(2, 77, 768, generator=g), **syn.make_batch("text", 2, n_valid=2, seed=i))
        i += 1


def tiny_config(out, **kw):
    return dict(dict(model=TINY_CFG, base_learning_rate=0.01, weight_decay=0.01, warmup_steps=2, scheduler_type="constant", total_iters=4, enable_ema=False,
                     inpaint_mode=False, save_every_iters=2, output_dir=str(out), ckpt=None, gradient_accumulation_steps=2, max_grad_norm=1.0, min_snr_gamma=5.0), **kw)


def test_trainer_counts_optimizer_steps_and_refuses_another_k(tmp_path):
    """total_iters, warmup_steps and save_every_iters count optimizer steps and an iteration draws K batches; the batch callable gets
    the number of batches consumed; the checkpoint's config_dict carries the three keys; a run in two pieces ends where the run in one
    does; min-SNR weights reach the engine per micro-batch as weights[t]; resuming with another K is refused by name, and a checkpoint
    without the key counts as K = 1."""
    from gligen_amd import trainer as T
    starts, logs = [], []

    def batches(start):
        starts.append(start)
        return tiny_batches(start)

    eng = RecEngine()
    tr = T.Trainer(eng, tiny_config(tmp_path / "a"), tiny_state_dict(), batches, seed=5, log=logs.append)
    assert tr.start_training() == 4 and tr.iters == 4 and tr.ts.steps == 4 and eng.n_steps == 8 and starts == [0]
    nb = len(tr.ts.pbuf.buckets)
    sched = warmup_schedule(0.01, 2)
    assert [c[3] for c in eng.calls if c[0] == "adamw_clip"][::nb] == [sched(i + 1) for i in range(4)]
    assert sorted(os.listdir(tmp_path / "a")) == ["checkpoint_00000001.pth", "checkpoint_00000003.pth", "checkpoint_00000004.pth", "checkpoint_latest.pth"]
    ck = torch.load(tmp_path / "a" / "checkpoint_latest.pth", weights_only=False)
    assert ck["iters"] == 4 and float(ck["opt"]["state"][0]["step"]) == 4
    assert (ck["config_dict"]["gradient_accumulation_steps"], ck["config_dict"]["max_grad_norm"], ck["config_dict"]["min_snr_gamma"]) == (2, 1.0, 5.0)
    assert "grad_norm" in logs[0] and "loss 1.5" in logs[0]          # the mean of the two micro-losses (the stand-in's are 1 and 2)
    table = min_snr_weights(tr.diffusion.alphas_cumprod, 5.0)
    fbs = [c for c in eng.calls if c[0] == "fb"]
    assert len(fbs) == 8 and all(len(c) == 2 and c[1][0] == "loss_weights" for c in fbs)
    assert fbs[-1][1][1] == tuple(table[eng.last_t].tolist())
    # two pieces
    e1 = RecEngine()
    t1 = T.Trainer(e1, tiny_config(tmp_path / "b", total_iters=2), tiny_state_dict(), batches, seed=5, log=lambda s: None)
    t1.start_training()
    e2 = RecEngine()
    e2.n_steps = 4
    t2 = T.Trainer(e2, tiny_config(tmp_path / "b"), tiny_state_dict(), batches, seed=77, log=lambda s: None)
    assert t2.starting_iter == 2 and starts[-1] == 4
    assert t2.start_training() == 4
    a, b = tr.state(), t2.state()
    assert all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"])
    assert all(torch.equal(torch.as_tensor(a["opt"]["state"][i][k]), torch.as_tensor(b["opt"]["state"][i][k])) for i in a["opt"]["state"] for k in a["opt"]["state"][i])
    assert torch.equal(e2.last_t, eng.last_t)
    with pytest.raises(ValueError, match="gradient_accumulation_steps"):
        T.Trainer(RecEngine(), tiny_config(tmp_path / "b", gradient_accumulation_steps=3), tiny_state_dict(), batches, log=lambda s: None)
    ck = torch.load(tmp_path / "b" / "checkpoint_latest.pth", weights_only=False)
    del ck["config_dict"]["gradient_accumulation_steps"]
    torch.save(ck, tmp_path / "nokey.pth")
    with pytest.raises(ValueError, match="gradient_accumulation_steps = 1"):
        T.Trainer(RecEngine(), tiny_config(tmp_path / "c"), tiny_state_dict(), batches, resume=str(tmp_path / "nokey.pth"), log=lambda s: None)
    assert T.Trainer(RecEngine(), tiny_config(tmp_path / "d", gradient_accumulation_steps=1), tiny_state_dict(), batches, resume=str(tmp_path / "nokey.pth"),
                     log=lambda s: None).starting_iter == 4
    import inspect
    src = inspect.getsource(T.main)
    assert all(f'"--{o}"' in src for o in ("gradient_accumulation_steps", "max_grad_norm", "min_snr_gamma"))
    # the defaults: off, and today's engine is enough
    plain = T.Trainer(TodaysEngine(), {k: v for k, v in tiny_config(tmp_path / "e").items() if k not in ("gradient_accumulation_steps", "max_grad_norm", "min_snr_gamma")},
                      tiny_state_dict(), batches, log=lambda s: None)
    assert (plain.accumulate, plain.max_grad_norm, plain.min_snr_gamma, plain.snr_weights) == (1, None, None, None)
    assert plain.start_training() == 4 and plain.engine.n_steps == 4


# ---- 5. min-SNR
def test_min_snr_weights_against_float64():
    """min(snr, gamma) / snr on the reference's schedule (linear in sqrt(beta), 0.00085 -> 0.012, 1000 steps) against the float64 formula
    rounded once; exactly 1 where snr <= gamma, below 1 at t = 0, monotone, in (0, 1] for gamma = 5."""
    ac = R.reference_alphas_cumprod()
    snr = ac / (1.0 - ac)
    for gamma in (5.0, 1.0, 20.0):
        w = min_snr_weights(ac, gamma)
        assert w.dtype == torch.float32 and tuple(w.shape) == (1000,)
        assert torch.equal(w, R.min_snr_ref(ac, gamma).float())
        assert bool((w[snr <= gamma] == 1.0).all()) and bool((w[snr > gamma] < 1.0).all()) and float(w[0]) < 1.0
        assert bool((w[1:] >= w[:-1]).all())                              # snr falls with t, so the weight rises to 1 and stays
        assert bool((w > 0).all()) and bool((w <= 1).all())
        assert 0 < int((snr > gamma).sum()) < 1000
    w5 = min_snr_weights(ac, 5.0)
    assert float(w5[20]) < 0.2 and float(w5[600]) == 1.0                # the two timesteps of the device test: both branches
    from ldm.models.diffusion.ldm import LatentDiffusion
    d = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
    # the model's buffer is the fp32 rounding of ac: w = gamma (1 - a) / a moves by u (1 / (1 - a) + 1) relatively, most at t = 0
    rtol = R.U32 * (1.0 / float(1.0 - ac[0]) + 1.0) + R.U32
    assert 5e-5 < rtol < 1e-4
    torch.testing.assert_close(min_snr_weights(d.alphas_cumprod, 5.0), w5, rtol=rtol, atol=0)
    with pytest.raises(ValueError, match="gamma"):
        min_snr_weights(ac, 0.0)


# ---- 6. the ref module's own consistency
def test_weighted_loss_restatement_is_autograds():
    g = torch.Generator().manual_seed(1)
    eps = torch.randn(2, 4, 16, 16, generator=g, dtype=torch.float64).requires_grad_(True)
    noise = torch.randn(2, 4, 16, 16, generator=g, dtype=torch.float64)
    w = torch.tensor([0.125, 1.75], dtype=torch.float64)
    loss = (w[:, None, None, None] * (eps - noise) ** 2).mean()
    loss.backward()
    loss_r, dy_r = R.weighted_loss_ref(eps.detach(), noise, w)
    torch.testing.assert_close(loss_r, loss.detach(), rtol=1e-14, atol=0)
    torch.testing.assert_close(dy_r, eps.grad, rtol=1e-13, atol=1e-300)
    ones_loss, _ = R.weighted_loss_ref(eps.detach(), noise, torch.ones(2))
    torch.testing.assert_close(ones_loss, torch.nn.functional.mse_loss(eps.detach(), noise), rtol=1e-14, atol=0)


def sqnorm_cases(n, seed=0):
    """The device test's data kinds for one n."""
    g = torch.Generator().manual_seed(seed + n % 9973)
    x = torch.randn(n, generator=g)
    spike = x.clone()
    spike[n // 2] = 1e6
    return {"normal": x, "zeros": torch.zeros(n), "one element 1e6": spike}


@pytest.mark.parametrize("n", [1, 5, 1027, 16384, 16385, 100003])
def test_sqnorm_chain_emulation_stays_within_the_derived_bound(n):
    """The fp32 emulation of grad_sqnorm_kernel's chain (fp32 thread chains, butterfly, wave sums; the partials summed in double)
    against the float64 norm: inside norm_bound for every data kind of the device test, the zeros exactly; the bound itself is a
    few 1e-6 relative -- it has to be able to fail."""
    assert R.partial_count(n) == -(-n // R.GRID[0])
    for kind, x in sqnorm_cases(n).items():
        partials = R.emulate_sqnorm_partials(x)
        assert partials.numel() == R.partial_count(n)
        norm = float(partials.double().sum().sqrt().float())
        norm64 = float(x.double().pow(2).sum().sqrt())
        bound = R.norm_bound(norm64, n)
        assert abs(norm - norm64) <= bound, (kind, norm, norm64, bound)
        if kind == "zeros":
            assert norm == 0.0 and bound == pytest.approx((1 + 4.4e-6) * (n * R.TINY) ** 0.5, rel=1e-3)
        else:
            assert bound <= 4.5e-6 * norm64 + 1e-12, (kind, bound / norm64)
        if norm64 > 0:       # the coefficient formed in fp32 from the emulated norm, as clip_coef_kernel forms it
            mx = R.f32(0.5 * norm64)
            c = float(torch.tensor(mx, dtype=torch.float32) / (torch.tensor(norm, dtype=torch.float32) + torch.tensor(1e-6, dtype=torch.float32)))
            assert abs(min(1.0, c) - R.coef_ref(norm64, mx)) <= R.coef_bound(norm64, n, mx), (kind, c)
            assert R.coef_bound(norm64, n, mx) < 3e-6
