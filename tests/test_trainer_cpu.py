"""The training run around TrainStep, host side and pinning, no GPU: the entry point of include/gligen_amd_trainer.h (declared,
exported, bound), the ISA of the fused AdamW + EMA kernel, the trainable parameter order against the reference's
(tests/golden/trainable_order.json, tools/make_golden_trainer.py), the optimizer state in torch.optim.AdamW's layout in both
directions, TrainStep's call pattern with and without an EMA, the Trainer's loop / checkpoints / resume / timestep draw on a CPU
stand-in engine, and Engine.count_spatial_transformers with the guard it makes live."""
import ctypes
import json
import os
import random
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

from helpers import GOLDEN, ROOT
from gligen_amd import synthetic as syn
from gligen_amd.train import TrainStep, trainable_names, warmup_schedule

FUSER_W = "input_blocks.1.1.transformer_blocks.0.fuser.linear.weight"
FUSER_A = "input_blocks.1.1.transformer_blocks.0.fuser.alpha_attn"
PN_W = "position_net.linears.0.weight"
TINY_CFG = dict(in_channels=4, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=False)


def tiny_state_dict():
    """A state_dict with the reference's key names and a handful of values: three trainable tensors (module order: the first conv
    in front, the fuser's, position_net's at the end) and two frozen ones."""
    g = torch.Generator().manual_seed(3)
    return {"input_blocks.0.0.weight": torch.randn(8, 4, 3, 3, generator=g), FUSER_A: torch.randn((), generator=g), FUSER_W: torch.randn(16, 8, generator=g),
            "out.2.weight": torch.randn(4, 4, generator=g), PN_W: torch.randn(12, 5, generator=g)}


class FakeEngine:
    """What Engine does for TrainStep and the Trainer, on the CPU: gradients drawn from a generator seeded by the call count (or the
    ones in `self.grads`), torch's AdamW arithmetic, the EMA as the reference's update_ema, q_sample rows in torch."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls, self.grads, self.n_steps = [], None, 0

    def unet_train_step(self, cfg, params, batch, fuser_scale=1.0, trainable=None, grads=None, checkpoint=False):
        g = torch.Generator().manual_seed(100 + self.n_steps)
        self.n_steps += 1
        for k in sorted(grads):
            grads[k].copy_(self.grads[k] if self.grads is not None else torch.randn(grads[k].shape, generator=g))
        return torch.tensor([float(sum(float(p.double().sum()) for p in params.values()))]), torch.zeros(1), grads

    def train_wait_grads(self, index, stream=None):
        pass

    def op_adamw_step(self, p, g, m, v, step, lr, betas, eps, weight_decay):
        self.calls.append(("adamw", p.data_ptr(), None, step, lr))
        m.mul_(betas[0]).add_(g, alpha=1 - betas[0]); v.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
        p.mul_(1 - lr * weight_decay).addcdiv_(m / (1 - betas[0] ** step), (v / (1 - betas[1] ** step)).sqrt() + eps, value=-lr)

    def op_adamw_ema_step(self, p, g, m, v, ema, step, *, ema_rate, lr, betas, eps, weight_decay):
        FakeEngine.op_adamw_step(self, p, g, m, v, step, lr, betas, eps, weight_decay)
        self.calls[-1] = ("adamw_ema", p.data_ptr(), ema.data_ptr(), step, lr)
        ema.mul_(ema_rate).add_(p, alpha=1 - ema_rate)

    def train_step_inputs(self, z, noise, timesteps, schedule, *, boxes=None, mask=None, inpaint=False):
        a = schedule["sqrt_alphas_cumprod"][timesteps].reshape(-1, 1, 1, 1)
        s = schedule["sqrt_one_minus_alphas_cumprod"][timesteps].reshape(-1, 1, 1, 1)
        self.last_t = timesteps.clone()
        return dict(x_rows=(a * z + s * noise).permute(0, 2, 3, 1).contiguous(), target_rows=noise.permute(0, 2, 3, 1).contiguous(), timesteps=timesteps.float())


def _declared(header):
    return set(re.findall(r"\bint (gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_trainer_entry_point_is_declared_exported_and_bound():
    """include/gligen_amd_trainer.h declares exactly the names of TRAINER_SYMBOLS, the built library exports them with the table's
    argument types, and the table shares no name with the other tables or headers."""
    from gligen_amd import _lib as table
    from gligen_amd.build import SOURCES, build_native
    assert "train_optim.hip" in SOURCES
    build_native()
    lib = table.load()
    declared = _declared("gligen_amd_trainer.h")
    assert declared == set(table.TRAINER_SYMBOLS) == {"gl_op_adamw_ema_step"}
    raw = ctypes.CDLL(str(table.LIB_PATH))
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes == table.TRAINER_SYMBOLS[name][1] and getattr(lib, name).restype == table.TRAINER_SYMBOLS[name][0]
    others = [table.SYMBOLS, table.IMAGE_SYMBOLS, table.MAP_SYMBOLS, table.TRAIN_MAP_SYMBOLS, table.TRAIN_INPUT_SYMBOLS, table.TRAIN_FUSER_SYMBOLS]
    assert not any(declared & set(t) for t in others)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "gligen_amd_trainer.h":
            assert not declared & set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read())), other
    # gl_op_adamw_step's arguments with `ema` behind `v` and `ema_rate` behind `weight_decay`
    a, b = table.SYMBOLS["gl_op_adamw_step"][1], table.TRAINER_SYMBOLS["gl_op_adamw_ema_step"][1]
    assert b == a[:5] + [a[4]] + a[5:11] + [ctypes.c_double] + a[11:]


def test_optimizer_unit_isa(tmp_path):
    """train_optim.hip for gfx950, device only: adamw_ema_kernel uses no scratch and no LDS, moves its data with 16-byte loads and
    stores, and the unit defines no kernel that one of the five units behind train_impl.h defines (tests/test_isa_cpu.py pins
    those at 80; the build has no relocatable device code, so a kernel is launched from the unit that defines it)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    units = ["train_optim", "train_ops", "train_attention", "train_layers", "train_spatial", "train_unet"]

    def listing(unit):
        out = tmp_path / (unit + ".s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--offload-device-only", "-S",
                            os.path.join(ROOT, "gligen_amd", "csrc", unit + ".hip"), "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return out.read_text()

    with ThreadPoolExecutor(max_workers=len(units)) as ex:
        asm = dict(zip(units, ex.map(listing, units)))
    kernels = {u: set(re.findall(r"\.amdhsa_kernel (\S+)", a)) for u, a in asm.items()}
    mine = kernels["train_optim"]
    assert len(mine) == 1 and "adamw_ema_kernel" in next(iter(mine)), mine
    for u in units[1:]:
        assert not mine & kernels[u], (u, mine & kernels[u])
    assert any("adamw_kernel" in k for k in kernels["train_ops"])          # AdamW alone stays where it was
    name = next(iter(mine))
    a = asm["train_optim"]
    blk = a[a.index(".amdhsa_kernel " + name):a.index(".end_amdhsa_kernel")]
    assert int(re.search(r"private_segment_fixed_size (\d+)", blk).group(1)) == 0
    assert int(re.search(r"group_segment_fixed_size (\d+)", blk).group(1)) == 0
    body = a[a.index(name + ":"):a.index(".Lfunc_end", a.index(name + ":"))]
    assert body.count("global_load_dwordx4") == 5 and body.count("global_store_dwordx4") == 4, (body.count("global_load_dwordx4"), body.count("global_store_dwordx4"))
    assert "scratch_" not in body and "atomic" not in body and "ds_" not in body
    # the shared update keeps its products and sums apart (adamw_update.h: contraction off), in both kernels
    assert "v_pk_fma_f32" not in body
    ops = asm["train_ops"]
    k = next(k for k in kernels["train_ops"] if "adamw_kernel" in k)
    assert "v_pk_fma_f32" not in ops[ops.index(k + ":"):ops.index(".Lfunc_end", ops.index(k + ":"))]


def fixture():
    return json.load(open(os.path.join(GOLDEN, "trainable_order.json")))


@pytest.mark.parametrize("entry", ["small_text", "small_canny", "small_text_inpaint"])
def test_trainable_parameter_order_is_the_references(entry):
    """trainable_names over this repository's UNetModel.state_dict() gives the reference's trainable named_parameters(), order
    included: the numbering of torch.optim.AdamW's state in a reference checkpoint."""
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    e = fixture()[entry]
    assert e["parameters_equal_state_dict_keys"]
    sd = UNetModel(**e["cfg"]).state_dict()
    assert len(sd) == e["n_parameters"]
    names = trainable_names(sd, e["cfg"])
    assert names == e["trainable"]
    if entry == "small_text":
        assert len(sd) == 413 and len(names) == 127 and names[0].endswith("fuser.alpha_attn") and names[-1] == "position_net.linears.4.bias"
    ts_order = TrainStep(FakeEngine(), e["cfg"], {k: torch.zeros(()) for k in sd}, world=1).param_order      # (scalars: the order alone)
    assert ts_order == e["trainable"]


def adamw_reference(sd, names, grads_per_step, lr, wd):
    ref = {k: sd[k].clone().requires_grad_(True) for k in names}
    opt = torch.optim.AdamW([ref[k] for k in names], lr=lr, weight_decay=wd)
    for grads in grads_per_step:
        for k in names:
            ref[k].grad = grads[k].clone()
        opt.step()
    return ref, opt


def test_torch_optimizer_state_both_directions():
    """Two steps of a real torch.optim.AdamW, its state_dict() loaded into a TrainStep, given back equal (tensors, step, params,
    the installed torch's param_groups keys), accepted by a fresh torch.optim.AdamW, and a third step taken by both sides from the
    same gradient agrees at the bar of test_adamw_step_matches_torch."""
    sd = tiny_state_dict()
    lr, wd = 0.1, 0.01
    names = trainable_names(sd, {})
    assert names == [FUSER_A, FUSER_W, PN_W]
    g = torch.Generator().manual_seed(9)
    grads = [{k: torch.randn(sd[k].shape, generator=g) for k in names} for _ in range(3)]
    ref, opt = adamw_reference(sd, names, grads[:2], lr, wd)
    saved = opt.state_dict()
    eng = FakeEngine()
    ts = TrainStep(eng, {}, sd, lr=lr, weight_decay=wd, bucket_mb=1e-4, world=1)
    assert len(ts.gbuf.buckets) >= 2 and ts.param_order == names
    fresh = ts.torch_optimizer_state_dict()
    assert fresh["state"] == {} and fresh["param_groups"][0]["params"] == [0, 1, 2]          # before the first step: torch's is empty too
    ts.load_state_dict({k: ref[k].detach() for k in names})
    ts.load_torch_optimizer_state_dict(saved)
    assert ts.steps == 2
    back = ts.torch_optimizer_state_dict()
    assert back["param_groups"][0]["params"] == list(range(len(names))) and len(back["param_groups"]) == 1
    assert set(back["param_groups"][0]) == set(saved["param_groups"][0])
    for key in ("lr", "betas", "eps", "weight_decay"):
        assert back["param_groups"][0][key] == saved["param_groups"][0][key], key
    assert sorted(back["state"]) == sorted(saved["state"]) == [0, 1, 2]
    for i in saved["state"]:
        assert set(back["state"][i]) == set(saved["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert type(back["state"][i]["step"]) is type(saved["state"][i]["step"]) and float(back["state"][i]["step"]) == float(saved["state"][i]["step"]) == 2
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][key], saved["state"][i][key]) and back["state"][i][key].shape == saved["state"][i][key].shape
    assert ts.torch_optimizer_state_dict(initial_lr=0.2)["param_groups"][0]["initial_lr"] == 0.2
    # a fresh torch optimizer takes it and steps on
    ref2 = {k: ref[k].detach().clone().requires_grad_(True) for k in names}
    opt2 = torch.optim.AdamW([ref2[k] for k in names], lr=lr, weight_decay=wd)
    opt2.load_state_dict(back)
    for k in names:
        ref2[k].grad = grads[2][k].clone()
    opt2.step()
    eng.grads = grads[2]
    ts.step({})
    out = ts.state_dict()
    assert ts.steps == 3
    for k in names:
        torch.testing.assert_close(out[k], ref2[k].detach(), rtol=1e-5, atol=1e-6)
    assert torch.equal(out["out.2.weight"], sd["out.2.weight"])
    # what does not fit is refused by name
    short = dict(saved, param_groups=[dict(saved["param_groups"][0], params=[0, 1])])
    with pytest.raises(ValueError, match=re.escape(PN_W)):
        ts.load_torch_optimizer_state_dict(short)
    bad = dict(saved, state={i: dict(s) for i, s in saved["state"].items()})
    bad["state"][1]["exp_avg"] = torch.zeros(8, 16)
    with pytest.raises(ValueError, match=re.escape(FUSER_W)):
        ts.load_torch_optimizer_state_dict(bad)


def test_train_step_call_pattern_with_and_without_ema():
    """ema_rate=None: op_adamw_step per bucket, never op_adamw_ema_step, no EMA buffer. A rate: only op_adamw_ema_step, once per
    bucket and step with that bucket's EMA buffer, in both schedules, which agree bit for bit; the EMA follows update_ema on the
    parameters after each update, and ema_state_dict / load_ema_state_dict are inverses."""
    sd = tiny_state_dict()
    eng = FakeEngine()
    ts = TrainStep(eng, {}, sd, lr=0.1, bucket_mb=1e-4, world=1)
    assert ts.ema is None and ts.ema_rate is None
    ts.step({}); ts.step({})
    nb = len(ts.pbuf.buckets)
    assert nb >= 2 and [c[0] for c in eng.calls] == ["adamw"] * (2 * nb)
    with pytest.raises(ValueError):
        ts.ema_state_dict()
    with pytest.raises(ValueError):
        TrainStep(FakeEngine(), {}, sd, world=1, ema_rate=1.5)
    runs = {}
    for overlap in (True, False):
        e = FakeEngine()
        t = TrainStep(e, {}, sd, lr=0.1, bucket_mb=1e-4, world=1, ema_rate=0.5, overlap=overlap)
        assert len(t.ema) == nb and all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(t.ema, t.pbuf.buckets))
        snaps = []
        for _ in range(3):
            t.step({})
            snaps.append(t.state_dict())
        assert [c[0] for c in e.calls] == ["adamw_ema"] * (3 * nb)
        for s in range(3):
            assert [(c[1], c[2], c[3]) for c in e.calls[s * nb:(s + 1) * nb]] == [(t.pbuf.buckets[i].data_ptr(), t.ema[i].data_ptr(), s + 1) for i in range(nb)]
        runs[overlap] = (t, snaps)
    (t, snaps), (t2, _) = runs[True], runs[False]
    ema = t.ema_state_dict()
    assert all(torch.equal(ema[k], t2.ema_state_dict()[k]) for k in ema) and all(torch.equal(a, b) for a, b in zip(t.pbuf.buckets, t2.pbuf.buckets))
    assert list(ema) == list(sd)
    for k in sd:
        if k in t.param_order:
            ref = sd[k].clone()
            for s in snaps:
                ref = ref * 0.5 + s[k] * 0.5
            torch.testing.assert_close(ema[k], ref, rtol=1e-6, atol=1e-7)
            assert not torch.equal(ema[k], snaps[-1][k])
        else:
            assert torch.equal(ema[k], sd[k])
    # the parameters are those of the run without an EMA
    plain = TrainStep(FakeEngine(), {}, sd, lr=0.1, bucket_mb=1e-4, world=1)
    for _ in range(3):
        plain.step({})
    assert all(torch.equal(plain.state_dict()[k], snaps[-1][k]) for k in sd)
    t3 = TrainStep(FakeEngine(), {}, sd, lr=0.1, bucket_mb=1e-4, world=1, ema_rate=0.5)
    t3.load_ema_state_dict(ema)
    assert all(torch.equal(t3.ema_state_dict()[k], ema[k]) for k in t.param_order)
    with pytest.raises(ValueError, match=re.escape(FUSER_W)):
        t3.load_ema_state_dict({k: v for k, v in ema.items() if k != FUSER_W})


def tiny_batches(start=0):
    i = start
    while True:
        g = torch.Generator().manual_seed(500 + i)
        yield dict(z=torch.randn(2, 4, 8, 8, generator=g), context=torch.randn(2, 77, 768, generator=g), **syn.make_batch("text", 2, n_valid=2, seed=i))
        i += 1


def tiny_config(out, **kw):
    return dict(dict(model=TINY_CFG, base_learning_rate=0.01, weight_decay=0.01, warmup_steps=4, scheduler_type="constant", total_iters=7, enable_ema=True,
                     ema_rate=0.9, inpaint_mode=False, save_every_iters=3, output_dir=str(out), ckpt=None), **kw)


def test_trainer_loop_checkpoints_and_resume(tmp_path):
    """Trainer on the stand-in engine: save() fires at iteration 0, at the multiples of save_every_iters and at the end (trainer.py:397);
    the file holds the reference's keys and layouts; iters positions the schedule (the first rate after a resume is
    warmup_schedule(...)(iters + 1)); a resumed run ends where the uninterrupted one does."""
    from gligen_amd import trainer as T
    saves = []
    real_save = T.Trainer.save

    def counted(self, path=None):
        saves.append(self.iters)
        return real_save(self, path)

    T.Trainer.save = counted
    try:
        eng = FakeEngine()
        tr = T.Trainer(eng, tiny_config(tmp_path / "a"), tiny_state_dict(), tiny_batches, seed=5, log=lambda s: None)
        assert tr.start_training() == 7
    finally:
        T.Trainer.save = real_save
    assert saves == [1, 4, 7]                   # iter_idx 0, 3, 6: "iter_idx + 1 as the actual name"
    assert sorted(os.listdir(tmp_path / "a")) == ["checkpoint_00000001.pth", "checkpoint_00000004.pth", "checkpoint_00000007.pth", "checkpoint_latest.pth"]
    sched = warmup_schedule(0.01, 4)
    assert [c[4] for c in eng.calls[::len(tr.ts.pbuf.buckets)]] == [sched(i + 1) for i in range(7)]
    ck = torch.load(tmp_path / "a" / "checkpoint_latest.pth", weights_only=False)
    assert set(ck) == {"model", "diffusion", "opt", "scheduler", "iters", "config_dict", "ema", "rng"}        # (no autoencoder / text encoder given)
    assert set(ck) - {"rng", "ema"} <= set(T.CKPT_KEYS) and ck["iters"] == 7
    sd = tiny_state_dict()
    assert list(ck["model"]) == list(sd) == list(ck["ema"]) and all(v.dtype == torch.float32 and v.device.type == "cpu" for v in ck["model"].values())
    assert ck["opt"]["param_groups"][0]["params"] == [0, 1, 2] and float(ck["opt"]["state"][0]["step"]) == 7
    assert ck["opt"]["param_groups"][0]["lr"] == sched(8) and ck["opt"]["param_groups"][0]["initial_lr"] == 0.01
    assert tuple(ck["opt"]["state"][1]["exp_avg"].shape) == tuple(sd[FUSER_W].shape)
    assert ck["config_dict"]["total_iters"] == 7 and set(ck["diffusion"]) >= {"betas", "sqrt_alphas_cumprod"}
    # the scheduler entry is what a real LambdaLR holds after 7 scheduler.step() calls, and a real one accepts it
    for stype, total in (("constant", None), ("cosine", 7)):
        factor = warmup_schedule(1.0, 4, total)
        opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=0.01)
        real = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: factor(k + 1))
        for _ in range(5):
            opt.step(); real.step()
        want, got = real.state_dict(), T.scheduler_state_dict(0.01, 4, total, 5)
        assert set(got) == set(want)
        for key in want:
            if key != "lr_lambdas":
                assert got[key] == pytest.approx(want[key]) if key == "_last_lr" else got[key] == want[key], (stype, key, got[key], want[key])
        real.load_state_dict(got)
    assert ck["scheduler"]["last_epoch"] == 7 and ck["scheduler"]["_last_lr"] == [sched(8)]
    # ---- resume: 4 iterations, a new Trainer from the file (auto-resume from output_dir), 3 more: the uninterrupted run's state
    e1 = FakeEngine()
    t1 = T.Trainer(e1, tiny_config(tmp_path / "b", total_iters=4), tiny_state_dict(), tiny_batches, seed=5, log=lambda s: None)
    t1.start_training()
    e2 = FakeEngine()
    e2.n_steps = 4                               # (the stand-in's gradients are a function of its call count)
    t2 = T.Trainer(e2, tiny_config(tmp_path / "b"), tiny_state_dict(), tiny_batches, seed=77, log=lambda s: None)
    assert t2.starting_iter == 4 and t2.ts.steps == 4
    assert t2.start_training() == 7
    assert e2.calls[0][3] == 5 and e2.calls[0][4] == sched(5)           # the first update after the resume: step iters + 1 at its rate
    a, b = tr.state(), t2.state()
    for key in ("model", "ema"):
        assert all(torch.equal(a[key][k], b[key][k]) for k in a[key]), key
    for i in a["opt"]["state"]:
        assert all(torch.equal(torch.as_tensor(a["opt"]["state"][i][k]), torch.as_tensor(b["opt"]["state"][i][k])) for k in a["opt"]["state"][i])
    assert torch.equal(a["rng"]["device"], b["rng"]["device"]) and a["rng"]["python"] == b["rng"]["python"]
    assert torch.equal(e2.last_t, eng.last_t)
    # iters >= total_iters returns at once
    e3 = FakeEngine()
    t3 = T.Trainer(e3, tiny_config(tmp_path / "b"), tiny_state_dict(), tiny_batches, log=lambda s: None)
    assert t3.starting_iter == 7 and t3.start_training() == 7 and e3.calls == []
    # resume=False starts over; a scheduler_type the reference does not have is refused
    assert T.Trainer(FakeEngine(), tiny_config(tmp_path / "b"), tiny_state_dict(), tiny_batches, resume=False, log=lambda s: None).starting_iter == 0
    with pytest.raises(ValueError):
        T.Trainer(FakeEngine(), tiny_config(tmp_path / "c", scheduler_type="linear"), tiny_state_dict(), tiny_batches)


def test_trainer_extends_the_first_conv_and_reads_the_reference_config_shape(tmp_path):
    """inpaint_mode zero-extends a 4-channel first conv by five channels and trains its weight (trainer.py:189-194, 233), `ckpt` loads a
    first-stage model over the starting weights (trainer.py:211-213), and config["model"] may be the reference's {target, params}."""
    from gligen_amd import trainer as T
    first = dict(tiny_state_dict())
    first["out.2.weight"] = torch.full((4, 4), 7.0)
    torch.save(dict(model=first), tmp_path / "first.pth")
    cfg = tiny_config(tmp_path / "o", inpaint_mode=True, enable_ema=False, ckpt=str(tmp_path / "first.pth"),
                      model=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(TINY_CFG)))
    tr = T.Trainer(FakeEngine(), cfg, tiny_state_dict(), tiny_batches, resume=False, log=lambda s: None)
    w = tr.ts.params["input_blocks.0.0.weight"]
    assert tuple(w.shape) == (8, 9, 3, 3) and torch.count_nonzero(w[:, 4:]) == 0 and torch.equal(w[:, :4], tiny_state_dict()["input_blocks.0.0.weight"])
    assert tr.ts.param_order[0] == "input_blocks.0.0.weight" and len(tr.ts.param_order) == 4 and tr.cfg["inpaint_mode"] is True
    assert bool((tr.ts.params["out.2.weight"] == 7.0).all())
    assert "ema" not in tr.state()


def test_timestep_draw():
    """trainer.py:335-337: (rand * 1000).long() with a 1000 replaced by 999; every draw lies in [0, 999]."""
    from gligen_amd.trainer import draw_timesteps
    g = torch.Generator().manual_seed(0)
    forced = draw_timesteps(4, g, "cpu", _t=torch.tensor([1.0, 0.0, 0.9995, 0.4567]))
    assert forced.dtype == torch.int64 and forced.tolist() == [999, 0, 999, 456]
    t = draw_timesteps(200000, g, "cpu")
    assert int(t.min()) >= 0 and int(t.max()) <= 999 and len(torch.unique(t)) == 1000
    g2 = torch.Generator().manual_seed(0)
    assert torch.equal(draw_timesteps(16, g2, "cpu"), draw_timesteps(16, torch.Generator().manual_seed(0), "cpu"))


def test_count_spatial_transformers_and_the_guard():
    """Engine.count_spatial_transformers walks the config as gl_unet_train_step numbers the blocks: 16 for the shipped topology, 7
    for the small golden config; TrainStep now refuses a state_dict whose fuser blocks do not match the config's."""
    from gligen_amd.engine import Engine
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    assert Engine.count_spatial_transformers(syn.UNET_CFG) == 16
    small = fixture()["small_text"]["cfg"]
    assert Engine.count_spatial_transformers(small) == 7
    assert Engine.count_spatial_transformers(dict(small, attention_resolutions=[2])) == 4          # input 1, middle 1, output 2
    assert Engine.count_spatial_transformers(dict(small, channel_mult=[1, 2, 4], num_res_blocks=2, attention_resolutions=[4, 1])) == 2 + 2 + 1 + 3 + 3
    for cfg in (small, dict(small, channel_mult=[1, 2, 4], num_res_blocks=2, attention_resolutions=[4, 1])):
        keys = UNetModel(**cfg).state_dict().keys()
        assert len({k.split(".transformer_blocks.")[0] for k in keys if ".fuser." in k}) == Engine.count_spatial_transformers(cfg)

    class Counting(FakeEngine):
        count_spatial_transformers = staticmethod(Engine.count_spatial_transformers)

    shapes = {k: torch.zeros(()) for k in UNetModel(**small).state_dict()}
    assert max(TrainStep(Counting(), small, shapes, world=1).milestone.values()) == 7
    cut = {k: v for k, v in shapes.items() if not k.startswith("middle_block.1.transformer_blocks.0.fuser.")}
    with pytest.raises(ValueError, match="6 fuser blocks in the state_dict, 7 SpatialTransformers"):
        TrainStep(Counting(), small, cut, world=1)
