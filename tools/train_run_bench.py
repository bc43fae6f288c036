"""What gradient accumulation and norm clipping cost a training iteration, on the shipped topology at B = 4, 64 x 64 latent,
checkpoint=True, the frozen-weight operand cache on: whole optimizer steps (K micro-batches of forward, loss, backward, then the
update) of
    defaults          gligen_amd.train.TrainStep as before this tool existed
    clip              max_grad_norm = 1
    K4                accumulate = 4
    K4+clip           both
    lora_r16+clip     gligen_amd.lora_train.LoraTrainStep, rank 16, families attn ff, max_grad_norm = 1
run in alternation in one process, medians after a warm-up, reported per optimizer step and per micro-batch; and the kernels of
csrc/train_run.hip alone on one 32.7 M-element bucket (the largest of the shipped model) as GB/s of the bytes each has to move: HIP
events around one launch, median of 20.
    PYTHONPATH=. python tools/train_run_bench.py [--reps 3] [--small] [--out profiles/train_run/bench.jsonl]
--small: the two-level test UNet at B = 2, 16 x 16 and a 1 M-element range (a smoke run of the tool itself)."""
import argparse
import json
import time

import torch

from gligen_amd import synthetic as syn
from gligen_amd.engine import Engine
from gligen_amd.lora_train import LoraSpec, LoraTrainStep
from gligen_amd.train import TrainStep
from gligen_amd.trainer import synthetic_state_dict


def event_ms(fn, reps=20):
    out = []
    for _ in range(reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); z.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(z))
    return sorted(out)[reps // 2]


def kernel_rates(eng, n, emit):
    dev = eng.device
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda: torch.randn(n, generator=gen, device=dev)
    p, g, m, v, ema, acc = rnd(), rnd(), rnd() * 0.1, rnd().abs() * 0.01, rnd(), rnd()
    partials = torch.empty(eng.grad_sqnorm_partials(n), device=dev)
    out2 = eng.op_clip_coef(eng.op_grad_sqnorm(g, partials), 1.0)
    hyper = dict(lr=1e-5, weight_decay=0.01)
    kernels = {           # name -> (call, bytes per element)
        "grad_accum_kernel first": (lambda: eng.op_grad_accumulate(acc, g, "first", 4), 8),
        "grad_accum_kernel middle": (lambda: eng.op_grad_accumulate(acc, g, "middle", 4), 12),
        "grad_accum_kernel last": (lambda: eng.op_grad_accumulate(acc, g, "last", 4), 12),
        "grad_sqnorm_kernel": (lambda: eng.op_grad_sqnorm(g, partials), 4),
        "adamw_clip_kernel": (lambda: eng.op_adamw_clip_step(p, g, m, v, 3, coef=out2[1:2], **hyper), 28),
        "adamw_clip_kernel + EMA": (lambda: eng.op_adamw_ema_clip_step(p, g, m, v, ema, 3, ema_rate=0.9999, coef=out2[1:2], **hyper), 36),
        "adamw_ema_kernel (unclipped, for comparison)": (lambda: eng.op_adamw_ema_step(p, g, m, v, ema, 3, ema_rate=0.9999, **hyper), 36),
    }
    for name, (call, bpe) in kernels.items():
        call()
        ms = event_ms(call)
        emit(dict(config="kernels alone", kernel=name, elements=n, us=round(ms * 1e3, 1), bytes_per_element=bpe, gb_per_s=round(n * bpe / ms / 1e6, 1),
                  timing="HIP events around one launch, median of 20"))
    call = lambda: eng.op_clip_coef(partials, 1.0, out2)
    call()
    emit(dict(config="kernels alone", kernel="clip_coef_kernel", partials=int(partials.numel()), us=round(event_ms(call) * 1e3, 1),
              timing="HIP events around one launch, median of 20"))
    big = torch.empty(eng.grad_sqnorm_partials(209_000_000), device=dev).fill_(1.0)
    call = lambda: eng.op_clip_coef(big, 1.0, out2)
    call()
    emit(dict(config="kernels alone", kernel="clip_coef_kernel", partials=int(big.numel()), note="the partials of the whole 209 M-element set",
              us=round(event_ms(call) * 1e3, 1), timing="HIP events around one launch, median of 20"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    cfg = dict(syn.UNET_CFG_SMALL if a.small else syn.UNET_CFG, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=False)
    B, hw = (2, 16) if a.small else (4, 64)
    eng = Engine(0, arena_gb=4.0 if a.small else 24.0)
    dev = eng.device
    sd = synthetic_state_dict(cfg)
    make = {
        "defaults": lambda: TrainStep(eng, cfg, sd, lr=5e-5, world=1),
        "clip": lambda: TrainStep(eng, cfg, sd, lr=5e-5, world=1, max_grad_norm=1.0),
        "K4": lambda: TrainStep(eng, cfg, sd, lr=5e-5, world=1, accumulate=4),
        "K4+clip": lambda: TrainStep(eng, cfg, sd, lr=5e-5, world=1, accumulate=4, max_grad_norm=1.0),
        "lora_r16+clip": lambda: LoraTrainStep(eng, cfg, sd, LoraSpec(16, families=("attn", "ff")), lr=1e-4, world=1, max_grad_norm=1.0),
    }
    arms = {n: f() for n, f in make.items()}          # (every constructor empties the operand cache; it fills again in the warm-up)
    b = syn.make_batch("text", B, n_valid=3, seed=5)
    batch = {k: v.to(dev) for k, v in dict(x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441, 300, 77][:B]).float(),
                                           context=syn.make_context(B, seed=6), boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"],
                                           target=syn.make_latent(B, 4, hw, hw, seed=7)).items()}

    def group(ts):
        for _ in range(ts.accumulate):
            ts.step(batch)
        assert ts.at_boundary

    for ts in arms.values():                           # warm-up: GEMM tile selection, the operand cache, one whole group per arm
        group(ts)
        group(ts)
        torch.cuda.synchronize()
    times = {n: [] for n in arms}
    for _ in range(a.reps):
        for n, ts in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            group(ts)
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    for n, ts in arms.items():
        emit(dict(config="shipped topology" if not a.small else "small UNet", arm=n, B=B, latent=hw, accumulate=ts.accumulate, max_grad_norm=ts.max_grad_norm,
                  s_per_optimizer_step=round(med[n], 4), s_per_micro_batch=round(med[n] / ts.accumulate, 4), readings_s=[round(t, 4) for t in times[n]],
                  per_micro_batch_over_defaults=round(med[n] / ts.accumulate / med["defaults"], 4),
                  grad_norm=None if ts.grad_norm is None else float(ts.grad_norm), trainable_values=sum(int(x.numel()) for x in ts.pbuf.buckets),
                  buckets=len(ts.pbuf.buckets), timing=f"host wall time around one synchronised optimizer step, median of {a.reps}, the arms in alternation"))
    if not a.no_kernels:
        kernel_rates(eng, 1 << 20 if a.small else max(int(x.numel()) for x in arms["defaults"].pbuf.buckets), emit)
    eng.train_weight_cache(False)
    eng.close()
    if a.out:
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
