"""Iteration time and arena high-water mark of LoRA training next to the fuser step it is built on, on the shipped topology at B = 4,
64 x 64 latent, checkpoint=True, the frozen-weight operand cache on: whole iterations (forward, loss, backward, AdamW over the buckets)
of
    base            gligen_amd.train.TrainStep: the reference's set (fusers + position_net, ~209 M values)
    lora_r4 / lora_r16 / lora_r128   gligen_amd.lora_train.LoraTrainStep, adapters alone, families attn ff
    lora_r16+base   adapters and the reference's set together
run in alternation in one process (one engine, one arena: the high-water mark is read after each arm's iterations and is the
largest seen so far, so the arms are ordered from the smallest working set to the largest on the first pass), and the time of the
four low-rank kernels at the shapes of the 64 x 64 level (M = 16 384 rows; cross-attention to_k / to_v: M = 308) through
Engine.op_lora_linear: HIP events around calls that launch the down product alone, down + up, the two down products of a backward,
and those + a weight gradient (partials + reduce); a kernel's time is the difference of two medians of 20.
    PYTHONPATH=. python tools/lora_train_bench.py [--reps 3] [--small] [--out profiles/lora_train/bench.jsonl]
--small: the two-level test UNet at B = 2, 16 x 16 (a smoke run of the tool itself)."""
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


def kernel_times(eng, emit):
    dev = eng.device
    g = torch.Generator().manual_seed(3)
    for M, K, N, what in ((16384, 320, 320, "attn1 / proj"), (16384, 320, 2560, "ff.net.0.proj"), (16384, 1280, 320, "ff.net.2"), (308, 768, 320, "attn2 to_k / to_v")):
        for r in (4, 16, 128):
            x, dy = torch.randn(M, K, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
            down, up = (torch.randn(r, K, generator=g) * K ** -0.5).to(dev), (torch.randn(N, r, generator=g) * 0.03).to(dev)
            o = {k: torch.zeros(s, device=dev) for k, s in dict(t=(M, r), y=(M, N), u=(M, r), dx=(M, K), g_down=(r, K), g_up=(N, r)).items()}
            pick = lambda *names: {k: o[k] for k in names}
            call = lambda out, with_dy: eng.op_lora_linear(x, down, up, scale=1.0, dy=dy if with_dy else None, out=out)
            call(o, True)
            t_down = event_ms(lambda: call(pick("t"), False))
            t_fwd = event_ms(lambda: call(pick("t", "y"), False))
            t_2down = event_ms(lambda: call(pick("t", "u"), True))
            t_dx = event_ms(lambda: call(pick("t", "u", "dx"), True))
            t_gdown = event_ms(lambda: call(pick("t", "u", "g_down"), True))
            t_gup = event_ms(lambda: call(pick("t", "u", "g_up"), True))
            us = lambda v: round(v * 1e3, 1)
            emit(dict(config="low-rank kernels", site=what, M=M, K=K, N=N, rank=r, down_x_us=us(t_down), up_y_us=us(t_fwd - t_down), down_dy_us=us(t_2down - t_down),
                      up_dx_us=us(t_dx - t_2down), wgrad_down_us=us(t_gdown - t_2down), wgrad_up_us=us(t_gup - t_2down),
                      wgrad_chunk_rows=eng.lora_wgrad_chunk_rows(M), timing="HIP events, differences of medians of 20; a weight gradient is two launches"))


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
    fam = ("attn", "ff")
    make = {
        "lora_r4": lambda: LoraTrainStep(eng, cfg, sd, LoraSpec(4, families=fam), lr=1e-4, world=1),
        "lora_r16": lambda: LoraTrainStep(eng, cfg, sd, LoraSpec(16, families=fam), lr=1e-4, world=1),
        "lora_r128": lambda: LoraTrainStep(eng, cfg, sd, LoraSpec(128, families=fam), lr=1e-4, world=1),
        "base": lambda: TrainStep(eng, cfg, sd, lr=5e-5, world=1),
        "lora_r16+base": lambda: LoraTrainStep(eng, cfg, sd, LoraSpec(16, families=fam), lr=1e-4, world=1, train_base=True),
    }
    arms = {n: f() for n, f in make.items()}          # (every constructor empties the operand cache; it fills again in the warm-up)
    b = syn.make_batch("text", B, n_valid=3, seed=5)
    batch = {k: v.to(dev) for k, v in dict(x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441, 300, 77][:B]).float(),
                                           context=syn.make_context(B, seed=6), boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"],
                                           target=syn.make_latent(B, 4, hw, hw, seed=7)).items()}
    high = {}
    for n, ts in arms.items():                         # warm-up: GEMM tile selection, the operand cache of this arm's tensors
        for _ in range(2):
            ts.step(batch)
        torch.cuda.synchronize()
        high[n] = eng.arena_high_water()
    times = {n: [] for n in arms}
    for _ in range(a.reps):
        for n, ts in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = ts.step(batch)
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    for n, ts in arms.items():
        emit(dict(config="shipped topology" if not a.small else "small UNet", arm=n, B=B, latent=hw, checkpoint=True, weight_cache=True,
                  s_per_iteration=round(med[n], 4), s_per_iteration_min=round(min(times[n]), 4), over_base=round(med[n] / med["base"], 3),
                  arena_high_water_gb_so_far=round(high[n] / 2 ** 30, 2), trainable_values=sum(int(x.numel()) for x in ts.pbuf.buckets),
                  buckets=len(ts.pbuf.buckets),
                  timing=f"host wall time around one synchronised iteration, median of {a.reps}, the arms in alternation"))
    if not a.no_kernels:
        kernel_times(eng, emit)
    eng.train_weight_cache(False)
    eng.close()
    if a.out:
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
