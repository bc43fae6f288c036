"""Iteration time and arena high-water mark of LoRA training with adapters on the convolutions (LoraSpec's conv_families: ResBlock
convs and skip_connection, emb_layers.1, Downsample / Upsample convs) next to the fuser step and the Linear adapters, on the shipped
topology at B = 4, 64 x 64 latent, checkpoint=True, the frozen-weight operand cache on: whole iterations of
    base                 gligen_amd.train.TrainStep: the reference's set
    lora_attn_ff_r16     LoraTrainStep, adapters alone, families attn ff, rank 16 (the arm of tools/lora_train_bench.py)
    conv_r4 / conv_r16 / conv_r64   adapters alone on conv + emb + sample, conv rank 4 / 16 / 64 (rank 16 on the Linears among them)
    all_r16              attn + ff + conv + emb + sample, rank 16 everywhere
run in alternation in one process as tools/lora_train_bench.py does, and the time of the three kernels of csrc/train_lora_conv.hip at
the 64 x 64 / Ci = 320 level and the 16 x 16 / Ci = 1280 level (B = 4) through Engine.op_lora_conv3 -- HIP events around calls that
launch the down product alone, down + u, and those + the data gradient / the weight gradient; a kernel's time is the difference of two
medians of 20 -- against the bytes each has to move at least once (x or dx read / written once, t or u once).
    PYTHONPATH=. python tools/lora_conv_bench.py [--reps 3] [--small] [--out profiles/lora_conv/lora_conv_bench.jsonl]"""
import argparse
import json
import time

import torch

from gligen_amd import synthetic as syn
from gligen_amd.engine import Engine
from gligen_amd.lora_train import LoraSpec, LoraTrainStep
from gligen_amd.train import TrainStep
from gligen_amd.trainer import synthetic_state_dict
from lora_train_bench import event_ms

CONV = ("conv", "emb", "sample")


def kernel_times(eng, emit, small):
    dev = eng.device
    g = torch.Generator().manual_seed(3)
    levels = ((2, 16, 64, "small"),) if small else ((4, 64, 320, "64 x 64 level"), (4, 16, 1280, "16 x 16 level"))
    for B, hw, C, what in levels:
        for geom in (0, 1, 2):
            for r in (4, 16, 64):
                Ho = hw // 2 if geom == 1 else 2 * hw if geom == 2 else hw
                x, dy = torch.randn(B, hw, hw, C, generator=g).to(dev), torch.randn(B, Ho, Ho, C, generator=g).to(dev)
                down, up = (torch.randn(r, C, 3, 3, generator=g) * (9 * C) ** -0.5).to(dev), (torch.randn(C, r, generator=g) * 0.03).to(dev)
                shapes = dict(t=(B, Ho, Ho, r), y=dy.shape, u=(B, Ho, Ho, r), dx=x.shape, g_down=down.shape, g_up=up.shape)
                o = {k: torch.zeros(tuple(s), device=dev) for k, s in shapes.items()}
                pick = lambda *names: {k: o[k] for k in names}
                call = lambda out, with_dy: eng.op_lora_conv3(x, down, up, scale=1.0, geom=geom, dy=dy if with_dy else None, out=out)
                call(o, True)
                t_down = event_ms(lambda: call(pick("t"), False))
                t_2 = event_ms(lambda: call(pick("t", "u"), True))
                t_dx = event_ms(lambda: call(pick("t", "u", "dx"), True))
                t_gd = event_ms(lambda: call(pick("t", "u", "g_down"), True))
                Mi, Mo = B * hw * hw, B * Ho * Ho
                us = lambda v: round(v * 1e3, 1)
                gbs = lambda nbytes, ms: round(nbytes / max(ms, 1e-6) / 1e6, 1)
                b_down, b_dx, b_w = 4 * (Mi * C + Mo * r), 4 * (2 * Mi * C + Mo * r), 4 * (Mi * C + Mo * r + 9 * r * C)
                emit(dict(config="conv low-rank kernels", level=what, geom=geom, B=B, H=hw, C=C, rank=r, conv_down_us=us(t_down), conv_dgrad_us=us(t_dx - t_2),
                          conv_wgrad_us=us(t_gd - t_2), conv_down_min_MB=round(b_down / 1e6, 2), conv_dgrad_min_MB=round(b_dx / 1e6, 2),
                          conv_wgrad_min_MB=round(b_w / 1e6, 2), conv_down_GBps=gbs(b_down, t_down), conv_dgrad_GBps=gbs(b_dx, t_dx - t_2),
                          conv_wgrad_GBps=gbs(b_w, t_gd - t_2), timing="HIP events, differences of medians of 20; the weight gradient is two or eighteen launches"))


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
    conv = lambda r: LoraTrainStep(eng, cfg, sd, LoraSpec(16, families=(), conv_families=CONV, conv_rank=r), lr=1e-4, world=1)
    make = {
        "lora_attn_ff_r16": lambda: LoraTrainStep(eng, cfg, sd, LoraSpec(16, families=("attn", "ff")), lr=1e-4, world=1),
        "conv_r4": lambda: conv(4),
        "conv_r16": lambda: conv(16),
        "conv_r64": lambda: conv(64),
        "all_r16": lambda: LoraTrainStep(eng, cfg, sd, LoraSpec(16, families=("attn", "ff"), conv_families=CONV), lr=1e-4, world=1),
        "base": lambda: TrainStep(eng, cfg, sd, lr=5e-5, world=1),
    }
    arms = {n: f() for n, f in make.items()}
    b = syn.make_batch("text", B, n_valid=3, seed=5)
    batch = {k: v.to(dev) for k, v in dict(x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441, 300, 77][:B]).float(),
                                           context=syn.make_context(B, seed=6), boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"],
                                           target=syn.make_latent(B, 4, hw, hw, seed=7)).items()}
    high = {}
    for n, ts in arms.items():
        for _ in range(2):
            ts.step(batch)
        torch.cuda.synchronize()
        high[n] = eng.arena_high_water()
    times = {n: [] for n in arms}
    for _ in range(a.reps):
        for n, ts in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ts.step(batch)
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    for n, ts in arms.items():
        emit(dict(config="shipped topology" if not a.small else "small UNet", arm=n, B=B, latent=hw, checkpoint=True, weight_cache=True,
                  s_per_iteration=round(med[n], 4), s_per_iteration_min=round(min(times[n]), 4), over_base=round(med[n] / med["base"], 3),
                  arena_high_water_gb_so_far=round(high[n] / 2 ** 30, 2), trainable_values=sum(int(x.numel()) for x in ts.pbuf.buckets),
                  adapters=len(getattr(ts, "adapters", [])),
                  timing=f"host wall time around one synchronised iteration, median of {a.reps}, the arms in alternation"))
    if not a.no_kernels:
        kernel_times(eng, emit, a.small)
    eng.train_weight_cache(False)
    eng.close()
    if a.out:
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
