"""What a LoRA adapter costs at load time: the merge, the engine rebuild that follows, and the first generate() after it.

    python tools/lora_bench.py [--ranks 16 128] [--batch 4] [--steps 20] [--out profiles/lora/lora_bench.txt]

Full-size synthetic text model, one synthetic adapter per rank over every attention and feed-forward matrix of the UNet (fp16 on the
host, as adapters are distributed). Per rank: apply_loras() from parsed host tensors (upload of the factors, one gl_op_lora_merge
launch per matrix, the host stash of the originals on first touch) -- first call and a second call, which finds the stash --, the
merge launches alone (device time, the factors already on the device), the engine rebuild (model.engine after _drop_engine), the first
generate() (tile tuning, the eager pass, graph capture) and a second one, and remove_loras().
Image quality with a real adapter is not something this tool can see: the weights are random.
"""
import argparse
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "lora", "lora_bench.txt"))
    args = ap.parse_args()
    import gligen_inference as gi
    from gligen_amd import lora, runtime, synthetic as syn
    from gligen_amd.build import build_native
    build_native()
    dev = torch.device("cuda:0")
    gi.device = dev
    B = args.batch
    model, ae, diffusion, mcfg = gi.load_synthetic("text", seed=1234, fast=True)
    model.grounding_tokenizer_input = gi.instantiate_from_config(mcfg["grounding_tokenizer_input"])
    batch = {k: v.to(dev) for k, v in syn.make_batch("text", B, n_valid=8, seed=0).items()}
    context, uc = syn.make_context(B, seed=0).to(dev), syn.make_context(B, seed=1).to(dev)
    x_T = syn.make_latent(B, 4, 64, 64, seed=0).to(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def gen():
        return gi.generate(model, ae, diffusion, batch, context, uc, starting_noise=x_T.clone(), guidance_scale=7.5, sampler="dpmpp_2m", steps=args.steps)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    say(f"lora_bench: synthetic text (full size), adapters over every attention and feed-forward matrix of the UNet, fp16 on the host; "
        f"generate(): batch {B}, dpmpp_2m {args.steps} steps, 512 x 512, sampling + decode; commit {commit}")
    t_build, _ = clock(lambda: (model.engine, ae.engine))
    t_first, base = clock(gen)
    t_second, _ = clock(gen)
    say(f"no adapter: engine build {t_build:.3f} s, first generate() {t_first:.3f} s, second {t_second:.3f} s")
    scratch = runtime.scratch_engine(dev)
    for rank in args.ranks:
        adapter = syn.synthetic_lora(model, rank=rank, families=("attn", "ff"), dtype=torch.float16, seed=7)
        n_mod = sum(1 for k in adapter if k.endswith(".lora_down.weight"))
        flop = 0
        params = dict(model.named_parameters())
        table = lora.unet_name_table(model)
        pairs = []
        for e in lora.parse_adapter(adapter):
            w = params[table[e.name] + ".weight"]
            flop += 2 * w.numel() * e.rank
            pairs.append((w, e.up.to(dev, torch.float32).reshape(w.shape[0], e.rank).contiguous(), e.down.to(dev, torch.float32).reshape(e.rank, -1).contiguous()))
        t_apply, report = clock(lambda: lora.apply_loras(model, None, [(adapter, 1.0)]))
        t_apply2, _ = clock(lambda: lora.apply_loras(model, None, [(adapter, 1.0)]))
        t_rebuild, _ = clock(lambda: model.engine)
        t_gen1, out = clock(gen)
        t_gen2, _ = clock(gen)
        moved = float((out - base).abs().mean())
        t_remove, _ = clock(lambda: lora.remove_loras(model, None))
        # the launches alone, on scratch copies of the weights (the factors are on the device already)
        copies = [(w.detach().clone(), u, d) for w, u, d in pairs]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for w, u, d in copies:
            scratch.op_lora_merge(w, u, d, 0.5)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        del copies, pairs
        say(f"rank {rank:3d}: {n_mod} matrices, {flop / 1e9:.1f} GFLOP, {sum(t.numel() * t.element_size() for t in adapter.values()) / 2 ** 20:.1f} MiB | "
            f"apply_loras {t_apply:.3f} s (again, stash in place: {t_apply2:.3f} s) | merge launches alone {ms:.1f} ms = {flop / ms / 1e9:.2f} TFLOP/s fp32 | "
            f"engine rebuild {t_rebuild:.3f} s | first generate() {t_gen1:.3f} s, second {t_gen2:.3f} s | remove_loras {t_remove:.3f} s | "
            f"mean |image - unadapted image| {moved:.4f}, skipped {len(report['skipped'])}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
