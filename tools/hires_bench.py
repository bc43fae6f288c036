"""Two-pass ("hires") generation against a direct large sample: synthetic text grounding, batch 4, DPM-Solver++ (2M) 20 steps, guidance 7.5.

    python tools/hires_bench.py [--batch 4] [--repeat 5] [--strength 0.5] [--out profiles/hires/hires_bench.txt]

Arms, alternated in one process: 1024 x 1024 sampled directly; 512 x 512 -> 1024 x 1024 with the latent enlarged (latent-bicubic) and
with the decoded image enlarged (pixel-bicubic), second pass at the given strength. Per arm: UNet evaluations per size, the batch time of
calls 2 and 3 one by one (call 1 tunes and captures; a later call that is slower than its neighbours would be a recapture or an
allocation) and the median of calls 2 .. --repeat + 1, with the device bytes each context holds after call 2 and after the last call.
Then one latent_renoise launch at 64 x 64 -> 128 x 128, batch 4 (device time, mean of 200). The direct arm runs on the second pass's
forked context, which is the one that has the 128 x 128 latent's graphs: the model's own context never leaves 64 x 64.
The claim is evaluations and seconds; what the second pass does for the composition of SD-1.4 weights is not something this tool can see.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=5, help="timed calls per arm after the warm-up call")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--strength", type=float, default=0.5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "hires", "hires_bench.txt"))
    args = ap.parse_args()
    import gligen_inference as gi
    from gligen_amd import synthetic as syn
    from gligen_amd.build import build_native
    build_native()
    dev = torch.device("cuda:0")
    gi.device = dev
    B, S = args.batch, args.steps
    model, ae, diffusion, mcfg = gi.load_synthetic("text", seed=1234, fast=True)
    model.grounding_tokenizer_input = gi.instantiate_from_config(mcfg["grounding_tokenizer_input"])
    batch = {k: v.to(dev) for k, v in syn.make_batch("text", B, n_valid=8, seed=0).items()}
    context, uc = syn.make_context(B, seed=0).to(dev), syn.make_context(B, seed=1).to(dev)
    lo, hi = 512, 1024
    x_lo, x_hi = syn.make_latent(B, 4, lo // 8, lo // 8, seed=0).to(dev), syn.make_latent(B, 4, hi // 8, hi // 8, seed=0).to(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    say(f"hires_bench: synthetic text, batch {B}, dpmpp_2m {S} steps (uniform grid), guidance 7.5, second pass strength {args.strength}, hipGraph on; commit {commit}")
    common = dict(guidance_scale=7.5, sampler="dpmpp_2m", steps=S)
    fork = lambda: gi._hires_context(model, (B, hi // 8, hi // 8))

    def direct():
        m2 = fork()
        out = gi.generate(m2, ae, diffusion, batch, context, uc, starting_noise=x_hi.clone(), height=hi, width=hi, **common)
        return out, {f"{hi}": m2.engine.sampler_timing()[2]}

    def hires(upscaler):
        def run():
            out = gi.generate(model, ae, diffusion, batch, context, uc, starting_noise=x_lo.clone(), height=lo, width=lo, hires=(hi, hi),
                              hires_strength=args.strength, hires_upscaler=upscaler, **common)
            return out, {f"{lo}": model.engine.sampler_timing()[2], f"{hi}": fork().engine.sampler_timing()[2]}
        return run

    arms = [(f"direct {hi}x{hi}", direct), (f"{lo} -> {hi} latent-bicubic", hires("latent-bicubic")), (f"{lo} -> {hi} pixel-bicubic", hires("pixel-bicubic"))]
    memory = lambda: dict(model=model.engine.memory()["own_bytes"], fork=fork().engine.memory()["own_bytes"], vae=ae.engine.memory()["own_bytes"])

    def timed(fn):
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, evals = fn()
        u8 = ae.engine.to_uint8(out)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, evals, tuple(out.shape), bool(torch.isfinite(u8.float()).all())

    times = {name: [] for name, _ in arms}
    info = {}
    mem = {}
    for call in range(1 + args.repeat):          # call 0: tile tuning, the eager pass, graph capture -- every arm, then the timed rounds
        for name, fn in arms:
            dt, evals, shape, finite = timed(fn)
            times[name].append(dt)
            info[name] = (evals, shape, finite)
        if call in (1, args.repeat):
            mem[call] = memory()
    for name, _ in arms:
        t = times[name]
        evals, shape, finite = info[name]
        say(f"{name:28s} evaluations {evals}  image {shape[2]}x{shape[3]}  call 1 {t[0]:.3f} s  call 2 {t[1]:.3f} s  call 3 {t[2]:.3f} s  "
            f"median of calls 2..{len(t)} {statistics.median(t[1:]):.3f} s = {B / statistics.median(t[1:]):.2f} images/s  finite {finite}")
    say(f"device bytes held outside the arenas after call 2: {mem[1]}")
    say(f"device bytes held outside the arenas after call {1 + args.repeat}: {mem[args.repeat]}  ({'unchanged' if mem[1] == mem[args.repeat] else 'CHANGED'})")
    base = statistics.median(times[arms[0][0]][1:])
    for name, _ in arms[1:]:
        say(f"  {name}: {statistics.median(times[name][1:]) / base:.2f} of the direct arm's time")

    # one latent_renoise launch, 64 x 64 -> 128 x 128
    eng = model.engine
    src, noise = syn.make_latent(B, 4, 64, 64, seed=3).to(dev), syn.make_latent(B, 4, 128, 128, seed=4).to(dev)
    out = torch.empty_like(noise)
    for mode in ("nearest-exact", "bilinear", "bicubic"):
        for _ in range(10):
            eng.latent_renoise(src, (128, 128), mode, 0.8, 0.6, noise, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            eng.latent_renoise(src, (128, 128), mode, 0.8, 0.6, noise, out=out)
        e1.record()
        torch.cuda.synchronize()
        say(f"latent_renoise {mode:13s} [{B},4,64,64] -> [{B},4,128,128] with noise: {e0.elapsed_time(e1) / 200 * 1000:.1f} us per launch (200 back to back, launch overhead included)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
