"""Samplers side by side on the flagship shapes: synthetic text grounding, batch 4, 512 x 512 (latent 64 x 64), guidance 7.5.

    python tools/sampler_bench.py [--batch 4] [--repeat 3] [--height H] [--width W] [--samplers plms,ddim] [--out FILE]

Prints, per sampler, the UNet evaluations of one image batch, the time of a batch (sampling + decode, best and mean of --repeat after a
warm-up pass that tunes and captures) and images/s: 50-step PLMS, 20-step DPM-Solver++ (2M) on the uniform and on the log-SNR grid, and
250-step DDIM. Then the mean device time of solver_update_kernel against plms_update_kernel at the same n, from torch's profiler over
one run of each. The claim is the evaluation count; image quality on pretrained weights is not something this tool can see.
--height / --width (pixels, multiples of 64): the same at another image size; the report then ends with the arena high-water marks of the
UNet's and the autoencoder's contexts. --samplers: a comma-separated subset of the case names (the update-kernel comparison needs none).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("plms", dict(steps=50)), ("dpmpp_2m uniform", dict(sampler="dpmpp_2m", discretize="uniform", steps=20)),
         ("dpmpp_2m logsnr", dict(sampler="dpmpp_2m", discretize="logsnr", steps=20)), ("ddim", dict(sampler="ddim", steps=250))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--height", type=int, default=None, help="image height in pixels (default 512)")
    ap.add_argument("--width", type=int, default=None, help="image width in pixels (default 512)")
    ap.add_argument("--samplers", type=str, default=None, help="comma-separated case names (default: all): " + ", ".join(n for n, _ in CASES))
    ap.add_argument("--no_update_kernels", action="store_true", help="skip the profiler pass over the two update kernels")
    ap.add_argument("--out", type=str, default=None, help="also write the report to this file")
    args = ap.parse_args()
    cases = CASES if not args.samplers else [c for c in CASES if c[0] in [n.strip() for n in args.samplers.split(",")]]
    if not cases:
        ap.error("--samplers names none of: " + ", ".join(n for n, _ in CASES))
    import gligen_inference as gi
    from gligen_amd import synthetic as syn
    from gligen_amd.build import build_native
    build_native()
    dev = torch.device("cuda:0")
    gi.device = dev
    B = args.batch
    model, ae, diffusion, mcfg = gi.load_synthetic("text", seed=1234, fast=True)
    model.grounding_tokenizer_input = gi.instantiate_from_config(mcfg["grounding_tokenizer_input"])
    batch = {k: v.to(dev) for k, v in syn.make_batch("text", B, n_valid=8, seed=0).items()}
    context, uc = syn.make_context(B, seed=0).to(dev), syn.make_context(B, seed=1).to(dev)
    lat_h, lat_w = gi.latent_hw(model, ae, args.height, args.width)
    x_T = syn.make_latent(B, 4, lat_h, lat_w, seed=0).to(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    say(f"sampler_bench: synthetic text, batch {B}, {8 * lat_h}x{8 * lat_w} (height x width), guidance 7.5, hipGraph on; commit {commit}")

    def one(kw):
        imgs = gi.generate(model, ae, diffusion, batch, context, uc, guidance_scale=7.5, starting_noise=x_T.clone(), height=args.height, width=args.width, **kw)
        out = ae.engine.to_uint8(imgs)
        torch.cuda.synchronize()
        return out

    results = {}
    for name, kw in cases:
        one(kw)                                   # tile tuning, the eager pass, graph capture
        times = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            out = one(kw)
            times.append(time.perf_counter() - t0)
        avg_ms, first_ms, n_evals = model.engine.sampler_timing()
        finite = bool(torch.isfinite(out.float()).all())
        best, mean = min(times), sum(times) / len(times)
        results[name] = dict(steps=kw["steps"], evaluations=n_evals, best_s=best, mean_s=mean, images_per_s=B / best, unet_eval_ms=avg_ms, finite=finite)
        say(f"{name:18s} steps {kw['steps']:3d}  evaluations {n_evals:3d}  batch {best:.3f} s best / {mean:.3f} s mean  "
            f"{B / best:6.2f} images/s  UNet evaluation {avg_ms:.2f} ms  finite {finite}")
    base = results["plms"]["best_s"] if "plms" in results else None
    for name in results if base else ():
        say(f"  {name:18s} {base / results[name]['best_s']:.2f}x the images/s of 50-step PLMS")

    # the two update kernels at the same n = B * 4 * 64 * 64
    from torch.profiler import ProfilerActivity, profile
    kernels = {}
    try:
        if args.no_update_kernels:
            raise RuntimeError("skipped by --no_update_kernels")
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            one(dict(steps=10))
            one(dict(sampler="dpmpp_2m", steps=10))
        for ev in prof.key_averages():
            for k in ("plms_update_kernel", "solver_update_kernel"):
                if k in ev.key:
                    t = getattr(ev, "device_time_total", None)
                    t = ev.cuda_time_total if t is None else t
                    c, tot = kernels.get(k, (0, 0.0))
                    kernels[k] = (c + ev.count, tot + t)
    except Exception as e:  # the profiler is a measuring aid, not part of the product
        say(f"update kernels: torch profiler unavailable ({type(e).__name__}: {e})")
    for k, (c, tot) in sorted(kernels.items()):
        say(f"{k:22s} n {B * 4 * lat_h * lat_w}  launches {c}  mean {tot / max(c, 1):.2f} us")
    if not kernels:
        say("update kernels: the profiler reported no kernel of either name")
    say("arena high water: " + json.dumps(dict(unet=model.engine.memory()["arena_high_water"], vae=ae.engine.memory()["arena_high_water"])))
    say("box calibration: " + json.dumps(model.engine.box_calibrate()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
