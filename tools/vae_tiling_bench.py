"""What tiling the autoencoder costs and buys: decode time, arena high-water mark, tile and pass counts, untiled against tiled.

    python tools/vae_tiling_bench.py [--sizes 1024 2048 3072 4096] [--batches 1 4] [--arena_gb 12] [--out profiles/vae_tiling/vae_tiling_bench.txt]

Full-size synthetic VAE (random weights) in a 12 GB arena. Per size and batch: the untiled decode (where the arena takes it) and the
tiled one (default tile 64, overlap 16), each on a context of its own so that the arena's high-water mark is that call's, timed with HIP
events, medians of five calls after one warm-up, untiled and tiled alternated in one process. Then the largest square of --reach that
the tiled decode reaches, and the relative MSE of tiled against untiled at 1024 x 1024 for overlaps 8, 16 and 32: the effect of
tile-local GroupNorm statistics and attention on RANDOM weights -- it says nothing about seams on trained weights.
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 3072, 4096])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reach", type=int, nargs="+", default=[6144, 8192], help="squares tried, batch 1, tiled, in this order, to find the largest that decodes")
    ap.add_argument("--arena_gb", type=float, default=12.0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "vae_tiling", "vae_tiling_bench.txt"))
    args = ap.parse_args()
    from ldm.models.autoencoder import AutoencoderKL
    from gligen_amd import GligenAmdError, runtime, synthetic as syn, vae_tiling as vt
    from gligen_amd.build import build_native
    build_native()
    dev = torch.device("cuda:0")
    ae = syn.fill_module_(AutoencoderKL(ddconfig=syn.VAE_DDCONFIG, embed_dim=4, scale_factor=0.18215).eval(), 4321).to(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def attempt(eng, z, **kw):
        """(ms or None, image or None, message): one decode; an exhausted arena is an answer, not an error."""
        try:
            ms, img = timed(lambda: eng.vae_decode(z, **kw))
            return ms, img, ""
        except GligenAmdError as e:
            if "workspace arena exhausted" not in str(e):
                raise
            torch.cuda.synchronize()
            return None, None, "workspace arena exhausted"

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    say(f"vae_tiling_bench: full-size synthetic VAE (random weights), {args.arena_gb:g} GB arena, decode, HIP events, median of {args.calls} calls after one "
        f"warm-up, untiled and tiled alternated; tile {vt.DEFAULT_TILE}, overlap {vt.DEFAULT_OVERLAP} latent pixels; commit {commit}")
    say(f"{'size':>11} {'batch':>5} | {'untiled ms':>10} {'high-water MB':>13} | {'tiled ms':>9} {'high-water MB':>13} {'tiles':>6} {'passes':>6}")
    for size in args.sizes:
        for B in args.batches:
            h = size // 8
            z = (syn.make_latent(B, 4, h, h, seed=21) * 0.18215 * 4).to(dev)
            p = vt.Plan2D(h, h)
            per_pass = max(1, (8 * 64 * 64) // (p.th * p.tw))
            n_tiles = B * p.ny * p.nx
            eu, et = runtime.build_vae_engine(ae, arena_gb=args.arena_gb), runtime.build_vae_engine(ae, arena_gb=args.arena_gb)
            tu, tt, fits = [], [], True
            for i in range(args.calls + 1):
                if fits:
                    ms, _, why = attempt(eu, z)
                    fits = ms is not None
                    if fits and i:
                        tu.append(ms)
                ms, _, why_t = attempt(et, z, tiling="on")
                if ms is None:
                    break
                if i:
                    tt.append(ms)
            mb = lambda e: e.arena_high_water() / 1e6
            left = f"{statistics.median(tu):10.1f} {mb(eu):13.1f}" if tu else f"{'arena exhausted':>24}"
            right = f"{statistics.median(tt):9.1f} {mb(et):13.1f}" if tt else f"{'arena exhausted':>23}"
            say(f"{size:>5} x {size:<5}{B:>4} | {left} | {right} {n_tiles:>6} {-(-n_tiles // per_pass):>6}")
            eu.close()
            et.close()
            del z
            torch.cuda.empty_cache()
    reached = None
    for size in args.reach:
        h = size // 8
        z = (syn.make_latent(1, 4, h, h, seed=21) * 0.18215 * 4).to(dev)
        e = runtime.build_vae_engine(ae, arena_gb=args.arena_gb)
        try:
            ms, img, why = attempt(e, z, tiling="on")
        except (GligenAmdError, torch.cuda.OutOfMemoryError) as err:
            ms, img, why = None, None, str(err).splitlines()[0][:120]
        p = vt.Plan2D(h, h)
        if ms is None:
            say(f"reach: {size} x {size}, batch 1, tiled: {why}")
            e.close()
            break
        say(f"reach: {size} x {size}, batch 1, tiled: {ms:.1f} ms (first call), high-water {e.arena_high_water() / 1e6:.1f} MB, {p.ny * p.nx} tiles, finite {bool(torch.isfinite(img).all())}")
        reached = size
        e.close()
        del z, img
        torch.cuda.empty_cache()
    say(f"largest square the tiled decode reached, of {args.reach} after {max(args.sizes)}: {reached if reached else max(args.sizes)}")
    h = 128
    z = (syn.make_latent(1, 4, h, h, seed=21) * 0.18215 * 4).to(dev)
    e = runtime.build_vae_engine(ae, arena_gb=args.arena_gb)
    untiled = e.vae_decode(z).clone()
    for ov in (8, 16, 32):
        tiled = e.vae_decode(z, tiling="on", overlap=ov)
        rel = float(((tiled - untiled) ** 2).mean() / untiled.var())
        say(f"tiled against untiled at 1024 x 1024, batch 1, overlap {ov:>2}: relative MSE {rel:.3e}, max |difference| {float((tiled - untiled).abs().max()):.3f} "
            f"(image range {float(untiled.min()):.2f} .. {float(untiled.max()):.2f}; random weights: tile-local GroupNorm statistics and attention, not seams)")
    e.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
