"""The autoencoder's attention by itself (gl_op_vae_attention): the score-matrix form against vae_attn_flash_kernel.

    python tools/vae_attn_bench.py [--C 512] [--tokens 4096,9216,16384] [--rounds 7] [--arena_gb 4] [--largest_decode GB] [--out FILE]

Per token count, B = 1, seeded bf16 q, k, v: both forms alternate in ONE process, `--rounds` rounds after one untimed round (GEMM tile
tuning); the report has the median and the minimum of each form (HIP events around one call) and the arena high-water mark of a context
that ran only that form. Where the matrix form does not fit the arena the flash form runs alone and the arena's message is printed.
Auto's threshold (4096 tokens) is a bit-compatibility line, not a tuning result: this tool reports, it decides nothing.

--largest_decode GB: also find, by bisection over multiples of 64 pixels, the largest square image the full autoencoder decodes at batch 1
on a context with an arena of that many GB (a size that does not fit fails with the arena's own message, which ends the probe of it).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--C", type=int, default=512)
    ap.add_argument("--tokens", type=str, default="4096,9216,16384")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--arena_gb", type=float, default=4.0)
    ap.add_argument("--largest_decode", type=float, default=None, metavar="GB")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from gligen_amd import GligenAmdError
    from gligen_amd import synthetic as syn
    from gligen_amd.engine import Engine
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    C = args.C
    say(f"vae_attn_bench: C {C}, B 1, arena {args.arena_gb} GB per context; ms per call, median / min of {args.rounds} alternating rounds")
    for T in [int(t) for t in args.tokens.split(",")]:
        g = torch.Generator().manual_seed(T)
        q, k, v = ((torch.randn((1, T, C), generator=g) * s).to(torch.bfloat16).to(dev) for s in (0.25, 0.25, 1.0))
        engines = {m: Engine(dev, arena_gb=args.arena_gb) for m in ("matrix", "flash")}
        times, outs = {m: [] for m in engines}, {}
        try:
            try:
                outs["matrix"] = engines["matrix"].vae_attention(q, k, v, mode="matrix")
            except GligenAmdError as e:
                say(f"T {T:6d}  matrix form: {e}")
                times.pop("matrix")
            outs["flash"] = engines["flash"].vae_attention(q, k, v, mode="flash")
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for m in times:
                    times[m].append(timed(lambda: engines[m].vae_attention(q, k, v, mode=m)))
            rec = dict(T=T, C=C, matrix_bytes=6 * T * T)
            for m in times:
                rec[m] = dict(median_ms=statistics.median(times[m]), min_ms=min(times[m]), arena_high_water=engines[m].memory()["arena_high_water"])
            if "matrix" in outs:
                d = (outs["flash"].double() - outs["matrix"].double()).abs().max()
                rec["max_abs_diff_over_vmax"] = float(d / v.double().abs().max())
                rec["flash_over_matrix"] = rec["flash"]["median_ms"] / rec["matrix"]["median_ms"]
            say(json.dumps(rec))
        finally:
            for e in engines.values():
                e.close()

    if args.largest_decode:
        from gligen_amd.runtime import build_vae_engine
        from ldm.models.autoencoder import AutoencoderKL
        with torch.device("meta"):
            ae = AutoencoderKL(ddconfig=syn.VAE_DDCONFIG, embed_dim=4, scale_factor=0.18215).eval()
        ae = syn.fill_module_on_device_(ae.to_empty(device=dev), 4321)
        eng = build_vae_engine(ae, arena_gb=args.largest_decode)

        def fits(px):
            z = (syn.make_latent(1, 4, px // 8, px // 8, seed=1) * 0.18215 * 4).to(dev)
            ctx = eng.fork(arena_gb=args.largest_decode)        # a fresh arena per size: its high-water mark is this size's
            try:
                img = ctx.vae_decode(z)                          # (tunes the GEMM tiles of the new shapes)
                t = timed(lambda: ctx.vae_decode(z))
                ok = bool(torch.isfinite(img).all())
            except GligenAmdError as e:
                say(f"  {px} x {px}: {e}")
                return False
            finally:
                hw = ctx.memory()["arena_high_water"]
                ctx.close()
            say(f"  {px} x {px}: decoded in {t:.1f} ms, finite {ok}, arena high water {hw} bytes")
            return ok

        lo, hi = 512, 3072          # lo fits (the shipped size); hi is where the search stops, fitting or not
        if fits(hi):
            lo = hi
        while hi - lo > 64 and lo != hi:
            mid = (lo + hi) // 2 // 64 * 64
            if fits(mid):
                lo = mid
            else:
                hi = mid
        say(json.dumps(dict(largest_square_decode_px=lo, arena_gb=args.largest_decode, batch=1, search_cap_px=3072)))
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
