"""Time one prompt's semantic-map conditioning for B = 4 at 512 x 512 with the reference's default sizes (tokenizer resize_input 448,
downsampler 256): the one-hot planes against the class map, alternating in one process on the same device, wall clock around a
device synchronisation (both arms contain host work), medians.

planes arm: the host's one-hot scatter into 152 fp32 planes repeated over the batch (prepare_batch_sem's work behind the file), the
upload, tokens (gl_op_spatial_tokens) and downsample (gl_op_grounding_downsample).
class arm: the upload of the u8 map, crop + nearest resize on the device (gl_op_class_map_resize), tokens
(gl_op_spatial_tokens_classes) and downsample (gl_op_grounding_downsample_classes).
Both start from the same decoded 640 x 480 class-index image; the planes arm's Pillow crop + resize is inside its time, as the
class arm's resize is. Prints one JSON line (and appends it to --out when given) with both times, their ratio and whether the two
arms' outputs were torch.equal.

    PYTHONPATH=. python tools/sem_bench.py [--reps 20] [--warmup 3] [--out profiles/sem/sem_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    from PIL import Image
    from gligen_amd import synthetic as syn
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    dev = torch.device("cuda:0")
    B, n_cls = args.batch, 152
    mod = "ldm.modules.diffusionmodules.sem_grounding_"
    cfg = dict(syn.UNET_CFG_SMALL,      # the small UNet carries the tokenizer's weights; it is not run
               grounding_downsampler=dict(target=mod + "downsampler.GroundingDownsampler", params=dict(resize_input=256, in_dim=n_cls, out_dim=8)),
               grounding_tokenizer=dict(target=mod + "net.PositionNet", params=dict(resize_input=448, in_dim=n_cls, out_dim=768)))
    model = syn.fill_module_(UNetModel(**cfg).eval(), 1234).to(dev)
    eng, pn, ds = model.engine, model.position_net, model.downsample_net
    w, h = 640, 480
    src = np.random.RandomState(0).randint(0, n_cls, (h // 8, w // 8), dtype=np.uint8).repeat(8, 0).repeat(8, 1)     # 8 x 8 segments
    c = min(w, h)
    left, top = int(round((w - c) / 2.0)), int(round((h - c) / 2.0))
    mask = torch.ones(B, 1, device=dev)
    out = {}

    def planes_arm():
        im = Image.fromarray(src).crop((left, top, left + c, top + c)).resize((512, 512), Image.NEAREST)
        sem = torch.from_numpy(np.asarray(im).copy()).long()
        planes = torch.zeros(n_cls, 512, 512).scatter_(0, sem.unsqueeze(0), 1.0).unsqueeze(0).repeat(B, 1, 1, 1).to(dev)
        out["planes"] = (pn.tokens(engine=eng, sem=planes, mask=mask), ds(planes, engine=eng))

    def class_arm():
        cls = eng.class_map_resize([torch.from_numpy(src)], (512, 512), [(left, top, c, c)]).unsqueeze(1).repeat(B, 1, 1, 1)
        out["classes"] = (pn.tokens(engine=eng, sem=cls, mask=mask), ds(cls, engine=eng))

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        planes_arm(); class_arm()
    tp, tc = [], []
    for _ in range(args.reps):
        tp.append(timed(planes_arm))
        tc.append(timed(class_arm))
    equal = all(torch.equal(a, b) for a, b in zip(out["planes"], out["classes"]))
    mp, mc = statistics.median(tp), statistics.median(tc)
    line = json.dumps(dict(bench="sem_conditioning", batch=B, size=512, tok_resize=448, ds_resize=256, reps=args.reps, planes_ms=round(mp, 3),
                           classes_ms=round(mc, 3), planes_min_ms=round(min(tp), 3), classes_min_ms=round(min(tc), 3), speedup=round(mp / mc, 2),
                           outputs_equal=bool(equal)))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    model._drop_engine()
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
