"""Time the CLIP text tower: transformers on the device (FrozenCLIPEmbedder backend="hf", what run() does without --native_clip)
against the native engine (backend="hip"), alternating in one process on the same device, HIP events, medians.

Line 1: S = 32 sequences of 77 tokens through the full seeded tower (12 layers, width 768: 13.3 GFLOP per sequence, 426 GF per call).
Line 2: the phrase path of prepare_batch with 8 phrases -- parent: get_clip_feature through CLIPModel, one call per phrase, each with
its dummy 224 x 224 vision-tower pass (reference gligen_inference.py:104-128), on seeded weights; native: one batched encode_ids.
Line 3: 8 image features (ViT-L/14, 257 tokens) -- parent: get_clip_feature(..., is_image=True) through CLIPModel on the device, one
call per image, each with its dummy four-token text pass; native: get_clip_image_features, one batched call through the native
vision tower. The pixel tensors are prepared beforehand (the processor and Image.open are stand-ins that hand them out), so PIL is in
neither arm; both read `projection_matrix` as the functions do. Also the time of one clip_attn_long_kernel launch at S = 8, T = 257.
Line 4: the image preprocessing in front of line 3, for eight 640 x 480 and for eight 1920 x 1080 u8 images -- host: transformers'
CLIPImageProcessor on PIL images (what get_clip_image_features(..., preprocess="processor") calls), its pixel_values left on the host
as the processor returns them; native: Engine.clip_vision_preprocess on the same pixels as host arrays, i.e. INCLUDING the
host-to-device copy of the u8 pixels, pixel_values left on the device where the tower reads them. native_GBps = source bytes / time.

    PYTHONPATH=. python tools/clip_bench.py [--reps 20] [--warmup 3] [--no-phrases] [--no-images] [--no-preprocess] [--preprocess-only]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
_spec = importlib.util.spec_from_file_location("make_golden_clip", os.path.join(REPO, "tools", "make_golden_clip.py"))
mgc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgc)


def timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(torch.cuda.current_stream(dev))
    fn()
    e1.record(torch.cuda.current_stream(dev))
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(a, b, dev, warmup, reps):
    for _ in range(warmup):
        a(); b()
    torch.cuda.synchronize(dev)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a, dev))
        tb.append(timed(b, dev))
    return statistics.median(ta), statistics.median(tb)


def bench_preprocess(dev, warmup, reps):
    import numpy as np
    import transformers
    from PIL import Image
    from gligen_amd.runtime import clip_preprocess_settings, scratch_engine
    proc = transformers.CLIPImageProcessor()
    kw = clip_preprocess_settings(proc, 224)
    eng = scratch_engine(dev)
    rec = dict(bench="image_preprocess", images=8, reps=reps)
    for name, (w, h) in (("640x480", (640, 480)), ("1920x1080", (1920, 1080))):
        arrays = [np.random.RandomState(i).randint(0, 256, (h, w, 3), dtype=np.uint8) for i in range(8)]
        pils = [Image.fromarray(a) for a in arrays]
        host = lambda: proc(images=pils, return_tensors="pt")["pixel_values"]
        native = lambda: eng.clip_vision_preprocess(arrays, **kw)
        equal = bool(torch.equal(host(), native().cpu()))
        t_host, t_nat = alternate(host, native, dev, warmup, reps)
        src = sum(a.nbytes for a in arrays)
        rec[name] = dict(processor_host_ms=round(t_host, 3), native_ms=round(t_nat, 3), speedup=round(t_host / t_nat, 2), source_MB=round(src / 1e6, 2),
                         native_GBps=round(src / t_nat / 1e6, 2), bit_equal=equal)
    print(json.dumps(rec))


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-phrases", action="store_true")
    ap.add_argument("--no-images", action="store_true")
    ap.add_argument("--no-preprocess", action="store_true")
    ap.add_argument("--preprocess-only", action="store_true")
    a = ap.parse_args()
    if a.preprocess_only:
        return bench_preprocess(torch.device("cuda:0"), a.warmup, a.reps)
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    import gligen_inference as gi
    dev = torch.device("cuda:0")
    gi.device = dev
    tower = mgc.build_tower(12, 3072)
    hf = FrozenCLIPEmbedder(device=str(dev), backend="hf")
    hf.transformer = tower
    hf = hf.to(dev)
    hip = FrozenCLIPEmbedder(device=str(dev), backend="hip")
    hip.transformer = tower                      # the same parameters: the native engine packs its own copy
    hip = hip.to(dev)
    g = torch.Generator().manual_seed(11)
    S = 32
    ids = torch.full((S, 77), mgc.EOS, dtype=torch.int64)
    ids[:, 0] = mgc.BOS
    for i in range(S):
        n = 1 + int(torch.randint(0, 75, (1,), generator=g))
        ids[i, 1:1 + n] = torch.randint(0, mgc.BOS, (n,), generator=g)
    ids_dev = ids.to(dev)
    n0 = hip.engine.launch_count()
    hip.encode_ids(ids)
    launches = hip.engine.launch_count() - n0      # first call: includes the tile tuner's timed launches
    hip.encode_ids(ids)
    n1 = hip.engine.launch_count()
    hip.encode_ids(ids)
    launches = hip.engine.launch_count() - n1
    t_hf, t_hip = alternate(lambda: hf.encode_ids(ids_dev), lambda: hip.encode_ids(ids), dev, a.warmup, a.reps)
    gf = S * 13.3
    print(json.dumps(dict(bench="clip_text_encode", sequences=S, tokens=77, reps=a.reps, hf_ms=round(t_hf, 3), hip_ms=round(t_hip, 3),
                          speedup=round(t_hf / t_hip, 3), launches=launches, hip_tflops=round(gf / t_hip, 2), hf_tflops=round(gf / t_hf, 2))))
    if a.no_phrases:
        return
    # ---- the phrase path: 8 phrases of 2 .. 9 tokens
    import transformers
    from gligen_amd import synthetic as syn
    tcfg = tower.config
    vcfg = transformers.CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, patch_size=14,
                                         image_size=224, projection_dim=768)      # openai/clip-vit-large-patch14's vision tower
    clip = transformers.CLIPModel(transformers.CLIPConfig(text_config=tcfg.to_dict(), vision_config=vcfg.to_dict(), projection_dim=768)).eval()
    syn.fill_module_on_device_(clip.to(dev), seed=778)
    phrases = []
    for i in range(8):
        n = 2 + i
        phrases.append(torch.cat([torch.tensor([mgc.BOS]), torch.randint(0, mgc.BOS, (n,), generator=g), torch.tensor([mgc.EOS])]))

    class Processor:                               # the tokenizer's output for a phrase (no tokenizer files offline)
        def __call__(self, text=None, **kw):
            return dict(input_ids=text[None], attention_mask=torch.ones(1, len(text), dtype=torch.int64))

    proc = Processor()
    padded = torch.full((8, 77), mgc.EOS, dtype=torch.int64)
    for i, p in enumerate(phrases):
        padded[i, :len(p)] = p
    t_par, t_nat = alternate(lambda: [gi.get_clip_feature(clip, proc, p, is_image=False) for p in phrases],
                             lambda: hip.encode_ids(padded, return_pooler_output=True), dev, a.warmup, a.reps)
    print(json.dumps(dict(bench="phrase_features", phrases=8, reps=a.reps, hf_clipmodel_ms=round(t_par, 3), hip_ms=round(t_nat, 3),
                          speedup=round(t_par / t_nat, 3))))
    if a.no_images:
        return
    # ---- the image path: 8 reference images, already preprocessed
    from gligen_amd.runtime import build_clip_vision_engine, scratch_engine
    pixels = (1.2 * torch.randn((8, 3, 224, 224), generator=g)).to(dev)

    class Opened:                                  # what Image.open(i).convert("RGB") hands to the processor: the index of a prepared tensor
        def __init__(self, i):
            self.i = i

        def convert(self, mode):
            return self

    class ImageProcessor:
        def __call__(self, images=None, **kw):
            return dict(pixel_values=pixels[[im.i for im in images]])

    class Images:
        open = staticmethod(Opened)

    gi.Image = Images
    iproc = ImageProcessor()
    vision = build_clip_vision_engine(clip)
    keep = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            torch.save(torch.randn(768, 768, generator=torch.Generator().manual_seed(5)) * 0.03, "projection_matrix")
            n0 = vision.launch_count()
            gi.get_clip_image_features(clip, iproc, list(range(8)), vision)      # first call: includes the tile tuner's timed launches
            n1 = vision.launch_count()
            nat = gi.get_clip_image_features(clip, iproc, list(range(8)), vision)
            launches = vision.launch_count() - n1
            par = [gi.get_clip_feature(clip, iproc, i, is_image=True) for i in range(8)]
            rel = float(((torch.cat(nat).double() - torch.cat(par).double()) ** 2).mean() / (torch.cat(par).double() ** 2).mean())
            t_par, t_nat = alternate(lambda: [gi.get_clip_feature(clip, iproc, i, is_image=True) for i in range(8)],
                                     lambda: gi.get_clip_image_features(clip, iproc, list(range(8)), vision), dev, a.warmup, a.reps)
        finally:
            os.chdir(keep)
    # one attention launch of the tower's shape on its own
    sc = scratch_engine(dev)
    qkv = torch.randn((8 * 257, 3 * 1024), generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(dev)
    out = torch.empty((8 * 257, 1024), dtype=torch.bfloat16, device=dev)
    attn = lambda: [sc.op_clip_attention(qkv, 8, 257, 16, False, out=out) for _ in range(50)]
    attn()
    t_attn = statistics.median(timed(attn, dev) for _ in range(a.reps)) / 50
    gf = 8 * 2 * (256 * 640 * 1024 + 24 * 257 * (4 * 1024 * 1024 + 2 * 1024 * 4096 + 2 * 257 * 1024)) / 1e9
    print(json.dumps(dict(bench="image_features", images=8, tokens=257, reps=a.reps, hf_clipmodel_ms=round(t_par, 3), hip_ms=round(t_nat, 3),
                          speedup=round(t_par / t_nat, 3), launches=launches, hip_tflops=round(gf / t_nat, 2), rel_mse_vs_hf_fp32_device=rel,
                          attn_long_us_per_launch_S8_T257_H16=round(1e3 * t_attn, 2))))
    if not a.no_preprocess:
        bench_preprocess(dev, a.warmup, a.reps)


if __name__ == "__main__":
    main()
