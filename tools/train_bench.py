"""Wall time of one training iteration (gl_unet_train_step: forward + loss + backward) of the correctness path, per configuration:
small UNet at a 16 x 16 latent, the shipped topology at 16 x 16 and at the real 64 x 64 latent. Synthetic inputs, seeded weights.
--spatial MODALITY: the shipped topology with that spatial-map tokenizer (ConvNeXt-tiny, resize 256: 64 tokens) and grounding
downsampler instead (gl_unet_train_step_spatial), B = 4, 64 x 64 latent, checkpoint=True. --class-maps (with --spatial sem): the same
iteration fed from the u8 class maps of those planes (gl_unet_train_step_spatial_classes).
--inpaint: the shipped topology with inpaint_mode (9-channel first conv, its weight trained), B = 4, 64 x 64 latent with --full64
(else B = 1, 16 x 16), checkpoint=True, the step inputs made by Engine.train_step_inputs inside the timed region; next to the text
model's line, and the time of one train_step_inputs launch next to the torch sequence it replaces (q_sample, mask, concat, two
permutes), medians of 20.
--fuser gatedSA2|gatedCA: the shipped topology with that fuser type, next to the gatedSA text model's line on the same box (with
--full64: B = 4, 64 x 64 latent, checkpoint=True; else B = 1, 16 x 16): gatedCA with the text tokenizer (30 slots); gatedSA2 with
--spatial canny (resize 256: an 8 x 8 token grid) or with the text tokenizer and 16 box slots (a 4 x 4 grid). gatedSA2 also prints one
grid_resize forward + backward (8 -> 64, C 320, B 4) next to torch's F.interpolate forward + backward on the device, medians of 20.
--ema: whole TrainStep iterations (forward, loss, backward, AdamW over the buckets) of the shipped text model, B = 4, 64 x 64 latent,
checkpoint=True, in three settings run in alternation on one box: no EMA, the EMA fused into the optimizer launch
(gl_op_adamw_ema_step), and the EMA as the two torch ops per bucket (mul_, add_: the reference's update_ema) behind gl_op_adamw_step
on the communication stream; then the two optimizer kernels alone on the largest bucket (HIP events, median of 20, bytes / time).
   PYTHONPATH=. python tools/train_bench.py [--full64] [--spatial {canny,depth,normal,hed,sem} [--class-maps] | --inpaint]
                                            [--fuser {gatedSA2,gatedCA}] | --ema"""
import json
import sys
import time

import torch

from gligen_amd import synthetic as syn
from gligen_amd.engine import Engine


def run(name, cfg, B, hw, reps, eng, checkpoint=False, cache=False, max_objs=30):
    model_shapes = None
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    if cfg.get("fuser_type", "gatedSA") != "gatedSA":
        name = f"{name}, {cfg['fuser_type']} fusers, {max_objs} box slots"
    m = UNetModel(**dict(cfg, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=False))
    sd = {k: v.float().to(eng.device).contiguous() for k, v in syn.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 1234).items()}
    del m
    b = syn.make_batch("text", B, n_valid=3, seed=5, max_objs=max_objs)
    batch = dict(x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441, 300, 77][:B]).float(), context=syn.make_context(B, seed=6),
                 boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"], target=syn.make_latent(B, 4, hw, hw, seed=7))
    grads = {k: torch.zeros_like(v) for k, v in sd.items() if ".fuser." in k or k.startswith("position_net.")}
    eng = Engine(0, arena_gb=160.0)                      # a fresh arena per line: its high water is this configuration's
    if cache:
        eng.train_weight_cache(True)                     # the frozen parameters' bf16 operand copies kept across iterations (gl_train_weight_cache)
    eng.unet_train_step(cfg, sd, batch, grads=grads, checkpoint=checkpoint, use_weight_cache=cache)     # warm-up (GEMM tile selection; fills the cache)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(reps):
        loss, _, _ = eng.unet_train_step(cfg, sd, batch, grads=grads, checkpoint=checkpoint, use_weight_cache=cache)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / reps
    print(json.dumps(dict(config=name, B=B, latent=hw, checkpoint=bool(checkpoint), weight_cache=bool(cache), weight_cache_gb=round(eng.train_weight_cache(True) / 2 ** 30, 2) if cache else 0,
                          s_per_iteration=round(dt, 4), loss=float(loss), arena_high_water_gb=round(eng.arena_high_water() / 2 ** 30, 2),
                          trainable_values=sum(int(g.numel()) for g in grads.values()))), flush=True)
    if cache:
        eng.train_weight_cache(False)


def run_spatial(modality, B, hw, reps, checkpoint=True, class_maps=False, fuser="gatedSA"):
    """The shipped topology (syn.UNET_CFG) with a spatial-map tokenizer and its downsampler (configs/cc3m_canny.yaml etc.).
    class_maps: sem's one-hot planes replaced by their u8 class map, argmax over the planes."""
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from gligen_amd.engine import SPATIAL_MAP_KEYS
    from gligen_amd.train import trainable_names
    ds_params = dict(out_dim=1) if modality == "hed" else dict(resize_input=4 * hw, out_dim=8)
    tk_params = dict(resize_input=256, out_dim=768)
    if modality == "sem":
        ds_params["in_dim"], tk_params["in_dim"] = 152, 152
    cfg = dict(syn.UNET_CFG, fuser_type=fuser, grounding_downsampler=dict(target=f"ldm.modules.diffusionmodules.{modality}_grounding_downsampler.GroundingDownsampler", params=ds_params),
               grounding_tokenizer=dict(target=f"ldm.modules.diffusionmodules.{modality}_grounding_net.PositionNet", params=tk_params))
    m = UNetModel(**dict(cfg, inpaint_mode=False))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    del m
    eng = Engine(0, arena_gb=160.0)
    sd = {k: v.float().to(eng.device).contiguous() for k, v in syn.seeded_state_dict(shapes, 1234).items()}
    img = syn.make_spatial_map(modality, B, 256, seed=3)
    if class_maps:
        if modality != "sem":
            raise SystemExit("--class-maps: only the sem model reads class maps")
        img = img.argmax(1, keepdim=True).to(torch.uint8)
    batch = {SPATIAL_MAP_KEYS[modality]: img, "mask": torch.ones(B, 1), "grounding_extra_input": img, "x": syn.make_latent(B, 4, hw, hw, seed=6),
             "timesteps": torch.tensor([981, 441, 300, 77][:B]).float(), "context": syn.make_context(B, seed=6), "target": syn.make_latent(B, 4, hw, hw, seed=7)}
    grads = {k: torch.zeros_like(sd[k]) for k in trainable_names(sd, cfg)}
    eng.unet_train_step(cfg, sd, batch, grads=grads, checkpoint=checkpoint)     # warm-up (GEMM tile selection)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(reps):
        loss, _, _ = eng.unet_train_step(cfg, sd, batch, grads=grads, checkpoint=checkpoint)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / reps
    print(json.dumps(dict(config=f"shipped topology, {modality} tokenizer + downsampler" + ("" if fuser == "gatedSA" else f", {fuser} fusers"), inputs="u8 class maps" if class_maps else "fp32 planes", B=B, latent=hw,
                          tok_resize=256, checkpoint=bool(checkpoint),
                          s_per_iteration=round(dt, 4), loss=float(loss), arena_high_water_gb=round(eng.arena_high_water() / 2 ** 30, 2),
                          trainable_values=sum(int(g.numel()) for g in grads.values()))), flush=True)


def run_inpaint(B, hw, reps, checkpoint=True):
    """The shipped topology (syn.UNET_CFG) with inpaint_mode: z, noise, timesteps and boxes on the device, train_step_inputs and
    unet_train_step per iteration."""
    from gligen_amd.train import trainable_names
    from ldm.models.diffusion.ldm import LatentDiffusion
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    cfg = dict(syn.UNET_CFG, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=True)
    m = UNetModel(**cfg)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    del m
    eng = Engine(0, arena_gb=160.0)
    dev = eng.device
    sd = {k: v.float().to(dev).contiguous() for k, v in syn.seeded_state_dict(shapes, 1234).items()}
    diff = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
    sched = {k: getattr(diff, k).float().to(dev).contiguous() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}
    b = syn.make_batch("text", B, n_valid=3, seed=5)
    z, noise = syn.make_latent(B, 4, hw, hw, seed=6).to(dev), syn.make_latent(B, 4, hw, hw, seed=7).to(dev)
    t = torch.tensor([981, 441, 300, 77][:B], device=dev)
    boxes = b["boxes"].to(dev)
    rest = dict(context=syn.make_context(B, seed=6).to(dev), boxes=boxes, masks=b["masks"].to(dev), positive_embeddings=b["text_embeddings"].to(dev))
    grads = {k: torch.zeros_like(sd[k]) for k in trainable_names(sd, cfg)}
    step = lambda: eng.unet_train_step(cfg, sd, dict(rest, **eng.train_step_inputs(z, noise, t, sched, boxes=boxes, inpaint=True)), grads=grads, checkpoint=checkpoint)
    step()                                               # warm-up (GEMM tile selection)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(reps):
        loss, _, _ = step()
    torch.cuda.synchronize()
    dt = (time.time() - t0) / reps
    print(json.dumps(dict(config="shipped topology, inpaint_mode (9-channel first conv)", B=B, latent=hw, checkpoint=bool(checkpoint),
                          s_per_iteration=round(dt, 4), loss=float(loss), arena_high_water_gb=round(eng.arena_high_water() / 2 ** 30, 2),
                          trainable_values=sum(int(g.numel()) for g in grads.values()))), flush=True)

    # the input stage alone: one launch against the torch sequence of trainer.py:342-344, 356 plus the two permute copies of the NCHW form
    def torch_inputs():
        a = sched["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1)
        s1 = sched["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1)
        x_noisy = a * z + s1 * noise
        q = (boxes * hw).to(torch.int64)
        ar = torch.arange(hw, device=dev)
        inx = (ar[None, None, :] >= q[:, :, 0, None]) & (ar[None, None, :] < q[:, :, 2, None])
        iny = (ar[None, None, :] >= q[:, :, 1, None]) & (ar[None, None, :] < q[:, :, 3, None])
        mask = 1.0 - (iny[:, :, :, None] & inx[:, :, None, :]).any(dim=1, keepdim=True).float()
        x9 = torch.cat([x_noisy, z * mask, mask], dim=1)
        return x9.permute(0, 2, 3, 1).contiguous(), noise.permute(0, 2, 3, 1).contiguous()

    ref_rows, ref_target = torch_inputs()
    out = eng.train_step_inputs(z, noise, t, sched, boxes=boxes, inpaint=True)
    same = bool(torch.equal(out["target_rows"], ref_target) and torch.equal(out["x_rows"][..., 4:], ref_rows[..., 4:]))     # (torch on the GPU may contract a z + s n)

    print(json.dumps(dict(config="step inputs", B=B, latent=hw, train_step_inputs_ms=round(median_ms(lambda: eng.train_step_inputs(z, noise, t, sched, boxes=boxes, inpaint=True)), 4),
                          torch_sequence_ms=round(median_ms(torch_inputs), 4), mask_and_target_equal=same, timing="host wall time around one synchronised call, median of 20")), flush=True)
    eng.close()


def run_ema(B=4, hw=64, reps=5, rate=0.9999):
    """One TrainStep, switched between the three settings from iteration to iteration: the same parameters, buckets and cached
    operand copies under all of them."""
    from gligen_amd.train import TrainStep
    from gligen_amd.trainer import synthetic_state_dict
    cfg = dict(syn.UNET_CFG, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=False)
    eng = Engine(0, arena_gb=24.0)
    dev = eng.device
    ts = TrainStep(eng, cfg, synthetic_state_dict(cfg), lr=5e-5, weight_decay=0.0, world=1, checkpoint=True, ema_rate=rate)
    b = syn.make_batch("text", B, n_valid=3, seed=5)
    batch = {k: v.to(dev) for k, v in dict(x=syn.make_latent(B, 4, hw, hw, seed=6), timesteps=torch.tensor([981, 441, 300, 77][:B]).float(),
                                           context=syn.make_context(B, seed=6), boxes=b["boxes"], masks=b["masks"], positive_embeddings=b["text_embeddings"],
                                           target=syn.make_latent(B, 4, hw, hw, seed=7)).items()}
    bufs = ts.ema
    ema_of = {p.data_ptr(): e for p, e in zip(ts.pbuf.buckets, bufs)}
    plain_step = eng.op_adamw_step

    def adamw_then_torch_ema(p, g, m, v, step, **kw):        # update_ema (trainer.py:121-123) behind the update, on the stream it ran on
        plain_step(p, g, m, v, step, **kw)
        ema_of[p.data_ptr()].mul_(rate).add_(p, alpha=1 - rate)

    def setting(name):
        ts.ema = bufs if name == "fused" else None
        eng.op_adamw_step = adamw_then_torch_ema if name == "torch_ops" else plain_step

    names = ("off", "fused", "torch_ops")
    times = {n: [] for n in names}
    for n in names:                                          # warm-up: GEMM tile selection, the operand cache, the allocator
        setting(n)
        ts.step(batch)
    torch.cuda.synchronize()
    for _ in range(reps):
        for n in names:
            setting(n)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = ts.step(batch)
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
    setting("off")
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    print(json.dumps(dict(config="shipped topology, TrainStep iteration (forward + loss + backward + AdamW), EMA off / fused / two torch ops per bucket", B=B, latent=hw,
                          checkpoint=True, ema_rate=rate, buckets=len(ts.pbuf.buckets), trainable_values=sum(int(x.numel()) for x in ts.pbuf.buckets),
                          s_per_iteration={n: round(med[n], 4) for n in names}, s_per_iteration_min={n: round(min(times[n]), 4) for n in names},
                          timing=f"host wall time around one synchronised iteration, median of {reps}, the three settings in alternation", loss=float(loss))), flush=True)
    i = max(range(len(ts.pbuf.buckets)), key=lambda k: ts.pbuf.buckets[k].numel())
    p, g, m, v, e = ts.pbuf.buckets[i], ts.gbuf.buckets[i], ts.m[i], ts.v[i], bufs[i]
    n = int(p.numel())

    def event_ms(fn, reps=20):
        out = []
        for _ in range(reps):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); z.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(z))
        return sorted(out)[reps // 2]

    kw = dict(lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    t_fused = event_ms(lambda: eng.op_adamw_ema_step(p, g, m, v, e, 3, ema_rate=rate, **kw))
    t_adamw = event_ms(lambda: plain_step(p, g, m, v, 3, **kw))
    t_torch = event_ms(lambda: e.mul_(rate).add_(p, alpha=1 - rate))
    print(json.dumps(dict(config="optimizer kernels on the largest bucket", elements=n, adamw_ema_us=round(t_fused * 1e3, 1), adamw_ema_GBps=round(36.0 * n / t_fused / 1e6, 1),
                          adamw_us=round(t_adamw * 1e3, 1), adamw_GBps=round(28.0 * n / t_adamw / 1e6, 1), torch_mul_add_us=round(t_torch * 1e3, 1),
                          torch_mul_add_GBps=round(20.0 * n / t_torch / 1e6, 1), timing="HIP events around one launch (torch: two), median of 20",
                          bytes="36 B / 28 B / 20 B per element")), flush=True)
    eng.train_weight_cache(False)
    eng.close()


def median_ms(fn, n=20):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t1) * 1e3)
    return sorted(ts)[n // 2]


def run_grid_resize(B=4, sg=8, sv=64, C=320):
    """One grid_resize forward + backward (the gatedSA2 residual of the 64 x 64 level) next to F.interpolate(mode="bicubic") forward +
    backward on the device for the same tensor (NCHW there: torch's layout)."""
    eng = Engine(0, arena_gb=1.0)
    dev = eng.device
    gen = torch.Generator().manual_seed(11)
    t = torch.randn(B, sg * sg, C, generator=gen).to(dev)
    g = torch.randn(B, sv * sv, C, generator=gen).to(dev)
    x = t.permute(0, 2, 1).reshape(B, C, sg, sg).contiguous().requires_grad_(True)
    gy = g.permute(0, 2, 1).reshape(B, C, sv, sv).contiguous()

    def ours():
        eng.op_grid_resize(t, sg, sv)
        eng.op_grid_resize_backward(g, sg, sv)

    def torchs():
        x.grad = None
        torch.nn.functional.interpolate(x, (sv, sv), mode="bicubic").backward(gy)

    ours(); torchs()
    print(json.dumps(dict(config="grid resize forward + backward", B=B, sg=sg, sv=sv, C=C, grid_resize_ms=round(median_ms(ours), 4),
                          torch_interpolate_ms=round(median_ms(torchs), 4), timing="host wall time around one synchronised forward + backward, median of 20")), flush=True)
    eng.close()


if __name__ == "__main__":
    fuser = sys.argv[sys.argv.index("--fuser") + 1] if "--fuser" in sys.argv else "gatedSA"
    if fuser not in ("gatedSA", "gatedSA2", "gatedCA"):
        raise SystemExit("--fuser gatedSA2 | gatedCA")
    if fuser == "gatedCA" and "--spatial" in sys.argv:
        raise SystemExit("--fuser gatedCA: with the text tokenizer")
    if "--ema" in sys.argv:
        run_ema()
        sys.exit(0)
    if fuser != "gatedSA" and "--spatial" not in sys.argv:
        full = "--full64" in sys.argv
        shape = (4, 64, 1) if full else (1, 16, 2)
        run("shipped topology", syn.UNET_CFG, *shape, Engine(0, arena_gb=1.0), checkpoint=True)     # the gatedSA text model's line, same box
        run("shipped topology", dict(syn.UNET_CFG, fuser_type=fuser), *shape, Engine(0, arena_gb=1.0), checkpoint=True, max_objs=16 if fuser == "gatedSA2" else 30)
        if fuser == "gatedSA2":
            run_grid_resize()
        sys.exit(0)
    if "--inpaint" in sys.argv:
        full = "--full64" in sys.argv
        run("shipped topology", syn.UNET_CFG, 4 if full else 1, 64 if full else 16, 1 if full else 2, Engine(0, arena_gb=1.0), checkpoint=True)     # the text model's line, same box
        run_inpaint(4 if full else 1, 64 if full else 16, 1 if full else 2)
        sys.exit(0)
    if "--spatial" in sys.argv:
        modality = sys.argv[sys.argv.index("--spatial") + 1]
        if "--full64" in sys.argv:
            run("shipped topology", syn.UNET_CFG, 4, 64, 1, Engine(0, arena_gb=1.0), checkpoint=True)     # the text model's line, same box
            run_spatial(modality, 4, 64, 1, class_maps="--class-maps" in sys.argv, fuser=fuser)
        else:
            run_spatial(modality, 1, 16, 2, class_maps="--class-maps" in sys.argv, fuser=fuser)
        if fuser == "gatedSA2":
            run_grid_resize()
        sys.exit(0)
    eng = Engine(0, arena_gb=160.0)
    if "--b4only" in sys.argv:          # the profiled line (tools/gpu_run.sh train with TRAIN_PROF=1): the bench line's train_step shape
        run("shipped topology", syn.UNET_CFG, 4, 64, 2, eng, checkpoint=True)
        run("shipped topology", syn.UNET_CFG, 4, 64, 2, eng, checkpoint=True, cache=True)
        sys.exit(0)
    run("small UNet", syn.UNET_CFG_SMALL, 2, 16, 3, eng)
    run("shipped topology", syn.UNET_CFG, 1, 16, 2, eng)
    if "--full64" in sys.argv:
        run("shipped topology", syn.UNET_CFG, 1, 64, 1, eng)
        run("shipped topology", syn.UNET_CFG, 1, 64, 1, eng, checkpoint=True)
        run("shipped topology", syn.UNET_CFG, 4, 64, 1, eng, checkpoint=True)
