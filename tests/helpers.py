"""Shared test plumbing: golden loading, seeded models (product side) and oracle inputs."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gligen_amd import synthetic as syn  # noqa: E402

GINPUT = {
    "text": "grounding_input.text_grounding_tokinzer_input.GroundingNetInput",
    "text_image": "grounding_input.text_image_grounding_tokinzer_input.GroundingNetInput",
    "keypoint": "grounding_input.keypoint_grounding_tokinzer_input.GroundingNetInput",
}


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    out = {k: z[k] for k in z.files}
    if "meta" in out:
        out["meta"] = json.loads(str(out["meta"]))
    return out


def golden_shapes(name):
    return json.load(open(os.path.join(GOLDEN, "state_dict_shapes.json")))[name]


def oracle_cfg(cfg, kind):
    return dict(model_channels=cfg["model_channels"], channel_mult=cfg["channel_mult"], num_res_blocks=cfg["num_res_blocks"],
                attention_resolutions=cfg["attention_resolutions"], num_heads=cfg["num_heads"], grounding_kind=kind,
                fuser_type=cfg.get("fuser_type", "gatedSA"))


def unet_inputs(meta):
    """The exact inputs oracle/make_golden.py:unet_case fed to the reference."""
    B, hw, kind = meta["B"], meta["hw"], meta["kind"]
    batch = syn.make_batch(kind, B, n_valid=meta["n_valid"], seed=1, max_objs=meta.get("max_objs", 30))
    x = syn.make_latent(B, 4, hw, hw, seed=1)
    ctx = syn.make_context(B, seed=1)
    t = torch.tensor([981, 441][:B] if B <= 2 else [981] * B, dtype=torch.long)
    extra = None
    if meta["inpaint"]:
        from oracle.gligen_oracle import draw_masks_from_boxes
        mask = draw_masks_from_boxes(batch["boxes"], hw)
        z0 = syn.make_latent(B, 4, hw, hw, seed=2)
        extra = torch.cat([z0 * mask, mask], dim=1)
    return batch, x, ctx, t, extra


def grounding_kwargs(kind, batch):
    if kind == "text":
        return dict(boxes=batch["boxes"], masks=batch["masks"], positive_embeddings=batch["text_embeddings"])
    return dict(batch)


def build_product_unet(cfg, kind, inpaint=False, seed=1234, device=None):
    """This repo's drop-in UNetModel with seeded weights (+ its grounding_tokenizer_input)."""
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from ldm.util import instantiate_from_config
    model = UNetModel(**dict(cfg, grounding_tokenizer=syn.GROUNDING_TOKENIZERS[kind], inpaint_mode=inpaint)).eval()
    syn.fill_module_(model, seed)
    model.grounding_tokenizer_input = instantiate_from_config(dict(target=GINPUT[kind]))
    if device is not None:
        model = model.to(device)
    return model


def build_product_vae(ddconfig, seed=4321, device=None):
    from ldm.models.autoencoder import AutoencoderKL
    ae = AutoencoderKL(ddconfig=ddconfig, embed_dim=4, scale_factor=0.18215).eval()
    syn.fill_module_(ae, seed)
    if device is not None:
        ae = ae.to(device)
    return ae


def mse(a, b):
    a = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).float().cpu()
    b = torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).float().cpu()
    return float(((a - b) ** 2).mean())


def scripted_randn_like(noise, multistep=True):
    """A stand-in for torch.randn_like that replays recorded q_sample draws in the call order of the reference's sampling
    loop (plms.py:96-99 then the sigma_t * randn_like(x) of get_x_prev_and_pred_x0, twice on the first PLMS step):
    noise[i] for the q_sample slot of step i, zeros for the sigma = 0 draws."""
    state = dict(step=0, slot=0)

    def fn(like, *a, **k):
        i, slot = state["step"], state["slot"]
        n_dummy = 2 if (i == 0 and multistep) else 1
        out = noise[i].to(like) if slot == 0 else torch.zeros_like(like)
        if slot == 0:
            assert tuple(out.shape) == tuple(like.shape), (out.shape, like.shape)
        state["slot"] += 1
        if state["slot"] > n_dummy:
            state["step"], state["slot"] = i + 1, 0
        return out
    return fn


def block_backward_inputs(meta):
    """The inputs of the training-slice golden (oracle/make_golden.py: block_backward_case), regenerated from the same seeded
    CPU generator in the same order: x, objs, context, target."""
    import torch
    g = torch.Generator().manual_seed(4242)
    B, N, C, Ng, D, T = meta["B"], meta["hw"] ** 2, meta["C"], meta["Ng"], meta["ctx_dim"], meta["ctx_T"]
    x = torch.randn(B, N, C, generator=g)
    objs = torch.randn(B, Ng, D, generator=g) * 0.5
    context = torch.randn(B, T, D, generator=g)
    target = torch.randn(B, N, C, generator=g)
    return x, objs, context, target


def resblock_backward_inputs(meta):
    """The inputs of the ResBlock training-slice goldens (oracle/make_golden.py: resblock_backward_case), regenerated from the same
    seeded CPU generator in the same order: x, emb, target."""
    import torch
    g = torch.Generator().manual_seed(4343)
    B, hw = meta["B"], meta["hw"]
    x = torch.randn(B, meta["Cin"], hw, hw, generator=g)
    emb = torch.randn(B, meta["emb_dim"], generator=g)
    target = torch.randn(B, meta["Cout"], hw, hw, generator=g)
    return x, emb, target


def st_backward_inputs(meta):
    """The inputs of the SpatialTransformer training-slice golden (oracle/make_golden.py: st_backward_case): x, objs, context, target."""
    import torch
    g = torch.Generator().manual_seed(4444)
    B, hw, C, Ng, D, T = meta["B"], meta["hw"], meta["C"], meta["Ng"], meta["ctx_dim"], meta["ctx_T"]
    x = torch.randn(B, C, hw, hw, generator=g)
    objs = torch.randn(B, Ng, D, generator=g) * 0.5
    context = torch.randn(B, T, D, generator=g)
    target = torch.randn(B, C, hw, hw, generator=g)
    return x, objs, context, target


# ---- fabricated checkpoint pieces shared by the CPU loader tests and the GPU file -> image test ----------------------------
def _fake_omegaconf_pickle(path, payload):
    """Write `payload` (a dict of state_dicts + a nested config) the way the reference's trainer does
    (trainer.py:176,472-480: config_dict = vars(OmegaConf DictConfig)), with stand-in classes living in modules NAMED
    omegaconf.* so that the pickle stream references 'omegaconf.dictconfig DictConfig' etc. exactly like a real checkpoint."""
    import sys
    import types

    mods = {n: types.ModuleType(n) for n in ("omegaconf", "omegaconf.dictconfig", "omegaconf.listconfig", "omegaconf.nodes", "omegaconf.base")}

    def cls(mod, name):
        c = type(name, (), {"__module__": mod, "__getstate__": lambda self: dict(self.__dict__),
                            "__setstate__": lambda self, st: self.__dict__.update(st)})
        setattr(mods[mod], name, c)
        return c

    DictConfig, ListConfig = cls("omegaconf.dictconfig", "DictConfig"), cls("omegaconf.listconfig", "ListConfig")
    AnyNode, Meta = cls("omegaconf.nodes", "AnyNode"), cls("omegaconf.base", "ContainerMetadata")

    def wrap(v):
        if isinstance(v, dict):
            n = DictConfig()
            n.__dict__.update(_content={k: wrap(x) for k, x in v.items()}, _metadata=Meta(), _parent=None, _flags_cache=None)
            return n
        if isinstance(v, (list, tuple)):
            n = ListConfig()
            n.__dict__.update(_content=[wrap(x) for x in v], _metadata=Meta(), _parent=None, _flags_cache=None)
            return n
        n = AnyNode()
        n.__dict__.update(_val=v, _metadata=Meta(), _parent=None)
        return n

    cfg = payload.pop("config")
    payload["config_dict"] = dict(_content={k: wrap(v) for k, v in cfg.items()}, _metadata=Meta(), _parent=None, _flags_cache=None)
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        torch.save(payload, path)
    finally:
        for k, v in saved.items():
            if v is None:
                del sys.modules[k]
            else:
                sys.modules[k] = v


def _fabricated_clip(tmp_path, hidden=768, proj=768):
    import json as _json
    from transformers import CLIPConfig, CLIPImageProcessor, CLIPModel, CLIPProcessor, CLIPTextConfig, CLIPTokenizer, CLIPVisionConfig
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b); cs.append(256 + n); n += 1
    chars = [chr(c) for c in cs]
    vocab = {c: i for i, c in enumerate(chars)}
    vocab.update({c + "</w>": len(chars) + i for i, c in enumerate(chars)})
    vocab["<|startoftext|>"], vocab["<|endoftext|>"] = len(vocab), len(vocab) + 1
    (tmp_path / "vocab.json").write_text(_json.dumps(vocab))
    (tmp_path / "merges.txt").write_text("#version: 0.2\n")
    tok = CLIPTokenizer(str(tmp_path / "vocab.json"), str(tmp_path / "merges.txt"))
    tcfg = CLIPTextConfig(vocab_size=49408, hidden_size=hidden, intermediate_size=256, num_hidden_layers=2, num_attention_heads=8,
                          max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=proj, eos_token_id=vocab["<|endoftext|>"],
                          bos_token_id=vocab["<|startoftext|>"], pad_token_id=vocab["<|endoftext|>"])
    vcfg = CLIPVisionConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, image_size=224, patch_size=32,
                            projection_dim=proj)
    torch.manual_seed(0)
    model = CLIPModel(CLIPConfig(text_config=tcfg.to_dict(), vision_config=vcfg.to_dict(), projection_dim=proj)).eval()
    return model, CLIPProcessor(image_processor=CLIPImageProcessor(), tokenizer=tok), tok


# ---- attention with a spike channel: inputs that put chosen rows into a chosen softmax-stabiliser regime --------------------------
# Identity wq / wk and, per head, one reserved channel (channel 0 of the head: zero in xq, in xkv and in the matching columns of wv,
# so V never sees it). a_i in the reserved channel of query i and b_j in that of key j add exactly a_i b_j d^-0.5 log2(e) log2 units
# to the score (i, j) of that head: a rank-one bump that leaves every row with a_i = 0 bit-for-bit alone, unlike xkv[j] = gain * xq[i],
# which moves every query's score against key j. a is a power of two (16 by default) and b is rounded to bf16: exact operands.
# Key i carries the features of query i (self-attention's diagonal: ordinary rows have a dominant key somewhere along the row).
SPIKE_A = 16.0
# bump sizes in log2 units (at a = 16), and the band of log2(l / 2^stabiliser) each regime needs at the jump. From attn3_kernel's
# constants: the lazy move at l > 2^40, the rerun at l >= 1e30 = 2^99.7, exp2 overflow at 2^128 -- with a margin of a few units for
# the row's ordinary scores and for the bf16 roundings of b and of q * scale.
SPIKE_UNITS = {"quiet": 20.0, "lazy": 75.0, "overshoot": 122.0, "overflow": 360.0}
SPIKE_BANDS = {"quiet": (-1e9, 36.0), "lazy": (48.0, 90.0), "overshoot": (105.0, 120.0), "overflow": (140.0, 1e9)}
SPIKE_ROW, SPIKE_HEAD = 37, 3        # the grid's bump row: wave 1 of query block 0; its own key (37) lies in tile 0


def spike_attention_case(B, Nq, Nk, C, H, bumps=(), rows=None, device="cpu", seed=1):
    """bumps: [(sample, head, query rows, {key or (first key, end key): bump in log2 units}[, a])]. The rows of an entry see its
    bumps times a / 16; entries of one (sample, head) share their keys (the bump is rank one: every bumped row sees every bumped key).
    rows: the query rows to build the reference for (default: all). Returns the tensors op_attention takes, the float64 reference
    [B][len(rows)][C] of the softmax in float64 on the same bf16 inputs, and the score statistics of the regime checks."""
    import math
    from types import SimpleNamespace
    d = C // H
    c = d ** -0.5 * math.log2(math.e)
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, max(Nq, Nk), C, generator=g).to(torch.bfloat16)
    wv = torch.randn(C, C, generator=g) * C ** -0.5
    ch0 = torch.arange(H) * d
    base[:, :, ch0] = 0
    wv[:, ch0] = 0
    xq, xkv = base[:, :Nq].clone(), base[:, :Nk].clone()
    bumped = torch.zeros(B, H, Nq, dtype=torch.bool)
    for item in bumps:
        b, h, qrows, keys = item[:4]
        a = item[4] if len(item) > 4 else SPIKE_A
        assert math.log2(a) == int(math.log2(a)), "a is a power of two"
        xq[b, list(qrows), h * d] = a
        bumped[b, h, list(qrows)] = True
        for key, units in keys.items():
            k0, k1 = key if isinstance(key, tuple) else (key, key + 1)
            assert 0 <= k0 < k1 <= Nk
            val = torch.tensor(units / (SPIKE_A * c)).to(torch.bfloat16)
            old = xkv[b, k0:k1, h * d]
            assert bool(((old == 0) | (old == val)).all()), "two entries disagree about a key's bump"
            xkv[b, k0:k1, h * d] = val
    rows_t = torch.arange(Nq) if rows is None else torch.as_tensor(sorted(set(rows)))
    pos = {int(r): i for i, r in enumerate(rows_t.tolist())}
    R = len(rows_t)
    out = SimpleNamespace(B=B, Nq=Nq, Nk=Nk, C=C, H=H, d=d, rows=rows_t, xq=xq.to(device), xkv=xkv.to(device),
                          wq=torch.eye(C, device=device), wk=torch.eye(C, device=device), wv=wv.to(device))
    q = out.xq[:, rows_t.to(device)].double()
    k = out.xkv.double()
    v = k @ out.wv.to(torch.bfloat16).double().t()
    ref = torch.empty(B, R, C, dtype=torch.float64, device=device)
    excess0 = torch.empty(B, H, R, dtype=torch.float64, device=device)   # log2 sum_j 2^(s_j - max over tile 0)
    smin, smax = float("inf"), float("-inf")
    info = []
    for b in range(B):
        for h in range(H):
            hs = slice(h * d, (h + 1) * d)
            s = (q[b, :, hs] @ k[b, :, hs].t()) * c             # [R][Nk], log2 units
            m = s.max(1).values
            p = torch.exp2(s - m[:, None])
            l = p.sum(1)
            ref[b, :, hs] = (p @ v[b, :, hs]) / l[:, None]
            lse = m + torch.log2(l)
            excess0[b, h] = lse - s[:, :64].max(1).values
            ordinary = ~bumped[b, h][rows_t].to(device)
            if bool(ordinary.any()):
                smin, smax = min(smin, float(s[ordinary].min())), max(smax, float(s[ordinary].max()))
            for item in bumps:
                if item[0] != b or item[1] != h:
                    continue
                # the jump: the first tile that holds a key bumped upwards (downward bumps make the tiles after them jump)
                ups = [(key if isinstance(key, tuple) else (key, key + 1)) for key, u in item[3].items() if u > 0]
                downs = [(key if isinstance(key, tuple) else (key, key + 1)) for key, u in item[3].items() if u < 0]
                jt = min([k0 // 64 for k0, _ in ups] + [(k1 + 63) // 64 for _, k1 in downs if k1 < Nk] + [1 << 30])
                for r in item[2]:
                    if r not in pos:
                        continue
                    i = pos[r]
                    before = float(s[i, : 64 * jt].max()) if 0 < jt < (1 << 30) else None
                    info.append(dict(b=b, h=h, q=r, i=i, tile=jt if jt < (1 << 30) else None, a=item[4] if len(item) > 4 else SPIKE_A,
                                     excess0=float(excess0[b, h, i]),
                                     excess_before=None if before is None else float(lse[i]) - before))
    out.ref, out.excess0, out.bump_rows, out.bumped = ref, excess0, info, bumped
    out.ordinary_span = (smin, smax)
    return out


def spike_attention_metrics(case, y):
    """The figures every spike case is judged by (y: what op_attention returned for case.xq ...): all finite; max |y - ref| over all rows
    / max |ref| over the ordinary rows (no bump in any head); mean |y - ref| / mean |ref|; per bumped (row, head), max |y - ref| over
    that head's slice of the row / its own max |ref| -- the worst of them."""
    dev = case.ref.device
    rows = case.rows.to(dev)
    yy = y.to(dev).double()[:, rows]
    err = (yy - case.ref).abs()
    ordinary = ~case.bumped.any(1)[:, case.rows].to(dev)            # [B][R]
    d = case.d
    worst_row = 0.0
    for br in case.bump_rows:
        hs = slice(br["h"] * d, (br["h"] + 1) * d)
        worst_row = max(worst_row, float(err[br["b"], br["i"], hs].max() / case.ref[br["b"], br["i"], hs].abs().max()))
    return dict(finite=bool(torch.isfinite(yy).all()),
                max_rel=float(err.max() / case.ref[ordinary].abs().max()),
                mean_rel=float(err.mean() / case.ref.abs().mean()),
                row_rel=worst_row)


def spike_positions(Nk):
    """{position name: (key, tile)} of the jump positions: tile 0, tile 1, a middle tile (31 where the row has it), the tile before the
    last full tile, the last full tile, and a key inside the ragged tail where there is one. Positions that fall on the same tile
    are listed once."""
    nt = (Nk + 63) // 64
    full = Nk // 64
    want = [("tile0", 0), ("tile1", 1), ("mid", 31 if nt > 34 else nt // 2), ("before_last_full", full - 2), ("last_full", full - 1)]
    out, seen = {}, set()
    for name, t in want:
        if 0 <= t < full and t not in seen:
            seen.add(t)
            out[name] = (64 * t + 20, t)
    if Nk % 64:
        out["ragged_tail"] = (64 * full + (Nk % 64) // 2, full)
    return out


SPIKE_GRID_SHAPES = {40: [(1, 4096, 4096, 320), (1, 4096, 4126, 320), (1, 256, 160, 320)],
                     80: [(1, 1024, 1054, 640), (1, 4096, 4126, 640)]}


def spike_grid(d):
    """[(id, (B, Nq, Nk, C), regime, position name, tile, bumps)]: every jump position x {lazy, finite overshoot, overflow} at d = 40,
    x {lazy, overflow} at d = 80 (H = 8), one bumped row (SPIKE_ROW of head SPIKE_HEAD)."""
    out = []
    for shape in SPIKE_GRID_SHAPES[d]:
        B, Nq, Nk, C = shape
        for pname, (key, tile) in spike_positions(Nk).items():
            for regime in (("lazy", "overshoot", "overflow") if d == 40 else ("lazy", "overflow")):
                bumps = [(0, SPIKE_HEAD, [SPIKE_ROW], {key: SPIKE_UNITS[regime]})]
                out.append((f"d{d}-{Nq}x{Nk}-{pname}-{regime}", shape, regime, pname, tile, bumps))
    return out


# ---- the small training slices against their goldens: one report (relative MSE per tensor; "loss": relative error) per slice, shared by
# test_ops_gpu.py (default path) and train_switches_child.py (the developer switches' paths)
def rel_mse(a, ref):
    a, ref = a.detach().float().cpu(), torch.as_tensor(ref).float()
    return float(((a - ref) ** 2).mean() / (ref ** 2).mean().clamp_min(1e-30))


def _npz(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    return g, json.loads(bytes(g["meta"]).decode())


def fuser_block_train_report(engine):
    """gl_op_block_train on tests/golden/block_backward_gatedsa.npz -> (report, case): case holds the golden, its meta, the state_dict
    and the inputs."""
    from ldm.modules.attention import BasicTransformerBlock
    g, meta = _npz("block_backward_gatedsa")
    x, objs, context, target = block_backward_inputs(meta)
    assert abs(float(x.double().sum()) - float(g["x_sum"])) < 1e-6 and abs(float(target.double().sum()) - float(g["target_sum"])) < 1e-6
    blk = BasicTransformerBlock(meta["C"], meta["ctx_dim"], meta["ctx_dim"], meta["heads"], meta["C"] // meta["heads"], "gatedSA")
    sd = syn.seeded_state_dict({k: tuple(v.shape) for k, v in blk.state_dict().items()}, meta["seed"])
    sd["fuser.alpha_attn"] = torch.tensor(meta["alpha_attn"])
    sd["fuser.alpha_dense"] = torch.tensor(meta["alpha_dense"])
    assert sorted(engine.block_train_param_names()) == sorted(sd.keys())
    y, loss, dx, dobjs, grads = engine.op_block_train(sd, x, objs, context, target, meta["heads"])
    report = {"y": rel_mse(y, g["y"]), "loss": abs(float(loss) - float(g["loss"])) / float(g["loss"]), "dx": rel_mse(dx, g["dx"]), "dobjs": rel_mse(dobjs, g["dobjs"])}
    names = sorted(k[5:] for k in g.files if k.startswith("grad."))
    assert names == sorted(grads.keys()) and len(names) == 17
    for n in names:
        ref = torch.from_numpy(g["grad." + n].astype(np.float32)) * float(g["scale." + n])
        report["grad." + n] = rel_mse(grads[n], ref)
    return report, dict(g=g, meta=meta, sd=sd, x=x, objs=objs, context=context, target=target)


def resblock_train_report(engine, name):
    """gl_op_resblock_train on tests/golden/<name>.npz -> (report, case)"""
    g, meta = _npz(name)
    x, emb, target = resblock_backward_inputs(meta)
    assert abs(float(x.double().sum()) - float(g["x_sum"])) < 1e-6
    sd = syn.seeded_state_dict({k: tuple(v) for k, v in golden_shapes(name).items()}, meta["seed"])
    assert set(sd.keys()) <= set(engine.resblock_train_param_names())
    y, loss, dx = engine.op_resblock_train(sd, x, emb, target)
    report = {"y": rel_mse(y, g["y"]), "loss": abs(float(loss) - float(g["loss"])) / float(g["loss"]), "dx": rel_mse(dx, g["dx"])}
    return report, dict(meta=meta, sd=sd, x=x, emb=emb, target=target)


def resample_train_report(engine, mode):
    """gl_op_resample_train ("down" / "up") on tests/golden/resample_backward.npz -> report"""
    g, meta = _npz("resample_backward")
    B, hw, Cc = meta["B"], meta["hw"], meta["C"]
    gen = torch.Generator().manual_seed(4545)
    for key, ho in (("down", hw // 2), ("up", hw * 2)):      # the generator order of the golden: down's x, target, then up's
        x = torch.randn(B, Cc, hw, hw, generator=gen)
        target = torch.randn(B, Cc, ho, ho, generator=gen)
        if key == mode:
            break
    assert abs(float(x.double().sum()) - float(g[mode + "_x_sum"])) < 1e-6
    sd = syn.seeded_state_dict({"op.weight" if mode == "down" else "conv.weight": (Cc, Cc, 3, 3), "op.bias" if mode == "down" else "conv.bias": (Cc,)}, meta["seed"])
    w = sd["op.weight" if mode == "down" else "conv.weight"]
    b = sd["op.bias" if mode == "down" else "conv.bias"]
    y, loss, dx = engine.op_resample_train(mode, w, b, x, target)
    return {"y": rel_mse(y, g[mode + "_y"]), "loss": abs(float(loss) - float(g[mode + "_loss"])) / float(g[mode + "_loss"]), "dx": rel_mse(dx, g[mode + "_dx"])}
