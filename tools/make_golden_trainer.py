"""Generate tests/golden/trainable_order.json by RUNNING THE REFERENCE's UNetModel (read-only import, as oracle/make_golden.py does):
for the small text, small canny and small inpainting configs, the names of the reference's trainable parameters in the order
torch.optim.AdamW numbers them -- named_parameters() filtered as trainer.py:217-236 filters it (fuser.* inside transformer_blocks,
position_net, downsample_net, and input_blocks.0.0.weight when the first conv was widened: a grounding downsampler or inpaint_mode,
trainer.py:189-194). That order is the `params` numbering of a reference checkpoint's "opt"
(gligen_amd.train.TrainStep.torch_optimizer_state_dict). The file holds, per entry, the UNetModel kwargs the names were read
under, the names, and the number of named parameters; no tensor. Needs the reference checkout that oracle/make_golden.py reads
(REF there); no test imports this script:

    cd /tmp && python <repo>/tools/make_golden_trainer.py
"""
import importlib.util
import json
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gl_make_golden", os.path.join(REPO, "oracle", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)      # puts the reference first on sys.path and loads gligen_amd/synthetic.py by file path

import torch  # noqa: E402

from ldm.modules.diffusionmodules.openaimodel import UNetModel  # noqa: E402  (reference)

syn = mg.syn


def configs():
    small = dict(syn.UNET_CFG_SMALL, use_checkpoint=False)
    text = dict(small, grounding_tokenizer=syn.GROUNDING_TOKENIZERS["text"], inpaint_mode=False)
    canny = dict(small, inpaint_mode=False,
                 grounding_downsampler=dict(target="ldm.modules.diffusionmodules.canny_grounding_downsampler.GroundingDownsampler", params=dict(resize_input=64, out_dim=8)),
                 grounding_tokenizer=dict(target="ldm.modules.diffusionmodules.canny_grounding_net.PositionNet", params=dict(resize_input=128, out_dim=768)))
    return {"small_text": text, "small_canny": canny, "small_text_inpaint": dict(text, inpaint_mode=True)}


def reference_trainable(cfg):
    mg._timm_shim()
    real_hub = torch.hub.load_state_dict_from_url
    torch.hub.load_state_dict_from_url = lambda *a, **k: {"model": {}}   # pretrained=True would download ImageNet weights
    try:
        model = UNetModel(**cfg)
    finally:
        torch.hub.load_state_dict_from_url = real_hub
    additional_channels = model.additional_channel_from_downsampler + (5 if cfg["inpaint_mode"] else 0)      # trainer.py:190-192
    input_conv_train = additional_channels > 0                                                              # trainer.py:194
    names, every = [], []
    for name, _ in model.named_parameters():                                                                # trainer.py:220-242
        if ("transformer_blocks" in name) and ("fuser" in name):
            names.append(name)
        elif "position_net" in name:
            names.append(name)
        elif "downsample_net" in name:
            names.append(name)
        elif input_conv_train and ("input_blocks.0.0.weight" in name):
            names.append(name)
        every.append(name)
    return names, every, list(model.state_dict().keys())


if __name__ == "__main__":
    out = {}
    for key, cfg in configs().items():
        names, every, sd_keys = reference_trainable(cfg)
        out[key] = dict(cfg=cfg, n_parameters=len(every), parameters_equal_state_dict_keys=every == sd_keys, trainable=names)
        print(f"{key}: {len(every)} named parameters ({'=' if every == sd_keys else '!='} state_dict keys), {len(names)} trainable; first {names[0]}, last {names[-1]}")
    path = os.path.join(mg.OUT, "trainable_order.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")
