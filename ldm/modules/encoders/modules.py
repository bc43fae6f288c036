"""Text encoder front-end (reference ldm/modules/encoders/modules.py:144-173): CLIP ViT-L/14 text
tower, last_hidden_state (B,77,768). Weights come from the GLIGEN checkpoint (load_ckpt) and the tokenizer from
the local HF cache. backend="hf" (default) runs transformers' CLIPTextModel as the reference does;
backend="hip" runs the tower in the native engine (Engine::clip_text_encode) -- the HF module then only holds
the parameters."""
import torch
import torch.nn as nn

from gligen_amd import lora as _lora
from gligen_amd import runtime as _rt


class AbstractEncoder(nn.Module):
    def encode(self, *args, **kwargs):
        raise NotImplementedError


def eos_positions(input_ids, eos_token_id):
    """The position CLIPTextModel pools from, per row: the first argmax of the ids when eos_token_id == 2 (the legacy config
    real checkpoints were written with: EOS is the largest id of the vocabulary), else the first position equal to eos_token_id."""
    ids = torch.as_tensor(input_ids).to(torch.int64)
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == int(eos_token_id)).to(torch.int64).argmax(dim=-1)


class FrozenCLIPEmbedder(AbstractEncoder):
    """Uses the CLIP transformer encoder for text (from Hugging Face)."""

    def __init__(self, version="openai/clip-vit-large-patch14", device="cuda", max_length=77, backend="hf"):
        super().__init__()
        if backend not in ("hf", "hip"):
            raise ValueError(f"FrozenCLIPEmbedder backend must be 'hf' or 'hip', not {backend!r}")
        from transformers import CLIPTextConfig, CLIPTextModel, CLIPTokenizer
        try:
            self.tokenizer = CLIPTokenizer.from_pretrained(version)
            self.transformer = CLIPTextModel.from_pretrained(version)
        except Exception:  # offline: architecture from constants, weights arrive via load_state_dict
            self.tokenizer = None
            cfg = CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                                 num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=768)
            self.transformer = CLIPTextModel(cfg)
        self.device = device
        self.max_length = max_length
        self.backend = backend
        self._engine = None
        self.freeze()

    def _apply(self, fn, *a, **k):
        self._drop_engine()
        return super()._apply(fn, *a, **k)

    def _drop_engine(self):
        eng = self.__dict__.get("_engine")
        if eng is not None:
            eng.close()
        self.__dict__["_engine"] = None

    @property
    def engine(self):
        if self._engine is None:
            self._engine = _rt.build_clip_text_engine(self)
        return self._engine

    def load_state_dict(self, state_dict, strict=True, **kw):
        """GLIGEN checkpoints were written under transformers 4.x, whose CLIPTextModel wraps the tower in `.text_model`
        (keys `transformer.text_model.embeddings...`); transformers 5.x dropped that level (`transformer.embeddings...`). Keys are
        renamed to whatever the installed class uses, so an existing checkpoint loads unchanged under either version."""
        self._drop_engine()
        _lora.forget_loras(self)                  # new weights: the originals stashed under merged adapters are not this tower's any more
        own = self.state_dict().keys()
        wrapped_here = any(k.startswith("transformer.text_model.") for k in own)
        out = {}
        for k, v in state_dict.items():
            if k.endswith("position_ids") and k not in own:
                continue                          # a registered buffer in old versions only
            if wrapped_here and k.startswith("transformer.") and not k.startswith("transformer.text_model."):
                k = "transformer.text_model." + k[len("transformer."):]
            elif not wrapped_here and k.startswith("transformer.text_model."):
                k = "transformer." + k[len("transformer.text_model."):]
            out[k] = v
        return super().load_state_dict(out, strict=strict, **kw)

    def freeze(self):
        self.transformer = self.transformer.eval()
        for p in self.parameters():
            p.requires_grad = False

    @torch.no_grad()
    def encode_ids(self, input_ids, return_pooler_output=False):
        """Pre-tokenized input: ids [B, T] -> last_hidden_state [B, T, width] (and pooler_output [B, width]). backend="hip"
        encodes each DISTINCT row once and expands (the reference encodes [prompt] * B: B identical rows)."""
        input_ids = torch.as_tensor(input_ids)
        if self.backend == "hf":
            out = self.transformer(input_ids=input_ids.to(self.device))
            hidden, pooled = out.last_hidden_state, out.pooler_output
        else:
            ids = input_ids.detach().cpu().to(torch.int64)
            uniq, inverse = torch.unique(ids, dim=0, return_inverse=True)
            eos = eos_positions(uniq, getattr(self.transformer.config, "eos_token_id", 2))
            h, p = self.engine.clip_text_encode(uniq, eos)
            inverse = inverse.to(h.device)
            hidden, pooled = h[inverse], p[inverse]
        return (hidden, pooled) if return_pooler_output else hidden

    def forward(self, text, return_pooler_output=False):
        if self.tokenizer is None:
            raise RuntimeError("CLIP tokenizer files are not available offline; pass precomputed context embeddings instead")
        enc = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                             return_overflowing_tokens=False, padding="max_length", return_tensors="pt")
        if self.backend == "hip":
            return self.encode_ids(enc["input_ids"], return_pooler_output)
        out = self.transformer(input_ids=enc["input_ids"].to(self.device))
        if return_pooler_output:
            return out.last_hidden_state, out.pooler_output
        return out.last_hidden_state

    def encode(self, text, return_pooler_output=False):
        return self(text, return_pooler_output)
