"""CLIPTextEncoder -- host-side mirror of `transformers.CLIPTextModel` (the `text_encoder` of runwayml/stable-diffusion-v1-5) over
libseer_hip.so.

The module every Seer script runs between the tokenizer and everything else (train.py:330-334 inside every training step,
inference_img.py:147-161 and eval.py once per sample): prompt token ids `[b, L <= 77]` -> the text context `[b, L, 768]` that
`FSTextTransformer` and the UNet are conditioned on.  Same constructor keywords as `CLIPTextConfig`, same `state_dict()` keys as
the checkpoint (`text_model.…`; the un-prefixed spelling of transformers 5.x loads too), same call
`enc(input_ids, attention_mask)[0]` / `.last_hidden_state`.  There is NO `pooler_output`: no reference script reads it.

A 12-layer pre-LayerNorm transformer (width 768, 12 heads of 64, MLP 3072 with quick-GELU, eps 1e-5).  Per layer:
  layernorm -> ONE q|k|v GEMM (packed [3C, C], fused bias, col_scale on the q columns) -> seer_attn_causal64 (causal + key
  padding mask, one pass) -> out_proj GEMM + bias + residual in place -> layernorm -> fc1 GEMM with SEER_EPI_QUICKGELU -> fc2
  GEMM + bias + residual in place;
seer_embed_tokens in front, the final LayerNorm behind.  Activations are token-major bf16 [b*L, C], as in FSTextTransformer, whose
input this is.  Key j is visible to query i of sample b iff j <= i and attention_mask[b, j] != 0; a query without a visible key
(a mask that hides position 0) comes out of the attention as zeros -- transformers leaves that case undefined.  No CPU path.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import ops as hip_ops
from . import synth
from .unet import _build_tree

bf16 = torch.bfloat16
_PREFIX = "text_model."


class CLIPTextOutput:
    """what the scripts read of transformers' BaseModelOutputWithPooling: `out[0]` and `out.last_hidden_state`"""
    __slots__ = ("last_hidden_state",)

    def __init__(self, last_hidden_state: torch.Tensor):
        self.last_hidden_state = last_hidden_state

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]

    def __len__(self):
        return 1

    def __iter__(self):
        return iter((self.last_hidden_state,))


class CLIPTextEncoder(nn.Module):
    config_name = "config.json"

    def __init__(self, vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                 max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="quick_gelu", **ignored):
        super().__init__()
        if hidden_act != "quick_gelu":
            raise NotImplementedError(f"hidden_act={hidden_act!r}: the fc1 epilogue built is 'quick_gelu' (SEER_EPI_QUICKGELU), the "
                                      "activation of the SD-v1-5 text encoder")
        if hidden_size % num_attention_heads or hidden_size // num_attention_heads != 64:
            raise ValueError("head dim must be 64 (seer_attn_causal64): hidden_size // num_attention_heads = "
                             f"{hidden_size / num_attention_heads:g}")
        if hidden_size % 64 or intermediate_size % 64:
            raise ValueError("hidden_size and intermediate_size must be multiples of 64 (the GEMM's K step)")
        if max_position_embeddings > 128:
            raise ValueError("max_position_embeddings > 128: seer_attn_causal64 holds one sequence of up to 128 keys")
        self.vocab_size, self.hidden_size, self.intermediate_size = vocab_size, hidden_size, intermediate_size
        self.num_hidden_layers, self.num_attention_heads = num_hidden_layers, num_attention_heads
        self.max_position_embeddings, self.layer_norm_eps = max_position_embeddings, float(layer_norm_eps)
        _build_tree(self, synth.clip_text_param_shapes(vocab_size, hidden_size, intermediate_size, num_hidden_layers,
                                                       max_position_embeddings))
        self._w: Optional[Dict[str, torch.Tensor]] = None
        self._ops_backend = hip_ops    # tests may inject the plain-torch stand-in of tests/clip_oracle.py (CPU host-logic tests)

    # ---- checkpoints ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder: Optional[str] = None, **ignored):
        """A LOCAL directory (plus `subfolder`) holding config.json and model.safetensors or pytorch_model.bin.  Never contacts a
        hub: anything that is not an existing directory raises FileNotFoundError.  Other keywords (revision, torch_dtype, ...) are
        accepted and ignored."""
        path = os.fspath(pretrained_model_name_or_path)
        if subfolder:
            path = os.path.join(path, subfolder)
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path!r} is not an existing directory: CLIPTextEncoder.from_pretrained loads a local directory "
                                    "(config.json + model.safetensors or pytorch_model.bin) and never downloads")
        cfg_file = os.path.join(path, cls.config_name)
        if not os.path.isfile(cfg_file):
            raise FileNotFoundError(f"{cfg_file!r} not found")
        with open(cfg_file) as f:
            cfg = json.load(f)
        cfg = cfg.get("text_config") or cfg
        keys = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                "max_position_embeddings", "layer_norm_eps", "hidden_act")
        model = cls(**{k: cfg[k] for k in keys if k in cfg})
        st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
        if os.path.isfile(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        elif os.path.isfile(pt):
            sd = torch.load(pt, map_location="cpu", weights_only=True)
        else:
            raise FileNotFoundError(f"neither model.safetensors nor pytorch_model.bin in {path!r}")
        model.load_state_dict(sd, strict=True)
        return model

    def load_state_dict(self, state_dict, strict=True, **kw):
        """both key spellings load: `text_model.…` (the SD-v1-5 checkpoint, transformers 4.x) and the un-prefixed one of
        transformers 5.x; the `embeddings.position_ids` buffer is accepted and ignored"""
        sd = {}
        for k, v in state_dict.items():
            k = k if k.startswith(_PREFIX) else _PREFIX + k
            if k != _PREFIX + "embeddings.position_ids":
                sd[k] = v
        out = super().load_state_dict(sd, strict=strict, **kw)
        self._invalidate()
        return out

    def _apply(self, fn, *a, **k):
        self._invalidate()
        return super()._apply(fn, *a, **k)

    def _invalidate(self):
        self._w = None

    # ---- packed weights ------------------------------------------------------------------------------------------------
    def prepare(self):
        sd = {k[len(_PREFIX):]: v.detach() for k, v in self.state_dict().items()}
        dev = next(self.parameters()).device
        f32 = lambda t: t.to(dev, torch.float32).contiguous()
        b16 = lambda t: t.to(dev, torch.float32).to(bf16).contiguous()
        w: Dict[str, torch.Tensor] = {}
        w["tok"] = b16(sd["embeddings.token_embedding.weight"])
        w["pos"] = b16(sd["embeddings.position_embedding.weight"])
        for n in range(self.num_hidden_layers):
            p = f"encoder.layers.{n}"
            a = p + ".self_attn"
            w[a + ".qkv.w"] = b16(torch.cat([sd[a + ".q_proj.weight"], sd[a + ".k_proj.weight"], sd[a + ".v_proj.weight"]], 0))
            w[a + ".qkv.b"] = f32(torch.cat([sd[a + ".q_proj.bias"], sd[a + ".k_proj.bias"], sd[a + ".v_proj.bias"]], 0))
            w[a + ".out.w"], w[a + ".out.b"] = b16(sd[a + ".out_proj.weight"]), f32(sd[a + ".out_proj.bias"])
            for nm in ("fc1", "fc2"):
                w[f"{p}.{nm}.w"], w[f"{p}.{nm}.b"] = b16(sd[f"{p}.mlp.{nm}.weight"]), f32(sd[f"{p}.mlp.{nm}.bias"])
            for nm in ("layer_norm1", "layer_norm2"):
                w[f"{p}.{nm}.w"], w[f"{p}.{nm}.b"] = f32(sd[f"{p}.{nm}.weight"]), f32(sd[f"{p}.{nm}.bias"])
        w["norm.w"], w["norm.b"] = f32(sd["final_layer_norm.weight"]), f32(sd["final_layer_norm.bias"])
        self._w = w
        return self

    # ---- forward -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, **ignored) -> CLIPTextOutput:
        ops = self._ops_backend
        if input_ids.dim() != 2 or input_ids.dtype != torch.int64:
            raise TypeError("input_ids: expected an int64 tensor [batch, length]")
        b, L = input_ids.shape
        if not 1 <= L <= self.max_position_embeddings:
            raise ValueError(f"sequence length {L} outside 1..{self.max_position_embeddings}")
        if not input_ids.is_cuda and input_ids.numel():      # the tokenizer's output: checked here, without a device round trip
            lo, hi = int(input_ids.min()), int(input_ids.max())
            if lo < 0 or hi >= self.vocab_size:
                raise ValueError(f"input_ids outside [0, {self.vocab_size - 1}]: min {lo}, max {hi}")
        dev = next(self.parameters()).device
        if dev.type != "cuda" and ops is hip_ops:
            raise hip_ops._lib.SeerHipError("CLIPTextEncoder.forward needs the module on a ROCm device: the HIP kernels are the only "
                                            "compute path")
        if self._w is None:
            self.prepare()
        w = self._w
        C, heads, eps = self.hidden_size, self.num_attention_heads, self.layer_norm_eps
        ids = input_ids.to(dev).contiguous()
        mask = None
        if attention_mask is not None:
            if attention_mask.shape != (b, L):
                raise ValueError(f"attention_mask {tuple(attention_mask.shape)} next to input_ids {(b, L)}")
            mask = (attention_mask.to(dev) != 0).to(torch.uint8).contiguous()
        x = ops.embed_tokens(ids, w["tok"], w["pos"])          # [b*L, C] bf16
        a = torch.empty_like(x)
        qs = (ops.qk_prescale(64), C)
        for n in range(self.num_hidden_layers):
            p = f"encoder.layers.{n}"
            n1 = ops.layernorm(x, w[p + ".layer_norm1.w"], w[p + ".layer_norm1.b"], eps)
            qkv = ops.gemm(n1, w[p + ".self_attn.qkv.w"], bias=w[p + ".self_attn.qkv.b"], col_scale=qs)
            ops.attn_causal64(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], a, batch=b, heads=heads, L=L, key_mask=mask)
            ops.gemm(a, w[p + ".self_attn.out.w"], bias=w[p + ".self_attn.out.b"], residual=x, out=x)
            n2 = ops.layernorm(x, w[p + ".layer_norm2.w"], w[p + ".layer_norm2.b"], eps)
            h = ops.gemm(n2, w[p + ".fc1.w"], bias=w[p + ".fc1.b"], quick_gelu=True)
            ops.gemm(h, w[p + ".fc2.w"], bias=w[p + ".fc2.b"], residual=x, out=x)
        y = ops.layernorm(x, w["norm.w"], w["norm.b"], eps)
        return CLIPTextOutput(y.float().reshape(b, L, C))
