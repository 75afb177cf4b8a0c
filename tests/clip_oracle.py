"""The CLIP text tower (transformers CLIPTextModel: models/clip/modeling_clip.py) restated in plain fp32 torch, and a plain-torch
stand-in of the three kernels it added to the library: the CPU side of tests/test_clip_text.py and tests/test_gpu_clip_text.py.

Visibility: key j is visible to query i of sample b iff j <= i and attention_mask[b, j] != 0; softmax over the visible keys.
`storage=torch.bfloat16` rounds the weight matrices and every activation the product stores (embedding sum, LayerNorm outputs,
q|k|v, attention output, the residual stream after each add, the fc1 activation) with fp32 arithmetic in between: the
emulation the whole-encoder tolerances are calibrated on."""
import types

import torch

from tests import torch_ops_backend as tob

bf16 = torch.bfloat16
PREFIX = "text_model."


def _visible(L, mask):
    """[b or 1, L(query), L(key)] bool"""
    vis = torch.tril(torch.ones(L, L, dtype=torch.bool))[None]
    if mask is not None:
        vis = vis & (mask != 0)[:, None, :]
    return vis


def quick_gelu(v):
    return v * torch.sigmoid(1.702 * v)


def clip_forward(sd, ids, mask=None, *, heads, eps=1e-5, storage=None):
    """sd: CLIPTextModel state dict (with or without the `text_model.` prefix), ids int64 [b, L], mask [b, L] or None ->
    last_hidden_state fp32 [b, L, C]"""
    sd = {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v.float() for k, v in sd.items() if v.is_floating_point()}
    r = (lambda t: t.to(storage).float()) if storage is not None else (lambda t: t)
    W = lambda k: r(sd[k])                      # 2-D matrices are stored in `storage`; biases and LayerNorm parameters stay fp32
    ln = lambda x, p: torch.nn.functional.layer_norm(x, x.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], eps)
    b, L = ids.shape
    C = sd["embeddings.token_embedding.weight"].shape[1]
    d = C // heads
    vis = _visible(L, mask)
    x = r(W("embeddings.token_embedding.weight")[ids] + W("embeddings.position_embedding.weight")[:L][None])
    n = 0
    while f"encoder.layers.{n}.layer_norm1.weight" in sd:
        p = f"encoder.layers.{n}"
        h = r(ln(x, p + ".layer_norm1"))
        lin = lambda t, nm: t @ W(f"{p}.{nm}.weight").t() + sd[f"{p}.{nm}.bias"]
        q = r(lin(h, "self_attn.q_proj") * d ** -0.5).reshape(b, L, heads, d).transpose(1, 2)
        k = r(lin(h, "self_attn.k_proj")).reshape(b, L, heads, d).transpose(1, 2)
        v = r(lin(h, "self_attn.v_proj")).reshape(b, L, heads, d).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)).masked_fill(~vis[:, None], float("-inf"))
        a = r((torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(b, L, C))
        x = r(x + lin(a, "self_attn.out_proj"))
        h = r(ln(x, p + ".layer_norm2"))
        h = r(quick_gelu(lin(h, "mlp.fc1")))
        x = r(x + lin(h, "mlp.fc2"))
        n += 1
    return ln(x, "final_layer_norm")


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


# ---- plain-torch stand-in of the ops the encoder calls: tests/torch_ops_backend.py plus the three new ones -----------------------
def attn_causal64_ref(q, k, v, *, batch, heads, L, key_mask=None, round_p=True):
    """the contract of seer_attn_causal64 on its own inputs in fp32: q PRESCALED by scale * log2(e), exp2 of the raw dot products,
    (P rounded to bf16 for the PV product,) zeros for a query without a visible key.  Returns fp32 [batch*L, heads*64]."""
    f = lambda t: t[:, :heads * 64].float().reshape(batch, L, heads, 64).transpose(1, 2)
    qf, kf, vf = f(q), f(k), f(v)
    vis = _visible(L, key_mask)[:, None]
    s = (qf @ kf.transpose(-1, -2)).masked_fill(~vis, float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp2(s - m)
    l = p.sum(dim=-1, keepdim=True)
    if round_p:
        p = p.to(bf16).float()
    o = (p @ vf) * torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    return o.transpose(1, 2).reshape(batch * L, heads * 64)


def _attn_causal64(q, k, v, out, *, batch, heads, L, key_mask=None):
    out[:, :heads * 64] = attn_causal64_ref(q, k, v, batch=batch, heads=heads, L=L, key_mask=key_mask).to(out.dtype)
    return out


def _embed_tokens(ids, tok, pos, out=None):
    b, L = ids.shape
    x = (tok[ids.clamp(0, tok.shape[0] - 1)].float() + pos[:L].float()[None]).to(bf16).reshape(b * L, -1)
    if out is not None:
        out.copy_(x)
        return out
    return x


def _gemm(a, w, *, quick_gelu=False, bias=None, **kw):
    if not quick_gelu:
        return tob.gemm(a, w, bias=bias, **kw)
    assert not kw, "the quick-GELU launch of the encoder carries a bias and nothing else"
    return quick_gelu_fn(tob.gemm(a, w, bias=bias, out_f32=True)).to(bf16)


quick_gelu_fn = quick_gelu
ops_standin = types.SimpleNamespace(gemm=_gemm, layernorm=tob.layernorm, qk_prescale=tob.qk_prescale, attn_causal64=_attn_causal64,
                                    embed_tokens=_embed_tokens)
