"""CLIPTextEncoder on a real MI355X: the three new kernels against their fp32 formulas on their own inputs, and the whole encoder
against the fp32 restatement of transformers' CLIPTextModel (tests/clip_oracle.py), tiny (the transformers-made fixture) and at
the size of the SD-v1-5 text encoder.

Whole-encoder bound: 2 x the rel-L2 error of the oracle's bf16-storage emulation against the fp32 oracle ON THE SAME INPUTS,
measured in the test (the kernels' summation order and the bf16 P differ from the emulation; FSTextTransformer's 2e-2 / 3e-2 have
the same ratio to their emulation).  Measured on MI355X (rel-L2 against fp32):
    tiny fixture   emulation 5.83e-3   GPU 6.03e-3   bound 1.17e-2
    full size      emulation 7.69e-3   GPU 7.82e-3   bound 1.54e-2     (mask against no mask: 0.16)
"""
import numpy as np
import pytest
import torch

from seervideoldm_amd import CLIPTextEncoder, _lib, ops
from tests import clip_oracle as CO
from tests.make_clip_golden import CFG
from tests.test_clip_text import G
from tests.test_gpu_kernels import _close, _rand

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------- kernel (a)
def _mask(kind, batch, L):
    if kind == "null":
        return None
    m = torch.ones((batch, L), dtype=torch.uint8)
    if kind == "len1":
        m[:, 1:] = 0
    elif kind == "len20":
        m[:, 20:] = 0
    elif kind == "holes":
        m[:, 5:9] = 0
        m[0, L // 2] = 0
    elif kind == "zero":                       # sample 1 sees nothing at all; sample 0 hides key 0: its query 0 sees nothing either
        m[1] = 0
        m[0, 0] = 0
    return m


@pytest.mark.parametrize("kind", ["null", "ones", "len1", "len20", "holes", "zero"])
@pytest.mark.parametrize("L", [1, 16, 17, 77, 128])
def test_attn_causal64(device, L, kind):
    """tile edges: one row, exactly one 16-query tile, one past, CLIP's own length, the maximum; q / k / v are the column slices of
    one fused projection, q prescaled; the bound is the generic attention cases' of tests/test_gpu_kernels.py (P is rounded to
    bf16 in the same way)"""
    batch, heads = 2, 2
    C = heads * 64
    qkv = _rand((batch * L, 3 * C), device, 100 + L).to(bf16)
    qkv[:, :C] = (qkv[:, :C].float() * ops.qk_prescale(64)).to(bf16)
    mask = _mask(kind, batch, L)
    out = torch.full((batch * L, C), float("nan"), device=device, dtype=bf16)
    ops.attn_causal64(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, batch=batch, heads=heads, L=L,
                      key_mask=None if mask is None else mask.to(device))
    c = qkv.cpu()
    ref = CO.attn_causal64_ref(c[:, :C], c[:, C:2 * C], c[:, 2 * C:], batch=batch, heads=heads, L=L, key_mask=mask, round_p=False)
    _close(out.cpu(), ref, rtol=2e-2, atol=1e-2, what=f"attn_causal64 L{L} {kind}")
    if kind == "zero":
        o = out.cpu().float().reshape(batch, L, C)
        assert torch.isfinite(o).all() and bool((o[1] == 0).all()) and bool((o[0, 0] == 0).all())
        if L > 1:
            assert bool((o[0, 1:].abs().sum(-1) > 0).all())       # the rows that do see a key are not zeroed with them


def test_attn_causal64_wide_rows_and_many_heads(device):
    """the fused projection may be wider than 3 * heads * 64 and the output wider than heads * 64; 12 heads as in CLIP"""
    batch, heads, L = 3, 12, 77
    C = heads * 64
    qkv = _rand((batch * L, 3 * C + 64), device, 7).to(bf16)
    qkv[:, :C] = (qkv[:, :C].float() * ops.qk_prescale(64)).to(bf16)
    mask = torch.ones((batch, L), dtype=torch.uint8)
    mask[0, 9:] = 0
    mask[2, 30:40] = 0
    out = torch.zeros((batch * L, C + 8), device=device, dtype=bf16)
    ops.attn_causal64(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:3 * C], out[:, :C], batch=batch, heads=heads, L=L, key_mask=mask.to(device))
    c = qkv.cpu()
    ref = CO.attn_causal64_ref(c[:, :C], c[:, C:2 * C], c[:, 2 * C:3 * C], batch=batch, heads=heads, L=L, key_mask=mask, round_p=False)
    _close(out[:, :C].cpu(), ref, rtol=2e-2, atol=1e-2, what="attn_causal64 12 heads")
    assert bool((out[:, C:] == 0).all())


# ------------------------------------------------------------------------------------------------------- kernel (b)
@pytest.mark.parametrize("C", [128, 768])
def test_embed_tokens_exact(device, C):
    vocab, L_max = 1000, 77
    tok, pos = _rand((vocab, C), device, 1).to(bf16), _rand((L_max, C), device, 2).to(bf16)
    for b, L in ((2, 77), (3, 5)):
        ids = torch.randint(0, vocab, (b, L), generator=torch.Generator().manual_seed(L))
        ids[0, 0], ids[-1, -1], ids[0, L // 2] = 0, vocab - 1, vocab - 1
        x = ops.embed_tokens(ids.to(device), tok, pos)
        ref = (tok.cpu()[ids].float() + pos.cpu()[:L].float()[None]).to(bf16).reshape(b * L, C)
        assert x.shape == (b * L, C) and torch.equal(x.cpu(), ref)
    wild = torch.tensor([[-3, vocab + 10, 5]])                  # device ids are clamped into the table, never read outside it
    got = ops.embed_tokens(wild.to(device), tok, pos).cpu()
    assert torch.equal(got, (tok.cpu()[wild.clamp(0, vocab - 1)].float() + pos.cpu()[:3].float()[None]).to(bf16).reshape(3, C))


# ------------------------------------------------------------------------------------------------------- flag (c)
@pytest.mark.parametrize("M,N", [(77, 128), (77, 3072), (154, 128), (154, 3072)])
def test_gemm_quick_gelu(device, M, N):
    """against the same product with an fp32 output, activated in torch.  Bound: the one bf16 rounding of the stored value,
    2^-8 relative (the fp32 paths differ by summation order and __expf, ~1e-6)"""
    K = 128
    a, w = _rand((M, K), device, 3).to(bf16), _rand((N, K), device, 4, K ** -0.5).to(bf16)
    bias = _rand((N,), device, 5, 0.5)
    v = ops.gemm(a, w, bias=bias, out_f32=True)
    ref = v * torch.sigmoid(1.702 * v)
    got = ops.gemm(a, w, bias=bias, quick_gelu=True)
    assert got.dtype == bf16
    _close(got, ref, rtol=2.0 ** -8, atol=1e-5, what=f"quick_gelu {M}x{N}")
    far = (got.float() - v).abs().max().item()
    assert far > 0.1                                              # the activation was applied (v itself is far from it)
    ws = ops.gemm(a, w, bias=bias, quick_gelu=True, tile=_lib.SEER_TILE_WS)       # not the weight-stationary kernel's: falls back
    _close(ws, ref, rtol=2.0 ** -8, atol=1e-5, what=f"quick_gelu {M}x{N} asked of the weight-stationary kernel")
    with pytest.raises(_lib.SeerHipError):
        ops.gemm(a, w, bias=bias, quick_gelu=True, silu=True)


# ------------------------------------------------------------------------------------------------------- whole encoder
def _golden():
    g = {k: torch.from_numpy(v) for k, v in np.load(G).items()}
    return {k: v.float() for k, v in g.items() if k.startswith("text_model.")}, g["ids"], g["mask"], g["out"]


def test_encoder_tiny_fixture(device):
    sd, ids, mask, out = _golden()
    m = CLIPTextEncoder(**CFG)
    m.load_state_dict(sd, strict=True)
    m.to(device)
    got = m(ids, attention_mask=mask)[0]                          # CPU ids, as the tokenizer hands them over
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == out.shape
    emu = CO.rel_l2(CO.clip_forward(sd, ids, mask, heads=2, storage=bf16), out)
    rel = CO.rel_l2(got.cpu(), out)
    print(f"CLIPTextEncoder tiny: bf16 emulation {emu:.3e}  GPU {rel:.3e}  bound {2 * emu:.3e}")
    assert rel < 2 * emu, (rel, emu)
    assert torch.equal(m(ids.to(device), attention_mask=mask.to(device))[0], got)       # device ids: the same bits


def _full_state_dict(seed=0):
    """the SD-v1-5 text encoder's shapes with transformers' initialisation scales (CLIPPreTrainedModel._init_weights) from a seeded
    generator, and non-trivial 1-D parameters"""
    from seervideoldm_amd import synth
    g = torch.Generator().manual_seed(seed)
    C, layers = 768, 12
    std = {"token_embedding": 0.02, "position_embedding": 0.02, "q_proj": C ** -0.5 * (2 * layers) ** -0.5,
           "k_proj": C ** -0.5 * (2 * layers) ** -0.5, "v_proj": C ** -0.5 * (2 * layers) ** -0.5, "out_proj": C ** -0.5,
           "fc1": (2 * C) ** -0.5, "fc2": C ** -0.5 * (2 * layers) ** -0.5}
    sd = {}
    for k, shape in synth.clip_text_param_shapes().items():
        if len(shape) == 2:
            sd[k] = torch.randn(shape, generator=g) * std[k.split(".")[-2]]
        else:
            sd[k] = 0.1 * torch.randn(shape, generator=g) + (1.0 if "norm" in k and k.endswith("weight") else 0.0)
    return sd


def test_encoder_full_size(device):
    sd = _full_state_dict()
    m = CLIPTextEncoder()
    m.load_state_dict(sd, strict=True)
    m.to(device)
    ids = torch.randint(0, 49408, (2, 77), generator=torch.Generator().manual_seed(1))
    mask = torch.ones((2, 77), dtype=torch.int64)
    mask[0, 9:] = 0                                               # one prompt padded to length 9, one unpadded
    got = m(ids, attention_mask=mask)[0].cpu()
    ref = CO.clip_forward(sd, ids, mask, heads=12)
    emu = CO.rel_l2(CO.clip_forward(sd, ids, mask, heads=12, storage=bf16), ref)
    rel = CO.rel_l2(got, ref)
    print(f"CLIPTextEncoder full size: bf16 emulation {emu:.3e}  GPU {rel:.3e}  bound {2 * emu:.3e}")
    assert got.shape == (2, 77, 768) and torch.isfinite(got).all()
    assert rel < 2 * emu, (rel, emu)
    nomask = m(ids)[0].cpu()
    diff = CO.rel_l2(nomask, got)
    print(f"CLIPTextEncoder full size: with mask vs without, rel-L2 {diff:.3f}")
    assert diff > 0.05                                            # a mask that is silently ignored


def test_encoder_reload_equals_fresh(device):
    sd, ids, mask, _ = _golden()
    sd2 = {k: (v * 1.25 if v.dim() == 2 else v + 0.05) for k, v in sd.items()}
    m = CLIPTextEncoder(**CFG)
    m.load_state_dict(sd, strict=True)
    m.to(device)
    y1 = m(ids, attention_mask=mask)[0]
    m.load_state_dict(sd2, strict=True)
    y2 = m(ids, attention_mask=mask)[0]
    fresh = CLIPTextEncoder(**CFG)
    fresh.load_state_dict(sd2, strict=True)
    fresh.to(device)
    assert torch.equal(y2, fresh(ids, attention_mask=mask)[0]) and not torch.equal(y1, y2)
