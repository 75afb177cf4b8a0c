"""CLIPTextEncoder without a GPU: the fp32 restatement of the tower (tests/clip_oracle.py) against transformers' own CLIPTextModel
(tests/golden/clip_text_tiny.npz, written by tests/make_clip_golden.py, and the installed module where it imports), the product's
kernel schedule through the plain-torch stand-in of the kernel library, checkpoint loading in both key spellings, the opt-in swap
of `transformers.CLIPTextModel`, and the refusals of the new entry points."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from seervideoldm_amd import CLIPTextEncoder, _lib, compat, synth
from seervideoldm_amd._lib import SeerHipError
from tests import clip_oracle as CO
from tests.make_clip_golden import CFG

ROOT = Path(__file__).resolve().parents[1]
G = Path(__file__).parent / "golden" / "clip_text_tiny.npz"
NEW = ("seer_attn_causal64", "seer_embed_tokens")


@pytest.fixture(scope="module")
def golden():
    g = {k: torch.from_numpy(v) for k, v in np.load(G).items()}
    sd = {k: v.float() for k, v in g.items() if k.startswith("text_model.")}
    return sd, g["ids"], g["mask"], g["out"]


def _encoder(sd, backend=None):
    m = CLIPTextEncoder(**CFG)
    m.load_state_dict(sd, strict=True)
    if backend is not None:
        m._ops_backend = backend
    return m


def test_oracle_matches_transformers_golden(golden):
    sd, ids, mask, out = golden
    assert set(sd) == set(synth.clip_text_param_shapes(CFG["vocab_size"], CFG["hidden_size"], CFG["intermediate_size"],
                                                       CFG["num_hidden_layers"], CFG["max_position_embeddings"]))
    assert [int(n) for n in mask.sum(1)] == [1, 2, 20, 77, 73] and bool((mask[:, 0] == 1).all())
    y = CO.clip_forward(sd, ids, mask, heads=CFG["num_attention_heads"])
    torch.testing.assert_close(y, out, rtol=1e-4, atol=2e-5)
    # the padding mask matters: a restatement (or a kernel) that ignores it is far away
    assert CO.rel_l2(CO.clip_forward(sd, ids, None, heads=2), out) > 0.05


def test_oracle_matches_live_transformers():
    tr = pytest.importorskip("transformers")
    torch.manual_seed(5)
    model = tr.CLIPTextModel(tr.CLIPTextConfig(**CFG)).eval()
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(0, CFG["vocab_size"], (3, 31), generator=g)
    mask = torch.ones((3, 31), dtype=torch.int64)
    mask[0, 7:] = 0
    mask[1, 3:6] = 0
    with torch.no_grad():
        ref = model(ids, attention_mask=mask)[0]
        ref_nomask = model(ids)[0]
    sd = model.state_dict()
    torch.testing.assert_close(CO.clip_forward(sd, ids, mask, heads=2), ref, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(CO.clip_forward(sd, ids, None, heads=2), ref_nomask, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("with_mask", [True, False])
def test_schedule_matches_oracle_cpu(golden, with_mask):
    """host logic (packing of q|k|v and its bias, col_scale on the q columns, mask conversion, in-place residual GEMMs) on the
    stand-in; the bound is the bf16-storage bound of the GPU test of the same fixture (tests/test_gpu_clip_text.py)"""
    sd, ids, mask, out = golden
    m = _encoder(sd, CO.ops_standin)
    res = m(ids, attention_mask=mask if with_mask else None)
    got = res[0]
    assert got is res.last_hidden_state and got.shape == out.shape and got.dtype == torch.float32
    ref = out if with_mask else CO.clip_forward(sd, ids, None, heads=2)
    emu = CO.rel_l2(CO.clip_forward(sd, ids, mask if with_mask else None, heads=2, storage=torch.bfloat16), ref)
    rel = CO.rel_l2(got, ref)
    print(f"tiny schedule on the stand-in: rel-L2 {rel:.3e}, bf16 emulation {emu:.3e}")
    assert rel < 2 * emu, (rel, emu)
    short = m(ids[:2, :9], attention_mask=mask[:2, :9])[0]               # L < 77: the position table is cut, not the output padded
    assert CO.rel_l2(short, CO.clip_forward(sd, ids[:2, :9], mask[:2, :9], heads=2)) < 2 * emu


def test_state_dict_both_spellings(golden):
    sd, ids, mask, _ = golden
    shapes = synth.clip_text_param_shapes(CFG["vocab_size"], CFG["hidden_size"], CFG["intermediate_size"], CFG["num_hidden_layers"],
                                          CFG["max_position_embeddings"])
    n_full = sum(int(np.prod(s)) for s in synth.clip_text_param_shapes().values())
    assert abs(n_full / 1e6 - 123.06) < 0.01                             # the SD-v1-5 text encoder
    a = _encoder(sd)
    assert list(a.state_dict()) == list(shapes) and all(tuple(v.shape) == shapes[k] for k, v in a.state_dict().items())
    bare = {k[len("text_model."):]: v for k, v in sd.items()}
    bare["embeddings.position_ids"] = torch.arange(77)[None]             # the buffer of transformers 5.x
    b = CLIPTextEncoder(**CFG)
    b.load_state_dict(bare, strict=True)
    pre = dict(sd)
    pre["text_model.embeddings.position_ids"] = torch.arange(77)[None]   # ... and of the checkpoint on disk
    c = CLIPTextEncoder(**CFG)
    c.load_state_dict(pre, strict=True)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]) and torch.equal(v, c.state_dict()[k]) and torch.equal(v, sd[k])
    with pytest.raises(RuntimeError):
        CLIPTextEncoder(**CFG).load_state_dict({k: v for k, v in sd.items() if "fc1.bias" not in k}, strict=True)
    # packed weights do not outlive a load
    a._ops_backend = CO.ops_standin
    y0 = a(ids[:1], mask[:1])[0]
    a.load_state_dict({k: v * 1.5 for k, v in sd.items()}, strict=True)
    assert a._w is None and not torch.equal(a(ids[:1], mask[:1])[0], y0)


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_from_pretrained_local_directory(golden, tmp_path, fmt):
    sd, ids, mask, _ = golden
    d = tmp_path / "sd15" / "text_encoder"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps(dict(CFG, architectures=["CLIPTextModel"], model_type="clip_text_model",
                                                   projection_dim=768, torch_dtype="float32")))
    if fmt == "safetensors":
        st = pytest.importorskip("safetensors.torch")
        st.save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    else:
        torch.save(sd, d / "pytorch_model.bin")
    m = CLIPTextEncoder.from_pretrained(str(tmp_path / "sd15"), subfolder="text_encoder", revision=None, torch_dtype=torch.float16)
    assert m.hidden_size == 128 and m.num_hidden_layers == 2
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k])
    with pytest.raises(FileNotFoundError, match="not an existing directory"):
        CLIPTextEncoder.from_pretrained("runwayml/stable-diffusion-v1-5", subfolder="text_encoder")
    with pytest.raises(FileNotFoundError, match="not an existing directory"):
        CLIPTextEncoder.from_pretrained(str(d / "config.json"))


def test_compat_swaps_clip_text_model(monkeypatch):
    tr = pytest.importorskip("transformers")
    own = tr.CLIPTextModel
    monkeypatch.delenv("SEER_COMPAT_CLIP", raising=False)
    try:
        compat.install()
        assert tr.CLIPTextModel is own                    # unset: nothing changes
        compat.install(clip="native")
        ns = {}
        exec("from transformers import CLIPTextModel, CLIPTokenizer", ns)                # train.py:21
        assert ns["CLIPTextModel"] is CLIPTextEncoder and tr.CLIPTextModel is CLIPTextEncoder
        compat.install(clip="native")                     # twice: the saved class stays transformers' own
        compat.uninstall()
        assert tr.CLIPTextModel is own
        monkeypatch.setenv("SEER_COMPAT_CLIP", "native")  # the runner's way
        compat.install()
        assert tr.CLIPTextModel is CLIPTextEncoder
    finally:
        compat.uninstall()
    assert tr.CLIPTextModel is own


def test_no_cpu_fallback_and_argument_errors(golden):
    sd, ids, mask, _ = golden
    m = _encoder(sd)
    with pytest.raises(SeerHipError):
        m(ids, attention_mask=mask)
    bad = ids.clone()
    bad[1, 3] = CFG["vocab_size"]
    with pytest.raises(ValueError):
        m(bad, attention_mask=mask)
    with pytest.raises(ValueError):
        _encoder(sd, CO.ops_standin)(-ids - 1)
    with pytest.raises(NotImplementedError, match="quick_gelu"):
        CLIPTextEncoder(**dict(CFG, hidden_act="gelu"))
    with pytest.raises(ValueError):
        CLIPTextEncoder(**dict(CFG, num_attention_heads=4))              # head dim 32


@pytest.fixture(scope="module")
def lib():
    from seervideoldm_amd.build import build_library
    build_library()
    return _lib.load()


def test_new_entry_points_refuse_bad_arguments_without_gpu(lib):
    P = 4096                                  # an aligned non-NULL pointer; none of these calls reaches a launch
    ok = dict(Q=P, K=P + 256, V=P + 512, ld=3 * 128, O=P, ldo=128, mask=None, batch=2, heads=2, L=77)

    def attn(**kw):
        a = dict(ok, **kw)
        return lib.seer_attn_causal64(a["Q"], a["K"], a["V"], a["ld"], a["O"], a["ldo"], a["mask"], a["batch"], a["heads"], a["L"], None)

    assert attn(Q=None) == -22 and attn(V=None) == -22 and attn(O=None) == -22
    assert attn(K=P + 2) == -22                                   # 16-byte alignment of the fused projection's slices
    assert attn(ld=120) == -22 and attn(ld=3 * 128 + 4) == -22    # stride below heads * 64 / off its multiple
    assert attn(ldo=64) == -22 and attn(ldo=130) == -22
    assert attn(L=0) == -22 and attn(batch=0) == -22 and attn(heads=0) == -22
    assert attn(L=129) == -38                                     # one-pass kernel: up to 128 keys are built
    emb = lambda ids=P, L=77, vocab=64, L_max=77, C=128, ldx=128, tok=P: \
        lib.seer_embed_tokens(ids, 2, L, tok, vocab, P, L_max, C, P, ldx, None)
    assert emb(ids=None) == -22 and emb(tok=P + 8) == -22
    assert emb(C=132) == -22 and emb(L=78) == -22 and emb(L=0) == -22 and emb(vocab=0) == -22 and emb(ldx=64) == -22
    # SEER_EPI_QUICKGELU: together with SEER_EPI_SILU it is refused before anything else is looked at
    d = _lib.GemmDesc()
    d.A = d.W = d.C = P
    d.M, d.N, d.K, d.K1, d.lda, d.ldc = 77, 128, 128, 128, 128, 128
    d.epilogue = _lib.SEER_EPI_QUICKGELU | _lib.SEER_EPI_SILU
    assert lib.seer_gemm_workspace_bytes(ctypes.byref(d)) == -22 and lib.seer_gemm_bf16(ctypes.byref(d), None) == -22
    d.epilogue = _lib.SEER_EPI_QUICKGELU
    assert lib.seer_gemm_workspace_bytes(ctypes.byref(d)) == 0
    d.ln_rowstat = d.ln_wsum = P
    assert lib.seer_gemm_lnfold_ok(ctypes.byref(d)) == 0          # as SILU: no folded LayerNorm in front of the activation


def test_new_symbols_are_declared_bound_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "seer_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(seer_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("seer_")}
    assert exported == declared == set(_lib.SIGNATURES)
    for n in NEW:
        assert n in declared and n in exported and n in _lib.SIGNATURES
    assert re.search(r"#define SEER_EPI_QUICKGELU 128u", header) and _lib.SEER_EPI_QUICKGELU == 128
    assert lib.seer_abi_version() == 27                   # no struct changed
