"""8-bit AdamW (SeerTrainer(use_8bit_adam=True), seer_adamw8_step) without a GPU: the code books, the block-aligned parameter
layout, and the trainer's wiring of the new mode through the plain-torch stand-ins (tests/adam8_ref.py: the format restated
independently of the product).  The kernel itself is tested on the GPU (tests/test_gpu_adam8.py)."""
import pytest
import torch

from seervideoldm_amd import FSTextTransformer, SeerUNet, synth, train_ops
from seervideoldm_amd.trainer import SeerTrainer, _pack_fstext_fp32, _pack_temporal_fp32, _Params
from tests import adam8_ref as R
from tests import torch_ops_backend as tob
from tests import torch_train_ops_backend as ttob

# the tiny trainer of tests/test_trainer_cpu.py
CFG = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=192, attention_head_dim=8)
FS = dict(num_frames=16, num_layers=1, channels=192, n_heads=2, cross_attention_dim=192)
HP = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=0.3)
TOPS8 = R.Adam8Tops()


def _models():
    unet = SeerUNet(**CFG)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG)), strict=True)
    fst = FSTextTransformer(num_frames=FS["num_frames"], in_channels=192, out_channels=192, n_heads=2, num_layers=1,
                            cross_attention_dim=192)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(**FS)), strict=True)
    fst.set_numframe(3)
    return unet, fst


@pytest.fixture(scope="module")
def models():
    return _models()


def _set_grads(tr, seed):
    """seeded gradients on the tensors only (the padding keeps its zero gradient, as after a backward pass)"""
    gen = torch.Generator().manual_seed(seed)
    for P in (tr.pu, tr.pf):
        P.g.zero_()
        for k in P.names:
            P.view(P.g, k).copy_(torch.randn(P.shapes[k], generator=gen) * 0.01)


def test_code_book_facts():
    qm, qv = train_ops.adam8_codebooks()
    for q in (qm, qv):
        assert q.dtype == torch.float32 and q.shape == (256,)
        assert torch.unique(q).numel() == 256 and bool((q[1:] > q[:-1]).all())          # 256 distinct values, ascending
    assert float(qm[127]) == 0.0 and float(qv[0]) == 0.0                                  # the zero codes
    assert train_ops.ADAM8_ZERO_CODES == (127, 0)
    assert float(qm[128]) == pytest.approx(5.5e-7, rel=1e-6) and float(qv[1]) == pytest.approx(3.25e-7, rel=1e-6)
    assert float(qm[126]) == -float(qm[128])
    assert float(qm[0]) == pytest.approx(-0.99296874, abs=1e-8) and float(qm[255]) == 1.0 and float(qv[255]) == 1.0
    # the product's books are the restated ones, bit for bit
    assert torch.equal(qm, R.QMAP_M) and torch.equal(qv, R.QMAP_V)


def test_params_alignment(models):
    unet, fst = models
    for packed in (_pack_temporal_fp32(dict(unet.state_dict())), _pack_fstext_fp32(dict(fst.state_dict()), fst.num_layers)):
        P8 = _Params(packed, "cpu")
        off, want = 0, {}
        for k, v in packed.items():                      # the layout before `align` existed: every tensor on a multiple of 8
            want[k] = off
            off += (v.numel() + 7) // 8 * 8
        assert P8.offsets == want and P8.n == off and P8.m is not None and P8.cm is None
        assert _Params(packed, "cpu", align=8).offsets == want
        P = _Params(packed, "cpu", align=256, adam8=True)
        assert P.n % 256 == 0 and all(o % 256 == 0 for o in P.offsets.values()) and list(P.offsets) == list(packed)
        assert P.m is None and P.v is None
        assert bool((P.cm == 127).all()) and bool((P.cv == 0).all()) and not P.absmax_m.any() and not P.absmax_v.any()
        assert P.cm.numel() == P.n and P.absmax_m.numel() == P.absmax_v.numel() == P.n // 256
        for k in P.names:
            assert torch.equal(P.view(P.p, k), P8.view(P8.p, k))
        assert int((P.p != 0).sum()) == int((P8.p != 0).sum())            # the padding is zero


def test_first_step_equals_the_fp32_mode(models):
    """the states start at zero and the update uses the unquantised moments: step 1 is the fp32 step (fp32 rounding: the stand-in
    of the fp32 mode uses torch's fused in-place forms)"""
    unet, fst = models
    tr8 = SeerTrainer(unet, fst, ops=tob, tops=TOPS8, use_8bit_adam=True, **HP)
    tr = SeerTrainer(unet, fst, ops=tob, tops=ttob, **HP)
    assert tr8.pu.adam8 and tr8.pu.m is None and tr8.pf.v is None and not tr.pu.adam8
    _set_grads(tr8, 5)
    _set_grads(tr, 5)
    tr8.optimizer_step()
    tr.optimizer_step()
    a, b = tr8.trainable_state_dict(), tr.trainable_state_dict()
    moved = 0.0
    for seg in ("unet", "fstext"):
        assert list(a[seg]) == list(b[seg])
        for k in a[seg]:
            assert (a[seg][k] - b[seg][k]).abs().max() <= 4 * R.U * b[seg][k].abs().max() + 1e-9, (seg, k)
    for P, P0 in ((tr8.pu, tr.pu), (tr8.pf, tr.pf)):
        assert torch.equal(P.pb, P.p.to(torch.bfloat16))
        moved += float((P0.p != 0).sum())
    assert moved > 0
    # the dequantised moments are the fp32 mode's within the code books' resolution, and the padding sits at the zero codes
    m8, m32 = tr8.optimizer_moments(), tr.optimizer_moments()
    u8, u32 = tr8.trainable_state_dict_of(m8["unet"][0], m8["fstext"][0]), tr.trainable_state_dict_of(m32["unet"][0], m32["fstext"][0])
    for seg in u8:
        for k in u8[seg]:
            assert (u8[seg][k] - u32[seg][k]).abs().max() <= 0.02 * u32[seg][k].abs().max(), (seg, k)
    for P in (tr8.pu, tr8.pf):
        pad = torch.ones(P.n, dtype=torch.bool)
        for k in P.names:
            o = P.offsets[k]
            pad[o:o + P.view(P.p, k).numel()] = False
        assert bool((P.cm[pad] == 127).all()) and bool((P.cv[pad] == 0).all()) and not P.p[pad].any()


def test_state_bytes(models):
    unet, fst = models
    tr8 = SeerTrainer(unet, fst, ops=tob, tops=TOPS8, use_8bit_adam=True, **HP)
    tr = SeerTrainer(unet, fst, ops=tob, tops=ttob, **HP)
    assert tr.optimizer_state_bytes() == 8 * (tr.pu.n + tr.pf.n)
    assert tr8.optimizer_state_bytes() == (tr8.pu.n + tr8.pf.n) * 2 + (tr8.pu.n + tr8.pf.n) // 256 * 8
    assert tr8.optimizer_state_bytes() <= 0.26 * tr.optimizer_state_bytes()      # (2 + 8/256) / 8 = 0.254 plus the block padding


def test_save_and_resume_bit_for_bit_and_across_modes(tmp_path):
    unet, fst = _models()
    tr = SeerTrainer(unet, fst, ops=tob, tops=TOPS8, use_8bit_adam=True, **HP)
    for s in (1, 2):
        _set_grads(tr, s)
        tr.optimizer_step()
    path = tr.save_state(str(tmp_path / "s8"), global_step=2)
    st = torch.load(str(tmp_path / "s8" / "optimizer.bin"), map_location="cpu")
    assert st["format"] == "adam8-block256" and st["step_count"] == 2
    assert set(st["unet"]) == {"cm", "cv", "absmax_m", "absmax_v"} and st["unet"]["cm"].dtype == torch.uint8
    # a fresh trainer on the saved weights continues exactly where this one does
    from seervideoldm_amd.io import load_seer_checkpoint
    u2, f2 = SeerUNet(**CFG), FSTextTransformer(num_frames=16, in_channels=192, out_channels=192, n_heads=2, num_layers=1,
                                                cross_attention_dim=192)
    load_seer_checkpoint(path, u2, f2)
    f2.set_numframe(3)
    tr2 = SeerTrainer(u2, f2, ops=tob, tops=TOPS8, use_8bit_adam=True, **HP)
    tr2.load_optimizer_state(path)
    assert tr2.step_count == 2
    for P, Q in ((tr.pu, tr2.pu), (tr.pf, tr2.pf)):
        assert torch.equal(P.p, Q.p) and all(torch.equal(a, b) for a, b in zip(P.state().values(), Q.state().values()))
    for t in (tr, tr2):
        _set_grads(t, 3)
        t.optimizer_step()
    for P, Q in ((tr.pu, tr2.pu), (tr.pf, tr2.pf)):
        assert torch.equal(P.p, Q.p) and torch.equal(P.pb, Q.pb)
        assert all(torch.equal(a, b) for a, b in zip(P.state().values(), Q.state().values()))
    # across modes: refused, both formats named
    tr32 = SeerTrainer(u2, f2, ops=tob, tops=ttob, **HP)
    with pytest.raises(ValueError, match="adam8-block256.*adam-fp32|adam-fp32.*adam8-block256"):
        tr32.load_optimizer_state(path)
    _set_grads(tr32, 4)
    tr32.optimizer_step()
    p32 = tr32.save_state(str(tmp_path / "s32"), global_step=1)
    assert "format" not in torch.load(str(tmp_path / "s32" / "optimizer.bin"), map_location="cpu")      # today's fp32 file
    with pytest.raises(ValueError, match="adam8-block256.*adam-fp32|adam-fp32.*adam8-block256"):
        tr2.load_optimizer_state(p32)
    tr32b = SeerTrainer(u2, f2, ops=tob, tops=ttob, **HP)
    tr32b.load_optimizer_state(p32)
    assert tr32b.step_count == 1 and torch.equal(tr32b.pu.m, tr32.pu.m) and torch.equal(tr32b.pf.v, tr32.pf.v)
    # the torch.optim.AdamW-format checkpoint holds fp32 moments: refused in 8-bit mode with a pointer to save_state
    from seervideoldm_amd import checkpoint
    with pytest.raises(ValueError, match="save_state"):
        checkpoint.optimizer_state_dict(tr2)


@pytest.mark.parametrize("step,mode", [(1, "clipped"), (7, "unclipped"), (7, "no_sumsq")])
def test_fp32_evaluation_stays_inside_the_float64_bounds(step, mode):
    """the bounds the GPU test asserts (tests/adam8_ref.py: step_f64, check_against_f64) hold for an fp32 evaluation of the same
    expressions on the CPU, on the GPU test's inputs: the bounds are about fp32 arithmetic, not about one implementation"""
    n = 256 * 1031
    p, g, cm, cv, am, av = R.random_state(n, 11)
    ss = None if mode == "no_sumsq" else (g.double() ** 2).sum().float().reshape(1)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, step=step, grad_sumsq=ss,
              max_norm=1e9 if mode == "unclipped" else 0.3)
    ref = R.step_f64(p, g, cm, cv, am, av, **kw)
    pb = torch.empty(n, dtype=torch.bfloat16)
    R.adamw8_step(p, g, cm, cv, am, av, p_bf16=pb, **kw)
    assert R.check_against_f64(ref, p, cm, cv, am, av, pb) == []
    # and the check has teeth: one code off by one entry, one scale off by 1e-5 relative
    cm2 = cm.clone()
    i = int((cm2 > 0).nonzero()[0])
    cm2[i] -= 1
    am2 = am.clone()
    am2[3] *= 1 + 1e-5
    what = [b[0] for b in R.check_against_f64(ref, p, cm2, cv, am2, av, pb)]
    assert "cm" in what and "absmax_m" in what
