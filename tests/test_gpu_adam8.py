"""seer_adamw8_step (8-bit AdamW: block-wise quantised moments) on a real MI355X: one step against the float64 emulation of
tests/adam8_ref.py with bounds counted from the fp32 roundings of the expressions, the edges of the format, and SeerTrainer in
8-bit mode on the HIP kernels against its fp32 mode."""
import functools
import json
from pathlib import Path

import pytest
import torch

from seervideoldm_amd import FSTextTransformer, SeerUNet, _lib, synth, train_ops
from seervideoldm_amd.trainer import SeerTrainer
from tests import adam8_ref as R

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
GUARD = 64                       # sentinel elements on either side of every output array (64 floats keep p 16-byte aligned)
SENT8 = 0xA5


def _guarded(t: torch.Tensor, device):
    """(the array on the device with sentinels around it, its inner view): NaN for the float types, 0xA5 for the codes"""
    full = torch.empty((t.numel() + 2 * GUARD,), dtype=t.dtype).fill_(SENT8 if t.dtype == torch.uint8 else float("nan"))
    full[GUARD:-GUARD] = t
    full = full.to(device)
    return full, full[GUARD:-GUARD]


def _sentinels_intact(full: torch.Tensor) -> bool:
    ends = torch.cat([full[:GUARD], full[-GUARD:]]).cpu()
    return bool((ends == SENT8).all()) if full.dtype == torch.uint8 else bool(torch.isnan(ends.float()).all())


@functools.lru_cache(maxsize=None)
def _case(n, step, mode):
    """inputs and the float64 reference of one (n, step, mode): computed once, shared by the cases with and without p_bf16"""
    inp = R.random_state(n, 1000 + n % 997 + step)
    ss = None if mode == "no_sumsq" else (inp[1].double() ** 2).sum().float().reshape(1)
    kw = dict(step=step, grad_sumsq=ss, max_norm=1e9 if mode == "unclipped" else 0.3, **HP)
    return inp, kw, R.step_f64(*inp, **kw)


def _run(device, inp, kw, with_bf16=True):
    """one launch on guarded copies; returns the CPU outputs (p, cm, cv, am, av, pb) and whether every sentinel survived"""
    p, g, cm, cv, am, av = inp
    fulls, views = zip(*[_guarded(t, device) for t in (p, cm, cv, am, av, torch.zeros(p.numel(), dtype=torch.bfloat16))])
    pv, cmv, cvv, amv, avv, pbv = views
    kw = dict(kw)
    if kw.get("grad_sumsq") is not None:
        kw["grad_sumsq"] = kw["grad_sumsq"].to(device)
    train_ops.adamw8_step(pv, g.to(device), cmv, cvv, amv, avv, p_bf16=pbv if with_bf16 else None, **kw)
    torch.cuda.synchronize()
    outs = [v.cpu() for v in views]
    if not with_bf16:
        assert not outs[5].any(), "p_bf16 = NULL: nothing may be written there"
        outs[5] = None
    return outs, all(_sentinels_intact(f) for f in fulls)


@pytest.mark.parametrize("with_bf16", [True, False])
@pytest.mark.parametrize("mode", ["clipped", "no_sumsq"])
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", [256, 512, 256 * 1031])
def test_one_step_against_float64(device, n, step, mode, with_bf16):
    """One step from a random valid state (codes uniform over 0..255, scales log-uniform in [1e-12, 1e3]) against the float64
    emulation; n = 256 * 1031 is an odd number of blocks (the last trip of the grid-stride loop is partial: 1031 = 4 * 257 + 3).  No
    element is excluded.  The bounds are counts of fp32 roundings times 2^-24 times the sum of the term magnitudes, derived in
    tests/adam8_ref.py:
      m: 9 U (|b1 m0| + |(1-b1) g'|),  v: 13 U (b2 v0 + (1-b2) g'^2)   -> each new scale within the largest element bound of its block
      code c: |qmap[c] absmax' - x64| <= min_k |qmap[k] absmax' - x64| + 2 bound_x + 3 U absmax'
      p: U (4 |A| + 14 |B|) + (lr/bc1)/denom * bound_m;  p_bf16: that + 2^-8 |p|
    tests/test_adam8_cpu.py holds an fp32 evaluation on the CPU to the same bounds on inputs of this generator."""
    inp, kw, ref = _case(n, step, mode)
    (p, cm, cv, am, av, pb), intact = _run(device, inp, kw, with_bf16)
    bad = R.check_against_f64(ref, p, cm, cv, am, av, pb)
    print(f"adamw8 n{n} step{step} {mode} bf16={with_bf16}: violations {bad}")
    assert bad == []
    assert intact, "a sentinel around an output array was overwritten"


def test_clip_coefficient_is_capped_at_one(device):
    """a gradient norm below max_norm: the coefficient is min(1, .) = 1, the step equals the one without grad_sumsq bit for bit"""
    inp, kw, _ = _case(512, 7, "unclipped")
    a, _ = _run(device, inp, kw)
    b, _ = _run(device, inp, dict(kw, grad_sumsq=None))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def _fresh(n):
    return (torch.full((n,), 127, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8), torch.zeros(n // 256), torch.zeros(n // 256))


def test_zero_gradient_on_a_fresh_state(device):
    n = 256 * 5
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(1))
    (p, cm, cv, am, av, pb), intact = _run(device, (p0, torch.zeros(n), *_fresh(n)), dict(step=1, grad_sumsq=None, **HP))
    assert bool((cm == 127).all()) and bool((cv == 0).all()) and not am.any() and not av.any() and intact
    h = R.hyper(step=1, lr=HP["lr"], betas=HP["betas"], eps=HP["eps"], weight_decay=HP["weight_decay"])
    want = p0.double() * (1.0 - h["lr"] * h["wd"])                  # p only decays: lr*wd, 1 - ., and the product round (3 U |p|)
    assert bool(((p.double() - want).abs() <= 3 * R.U * p0.double().abs()).all()) and torch.equal(pb, p.to(torch.bfloat16))


def test_zero_codes_and_end_codes(device):
    """From a fresh state m = (1-b1) g and v = (1-b2) g^2, so the ratios to the block maximum are those of g and g^2.
    Block 0: one element g = +1, the rest +-1e-7: m / absmax = 1e-7 and v / absmax = 1e-14 land on the zero codes (127, 0); the
    element at +absmax gets 255 in both books.  Block 1: one element g = -1 (code 0 signed: the lowest entry, -0.993, is the nearest
    to -1; 255 unsigned), the rest sqrt(1e-7): v / absmax = 1e-7 lands on the zero code, m / absmax = 3.2e-4 does not.
    (1e-7 sits under 3e-7 and under both books' own thresholds: half their smallest positive entries, 2.75e-7 signed and
    1.625e-7 unsigned.)"""
    n = 512
    g = torch.empty(n)
    sign = torch.where(torch.arange(256) % 2 == 0, 1.0, -1.0)
    g[:256] = 1e-7 * sign
    g[256:] = 1e-7 ** 0.5 * sign
    g[5], g[256 + 77] = 1.0, -1.0
    (p, cm, cv, am, av, _), intact = _run(device, (torch.zeros(n), g, *_fresh(n)), dict(step=1, grad_sumsq=None, **HP))
    b1, b2 = torch.tensor(HP["betas"][0]), torch.tensor(HP["betas"][1])
    assert torch.equal(am, ((1 - b1) * torch.ones(2))) and torch.equal(av, ((1 - b2) * torch.ones(2))) and intact
    rest0 = torch.arange(256) != 5
    assert int(cm[5]) == 255 and int(cv[5]) == 255 and bool((cm[:256][rest0] == 127).all()) and bool((cv[:256][rest0] == 0).all())
    rest1 = torch.arange(256) != 77
    assert int(cm[256 + 77]) == 0 and int(cv[256 + 77]) == 255
    assert bool((cv[256:][rest1] == 0).all()) and not bool((cm[256:][rest1] == 127).any())


def test_blocks_are_independent_and_a_nonfinite_gradient_stays_in_its_block(device):
    """changing g inside block j changes no byte of any other block's p, p_bf16, codes or scales; a NaN / an infinite gradient in a
    block leaves that block's codes and scales defined (finite scales) and every other block as it was"""
    nb, j = 9, 4
    inp = R.random_state(256 * nb, 77)
    kw = dict(step=3, grad_sumsq=torch.tensor([2.5]), max_norm=0.3, **HP)          # the same clip coefficient in every run
    base, _ = _run(device, inp, kw)
    for what in ("other", "nan", "inf"):
        g2 = inp[1].clone()
        if what == "other":
            g2[256 * j:256 * (j + 1)] = torch.randn(256, generator=torch.Generator().manual_seed(3))
        else:
            g2[256 * j + 17] = float("nan") if what == "nan" else float("-inf")
        out, intact = _run(device, (inp[0], g2, *inp[2:]), kw)
        assert intact
        for name, a, b in zip(("p", "cm", "cv", "am", "av", "pb"), base, out):
            per = 1 if name in ("am", "av") else 256
            keep = torch.ones(a.numel(), dtype=torch.bool)
            keep[per * j:per * (j + 1)] = False
            ab, bb = a.view(torch.uint8) if a.dtype == torch.uint8 else a, b.view(torch.uint8) if b.dtype == torch.uint8 else b
            assert torch.equal(ab[keep], bb[keep]), (what, name)
        assert not torch.equal(base[0][256 * j:256 * (j + 1)], out[0][256 * j:256 * (j + 1)])
        assert bool(torch.isfinite(out[3]).all()) and bool(torch.isfinite(out[4]).all()), what
        if what != "other":         # the rest of the struck block is still quantised against the finite maximum
            ok = torch.arange(256) != 17
            blk = slice(256 * j, 256 * (j + 1))
            ref = R.step_f64(inp[0], torch.where(torch.isfinite(g2), g2, torch.zeros_like(g2)), *inp[2:], **kw)
            err = (R.QMAP_M.double()[out[1][blk].long()] * out[3][j].double() - ref["m"][blk]).abs()[ok]
            assert float(err.max()) <= 0.01 * float(out[3][j]), what           # (the books' largest gap is 0.0070)


def test_invalid_arguments_return_einval_without_launching(device):
    n = 512
    p, g = torch.ones(n + 4, device=device), torch.ones(n + 4, device=device)
    cm, cv = torch.full((n + 4,), 127, device=device, dtype=torch.uint8), torch.zeros(n + 4, device=device, dtype=torch.uint8)
    am, av = torch.zeros(2, device=device), torch.zeros(2, device=device)
    qm, qv = train_ops.adam8_qmaps(device)
    pb = torch.zeros(n + 4, device=device, dtype=torch.bfloat16)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ptrs = [t.data_ptr() for t in (p, g, cm, cv, am, av, qm, qv)]

    def call(ptrs=ptrs, n=n, step=1, pb=pb.data_ptr()):
        return lib.seer_adamw8_step(*ptrs, n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step, None, 1.0, pb, st)

    for i in range(8):                                                   # a NULL required pointer
        assert call(ptrs[:i] + [None] + ptrs[i + 1:]) == -22, i
    for bad_n in (0, -256, 300, 255):
        assert call(n=bad_n) == -22, bad_n
    for bad_step in (0, -1):
        assert call(step=bad_step) == -22
    for i, off in ((0, 4), (1, 8), (2, 1), (3, 2)):                      # p / g off 16 bytes, cm / cv off 4 bytes
        assert call(ptrs[:i] + [ptrs[i] + off] + ptrs[i + 1:]) == -22, (i, off)
    assert call(pb=pb.data_ptr() + 2) == -22
    torch.cuda.synchronize()
    assert bool((p == 1).all()) and bool((cm == 127).all()) and not cv.any() and not am.any() and not av.any() and not pb.any()
    assert call() == 0                                                   # and the same arguments, valid, do launch
    torch.cuda.synchronize()
    assert not bool((p[:n] == 1).any()) and bool((p[n:] == 1).all()) and float(am[0]) > 0


# ------------------------------------------------------------------------------------------------------------- the trainer
def _tiny(device):
    unet = SeerUNet(**R.TINY_CFG).to(device)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(R.TINY_CFG), device=device), strict=True)
    fst = FSTextTransformer(num_frames=16, in_channels=192, out_channels=192, n_heads=2, num_layers=1, cross_attention_dim=192).to(device)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(num_frames=16, num_layers=1, channels=192, n_heads=2,
                                                                         cross_attention_dim=192), device=device), strict=True)
    fst.set_numframe(3)
    return unet, fst


def test_trainer_8bit_against_fp32_mode(device):
    """The tiny configuration of tests/test_gpu_train.py (width 320, 3 frames, 16x16 latent), 8 steps on one fixed batch, in both modes.
    Step 1: the states start at zero and the update takes the unquantised moments, so the parameters agree within fp32 rounding: per
    kernel 4 U |p| + 23 U lr against float64 (tests/adam8_ref.py's bound_p at step 1, where |B| <= lr and (lr/bc1)/denom * bound_m =
    9 U lr), twice that between the two kernels.
    Steps 1..8: the relative L2 distance between the two modes' parameter movement, asserted against 3x the same quantity of the CPU
    emulation on the plain-torch stand-ins (tests/golden/adam8_movement_cpu.json, `python -m tests.adam8_ref`; the factor covers the
    bf16 forward / backward noise).  Figures: profiles/adam8.md."""
    x, noise, t, text = [a.to(device) for a in R.tiny_batch(16)]
    res = {}
    for mode in (False, True):
        tr = SeerTrainer(*_tiny(device), use_8bit_adam=mode, **R.TINY_HP)
        res["p0"] = R.flat_params(tr)
        for s in range(8):
            tr.forward_backward(x, noise, t, text, 1)
            tr.optimizer_step()
            if s == 0:
                res[(mode, 1)] = R.flat_params(tr)
        res[(mode, 8)] = R.flat_params(tr)
        if mode:
            assert tr.pu.m is None and tr.pu.cm.dtype == torch.uint8
            assert tr.optimizer_state_bytes() == (tr.pu.n + tr.pf.n) * 2 + (tr.pu.n + tr.pf.n) // 256 * 8
    tol = 2 * (4 * R.U * res["p0"].abs() + 23 * R.U * R.TINY_HP["lr"])
    assert bool(((res[(True, 1)] - res[(False, 1)]).abs() <= tol).all())
    assert float((res[(False, 1)] - res["p0"]).abs().max()) > 0.5 * R.TINY_HP["lr"]
    d_gpu = R.movement_distance(res["p0"], res[(False, 8)], res[(True, 8)])
    d_cpu = json.loads((Path(__file__).parent / "golden" / R.GOLDEN_MOVEMENT).read_text())["H16_steps8"]
    print(f"[adam8 movement] 8 steps, relative L2 distance 8-bit vs fp32 mode: MI355X {d_gpu:.4g}, CPU emulation {d_cpu:.4g}")
    assert d_gpu <= 3 * d_cpu, (d_gpu, d_cpu)


def test_trainer_8bit_save_and_resume_bit_for_bit(device, tmp_path):
    from seervideoldm_amd.io import load_seer_checkpoint
    x, noise, t, text = [a.to(device) for a in R.tiny_batch(16)]
    tr = SeerTrainer(*_tiny(device), use_8bit_adam=True, **R.TINY_HP)
    for _ in range(2):
        tr.forward_backward(x, noise, t, text, 1)
        tr.optimizer_step()
    path = tr.save_state(str(tmp_path / "s8"), global_step=2)
    u2 = SeerUNet(**R.TINY_CFG)
    f2 = FSTextTransformer(num_frames=16, in_channels=192, out_channels=192, n_heads=2, num_layers=1, cross_attention_dim=192)
    load_seer_checkpoint(path, u2, f2)
    f2.set_numframe(3)
    tr2 = SeerTrainer(u2.to(device), f2.to(device), use_8bit_adam=True, **R.TINY_HP)
    tr2.load_optimizer_state(path)
    for a in (tr, tr2):
        a.forward_backward(x, noise, t, text, 1)
        a.optimizer_step()
    assert tr2.step_count == 3
    for P, Q in ((tr.pu, tr2.pu), (tr.pf, tr2.pf)):
        assert torch.equal(P.p, Q.p) and torch.equal(P.pb, Q.pb)
        assert all(torch.equal(a, b) for a, b in zip(P.state().values(), Q.state().values()))
    with pytest.raises(ValueError, match="adam8-block256"):
        SeerTrainer(u2, f2, **R.TINY_HP).load_optimizer_state(path)
