"""Masked sampling, stochastic_encode and decode on a real MI355X.  The three kernels of the given latents (include/seer_hip.h):
the seeded forms against the noise-tensor forms fed seer_philox_normal(seed, 2, index), with torch.equal; the noise-tensor forms
against float64 per element; the edges of the mask; the slot form against the single-clip kernel slot by slot; a chain of captured-form
steps; every refusal; the samplers on the mini UNet of tests/test_gpu_stoch.py under the layout-invariant mode; edit_clips.

Measured (profiles/edit_sampler.md): the largest |device - float64| over the cases of test 2 is 0.22 of its bound."""
import pytest
import torch

from seervideoldm_amd import (AutoencoderKL, DDIMSampler, FSTextTransformer, SeerUNet, SlotSampler, _lib, edit_clips, ops, synth)
from seervideoldm_amd.vae import ldm_to_diffusers_vae
from tests.test_edit_host import refusal_cases
from tests.test_gpu_slots import CFG_MINI, _model, _randn
from tests.test_gpu_stoch import ETA, F1, FL, HL, S_STEPS, SCALE, SEEDS, _coef, _inputs

pytestmark = pytest.mark.gpu

C, FP, B = 4, 3, 2
HWS = [(8, 12), (7, 5)]                                  # HW % 4 == 0, and 35: rows straddle the Philox blocks of four
NAN = float("nan")


def _case(device, hw, soft=True):
    h, w = hw
    x = _randn((B, C, FP, h, w), 2).to(device)
    known = _randn((B, C, FP, h, w), 3, 0.8).to(device)
    u = torch.rand((B, FP, h, w), generator=torch.Generator().manual_seed(4))
    mask = torch.where(u < 0.3, torch.zeros_like(u), torch.where(u > 0.7, torch.ones_like(u), u if soft else (u > 0.5).float()))
    return x, known, mask.to(device), ops.seed_words(SEEDS).to(device), C * FP * h * w


def _known_noise(seeds, index, per_clip, shape, device):
    return torch.stack([ops.philox_normal(s, ops.PHILOX_STREAM_KNOWN, index, per_clip, device) for s in seeds]).reshape(shape).contiguous()


# ---- 1. seeded against noise-tensor ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", HWS)
def test_seeded_forms_equal_the_noise_tensor_forms(device, hw):
    x, known, mask, seeds, per_clip = _case(device, hw)
    coef = _coef(device, 10, 0.0)[0]
    assert coef.shape[0] == 10
    other = ops.seed_words((SEEDS[0], SEEDS[0])).to(device)
    for index in (0, 5):
        noise = _known_noise(SEEDS, index, per_clip, x.shape, device)
        idx = torch.full((B,), index, dtype=torch.int32, device=device)
        want = ops.q_sample(known, coef, idx, noise=noise)
        got = ops.q_sample(known, coef, idx, seeds=seeds)
        assert torch.equal(got, want) and torch.isfinite(got).all(), index
        one = ops.q_sample(known[1:2].contiguous(), coef, idx[1:], seeds=seeds[1:2].contiguous())
        assert torch.equal(one, got[1:2]), index                       # row 1 of the b = 2 call is the b = 1 call with that seed
        diff = ops.q_sample(known, coef, idx, seeds=other)
        assert torch.equal(diff[0], got[0]) and not torch.equal(diff[1], got[1])
        want = ops.known_blend(x.clone(), mask, known, coef, index, noise=noise)
        got = ops.known_blend(x.clone(), mask, known, coef, index, seeds=seeds)
        assert torch.equal(got, want) and not torch.equal(got, x), index
        one = ops.known_blend(x[1:2].clone(), mask[1:2].contiguous(), known[1:2].contiguous(), coef, index, seeds=seeds[1:2].contiguous())
        assert torch.equal(one, got[1:2]), index
        diff = ops.known_blend(x.clone(), mask, known, coef, index, seeds=other)
        assert torch.equal(diff[0], got[0]) and not torch.equal(diff[1], got[1])
    # one index per row: rows 5 and 0 of the table
    idx = torch.tensor([5, 0], dtype=torch.int32, device=device)
    got = ops.q_sample(known, coef, idx, seeds=seeds)
    for bi, index in enumerate((5, 0)):
        row = ops.q_sample(known[bi:bi + 1].contiguous(), coef, idx[bi:bi + 1].contiguous(), seeds=seeds[bi:bi + 1].contiguous())
        assert torch.equal(got[bi:bi + 1], row)


# ---- 2. the noise-tensor forms against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", HWS)
def test_noise_tensor_forms_against_float64(device, hw):
    """|err| <= 2^-21 (|sqrt(a_t) x0| + |s1m n| + |x|) per element: at most eight fp32 roundings of half an ulp each (sqrtf, four
    products, 1 - m, two adds) on terms bounded by that sum, doubled for margin.  Measured maximum: 0.22 of the bound (hw 8 x 12; 0.20 at 7 x 5)."""
    x, known, mask, _, _ = _case(device, hw)
    coef = _coef(device, 10, 0.0)[0]
    noise = _randn(tuple(x.shape), 9).to(device)
    worst = 0.0
    for index in (0, 5, 9):
        a_t, s1m = float(coef[index, 0]), float(coef[index, 3])
        t1, t2 = a_t ** 0.5 * known.double().cpu(), s1m * noise.double().cpu()
        q = t1 + t2
        got = ops.q_sample(known, coef, torch.full((B,), index, dtype=torch.int32, device=device), noise=noise).double().cpu()
        ratio = ((got - q).abs() / (2.0 ** -21 * (t1.abs() + t2.abs()))).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, ("q_sample", index, ratio)
        m = mask.double().cpu()[:, None]
        xd = x.double().cpu()
        want = torch.where(m == 0, xd, torch.where(m == 1, q, q * m + (1.0 - m) * xd))
        got = ops.known_blend(x.clone(), mask, known, coef, index, noise=noise).double().cpu()
        ratio = ((got - want).abs() / (2.0 ** -21 * (t1.abs() + t2.abs() + xd.abs()))).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, ("known_blend", index, ratio)
    print(f"[edit] hw {hw}: max |device - float64| / bound = {worst:.3g}")


# ---- 3. the edges of the mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", HWS)
def test_mask_edges(device, hw):
    x, known, _, seeds, per_clip = _case(device, hw)
    h, w = hw
    coef = _coef(device, 10, 0.0)[0]
    q = ops.q_sample(known, coef, torch.full((B,), 5, dtype=torch.int32, device=device), seeds=seeds)
    bits = lambda t: t.view(torch.int32)
    # mask == 0: x keeps its bits (a -0.0 included) and `known` is not read into it (NaN sentinels)
    xs = x.clone()
    xs[0, 0, 0, 0, 0] = -0.0
    got = ops.known_blend(xs.clone(), torch.zeros((B, FP, h, w), device=device), torch.full_like(x, NAN), coef, 5, seeds=seeds)
    assert torch.equal(bits(got), bits(xs)) and bits(got)[0, 0, 0, 0, 0].item() == -(1 << 31)
    # mask == 1: q whatever x holds (NaN sentinels in x)
    got = ops.known_blend(torch.full_like(x, NAN), torch.ones((B, FP, h, w), device=device), known, coef, 5, seeds=seeds)
    assert torch.equal(got, q)
    # a mask that is 1 on one frame of one row touches that frame only, in every channel
    mask = torch.zeros((B, FP, h, w), device=device)
    mask[1, 2] = 1.0
    got = ops.known_blend(x.clone(), mask, known, coef, 5, seeds=seeds)
    want = x.clone()
    want[1, :, 2] = q[1, :, 2]
    assert torch.equal(got, want)
    # step non-NULL: index = step[0], both words stay; the host's index is then ignored
    mask = _case(device, hw)[2]
    want = ops.known_blend(x.clone(), mask, known, coef, 5, seeds=seeds)
    step = torch.tensor([5, 77], dtype=torch.int32, device=device)
    got = ops.known_blend(x.clone(), mask, known, coef, 0, step=step, seeds=seeds)
    assert torch.equal(got, want) and step.tolist() == [5, 77]
    noise = _known_noise(SEEDS, 5, per_clip, x.shape, device)
    assert torch.equal(ops.known_blend(x.clone(), mask, known, coef, 0, step=step, noise=noise), want)
    # index = -1 writes nothing, from the host and from the step word
    assert torch.equal(ops.known_blend(x.clone(), torch.ones_like(mask), torch.full_like(x, NAN), coef, -1, seeds=seeds), x)
    step = torch.tensor([-1, 3], dtype=torch.int32, device=device)
    assert torch.equal(ops.known_blend(x.clone(), torch.ones_like(mask), torch.full_like(x, NAN), coef, 4, step=step, seeds=seeds), x)
    assert step.tolist() == [-1, 3]
    # q_sample: a row whose index is outside the table is not written
    out = torch.full_like(x, NAN)
    ops.q_sample(known, coef, torch.tensor([10, 5], dtype=torch.int32, device=device), seeds=seeds, out=out)
    assert torch.isnan(out[0]).all() and torch.equal(out[1], q[1])


# ---- 4. the slot form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", HWS)
def test_slot_blend_equals_the_single_clip_kernel_slot_by_slot(device, hw):
    slots, nsched, (h, w) = 4, 16, hw
    lengths, index = (10, 4, 4, 10), (-1, 2, 3, 5)       # slot 0 is idle, slot 1 has an all-zero mask
    solo = [_coef(device, S, 0.0)[0] for S in lengths]
    coef = torch.zeros((slots, nsched, 4), device=device)
    coef[:, :, 0] = 1.0
    for s, t in enumerate(solo):
        coef[s, :t.shape[0]] = t
    seed_list = (5, 99, SEEDS[0], SEEDS[1])
    seeds = ops.seed_words(seed_list).to(device)
    x = _randn((slots, C, FP, h, w), 2).to(device)
    known = _randn((slots, C, FP, h, w), 3, 0.8).to(device)
    u = torch.rand((slots, FP, h, w), generator=torch.Generator().manual_seed(6))
    mask = torch.where(u < 0.3, torch.zeros_like(u), torch.where(u > 0.7, torch.ones_like(u), u)).to(device)
    mask[1] = 0.0
    known[0] = NAN                                       # idle and unmasked slots do not read their given latents
    known[1] = NAN
    step = torch.tensor([[i, 77] for i in index], dtype=torch.int32, device=device)
    got = x.clone()
    ops.slot_known_blend(got, mask, known, coef, step, seeds)
    assert step.tolist() == [[i, 77] for i in index]     # no step word is written
    assert torch.equal(got[0], x[0]) and torch.equal(got[1], x[1])
    for s in (2, 3):
        want = ops.known_blend(x[s:s + 1].clone(), mask[s:s + 1].contiguous(), known[s:s + 1].contiguous(), solo[s], index[s],
                               seeds=seeds[s:s + 1].contiguous())
        assert torch.equal(got[s:s + 1], want) and not torch.equal(want, x[s:s + 1]), s
    # an index past the slot's table: nothing is written
    step = torch.tensor([[nsched, 0]] * slots, dtype=torch.int32, device=device)
    got = x.clone()
    ops.slot_known_blend(got, torch.ones_like(mask), torch.full_like(x, NAN), coef, step, seeds)
    assert torch.equal(got, x)


# ---- 5. a chain of captured-form steps -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f1", [0, 2])
def test_a_chain_of_blend_and_rng_dev_steps_equals_the_host_index_kernels(device, f1):
    """known_blend(step) -> begin -> given eps -> seer_cfg_ddim_step_rng_dev, four times with no host write: every step is what the
    host-index kernels give, and the step words move as before"""
    b, h, w = 2, 7, 5
    coef, ttab = _coef(device, 4, 1.0)
    n = coef.shape[0]
    assert n == 4
    x = _randn((b, C, FP, h, w), 3).to(device)
    x0 = _randn((b, C, f1, h, w), 4).to(device) if f1 else None
    known = _randn((b, C, FP, h, w), 5, 0.8).to(device)
    mask = _case(device, (h, w))[2]
    seeds = ops.seed_words(SEEDS).to(device)
    pred = torch.empty_like(x)
    step = torch.tensor([n - 1, 99], dtype=torch.int32, device=device)
    sample = torch.empty((2 * b, C, f1 + FP, h, w), device=device)
    t_out = torch.empty((2 * b,), dtype=torch.long, device=device)
    ref = x.clone()
    for index in reversed(range(n)):
        eps = _randn((2 * b, C, f1 + FP, h, w), 100 + index).to(device)
        before = step.tolist()
        ops.known_blend(x, mask, known, coef, step=step, seeds=seeds)
        assert step.tolist() == before
        ops.ddim_step_begin(x0, x, ttab, step, 2, sample, t_out)
        ops.cfg_ddim_step_rng_dev(eps, x, coef, step, seeds, cfg=True, scale=3.0, cond_f=f1, temperature=0.7, x_prev=x, pred_x0=pred)
        assert step.tolist() == [index - 1, index]
        ops.known_blend(ref, mask, known, coef, index, seeds=seeds)
        assert torch.equal(sample[:b, :, f1:], ref)      # the UNet saw the blended latent
        ref, p = ops.cfg_ddim_step_rng(eps, ref, coef, index, seeds, cfg=True, scale=3.0, cond_f=f1, temperature=0.7)
        assert torch.equal(x, ref) and torch.equal(pred, p), index
    assert step.tolist() == [-1, 0] and torch.isfinite(x).all()
    # a fifth blend, past the schedule's end, writes nothing
    ops.known_blend(x, torch.ones_like(mask), torch.full_like(x, NAN), coef, step=step, seeds=seeds)
    assert torch.equal(x, ref)


# ---- 6. every refusal --------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_einval(device):
    buf = torch.zeros(1 << 18, device=device)
    lib = _lib.load()
    n = 0
    for fn, args, why in refusal_cases(buf.data_ptr()):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    assert n >= 30
    torch.cuda.synchronize()
    assert not buf.any()                                  # nothing ran
    x = torch.zeros((1, C, FP, 8, 8), device=device)
    with pytest.raises(ValueError):
        ops.known_blend(x, x[:, 0].contiguous(), x, _coef(device, 10, 0.0)[0], 10, seeds=ops.seed_words([1]).to(device))
    with pytest.raises(ValueError):
        ops.known_blend(x, x[:, 0].contiguous(), x, _coef(device, 10, 0.0)[0], 1)


# ---- 7. the samplers on the mini UNet ------------------------------------------------------------------------------------------------
_cache = {}


def _edit_model(device):
    """the mini UNet of tests/test_gpu_stoch.py as an instance of its own (a default spelled out makes another cache entry): the graphs
    captured here stay out of the graph caches that other test files count"""
    return _model(device, None, layout_invariant=True, downsample_padding=1)


def _edit_inputs(device):
    if "edit" not in _cache:
        mask = (torch.rand((1, 1, FL, HL, HL), generator=torch.Generator().manual_seed(8)) < 0.5).float()
        mask[0, 0, 0, :2] = 0.4                          # a soft band
        _cache["edit"] = dict(mask=mask.to(device), zero=torch.zeros((1, 1, FL, HL, HL), device=device),
                              known=_randn((1, 4, FL, HL, HL), 45, 0.8).to(device))
    return _cache["edit"]


def _sample(device, use_graph, seed, mask=None, known=None, sampler=None, **kw):
    m = _edit_model(device)
    i = _inputs(device)
    m.use_graph = use_graph
    try:
        return (sampler or DDIMSampler(device)).sample(
            m, S_STEPS, batch_size=1, shape=(4, FL, HL, HL), x0_emb=i["x0"], conditioning=i["c"], verbose=False, cond_frames=F1,
            unconditional_guidance_scale=SCALE, unconditional_conditioning=i["uc"], eta=kw.pop("eta", ETA), is_3d=True, seed=seed,
            mask=mask, x0=known, **kw)
    finally:
        m.use_graph = False


def _masked_solo(device):
    if "solo" not in _cache:
        e = _edit_inputs(device)
        _cache["solo"] = _sample(device, False, SEEDS[1], e["mask"], e["known"])[0]
    return _cache["solo"]


def test_seeded_masked_sample_captured_equals_launch_by_launch(device):
    e = _edit_inputs(device)
    want = _masked_solo(device)
    assert torch.isfinite(want).all() and want.shape == (1, 4, FL, HL, HL)
    state = torch.cuda.get_rng_state(device)
    got = _sample(device, True, SEEDS[1], e["mask"], e["known"])[0]
    assert torch.equal(torch.cuda.get_rng_state(device), state)         # nothing is drawn from torch's generator
    assert torch.equal(got, want)
    kinds = [k[0] for k in _edit_model(device)._engine._graphs if isinstance(k, tuple) and k]
    assert "step-mask" in kinds
    # a second call through the captured step, with other given latents: the static copies are refreshed
    other = _sample(device, True, SEEDS[1], e["mask"], e["known"] * 0.5)[0]
    assert torch.equal(other, _sample(device, False, SEEDS[1], e["mask"], e["known"] * 0.5)[0]) and not torch.equal(other, want)
    assert torch.equal(_sample(device, True, SEEDS[1], e["mask"], e["known"])[0], want)
    # eta = 0 with a seed and a mask takes the captured step too, and a given start code is left as it was
    xT = _inputs(device)["xT"].clone()
    a = _sample(device, True, SEEDS[1], e["mask"], e["known"], eta=0.0, x_T=xT)[0]
    assert torch.equal(xT, _inputs(device)["xT"])
    assert torch.equal(a, _sample(device, False, SEEDS[1], e["mask"], e["known"], eta=0.0, x_T=xT)[0])
    # the mask is in the result
    assert not torch.equal(want, _sample(device, False, SEEDS[1])[0])


@pytest.mark.parametrize("use_graph", [False, True])
def test_an_all_zero_mask_is_the_call_without_a_mask(device, use_graph):
    e = _edit_inputs(device)
    assert torch.equal(_sample(device, use_graph, SEEDS[1], e["zero"], e["known"])[0], _sample(device, use_graph, SEEDS[1])[0])


@pytest.mark.parametrize("use_graph", [False, True])
def test_decode_from_a_recorded_latent_returns_the_samples_result(device, use_graph):
    smp = DDIMSampler(device)
    final, inter = _sample(device, use_graph, SEEDS[1], sampler=smp, log_every_t=1)
    n = int(smp.ddim_coef.shape[0])
    assert n == S_STEPS and len(inter["x_inter"]) == n + 1 and torch.equal(inter["x_inter"][-1], final)
    m = _edit_model(device)
    i = _inputs(device)
    m.use_graph = use_graph
    try:
        for k in (1, 3):
            x_k = inter["x_inter"][n - k].clone()
            got = smp.decode(m, x_k, i["c"], k, SCALE, i["uc"], x0_emb=i["x0"], cond_frames=F1, seed=SEEDS[1])
            assert torch.equal(got, final), k
            assert torch.equal(x_k, inter["x_inter"][n - k])
    finally:
        m.use_graph = False


@pytest.mark.parametrize("use_graph", [False, True])
def test_a_masked_clip_in_a_slot_beside_a_plain_clip(device, use_graph):
    m = _edit_model(device)
    i, e = _inputs(device), _edit_inputs(device)
    want_plain = {}
    m.use_graph = use_graph
    try:
        for editing in (False, True):
            smp = SlotSampler(m, 2, shape=(4, FL, HL, HL), cond_frames=F1, context_shape=(77, CFG_MINI["cross_attention_dim"]), device=device,
                              model_cond_frame=F1, stochastic=True, **(dict(editing=True) if editing else {}))
            assert smp.submit(i["xT"], i["x0"], i["c2"], i["uc"], S_STEPS + 2, 3.0) == 0           # S = 6: seven entries
            done = smp.step()
            if editing:
                assert smp.submit(None, i["x0"], i["c"], i["uc"], S_STEPS, SCALE, eta=ETA, seed=SEEDS[1], mask=e["mask"], x0=e["known"]) == 1
            while smp.active():
                done += smp.step()
            want_plain[editing] = dict(done)[0]
            keys = [k[0] for k in m._engine._graphs if isinstance(k, tuple) and k]
            if use_graph:
                assert keys.count("slots-edit-rng" if editing else "slots-rng") == 1
    finally:
        m.use_graph = False
    assert [s for s, _ in done] == [1, 0] and not smp._mask.any()
    assert torch.equal(dict(done)[1], _masked_solo(device)), (dict(done)[1] - _masked_solo(device)).abs().max().item()
    assert torch.equal(want_plain[True], want_plain[False])


# ---- 8. edit_clips -------------------------------------------------------------------------------------------------------------------
def test_edit_clips_on_the_tiny_pipeline(device):
    unet_cfg = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=192, attention_head_dim=8)
    fst_cfg = dict(num_frames=6, num_layers=2, channels=192, n_heads=2, cross_attention_dim=192)
    vae_kw = dict(ch=128, ch_mult=(1, 1, 2, 2), num_res_blocks=1)
    unet = SeerUNet(**unet_cfg, layout_invariant=True)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(unet_cfg)), strict=True)
    fst = FSTextTransformer(num_frames=6, in_channels=192, out_channels=192, n_heads=2, num_layers=2, cross_attention_dim=192)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(**fst_cfg)), strict=True)
    vsd = {**synth.synth_state_dict(synth.vae_param_shapes(**vae_kw)),
           **synth.synth_state_dict(synth.vae_encoder_param_shapes(**vae_kw, z_channels=4))}
    vae = AutoencoderKL(block_out_channels=(128, 128, 256, 256), layers_per_block=1)
    vae.load_state_dict(ldm_to_diffusers_vae(vsd, 4), strict=True)
    unet, fst, vae = unet.to(device).eval(), fst.to(device).eval(), vae.to(device)
    video = torch.tanh(_randn((1, 3, 3, 64, 64), 50)).to(device)
    text, empty = _randn((1, 77, 192), 60).to(device), _randn((1, 77, 192), 3).to(device)
    keep = torch.zeros((1, 1, 2, 8, 8), device=device)
    keep[:, :, :, :, :4] = 1.0
    run = lambda seed, **kw: edit_clips(unet, fst, vae, DDIMSampler(device), video, text, empty, cond_frames=1, ddim_steps=4, seed=seed,
                                        latent_generator=torch.Generator(device=device).manual_seed(5), **kw)
    for kw in (dict(strength=0.5), dict(keep_mask=keep)):
        clip = run(11, **kw)
        assert clip.shape == (1, 3, 2, 64, 64) and torch.isfinite(clip).all() and clip.min() >= 0 and clip.max() <= 1
        assert torch.equal(run(11, **kw), clip)
        assert not torch.equal(run(12, **kw), clip)
