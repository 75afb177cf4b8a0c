"""Seeded stochastic DDIM on a real MI355X.  The generator against the Random123 vectors and the CPU restatement bit for bit, its
normals against float64; the three *_rng step kernels against the two-stage form -- seer_philox_normal into a noise tensor, then the
existing kernel -- with torch.equal; the samplers on the mini UNet under the layout-invariant mode: a seeded clip has the same bits
alone, as a row of a batch, in a slot beside another clip, captured or launch by launch."""
import numpy as np
import pytest
import torch

from seervideoldm_amd import (AutoencoderKL, DDIMSampler, FSTextTransformer, SeerUNet, SlotSampler, _lib, ops, synth)
from seervideoldm_amd.pipeline import generate_queue
from seervideoldm_amd.vae import ldm_to_diffusers_vae
from tests import stoch_ref
from tests.test_gpu_slots import CFG_MINI, _model, _randn
from tests.test_stoch_host import refusal_cases

pytestmark = pytest.mark.gpu

SEEDS = (1234, (7 << 32) | 5)                           # the second has a non-zero high word
C, FP = 4, 3
_tables = {}


def _coef(device, S, eta):
    if (S, eta) not in _tables:
        smp = DDIMSampler(device)
        smp.make_schedule(S, ddim_eta=eta, verbose=False)
        _tables[(S, eta)] = (smp.ddim_coef, smp._t_table)
    return _tables[(S, eta)]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1. the generator ------------------------------------------------------------------------------------------------------------
def test_philox_words_are_the_known_answers_and_the_restatement(device):
    for counter, key, want in stoch_ref.KAT:
        got = _u32(ops.philox_u32(key[0] | key[1] << 32, counter[2] | counter[3] << 32, counter[1], counter[0], 1, device))
        assert tuple(int(v) for v in got[0]) == want, [hex(int(v)) for v in got[0]]
    for seed, stream, index, first, n in ((SEEDS[0], 1, 3, (1 << 16) - 3, 8), (SEEDS[1], 1, 49, (1 << 32) - 6, 6),
                                          (SEEDS[1], 0, 0, 0, 1031)):
        got = _u32(ops.philox_u32(seed, stream, index, first, n, device))
        assert np.array_equal(got, stoch_ref.words(seed, stream, index, first, n)), (hex(seed), first)


def test_philox_normals_against_float64(device):
    """|device - float64| <= 2^-18 per element: logf and sincospif within 2 ulp and sqrtf within 1 give |dn| <= r (2^-22 + 2^-23) +
    2^-24 |n| < 2^-19 at r <= 5.77, doubled for margin.  Measured maximum over 2^20 numbers: 2^-20.7 (profiles/stoch_sampler.md)."""
    outs = {}
    for n in (1, 3, 1155, 4096):
        buf = torch.full((n + 9,), float("nan"), device=device)
        ops.philox_normal(SEEDS[1], 1, 5, n, out=buf)
        assert torch.isnan(buf[n:]).all(), n             # nothing past out[n - 1]
        outs[n] = buf[:n].cpu()
        err = np.abs(outs[n].numpy().astype(np.float64) - stoch_ref.normals64(SEEDS[1], 1, 5, n)).max()
        print(f"[stoch] philox_normal n = {n}: max |device - float64| = {err:.3g} = 2^{np.log2(max(err, 1e-300)):.2f}")
        assert torch.isfinite(outs[n]).all() and err <= 2.0 ** -18, (n, err)
    for n in (1, 3, 1155):
        assert torch.equal(outs[n], outs[4096][:n]), n   # a prefix is a prefix
    big = ops.philox_normal(SEEDS[0], 0, 0, 1 << 20, device).cpu().numpy().astype(np.float64)
    err = np.abs(big - stoch_ref.normals64(SEEDS[0], 0, 0, 1 << 20)).max()
    print(f"[stoch] philox_normal n = 2^20: max |device - float64| = {err:.3g} = 2^{np.log2(err):.2f}, max|n| {np.abs(big).max():.4f}")
    assert err <= 2.0 ** -18 and np.abs(big).max() <= 5.7683


# ---- 2. the step kernels -----------------------------------------------------------------------------------------------------------
def _noise(seeds, index, per_clip, shape, temperature, device):
    rows = [ops.philox_normal(s, ops.PHILOX_STREAM_STEP, index, per_clip, device) for s in seeds]
    return (torch.stack(rows).reshape(shape) * temperature).contiguous()


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("cond_f", [0, 2])
@pytest.mark.parametrize("hw", [(8, 12), (7, 5)])        # HW % 4 == 0, and 35: rows straddle the blocks of four
def test_rng_step_equals_the_two_stage_form(device, hw, cond_f, cfg):
    b, (h, w) = 2, hw
    per_clip = C * FP * h * w
    coef1, coef0 = _coef(device, 10, 1.0)[0], _coef(device, 10, 0.0)[0]
    eps = _randn(((2 if cfg else 1) * b, C, FP + cond_f, h, w), 1).to(device)
    x = _randn((b, C, FP, h, w), 2).to(device)
    seeds = ops.seed_words(SEEDS).to(device)
    kw = dict(cfg=cfg, scale=7.5, cond_f=cond_f)
    for index in (0, 5):
        assert float(coef1[index, 2]) != 0
        for temperature in (1.0, 0.7):
            want = ops.cfg_ddim_step(eps, x, coef1, index, noise=_noise(SEEDS, index, per_clip, x.shape, temperature, device), **kw)
            got = ops.cfg_ddim_step_rng(eps, x, coef1, index, seeds, temperature=temperature, **kw)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (index, temperature)
            xs = x.clone()                               # x_prev aliases x, pred_x0 NULL
            alias = ops.cfg_ddim_step_rng(eps, xs, coef1, index, seeds, temperature=temperature, x_prev=xs, want_pred_x0=False, **kw)
            assert alias[1] is None and alias[0] is xs and torch.equal(xs, want[0]), (index, temperature)
        # row 1 of the b = 2 call is the b = 1 call with that seed
        rows = [1, b + 1] if cfg else [1]
        one = ops.cfg_ddim_step_rng(eps[rows].contiguous(), x[1:2].contiguous(), coef1, index, seeds[1:2].contiguous(), temperature=0.7, **kw)
        assert torch.equal(one[0], got[0][1:2]) and torch.equal(one[1], got[1][1:2]), index
        # the noise is there: another seed, another result
        other = ops.cfg_ddim_step_rng(eps, x, coef1, index, ops.seed_words((SEEDS[0], SEEDS[0])).to(device), temperature=0.7, **kw)
        assert torch.equal(other[0][0], got[0][0]) and not torch.equal(other[0][1], got[0][1])
    # sigma == 0: nothing is drawn, the bits of the existing kernel without a noise tensor
    want = ops.cfg_ddim_step(eps, x, coef0, 5, noise=None, **kw)
    got = ops.cfg_ddim_step_rng(eps, x, coef0, 5, seeds, temperature=0.7, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("f1", [0, 2])
def test_a_chain_of_rng_dev_steps_equals_the_host_index_kernel(device, f1):
    """begin -> given eps -> seer_cfg_ddim_step_rng_dev, call after call with no host write: every step is the host-index kernel's,
    and the step words move as seer_cfg_ddim_step_dev moves them"""
    b, h, w = 2, 7, 5
    coef, ttab = _coef(device, 4, 1.0)
    n = coef.shape[0]
    x = _randn((b, C, FP, h, w), 3).to(device)
    x0 = _randn((b, C, f1, h, w), 4).to(device) if f1 else None
    seeds = ops.seed_words(SEEDS).to(device)
    pred = torch.empty_like(x)
    step = torch.tensor([n - 1, 99], dtype=torch.int32, device=device)
    sample = torch.empty((2 * b, C, f1 + FP, h, w), device=device)
    t_out = torch.empty((2 * b,), dtype=torch.long, device=device)
    ref = x.clone()
    for index in reversed(range(n)):
        eps = _randn((2 * b, C, f1 + FP, h, w), 100 + index).to(device)
        ops.ddim_step_begin(x0, x, ttab, step, 2, sample, t_out)
        twin = step.clone()                              # the deterministic _dev kernel on a copy of the words
        ops.cfg_ddim_step_dev(eps, x, coef, twin, cfg=True, scale=3.0, cond_f=f1, x_prev=torch.empty_like(x), pred_x0=None)
        ops.cfg_ddim_step_rng_dev(eps, x, coef, step, seeds, cfg=True, scale=3.0, cond_f=f1, temperature=0.7, x_prev=x, pred_x0=pred)
        assert step.tolist() == twin.tolist() == [index - 1, index]
        ref, p = ops.cfg_ddim_step_rng(eps, ref, coef, index, seeds, cfg=True, scale=3.0, cond_f=f1, temperature=0.7)
        assert torch.equal(x, ref) and torch.equal(pred, p), index
    assert step.tolist() == [-1, 0] and torch.isfinite(x).all()


@pytest.mark.parametrize("cond_f", [0, 2])
@pytest.mark.parametrize("hw", [(8, 12), (7, 5)])
def test_slot_rng_update_equals_the_single_clip_kernel_slot_by_slot(device, hw, cond_f):
    slots, nsched, (h, w) = 4, 16, hw
    etas, lengths, index = (1.0, 0.5, 0.0, 1.0), (10, 4, 4, 4), (5, 0, 2, -1)       # a deterministic slot; the fourth slot is idle
    solo = [_coef(device, S, eta)[0] for S, eta in zip(lengths, etas)]
    coef = torch.zeros((slots, nsched, 4), device=device)
    coef[:, :, 0] = 1.0
    for s, t in enumerate(solo):
        coef[s, :t.shape[0]] = t
    scale = torch.tensor([7.5, 3.0, 2.0, 7.5], device=device)
    temp = torch.tensor([1.0, 0.7, 0.7, 1.0], device=device)
    seed_list = (SEEDS[0], SEEDS[1], 99, 5)
    seeds = ops.seed_words(seed_list).to(device)
    eps = _randn((2 * slots, C, FP + cond_f, h, w), 1).to(device)
    x = _randn((slots, C, FP, h, w), 2).to(device)
    want = [ops.cfg_ddim_step_rng(eps[[s, slots + s]].contiguous(), x[s:s + 1].contiguous(), solo[s], index[s], seeds[s:s + 1].contiguous(),
                                  cfg=True, scale=float(scale[s]), cond_f=cond_f, temperature=float(temp[s])) for s in range(3)]
    det = ops.cfg_ddim_step(eps[[2, slots + 2]].contiguous(), x[2:3].contiguous(), solo[2], 2, cfg=True, scale=2.0, cond_f=cond_f)
    assert torch.equal(want[2][0], det[0])
    for alias in (False, True):
        step = torch.tensor([[77, i] for i in index], dtype=torch.int32, device=device)
        xs = x.clone()
        x_prev = xs if alias else torch.full_like(x, float("nan"))
        pred = torch.full_like(x, float("nan"))
        ops.slot_cfg_ddim_step_rng(eps, xs, scale, coef, step, seeds, temp, cond_f=cond_f, x_prev=x_prev, pred_x0=pred)
        for s in range(3):
            assert torch.equal(x_prev[s:s + 1], want[s][0]) and torch.equal(pred[s:s + 1], want[s][1]), (alias, s)
        assert step.tolist() == [[4, 5], [-1, 0], [1, 2], [77, -1]]             # the idle slot's words are untouched
        assert torch.isnan(pred[3]).all()
        assert torch.equal(x_prev[3], x[3]) if alias else torch.isnan(x_prev[3]).all()
        if not alias:
            assert torch.equal(xs, x)
    ops.slot_cfg_ddim_step_rng(eps, x.clone(), scale, coef, torch.tensor([[77, i] for i in index], dtype=torch.int32, device=device),
                               seeds, temp, cond_f=cond_f, x_prev=torch.empty_like(x), pred_x0=None)     # pred_x0 may be NULL


def test_every_refusal_returns_einval(device):
    buf = torch.zeros(1 << 18, device=device)
    lib = _lib.load()
    n = 0
    for fn, args, why in refusal_cases(buf.data_ptr()):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    assert n >= 60
    torch.cuda.synchronize()
    assert not buf.any()                                  # nothing ran


# ---- 3. the samplers on the mini UNet -----------------------------------------------------------------------------------------------
F1, FL, HL, S_STEPS, ETA, SCALE = 1, 2, 8, 4, 0.5, 7.5
_cache = {}


def _inputs(device):
    D = CFG_MINI["cross_attention_dim"]
    return dict(c=_randn((1, F1 + FL, 77, D), 20).to(device), c2=_randn((1, F1 + FL, 77, D), 21).to(device),
                uc=_randn((1, 1, 77, D), 29).expand(-1, F1 + FL, -1, -1).contiguous().to(device),
                x0=_randn((1, 4, F1, HL, HL), 40, 0.9).to(device), x0b=_randn((1, 4, F1, HL, HL), 41, 0.9).to(device),
                xT=_randn((1, 4, FL, HL, HL), 30).to(device))


def _sample(device, use_graph, seed, *, eta=ETA, rows=1, x_T=None, temperature=1.0):
    """DDIMSampler.sample of `rows` clips; with rows = 2 the clip under test is row 1 behind another clip"""
    m = _model(device, None, layout_invariant=True)
    i = _inputs(device)
    c = i["c"] if rows == 1 else torch.cat([i["c2"], i["c"]])
    x0 = i["x0"] if rows == 1 else torch.cat([i["x0b"], i["x0"]])
    m.use_graph = use_graph
    try:
        lat, _ = DDIMSampler(device).sample(m, S_STEPS, batch_size=rows, shape=(4, FL, HL, HL), x0_emb=x0, conditioning=c, verbose=False,
                                            cond_frames=F1, unconditional_guidance_scale=SCALE, temperature=temperature,
                                            unconditional_conditioning=i["uc"].expand(rows, -1, -1, -1).contiguous(), eta=eta, x_T=x_T,
                                            is_3d=True, seed=seed)
    finally:
        m.use_graph = False
    return lat


def _solo(device):
    if "solo" not in _cache:
        _cache["solo"] = _sample(device, False, SEEDS[1])
    return _cache["solo"]


@pytest.mark.parametrize("use_graph", [False, True])
def test_a_seeded_clip_alone_and_as_a_row_of_a_batch(device, use_graph):
    want = _solo(device)
    assert torch.isfinite(want).all() and want.shape == (1, 4, FL, HL, HL)
    state = torch.cuda.get_rng_state(device)
    again = _sample(device, use_graph, SEEDS[1])
    assert torch.equal(torch.cuda.get_rng_state(device), state)         # nothing is drawn from torch's generator
    assert torch.equal(again, want)                                      # the same seed twice; captured == launch by launch
    assert not torch.equal(_sample(device, use_graph, SEEDS[1] + 1), want)
    assert not torch.equal(_sample(device, use_graph, SEEDS[1], eta=0.0), want)
    pair = _sample(device, use_graph, [77, SEEDS[1]], rows=2)
    assert torch.equal(pair[1:2], want)
    assert torch.equal(_sample(device, use_graph, SEEDS[1] - 1, rows=2)[1:2], want)        # an int s: row i runs seed s + i
    if use_graph:
        kinds = [k[0] for k in _model(device, None, layout_invariant=True)._engine._graphs if isinstance(k, tuple) and k]
        assert "step-rng" in kinds


def test_a_seed_at_eta_zero_with_a_start_code_is_the_unseeded_result(device):
    xT = _inputs(device)["xT"]
    for use_graph in (False, True):
        assert torch.equal(_sample(device, use_graph, 5, eta=0.0, x_T=xT), _sample(device, use_graph, None, eta=0.0, x_T=xT))


@pytest.mark.parametrize("use_graph", [False, True])
def test_a_seeded_clip_in_a_slot_beside_a_deterministic_clip(device, use_graph):
    """three slots; a deterministic clip runs two steps, then the seeded clip is admitted beside it: its latent is the solo
    sampler's, and the deterministic clip's is what DDIMSampler gives it alone"""
    m = _model(device, None, layout_invariant=True)
    i = _inputs(device)
    want_det = _sample(device, False, None, eta=0.0, x_T=i["xT"])
    m.use_graph = use_graph
    try:
        smp = SlotSampler(m, 3, shape=(4, FL, HL, HL), cond_frames=F1, context_shape=(77, CFG_MINI["cross_attention_dim"]), device=device,
                          model_cond_frame=F1, stochastic=True)
        assert smp.submit(i["xT"], i["x0"], i["c"], i["uc"], S_STEPS, SCALE) == 0
        done = smp.step() + smp.step()
        assert done == [] and smp.submit(None, i["x0"], i["c"], i["uc"], S_STEPS, SCALE, eta=ETA, seed=SEEDS[1]) == 1
        while smp.active():
            done += smp.step()
        if use_graph:
            assert sum(isinstance(k, tuple) and k and k[0] == "slots-rng" for k in m._engine._graphs) == 1
    finally:
        m.use_graph = False
    assert [s for s, _ in done] == [0, 1]
    assert torch.equal(done[0][1], want_det)
    assert torch.equal(done[1][1], _solo(device)), (done[1][1] - _solo(device)).abs().max().item()


def test_generate_queue_stochastic_equals_each_request_alone(device):
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
    empty = _randn((1, 77, 192), 3).to(device)
    reqs = []
    for k, (S, extra) in enumerate(((4, dict(seed=11, eta=0.5)), (5, dict(seed=12, eta=1.0, temperature=0.7)),
                                    (4, dict(noise=_randn((1, 4, 2, 8, 8), 72))))):
        reqs.append(dict(x0_image=torch.tanh(_randn((1, 3, 1, 64, 64), 50 + k)).to(device), text_emb=_randn((1, 77, 192), 60 + k % 2).to(device),
                         empty_emb=empty, ddim_steps=S, scale=7.5, tag=f"clip{k}", **extra))
    queue = lambda rs, slots: dict(generate_queue(unet, fst, vae, iter(rs), slots=slots, num_frames=3, cond_frames=1, stochastic=True,
                                                  latent_generator=torch.Generator(device=device).manual_seed(5)))
    got = queue(reqs, 2)
    assert list(got) == ["clip0", "clip1", "clip2"]
    lg = torch.Generator(device=device).manual_seed(5)   # the queue draws the conditioning latents in admission order: so does this loop
    for r in reqs:
        want = dict(generate_queue(unet, fst, vae, iter([r]), slots=1, num_frames=3, cond_frames=1, stochastic=True, latent_generator=lg))
        clip = got[r["tag"]]
        assert clip.shape == (1, 3, 2, 64, 64) and torch.isfinite(clip).all() and clip.min() >= 0 and clip.max() <= 1
        assert torch.equal(clip, want[r["tag"]]), (r["tag"], (clip - want[r["tag"]]).abs().max().item())
    assert not torch.equal(got["clip0"], queue([dict(reqs[0], seed=13)], 1)["clip0"])
