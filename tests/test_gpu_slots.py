"""SlotSampler on a real MI355X.  The two slot kernels against the single-clip kernels they restate, slot by slot and bit for bit
(an idle slot with NaN sentinels, x_prev aliasing x, a chain of replays, every refusal); the sampler on the mini UNet under the
layout-invariant mode against DDIMSampler.sample of each clip alone, torch.equal, launch by launch and captured (one capture for
three schedules and two scales); captured against launch by launch in the default mode; pipeline.generate_queue against
generate_clips of each request alone."""
import pytest
import torch

from seervideoldm_amd import (AutoencoderKL, DDIMSampler, FSTextTransformer, SeerUNet, SlotSampler, _lib, ops, synth)
from seervideoldm_amd.pipeline import generate_clips, generate_queue
from seervideoldm_amd.vae import ldm_to_diffusers_vae
from tests.test_slots_host import refusal_cases

pytestmark = pytest.mark.gpu

CFG_MINI = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)
NSCHED = 16
_models, _solo = {}, {}


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tables(device, lengths):
    """per-slot schedule tables [slots, NSCHED, ...] from DDIMSampler.make_schedule(S) per slot, and the per-slot originals"""
    coef = torch.zeros((len(lengths), NSCHED, 4), device=device)
    coef[:, :, 0] = 1.0
    ttab = torch.zeros((len(lengths), NSCHED), device=device, dtype=torch.long)
    solo = []
    for s, S in enumerate(lengths):
        smp = DDIMSampler(device)
        smp.make_schedule(S, verbose=False)
        n = smp.ddim_coef.shape[0]
        coef[s, :n], ttab[s, :n] = smp.ddim_coef, smp._t_table
        solo.append((smp.ddim_coef, smp._t_table))
    return coef, ttab, solo


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond_f", [0, 2])
def test_slot_update_equals_the_single_clip_kernel_slot_by_slot(device, cond_f):
    slots, C, Fp, h, w = 3, 4, 3, 8, 12                   # 1152 elements per slot: slot boundaries inside a block, a ragged last block
    coef, _, solo = _tables(device, (10, 4, 4))
    scale = torch.tensor([7.5, 3.0, 2.0], device=device)
    eps = _randn((2 * slots, C, Fp + cond_f, h, w), 1).to(device)
    x = _randn((slots, C, Fp, h, w), 2).to(device)
    index = (5, 0, -1)                                    # the third slot is idle
    want = [ops.cfg_ddim_step(eps[[s, slots + s]].contiguous(), x[s:s + 1].contiguous(), solo[s][0], index[s], cfg=True,
                              scale=float(scale[s]), cond_f=cond_f) for s in range(2)]
    for alias in (False, True):
        step = torch.tensor([[77, i] for i in index], dtype=torch.int32, device=device)
        xs = x.clone()
        x_prev = xs if alias else torch.full_like(x, float("nan"))
        pred = torch.full_like(x, float("nan"))
        ops.slot_cfg_ddim_step(eps, xs, scale, coef, step, cond_f=cond_f, x_prev=x_prev, pred_x0=pred)
        for s in range(2):
            assert torch.equal(x_prev[s:s + 1], want[s][0]) and torch.equal(pred[s:s + 1], want[s][1]), (alias, s)
        assert step.tolist() == [[4, 5], [-1, 0], [77, -1]]                  # the idle slot's words are untouched
        assert torch.isnan(pred[2]).all()
        assert torch.equal(x_prev[2], x[2]) if alias else torch.isnan(x_prev[2]).all()
        if not alias:
            assert torch.equal(xs, x)


@pytest.mark.parametrize("f1", [0, 2])
def test_slot_begin_equals_the_single_clip_kernel_slot_by_slot(device, f1):
    slots, reps, C, Fp, h, w = 3, 2, 4, 3, 8, 12
    _, ttab, solo = _tables(device, (10, 4, 4))
    x = _randn((slots, C, Fp, h, w), 3).to(device)
    x0 = _randn((slots, C, f1, h, w), 4).to(device) if f1 else None
    x[2].zero_()                                          # the idle slot as the host leaves it
    if f1:
        x0[2].zero_()
    step = torch.tensor([[5, 99], [0, 99], [-1, 99]], dtype=torch.int32, device=device)
    sample = torch.full((reps * slots, C, f1 + Fp, h, w), float("nan"), device=device)
    t_out = torch.full((reps * slots,), -7, dtype=torch.long, device=device)
    ops.slot_step_begin(x0, x, ttab, step, reps, sample, t_out)
    assert step.tolist() == [[5, 5], [0, 0], [-1, -1]]
    for s in range(2):
        st = step[s].clone()
        st[1] = 99
        one, t_one = torch.empty((reps, C, f1 + Fp, h, w), device=device), torch.empty((reps,), dtype=torch.long, device=device)
        ops.ddim_step_begin(None if x0 is None else x0[s:s + 1].contiguous(), x[s:s + 1].contiguous(), solo[s][1], st, reps, one, t_one)
        assert torch.equal(sample[[s, slots + s]], one) and torch.equal(t_out[[s, slots + s]], t_one), s
    assert t_out[[2, slots + 2]].tolist() == [int(ttab[2, 0])] * 2 and int(ttab[2, 0]) == 1
    assert torch.isfinite(sample).all() and not sample[[2, slots + 2]].any()


def test_a_chain_of_replays_walks_every_slots_schedule(device):
    """begin -> given eps -> update, call after call, with no host write between the calls but the admission of the second clip: an
    S = 6 slot (stride 166: 7 entries, so seven calls walk it) and an S = 4 slot admitted two calls later, which then idles through the
    last call.  Every call against the host-index kernel of each clip; the counters end at -1."""
    slots, C, Fp, f1, h, w = 2, 4, 3, 1, 8, 12
    coef, ttab, solo = _tables(device, (6, 4))
    n0, n1 = solo[0][0].shape[0], solo[1][0].shape[0]
    assert (n0, n1) == (7, 4)
    scale = torch.tensor([7.5, 3.0], device=device)
    x = torch.zeros((slots, C, Fp, h, w), device=device)
    x0 = _randn((slots, C, f1, h, w), 5).to(device)
    pred = torch.zeros_like(x)
    step = torch.full((slots, 2), -1, dtype=torch.int32, device=device)
    sample = torch.empty((2 * slots, C, f1 + Fp, h, w), device=device)
    t_out = torch.empty((2 * slots,), dtype=torch.long, device=device)
    x[0] = _randn((C, Fp, h, w), 6).to(device)
    step[0, 0] = n0 - 1
    ref = [x[0:1].clone(), None]
    for call in range(n0):
        if call == 2:                                    # the second clip is admitted
            x[1] = _randn((C, Fp, h, w), 7).to(device)
            step[1, 0] = n1 - 1
            ref[1] = x[1:2].clone()
        idx = (n0 - 1 - call, n1 - 1 - (call - 2) if 2 <= call < 2 + n1 else -1)
        eps = _randn((2 * slots, C, f1 + Fp, h, w), 100 + call).to(device)
        ops.slot_step_begin(x0, x, ttab, step, 2, sample, t_out)
        assert t_out.tolist() == [int(ttab[s, max(idx[s], 0)]) for s in (0, 1)] * 2, call
        assert torch.equal(sample[:slots, :, f1:], x) and torch.equal(sample[slots:, :, :f1], x0)
        before = x.clone()
        ops.slot_cfg_ddim_step(eps, x, scale, coef, step, cond_f=f1, x_prev=x, pred_x0=pred)
        for s in (0, 1):
            if idx[s] < 0:
                assert torch.equal(x[s], before[s]), (call, s)
                continue
            ref[s], p = ops.cfg_ddim_step(eps[[s, slots + s]].contiguous(), ref[s], solo[s][0], idx[s], cfg=True, scale=float(scale[s]),
                                          cond_f=f1)
            assert torch.equal(x[s:s + 1], ref[s]) and torch.equal(pred[s:s + 1], p), (call, s)
        assert step[:, 0].tolist() == [max(i - 1, -1) for i in idx], call
    assert step[:, 0].tolist() == [-1, -1]


def test_every_refusal_returns_einval(device):
    """the same list the CPU suite runs on made-up pointers, here on one real buffer that every good argument set would fit in"""
    buf = torch.zeros(1 << 18, device=device)
    lib = _lib.load()
    n = 0
    for fn, args, why in refusal_cases(buf.data_ptr()):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    assert n >= 40
    torch.cuda.synchronize()
    assert not buf.any()                                  # nothing ran


# ---- 2. the sampler on the mini UNet ---------------------------------------------------------------------------------------------
def _model(device, dtype=None, **kw):
    key = (dtype, tuple(sorted(kw.items())))
    if key not in _models:
        m = SeerUNet(**CFG_MINI, compute_dtype=dtype, **kw)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI)), strict=True)
        _models[key] = m.to(device).eval()
    return _models[key]


F1, FP, HL = 1, 3, 16


def _requests(device):
    """three requests, two prompts (the third repeats the first's), three schedule lengths, two scales"""
    D = CFG_MINI["cross_attention_dim"]
    prompts = [_randn((1, F1 + FP, 77, D), 20 + k).to(device) for k in range(2)]
    uc = _randn((1, 1, 77, D), 29).expand(-1, F1 + FP, -1, -1).contiguous().to(device)
    reqs = []
    for k, (S, scale) in enumerate(((4, 7.5), (6, 3.0), (5, 7.5))):
        reqs.append(dict(x_T=_randn((1, 4, FP, HL, HL), 30 + k).to(device), x0_emb=_randn((1, 4, F1, HL, HL), 40 + k, 0.9).to(device),
                         c=prompts[k % 2], uc=uc, S=S, scale=scale, tag=k))
    return reqs


def _solo_latents(device, dtype):
    """every request alone through DDIMSampler.sample (launch by launch), once per storage type for the module"""
    if dtype not in _solo:
        m = _model(device, dtype, layout_invariant=True)
        m.use_graph = False
        out = []
        for r in _requests(device):
            lat, _ = DDIMSampler(device).sample(m, r["S"], batch_size=1, shape=(4, FP, HL, HL), x0_emb=r["x0_emb"], conditioning=r["c"],
                                                verbose=False, cond_frames=F1, unconditional_guidance_scale=r["scale"],
                                                unconditional_conditioning=r["uc"], eta=0., x_T=r["x_T"], is_3d=True)
            out.append(lat)
        _solo[dtype] = out
    return _solo[dtype]


def _slot_sampler(m, device, slots=2):
    return SlotSampler(m, slots, shape=(4, FP, HL, HL), cond_frames=F1, context_shape=(77, CFG_MINI["cross_attention_dim"]),
                       device=device, model_cond_frame=F1)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("dtype", [None, torch.float16])
def test_a_slot_returns_the_bits_of_the_solo_run(device, monkeypatch, dtype, use_graph):
    """two slots, three requests, the third entering when the first leaves: every latent is the solo sampler's, and the captured run
    captures ONE graph for three schedule lengths and two scales"""
    m = _model(device, dtype, layout_invariant=True)
    captures = []
    real = torch.cuda.CUDAGraph

    def spy(*a, **k):
        captures.append(1)
        return real(*a, **k)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", spy)
    m.use_graph = use_graph
    try:
        smp = _slot_sampler(m, device)
        got = list(smp.run(iter(_requests(device))))
        assert m._engine.inv and m._engine.dt == (dtype or torch.bfloat16)
        slot_graphs = [k for k in m._engine._graphs if isinstance(k, tuple) and k and k[0] == "slots"]
        assert (len(captures), len(slot_graphs)) == ((1, 1) if use_graph else (0, 0))
    finally:
        m.use_graph = False
    monkeypatch.setattr(torch.cuda, "CUDAGraph", real)
    assert [tag for tag, _ in got] == [0, 1, 2]          # 4, 7 and 5 entries: steps 4, 7 and 9
    want = _solo_latents(device, dtype)
    for tag, lat in got:
        assert torch.isfinite(lat).all() and lat.shape == want[tag].shape
        assert torch.equal(lat, want[tag]), (tag, (lat - want[tag]).abs().max().item())
    assert not torch.equal(got[0][1], got[2][1])


def test_captured_and_launch_by_launch_steps_agree_in_the_default_mode(device):
    m = _model(device)
    runs = {}
    try:
        for use_graph in (False, True):
            m.use_graph = use_graph
            smp = _slot_sampler(m, "cuda")               # no index: still the engine's device (a mismatch would re-pack per step)
            reqs = _requests(device)
            trace, finished, engines = [], [], []
            for r in reqs[:2]:
                smp.submit(**{k: v for k, v in r.items() if k != "tag"})
            for n in range(1, 10):
                live = smp.active()
                done = smp.step()
                engines.append(m._engine)
                trace.append([smp.pred_x0(s) for s in live])
                finished += [lat for _, lat in done]
                if n == 4:
                    assert [s for s, _ in done] == [0]
                    smp.submit(**{k: v for k, v in reqs[2].items() if k != "tag"})
            assert len(finished) == 3 and smp.free_slots() == [0, 1] and not m._engine.inv
            assert all(e is engines[0] for e in engines) and smp.device == m._engine.device
            if use_graph:
                assert sum(isinstance(k, tuple) and k and k[0] == "slots" for k in m._engine._graphs) == 1
            runs[use_graph] = (trace, finished)
        assert any(isinstance(k, tuple) and k and k[0] == "slots" for k in m._engine._graphs), "the captured step never ran"
    finally:
        m.use_graph = False
    for a, b in zip(runs[False][1], runs[True][1]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    for n, (pa, pb) in enumerate(zip(runs[False][0], runs[True][0])):
        assert len(pa) == len(pb) and all(torch.equal(a, b) for a, b in zip(pa, pb)), n


# ---- 3. the queue -----------------------------------------------------------------------------------------------------------------
def test_generate_queue_returns_the_clips_of_generate_clips(device):
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
    for k, (S, scale) in enumerate(((4, 7.5), (5, 3.0), (4, 7.5))):
        reqs.append(dict(x0_image=torch.tanh(_randn((1, 3, 1, 64, 64), 50 + k)).to(device), text_emb=_randn((1, 77, 192), 60 + k % 2).to(device),
                         empty_emb=empty, ddim_steps=S, scale=scale, noise=_randn((1, 4, 2, 8, 8), 70 + k), tag=f"clip{k}"))
    got = dict(generate_queue(unet, fst, vae, iter(reqs), slots=2, num_frames=3, cond_frames=1,
                              latent_generator=torch.Generator(device=device).manual_seed(5)))
    assert list(got) == ["clip0", "clip1", "clip2"]     # 4 entries: step 4; 5 entries: step 5; 4 more from step 5 on: step 8
    lg = torch.Generator(device=device).manual_seed(5)   # the queue draws the conditioning latents in admission order: so does this loop
    for k, r in enumerate(reqs):
        want = generate_clips(unet, fst, vae, DDIMSampler(device), r["x0_image"], r["text_emb"], r["empty_emb"], num_frames=3,
                              cond_frames=1, ddim_steps=r["ddim_steps"], scale=r["scale"], num_samples=1,
                              noise_generator=torch.Generator().manual_seed(70 + k), latent_generator=lg)[0]
        clip = got[r["tag"]]
        assert clip.shape == want.shape == (1, 3, 2, 64, 64) and torch.isfinite(clip).all() and clip.min() >= 0 and clip.max() <= 1
        assert torch.equal(clip, want), (k, (clip - want).abs().max().item())
