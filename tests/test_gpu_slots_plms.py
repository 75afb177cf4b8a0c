"""SlotSampler(plms=True) on a real MI355X.  The two kernels that carry a sampler per slot against the single-clip kernels they
restate, slot by slot and bit for bit (a DDIM slot, the three PLMS phases and an idle slot side by side, NaN sentinels wherever
nothing may be read or written, x_prev aliasing x, the state words, a chain walked by the kernels alone, every refusal); the sampler
on the mini UNet under the layout-invariant mode against PLMSSampler.sample / DDIMSampler.sample of each clip alone, torch.equal,
launch by launch and captured (one capture for three schedules, two scales and two methods); captured against launch by launch in
the default mode; pipeline.generate_queue(plms=True) against generate_clips over PLMSSampler of each request alone."""
import pytest
import torch

from seervideoldm_amd import (AutoencoderKL, DDIMSampler, FSTextTransformer, PLMSSampler, SeerUNet, SlotSampler, _lib, ops, synth)
from seervideoldm_amd.pipeline import generate_clips, generate_queue
from seervideoldm_amd.vae import ldm_to_diffusers_vae
from tests.test_gpu_slots import CFG_MINI, F1, FP, HL, _model, _randn, _requests, _solo_latents, _tables
from tests.test_slots_plms_host import plms_refusal_cases

pytestmark = pytest.mark.gpu

NAN = float("nan")
_solo_plms = {}


def _same(a, b):
    """bit for bit, NaN included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------
SLOTS, C, FPK, HK, WK = 4, 4, 3, 5, 5                     # HW = 25: 300 / 500 elements per slot, 256-thread blocks straddle the slots
PHASE = (0, 1, 2, 3)                                      # a DDIM slot, the two evaluations of a PLMS clip's first step, a later step
INDEX = (5, 3, 3, 1)
RING = ((0, 0), (0, 2), (1, 1), (3, 1))                   # (valid, newest) in flight; the phase-3 slot runs order 4
LENGTHS = (10, 4, 4, 6)


def _kernel_inputs(device, f1, idle):
    coef, ttab, solo = _tables(device, LENGTHS)
    scale = torch.tensor([7.5, 3.0, 2.0, 5.0], device=device)
    eps = _randn((2 * SLOTS, C, f1 + FPK, HK, WK), 1).to(device)
    x = _randn((SLOTS, C, FPK, HK, WK), 2).to(device)
    x_prov = _randn((SLOTS, C, FPK, HK, WK), 3).to(device)
    x0 = _randn((SLOTS, C, f1, HK, WK), 4).to(device) if f1 else None
    ring = torch.full((SLOTS, 3, C, FPK, HK, WK), NAN, device=device)      # NaN in every entry the slot's order does not read
    ring[2, 1] = _randn((C, FPK, HK, WK), 5).to(device)
    ring[3] = _randn((3, C, FPK, HK, WK), 6).to(device)
    index = list(INDEX)
    if idle is not None:                                  # the idle slot: a counter of -1 and NaN wherever the kernels could touch it
        index[idle] = -1
        x[idle], x_prov[idle], ring[idle] = NAN, NAN, NAN
    return coef, ttab, solo, scale, eps, x, x_prov, x0, ring, index


@pytest.mark.parametrize("idle", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("cond_f", [0, 2])
def test_slot_plms_update_equals_the_single_clip_kernels_slot_by_slot(device, cond_f, idle):
    coef, _, solo, scale, eps, x, x_prov, _, ring, index = _kernel_inputs(device, cond_f, idle)
    pair = lambda s: eps[[s, SLOTS + s]].contiguous()
    kw = lambda s: dict(cfg=True, scale=float(scale[s]), cond_f=cond_f)
    one = lambda t, s: t[s:s + 1].contiguous()
    want = {}
    if idle != 0:
        want[0] = ops.cfg_ddim_step(pair(0), one(x, 0), solo[0][0], index[0], **kw(0))
    if idle != 1:
        want[1] = ops.cfg_plms_step(pair(1), one(x, 1), solo[1][0], index[1], 0, want_pred_x0=False, **kw(1))
    if idle != 2:
        want[2] = ops.cfg_plms_step(pair(2), one(x, 2), solo[2][0], index[2], 1, history=[one(ring[2], 1)], **kw(2))
    if idle != 3:                                         # newest = 1: h1, h2, h3 = entries 1, 0, 2 and e goes into entry 2
        want[3] = ops.cfg_plms_step(pair(3), one(x, 3), solo[3][0], index[3], 4, history=[one(ring[3], k) for k in (1, 0, 2)], **kw(3))
    for alias in (False, True):
        step = torch.tensor([[77, i] for i in index], dtype=torch.int32, device=device)
        state0 = torch.tensor([[55, 56, 57, 58, p, v, n, 59] for p, (v, n) in zip(PHASE, RING)], dtype=torch.int32, device=device)
        state, xs, xp, rg = state0.clone(), x.clone(), x_prov.clone(), ring.clone()
        x_prev = xs if alias else torch.full_like(x, NAN)
        pred = torch.full_like(x, NAN)
        ops.slot_cfg_plms_step(eps, xs, scale, coef, step, state, rg, xp, cond_f=cond_f, x_prev=x_prev, pred_x0=pred)
        untouched = lambda s: _same(x_prev[s], x[s]) if alias else torch.isnan(x_prev[s]).all()
        st, sw = step.tolist(), state.tolist()
        for s in range(SLOTS):
            assert sw[s][3:] == state0[s, 3:].tolist(), (alias, s)               # nothing writes an in-flight word
            if s == idle:                                 # no latent, no ring entry, no word of step or state
                assert untouched(s) and torch.isnan(pred[s]).all() and torch.isnan(xp[s]).all() and torch.isnan(rg[s]).all()
                assert torch.isnan(xs[s]).all() and st[s] == [77, -1] and sw[s] == state0[s].tolist(), (alias, s)
                continue
            if s == 1:                                    # the provisional update: x_prov and ring entry 0, nothing else
                assert torch.equal(xp[1:2], want[1][0]) and torch.equal(rg[1:2, 0], want[1][2]) and torch.isnan(rg[1, 1:]).all()
                assert untouched(1) and torch.isnan(pred[1]).all() and st[1] == [77, index[1]] and sw[1][:3] == [2, 1, 0], alias
                continue
            assert torch.equal(x_prev[s:s + 1], want[s][0]) and torch.equal(pred[s:s + 1], want[s][1]), (alias, s)
            assert _same(xp[s], x_prov[s]) and st[s] == [index[s] - 1, index[s]], (alias, s)
            if s == 3:
                assert torch.equal(rg[3:4, 2], want[3][2]) and _same(rg[3, :2], ring[3, :2]) and sw[3][:3] == [55, 3, 2], alias
            else:
                assert _same(rg[s], ring[s]) and sw[s][:3] == [[55, 56, 57], None, [3, 56, 57]][s], (alias, s)
        if not alias:
            assert _same(xs, x)


@pytest.mark.parametrize("idle", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("f1", [0, 2])
def test_slot_plms_begin_equals_the_single_clip_kernel_slot_by_slot(device, f1, idle):
    reps = 2
    _, ttab, solo, _, _, x, x_prov, x0, ring, index = _kernel_inputs(device, f1, idle)
    step = torch.tensor([[i, 99] for i in index], dtype=torch.int32, device=device)
    state0 = torch.tensor([[p, v, n, 58, 65, 66, 67, 59] for p, (v, n) in zip(PHASE, RING)], dtype=torch.int32, device=device)
    state, xs, xp = state0.clone(), x.clone(), x_prov.clone()
    sample = torch.full((reps * SLOTS, C, f1 + FPK, HK, WK), 123.0, device=device)
    t_out = torch.full((reps * SLOTS,), -7, dtype=torch.long, device=device)
    ops.slot_plms_step_begin(x0, xs, xp, ttab, step, state, reps, sample, t_out)
    assert step.tolist() == [[i, i] for i in index]
    assert state.tolist() == [[p, v, n, 58, p, v, n, 59] for p, (v, n) in zip(PHASE, RING)]          # the next words, copied
    assert _same(xs, x) and _same(xp, x_prov)
    for s in range(SLOTS):
        if s == idle:
            assert t_out[[s, SLOTS + s]].tolist() == [int(ttab[s, 0])] * 2
            continue
        # the second evaluation of the first PLMS step runs at the provisional latent and at the next timestep
        lat, at = (x_prov, index[s] - 1) if PHASE[s] == 2 else (x, index[s])
        st = torch.tensor([at, 99], dtype=torch.int32, device=device)
        one, t_one = torch.empty((reps, C, f1 + FPK, HK, WK), device=device), torch.empty((reps,), dtype=torch.long, device=device)
        ops.ddim_step_begin(None if x0 is None else x0[s:s + 1].contiguous(), lat[s:s + 1].contiguous(), solo[s][1], st, reps, one, t_one)
        assert torch.equal(sample[[s, SLOTS + s]], one) and torch.equal(t_out[[s, SLOTS + s]], t_one), s
    assert int(t_out[2]) == int(solo[2][1][INDEX[2] - 1]) != int(solo[2][1][INDEX[2]]) or idle == 2


def _eps_of(sample, t):
    """an elementwise model: rows of the first half are the empty-prompt rows"""
    half = sample.shape[0] // 2
    prompt = (torch.arange(sample.shape[0], device=sample.device) >= half).float().view(-1, 1, 1, 1, 1)
    return torch.sin(1.3 * sample + 0.01 * t.float().view(-1, 1, 1, 1, 1)) + 0.25 * prompt * torch.cos(sample)


def test_a_chain_walks_every_slots_schedule_and_phases(device):
    """begin -> eps(sample, t) -> update, call after call, with NO host write after the admission: PLMS clips of 1, 2 and 4 entries
    (two, three and five calls) and a DDIM clip of 7, against the same chains through the single-clip kernels.  The ring, x_prov and
    pred_x0 start as NaN: an entry the order does not use is never read."""
    f1, methods = 1, ("plms", "plms", "plms", "ddim")
    coef, ttab, solo = _tables(device, (1, 2, 4, 6))
    lengths = [c.shape[0] for c, _ in solo]
    assert lengths == [1, 2, 4, 7]
    scale = torch.tensor([7.5, 3.0, 2.0, 5.0], device=device)
    x_T = _randn((SLOTS, C, FPK, HK, WK), 7).to(device)
    x0 = _randn((SLOTS, C, f1, HK, WK), 8).to(device)
    # the single-clip chains: PLMSSampler.plms_sampling / DDIMSampler.ddim_sampling over seer_cfg_plms_step / seer_cfg_ddim_step
    ref, ref_pred = [], []
    for s in range(SLOTS):
        (cf, tt), kw = solo[s], dict(cfg=True, scale=float(scale[s]), cond_f=f1)
        model = lambda lat, i: _eps_of(torch.cat([x0[s:s + 1], lat], dim=2).repeat(2, 1, 1, 1, 1), tt[i].expand(2)).contiguous()
        lat, old, pred = x_T[s:s + 1].clone(), [], None
        for index in reversed(range(lengths[s])):
            if methods[s] == "ddim":
                lat, pred = ops.cfg_ddim_step(model(lat, index), lat, cf, index, **kw)
                continue
            if not old:
                prov, _, e = ops.cfg_plms_step(model(lat, index), lat, cf, index, 0, want_pred_x0=False, **kw)
                lat, pred, _ = ops.cfg_plms_step(model(prov, max(index - 1, 0)), lat, cf, index, 1, history=[e], **kw)
            else:
                lat, pred, e = ops.cfg_plms_step(model(lat, index), lat, cf, index, len(old) + 1, history=old[::-1], **kw)
            old = (old + [e])[-3:]
        ref.append(lat), ref_pred.append(pred)
    # the slots: everything admitted up front
    x = x_T.clone()
    x_prov, pred = torch.full_like(x, NAN), torch.full_like(x, NAN)
    ring = torch.full((SLOTS, 3, C, FPK, HK, WK), NAN, device=device)
    step = torch.tensor([[n - 1, -1] for n in lengths], dtype=torch.int32, device=device)
    state = torch.tensor([[1 if m == "plms" else 0, 0, 2, 0, 0, 0, 0, 0] for m in methods], dtype=torch.int32, device=device)
    sample = torch.empty((2 * SLOTS, C, f1 + FPK, HK, WK), device=device)
    t_out = torch.empty((2 * SLOTS,), dtype=torch.long, device=device)
    calls = max(n + (m == "plms") for n, m in zip(lengths, methods))
    assert calls == 7
    for call in range(calls):
        ops.slot_plms_step_begin(x0, x, x_prov, ttab, step, state, 2, sample, t_out)
        if call == 1:                                    # the 1-entry clip's second evaluation: t_next = t, the provisional latent
            assert int(t_out[0]) == int(solo[0][1][0]) and torch.equal(sample[0, :, f1:], x_prov[0])
        ops.slot_cfg_plms_step(_eps_of(sample, t_out), x, scale, coef, step, state, ring, x_prov, cond_f=f1, x_prev=x, pred_x0=pred)
    for s in range(SLOTS):
        assert torch.equal(x[s:s + 1], ref[s]) and torch.equal(pred[s:s + 1], ref_pred[s]), s
    assert step[:, 0].tolist() == [-1] * SLOTS
    assert state[:, :3].tolist() == [[3, 1, 0], [3, 2, 1], [3, 3, 0], [0, 0, 2]]
    assert torch.isnan(ring[3]).all() and torch.isnan(x_prov[3]).all() and torch.isnan(ring[0, 1:]).all()


def test_every_refusal_returns_einval(device):
    """the same list the CPU suite runs on made-up pointers, here on one real buffer that every good argument set would fit in"""
    buf = torch.zeros(1 << 18, device=device)
    lib = _lib.load()
    n = 0
    for fn, args, why in plms_refusal_cases(buf.data_ptr()):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    assert n >= 54
    torch.cuda.synchronize()
    assert not buf.any()                                  # nothing ran


# ---- 2. the sampler on the mini UNet ---------------------------------------------------------------------------------------------
METHODS = ("plms", "ddim", "plms")


def _mixed(device):
    return [dict(r, method=m) for r, m in zip(_requests(device), METHODS)]


def _solo_mixed(device, dtype):
    """every request alone through its own sampler (launch by launch), once per storage type for the module"""
    if dtype not in _solo_plms:
        m = _model(device, dtype, layout_invariant=True)
        m.use_graph = False
        out = list(_solo_latents(device, dtype))
        for k, r in enumerate(_requests(device)):
            if METHODS[k] != "plms":
                continue
            out[k], _ = PLMSSampler(device).sample(m, r["S"], batch_size=1, shape=(4, FP, HL, HL), x0_emb=r["x0_emb"], conditioning=r["c"],
                                                   verbose=False, cond_frames=F1, unconditional_guidance_scale=r["scale"],
                                                   unconditional_conditioning=r["uc"], eta=0., x_T=r["x_T"], is_3d=True)
        _solo_plms[dtype] = out
    return _solo_plms[dtype]


def _slot_sampler(m, device, slots=2):
    return SlotSampler(m, slots, shape=(4, FP, HL, HL), cond_frames=F1, context_shape=(77, CFG_MINI["cross_attention_dim"]),
                       device=device, model_cond_frame=F1, plms=True)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("dtype", [None, torch.float16])
def test_a_slot_returns_the_bits_of_the_solo_run_of_its_sampler(device, monkeypatch, dtype, use_graph):
    """two slots, (plms S = 4, ddim S = 6, plms S = 5), the third entering when the first leaves: every latent is its solo sampler's,
    and the captured run captures ONE graph for three schedules, two scales and two methods"""
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
        got = list(smp.run(iter(_mixed(device))))
        assert m._engine.inv and m._engine.dt == (dtype or torch.bfloat16)
        mine = [k for k, G in m._engine._graphs.items() if isinstance(k, tuple) and k and k[0] == "slots-plms" and G.get("owner") is smp]
        assert (len(captures), len(mine)) == ((1, 1) if use_graph else (0, 0))
    finally:
        m.use_graph = False
    monkeypatch.setattr(torch.cuda, "CUDAGraph", real)
    assert [tag for tag, _ in got] == [0, 1, 2]          # 4 + 1, 7 and 5 + 1 steps: steps 5, 7 and 11
    assert smp._step[:, 0].tolist() == [-1, -1]
    want = _solo_mixed(device, dtype)
    for tag, lat in got:
        assert torch.isfinite(lat).all() and lat.shape == want[tag].shape
        assert torch.equal(lat, want[tag]), (tag, METHODS[tag], (lat - want[tag]).abs().max().item())
    assert not torch.equal(want[0], _solo_latents(device, dtype)[0])         # PLMS is not DDIM on the same clip


def test_captured_and_launch_by_launch_steps_agree_in_the_default_mode(device):
    m = _model(device)
    runs = {}
    try:
        for use_graph in (False, True):
            m.use_graph = use_graph
            smp = _slot_sampler(m, "cuda")
            reqs = [{k: v for k, v in r.items() if k != "tag"} for r in _mixed(device)]
            trace, finished = [], []
            for r in reqs[:2]:
                smp.submit(**r)
            for n in range(1, 12):
                live = smp.active()
                done = smp.step()
                trace.append([smp.pred_x0(s) for s in live])
                finished += [lat for _, lat in done]
                if n == 5:
                    assert [s for s, _ in done] == [0]
                    smp.submit(**reqs[2])
            assert len(finished) == 3 and smp.free_slots() == [0, 1] and not m._engine.inv
            if use_graph:
                assert any(isinstance(k, tuple) and k and k[0] == "slots-plms" and G.get("owner") is smp
                           for k, G in m._engine._graphs.items()), "the captured step never ran"
            runs[use_graph] = (trace, finished)
    finally:
        m.use_graph = False
    for a, b in zip(runs[False][1], runs[True][1]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    for n, (pa, pb) in enumerate(zip(runs[False][0], runs[True][0])):
        assert len(pa) == len(pb) and all(torch.equal(a, b) for a, b in zip(pa, pb)), n


# ---- 3. the queue -----------------------------------------------------------------------------------------------------------------
def test_generate_queue_returns_the_clips_of_generate_clips_over_plms(device):
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
                         empty_emb=empty, ddim_steps=S, scale=scale, noise=_randn((1, 4, 2, 8, 8), 70 + k), tag=f"clip{k}",
                         sampler="plms"))
    got = dict(generate_queue(unet, fst, vae, iter(reqs), slots=2, num_frames=3, cond_frames=1, plms=True,
                              latent_generator=torch.Generator(device=device).manual_seed(5)))
    assert list(got) == ["clip0", "clip1", "clip2"]     # 4 + 1 steps: step 5; 5 + 1: step 6; 4 + 1 more from step 6 on: step 10
    assert any(isinstance(k, tuple) and k and k[0] == "slots-plms" for k in unet._engine._graphs) == bool(unet.use_graph)
    lg = torch.Generator(device=device).manual_seed(5)   # the queue draws the conditioning latents in admission order: so does this loop
    for k, r in enumerate(reqs):
        want = generate_clips(unet, fst, vae, PLMSSampler(device), r["x0_image"], r["text_emb"], r["empty_emb"], num_frames=3,
                              cond_frames=1, ddim_steps=r["ddim_steps"], scale=r["scale"], num_samples=1,
                              noise_generator=torch.Generator().manual_seed(70 + k), latent_generator=lg)[0]
        clip = got[r["tag"]]
        assert clip.shape == want.shape == (1, 3, 2, 64, 64) and torch.isfinite(clip).all() and clip.min() >= 0 and clip.max() <= 1
        assert torch.equal(clip, want), (k, (clip - want).abs().max().item())
