"""SlotSampler(dpm=True) on a real MI355X.  The update kernel that carries a sampler per slot, DDIM or DPM-Solver++, against the
single-clip kernels it restates, slot by slot and bit for bit (a DDIM slot, first-order and 2M slots at both index parities, the
final-step rule, an idle slot rotated through every position, NaN sentinels wherever nothing may be read or written, x_prev aliasing
x, the step and state words, a counter beyond the table, a chain walked by the kernels alone, every refusal); the sampler on the mini
UNet under the layout-invariant mode against DPMSolverSampler.sample / DDIMSampler.sample of each clip alone, torch.equal, launch by
launch and captured (one capture for four schedules, two scales, both orders and both discretisations); captured against launch by
launch in the default mode; pipeline.generate_queue(dpm=True) against generate_clips over DPMSolverSampler of each request alone."""
import pytest
import torch

from seervideoldm_amd import (AutoencoderKL, DDIMSampler, FSTextTransformer, SeerUNet, SlotSampler, _lib, ops, synth)
from seervideoldm_amd.dpm import DPMSolverSampler
from seervideoldm_amd.pipeline import generate_clips, generate_queue
from seervideoldm_amd.vae import ldm_to_diffusers_vae
from tests.test_gpu_slots import CFG_MINI, F1, FP, HL, NSCHED, _model, _randn, _requests, _solo_latents
from tests.test_slots_dpm_host import dpm_refusal_cases

pytestmark = pytest.mark.gpu

NAN = float("nan")
_solo_dpm = {}


def _same(a, b):
    """bit for bit, NaN included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dpm_tables(device, lengths, **solver):
    """per-slot tables [slots, NSCHED, ...] from DPMSolverSampler.make_schedule(S) per slot, and the per-slot samplers"""
    coef = torch.zeros((len(lengths), NSCHED, 4), device=device)
    coef[:, :, 0] = 1.0
    dpm_coef = torch.zeros((len(lengths), NSCHED, ops.DPM_ROW_WORDS), device=device)
    ttab = torch.zeros((len(lengths), NSCHED), device=device, dtype=torch.long)
    solo = []
    for s, S in enumerate(lengths):
        smp = DPMSolverSampler(device, **{k: v[s] for k, v in solver.items()})
        smp.make_schedule(S, verbose=False)
        n = smp.ddim_coef.shape[0]
        coef[s, :n], ttab[s, :n], dpm_coef[s, :n] = smp.ddim_coef, smp._t_table, smp.dpm_coef
        solo.append(smp)
    return coef, ttab, dpm_coef, solo


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
SLOTS, C, FPK, HK, WK = 4, 4, 3, 5, 5                     # HW = 25: 300 elements per slot, 256-thread blocks straddle the slots
LENGTHS = (10, 4, 6, 5)                                   # 10, 4, 7 and 5 entries
# per slot (index in flight, state words, what must run: "ddim", or the order of the DPM-Solver++ update).  Wherever the order is not
# 2 the slot's history is NaN on entry: it may not be read.
CASES = {
    # a DDIM slot (its valid words say nothing); the top entry of a DPM clip, no history; 2M with history valid for an odd index
    # (word 3 set, but the index is not 0; the even word is 0: the parity is respected); index 0 with history and word 3: first order
    "four": ((5, [1, 1, 0, 1], "ddim"), (3, [0, 0, 2, 0], 1), (3, [0, 1, 2, 1], 2), (0, [1, 1, 2, 1], 1)),
    # 2M with history valid for an even index; an order-1 sampler with history; index 0 with history and word 3 == 0: 2M to the end;
    # a sampler word outside 0..2 is DDIM
    "more": ((2, [1, 0, 2, 1], 2), (2, [1, 1, 1, 0], 1), (0, [1, 0, 2, 0], 2), (1, [1, 1, 7, 1], "ddim")),
}


@pytest.mark.parametrize("idle", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("cond_f", [0, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_slot_dpm_update_equals_the_single_clip_kernels_slot_by_slot(device, case, cond_f, idle):
    coef, _, dpm_coef, solo = _dpm_tables(device, LENGTHS)
    scale = torch.tensor([7.5, 3.0, 2.0, 5.0], device=device)
    eps = _randn((2 * SLOTS, C, cond_f + FPK, HK, WK), 1).to(device)
    x = _randn((SLOTS, C, FPK, HK, WK), 2).to(device)
    hist = _randn((SLOTS, C, FPK, HK, WK), 3).to(device)
    index, words, runs = (list(v) for v in zip(*CASES[case]))
    for s in range(SLOTS):
        if runs[s] != 2:
            hist[s] = NAN
    if idle is not None:                                  # the idle slot: a counter of -1 and NaN wherever the kernel could touch it
        index[idle] = -1
        x[idle], hist[idle] = NAN, NAN
    pair = lambda s: eps[[s, SLOTS + s]].contiguous()
    one = lambda t, s: t[s:s + 1].contiguous()
    want = {}
    for s in range(SLOTS):
        kw = dict(cfg=True, scale=float(scale[s]), cond_f=cond_f)
        if s == idle:
            continue
        if runs[s] == "ddim":
            want[s] = ops.cfg_ddim_step(pair(s), one(x, s), solo[s].ddim_coef, index[s], **kw)
        else:
            want[s] = ops.cfg_dpm_step(pair(s), one(x, s), solo[s].dpm_coef, index[s], runs[s],
                                       d_prev=one(hist, s) if runs[s] == 2 else None, **kw)
    for alias in (False, True):
        step = torch.tensor([[77, i] for i in index], dtype=torch.int32, device=device)
        state = torch.tensor(words, dtype=torch.int32, device=device)
        xs, pred = x.clone(), hist.clone()
        x_prev = xs if alias else torch.full_like(x, NAN)
        ops.slot_cfg_dpm_step(eps, xs, scale, coef, step, dpm_coef, state, cond_f=cond_f, x_prev=x_prev, pred_x0=pred)
        st, sw = step.tolist(), state.tolist()
        for s in range(SLOTS):
            if s == idle:                                 # no latent, no element of the history, no word of step or state
                assert _same(x_prev[s], x[s]) if alias else torch.isnan(x_prev[s]).all()
                assert torch.isnan(pred[s]).all() and torch.isnan(xs[s]).all() and st[s] == [77, -1] and sw[s] == words[s], (alias, s)
                continue
            assert torch.equal(x_prev[s:s + 1], want[s][0]) and torch.equal(pred[s:s + 1], want[s][1]), (alias, s, runs[s])
            assert torch.isfinite(x_prev[s]).all() and torch.isfinite(pred[s]).all() and st[s] == [index[s] - 1, index[s]], (alias, s)
            after = list(words[s])
            if runs[s] != "ddim":
                after[(index[s] - 1) & 1] = 1             # the valid word of the NEXT index's parity, and no other
            assert sw[s] == after, (alias, s)
        if not alias:
            assert _same(xs, x)
    # the orders are told apart by these inputs: a 2M slot run first order would be another latent
    for s in range(SLOTS):
        if s != idle and runs[s] == 2:
            other, _ = ops.cfg_dpm_step(pair(s), one(x, s), solo[s].dpm_coef, index[s], 1, cfg=True, scale=float(scale[s]), cond_f=cond_f)
            assert not torch.equal(other, want[s][0]), s


@pytest.mark.parametrize("beyond", [NSCHED, NSCHED + 1, 1 << 30])
def test_a_counter_beyond_the_table_writes_nothing(device, beyond):
    coef, _, dpm_coef, _ = _dpm_tables(device, LENGTHS)
    scale = torch.tensor([7.5, 3.0, 2.0, 5.0], device=device)
    eps = _randn((2 * SLOTS, C, 1 + FPK, HK, WK), 1).to(device)
    words = [[1, 1, 2, 0], [0, 0, 0, 0], [1, 1, 1, 1], [0, 1, 2, 1]]
    step = torch.tensor([[77, beyond]] * SLOTS, dtype=torch.int32, device=device)
    state = torch.tensor(words, dtype=torch.int32, device=device)
    x, pred = torch.full((SLOTS, C, FPK, HK, WK), NAN, device=device), torch.full((SLOTS, C, FPK, HK, WK), NAN, device=device)
    ops.slot_cfg_dpm_step(eps, x, scale, coef, step, dpm_coef, state, cond_f=1, x_prev=x, pred_x0=pred)
    assert torch.isnan(x).all() and torch.isnan(pred).all()
    assert step.tolist() == [[77, beyond]] * SLOTS and state.tolist() == words


def _eps_of(sample, t):
    """an elementwise model: rows of the first half are the empty-prompt rows"""
    half = sample.shape[0] // 2
    prompt = (torch.arange(sample.shape[0], device=sample.device) >= half).float().view(-1, 1, 1, 1, 1)
    return torch.sin(1.3 * sample + 0.01 * t.float().view(-1, 1, 1, 1, 1)) + 0.25 * prompt * torch.cos(sample)


def test_a_chain_walks_every_slots_schedule_and_orders(device):
    """begin -> eps(sample, t) -> update, call after call, with NO host write after the admission: DPM-Solver++ clips of 1, 2 and 4
    entries and a DDIM clip of 7, against the same chains through the single-clip kernels with the orders the host sampler chooses
    (DPMSolverSampler.step_order).  pred_x0 starts as NaN: the history is never read by a first-order step."""
    f1, methods = 1, ("dpmpp", "dpmpp", "dpmpp", "ddim")
    coef, ttab, dpm_coef, solo = _dpm_tables(device, (1, 2, 4, 6), lower_order_final=(True, False, True, True))
    lengths = [int(smp.ddim_timesteps.shape[0]) for smp in solo]
    assert lengths == [1, 2, 4, 7]
    scale = torch.tensor([7.5, 3.0, 2.0, 5.0], device=device)
    x_T = _randn((SLOTS, C, FPK, HK, WK), 7).to(device)
    x0 = _randn((SLOTS, C, f1, HK, WK), 8).to(device)
    ref, ref_pred, orders = [], [], []
    for s in range(SLOTS):
        smp, kw = solo[s], dict(cfg=True, scale=float(scale[s]), cond_f=f1)
        model = lambda lat, i: _eps_of(torch.cat([x0[s:s + 1], lat], dim=2).repeat(2, 1, 1, 1, 1), smp._t_table[i].expand(2)).contiguous()
        lat, pred, ran = x_T[s:s + 1].clone(), None, []
        for index in reversed(range(lengths[s])):
            if methods[s] == "ddim":
                lat, pred = ops.cfg_ddim_step(model(lat, index), lat, smp.ddim_coef, index, **kw)
                continue
            order = smp.step_order(index, pred is not None)
            ran.append(order)
            lat, pred = ops.cfg_dpm_step(model(lat, index), lat, smp.dpm_coef, index, order, d_prev=pred if order == 2 else None, **kw)
        ref.append(lat), ref_pred.append(pred), orders.append(ran)
    assert orders == [[1], [1, 2], [1, 2, 2, 1], []]     # lower_order_final off for the second clip, on for the third
    # the slots: everything admitted up front
    x, pred = x_T.clone(), torch.full_like(x_T, NAN)
    step = torch.tensor([[n - 1, -1] for n in lengths], dtype=torch.int32, device=device)
    state = torch.tensor([[0, 0, 2 if m == "dpmpp" else 0, int(m == "dpmpp" and smp._final_first_order())]
                          for m, smp in zip(methods, solo)], dtype=torch.int32, device=device)
    assert state.tolist() == [[0, 0, 2, 1], [0, 0, 2, 0], [0, 0, 2, 1], [0, 0, 0, 0]]
    sample = torch.empty((2 * SLOTS, C, f1 + FPK, HK, WK), device=device)
    t_out = torch.empty((2 * SLOTS,), dtype=torch.long, device=device)
    for call in range(max(lengths)):
        ops.slot_step_begin(x0, x, ttab, step, 2, sample, t_out)
        ops.slot_cfg_dpm_step(_eps_of(sample, t_out), x, scale, coef, step, dpm_coef, state, cond_f=f1, x_prev=x, pred_x0=pred)
    for s in range(SLOTS):
        assert torch.equal(x[s:s + 1], ref[s]) and torch.equal(pred[s:s + 1], ref_pred[s]), s
    assert step[:, 0].tolist() == [-1] * SLOTS
    assert state.tolist() == [[0, 1, 2, 1], [1, 1, 2, 0], [1, 1, 2, 1], [0, 0, 0, 0]]


def test_every_refusal_returns_einval(device):
    """the same list the CPU suite runs on made-up pointers, here on one real NaN-filled buffer that every good argument set would fit
    in: the error comes back and no word of the buffer changes"""
    buf = torch.full((1 << 18,), NAN, device=device)
    lib = _lib.load()
    n = 0
    for args, why in dpm_refusal_cases(buf.data_ptr()):
        assert lib.seer_slot_cfg_dpm_step(*args, None) == -22, why
        n += 1
    assert n >= 32
    torch.cuda.synchronize()
    assert _same(buf, torch.full_like(buf, NAN))          # nothing ran


# ---- 2. the sampler on the mini UNet ---------------------------------------------------------------------------------------------
# (method, S, the solver keywords of a "dpmpp" request): 4, 7, 5 and 6 entries, both orders, both discretisations
MIXED = (("dpmpp", 4, dict()), ("ddim", 6, dict()), ("dpmpp", 5, dict(order=1, discretize="logsnr")),
         ("dpmpp", 6, dict(discretize="logsnr", lower_order_final=False)))


def _mixed(device):
    """the three requests of tests/test_gpu_slots.py and a fourth on the second's prompt and scale with a start code of its own"""
    reqs = _requests(device)
    reqs.append(dict(reqs[1], x_T=_randn((1, 4, FP, HL, HL), 33).to(device), tag=3))
    return [dict(r, S=S, method=m, **solver) for r, (m, S, solver) in zip(reqs, MIXED)]


def _solo_mixed(device, dtype):
    """every request alone through its own sampler (launch by launch), once per storage type for the module"""
    if dtype not in _solo_dpm:
        m = _model(device, dtype, layout_invariant=True)
        m.use_graph = False
        out = []
        for k, r in enumerate(_mixed(device)):
            if MIXED[k][0] == "ddim":
                out.append(_solo_latents(device, dtype)[k])
                continue
            lat, _ = DPMSolverSampler(device, **MIXED[k][2]).sample(
                m, r["S"], batch_size=1, shape=(4, FP, HL, HL), x0_emb=r["x0_emb"], conditioning=r["c"], verbose=False, cond_frames=F1,
                unconditional_guidance_scale=r["scale"], unconditional_conditioning=r["uc"], eta=0., x_T=r["x_T"], is_3d=True)
            out.append(lat)
        _solo_dpm[dtype] = out
    return _solo_dpm[dtype]


def _slot_sampler(m, device, slots=2):
    return SlotSampler(m, slots, shape=(4, FP, HL, HL), cond_frames=F1, context_shape=(77, CFG_MINI["cross_attention_dim"]),
                       device=device, model_cond_frame=F1, dpm=True)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("dtype", [None, torch.float16])
def test_a_slot_returns_the_bits_of_the_solo_run_of_its_sampler(device, monkeypatch, dtype, use_graph):
    """two slots, four requests, each entering when one leaves: every latent is its solo sampler's, and the captured run captures
    ONE graph for four schedule lengths, two scales, both orders and both discretisations"""
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
        mine = [k for k, G in m._engine._graphs.items() if isinstance(k, tuple) and k and k[0] == "slots-dpm" and G.get("owner") is smp]
        assert (len(captures), len(mine)) == ((1, 1) if use_graph else (0, 0))
    finally:
        m.use_graph = False
    monkeypatch.setattr(torch.cuda, "CUDAGraph", real)
    assert [tag for tag, _ in got] == [0, 1, 2, 3]       # 4, 7, 5 and 6 entries in two slots: steps 4, 7, 9 and 13
    assert smp._step[:, 0].tolist() == [-1, -1]
    want = _solo_mixed(device, dtype)
    for tag, lat in got:
        assert torch.isfinite(lat).all() and lat.shape == want[tag].shape
        assert torch.equal(lat, want[tag]), (tag, MIXED[tag], (lat - want[tag]).abs().max().item())
    assert not torch.equal(want[0], _solo_latents(device, dtype)[0])         # 2M is not DDIM on the same clip


# How far a default-mode slot may be from its solo run.  tests/test_gpu_slots.py, which the default-mode comparison was to take its
# bound from, holds none, so this one is derived, from bounds the suite already holds and not from what the slots give.  Slot and
# solo run are two bf16 evaluations of ONE exact chain -- the same sampler, schedule, start code, prompt and scale on the same
# weights; only the batch layout of the UNet's kernels differs (a row of 2 x slots rows against a row of 2), and with it the order of
# their bf16 accumulations.  On this model at guidance 7.5 the suite holds a sampler's latent to rel_l2 <= 8e-2 of the exact chain
# (the float64 restatement over the oracle) after S = 10 steps: tests/test_gpu_dpm.py::test_dpm_sampler_matches_oracle for this
# solver, tests/test_gpu_plms.py for PLMS.  The chains here are shorter (4 to 7 entries) and at guidance 7.5 or 3, so each of the two
# runs is inside that bound of the exact latent r, and by the triangle inequality |slot - solo| <= 2 * 8e-2 |r|, with |solo| >=
# (1 - 8e-2) |r|.  Unrelated latents are about 1.4 apart on this scale.
SOLO_BOUND = 2 * 8e-2 / (1 - 8e-2)


def test_captured_and_launch_by_launch_steps_agree_in_the_default_mode(device):
    """Captured against launch by launch: the same bits, every step's pred_x0 included.  Then every clip against its solo sampler on
    the same default-mode model, within SOLO_BOUND (measured on an MI355X: rel_l2 0.036 for 2M at S = 4, 0.044 for first order on the
    log-SNR grid at S = 5, 0.019 for 2M on it at S = 6)."""
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
            for n in range(1, 14):
                live = smp.active()
                done = smp.step()
                trace.append([smp.pred_x0(s) for s in live])
                finished += [lat for _, lat in done]
                if n in (4, 7):
                    assert [s for s, _ in done] == [0 if n == 4 else 1]
                    smp.submit(**reqs[2 if n == 4 else 3])
            assert len(finished) == 4 and smp.free_slots() == [0, 1] and not m._engine.inv
            if use_graph:
                assert any(isinstance(k, tuple) and k and k[0] == "slots-dpm" and G.get("owner") is smp
                           for k, G in m._engine._graphs.items()), "the captured step never ran"
            runs[use_graph] = (trace, finished)
    finally:
        m.use_graph = False
    for a, b in zip(runs[False][1], runs[True][1]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    for n, (pa, pb) in enumerate(zip(runs[False][0], runs[True][0])):
        assert len(pa) == len(pb) and all(torch.equal(a, b) for a, b in zip(pa, pb)), n
    # Against the solo run: not its bits in this mode, but within SOLO_BOUND.  Clips finish in request order (steps 4, 7, 9, 13).
    for k, (r, lat) in enumerate(zip(_mixed(device), runs[True][1])):
        solo_sampler = DPMSolverSampler(device, **MIXED[k][2]) if MIXED[k][0] == "dpmpp" else DDIMSampler(device)
        solo, _ = solo_sampler.sample(
            m, r["S"], batch_size=1, shape=(4, FP, HL, HL), x0_emb=r["x0_emb"], conditioning=r["c"], verbose=False, cond_frames=F1,
            unconditional_guidance_scale=r["scale"], unconditional_conditioning=r["uc"], eta=0., x_T=r["x_T"], is_3d=True)
        rel = ((lat.double() - solo.double()).norm() / solo.double().norm()).item()
        print(f"[slots-dpm] default mode, request {k} {MIXED[k]}: rel_l2 to its solo sampler {rel:.3g} (bound {SOLO_BOUND:.3g})")
        assert torch.isfinite(solo).all() and lat.shape == solo.shape
        assert rel <= SOLO_BOUND, (k, MIXED[k], rel)


# ---- 3. the queue -----------------------------------------------------------------------------------------------------------------
def test_generate_queue_returns_the_clips_of_generate_clips_over_dpm(device):
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
    solvers = (dict(), dict(order=1), dict(discretize="logsnr", lower_order_final=False))
    reqs = []
    for k, (S, scale) in enumerate(((4, 7.5), (5, 3.0), (4, 7.5))):
        reqs.append(dict(x0_image=torch.tanh(_randn((1, 3, 1, 64, 64), 50 + k)).to(device), text_emb=_randn((1, 77, 192), 60 + k % 2).to(device),
                         empty_emb=empty, ddim_steps=S, scale=scale, noise=_randn((1, 4, 2, 8, 8), 70 + k), tag=f"clip{k}",
                         sampler="dpmpp", **solvers[k]))
    got = dict(generate_queue(unet, fst, vae, iter(reqs), slots=2, num_frames=3, cond_frames=1, dpm=True,
                              latent_generator=torch.Generator(device=device).manual_seed(5)))
    assert list(got) == ["clip0", "clip1", "clip2"]     # 4 entries: step 4; 5 entries: step 5; 4 more from step 5 on: step 8
    assert any(isinstance(k, tuple) and k and k[0] == "slots-dpm" for k in unet._engine._graphs) == bool(unet.use_graph)
    lg = torch.Generator(device=device).manual_seed(5)   # the queue draws the conditioning latents in admission order: so does this loop
    for k, r in enumerate(reqs):
        want = generate_clips(unet, fst, vae, DPMSolverSampler(device, **solvers[k]), r["x0_image"], r["text_emb"], r["empty_emb"],
                              num_frames=3, cond_frames=1, ddim_steps=r["ddim_steps"], scale=r["scale"], num_samples=1,
                              noise_generator=torch.Generator().manual_seed(70 + k), latent_generator=lg)[0]
        clip = got[r["tag"]]
        assert clip.shape == want.shape == (1, 3, 2, 64, 64) and torch.isfinite(clip).all() and clip.min() >= 0 and clip.max() <= 1
        assert torch.equal(clip, want), (k, (clip - want).abs().max().item())
