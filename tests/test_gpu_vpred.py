"""v-prediction on a real MI355X: the conversion kernel in its three forms (seer_v_to_eps, seer_v_to_eps_dev, seer_slot_v_to_eps) --
exact on integers, against float64 on normals, the same bits from all three, nothing written for a counter outside the table or an
idle slot, the provisional latent and the row below in a PLMS slot's second evaluation; seer_velocity_target exact, against float64,
on its 16-byte and its scalar path; every refusal; then the mini UNet's output read as v: captured step against launches for DDIM,
PLMS and DPM-Solver++, a clip in a queue against its solo run under the layout-invariant mode, and step_from_batch against
forward_backward on the velocity target."""
import math

import pytest
import torch

from seervideoldm_amd import DDIMSampler, DPMSolverSampler, PLMSSampler, SeerUNet, SlotSampler, _lib, ops, synth, train_ops
from seervideoldm_amd.trainer import SeerTrainer
from tests import norm_edge_ref as N
from tests import vpred_ref as V
from tests.test_gpu_dpm import _fence_intact, _fenced, _mini_inputs
from tests.test_vpred_host import refusal_cases

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASE_IDS = lambda c: "x".join(map(str, c))
# (a_t, -, -, sqrt(1 - a_t)) with exact sqrtf(a_t): words 1 and 2 are not the conversion's and hold NaN
EXACT_COEF = [(1.0, NAN, NAN, 0.0), (1.0, NAN, NAN, 1.0), (0.25, NAN, NAN, 2.0), (0.0, NAN, NAN, 1.0)]


def _ints(shape, seed, device):
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float().to(device)


def _randn(shape, seed, device):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(device)


def _bits(a, b):
    """bit for bit, NaN included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _problem(case, reps, device, seed, exact):
    b, C, Ft, cond_f, HW = case
    make = _ints if exact else _randn
    v, x = make((reps * b, C, Ft, HW, 1), seed, device), make((b, C, Ft - cond_f, HW, 1), seed + 1, device)
    v[:, :, :cond_f] = NAN
    return v, x


def _want64(v, x, row, cond_f, reps):
    """(eps, magnitude) of the predicted frames in float64 on the CPU"""
    v, x = v.double().cpu()[:, :, cond_f:], x.double().cpu().repeat(reps, 1, 1, 1, 1)
    sa, s1m = math.sqrt(float(row[0])), float(row[3])
    return sa * v + s1m * x, sa * v.abs() + s1m * x.abs()


# ---- 1. seer_v_to_eps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("reps", [1, 2])
@pytest.mark.parametrize("case", N.CFG_CASES, ids=CASE_IDS)
def test_v_to_eps_is_exact_on_integers(device, case, reps, inplace):
    """integers in -8..8 and coefficient rows whose sqrtf and products are exact: every predicted element bit for bit; the conditioning
    frames (NaN on input) keep what was planted in the output -- the input's NaN in place, -77 out of place --; fences intact"""
    b, C, Ft, cond_f, HW = case
    coef = torch.tensor(EXACT_COEF, device=device)
    v, x = _problem(case, reps, device, 3, exact=True)
    for index, row in enumerate(EXACT_COEF):
        out, whole = _fenced(v.shape, device)
        out.copy_(v) if inplace else out.fill_(-77.0)
        got = ops.v_to_eps(out if inplace else v, x, coef, index, cond_f=cond_f, out=out)
        assert got is out and _fence_intact(whole)
        want, _ = _want64(v, x, row, cond_f, reps)
        assert torch.equal(out[:, :, cond_f:].cpu(), want.float()) and torch.equal(want.float().double(), want), (index, row)
        planted = v[:, :, :cond_f] if inplace else torch.full_like(v[:, :, :cond_f], -77.0)
        assert _bits(out[:, :, :cond_f], planted)
    fresh = ops.v_to_eps(v, x, coef, 2, cond_f=cond_f)                                   # a new tensor: the predicted frames are defined
    assert fresh.data_ptr() != v.data_ptr() and torch.equal(fresh[:, :, cond_f:].cpu(), _want64(v, x, EXACT_COEF[2], cond_f, reps)[0].float())
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            ops.v_to_eps(v, x, coef, bad, cond_f=cond_f)


@pytest.mark.parametrize("reps", [1, 2])
@pytest.mark.parametrize("case", N.CFG_CASES, ids=CASE_IDS)
def test_v_to_eps_on_normals_against_float64(device, case, reps):
    """|err| <= 5 * 2^-24 * (sqrt(a) |v| + s1m |x|) + 2^-126: sqrtf at 1 ulp (2 of 2^-24), two products and one sum; over every row of
    a real schedule, eta > 0 so that no word of a row is trivial"""
    b, C, Ft, cond_f, HW = case
    smp = DDIMSampler(device)
    smp.make_schedule(10, ddim_eta=0.5, verbose=False)
    v, x = _problem(case, reps, device, 5, exact=False)
    worst = 0.0
    for index in range(smp.ddim_coef.shape[0]):
        got = ops.v_to_eps(v, x, smp.ddim_coef, index, cond_f=cond_f)[:, :, cond_f:].double().cpu()
        want, mag = _want64(v, x, smp.ddim_coef[index].cpu(), cond_f, reps)
        bound = 5 * V.U * mag + 2.0 ** -126
        err = (got - want).abs()
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (index, float((err / bound).max()))
    print(f"[vpred] seer_v_to_eps {case} reps {reps}: worst |err| / bound {worst:.3f}")


# ---- 2. the three forms ------------------------------------------------------------------------------------------------------------------
def _slot_tables(smp, slots, device, nsched=16):
    coef = torch.zeros((slots, nsched, 4), device=device)
    coef[:, :, 0] = 1.0
    coef[:, :smp.ddim_coef.shape[0]] = smp.ddim_coef
    return coef


@pytest.mark.parametrize("case", N.CFG_CASES, ids=CASE_IDS)
def test_the_three_forms_give_the_same_bits(device, case):
    """host index, device counter and slots (a slot per batch row: rows s and slots + s read x[s], as row r reads x[r mod b]); a counter
    outside the table or an idle slot writes nothing; no step or state word changes; a slot whose IN-FLIGHT phase is 2 reads x_prov and
    the row below, whatever its next phase word says"""
    b, C, Ft, cond_f, HW = case
    smp = DDIMSampler(device)
    smp.make_schedule(10, verbose=False)
    n = smp.ddim_coef.shape[0]
    v, x = _problem(case, 2, device, 7, exact=False)
    x_prov = _randn(x.shape, 9, device)
    coef = _slot_tables(smp, b, device)
    nsched = coef.shape[1]
    for index in (0, 3, n - 1):
        want = ops.v_to_eps(v, x, smp.ddim_coef, index, cond_f=cond_f)
        step = torch.tensor([-9, index], dtype=torch.int32, device=device)
        dev = ops.v_to_eps_dev(v.clone(), x, coef[0], step, cond_f=cond_f)
        assert torch.equal(dev[:, :, cond_f:], want[:, :, cond_f:]) and step.tolist() == [-9, index]
        steps = torch.tensor([[-9, index]] * b, dtype=torch.int32, device=device)
        buf = v.clone()
        slot = ops.slot_v_to_eps(buf, x, coef, steps, cond_f=cond_f, out=buf)
        assert slot is buf and torch.equal(slot[:, :, cond_f:], want[:, :, cond_f:]) and _bits(slot[:, :, :cond_f], v[:, :, :cond_f])
        assert steps.tolist() == [[-9, index]] * b
        # with a sampler per slot: in-flight phases 0, 1, 3 read x and the row itself; phase 2 reads x_prov and the row below
        for two in range(b):
            state = torch.tensor([[2, 7, 7, 7, (0, 1, 3)[s % 3], 7, 7, 7] for s in range(b)], dtype=torch.int32, device=device)
            state[two, 4], state[two, 0] = 2, 3
            before = state.clone()
            got = ops.slot_v_to_eps(v, x, coef, steps, cond_f=cond_f, state=state, x_prov=x_prov)
            x_mixed = x.clone()
            x_mixed[two] = x_prov[two]
            below = ops.v_to_eps(v, x_mixed, smp.ddim_coef, max(index - 1, 0), cond_f=cond_f)
            for s in range(b):
                src = below if s == two else want
                for r in (s, b + s):
                    assert torch.equal(got[r, :, cond_f:], src[r, :, cond_f:]), (index, two, r)
            assert torch.equal(state, before) and steps.tolist() == [[-9, index]] * b
            if index > 0:
                assert not torch.equal(below[two, :, cond_f:], want[two, :, cond_f:])
    # outside the table: nothing is written, no word changes
    for index in (-1, -7, nsched, nsched + 5):
        step = torch.tensor([4, index], dtype=torch.int32, device=device)
        out, whole = _fenced(v.shape, device)
        out.fill_(-77.0)
        ops.v_to_eps_dev(v, x, coef[0], step, cond_f=cond_f, out=out)
        assert bool((out == -77.0).all()) and _fence_intact(whole) and step.tolist() == [4, index]
    if b > 1:                                            # slot 0 idle or beyond its table, the others running
        for index in (-1, nsched):
            steps = torch.tensor([[4, index]] + [[4, 2]] * (b - 1), dtype=torch.int32, device=device)
            state = torch.zeros((b, 8), dtype=torch.int32, device=device)
            state[0, 4] = 2
            out, whole = _fenced(v.shape, device)
            out.fill_(-77.0)
            ops.slot_v_to_eps(v, x, coef, steps, cond_f=cond_f, state=state, x_prov=x_prov, out=out)
            want = ops.v_to_eps(v, x, smp.ddim_coef, 2, cond_f=cond_f)
            for r in range(2 * b):
                if r % b == 0:
                    assert bool((out[r] == -77.0).all())
                else:
                    assert torch.equal(out[r, :, cond_f:], want[r, :, cond_f:]) and bool((out[r, :, :cond_f] == -77.0).all())
            assert _fence_intact(whole) and steps[0].tolist() == [4, index] and int(state[0, 4]) == 2 and int(state.sum()) == 2


# ---- 3. seer_velocity_target --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_row", [1028, 1029, 4, 1])
def test_velocity_target(device, per_row):
    """per_row = 4 k: the 16-byte path (257 vectors: two blocks), and the scalar path from a base that is only 4-byte aligned; 4 k + 1:
    the scalar path.  Exact on integers at table entries 0 and 1; on normals |err| <= 6 * 2^-24 * (sqrt(a) |noise| + sqrt(1 - a)
    |latents|) + 2^-126 -- sqrtf(a) and sqrtf(1 - a) at 1 ulp, the rounding of 1 - a at half its weight under the root, two products
    and the difference, at most 4.5 on either term --; timesteps outside the table are clamped into it"""
    b = 3
    acp = torch.tensor([0.0, 1.0, 0.25, 0.8125], device=device)
    t = torch.tensor([1, 0, 1], device=device)           # a = 1: the noise; a = 0: minus the latents
    lat, nz = _ints((b, per_row), 1, device), _ints((b, per_row), 2, device)
    for shifted in (False, True):
        hold = [torch.full((b * per_row + 8,), NAN, device=device) for _ in range(3)]
        # bases 16 bytes past an allocation's start, or 4 bytes past that: the latter is the scalar path at per_row % 4 == 0 too
        l_, n_, out = (h[4 + shifted:4 + shifted + b * per_row].view(b, per_row) for h in hold)
        assert (out.data_ptr() % 16 == 0) != shifted
        l_.copy_(lat), n_.copy_(nz)
        got = train_ops.velocity_target(l_, n_, t, acp, out=out)
        assert got is out and torch.isnan(hold[2][:4 + shifted]).all() and torch.isnan(hold[2][4 + shifted + b * per_row:]).all()
        assert torch.equal(out[0], nz[0]) and torch.equal(out[1], -lat[1]) and torch.equal(out[2], nz[2])
    smp = DDIMSampler("cpu")
    smp.make_schedule(10, verbose=False)
    table = smp.alphas_cumprod.to(device)
    T = table.numel()
    lat, nz = _randn((b, per_row), 3, device), _randn((b, per_row), 4, device)
    for ts in ([0, 417, T - 1], [-5, T + 3, 2 ** 40]):
        t = torch.tensor(ts, device=device)
        got = train_ops.velocity_target(lat, nz, t, table)
        want, mag = V.velocity64(lat, nz, t, table)
        bound = 6 * V.U * mag + 2.0 ** -126
        err = (got.double().cpu() - want).abs()
        assert (err <= bound).all(), float((err / bound).max())
    with pytest.raises(AssertionError):
        train_ops.velocity_target(lat, nz[:, :-1].contiguous() if per_row > 1 else nz[:2], t, table)


def test_entry_points_refuse_bad_arguments_and_launch_nothing(device):
    """real, aligned buffers: a refused call returns SEER_EINVAL and leaves every buffer as it was"""
    lib = _lib.load()
    buf = torch.full((8192,), NAN, device=device)
    words = torch.full((16,), -7, dtype=torch.int32, device=device)
    ts = torch.full((4,), 3, dtype=torch.int64, device=device)
    n = 0
    for fn, args, why in refusal_cases(buf.data_ptr(), words.data_ptr(), ts.data_ptr()):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    torch.cuda.synchronize()
    assert n >= 85 and torch.isnan(buf).all() and bool((words == -7).all()) and bool((ts == 3).all())


# ---- 4. the mini UNet's output read as v ----------------------------------------------------------------------------------------------------
SAMPLERS = {"ddim": (DDIMSampler, "step"), "plms": (PLMSSampler, "plms"), "dpm": (DPMSolverSampler, "dpm")}
_unets = {}


def _unet(device, cfg, **kw):
    """this module's own models (synthetic weights, as tests/test_gpu_dpm.py builds its one): the graphs these tests capture stay out
    of the engines whose graph caches other modules' tests count"""
    key = (tuple(sorted(cfg.items())), tuple(sorted(kw.items())))
    if key not in _unets:
        m = SeerUNet(**cfg, **kw)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg)), strict=True)
        _unets[key] = m.to(device).eval()
    return _unets[key]


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_captured_v_step_equals_the_launch_by_launch_step(device, name):
    """unet.use_graph: the conversion is one more node of the captured step.  Same bits as the launches of a fresh sampler over a whole
    sample, every pred_x0 included; the graph key ends in "v_prediction", and the eps-sampler on the same inputs captures under the
    key it always had and gives another latent"""
    cls, kind = SAMPLERS[name]
    from tests.test_dist_gpu import CFG_MINI as cfg
    m = _unet(device, cfg)
    b, Fp, H, S = 1, 2, 16, 5
    x0, c, uc, noise = (t.to(device) for t in _mini_inputs(cfg, seed=70))

    def sample(sampler, graph):
        m.use_graph = graph
        torch.manual_seed(5)
        preds = []
        lat, _ = sampler.sample(unet=m, S=S, conditioning=c, batch_size=b, shape=(4, Fp, H, H), x0_emb=x0, verbose=False,
                                unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0, x_T=noise, is_3d=True,
                                img_callback=lambda p, i: preds.append(p))
        return lat, preds, torch.rand(3, device=device)

    def keys():
        return [k for k in m._engine._graphs if isinstance(k, tuple) and k and k[0] == kind]
    try:
        want, wp, wr = sample(cls(device, prediction_type="v_prediction"), False)
        captured = cls(device, prediction_type="v_prediction")
        got, gp, gr = sample(captured, True)
        assert not captured._capture_refused and torch.isfinite(got).all()
        assert torch.equal(got, want) and torch.equal(gr, wr) and len(gp) == len(wp) == S
        assert all(torch.equal(a, b_) for a, b_ in zip(gp, wp))
        v_keys = keys()
        assert len(v_keys) == 1 and v_keys[0][-1] == "v_prediction"
        eps_lat, _, _ = sample(cls(device), True)
        both = keys()
        assert len(both) == 2 and [k for k in both if k[-1] != "v_prediction"][0] == v_keys[0][:-1]
        assert not torch.equal(eps_lat, got)
    finally:
        m.use_graph = False


@pytest.mark.parametrize("use_graph", [False, True])
def test_a_v_clip_in_a_queue_equals_its_solo_run_under_the_invariant_mode(device, use_graph):
    """SeerUNet(layout_invariant=True): two slots, three staggered requests of three schedule lengths and two scales, each latent
    torch.equal to DDIMSampler(prediction_type="v_prediction").sample of the clip alone"""
    from tests.test_gpu_slots import CFG_MINI, F1, FP, HL, _requests
    m = _unet(device, CFG_MINI, layout_invariant=True)
    reqs = _requests(device)
    m.use_graph = False
    want = []
    for r in reqs:
        lat, _ = DDIMSampler(device, prediction_type="v_prediction").sample(
            m, r["S"], batch_size=1, shape=(4, FP, HL, HL), x0_emb=r["x0_emb"], conditioning=r["c"], verbose=False, cond_frames=F1,
            unconditional_guidance_scale=r["scale"], unconditional_conditioning=r["uc"], eta=0., x_T=r["x_T"], is_3d=True)
        want.append(lat)
    m.use_graph = use_graph
    try:
        smp = SlotSampler(m, 2, shape=(4, FP, HL, HL), cond_frames=F1, context_shape=(77, CFG_MINI["cross_attention_dim"]), device=device,
                          model_cond_frame=F1, prediction_type="v_prediction")
        got = dict(smp.run(iter(reqs)))
        mine = [k for k, G in m._engine._graphs.items() if isinstance(k, tuple) and k and k[0] == "slots" and G.get("owner") is smp]
        assert len(mine) == (1 if use_graph else 0) and all(k[-1] == "v_prediction" for k in mine)
    finally:
        m.use_graph = False
    for r, w in zip(reqs, want):
        assert torch.isfinite(w).all() and torch.equal(got[r["tag"]], w), (r["tag"], (got[r["tag"]] - w).abs().max().item())


def test_step_from_batch_trains_on_the_velocity(device):
    """the trainer config of tests/test_gpu_train_batch.py: step_from_batch with "v_prediction" is forward_backward of a twin on the same
    inputs with the velocity of (the clean latents seer_train_inputs writes, the noise) as its target -- loss and both gradient
    segments bit for bit --, that target is inside the kernel's bound of the float64 formula, and the eps step differs"""
    from seervideoldm_amd import AutoencoderKL, FSTextTransformer, SeerUNet, synth
    from seervideoldm_amd.trainer import ddpm_alphas_cumprod
    from seervideoldm_amd.vae import ldm_to_diffusers_vae
    from tests.test_gpu_train_batch import B, CFG_MINI, FR, FS, HP, PIX, StubTextEncoder, T, _batch
    unet = SeerUNet(**CFG_MINI).to(device)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI), device=device), strict=True)
    fst = FSTextTransformer(num_frames=FS["num_frames"], in_channels=192, out_channels=192, n_heads=2, num_layers=1,
                            cross_attention_dim=192).to(device)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(**FS), device=device), strict=True)
    fst.set_numframe(FR)
    vae = AutoencoderKL(block_out_channels=(128, 128, 256, 256), layers_per_block=1)
    vae.load_state_dict(ldm_to_diffusers_vae(synth.synth_state_dict(synth.vae_encoder_param_shapes(
        ch=128, ch_mult=(1, 1, 2, 2), num_res_blocks=1, z_channels=4)), 4), strict=True)
    vae, text, acp, cond = vae.to(device), StubTextEncoder(device), ddpm_alphas_cumprod(T), 2
    batch, inj = _batch(61, cond, device, [0, T - 1])
    kw = dict(vae=vae, text_encoder=text, cond_frames=cond, alphas_cumprod=acp, **inj)
    tr = SeerTrainer(unet, fst, gradient_accumulation_steps=2, prediction_type="v_prediction", **HP)
    loss = tr.step_from_batch(*batch, **kw)
    model_input, noise, t, text_emb = tr.last_inputs
    frames = batch[0].to(device).permute(0, 2, 1, 3, 4).reshape(B * FR, 3, PIX, PIX)
    latents = torch.empty_like(noise)
    again = train_ops.train_inputs(vae.encode(frames).latent_dist.parameters.contiguous(), inj["posterior_noise"], noise, t,
                                   acp.to(device), cond, latents=latents)
    assert torch.equal(again, model_input)
    target = train_ops.velocity_target(latents, noise, t, acp.to(device))
    want, mag = V.velocity64(latents, noise, t, acp)
    assert ((target.double().cpu() - want).abs() <= 6 * V.U * mag + 2.0 ** -126).all()
    twin = SeerTrainer(unet, fst, gradient_accumulation_steps=2, **HP)
    loss2 = twin.forward_backward(model_input, target, t, text_emb, cond)
    assert torch.isfinite(loss).all() and torch.equal(loss, loss2)
    assert torch.equal(tr.pu.g, twin.pu.g) and torch.equal(tr.pf.g, twin.pf.g)
    eps_tr = SeerTrainer(unet, fst, gradient_accumulation_steps=2, **HP)
    assert not torch.equal(eps_tr.step_from_batch(*batch, **kw), loss) and tr.step_count == 0
