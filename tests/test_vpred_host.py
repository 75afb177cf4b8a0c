"""v-prediction without a GPU, on the torch stand-ins (tests/vpred_ref.py in front of the existing tests/*_ref.py modules): a v-sampler
on the analytic v-model against the pinned eps-sampler on the eps-model it was made from, within a rounding allowance worked out in
float64; where the conversion is launched and with what; slots against solo runs; the trainer's velocity target; the refusals, the
compat switch and the entry points' own refusals.  Runs everywhere (CPU)."""
import inspect

import pytest
import torch

from seervideoldm_amd import DDIMSampler, DPMSolverSampler, PLMSSampler, SlotSampler, compat, pipeline
from tests import dpm_ref as D
from tests import slot_dpm_ref, slot_plms_ref, slot_ref, stoch_ref
from tests import vpred_ref as V
from tests.test_slots_host import C as SC, F1 as SF1, FP as SFP, H as SH, W as SW, _Gaussian

f64 = torch.float64
OPS = V.backend(D)                                       # dpm_ref re-exports the DDIM, seeded, masked and inversion stand-ins
B, CH, FP, H, W, S, SCALE = 2, 3, 3, 4, 5, 10, 7.5
SEED, ETA = 7, 0.5
# (method, sampler class, constructor keywords, sample keywords)
SAMPLERS = {"ddim": (DDIMSampler, {}, {}), "ddim-eta": (DDIMSampler, {}, dict(eta=ETA, seed=SEED)), "plms": (PLMSSampler, {}, {}),
            "dpm-uniform": (DPMSolverSampler, dict(discretize="uniform"), {}),
            "dpm-logsnr": (DPMSolverSampler, dict(discretize="logsnr"), {})}
# roundings per quantity, counted from the fp32 operations that make it (the docstring of test_v_sampler_reproduces_the_eps_sampler)
K_E = {"epsilon": 4, "v_prediction": 8}
K_X = {"ddim": 12, "plms": 20, "dpm": 8}
K_P, K_D = 12, 3


def _sampler(name, prediction_type, ops=OPS, **kw):
    cls, ckw, _ = SAMPLERS[name]
    smp = cls("cpu", ops=ops, prediction_type=prediction_type, **ckw, **kw)
    smp.make_schedule(S, ddim_eta=SAMPLERS[name][2].get("eta", 0.), verbose=False)
    return smp


def _problem(f1, seed=1):
    g = torch.Generator().manual_seed(seed)
    shift = 0.2 * torch.randn((B, CH, FP, H, W), generator=g, dtype=f64)
    x_T = torch.randn((B, CH, FP, H, W), generator=g)
    x0_emb = torch.randn((B, CH, f1, H, W), generator=g) if f1 else None
    return shift, x_T, x0_emb, torch.zeros((B, f1 + FP, 1, 1))


def _models(smp, shift, f1, cfg):
    """E(x, t) of tests/dpm_ref.py -- the conditional rows see the data mean moved by `shift` -- and V(x, t) = (E - sqrt(1 - a) x) /
    sqrt(a), both as the Python model a sampler calls (float64 inside, fp32 out, zeros in the conditioning frames) and as the rows
    tests/vpred_ref.chain64 reads.  -> {prediction_type: (model, model_rows)}"""
    eps, _ = D.gaussian(smp.alphas_cumprod)
    ac, ts = smp.alphas_cumprod.double(), smp.ddim_timesteps

    def out64(lat, t, off, prediction_type):
        e = eps(lat - off, t)
        if prediction_type == "epsilon":
            return e
        a = ac[t.long()].view(-1, 1, 1, 1, 1)
        return (e - (1 - a).sqrt() * lat) / a.sqrt()

    def pair(prediction_type):
        def model(x, t, c, cond_frame=0):
            lat = x[:, :, f1:].double()
            off = torch.cat([torch.zeros_like(shift), shift]) if x.shape[0] == 2 * B else shift
            return torch.cat([torch.zeros_like(x[:, :, :f1]), out64(lat, t, off, prediction_type).float()], 2)

        def rows(x, row):
            t = torch.full((B,), int(ts[row]), dtype=torch.long)
            offs = (torch.zeros_like(shift), shift) if cfg else (shift,)
            return tuple(out64(x, t, off, prediction_type) for off in offs)
        return model, rows
    return {p: pair(p) for p in ("epsilon", "v_prediction")}


def _chain64(name, smp, x_T, rows, prediction_type, cfg, bump=None):
    method = name.split("-")[0]
    kw = {}
    if method == "dpm":
        n = smp.ddim_coef.shape[0]
        kw = dict(dpm_coef=smp.dpm_coef, orders=[smp.step_order(i, k > 0) for k, i in enumerate(reversed(range(n)))])
    if name == "ddim-eta":
        def noise(index):                                # the fp32 normals the seeded stand-in draws, row bi from seed SEED + bi
            per = x_T[0].numel()
            return torch.stack([stoch_ref.philox_normal(SEED + bi, 1, index, per).reshape(x_T[0].shape) for bi in range(B)]).double()
        kw = dict(noise=noise)
    return V.chain64(method, smp.ddim_coef, x_T, rows, prediction_type, SCALE if cfg else 1.0, bump=bump, **kw)


def _allowance(name, smp, x_T, rows, prediction_type, cfg):
    """-> (the float64 latent, sum over the chain's fp32 quantities of |d latent / d quantity| * roundings * 2^-24 * magnitude)"""
    base, marks = _chain64(name, smp, x_T, rows, prediction_type, cfg)
    method = name.split("-")[0]
    k_of = {"e": K_E[prediction_type], "x": K_X[method], "p": K_P, "d": K_D}
    total = torch.zeros_like(base)
    for what, k, mag in marks:
        bumped, _ = _chain64(name, smp, x_T, rows, prediction_type, cfg, bump=(what, k))
        total += (bumped - base).abs() * k_of[what] * V.U * mag           # the chain is affine in every quantity: an exact derivative
    return base, total


@pytest.mark.parametrize("f1", [0, 2])
@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_v_sampler_reproduces_the_eps_sampler(name, cfg, f1):
    """S = 10, b = 2.  The eps path is the yardstick (goldens pin it to the reference); the v-sampler on V must land where the
    eps-sampler lands on E, per element within
        |x64(V) - x64(E)|  +  sum over both fp32 chains, over every quantity q a chain rounds, of |d x_final / d q| k_q 2^-24 M_q
    x64: the same chain in float64 (tests/vpred_ref.chain64: V is made with sqrt(1 - a) in float64, the conversion reads the table's
    fp32 word, so the two float64 chains differ by a few 2^-24 of their own); d x_final / d q: exact, from a unit bump of q in the
    float64 chain, which is affine in each of them; M_q: the sum of the magnitudes of q's operands (for a CFG pair as
    cfg_ddim_allowance of tests/norm_edge_ref.py sums them); k_q, the roundings that make q, counted from the operations:
      e, an evaluation's CFG-combined eps    eps-model 4: the model's fp32 output, the pair's difference, product and sum
                                             v-model   8: that, and sqrtf(a_t), the two products and the sum of the conversion
      x, a DDIM update                       12, cfg_ddim_allowance's count (sigma * noise included)
      x, a PLMS update                       20: the 12, and at most 4 products, 3 sums and a division for e'
      p, PLMS' provisional latent            12
      x, a DPM-Solver++ update               8: s e, x - ., . / alpha for D, three products and two sums
      d, the D a 2M step hands on            3
    plus 2^-126."""
    shift, x_T, x0_emb, c = _problem(f1)
    cls, ckw, skw = SAMPLERS[name]
    got, x64, allow = {}, {}, {}
    for p in ("epsilon", "v_prediction"):
        smp = _sampler(name, p)
        model, rows = _models(smp, shift, f1, cfg)[p]
        kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=torch.ones_like(c), cond_frames=f1) if cfg else {}
        got[p] = smp.sample(model, S, B, (CH, FP, H, W), x0_emb=x0_emb, conditioning=c, x_T=x_T, verbose=False, is_3d=True, **skw,
                            **kw)[0]
        x64[p], allow[p] = _allowance(name, smp, x_T, rows, p, cfg)
        assert got[p].dtype == torch.float32 and torch.isfinite(got[p]).all()
        assert ((got[p].double() - x64[p]).abs() <= allow[p] + 2.0 ** -126).all(), p       # each fp32 chain is the restated one
    bound = (x64["v_prediction"] - x64["epsilon"]).abs() + allow["epsilon"] + allow["v_prediction"] + 2.0 ** -126
    err = (got["v_prediction"].double() - got["epsilon"].double()).abs()
    print(f"[vpred] {name} cfg={cfg} f1={f1}: max |v - eps| = {err.max():.3g}, worst err / allowance = {(err / bound).max():.3g}, "
          f"largest allowance = {bound.max():.3g}, float64 difference = {(x64['v_prediction'] - x64['epsilon']).abs().max():.3g}")
    assert (err <= bound).all()
    # the allowance has teeth: a v-sampler that is handed eps (or the wrong row) is far outside it
    wrong = _sampler(name, "v_prediction").sample(_models(_sampler(name, "epsilon"), shift, f1, cfg)["epsilon"][0], S, B,
                                                   (CH, FP, H, W), x0_emb=x0_emb, conditioning=c, x_T=x_T, verbose=False, is_3d=True,
                                                   **skw, **kw)[0]
    assert ((wrong.double() - got["epsilon"].double()).abs() > bound).any()


# ---- where the conversion is launched ---------------------------------------------------------------------------------------------------
class _Recording:
    """a backend with every call of a step-boundary entry written down as (name, arguments, keywords); the model logs itself as "unet" """

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if not (name.startswith(("cfg_", "slot_", "v_to_eps", "ddim_step")) and callable(fn)):
            return fn

        def recorded(*a, **kw):
            self.calls.append((name, a, kw))
            out = fn(*a, **kw)
            self.calls[-1] += (out,)
            return out
        return recorded

    def names(self):
        return [c[0] for c in self.calls]


def _recorded_sample(name, prediction_type, cfg=True, f1=2):
    rec = _Recording(OPS)
    smp = _sampler(name, prediction_type, ops=rec)
    shift, x_T, x0_emb, c = _problem(f1)
    inner = _models(smp, shift, f1, cfg)[prediction_type][0]

    def model(x, t, cc, cond_frame=0):
        rec.calls.append(("unet", (x, t), {}, None))
        return inner(x, t, cc, cond_frame)
    kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=torch.ones_like(c), cond_frames=f1) if cfg else {}
    smp.sample(model, S, B, (CH, FP, H, W), x0_emb=x0_emb, conditioning=c, x_T=x_T, verbose=False, is_3d=True, **SAMPLERS[name][2], **kw)
    return smp, rec


STEP_ENTRY = {"ddim": "cfg_ddim_step", "ddim-eta": "cfg_ddim_step_rng", "plms": "cfg_plms_step", "dpm-uniform": "cfg_dpm_step",
              "dpm-logsnr": "cfg_dpm_step"}


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_epsilon_launches_no_conversion_and_v_exactly_one_per_evaluation(name):
    smp, rec = _recorded_sample(name, "epsilon")
    n = smp.ddim_coef.shape[0]
    evals = n + 1 if name == "plms" else n
    assert rec.names() == ["unet", STEP_ENTRY[name]] * evals
    smp, rec = _recorded_sample(name, "v_prediction")
    assert rec.names() == ["unet", "v_to_eps", STEP_ENTRY[name]] * evals
    conv = [c for c in rec.calls if c[0] == "v_to_eps"]
    steps = [c for c in rec.calls if c[0] == STEP_ENTRY[name]]
    rows = [int(c[1][3]) for c in conv]
    want = [n - 1, max(n - 2, 0)] + list(reversed(range(n - 1))) if name == "plms" else list(reversed(range(n)))
    assert rows == want
    for k, (cv, st) in enumerate(zip(conv, steps)):
        assert cv[1][2] is smp.ddim_coef and cv[2] == dict(cond_f=2)
        assert st[1][0] is cv[3]                         # the step entry reads what the conversion returned
        assert cv[1][0].shape[0] == 2 * B and torch.isnan(cv[3][:, :, :2]).all()           # nobody needed the conditioning frames
        if name == "plms" and k == 1:
            assert cv[1][1] is steps[0][3][0] and st[1][1] is not cv[1][1]                  # converted at x_prov, applied to x
        else:
            assert cv[1][1] is st[1][1]                  # converted at the latent the step updates
    # without CFG: one row per clip
    _, rec = _recorded_sample(name, "v_prediction", cfg=False, f1=0)
    assert rec.names() == ["unet", "v_to_eps", STEP_ENTRY[name]] * evals
    assert all(c[1][0].shape[0] == B and c[2] == dict(cond_f=0) for c in rec.calls if c[0] == "v_to_eps")


# ---- slots --------------------------------------------------------------------------------------------------------------------------------
class _VGaussian(_Gaussian):
    """tests/test_slots_host.py's per-request Gaussian model, predicting v: (eps - sqrt(1 - a) x) / sqrt(a) of every row, in float64"""

    def exact(self, x, t, mu):
        a = self.ac[int(t)]
        return (super().exact(x, t, mu) - (1 - a).sqrt() * x) / a.sqrt()


def _slot_request(model, k, seed, S_, scale, **kw):
    g = torch.Generator().manual_seed(seed)
    return dict(x_T=torch.randn((1, SC, SFP, SH, SW), generator=g), x0_emb=0.9 * torch.randn((1, SC, SF1, SH, SW), generator=g),
                c=model.context(k, True), uc=model.context(k, False), S=S_, scale=scale, tag=k, **kw)


def _solo(model, r, prediction_type="v_prediction"):
    method = r.get("method", "ddim")
    cls = {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp": DPMSolverSampler}[method]
    ckw = {k: r[k] for k in ("order", "lower_order_final", "discretize") if k in r}
    smp = cls("cpu", ops=OPS, prediction_type=prediction_type, **ckw)
    smp.consume_rng_when_deterministic = False
    return smp.sample(model, r["S"], 1, (SC, SFP, SH, SW), x0_emb=r["x0_emb"], conditioning=r["c"][None], x_T=r["x_T"], verbose=False,
                      is_3d=True, unconditional_guidance_scale=r["scale"], unconditional_conditioning=r["uc"][None])[0]


@pytest.mark.parametrize("mode", ["plms", "dpm"])
def test_a_v_clip_in_a_queue_equals_its_solo_run_bit_for_bit(mode):
    """2 slots, three staggered requests: a DDIM clip beside a PLMS clip (a queue built with plms=True), and a DDIM clip beside two
    DPM-Solver++ clips, 2M on the log-SNR grid and first order (one built with dpm=True; the two samplers do not share a queue).  On the
    stand-ins the slot forms and the solo forms are one torch expression per element, so a clip's latent has the solo run's bits."""
    model = _VGaussian(3)
    if mode == "plms":
        reqs = [_slot_request(model, 0, 21, 4, 7.5, method="plms"), _slot_request(model, 1, 22, 6, 3.0),
                _slot_request(model, 2, 23, 1, 5.0, method="plms")]
        ref = slot_plms_ref
    else:
        reqs = [_slot_request(model, 0, 21, 5, 7.5, method="dpmpp", discretize="logsnr"), _slot_request(model, 1, 22, 6, 3.0),
                _slot_request(model, 2, 23, 4, 5.0, method="dpmpp", order=1)]
        ref = slot_dpm_ref
    rec = _Recording(V.backend(ref))
    smp = SlotSampler(model, 2, shape=(SC, SFP, SH, SW), cond_frames=SF1, context_shape=(1, 2), device="cpu", ops=rec,
                      prediction_type="v_prediction", **{mode: True})
    got = dict(smp.run(iter(reqs)))
    assert sorted(got) == [0, 1, 2]
    for r in reqs:
        want = _solo(model, r)
        assert torch.equal(got[r["tag"]], want), (mode, r["tag"], (got[r["tag"]] - want).abs().max())
        assert not torch.equal(want, _solo(model, r, "epsilon"))
    names = rec.names()
    begin, update = ("slot_plms_step_begin", "slot_cfg_plms_step") if mode == "plms" else ("slot_step_begin", "slot_cfg_dpm_step")
    assert names == [begin, "slot_v_to_eps", update] * (len(names) // 3)
    conv = [c for c in rec.calls if c[0] == "slot_v_to_eps"]
    assert all(c[2]["out"] is c[1][0] and c[2]["cond_f"] == SF1 and (("state" in c[2]) == (mode == "plms")) for c in conv)
    # the same queue on an eps-model: no conversion anywhere
    rec = _Recording(V.backend(ref))
    eps_model = _Gaussian(3)
    smp = SlotSampler(eps_model, 2, shape=(SC, SFP, SH, SW), cond_frames=SF1, context_shape=(1, 2), device="cpu", ops=rec, **{mode: True})
    got = dict(smp.run(iter(reqs)))
    assert "slot_v_to_eps" not in rec.names() and all(torch.equal(got[r["tag"]], _solo(eps_model, r, "epsilon")) for r in reqs)


def test_generate_queue_hands_the_prediction_type_on(monkeypatch):
    import seervideoldm_amd.slots as slots
    seen = {}

    class _Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise _Stop
    monkeypatch.setattr(slots, "SlotSampler", fake)
    monkeypatch.setattr(pipeline, "frames_to_latents", lambda vae, x, g: torch.zeros((1, 4, 1, 2, 2)))
    fst = type("F", (), {"set_numframe": lambda self, n: None, "__call__": lambda self, context: torch.zeros((1, 3, 2, 3))})()
    req = dict(x0_image=torch.zeros((1, 3, 1, 16, 16)), text_emb=torch.zeros((1, 2, 3)), empty_emb=torch.zeros((1, 2, 3)),
               noise=torch.zeros((1, 4, 2, 2, 2)))
    for ptype, want in (("v_prediction", "v_prediction"), ("epsilon", None)):
        seen.clear()
        with pytest.raises(_Stop):
            list(pipeline.generate_queue(None, fst, None, [req], slots=2, num_frames=3, cond_frames=1, prediction_type=ptype))
        assert seen.get("prediction_type") == want


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_models():
    from seervideoldm_amd import FSTextTransformer, SeerUNet, synth
    from tests.test_train_batch_cpu import CFG, FS
    unet = SeerUNet(**CFG)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG)), strict=True)
    fst = FSTextTransformer(num_frames=FS["num_frames"], in_channels=192, out_channels=192, n_heads=2, num_layers=1, cross_attention_dim=192)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(**FS)), strict=True)
    return unet, fst


def _trainer(train_models, Fr, prediction_type, tops=None):
    """gradient_accumulation_steps = 2: the call under test back-propagates and does not step, so two trainers stay comparable"""
    from seervideoldm_amd.trainer import SeerTrainer
    from tests import torch_ops_backend as tob
    from tests.test_train_batch_cpu import HP
    unet, fst = train_models
    fst.set_numframe(Fr)
    tops = V.train_ops() if tops is None else tops
    return SeerTrainer(unet, fst, ops=tob, tops=tops, gradient_accumulation_steps=2, prediction_type=prediction_type, **HP), tops


def _hand_velocity(latents, noise, t, acp):
    a = acp[t].view(-1, 1, 1, 1, 1)
    return a.sqrt() * noise - (1 - a).sqrt() * latents


def test_trainer_passes_the_velocity_to_the_unchanged_forward_backward(train_models):
    from seervideoldm_amd.trainer import ddpm_alphas_cumprod
    from tests.test_train_batch_cpu import _Text, _Vae, _batch
    from tests.train_inputs_ref import reference
    b, Fr, cond = 1, 3, 1
    acp = ddpm_alphas_cumprod()
    video, ids, mask = _batch(b, Fr, 1)
    table = torch.randn((8, 77, 192), generator=torch.Generator().manual_seed(4))
    runs = {}
    for p in ("epsilon", "v_prediction"):                 # nothing injected: every draw is the trainer's own
        tr, tops = _trainer(train_models, Fr, p)
        torch.manual_seed(31)
        loss = tr.step_from_batch(video, ids, mask, vae=_Vae([]), text_encoder=_Text([], table), cond_frames=cond, alphas_cumprod=acp)
        runs[p] = (tr, tops, loss, torch.get_rng_state())
    tr_e, tops_e, loss_e, rng_e = runs["epsilon"]
    tr_v, tops_v, loss_v, rng_v = runs["v_prediction"]
    assert torch.equal(rng_e, rng_v)                     # the draws and their order did not change
    assert tops_e.velocity_calls == [] and len(tops_v.velocity_calls) == 1 and len(tops_v.calls) == 1
    for a, b_ in zip(tr_e.last_inputs, tr_v.last_inputs):
        assert torch.equal(a, b_)
    model_input, noise, t, text = tr_v.last_inputs
    call = tops_v.calls[0]
    latents = reference(_Vae([]).encode(video.permute(0, 2, 1, 3, 4).reshape(b * Fr, 3, 64, 64)).latent_dist.parameters, call["eps_post"],
                        noise, t, acp, cond, 0.18215)[1].float()
    assert torch.equal(tops_v.velocity_calls[0][0], latents) and tops_v.velocity_calls[0][1] is noise
    target = _hand_velocity(latents, noise, t, acp)
    ref, _ = _trainer(train_models, Fr, "epsilon")
    want = ref.forward_backward(model_input, target, t, text, cond)
    assert torch.equal(loss_v, want) and not torch.equal(loss_v, loss_e)
    assert torch.equal(tr_v.pu.g, ref.pu.g) and torch.equal(tr_v.pf.g, ref.pf.g) and not torch.equal(tr_v.pu.g, tr_e.pu.g)
    # train_step, from latents
    g = torch.Generator().manual_seed(6)
    lat_x0, lat, nz = (torch.randn((b, 4, n, 8, 8), generator=g) for n in (cond, Fr - cond, Fr - cond))
    t2 = torch.tensor([612])
    tv, tops2 = _trainer(train_models, Fr, "v_prediction")
    state = torch.get_rng_state()
    loss2 = tv.train_step(lat_x0, lat, nz, t2, text, acp)
    assert torch.equal(torch.get_rng_state(), state) and len(tops2.velocity_calls) == 1
    a = acp[t2].view(-1, 1, 1, 1, 1)
    x = torch.cat([lat_x0, a.sqrt() * lat + (1 - a).sqrt() * nz], 2)
    ref2, _ = _trainer(train_models, Fr, "epsilon")
    assert torch.equal(loss2, ref2.forward_backward(x, _hand_velocity(lat, nz, t2, acp), t2, text, cond))
    assert torch.equal(tv.pu.g, ref2.pu.g) and torch.equal(tv.pf.g, ref2.pf.g)


def test_trainer_backend_without_velocity_target_fails_only_for_v(train_models):
    from tests.train_inputs_ref import TrainOpsWithInputs
    tr, _ = _trainer(train_models, 3, "epsilon", tops=TrainOpsWithInputs())
    assert tr.prediction_type == "epsilon"
    with pytest.raises(ValueError, match="velocity_target"):
        _trainer(train_models, 3, "v_prediction", tops=TrainOpsWithInputs())
    with pytest.raises(ValueError, match="Unknown prediction type sample"):
        _trainer(train_models, 3, "sample")


# ---- refusals, the surface, compat --------------------------------------------------------------------------------------------------------
def test_unknown_prediction_type_and_inversion_are_refused():
    for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler):
        assert cls("cpu").prediction_type == "epsilon"
        for bad in ("sample", "V_PREDICTION", "", None):
            with pytest.raises(ValueError, match="Unknown prediction type"):
                cls("cpu", prediction_type=bad)
    model = _Gaussian(1)
    for bad in ("sample", "eps"):
        with pytest.raises(ValueError, match=f"Unknown prediction type {bad}"):
            SlotSampler(model, 2, shape=(SC, SFP, SH, SW), cond_frames=SF1, context_shape=(1, 2), device="cpu", ops=slot_ref,
                        prediction_type=bad)
    x, c = torch.ones((1, 2, 1, 2, 2)), torch.zeros((1, 1, 1, 1))
    calls = []
    unet = lambda *a, **k: calls.append(a) or a[0]
    for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler):
        smp = cls("cpu", ops=OPS, prediction_type="v_prediction")
        smp.make_schedule(10, verbose=False)
        with pytest.raises(NotImplementedError, match="v-prediction"):
            smp.encode(unet, x, c, 3)
        with pytest.raises(NotImplementedError, match="v-prediction"):
            smp.p_invert_ddim(unet, x, c, smp._t_table[0].expand(1), 0)
        with pytest.raises(NotImplementedError, match="v-prediction"):      # before the VAE, the text model or the UNet is touched
            pipeline.edit_clips(unet, None, None, smp, torch.zeros((1, 3, 3, 16, 16)), None, None, cond_frames=1, strength=0.5,
                                seed=None, invert=True)
        eps_smp = cls("cpu", ops=OPS)
        eps_smp.make_schedule(10, verbose=False)
        assert eps_smp.encode(lambda x_, t, c_, cond_frame=0: 0.1 * x_, x, c, 3)[0].shape == x.shape          # the default still inverts
    assert calls == []
    # stochastic_encode and decode of a v-sampler are DDIMSampler's, on latents
    smp = _sampler("ddim", "v_prediction")
    assert torch.equal(smp.stochastic_encode(x, 4, seed=3), _sampler("ddim", "epsilon").stochastic_encode(x, 4, seed=3))


def test_surface():
    from seervideoldm_amd import _lib, ops, train_ops
    from seervideoldm_amd.trainer import SeerTrainer
    assert {"seer_v_to_eps", "seer_slot_v_to_eps", "seer_velocity_target"} <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 27                        # declarations only: no struct changed
    assert all(callable(getattr(ops, n)) for n in ("v_to_eps", "v_to_eps_dev", "slot_v_to_eps")) and callable(train_ops.velocity_target)
    assert ops.PREDICTION_TYPES == ("epsilon", "v_prediction")
    for fn in (SlotSampler.__init__, SeerTrainer.__init__, pipeline.generate_queue):
        assert inspect.signature(fn).parameters["prediction_type"].default == "epsilon"
    for name, fn in (("v_to_eps", ops.v_to_eps), ("v_to_eps_dev", ops.v_to_eps_dev), ("slot_v_to_eps", ops.slot_v_to_eps),
                     ("velocity_target", train_ops.velocity_target)):
        ours = inspect.signature(getattr(V, name)).parameters
        theirs = inspect.signature(fn).parameters
        assert list(ours) == list(theirs) and all(ours[k].kind == theirs[k].kind for k in ours), name


@pytest.fixture
def compat_env(monkeypatch):
    yield monkeypatch
    compat.uninstall()


@pytest.mark.parametrize("sampler,base", [(None, DDIMSampler), ("plms", PLMSSampler), ("dpmpp", DPMSolverSampler)])
@pytest.mark.parametrize("how", ["env", "argument", "upper"])
def test_compat_v_prediction(compat_env, how, sampler, base):
    compat_env.delenv("SEER_COMPAT_SAMPLER", raising=False)
    if sampler:
        compat_env.setenv("SEER_COMPAT_SAMPLER", sampler)
    if how == "argument":
        compat_env.delenv("SEER_COMPAT_PREDICTION", raising=False)
        compat.install(prediction="v_prediction")
    else:
        compat_env.setenv("SEER_COMPAT_PREDICTION", "v_prediction" if how == "env" else " V_Prediction ")
        compat.install()
    from ldm.models.diffusion.ddim_video import DDIMSampler as Aliased
    assert issubclass(Aliased, base) and Aliased is not base and Aliased.__name__ == base.__name__
    smp = Aliased("cpu")                                  # as the scripts build it
    assert smp.prediction_type == "v_prediction" and type(smp).sample is base.sample
    assert Aliased("cpu", prediction_type="epsilon").prediction_type == "epsilon"
    compat.install(prediction="v_prediction")             # the same class again: one per sampler
    from ldm.models.diffusion.ddim_video import DDIMSampler as Again
    assert Again is Aliased


@pytest.mark.parametrize("value", [None, "", "epsilon", " EPSILON "])
def test_compat_other_values_behave_as_before(compat_env, value):
    compat_env.delenv("SEER_COMPAT_SAMPLER", raising=False)
    if value is None:
        compat_env.delenv("SEER_COMPAT_PREDICTION", raising=False)
    else:
        compat_env.setenv("SEER_COMPAT_PREDICTION", value)
    compat.install()
    from ldm.models.diffusion.ddim_video import DDIMSampler as Aliased
    assert Aliased is DDIMSampler


def test_compat_unknown_prediction_is_the_references_error(compat_env):
    compat_env.setenv("SEER_COMPAT_PREDICTION", "sample")
    with pytest.raises(ValueError, match="Unknown prediction type sample"):
        compat.install()


# ---- the entry points' refusals ---------------------------------------------------------------------------------------------------------
def refusal_cases(P, W, T8):
    """(entry point, arguments without the stream, what is wrong) for every refusal of the three entry points (seer_v_to_eps in its two forms).  P stands for every fp32
    buffer, W for the int32 ones and T8 for the int64 timesteps; all aligned and non-NULL (tests/test_gpu_vpred.py passes real ones)"""
    good = dict(v=P, reps=2, b=2, C=4, F_total=5, cond_f=2, HW=96, coef=P, nsched=10, index=3, step=None, x=P, out=P)
    shape = (dict(b=0), dict(b=-1), dict(C=0), dict(HW=0), dict(HW=-4), dict(cond_f=-1), dict(cond_f=5), dict(cond_f=6),
             dict(F_total=0, cond_f=0), dict(nsched=0), dict(nsched=-3))
    huge = dict(b=1 << 16, C=1 << 16, F_total=1 << 8, cond_f=0, HW=1)                        # 2^40 elements: a grid beyond one dimension
    for kw in (dict(v=None), dict(coef=None), dict(x=None), dict(out=None), dict(reps=0), dict(reps=3), dict(reps=-1), *shape,
               dict(index=-1), dict(index=10), dict(index=11), dict(v=P + 2), dict(coef=P + 1), dict(x=P + 2), dict(out=P + 3), huge,
               dict(step=W)):
        yield "seer_v_to_eps", tuple({**good, **kw}.values()), kw
    good = dict(v=P, reps=2, b=2, C=4, F_total=5, cond_f=2, HW=96, coef=P, nsched=10, index=-1, step=W, x=P, out=P)
    for kw in (dict(v=None), dict(coef=None), dict(step=None), dict(x=None), dict(out=None), dict(reps=0), dict(reps=3), *shape,
               dict(v=P + 2), dict(coef=P + 1), dict(step=W + 2), dict(x=P + 2), dict(out=P + 3), huge, dict(index=3)):
        yield "seer_v_to_eps", tuple({**good, **kw}.values()), kw
    good = dict(v=P, slots=2, C=4, F_total=5, cond_f=2, HW=96, coef=P, nsched=10, step=W, state=W, x=P, x_prov=P + 4096, out=P)
    shape = tuple(kw for kw in shape if "b" not in kw)
    for kw in (dict(v=None), dict(coef=None), dict(step=None), dict(x=None), dict(out=None), dict(state=None), dict(x_prov=None),
               dict(x_prov=P), dict(slots=0), dict(slots=5), dict(slots=-1), *shape, dict(v=P + 2), dict(coef=P + 1), dict(step=W + 2),
               dict(state=W + 1), dict(x=P + 2), dict(x_prov=P + 4098), dict(out=P + 3), dict(slots=4, C=1 << 20, F_total=1 << 20, cond_f=0,
                                                                                                 HW=1 << 10)):
        yield "seer_slot_v_to_eps", tuple({**good, **kw}.values()), kw
    good = dict(latents=P, noise=P, timesteps=T8, alphas_cumprod=P, T=1000, b=2, per_row=96, target=P)
    for kw in (dict(latents=None), dict(noise=None), dict(timesteps=None), dict(alphas_cumprod=None), dict(target=None), dict(T=0),
               dict(T=-1), dict(b=0), dict(b=-2), dict(b=65536), dict(per_row=0), dict(per_row=-4), dict(latents=P + 2), dict(noise=P + 1),
               dict(target=P + 3), dict(alphas_cumprod=P + 2), dict(timesteps=T8 + 4), dict(per_row=1 << 41)):
        yield "seer_velocity_target", tuple({**good, **kw}.values()), kw


def test_kernel_entry_points_refuse_bad_arguments_before_any_launch():
    """every refusal returns SEER_EINVAL on the host (the pointers are aligned non-NULL integers that are no memory; no call here would
    pass its checks, so nothing is launched)"""
    from seervideoldm_amd import _lib
    from seervideoldm_amd.build import build_library
    build_library()
    lib = _lib.load()
    n = 0
    for fn, args, why in refusal_cases(1 << 20, 1 << 20, 1 << 20):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    assert n >= 85
