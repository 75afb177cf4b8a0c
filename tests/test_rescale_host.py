"""Guidance rescale without a GPU, on the torch stand-ins (tests/rescale_ref.py in front of tests/vpred_ref.py and the existing
tests/*_ref.py modules): the float64 restatement against the textbook std form; every sampler at CFG 7.5 against a float64 chain within
a rounding allowance counted per fp32 operation; where the node is launched and with what; the graph keys; slots against solo runs and
against plain queues, exactly; the refusals, the compat switch and the ABI version.  Runs everywhere (CPU)."""
import json
from pathlib import Path

import pytest
import torch

from seervideoldm_amd import DDIMSampler, DPMSolverSampler, PLMSSampler, SlotSampler, _lib, compat, ops, pipeline
from seervideoldm_amd import ddim as ddim_module
from seervideoldm_amd import plms as plms_module
from tests import dpm_ref as D
from tests import edit_ref, slot_dpm_ref, slot_plms_ref, slot_ref, stoch_ref
from tests import rescale_ref as R
from tests import sampler_graph_cases as sg
from tests import test_vpred_host as H
from tests import vpred_ref as V
from tests.test_slots_host import C as SC, F1 as SF1, FP as SFP, H as SH, W as SW, _Gaussian

f64 = torch.float64
OPS = R.backend(D)
B, CH, FP, HH, WW, S, SCALE = H.B, H.CH, H.FP, H.H, H.W, H.S, H.SCALE
F1 = 2
PHIS = (0.7, 1.0)
K_RESCALE = 2                                            # roundings the node adds to an evaluation's eps: m's own, and the product m * g


def _sampler(name, prediction_type, ops_=OPS, **kw):
    cls, ckw, skw = H.SAMPLERS[name]
    smp = cls("cpu", ops=ops_, prediction_type=prediction_type, **ckw, **kw)
    smp.make_schedule(S, ddim_eta=skw.get("eta", 0.), verbose=False)
    return smp


def _sample(smp, name, model, x_T, x0_emb, c, cfg=True, **kw):
    guided = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=torch.ones_like(c), cond_frames=F1) if cfg else {}
    return smp.sample(model, S, B, (CH, FP, HH, WW), x0_emb=x0_emb, conditioning=c, x_T=x_T, verbose=False, is_3d=True,
                      **H.SAMPLERS[name][2], **guided, **kw)[0]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.5, 7.5])
@pytest.mark.parametrize("phi", [0.3, 0.7, 1.0])
def test_restatement_is_the_textbook_std_form(scale, phi):
    """rescale64 (the all-integer form q = n S2 - S1^2, the n - 1 cancelled) against rescale_noise_cfg with unbiased stds over all
    non-batch dims, on normals of shape (2, 4, 5, 300): 1e-12 relative"""
    g_ = torch.Generator().manual_seed(5)
    eu, ec = torch.randn((2, 4, 5, 300), generator=g_, dtype=f64), torch.randn((2, 4, 5, 300), generator=g_, dtype=f64) + 0.3
    g = eu + scale * (ec - eu)
    got, want = R.rescale64(g, ec, phi), R.textbook64(g, ec, R.widened(phi))
    err = ((got - want).abs() / want.abs().clamp_min(1e-300)).max()
    print(f"[rescale] restatement scale={scale} phi={phi}: max relative difference {err:.3g}")
    assert err <= 1e-12
    if phi == 1.0:                                       # the point of it: the result has the conditional row's std
        assert torch.allclose(got.reshape(2, -1).std(1), ec.reshape(2, -1).std(1), rtol=1e-12, atol=0)
    # degenerate: a constant g has no std to match; m = 1 where diffusers divides by zero
    assert torch.equal(R.multiplier64(torch.full((1, 6), 2.0), torch.randn((1, 6), generator=g_), phi), torch.ones((1, 1), dtype=f64))
    assert torch.equal(R.multiplier64(torch.randn((3, 1), generator=g_), torch.randn((3, 1), generator=g_), phi), torch.ones((3, 1), dtype=f64))


# ---- sampler chains -------------------------------------------------------------------------------------------------------------------------
def _allowance(name, smp, x_T, raw_rows, prediction_type, phi):
    """tests/test_vpred_host._allowance with the multipliers in the chain: the float64 chain is run once, its multipliers are kept, and
    the unit bumps run over those (the chain is then affine in each of its quantities, as that function needs)"""
    rows = R.RescaledRows(raw_rows, SCALE, phi)

    def run(bump=None):
        rows.restart()
        return H._chain64(name, smp, x_T, rows, prediction_type, True, bump=bump)
    base, marks = run()
    rows.freeze()
    method = name.split("-")[0]
    k_of = {"e": H.K_E[prediction_type] + K_RESCALE, "x": H.K_X[method], "p": H.K_P, "d": H.K_D}
    total = torch.zeros_like(base)
    for what, k, mag in marks:
        bumped, _ = run(bump=(what, k))
        total += (bumped - base).abs() * k_of[what] * V.U * mag
    return base, total, rows.frozen


@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("phi", PHIS)
@pytest.mark.parametrize("name", list(H.SAMPLERS))
def test_sampler_follows_the_float64_chain(name, phi, prediction_type):
    """S = 10, b = 2, two conditioning latents, CFG 7.5, on the analytic Gaussian model of tests/dpm_ref.py.  The sampler on the
    stand-ins against tests/vpred_ref.chain64 in float64, whose model rows carry the float64 multiplier of every evaluation
    (tests/rescale_ref.RescaledRows), per element within
        sum over every quantity q the fp32 chain rounds of |d x_final / d q| k_q 2^-24 M_q  +  2^-126
    with d x_final / d q and M_q as in tests/test_vpred_host.py (M_q of an evaluation is m times the operand magnitudes of the
    unscaled CFG combine: the rows handed to chain64 are m uc and m c) and k_q that file's counts, except
      e, an evaluation's rescaled eps    K_E + 2: the 4 (eps-model) or 8 (v-model) roundings of test_vpred_host, the rounding of m to
                                         fp32 and the one product m * g.  The combine behind the node adds none: eu == ec there, and
                                         eu + scale * (ec - eu) is eu exactly.
    The four sums are double sums of exact products, so m carries no rounding of its own beyond its conversion to fp32.  phi = 0.7 is
    the constructor's keyword, phi = 1 the per-call override on sample()."""
    shift, x_T, x0_emb, c = H._problem(F1)
    ctor = dict(guidance_rescale=phi) if phi == 0.7 else {}
    call = {} if phi == 0.7 else dict(guidance_rescale=phi)
    smp = _sampler(name, prediction_type, **ctor)
    model, rows = H._models(smp, shift, F1, True)[prediction_type]
    got = _sample(smp, name, model, x_T, x0_emb, c, **call)
    x64, allow, mults = _allowance(name, smp, x_T, rows, prediction_type, phi)
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    err = (got.double() - x64).abs()
    m_all = torch.cat([m.reshape(-1) for m in mults])
    print(f"[rescale] {name} phi={phi} {prediction_type}: worst err / allowance = {(err / (allow + 2.0 ** -126)).max():.3g}, largest "
          f"allowance = {allow.max():.3g}, multipliers {m_all.min():.4f} .. {m_all.max():.4f}")
    assert (err <= allow + 2.0 ** -126).all()
    # the allowance has teeth: the same sampler without the rescale, or with another factor, is far outside it
    plain = _sample(_sampler(name, prediction_type), name, model, x_T, x0_emb, c)
    other = _sample(_sampler(name, prediction_type), name, model, x_T, x0_emb, c, guidance_rescale=0.5)
    for wrong in (plain, other):
        assert ((wrong.double() - x64).abs() > allow + 2.0 ** -126).any()
    # CFG off: the factor has nothing to act on, and the result is the plain sampler's bit for bit
    off = _sample(_sampler(name, prediction_type, **ctor), name, H._models(smp, shift, F1, False)[prediction_type][0], x_T, x0_emb, c,
                  cfg=False, **call)
    assert torch.equal(off, _sample(_sampler(name, prediction_type), name, H._models(smp, shift, F1, False)[prediction_type][0], x_T,
                                    x0_emb, c, cfg=False))


# ---- where the node is launched ---------------------------------------------------------------------------------------------------------
def _recorded(name, prediction_type, phi, cfg=True, two_calls=False, per_call=False):
    rec = H._Recording(OPS)
    smp = _sampler(name, prediction_type, ops_=rec, **({} if per_call else dict(guidance_rescale=phi)))
    shift, x_T, x0_emb, c = H._problem(F1)
    inner = H._models(smp, shift, F1, cfg)[prediction_type][0]

    def model(x, t, cc, cond_frame=0):
        rec.calls.append(("unet", (x, t), {}, None))
        return inner(x, t, cc, cond_frame)
    kw = {}
    if cfg:
        uc = torch.ones((B, F1 + FP, 2, 1)) if two_calls else torch.ones_like(c)      # another token count: the two-call branch
        kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, cond_frames=F1)
    smp.sample(model, S, B, (CH, FP, HH, WW), x0_emb=x0_emb, conditioning=c, x_T=x_T, verbose=False, is_3d=True, **H.SAMPLERS[name][2],
               **kw, **(dict(guidance_rescale=phi) if per_call else {}))
    return smp, rec


@pytest.mark.parametrize("name", list(H.SAMPLERS))
def test_node_sits_between_the_model_and_the_conversion_once_per_evaluation(name):
    entry = H.STEP_ENTRY[name]
    for prediction_type, conv in (("epsilon", []), ("v_prediction", ["v_to_eps"])):
        smp, rec = _recorded(name, prediction_type, 0.7)
        n = smp.ddim_coef.shape[0]
        evals = n + 1 if name == "plms" else n           # the PLMS first step evaluates twice: the node runs for both
        assert rec.names() == ["unet", "cfg_rescale", *conv, entry] * evals
        calls = rec.calls
        for k, call in enumerate(calls):
            if call[0] != "cfg_rescale":
                continue
            assert call[2] == dict(scale=SCALE, rescale=0.7, cond_f=F1) and call[1][0].shape[0] == 2 * B
            assert calls[k + 1][1][0] is call[3]         # the next launch reads what the node wrote
            out = call[3][:, :, F1:]
            assert torch.equal(out[:B], out[B:])          # both rows of every clip
        # the keyword on sample() alone does the same
        assert _recorded(name, prediction_type, 1.0, per_call=True)[1].names() == ["unet", "cfg_rescale", *conv, entry] * evals
        # never at phi = 0, never with CFG off
        assert _recorded(name, prediction_type, 0.0)[1].names() == ["unet", *conv, entry] * evals
        assert _recorded(name, prediction_type, 0.7, cfg=False)[1].names() == ["unet", *conv, entry] * evals
    # the two-call CFG branch: one node behind the second call
    assert _recorded(name, "epsilon", 0.7, two_calls=True)[1].names() == ["unet", "unet", "cfg_rescale", entry] * evals


def test_inversion_rescales_too():
    rec = H._Recording(OPS)
    smp = DDIMSampler("cpu", ops=rec)
    smp.make_schedule(S, verbose=False)
    x, c = torch.randn((1, 2, 1, 2, 2), generator=torch.Generator().manual_seed(2)), torch.zeros((1, 1, 1, 1))
    model = lambda x_, t, c_, cond_frame=0: 0.1 * x_ * (1.0 + torch.arange(x_.shape[0]).view(-1, 1, 1, 1, 1))
    kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=torch.ones_like(c))
    plain = smp.encode(model, x, c, 3, **kw)[0]
    assert rec.names() == ["cfg_ddim_invert_step"] * 3
    del rec.calls[:]
    got = smp.encode(model, x, c, 3, guidance_rescale=0.7, **kw)[0]
    assert rec.names() == ["cfg_rescale", "cfg_ddim_invert_step"] * 3 and not torch.equal(got, plain)
    del rec.calls[:]
    smp.p_invert_ddim(model, x, c, smp._t_table[0].expand(1), 0, guidance_rescale=1.0, **kw)
    assert rec.names() == ["cfg_rescale", "cfg_ddim_invert_step"] and rec.calls[0][2]["rescale"] == 1.0


# ---- graph keys -------------------------------------------------------------------------------------------------------------------------------
class _KeyEngine:
    """what _step_graph asks of an engine, with the context geometry and the mode word of the mini UNet of tests/sampler_graph_cases.py;
    every key looked up is written down and nothing is ever found"""
    inv = True

    def __init__(self):
        self.keys = []

    def _context(self, context):
        rows, frames, L, Dm = context.shape
        return torch.empty((rows * frames * L, Dm)), L

    def graph_get(self, key):
        self.keys.append(key)
        return None


def _keys(monkeypatch, cls, run, **ctor):
    eng = _KeyEngine()
    monkeypatch.setattr(ddim_module, "capture_engine", lambda unet, backend, device: eng)
    monkeypatch.setattr(plms_module, "capture_engine", lambda unet, backend, device: eng)
    monkeypatch.setattr(DDIMSampler, "_capture_step", lambda self, *a, **kw: None)        # every step then runs launch by launch
    smp = cls("cpu", ops=OPS, **ctor)
    run(smp)
    assert eng.keys and all(k == eng.keys[0] for k in eng.keys)
    return eng.keys[0]


def _scenario(name):
    """the sample of tests/sampler_graph_cases.py's scenario `name` (its shapes, S and scale) on CPU tensors"""
    r = sg.inputs("cpu", 0)[0]
    kw = sg.SCENARIOS[name][2]
    seeded, masked = kw.get("seeded", False), kw.get("masked", False)
    model = lambda x, t, c, cond_frame=0: 0.1 * x

    def run(smp, **more):
        smp.sample(model, sg.S, batch_size=1, shape=sg.SHAPE, x0_emb=r["x0_emb"], conditioning=r["c"], verbose=False, cond_frames=sg.F1,
                   unconditional_guidance_scale=kw.get("scale", sg.SCALE), unconditional_conditioning=r["uc"], eta=kw.get("eta", 0.),
                   x_T=None if seeded and not masked else r["x_T"], is_3d=True, **(dict(seed=r["seed"]) if seeded else {}),
                   **(dict(mask=r["mask"], x0=r["known"]) if masked else {}), **more)
    return run


@pytest.mark.parametrize("name", ["ddim_cfg", "ddim_plain", "ddim_seeded", "ddim_masked", "plms_cfg"])
def test_default_keys_are_the_recorded_ones_and_a_factor_appends_two_words(monkeypatch, name):
    golden = json.loads((Path(__file__).resolve().parent / "golden" / "sampler_graph_keys.json").read_text())[name]
    cls, run = sg.SCENARIOS[name][0], _scenario(name)
    default = _keys(monkeypatch, cls, run)
    assert [repr(default)] == golden
    assert _keys(monkeypatch, cls, run, guidance_rescale=0.0) == default
    for phi in PHIS:
        want = default if name == "ddim_plain" else default + ("rescale", phi)             # CFG off: the key does not know of it
        assert _keys(monkeypatch, cls, run, guidance_rescale=phi) == want
        assert _keys(monkeypatch, cls, lambda smp: run(smp, guidance_rescale=phi)) == want
    v = _keys(monkeypatch, cls, run, prediction_type="v_prediction")
    assert v == default + ("v_prediction",)
    if name != "ddim_plain":
        assert _keys(monkeypatch, cls, run, prediction_type="v_prediction", guidance_rescale=0.7) == v + ("rescale", 0.7)


def test_dpm_and_invert_keys_append_the_same_two_words(monkeypatch):
    assert set(ddim_module.STEP_KINDS) == {"step", "step-rng", "step-mask", "invert", "plms", "dpm"}      # every kind is covered here
    run = _scenario("ddim_cfg")
    default = _keys(monkeypatch, DPMSolverSampler, run)
    assert default[0] == "dpm" and default[1:] == _keys(monkeypatch, DDIMSampler, run)[1:]
    assert _keys(monkeypatch, DPMSolverSampler, run, guidance_rescale=0.7) == default + ("rescale", 0.7)
    r = sg.inputs("cpu", 0)[0]
    model = lambda x, t, c, cond_frame=0: 0.1 * x

    def invert(smp, **more):
        smp.make_schedule(sg.S, verbose=False)
        smp.encode(model, r["x_T"], r["c"], 3, unconditional_guidance_scale=sg.SCALE, unconditional_conditioning=r["uc"],
                   x0_emb=r["x0_emb"], cond_frames=sg.F1, **more)
    default = _keys(monkeypatch, DDIMSampler, invert)
    assert default[0] == "invert" and "rescale" not in default
    assert _keys(monkeypatch, DDIMSampler, lambda smp: invert(smp, guidance_rescale=0.7)) == default + ("rescale", 0.7)


# ---- slots --------------------------------------------------------------------------------------------------------------------------------------
SLOT_MODES = {"ddim": (slot_ref, {}, "epsilon"), "plms": (slot_plms_ref, dict(plms=True), "epsilon"),
              "dpm": (slot_dpm_ref, dict(dpm=True), "epsilon"), "plms-v": (slot_plms_ref, dict(plms=True), "v_prediction")}


def _slot_requests(model, mode):
    m = {"ddim": "ddim", "plms": "plms", "dpm": "dpmpp", "plms-v": "plms"}[mode]
    extra = dict(method=m) if m != "ddim" else {}
    return [H._slot_request(model, 0, 21, 4, 7.5, guidance_rescale=0.7, **extra), H._slot_request(model, 1, 22, 6, 3.0),
            H._slot_request(model, 2, 23, 1, 5.0, guidance_rescale=1.0), H._slot_request(model, 0, 24, 5, 7.5, **extra)]


def _solo(model, r, prediction_type):
    cls = {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp": DPMSolverSampler}[r.get("method", "ddim")]
    smp = cls("cpu", ops=OPS, prediction_type=prediction_type)
    smp.consume_rng_when_deterministic = False
    return smp.sample(model, r["S"], 1, (SC, SFP, SH, SW), x0_emb=r["x0_emb"], conditioning=r["c"][None], x_T=r["x_T"], verbose=False,
                      is_3d=True, unconditional_guidance_scale=r["scale"], unconditional_conditioning=r["uc"][None],
                      guidance_rescale=r.get("guidance_rescale", 0.))[0]


@pytest.mark.parametrize("mode", list(SLOT_MODES))
def test_a_rescaled_clip_equals_its_solo_run_and_a_plain_clip_its_plain_queue(mode):
    """2 slots, four staggered requests, two of them rescaled (phi 0.7 and 1) and two plain.  On the stand-ins the slot form and the solo
    form of the node are one torch expression, so a rescaled clip has the bits of its solo run; the node does not touch a phi = 0 slot,
    so a plain clip has the bits it has in a queue built without the keyword."""
    ref, flags, prediction_type = SLOT_MODES[mode]
    model = (H._VGaussian if prediction_type == "v_prediction" else _Gaussian)(3)
    reqs = _slot_requests(model, mode)
    for r, tag in zip(reqs, "abcd"):
        r["tag"] = tag
    rec = H._Recording(R.backend(ref))
    build = lambda ops_, **kw: SlotSampler(model, 2, shape=(SC, SFP, SH, SW), cond_frames=SF1, context_shape=(1, 2), device="cpu", ops=ops_,
                                           prediction_type=prediction_type, **flags, **kw)
    got = dict(build(rec, rescale=True).run(iter(reqs)))
    assert sorted(got) == list("abcd")
    for r in reqs:
        want = _solo(model, r, prediction_type)
        assert torch.equal(got[r["tag"]], want), (mode, r["tag"], (got[r["tag"]] - want).abs().max())
        if r.get("guidance_rescale"):
            assert not torch.equal(want, _solo(model, dict(r, guidance_rescale=0.), prediction_type))
    plain_reqs = [{k: v for k, v in r.items() if k != "guidance_rescale"} for r in reqs if not r.get("guidance_rescale")]
    plain = dict(build(R.backend(ref)).run(iter(plain_reqs)))
    for r in plain_reqs:
        assert torch.equal(got[r["tag"]], plain[r["tag"]])
    # the node: once per step, behind the model, in front of the conversion, in place on the model's rows with the per-slot buffers
    names = [n for n in rec.names() if n != "cfg_rescale_workspace"]
    conv = ["slot_v_to_eps"] if prediction_type == "v_prediction" else []
    step = [names[0], "slot_cfg_rescale", *conv, names[-1]]
    assert names == step * (len(names) // len(step)) and names[0].endswith("step_begin")
    node = [c for c in rec.calls if c[0] == "slot_cfg_rescale"]
    assert all(c[1][2].dtype == torch.float32 and c[1][2].shape == (2,) and c[2]["cond_f"] == SF1 and c[3] is c[1][0] for c in node)


@pytest.mark.parametrize("flags, ref", [(dict(stochastic=True), stoch_ref), (dict(editing=True), edit_ref),
                                        (dict(editing=True, stochastic=True), edit_ref)])
def test_rescale_goes_with_the_seeded_and_the_editing_queue(flags, ref):
    model = _Gaussian(3)
    rec = H._Recording(R.backend(ref))
    smp = SlotSampler(model, 2, shape=(SC, SFP, SH, SW), cond_frames=SF1, context_shape=(1, 2), device="cpu", ops=rec, rescale=True,
                      **flags)
    seeded = dict(seed=5, eta=0.5) if flags.get("stochastic") else {}
    r = dict(H._slot_request(model, 0, 21, 4, 7.5, guidance_rescale=0.7), **seeded)
    got = dict(smp.run(iter([r])))[0]
    assert "slot_cfg_rescale" in rec.names()
    plain = SlotSampler(model, 2, shape=(SC, SFP, SH, SW), cond_frames=SF1, context_shape=(1, 2), device="cpu", ops=R.backend(ref), **flags)
    assert not torch.equal(got, dict(plain.run(iter([{k: v for k, v in r.items() if k != "guidance_rescale"}])))[0])
    if seeded:                                           # against the solo seeded sampler, exactly
        solo = DDIMSampler("cpu", ops=OPS)
        want = solo.sample(model, 4, 1, (SC, SFP, SH, SW), x0_emb=r["x0_emb"], conditioning=r["c"][None], x_T=r["x_T"], verbose=False,
                           is_3d=True, unconditional_guidance_scale=7.5, unconditional_conditioning=r["uc"][None], eta=0.5, seed=5,
                           guidance_rescale=0.7)[0]
        assert torch.equal(got, want)


def test_generate_queue_and_the_batch_helpers_hand_the_factor_on(monkeypatch):
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
    for flag, want in ((True, True), (False, None)):
        seen.clear()
        with pytest.raises(_Stop):
            list(pipeline.generate_queue(None, fst, None, [req], slots=2, num_frames=3, cond_frames=1, rescale=flag))
        assert seen.get("rescale") == want
    # a request's factor reaches submit; without rescale=True a non-zero one is refused before anything is built
    submitted = []

    class _Queue:
        def __init__(self, *a, **kw):
            pass

        def run(self, requests):
            submitted.extend(requests)
            return iter(())
    monkeypatch.setattr(slots, "SlotSampler", _Queue)
    list(pipeline.generate_queue(None, fst, None, [dict(req, guidance_rescale=0.7)], slots=2, num_frames=3, cond_frames=1, rescale=True))
    assert submitted[0]["guidance_rescale"] == 0.7
    with pytest.raises(ValueError, match="rescale=True"):
        list(pipeline.generate_queue(None, fst, None, [dict(req, guidance_rescale=0.7)], slots=2, num_frames=3, cond_frames=1))
    # evaluate_batch / generate_clips: the sampler's default stands aside for the call and comes back
    smp = DDIMSampler("cpu", ops=OPS, guidance_rescale=0.25)
    during = []
    monkeypatch.setattr(pipeline, "ddim_sample", lambda sampler, *a, **kw: during.append(sampler.guidance_rescale) or torch.zeros((1, 3, 2, 16, 16)))
    pipeline.evaluate_batch(None, fst, None, smp, torch.zeros((1, 3, 3, 16, 16)), torch.zeros((1, 2, 3)), torch.zeros((1, 2, 3)),
                            cond_frames=1, gather=False, guidance_rescale=0.7)
    pipeline.evaluate_batch(None, fst, None, smp, torch.zeros((1, 3, 3, 16, 16)), torch.zeros((1, 2, 3)), torch.zeros((1, 2, 3)),
                            cond_frames=1, gather=False)
    assert during == [0.7, 0.25] and smp.guidance_rescale == 0.25
    # edit_clips: every sampler call it makes carries the keyword
    calls = []

    class _Smp:
        ddim_timesteps = torch.zeros(10)

        def make_schedule(self, **kw):
            pass

        def stochastic_encode(self, x, t, seed=None):
            return x

        def decode(self, *a, **kw):
            calls.append(kw.get("guidance_rescale"))
            return torch.zeros((1, 4, 2, 2, 2))
    monkeypatch.setattr(pipeline, "frames_to_latents", lambda vae, x, g: torch.zeros((1, 4, 3, 2, 2)))
    monkeypatch.setattr(pipeline, "latents_to_clip", lambda vae, lat: lat)
    pipeline.edit_clips(None, fst, None, _Smp(), torch.zeros((1, 3, 3, 16, 16)), torch.zeros((1, 2, 3)), torch.zeros((1, 2, 3)),
                        cond_frames=1, strength=0.5, seed=1, guidance_rescale=0.7)
    assert calls == [0.7]


# ---- refusals, compat, the surface --------------------------------------------------------------------------------------------------------------
def test_factor_outside_the_unit_interval_is_refused_everywhere():
    x, c = torch.ones((1, 2, 1, 2, 2)), torch.zeros((1, 1, 1, 1))
    unet = lambda *a, **k: pytest.fail("the model was called")
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "much", None):
        for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler):
            with pytest.raises(ValueError, match="guidance_rescale"):
                cls("cpu", guidance_rescale=bad)
        with pytest.raises(ValueError, match="guidance_rescale"):
            ops.check_guidance_rescale(bad)
    for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler):
        assert cls("cpu").guidance_rescale == 0.0 and cls("cpu", guidance_rescale=1).guidance_rescale == 1.0
        smp = cls("cpu", ops=OPS)
        kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=torch.ones_like(c))
        with pytest.raises(ValueError, match="guidance_rescale"):
            smp.sample(unet, 4, 1, (2, 1, 2, 2), conditioning=c, x_T=x, verbose=False, is_3d=True, guidance_rescale=1.5, **kw)
        with pytest.raises(ValueError, match="guidance_rescale"):
            smp.encode(unet, x, c, 3, guidance_rescale=-1.0, **kw) if cls is DDIMSampler else smp.sample(
                unet, 4, 1, (2, 1, 2, 2), conditioning=c, x_T=x, verbose=False, is_3d=True, guidance_rescale=-1.0, **kw)
        smp.make_schedule(4, verbose=False)
        if cls is not PLMSSampler:
            with pytest.raises(ValueError, match="guidance_rescale"):
                smp.decode(unet, x, c, 2, guidance_rescale=2.0, **kw)
    step = {DDIMSampler: "p_sample_ddim", PLMSSampler: "p_sample_plms", DPMSolverSampler: "p_sample_dpm"}
    for cls, name in step.items():
        smp = cls("cpu", ops=OPS)
        smp.make_schedule(4, verbose=False)
        model = lambda x_, t, c_, cond_frame=0: 0.1 * x_
        with pytest.raises(ValueError, match="guidance_rescale"):
            getattr(smp, name)(model, x, c, smp._t_table[3].expand(1), 3, guidance_rescale=7.0, t_next=smp._t_table[2].expand(1),
                               **kw) if cls is PLMSSampler else getattr(smp, name)(model, x, c, smp._t_table[3].expand(1), 3,
                                                                                   guidance_rescale=7.0, **kw)


def test_submit_needs_a_queue_built_for_it():
    model = _Gaussian(1)
    r = H._slot_request(model, 0, 21, 4, 7.5)
    r.pop("tag")
    build = lambda **kw: SlotSampler(model, 2, shape=(SC, SFP, SH, SW), cond_frames=SF1, context_shape=(1, 2), device="cpu",
                                     ops=R.backend(slot_ref), **kw)
    smp = build()
    with pytest.raises(ValueError, match="guidance_rescale needs a sampler built with rescale=True"):
        smp.submit(**r, guidance_rescale=0.7)
    assert smp.submit(**r, guidance_rescale=0.0) == 0 and smp.free_slots() == [1]       # zero is every clip's default
    smp = build(rescale=True)
    for bad in (-0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            smp.submit(**r, guidance_rescale=bad)
    assert smp.free_slots() == [0, 1]
    assert smp.submit(**r, guidance_rescale=0.7) == 0 and smp.submit(**r) == 1
    assert smp._phi.tolist() == [float(torch.tensor(0.7)), 0.0]
    # a slot's factor is written when it is filled: the next plain clip of slot 0 is plain
    while smp.active():
        smp.step()
    assert smp.submit(**r) == 0 and smp._phi.tolist() == [0.0, 0.0]


def test_a_sharded_model_is_refused():
    class _Sharded:
        _shard = type("Shard", (), {"world": 1})()

        def __call__(self, *a, **kw):
            pytest.fail("the model was called")
    x, c = torch.ones((1, 2, 1, 2, 2)), torch.zeros((1, 1, 1, 1))
    kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=torch.ones_like(c))
    for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler):
        smp = cls("cpu", ops=OPS, guidance_rescale=0.7)
        with pytest.raises(ValueError, match="guidance_rescale: a sharded model"):
            smp.sample(_Sharded(), 4, 1, (2, 1, 2, 2), conditioning=c, x_T=x, verbose=False, is_3d=True, **kw)
    inv = DDIMSampler("cpu", ops=OPS)
    inv.make_schedule(4, verbose=False)
    with pytest.raises(ValueError, match="guidance_rescale: a sharded model"):
        inv.encode(_Sharded(), x, c, 3, guidance_rescale=0.7, **kw)
    # with CFG off, or at phi = 0, there is nothing to refuse: the sharded model is sampled as before
    calls = []

    class _Quiet:
        _shard = None

        def __call__(self, x_, t, c_, cond_frame=0):
            calls.append(1)
            return 0.1 * x_
    quiet = _Quiet()
    quiet._shard = type("S", (), {"world": 1})()
    DDIMSampler("cpu", ops=OPS, guidance_rescale=0.7).sample(quiet, 4, 1, (2, 1, 2, 2), conditioning=c, x_T=x, verbose=False, is_3d=True)
    DDIMSampler("cpu", ops=OPS).sample(quiet, 4, 1, (2, 1, 2, 2), conditioning=c, x_T=x, verbose=False, is_3d=True, **kw)
    assert calls


def test_compat_switch(monkeypatch):
    try:
        for env, arg, want in (("0.7", None, 0.7), ("", None, 0.0), ("0.2", 1.0, 1.0), ("0", None, 0.0)):
            monkeypatch.setenv("SEER_COMPAT_GUIDANCE_RESCALE", env)
            compat.install(guidance_rescale=arg)
            from ldm.models.diffusion.ddim_video import DDIMSampler as Aliased
            smp = Aliased("cpu")
            assert isinstance(smp, DDIMSampler) and smp.guidance_rescale == want and Aliased.__name__ == "DDIMSampler"
            assert Aliased("cpu", guidance_rescale=0.5).guidance_rescale == 0.5
            compat.uninstall()
        monkeypatch.setenv("SEER_COMPAT_GUIDANCE_RESCALE", "0.7")
        monkeypatch.setenv("SEER_COMPAT_SAMPLER", "dpmpp")
        monkeypatch.setenv("SEER_COMPAT_PREDICTION", "v_prediction")
        compat.install()
        from ldm.models.diffusion.ddim_video import DDIMSampler as Aliased
        smp = Aliased("cpu")
        assert isinstance(smp, DPMSolverSampler) and smp.guidance_rescale == 0.7 and smp.prediction_type == "v_prediction"
        compat.uninstall()
        for bad in ("1.5", "-1", "seven"):
            monkeypatch.setenv("SEER_COMPAT_GUIDANCE_RESCALE", bad)
            with pytest.raises(ValueError, match="guidance_rescale"):
                compat.install()
    finally:
        compat.uninstall()


def test_surface():
    assert _lib.ABI_VERSION == 27
    assert {"seer_cfg_rescale_ws_bytes", "seer_cfg_rescale", "seer_slot_cfg_rescale"} <= set(_lib.SIGNATURES)
    header = (Path(__file__).resolve().parents[1] / "include" / "seer_hip.h").read_text()
    assert f"#define SEER_RESCALE_TILE {ops.RESCALE_TILE}" in header and ops.RESCALE_TILE % 256 == 0
    for name in ("cfg_rescale", "slot_cfg_rescale", "cfg_rescale_workspace", "check_guidance_rescale"):
        assert callable(getattr(ops, name))
