"""Step caching without a GPU (tests/step_cache_ref.py): the policy's phases and weights, the engine's storing and cached walks through
the plain-torch stand-in -- bit for bit where the definition says so, against the oracle's blocks elsewhere, and by the weight keys a
cached evaluation touches -- the phases the samplers hand the model, the graph keys, every refusal, the library's argument validation
and the public surface.

WITHOUT THE FEATURE every test here fails at its first enable_step_cache, cache_phase= or step_cache import."""
import pytest
import torch

from seervideoldm_amd import DDIMSampler, DPMSolverSampler, PLMSSampler, SeerUNet, SlotSampler, _lib, compat, parallel, pipeline, synth
from seervideoldm_amd import ddim as ddim_module
from seervideoldm_amd import step_cache
from seervideoldm_amd.ddim import STEP_KINDS
from tests import dpm_ref, slot_ref
from tests import step_cache_ref as R
from tests import vpred_ref
from tests.test_engine_cpu import CFG_MINI
from tests.test_gpu_unet import REL_L2, REL_MAX

L = CFG_MINI["layers_per_block"]
BRANCHES = list(range(L + 1))
B, FR, H, COND = 2, 3, 8, 1


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _inputs(seed=1):
    return _randn((B, 4, FR, H, H), seed), _randn((B, FR, 77, 256), seed + 1), torch.tensor([501 - 20 * (seed - 1)] * B)


# ---- the policy --------------------------------------------------------------------------------------------------------------------------
def test_policy_phases_and_effective_orders():
    p = step_cache.StepCachePolicy(interval=3, branch=1, order=2)
    p.begin()
    got = [p.next() for _ in range(8)]
    assert [g[0] for g in got] == [0, 1, 2, 0, 1, 2, 0, 1]
    assert [g[1] is None for g in got] == [True, False, False, True, False, False, True, False]
    # effective order 0, 0 after the first full evaluation; 1, 1 after the second; 2 after the third
    assert got[1][1] == R.weights(1, 3, 0, 1) == (1.0, 0.0, 0.0) and got[2][1] == (1.0, 0.0, 0.0)
    assert got[4][1] == R.weights(1, 3, 1, 2) and got[5][1] == R.weights(2, 3, 1, 2) and got[4][1][2] == 0.0 and got[4][1][1] != 0.0
    assert got[7][1] == R.weights(1, 3, 2, 3) and got[7][1][2] != 0.0
    p.begin()
    assert p.next() == (0, None) and p.next() == (1, (1.0, 0.0, 0.0))       # begin() resets the chain and the valid slots


@pytest.mark.parametrize("interval", [2, 3, 4, 5])
def test_policy_weights_reproduce_polynomials(interval):
    a, b, c = 0.7, -1.3, 0.45
    for order in (0, 1, 2):
        for d in range(1, interval):
            u = d / interval
            q = u * (u + 1)
            w = [(1.0, 0.0, 0.0), (1 + u, -u, 0.0), (1 + u + q / 2, -u - q, q / 2)][order]      # float64, before the fp32 rounding
            assert abs(sum(w) - 1.0) <= 1e-15
            w32 = step_cache.forecast_weights(d, interval, order, 3)
            assert w32 == tuple(float(torch.tensor(v, dtype=torch.float64).to(torch.float32)) for v in w) == R.weights(d, interval, order, 3)
            assert abs(sum(w32) - 1.0) <= 3 * 2.0 ** -23
            # f sampled at the full evaluations k0, k0 - interval, k0 - 2 interval (slot 0 the newest), forecast at k0 + d
            k0 = 4 * interval
            for coef in ((a, b, 0.0), (a, b, c)):
                f = lambda k: coef[0] + coef[1] * k + coef[2] * k * k
                want = f(k0 + d)
                got = sum(wk * f(k0 - s * interval) for s, wk in enumerate(w))
                exact = order == 2 or (order == 1 and coef[2] == 0.0)
                assert (abs(got - want) <= 1e-12 * abs(want)) == exact, (order, d, coef, got, want)
    assert step_cache.forecast_weights(2, 3, 2, 1) == (1.0, 0.0, 0.0) and step_cache.forecast_weights(2, 3, 2, 2)[2] == 0.0


# ---- the engine on the stand-in ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI))


def _model(sd, inv=False, backend=None):
    m = SeerUNet(**CFG_MINI, **({"layout_invariant": True} if inv else {}))
    m.load_state_dict(sd, strict=True)
    m._ops_backend = backend or R.TorchOpsWithStepCache()
    return m


@pytest.fixture(scope="module")
def models(sd):
    return {False: _model(sd), True: _model(sd, inv=True)}


@pytest.mark.parametrize("inv", [False, True], ids=["default", "layout_invariant"])
@pytest.mark.parametrize("branch", BRANCHES)
def test_phase0_is_the_plain_evaluation_bit_for_bit(models, inv, branch):
    m = models[inv]
    x, ctx, t = _inputs()
    plain = m(x, t, ctx, cond_frame=COND)
    try:
        m.enable_step_cache(3, branch, 1)
        on_none = m(x, t, ctx, cond_frame=COND)
        stored = m(x, t, ctx, cond_frame=COND, cache_phase=0)
        assert m._engine.inv == inv and m._engine.cache_valid == 1
    finally:
        m.disable_step_cache()
    assert torch.equal(on_none, plain) and torch.equal(stored, plain)


@pytest.mark.parametrize("branch", BRANCHES)
def test_cached_at_the_same_inputs_is_the_full_output_under_layout_invariant(models, branch):
    """order 0 hands back the kept feature's bits, and that mode's GroupNorms sum the stored values exactly with or without the
    producer's sums: every launch behind the cut sees what it saw"""
    m = models[True]
    x, ctx, t = _inputs()
    try:
        m.enable_step_cache(3, branch, 0)
        full = m(x, t, ctx, cond_frame=COND, cache_phase=0)
        cached = m(x, t, ctx, cond_frame=COND, cache_phase=1)
        # interval 2, order 1 after two full evaluations at the same inputs: 1.5 f - 0.5 f is exact on 16-bit data
        m.enable_step_cache(2, branch, 1)
        m(x, t, ctx, cond_frame=COND, cache_phase=0)
        m(x, t, ctx, cond_frame=COND, cache_phase=0)
        assert m._engine.cache_valid == 3              # (the same branch: the first evaluation's slot still counts)
        lin = m(x, t, ctx, cond_frame=COND, cache_phase=1)
    finally:
        m.disable_step_cache()
    assert torch.equal(cached, full) and torch.equal(lin, full)


@pytest.mark.parametrize("branch", BRANCHES)
def test_cached_evaluation_touches_no_weight_of_the_skipped_blocks(sd, branch):
    rec = R.RecordingStepCache()
    m = _model(sd, backend=rec)
    x, ctx, t = _inputs()
    m.enable_step_cache(3, branch, 1)
    m(x, t, ctx, cond_frame=COND, cache_phase=0)
    n = B * FR * H * H * 320
    assert rec.calls == [("push", n)]
    eng = m._engine
    eng.w = R.RecordingWeights(eng.w)
    del rec.calls[:]
    m(x, t, ctx, cond_frame=COND, cache_phase=1)
    assert rec.calls == [("forecast", n, (1.0, 0.0, 0.0))]
    touched = set(eng.w.touched)
    skipped = R.skipped_prefixes(4, L, branch)
    assert touched and not [k for k in touched if k.startswith(skipped)]
    # what it does touch: conv_in, the kept layers of the two outer blocks, the head
    kept = {"conv_in.weight", "conv_out.weight", "conv_norm_out.weight", f"up_blocks.3.resnets.{L}.conv1.weight",
            *(f"down_blocks.0.resnets.{j}.conv1.weight" for j in range(branch)),
            *(f"up_blocks.3.resnets.{j}.conv1.weight" for j in range(L - branch, L + 1))}
    assert kept <= touched, kept - touched
    # the storing walk, by contrast, goes everywhere
    del eng.w.touched[:]
    m(x, t, ctx, cond_frame=COND, cache_phase=0)
    assert [k for k in set(eng.w.touched) if k.startswith("mid_block.")]


_walks = {}


def _oracle_walks(sd, branch):
    """full at inputs A (and at A2), cached at inputs B from A's feature and from the order-1 forecast: once per branch"""
    if branch not in _walks:
        xa, ca, ta = _inputs(1)
        xa2, _, ta2 = _inputs(3)
        xb, _, tb = _inputs(2)
        with torch.no_grad():
            full_a, fa = R.full_walk(sd, CFG_MINI, xa, ta, ca, COND, branch)
            _, fa2 = R.full_walk(sd, CFG_MINI, xa2, ta2, ca, COND, branch)
            w = R.weights(1, 3, 1, 2)
            _walks[branch] = dict(full_a=full_a, reuse=R.cached_walk(sd, CFG_MINI, xb, tb, ca, COND, branch, fa),
                                  linear=R.cached_walk(sd, CFG_MINI, xb, tb, ca, COND, branch, w[0] * fa2 + w[1] * fa))
    return _walks[branch]


def _close(got, ref):
    rel = ((got - ref).norm() / ref.norm()).item()
    mx = ((got - ref).abs().max() / ref.abs().max()).item()
    assert rel <= REL_L2 and mx <= REL_MAX, (rel, mx)


@pytest.mark.parametrize("branch", BRANCHES)
def test_cached_at_other_inputs_matches_the_oracle_walk(sd, models, branch):
    from oracle import seer_oracle as O
    m = models[False]
    (xa, ca, ta), (xa2, _, ta2), (xb, _, tb) = _inputs(1), _inputs(3), _inputs(2)
    ref = _oracle_walks(sd, branch)
    try:
        m.enable_step_cache(3, branch, 1)
        full = m(xa, ta, ca, cond_frame=COND, cache_phase=0)
        reuse = m(xb, tb, ca, cond_frame=COND, cache_phase=1)          # one valid slot: order 0
        m(xa2, ta2, ca, cond_frame=COND, cache_phase=0)
        linear = m(xb, tb, ca, cond_frame=COND, cache_phase=1)         # two: the linear forecast
    finally:
        m.disable_step_cache()
    with torch.no_grad():
        _close(full, O.unet_forward(sd, CFG_MINI, xa, ta, ca, cond_frame=COND))
    _close(full, ref["full_a"])           # the written-out walk is the oracle's forward
    _close(reuse, ref["reuse"])
    _close(linear, ref["linear"])
    assert not torch.equal(reuse, linear)
    # the guard: a cached walk is a different function of its inputs than the full one
    with torch.no_grad():
        full_b = O.unet_forward(sd, CFG_MINI, xb, tb, ca, cond_frame=COND)
    assert ((ref["reuse"] - full_b).norm() / full_b.norm()).item() > 2 * REL_L2


CFG_TWO_WIDTHS = dict(block_out_channels=(320, 640, 640, 640), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)


def test_cut_feature_at_the_deepest_branch_has_level_1_width():
    """branch = layers_per_block cuts behind the last upsampler, whose output is as wide as level 1: 640 channels here (CFG_MINI's
    levels are all 320 wide and cannot tell)"""
    sd = synth.synth_state_dict(synth.unet_param_shapes(CFG_TWO_WIDTHS))
    rec = R.RecordingStepCache()
    m = SeerUNet(**CFG_TWO_WIDTHS)
    m.load_state_dict(sd, strict=True)
    m._ops_backend = rec
    xa, xb = _randn((1, 4, 2, 8, 8), 1), _randn((1, 4, 2, 8, 8), 2)
    ctx, t = _randn((1, 2, 77, 256), 3), torch.tensor([501])
    rows = 2 * 8 * 8
    for branch, width in ((0, 320), (1, 640)):
        m.enable_step_cache(3, branch, 1)
        del rec.calls[:]
        plain = m(xa, t, ctx)
        assert torch.equal(m(xa, t, ctx, cache_phase=0), plain)
        got = m(xb, t, ctx, cache_phase=1)
        assert rec.calls == [("push", rows * width), ("forecast", rows * width, (1.0, 0.0, 0.0))]
        with torch.no_grad():
            _, feat = R.full_walk(sd, CFG_TWO_WIDTHS, xa, t, ctx, 0, branch)
            assert feat.shape[1] == width
            _close(got, R.cached_walk(sd, CFG_TWO_WIDTHS, xb, t, ctx, 0, branch, feat))


# ---- the samplers ------------------------------------------------------------------------------------------------------------------------
SOPS = vpred_ref.backend(dpm_ref)


@pytest.fixture()
def spied(sd, monkeypatch):
    """a SeerUNet whose forward is a spy: it writes down the cache_phase it is handed and returns 0.1 x"""
    m = _model(sd)
    seen = []

    def forward(self, sample, timestep, context, cond_frame=0, return_attn=False, **kw):
        assert set(kw) <= {"cache_phase"}
        seen.append(kw.get("cache_phase"))
        return 0.1 * sample
    monkeypatch.setattr(SeerUNet, "forward", forward)
    return m, seen


def _args(S, cfg=True, uc_tokens=77):
    x_T, c = _randn((1, 4, 2, 8, 8), 11), _randn((1, 2, 77, 256), 12)
    kw = dict(S=S, batch_size=1, shape=(4, 2, 8, 8), conditioning=c, verbose=False, eta=0.0, x_T=x_T, is_3d=True)
    if cfg:
        kw.update(unconditional_guidance_scale=7.5, unconditional_conditioning=_randn((1, 2, uc_tokens, 256), 13))
    return kw


# (S = 6 has stride 166 and therefore 7 schedule entries; PLMS's first step evaluates twice: 4 + 1)
@pytest.mark.parametrize("cls,S,want", [(DDIMSampler, 6, [0, 1, 2, 0, 1, 2, 0]), (PLMSSampler, 4, [0, 1, 2, 0, 1]),
                                        (DPMSolverSampler, 6, [0, 1, 2, 0, 1, 2, 0])], ids=["ddim", "plms", "dpm"])
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "plain"])
def test_samplers_hand_the_model_its_phase(spied, cls, S, want, cfg):
    m, seen = spied
    m.enable_step_cache(3, 1, 1)
    smp = cls("cpu", ops=SOPS)
    lat, _ = smp.sample(m, **_args(S, cfg))
    assert seen == want
    del seen[:]
    lat2, _ = smp.sample(m, **_args(S, cfg))            # a second sample begins a new chain
    assert seen == want and torch.equal(lat2, lat)
    # a plain callable is called as it always was, and the latents are those of a run no SeerUNet took part in
    calls = []

    def plain(x, t, c, cond_frame=0):
        calls.append(cond_frame)
        return 0.1 * x
    ref, _ = cls("cpu", ops=SOPS).sample(plain, **_args(S, cfg))
    assert len(calls) == len(want) and torch.equal(ref, lat)
    # off: the keyword is not passed at all
    m.disable_step_cache()
    del seen[:]
    smp.sample(m, **_args(S, cfg))
    assert seen == [None] * len(want)


def test_decode_restarts_and_encode_and_unbatched_cfg_pass_none(spied):
    m, seen = spied
    m.enable_step_cache(3, 1, 1)
    for cls in (DDIMSampler, DPMSolverSampler):
        smp = cls("cpu", ops=SOPS)
        smp.sample(m, **_args(4))
        assert seen == [0, 1, 2, 0]
        del seen[:]
        a = _args(4)
        smp.decode(m, a["x_T"], a["conditioning"], 3, unconditional_guidance_scale=7.5,
                   unconditional_conditioning=a["unconditional_conditioning"])
        assert seen == [0, 1, 2]                            # a chain of its own, from a full evaluation
        del seen[:]
    smp = DDIMSampler("cpu", ops=SOPS)
    smp.make_schedule(4, verbose=False)
    a = _args(4)
    smp.encode(m, a["x_T"], a["conditioning"], 3, unconditional_guidance_scale=7.5,
               unconditional_conditioning=a["unconditional_conditioning"])
    assert seen == [None] * 3                               # inversion: every step in full, the cache left alone
    del seen[:]
    smp.sample(m, **_args(4, uc_tokens=50))                 # uc of another length: two model calls per step
    assert seen == [None] * 8
    assert m._step_cache.k == 0                             # ... and the policy was not advanced


# ---- keys ----------------------------------------------------------------------------------------------------------------------------------
class _Seen(Exception):
    pass


def _key_of(eng, monkeypatch, fn):
    def graph_get(key):
        raise _Seen(key)
    monkeypatch.setattr(eng, "graph_get", graph_get)
    try:
        with pytest.raises(_Seen) as e:
            fn()
    finally:
        monkeypatch.undo()
    return e.value.args[0]


def test_graph_keys(models, monkeypatch):
    m = models[False]
    m.prepare(torch.bfloat16)
    eng = m._engine
    x, ctx, t = _randn((1, 4, 3, 8, 8), 1), _randn((1, 3, 77, 256), 2), torch.tensor([501])
    smp = DDIMSampler("cpu")
    smp.make_schedule(4, verbose=False)
    xs, x0e, c = _randn((1, 4, 2, 8, 8), 3), _randn((1, 4, 1, 8, 8), 4), _randn((1, 3, 77, 256), 5)

    def keys(kind="step"):
        monkeypatch.setattr(ddim_module, "capture_engine", lambda *a: eng)
        return _key_of(eng, monkeypatch, lambda: smp._step_graph(m, xs, c, None, x0e, 1, 1.0, kind))

    def unet_key(phase):
        c16, n = eng._context(ctx)
        return _key_of(eng, monkeypatch, lambda: eng._run_graph(x, t, c16, n, 1, phase))
    try:
        off = keys()
        assert off == ("step", (1, 4, 2, 8, 8), 1, False, 1, None, 77, (231, 256), False)       # the parent commit's tuple
        assert eng.step_cache_key == ()
        for b in BRANCHES:
            m.enable_step_cache(3, b, 1)
            assert eng.step_cache_key == ("cache", b)
            on = keys()
            assert on == off + ("cache", b)
            m.enable_step_cache(5, b, 2)                   # interval and order are policy: the same graph
            assert keys() == on
            assert keys("invert") == ("invert",) + off[1:]  # inversion runs in full: its key is what it was
            plain = unet_key(None)
            assert plain == ((1, 4, 3, 8, 8), 77, 1, (231, 256), False)
            assert unet_key(0) == plain + ("store", b) and unet_key(1) == unet_key(2) == plain + ("cached", b)
        m.disable_step_cache()
        assert keys() == off and eng.step_cache_key == ()
    finally:
        m.disable_step_cache()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(sd, models):
    m = _model(sd)
    for kw in (dict(interval=1), dict(interval=0), dict(branch=-1), dict(branch=L + 1), dict(order=3), dict(order=-1), dict(interval=2.5)):
        with pytest.raises(ValueError, match="enable_step_cache"):
            m.enable_step_cache(**kw)
    assert m._step_cache is None
    x, ctx, t = _inputs()
    with pytest.raises(ValueError, match="off"):
        m(x, t, ctx, cond_frame=COND, cache_phase=0)
    assert m.enable_step_cache() is m and (m._step_cache.interval, m._step_cache.branch, m._step_cache.order) == (3, 1, 1)
    with pytest.raises(ValueError, match="no full evaluation"):
        m(x, t, ctx, cond_frame=COND, cache_phase=1)                   # cold
    with pytest.raises(ValueError, match="return_attn"):
        m(x, t, ctx, cond_frame=COND, cache_phase=0, return_attn=True)
    with pytest.raises(ValueError, match="cache_phase"):
        m(x, t, ctx, cond_frame=COND, cache_phase=-1)
    m(x, t, ctx, cond_frame=COND, cache_phase=0)
    m(x, t, ctx, cond_frame=COND, cache_phase=1)
    # another shape, another branch, a new chain: cold again
    with pytest.raises(ValueError, match="no full evaluation"):
        m(x[:1], t[:1], ctx[:1], cond_frame=COND, cache_phase=1)
    m(x, t, ctx, cond_frame=COND, cache_phase=0)
    m.enable_step_cache(3, 0, 1)
    with pytest.raises(ValueError, match="no full evaluation"):
        m(x, t, ctx, cond_frame=COND, cache_phase=1)
    m(x, t, ctx, cond_frame=COND, cache_phase=0)
    ddim_module._begin_cache_chain(m)
    with pytest.raises(ValueError, match="no full evaluation"):
        m(x, t, ctx, cond_frame=COND, cache_phase=1)
    # the engine itself, without the model's checks
    with pytest.raises(ValueError, match="return_attn"):
        m._engine.run(x, t, ctx, COND, return_attn=True, cache_phase=0)
    with pytest.raises(ValueError, match="no full evaluation"):
        m._engine.run(x, t, ctx, COND, cache_phase=2, cache_weights=(1.0, 0.0, 0.0))
    # a sharded model
    with pytest.raises(ValueError, match="step cache"):
        parallel.attach(m, 1, 0)
    assert m._shard is None
    m.disable_step_cache()
    m._shard = object()
    try:
        with pytest.raises(ValueError, match="sharded"):
            m.enable_step_cache()
    finally:
        m._shard = None
    # slots and queues
    m.enable_step_cache()
    slot_kw = dict(shape=(4, 2, 8, 8), cond_frames=1, context_shape=(77, 256), device="cpu", ops=slot_ref, model_cond_frame=1)
    with pytest.raises(ValueError, match="SlotSampler"):
        SlotSampler(m, 2, **slot_kw)
    with pytest.raises(ValueError, match="generate_queue"):
        next(pipeline.generate_queue(m, None, None, [], slots=2, num_frames=3, cond_frames=1))
    m.disable_step_cache()
    slot = SlotSampler(m, 2, **slot_kw)
    m.enable_step_cache()
    with pytest.raises(ValueError, match="SlotSampler"):           # enabled after the sampler was built
        slot._run_step()
    m.disable_step_cache()


def test_library_refusals_without_gpu():
    """every SEER_EINVAL of the two entry points before the device is touched (aligned fake pointers, 64 KiB apart; with good
    arguments these calls would launch: only bad ones here)"""
    from seervideoldm_amd.build import build_library
    build_library()
    lib = _lib.load()
    X, RING, W = 0x10000, 0x40000, 0x90000
    n, stride = 1000, 1008                     # the ring spans 2 * 1008 + 1000 elements = 6032 bytes
    ok = dict(x=X, ring=RING, n=n, stride=stride, w=W, dt=_lib.SEER_DT_BF16)
    bad = [dict(x=None), dict(ring=None), dict(n=0), dict(n=-8), dict(stride=n - 1), dict(stride=992), dict(dt=2), dict(dt=-1),
           dict(x=X + 2), dict(x=X + 8), dict(ring=RING + 4), dict(stride=1004), dict(stride=1001),
           dict(x=RING), dict(x=RING + 16), dict(x=RING + 2 * 2016 + 1984), dict(x=RING - 1984), dict(ring=X + 1984)]
    for kw in bad:
        a = {**ok, **kw}
        assert lib.seer_cache_push(a["x"], a["ring"], a["n"], a["stride"], a["dt"], None) == -22, ("push", kw)
        assert lib.seer_cache_forecast(a["ring"], a["n"], a["stride"], a["w"], a["x"], a["dt"], None) == -22, ("forecast", kw)
    for kw in (dict(w=None), dict(w=W + 2)):
        a = {**ok, **kw}
        assert lib.seer_cache_forecast(a["ring"], a["n"], a["stride"], a["w"], a["x"], a["dt"], None) == -22, kw
    for dt in (_lib.SEER_DT_F16,):
        assert lib.seer_cache_push(None, RING, n, stride, dt, None) == -22
        assert lib.seer_cache_forecast(RING, n, stride, W, None, dt, None) == -22


# ---- surface -------------------------------------------------------------------------------------------------------------------------------
def test_surface(sd):
    assert "seer_cache_push" in _lib.SIGNATURES and "seer_cache_forecast" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["seer_cache_push"][0]) == 6 and len(_lib.SIGNATURES["seer_cache_forecast"][0]) == 7
    assert _lib.ABI_VERSION == 27
    assert set(STEP_KINDS) == {"step", "step-rng", "step-mask", "invert", "plms", "dpm"}
    m = _model(sd)
    assert m._step_cache is None                                     # off by default
    assert m.enable_step_cache(interval=4, branch=0, order=2) is m and m.disable_step_cache() is m and m._step_cache is None
    # an engine built later starts with the model's setting
    m.enable_step_cache(2, 1, 0)
    assert m._engine is None
    m.prepare(torch.bfloat16)
    assert m._engine.step_cache_key == ("cache", 1) and m._engine.cache_valid == 0
    m.disable_step_cache()
    assert m._engine.step_cache_key == ()


def test_compat_switch(monkeypatch):
    try:
        monkeypatch.setenv("SEER_COMPAT_STEP_CACHE", "3,1,1")
        compat.install()
        from seer.models.unet_3d_condition import SeerUNet as Aliased
        u = Aliased(**CFG_MINI)
        assert isinstance(u, SeerUNet) and Aliased.__name__ == "SeerUNet"
        assert (u._step_cache.interval, u._step_cache.branch, u._step_cache.order) == (3, 1, 1)
        compat.uninstall()
        monkeypatch.setenv("SEER_COMPAT_STEP_CACHE", "")
        compat.install()
        from seer.models.unet_3d_condition import SeerUNet as Plain
        assert Plain is SeerUNet
        compat.uninstall()
        compat.install(step_cache=(5, 0, 2))                         # the argument goes before the environment
        from seer.models.unet_3d_condition import SeerUNet as Aliased2
        p = Aliased2(**CFG_MINI)._step_cache
        assert (p.interval, p.branch, p.order) == (5, 0, 2)
        compat.uninstall()
        for bad in ("3,1", "a,b,c", "1,1,1", "3,-1,1", "3,1,3", "3;1;1", "3,1,1,0", "2.5,1,1"):
            monkeypatch.setenv("SEER_COMPAT_STEP_CACHE", bad)
            with pytest.raises(ValueError, match="SEER_COMPAT_STEP_CACHE"):
                compat.install()
    finally:
        compat.uninstall()
        monkeypatch.delenv("SEER_COMPAT_STEP_CACHE", raising=False)
        compat.install()
        compat.uninstall()
