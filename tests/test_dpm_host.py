"""DPMSolverSampler without a GPU: its coefficient table against the float64 restatement written from the definition
(tests/dpm_ref.py), the first-order row against the eta = 0 DDIM update, the log-SNR grid, the solver's accuracy on the analytic
Gaussian model through DPMSolverSampler("cpu", ops=tests.dpm_ref).sample, the order rule, every refusal, the compat switch, and
ddim_sample / generate_clips driving it.  Runs everywhere (CPU)."""
import inspect
import math

import numpy as np
import pytest
import torch

from seervideoldm_amd import DDIMSampler, DPMSolverSampler, PLMSSampler, compat, ddim, ddim_sample, pipeline
from tests import dpm_ref as R

f64 = torch.float64
GRIDS = ("uniform", "logsnr")


def _sampler(S, grid="uniform", ops=R, **kw):
    smp = DPMSolverSampler("cpu", discretize=grid, ops=ops, **kw)
    smp.make_schedule(S, verbose=False)
    return smp


def _rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("S", [10, 20, 50])
def test_table_against_the_definition(S, grid):
    """every row of the fp32 table, applied in float64 to random (x, eps, D_prev), against the update written in lambda, h and r:
    1e-6 relative, a few roundings of a 2^-24 format with no cancellation between the terms"""
    smp = _sampler(S, grid)
    n = smp.ddim_timesteps.shape[0]
    assert tuple(smp.dpm_coef.shape) == (n, 6) and smp.dpm_coef.dtype == torch.float32
    g = torch.Generator().manual_seed(S)
    x, e, dp = (torch.randn((257,), generator=g, dtype=f64) for _ in range(3))
    table = smp.dpm_coef.double()
    for i in range(n):
        s0, ia, cx, c1, c2, cp = table[i].tolist()
        d = (x - s0 * e) * ia
        want1, want_d = R.step64(e, x, smp.ddim_alphas, smp.ddim_alphas_prev, i, 1)
        assert _rel(d, want_d) <= 1e-6 and _rel(cx * x + c1 * d, want1) <= 1e-6, i
        if i < n - 1:
            want2, _ = R.step64(e, x, smp.ddim_alphas, smp.ddim_alphas_prev, i, 2, dp)
            assert _rel(cx * x + c2 * d + cp * dp, want2) <= 1e-6, i
        else:                                            # no entry above the top one: its second-order words are the first-order ones
            assert c2 == c1 and cp == 0.0


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("S", [10, 20, 50])
def test_first_order_row_is_the_deterministic_ddim_update(S, grid):
    smp = _sampler(S, grid)
    g = torch.Generator().manual_seed(S + 1)
    x, e = (torch.randn((257,), generator=g, dtype=f64) for _ in range(2))
    for i in range(smp.ddim_timesteps.shape[0]):
        a_t, a_prev, sigma, s1m = smp.ddim_coef[i].double().tolist()
        assert sigma == 0.0
        x0 = (x - s1m * e) / math.sqrt(a_t)
        ddim_prev = math.sqrt(a_prev) * x0 + math.sqrt(1.0 - a_prev) * e
        s0, ia, cx, c1, _, _ = smp.dpm_coef[i].double().tolist()
        d = (x - s0 * e) * ia
        assert _rel(d, x0) <= 1e-6 and _rel(cx * x + c1 * d, ddim_prev) <= 1e-6, i


@pytest.mark.parametrize("S", [1, 2, 10, 20, 50, 100, 999])
def test_logsnr_timesteps(S):
    smp = _sampler(S, "logsnr")
    ts = smp.ddim_timesteps
    assert ts.dtype == np.int64 and 1 <= len(ts) <= S
    assert np.all(np.diff(ts) > 0) and ts[0] >= 1 and ts[-1] <= 999
    if S >= 2:
        assert ts[0] == 1 and ts[-1] == 999
    # the tables are DDIMSampler's over these steps: a_prev of entry i is a_t of entry i - 1, the last step lands on alphas_cumprod[0]
    ac = smp.alphas_cumprod.double().numpy()
    assert np.array_equal(smp.ddim_alphas, ac[ts]) and smp.ddim_alphas_prev[0] == ac[0]
    assert np.array_equal(smp.ddim_alphas_prev[1:], ac[ts[:-1]])
    assert torch.equal(smp._t_table, torch.from_numpy(ts))
    if S == 20:                                          # evenly spaced in lambda, to the resolution of a training step
        lam = [0.5 * math.log(a / (1 - a)) for a in ac.tolist()]
        assert len(ts) == 20
        for k, t in enumerate(ts.tolist()):
            target = lam[1] + (lam[999] - lam[1]) * k / 19
            assert abs(lam[t] - target) <= min(abs(lam[u] - target) for u in range(1, 1000)) + 1e-12, (k, t)


def test_uniform_schedule_is_ddims():
    d = DDIMSampler("cpu")
    d.make_schedule(30, verbose=False)
    p = _sampler(30)
    assert np.array_equal(p.ddim_timesteps, d.ddim_timesteps) and len(p.ddim_timesteps) == 31
    assert torch.equal(p.ddim_coef, d.ddim_coef) and torch.equal(p._t_table, d._t_table)


# ---- 2. the solver on the analytic model ----------------------------------------------------------------------------------------------
def _errors(run):
    x_T = R.start_codes()
    err = {}
    for method, grid, S in R.ACCURACY_CASES:
        smp = _sampler(S, grid) if method == "2m" else DDIMSampler("cpu", ops=R)
        smp.make_schedule(S, verbose=False)
        err[method, grid, S] = R.max_error(run(method, smp, S, x_T), smp, x_T)
    return err


def test_accuracy_on_the_gaussian_probability_flow_ode():
    """the three conditions, for the float64 restatement and for the sampler's own fp32 chain over the torch stand-in"""
    def run64(method, smp, S, x_T):
        eps, _ = R.gaussian(smp.alphas_cumprod)
        if method == "ddim":
            return R.ddim_sampling64(eps, x_T, smp.ddim_alphas, smp.ddim_alphas_prev, smp.ddim_timesteps)
        return R.sampling64(eps, x_T, smp.ddim_alphas, smp.ddim_alphas_prev, smp.ddim_timesteps)[0]

    def run32(method, smp, S, x_T):
        eps, _ = R.gaussian(smp.alphas_cumprod)
        model = lambda x, t, c, cond_frame=0: eps(x, t).float()
        return smp.sample(model, S, x_T.shape[0], x_T.shape[1:], conditioning=torch.zeros((1, 1, 1, 1)), x_T=x_T.float(),
                          verbose=False, is_3d=True)[0]
    e64, e32 = _errors(run64), _errors(run32)
    print(f"[dpm] float64 {e64}\n[dpm] sampler {e32}")
    R.assert_accuracy(e64)
    R.assert_accuracy(e32)
    for k in e64:                                        # the fp32 chain is the restated one
        assert abs(e32[k] - e64[k]) <= 1e-4 + 1e-2 * e64[k], (k, e32[k], e64[k])


def test_sample_follows_the_restatement_step_by_step():
    """with guidance and conditioning frames, every latent and every pred_x0 of a chain"""
    smp = _sampler(10, "logsnr")
    eps, _ = R.gaussian(smp.alphas_cumprod)
    b, C, f1, Fp, h, w = 2, 3, 2, 3, 4, 5
    g = torch.Generator().manual_seed(1)
    shift = 0.2 * torch.randn((b, C, Fp, h, w), generator=g, dtype=f64)

    def model(x, t, c, cond_frame=0):
        """rows [uc | c]: the conditional half sees another mean; the conditioning frames' output is sliced off by the update"""
        lat = x[:, :, f1:].double()
        off = torch.cat([torch.zeros_like(shift), shift]) if x.shape[0] == 2 * b else shift
        return torch.cat([torch.zeros_like(x[:, :, :f1]), (eps(lat - off, t)).float()], 2)
    eps64 = lambda x, t: eps(x, t) + 7.5 * (eps(x - shift, t) - eps(x, t))
    x_T = torch.randn((b, C, Fp, h, w), generator=g)
    x0_emb, c = torch.randn((b, C, f1, h, w), generator=g), torch.zeros((b, f1 + Fp, 1, 1))
    preds = []
    lat, inter = smp.sample(model, 10, b, (C, Fp, h, w), x0_emb=x0_emb, conditioning=c, x_T=x_T, verbose=False, is_3d=True,
                            unconditional_guidance_scale=7.5, unconditional_conditioning=torch.ones_like(c), cond_frames=f1,
                            log_every_t=1, img_callback=lambda p, i: preds.append(p))
    want, steps = R.sampling64(eps64, x_T, smp.ddim_alphas, smp.ddim_alphas_prev, smp.ddim_timesteps)
    assert [k for _, _, k in steps] == [1] + [2] * 8 + [1]
    assert len(inter["x_inter"]) == len(steps) + 1 == len(preds) + 1
    for got_x, got_d, (x_prev, d, _) in zip(inter["x_inter"][1:], preds, steps):
        assert _rel(got_x, x_prev) <= 1e-5 and _rel(got_d, d) <= 1e-5
    assert _rel(lat, want) <= 1e-5 and lat.dtype == torch.float32


# ---- 3. the order rule ----------------------------------------------------------------------------------------------------------------
class _Recording:
    """tests.dpm_ref with (index, order, whether d_prev was handed over) of every update recorded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(R, name)
        if name != "cfg_dpm_step":
            return fn

        def recorded(eps, x, coef, index, order, **kw):
            self.calls.append((int(index), int(order), kw.get("d_prev") is not None))
            return fn(eps, x, coef, index, order, **kw)
        return recorded


def _recorded_chain(S, grid="uniform", **kw):
    rec = _Recording()
    smp = _sampler(S, grid, rec, **kw)
    model = lambda x, t, c, cond_frame=0: 0.1 * x
    smp.sample(model, S, 1, (2, 1, 2, 2), conditioning=torch.zeros((1, 1, 1, 1)), x_T=torch.ones((1, 2, 1, 2, 2)), verbose=False,
               is_3d=True)
    n = smp.ddim_timesteps.shape[0]
    assert [c[0] for c in rec.calls] == list(reversed(range(n)))
    return [c[1] for c in rec.calls], [c[2] for c in rec.calls]


def test_order_and_lower_order_final():
    orders, hist = _recorded_chain(10)
    assert orders == [1] + [2] * 8 + [1] and hist == [o == 2 for o in orders]         # 10 entries end first order
    orders, _ = _recorded_chain(20)
    assert orders == [1] + [2] * 19                                                 # 20 entries end second order
    orders, _ = _recorded_chain(14)
    assert len(orders) == 15 and orders[-1] == 2                                    # the rule counts entries, not S: 14 -> 15 entries
    orders, _ = _recorded_chain(10, lower_order_final=False)
    assert orders == [1] + [2] * 9
    orders, hist = _recorded_chain(10, order=1)
    assert orders == [1] * 10 and not any(hist)                                     # order 1 never reads history
    orders, hist = _recorded_chain(20, "logsnr", order=1)
    assert set(orders) == {1} and not any(hist)


def test_decode_starts_first_order_from_t_start():
    rec = _Recording()
    smp = _sampler(20, "uniform", rec)
    model = lambda x, t, c, cond_frame=0: 0.1 * x
    x, c = torch.ones((1, 2, 1, 2, 2)), torch.zeros((1, 1, 1, 1))
    got = smp.decode(model, x, c, 7, seed=3)
    assert rec.calls == [(6, 1, False)] + [(i, 2, True) for i in (5, 4, 3, 2, 1, 0)]
    d_prev, want = None, x
    for i in reversed(range(7)):
        want, d_prev = smp.p_sample_dpm(model, want, c, smp._t_table[i].expand(1), i, d_prev=d_prev)
    assert torch.equal(got, want)
    # encode and stochastic_encode are DDIMSampler's
    assert DPMSolverSampler.encode is DDIMSampler.encode and DPMSolverSampler.stochastic_encode is DDIMSampler.stochastic_encode
    d = DDIMSampler("cpu", ops=R)
    d.make_schedule(20, verbose=False)
    up, _ = smp.encode(model, x, c, 5)
    assert torch.equal(up, d.encode(model, x, c, 5)[0])


def test_rng_draws_follow_plms_convention():
    smp = _sampler(10)
    model = lambda x, t, c, cond_frame=0: 0.1 * x
    kw = dict(conditioning=torch.zeros((1, 1, 1, 1)), x_T=torch.ones((1, 2, 1, 2, 2)), verbose=False, is_3d=True)
    torch.manual_seed(5)
    smp.sample(model, 10, 1, (2, 1, 2, 2), **kw)
    after = torch.rand(3)
    torch.manual_seed(5)
    for _ in range(10):
        torch.randn((1, 2, 1, 2, 2))
    assert torch.equal(after, torch.rand(3))
    smp.consume_rng_when_deterministic = False
    torch.manual_seed(5)
    before = torch.get_rng_state()
    smp.sample(model, 10, 1, (2, 1, 2, 2), **kw)
    assert torch.equal(torch.get_rng_state(), before)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    s = DPMSolverSampler("cpu", ops=R)
    kw = dict(unet=None, S=4, batch_size=1, shape=(4, 2, 8, 8), verbose=False, is_3d=True)
    with pytest.raises(ValueError, match="DPM-Solver"):
        s.make_schedule(4, ddim_eta=0.1, verbose=False)
    with pytest.raises(ValueError, match="DPM-Solver"):
        s.sample(**{**kw, "eta": 0.1})
    x = torch.zeros((1, 4, 2, 8, 8))
    for bad in (dict(mask=torch.ones((1, 1, 2, 8, 8)), x0=x), dict(mask=torch.ones((1, 1, 2, 8, 8))), dict(x0=x), dict(seed=3),
                dict(noise_dropout=0.1)):
        with pytest.raises(NotImplementedError, match="DPM-Solver"):
            s.sample(**{**kw, **bad})
    with pytest.raises(NotImplementedError):
        s.sample(**{**kw, "shape": (4, 8, 8), "is_3d": False})
    with pytest.raises(NotImplementedError, match="logsnr"):
        DPMSolverSampler("cpu", discretize="quad").make_schedule(4, verbose=False)
    for order in (0, 3):
        with pytest.raises(NotImplementedError, match="DPM-Solver"):
            DPMSolverSampler("cpu", order=order)
    s.make_schedule(4, verbose=False)
    t = torch.ones(1, dtype=torch.long)
    for bad in (dict(noise_dropout=0.5), dict(use_original_steps=True), dict(repeat_noise=True), dict(quantize_denoised=True),
                dict(score_corrector=object())):
        with pytest.raises(NotImplementedError):
            s.p_sample_dpm(None, x, None, t, 3, **bad)
    with pytest.raises(NotImplementedError, match="p_sample_dpm"):
        s.p_sample_ddim(None, x, None, t, 3)
    with pytest.raises(NotImplementedError, match="dpm_sampling"):
        s.ddim_sampling(None, None, x.shape, True)
    for bad in (0, 5):
        with pytest.raises(ValueError, match="t_start"):
            s.decode(None, x, None, bad)
    with pytest.raises(NotImplementedError):
        s.decode(None, x, None, 2, use_original_steps=True)
    with pytest.raises(NotImplementedError, match="mask"):
        s.decode(None, x, None, 2, mask=torch.ones((1, 1, 2, 8, 8)), x0=x)
    # the stand-in and the binding refuse the same things
    e, table = torch.zeros((1, 4, 2, 8, 8)), s.dpm_coef
    for args in ((4, 1), (-1, 1), (1, 0), (1, 3), (1, 2)):                            # order 2 without d_prev last
        with pytest.raises(ValueError):
            R.cfg_dpm_step(e, x, table, *args, cfg=False, scale=1.0, cond_f=0)


def test_surface():
    from seervideoldm_amd import _lib, ops
    from seervideoldm_amd.ddim import STEP_KINDS
    import seervideoldm_amd
    assert "DPMSolverSampler" in seervideoldm_amd.__all__
    assert "seer_cfg_dpm_step" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 27                        # declarations only: no struct changed
    assert callable(ops.cfg_dpm_step) and callable(ops.cfg_dpm_step_dev) and ops.DPM_ROW_WORDS == 6
    assert "dpm" in STEP_KINDS
    ours, theirs = inspect.signature(DPMSolverSampler.sample).parameters, inspect.signature(DDIMSampler.sample).parameters
    assert list(ours) == list(theirs) and all(ours[k].default == theirs[k].default for k in ours)
    init = inspect.signature(DPMSolverSampler.__init__).parameters
    assert (init["order"].default, init["lower_order_final"].default, init["discretize"].default) == (2, True, "uniform")
    assert list(inspect.signature(DPMSolverSampler.decode).parameters) == list(inspect.signature(DDIMSampler.decode).parameters)


# ---- 5. compat ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def compat_env(monkeypatch):
    yield monkeypatch
    compat.uninstall()


@pytest.mark.parametrize("how", ["env", "argument", "upper"])
def test_compat_dpmpp(compat_env, how):
    if how == "argument":
        compat_env.delenv("SEER_COMPAT_SAMPLER", raising=False)
        compat.install(sampler="dpmpp")
    else:
        compat_env.setenv("SEER_COMPAT_SAMPLER", "dpmpp" if how == "env" else " DPMPP ")
        compat.install()
    from ldm.models.diffusion.ddim_video import DDIMSampler as Aliased
    assert Aliased is DPMSolverSampler


@pytest.mark.parametrize("value,cls", [(None, DDIMSampler), ("", DDIMSampler), ("ddim", DDIMSampler), ("plms", PLMSSampler),
                                       ("dpm", DDIMSampler), ("dpmpp2m", DDIMSampler)])
def test_compat_other_values_behave_as_before(compat_env, value, cls):
    if value is None:
        compat_env.delenv("SEER_COMPAT_SAMPLER", raising=False)
    else:
        compat_env.setenv("SEER_COMPAT_SAMPLER", value)
    compat.install()
    from ldm.models.diffusion.ddim_video import DDIMSampler as Aliased
    assert Aliased is cls


# ---- 6. the drivers -------------------------------------------------------------------------------------------------------------------
class _Dist:
    def sample(self, generator=None):
        return torch.full((2, 4, 2, 2), 0.5)             # 1 clip x 2 conditioning frames


class _Vae:
    def encode(self, frames):
        return type("E", (), {"latent_dist": _Dist()})()


class _Fst:
    def set_numframe(self, n):
        self.frames = n

    def __call__(self, context):
        return context.unsqueeze(1).expand(-1, self.frames, -1, -1)


def test_ddim_sample_and_generate_clips_drive_it(monkeypatch):
    monkeypatch.setattr(ddim, "latents_to_clip", lambda vae, latents: latents)
    smp = DPMSolverSampler("cpu", ops=R)
    eps, _ = R.gaussian(_sampler(4).alphas_cumprod)
    calls = []

    def model(x, t, c, cond_frame=0):
        calls.append((tuple(x.shape), cond_frame))
        return eps(x, t).float()
    b, C, f1, Fp, h = 1, 4, 2, 3, 2
    g = torch.Generator().manual_seed(2)
    x_T, x0_emb = torch.randn((b, C, Fp, h, h), generator=g), torch.randn((b, C, f1, h, h), generator=g)
    c, uc = torch.zeros((b, f1 + Fp, 2, 3)), torch.ones((b, f1 + Fp, 2, 3))
    got = ddim_sample(smp, model, None, (b, C, Fp, h, h), c, x_T, x0_emb, ddim_steps=10, scale=7.5, uc=uc)
    assert len(calls) == 10 and calls[0] == ((2 * b, C, f1 + Fp, h, h), 0)
    want, _ = _sampler(10).sample(model, 10, b, (C, Fp, h, h), x0_emb=x0_emb, conditioning=c, x_T=x_T, verbose=False, is_3d=True,
                                  unconditional_guidance_scale=7.5, unconditional_conditioning=uc)
    assert torch.equal(got, want) and torch.isfinite(got).all()
    del calls[:]
    clips = pipeline.generate_clips(model, _Fst(), _Vae(), smp, torch.zeros((b, 3, 1, 16, 16)), torch.zeros((b, 2, 3)),
                                    torch.ones((b, 2, 3)), num_frames=f1 + Fp, cond_frames=f1, ddim_steps=20, scale=7.5,
                                    num_samples=2, noise_generator=torch.Generator().manual_seed(4))
    assert len(clips) == 2 and clips[0].shape == (b, C, Fp, h, h) and len(calls) == 40
    assert all(torch.isfinite(k).all() for k in clips) and not torch.equal(clips[0], clips[1])


# ---- 7. the entry points' refusals ----------------------------------------------------------------------------------------------------
def refusal_cases(P, W):
    """(entry point, arguments without the stream, what is wrong) for every refusal of the entry point's two forms.  P stands for every fp32
    buffer and W for the two int32 ones; both are 4-byte aligned and non-NULL (tests/test_gpu_dpm.py passes real ones)"""
    good = dict(eps=P, cfg=1, b=2, C=4, F_total=5, cond_f=2, HW=96, scale=7.5, x=P, coef=P, nsched=10, index=3, order=2, step=None, state=None,
                d_prev=P, x_prev=P, pred_x0=P)
    for kw in (dict(eps=None), dict(x=None), dict(coef=None), dict(x_prev=None), dict(d_prev=None), dict(b=0), dict(b=-1), dict(C=0),
               dict(HW=0), dict(HW=-4), dict(cond_f=-1), dict(cond_f=5), dict(cond_f=6), dict(F_total=0, cond_f=0), dict(nsched=0),
               dict(index=-1), dict(index=10), dict(index=11), dict(order=0), dict(order=3), dict(order=-1), dict(eps=P + 2),
               dict(x=P + 2), dict(coef=P + 1), dict(d_prev=P + 2), dict(x_prev=P + 3), dict(pred_x0=P + 2),
               dict(b=1 << 16, C=1 << 16, F_total=1 << 8, cond_f=0, HW=1),                   # 2^40 elements: a grid beyond one dimension
               dict(state=W), dict(step=W)):                                                 # a half-set device form
        yield "seer_cfg_dpm_step", tuple({**good, **kw}.values()), kw
    # the device form: pred_x0 is the history (d_hist of ABI <= 26)
    good = dict(eps=P, cfg=1, b=2, C=4, F_total=5, cond_f=2, HW=96, scale=7.5, x=P, coef=P, nsched=10, index=-1, order=0, step=W, state=W,
                d_prev=None, x_prev=P, pred_x0=P)
    for kw in (dict(eps=None), dict(x=None), dict(coef=None), dict(step=None), dict(state=None), dict(x_prev=None), dict(pred_x0=None),
               dict(b=0), dict(C=0), dict(HW=0), dict(cond_f=-1), dict(cond_f=5), dict(nsched=0), dict(nsched=-3), dict(eps=P + 2),
               dict(x=P + 1), dict(coef=P + 2), dict(step=W + 2), dict(state=W + 1), dict(x_prev=P + 2), dict(pred_x0=P + 3),
               dict(index=3), dict(d_prev=P)):
        yield "seer_cfg_dpm_step", tuple({**good, **kw}.values()), kw


def test_kernel_entry_points_refuse_bad_arguments_before_any_launch():
    """every refusal returns SEER_EINVAL on the host (16 = an aligned non-NULL pointer; no call here would pass its checks, so
    nothing is launched)"""
    from seervideoldm_amd import _lib
    from seervideoldm_amd.build import build_library
    build_library()
    lib = _lib.load()
    n = 0
    for fn, args, why in refusal_cases(16, 16):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    assert n >= 45
