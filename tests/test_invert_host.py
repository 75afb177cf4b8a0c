"""DDIM inversion without a GPU: DDIMSampler("cpu", ops=tests.invert_ref).encode against its float64 restatement over the oracle's tiny
UNet (every step, every CFG form), the solver on the analytic Gaussian model with a closed-form answer (accuracy, first-order
convergence, the round trip against stochastic_encode's), the argument checks, torch's generator, the coefficient rows an encode /
decode pair visits, edit_clips(invert=True) and PLMSSampler.  Runs everywhere (CPU)."""
import inspect

import numpy as np
import pytest
import torch

from oracle import seer_oracle as O
from seervideoldm_amd import DDIMSampler, PLMSSampler, pipeline, synth
from tests import invert_ref as R
from tests import plms_oracle as P
from tests.test_plms_host import TINY_UNET

f64 = torch.float64
B, F1, FP, H = 1, 1, 2, 16


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def _sampler(S, cls=DDIMSampler, ops=R):
    smp = cls("cpu", ops=ops)
    smp.make_schedule(S, verbose=False)
    return smp


@pytest.fixture(scope="module")
def tiny():
    sd = synth.synth_state_dict(synth.unet_param_shapes(TINY_UNET))
    unet_fn = lambda x, t, c, cf: O.unet_forward(sd, TINY_UNET, x, t, c, cond_frame=cf)
    model = lambda x, t, c, cond_frame=0: unet_fn(x, t, c, cond_frame)
    return unet_fn, model


# ---- 1. encode over the tiny UNet against float64, step by step ------------------------------------------------------------------
@pytest.mark.parametrize("cond_frames", [0, 1])
@pytest.mark.parametrize("form", ["batched", "unbatched", "plain"])
def test_encode_follows_its_float64_restatement(tiny, form, cond_frames):
    """the model runs in fp32 on both sides (the oracle's UNet); the update is fp32 torch arithmetic on ours, float64 on the
    restatement's.  test_plms_host.py's tolerances: a step, and the sample.

    S = 4 has the rows a_prev -> a_t = 0.9999 -> 0.9998 -> 0.82 -> 0.33 -> 0.038.  Without guidance all four run.  With guidance 7.5
    the chain stops at row 2: upward, on random weights, guidance makes the two chains -- which feed the model latents that differ by
    an fp32 rounding -- drift apart by about 3x per row (measured: |x_next - x_next64| 3e-7, 1.5e-5, 4.2e-5, 1.4e-4 over rows 0..3, and
    in row 3 pred_x0 reaches 14 with a difference of 3.0e-4 to 4.4e-4, past 2e-4 + 1e-4 |pred_x0| in three of the four guided
    cases).  That drift is the model's sensitivity, the same for any two fp32 roundings of one chain, not the update's error; the
    update on row 3 is checked here unguided and, per element with a derived bound, in tests/test_gpu_invert.py."""
    unet_fn, model = tiny
    x0_emb, x0 = _randn((B, 4, F1, H, H), 60) * 0.9, _randn((B, 4, FP, H, H), 63) * 0.8
    c = _randn((B, F1 + FP, 77, 64), 61)
    # uc with c's token count takes the batched CFG branch, any other the two-call branch (ddim_video.py:200-207)
    uc = _randn((B, 1, 50 if form == "unbatched" else 77, 64), 62).expand(-1, F1 + FP, -1, -1).contiguous()
    scale = 1.0 if form == "plain" else 7.5
    smp = _sampler(4)
    assert smp.ddim_coef.shape[0] == 4
    n = 4 if form == "plain" else 3
    lat, inter = smp.encode(model, x0, c, n, return_intermediates=1, unconditional_guidance_scale=scale,
                            unconditional_conditioning=uc, x0_emb=x0_emb, cond_frames=cond_frames)
    eps_fn = lambda x, t: P.model_eps(unet_fn, x.float(), c, t, x0_emb, scale, uc, cond_frames).double()
    with torch.no_grad():
        want, steps = R.encode64(eps_fn, x0, smp.ddim_coef, smp.ddim_timesteps, n)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == len(steps) == n
    for i, (x_next, pred_x0) in enumerate(steps):
        torch.testing.assert_close(inter["x_inter"][i], x_next.float(), rtol=1e-4, atol=1e-4, msg=f"{form} step {i} x_next")
        torch.testing.assert_close(inter["pred_x0"][i], pred_x0.float(), rtol=1e-4, atol=2e-4, msg=f"{form} step {i} pred_x0")
    torch.testing.assert_close(lat, want.float(), rtol=1e-3, atol=1e-3)
    assert torch.equal(lat, inter["x_inter"][-1]) and lat.dtype == torch.float32
    # every k-th latent, and none when nobody asks
    _, sparse = smp.encode(model, x0, c, 2, return_intermediates=2, unconditional_guidance_scale=scale,
                           unconditional_conditioning=uc, x0_emb=x0_emb, cond_frames=cond_frames)
    assert len(sparse["x_inter"]) == 1 and torch.equal(sparse["x_inter"][0], inter["x_inter"][1])
    assert torch.equal(sparse["pred_x0"][0], inter["pred_x0"][1])


# ---- 2. the solver on the analytic Gaussian model ---------------------------------------------------------------------------------
def _gaussian_round_trips(S):
    """-> figures of the float64 restatement and of the sampler's own fp32 chain (ops = the torch stand-in) on the same case"""
    smp = _sampler(S)
    n = int(smp.ddim_timesteps.shape[0])
    G = R.gaussian_case(smp.alphas_cumprod)
    coef, ts, x0 = smp.ddim_coef, smp.ddim_timesteps, G["x0"]
    exact = G["flow"](x0, float(coef[0, 1]), float(coef[n - 1, 0]))
    noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9), dtype=f64)
    lat64, _ = R.encode64(G["eps"], x0, coef, ts, n)
    back64 = R.decode64(G["eps"], lat64, coef, ts, n)
    a_top = float(coef[n - 1, 0])
    sde64 = R.decode64(G["eps"], a_top ** 0.5 * x0 + (1 - a_top) ** 0.5 * noise, coef, ts, n)
    fig64 = dict(end=_rel(lat64, exact), trip=_rel(back64, x0), sde=_rel(sde64, x0))
    model = lambda x, t, c, cond_frame=0: G["eps"](x, t).float()
    c = torch.zeros((1, x0.shape[2], 1, 1))
    lat, _ = smp.encode(model, x0.float(), c, n)
    back = smp.decode(model, lat, c, n)
    sde = smp.decode(model, smp.stochastic_encode(x0.float(), n - 1, noise=noise.float()), c, n)
    fig32 = dict(end=_rel(lat, exact), trip=_rel(back, x0), sde=_rel(sde, x0))
    return fig64, fig32, (_rel(lat, lat64), _rel(back, back64))


def test_inversion_on_the_gaussian_probability_flow_ode():
    """N = 20 000 elements, data N(mu, 0.5^2), the exact eps, no guidance, t_enc = the whole schedule.  Computed in float64: the
    inversion is 6.5e-2 from the closed-form end point at S = 20; the round-trip error at S = 50 is 0.42 of that at S = 20 (first
    order in the step); the inversion's round trip at S = 20, 9.8e-2, is 1/12 of stochastic_encode's, 1.15."""
    f20, s20, close20 = _gaussian_round_trips(20)
    f50, s50, close50 = _gaussian_round_trips(50)
    print(f"[invert] float64 S=20 {f20}  S=50 {f50}")
    print(f"[invert] sampler S=20 {s20}  S=50 {s50}; fp32 chain to float64 {close20} {close50}")
    for fig20, fig50 in ((f20, f50), (s20, s50)):
        assert fig20["end"] <= 8e-2, fig20
        assert fig50["trip"] <= 0.6 * fig20["trip"], (fig20, fig50)
        assert fig20["trip"] <= fig20["sde"] / 5, fig20
    assert max(close20 + close50) <= 1e-5, (close20, close50)         # the sampler's fp32 chain is the restated one


# ---- 3. argument checks, the generator, exports -----------------------------------------------------------------------------------
def test_refusals_and_rng():
    smp = _sampler(4)
    x0, c = torch.zeros((1, 4, 2, 2, 2)), torch.zeros((1, 2, 1, 1))
    model = lambda x, t, c, cond_frame=0: torch.full_like(x, 0.5)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="t_enc"):
            smp.encode(model, x0, c, bad)
    with pytest.raises(NotImplementedError):
        smp.encode(model, x0, c, 2, use_original_steps=True)
    with pytest.raises(ValueError, match="return_intermediates"):
        smp.encode(model, x0, c, 2, return_intermediates=0)
    for index, limit in ((-1, None), (4, None), (2, 2), (0, 5)):
        with pytest.raises(ValueError, match="index"):
            smp.p_invert_ddim(model, x0, c, smp._t_table[0].expand(1), index, limit=limit)
    # nothing is drawn: the generator is where it was, whatever the sampler does when it samples
    assert smp.consume_rng_when_deterministic
    torch.manual_seed(5)
    before = torch.get_rng_state()
    seen = []
    lat, inter = smp.encode(model, x0, c, 4, callback=seen.append)
    assert torch.equal(torch.get_rng_state(), before)
    assert seen == [0, 1, 2, 3] and inter == {"x_inter": [], "pred_x0": []} and torch.isfinite(lat).all()
    assert not torch.equal(lat, x0) and torch.equal(x0, torch.zeros_like(x0))          # the caller's latent is not written


def test_exports():
    from seervideoldm_amd import _lib, ops
    from seervideoldm_amd.ddim import STEP_KINDS
    assert "seer_cfg_ddim_invert_step" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 27                        # declarations only: no struct changed
    for name in ("cfg_ddim_invert_step", "cfg_ddim_invert_step_dev"):
        assert callable(getattr(ops, name)), name
    assert callable(R.cfg_ddim_invert_step) and callable(R.cfg_ddim_step) and callable(R.q_sample)
    assert {"step", "step-rng", "step-mask", "invert"} <= set(STEP_KINDS)
    enc = inspect.signature(DDIMSampler.encode).parameters
    assert list(enc)[1:10] == ["unet", "x0", "c", "t_enc", "use_original_steps", "return_intermediates",
                               "unconditional_guidance_scale", "unconditional_conditioning", "callback"]
    assert enc["x0_emb"].kind is enc["cond_frames"].kind is inspect.Parameter.KEYWORD_ONLY
    ec = inspect.signature(pipeline.edit_clips).parameters
    assert ec["invert"].default is False and ec["source_emb"].default is None and ec["source_scale"].default == 1.0
    assert ec["seed"].default is inspect.Parameter.empty


# ---- 4. encode and decode walk the same rows --------------------------------------------------------------------------------------
class _Recording:
    """tests.invert_ref with the coefficient row of every update recorded"""

    def __init__(self):
        self.rows = []

    def __getattr__(self, name):
        fn = getattr(R, name)
        if name not in ("cfg_ddim_invert_step", "cfg_ddim_step"):
            return fn

        def recorded(eps, x, coef, index, **kw):
            self.rows.append((name, int(index)))
            return fn(eps, x, coef, index, **kw)
        return recorded


def test_encode_then_decode_visit_the_same_rows_in_reverse():
    rec = _Recording()
    smp = _sampler(6, DDIMSampler, rec)                  # 7 entries
    G = R.gaussian_case(smp.alphas_cumprod, shape=(2, 4, 2, 3, 5))
    model = lambda x, t, c, cond_frame=0: G["eps"](x, t).float()
    c = torch.zeros((2, 2, 1, 1))
    lat, _ = smp.encode(model, G["x0"].float(), c, 5)
    up, rec.rows = rec.rows, []
    smp.decode(model, lat, c, 5)
    assert up == [("cfg_ddim_invert_step", i) for i in range(5)]
    assert rec.rows == [("cfg_ddim_step", i) for i in reversed(range(5))]
    # PLMSSampler inherits encode as it is: the same chain, the same bits, and its RNG draws stay out of it
    torch.manual_seed(5)
    before = torch.get_rng_state()
    got, _ = _sampler(6, PLMSSampler, R).encode(model, G["x0"].float(), c, 5)
    assert torch.equal(got, lat) and torch.equal(torch.get_rng_state(), before)


# ---- 5. edit_clips(invert=True) ---------------------------------------------------------------------------------------------------
class _Dist:
    def sample(self, generator=None):
        return torch.ones((3, 4, 2, 2))                  # 1 clip x 3 frames


class _Vae:
    def encode(self, frames):
        return type("E", (), {"latent_dist": _Dist()})()


class _Fst:
    def set_numframe(self, n):
        self.frames = n

    def __call__(self, context):
        return context.unsqueeze(1).expand(-1, self.frames, -1, -1)


class _EditSampler:
    def __init__(self):
        self.calls = []

    def make_schedule(self, ddim_num_steps, ddim_eta=0.0, verbose=True):
        self.ddim_timesteps = np.arange(ddim_num_steps)

    def encode(self, unet, x0, c, t_enc, **kw):
        self.calls.append(("encode", c, t_enc, kw))
        return x0 + 1.0, {}

    def decode(self, unet, x_latent, cond, t_start, **kw):
        self.calls.append(("decode", cond, t_start, kw, x_latent))
        return x_latent


def test_edit_clips_invert(monkeypatch):
    monkeypatch.setattr(pipeline, "latents_to_clip", lambda vae, latents: latents)
    video = torch.zeros((1, 3, 3, 16, 16))
    text, source, empty = torch.full((1, 2, 3), 1.0), torch.full((1, 2, 3), 2.0), torch.full((1, 2, 3), 3.0)
    with pytest.raises(ValueError, match="keep_mask"):
        pipeline.edit_clips(None, None, None, None, video, text, empty, cond_frames=1, seed=None, invert=True, strength=0.5,
                            keep_mask=torch.ones((1, 1, 2, 2, 2)))
    with pytest.raises(ValueError, match="strength"):
        pipeline.edit_clips(None, None, None, None, video, text, empty, cond_frames=1, seed=None, invert=True)
    smp = _EditSampler()
    out = pipeline.edit_clips("unet", _Fst(), _Vae(), smp, video, text, empty, cond_frames=1, ddim_steps=10, scale=7.5, strength=0.5,
                              seed=None, invert=True, source_emb=source, source_scale=3.0)
    (enc, c_enc, t_enc, kw_enc), (dec, c_dec, t_start, kw_dec, x_latent) = smp.calls
    assert (enc, dec) == ("encode", "decode") and t_enc == t_start == pipeline.edit_t_enc(0.5, 10) == 5
    assert bool((c_enc == 2.0).all()) and kw_enc["unconditional_guidance_scale"] == 3.0
    assert bool((kw_enc["unconditional_conditioning"] == 3.0).all()) and kw_enc["unconditional_conditioning"].shape == c_enc.shape
    assert bool((c_dec == 1.0).all()) and kw_dec["unconditional_guidance_scale"] == 7.5
    assert bool((kw_dec["unconditional_conditioning"] == 3.0).all())
    assert "seed" not in kw_dec and "seed" not in kw_enc                       # nothing is drawn on this path
    lat = torch.ones((1, 4, 1, 2, 2)) * 0.18215                                # frames_to_latents of the posterior draw (ones)
    assert x_latent.shape == (1, 4, 2, 2, 2) and bool((x_latent == lat[0, 0, 0, 0, 0] + 1.0).all())     # ... through encode
    assert torch.equal(out, x_latent)
    assert torch.equal(kw_enc["x0_emb"], lat) and kw_dec["x0_emb"] is kw_enc["x0_emb"]
    # the defaults: the source prompt is the target's, at scale 1 with no unconditional branch
    smp = _EditSampler()
    pipeline.edit_clips("unet", _Fst(), _Vae(), smp, video, text, empty, cond_frames=1, ddim_steps=10, scale=1.0, strength=1.0,
                        seed=None, invert=True)
    (_, c_enc, t_enc, kw_enc), (_, c_dec, _, kw_dec, _) = smp.calls
    assert t_enc == 9 and c_enc is c_dec and kw_enc["unconditional_conditioning"] is None and kw_enc["unconditional_guidance_scale"] == 1.0
    assert kw_dec["unconditional_conditioning"] is None


# ---- 6. the entry points' refusals ------------------------------------------------------------------------------------------------
def refusal_cases(P, W):
    """(entry point, arguments without the stream, what is wrong) for every refusal of the entry point's two forms.  P stands for every fp32
    buffer and W for the two int32 ones; both are 4-byte aligned and non-NULL (tests/test_gpu_invert.py passes real ones)"""
    good = dict(eps=P, cfg=1, b=2, C=4, F_total=5, cond_f=2, HW=50, scale=7.5, coef=P, index=0, step=None, limit=None, x=P, x_next=P,
                pred_x0=P)
    for kw in (dict(eps=None), dict(coef=None), dict(x=None), dict(x_next=None), dict(b=0), dict(b=-1), dict(C=0), dict(HW=0), dict(HW=-4),
               dict(cond_f=-1), dict(cond_f=5), dict(cond_f=6), dict(F_total=0, cond_f=0), dict(index=-1), dict(eps=P + 2),
               dict(coef=P + 1), dict(x=P + 2), dict(x_next=P + 3), dict(pred_x0=P + 2),
               dict(b=1 << 16, C=1 << 16, F_total=1 << 8, cond_f=0, HW=1),                   # 2^40 elements: a grid beyond one dimension
               dict(step=W), dict(limit=W)):                                                 # a half-set device form
        yield "seer_cfg_ddim_invert_step", tuple({**good, **kw}.values()), kw
    good = dict(eps=P, cfg=1, b=2, C=4, F_total=5, cond_f=2, HW=50, scale=7.5, coef=P, index=-1, step=W, limit=W, x=P, x_next=P,
                pred_x0=P)
    for kw in (dict(eps=None), dict(coef=None), dict(step=None), dict(limit=None), dict(x=None), dict(x_next=None), dict(b=0), dict(C=0),
               dict(HW=0), dict(cond_f=-1), dict(cond_f=5), dict(eps=P + 2), dict(coef=P + 2), dict(step=W + 2), dict(limit=W + 1),
               dict(x=P + 2), dict(x_next=P + 2), dict(pred_x0=P + 1), dict(index=0)):
        yield "seer_cfg_ddim_invert_step", tuple({**good, **kw}.values()), kw


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
    assert n >= 30
