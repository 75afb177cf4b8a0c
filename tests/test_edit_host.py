"""Masked sampling, stochastic_encode and decode without a GPU.  DDIMSampler("cpu", ops=tests.edit_ref) against the vendored CompVis
sampler (ldm/models/diffusion/ddim.py: the mask loop :144-147, stochastic_encode :207-221, decode :223-241) over the analytic Gaussian
model of tests/test_slots_host.py with the frames folded into the height; SlotSampler(editing=True, ops=tests.edit_ref) against a solo
float64 loop per request; every refusal; the exports.

Measured here (fp32 on both sides, rel-L2 of ours to CompVis; profiles/edit_sampler.md): stochastic_encode and decode 0 (the same
bits); sample with a binary mask 6.67e-7 (eta 0) and 6.65e-7 (eta 0.5), with a soft mask 6.17e-7 and 6.14e-7.  All of the masked
figure is the table q is made from: CompVis's loop calls the MODEL's q_sample, whose sqrt(1 - alphas_cumprod) is made in float64
(ddpm.py:117-118), the kernels use the DDIM tables' sqrt(1 - a_t) made in fp32 from the fp32 a_t, as stochastic_encode does -- at
the schedule's last index, a_t = 0.9999, that is 3e-4 of a coefficient of 0.01.  Four times the measured value would be 2.7e-6; the
bound is the 1e-6 the other host tests allow fp32 against float64, which is the tighter of the two."""
import inspect

import numpy as np
import pytest
import torch

from oracle import ref_import
from oracle import seer_oracle as O
from tests import edit_ref, stoch_ref
from tests.test_slots_host import C, F1, FP, H, W, _Gaussian, _rel

f64 = torch.float64
PER_CLIP = C * FP * H * W
REF_BOUND = 1e-6


# ---- 1. against the vendored CompVis sampler -----------------------------------------------------------------------------------------
class _Model(_Gaussian):
    """the Gaussian eps on a latent without conditioning frames ([rows, C, FP, H, W]); as a CompVis model it takes the same latent
    with the frames folded into the height ([rows, C, FP * H, W])"""

    def __init__(self):
        super().__init__(2)
        from seervideoldm_amd.ddim import _betas
        betas = _betas(1000, 1e-4, 2e-2)
        ac = np.cumprod(1.0 - betas, axis=0)
        self.num_timesteps = 1000
        self.betas = torch.tensor(betas, dtype=torch.float32)
        self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
        self.alphas_cumprod_prev = torch.tensor(np.append(1.0, ac[:-1]), dtype=torch.float32)
        self.sqrt_alphas_cumprod = torch.tensor(np.sqrt(ac), dtype=torch.float32)                       # ddpm.py:117-118
        self.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1.0 - ac), dtype=torch.float32)
        self.device = torch.device("cpu")

    def _eps(self, sample, t, context):
        out = []
        for r in range(sample.shape[0]):
            k, prompt = int(context[r, 0, 0, 0]), bool(context[r, 0, 0, 1])
            out.append(self.exact(sample[r].double(), t[r], (self.mu_c if prompt else self.mu_u)[k][:, F1:]))
        return torch.stack(out).float()

    def __call__(self, sample, t, context, cond_frame=0):
        self.calls += 1
        return self._eps(sample, t, context)

    def apply_model(self, x, t, c):
        return self._eps(x.reshape(x.shape[0], C, FP, H, W), t, c).reshape(x.shape)

    def q_sample(self, x_start, t, noise=None):                                                          # ddpm.py:272-275
        noise = torch.randn_like(x_start) if noise is None else noise
        return (self.sqrt_alphas_cumprod[t].reshape(-1, 1, 1, 1) * x_start
                + self.sqrt_one_minus_alphas_cumprod[t].reshape(-1, 1, 1, 1) * noise)


def _compvis(model):
    if not ref_import.available():
        pytest.skip("the reference tree is not present")
    ref_import.load_reference()                          # the stubs and the import path of the reference
    import importlib
    mod = importlib.import_module("ldm.models.diffusion.ddim")
    mod.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    return mod.DDIMSampler(model)


def _case_inputs(model):
    g = torch.Generator().manual_seed(21)
    b = 2
    x_T = torch.randn((b, C, FP, H, W), generator=g)
    x0 = 0.8 * torch.randn((b, C, FP, H, W), generator=g)
    binary = (torch.rand((b, 1, FP, H, W), generator=g) < 0.5).float()
    binary[1, :, 0] = 1.0                                # a whole frame kept
    soft = torch.rand((b, 1, FP, H, W), generator=g)
    soft[0, :, 1] = 0.0
    soft[1, :, 2] = 1.0
    c = torch.stack([model.context(k, True)[F1:] for k in range(b)])
    uc = torch.stack([model.context(k, False)[F1:] for k in range(b)])
    return dict(b=b, x_T=x_T, x0=x0, binary=binary, soft=soft, c=c, uc=uc)


def _fold(t):
    return t.reshape(t.shape[0], t.shape[1], FP * H, W)


def _ours(model):
    from seervideoldm_amd import DDIMSampler
    return DDIMSampler("cpu", ops=edit_ref)


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["binary", "soft"])
def test_masked_sample_against_compvis(kind, eta):
    model = _Model()
    ref = _compvis(model)
    i = _case_inputs(model)
    torch.manual_seed(7)
    want, _ = ref.sample(4, i["b"], (C, FP * H, W), conditioning=i["c"], eta=eta, mask=_fold(i[kind]), x0=_fold(i["x0"]), verbose=False,
                         x_T=_fold(i["x_T"]), unconditional_guidance_scale=3.0, unconditional_conditioning=i["uc"])
    torch.manual_seed(7)
    x_T = i["x_T"].clone()
    got, _ = _ours(model).sample(model, 4, i["b"], (C, FP, H, W), conditioning=i["c"], eta=eta, mask=i[kind], x0=i["x0"], verbose=False,
                                 x_T=x_T, unconditional_guidance_scale=3.0, unconditional_conditioning=i["uc"], is_3d=True)
    assert torch.equal(x_T, i["x_T"])                    # the blend works on a copy of the caller's start code
    rel = _rel(_fold(got), want)
    print(f"[edit] masked sample, {kind} mask, eta {eta}: rel_l2 to CompVis {rel:.3g}")
    assert got.shape == (i["b"], C, FP, H, W) and torch.isfinite(got).all() and rel <= REF_BOUND, rel
    # the mask is in the result: without it the same call gives another latent
    torch.manual_seed(7)
    plain, _ = _ours(model).sample(model, 4, i["b"], (C, FP, H, W), conditioning=i["c"], eta=eta, verbose=False, x_T=i["x_T"],
                                   unconditional_guidance_scale=3.0, unconditional_conditioning=i["uc"], is_3d=True)
    assert _rel(plain, got) > 1e-3


def test_stochastic_encode_and_decode_against_compvis():
    model = _Model()
    ref = _compvis(model)
    i = _case_inputs(model)
    ours = _ours(model)
    ref.make_schedule(6, ddim_eta=0.5, verbose=False)
    ours.make_schedule(6, ddim_eta=0.5, verbose=False)
    n = ours.ddim_coef.shape[0]
    assert n == 7
    noise = torch.randn((i["b"], C, FP, H, W), generator=torch.Generator().manual_seed(5))
    t = torch.tensor([5, 2])
    want = ref.stochastic_encode(_fold(i["x0"]), t, noise=_fold(noise))
    got = ours.stochastic_encode(i["x0"], t, noise=noise)
    rel = _rel(_fold(got), want)
    print(f"[edit] stochastic_encode: rel_l2 to CompVis {rel:.3g}")
    assert rel <= REF_BOUND, rel
    torch.manual_seed(9)                                 # with neither noise nor seed: torch.randn_like, as CompVis
    want = ref.stochastic_encode(_fold(i["x0"]), torch.tensor([4, 4]))
    torch.manual_seed(9)
    assert _rel(_fold(ours.stochastic_encode(i["x0"], 4)), want) <= REF_BOUND
    # with a seed: stream 2 of the row's seed at index t
    got = ours.stochastic_encode(i["x0"], t, seed=[11, 12])
    for bi, (seed, idx) in enumerate(zip((11, 12), (5, 2))):
        nz = torch.from_numpy(stoch_ref.normals64(seed, 2, idx, PER_CLIP)).reshape(C, FP, H, W)
        a = float(ours.ddim_coef[idx, 0])
        assert _rel(got[bi], a ** 0.5 * i["x0"][bi].double() + float(ours.ddim_coef[idx, 3]) * nz) <= 1e-6
    assert torch.equal(ours.stochastic_encode(i["x0"], 3, seed=11)[1], ours.stochastic_encode(i["x0"][1:], 3, seed=12)[0])
    torch.manual_seed(3)
    want = ref.decode(_fold(i["x_T"]), i["c"], 4, unconditional_guidance_scale=3.0, unconditional_conditioning=i["uc"])
    torch.manual_seed(3)
    got = ours.decode(model, i["x_T"], i["c"], 4, unconditional_guidance_scale=3.0, unconditional_conditioning=i["uc"])
    rel = _rel(_fold(got), want)
    print(f"[edit] decode(t_start = 4 of {n}, eta 0.5): rel_l2 to CompVis {rel:.3g}")
    assert rel <= REF_BOUND, rel


# ---- 2. SlotSampler(editing=True) over the stand-in ----------------------------------------------------------------------------------
def _requests(model):
    g = torch.Generator().manual_seed(13)
    reqs = []
    for k, (S, scale, eta, seed, masked, t_start) in enumerate(((4, 7.5, 0.0, 1234, True, None), (6, 3.0, 0.0, None, False, 3),
                                                                (5, 7.5, 0.0, None, False, None), (4, 3.0, 0.5, (7 << 32) | 5, True, None))):
        x_T = torch.randn((1, C, FP, H, W), generator=g)
        r = dict(x_T=x_T, x0_emb=0.9 * torch.randn((1, C, F1, H, W), generator=g), c=model.context(k, True), uc=model.context(k, False),
                 S=S, scale=scale, tag=f"r{k}")
        if eta or seed is not None:
            r.update(eta=eta, seed=seed)
        if masked:
            mask = (torch.rand((1, 1, FP, H, W), generator=g) < 0.5).float()
            mask[0, 0, k % FP] = 0.3                     # one soft frame
            r.update(mask=mask, x0=0.8 * torch.randn((1, C, FP, H, W), generator=g))
        if t_start is not None:
            r.update(t_start=t_start)
        reqs.append(r)
    return reqs


def _solo64(model, k, r):
    """the request alone in float64: DDIMSampler.ddim_sampling's loop over the oracle's p_sample_ddim, the mask blend in front of
    every step with the restatement's normals of (seed, stream 2, index), the step noise those of stream 1"""
    eta = r.get("eta", 0.0)
    sched = O.make_schedule(r["S"], eta)
    ts = sched["ddim_timesteps"]

    def unet_fn(x, t, ctx, cond_frames):
        return torch.stack([model.exact(x[0], t[0], model.mu_u[k]), model.exact(x[1], t[1], model.mu_c[k])])
    x = r["x_T"].double()
    first = r.get("t_start", len(ts))
    for index in reversed(range(first)):
        if "mask" in r:
            nz = torch.from_numpy(stoch_ref.normals64(r["seed"], 2, index, PER_CLIP)).reshape(x.shape)
            q = float(np.float32(sched["alphas"][index])) ** 0.5 * r["x0"].double() + float(np.float32(sched["sqrt_one_minus_alphas"][index])) * nz
            m = r["mask"].double()
            x = q * m + (1.0 - m) * x
        noise = torch.zeros_like(x)
        if eta:
            noise = torch.from_numpy(stoch_ref.normals64(r["seed"], 1, index, PER_CLIP)).reshape(x.shape)
        t = torch.full((1,), int(ts[index]), dtype=torch.long)
        x, _ = O.p_sample_ddim(unet_fn, x, model.context(k, True)[None], t, index, sched, x0_emb=r["x0_emb"].double(),
                               scale=r["scale"], uc=model.context(k, False)[None], noise=noise)
        assert x.dtype == f64
    return x, first


def _sampler(model, slots=2, editing=True, stochastic=True, **kw):
    from seervideoldm_amd import SlotSampler
    return SlotSampler(model, slots, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=edit_ref,
                       stochastic=stochastic, **(dict(editing=True) if editing else {}), **kw)


def test_staggered_edit_requests_equal_their_solo_runs():
    model = _Gaussian(4)
    reqs = _requests(model)
    want = [_solo64(model, k, r) for k, r in enumerate(reqs)]
    assert [n for _, n in want] == [4, 3, 5, 4]
    smp = _sampler(model)
    got = dict(smp.run(iter(reqs)))
    assert sorted(got) == ["r0", "r1", "r2", "r3"] and smp.free_slots() == [0, 1]
    assert not smp._mask.any() and not smp._known.any()          # a retired slot's mask is zeroed
    for (ref, n), r in zip(want, reqs):
        lat = got[r["tag"]]
        rel = _rel(lat, ref)
        print(f"[edit] request {r['tag']} ({n} steps, mask {'mask' in r}, eta {r.get('eta', 0.0)}): rel_l2 to its solo float64 loop "
              f"{rel:.3g}")
        assert lat.shape == (1, C, FP, H, W) and torch.isfinite(lat).all() and rel <= 1e-6, (r["tag"], rel)
    # the slot is held for t_start steps: r0 and r1 go in, r1 leaves after 3 steps, r0 after 4
    smp = _sampler(model)
    sub = lambda r: smp.submit(**{k: v for k, v in r.items() if k != "tag"})
    assert (sub(reqs[0]), sub(reqs[1])) == (0, 1) and smp._step[:, 0].tolist() == [3, 2]
    done = [[s for s, _ in smp.step()] for _ in range(4)]
    assert done == [[], [], [1], [0]]
    # the mask is in the result
    other = dict(_sampler(model).run(iter([{k: v for k, v in reqs[0].items() if k not in ("mask", "x0")}])))
    assert _rel(other["r0"], got["r0"]) > 1e-3


def test_a_masked_clip_does_not_depend_on_its_neighbours_or_the_slot_count():
    model = _Gaussian(4)
    reqs = _requests(model)
    pair = dict(_sampler(model).run(iter(reqs[:2])))
    other = dict(_sampler(model, slots=3).run(iter([reqs[2], reqs[0], reqs[3]])))
    alone = dict(_sampler(model, slots=1).run(iter([reqs[0]])))
    late = dict(_sampler(model, slots=2).run(iter([reqs[1], reqs[3], reqs[0]])))         # admitted when r1 leaves, into slot 0
    for run in (other, alone, late):
        assert torch.equal(run["r0"], pair["r0"])
    assert torch.equal(late["r3"], other["r3"]) and torch.equal(late["r1"], pair["r1"])


def test_a_plain_clip_in_an_editing_queue_has_the_bits_of_a_plain_queue():
    model = _Gaussian(4)
    reqs = _requests(model)
    for stochastic in (False, True):
        edit = dict(_sampler(model, stochastic=stochastic).run(iter([reqs[0], reqs[2]])))
        plain = dict(_sampler(model, editing=False, stochastic=stochastic).run(iter([reqs[2]])))
        assert torch.equal(edit["r2"], plain["r2"]), stochastic
    assert not hasattr(_sampler(model, editing=False), "_mask")


class _Recording:
    """the stand-in backend with every kernel call written down by name"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(edit_ref, name)

        def call(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return call


def test_without_a_mask_the_launches_are_what_they_were():
    from seervideoldm_amd import DDIMSampler, SlotSampler
    gm = _Gaussian(4)
    plain = {k: v for k, v in _requests(gm)[2].items() if k != "tag"}
    for kw in (dict(), dict(stochastic=True)):
        rec = _Recording()
        smp = SlotSampler(gm, 2, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=rec, **kw)
        smp.submit(**plain)
        while smp.active():
            smp.step()
        assert rec.calls == ["slot_step_begin", "slot_cfg_ddim_step_rng" if kw else "slot_cfg_ddim_step"] * 5
        rec = _Recording()                               # editing=True puts exactly one launch in front of each step
        smp = SlotSampler(gm, 2, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=rec, editing=True, **kw)
        smp.submit(**plain)
        while smp.active():
            smp.step()
        assert rec.calls == ["slot_known_blend", "slot_step_begin", "slot_cfg_ddim_step_rng" if kw else "slot_cfg_ddim_step"] * 5
    model = _Model()
    i = _case_inputs(model)
    kw = dict(conditioning=i["c"], verbose=False, x_T=i["x_T"], unconditional_guidance_scale=3.0, unconditional_conditioning=i["uc"], is_3d=True)
    rec = _Recording()
    DDIMSampler("cpu", ops=rec).sample(model, 4, i["b"], (C, FP, H, W), eta=0.5, **kw)
    assert rec.calls == ["cfg_ddim_step"] * 4
    rec = _Recording()
    DDIMSampler("cpu", ops=rec).sample(model, 4, i["b"], (C, FP, H, W), eta=0.5, seed=3, **kw)
    assert rec.calls == ["cfg_ddim_step_rng"] * 4
    rec = _Recording()
    DDIMSampler("cpu", ops=rec).sample(model, 4, i["b"], (C, FP, H, W), eta=0.5, seed=3, mask=i["soft"], x0=i["x0"], **kw)
    assert rec.calls == ["known_blend", "cfg_ddim_step_rng"] * 4


# ---- 3. refusals, exports, arithmetic -------------------------------------------------------------------------------------------------
def test_refusals():
    from seervideoldm_amd import DDIMSampler, SlotSampler, edit_clips
    model = _Model()
    i = _case_inputs(model)
    d = DDIMSampler("cpu", ops=edit_ref)
    kw = dict(conditioning=i["c"], verbose=False, x_T=i["x_T"], is_3d=True)
    with pytest.raises(ValueError, match="x0"):
        d.sample(model, 4, i["b"], (C, FP, H, W), mask=i["binary"], **kw)                  # mask without x0
    with pytest.raises(ValueError, match="mask"):
        d.sample(model, 4, i["b"], (C, FP, H, W), x0=i["x0"], **kw)                        # x0 without mask
    with pytest.raises(ValueError, match="channel"):
        d.sample(model, 4, i["b"], (C, FP, H, W), mask=i["binary"].expand(-1, C, -1, -1, -1), x0=i["x0"], **kw)
    with pytest.raises(ValueError, match="broadcast"):
        d.sample(model, 4, i["b"], (C, FP, H, W), mask=torch.ones((i["b"], 1, FP + 1, H, W)), x0=i["x0"], **kw)
    with pytest.raises(ValueError, match="x0"):
        d.sample(model, 4, i["b"], (C, FP, H, W), mask=i["binary"], x0=i["x0"][:, :, :1], **kw)
    model._shard = object()
    with pytest.raises(ValueError, match="shard"):
        d.sample(model, 4, i["b"], (C, FP, H, W), mask=i["binary"], x0=i["x0"], **kw)
    model._shard = None
    d.make_schedule(4, verbose=False)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="t_start"):
            d.decode(model, i["x_T"], i["c"], bad)
    for bad in (4, -1, torch.tensor([0, 4]), torch.tensor([1, 2, 3])):
        with pytest.raises(ValueError, match="schedule"):
            d.stochastic_encode(i["x0"], bad)
    with pytest.raises(ValueError, match="not both"):
        d.stochastic_encode(i["x0"], 1, noise=i["x_T"], seed=3)
    with pytest.raises(NotImplementedError):
        d.stochastic_encode(i["x0"], 1, use_original_steps=True)
    with pytest.raises(NotImplementedError):
        d.decode(model, i["x_T"], i["c"], 2, use_original_steps=True)
    # slots
    gm = _Gaussian(4)
    reqs = [{k: v for k, v in r.items() if k != "tag"} for r in _requests(gm)]
    smp = _sampler(gm)
    with pytest.raises(ValueError, match="seed"):
        smp.submit(**{**reqs[0], "seed": None})                                            # mask without a seed
    with pytest.raises(ValueError, match="x0"):
        smp.submit(**{k: v for k, v in reqs[0].items() if k != "x0"})
    with pytest.raises(ValueError, match="mask"):
        smp.submit(**{**reqs[0], "mask": torch.ones((1, C, FP, H, W))})                    # a mask per channel
    for bad in (0, 8, -2):                                                                 # S = 6 has 7 entries
        with pytest.raises(ValueError, match="t_start"):
            smp.submit(**{**reqs[1], "t_start": bad})
    with pytest.raises(ValueError, match="x_T"):
        smp.submit(**{**reqs[1], "x_T": None, "seed": 3})                                  # t_start takes x_T as the latent of that level
    assert smp.free_slots() == [0, 1]                    # a refused request takes no slot
    with pytest.raises(ValueError, match="plms"):
        SlotSampler(gm, 2, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=edit_ref, plms=True, editing=True)
    plain = _sampler(gm, editing=False)
    for extra in (dict(mask=reqs[0]["mask"], x0=reqs[0]["x0"], seed=3), dict(t_start=2), dict(x0=reqs[0]["x0"])):
        with pytest.raises(ValueError, match="editing"):
            plain.submit(**{**reqs[2], **extra})
    # an editing queue without stochastic=True takes a seed with a mask only
    det = _sampler(gm, stochastic=False)
    with pytest.raises(ValueError, match="stochastic"):
        det.submit(**reqs[2], seed=3)
    assert det.submit(**reqs[0]) == 0
    # edit_clips: exactly one of strength and keep_mask (checked before any model runs)
    v = torch.zeros((1, 3, 3, 16, 16))
    for extra in (dict(strength=0.5, keep_mask=torch.ones((1, 1, 2, 2, 2))), dict()):
        with pytest.raises(ValueError, match="exactly one"):
            edit_clips(None, None, None, d, v, None, None, cond_frames=1, seed=1, **extra)


def test_generate_queue_refuses_edit_requests_without_editing():
    from seervideoldm_amd.pipeline import generate_queue

    class _Dist:
        def sample(self, generator=None):
            return torch.zeros((1, 4, 2, 2))

    class _Vae:
        def encode(self, frames):
            return type("E", (), {"latent_dist": _Dist()})()

    class _Fst:
        def set_numframe(self, n):
            pass

        def __call__(self, context):
            return torch.zeros((1, 3, 1, 2))
    r = dict(x0_image=torch.zeros((1, 3, 1, 16, 16)), text_emb=torch.zeros((1, 1, 2)), empty_emb=torch.zeros((1, 1, 2)), ddim_steps=4,
             scale=7.5, tag="a", noise=torch.zeros((1, 4, 2, 2, 2)))
    for extra in (dict(t_start=2), dict(mask=torch.ones((1, 1, 2, 2, 2)), known=torch.zeros((1, 4, 2, 2, 2)), seed=3)):
        with pytest.raises(ValueError, match="editing"):
            list(generate_queue(_Gaussian(1), _Fst(), _Vae(), [dict(r, **extra)], slots=1, num_frames=3, cond_frames=1))


def test_edit_t_enc():
    from seervideoldm_amd.pipeline import edit_t_enc
    # S = 30 makes 31 entries, S = 4 makes 4
    assert [edit_t_enc(s, 31) for s in (0.01, 0.5, 1.0)] == [1, 15, 30]
    assert [edit_t_enc(s, 4) for s in (0.01, 0.5, 1.0)] == [1, 2, 3]
    assert edit_t_enc(0.99, 2) == 1
    for bad in (0.0, -0.1, 1.01):
        with pytest.raises(ValueError, match="strength"):
            edit_t_enc(bad, 31)
    with pytest.raises(ValueError, match="entries"):
        edit_t_enc(0.5, 1)


def test_exports():
    import seervideoldm_amd
    from seervideoldm_amd import DDIMSampler, SlotSampler, _lib, ops, pipeline
    new = {"seer_q_sample", "seer_known_blend", "seer_slot_known_blend"}
    assert new <= set(_lib.SIGNATURES)
    assert ops.PHILOX_STREAM_KNOWN == 2 == edit_ref.STREAM_KNOWN
    for name in ("q_sample", "known_blend", "slot_known_blend"):
        assert callable(getattr(ops, name)) and callable(getattr(edit_ref, name)), name
    for name in ("slot_step_begin", "slot_cfg_ddim_step", "slot_cfg_ddim_step_rng", "cfg_ddim_step", "cfg_ddim_step_rng", "philox_normal"):
        assert callable(getattr(edit_ref, name)), name
    assert seervideoldm_amd.edit_clips is pipeline.edit_clips and "edit_clips" in seervideoldm_amd.__all__
    assert inspect.signature(SlotSampler.__init__).parameters["editing"].default is False
    assert inspect.signature(pipeline.generate_queue).parameters["editing"].default is False
    assert {"mask", "x0", "t_start"} <= set(inspect.signature(SlotSampler.submit).parameters)
    assert {"mask", "x0"} <= set(inspect.signature(DDIMSampler.ddim_sampling).parameters)
    dec = inspect.signature(DDIMSampler.decode).parameters
    assert list(dec)[1:5] == ["unet", "x_latent", "cond", "t_start"] and dec["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    enc = inspect.signature(DDIMSampler.stochastic_encode).parameters
    assert list(enc)[1:] == ["x0", "t", "use_original_steps", "noise", "seed"]
    ec = inspect.signature(pipeline.edit_clips).parameters
    assert ec["strength"].default is None and ec["keep_mask"].default is None and ec["seed"].default is inspect.Parameter.empty


def refusal_cases(P):
    """(entry point, arguments without the stream, what is wrong) for every refusal of the three entry points; P is a 4-byte aligned
    non-NULL pointer that stands for every buffer (tests/test_gpu_edit.py passes a real one)"""
    good = dict(x0=P, b=2, per_row=96, coef=P, nsched=8, index=P, noise=P, seeds=None, out=P)
    for kw in (dict(x0=None), dict(coef=None), dict(index=None), dict(out=None), dict(seeds=P), dict(noise=None), dict(b=0), dict(b=-1),
               dict(per_row=0), dict(per_row=1 << 31), dict(nsched=0), dict(x0=P + 2), dict(index=P + 1), dict(noise=P + 2),
               dict(noise=None, seeds=P + 2), dict(out=P + 3)):
        yield "seer_q_sample", tuple({**good, **kw}.values()), kw
    good = dict(x=P, mask=P, known=P, b=2, C=4, F_pred=3, HW=64, coef=P, index=0, step=None, noise=None, seeds=P)
    for kw in (dict(x=None), dict(mask=None), dict(known=None), dict(coef=None), dict(noise=P), dict(seeds=None), dict(b=0), dict(C=0),
               dict(F_pred=0), dict(HW=0), dict(HW=-4), dict(C=1 << 15, F_pred=1, HW=1 << 16), dict(C=1 << 14, F_pred=8, HW=1 << 14),
               dict(x=P + 2), dict(mask=P + 1), dict(known=P + 2), dict(step=P + 2), dict(seeds=P + 1), dict(seeds=None, noise=P + 2)):
        yield "seer_known_blend", tuple({**good, **kw}.values()), kw
    good = dict(x=P, mask=P, known=P, slots=2, C=4, F_pred=3, HW=64, coef=P, nsched=8, step=P, seeds=P)
    for kw in (dict(x=None), dict(mask=None), dict(known=None), dict(coef=None), dict(step=None), dict(seeds=None), dict(slots=0),
               dict(nsched=0), dict(C=0), dict(F_pred=0), dict(HW=0), dict(C=1 << 15, F_pred=1, HW=1 << 16), dict(x=P + 2),
               dict(mask=P + 1), dict(known=P + 3), dict(coef=P + 2), dict(step=P + 2), dict(seeds=P + 2)):
        yield "seer_slot_known_blend", tuple({**good, **kw}.values()), kw


def test_kernel_entry_points_refuse_bad_arguments_before_any_launch():
    """every refusal returns SEER_EINVAL on the host (16 = an aligned non-NULL pointer; no call here would pass its checks, so
    nothing is launched)"""
    from seervideoldm_amd import _lib
    from seervideoldm_amd.build import build_library
    build_library()
    lib = _lib.load()
    n = 0
    for fn, args, why in refusal_cases(16):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    assert n >= 30
