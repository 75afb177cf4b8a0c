"""SlotSampler's host logic without a GPU: SlotSampler(ops=tests.slot_ref) over a Python model -- the analytic Gaussian eps of
tests/test_gpu_plms.py::test_plms_solves_the_gaussian_probability_flow_ode, one (mu_u, mu_c) pair per request -- on CPU tensors.
Staggered requests against a float64 solo DDIM loop per request, the slot bookkeeping by hand, the refusals, the exports."""
import pytest
import torch

from seervideoldm_amd import DDIMSampler
from tests import slot_ref

C, F1, FP, H, W = 4, 1, 3, 6, 10
SIGMA_DATA = 0.5
f64 = torch.float64


def _rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


class _Gaussian:
    """eps of Gaussian data N(mu, s^2): sigma (x - alpha mu) / (alpha^2 s^2 + sigma^2), in float64.  A context row says whose mu the
    row takes: context[row, :, 0, 0] = the request's number, context[row, :, 0, 1] = 1 for the prompt row, 0 for the empty prompt."""

    def __init__(self, n_requests):
        g = torch.Generator().manual_seed(3)
        self.mu_u = [0.3 * torch.randn((C, F1 + FP, H, W), generator=g, dtype=f64) for _ in range(n_requests)]
        self.mu_c = [u + 0.1 * torch.randn(u.shape, generator=g, dtype=f64) for u in self.mu_u]
        smp = DDIMSampler("cpu")
        smp.make_schedule(4, verbose=False)
        self.ac = smp.alphas_cumprod.double()
        self.calls = 0
        self._shard = None

    def exact(self, x, t, mu):
        a2 = self.ac[int(t)]
        return (1 - a2).sqrt() * (x - a2.sqrt() * mu) / (a2 * SIGMA_DATA ** 2 + (1 - a2))

    def context(self, k, prompt):
        ctx = torch.zeros((F1 + FP, 1, 2))
        ctx[:, 0, 0], ctx[:, 0, 1] = float(k), float(prompt)
        return ctx

    def __call__(self, sample, t, context, cond_frame=0):
        self.calls += 1
        out = []
        for r in range(sample.shape[0]):
            k, prompt = int(context[r, 0, 0, 0]), bool(context[r, 0, 0, 1])
            out.append(self.exact(sample[r].double(), t[r], (self.mu_c if prompt else self.mu_u)[k]))
        return torch.stack(out).float()


def _requests(model):
    g = torch.Generator().manual_seed(11)
    reqs = []
    for k, (S, scale) in enumerate(((4, 7.5), (6, 3.0), (5, 7.5))):
        reqs.append(dict(x_T=torch.randn((1, C, FP, H, W), generator=g), x0_emb=0.9 * torch.randn((1, C, F1, H, W), generator=g),
                         c=model.context(k, True), uc=model.context(k, False), S=S, scale=scale, tag=f"r{k}"))
    return reqs


def _solo64(model, k, r):
    """the request alone: the DDIM loop of DDIMSampler.ddim_sampling over DDIMSampler("cpu")'s own tables, in float64"""
    smp = DDIMSampler("cpu")
    smp.make_schedule(r["S"], verbose=False)
    coef, ttab = smp.ddim_coef.double(), smp._t_table
    x, x0_emb = r["x_T"][0].double(), r["x0_emb"][0].double()
    for index in reversed(range(coef.shape[0])):
        x_cat = torch.cat([x0_emb, x], dim=1)
        eu, ec = model.exact(x_cat, ttab[index], model.mu_u[k]), model.exact(x_cat, ttab[index], model.mu_c[k])
        e = (eu + r["scale"] * (ec - eu))[:, F1:]
        a_t, a_prev, sigma, s1m = coef[index].tolist()
        pred = (x - s1m * e) / a_t ** 0.5
        x = a_prev ** 0.5 * pred + (1 - a_prev - sigma ** 2) ** 0.5 * e
    return x[None], coef.shape[0]


def _sampler(model, slots=2, **kw):
    from seervideoldm_amd import SlotSampler
    return SlotSampler(model, slots, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=slot_ref, **kw)


def test_staggered_requests_equal_their_solo_runs():
    model = _Gaussian(3)
    reqs = _requests(model)
    want = [_solo64(model, k, r) for k, r in enumerate(reqs)]
    assert [n for _, n in want] == [4, 7, 5]             # S = 6 has stride 166 and therefore 7 entries
    smp = _sampler(model)
    sub = lambda r: smp.submit(**{k: v for k, v in r.items() if k != "tag"})
    assert smp.step() == [] and model.calls == 0         # every slot idle: nothing runs
    assert (sub(reqs[0]), sub(reqs[1])) == (0, 1) and smp.free_slots() == [] and smp.active() == [0, 1]
    # by hand: r0 (4 entries) leaves slot 0 with step 4, r2 (5 entries) takes it and leaves with step 9; r1 (7 entries) leaves slot 1
    # with step 7
    free_after = {1: [], 2: [], 3: [], 4: [0], 5: [], 6: [], 7: [1], 8: [1], 9: [0, 1]}
    finished = []
    for n in range(1, 10):
        done = smp.step()
        assert smp.free_slots() == free_after[n], n
        finished += [(n, s) for s, _ in done]
        for s, lat in done:
            k = {(4, 0): 0, (7, 1): 1, (9, 0): 2}[(n, s)]
            assert lat.shape == (1, C, FP, H, W) and torch.isfinite(lat).all()
            rel = _rel(lat, want[k][0])
            print(f"[slots] request {k} (S = {reqs[k]['S']}, scale {reqs[k]['scale']}) left slot {s} with step {n}: rel_l2 to its solo "
                  f"float64 loop {rel:.3g}")
            assert rel <= 1e-6, (k, rel)
            assert not smp._x[s].any() and not smp._x0[s].any()          # a retired slot's latents are zeroed
        if n == 4:
            assert sub(reqs[2]) == 0 and smp.free_slots() == []
    assert finished == [(4, 0), (7, 1), (9, 0)] and model.calls == 9
    assert smp._step[:, 0].tolist() == [-1, -1]          # the counters ran down on their own
    assert smp.step() == [] and model.calls == 9
    # run() drives the same sequence: the same latents, in finishing order
    model2 = _Gaussian(3)
    smp2 = _sampler(model2)
    got = list(smp2.run(iter(reqs)))
    assert [tag for tag, _ in got] == ["r0", "r1", "r2"] and model2.calls == 9 and smp2.free_slots() == [0, 1]
    for (tag, lat), (ref, _) in zip(got, want):
        assert _rel(lat, ref) <= 1e-6, tag


def test_a_slot_does_not_depend_on_its_neighbours():
    """the host logic moves nothing between slots: r1 behind r0 in two slots, and behind r2 in three with one idle, are the same bits"""
    model = _Gaussian(3)
    reqs = _requests(model)
    pair = dict(_sampler(model).run(iter(reqs[:2])))
    other = dict(_sampler(model, slots=3).run(iter([reqs[2], reqs[1]])))
    assert torch.equal(other["r1"], pair["r1"])


def test_refusals():
    model = _Gaussian(3)
    reqs = [{k: v for k, v in r.items() if k != "tag"} for r in _requests(model)]
    smp = _sampler(model, max_steps=6)
    with pytest.raises(ValueError, match="max_steps"):
        smp.submit(**reqs[1])                            # S = 6 makes 7 entries
    with pytest.raises(ValueError, match="eta"):
        smp.submit(**reqs[0], eta=0.5)
    for key, bad in (("x_T", torch.zeros((1, C, FP + 1, H, W))), ("x0_emb", torch.zeros((1, C, F1, H, W + 1))),
                     ("c", torch.zeros((F1 + FP, 2, 2))), ("uc", torch.zeros((FP, 1, 2))), ("x0_emb", None)):
        with pytest.raises(ValueError, match=key):
            smp.submit(**{**reqs[0], key: bad})
    assert smp.free_slots() == [0, 1]                    # a refused request takes no slot
    model._shard = object()
    with pytest.raises(ValueError, match="shard"):
        smp.submit(**reqs[0])
    model._shard = None
    smp.submit(**reqs[0]), smp.submit(**reqs[2])
    with pytest.raises(RuntimeError, match="busy"):
        smp.submit(**reqs[0])
    from seervideoldm_amd import SlotSampler
    with pytest.raises(ValueError, match="slots"):
        SlotSampler(model, 5, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=slot_ref)


def test_exports():
    import seervideoldm_amd
    from seervideoldm_amd import SlotSampler, _lib, ops, pipeline
    assert "SlotSampler" in seervideoldm_amd.__all__ and SlotSampler is seervideoldm_amd.slots.SlotSampler
    assert {"seer_slot_step_begin", "seer_slot_cfg_ddim_step"} <= set(_lib.SIGNATURES)
    assert callable(ops.slot_step_begin) and callable(ops.slot_cfg_ddim_step) and callable(pipeline.generate_queue)


def refusal_cases(P):
    """(entry point, arguments without the stream, what is wrong) for every refusal of the two slot entry points in their plain modes
    (no sampler per slot, no seeds); P is a 4-byte aligned non-NULL pointer with at least 128 bytes behind it that stands for every
    buffer (tests/test_gpu_slots.py passes a real one)"""
    good = dict(x0_emb=P, x=P, x_prov=None, slots=2, reps=2, C=4, f1=1, F_pred=3, HW=64, t_table=P, nsched=8, step=P, state=None,
                sample=P, t_out=P)
    for kw in (dict(x=None), dict(t_table=None), dict(step=None), dict(sample=None), dict(t_out=None), dict(x0_emb=None),
               dict(slots=0), dict(nsched=0), dict(reps=0), dict(reps=3), dict(C=0), dict(F_pred=0), dict(HW=0), dict(f1=-1),
               dict(x=P + 2), dict(t_table=P + 1), dict(t_out=P + 3), dict(step=P + 2), dict(sample=P + 1), dict(x0_emb=P + 2),
               dict(x_prov=P + 64), dict(state=P)):                                          # one of the pair without the other
        yield "seer_slot_step_begin", tuple({**good, **kw}.values()), kw
    good = dict(eps=P, slots=2, C=4, F_total=4, cond_f=1, HW=64, scale=P, coef=P, nsched=8, step=P, x=P, seeds=None, temperature=None,
                x_prev=P, pred_x0=P)
    for kw in (dict(eps=None), dict(scale=None), dict(coef=None), dict(step=None), dict(x=None), dict(x_prev=None), dict(slots=0),
               dict(nsched=0), dict(cond_f=4), dict(cond_f=5), dict(cond_f=-1), dict(C=0), dict(HW=0), dict(eps=P + 2),
               dict(scale=P + 1), dict(coef=P + 2), dict(step=P + 3), dict(x=P + 1), dict(x_prev=P + 2), dict(pred_x0=P + 2),
               dict(seeds=P), dict(temperature=P)):                                          # one of the pair without the other
        yield "seer_slot_cfg_ddim_step", tuple({**good, **kw}.values()), kw


def test_kernel_entry_points_refuse_bad_arguments_before_any_launch():
    """every refusal of the two entry points returns SEER_EINVAL on the host (16 = an aligned non-NULL pointer; no call here
    would pass its checks, so nothing is launched)"""
    from seervideoldm_amd import _lib
    from seervideoldm_amd.build import build_library
    build_library()
    lib = _lib.load()
    for fn, args, why in refusal_cases(16):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
