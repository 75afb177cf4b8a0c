"""SlotSampler(plms=True) without a GPU: the host logic of a mixed DDIM / PLMS queue over tests/slot_plms_ref.py and the analytic
Gaussian model of tests/test_slots_host.py.  Staggered requests with methods (plms, ddim, plms, plms at S = 1) against a float64
solo loop per request, the n + 1 bookkeeping by hand, isolation from the neighbours, a plms=True sampler on DDIM requests against
a plms=False one, the refusals and the exports."""
import pytest
import torch

from seervideoldm_amd import DDIMSampler
from tests import plms_oracle, slot_plms_ref, slot_ref
from tests.test_slots_host import C, F1, FP, H, W, _Gaussian, _rel, _requests, _solo64

METHODS = ("plms", "ddim", "plms", "plms")


def _mixed_requests(model):
    """the three seeded requests of tests/test_slots_host.py and a fourth with S = 1 (one entry: two evaluations, t_next = t)"""
    reqs = _requests(model)
    g = torch.Generator().manual_seed(12)
    reqs.append(dict(x_T=torch.randn((1, C, FP, H, W), generator=g), x0_emb=0.9 * torch.randn((1, C, F1, H, W), generator=g),
                     c=model.context(3, True), uc=model.context(3, False), S=1, scale=5.0, tag="r3"))
    return [dict(r, method=m) for r, m in zip(reqs, METHODS)]


def _solo_plms64(model, k, r):
    """the request alone: the PLMS loop of PLMSSampler.plms_sampling over DDIMSampler("cpu")'s own tables, in float64"""
    smp = DDIMSampler("cpu")
    smp.make_schedule(r["S"], verbose=False)
    coef, ttab = smp.ddim_coef.double(), smp._t_table
    x, x0_emb = r["x_T"][0].double(), r["x0_emb"][0].double()

    def eps(x, t):
        x_cat = torch.cat([x0_emb, x], dim=1)
        eu, ec = model.exact(x_cat, t, model.mu_u[k]), model.exact(x_cat, t, model.mu_c[k])
        return (eu + r["scale"] * (ec - eu))[:, F1:]

    def update(x, e, index):
        a_t, a_prev, sigma, s1m = coef[index].tolist()
        pred = (x - s1m * e) / a_t ** 0.5
        return a_prev ** 0.5 * pred + (1 - a_prev - sigma ** 2) ** 0.5 * e

    old = []
    for index in reversed(range(coef.shape[0])):
        e = eps(x, ttab[index])
        if not old:
            ep = (e + eps(update(x, e, index), ttab[max(index - 1, 0)])) / 2
        else:
            ep = plms_oracle.combine(e, old)
        x = update(x, ep, index)
        old = (old + [e])[-3:]
    return x[None], coef.shape[0]


def _sampler(model, slots=2, plms=True, **kw):
    from seervideoldm_amd import SlotSampler
    return SlotSampler(model, slots, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu",
                       ops=slot_plms_ref if plms else slot_ref, plms=plms, **kw)


def test_a_mixed_staggered_queue_equals_the_solo_runs():
    model = _Gaussian(4)
    reqs = _mixed_requests(model)
    want = [(_solo_plms64 if r["method"] == "plms" else _solo64)(model, k, r) for k, r in enumerate(reqs)]
    assert [n for _, n in want] == [4, 7, 5, 1]
    smp = _sampler(model)
    sub = lambda r: smp.submit(**{k: v for k, v in r.items() if k != "tag"})
    assert smp.step() == [] and model.calls == 0
    assert (sub(reqs[0]), sub(reqs[1])) == (0, 1) and smp.active() == [0, 1]
    assert smp._state[:, :3].tolist() == [[1, 0, 2], [0, 0, 2]] and smp._step[:, 0].tolist() == [3, 6]
    # by hand, a PLMS clip of n entries staying n + 1 steps: r0 (plms, 4) leaves slot 0 with step 5; r2 (plms, 5) takes it and leaves
    # with step 11; r1 (ddim, 7) leaves slot 1 with step 7; r3 (plms, 1) takes it and leaves with step 9
    free_after = {1: [], 2: [], 3: [], 4: [], 5: [0], 6: [], 7: [1], 8: [], 9: [1], 10: [1], 11: [0, 1]}
    admit_after = {5: 2, 7: 3}
    who = {(5, 0): 0, (7, 1): 1, (9, 1): 3, (11, 0): 2}
    finished = []
    for n in range(1, 12):
        if n == 1:
            held = smp.pred_x0(0)
        done = smp.step()
        if n == 1:                                       # the first evaluation of a PLMS clip: no pred_x0, no latent, no count
            assert torch.equal(smp.pred_x0(0), held) and torch.equal(smp._x[0], reqs[0]["x_T"][0])
            assert smp._step[:, 0].tolist() == [3, 5] and smp._state[0, :3].tolist() == [2, 1, 0]
        if n == 2:
            assert smp._step[:, 0].tolist() == [2, 4] and int(smp._state[0, 0]) == 3
        assert smp.free_slots() == free_after[n], n
        finished += [(n, s) for s, _ in done]
        for s, lat in done:
            k = who[(n, s)]
            assert lat.shape == (1, C, FP, H, W) and torch.isfinite(lat).all()
            rel = _rel(lat, want[k][0])
            print(f"[slots-plms] request {k} ({reqs[k]['method']}, S = {reqs[k]['S']}, scale {reqs[k]['scale']}) left slot {s} with step "
                  f"{n}: rel_l2 to its solo float64 loop {rel:.3g}")
            assert rel <= 2e-6, (k, rel)
            assert not smp._x[s].any() and not smp._x0[s].any() and not smp._xprov[s].any()      # a retired slot is zeroed
        if n in admit_after:
            assert sub(reqs[admit_after[n]]) == (0 if n == 5 else 1) and smp.free_slots() == []
    assert finished == list(who) and model.calls == 11
    assert smp._step[:, 0].tolist() == [-1, -1]          # the counters ran down on their own
    assert smp.step() == [] and model.calls == 11
    # run() drives the same sequence: the same latents, in finishing order
    model2 = _Gaussian(4)
    smp2 = _sampler(model2)
    got = list(smp2.run(iter(reqs)))
    assert [tag for tag, _ in got] == ["r0", "r1", "r3", "r2"] and model2.calls == 11 and smp2.free_slots() == [0, 1]
    for tag, lat in got:
        assert _rel(lat, want[int(tag[1])][0]) <= 2e-6, tag


def test_a_slot_does_not_depend_on_its_neighbours_or_their_samplers():
    model = _Gaussian(4)
    reqs = _mixed_requests(model)
    a = dict(_sampler(model).run(iter(reqs[:3])))                                   # r2 behind r0 in slot 0, next to the DDIM clip
    b = dict(_sampler(model, slots=3).run(iter([reqs[2], reqs[1]])))                # three slots, one idle throughout
    c = dict(_sampler(model).run(iter([reqs[1], reqs[2], reqs[3], reqs[0]])))       # other slots, other neighbours, other times
    for tag in ("r1", "r2"):
        assert torch.equal(a[tag], b[tag]) and torch.equal(a[tag], c[tag]), tag
    assert torch.equal(a["r0"], c["r0"])
    # the same clip through the other sampler is another latent: the method reaches the kernels
    d = dict(_sampler(model).run(iter([dict(reqs[2], method="ddim")])))
    assert not torch.equal(d["r2"], a["r2"])


def test_a_plms_sampler_runs_ddim_requests_as_a_plain_one_does():
    model = _Gaussian(3)
    reqs = _requests(model)
    plain = dict(_sampler(model, plms=False).run(iter(reqs)))
    for extra in ({}, {"method": "ddim"}):
        both = dict(_sampler(model, plms=True).run(iter([dict(r, **extra) for r in reqs])))
        assert list(both) == list(plain)
        for tag in plain:
            assert torch.equal(both[tag], plain[tag]), tag


def test_refusals():
    model = _Gaussian(4)
    reqs = [{k: v for k, v in r.items() if k != "tag"} for r in _mixed_requests(model)]
    plain = _sampler(model, plms=False)
    assert not plain.plms and not hasattr(plain, "_ring")
    with pytest.raises(ValueError, match="plms=True"):
        plain.submit(**reqs[0])
    assert plain.free_slots() == [0, 1]
    assert plain.submit(**reqs[1]) == 0                  # method="ddim" is what it runs anyway
    smp = _sampler(model, max_steps=6)
    with pytest.raises(ValueError, match="method"):
        smp.submit(**{**reqs[0], "method": "dpm"})
    with pytest.raises(ValueError, match="eta"):
        smp.submit(**reqs[0], eta=0.5)
    with pytest.raises(ValueError, match="max_steps"):
        smp.submit(**{**reqs[1], "method": "plms"})      # 7 entries: the table is what max_steps bounds, not the n + 1 steps
    with pytest.raises(ValueError, match="x_T"):
        smp.submit(**{**reqs[0], "x_T": torch.zeros((1, C, FP + 1, H, W))})
    model._shard = object()
    with pytest.raises(ValueError, match="shard"):
        smp.submit(**reqs[0])
    model._shard = None
    assert smp.free_slots() == [0, 1]                    # a refused request takes no slot


def test_generate_queue_refuses_plms_without_its_keyword():
    from seervideoldm_amd.pipeline import generate_queue

    class _FSText:
        def set_numframe(self, n):
            pass
    for bad in ("plms", "dpm"):
        with pytest.raises(ValueError, match="sampler"):
            next(generate_queue(None, _FSText(), None, iter([dict(sampler=bad)]), slots=2, num_frames=3, cond_frames=1))
    with pytest.raises(ValueError, match="sampler"):
        next(generate_queue(None, _FSText(), None, iter([dict(sampler="dpm")]), slots=2, num_frames=3, cond_frames=1, plms=True))


def test_exports():
    from seervideoldm_amd import _lib, ops
    assert {"seer_slot_step_begin", "seer_slot_cfg_plms_step"} <= set(_lib.SIGNATURES)
    assert callable(ops.slot_plms_step_begin) and callable(ops.slot_cfg_plms_step)
    assert ops.SLOT_STATE_WORDS == slot_plms_ref.WORDS == 8


def plms_refusal_cases(P):
    """(entry point, arguments without the stream, what is wrong) for every refusal of the two entry points; P is a 4-byte aligned
    non-NULL pointer with at least 128 bytes behind it: x_prov stands 64 bytes after every other buffer, since it may not be x
    (tests/test_gpu_slots_plms.py passes a real pointer)"""
    Q = P + 64
    good = dict(x0_emb=P, x=P, x_prov=Q, slots=2, reps=2, C=4, f1=1, F_pred=3, HW=64, t_table=P, nsched=8, step=P, state=P, sample=P,
                t_out=P)
    for kw in (dict(x=None), dict(t_table=None), dict(step=None), dict(sample=None), dict(t_out=None), dict(x0_emb=None),
               dict(slots=0), dict(nsched=0), dict(reps=0), dict(reps=3), dict(C=0), dict(F_pred=0), dict(HW=0), dict(f1=-1),
               dict(x=P + 2), dict(t_table=P + 1), dict(t_out=P + 3), dict(step=P + 2), dict(sample=P + 1), dict(x0_emb=P + 2),
               dict(x_prov=None), dict(state=None), dict(x_prov=Q + 2), dict(state=P + 1), dict(x_prov=P), dict(x=Q)):
        yield "seer_slot_step_begin", tuple({**good, **kw}.values()), kw
    good = dict(eps=P, slots=2, C=4, F_total=4, cond_f=1, HW=64, scale=P, coef=P, nsched=8, step=P, state=P, ring=P, x=P, x_prov=Q,
                x_prev=P, pred_x0=P)
    for kw in (dict(eps=None), dict(scale=None), dict(coef=None), dict(step=None), dict(x=None), dict(x_prev=None), dict(slots=0),
               dict(nsched=0), dict(cond_f=4), dict(cond_f=5), dict(cond_f=-1), dict(C=0), dict(HW=0), dict(eps=P + 2),
               dict(scale=P + 1), dict(coef=P + 2), dict(step=P + 3), dict(x=P + 1), dict(x_prev=P + 2), dict(pred_x0=P + 2),
               dict(state=None), dict(ring=None), dict(x_prov=None), dict(state=P + 2), dict(ring=P + 1), dict(x_prov=Q + 3),
               dict(x_prov=P), dict(x=Q)):
        yield "seer_slot_cfg_plms_step", tuple({**good, **kw}.values()), kw


def test_kernel_entry_points_refuse_bad_arguments_before_any_launch():
    """every refusal of the two entry points returns SEER_EINVAL on the host (no call here would pass its checks, so nothing is
    launched)"""
    from seervideoldm_amd import _lib
    from seervideoldm_amd.build import build_library
    build_library()
    lib = _lib.load()
    n = 0
    for fn, args, why in plms_refusal_cases(1 << 12):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    assert n == 26 + 28
