"""SlotSampler(dpm=True) without a GPU: the host logic of a mixed DDIM / DPM-Solver++ queue over tests/slot_dpm_ref.py and the analytic
Gaussian model of tests/test_slots_host.py.  Staggered requests -- S in {1, 2, 4, 6}, both orders, both discretisations,
lower_order_final on and off, DDIM clips between them -- in two slots, each against its own solo sampler (DPMSolverSampler over
tests/dpm_ref.py, DDIMSampler over the same backend); isolation from slot, neighbours and admission time; a dpm=True sampler on DDIM
requests against a plain one; the state words written at admission and by nobody but the kernel afterwards; a log-SNR schedule of
fewer entries than S; the refusals and the exports."""
import pytest
import torch

from seervideoldm_amd import DDIMSampler
from seervideoldm_amd.dpm import DPMSolverSampler
from tests import dpm_ref, slot_dpm_ref, slot_ref
from tests.test_slots_host import C, F1, FP, H, W, _Gaussian, _rel, _requests

# (method, S, scale, then the solver keywords of a "dpmpp" request); ENTRIES is what their schedules come to: S = 6 has stride 166 and
# therefore 7 entries on the uniform grid, 6 on the log-SNR one
SPECS = (("dpmpp", 4, 7.5, dict()),
         ("ddim", 6, 3.0, dict()),
         ("dpmpp", 6, 7.5, dict(discretize="logsnr", lower_order_final=False)),
         ("dpmpp", 1, 5.0, dict()),
         ("dpmpp", 2, 3.0, dict(order=1)),
         ("ddim", 2, 7.5, dict()),
         ("dpmpp", 6, 2.0, dict(lower_order_final=False)),
         ("dpmpp", 4, 7.5, dict(order=1, discretize="logsnr")))
ENTRIES = [4, 7, 6, 1, 2, 2, 7, 4]


def _mixed_requests(model):
    g = torch.Generator().manual_seed(13)
    reqs = []
    for k, (method, S, scale, solver) in enumerate(SPECS):
        reqs.append(dict(x_T=torch.randn((1, C, FP, H, W), generator=g), x0_emb=0.9 * torch.randn((1, C, F1, H, W), generator=g),
                         c=model.context(k, True), uc=model.context(k, False), S=S, scale=scale, tag=f"r{k}", method=method, **solver))
    return reqs


def _solo(model, r):
    """the request alone through its own sampler, batch 1 -> (latent, schedule entries)"""
    solver = {k: r[k] for k in ("order", "lower_order_final", "discretize") if k in r}
    smp = DPMSolverSampler("cpu", ops=dpm_ref, **solver) if r["method"] == "dpmpp" else DDIMSampler("cpu", ops=dpm_ref)
    lat, _ = smp.sample(model, r["S"], 1, (C, FP, H, W), x0_emb=r["x0_emb"], conditioning=r["c"][None], x_T=r["x_T"], verbose=False,
                        is_3d=True, unconditional_guidance_scale=r["scale"], unconditional_conditioning=r["uc"][None])
    return lat, int(smp.ddim_timesteps.shape[0])


def _sampler(model, slots=2, dpm=True, **kw):
    from seervideoldm_amd import SlotSampler
    return SlotSampler(model, slots, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu",
                       ops=slot_dpm_ref if dpm else slot_ref, **(dict(dpm=True) if dpm else {}), **kw)


def _by_hand(entries, slots=2):
    """the queue by hand: a clip of n entries stays n steps, a free slot (lowest first) takes the next request before the next step
    -> [(step, slot, request)] in finishing order, and the number of steps"""
    left, who, nxt, finished, n = [0] * slots, [None] * slots, 0, [], 0
    while True:
        for s in range(slots):
            if left[s] == 0 and nxt < len(entries):
                left[s], who[s], nxt = entries[nxt], nxt, nxt + 1
        if not any(left):
            return finished, n
        n += 1
        for s in range(slots):
            if left[s]:
                left[s] -= 1
                if left[s] == 0:
                    finished.append((n, s, who[s]))


def test_a_mixed_staggered_queue_equals_the_solo_runs():
    model = _Gaussian(len(SPECS))
    reqs = _mixed_requests(model)
    want = [_solo(model, r) for r in reqs]
    assert [n for _, n in want] == ENTRIES
    finish, steps = _by_hand(ENTRIES)
    # r0 (4) and r1 (7) open; r2 (6) follows r0 in slot 0 and leaves with step 10; r3 (1), r4 (2), r5 (2) pass through slot 1 meanwhile
    assert finish[:5] == [(4, 0, 0), (7, 1, 1), (8, 1, 3), (10, 0, 2), (10, 1, 4)] and steps == 17
    model.calls = 0
    smp = _sampler(model)
    assert smp.step() == [] and model.calls == 0
    got = list(smp.run(iter(reqs)))
    assert [tag for tag, _ in got] == [f"r{k}" for _, _, k in finish]
    assert model.calls == steps and smp.free_slots() == [0, 1]
    assert smp._step[:, 0].tolist() == [-1, -1]          # the counters ran down on their own
    for tag, lat in got:
        k = int(tag[1:])
        assert lat.shape == (1, C, FP, H, W) and torch.isfinite(lat).all()
        rel = _rel(lat, want[k][0])
        print(f"[slots-dpm] request {k} {SPECS[k]}: rel_l2 to its solo sampler {rel:.3g}")
        assert rel <= 2e-6, (k, rel)
    assert smp.step() == [] and model.calls == steps
    assert not smp._x.any() and not smp._x0.any()        # retired slots are zeroed; pred_x0 stays readable
    assert smp.pred_x0(0).shape == (1, C, FP, H, W) and smp._pred.any()


def test_a_slot_does_not_depend_on_its_slot_its_neighbours_or_its_admission_time():
    model = _Gaussian(len(SPECS))
    reqs = _mixed_requests(model)
    pick = lambda *ks: iter([reqs[k] for k in ks])
    a = dict(_sampler(model).run(pick(0, 1, 2, 6)))
    b = dict(_sampler(model, slots=3).run(pick(2, 1, 6)))               # three slots, one idle at times; other slots
    c = dict(_sampler(model).run(pick(1, 6, 3, 4, 2, 0)))               # behind other clips, beside other samplers, at other times
    for tag in ("r1", "r2", "r6"):
        assert torch.equal(a[tag], b[tag]) and torch.equal(a[tag], c[tag]), tag
    assert torch.equal(a["r0"], c["r0"])
    # the same clip through the other sampler, and at the other order, is another latent: method and order reach the kernel
    d = dict(_sampler(model).run(iter([{k: v for k, v in reqs[6].items() if k != "lower_order_final"} | dict(method="ddim")])))
    e = dict(_sampler(model).run(iter([dict(reqs[6], order=1)])))
    assert not torch.equal(d["r6"], a["r6"]) and not torch.equal(e["r6"], a["r6"])


def test_a_dpm_sampler_runs_ddim_requests_as_a_plain_one_does():
    model = _Gaussian(3)
    reqs = _requests(model)
    plain = dict(_sampler(model, dpm=False).run(iter(reqs)))
    for extra in ({}, {"method": "ddim"}, {"method": "ddim", "order": 2, "lower_order_final": True, "discretize": "uniform"},
                  {"lower_order_final": 1}):                # a default is a default by its truth, not by its type
        both = dict(_sampler(model, dpm=True).run(iter([dict(r, **extra) for r in reqs])))
        assert list(both) == list(plain)
        for tag in plain:
            assert torch.equal(both[tag], plain[tag]), tag


class _Watching:
    """tests.slot_dpm_ref with the state words recorded as every update finds and leaves them"""

    def __init__(self):
        self.found, self.left = [], []

    def __getattr__(self, name):
        return getattr(slot_dpm_ref, name)

    def slot_cfg_dpm_step(self, eps, x, scale, coef, step, dpm_coef, state, **kw):
        self.found.append(state.clone())
        slot_dpm_ref.slot_cfg_dpm_step(eps, x, scale, coef, step, dpm_coef, state, **kw)
        self.left.append(state.clone())


def test_the_host_writes_the_state_words_at_admission_only():
    from seervideoldm_amd import SlotSampler
    model = _Gaussian(len(SPECS))
    reqs = [{k: v for k, v in r.items() if k != "tag"} for r in _mixed_requests(model)]
    ops = _Watching()
    smp = SlotSampler(model, 2, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=ops, dpm=True)
    assert smp._dpm_state.dtype == torch.int32 and smp._dpm_state.tolist() == [[0, 0, 0, 0]] * 2
    assert tuple(smp._dpm_coef.shape) == (2, 64, 6) and not smp._dpm_coef.any()
    # (valid, valid, sampler, final step first order): r0 is 2M with the rule, r2 2M without, r4 first order, r1 DDIM; r6 has
    # lower_order_final=False, r0's 4 entries are fewer than 15
    words = {0: [0, 0, 2, 1], 1: [0, 0, 0, 0], 2: [0, 0, 2, 0], 4: [0, 0, 1, 1], 6: [0, 0, 2, 0]}
    admitted = {}                                        # slot -> words, since the last step
    for k in (0, 1):
        admitted[smp.submit(**reqs[k])] = words[k]
    assert smp._dpm_state.tolist() == [words[0], words[1]]
    queue, n = [2, 4, 6], 0
    while smp.active():
        smp.step()
        expect = ops.left[n - 1].clone() if n else torch.zeros((2, 4), dtype=torch.int32)
        for s, w in admitted.items():
            expect[s] = torch.tensor(w, dtype=torch.int32)
        assert torch.equal(ops.found[n], expect), n      # what the kernel left, but for the slots filled since: no other host write
        n, admitted = n + 1, {}
        while queue and smp.free_slots():
            k = queue.pop(0)
            admitted[smp.submit(**reqs[k])] = words[k]
    assert n == len(ops.found) == 7 + 2 + 7              # slot 1: r1, r4, r6 one behind the other (slot 0: r0, r2 in 10 steps)
    # the kernel's own walk of r0 (entries 3 .. 0, order 2 from its second step): the valid word of the other parity, one per step
    assert [t[0].tolist() for t in ops.left[:4]] == [[1, 0, 2, 1], [1, 1, 2, 1], [1, 1, 2, 1], [1, 1, 2, 1]]
    assert [t[1].tolist() for t in ops.left[:7]] == [[0, 0, 0, 0]] * 7                      # a DDIM slot: no word is written


def test_a_logsnr_schedule_of_fewer_entries_than_S_takes_its_slot_for_its_entries():
    model = _Gaussian(1)
    r = {k: v for k, v in _requests(model)[0].items() if k != "tag"}
    solo = DPMSolverSampler("cpu", discretize="logsnr")
    solo.make_schedule(60, verbose=False)
    n = int(solo.ddim_timesteps.shape[0])
    assert n == 59                                       # the targets crowd where lambda is steep: two of 60 share a training step
    smp = _sampler(model)
    s = smp.submit(**{**r, "S": 60, "method": "dpmpp", "discretize": "logsnr"})
    assert smp._left[s] == n and int(smp._step[s, 0]) == n - 1 and smp._dpm_state[s].tolist() == [0, 0, 2, 0]
    # the tables are the solo sampler's, bit for bit, and the rows behind them are as the constructor left them
    assert torch.equal(smp._dpm_coef[s, :n], solo.dpm_coef) and not smp._dpm_coef[s, n:].any()
    assert torch.equal(smp._coef[s, :n], solo.ddim_coef) and torch.equal(smp._ttab[s, :n], solo._t_table)
    assert smp._dpm_schedule(60, "logsnr")[2] is smp._dpm_schedule(60, "logsnr")[2]         # made once per (S, discretize)
    assert set(smp._dpm_tables) == {(60, "logsnr")}
    for _ in range(n - 1):
        assert smp.step() == []
    (slot, lat), = smp.step()
    assert slot == s and torch.isfinite(lat).all() and model.calls == n and smp.free_slots() == [0, 1]


def test_refusals():
    from seervideoldm_amd import SlotSampler
    model = _Gaussian(len(SPECS))
    reqs = [{k: v for k, v in r.items() if k != "tag"} for r in _mixed_requests(model)]
    kw = dict(shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=slot_dpm_ref)
    for other in ("plms", "stochastic", "editing"):
        with pytest.raises(ValueError, match=f"{other}=True"):
            SlotSampler(model, 2, dpm=True, **{other: True}, **kw)
    plain = _sampler(model, dpm=False)
    assert not plain.dpm and not hasattr(plain, "_dpm_state") and plain._kind == "slots"
    with pytest.raises(ValueError, match="dpm=True"):
        plain.submit(**reqs[0])
    assert plain.free_slots() == [0, 1]
    smp = _sampler(model, max_steps=6)
    assert smp.dpm and smp._kind == "slots-dpm" and smp._update[0] == "slot_cfg_dpm_step" and smp._front[0][0] == "slot_step_begin"
    with pytest.raises(ValueError, match="method"):
        smp.submit(**{**reqs[0], "method": "dpm"})
    with pytest.raises(ValueError, match="plms=True"):
        smp.submit(**{**reqs[1], "method": "plms"})
    for solver in (dict(order=1), dict(lower_order_final=False), dict(discretize="logsnr")):
        with pytest.raises(ValueError, match="dpmpp"):
            smp.submit(**reqs[1], **solver)              # the solver's keywords with method="ddim"
    for bad in (0, 3):
        with pytest.raises(ValueError, match="order"):
            smp.submit(**{**reqs[0], "order": bad})
    with pytest.raises(ValueError, match="discretize"):
        smp.submit(**{**reqs[0], "discretize": "quad"})
    with pytest.raises(ValueError, match="eta"):
        smp.submit(**reqs[0], eta=0.5)
    with pytest.raises(ValueError, match="stochastic=True"):
        smp.submit(**reqs[0], seed=3)
    with pytest.raises(ValueError, match="editing=True"):
        smp.submit(**reqs[0], t_start=2)
    with pytest.raises(ValueError, match="max_steps"):
        smp.submit(**reqs[6])                            # 7 entries
    assert smp.free_slots() == [0, 1]                    # a refused request takes no slot
    assert smp.submit(**reqs[0]) == 0 and smp.submit(**reqs[5]) == 1
    with pytest.raises(RuntimeError, match="busy"):
        smp.submit(**reqs[3])


def test_generate_queue_refuses_dpmpp_without_its_keyword():
    from seervideoldm_amd.pipeline import generate_queue

    class _FSText:
        def set_numframe(self, n):
            pass
    for kw in (dict(), dict(plms=True)):
        with pytest.raises(ValueError, match="sampler"):
            next(generate_queue(None, _FSText(), None, iter([dict(sampler="dpmpp")]), slots=2, num_frames=3, cond_frames=1, **kw))
    with pytest.raises(ValueError, match="sampler"):
        next(generate_queue(None, _FSText(), None, iter([dict(sampler="dpm")]), slots=2, num_frames=3, cond_frames=1, dpm=True))
    with pytest.raises(ValueError, match="sampler"):
        next(generate_queue(None, _FSText(), None, iter([dict(sampler="plms")]), slots=2, num_frames=3, cond_frames=1, dpm=True))


def test_exports():
    from seervideoldm_amd import _lib, ops
    assert "seer_slot_cfg_dpm_step" in _lib.SIGNATURES and callable(ops.slot_cfg_dpm_step)
    assert _lib.ABI_VERSION == 27
    assert ops.SLOT_DPM_STATE_WORDS == slot_dpm_ref.WORDS == 4 and ops.DPM_ROW_WORDS == slot_dpm_ref.ROW == 6


def dpm_refusal_cases(P):
    """(arguments of seer_slot_cfg_dpm_step without the stream, what is wrong) for every refusal of the entry point; P is a 4-byte
    aligned non-NULL pointer with at least 128 bytes behind it: d_hist stands 64 bytes after every other buffer, since it may be
    neither x nor x_prev (tests/test_gpu_slots_dpm.py passes a real pointer)"""
    Q = P + 64
    good = dict(eps=P, slots=2, C=4, F_total=4, cond_f=1, HW=64, scale=P, coef=P, dpm_coef=P, nsched=8, step=P, state=P, x=P, x_prev=P,
                d_hist=Q)
    for kw in (dict(eps=None), dict(scale=None), dict(coef=None), dict(dpm_coef=None), dict(step=None), dict(state=None), dict(x=None),
               dict(x_prev=None), dict(d_hist=None), dict(slots=0), dict(slots=-1), dict(slots=5), dict(nsched=0), dict(nsched=-3),
               dict(cond_f=4), dict(cond_f=5), dict(cond_f=-1), dict(C=0), dict(HW=0), dict(F_total=0, cond_f=0), dict(eps=P + 2),
               dict(scale=P + 1), dict(coef=P + 2), dict(dpm_coef=P + 3), dict(step=P + 3), dict(state=P + 2), dict(x=P + 1),
               dict(x_prev=P + 2), dict(d_hist=Q + 2), dict(d_hist=P), dict(x=Q), dict(x_prev=Q)):
        yield tuple({**good, **kw}.values()), kw


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    """every refusal of the entry point returns SEER_EINVAL on the host (no call here would pass its checks, so nothing is launched)"""
    from seervideoldm_amd import _lib
    from seervideoldm_amd.build import build_library
    build_library()
    lib = _lib.load()
    n = 0
    for args, why in dpm_refusal_cases(1 << 12):
        assert lib.seer_slot_cfg_dpm_step(*args, None) == -22, why
        n += 1
    assert n == 32
