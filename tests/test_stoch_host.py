"""Seeded stochastic sampling without a GPU: the CPU restatement of the generator (tests/stoch_ref.py) against the Random123
known-answer vectors and the moments of its normals, SlotSampler(stochastic=True, ops=tests.stoch_ref) over the analytic Gaussian
model of tests/test_slots_host.py against a solo float64 loop on the oracle's p_sample_ddim, every refusal, the exports."""
import numpy as np
import pytest
import torch

from oracle import seer_oracle as O
from tests import stoch_ref
from tests.test_slots_host import C, F1, FP, H, W, _Gaussian, _rel

f64 = torch.float64
PER_CLIP = C * FP * H * W


def test_known_answer_vectors():
    for counter, key, want in stoch_ref.KAT:
        got = stoch_ref.philox4x32_10(counter, key)
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    # the same three through the entry point's argument order: seed = the key, stream = counter words 2 and 3
    for counter, key, want in stoch_ref.KAT:
        got = stoch_ref.words(key[0] | key[1] << 32, counter[2] | counter[3] << 32, counter[1], counter[0], 1)
        assert tuple(int(v) for v in got[0]) == want


def test_the_normals_of_one_seed():
    n = stoch_ref.normals64(0x1234, stoch_ref.STREAM_STEP, 7, 1 << 20)
    assert n.shape == (1 << 20,) and np.isfinite(n).all()
    print(f"[stoch] 2^20 normals: max|n| {np.abs(n).max():.4f}, mean {n.mean():.5f}, var {n.var():.5f}")
    assert np.abs(n).max() <= 5.7683
    assert abs(n.mean()) <= 0.005 and abs(n.var() - 1.0) <= 0.01
    # the bound itself: u_a = 2^-24 is the smallest uniform
    assert abs(np.sqrt(-2.0 * np.log(2.0 ** -24)) - stoch_ref.MAX_ABS_NORMAL) < 1e-4
    u = stoch_ref.uniforms(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert u[0] == 2.0 ** -24 and u[1] == 1.0 - 2.0 ** -24 and (u.astype(np.float32) == u).all()
    # element e takes normal e & 3 of block e >> 2: a prefix is a prefix, whatever n
    assert np.array_equal(stoch_ref.normals64(0x1234, 1, 7, 1155), n[:1155])
    assert not np.array_equal(stoch_ref.normals64(0x1235, 1, 7, 64), n[:64])
    assert not np.array_equal(stoch_ref.normals64(0x1234, 1, 6, 64), n[:64])
    assert not np.array_equal(stoch_ref.normals64(0x1234, 0, 7, 64), n[:64])
    assert not np.array_equal(stoch_ref.normals64(0x1234 | 1 << 32, 1, 7, 64), n[:64])     # the high word is part of the key


# ---- SlotSampler(stochastic=True) over the stand-in -------------------------------------------------------------------------------
def _requests(model):
    g = torch.Generator().manual_seed(11)
    reqs = []
    for k, (S, scale, eta, seed, temp, given) in enumerate(((4, 7.5, 0.5, 1234, 1.0, False), (6, 3.0, 1.0, (7 << 32) | 5, 0.7, True),
                                                            (5, 7.5, 0.0, None, 1.0, True))):
        x_T = torch.randn((1, C, FP, H, W), generator=g)
        reqs.append(dict(x_T=x_T if given else None, x0_emb=0.9 * torch.randn((1, C, F1, H, W), generator=g), c=model.context(k, True),
                         uc=model.context(k, False), S=S, scale=scale, eta=eta, seed=seed, temperature=temp, tag=f"r{k}"))
    return reqs


def _solo64(model, k, r):
    """the request alone: the loop of DDIMSampler.ddim_sampling over the oracle's p_sample_ddim in float64, its noise the
    restatement's normals of (seed, stream 1, index) times the temperature"""
    sched = O.make_schedule(r["S"], r["eta"])
    ts = sched["ddim_timesteps"]

    def unet_fn(x, t, ctx, cond_frames):                 # rows: [uc | c] of the one clip
        return torch.stack([model.exact(x[0], t[0], model.mu_u[k]), model.exact(x[1], t[1], model.mu_c[k])])
    if r["x_T"] is None:
        x = torch.from_numpy(stoch_ref.normals64(r["seed"], stoch_ref.STREAM_START, 0, PER_CLIP)).reshape(1, C, FP, H, W)
    else:
        x = r["x_T"].double()
    for index in reversed(range(len(ts))):
        if r["eta"]:
            noise = r["temperature"] * torch.from_numpy(stoch_ref.normals64(r["seed"], stoch_ref.STREAM_STEP, index, PER_CLIP))
            noise = noise.reshape(x.shape)
        else:
            noise = torch.zeros_like(x)
        t = torch.full((1,), int(ts[index]), dtype=torch.long)
        x, _ = O.p_sample_ddim(unet_fn, x, model.context(k, True)[None], t, index, sched, x0_emb=r["x0_emb"].double(),
                               scale=r["scale"], uc=model.context(k, False)[None], noise=noise)
        assert x.dtype == f64
    return x, len(ts)


def _sampler(model, slots=2, **kw):
    from seervideoldm_amd import SlotSampler
    return SlotSampler(model, slots, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=stoch_ref,
                       stochastic=True, **kw)


def test_staggered_stochastic_requests_equal_their_solo_runs():
    model = _Gaussian(3)
    reqs = _requests(model)
    want = [_solo64(model, k, r) for k, r in enumerate(reqs)]
    assert [n for _, n in want] == [4, 7, 5]
    smp = _sampler(model)
    got = list(smp.run(iter(reqs)))
    assert [tag for tag, _ in got] == ["r0", "r1", "r2"] and model.calls == 9 and smp.free_slots() == [0, 1]
    for (tag, lat), (ref, _), r in zip(got, want, reqs):
        rel = _rel(lat, ref)
        print(f"[stoch] request {tag} (S = {r['S']}, eta {r['eta']}, temperature {r['temperature']}): rel_l2 to its solo float64 loop "
              f"{rel:.3g}")
        assert lat.shape == (1, C, FP, H, W) and torch.isfinite(lat).all() and rel <= 1e-6, (tag, rel)
    # the noise is in the result: the same request with eta = 0, or with another seed, is another latent
    other = dict(_sampler(model).run(iter([{**reqs[0], "eta": 0.0}, {**reqs[0], "seed": 1235, "tag": "s"}])))
    assert not torch.equal(other["r0"], got[0][1]) and not torch.equal(other["s"], got[0][1])
    assert _sampler(model)._seeds.dtype == torch.int32 and tuple(_sampler(model, slots=3)._temp.shape) == (3,)


def test_a_stochastic_clip_does_not_depend_on_its_neighbours_or_the_slot_count():
    model = _Gaussian(3)
    reqs = _requests(model)
    pair = dict(_sampler(model).run(iter(reqs[:2])))
    other = dict(_sampler(model, slots=3).run(iter([reqs[2], reqs[1]])))          # slot 1 of three, behind another neighbour
    alone = dict(_sampler(model, slots=1).run(iter([reqs[1]])))
    late = dict(_sampler(model, slots=2).run(iter([reqs[0], reqs[2], reqs[1]])))  # admitted when r0 leaves, into slot 0
    for run in (other, alone, late):
        assert torch.equal(run["r1"], pair["r1"])
    assert torch.equal(late["r0"], pair["r0"])


def test_refusals():
    from seervideoldm_amd import DDIMSampler, SlotSampler
    model = _Gaussian(3)
    reqs = [{k: v for k, v in r.items() if k != "tag"} for r in _requests(model)]
    smp = _sampler(model)
    with pytest.raises(ValueError, match="seed"):
        smp.submit(**{**reqs[0], "seed": None, "x_T": torch.zeros((1, C, FP, H, W))})       # eta > 0 without a seed
    with pytest.raises(ValueError, match="x_T"):
        smp.submit(**{**reqs[2], "x_T": None})                                              # no start code and no seed
    with pytest.raises(ValueError, match="seed"):
        smp.submit(**{**reqs[0], "seed": 1 << 64})
    with pytest.raises(ValueError, match="plms"):
        smp.submit(**reqs[0], method="plms")
    assert smp.free_slots() == [0, 1]                    # a refused request takes no slot
    with pytest.raises(ValueError, match="plms"):
        SlotSampler(model, 2, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=stoch_ref, plms=True,
                    stochastic=True)
    # without stochastic=True everything is as it was: eta, seed and temperature are refused
    plain = SlotSampler(model, 2, shape=(C, FP, H, W), cond_frames=F1, context_shape=(1, 2), device="cpu", ops=stoch_ref)
    base = {k: v for k, v in reqs[2].items() if k not in ("eta", "seed", "temperature")}
    for kw in (dict(eta=0.5), dict(eta=0.5, seed=3), dict(seed=3), dict(temperature=0.7)):
        with pytest.raises(ValueError, match="eta" if "eta" in kw else "stochastic"):
            plain.submit(**base, **kw)
    assert plain.free_slots() == [0, 1] and not hasattr(plain, "_seeds")
    # DDIMSampler.sample: what is not built stays NotImplementedError, a sharded model with a seed is a ValueError
    d = DDIMSampler("cpu")
    d.make_schedule(4, ddim_eta=0.5, verbose=False)
    x = torch.zeros((1, C, FP, H, W))
    for kw in (dict(noise_dropout=0.1), dict(repeat_noise=True)):
        with pytest.raises(NotImplementedError):
            d.p_sample_ddim(model, x, None, torch.tensor([1]), 0, seeds=torch.zeros((1, 2), dtype=torch.int32), **kw)
    model._shard = object()
    with pytest.raises(ValueError, match="shard"):
        d.sample(model, 4, 1, (C, FP, H, W), eta=0.5, is_3d=True, verbose=False, seed=3)
    model._shard = None
    for bad in ([1, 2], -1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            d.sample(model, 4, 1, (C, FP, H, W), eta=0.5, is_3d=True, verbose=False, seed=bad)


def test_generate_queue_refuses_seeded_requests_without_stochastic():
    """the keys are checked when a request is admitted; the model objects are only called after that"""
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
             scale=7.5, tag="a")
    with pytest.raises(ValueError, match="stochastic"):
        list(generate_queue(_Gaussian(1), _Fst(), _Vae(), [dict(r, seed=3)], slots=1, num_frames=3, cond_frames=1))
    with pytest.raises(ValueError, match="noise"):
        list(generate_queue(_Gaussian(1), _Fst(), _Vae(), [r], slots=1, num_frames=3, cond_frames=1, stochastic=True))


def test_seed_words_and_row_seeds():
    from seervideoldm_amd import ops
    from seervideoldm_amd.ddim import _row_seeds
    w = ops.seed_words([0, 1234, (7 << 32) | 5, (1 << 64) - 1, 0x80000000])
    assert w.dtype == torch.int32 and w.tolist() == [[0, 0], [1234, 0], [5, 7], [-1, -1], [-(1 << 31), 0]]
    assert [stoch_ref.seed_of(r) for r in w] == [0, 1234, (7 << 32) | 5, (1 << 64) - 1, 0x80000000]
    assert _row_seeds(None, 3) is None and _row_seeds(10, 3) == [10, 11, 12] and _row_seeds([5, 9], 2) == [5, 9]
    assert _row_seeds((1 << 64) - 1, 2) == [(1 << 64) - 1, 0]                               # s + i wraps like a uint64
    with pytest.raises(ValueError):
        ops.seed_words([-1])


def test_exports():
    import inspect

    from seervideoldm_amd import SlotSampler, _lib, ops, pipeline
    new = {"seer_philox_u32", "seer_philox_normal", "seer_cfg_ddim_step", "seer_slot_cfg_ddim_step"}
    assert new <= set(_lib.SIGNATURES)
    for name in ("philox_u32", "philox_normal", "cfg_ddim_step_rng", "cfg_ddim_step_rng_dev", "slot_cfg_ddim_step_rng", "seed_words"):
        assert callable(getattr(ops, name)), name
    for name in ("philox_normal", "cfg_ddim_step_rng", "slot_cfg_ddim_step_rng", "slot_step_begin"):
        assert callable(getattr(stoch_ref, name)), name
    assert inspect.signature(SlotSampler.__init__).parameters["stochastic"].default is False
    assert inspect.signature(pipeline.generate_queue).parameters["stochastic"].default is False
    assert {"seed", "temperature", "eta"} <= set(inspect.signature(SlotSampler.submit).parameters)


def refusal_cases(P):
    """(entry point, arguments without the stream, what is wrong) for every refusal of the two generator entry points and of the
    seeded modes of seer_cfg_ddim_step (host index, then device index) and seer_slot_cfg_ddim_step; P is a 4-byte aligned non-NULL
    pointer that stands for every buffer (tests/test_gpu_stoch.py passes a real one)"""
    good = dict(seed=1, stream=1, index=0, first_block=0, n_blocks=4, out=P)
    for kw in (dict(out=None), dict(out=P + 2), dict(n_blocks=0), dict(n_blocks=-1), dict(first_block=1 << 32),
               dict(first_block=(1 << 32) - 2, n_blocks=3)):
        yield "seer_philox_u32", tuple({**good, **kw}.values()), kw
    good = dict(seed=1, stream=1, index=0, n=5, out=P)
    for kw in (dict(out=None), dict(out=P + 1), dict(n=0), dict(n=-3), dict(n=1 << 31)):
        yield "seer_philox_normal", tuple({**good, **kw}.values()), kw
    for idx in (dict(index=0, step=None), dict(index=-1, step=P)):
        good = dict(eps=P, cfg=1, b=2, C=4, F_total=4, cond_f=1, HW=64, scale=7.5, coef=P, **idx, x=P, noise=None, seeds=P, temperature=1.0,
                    x_prev=P, pred_x0=P)
        # seeds=None left the table: with noise NULL too that call is now the deterministic step.  Neither index source, both at once,
        # and both noise sources at once are refused
        bad_idx = (dict(index=-1), dict(step=P)) if idx["step"] is None else (dict(step=None), dict(index=0))
        for kw in (dict(eps=None), dict(coef=None), dict(x=None), dict(x_prev=None), *bad_idx, dict(noise=P), dict(b=0), dict(C=0),
                   dict(HW=0), dict(cond_f=4), dict(cond_f=5), dict(cond_f=-1), dict(seeds=P + 2), dict(x=P + 1),
                   dict(C=1 << 15, F_total=2, HW=1 << 16), dict(C=1 << 14, F_total=9, cond_f=1, HW=1 << 14)):        # 2^31 and 2^31 elements
            yield "seer_cfg_ddim_step", tuple({**good, **kw}.values()), kw
    good = dict(eps=P, slots=2, C=4, F_total=4, cond_f=1, HW=64, scale=P, coef=P, nsched=8, step=P, x=P, seeds=P, temperature=P,
                x_prev=P, pred_x0=P)
    for kw in (dict(eps=None), dict(scale=None), dict(coef=None), dict(step=None), dict(x=None), dict(seeds=None),
               dict(temperature=None), dict(x_prev=None), dict(slots=0), dict(nsched=0), dict(cond_f=4), dict(cond_f=5),
               dict(cond_f=-1), dict(C=0), dict(HW=0), dict(seeds=P + 2), dict(temperature=P + 1), dict(step=P + 3),
               dict(pred_x0=P + 2), dict(C=1 << 15, F_total=2, HW=1 << 16)):
        yield "seer_slot_cfg_ddim_step", tuple({**good, **kw}.values()), kw


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
    assert n >= 60
