"""The exponential moving average of the trained weights without a GPU, on the torch stand-ins (tests/ema_ref.py): the schedule against
the reference's own LitEma (tests/golden/ema_litema.npz), the trainer's wiring in both optimizer modes -- once per optimizer step,
bit for bit the host recurrence, a passenger of the step --, ema_scope, the checkpoint files, the refusals, the surface and a 2-rank
gloo run.  Runs everywhere (CPU)."""
import inspect
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist

from seervideoldm_amd.trainer import SeerTrainer, ema_one_minus_decay
from tests import ema_ref as R
from tests.test_dist_gloo import ROOT, _spawn
from tests.test_train_batch_cpu import CFG, FS, HP

FR, COND = 3, 1


def _models():
    """fresh 320-wide one-layer models (sync_modules writes into them: no two trainers of a test share them)"""
    from seervideoldm_amd import FSTextTransformer, SeerUNet, synth
    unet = SeerUNet(**CFG)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG)), strict=True)
    fst = FSTextTransformer(num_frames=FS["num_frames"], in_channels=192, out_channels=192, n_heads=2, num_layers=1, cross_attention_dim=192)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(**FS)), strict=True)
    fst.set_numframe(FR)
    return unet, fst


def _trainer(tops, models=None, **kw):
    from tests import torch_ops_backend as tob
    unet, fst = models or _models()
    return SeerTrainer(unet, fst, ops=tob, tops=tops, **{**HP, **kw})


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((1, 4, FR, 8, 8), generator=g), torch.randn((1, 4, FR - COND, 8, 8), generator=g), torch.tensor([100 + 37 * seed]),
            torch.randn((1, 77, 192), generator=g))


def _micro(tr, seed):
    """one micro-batch; the optimizer steps when the accumulation says so.  -> (loss, stepped)"""
    x, noise, t, text = _batch(seed)
    loss = tr.forward_backward(x, noise, t, text, COND)
    stepped = tr.accumulate()
    if stepped:
        tr.optimizer_step()
    return loss, stepped


def _flat(tr, what):
    return torch.cat([getattr(tr.pu, what).reshape(-1), getattr(tr.pf, what).reshape(-1)]).clone()


def _state(tr):
    return [t.clone() for P in (tr.pu, tr.pf) for t in P.state().values()]


def _same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x.numpy().view(np.uint8), y.numpy().view(np.uint8)) for x, y in zip(a, b)) and len(a) == len(b)


# ---- the schedule -------------------------------------------------------------------------------------------------------------------------
def test_one_minus_decay_equals_litemas_at_every_update_of_the_three_runs():
    fx = R.fixture()
    assert [len(fx[r]["omd"]) for r in R.RUNS] == [100, 20, 5]
    for r in R.RUNS:
        run = fx[r]
        got = [ema_one_minus_decay(run["decay"], n, run["warmup"]) for n in range(1, len(run["omd"]) + 1)]
        assert all(isinstance(o, float) and float(np.float32(o)) == o for o in got)              # exactly an fp32 value
        assert np.array_equal(R.bits(got), R.bits(run["omd"])), r
        assert np.array_equal(R.bits([R.omd32(run["decay"], n, run["warmup"]) for n in range(1, len(got) + 1)]), R.bits(run["omd"]))
        # ... and the recorded shadows are the host recurrence over the recorded snapshots: the restatement the other tests lean on
        assert np.array_equal(R.bits(R.recurrence(run["p0"], run["p"], run["omd"])), R.bits(run["shadow"])), r
    o = fx["d0.9"]["omd"]
    assert R.bits(o[78]) != R.bits(o[79]) and len({int(b) for b in R.bits(o[79:])}) == 1        # the min changes sides at n = 80
    assert len({int(b) for b in R.bits(fx["nowarm"]["omd"])}) == 1 and ema_one_minus_decay(0.9999, 10 ** 6, True) == fx["nowarm"]["omd"][0]
    assert ema_one_minus_decay(1.0, 5, False) == 0.0 and ema_one_minus_decay(0.0, 5, False) == 1.0


@pytest.mark.parametrize("bad", [-1e-9, 1.0000001, -1.0, 2.0, math.nan, math.inf, -math.inf])
def test_values_outside_the_unit_interval_are_refused(bad):
    with pytest.raises(ValueError, match="ema_decay"):
        ema_one_minus_decay(bad, 1, True)


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adam8", [False, True])
def test_three_optimizer_steps_of_two_micro_batches(adam8):
    """gradient_accumulation_steps = 2, six micro-batches: the average moved 3 times, equals the host recurrence over the parameter
    snapshots bit for bit, and p, the optimizer state and the losses are those of a use_ema=False trainer fed the same inputs"""
    tops_e, tops_p = R.train_ops(), R.train_ops()
    kw = dict(gradient_accumulation_steps=2, use_8bit_adam=adam8)
    tr = _trainer(tops_e, use_ema=True, ema_decay=0.9, **kw)
    plain = _trainer(tops_p, **kw)
    assert plain.pu.ema is None and plain.pf.ema is None and plain.ema_state_bytes() == 0 and not plain.use_ema
    assert torch.equal(tr.pu.ema, tr.pu.p) and tr.pu.ema.data_ptr() != tr.pu.p.data_ptr() and tr.pu.ema.numel() == tr.pu.n
    assert tr.ema_state_bytes() == 4 * (tr.pu.n + tr.pf.n) and tr.optimizer_state_bytes() == plain.optimizer_state_bytes()
    ema0, snaps = _flat(tr, "ema"), []
    for i in range(6):
        la, sa = _micro(tr, i)
        lb, sb = _micro(plain, i)
        assert torch.equal(la, lb) and sa == sb == (i % 2 == 1)
        if sa:
            snaps.append(_flat(tr, "p"))
            assert tr.ema_num_updates == len(snaps)
        assert torch.equal(_flat(tr, "p"), _flat(plain, "p")) and _same(_state(tr), _state(plain))
        assert torch.equal(tr.pu.pb, plain.pu.pb) and torch.equal(tr.pf.pb, plain.pf.pb)
    name = "adamw8_ema_step" if adam8 else "adamw_ema_step"
    omds = [R.omd32(0.9, n, True) for n in (1, 2, 3)]
    assert [c[0] for c in tops_e.ema_calls] == [name] * 6 and tops_e.plain_calls == []          # two segments per step, 3 steps
    assert np.array_equal(R.bits([c[1] for c in tops_e.ema_calls]), R.bits(np.repeat(omds, 2)))
    assert tops_p.ema_calls == [] and tops_p.plain_calls == [name.replace("_ema", "")] * 6
    want = R.recurrence(ema0.numpy(), [s.numpy() for s in snaps], omds)
    assert np.array_equal(R.bits(_flat(tr, "ema")), R.bits(want[-1]))
    assert not torch.equal(_flat(tr, "ema"), ema0) and not torch.equal(_flat(tr, "ema"), snaps[-1])
    pad = torch.ones(tr.pu.n, dtype=torch.bool)                                                  # the padding of the average stays zero
    for k in tr.pu.names:
        o = tr.pu.offsets[k]
        pad[o:o + tr.pu.view(tr.pu.p, k).numel()] = False
    assert not tr.pu.ema[pad].any()
    # without the warm-up the first update already uses 1 - decay
    tr2 = _trainer(R.train_ops(), use_ema=True, ema_decay=0.75, ema_warmup=False, use_8bit_adam=adam8)
    _micro(tr2, 0)
    assert tr2.tops.ema_calls[0][1] == 0.25 and tr2.ema_num_updates == 1


@pytest.fixture(scope="module")
def stepped():
    """a trainer with the average after two optimizer steps (fp32 mode); tests that change it put it back"""
    tr = _trainer(R.train_ops(), use_ema=True, ema_decay=0.9)
    for i in range(2):
        _micro(tr, i)
    return tr


def _module_bits(tr):
    return {s: {k: v.detach().clone() for k, v in m.state_dict().items()} for s, m in (("unet", tr.unet), ("fstext", tr.fstext))}


def test_ema_scope_exchanges_in_place_and_restores_every_bit(stepped):
    tr = stepped
    tr.sync_modules()
    before = dict(p=_flat(tr, "p"), pb=_flat(tr, "pb"), ema=_flat(tr, "ema"), mods=_module_bits(tr))
    ptrs = [t.data_ptr() for P in (tr.pu, tr.pf) for t in (P.p, P.pb, P.ema)]
    avg = tr.ema_state_dict()
    raw = tr.trainable_state_dict()
    assert set(avg["unet"]) == set(raw["unet"]) and any(not torch.equal(avg["unet"][k], raw["unet"][k]) for k in raw["unet"])
    with tr.ema_scope() as inside:
        assert inside is tr
        assert [t.data_ptr() for P in (tr.pu, tr.pf) for t in (P.p, P.pb, P.ema)] == ptrs                 # in place
        assert torch.equal(_flat(tr, "p"), before["ema"]) and torch.equal(_flat(tr, "ema"), before["p"])
        assert torch.equal(_flat(tr, "pb"), before["ema"].to(torch.bfloat16))
        now = _module_bits(tr)
        again = tr.ema_state_dict()
        for s in ("unet", "fstext"):
            n_train = 0
            for k, v in now[s].items():
                if k in avg[s]:
                    assert torch.equal(v, avg[s][k].reshape(v.shape)) and torch.equal(again[s][k], avg[s][k]), k
                    n_train += 1
                else:
                    assert torch.equal(v, before["mods"][s][k]), k                                       # frozen: untouched
            assert n_train == len(avg[s]) > 0
        x, noise, t, text = _batch(0)
        with pytest.raises(RuntimeError, match="ema_scope"):
            tr.optimizer_step()
        with pytest.raises(RuntimeError, match="ema_scope"):
            tr.forward_backward(x, noise, t, text, COND)
        with pytest.raises(RuntimeError, match="ema_scope"):
            with tr.ema_scope():
                pass
    assert torch.equal(_flat(tr, "p"), before["p"]) and torch.equal(_flat(tr, "ema"), before["ema"])
    assert torch.equal(_flat(tr, "pb"), before["pb"])
    after = _module_bits(tr)
    assert all(torch.equal(after[s][k], before["mods"][s][k]) for s in after for k in after[s])
    # an exception inside the scope still exchanges back
    with pytest.raises(KeyError):
        with tr.ema_scope():
            raise KeyError("x")
    assert torch.equal(_flat(tr, "p"), before["p"]) and torch.equal(_flat(tr, "ema"), before["ema"]) and not tr._in_ema_scope


@pytest.mark.parametrize("adam8", [False, True])
def test_save_and_resume_bit_for_bit(tmp_path, adam8):
    kw = dict(use_ema=True, ema_decay=0.9, use_8bit_adam=adam8)
    tr = _trainer(R.train_ops(), **kw)
    for i in range(2):
        _micro(tr, i)
    path = tr.save_state(str(tmp_path / "s"), global_step=2)
    st = torch.load(os.path.join(path, "ema.bin"))
    assert st["format"] == "seer-ema-fp32-v1" and st["decay"] == 0.9 and st["warmup"] is True and st["num_updates"] == 2
    assert torch.equal(st["unet"], tr.pu.ema) and torch.equal(st["fstext"], tr.pf.ema) and st["unet"].dtype == torch.float32

    def resumed(**kw2):
        from seervideoldm_amd.io import load_seer_checkpoint
        unet, fst = _models()
        with torch.no_grad():
            for m in (unet, fst):
                for p in m.parameters():
                    p.add_(1.0)                                       # whatever the fresh objects held must not survive
        load_seer_checkpoint(path, unet, fst)
        fst.set_numframe(FR)
        new = _trainer(R.train_ops(), models=(unet, fst), **kw2)
        new.reload_from_modules()
        return new
    tr2 = resumed(**kw)
    for P in (tr2.pu, tr2.pf):
        P.ema.fill_(3.0)
    junk = _flat(tr2, "ema")
    tr2.reload_from_modules()
    assert torch.equal(_flat(tr2, "ema"), junk)                       # reload_from_modules leaves the average alone
    tr2.load_optimizer_state(path)
    assert tr2.ema_num_updates == 2 and torch.equal(_flat(tr2, "ema"), _flat(tr, "ema"))
    for i in (2, 3):
        la, _ = _micro(tr, i)
        lb, _ = _micro(tr2, i)
        assert torch.equal(la, lb)
    assert tr2.ema_num_updates == tr.ema_num_updates == 4 and tr2.step_count == 4
    assert torch.equal(_flat(tr2, "p"), _flat(tr, "p")) and _same(_state(tr2), _state(tr))
    assert np.array_equal(R.bits(_flat(tr2, "ema")), R.bits(_flat(tr, "ema")))
    # a trainer without the average ignores the file
    plain = resumed(use_8bit_adam=adam8)
    plain.load_optimizer_state(path)
    assert plain.pu.ema is None and plain.ema_num_updates == 0
    # wrong format, wrong length
    good = torch.load(os.path.join(path, "ema.bin"))
    tr3 = resumed(**kw)
    for bad, what in (({**good, "format": "seer-ema-fp16-v0"}, "format"), ({k: v for k, v in good.items() if k != "format"}, "format"),
                      ({**good, "unet": good["unet"][:-8]}, "elements"), ({**good, "fstext": torch.cat([good["fstext"], torch.zeros(8)])}, "elements")):
        torch.save(bad, os.path.join(path, "ema.bin"))
        keep = _flat(tr3, "ema")
        with pytest.raises(ValueError, match=what):
            tr3.load_optimizer_state(path)
        assert torch.equal(_flat(tr3, "ema"), keep)
    # the file is missing: a warning, and the average restarts from the loaded parameters
    os.remove(os.path.join(path, "ema.bin"))
    tr3.ema_num_updates = 7
    with pytest.warns(UserWarning, match="ema.bin"):
        tr3.load_optimizer_state(path)
    assert tr3.ema_num_updates == 0 and torch.equal(_flat(tr3, "ema"), _flat(tr3, "p")) and tr3.step_count == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)
        plain.load_optimizer_state(path)                              # no average, no file: nothing to say


def test_save_ema_weights_writes_the_averaged_model(stepped, tmp_path):
    tr = stepped
    tr.sync_modules()
    before = dict(p=_flat(tr, "p"), ema=_flat(tr, "ema"), mods=_module_bits(tr))
    path = tr.save_ema_weights(str(tmp_path / "ema_model"))
    assert sorted(os.listdir(path)) == ["pytorch_model.bin", "pytorch_model_1.bin"]
    avg = tr.ema_state_dict()
    for s, fn in (("unet", "pytorch_model.bin"), ("fstext", "pytorch_model_1.bin")):
        sd = torch.load(os.path.join(path, fn))
        assert set(sd) == set(before["mods"][s])
        for k, v in sd.items():
            want = avg[s][k].reshape(v.shape) if k in avg[s] else before["mods"][s][k]
            assert torch.equal(v, want), k
        assert any(not torch.equal(sd[k], before["mods"][s][k]) for k in avg[s])
    assert torch.equal(_flat(tr, "p"), before["p"]) and torch.equal(_flat(tr, "ema"), before["ema"])
    after = _module_bits(tr)
    assert all(torch.equal(after[s][k], before["mods"][s][k]) for s in after for k in after[s])


def test_reset_ema(stepped):
    tr = stepped
    keep, n = _flat(tr, "ema"), tr.ema_num_updates
    assert n == 2 and not torch.equal(keep, _flat(tr, "p"))
    tr.reset_ema()
    assert tr.ema_num_updates == 0 and torch.equal(_flat(tr, "ema"), _flat(tr, "p")) and tr.pu.ema.data_ptr() != tr.pu.p.data_ptr()
    for P, part in ((tr.pu, keep[:tr.pu.n]), (tr.pf, keep[tr.pu.n:])):          # put it back for the other tests
        P.ema.copy_(part)
    tr.ema_num_updates = n


def test_constructor_refusals_and_a_trainer_without_the_average():
    models = _models()
    for adam8, need in ((False, "adamw_ema_step"), (True, "adamw8_ema_step")):
        with pytest.raises(ValueError, match=need):
            _trainer(R.train_ops(with_ema=False), models=models, use_ema=True, use_8bit_adam=adam8)
        assert _trainer(R.train_ops(with_ema=False), models=models, use_8bit_adam=adam8).use_ema is False
    for bad in (-0.5, 1.5, math.nan, math.inf):
        with pytest.raises(ValueError, match="ema_decay"):
            _trainer(R.train_ops(), models=models, use_ema=True, ema_decay=bad)
    plain = _trainer(R.train_ops(), models=models)
    for call in (plain.ema_state_dict, plain.reset_ema, lambda: plain.ema_scope().__enter__(), lambda: plain.save_ema_weights("/nonexistent")):
        with pytest.raises(RuntimeError, match="use_ema"):
            call()


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_surface():
    from seervideoldm_amd import _lib, train_ops
    assert _lib.ABI_VERSION == 27                        # two declarations: no struct changed
    for name, plain in (("seer_adamw_ema_step", "seer_adamw_step"), ("seer_adamw8_ema_step", "seer_adamw8_step")):
        a, r = _lib.SIGNATURES[name]
        assert a == _lib.SIGNATURES[plain][0] + [_lib.C.c_void_p, _lib.C.c_float] and r is _lib.C.c_int
    for ours, theirs in ((R.adamw_ema_step, train_ops.adamw_ema_step), (R.adamw8_ema_step, train_ops.adamw8_ema_step)):
        a, b = inspect.signature(ours).parameters, inspect.signature(theirs).parameters
        assert list(a) == list(b) and all(a[k].kind == b[k].kind and a[k].default == b[k].default for k in a)
    init = inspect.signature(SeerTrainer.__init__).parameters
    assert (init["use_ema"].default, init["ema_decay"].default, init["ema_warmup"].default) == (False, 0.9999, True)
    assert all(init[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("use_ema", "ema_decay", "ema_warmup"))
    header = (ROOT / "include" / "seer_hip.h").read_text()
    assert "int seer_adamw_ema_step(" in header and "int seer_adamw8_ema_step(" in header


@pytest.mark.parametrize("adam8", [False, True])
def test_entry_points_refuse_bad_arguments_before_any_launch(adam8):
    """every refusal returns SEER_EINVAL on the host (the pointers are aligned non-NULL integers that are no memory; the one call that
    would pass its checks is not made here)"""
    from seervideoldm_amd import _lib
    from seervideoldm_amd.build import build_library
    build_library()
    lib = _lib.load()
    fn = lib.seer_adamw8_ema_step if adam8 else lib.seer_adamw_ema_step
    n = 0
    for args, why in R.refusal_cases(adam8, 1 << 30):
        if why is not None:
            assert fn(*args) == -22, why
            n += 1
    assert n >= 30


# ---- two ranks ----------------------------------------------------------------------------------------------------------------------------
def _ema_worker(rank, world, port, out_path):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tr = _trainer(R.train_ops(), use_ema=True, ema_decay=0.9, process_group=dist.group.WORLD)
        start = _flat(tr, "ema")
        losses = []
        for s in range(2):
            loss, stepped = _micro(tr, 10 * rank + s)              # every rank its own micro-batches
            assert stepped
            losses.append(loss)
        torch.save(dict(ema=_flat(tr, "ema"), p=_flat(tr, "p"), start=start, n=tr.ema_num_updates, losses=losses), f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_the_same_average(tmp_path):
    out = tmp_path / "ema"
    _spawn(_ema_worker, 2, str(out))
    r0, r1 = torch.load(f"{out}.0"), torch.load(f"{out}.1")
    assert r0["n"] == r1["n"] == 2 and not torch.equal(r0["losses"][0], r1["losses"][0])
    assert np.array_equal(R.bits(r0["ema"]), R.bits(r1["ema"])) and torch.equal(r0["p"], r1["p"])
    assert not torch.equal(r0["ema"], r0["start"]) and not torch.equal(r0["ema"], r0["p"])
