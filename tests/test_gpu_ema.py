"""seer_adamw_ema_step / seer_adamw8_ema_step on a real MI355X: the average is a passenger of the step (every other output has the
plain entry point's bits) and its own bits are LitEma's three separately rounded fp32 operations -- against torch's three operations
on the kernel's own new parameters, and against the shadows the reference's LitEma recorded (tests/golden/ema_litema.npz), which a
contracted multiply-add misses --, the refusals, and SeerTrainer(use_ema=True) on the HIP kernels in both optimizer modes."""
import functools
import os

import numpy as np
import pytest
import torch

from seervideoldm_amd import FSTextTransformer, SeerUNet, _lib, train_ops
from seervideoldm_amd.trainer import SeerTrainer, ema_one_minus_decay
from tests import adam8_ref as A8
from tests import ema_ref as R
from tests.test_gpu_adam8 import GUARD, HP, _guarded, _sentinels_intact, _tiny

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
OMDS = (0.0, 1.0, float(np.float32(1.0) - np.float32(0.9999)), float(np.float32(0.3)))
# fp32: one element; off any multiple of 256; past the 4096-block cap (the grid-stride loop makes more than one trip, ragged tail)
N_FP32 = (1, 1000, 4096 * 2048 + 2048 + 3)
# 8-bit: one block; a partial workgroup of waves (5 blocks); past the 2048-block cap
N_8BIT = (256, 1280, 2048 * 4 * 256 + 768)
LATE = 1000


def _eq(a, b):
    """same bits (the float types compared as integers: a NaN or a signed zero cannot hide)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {f32: torch.int32, bf16: torch.int16}.get(a.dtype)
    return bool(torch.equal(a.view(view), b.view(view))) if view is not None else bool(torch.equal(a, b))


@functools.lru_cache(maxsize=2)
def _inputs(n, adam8, warm):
    """CPU inputs of one (n, mode, state): p, g, the optimizer state, the average before the step"""
    gen = torch.Generator().manual_seed(7 + n % 1009 + 2 * warm + adam8)
    if adam8:
        p, g, cm, cv, am, av = A8.random_state(n, 11 + n % 997)
        if not warm:
            cm, cv, am, av = torch.full((n,), 127, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8), torch.zeros(n // 256), torch.zeros(n // 256)
        state = (cm, cv, am, av)
    else:
        p, g = torch.randn((n,), generator=gen), torch.randn((n,), generator=gen) * 0.1
        m = torch.randn((n,), generator=gen) * 0.05 if warm else torch.zeros(n)
        v = torch.rand((n,), generator=gen) * 0.01 if warm else torch.zeros(n)
        state = (m, v)
    ema = p + 0.01 * torch.randn((n,), generator=gen)          # an average lags the parameters by a little
    ema[::7] = p[::7]                                           # ... and some elements sit exactly on them
    return p, g, state, ema


def _launch(device, adam8, inp, kw, with_bf16, omd=None):
    """one launch on device clones; omd=None: the plain entry point.  -> (p, state..., pb or None, guarded ema buffer, ema view)"""
    p0, g, state, ema0 = inp
    p, g = p0.to(device), g.to(device)
    st = [t.to(device) for t in state]
    pb = torch.zeros(p.numel(), dtype=bf16, device=device) if with_bf16 else None
    full = view = None
    if omd is None:
        (train_ops.adamw8_step if adam8 else train_ops.adamw_step)(p, g, *st, p_bf16=pb, **kw)
    else:
        full, view = _guarded(ema0, device)
        (train_ops.adamw8_ema_step if adam8 else train_ops.adamw_ema_step)(p, g, *st, view, one_minus_decay=omd, p_bf16=pb, **kw)
    return [p, *st, pb], full, view


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("with_bf16", [True, False])
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("adam8,n", [(False, n) for n in N_FP32] + [(True, n) for n in N_8BIT])
def test_the_average_is_a_passenger_and_has_the_three_operations_bits(device, adam8, n, warm, with_bf16, clipped):
    """step 1 on a fresh state / step 1000 on a warm one; for every one_minus_decay of (0, 1, fl32(1 - 0.9999), 0.3):
    1. p, the optimizer state and p_bf16 after the _ema entry point are bit for bit the plain entry point's on clones of the inputs;
    2. ema' is bit for bit ema0 - omd * (ema0 - p'), three torch operations on the kernel's own p';
    3. the NaN guards on both sides of ema are intact."""
    inp = _inputs(n, adam8, warm)
    kw = dict(step=LATE if warm else 1, **HP)
    if clipped:
        kw.update(grad_sumsq=(inp[1].double() ** 2).sum().float().reshape(1).to(device), max_norm=0.3)
    plain, _, _ = _launch(device, adam8, inp, kw, with_bf16)
    assert not _eq(plain[0], inp[0].to(device))                                 # the step did move p
    ema0 = inp[3].to(device)
    for omd in OMDS:
        outs, full, ema = _launch(device, adam8, inp, kw, with_bf16, omd)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(outs, plain)):
            assert (a is None and b is None) or _eq(a, b), (omd, i)
        want = ema0 - torch.tensor(omd, dtype=f32) * (ema0 - outs[0])
        assert _eq(ema, want), (omd, int((ema.view(torch.int32) != want.view(torch.int32)).sum()))
        if omd == 0.0:
            assert _eq(ema, ema0)                                                # bits untouched
        assert _sentinels_intact(full), omd


def test_three_operations_cross_checked_on_cpu_tensors(device):
    """the same expression evaluated by torch on the CPU from the kernel's p' (the device's three elementwise kernels are not the
    yardstick of themselves)"""
    for adam8, n in ((False, 1000), (True, 1280)):
        inp = _inputs(n, adam8, True)
        kw = dict(step=LATE, **HP)
        for omd in OMDS:
            outs, _, ema = _launch(device, adam8, inp, kw, True, omd)
            torch.cuda.synchronize()
            want = R.ema3_(inp[3].clone(), outs[0].cpu(), omd)
            assert _eq(ema.cpu(), want), (adam8, omd)
            assert np.array_equal(R.bits(ema), R.bits(R.recurrence(inp[3].numpy(), [outs[0].cpu().numpy()], [omd])[0]))


@pytest.mark.parametrize("adam8", [False, True])
def test_litema_replay(device, adam8):
    """lr = 0, weight_decay = 0, g = 0: the step leaves p as it is.  Every recorded parameter snapshot of the reference's LitEma runs
    is loaded into p and stepped; ema equals the recorded shadow after EVERY update of all three runs, bit for bit (1001 elements; for
    the 8-bit entry point padded with zeros to 1024).  A multiply-add contracted from the product and the second difference rounds
    once where LitEma rounds twice, and misses these bits."""
    fx = R.fixture()
    for r in R.RUNS:
        run = fx[r]
        U, n0 = run["p"].shape
        n = (n0 + 255) // 256 * 256 if adam8 else n0
        pad = lambda a: torch.cat([torch.from_numpy(a), torch.zeros(n - n0)]).to(device)
        p, g, ema = pad(run["p0"]), torch.zeros(n, device=device), pad(run["p0"])
        snaps = torch.cat([torch.from_numpy(run["p"]), torch.zeros((U, n - n0))], 1).to(device)
        if adam8:
            st = [torch.full((n,), 127, dtype=torch.uint8, device=device), torch.zeros(n, dtype=torch.uint8, device=device),
                  torch.zeros(n // 256, device=device), torch.zeros(n // 256, device=device)]
            fn = train_ops.adamw8_ema_step
        else:
            st = [torch.zeros(n, device=device), torch.zeros(n, device=device)]
            fn = train_ops.adamw_ema_step
        got = torch.empty((U, n), device=device)
        for u in range(U):
            p.copy_(snaps[u])
            omd = ema_one_minus_decay(run["decay"], u + 1, run["warmup"])
            fn(p, g, *st, ema, one_minus_decay=omd, lr=0.0, weight_decay=0.0, step=u + 1, betas=HP["betas"], eps=HP["eps"])
            assert _eq(p, snaps[u]), (r, u)
            got[u].copy_(ema)
        got = got.cpu().numpy()
        bad = (R.bits(got[:, :n0]) != R.bits(run["shadow"])).sum(1)
        print(f"[ema replay] {'8-bit' if adam8 else 'fp32'} {r}: {U} updates, elements off per update max {int(bad.max())}")
        assert not bad.any(), (r, np.nonzero(bad)[0][:5])
        assert not got[:, n0:].any()


@pytest.mark.parametrize("adam8", [False, True])
def test_refusals_return_einval_and_leave_a_nan_filled_average_alone(device, adam8):
    buf = torch.ones(16384, device=device)
    buf[4096:4608] = float("nan")                                        # the average of the good call
    buf[8192] = 4.0
    qm, qv = train_ops.adam8_qmaps(device)
    buf[7168:7424], buf[7680:7936] = qm, qv
    if adam8:
        buf[2048:2176].view(torch.uint8).fill_(127)
        buf[3072:3200].view(torch.uint8).zero_()
        buf[6144:6146], buf[6208:6210] = 0.0, 0.0
    before = buf.clone()
    lib = _lib.load()
    fn = lib.seer_adamw8_ema_step if adam8 else lib.seer_adamw_ema_step
    st = torch.cuda.current_stream().cuda_stream
    good, n = None, 0
    for args, why in R.refusal_cases(adam8, buf.data_ptr()):
        args = tuple(st if i == len(args) - 3 else a for i, a in enumerate(args))     # the stream sits before (ema, one_minus_decay)
        if why is None:
            good = args
        else:
            assert fn(*args) == -22, why
            n += 1
    torch.cuda.synchronize()
    assert n >= 30 and _eq(buf, before)                                   # nothing was launched: every float has its former bits
    assert fn(*good) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[4096:4608]).all()) and not bool((buf[:512] == 1).any())     # a NaN average stays NaN; p moved
    assert _eq(buf[4608:5120], before[4608:5120]) and _eq(buf[512:1024], before[512:1024])


# ------------------------------------------------------------------------------------------------------------- the trainer
def _flat(tr, what):
    return torch.cat([getattr(tr.pu, what).reshape(-1), getattr(tr.pf, what).reshape(-1)]).clone()


def _same_trainers(a, b):
    return (_eq(_flat(a, "p"), _flat(b, "p")) and _eq(_flat(a, "pb"), _flat(b, "pb")) and _eq(_flat(a, "ema"), _flat(b, "ema"))
            and all(_eq(x, y) for P, Q in ((a.pu, b.pu), (a.pf, b.pf)) for x, y in zip(P.state().values(), Q.state().values()))
            and a.ema_num_updates == b.ema_num_updates and a.step_count == b.step_count)


@pytest.mark.parametrize("adam8", [False, True])
def test_tiny_trainer_with_the_average(device, tmp_path, adam8):
    """tests/test_gpu_adam8.py's tiny configuration, 3 steps with use_ema=True: the average is the host recurrence over the parameter
    snapshots; save after step 2 and resume give step 3 bit for bit; inside ema_scope the module's UNet forward is that of a fresh
    SeerUNet loaded from save_ema_weights' files; and a step after the scope has the bits of a trainer that never entered one"""
    from seervideoldm_amd.io import load_seer_checkpoint
    x, noise, t, text = [a.to(device) for a in A8.tiny_batch(16)]
    kw = dict(use_ema=True, ema_decay=0.9, use_8bit_adam=adam8, **A8.TINY_HP)

    def step(tr):
        tr.forward_backward(x, noise, t, text, 1)
        tr.optimizer_step()

    tr, twin = SeerTrainer(*_tiny(device), **kw), SeerTrainer(*_tiny(device), **kw)
    ema0, snaps = _flat(tr, "ema").cpu().numpy(), []
    path = None
    for s in range(3):
        step(tr)
        step(twin)
        snaps.append(_flat(tr, "p").cpu().numpy())
        if s == 1:
            path = tr.save_state(str(tmp_path / "state"), global_step=2)
    want = R.recurrence(ema0, snaps, [R.omd32(0.9, n, True) for n in (1, 2, 3)])[-1]
    assert np.array_equal(R.bits(_flat(tr, "ema")), R.bits(want)) and tr.ema_num_updates == 3
    assert not np.array_equal(want, snaps[-1]) and _same_trainers(tr, twin)
    assert tr.ema_state_bytes() == 4 * (tr.pu.n + tr.pf.n)
    # resume from the files of step 2
    u2 = SeerUNet(**A8.TINY_CFG)
    f2 = FSTextTransformer(num_frames=16, in_channels=192, out_channels=192, n_heads=2, num_layers=1, cross_attention_dim=192)
    load_seer_checkpoint(path, u2, f2)
    f2.set_numframe(3)
    tr2 = SeerTrainer(u2.to(device), f2.to(device), **kw)
    tr2.load_optimizer_state(path)
    assert tr2.ema_num_updates == 2 and not _eq(_flat(tr2, "ema"), _flat(tr2, "p"))
    step(tr2)
    assert _same_trainers(tr2, tr)
    # the averaged model: the same module objects inside the scope, and a fresh module from the files
    epath = tr.save_ema_weights(str(tmp_path / "ema_model"))
    assert sorted(os.listdir(epath)) == ["pytorch_model.bin", "pytorch_model_1.bin"]
    g = torch.Generator().manual_seed(5)
    xs, ctx = torch.randn((1, 4, 3, 16, 16), generator=g).to(device), torch.randn((1, 3, 77, 192), generator=g).to(device)
    ts = torch.tensor([501], device=device)
    with torch.no_grad():
        raw = tr.unet(xs, ts, ctx, cond_frame=1).clone()
        with tr.ema_scope():
            inside = tr.unet(xs, ts, ctx, cond_frame=1).clone()
        u3 = SeerUNet(**A8.TINY_CFG)
        load_seer_checkpoint(epath, u3, None)
        fresh = u3.to(device)(xs, ts, ctx, cond_frame=1)
        again = tr.unet(xs, ts, ctx, cond_frame=1)
    assert _eq(inside, fresh) and _eq(again, raw) and not _eq(inside, raw) and bool(torch.isfinite(inside).all())
    assert _same_trainers(tr, twin)                                         # the scopes left every bit where it was
    step(tr)
    step(twin)
    assert _same_trainers(tr, twin) and tr.ema_num_updates == 4
