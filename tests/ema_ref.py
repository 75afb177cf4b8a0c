"""The exponential moving average of the trained weights restated (include/seer_hip.h: seer_adamw_ema_step, seer_adamw8_ema_step):
LitEma's update as the three torch operations it is, the schedule of `one_minus_decay` in numpy float32, the host recurrence over
parameter snapshots, plain-torch stand-ins with the signatures of train_ops.adamw_ema_step / adamw8_ema_step -- the plain stand-in
step followed by the three operations -- behind a `tops=` backend that records its calls, and the fixture of the reference's own
LitEma (tests/golden/ema_litema.npz, written by tests/make_ema_golden.py).  Nothing here comes from a kernel.

  * ema3_(ema, p, omd): ema.sub_(omd * (ema - p)), omd an fp32 scalar -- ldm/modules/ema.py:42;
  * omd32(decay, n, warmup): numpy float32: 1 - min(decay, (1 + n) / (10 + n)), or 1 - decay;
  * recurrence(ema0, snapshots, omds): the average after every update, in numpy float32 (each operation rounded on its own);
  * adamw_ema_step / adamw8_ema_step: tests/torch_train_ops_backend.adamw_step / tests/adam8_ref.adamw8_step, then ema3_;
  * train_ops(): tests/minsnr_ref.train_ops() + the 8-bit entry points of tests/adam8_ref.py + the two stand-ins; `ema_calls` lists
    (name, one_minus_decay) of every _ema call, `plain_calls` the names of the plain AdamW calls."""
from pathlib import Path

import numpy as np
import torch

from tests import adam8_ref as A8
from tests import minsnr_ref as M
from tests import torch_train_ops_backend as _ttob

f32 = torch.float32
GOLDEN = Path(__file__).parent / "golden" / "ema_litema.npz"
RUNS = ("d0.9", "d0.9999", "nowarm")


def ema3_(ema, p, omd):
    """in place; three separately rounded fp32 operations, on any device"""
    assert ema.dtype == f32 and p.dtype == f32
    ema.sub_(torch.tensor(omd, dtype=f32) * (ema - p))
    return ema


def omd32(decay, n, warmup):
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + n) / np.float32(10 + n))
    return np.float32(1.0) - d


def bits(x):
    """the int32 bit patterns of an fp32 array / tensor / Python float (NaNs and signed zeros compare as bits)"""
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32)


def recurrence(ema0, snapshots, omds):
    """[U, n] numpy float32: the average after each of the U updates from ema0 over the parameter snapshots"""
    e = np.asarray(ema0, dtype=np.float32).copy()
    out = []
    for p, o in zip(snapshots, omds):
        d = e - np.asarray(p, dtype=np.float32)
        s = np.float32(o) * d
        e = e - s
        out.append(e)
    return np.stack(out)


def fixture():
    """{run: dict(p0 fp32 [n], p fp32 [U, n], shadow fp32 [U, n], omd fp32 [U], decay, warmup)} of the reference's LitEma"""
    z = np.load(GOLDEN)
    assert z["sizes"].tolist() == [1, 1000]
    return {r: dict(p0=z[r + "_p0"].astype(np.float32), p=z[r + "_p"].astype(np.float32), shadow=z[r + "_shadow"], omd=z[r + "_omd"],
                    decay=float(z[r + "_decay"]), warmup=bool(z[r + "_warmup"])) for r in RUNS}


def adamw_ema_step(p, g, m, v, ema, *, one_minus_decay, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, step, grad_sumsq=None,
                   max_norm=1.0, p_bf16=None):
    _ttob.adamw_step(p, g, m, v, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, step=step, grad_sumsq=grad_sumsq,
                     max_norm=max_norm, p_bf16=p_bf16)
    ema3_(ema, p, one_minus_decay)


def adamw8_ema_step(p, g, cm, cv, absmax_m, absmax_v, ema, *, one_minus_decay, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                    step, grad_sumsq=None, max_norm=1.0, p_bf16=None):
    A8.adamw8_step(p, g, cm, cv, absmax_m, absmax_v, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, step=step,
                   grad_sumsq=grad_sumsq, max_norm=max_norm, p_bf16=p_bf16)
    ema3_(ema, p, one_minus_decay)


def train_ops(with_ema=True):
    """a `tops=` backend for both optimizer modes; with_ema=False: the same backend WITHOUT the two _ema functions"""
    base = M.train_ops()

    class Plain(type(base)):
        def __init__(self):
            super().__init__()
            self.ema_calls, self.plain_calls = [], []

        def adam8_qmaps(self, device):
            return A8.QMAP_M.to(device), A8.QMAP_V.to(device)

        def adamw_step(self, *a, **kw):
            self.plain_calls.append("adamw_step")
            return _ttob.adamw_step(*a, **kw)

        def adamw8_step(self, *a, **kw):
            self.plain_calls.append("adamw8_step")
            return A8.adamw8_step(*a, **kw)

    class WithEma(Plain):
        def adamw_ema_step(self, *a, **kw):
            self.ema_calls.append(("adamw_ema_step", kw["one_minus_decay"]))
            return adamw_ema_step(*a, **kw)

        def adamw8_ema_step(self, *a, **kw):
            self.ema_calls.append(("adamw8_ema_step", kw["one_minus_decay"]))
            return adamw8_ema_step(*a, **kw)
    return WithEma() if with_ema else Plain()


def refusal_cases(adam8, P):
    """(arguments of seer_adamw_ema_step / seer_adamw8_ema_step, what is wrong) for every refusal the header adds to the plain entry
    point's, and a few of the plain ones.  P: the address of a 16-byte aligned buffer of at least 16384 floats; n = 512; the good call
    keeps its arrays apart: p at 0, g at 1024, m / cm at 2048, v / cv at 3072, ema at 4096, p_bf16 at 5120, absmax_m at 6144, absmax_v
    at 6208, the code books at 7168 and 7680, grad_sumsq at 8192."""
    f = lambda i: P + 4 * i
    n = 512
    nan, inf = float("nan"), float("inf")
    if adam8:
        good = dict(p=f(0), g=f(1024), cm=f(2048), cv=f(3072), am=f(6144), av=f(6208), qm=f(7168), qv=f(7680), n=n, lr=1e-3, b1=0.9,
                    b2=0.999, eps=1e-8, wd=1e-2, step=1, ss=f(8192), max_norm=1.0, pb=f(5120), stream=None, ema=f(4096), omd=0.25)
        plain = [dict(p=None), dict(g=None), dict(cm=None), dict(cv=None), dict(am=None), dict(av=None), dict(qm=None), dict(qv=None),
                 dict(n=0), dict(n=300), dict(step=0), dict(p=f(0) + 4), dict(g=f(1024) + 8), dict(cm=f(2048) + 1), dict(pb=f(5120) + 2)]
        align = [dict(ema=f(4096) + 4), dict(ema=f(4096) + 8), dict(ema=f(4096) + 2)]
        over = [dict(ema=f(0)), dict(ema=f(256)), dict(ema=f(1024 - 256)), dict(ema=f(1024)), dict(ema=f(2048)),
                dict(ema=f(2048 + 124)),                                     # the last 16 bytes of the 512 codes of cm
                dict(ema=f(3072 - 512 + 4)), dict(ema=f(3072)), dict(ema=f(5120)), dict(ema=f(5120 + 252)),
                dict(ema=f(6144)), dict(ema=f(6144 - 508)),                   # the average's last floats on absmax_m [2]
                dict(ema=f(6208)), dict(ema=f(8192)), dict(ema=f(8192 - 508))]
    else:
        good = dict(p=f(0), g=f(1024), m=f(2048), v=f(3072), n=n, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=1, ss=f(8192),
                    max_norm=1.0, pb=f(5120), stream=None, ema=f(4096), omd=0.25)
        plain = [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-4), dict(step=0), dict(step=-2)]
        align = [dict(ema=f(4096) + 1), dict(ema=f(4096) + 2), dict(ema=f(4096) + 3)]
        over = [dict(ema=f(0)), dict(ema=f(511)), dict(ema=f(1024 - 511)), dict(ema=f(1024)), dict(ema=f(2048)), dict(ema=f(2048 + 100)),
                dict(ema=f(3072)), dict(ema=f(3072 + 511)), dict(ema=f(5120)), dict(ema=f(5120 + 255)), dict(ema=f(5120 - 511)),
                dict(ema=f(8192)), dict(ema=f(8192 - 511))]
    ema = [dict(ema=None), dict(omd=-1e-6), dict(omd=1.0000001), dict(omd=-1.0), dict(omd=2.0), dict(omd=nan), dict(omd=inf), dict(omd=-inf)]
    for kw in plain + ema + align + over:
        yield tuple({**good, **kw}.values()), kw
    yield tuple(good.values()), None                       # the good call itself: the caller decides whether it may launch
