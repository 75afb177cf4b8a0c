"""v-prediction restated: the three forms of the conversion kernel (include/seer_hip.h: seer_v_to_eps, seer_v_to_eps_dev,
seer_slot_v_to_eps) and seer_velocity_target, in float64 from the definition and as fp32 torch stand-ins with the signatures of
seervideoldm_amd.ops / train_ops (the kernel's expression order: equal to the kernel to rounding, not to the bit).  Nothing here comes
from a kernel.

  * eps_from_v64 / v_from_eps64 / velocity64: the definitions, v = sqrt(a) eps - sqrt(1 - a) x0 and eps = sqrt(a) v + sqrt(1 - a) x_t;
  * v_to_eps / v_to_eps_dev / slot_v_to_eps / velocity_target: the stand-ins; cfg_plms_step: the stand-in of ops.cfg_plms_step that
    the other restatements lack (PLMSSampler on the CPU);
  * backend(*modules): this module's stand-ins in front of those of the existing tests/*_ref.py modules, as an `ops=` backend --
    `DDIMSampler("cpu", ops=backend(dpm_ref), prediction_type="v_prediction")`, `SlotSampler(..., ops=backend(slot_plms_ref))`;
    TrainOps: tests/train_inputs_ref.TrainOpsWithInputs (over tests/torch_train_ops_backend.py) plus velocity_target, a `tops=` backend;
  * chain64: DDIM (any eta), PLMS and DPM-Solver++ chains in float64 over a model that predicts eps or v, with the magnitudes a
    rounding-error allowance is made of and a unit bump of any intermediate, for its sensitivity (tests/test_vpred_host.py)."""
import math

import torch

f64 = torch.float64
U = 2.0 ** -24                                           # half an ulp of 1.0f: the relative rounding error of one fp32 operation
STAND_INS = ("v_to_eps", "v_to_eps_dev", "slot_v_to_eps", "cfg_plms_step")


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def eps_from_v64(v, x, a_t, s1m):
    return math.sqrt(float(a_t)) * v.to(f64) + float(s1m) * x.to(f64)


def v_from_eps64(eps, x, a):
    """the v of a model whose eps at the latent x of level a is `eps`: x0 = (x - sqrt(1 - a) eps) / sqrt(a) put into the definition"""
    a = float(a)
    return (eps.to(f64) - math.sqrt(1.0 - a) * x.to(f64)) / math.sqrt(a)


def velocity64(latents, noise, timesteps, alphas_cumprod):
    """-> (target, magnitude sqrt(a) |noise| + sqrt(1 - a) |latents|) in float64, a the fp32 table entry"""
    T = alphas_cumprod.numel()
    a = alphas_cumprod.double().cpu()[timesteps.cpu().long().clamp(0, T - 1)].view(-1, *([1] * (noise.dim() - 1)))
    sa, sb = a.sqrt(), (1.0 - a).sqrt()
    n, l = noise.double().cpu(), latents.double().cpu()
    return sa * n - sb * l, sa * n.abs() + sb * l.abs()


# ---- the stand-ins --------------------------------------------------------------------------------------------------------------------
def _new_out(v, out):
    """ops.v_to_eps returns a fresh tensor whose conditioning frames hold nothing defined: here they hold NaN, so a reader shows"""
    if out is None:
        out = torch.full_like(v, float("nan"))
    assert out.shape == v.shape and out.dtype == torch.float32
    return out


def _convert(v, x, row, cond_f, out):
    out[:, :, cond_f:] = torch.sqrt(row[0]) * v[:, :, cond_f:] + row[3] * x


def v_to_eps(v, x, coef, index, *, cond_f, out=None):
    if not 0 <= int(index) < coef.shape[0]:
        raise ValueError(f"index {index}: the table has {coef.shape[0]} rows")
    b = x.shape[0]
    assert v.shape[0] in (b, 2 * b) and v.shape[2] == x.shape[2] + cond_f and tuple(coef.shape[1:]) == (4,)
    out = _new_out(v, out)
    for r in range(v.shape[0] // b):
        _convert(v[r * b:(r + 1) * b], x, coef[int(index)], cond_f, out[r * b:(r + 1) * b])
    return out


def v_to_eps_dev(v, x, coef, step, *, cond_f, out=None):
    out = _new_out(v, out)
    index = int(step[1])
    if 0 <= index < coef.shape[0]:
        v_to_eps(v, x, coef, index, cond_f=cond_f, out=out)
    return out


def slot_v_to_eps(v, x, coef, step, *, cond_f, state=None, x_prov=None, out=None):
    slots, nsched = x.shape[0], coef.shape[1]
    assert v.shape[0] == 2 * slots and tuple(coef.shape[::2]) == (slots, 4) and tuple(step.shape) == (slots, 2)
    if (state is None) != (x_prov is None):
        raise ValueError("state and x_prov go together")
    out = _new_out(v, out)
    for s in range(slots):
        index = int(step[s, 1])
        if index < 0 or index >= nsched:
            continue                                    # idle: the slot's rows are untouched
        lat = x[s]
        if state is not None and int(state[s, 4]) == 2:
            lat, index = x_prov[s], max(index - 1, 0)
        for r in (s, slots + s):
            _convert(v[r:r + 1], lat[None], coef[s, index], cond_f, out[r:r + 1])
    return out


def velocity_target(latents, noise, timesteps, alphas_cumprod, out=None):
    T = alphas_cumprod.numel()
    a = alphas_cumprod[timesteps.long().clamp(0, T - 1)].view(-1, *([1] * (noise.dim() - 1)))
    t = torch.sqrt(a) * noise - torch.sqrt(1.0 - a) * latents
    if out is None:
        return t
    out.copy_(t)
    return out


def cfg_plms_step(eps, x, coef, index, order, *, cfg, scale, cond_f, history=(), x_prev=None, pred_x0=None, e_out=None,
                  want_pred_x0=True, want_e=True):
    """ops.cfg_plms_step in fp32 torch: e' by order, then the eta = 0 DDIM update (csrc/sampler_step.hip, plms_update)"""
    order, history = int(order), list(history)
    need = (0, 1, 1, 2, 3)[order]
    assert 0 <= order <= 4 and need <= len(history) <= 3
    b = x.shape[0]
    e = eps[:, :, cond_f:]
    e = e[:b] + scale * (e[b:] - e[:b]) if cfg else e
    if order == 0:
        ep = e
    elif order == 1:
        ep = (history[0] + e) / 2.0
    elif order == 2:
        ep = (3.0 * e - history[0]) / 2.0
    elif order == 3:
        ep = (23.0 * e - 16.0 * history[0] + 5.0 * history[1]) / 12.0
    else:
        ep = (55.0 * e - 59.0 * history[0] + 37.0 * history[1] - 9.0 * history[2]) / 24.0
    a_t, a_prev, sigma, s1m = coef[int(index)]
    x0 = (x - s1m * ep) / torch.sqrt(a_t)
    new = torch.sqrt(a_prev) * x0 + torch.sqrt(1.0 - a_prev - sigma * sigma) * ep
    if x_prev is not None:
        x_prev.copy_(new)
        new = x_prev
    if pred_x0 is not None:
        pred_x0.copy_(x0)
        x0 = pred_x0
    if order == 1:
        kept = None
    elif e_out is not None:
        e_out.copy_(e)
        kept = e_out
    else:
        kept = e.clone() if want_e else None            # (e may be a view of eps)
    return new, (x0 if want_pred_x0 or pred_x0 is not None else None), kept


class _Backend:
    def __init__(self, modules):
        self._modules = modules

    def __getattr__(self, name):
        if name in STAND_INS:
            return globals()[name]
        for m in self._modules:
            if hasattr(m, name):
                return getattr(m, name)
        raise AttributeError(name)


def backend(*modules):
    """an `ops=` backend: this module's stand-ins, then every name of `modules` (tests/*_ref.py), first match first"""
    return _Backend(modules)


def train_ops():
    """a `tops=` backend: TrainOpsWithInputs (tests/torch_train_ops_backend.py + train_inputs) + velocity_target; `velocity_calls`
    lists the arguments of every velocity_target call"""
    from tests.train_inputs_ref import TrainOpsWithInputs

    class TrainOps(TrainOpsWithInputs):
        def __init__(self):
            super().__init__()
            self.velocity_calls = []

        def velocity_target(self, latents, noise, timesteps, alphas_cumprod, out=None):
            self.velocity_calls.append((latents, noise, timesteps, alphas_cumprod))
            return velocity_target(latents, noise, timesteps, alphas_cumprod, out)
    return TrainOps()


# ---- whole chains in float64 ----------------------------------------------------------------------------------------------------------
def chain64(method, coef, x_T, model_rows, prediction_type, scale, *, dpm_coef=None, orders=None, noise=None, bump=None):
    """A chain over the entries n - 1 ... 0 of the fp32 tables `coef` ([n, 4]; `dpm_coef` [n, 6] for method "dpm"), read as float64
    constants.  method: "ddim" (`noise`: None, or noise(index) -> the float64 noise of that step, already times the temperature),
    "plms", or "dpm" (`orders`: the order of every step, first to last).
    model_rows(x, row) -> the model's output rows (one, or the CFG pair (uc, c)) in float64 at the latent x and the timestep of entry
    `row`; with prediction_type "v_prediction" they are v and are converted with row `row` of coef, as the kernels do.
    bump = (what, k) adds 1.0 to: "e" the CFG-combined eps of evaluation k; "x" the latent after step k; "p" the provisional latent
    of PLMS' first step; "d" the data prediction DPM-Solver++ keeps after step k (after the step used it).
    -> (latent, marks): marks = [(what, k, magnitude)], the operand-magnitude sum of each of those quantities (see the allowance
    in tests/test_vpred_host.py)."""
    c = coef.double()
    n = c.shape[0]
    marks, ev = [], [0]
    hit = lambda what, k: 1.0 if bump == (what, k) else 0.0

    def evaluate(x, row):
        a_t, s1m = float(c[row, 0]), float(c[row, 3])
        outs = model_rows(x, row)
        if prediction_type == "v_prediction":
            mags = [math.sqrt(a_t) * o.abs() + s1m * x.abs() for o in outs]
            outs = [eps_from_v64(o, x, a_t, s1m) for o in outs]
        else:
            mags = [o.abs() for o in outs]
        if len(outs) == 2:
            e = outs[0] + scale * (outs[1] - outs[0])
            mag = mags[0] + (abs(scale) + 1.0) * (mags[0] + mags[1]) + mags[1]
        else:
            e, mag = outs[0], mags[0]
        k = ev[0]
        ev[0] += 1
        marks.append(("e", k, mag))
        return e + hit("e", k), mag

    def update(x, ep, ep_mag, row, nz=None):
        a_t, a_prev, sigma, s1m = (float(v) for v in c[row])
        x0 = (x - s1m * ep) / math.sqrt(a_t)
        dirc = math.sqrt(max(1.0 - a_prev - sigma * sigma, 0.0))
        new = math.sqrt(a_prev) * x0 + dirc * ep
        mag = math.sqrt(a_prev) * (x.abs() + s1m * ep_mag) / math.sqrt(a_t) + dirc * ep_mag
        if nz is not None:
            new, mag = new + sigma * nz, mag + sigma * nz.abs()
        return new, mag

    x = x_T.to(f64)
    if method == "ddim":
        for k, i in enumerate(reversed(range(n))):
            e, em = evaluate(x, i)
            x, mag = update(x, e, em, i, None if noise is None else noise(i))
            marks.append(("x", k, mag))
            x = x + hit("x", k)
        return x, marks
    if method == "plms":
        hist = []                                         # (e, magnitude), oldest first
        for k, i in enumerate(reversed(range(n))):
            e, em = evaluate(x, i)
            if not hist:
                prov, pm = update(x, e, em, i)
                marks.append(("p", 0, pm))
                e2, em2 = evaluate(prov + hit("p", 0), max(i - 1, 0))
                ep, epm = (e + e2) / 2.0, (em + em2) / 2.0
            else:
                w = {1: (3.0, -1.0), 2: (23.0, -16.0, 5.0), 3: (55.0, -59.0, 37.0, -9.0)}[len(hist)]
                terms = [(e, em)] + hist[::-1]
                ep = sum(wk * t[0] for wk, t in zip(w, terms)) / sum(w)
                epm = sum(abs(wk) * t[1] for wk, t in zip(w, terms)) / sum(w)
            x, mag = update(x, ep, epm, i)
            marks.append(("x", k, mag))
            x = x + hit("x", k)
            hist = (hist + [(e, em)])[-3:]
        return x, marks
    assert method == "dpm"
    t = dpm_coef.double()
    d_prev = None
    for k, i in enumerate(reversed(range(n))):
        e, em = evaluate(x, i)
        r = [float(v) for v in t[i]]
        d = (x - r[0] * e) * r[1]
        dm = (x.abs() + r[0] * em) * r[1]
        if orders[k] == 2:
            new, mag = r[2] * x + r[4] * d + r[5] * d_prev, abs(r[2]) * x.abs() + abs(r[4]) * dm + abs(r[5]) * d_prev.abs()
        else:
            new, mag = r[2] * x + r[3] * d, abs(r[2]) * x.abs() + abs(r[3]) * dm
        marks += [("x", k, mag), ("d", k, dm)]
        x, d_prev = new + hit("x", k), d + hit("d", k)
    return x, marks
