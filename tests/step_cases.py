"""The cases of tests/golden/step_parent.npz: every kernel of csrc/sampler_step.hip -- both ends of a sampler step and the given
latents -- on inputs made with seeded numpy, each case run through `ops` in every FORM that has to give the same bits (host index,
device counter, seeded fed the matching seer_philox_normal tensor, slot, x_prev aliasing x).

    shared, own = run(name, form, ops, device)

`shared` holds what every form of the case must agree on, `own` what belongs to that form alone (its counter and state words);
both map a name to int32 BIT PATTERNS, and every output buffer starts as NaN, so what a kernel did not write is there to compare.
oracle/make_goldens_step_parent.py records the fixture from the PARENT commit's library (`shared` from the case's first form);
tests/test_gpu_step_parent.py holds every form of the library under test to it.

Shapes: C = 3, F_pred = 3, cond_f = 2, HW = 20, so a clip has 180 elements; b = 2 is two blocks of 256 with a ragged tail, a block
straddling the clip boundary and the uc | c offset; 3 slots are 540 elements with a block straddling each slot boundary -- one slot
idle (counter -1), one with a counter >= nsched, one active.  The inputs hold zeros of both signs in x, eps and the history.  No
case runs a device-counter form without seeds at a negative index: the parent read coefficient row -1 there."""
import zlib

import numpy as np
import torch

C, FP, COND_F, H, W = 3, 3, 2, 4, 5
HW = H * W
PER_CLIP = C * FP * HW
NSCHED = 6
SEEDS = (1234, (7 << 32) | 5, (1 << 63) | 99)
SCALE = 7.5
TEMPERATURE = 0.7
NAN_BITS = np.int32(0x7fc00000)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def coef_table(eta: float, shift: float = 0.) -> np.ndarray:
    """fp32 [NSCHED][4] = (a_t, a_prev, sigma, sqrt(1 - a_t)), index 0 the least noisy; sigma is DDIM's for `eta`"""
    a = np.linspace(0.93 - shift, 0.12 + shift, NSCHED)
    a_prev = np.concatenate([[0.9991], a[:-1]])
    sigma = eta * np.sqrt((1 - a_prev) / (1 - a) * (1 - a / a_prev))
    return np.stack([a, a_prev, sigma, np.sqrt(1 - a)], 1).astype(np.float32)


T_TABLE = np.array([1, 181, 361, 541, 721, (1 << 33) + 901], dtype=np.int64)        # the last needs its high word


def _rng(name: str, salt: int = 0):
    return np.random.default_rng([zlib.crc32(name.encode()), salt])


def _latent(rng, rows, zeros=()):
    """randn [rows, C, FP, H, W] fp32; element k of every row is a zero of sign zeros[k] (None: left alone)"""
    a = rng.standard_normal((rows, C, FP, H, W)).astype(np.float32)
    flat = a.reshape(rows, -1)
    for k, s in enumerate(zeros):
        if s is not None:
            flat[:, k] = np.float32(-0.0) if s < 0 else np.float32(0.0)
    return a


X_ZEROS = (+1, +1, -1, -1, +1, None, -1, None)
E_ZEROS = (+1, -1, +1, -1, None, -1, None, +1)
H_ZEROS = (-1, +1, None, -1, +1, -1, +1, None)


def _eps(rng, rows, cond_f, cfg=True):
    """the UNet output [2 rows or rows, C, cond_f + FP, H, W]; its predicted frames hold E_ZEROS in the uc and in the c half"""
    n = (2 if cfg else 1) * rows
    e = rng.standard_normal((n, C, cond_f + FP, H, W)).astype(np.float32)
    e[:, :, cond_f:] = _latent(rng, n, E_ZEROS)
    return e


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _nan(shape, device):
    return torch.full(tuple(shape), float("nan"), device=device, dtype=torch.float32)


def bits(t) -> np.ndarray:
    """a tensor's words as int32: fp32 and int32 one word an element, int64 two"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32).numpy().copy().reshape(-1)


def _step_noise(ops, seeds, index, device, temperature=TEMPERATURE):
    """what the seeded step draws for clips with `seeds` at `index`, as the noise tensor of the unseeded kernel"""
    rows = [ops.philox_normal(s, ops.PHILOX_STREAM_STEP, index, PER_CLIP, device) for s in seeds]
    return (torch.stack(rows).reshape(len(seeds), C, FP, H, W) * temperature).contiguous()


def _known_noise(ops, seeds, indices, device):
    rows = [ops.philox_normal(s, ops.PHILOX_STREAM_KNOWN, i, PER_CLIP, device) for s, i in zip(seeds, indices)]
    return torch.stack(rows).reshape(len(seeds), C, FP, H, W).contiguous()


def _slot_tables(device, etas):
    """a schedule per slot: coef [slots, NSCHED, 4] (every slot another table) and t_table [slots, NSCHED]"""
    coef = np.stack([coef_table(eta, 0.01 * s) for s, eta in enumerate(etas)])
    ttab = np.stack([T_TABLE + 7 * s for s in range(len(etas))])
    return _t(coef, device), _t(ttab, device)


# ---- DDIM: cfg x noise x index x pred_x0 --------------------------------------------------------------------------------------------
def _ddim(name, form, ops, device, *, cfg, noise, index, pred):
    b = 2
    rng = _rng(name)
    eps, x = _t(_eps(rng, b, COND_F, cfg), device), _t(_latent(rng, b, X_ZEROS), device)
    coef = _t(coef_table(0. if noise == "seeded0" else 0.8), device)
    seeds = ops.seed_words(SEEDS[:b]).to(device)
    kw = dict(cfg=bool(cfg), scale=SCALE, cond_f=COND_F)
    tensor = None
    if noise == "tensor":
        tensor = _t(_rng(name, 1).standard_normal((b, C, FP, H, W)).astype(np.float32), device)
    elif noise == "seeded" and form in ("host", "dev", "dev_alias"):
        tensor = _step_noise(ops, SEEDS[:b], index, device)          # the unseeded kernel fed what the seeded one draws
    step = _t(np.array([9, index], dtype=np.int32), device)
    own = {}
    if form == "host":
        x_prev, p = ops.cfg_ddim_step(eps, x, coef, index, noise=tensor, want_pred_x0=bool(pred), **kw)
    elif form == "rng_host":
        x_prev, p = ops.cfg_ddim_step_rng(eps, x, coef, index, seeds, temperature=TEMPERATURE, want_pred_x0=bool(pred), **kw)
    elif form == "rng_alias":
        x_prev, p = ops.cfg_ddim_step_rng(eps, x, coef, index, seeds, temperature=TEMPERATURE, x_prev=x, want_pred_x0=bool(pred), **kw)
    elif form in ("dev", "dev_alias", "rng_dev"):
        x_prev = x if form == "dev_alias" else _nan(x.shape, device)
        p = _nan(x.shape, device) if pred else None
        if form == "rng_dev":
            ops.cfg_ddim_step_rng_dev(eps, x, coef, step, seeds, temperature=TEMPERATURE, x_prev=x_prev, pred_x0=p, **kw)
        else:
            ops.cfg_ddim_step_dev(eps, x, coef, step, x_prev=x_prev, pred_x0=p, noise=tensor, **kw)
        own["step"] = bits(step)
    else:                                                            # slot, slot_rng: the clips as slots, each with its own tables
        assert cfg and form in ("slot", "slot_rng"), form
        coefs = coef[None].repeat(b, 1, 1).contiguous()
        scale = torch.full((b,), SCALE, device=device)
        steps = step[None].repeat(b, 1).contiguous()
        x_prev, p = _nan(x.shape, device), (_nan(x.shape, device) if pred else None)
        if form == "slot":
            ops.slot_cfg_ddim_step(eps, x, scale, coefs, steps, cond_f=COND_F, x_prev=x_prev, pred_x0=p)
        else:
            ops.slot_cfg_ddim_step_rng(eps, x, scale, coefs, steps, seeds, torch.full((b,), TEMPERATURE, device=device),
                                       cond_f=COND_F, x_prev=x_prev, pred_x0=p)
        own["step"] = bits(steps)
    shared = {"x_prev": bits(x_prev)}
    if pred:
        shared["pred_x0"] = bits(p)
    return shared, own


_DDIM_FORMS = {"none": ["host", "dev", "dev_alias", "slot"], "tensor": ["host", "dev", "dev_alias"],
               "seeded": ["host", "dev", "rng_host", "rng_dev", "rng_alias", "slot_rng"],
               "seeded0": ["host", "dev", "rng_host", "rng_dev", "rng_alias", "slot", "slot_rng"]}


# ---- PLMS: order x cfg, and a ring chain of the captured form ---------------------------------------------------------------------------
def _plms(name, form, ops, device, *, cfg, order):
    b = 2
    rng = _rng(name)
    eps, x = _t(_eps(rng, b, COND_F, cfg), device), _t(_latent(rng, b, X_ZEROS), device)
    coef = _t(coef_table(0.), device)
    need = (0, 1, 1, 2, 3)[order]
    # three history tensors whatever the order: the ones the order does not use are NaN and must not be read
    hist = [_t(_latent(rng, b, H_ZEROS), device) if k < need else _nan(x.shape, device) for k in range(3)]
    kw = dict(cfg=bool(cfg), scale=SCALE, cond_f=COND_F, history=hist)
    # host: fresh outputs.  alias: x_prev is x and e_out the oldest history tensor -- h3, which order 4 reads before e lands in it.
    # Order 1 keeps no e: its e_out (NaN in both forms) stays as it is.
    x_prev, e_out = (_nan(x.shape, device), _nan(x.shape, device)) if form == "host" else (x, hist[2])
    pred = _nan(x.shape, device)
    ops.cfg_plms_step(eps, x, coef, 3, order, x_prev=x_prev, pred_x0=pred, e_out=e_out, **kw)
    return {"x_prev": bits(x_prev), "pred_x0": bits(pred), "e": bits(e_out)}, {}


def _plms_ring(name, form, ops, device):
    """six replays of begin -> seer_cfg_plms_step_dev from index 5, the latent updated in place"""
    b, f1 = 2, COND_F
    rng = _rng(name)
    x, x0_emb = _t(_latent(rng, b, X_ZEROS), device), _t(rng.standard_normal((b, C, f1, H, W)).astype(np.float32), device)
    coef, ttab = _t(coef_table(0.), device), _t(T_TABLE, device)
    step = _t(np.array([NSCHED - 1, -7], dtype=np.int32), device)
    ring, ring_state = _nan((3, *x.shape), device), _t(np.array([5, 5, 0, 2], dtype=np.int32), device)    # index 5 is odd: pair 1
    sample, t_out = _nan((2 * b, C, f1 + FP, H, W), device), torch.zeros((2 * b,), dtype=torch.int64, device=device)
    shared = {}
    for r in range(NSCHED):
        eps, pred = _t(_eps(rng, b, f1), device), _nan(x.shape, device)
        ops.ddim_step_begin(x0_emb, x, ttab, step, 2, sample, t_out)
        if r == 0:
            shared["sample"] = bits(sample)
        ops.cfg_plms_step_dev(eps, x, coef, step, ring, ring_state, cfg=True, scale=SCALE, cond_f=f1, x_prev=x, pred_x0=pred)
        shared.update({f"x{r}": bits(x), f"pred{r}": bits(pred), f"t{r}": bits(t_out), f"step{r}": bits(step),
                       f"ring_state{r}": bits(ring_state)})
    shared["ring"] = bits(ring)
    return shared, {}


# ---- slots: chains of begin -> update, three slots ---------------------------------------------------------------------------------------
def _slot_chain(name, form, ops, device, *, kind):
    slots, f1 = 3, COND_F
    rng = _rng(name)
    x, x0_emb = _t(_latent(rng, slots, X_ZEROS), device), _t(rng.standard_normal((slots, C, f1, H, W)).astype(np.float32), device)
    coef, ttab = _slot_tables(device, (0.8, 0.8, 0.8) if kind == "rng" else (0., 0., 0.))
    scale = _t(np.array([SCALE, 3.0, 1.5], dtype=np.float32), device)
    sample, t_out = _nan((2 * slots, C, f1 + FP, H, W), device), torch.zeros((2 * slots,), dtype=torch.int64, device=device)
    shared = {}
    if kind == "plms":
        # slot 0 idle, slot 1 a DDIM clip (six steps, idle in the seventh), slot 2 a PLMS clip: phases 1, 2, then five times 3
        n_steps = NSCHED + 1
        step = _t(np.array([[-1, -1], [NSCHED - 1, -1], [NSCHED - 1, -1]], dtype=np.int32), device)
        state = _t(np.array([[0] * 8, [0] * 8, [1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32), device)
        ring, x_prov = _nan((slots, 3, C, FP, H, W), device), _nan(x.shape, device)
    else:
        # slot 0 idle, slot 1 with a counter no schedule produces, slot 2 four steps from index 3
        n_steps = 4
        step = _t(np.array([[-1, -1], [NSCHED + 3, -1], [3, -1]], dtype=np.int32), device)
        seeds = ops.seed_words(SEEDS).to(device)
        temperature = _t(np.array([1.0, 0.5, TEMPERATURE], dtype=np.float32), device)
    for r in range(n_steps):
        eps, pred = _t(_eps(rng, slots, f1), device), _nan(x.shape, device)
        if kind == "plms":
            ops.slot_plms_step_begin(x0_emb, x, x_prov, ttab, step, state, 2, sample, t_out)
            ops.slot_cfg_plms_step(eps, x, scale, coef, step, state, ring, x_prov, cond_f=f1, x_prev=x, pred_x0=pred)
            shared[f"state{r}"] = bits(state)
        else:
            ops.slot_step_begin(x0_emb, x, ttab, step, 2, sample, t_out)
            if kind == "rng":
                ops.slot_cfg_ddim_step_rng(eps, x, scale, coef, step, seeds, temperature, cond_f=f1, x_prev=x, pred_x0=pred)
            else:
                ops.slot_cfg_ddim_step(eps, x, scale, coef, step, cond_f=f1, x_prev=x, pred_x0=pred)
        shared.update({f"x{r}": bits(x), f"pred{r}": bits(pred), f"t{r}": bits(t_out), f"step{r}": bits(step)})
    if kind == "plms":
        shared["ring"], shared["x_prov"] = bits(ring), bits(x_prov)
    return shared, {}


# ---- the slot begin kernels: reps x f1 x phases ------------------------------------------------------------------------------------------
_PHASES = {"A": ((0, 1, 2), (-1, NSCHED + 3, 3)), "B": ((3, 2, 7), (2, 0, 4))}       # (phase per slot, step[s][0] per slot)


def _slot_begin(name, form, ops, device, *, reps, f1, phases):
    slots = 3
    rng = _rng(name)
    x, x_prov = _t(_latent(rng, slots, X_ZEROS), device), _t(_latent(rng, slots), device)
    x0_emb = _t(rng.standard_normal((slots, C, f1, H, W)).astype(np.float32), device) if f1 else None
    _, ttab = _slot_tables(device, (0., 0., 0.))
    sample = _nan((reps * slots, C, f1 + FP, H, W), device)
    t_out = torch.full((reps * slots,), -1, dtype=torch.int64, device=device)
    if phases is None:
        step = _t(np.array([[-1, -5], [NSCHED + 3, -5], [3, -5]], dtype=np.int32), device)
        ops.slot_step_begin(x0_emb, x, ttab, step, reps, sample, t_out)
        return {"sample": bits(sample), "t_out": bits(t_out), "step": bits(step)}, {}
    ph, idx = _PHASES[phases]
    step = _t(np.array([[i, -5] for i in idx], dtype=np.int32), device)
    state = _t(np.array([[p, 1 + s, 2 - s, -9, -9, -9, -9, -9] for s, p in enumerate(ph)], dtype=np.int32), device)
    ops.slot_plms_step_begin(x0_emb, x, x_prov, ttab, step, state, reps, sample, t_out)
    return {"sample": bits(sample), "t_out": bits(t_out), "step": bits(step), "state": bits(state)}, {}


# ---- given latents -----------------------------------------------------------------------------------------------------------------------
def _mask(rng, rows):
    return rng.choice(np.array([0., 1., 0.5], dtype=np.float32), size=(rows, FP, H, W))


def _known_blend(name, form, ops, device, *, noise, index_from):
    b, index = 2, 3
    rng = _rng(name)
    x, known, mask = _t(_latent(rng, b, X_ZEROS), device), _t(_latent(rng, b, H_ZEROS), device), _t(_mask(rng, b), device)
    coef = _t(coef_table(0.8), device)
    step = _t(np.array([index, 9], dtype=np.int32), device) if index_from == "step" else None
    kw = dict(step=step) if step is not None else {}
    if noise == "tensor":
        kw["noise"] = _t(rng.standard_normal((b, C, FP, H, W)).astype(np.float32), device)
    elif form == "seeds":
        kw["seeds"] = ops.seed_words(SEEDS[:b]).to(device)
    else:                                                            # tensor: the noise-tensor form fed what the seeded one draws
        kw["noise"] = _known_noise(ops, SEEDS[:b], [index] * b, device)
    ops.known_blend(x, mask, known, coef, 0 if step is not None else index, **kw)
    return {"x": bits(x)}, ({"step": bits(step)} if step is not None else {})


def _slot_known_blend(name, form, ops, device):
    slots = 3
    rng = _rng(name)
    x, known, mask = _t(_latent(rng, slots, X_ZEROS), device), _t(_latent(rng, slots, H_ZEROS), device), _t(_mask(rng, slots), device)
    coef, _ = _slot_tables(device, (0.8, 0.8, 0.8))
    idx = (-1, NSCHED + 3, 3)
    step = _t(np.array([[i, 9] for i in idx], dtype=np.int32), device)
    if form == "slot":
        ops.slot_known_blend(x, mask, known, coef, step, ops.seed_words(SEEDS).to(device))
    else:                                                            # clip: the active slot through seer_known_blend
        s = 2
        xs = x[s:s + 1].contiguous()
        ops.known_blend(xs, mask[s:s + 1].contiguous(), known[s:s + 1].contiguous(), coef[s].contiguous(), idx[s],
                        seeds=ops.seed_words(SEEDS[s:s + 1]).to(device))
        x[s:s + 1] = xs
    return {"x": bits(x)}, {"step": bits(step)}


def _q_sample(name, form, ops, device, *, noise):
    b = 3
    rng = _rng(name)
    x0, coef = _t(_latent(rng, b, X_ZEROS), device), _t(coef_table(0.8), device)
    idx = (4, NSCHED, 0)                                             # the middle row's index is outside the table
    index = _t(np.array(idx, dtype=np.int32), device)
    out = _nan(x0.shape, device)
    if noise == "tensor":
        ops.q_sample(x0, coef, index, noise=_t(rng.standard_normal((b, C, FP, H, W)).astype(np.float32), device), out=out)
    elif form == "seeds":
        ops.q_sample(x0, coef, index, seeds=ops.seed_words(SEEDS).to(device), out=out)
    else:
        ops.q_sample(x0, coef, index, noise=_known_noise(ops, SEEDS, [i % NSCHED for i in idx], device), out=out)
    return {"out": bits(out)}, {}


# ---- the case list -----------------------------------------------------------------------------------------------------------------------
def _cases():
    cases = {}
    for cfg in (0, 1):
        for noise in ("none", "tensor", "seeded", "seeded0"):
            for index in (0, 3):
                for pred in (0, 1):
                    forms = [f for f in _DDIM_FORMS[noise] if cfg or not f.startswith("slot")]
                    cases[f"ddim_cfg{cfg}_{noise}_i{index}_pred{pred}"] = (_ddim, dict(cfg=cfg, noise=noise, index=index, pred=pred), forms)
        for order in range(5):
            cases[f"plms_cfg{cfg}_order{order}"] = (_plms, dict(cfg=cfg, order=order), ["host", "alias"])
    cases["plms_ring_chain"] = (_plms_ring, {}, ["chain"])
    for kind in ("ddim", "rng", "plms"):
        cases[f"slot_chain_{kind}"] = (_slot_chain, dict(kind=kind), ["chain"])
    for reps, f1, phases in ((1, 0, "A"), (1, 2, "B"), (2, 0, "B"), (2, 2, "A")):
        cases[f"slot_begin_reps{reps}_f{f1}"] = (_slot_begin, dict(reps=reps, f1=f1, phases=None), ["begin"])
        cases[f"slot_plms_begin_reps{reps}_f{f1}_{phases}"] = (_slot_begin, dict(reps=reps, f1=f1, phases=phases), ["begin"])
    for index_from in ("host", "step"):
        cases[f"known_blend_tensor_{index_from}"] = (_known_blend, dict(noise="tensor", index_from=index_from), ["tensor"])
        cases[f"known_blend_seeded_{index_from}"] = (_known_blend, dict(noise="seeded", index_from=index_from), ["seeds", "tensor"])
    cases["slot_known_blend"] = (_slot_known_blend, {}, ["slot", "clip"])
    cases["q_sample_tensor"] = (_q_sample, dict(noise="tensor"), ["tensor"])
    cases["q_sample_seeded"] = (_q_sample, dict(noise="seeded"), ["seeds", "tensor"])
    return cases


CASES = _cases()


def forms(name):
    return list(CASES[name][2])


def run(name, form, ops, device):
    fn, kw, fs = CASES[name]
    assert form in fs, (name, form)
    return fn(name, form, ops, device, **kw)


def keys(name, form, shared, own):
    """the fixture's names for one run: what all forms share under the case, the rest under the form"""
    out = {f"{name}/{k}": v for k, v in shared.items()}
    out.update({f"{name}/{form}/{k}": v for k, v in own.items()})
    return out
