"""The kernels of masked sampling and stochastic_encode, restated on the CPU (include/seer_hip.h, "given latents"; DESIGN.md,
"Editing"): q_sample, known_blend and slot_known_blend in fp32 torch arithmetic with the kernels' expression order and the signatures of
seervideoldm_amd.ops.  Their noise is a given tensor or tests.stoch_ref.normals64 of (seed, stream 2, index) rounded to fp32, so they are
equal to the kernels to rounding, not to the bit.  With the step kernels of tests/stoch_ref.py and tests/slot_ref.py (and a restatement
of the unseeded cfg_ddim_step) this module is a whole backend: `SlotSampler(editing=True, ops=tests.edit_ref)` and
`DDIMSampler("cpu", ops=tests.edit_ref)` run the host logic on the CPU."""
import torch

from tests.slot_ref import slot_cfg_ddim_step  # noqa: F401
from tests.stoch_ref import (_update, cfg_ddim_step_rng, philox_normal, seed_of, slot_cfg_ddim_step_rng,  # noqa: F401
                             slot_step_begin)

STREAM_KNOWN = 2


def _q(coef_row, x0, n):
    return torch.sqrt(coef_row[0]) * x0 + coef_row[3] * n


def _known_noise(seed_words32, index, like):
    return philox_normal(seed_of(seed_words32), STREAM_KNOWN, index, like.numel()).reshape(like.shape).to(like.device)


def _blend(x, m, known, coef_row, n):
    """x [C, Fp, h, w], m [Fp, h, w]: the new x.  m == 0 keeps x's bits, m == 1 selects q, in between CompVis's operand order"""
    q = _q(coef_row, known, n)
    m = m[None].expand_as(x)
    mixed = q * m + (1.0 - m) * x
    return torch.where(m == 0, x, torch.where(m == 1, q, mixed))


def _one_of(noise, seeds):
    if (noise is None) == (seeds is None):
        raise ValueError("exactly one of `noise` and `seeds`")


def q_sample(x0, coef, index, *, noise=None, seeds=None, out=None):
    _one_of(noise, seeds)
    out = torch.empty_like(x0) if out is None else out
    for bi in range(x0.shape[0]):
        idx = int(index[bi])
        if not 0 <= idx < coef.shape[0]:
            continue
        n = noise[bi] if noise is not None else _known_noise(seeds[bi], idx, x0[bi])
        out[bi] = _q(coef[idx], x0[bi], n)
    return out


def known_blend(x, mask, known, coef, index=0, *, step=None, noise=None, seeds=None):
    _one_of(noise, seeds)
    assert tuple(mask.shape) == (x.shape[0], *x.shape[2:]) and known.shape == x.shape
    if step is not None:
        index = int(step[0])
    if index < 0:
        return x
    for bi in range(x.shape[0]):
        if not mask[bi].any():
            continue                                # nothing is drawn for a row that keeps nothing
        n = noise[bi] if noise is not None else _known_noise(seeds[bi], index, x[bi])
        x[bi] = _blend(x[bi], mask[bi], known[bi], coef[index], n)
    return x


def slot_known_blend(x, mask, known, coef, step, seeds):
    slots = x.shape[0]
    assert tuple(mask.shape) == (slots, *x.shape[2:]) and known.shape == x.shape and tuple(coef.shape[::2]) == (slots, 4)
    assert tuple(step.shape) == (slots, 2) and tuple(seeds.shape) == (slots, 2)
    for s in range(slots):
        index = int(step[s, 0])
        if index < 0 or index >= coef.shape[1] or not mask[s].any():
            continue                                # idle, or a plain clip: nothing of the slot is written
        x[s] = _blend(x[s], mask[s], known[s], coef[s, index], _known_noise(seeds[s], index, x[s]))


def cfg_ddim_step(eps, x, coef, index, *, cfg, scale, cond_f, noise=None, want_pred_x0=True):
    """the unseeded step (ops.cfg_ddim_step): stoch_ref's update with a noise tensor"""
    b = x.shape[0]
    e = eps[:, :, cond_f:]
    e = e[:b] + scale * (e[b:] - e[:b]) if cfg else e
    new, pred = _update(e, x, coef[index], noise)
    return new, (pred if want_pred_x0 else None)
