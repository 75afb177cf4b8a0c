"""A torch restatement of the slot update that carries a sampler per slot, DDIM or DPM-Solver++ (include/seer_hip.h:
seer_slot_cfg_dpm_step), with the signature of ops.slot_cfg_dpm_step, on tensors of any device: `SlotSampler(dpm=True,
ops=tests.slot_dpm_ref)` runs the host logic of a mixed DDIM / DPM-Solver++ queue on the CPU.  The update is fp32 torch arithmetic in
the kernel's expression order, as in tests/slot_ref.py (whose two functions are exported here too, so that one module serves a
sampler built with or without dpm).  state int32 [slots, 4]: (history valid for an even index, for an odd one, the slot's sampler --
0 DDIM, 1 first order, 2 2M --, the schedule's final step is first order)."""
import torch

from tests.slot_ref import slot_cfg_ddim_step, slot_step_begin  # noqa: F401

WORDS, ROW = 4, 6


def slot_cfg_dpm_step(eps, x, scale, coef, step, dpm_coef, state, *, cond_f, x_prev, pred_x0):
    slots, nsched = x.shape[0], coef.shape[1]
    assert eps.shape[0] == 2 * slots and eps.shape[2] == x.shape[2] + cond_f and tuple(coef.shape[::2]) == (slots, 4)
    assert tuple(dpm_coef.shape) == (slots, nsched, ROW) and tuple(state.shape) == (slots, WORDS) and state.dtype == torch.int32
    assert pred_x0 is not None and pred_x0.shape == x.shape and pred_x0.data_ptr() not in (x.data_ptr(), x_prev.data_ptr())
    for s in range(slots):
        index = int(step[s, 1])
        if index < 0 or index >= nsched:
            continue                                    # idle: nothing of the slot is written
        sampler, final_first = int(state[s, 2]), int(state[s, 3])
        eu, ec = eps[s, :, cond_f:], eps[slots + s, :, cond_f:]
        e = eu + scale[s] * (ec - eu)
        xs = x[s].clone()
        if sampler in (1, 2):
            order = 2 if int(state[s, index & 1]) == 1 and sampler == 2 and not (index == 0 and final_first != 0) else 1
            row = dpm_coef[s, index]
            d = (xs - row[0] * e) * row[1]
            if order == 2:
                x_prev[s] = row[2] * xs + row[4] * d + row[5] * pred_x0[s]      # the history is read here only: it may hold NaN
            else:
                x_prev[s] = row[2] * xs + row[3] * d
            pred_x0[s] = d
            state[s, (index - 1) & 1] = 1
        else:                                           # DDIM, and every sampler word outside 0..2
            a_t, a_prev, sigma, s1m = coef[s, index]
            x0 = (xs - s1m * e) / torch.sqrt(a_t)
            dirx = torch.sqrt(1.0 - a_prev - sigma * sigma) * e
            x_prev[s] = torch.sqrt(a_prev) * x0 + dirx
            pred_x0[s] = x0
        step[s, 0] = index - 1
