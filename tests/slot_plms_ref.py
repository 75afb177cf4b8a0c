"""A torch restatement of the two slot kernels that carry a sampler per slot (include/seer_hip.h: seer_slot_plms_step_begin,
seer_slot_cfg_plms_step) with the signatures of ops.slot_plms_step_begin / ops.slot_cfg_plms_step, on tensors of any device:
`SlotSampler(plms=True, ops=tests.slot_plms_ref)` runs the host logic of a mixed DDIM / PLMS queue on the CPU.  The update is fp32
torch arithmetic in the kernel's expression order, as in tests/slot_ref.py (whose two functions are exported here too, so that one
module serves a sampler built with or without plms).  state int32 [slots, 8]: words 0..2 = (phase, valid, newest) of the next step,
words 4..6 = of the step in flight."""
import torch

from tests.slot_ref import slot_cfg_ddim_step, slot_step_begin  # noqa: F401

WORDS, FLY = 8, 4


def slot_plms_step_begin(x0_emb, x, x_prov, t_table, step, state, reps, sample, t_out):
    slots = x.shape[0]
    assert reps in (1, 2) and tuple(step.shape) == (slots, 2) and t_table.shape[0] == slots and tuple(state.shape) == (slots, WORDS)
    assert x_prov.shape == x.shape and x_prov.data_ptr() != x.data_ptr()
    index = step[:, 0].clone()
    step[:, 1] = index
    state[:, FLY:FLY + 3] = state[:, :3].clone()
    second = state[:, 0] == 2                            # the second evaluation of a PLMS clip's first step: x_prov at t_next
    lat = torch.where(second.view(-1, 1, 1, 1, 1), x_prov, x)
    rows = torch.cat([x0_emb, lat], dim=2) if x0_emb is not None else lat
    assert tuple(sample.shape) == (reps * slots, *rows.shape[1:])
    row = (index - second.to(index.dtype)).clamp(min=0, max=t_table.shape[1] - 1).long()
    t = t_table[torch.arange(slots, device=x.device), row]
    for r in range(reps):
        sample[r * slots:(r + 1) * slots] = rows
        t_out[r * slots:(r + 1) * slots] = t


def _update(x, ep, row):
    a_t, a_prev, sigma, s1m = row
    x0 = (x - s1m * ep) / torch.sqrt(a_t)
    dirx = torch.sqrt(1.0 - a_prev - sigma * sigma) * ep
    return torch.sqrt(a_prev) * x0 + dirx, x0


def slot_cfg_plms_step(eps, x, scale, coef, step, state, ring, x_prov, *, cond_f, x_prev, pred_x0):
    slots, nsched = x.shape[0], coef.shape[1]
    assert eps.shape[0] == 2 * slots and eps.shape[2] == x.shape[2] + cond_f and tuple(coef.shape[::2]) == (slots, 4)
    assert tuple(state.shape) == (slots, WORDS) and tuple(ring.shape) == (slots, 3, *x.shape[1:]) and x_prov.shape == x.shape
    for s in range(slots):
        index = int(step[s, 1])
        if index < 0 or index >= nsched:
            continue                                    # idle: nothing of the slot is written
        phase, valid, newest = (int(v) for v in state[s, FLY:FLY + 3])
        eu, ec = eps[s, :, cond_f:], eps[slots + s, :, cond_f:]
        e = eu + scale[s] * (ec - eu)
        if phase == 1:
            x_prov[s], _ = _update(x[s], e, coef[s, index])
            ring[s, 0] = e
            state[s, :3] = torch.tensor([2, 1, 0], dtype=torch.int32)
            continue
        if phase == 2:
            newest = newest if 0 <= newest <= 2 else 0
            ep = (ring[s, newest] + e) / 2.0
            state[s, 0] = 3
        elif phase == 3:
            if not (0 <= valid <= 3 and 0 <= newest <= 2):
                valid, newest = 0, 2
            h1, h2, h3 = ring[s, newest], ring[s, (newest + 2) % 3], ring[s, (newest + 1) % 3]
            if valid == 0:
                ep = e
            elif valid == 1:
                ep = (3.0 * e - h1) / 2.0
            elif valid == 2:
                ep = (23.0 * e - 16.0 * h1 + 5.0 * h2) / 12.0
            else:
                ep = (55.0 * e - 59.0 * h1 + 37.0 * h2 - 9.0 * h3) / 24.0
            ring[s, (newest + 1) % 3] = e
            state[s, 1], state[s, 2] = min(valid + 1, 3), (newest + 1) % 3
        else:
            ep = e                                      # DDIM, and every phase outside 0..3
        x_prev[s], x0 = _update(x[s], ep, coef[s, index])
        if pred_x0 is not None:
            pred_x0[s] = x0
        step[s, 0] = index - 1
