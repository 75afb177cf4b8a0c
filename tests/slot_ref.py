"""A torch restatement of the two slot kernels (include/seer_hip.h: seer_slot_step_begin, seer_slot_cfg_ddim_step) with the
signatures of ops.slot_step_begin / ops.slot_cfg_ddim_step, on tensors of any device: `SlotSampler(ops=tests.slot_ref)` runs the
host logic of the slot queue on the CPU.  The update is fp32 torch arithmetic in the kernel's expression order (torch does not
fuse a multiply with an add, the device code may: equal to rounding, not to the bit)."""
import torch


def slot_step_begin(x0_emb, x, t_table, step, reps, sample, t_out):
    slots = x.shape[0]
    assert reps in (1, 2) and tuple(step.shape) == (slots, 2) and t_table.shape[0] == slots
    index = step[:, 0].clone()
    step[:, 1] = index
    rows = torch.cat([x0_emb, x], dim=2) if x0_emb is not None else x
    assert tuple(sample.shape) == (reps * slots, *rows.shape[1:])
    t = t_table[torch.arange(slots, device=x.device), index.clamp(min=0).long()]
    for r in range(reps):
        sample[r * slots:(r + 1) * slots] = rows
        t_out[r * slots:(r + 1) * slots] = t


def slot_cfg_ddim_step(eps, x, scale, coef, step, *, cond_f, x_prev, pred_x0):
    slots = x.shape[0]
    assert eps.shape[0] == 2 * slots and eps.shape[2] == x.shape[2] + cond_f and tuple(coef.shape[::2]) == (slots, 4)
    for s in range(slots):
        index = int(step[s, 1])
        if index < 0:
            continue                                # idle: nothing of the slot is written
        eu, ec = eps[s, :, cond_f:], eps[slots + s, :, cond_f:]
        e = eu + scale[s] * (ec - eu)
        a_t, a_prev, sigma, s1m = coef[s, index]
        x0 = (x[s] - s1m * e) / torch.sqrt(a_t)
        dirx = torch.sqrt(1.0 - a_prev - sigma * sigma) * e
        x_prev[s] = torch.sqrt(a_prev) * x0 + dirx
        if pred_x0 is not None:
            pred_x0[s] = x0
        step[s, 0] = index - 1
