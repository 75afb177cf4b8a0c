"""The PLMS sampler (ldm/models/diffusion/plms.py:114-236, eta = 0) restated over the oracle's model call: the CPU side of
tests/test_plms_host.py and tests/test_gpu_plms.py.  `unet_fn(x, t, c, cond_frame)` is e.g. oracle.seer_oracle.unet_forward over
closed-form weights; the model call around it is Seer's p_sample_ddim (ddim_video.py:187-207), as in oracle.seer_oracle."""
import numpy as np
import torch

from oracle import seer_oracle as O


def model_eps(unet_fn, x, c, t, x0_emb=None, scale=1.0, uc=None, cond_frames=0):
    """the CFG-combined eps of the prediction frames"""
    cond_f = 0 if x0_emb is None else x0_emb.shape[2]
    x_cat = x if x0_emb is None else torch.cat([x0_emb.to(x.dtype), x], dim=2)
    if uc is None or scale == 1.0:
        return unet_fn(x_cat, t, c, 0)[:, :, cond_f:]
    if uc.shape[2] == c.shape[2]:
        e_uc, e_c = unet_fn(torch.cat([x_cat] * 2), torch.cat([t] * 2), torch.cat([uc, c]), cond_frames).chunk(2)
    else:
        e_uc, e_c = unet_fn(x_cat, t, uc, cond_frames), unet_fn(x_cat, t, c, cond_frames)
    e_uc, e_c = e_uc[:, :, cond_f:], e_c[:, :, cond_f:]
    return e_uc + scale * (e_c - e_uc)


def update(x, e, index, sched, dtype=torch.float32):
    """get_x_prev_and_pred_x0 (plms.py:199-216) at sigma = 0 with the schedule's values as `dtype` scalars"""
    f = lambda v: torch.full((x.shape[0],) + (1,) * (x.dim() - 1), float(v), dtype=dtype)
    a_t, a_prev = f(sched["alphas"][index]), f(sched["alphas_prev"][index])
    sigma_t, s1m = f(sched["sigmas"][index]), f(sched["sqrt_one_minus_alphas"][index])
    pred_x0 = (x - s1m * e) / a_t.sqrt()
    dir_xt = (1.0 - a_prev - sigma_t ** 2).sqrt() * e
    return a_prev.sqrt() * pred_x0 + dir_xt, pred_x0


def combine(e, old_eps):
    """e' of plms.py:219-232 for a step with earlier eps (old_eps, oldest first, non-empty)"""
    if len(old_eps) == 1:
        return (3 * e - old_eps[-1]) / 2
    if len(old_eps) == 2:
        return (23 * e - 16 * old_eps[-1] + 5 * old_eps[-2]) / 12
    return (55 * e - 59 * old_eps[-1] + 37 * old_eps[-2] - 9 * old_eps[-3]) / 24


def p_sample_plms(eps_fn, x, t, index, sched, old_eps, t_next, draw=None, dtype=torch.float32):
    """plms.py:172-236 -> (x_prev, pred_x0, e_t); eps_fn(x, t) is the CFG-combined model output; `draw` is called once per
    update (the reference's noise_like draw, plms.py:212)"""
    draw = draw or (lambda: None)
    e_t = eps_fn(x, t)
    if len(old_eps) == 0:
        x_prev, _ = update(x, e_t, index, sched, dtype)
        draw()
        e_t_prime = (e_t + eps_fn(x_prev, t_next)) / 2
    else:
        e_t_prime = combine(e_t, old_eps)
    x_prev, pred_x0 = update(x, e_t_prime, index, sched, dtype)
    draw()
    return x_prev, pred_x0, e_t


def plms_sampling(eps_fn, S, x_T, draw=None, dtype=torch.float32):
    """plms.py:114-170 over the DDIM schedule of S steps -> (final latent, [(x_prev, pred_x0, e_t) per step])"""
    sched = O.make_schedule(S)
    ts = np.flip(sched["ddim_timesteps"])
    n = len(ts)
    img, old_eps, steps = x_T, [], []
    for i, step in enumerate(ts):
        index = n - i - 1
        t = torch.full((x_T.shape[0],), int(step), dtype=torch.long)
        t_next = torch.full((x_T.shape[0],), int(ts[min(i + 1, n - 1)]), dtype=torch.long)
        img, pred_x0, e_t = p_sample_plms(eps_fn, img, t, index, sched, old_eps, t_next, draw, dtype)
        steps.append((img, pred_x0, e_t))
        old_eps.append(e_t)
        if len(old_eps) >= 4:
            old_eps.pop(0)
    return img, steps


def seer_eps_fn(unet_fn, c, x0_emb=None, scale=1.0, uc=None, cond_frames=0):
    return lambda x, t: model_eps(unet_fn, x, c, t, x0_emb, scale, uc, cond_frames)
