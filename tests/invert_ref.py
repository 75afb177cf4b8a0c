"""DDIM inversion restated on the CPU (include/seer_hip.h, seer_cfg_ddim_invert_step; DESIGN.md, "Editing"; CompVis
ldm/models/diffusion/ddim.py, encode()).

  * invert_step64 / encode64: the update and the whole upward chain in float64 -- what the kernel and DDIMSampler.encode are measured
    against; nothing in them comes from a kernel;
  * decode64: the deterministic DDIM chain back down in float64, for round trips;
  * gaussian_case: the analytic model of the round-trip tests -- data N(mu, s^2) has the exact eps, and its probability-flow ODE a
    closed-form end point;
  * cfg_ddim_invert_step: an fp32 torch stand-in with the signature of seervideoldm_amd.ops, in the kernel's expression order: equal to
    the kernel to rounding, not to the bit.  With the names of tests/edit_ref.py, re-exported here, this module is a whole backend:
    `DDIMSampler("cpu", ops=tests.invert_ref)` runs the host logic on the CPU."""
import math

import torch

from tests.edit_ref import (cfg_ddim_step, cfg_ddim_step_rng, known_blend, philox_normal, q_sample, slot_cfg_ddim_step,  # noqa: F401
                            slot_cfg_ddim_step_rng, slot_known_blend, slot_step_begin)

f64 = torch.float64


def invert_step64(e, x, coef_row):
    """one step upward in float64: x at the level of a_prev, e the CFG-combined eps at the timestep of a_t -> (x_next, pred_x0).
    coef_row = (a_t, a_prev, sigma, sqrt(1 - a_t)) as the kernel reads it (fp32 values, taken to float64 as they are)"""
    a_t, a_prev, _, s1m = [float(v) for v in coef_row]
    x0 = (x.to(f64) - math.sqrt(1.0 - a_prev) * e.to(f64)) / math.sqrt(a_prev)
    return math.sqrt(a_t) * x0 + s1m * e.to(f64), x0


def ddim_step64(e, x, coef_row):
    """the deterministic DDIM step downward in float64 (sigma = 0) -> (x_prev, pred_x0)"""
    a_t, a_prev, _, s1m = [float(v) for v in coef_row]
    x0 = (x.to(f64) - s1m * e.to(f64)) / math.sqrt(a_t)
    return math.sqrt(a_prev) * x0 + math.sqrt(1.0 - a_prev) * e.to(f64), x0


def encode64(eps_fn, x0, coef, timesteps, t_enc):
    """DDIMSampler.encode in float64: indices 0 .. t_enc - 1 upward; eps_fn(x, t) is the CFG-combined model output at the long
    tensor t [b] (the target level's timestep).  -> (latent, [(x_next, pred_x0) per step])"""
    x, steps = x0.to(f64), []
    for index in range(int(t_enc)):
        t = torch.full((x.shape[0],), int(timesteps[index]), dtype=torch.long)
        x, pred = invert_step64(eps_fn(x, t), x, coef[index])
        steps.append((x, pred))
    return x, steps


def decode64(eps_fn, x_latent, coef, timesteps, t_start):
    """DDIMSampler.decode at eta = 0 in float64: indices t_start - 1 .. 0 downward -> the latent"""
    x = x_latent.to(f64)
    for index in reversed(range(int(t_start))):
        t = torch.full((x.shape[0],), int(timesteps[index]), dtype=torch.long)
        x, _ = ddim_step64(eps_fn(x, t), x, coef[index])
    return x


def gaussian_case(alphas_cumprod, shape=(1, 4, 5, 20, 50), s=0.5, seed=3):
    """Data N(mu, s^2), mu = 0.3 randn per element, no guidance: eps(x, t) = sqrt(1 - a) (x - sqrt(a) mu) / (a s^2 + 1 - a) exactly, and
    the probability-flow ODE carries x at level a to sqrt(a') mu + sqrt((a' s^2 + 1 - a') / (a s^2 + 1 - a)) (x - sqrt(a) mu) at
    level a'.  -> dict(mu, x0 (a draw of the data, float64), eps(x, t), flow(x, a_from, a_to)); N = 20 000 elements by default"""
    g = torch.Generator().manual_seed(seed)
    mu = 0.3 * torch.randn(shape, generator=g, dtype=f64)
    x0 = mu + s * torch.randn(shape, generator=g, dtype=f64)
    ac = alphas_cumprod.to(f64)

    def eps(x, t):
        a = ac[t.cpu().long()].view(-1, *([1] * (x.dim() - 1)))
        return (1 - a).sqrt() * (x.to(f64) - a.sqrt() * mu) / (a * s * s + (1 - a))

    def flow(x, a_from, a_to):
        return a_to ** 0.5 * mu + ((a_to * s * s + 1 - a_to) / (a_from * s * s + 1 - a_from)) ** 0.5 * (x.to(f64) - a_from ** 0.5 * mu)
    return dict(mu=mu, x0=x0, eps=eps, flow=flow)


# ---- the stand-in for seervideoldm_amd.ops ----------------------------------------------------------------------------------------
def cfg_ddim_invert_step(eps, x, coef, index, *, cfg, scale, cond_f, x_next=None, want_pred_x0=True):
    if not 0 <= int(index) < coef.shape[0]:
        raise ValueError(f"index {index}: the table has {coef.shape[0]} rows")
    b = x.shape[0]
    e = eps[:, :, cond_f:]
    e = e[:b] + scale * (e[b:] - e[:b]) if cfg else e
    a_t, a_prev, _, s1m = coef[index]
    x0 = (x - torch.sqrt(1.0 - a_prev) * e) / torch.sqrt(a_prev)
    new = torch.sqrt(a_t) * x0 + s1m * e
    if x_next is not None:
        x_next.copy_(new)
        new = x_next
    return new, (x0 if want_pred_x0 else None)
