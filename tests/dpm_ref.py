"""DPM-Solver++ restated in float64, straight from its definition in lambda, h and r (Lu et al. 2022; seervideoldm_amd/dpm.py's
docstring).  Nothing here reads the product's coefficient table or comes from a kernel.

  * levels / step64 / order_of / sampling64: the update, the order rule and a whole chain over a schedule given as its two abar tables;
  * ddim_sampling64: the eta = 0 DDIM chain over the same tables, to compare against;
  * gaussian: the analytic model -- data N(mu, s^2) per element has the exact eps, and its probability-flow ODE a closed-form end
    point -- and gaussian_errors, the figures the accuracy tests assert on;
  * cfg_dpm_step: an fp32 torch stand-in with the signature of seervideoldm_amd.ops, in the kernel's expression order (equal to the
    kernel to rounding, not to the bit).  With the names of tests/invert_ref.py, re-exported here, this module is a whole backend:
    `DPMSolverSampler("cpu", ops=tests.dpm_ref)` runs the host logic on the CPU."""
import math

import torch

from tests.invert_ref import (cfg_ddim_invert_step, cfg_ddim_step, cfg_ddim_step_rng, known_blend, philox_normal,  # noqa: F401
                              q_sample)

f64 = torch.float64


def levels(abar):
    """abar -> (alpha, sigma, lambda) in float64"""
    alpha, sigma = math.sqrt(float(abar)), math.sqrt(1.0 - float(abar))
    return alpha, sigma, math.log(alpha / sigma)


def h_of(alphas, alphas_prev, i):
    return levels(alphas_prev[i])[2] - levels(alphas[i])[2]


def step64(e, x, alphas, alphas_prev, i, order, d_prev=None):
    """one step at schedule entry i from the CFG-combined eps `e` -> (x_prev, D_i); d_prev = D_(i+1), read at order 2 only"""
    alpha_s, sigma_s, lam_s = levels(alphas[i])
    alpha_t, sigma_t, lam_t = levels(alphas_prev[i])
    h = lam_t - lam_s
    d = (x.to(f64) - sigma_s * e.to(f64)) / alpha_s
    dd = d
    if order == 2:
        r = h_of(alphas, alphas_prev, i + 1) / h
        dd = d + (d - d_prev.to(f64)) / (2.0 * r)
    return (sigma_t / sigma_s) * x.to(f64) - alpha_t * (math.exp(-h) - 1.0) * dd, d


def order_of(i, n, has_history, order=2, lower_order_final=True):
    """first order without history, with order = 1, and -- lower_order_final -- as the final step of a schedule of fewer than 15 entries"""
    if not has_history or order == 1:
        return 1
    return 1 if i == 0 and lower_order_final and n < 15 else 2


def sampling64(eps_fn, x_T, alphas, alphas_prev, timesteps, order=2, lower_order_final=True, t_start=None):
    """the chain over entries n - 1 ... 0 (t_start - 1 ... 0); eps_fn(x, t) is the CFG-combined model output at the long tensor t [b]
    -> (latent, [(x_prev, D, order) per step])"""
    n = len(timesteps)
    x, d_prev, steps = x_T.to(f64), None, []
    for i in reversed(range(n if t_start is None else int(t_start))):
        t = torch.full((x.shape[0],), int(timesteps[i]), dtype=torch.long)
        k = order_of(i, n, d_prev is not None, order, lower_order_final)
        x, d_prev = step64(eps_fn(x, t), x, alphas, alphas_prev, i, k, d_prev)
        steps.append((x, d_prev, k))
    return x, steps


def ddim_sampling64(eps_fn, x_T, alphas, alphas_prev, timesteps):
    """the deterministic DDIM chain in float64 -> the latent"""
    x = x_T.to(f64)
    for i in reversed(range(len(timesteps))):
        t = torch.full((x.shape[0],), int(timesteps[i]), dtype=torch.long)
        e = eps_fn(x, t).to(f64)
        x0 = (x - math.sqrt(1.0 - float(alphas[i])) * e) / math.sqrt(float(alphas[i]))
        x = math.sqrt(float(alphas_prev[i])) * x0 + math.sqrt(1.0 - float(alphas_prev[i])) * e
    return x


# ---- the analytic model -------------------------------------------------------------------------------------------------------------
MU, S = 0.3, 0.7


def gaussian(alphas_cumprod, mu=MU, s=S):
    """Data N(mu, s^2) per element: eps*(x, abar) = sigma (x - alpha mu) / (alpha^2 s^2 + sigma^2), and the probability-flow ODE
    carries x_T at abar_T to alpha_0 mu + sqrt(abar_0 s^2 + 1 - abar_0) / sqrt(abar_T s^2 + 1 - abar_T) (x_T - alpha_T mu) at abar_0.
    -> (eps(x, t) over the long tensor t, exact(x_T, abar_T, abar_0))"""
    ac = alphas_cumprod.to(f64)

    def eps(x, t):
        a = ac[t.cpu().long()].view(-1, *([1] * (x.dim() - 1)))
        return (1 - a).sqrt() * (x.to(f64) - a.sqrt() * mu) / (a * s * s + (1 - a))

    def exact(x_T, a_T, a_0):
        return math.sqrt(a_0) * mu + math.sqrt((a_0 * s * s + 1 - a_0) / (a_T * s * s + 1 - a_T)) * (x_T.to(f64) - math.sqrt(a_T) * mu)
    return eps, exact


def start_codes(shape=(1, 4, 1, 5, 10)):
    """x_T over [-3, 3], evenly spaced, as a latent"""
    n = 1
    for v in shape:
        n *= v
    return torch.linspace(-3.0, 3.0, n, dtype=f64).reshape(shape)


def max_error(latent, sampler, x_T):
    """max |latent - closed form| for a chain over the whole of `sampler`'s current schedule"""
    _, exact = gaussian(sampler.alphas_cumprod)
    a_T, a_0 = float(sampler.ddim_alphas[-1]), float(sampler.ddim_alphas_prev[0])
    return (latent.to(f64).cpu() - exact(x_T, a_T, a_0)).abs().max().item()


def assert_accuracy(err):
    """the three conditions of the accuracy tests on err[(method, grid, S)] -> max error; float64 gives 4.07 / 3.96, 0.23 and 0.35"""
    for grid in ("uniform", "logsnr"):
        ratio = err["2m", grid, 20] / err["2m", grid, 40]
        assert ratio >= 3.0, (grid, ratio, err)                                   # second order: half the step, a quarter of the error
    assert err["2m", "uniform", 50] <= err["ddim", "uniform", 50] / 3.0, err
    assert err["2m", "logsnr", 20] <= err["ddim", "uniform", 50] / 2.0, err


ACCURACY_CASES = [("2m", "uniform", 20), ("2m", "uniform", 40), ("2m", "uniform", 50), ("2m", "logsnr", 20), ("2m", "logsnr", 40),
                  ("ddim", "uniform", 50)]


# ---- the stand-in for seervideoldm_amd.ops ------------------------------------------------------------------------------------------
def cfg_dpm_step(eps, x, coef, index, order, *, cfg, scale, cond_f, d_prev=None, x_prev=None, pred_x0=None, want_pred_x0=True):
    if order not in (1, 2):
        raise ValueError(f"order {order}: 1 or 2")
    if not 0 <= int(index) < coef.shape[0]:
        raise ValueError(f"index {index}: the table has {coef.shape[0]} rows")
    if order == 2 and d_prev is None:
        raise ValueError("order 2 reads d_prev")
    b = x.shape[0]
    e = eps[:, :, cond_f:]
    e = e[:b] + scale * (e[b:] - e[:b]) if cfg else e
    row = coef[index]
    d = (x - row[0] * e) * row[1]
    new = row[2] * x + row[4] * d + row[5] * d_prev if order == 2 else row[2] * x + row[3] * d
    if x_prev is not None:
        x_prev.copy_(new)
        new = x_prev
    if pred_x0 is not None:
        pred_x0.copy_(d)
        d = pred_x0
    return new, (d if want_pred_x0 or pred_x0 is not None else None)
