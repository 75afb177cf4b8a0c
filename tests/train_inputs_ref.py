"""Helpers of the step_from_batch tests (NOT a product path):

* `reference(...)`: the float64 evaluation of seer_train_inputs' formula from the same fp32 inputs, with the per-element error bound
  of the kernel's fp32 arithmetic;
* `TrainOpsWithInputs`: the plain-torch training stand-ins of tests/torch_train_ops_backend.py plus a `train_inputs` stand-in, so that
  SeerTrainer.step_from_batch's host logic runs on the CPU; it records the calls it receives.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import torch_train_ops_backend as ttob

# Every term of an output element passes through at most eight fp32 operations, each rounded to within 1 ulp (expf taken at 2):
# sixteen half-ulps of the term's magnitude.
REL = 2.0 ** -20


def reference(moments, eps_post, noise, timesteps, alphas_cumprod, f1, latent_scale):
    """moments fp32 [b*F, 2C, h, w], eps_post fp32 [b*F, C, h, w] or None, noise fp32 [b, C, f2, h, w], timesteps int64 [b],
    alphas_cumprod fp32 [T] (all on the CPU) -> (model_input [b, C, F, h, w], latents [b, C, f2, h, w], bound like model_input, bound
    like latents), float64:
        z = mean + exp(0.5 * clamp(logvar, -30, 20)) * eps,   lat = z * scale,
        f < f1: lat;   f >= f1: sqrt(a) * lat + sqrt(1 - a) * noise,   a = alphas_cumprod[t[b]]
        bound = 2^-20 * (sqrt(a) * scale * (|mean| + |std * eps|) + sqrt(1 - a) * |noise|)
    with sqrt(a) = 1 and no noise term for the conditioning frames and for the clean latents"""
    b, C, f2, h, w = noise.shape
    F = f1 + f2
    m = moments.double().reshape(b, F, 2 * C, h, w)
    mean, logvar = m[:, :, :C], m[:, :, C:].clamp(-30.0, 20.0)
    se = torch.zeros_like(mean) if eps_post is None else torch.exp(0.5 * logvar) * eps_post.double().reshape(b, F, C, h, w)
    scale = float(np.float32(latent_scale))                     # the fp32 value the kernel multiplies by
    lat = ((mean + se) * scale).permute(0, 2, 1, 3, 4)          # [b, C, F, h, w]
    mag = (scale * (mean.abs() + se.abs())).permute(0, 2, 1, 3, 4)
    a = alphas_cumprod.double()[timesteps].reshape(b, 1, 1, 1, 1)
    sa, sb = a.sqrt(), (1.0 - a).sqrt()
    x, bound = lat.clone(), REL * mag
    x[:, :, f1:] = sa * lat[:, :, f1:] + sb * noise.double()
    bound[:, :, f1:] = REL * (sa * mag[:, :, f1:] + sb * noise.double().abs())
    return x.contiguous(), lat[:, :, f1:].contiguous(), bound.contiguous(), (REL * mag[:, :, f1:]).contiguous()


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (an element with bound 0 must be exact)"""
    err = (got.double().cpu() - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err[bound > 0] / bound[bound > 0]).max())


class TrainOpsWithInputs:
    """tests/torch_train_ops_backend.py (every attribute it has) + `train_inputs` in plain torch; `calls` lists the train_inputs calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return getattr(ttob, name)

    def train_inputs(self, moments, eps_post, noise, timesteps, alphas_cumprod, cond_frames, latent_scale=0.18215, *, out=None,
                     latents=None, _timesteps_in_range=False):
        T = alphas_cumprod.numel()
        if not _timesteps_in_range and (int(timesteps.min()) < 0 or int(timesteps.max()) >= T):
            raise ValueError(f"train_inputs: timesteps must lie in [0, {T})")
        self.calls.append(dict(moments=moments, eps_post=eps_post, noise=noise, timesteps=timesteps, cond_frames=cond_frames,
                               latent_scale=latent_scale, _timesteps_in_range=_timesteps_in_range))
        x, lat, _, _ = reference(moments, eps_post, noise, timesteps, alphas_cumprod, cond_frames, latent_scale)
        if latents is not None:
            latents.copy_(lat)
        if out is None:
            return x.float()
        out.copy_(x)
        return out
