"""Step caching -- the host policy (SeerUNet.enable_step_cache; DESIGN.md "Step caching").  Host only: no tensor, no kernel.

A chain of model evaluations k = 0, 1, ... runs in full when k % interval == 0 (phase 0: the engine also pushes the cut feature
into its three-slot ring) and cached otherwise (phase d = k % interval: the engine forecasts the cut feature from the ring and runs the
shallow layers around it).  The forecast is a weighted sum of the ring's slots, slot 0 the newest; the full evaluations are
`interval` apart, so with u = d / interval the feature at u intervals past the newest one is

    order 0   f0                                                     reuse (DeepCache)
    order 1   f0 + u (f0 - f1)                                       linear extrapolation
    order 2   f0 + u (f0 - f1) + u (u + 1) / 2 (f0 - 2 f1 + f2)      Newton's backward-difference form: exact for a quadratic

(TaylorSeer's forecast, in finite differences of the kept features).  The effective order is min(order, valid slots - 1): the first
interval after a chain starts reuses, the second extrapolates linearly.  interval and order are policy: no captured graph depends
on them, the three weights reach the kernel through a device buffer.
"""
from __future__ import annotations

import struct
from typing import Optional, Tuple

RING_SLOTS = 3


def forecast_weights(d: int, interval: int, order: int, valid: int) -> Tuple[float, float, float]:
    """(w0, w1, w2) of phase d: float64 arithmetic, each rounded to fp32 (and returned as the Python float of that fp32 value).
    valid: the ring's slots that hold a feature of this chain, 1 .. 3."""
    if d < 1 or interval < 1 or valid < 1:
        raise ValueError(f"forecast_weights: d = {d}, interval = {interval}, valid = {valid}: a cached phase d >= 1 with a valid slot")
    o = min(int(order), int(valid) - 1, RING_SLOTS - 1)
    u = float(d) / float(interval)
    if o <= 0:
        w = (1.0, 0.0, 0.0)
    elif o == 1:
        w = (1.0 + u, -u, 0.0)
    else:
        q = u * (u + 1.0)
        w = (1.0 + u + q / 2.0, -u - q, q / 2.0)
    return tuple(struct.unpack("f", struct.pack("f", v))[0] for v in w)


class StepCachePolicy:
    """interval / branch / order of an enabled step cache, and where a chain stands: begin() starts a chain, next() is called once per
    model evaluation and returns (phase, weights) -- weights None for a full evaluation."""

    def __init__(self, interval: int = 3, branch: int = 1, order: int = 1):
        self.interval, self.branch, self.order = int(interval), int(branch), int(order)
        self.k = 0              # evaluations of the chain so far
        self.valid = 0          # full evaluations of the chain so far, at most the ring's slots

    def begin(self) -> None:
        self.k = 0
        self.valid = 0

    def weights(self, d: int, valid: int) -> Tuple[float, float, float]:
        return forecast_weights(d, self.interval, self.order, valid)

    def next(self) -> Tuple[int, Optional[Tuple[float, float, float]]]:
        d = self.k % self.interval
        self.k += 1
        if d == 0:
            self.valid = min(self.valid + 1, RING_SLOTS)
            return 0, None
        return d, self.weights(d, self.valid)


def policy_of(model) -> Optional[StepCachePolicy]:
    """the policy a sampler drives for `model`, or None: only a SeerUNet with the cache enabled has one (a plain callable is called
    as it always was, without the keyword)"""
    from .unet import SeerUNet
    return model._step_cache if isinstance(model, SeerUNet) else None


def refuse(model, what: str) -> None:
    """what does not run while the model's step cache is enabled"""
    if policy_of(model) is not None:
        raise ValueError(f"{what}: the model's step cache is enabled (per-slot phases are not built); call disable_step_cache() first")
