"""Guidance rescale restated (include/seer_hip.h, "guidance rescale": seer_cfg_rescale, seer_slot_cfg_rescale), in float64 from the
definition and as fp32 torch stand-ins with the signatures of seervideoldm_amd.ops.  Nothing here comes from a kernel.

  * multiplier64 / rescale64: the pinned definition, m = phi sqrt(q_c / q_g) + (1 - phi) with q = n S2 - S1^2 per clip, and m g;
    textbook64: diffusers' rescale_noise_cfg, with unbiased stds over all non-batch dims;
  * cfg_rescale / slot_cfg_rescale / cfg_rescale_workspace: the stand-ins -- the guided value as the update stand-ins combine it (fp32),
    the four sums in float64 of those fp32 values, m rounded to fp32 once, one fp32 product; equal to the kernel to rounding (the
    kernel may contract the combine into an FMA), not to the bit;
  * backend(*modules): this module's stand-ins in front of tests/vpred_ref.backend(*modules);
  * RescaledRows: a CFG pair of model rows with the float64 multiplier folded into both, for tests/vpred_ref.chain64."""
import numpy as np
import torch

from tests import vpred_ref as V

f64 = torch.float64
STAND_INS = ("cfg_rescale", "slot_cfg_rescale", "cfg_rescale_workspace")


def widened(phi) -> float:
    """phi as the kernels see it: rounded to fp32 (a kernel argument, or a word of the slots' buffer), then widened"""
    return float(np.float32(phi))


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def multiplier64(g, c, phi):
    """g, c [b, ...] (the predicted frames only) -> m float64 [b, 1, ..., 1]; 1 where q_g <= 0 or the ratio is not finite"""
    g, c = g.to(f64), c.to(f64)
    dims = tuple(range(1, g.dim()))
    n = float(g[0].numel())
    q_c = (n * (c * c).sum(dims, keepdim=True) - c.sum(dims, keepdim=True) ** 2).clamp_min(0.0)
    q_g = n * (g * g).sum(dims, keepdim=True) - g.sum(dims, keepdim=True) ** 2
    ratio = q_c / torch.where(q_g > 0, q_g, torch.ones_like(q_g))
    phi = widened(phi)
    m = phi * ratio.sqrt() + (1.0 - phi)
    return torch.where((q_g > 0) & torch.isfinite(ratio), m, torch.ones_like(m))


def rescale64(g, c, phi):
    return multiplier64(g, c, phi) * g.to(f64)


def textbook64(g, c, phi):
    """rescale_noise_cfg(noise_cfg=g, noise_pred_text=c, guidance_rescale=phi) of diffusers, in float64"""
    g, c = g.to(f64), c.to(f64)
    dims = list(range(1, g.dim()))
    rescaled = g * (c.std(dim=dims, keepdim=True) / g.std(dim=dims, keepdim=True))
    return phi * rescaled + (1.0 - phi) * g


# ---- the stand-ins --------------------------------------------------------------------------------------------------------------------
def cfg_rescale_workspace(clips, C, F_total, cond_f, HW, device):
    from seervideoldm_amd.ops import RESCALE_TILE
    n = int(C) * (int(F_total) - int(cond_f)) * int(HW)
    return torch.full((int(clips) * ((n + RESCALE_TILE - 1) // RESCALE_TILE) * 4,), float("nan"), dtype=f64, device=device)


def _pair(eu, ec, scale, phi):
    """-> (m fp32 [b], m g fp32) of the rows eu, ec [b, C, F_pred, h, w]"""
    g = eu + scale * (ec - eu)                           # the update stand-ins' own expression (tests/*_ref.py)
    m = multiplier64(g, ec, phi).to(torch.float32)
    return m.reshape(-1), m * g


def cfg_rescale(out, *, scale, rescale, cond_f, ws=None, mult=None):
    from seervideoldm_amd.ops import check_guidance_rescale
    phi = check_guidance_rescale(rescale)
    assert out.dtype == torch.float32 and out.dim() == 5 and out.shape[0] % 2 == 0 and 0 <= cond_f < out.shape[2]
    if phi == 0.0:
        return out
    b = out.shape[0] // 2
    m, v = _pair(out[:b, :, cond_f:], out[b:, :, cond_f:], scale, phi)
    out[:b, :, cond_f:] = v
    out[b:, :, cond_f:] = v
    if mult is not None:
        mult.copy_(m)
    return out


def slot_cfg_rescale(out, scale, rescale, coef, step, *, cond_f, ws=None, mult=None):
    slots, nsched = out.shape[0] // 2, coef.shape[1]
    assert tuple(step.shape) == (slots, 2) and scale.numel() == slots and rescale.numel() == slots and rescale.dtype == torch.float32
    for s in range(slots):
        index, phi = int(step[s, 1]), float(rescale[s])
        if index < 0 or index >= nsched or phi == 0.0:
            continue                                    # idle, or a plain clip: no word of the slot is written
        m, v = _pair(out[s:s + 1, :, cond_f:], out[slots + s:slots + s + 1, :, cond_f:], float(scale[s]), phi)
        out[s:s + 1, :, cond_f:] = v
        out[slots + s:slots + s + 1, :, cond_f:] = v
        if mult is not None:
            mult[s] = m[0]
    return out


class _Backend:
    def __init__(self, modules):
        self._inner = V.backend(*modules)

    def __getattr__(self, name):
        if name in STAND_INS:
            return globals()[name]
        return getattr(self._inner, name)


def backend(*modules):
    """an `ops=` backend: this module's stand-ins, then tests/vpred_ref's, then every name of `modules`, first match first"""
    return _Backend(modules)


# ---- for the float64 chains -----------------------------------------------------------------------------------------------------------
class RescaledRows:
    """model_rows of tests/vpred_ref.chain64 with guidance rescale: the raw pair (uc, c) of every evaluation is returned as (m uc, m c),
    m = multiplier64 of its guided value -- chain64's own combine of that pair is m g, its conversion of a v-pair is the conversion of
    m v, and the operand magnitudes it sums are m times those of the unscaled combine.  `freeze()` keeps the multipliers of the run made
    so far and replays them, evaluation by evaluation, in every later run: the chain is then affine in each of its quantities again,
    which is what chain64's unit bumps need."""

    def __init__(self, rows, scale, phi):
        self.rows, self.scale, self.phi = rows, float(scale), phi
        self.made, self.frozen, self.k = [], None, 0

    def freeze(self):
        self.frozen = list(self.made)

    def restart(self):
        self.k = 0
        if self.frozen is None:
            self.made = []

    def __call__(self, x, row):
        uc, c = self.rows(x, row)
        if self.frozen is None:
            m = multiplier64(uc + self.scale * (c - uc), c, self.phi)
            self.made.append(m)
        else:
            m = self.frozen[self.k]
        self.k += 1
        return m * uc, m * c
