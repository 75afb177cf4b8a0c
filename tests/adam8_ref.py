"""TEST INFRASTRUCTURE ONLY -- the 8-bit AdamW state format restated independently of the product (no import from
seervideoldm_amd): the two code books, a float64 emulation of one step with the rounding bounds the GPU test asserts, the same step
evaluated in fp32 with plain torch, and `Adam8Tops`, the CPU stand-in for `seervideoldm_amd.train_ops` that adds the two 8-bit entry
points to tests/torch_train_ops_backend.py without editing it.

The format (one block = 256 consecutive elements; per element the codes cm / cv, per block the scales absmax_m / absmax_v):
    gi   = g * coef                                       coef = min(1, max_norm / (sqrt(grad_sumsq) + 1e-6)), or 1
    m    = qmap_m[cm] * absmax_m ;  v = qmap_v[cv] * absmax_v
    m    = b1*m + (1-b1)*gi ;       v = b2*v + (1-b2)*gi*gi
    p    = p*(1 - lr*wd) - (lr/bc1) * m / (sqrt(v)/bc2_sqrt + eps)              with the UNquantised new m, v
    absmax_m' = max_block |m| ;     absmax_v' = max_block v
    cm'  = code of the qmap_m entry nearest to m/absmax_m' (the zero code if absmax_m' == 0) ;  cv' likewise
"""
from __future__ import annotations

import numpy as np
import torch

from tests import torch_train_ops_backend as _ttob

BLOCK = 256
U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
TINY = 2.0 ** -149      # the absolute rounding error of an fp32 operation whose result is subnormal
f64, f32 = torch.float64, torch.float32


def codebooks():
    """(qmap_m, qmap_v): float64 construction, sorted ascending, rounded to fp32 [256]"""
    out = []
    for signed in (True, False):
        vals = [0.0, 1.0]
        for i in range(7):
            n_i = 2 ** i + 1 if signed else 2 ** (i + 1) + 1
            b = np.linspace(0.1, 1.0, n_i, dtype=np.float64)
            mid = (b[:-1] + b[1:]) / 2
            vals += list(10.0 ** (i - 6) * mid)
            if signed:
                vals += list(-(10.0 ** (i - 6)) * mid)
        out.append(torch.from_numpy(np.sort(np.asarray(vals, dtype=np.float64))).to(f32))
    return tuple(out)


QMAP_M, QMAP_V = codebooks()


def hyper(lr, betas, eps, weight_decay, step):
    """the scalars as the kernel receives them: fp32 values (as float64 numbers); the bias corrections are computed in double on the
    host and passed as fp32"""
    r = lambda x: float(np.float32(x))
    b1, b2 = r(betas[0]), r(betas[1])
    return dict(lr=r(lr), b1=b1, b2=b2, eps=r(eps), wd=r(weight_decay), bc1=r(1.0 - b1 ** step), bc2s=r((1.0 - b2 ** step) ** 0.5))


def nearest_code(q: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """code of the entry of the sorted book q nearest to x (same dtype; a tie goes to the lower code)"""
    lo = (torch.searchsorted(q, x.contiguous(), right=True) - 1).clamp_(0, 255)
    hi = (lo + 1).clamp_(max=255)
    return torch.where(x - q[lo] > q[hi] - x, hi, lo)


def step_f64(p, g, cm, cv, am, av, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, step, grad_sumsq=None, max_norm=1.0):
    """One step in float64 from the fp32 / uint8 inputs (CPU tensors; nothing is modified).  Returns a dict with the float64 results
    p, m, v (new, unquantised), absmax_m, absmax_v (block maxima), and the rounding bounds of an fp32 evaluation:

      bound_m = 9 U (|b1 m0| + |(1-b1) gi|)        roundings: q*absmax, b1*, [sqrt, +1e-6, / of coef], g*coef, 1-b1, *, +
      bound_v = 13 U (b2 v0 + (1-b2) gi^2)         q*absmax, b2*, coef (3), g*coef, 1-b2, *gi, *gi (gi's 4 roundings enter twice), +
      bound_p = U (4 |A| + 14 |B|) + (lr/bc1) / denom * bound_m,   A = p (1 - lr wd),  B = (lr/bc1) m / denom,
                denom = sqrt(v)/bc2_sqrt + eps:    A: lr*wd, 1-, *, and the final subtraction;  B: lr/bc1, sqrt, /bc2_sqrt, +eps,
                m/denom, the product, the final subtraction, and v's relative error 13 U halved by the square root (v is a sum of
                non-negative terms, so bound_v / v <= 13 U); m's error is absolute (its two terms can cancel) and passes through
                the factor (lr/bc1) / denom
    each plus the same count of subnormal-result errors (2^-149).  A fused multiply-add only removes roundings."""
    h = hyper(lr, betas, eps, weight_decay, step)
    d = lambda t: t.to(f64)
    coef = 1.0
    if grad_sumsq is not None:
        coef = min(1.0, float(np.float32(max_norm)) / (float(grad_sumsq.to(f64).reshape(())) ** 0.5 + float(np.float32(1e-6))))
    rep = lambda a: a.repeat_interleave(BLOCK)
    gi = d(g) * coef
    m0 = d(QMAP_M)[cm.long()] * rep(d(am))
    v0 = d(QMAP_V)[cv.long()] * rep(d(av))
    t1, t2 = h["b1"] * m0, (1.0 - h["b1"]) * gi
    s1, s2 = h["b2"] * v0, (1.0 - h["b2"]) * gi * gi
    m, v = t1 + t2, s1 + s2
    A = d(p) * (1.0 - h["lr"] * h["wd"])
    denom = v.sqrt() / h["bc2s"] + h["eps"]
    B = (h["lr"] / h["bc1"]) * m / denom
    bound_m = 9 * U * (t1.abs() + t2.abs()) + 9 * TINY
    bound_v = 13 * U * (s1 + s2) + 13 * TINY
    bound_p = U * (4 * A.abs() + 14 * B.abs()) + (h["lr"] / h["bc1"]) / denom * bound_m + 18 * TINY
    blk = lambda t: t.reshape(-1, BLOCK)
    return dict(p=A - B, m=m, v=v, absmax_m=blk(m.abs()).max(1).values, absmax_v=blk(v).max(1).values,
                bound_m=bound_m, bound_v=bound_v, bound_p=bound_p,
                bound_absmax_m=blk(bound_m).max(1).values, bound_absmax_v=blk(bound_v).max(1).values)


def check_against_f64(ref, p, cm, cv, am, av, p_bf16=None):
    """Every output of one step (CPU tensors: fp32 p, uint8 codes, fp32 scales, optional bf16 copy) against step_f64's result; no
    element is excluded.  Returns a list of violations (empty = pass), each (what, worst excess, index).
      scales: |absmax' - float64 block maximum| <= the largest element bound of the block (|max a - max b| <= max |a - b|)
      codes:  |qmap[c] absmax' - x64| <= min_k |qmap[k] absmax' - x64| + 2 bound_x + 3 U absmax'   with absmax' the scale under test:
              the kernel takes the nearest entry to r = fl(x32 / absmax'), so |q[c] - r| <= min_k |q[k] - r| + U (q[hi] - q[lo]) (the
              two fp32 differences it compares); times absmax', and x64 in the place of r absmax' = x32 (1 + delta) on both sides
              costs 2 (|x32 - x64| + U |x32|); |x32| <= absmax' and q[hi] - q[lo] <= 1 give the 3 U absmax'
      p:      within bound_p;   p_bf16: within bound_p + 2^-8 (|p64| + bound_p)   (bf16 keeps 8 significand bits: unit roundoff 2^-8)"""
    bad = []

    def over(what, err, bound):
        ex = err - bound
        if not bool(torch.isfinite(err).all()) or float(ex.max()) > 0:
            i = int(torch.where(torch.isfinite(ex), ex, torch.full_like(ex, float("inf"))).argmax())
            bad.append((what, float(err[i]), float(bound[i]), i))

    over("absmax_m", (am.to(f64) - ref["absmax_m"]).abs(), ref["bound_absmax_m"])
    over("absmax_v", (av.to(f64) - ref["absmax_v"]).abs(), ref["bound_absmax_v"])
    for what, q, c, a, x, bx in (("cm", QMAP_M, cm, am, ref["m"], ref["bound_m"]), ("cv", QMAP_V, cv, av, ref["v"], ref["bound_v"])):
        q64, A = q.to(f64), a.to(f64).repeat_interleave(BLOCK)
        got = (q64[c.long()] * A - x).abs()
        r = torch.where(A > 0, x / A, torch.zeros_like(x))
        lo = (torch.searchsorted(q64, r.contiguous(), right=True) - 1).clamp_(0, 255)     # the nearest entry is one of the two
        hi = (lo + 1).clamp_(max=255)                                                      # that enclose x / absmax'
        best = torch.minimum((q64[lo] * A - x).abs(), (q64[hi] * A - x).abs())
        over(what, got, best + 2 * bx + 3 * U * A)
    over("p", (p.to(f64) - ref["p"]).abs(), ref["bound_p"])
    if p_bf16 is not None:
        over("p_bf16", (p_bf16.to(f64) - ref["p"]).abs(), ref["bound_p"] + 2.0 ** -8 * (ref["p"].abs() + ref["bound_p"]))
    return bad


def adamw8_step(p, g, cm, cv, absmax_m, absmax_v, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, step, grad_sumsq=None,
                max_norm=1.0, p_bf16=None):
    """the step in fp32 with plain torch, in place (the call signature of seervideoldm_amd.train_ops.adamw8_step): one rounding per
    operation, in the kernel's order"""
    h = {k: torch.tensor(v, dtype=f32) for k, v in hyper(lr, betas, eps, weight_decay, step).items()}
    one = torch.tensor(1.0, dtype=f32)
    coef = one
    if grad_sumsq is not None:
        coef = torch.minimum(one, torch.tensor(max_norm, dtype=f32) / (grad_sumsq.to(f32).reshape(()).sqrt() + torch.tensor(1e-6, dtype=f32)))
    rep = lambda a: a.repeat_interleave(BLOCK)
    gi = g * coef
    m = h["b1"] * (QMAP_M[cm.long()] * rep(absmax_m)) + (one - h["b1"]) * gi
    v = h["b2"] * (QMAP_V[cv.long()] * rep(absmax_v)) + (one - h["b2"]) * gi * gi
    denom = v.sqrt() / h["bc2s"] + h["eps"]
    p.copy_(p * (one - h["lr"] * h["wd"]) - (h["lr"] / h["bc1"]) * (m / denom))
    fin = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))      # non-finite values stay out of the block maximum
    am = fin(m.abs()).reshape(-1, BLOCK).max(1).values
    av = fin(v).reshape(-1, BLOCK).max(1).values
    A, V = rep(am), rep(av)
    cm.copy_(torch.where(A > 0, nearest_code(QMAP_M, m / A), torch.full_like(cm, 127, dtype=torch.long)).to(torch.uint8))
    cv.copy_(torch.where(V > 0, nearest_code(QMAP_V, v / V), torch.zeros_like(cv, dtype=torch.long)).to(torch.uint8))
    absmax_m.copy_(am)
    absmax_v.copy_(av)
    if p_bf16 is not None:
        p_bf16.copy_(p.to(torch.bfloat16))


def random_state(n, seed, device="cpu"):
    """a random valid state and inputs for n elements: codes uniform over 0..255, scales log-uniform in [1e-12, 1e3], p ~ N(0, 1),
    g ~ N(0, 1) times a per-block magnitude log-uniform in [1e-4, 10]"""
    gen = torch.Generator().manual_seed(seed)
    nb = n // BLOCK
    logu = lambda lo, hi, k: torch.exp(torch.rand((k,), generator=gen, dtype=f64) * (np.log(hi) - np.log(lo)) + np.log(lo)).to(f32)
    p = torch.randn((n,), generator=gen)
    g = torch.randn((n,), generator=gen) * logu(1e-4, 10.0, nb).repeat_interleave(BLOCK)
    cm = torch.randint(0, 256, (n,), generator=gen).to(torch.uint8)
    cv = torch.randint(0, 256, (n,), generator=gen).to(torch.uint8)
    am, av = logu(1e-12, 1e3, nb), logu(1e-12, 1e3, nb)
    return tuple(t.to(device) for t in (p, g, cm, cv, am, av))


class Adam8Tops:
    """tests.torch_train_ops_backend plus the two 8-bit entry points, in plain torch: the `tops` of a CPU SeerTrainer with
    use_8bit_adam=True"""

    adamw8_step = staticmethod(adamw8_step)

    @staticmethod
    def adam8_qmaps(device):
        return QMAP_M.to(device), QMAP_V.to(device)

    def __getattr__(self, name):
        return getattr(_ttob, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# The 8-bit mode against the fp32 mode over several steps of the tiny trainer, on the CPU stand-ins.  The GPU test asserts its own
# figure against this one (tests/golden/adam8_movement_cpu.json, written by `python -m tests.adam8_ref`): the CPU run takes a minute.
TINY_CFG = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=192, attention_head_dim=8)
TINY_HP = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=0.3)
GOLDEN_MOVEMENT = "adam8_movement_cpu.json"


def tiny_batch(H):
    rn = lambda shape, seed: torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return rn((1, 4, 3, H, H), 1), rn((1, 4, 2, H, H), 2), torch.tensor([417]), rn((1, 77, 192), 3)


def flat_params(tr):
    sd = tr.trainable_state_dict()
    return torch.cat([sd[s][k].reshape(-1) for s in ("unet", "fstext") for k in sd[s]]).double().cpu()


def movement_distance(p0, p_fp32, p_8bit):
    """relative L2 distance of the parameter movement of the two modes: |(p8 - p0) - (p32 - p0)| / |p32 - p0|"""
    return float((p_8bit - p_fp32).norm() / (p_fp32 - p0).norm())


def movement_cpu(H, steps):
    """`steps` optimizer steps of the tiny trainer on one fixed batch in both modes, on the plain-torch stand-ins"""
    from seervideoldm_amd import FSTextTransformer, SeerUNet, synth
    from seervideoldm_amd.trainer import SeerTrainer
    from tests import torch_ops_backend as tob
    x, noise, t, text = tiny_batch(H)
    out = {}
    for mode in (False, True):
        unet = SeerUNet(**TINY_CFG)
        unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(TINY_CFG)), strict=True)
        fst = FSTextTransformer(num_frames=16, in_channels=192, out_channels=192, n_heads=2, num_layers=1, cross_attention_dim=192)
        fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(num_frames=16, num_layers=1, channels=192, n_heads=2,
                                                                             cross_attention_dim=192)), strict=True)
        fst.set_numframe(3)
        tr = SeerTrainer(unet, fst, ops=tob, tops=Adam8Tops() if mode else _ttob, use_8bit_adam=mode, **TINY_HP)
        out["p0"] = flat_params(tr)
        for _ in range(steps):
            tr.forward_backward(x, noise, t, text, 1)
            tr.optimizer_step()
        out[mode] = flat_params(tr)
    return movement_distance(out["p0"], out[False], out[True])


if __name__ == "__main__":
    import json
    from pathlib import Path
    res = {f"H{H}_steps{n}": movement_cpu(H, n) for H, n in ((8, 2), (16, 8))}
    (Path(__file__).parent / "golden" / GOLDEN_MOVEMENT).write_text(json.dumps(res, indent=1) + "\n")
    print(res)
