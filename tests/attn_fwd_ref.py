"""TEST INFRASTRUCTURE ONLY -- seer_attn_fwd restated in float64 torch, independently of the product (no import from seervideoldm_amd),
for tests/test_gpu_attn_fwd_matrix.py (the kernels) and tests/test_attn_fwd_ref_cpu.py (the constructions, without a GPU).  No tests here.

Three things:

1. `kernel_kind`: which of the three forward code paths a launch takes, restated from the dispatch in csrc/attention.hip (seer_attn_fwd)
   and csrc/attention40.hip (seer_attn40_launch).  It only selects the roundings of the emulation:
     "generic"    seer_attn_kernel<D>: fp32 scores scaled by fp32(scale) * fp32(log2 e), P rounded to nearest, O rounded
     "a40_track"  seer_attn40_kernel<.., TRACK_ONLY>: q * fp32(scale * log2 e) rounded to the storage type first (unless prescaled),
                  P rounded to nearest, O rounded
     "a40_fast"   seer_attn40_kernel fast path (variants 2, 3, 7 and what AUTO picks from 256 keys up, bf16, no lse): the same q rounding,
                  P TRUNCATED to bf16 (v_perm_b32 of the high halves), O rounded
   The denominator: wherever the kernel takes it out of the P V product (a ones column of V': the d = 40 kernel, and the generic kernel
   at head_dim 40 and 80, whose last 32-row tile of O^T has spare rows) it is the sum of the ROUNDED P; at head_dim 96 and 160 the
   generic kernel adds the unrounded fp32 P.  The emulation does the same (`l_rounded`): this is the one rounding the training
   matrix's emulation of the forward does not have, and with few keys it is what a row's error consists of.
2. `emulate`: the float64 softmax formula (the reference) and the emulation that rounds only where the kernels round, with the
   MUTATIONS of the mutation table applied to the emulation on request.
3. The exact Part 1 constructions (`uniform_v`, `ramp_v`) with their preconditions, and the derived lse allowance (`lse_allowance`).
"""
from __future__ import annotations

import torch

from tests.test_gpu_f16_matrix import _exact_pre, _ints, _rand, _store
from tests.test_gpu_train_matrix import _Plain, _r16, _Strided, _Window

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
LOG2E = 1.4426950408889634
U32 = 2.0 ** -24
KT = {"generic": 64, "a40_track": 128, "a40_fast": 128}      # keys per LDS tile / stage (KT, A40_KT)
MUTATIONS = ("drop_last", "drop_tile_first", "double", "admit_masked", "diag+1", "diag-1", "other_window", "ignore_offset", "skip_p_round")


def kernel_kind(d, variant, dt, Sk, lse=False, prescaled=False):
    if d != 40:
        return "generic"
    if dt == f16:
        return "generic" if variant == 1 or (variant == 0 and Sk < 256) else "a40_track"
    if variant in (1, 6) or (variant == 0 and Sk < 256) or (variant == 0 and lse and not prescaled):
        return "generic"
    return "a40_track" if (variant == 5 or lse) else "a40_fast"


def l_rounded(kind, d):
    return kind != "generic" or d in (40, 80)


def rnd(x64, dt):
    """one round-to-nearest-even to the storage type, back in float64"""
    return _r16(x64) if dt == bf16 else x64.to(dt).to(f64)


def trunc_bf16(x64):
    """the high 16 bits of the fp32 value (what the fast path's v_perm_b32 keeps), back in float64"""
    return (x64.to(f32).view(torch.int32) & -65536).view(f32).to(f64)


def scale32(scale):
    """the descriptor's scale field is a float"""
    return float(torch.tensor(scale, dtype=f32))


def visible(Sq, Sk, causal, off, dev):
    if not causal:
        return torch.ones((Sq, Sk), dtype=torch.bool, device=dev)
    return torch.arange(Sk, device=dev)[None, :] <= torch.arange(Sq, device=dev)[:, None] + off


def scores(q, k, *, scale, dt, kind, prescaled):
    """[B', heads, S, d] float64 -> (reference scores, the emulation's scores), log2 domain, unmasked.  The reference uses the fp32 value of
    `scale` (an input, stored as a float) times log2 e; the emulation multiplies where the kernel does"""
    qk = q @ k.transpose(-1, -2)
    if prescaled:
        return qk, qk
    c32 = torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)         # cscale = p.scale * 1.4426950408889634f
    if kind == "generic":
        return qk * (scale32(scale) * LOG2E), qk * float(c32)
    qs = (q.to(f32) * c32).to(dt).to(f64)                                           # include/seer_hip.h at SEER_ATTN_Q_PRESCALED
    return qk * (scale32(scale) * LOG2E), qs @ k.transpose(-1, -2)


class Emu:
    """o_ref: the float64 formula; o: the emulation (rounded to the storage type); s: the emulation's masked scores; lse: float64
    log2-sum-exp2 of s; n: visible keys per query"""


def emulate(q, k, v, *, scale, dt, kind, prescaled=False, causal=False, off=0, mut=None, windows=1):
    """q, k, v: [B', heads, S, d] float64, already rounded to the storage type (B' = windows x batch, window-major).  `mut`: one of MUTATIONS,
    applied to the EMULATION only (the reference stays the operation asked for); returns None where the mutation does not apply"""
    d, Sq, Sk, dev = q.shape[-1], q.shape[2], k.shape[2], q.device
    vis_ref = visible(Sq, Sk, causal, off, dev)
    ke, ve, off_e = k, v, off
    if mut == "other_window":
        if windows < 2:
            return None
        ke, ve = k.roll(k.shape[0] // windows, 0), v.roll(v.shape[0] // windows, 0)
    if mut in ("diag+1", "diag-1", "ignore_offset"):
        if not causal or (mut == "ignore_offset" and off == 0):
            return None
        off_e = 0 if mut == "ignore_offset" else off + (1 if mut == "diag+1" else -1)
    vis = visible(Sq, Sk, causal, off_e, dev)
    w = vis.to(f64)                                     # how often a key is counted
    if mut == "diag+1" and bool((w == vis_ref.to(f64)).all()):
        return None                                     # every query already sees every key
    if mut == "drop_last":
        if not bool(vis[:, Sk - 1].any()) or Sk < 2:
            return None
        w[:, Sk - 1] = 0
    if mut == "drop_tile_first":
        j = (Sk - 1) // KT[kind] * KT[kind]
        if not bool(vis[:, j].any()) or Sk < 2 or j == Sk - 1:
            return None
        w[:, j] = 0
    if mut == "double":                                 # (one key alone, counted twice, is the same softmax)
        if not bool(vis[:, Sk // 2].any()) or Sk < 2:
            return None
        w[:, Sk // 2] *= 2
    s_ref, s_emu = scores(q, k, scale=scale, dt=dt, kind=kind, prescaled=prescaled)
    if ke is not k:
        s_emu = scores(q, ke, scale=scale, dt=dt, kind=kind, prescaled=prescaled)[1]
    r = Emu()
    r.n = vis_ref.sum(-1)
    sr = s_ref.masked_fill(~vis_ref, float("-inf"))
    pr = torch.exp2(sr - sr.max(-1, keepdim=True).values)
    r.o_ref = (pr @ v) / pr.sum(-1, keepdim=True)
    r.s = s_emu.masked_fill(~vis, float("-inf"))
    m = r.s.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)          # a query without a key: the kernels write zeros
    p0 = torch.exp2(r.s - m) * w
    p16 = p0 if mut == "skip_p_round" else (trunc_bf16(p0) if kind == "a40_fast" else rnd(p0, dt))
    l = (p16 if l_rounded(kind, d) else p0).sum(-1, keepdim=True)
    if mut == "admit_masked":                           # a padded key that escapes its mask with P = 1 (the largest P of the row is 1) and V = 0
        if Sk % KT[kind] == 0:
            return None
        l = l + 1.0
    r.l0 = p0.sum(-1, keepdim=True)
    r.m = m
    r.lse = (m + torch.log2(r.l0)).squeeze(-1)
    r.o = rnd(torch.where(l > 0, (p16 @ ve) / l.clamp_min(1e-300), torch.zeros_like(l)), dt)
    return r


def row_floor(ref):
    """2^-6 of the tensor's rms row norm"""
    return 2.0 ** -6 * float(ref.norm(dim=-1).pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------- Part 1: exact constructions
def _signed(shape, dev, seed, lo, hi):
    return _ints(shape, dev, seed, lo, hi) * (2 * _ints(shape, dev, seed + 1000, 0, 1) - 1)


def uniform_v(Bp, Hh, Sk, d, dev, dt, seed=0, shift=0):
    """Q = 0, not causal: every P is 2^0 and O[i] = mean_j V[j].  Even columns BALANCE: (w, -w) pairs, |w| in [1, 100], mean 0 (odd Sk: the
    unpaired key holds 0 -- the last one, or with shift = 1 the first).  Odd columns LEVEL: V = c for every key, |c| in [lo, 255] with
    lo = max(128, Sk // 2 + 2), so that c n / (n + 1) -- one more key admitted with weight 1 and V = 0 -- rounds to another value than c
    (asserted for Sk <= 400: c / (n + 1) exceeds half an ulp of c).  -> (v [B', heads, Sk, d], the expected O row [B', heads, 1, d])"""
    w = _signed((Bp, Hh, Sk // 2, d), dev, seed + 1, 1, 100)
    bal = torch.zeros((Bp, Hh, Sk, d), device=dev, dtype=f64)
    bal[:, :, shift:shift + 2 * (Sk // 2)] = torch.stack([w, -w], 3).reshape(Bp, Hh, 2 * (Sk // 2), d)
    c = _signed((Bp, Hh, 1, d), dev, seed + 2, max(128, Sk // 2 + 2), 255)
    level = (torch.arange(d, device=dev) % 2 == 1)
    v = torch.where(level, c.expand(Bp, Hh, Sk, d), bal)
    want = torch.where(level, c, torch.zeros_like(c))
    _store(v, dt), _store(want, dt)
    _exact_pre(Sk, 255, 1)
    if Sk <= 400:
        moved = rnd(c * Sk / (Sk + 1), dt) != c
        assert bool(moved.all()), "a level column would not see one more key in the denominator"
    return v, want


RAMP_A = (1.0, -1.0, 0.5, -0.5, 0.25, -0.25)


def ramp_v(batch, Hh, Sq, Sk, d, dev, dt, off=0, windows=1):
    """Q = 0, causal: query i sees n_i = i + off + 1 keys with P = 2^0 each, and with V[j] = c + 2 a j per column O[i] = c + a (n_i - 1).
    a cycles through +-1, +-1/2, +-1/4 over the columns; c is the multiple of 2 |a| that centres the O range on zero (up to 64 visible
    keys: on 128 |a|), so that V (a grid of 2 |a|, at most 512 |a| in bf16) and O (a grid of |a|, at most 256 |a|) are both exact:
    asserted with _store.  Every eighth
    column (the WINDOW kind, |a| = 1) adds 64 x (window index) to c.  The whole of a (batch', head) is negated when batch' + head is
    odd, so that neighbours differ.  -> (v [B', heads, Sk, d], the expected O [B', heads, Sq, d]); B' = windows x batch, window-major"""
    e = torch.arange(d, device=dev)
    a = torch.tensor(RAMP_A, device=dev, dtype=f64)[e % 6]
    third = (e % 8 == 7) & (windows > 1)
    a = torch.where(third, torch.ones_like(a), a)
    nmax = Sq + off
    assert 1 <= nmax <= Sk
    span = a * (nmax - 1) + 64.0 * (windows - 1) * third
    c = -torch.round(span / 2 / (2 * a.abs())) * (2 * a.abs())
    if nmax <= 64:          # a short ramp centred on zero is all but zero (one key: O = c = 0 sees nothing): lift it by 128 |a|
        c = c + 128 * a.abs()
    Bp = windows * batch
    win = (torch.arange(Bp, device=dev) // batch).to(f64)[:, None, None, None]
    sign = 1.0 - 2.0 * ((torch.arange(Bp, device=dev)[:, None] + torch.arange(Hh, device=dev)[None, :]) % 2).to(f64)[:, :, None, None]
    cw = c + 64.0 * win * third                                                      # [B', 1, 1, d]
    j = torch.arange(Sk, device=dev, dtype=f64)[None, None, :, None]
    n = (torch.arange(Sq, device=dev, dtype=f64) + off + 1)[None, None, :, None]
    v = (sign * (cw + 2 * a * j)).expand(Bp, Hh, Sk, d).contiguous()
    want = (sign * (cw + a * (n - 1))).expand(Bp, Hh, Sq, d).contiguous()
    _store(v, dt), _store(want, dt)
    _exact_pre(Sk, 1024, 1)                             # partial sums in units of min |a| / ... = 1/4: below 2^24
    return v, want


# ------------------------------------------------------------------------------------------- lse: the derived allowance
def f32_intrinsics(r):
    """MI355X_MICROARCH.md gives no accuracy figure for v_exp_f32 / v_log_f32, so that term is the same quantity MEASURED on a float32 CPU
    evaluation of this case: (worst relative error of float32 exp2 over the case's arguments s - m, worst absolute error of float32 log2
    over the case's sums l and 16 l -- the generic kernel's deferred maximum may sit up to 2^4 below the true one)"""
    x = (r.s - r.m).clamp_min(-126.0).cpu().to(f32)
    e_exp = float(((torch.exp2(x).to(f64) - torch.exp2(x.to(f64))).abs() / torch.exp2(x.to(f64))).max())
    l = torch.cat([r.l0.flatten(), 16 * r.l0.flatten()]).clamp_min(2.0 ** -120).cpu().to(f32)
    e_log = float((torch.log2(l).to(f64) - torch.log2(l.to(f64))).abs().max())
    return e_exp, e_log


def lse_allowance(r, q, k, *, scale, prescaled, intr):
    """|lse_kernel - lse_float64| per query [B', heads, Sq], log2 units, three terms:
      1. the fp32 dot product behind every score: head_dim 2^-24 sum_e |q_e k_e| scale log2 e (the worst visible key of the query; lse is a
         P-weighted mean of score perturbations, so no more than the worst of them);
      2. the fp32 sum of up to Sk terms: n_i 2^-24 relative on l, times log2 e;
      3. exp2 and log2: 2 x the float32 CPU figures of f32_intrinsics (relative on every term of l: times log2 e; absolute on log2 l)."""
    d = q.shape[-1]
    c = 1.0 if prescaled else scale32(scale) * LOG2E
    mag = (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(torch.isinf(r.s), 0.0).max(-1).values * c
    return d * U32 * mag + r.n.to(f64) * U32 * LOG2E + 2 * (intr[0] * LOG2E + intr[1])


# ------------------------------------------------------------------------------------------- the cases, shared by the GPU and the CPU file
HEAD_DIMS = (40, 80, 96, 160)
# (head_dim, variant, storage type): every variant a storage type admits (fp16: 0, 1, 5); variant 7 has its own whole-tile shapes
ROUTES = [(d, 0, dt) for d in HEAD_DIMS for dt in (bf16, f16)] + [(40, v, dt) for v in (1, 5) for dt in (bf16, f16)] + \
         [(40, v, bf16) for v in (2, 3, 6)]
NONCAUSAL = [(1, 1), (1, 2), (33, 63), (65, 64), (129, 65), (127, 129), (257, 255), (130, 257), (256, 384)]
RING = [(256, 128), (256, 384), (512, 256)]                             # variant 7: Sq % 256 == 0, Sk % 128 == 0
CAUSAL = [(1, 1, 0), (33, 33, 0), (65, 65, 0), (129, 129, 0), (200, 200, 0), (100, 130, 30), (31, 65, 0), (31, 65, 17), (31, 65, 34)]
# ws, F, Fq, first frame of the shard, H, W: the last one is a frame shard (Fq != F) with the causal_offset the engine passes
WINDOWS = [(4, 3, 3, 0, 8, 8), (8, 2, 2, 0, 16, 16), (4, 5, 5, 0, 8, 12), (4, 5, 2, 3, 8, 8)]
CROSS = (300, 77)                                                        # the text cross-attention shape class


def route_id(r):
    return f"d{r[0]}-v{r[1]}-{'f16' if r[2] == f16 else 'bf16'}"


def lse_route(variant, dt):
    """fp16 admits no lse; variants 2, 3 would silently become the tracked form and 7 refuses"""
    return dt == bf16 and variant in (0, 1, 5, 6)


# ------------------------------------------------------------------------------------------- launch geometries and Part 2 inputs
class Case:
    """one launch geometry: layouts of Q / O and K / V rows, token counts, the keyword arguments of ops.attention"""
    def __init__(self, name, lay_q, lay_kv, Hh, d, tq, tk, kw, windows=1):
        self.name, self.lay_q, self.lay_kv, self.Hh, self.d, self.tq, self.tk, self.kw, self.windows = name, lay_q, lay_kv, Hh, d, tq, tk, kw, windows
        self.Sq, self.Sk, self.causal, self.off = kw["Sq"], kw["Sk"], kw["causal"], kw.get("causal_offset", 0)
        self.batch = kw["batch"]


def plain(B, Hh, d, Sq, Sk, causal=False, off=0):
    lay = _Plain(B, Hh, d)
    kw = dict(batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, causal=causal, causal_offset=off)
    return Case(f"{'causal' if causal else 'plain'} {Sq}x{Sk}+{off} B{B} h{Hh}", lay, lay, Hh, d, B * Sq, B * Sk, kw)


def window(B, Hh, d, ws, Fr, Fq, f0, H, W):
    kw = dict(batch=B, heads=Hh, head_dim=d, Sq=Fq * ws * ws, Sk=Fr * ws * ws, causal=True, window=(ws, Fr, H, W), Fq=Fq, causal_offset=f0 * ws * ws)
    return Case(f"window ws{ws} F{Fr} Fq{Fq}@{f0} {H}x{W}", _Window(B, Fq, H, W, ws, Hh, d), _Window(B, Fr, H, W, ws, Hh, d), Hh, d,
                 B * Fq * H * W, B * Fr * H * W, kw, windows=(H // ws) * (W // ws))


def strided(Fr, L, Hh, d):
    """FSTextTransformer's attention over frames: rows (frame, token), one causal sequence of Fr per token"""
    lay = _Strided(Fr, L, Hh, d)
    kw = dict(batch=L, heads=Hh, head_dim=d, Sq=Fr, Sk=Fr, causal=True, seq_stride_rows=L, batch_stride_rows=1)
    return Case(f"strided F{Fr} L{L}", lay, lay, Hh, d, Fr * L, Fr * L, kw)


def inputs(case, dt, dev, qamp=1.0, prescaled=False, scale=None, seed=11):
    """the Part 2 operands, token-major [tokens, C] in the storage type: N(0, 1), q times qamp; prescaled: q * scale * log2 e rounded once.
    Causal cases whose last key is visible: that key is seen by the last query alone, and under a sharp softmax it may weigh nothing
    there, so that dropping it moved no row (the mutation table found this at q x 3).  Its K row is therefore PLANTED: half the last
    query's own N(0, 1) row, a score of qamp sqrt(head_dim) log2(e) / 2 -- 4.5 log2 units or more above a typical one"""
    C = case.Hh * case.d
    q2 = _rand((case.tq, C), dev, seed)
    k2 = _rand((case.tk, C), dev, seed + 1)
    if case.causal and case.Sq + case.off == case.Sk:
        k4 = case.lay_kv.to4(k2, case.Sk).clone()
        k4[:, :, case.Sk - 1] = 0.5 * case.lay_q.to4(q2, case.Sq)[:, :, case.Sq - 1]
        k2 = case.lay_kv.to2(k4, case.Sk)
    q2 = (q2 * qamp).to(dt)
    if prescaled:
        q2 = (q2.to(f64) * ((case.d ** -0.5 if scale is None else scale) * LOG2E)).to(dt)
    return q2, k2.to(dt), _rand((case.tk, C), dev, seed + 2).to(dt)


def to4(case, q2, k2, v2):
    return case.lay_q.to4(q2.to(f64), case.Sq), case.lay_kv.to4(k2.to(f64), case.Sk), case.lay_kv.to4(v2.to(f64), case.Sk)
