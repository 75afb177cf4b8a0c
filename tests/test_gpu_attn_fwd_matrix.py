"""seer_attn_fwd (csrc/attention.hip, csrc/attention40.hip) tested exactly and per query row, every variant: part 3 of the series after
test_gpu_f16_matrix.py (GEMM and conv, bit for bit) and test_gpu_train_matrix.py (the attention backward per own row).  The older forward
tests compare N(0, 1) problems with rtol 2e-2 / atol 1e-2, a fifth of an output element at 1024 keys: a last key tile that drops a
key, a padded key that joins the denominator, a diagonal off by one for a query that sees hundreds of keys all pass.  Two parts:

1. EXACT, zero tolerance.  Q = 0 makes every visible score 0 and every P = 2^0 in either storage type, on EVERY path: the fixed
   reference of the d = 40 fast path (variants 2, 3, 7, and AUTO from 256 keys up) cannot overflow, so this is the exact construction
   that stays on it.  O[i] = (sum of the visible V[j]) / n_i, and V is built (tests/attn_fwd_ref.py: uniform_v, ramp_v) so that the
   quotient is exactly representable: the fp32 result is within a few ulp of it whatever reciprocal the kernel uses, and the 16-bit
   store is determined.  Not causal: BALANCE columns ((w, -w) pairs, O = 0: a dropped or doubled key leaves w / (n +- 1)) and LEVEL
   columns (V = c, O = c: a key past Sk admitted with weight 1 gives c n / (n + 1), another 16-bit value), interleaved inside every
   8-column group; odd Sk runs twice so that every key position carries a w.  Causal, with and without causal_offset, windowed and
   frame-sharded: V[j] = c + 2 a j, O[i] = c + a (n_i - 1), a in +-1, +-1/2, +-1/4 by column -- a diagonal off by one key moves a column
   by |a|, two half-ulps or more -- and WINDOW columns that add 64 x (window index).  lse, where requested: exactly log2(n_i) for every
   query whose n_i is a power of two.
2. PER OWN ROW -- one (batch', head, query) vector of head_dim values -- against the float64 softmax formula, on N(0, 1) inputs and with
   q x 3 (sharper, still inside the fast path's range): |got - ref|_2 / max(|ref|_2, 2^-6 rms row norm).  The allowance is derived: the
   kernel's worst row must be within 2x the worst row of a float64 emulation that rounds only where the kernels round (attn_fwd_ref.py
   lists the roundings: q * fp32(scale log2 e) in the d = 40 kernel, P -- truncated on the fast path --, the denominator where it comes
   out of the P V product, O).  2x is the project's margin for 16-bit emulations (test_gpu_clip_text.py, test_gpu_train_matrix.py).
   Nothing in the bound comes from the kernel.
   lse (bf16; generic kernel and variant 5) per query against the float64 log2-sum-exp2 of the emulation's scores.  Allowance
   (attn_fwd_ref.lse_allowance), log2 units: (1) the fp32 dot product, head_dim 2^-24 sum_e |q_e k_e| scale log2 e; (2) the fp32 sum
   of n_i terms, n_i 2^-24 log2 e; (3) the hardware exp2 / log2: MI355X_MICROARCH.md states no accuracy for v_exp_f32 / v_log_f32, so
   this term is 2 x the error of a float32 CPU evaluation of the same exp2 and log2 (attn_fwd_ref.f32_intrinsics; both figures are
   printed).  And per row sum_j exp2(s_ij - lse_i) = 1 within that allowance x ln 2.

Every case runs on the sentinel layout (_call): Q, K, V are column slices of NaN-filled [tokens + 1, 3C + 16] buffers, O a column slice
of a NaN-filled buffer.  After the call the inputs keep their bits, everything outside the O slice keeps its NaN bits, O is finite.

Arguments the header admits that no other forward test passes, and the assertion that covers each:
  O row stride % 8 == 4 (_call: every case; o_ss % 4 is all seer_attn_fwd asks) . heads = 1 and 3 (test_exact_uniform cycles 2, 1, 3;
  test_rows_heads) . an explicit scale (test_rows_explicit_scale) . lse with causal, windowed and strided addressing (test_exact_causal,
  test_exact_window, test_exact_strided, test_rows_causal, test_rows_window, test_rows_strided: every lse route) . variant 6
  (every route list) . the NaN frames (_call, _call_head_major).

FOUND BY THIS FILE and fixed with it: lse at head_dim 40 / 80 (generic kernel) and in the d = 40 tracked form came from the denominator
of O, which those kernels take out of the P V product: the sum of the bf16-ROUNDED P.  Right for O (its numerator holds the same P), but
as a statistic up to 2^-9 relative off: 127x this allowance (generic, causal 31 x 65) and 199x (variant 5, causal 33 x 33), where head_dim
96 / 160, which add the unrounded P, sit at 0.02x.  lse now has an fp32 sum of the unrounded P of its own in those launches (template parameter LSE).

All references are float64 torch on inputs already rounded to the storage type.  Measured values, the mutation table (run on the CPU by
tests/test_attn_fwd_ref_cpu.py) and the file's run time: profiles/attn_fwd_matrix.md."""
import math

import pytest
import torch

from tests import attn_fwd_ref as R
from tests.test_gpu_f16_matrix import _eq, _ints, _store
from tests.test_gpu_train_matrix import _Plain, _row_err

pytestmark = pytest.mark.gpu

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
ROUTES = [pytest.param(r, id=R.route_id(r)) for r in R.ROUTES]
DTS = [pytest.param(bf16, id="bf16"), pytest.param(f16, id="f16")]


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _call(dev, dt, case, variant, q2, k2, v2, want_lse, **extra):
    """one forward on the sentinel layout: q | 8 spare | k | 8 spare | v column slices of NaN [tokens + 1, 3C + 16] buffers (the layout of
    test_gpu_train_matrix._attn_run), O the columns 4 .. 4 + C of a NaN [tokens + 1, C + 12] buffer: a row stride that is a multiple of 4
    and not of 8.  Asserts: the inputs keep their bits, everything outside the O slice keeps its NaN bits, O is finite"""
    from seervideoldm_amd import ops, train_ops
    C, tq, tk = case.Hh * case.d, case.tq, case.tk
    LD = 3 * C + 16
    nanbuf = lambda rows, cols: torch.full((rows, cols), float("nan"), device=dev, dtype=dt)
    in_q, in_kv, obuf = nanbuf(tq + 1, LD), nanbuf(tk + 1, LD), nanbuf(tq + 1, C + 12)
    q, k, v = in_q[:tq, :C], in_kv[:tk, C + 8:2 * C + 8], in_kv[:tk, 2 * C + 16:]
    q.copy_(q2), k.copy_(k2), v.copy_(v2)
    out = obuf[:tq, 4:4 + C]
    assert out.stride(0) % 8 == 4
    lse = None
    if want_lse:
        lse = train_ops.attn_lse_buffer(case.batch, case.Hh, case.Sq, dev, window=case.kw.get("window")).fill_(float("nan"))
    before = [t.clone() for t in (in_q, in_kv, obuf)]
    ops.attention(q, k, v, out, lse=lse, variant=variant, **case.kw, **extra)
    what = f"{case.name} d{case.d} variant {variant} lse {want_lse}"
    assert _bits_equal(in_q, before[0]) and _bits_equal(in_kv, before[1]), f"{what}: the forward wrote into its inputs"
    keep = torch.ones(obuf.shape, dtype=torch.bool, device=dev)
    keep[:tq, 4:4 + C] = False
    moved = obuf.view(torch.int16)[keep] != before[2].view(torch.int16)[keep]
    assert not bool(moved.any()), f"{what}: {int(moved.sum())} stores outside the O slice (spare columns / guard row)"
    assert bool(torch.isfinite(out.float()).all()), f"{what}: O not finite (an element not written, or a read of a spare column)"
    if lse is not None:
        assert bool(torch.isfinite(lse).all()), f"{what}: lse not finite (a query not written)"
    return out, lse


# =========================================================================================== 1. exact, zero tolerance
def _exact(dev, case, route, v4, want4, tag):
    """Q = 0, K small integers, V and the expected O from the construction; without lse, and on the lse routes once more with it"""
    d, variant, dt = route
    C = case.Hh * d
    q2 = torch.zeros((case.tq, C), device=dev, dtype=dt)
    k2 = _store(_ints((case.tk, C), dev, 3), dt)
    v2 = _store(case.lay_kv.to2(v4, case.Sk), dt)
    want2 = case.lay_q.to2(want4.expand(v4.shape[0], case.Hh, case.Sq, d).contiguous(), case.Sq)
    n = R.visible(case.Sq, case.Sk, case.causal, case.off, dev).sum(-1)
    pow2 = (n & (n - 1)) == 0
    for want_lse in ([False, True] if R.lse_route(variant, dt) else [False]):
        out, lse = _call(dev, dt, case, variant, q2, k2, v2, want_lse)
        _eq(out, want2, dt, f"{case.name} {R.route_id(route)} {tag} lse {want_lse}: O of a uniform softmax")
        if want_lse:
            got = lse.view(-1, case.Sq)[:, pow2]
            assert bool((got == torch.log2(n[pow2].to(f32))).all()), f"{case.name} {R.route_id(route)} {tag}: lse != log2(n_i) at a power of two"


def _exact_uniform(dev, route, shapes):
    d, variant, dt = route
    for i, (Sq, Sk) in enumerate(shapes):
        B, Hh = (2, 2, 1)[i % 3], (2, 1, 3)[i % 3]
        case = R.plain(B, Hh, d, Sq, Sk)
        for shift in ((0, 1) if Sk % 2 else (0,)):
            v4, want4 = R.uniform_v(B, Hh, Sk, d, dev, dt, seed=10 * i, shift=shift)
            _exact(dev, case, route, v4, want4, f"shift {shift}")


@pytest.mark.parametrize("route", ROUTES)
def test_exact_uniform(device, route):
    """not causal, every (Sq, Sk) around the 32-key block, the 64- / 128-key tile and the 128- / 256-query workgroup; heads 2, 1, 3"""
    _exact_uniform(device, route, R.NONCAUSAL)


def test_exact_uniform_ring(device):
    """variant 7 (three-stage ring, whole tiles only) on the shapes it accepts: one, two and three stages"""
    _exact_uniform(device, (40, 7, bf16), R.RING)


@pytest.mark.parametrize("route", ROUTES)
def test_exact_causal(device, route):
    """causal squares and causal_offset: a diagonal off by one key moves a column by |a|"""
    d, variant, dt = route
    for Sq, Sk, off in R.CAUSAL:
        case = R.plain(2, 2, d, Sq, Sk, True, off)
        v4, want4 = R.ramp_v(2, 2, Sq, Sk, d, device, dt, off)
        _exact(device, case, route, v4, want4, "ramp")


@pytest.mark.parametrize("route", ROUTES)
def test_exact_window(device, route):
    """the temporal window form (ws 4 and 8, H != W) and a frame shard with the engine's causal_offset: j is the position in the window's
    (f, wy, wx) order; the window columns put every window on integers of its own"""
    d, variant, dt = route
    for ws, Fr, Fq, f0, H, W in R.WINDOWS:
        case = R.window(1, 2, d, ws, Fr, Fq, f0, H, W)
        v4, want4 = R.ramp_v(1, 2, case.Sq, case.Sk, d, device, dt, case.off, case.windows)
        _exact(device, case, route, v4, want4, "ramp")


def test_exact_strided(device):
    """seq_stride_rows = L, batch_stride_rows = 1 (d 96, F 12, L 77, causal), with and without lse"""
    case = R.strided(12, 77, 2, 96)
    for dt in (bf16, f16):
        v4, want4 = R.ramp_v(77, 2, 12, 12, 96, device, dt)
        _exact(device, case, (96, 0, dt), v4, want4, "ramp")


def _call_head_major(dev, dt, B, Hh, d, Sq, Sk, q4, k4, v4):
    """q_head_major and kv_head_major: [batch][head][token][head_dim] contiguous, each inside a NaN buffer with a guard row on both sides"""
    from seervideoldm_amd import ops

    def framed(t4):
        rows = t4.shape[0] * t4.shape[1] * t4.shape[2]
        buf = torch.full((rows + 2, d), float("nan"), device=dev, dtype=dt)
        buf[1:rows + 1] = t4.reshape(rows, d).to(dt)
        return buf, buf[1:rows + 1]
    (bq, q), (bk, k), (bv, v) = framed(q4), framed(k4), framed(v4)
    C = Hh * d
    obuf = torch.full((B * Sq + 1, C + 12), float("nan"), device=dev, dtype=dt)
    out = obuf[:B * Sq, 4:4 + C]
    before = [t.clone() for t in (bq, bk, bv, obuf)]
    ops.attention(q, k, v, out, batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, q_head_major=True, kv_head_major=True)
    for t, b in zip((bq, bk, bv), before):
        assert _bits_equal(t, b), "head-major: the forward wrote into its inputs"
    keep = torch.ones(obuf.shape, dtype=torch.bool, device=dev)
    keep[:B * Sq, 4:4 + C] = False
    assert _bits_equal(obuf[keep], before[3][keep]), "head-major: a store outside the O slice"
    assert bool(torch.isfinite(out.float()).all()), "head-major: O not finite"
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", [40, 80])
def test_exact_head_major(device, d, dt):
    """head-major Q, K and V on a ragged S: d = 40 at 257 keys (bf16: the d = 40 kernel's fast path by AUTO; fp16: its tracked form), d = 80
    the generic kernel"""
    B, Hh, Sq, Sk = 2, 3, 130, 257
    for shift in (0, 1):
        v4, want4 = R.uniform_v(B, Hh, Sk, d, device, dt, seed=5, shift=shift)
        q4 = torch.zeros((B, Hh, Sq, d), device=device, dtype=f64)
        k4 = _ints((B, Hh, Sk, d), device, 3)
        out = _call_head_major(device, dt, B, Hh, d, Sq, Sk, q4, k4, v4)
        _eq(out, _Plain(B, Hh, d).to2(want4.expand(B, Hh, Sq, d).contiguous(), Sq), dt, f"head-major d{d} shift {shift}")


# =========================================================================================== 2. per own row against float64
def _rows(dev, case, route, label, qamp=1.0, prescaled=False, scale=None, seed=11):
    """one Part 2 case: N(0, 1) x qamp inputs, the float64 formula, the emulation of the kernel the launch takes, the kernel's worst row
    within 2x the emulation's; on the lse routes once more with lse, which is then checked per query.  Returns the failures"""
    d, variant, dt = route
    C, Sq, Sk = case.Hh * d, case.Sq, case.Sk
    sc = d ** -0.5 if scale is None else scale
    q2, k2, v2 = R.inputs(case, dt, dev, qamp, prescaled, scale, seed)
    q4, k4, v4 = R.to4(case, q2, k2, v2)
    extra = dict(q_prescaled=prescaled)
    if scale is not None:
        extra["scale"] = scale
    fails, emus = [], {}
    for want_lse in ([False, True] if R.lse_route(variant, dt) else [False]):
        kind = R.kernel_kind(d, variant, dt, Sk, want_lse, prescaled)
        if kind not in emus:
            emus[kind] = R.emulate(q4, k4, v4, scale=sc, dt=dt, kind=kind, prescaled=prescaled, causal=case.causal, off=case.off)
        r = emus[kind]
        out, lse = _call(dev, dt, case, variant, q2, k2, v2, want_lse, **extra)
        got4 = case.lay_q.to4(out.to(f64), Sq)
        floor = R.row_floor(r.o_ref)
        e_emu, e_got = _row_err(r.o, r.o_ref, floor), _row_err(got4, r.o_ref, floor)
        tag = f"{case.name} | {R.route_id(route)} | {kind} | {label} | lse {int(want_lse)}"
        print(f"attn_fwd_matrix part2 | {tag} | O | emulation {e_emu:.3e} | kernel {e_got:.3e} | ratio {e_got / max(e_emu, 1e-300):.3f}")
        if not e_got <= 2 * e_emu:
            fails.append(f"{tag}: worst row {e_got:.4g} > 2 x emulation = {2 * e_emu:.4g}")
        if want_lse:
            intr = R.f32_intrinsics(r)
            allow = R.lse_allowance(r, q4, k4, scale=sc, prescaled=prescaled, intr=intr)
            g = lse.view(r.lse.shape).to(f64)
            ratio = float(((g - r.lse).abs() / allow).max())
            one = float(((torch.exp2(r.s - g[..., None]).sum(-1) - 1).abs() / (allow * math.log(2))).max())
            print(f"attn_fwd_matrix part2 | {tag} | lse | float32 CPU exp2 rel {intr[0]:.3e} log2 abs {intr[1]:.3e} | worst allowance "
                  f"{float(allow.max()):.3e} | worst |err| {float((g - r.lse).abs().max()):.3e} | err / allowance {ratio:.3f} | sum-to-one / allowance {one:.3f}")
            if not ratio <= 1:
                fails.append(f"{tag}: lse off by {ratio:.4g} x its allowance")
            if not one <= 1 + 1e-3:
                fails.append(f"{tag}: sum_j exp2(s - lse) - 1 is {one:.4g} x its allowance")
    return fails


def _rows_all(dev, route, cases, **kw):
    fails = []
    for case in cases:
        for qamp in (1.0, 3.0):
            fails += _rows(dev, case, route, f"q x {qamp:g}", qamp=qamp, **kw)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("route", ROUTES)
def test_rows_noncausal(device, route):
    _rows_all(device, route, [R.plain((2, 2, 1)[i % 3], (2, 1, 3)[i % 3], route[0], Sq, Sk) for i, (Sq, Sk) in enumerate(R.NONCAUSAL)])


def test_rows_ring(device):
    _rows_all(device, (40, 7, bf16), [R.plain(2, 2, 40, Sq, Sk) for Sq, Sk in R.RING])


@pytest.mark.parametrize("route", ROUTES)
def test_rows_causal(device, route):
    _rows_all(device, route, [R.plain(2, 2, route[0], Sq, Sk, True, off) for Sq, Sk, off in R.CAUSAL])


@pytest.mark.parametrize("route", ROUTES)
def test_rows_window(device, route):
    _rows_all(device, route, [R.window(1, 2, route[0], *w) for w in R.WINDOWS])


@pytest.mark.parametrize("route", ROUTES)
def test_rows_cross(device, route):
    """the text cross-attention shape class (Sq 1000 -> 300, Sk 77) at every head_dim and variant"""
    _rows_all(device, route, [R.plain(2, 2, route[0], *R.CROSS)])


@pytest.mark.parametrize("route", ROUTES)
def test_rows_heads(device, route):
    """heads = 1 and heads = 3, below and above the 256 keys from which AUTO takes the d = 40 kernel"""
    _rows_all(device, route, [R.plain(2, Hh, route[0], Sq, Sk) for Hh in (1, 3) for Sq, Sk in ((129, 65), (130, 257))])


@pytest.mark.parametrize("route", ROUTES)
def test_rows_prescaled(device, route):
    """q_prescaled = True: q holds q * scale * log2 e rounded to the storage type, no kernel multiplies or rounds it again"""
    d = route[0]
    _rows_all(device, route, [R.plain(2, 2, d, 129, 65), R.plain(2, 2, d, 130, 257), R.plain(2, 2, d, 100, 130, True, 30)], prescaled=True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d,variant", [(40, 1), (80, 0), (96, 0), (160, 0)])
def test_rows_explicit_scale(device, d, variant, dt):
    """a scale other than head_dim^-0.5 on the generic kernel"""
    _rows_all(device, (d, variant, dt), [R.plain(2, 2, d, 129, 65), R.plain(2, 2, d, 130, 257)], scale=0.3)


@pytest.mark.parametrize("dt", DTS)
def test_rows_strided(device, dt):
    _rows_all(device, (96, 0, dt), [R.strided(12, 77, 2, 96)])
