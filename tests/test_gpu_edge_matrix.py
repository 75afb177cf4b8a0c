"""csrc/elementwise.hip -- rotary, timestep embedding, seer_linear_smallm, seer_conv_in / seer_conv_out, cast and layout,
seer_conv1x1_nchw_f32, seer_clamp01 and seer_gaussian_sample -- and the DDIM step boundary of csrc/sampler_step.hip
(seer_ddim_step_begin, seer_cfg_ddim_step in its host and device forms), tested exactly, per owner and at their edges: the second half of part 5 of the series (the first is
test_gpu_norm_matrix.py).  The two PLMS entry points are left to test_gpu_plms.py, which holds them to 1e-6 per order.

0. Pure data movement bit for bit into guarded arenas: layout conversion, cast (ties, +-0, +-inf, NaN, fp16 overflow, subnormals)
   and the step's input assembly on random fp32 bit patterns.
1. EXACT, zero tolerance: integer or dyadic inputs on which the fp32 arithmetic is exact.  NaN-prefilled guarded outputs; every
   launch runs twice and must repeat its bits.
2. Random data per row or element against float64 with a derived allowance (tests/norm_edge_ref.py); nothing in it comes from a kernel.
3. Every SEER_EINVAL / SEER_ENOSYS branch, decided on the host: NaN-filled outputs keep their bits.

Measured values, the instantiation each shape reaches and run times: profiles/norm_edge_matrix.md."""
import pytest
import torch

from tests import fused320_ref as R
from tests import norm_edge_ref as N
from tests.test_gpu_f16_matrix import _eq, _store
from tests.test_gpu_train_matrix import _bound

pytestmark = pytest.mark.gpu

f16, bf16, f32, f64, i64, i32 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int64, torch.int32
DTS = [pytest.param(bf16, id="bf16"), pytest.param(f16, id="f16")]
EINVAL, ENOSYS = -22, -38
GUARD = N.GUARD


def _L():
    from seervideoldm_amd import _lib
    return _lib.load()


def _dtc(dt):
    return 1 if dt == f16 else 0


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _name(dt):
    return "f16" if dt == f16 else "bf16"


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _arena(n, dev, dtype=f32):
    """n NaN elements of output in front of GUARD NaN sentinels, one allocation"""
    return torch.full((n + GUARD,), float("nan"), device=dev, dtype=dtype)


def _guard_holds(a, n, what):
    assert bool(a[n:].isnan().all()), f"{what}: a store behind the output"


def _c32(t):
    return None if t is None else t.to(f32).contiguous()


# =========================================================================================== 0. data movement, bit for bit
@pytest.mark.parametrize("Nb,C,HW", [(1, 1, 1), (3, 37, 45), (2, 32, 32), (2, 33, 31), (1, 320, 64)])
def test_layout_bit_for_bit(device, Nb, C, HW):
    g = torch.Generator().manual_seed(C * HW)
    x = torch.randn((Nb, C, HW), generator=g).to(device)
    a = _arena(Nb * HW * C, device, bf16)
    assert _L().seer_nchw_f32_to_nhwc_bf16(_p(x), Nb, C, HW, _p(a), _s()) == 0
    torch.cuda.synchronize()
    want = x.permute(0, 2, 1).contiguous().to(bf16)
    assert torch.equal(_bits(a[:Nb * HW * C]), _bits(want.reshape(-1))), "seer_nchw_f32_to_nhwc_bf16"
    _guard_holds(a, Nb * HW * C, "nchw -> nhwc")
    words = torch.randint(-32768, 32768, (Nb, HW, C), generator=g, dtype=i32).to(torch.int16).to(device)
    words = torch.where((words & 0x7F80) == 0x7F80, words & ~0x0100, words)          # (no inf / NaN patterns: NaN payloads are not compared)
    xb = words.view(bf16)
    b = _arena(Nb * C * HW, device, f32)
    assert _L().seer_nhwc_bf16_to_nchw_f32(_p(xb), Nb, C, HW, _p(b), _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(b[:Nb * C * HW]), _bits(xb.permute(0, 2, 1).contiguous().to(f32).reshape(-1))), "seer_nhwc_bf16_to_nchw_f32"
    _guard_holds(b, Nb * C * HW, "nhwc -> nchw")


_CAST_SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 65520.0, 65519.0, -65520.0, 65504.0,
                  1.00390625, 1.01171875, 1.005859375,          # bf16 ties: 1 + 2^-8 (down to even), 1 + 3 2^-8 (up to even), just above a tie
                  1.00048828125, 1.00146484375,                 # fp16 ties: 1 + 2^-11, 1 + 3 2^-11
                  2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -134, 2.0 ** -126, 2.0 ** -14, 3.0e38, -3.4e38]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025])
def test_cast_bit_for_bit(device, dt, n):
    """torch's cast is the reference; the special values rotate through every position of the vector / tail split"""
    sp = torch.tensor(_CAST_SPECIALS, dtype=f32)
    g = torch.Generator().manual_seed(n)
    for shift in range(0, len(_CAST_SPECIALS), max(1, len(_CAST_SPECIALS) // 6) if n > 5 else 1):
        x = torch.randn((n,), generator=g) * 3
        k = min(n, len(sp))
        x[:k] = sp.roll(-shift)[:k]
        x = x.to(device)
        a = _arena(n, device, dt)
        assert _L().seer_cast_f32(_p(x), n, _p(a), _dtc(dt), _s()) == 0
        torch.cuda.synchronize()
        got, want = a[:n], x.to(dt)
        assert torch.equal(got.isnan(), want.isnan())
        same = (_bits(got) == _bits(want)) | want.isnan()
        assert bool(same.all()), f"seer_cast_f32 {_name(dt)} n{n}: {x[~same].tolist()} -> {got[~same].tolist()}, torch {want[~same].tolist()}"
        _guard_holds(a, n, "cast")


@pytest.mark.parametrize("b,C,f1,Fp,HW,reps", N.STEP_BEGIN_CASES)
def test_step_begin_bit_for_bit(device, b, C, f1, Fp, HW, reps):
    g = torch.Generator().manual_seed(HW + Fp)
    pat = lambda *shape: torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=i64).to(i32).to(device).view(f32)
    x0, x = (pat(b, C, f1, HW) if f1 else None), pat(b, C, Fp, HW)
    F = f1 + Fp
    n = b * C * F * HW
    t_table = (torch.arange(9, dtype=i64) * 111 + 5).to(device)
    step = torch.tensor([6, -3], dtype=i32, device=device)
    sample = torch.zeros((reps * n + GUARD,), dtype=i32, device=device)
    sample[:] = 0x7FC00001
    t_out = torch.full((reps * b + GUARD,), -77, dtype=i64, device=device)
    assert _L().seer_ddim_step_begin(_p(x0), _p(x), b, reps, C, f1, Fp, HW, _p(t_table), _p(step), _p(sample), _p(t_out), _s()) == 0
    torch.cuda.synchronize()
    want = (torch.cat([x0.view(i32), x.view(i32)], 2) if f1 else x.view(i32)).repeat(reps, 1, 1, 1)
    assert torch.equal(sample[:reps * n], want.reshape(-1)), "seer_ddim_step_begin: sample is not cat([x0_emb, x], frames) repeated"
    assert bool((sample[reps * n:] == 0x7FC00001).all()), "a store behind sample"
    assert bool((t_out[:reps * b] == t_table[6]).all()) and bool((t_out[reps * b:] == -77).all()), "t_out"
    assert step.tolist() == [6, 6], f"step = {step.tolist()}: step[1] must become step[0], step[0] must stay"


# =========================================================================================== 1. exact
@pytest.mark.parametrize("case", N.ROTARY_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_rotary_inplace(device, case):
    rows, heads, hd, rd, tokens, off, ld = case
    Cw = heads * hd
    n = rows * ld + ld
    buf = R.ints((n,), device, 101 + rows)
    table = R.dyadic_table(max(rows, tokens) + off, rd, device, 102 + rows)
    want = N.rotary_inplace(buf, case, table)
    assert float(want.abs().max()) <= 16 and bool((want * 2 == (want * 2).round()).all()) and not torch.equal(want, buf)
    outs = []
    for _ in range(2):
        x = _store(buf, bf16)
        rc = _L().seer_rotary_inplace(_p(x), rows, ld, N.ROT_COL0, N.ROT_COL0 + Cw, heads, hd, rd, tokens, off, _p(table), _s())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(x)
    _eq(outs[0], want, bf16, f"seer_rotary_inplace {case}: the rotated prefixes, and every other word of the buffer unchanged")
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,K,Nf", N.SMALLM_CASES)
def test_exact_linear_smallm(device, dt, B, K, Nf):
    x, w, bias = N.smallm_exact(B, K, Nf, device, 111 + K)
    want = N.linear_smallm(x, w, bias)
    xs = torch.full((8 * K,), float("nan"), device=device)                  # (slots B..7 hold NaN: an unused batch slot must not leak)
    xs[:B * K] = x.to(f32).reshape(-1)
    w16, b32 = _store(w, dt), _c32(bias)
    for use_bias in (True, False):
        outs = []
        for _ in range(2):
            y = _arena(B * Nf, device)
            rc = _L().seer_linear_smallm(_p(xs), B, K, _p(w16), _p(b32) if use_bias else None, Nf, 0, 0, _p(y), _dtc(dt), _s())
            assert rc == 0
            torch.cuda.synchronize()
            outs.append(y)
        ref = want if use_bias else N.linear_smallm(x, w, None)
        _eq(outs[0][:B * Nf], ref[:B * Nf], dt, f"seer_linear_smallm B{B} K{K} N{Nf} {_name(dt)} bias{use_bias}")
        _guard_holds(outs[0], B * Nf, "linear_smallm")
        assert torch.equal(_bits(outs[0][:B * Nf]), _bits(outs[1][:B * Nf]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", N.CONV_IN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_conv_in(device, dt, case):
    B, Cin, F, H, W, Cout = case
    x, w, bias = R.ints((B, Cin, F, H, W), device, 121 + Cout), R.ints((3, 3, Cin, Cout), device, 122 + Cout, -2, 2), R.ints((Cout,), device, 123, -8, 8)
    assert N.conv_in_lds_bytes(Cin, Cout) <= 160 * 1024 and 9 * Cin * 6 + 8 <= 256
    npix = B * F * H * W
    x32, w32, b32 = _c32(x), _c32(w), _c32(bias)
    for use_bias in (True, False):
        want = N.conv_in(x, w, bias if use_bias else None)
        outs = []
        for _ in range(2):
            y = _arena(npix * Cout, device, dt)
            rc = _L().seer_conv_in(_p(x32), B, Cin, F, H, W, _p(w32), _p(b32) if use_bias else None, Cout, _p(y), _dtc(dt), _s())
            assert rc == 0, rc
            torch.cuda.synchronize()
            outs.append(y)
        _eq(outs[0][:npix * Cout].reshape(npix, Cout), want, dt, f"seer_conv_in {case} {_name(dt)} bias{use_bias}")
        _guard_holds(outs[0], npix * Cout, "conv_in")
        assert torch.equal(_bits(outs[0][:npix * Cout]), _bits(outs[1][:npix * Cout]))


@pytest.mark.parametrize("dt,Cout", [(bf16, 4), (bf16, 3), (f16, 3)], ids=["bf16-4", "bf16-3", "f16-3"])
@pytest.mark.parametrize("B,C0,F,H,W", N.CONV_OUT_CASES)
def test_exact_conv_out(device, dt, Cout, B, C0, F, H, W):
    npix = B * F * H * W
    x, w, bias = R.ints((npix, C0), device, 131 + C0), R.ints((Cout, 3, 3, C0), device, 132 + C0, -2, 2), R.ints((Cout,), device, 133, -8, 8)
    assert 9 * C0 * 6 + 8 < 2 ** 24
    x16, w32, b32 = _store(x, dt), _c32(w), _c32(bias)
    for use_bias in (True, False):
        want = N.conv_out(x, w, bias if use_bias else None, B, F, H, W)
        outs = []
        for _ in range(2):
            y = _arena(npix * Cout, device)
            rc = _L().seer_conv_out(_p(x16), B, C0, F, H, W, _p(w32), _p(b32) if use_bias else None, Cout, _p(y), _dtc(dt), _s())
            assert rc == 0, rc
            torch.cuda.synchronize()
            outs.append(y)
        _eq(outs[0][:npix * Cout].reshape(B, Cout, F, H, W), want, dt, f"seer_conv_out {(B, C0, F, H, W)} Cout{Cout} {_name(dt)}")
        _guard_holds(outs[0], npix * Cout, "conv_out")
        assert torch.equal(_bits(outs[0][:npix * Cout]), _bits(outs[1][:npix * Cout]))


def _cfg_step(eps, x, noise, coef, index, cfg, scale, case, pred=True, dev_form=False):
    """one launch -> (x_prev [n], pred_x0 [n] or None, step after a _dev launch)"""
    b, C, Ft, cond_f, HW = case
    n = x.numel()
    device = x.device
    xp = _arena(n, device)
    px = _arena(n, device) if pred else None
    step = None
    if dev_form:
        step = torch.tensor([77, index], dtype=i32, device=device)
        xp[:n] = x.reshape(-1)                                            # x_prev aliases x
        rc = _L().seer_cfg_ddim_step(_p(eps), int(cfg), b, C, Ft, cond_f, HW, scale, _p(coef), -1, _p(step), _p(xp), _p(noise), None, 0.0, _p(xp), _p(px), _s())
    else:
        rc = _L().seer_cfg_ddim_step(_p(eps), int(cfg), b, C, Ft, cond_f, HW, scale, _p(coef), index, None, _p(x), _p(noise), None, 0.0, _p(xp), _p(px), _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _guard_holds(xp, n, "x_prev")
    if pred:
        _guard_holds(px, n, "pred_x0")
    return xp[:n].reshape(x.shape), (px[:n].reshape(x.shape) if pred else None), step


@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("case", N.CFG_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_cfg_ddim_step(device, case, cfg):
    eps, x, noise = N.cfg_problem(case, cfg, device, 141 + case[4])
    coef64 = torch.tensor(N.CFG_EXACT_COEF + [(float("nan"),) * 4], dtype=f64, device=device)
    coef, e32, x32, n32 = _c32(coef64), _c32(eps), _c32(x), _c32(noise)
    for index in range(4):
        for use_noise in (True, False):
            wp, w0 = N.cfg_ddim(eps, x, noise if use_noise else None, N.CFG_EXACT_COEF[index], cfg, 7.5, case)
            what = f"seer_cfg_ddim_step {case} cfg{int(cfg)} row {index} noise{int(use_noise)}"
            xp, px, _ = _cfg_step(e32, x32, n32 if use_noise else None, coef, index, cfg, 7.5, case)
            _eq(xp, wp, f32, f"{what}: x_prev")
            _eq(px, w0, f32, f"{what}: pred_x0")
            xp2, none, _ = _cfg_step(e32, x32, n32 if use_noise else None, coef, index, cfg, 7.5, case, pred=False)
            assert none is None and torch.equal(_bits(xp), _bits(xp2)), f"{what}: pred_x0 NULL changes x_prev"
            xd, pd, step = _cfg_step(e32, x32, n32 if use_noise else None, coef, index, cfg, 7.5, case, dev_form=True)
            assert torch.equal(_bits(xd), _bits(xp)) and torch.equal(_bits(pd), _bits(px)), f"{what}: the _dev form differs from the host-index form"
            assert step.tolist() == [index - 1, index], f"{what}: step = {step.tolist()}"
    if case[3]:
        assert bool(e32[:, :, :case[3]].isnan().all())


def test_exact_conv1x1_clamp_gaussian(device):
    L = _L()
    Nb, Cin, Cout, HW = 3, 4, 5, 300
    x, w, bias = R.ints((Nb, Cin, HW), device, 151), R.ints((Cout, Cin), device, 152), R.ints((Cout,), device, 153, -8, 8)
    for b64 in (bias, None):
        y = _arena(Nb * Cout * HW, device)
        assert L.seer_conv1x1_nchw_f32(_p(_c32(x)), Nb, Cin, Cout, HW, _p(_c32(w)), _p(_c32(b64)), _p(y), _s()) == 0
        torch.cuda.synchronize()
        _eq(y[:Nb * Cout * HW].reshape(Nb, Cout, HW), torch.einsum("oc,ncp->nop", w, x) + (b64[None, :, None] if b64 is not None else 0), f32, "seer_conv1x1_nchw_f32")
        _guard_holds(y, Nb * Cout * HW, "conv1x1")
    n = 3 * 301
    v = R.ints((n,), device, 154, -4, 4) * 0.5
    a = _arena(n, device)
    a[:n] = v.to(f32)
    assert L.seer_clamp01(_p(a), n, _s()) == 0
    torch.cuda.synchronize()
    _eq(a[:n], ((v + 1) * 0.5).clamp(0, 1), f32, "seer_clamp01")
    _guard_holds(a, n, "clamp01")
    C = 4
    mom = R.ints((Nb, 2 * C, HW), device, 155, -100, 100)
    mom[:, C:] = float("nan")                                              # (noise == NULL: the logvar half must not be read into the result)
    out = _arena(Nb * C * HW, device)
    assert L.seer_gaussian_sample(_p(_c32(mom)), Nb, C, HW, None, _p(out), _s()) == 0
    torch.cuda.synchronize()
    _eq(out[:Nb * C * HW].reshape(Nb, C, HW), mom[:, :C], f32, "seer_gaussian_sample without noise")
    _guard_holds(out, Nb * C * HW, "gaussian_sample")


# =========================================================================================== 2. random data, derived allowances
def test_rotary_table_against_float64(device):
    T, half = 640, 16
    freqs = N.unet_freqs(half, device)
    want, ang = N.rotary_table_ref(freqs, T)
    allow, torch_worst = N.sincos_allowance(ang)
    a = _arena(T * half * 2, device)
    assert _L().seer_rotary_table(_p(freqs), T, half, _p(a), _s()) == 0
    torch.cuda.synchronize()
    got = a[:T * half * 2].reshape(T, half, 2)
    worst = float((got.to(f64) - want).abs().max())
    print(f"edge_matrix | seer_rotary_table T{T} half{half} | worst error {worst:.4g} | torch float32 sin/cos {torch_worst:.4g} | allowance {allow:.4g}")
    assert worst <= allow
    _guard_holds(a, T * half * 2, "rotary_table")


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("shift", [0.0, 1.0])
@pytest.mark.parametrize("dim", N.TE_DIMS)
def test_timestep_embedding_against_float64(device, dim, flip, shift):
    nt = len(N.TE_TS)
    t = torch.tensor(N.TE_TS, dtype=i64, device=device)
    a = _arena(nt * dim, device)
    assert _L().seer_timestep_embedding(_p(t), nt, dim, flip, shift, _p(a), _s()) == 0
    torch.cuda.synchronize()
    want, arg, expo = N.timestep_embedding(t, dim, flip, shift)
    if dim == 2 and shift == 1.0:
        # half - shift = 0: the exponent is 0 / 0 in the reference formula as in the kernel
        assert bool(want.isnan().all()) and bool(a.isnan().all())
        return
    share = _bound(a[:nt * dim].reshape(nt, dim), want, N.timestep_allowance(arg, expo), f"seer_timestep_embedding dim{dim} flip{flip} shift{shift}")
    print(f"edge_matrix | seer_timestep_embedding dim{dim} flip{flip} shift{shift:g} | share of the allowance used {share:.3f}")
    _guard_holds(a, nt * dim, "timestep_embedding")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,K,Nf", [(2, 320, 1280), (5, 1280, 1283), (8, 1032, 16)])
def test_linear_smallm_silu_against_float64(device, dt, B, K, Nf):
    x = N.r32(R._randn((B, K), device, 161) * (1.0 + torch.arange(B, device=device, dtype=f64))[:, None])
    w = R.r16(R._randn((Nf, K), device, 162, K ** -0.5), dt)
    bias = N.r32(0.1 * R._randn((Nf,), device, 163))
    sx = N.silu64(x)
    pre = sx @ w.t() + bias
    want = N.silu64(pre)
    # fp32 accumulation of K products K 2^-24 sum |x w| (+ the bias), SiLU on both sides 4 ulp each: |silu'| <= 1.1
    allow = 1.1 * ((K + 8) * 2.0 ** -24 * (sx.abs() @ w.abs().t() + bias.abs())) + 4 * 2.0 ** -23 * want.abs() + 2.0 ** -40
    y = _arena(B * Nf, device)
    assert _L().seer_linear_smallm(_p(_c32(x)), B, K, _p(_store(w, dt)), _p(_c32(bias)), Nf, 1, 1, _p(y), _dtc(dt), _s()) == 0
    torch.cuda.synchronize()
    share = _bound(y[:B * Nf].reshape(B, Nf), want, allow, f"seer_linear_smallm silu B{B} K{K} N{Nf}")
    print(f"edge_matrix | seer_linear_smallm silu {_name(dt)} B{B} K{K} N{Nf} | share of the allowance used {share:.3f}")
    _guard_holds(y, B * Nf, "linear_smallm")


@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("case", N.CFG_CASES, ids=lambda c: "x".join(map(str, c)))
def test_cfg_ddim_step_against_float64(device, case, cfg):
    """a real schedule row (alpha_t 0.4216, alpha_prev 0.5541, sigma 0.31, sqrt(1 - alpha_t)) and noise, per element"""
    eps, x, noise = N.cfg_problem(case, cfg, device, 171 + case[4], exact=False)
    row = [float(torch.tensor(v, dtype=f32)) for v in (0.4216, 0.5541, 0.31, (1 - 0.4216) ** 0.5)]
    coef = torch.tensor([[float("nan")] * 4, row], dtype=f32, device=device)
    wp, w0 = N.cfg_ddim(eps, x, noise, row, cfg, 7.5, case)
    ap, a0 = N.cfg_ddim_allowance(eps, x, noise, row, cfg, 7.5, case)
    xp, px, _ = _cfg_step(_c32(eps), _c32(x), _c32(noise), coef, 1, cfg, 7.5, case)
    s1 = _bound(xp, wp, ap, f"seer_cfg_ddim_step {case}: x_prev")
    s0 = _bound(px, w0, a0, f"seer_cfg_ddim_step {case}: pred_x0")
    print(f"edge_matrix | seer_cfg_ddim_step {case} cfg{int(cfg)} | share of the allowance used: x_prev {s1:.3f} pred_x0 {s0:.3f}")


def test_gaussian_sample_against_float64(device):
    Nb, C, HW = 2, 4, 300
    mom = N.r32(R._randn((Nb, 2 * C, HW), device, 181))
    lv = torch.tensor([-40.0, -30.0, 0.0, 20.0, 25.0], device=device, dtype=f64)
    mom[:, C:] = lv[torch.arange(HW, device=device) % 5][None, None, :]
    noise = N.r32(R._randn((Nb, C, HW), device, 182))
    want = N.gaussian_sample(mom, noise)
    sd = torch.exp(0.5 * mom[:, C:].clamp(-30, 20))
    allow = 2.0 ** -23 * want.abs() + (4 + 0.5 * 30 * 1.4427) * 2.0 ** -23 * (sd * noise.abs()) + 2.0 ** -60          # expf: 2 ulp + the rounded argument 10 x log2(e)
    out = _arena(Nb * C * HW, device)
    assert _L().seer_gaussian_sample(_p(_c32(mom)), Nb, C, HW, _p(_c32(noise)), _p(out), _s()) == 0
    torch.cuda.synchronize()
    share = _bound(out[:Nb * C * HW].reshape(Nb, C, HW), want, allow, "seer_gaussian_sample")
    print(f"edge_matrix | seer_gaussian_sample | share of the allowance used {share:.3f}")
    _guard_holds(out, Nb * C * HW, "gaussian_sample")


# =========================================================================================== 3. refusals
def test_edge_refusals(device):
    L = _L()
    s = _s()
    buf = torch.zeros((1 << 16,), device=device)
    w16 = torch.zeros((1 << 16,), device=device, dtype=bf16)
    ints = torch.zeros((64,), device=device, dtype=i64)
    y = torch.full((1 << 16,), float("nan"), device=device)
    X, W, I, Y = _p(buf), _p(w16), _p(ints), _p(y)
    checks = [
        # seer_linear_smallm(x, B, K, W, bias, N, silu_in, silu_out, y, dtype)
        ("linear_smallm B = 9", L.seer_linear_smallm, (X, 9, 64, W, None, 8, 0, 0, Y, 0), EINVAL),
        ("linear_smallm K = 12", L.seer_linear_smallm, (X, 2, 12, W, None, 8, 0, 0, Y, 0), EINVAL),
        ("linear_smallm B = 0", L.seer_linear_smallm, (X, 0, 64, W, None, 8, 0, 0, Y, 0), EINVAL),
        ("linear_smallm N = 0", L.seer_linear_smallm, (X, 2, 64, W, None, 0, 0, 0, Y, 0), EINVAL),
        ("linear_smallm K = 0", L.seer_linear_smallm, (X, 2, 0, W, None, 8, 0, 0, Y, 0), EINVAL),
        ("linear_smallm x NULL", L.seer_linear_smallm, (None, 2, 64, W, None, 8, 0, 0, Y, 0), EINVAL),
        ("linear_smallm W NULL", L.seer_linear_smallm, (X, 2, 64, None, None, 8, 0, 0, Y, 0), EINVAL),
        ("linear_smallm y NULL", L.seer_linear_smallm, (X, 2, 64, W, None, 8, 0, 0, None, 0), EINVAL),
        ("linear_smallm bad dtype", L.seer_linear_smallm, (X, 2, 64, W, None, 8, 0, 0, Y, 7), EINVAL),
        ("linear_smallm B K above 160 KiB of LDS", L.seer_linear_smallm, (X, 8, 5128, W, None, 8, 0, 0, Y, 0), EINVAL),
        # seer_conv_in(x, B, Cin, F, H, W, Wt, bias, Cout, y, dtype)
        ("conv_in Cout = 2056", L.seer_conv_in, (X, 1, 1, 1, 3, 3, X, None, 2056, Y, 0), EINVAL),
        ("conv_in Cout % 8", L.seer_conv_in, (X, 1, 4, 1, 3, 3, X, None, 12, Y, 0), EINVAL),
        ("conv_in LDS above 160 KiB (Cin 4, Cout 1200)", L.seer_conv_in, (X, 1, 4, 1, 3, 3, X, None, 1200, Y, 0), EINVAL),
        ("conv_in LDS above 160 KiB (Cin 4, Cout 1824)", L.seer_conv_in, (X,) + N.CONV_IN_REFUSED[:5] + (X, None, 1824, Y, 0), EINVAL),
        ("conv_in H = 0", L.seer_conv_in, (X, 1, 4, 1, 0, 3, X, None, 8, Y, 0), EINVAL),
        ("conv_in x NULL", L.seer_conv_in, (None, 1, 4, 1, 3, 3, X, None, 8, Y, 0), EINVAL),
        ("conv_in weights NULL", L.seer_conv_in, (X, 1, 4, 1, 3, 3, None, None, 8, Y, 0), EINVAL),
        ("conv_in y NULL", L.seer_conv_in, (X, 1, 4, 1, 3, 3, X, None, 8, None, 0), EINVAL),
        ("conv_in bad dtype", L.seer_conv_in, (X, 1, 4, 1, 3, 3, X, None, 8, Y, 7), EINVAL),
        # seer_conv_out(x, B, C0, F, H, W, Wt, bias, Cout, y, dtype)
        ("conv_out f16 with Cout = 4", L.seer_conv_out, (W, 1, 8, 1, 3, 3, X, None, 4, Y, 1), ENOSYS),
        ("conv_out bf16 with Cout = 5", L.seer_conv_out, (W, 1, 8, 1, 3, 3, X, None, 5, Y, 0), ENOSYS),
        ("conv_out C0 % 8", L.seer_conv_out, (W, 1, 12, 1, 3, 3, X, None, 4, Y, 0), EINVAL),
        ("conv_out bad dtype", L.seer_conv_out, (W, 1, 8, 1, 3, 3, X, None, 4, Y, 7), EINVAL),
        ("conv_out x NULL", L.seer_conv_out, (None, 1, 8, 1, 3, 3, X, None, 4, Y, 0), EINVAL),
        ("conv_out y NULL", L.seer_conv_out, (W, 1, 8, 1, 3, 3, X, None, 4, None, 0), EINVAL),
        ("conv_out W = 0", L.seer_conv_out, (W, 1, 8, 1, 3, 0, X, None, 4, Y, 0), EINVAL),
        ("conv_out weights above 160 KiB of LDS", L.seer_conv_out, (W, 1, 1280, 1, 3, 3, X, None, 4, Y, 0), EINVAL),
        # seer_cfg_ddim_step(eps, cfg, b, C, F_total, cond_f, HW, scale, coef, index, step, x, noise, seeds, temperature, x_prev, pred_x0), host form
        ("cfg_ddim F_total == cond_f", L.seer_cfg_ddim_step, (X, 1, 1, 4, 2, 2, 8, 7.5, X, 0, None, X, None, None, 0.0, Y, None), EINVAL),
        ("cfg_ddim cond_f < 0", L.seer_cfg_ddim_step, (X, 1, 1, 4, 2, -1, 8, 7.5, X, 0, None, X, None, None, 0.0, Y, None), EINVAL),
        ("cfg_ddim index < 0", L.seer_cfg_ddim_step, (X, 1, 1, 4, 2, 1, 8, 7.5, X, -1, None, X, None, None, 0.0, Y, None), EINVAL),
        ("cfg_ddim b = 0", L.seer_cfg_ddim_step, (X, 1, 0, 4, 2, 1, 8, 7.5, X, 0, None, X, None, None, 0.0, Y, None), EINVAL),
        ("cfg_ddim eps NULL", L.seer_cfg_ddim_step, (None, 1, 1, 4, 2, 1, 8, 7.5, X, 0, None, X, None, None, 0.0, Y, None), EINVAL),
        ("cfg_ddim coef NULL", L.seer_cfg_ddim_step, (X, 1, 1, 4, 2, 1, 8, 7.5, None, 0, None, X, None, None, 0.0, Y, None), EINVAL),
        ("cfg_ddim x_prev NULL", L.seer_cfg_ddim_step, (X, 1, 1, 4, 2, 1, 8, 7.5, X, 0, None, X, None, None, 0.0, None, None), EINVAL),
        # the same, device form: index = -1 and step
        ("cfg_ddim_dev F_total == cond_f", L.seer_cfg_ddim_step, (X, 1, 1, 4, 2, 2, 8, 7.5, X, -1, I, X, None, None, 0.0, Y, None), EINVAL),
        ("cfg_ddim_dev step NULL", L.seer_cfg_ddim_step, (X, 1, 1, 4, 2, 1, 8, 7.5, X, -1, None, X, None, None, 0.0, Y, None), EINVAL),
        ("cfg_ddim_dev HW = 0", L.seer_cfg_ddim_step, (X, 1, 1, 4, 2, 1, 0, 7.5, X, -1, I, X, None, None, 0.0, Y, None), EINVAL),
        # seer_ddim_step_begin(x0_emb, x, b, reps, C, f1, F_pred, HW, t_table, step, sample, t_out)
        ("step_begin f1 > 0 without x0_emb", L.seer_ddim_step_begin, (None, X, 1, 2, 4, 1, 2, 8, I, I, Y, I), EINVAL),
        ("step_begin reps = 0", L.seer_ddim_step_begin, (X, X, 1, 0, 4, 1, 2, 8, I, I, Y, I), EINVAL),
        ("step_begin F_pred = 0", L.seer_ddim_step_begin, (X, X, 1, 2, 4, 1, 0, 8, I, I, Y, I), EINVAL),
        ("step_begin f1 < 0", L.seer_ddim_step_begin, (X, X, 1, 2, 4, -1, 2, 8, I, I, Y, I), EINVAL),
        ("step_begin t_table NULL", L.seer_ddim_step_begin, (X, X, 1, 2, 4, 1, 2, 8, None, I, Y, I), EINVAL),
        ("step_begin step NULL", L.seer_ddim_step_begin, (X, X, 1, 2, 4, 1, 2, 8, I, None, Y, I), EINVAL),
        ("step_begin sample NULL", L.seer_ddim_step_begin, (X, X, 1, 2, 4, 1, 2, 8, I, I, None, I), EINVAL),
        ("step_begin t_out NULL", L.seer_ddim_step_begin, (X, X, 1, 2, 4, 1, 2, 8, I, I, Y, None), EINVAL),
        # rotary
        ("rotary_table T = 0", L.seer_rotary_table, (X, 0, 16, Y), EINVAL), ("rotary_table half = 0", L.seer_rotary_table, (X, 8, 0, Y), EINVAL),
        ("rotary_table freqs NULL", L.seer_rotary_table, (None, 8, 16, Y), EINVAL),
        # seer_rotary_inplace(x, rows, ld, col0_q, col0_k, heads, head_dim, rot_dim, tokens_per_batch, pos_offset, cos_sin)
        ("rotary rot_dim % 8", L.seer_rotary_inplace, (Y, 4, 960, 0, 320, 8, 40, 20, 4, 0, X), EINVAL),
        ("rotary rot_dim > head_dim", L.seer_rotary_inplace, (Y, 4, 960, 0, 320, 8, 40, 48, 4, 0, X), EINVAL),
        ("rotary ld % 8", L.seer_rotary_inplace, (Y, 4, 964, 0, 320, 8, 40, 32, 4, 0, X), EINVAL),
        ("rotary col0_q % 8", L.seer_rotary_inplace, (Y, 4, 960, 4, 320, 8, 40, 32, 4, 0, X), EINVAL),
        ("rotary col0_k % 8", L.seer_rotary_inplace, (Y, 4, 960, 0, 324, 8, 40, 32, 4, 0, X), EINVAL),
        ("rotary head_dim % 8", L.seer_rotary_inplace, (Y, 4, 960, 0, 320, 8, 36, 32, 4, 0, X), EINVAL),
        ("rotary tokens_per_batch = 0", L.seer_rotary_inplace, (Y, 4, 960, 0, 320, 8, 40, 32, 0, 0, X), EINVAL),
        ("rotary heads = 0", L.seer_rotary_inplace, (Y, 4, 960, 0, 320, 0, 40, 32, 4, 0, X), EINVAL),
        ("rotary table NULL", L.seer_rotary_inplace, (Y, 4, 960, 0, 320, 8, 40, 32, 4, 0, None), EINVAL),
        # the rest
        ("timestep_embedding odd dim", L.seer_timestep_embedding, (I, 2, 321, 1, 0.0, Y), EINVAL),
        ("timestep_embedding B = 0", L.seer_timestep_embedding, (I, 0, 320, 1, 0.0, Y), EINVAL),
        ("timestep_embedding t NULL", L.seer_timestep_embedding, (None, 2, 320, 1, 0.0, Y), EINVAL),
        ("cast n = 0", L.seer_cast_f32, (X, 0, Y, 0), EINVAL), ("cast bad dtype", L.seer_cast_f32, (X, 8, Y, 7), EINVAL), ("cast y NULL", L.seer_cast_f32, (X, 8, None, 0), EINVAL),
        ("nchw -> nhwc C = 0", L.seer_nchw_f32_to_nhwc_bf16, (X, 1, 0, 8, Y), EINVAL), ("nchw -> nhwc y NULL", L.seer_nchw_f32_to_nhwc_bf16, (X, 1, 4, 8, None), EINVAL),
        ("nhwc -> nchw HW = 0", L.seer_nhwc_bf16_to_nchw_f32, (W, 1, 4, 0, Y), EINVAL), ("nhwc -> nchw x NULL", L.seer_nhwc_bf16_to_nchw_f32, (None, 1, 4, 8, Y), EINVAL),
        ("conv1x1 Cin = 0", L.seer_conv1x1_nchw_f32, (X, 1, 0, 4, 8, X, None, Y), EINVAL), ("conv1x1 weights NULL", L.seer_conv1x1_nchw_f32, (X, 1, 4, 4, 8, None, None, Y), EINVAL),
        ("clamp01 n = 0", L.seer_clamp01, (Y, 0), EINVAL), ("clamp01 x NULL", L.seer_clamp01, (None, 8), EINVAL),
        ("gaussian_sample C = 0", L.seer_gaussian_sample, (X, 1, 0, 8, None, Y), EINVAL), ("gaussian_sample out NULL", L.seer_gaussian_sample, (X, 1, 4, 8, None, None), EINVAL),
    ]
    for name, fn, args, code in checks:
        assert fn(*args, s) == code, f"{name}: expected {code}"
    torch.cuda.synchronize()
    assert bool(y.isnan().all()) and not bool(ints.any()), "a refused launch wrote"
