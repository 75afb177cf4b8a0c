"""csrc/norm.hip -- the seven GroupNorm entry points, seer_layernorm and seer_softmax_rows -- tested exactly, per owner and at their
edges: part 5 of the series after test_gpu_f16_matrix.py, test_gpu_train_matrix.py, test_gpu_attn_fwd_matrix.py and
test_gpu_fused320_matrix.py.  The older tests (test_groupnorm, test_layernorm, test_softmax_rows in test_gpu_kernels.py and their
twins in test_gpu_f16.py) read atol = rtol = 2e-2 on data with one distribution everywhere: statistics that miss the last row block or
a count wrong by a row pass there (tests/test_norm_edge_ref_cpu.py prints what they read on each mutation).

1. EXACT, zero tolerance.  Integer inputs with a distinct integer offset per (batch element, group) or row: the fp32 sums are exact,
   every 16-bit store is one round-to-nearest-even of a known number, and at rsqrtf the following 16-bit rounding absorbs the error
   (tests/norm_edge_ref.py asserts the preconditions on the float64 reference, case by case; a failing precondition is an error).
   Outputs are NaN-prefilled, guarded or row-strided where the entry point allows; every launch runs twice and must repeat its bits.
2. PER OWNER against float64 on N(b, 4^b) data at amplitudes 1 and 4: the kernel's worst (row, group) segment or row may be at most 2x
   the worst of the float64 emulation that rounds where the kernels round.  Nothing in the bound comes from the kernel.
3. Every SEER_EINVAL / SEER_ENOSYS branch, decided on the host: NaN-filled outputs keep their bits.

Measured values, the instantiation each shape reaches, the mutation table and run times: profiles/norm_edge_matrix.md."""
import pytest
import torch

from tests import fused320_ref as R
from tests import norm_edge_ref as N
from tests.test_gpu_f16_matrix import _eq, _store
from tests.test_gpu_train_matrix import _gapped, _gaps_hold

pytestmark = pytest.mark.gpu

f16, bf16, f32, f64, i64 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int64
DTS = [pytest.param(bf16, id="bf16"), pytest.param(f16, id="f16")]
EINVAL, ENOSYS = -22, -38
GUARD = 64


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


def _arena(n, dev, dtype):
    """n NaN elements of output in front of GUARD NaN sentinels, one allocation"""
    return torch.full((n + GUARD,), float("nan"), device=dev, dtype=dtype)


def _guard_holds(a, n, what):
    assert bool(a[n:].isnan().all()), f"{what}: a store behind the output"


def _split(x, C1, C2, dt):
    """x [B, rows, C1 + C2] float64 -> the two contiguous 16-bit sources [B rows, C1], [B rows, C2] (or None)"""
    B, rows, C = x.shape
    x1 = _store(x[..., :C1].reshape(B * rows, C1).contiguous(), dt)
    x2 = _store(x[..., C1:].reshape(B * rows, C2).contiguous(), dt) if C2 else None
    return x1, x2


# =========================================================================================== 1. GroupNorm statistics, exact
def _gn_stats(x1, x2, B, rows, G, dt):
    L = _L()
    C1, C2 = x1.shape[1], 0 if x2 is None else x2.shape[1]
    nws = L.seer_groupnorm_workspace_floats(C1 + C2, B, rows, G)
    assert nws > 0
    ws = _arena(nws, x1.device, f32)
    st = _arena(B * G * 2, x1.device, f32)
    assert L.seer_groupnorm_stats(_p(x1), C1, _p(x2), C2, B, rows, G, _p(st), _p(ws), _dtc(dt), _s()) == 0
    torch.cuda.synchronize()
    _guard_holds(st, B * G * 2, "stats")
    _guard_holds(ws, nws, "workspace")
    return st[:B * G * 2].reshape(B, G, 2).clone()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", N.GN_STATS_SHAPES, ids=N.gn_id)
def test_exact_gn_stats(device, dt, shape):
    B, rows, C1, C2, G = shape
    x, _ = N.gn_exact_x(B, rows, C1 + C2, G, device, 11 + rows)
    want = N.gn_sums(x, G)
    x1, x2 = _split(x, C1, C2, dt)
    got = _gn_stats(x1, x2, B, rows, G, dt)
    _eq(got, want, dt, f"seer_groupnorm_stats {N.gn_id(shape)}")
    assert torch.equal(_bits(got), _bits(_gn_stats(x1, x2, B, rows, G, dt))), "two launches differ"


@pytest.mark.parametrize("one,two", [((1, 1), None), ((4, 3), None), ((1, 40), (2, 17)), ((2, 17), (4, 3)), ((1, 1), (1, 40))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_exact_gn_stats_from_colsums(device, one, two):
    """synthetic [phases][tiles][C][2] integer partials in the header's layout, one and two sources with different (phases, tiles)"""
    B, G = 3, 32
    C1, C2 = (640, 320) if two else (960, 0)
    cs1 = N.colsum_partials(one[0], one[1], B, C1, G, device, 21)
    cs2 = N.colsum_partials(two[0], two[1], B, C2, G, device, 22) if two else None
    want = N.colsums_to_stats([cs1] + ([cs2] if two else []), B, G)
    c1, c2 = cs1.to(f32).contiguous(), None if cs2 is None else cs2.to(f32).contiguous()
    outs = []
    for _ in range(2):
        st = _arena(B * G * 2, device, f32)
        rc = _L().seer_groupnorm_stats_from_colsums(_p(c1), C1, one[0], B * one[1], _p(c2), C2, two[0] if two else 0, B * two[1] if two else 0, B, G,
                                                    _p(st), _s())
        assert rc == 0
        torch.cuda.synchronize()
        _guard_holds(st, B * G * 2, "stats")
        outs.append(st[:B * G * 2].reshape(B, G, 2))
    _eq(outs[0], want, f32, f"seer_groupnorm_stats_from_colsums {one} {two}")
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two launches differ"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mag", [1.0, 2.0 ** -12, 2.0 ** 7], ids=["x1", "x2^-12", "x2^7"])
@pytest.mark.parametrize("C,rows,B", N.FX_SHAPES)
def test_exact_gn_stats_fx(device, dt, C, rows, B, mag):
    """integer sums of round(v 2^20) and round(v v 2^20), ADDED to an arena that already holds non-zero totals"""
    x = (R.ints((B, rows, C), device, 31 + C) + (torch.arange(B, device=device, dtype=f64) - 1)[:, None, None]) * mag
    x16 = _store(x.reshape(B * rows, C), dt)
    want = N.fx_sums(x)
    pre = torch.randint(-(1 << 40), 1 << 40, (B * 2 * C + GUARD,), generator=torch.Generator().manual_seed(C)).to(device)
    outs = []
    for _ in range(2):
        a = pre.clone()
        assert _L().seer_groupnorm_stats_fx(_p(x16), C, B, rows, _p(a), _dtc(dt), _s()) == 0
        torch.cuda.synchronize()
        outs.append(a)
    assert torch.equal(outs[0][:B * 2 * C].reshape(B, 2, C) - pre[:B * 2 * C].reshape(B, 2, C), want), f"seer_groupnorm_stats_fx C{C} rows{rows} B{B} x{mag}"
    assert torch.equal(outs[0][B * 2 * C:], pre[B * 2 * C:]), "a store behind the arena"
    assert torch.equal(outs[0], outs[1]), "two launches differ"


# =========================================================================================== 1. GroupNorm apply, exact
def _apply(form, x1, x2, gn, B, rows, G, dt, silu=0, stats_out=None, y=None):
    """one launch of the apply entry point of `form` into a guarded NaN arena -> (rc, y [B, rows, C], arena)"""
    L = _L()
    dev = x1.device
    C1, C2 = x1.shape[1], 0 if x2 is None else x2.shape[1]
    C = C1 + C2
    a = _arena(B * rows * C, dev, dt) if y is None else y
    gamma, beta = gn["gamma"].to(f32).contiguous(), gn["beta"].to(f32).contiguous()
    if form == "stats":
        st = gn["stats"].to(f32).contiguous()
        assert torch.equal(st.to(f64), gn["stats"])
        rc = L.seer_groupnorm_apply(_p(x1), C1, _p(x2), C2, B, rows, G, _p(st), gn["count"], gn["eps"], _p(gamma), _p(beta), silu, _p(a), _dtc(dt), _s())
    elif form == "cs":
        cs = [c.to(f32).contiguous() for c in gn["cs"]]
        for c, c64 in zip(cs, gn["cs"]):
            assert torch.equal(c.to(f64), c64)
        c2 = cs[1] if len(cs) > 1 else None
        rc = L.seer_groupnorm_apply_from_colsums(_p(x1), C1, _p(x2), C2, _p(cs[0]), cs[0].shape[0], cs[0].shape[1], _p(c2), c2.shape[0] if c2 is not None else 0,
                                                 c2.shape[1] if c2 is not None else 0, B, rows, G, gn["count"], gn["eps"], _p(gamma), _p(beta), silu, _p(a),
                                                 _dtc(dt), _s())
    else:
        fx = [t.contiguous() for t in gn["fx"]]
        f2 = fx[1] if len(fx) > 1 else None
        rc = L.seer_groupnorm_apply_fx(_p(x1), C1, _p(x2), C2, _p(fx[0]), fx[0].shape[0], _p(f2), f2.shape[0] if f2 is not None else 0, B, rows, G,
                                       gn["count"], gn["eps"], _p(gamma), _p(beta), silu, _p(a), _p(stats_out), _dtc(dt), _s())
    torch.cuda.synchronize()
    return rc, a[:B * rows * C].reshape(B, rows, C), a


_FORM_VARIANTS = [("stats", 1), ("cs", 1), ("cs", 12), ("cs", 32), ("fx", 1), ("fx", 3)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form,n", _FORM_VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", N.GN_APPLY_SHAPES, ids=N.gn_id)
def test_exact_gn_apply(device, dt, shape, form, n):
    """the TEST supplies the statistics (mean a distinct integer, variance 1, count 1024); SiLU off.  n: partials per batch element
    (from_colsums) or replicas (fx).  A layout a form refuses on the host is asserted to be refused, with the output untouched"""
    B, rows, C1, C2, G = shape
    C = C1 + C2
    cpg = C // G
    x, m = N.gn_exact_x(B, rows, C, G, device, 41 + rows)
    gn = N.exact_gn(form, B, G, C, device, 41 + rows, reps=n, parts=n, m=m, splits=(C1, C2))
    x1, x2 = _split(x, C1, C2, dt)
    what = f"groupnorm apply {form}{n} {N.gn_id(shape)} {_name(dt)}"
    if form != "stats" and N.gn_cs_geom(C, G, B, rows) is None:
        rc, y, a = _apply(form, x1, x2, gn, B, rows, G, dt)
        assert rc == ENOSYS and bool(a.isnan().all()), f"{what}: the one-launch forms do not slice this layout into whole groups"
        return
    want = N.gn_apply(x, gn, dt, exact=True)                                # asserts every precondition; never skipped
    so = _arena(B * G * 2, device, f32) if form == "fx" else None
    rc, y, a = _apply(form, x1, x2, gn, B, rows, G, dt, stats_out=so)
    assert rc == 0, f"{what}: returned {rc}"
    _eq(y, want, dt, what)
    _guard_holds(a, B * rows * C, what)
    if so is not None:
        _eq(so[:B * G * 2].reshape(B, G, 2), gn["totals"], f32, f"{what}: stats_out")
        _guard_holds(so, B * G * 2, f"{what}: stats_out")
    first = y.clone()
    rc, y2, _ = _apply(form, x1, x2, gn, B, rows, G, dt)
    assert rc == 0 and torch.equal(_bits(first), _bits(y2)), f"{what}: two launches differ"
    # one statistic altered: exactly the block of that (batch element, group) changes
    b, g = B - 1 if B > 1 else 0, G // 2
    m2 = m.clone()
    m2[b, g] = m.max() + 7
    gn2 = N.exact_gn(form, B, G, C, device, 41 + rows, reps=n, parts=n, m=m2, splits=(C1, C2))
    rc, y3, _ = _apply(form, x1, x2, gn2, B, rows, G, dt)
    assert rc == 0
    diff = _bits(y3) != _bits(first)
    block = torch.zeros_like(diff)
    block[b, :, g * cpg:(g + 1) * cpg] = True
    assert torch.equal(diff, block), f"{what}: altering the statistics of (b {b}, g {g}) changed {int((diff & ~block).sum())} elements outside its block " \
                                     f"and left {int((~diff & block).sum())} inside it"


# =========================================================================================== 1. LayerNorm, exact
def _layernorm(x16, gamma, beta, eps, dt, alias=False):
    rows, C = x16.shape
    xb, xv = _gapped(x16)
    if alias:
        yb, yv = xb, xv
    else:
        yb, yv = _gapped(torch.full((rows, C), float("nan"), device=x16.device, dtype=dt))
    g, b = gamma.to(f32).contiguous(), beta.to(f32).contiguous()
    rc = _L().seer_layernorm(_p(xv), rows, C, xv.stride(0), _p(g), _p(b), eps, _p(yv), yv.stride(0), _dtc(dt), _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _gaps_hold(yb, rows, C, "layernorm: y")
    if not alias:
        assert torch.equal(_bits(xv), _bits(x16)), "layernorm wrote x"
    return yv


_LN_CASES = [(r, c) for c in N.LN_CS for r in N.LN_ROWS] + N.LN_LONG


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,C", _LN_CASES)
def test_exact_layernorm(device, dt, rows, C):
    x, pm, m = N.ln_exact_x(rows, C, device, 51 + C)
    gamma, beta = N.ln_affine(C, device, 52 + C)
    want = N.ln_exact(x, pm, gamma, beta, 1e-5, dt)
    x16 = _store(x, dt)
    what = f"seer_layernorm rows{rows} C{C} {_name(dt)}"
    y = _layernorm(x16, gamma, beta, 1e-5, dt)
    _eq(y, want, dt, what)
    y2 = _layernorm(x16, gamma, beta, 1e-5, dt)
    assert torch.equal(_bits(y), _bits(y2)), f"{what}: two launches differ"
    y3 = _layernorm(x16, gamma, beta, 1e-5, dt, alias=True)
    _eq(y3, want, dt, f"{what}, y aliasing x")


# =========================================================================================== 1. softmax rows, exact
def _softmax(x, x_is_f32, rows, n, ld, scale, dt, pad=56):
    """x: the tensor whose data_ptr / ld the entry point gets.  y has ldy = n + pad inside a NaN buffer with a guard row"""
    ldy = n + pad
    yb = torch.full((rows + 1, ldy), float("nan"), device=x.device, dtype=dt)
    rc = _L().seer_softmax_rows(_p(x), int(x_is_f32), rows, n, ld, scale, _p(yb), ldy, _dtc(dt), _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool(yb[:rows, n:].isnan().all()) and bool(yb[rows:].isnan().all()), "softmax: a store outside its rows"
    return yb[:rows, :n]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("in_f32", [True, False], ids=["x_f32", "x_16"])
@pytest.mark.parametrize("rows", N.SM_ROWS)
@pytest.mark.parametrize("n", N.SM_NS)
def test_exact_softmax_rows(device, dt, in_f32, rows, n):
    x, want = N.softmax_exact(rows, n, device, 61 + n + rows)
    xin = x.to(f32) if in_f32 else _store(x, dt)
    what = f"seer_softmax_rows rows{rows} n{n} {_name(dt)}"
    for scale in (1.0, 0.25):
        y = _softmax(xin, in_f32, rows, n, n, scale, dt)
        _eq(y, want, dt, f"{what} scale {scale}")
        assert torch.equal(_bits(y), _bits(_softmax(xin, in_f32, rows, n, n, scale, dt))), f"{what}: two launches differ"
    # a row-strided x (the C entry point: ops.softmax_rows asserts contiguity)
    xb = torch.full((rows, n + 24), float("nan"), device=device, dtype=xin.dtype)
    xb[:, 8:8 + n] = xin
    _eq(_softmax(xb[:, 8:], in_f32, rows, n, n + 24, 1.0, dt), want, dt, f"{what}, x strided")


# =========================================================================================== 2. per owner against float64
def _judge(tag, ek, ee):
    print(f"norm_matrix owners | {tag} | emulation {ee:.4g} | kernel {ek:.4g} | ratio {ek / ee if ee > 0 else float('inf'):.3f}")
    assert ek <= 2 * ee, f"{tag}: worst owner {ek:.4g} above 2x the emulation's {ee:.4g}"


_GN_ROWS = [(2, 100, 320, 0, 32, None), (3, 45, 640, 320, 32, None), (1, 9, 2560, 0, 32, None), (2, 61, 288, 0, 32, None), (2, 100, 320, 0, 32, 8.0)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("amp", [1.0, 4.0])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("form", ["stats", "cs", "fx"])
@pytest.mark.parametrize("B,rows,C1,C2,G,ratio", _GN_ROWS, ids=lambda v: str(v))
def test_owners_groupnorm(device, dt, amp, silu, form, B, rows, C1, C2, G, ratio):
    """statistics from the kernels' own statistics entry points (seer_groupnorm_stats, seer_groupnorm_stats_fx; the column sums of a
    producer per 16-row tile, formed here in float64 and stored as fp32 as a producer stores them), then the apply form"""
    C = C1 + C2
    x16, gamma, beta = N.gn_random(B, rows, C, G, dt, device, 71 + rows, amp, ratio)
    x1, x2 = _split(x16, C1, C2, dt)
    gn = N.stats_of(x16, G, form, device, 72, reps=1)
    gn.update(gamma=gamma, beta=beta)
    ref, emu = N.gn_apply(x16, dict(gn, form="stats", stats=N.gn_sums(x16, G)), None, bool(silu)), N.gn_apply(x16, gn, dt, bool(silu))
    run = dict(gn)
    if form == "stats":
        run["stats"] = _gn_stats(x1, x2, B, rows, G, dt).to(f64)
    elif form == "fx":
        fx = torch.zeros((1, B, 2, C), device=device, dtype=i64)
        xc = _store(x16.reshape(B * rows, C), dt)
        assert _L().seer_groupnorm_stats_fx(_p(xc), C, B, rows, _p(fx), _dtc(dt), _s()) == 0
        torch.cuda.synchronize()
        assert torch.equal(fx[0], N.fx_sums(x16)), "seer_groupnorm_stats_fx: not the integer sums"
        run["fx"] = [fx[..., :C1].contiguous()] + ([fx[..., C1:].contiguous()] if C2 else [])
    else:
        run["cs"] = [gn["cs"][0][:, :, :C1].contiguous()] + ([gn["cs"][0][:, :, C1:].contiguous()] if C2 else [])
    rc, y, a = _apply(form, x1, x2, run, B, rows, G, dt, silu=silu)
    assert rc == 0, rc
    assert bool(torch.isfinite(y.float()).all())
    _guard_holds(a, B * rows * C, "y")
    cpg = C // G
    _judge(f"groupnorm {form} {_name(dt)} B{B} r{rows} C{C1}+{C2} silu{silu} x{amp:g} ratio {ratio}", N.seg_err(y, ref, cpg), N.seg_err(emu, ref, cpg))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("amp", [1.0, 4.0])
@pytest.mark.parametrize("C", [320, 520, 1536])
def test_owners_layernorm(device, dt, amp, C):
    rows = 37
    x16, gamma, beta = N.ln_random(rows, C, dt, device, 81 + C, amp)
    ref, emu = N.layernorm(x16, gamma, beta, 1e-5), N.layernorm(x16, gamma, beta, 1e-5, dt)
    y = _layernorm(_store(x16, dt), gamma, beta, 1e-5, dt)
    floor = R.row_floor(ref)
    _judge(f"layernorm {_name(dt)} C{C} x{amp:g}", R.row_err(y, ref, floor), R.row_err(emu, ref, floor))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("in_f32", [True, False], ids=["x_f32", "x_16"])
@pytest.mark.parametrize("spread", [1.0, 30.0])
@pytest.mark.parametrize("n", [520, 2056, 4096])
def test_owners_softmax_rows(device, dt, in_f32, spread, n):
    rows = 13
    x = N.softmax_random(rows, n, spread, f32 if in_f32 else dt, device, 91 + n)
    ref, emu = N.softmax_rows(x, 0.125), N.softmax_rows(x, 0.125, dt)
    y = _softmax(x.to(f32) if in_f32 else _store(x, dt), in_f32, rows, n, n, 0.125, dt)
    floor = R.row_floor(ref)
    _judge(f"softmax {_name(dt)} {'f32' if in_f32 else '16'} n{n} spread {spread:g}", R.row_err(y, ref, floor), R.row_err(emu, ref, floor))


# =========================================================================================== 3. refusals
def test_layernorm_softmax_refusals(device):
    L = _L()
    x = torch.zeros((4, 4200), device=device, dtype=bf16)
    xf = torch.zeros((4, 4200), device=device, dtype=f32)
    g = torch.ones(4200, device=device)
    y = torch.full((4, 4200), float("nan"), device=device, dtype=bf16)
    X, XF, Gp, Y, s = _p(x), _p(xf), _p(g), _p(y), _s()
    ln = lambda **k: L.seer_layernorm(*[{**dict(x=X, rows=4, C=320, ldx=4200, gamma=Gp, beta=Gp, eps=1e-5, y=Y, ldy=4200, dtype=0, s=s), **k}[n] for n in
                                       ("x", "rows", "C", "ldx", "gamma", "beta", "eps", "y", "ldy", "dtype", "s")])
    for name, over, code in [("C = 1544", dict(C=1544), ENOSYS), ("C % 8", dict(C=324), EINVAL), ("ldx % 8", dict(ldx=4204), EINVAL),
                             ("ldy % 8", dict(ldy=4204), EINVAL), ("rows 0", dict(rows=0), EINVAL), ("C 0", dict(C=0), EINVAL),
                             ("x NULL", dict(x=None), EINVAL), ("y NULL", dict(y=None), EINVAL), ("gamma NULL", dict(gamma=None), EINVAL),
                             ("beta NULL", dict(beta=None), EINVAL), ("bad dtype", dict(dtype=7), EINVAL),
                             ("bad dtype ahead of ENOSYS", dict(dtype=7, C=1544), EINVAL)]:
        assert ln(**over) == code, f"seer_layernorm {name}"
    sm = lambda **k: L.seer_softmax_rows(*[{**dict(x=XF, f=1, rows=4, n=1024, ld=4200, scale=1.0, y=Y, ldy=4200, dtype=0, s=s), **k}[n] for n in
                                           ("x", "f", "rows", "n", "ld", "scale", "y", "ldy", "dtype", "s")])
    for name, over, code in [("n = 4104", dict(n=4104), ENOSYS), ("n = 60", dict(n=60), EINVAL), ("n 0", dict(n=0), EINVAL), ("ld % 8", dict(ld=4204), EINVAL),
                             ("ldy % 8", dict(ldy=4204), EINVAL), ("rows 0", dict(rows=0), EINVAL), ("x NULL", dict(x=None), EINVAL),
                             ("y NULL", dict(y=None), EINVAL), ("bad dtype", dict(dtype=7), EINVAL), ("bad dtype ahead of ENOSYS", dict(dtype=7, n=4104), EINVAL)]:
        assert sm(**over) == code, f"seer_softmax_rows {name}"
    torch.cuda.synchronize()
    assert bool(y.isnan().all()), "a refused launch wrote"
    assert ln() == 0 and sm() == 0, "the unchanged arguments must launch"


def test_groupnorm_refusals(device):
    L = _L()
    B, rows, C, G = 2, 16, 320, 32
    x = torch.zeros((B * rows, 640), device=device, dtype=bf16)
    st = torch.zeros((B, 64, 2), device=device)
    ws = torch.zeros((1 << 16,), device=device)
    gb = torch.ones(640, device=device)
    cs = torch.zeros((40 * B * 640 * 2,), device=device)
    fx = torch.zeros((3 * B * 2 * 640,), device=device, dtype=i64)
    y = torch.full((B * rows, 640), float("nan"), device=device, dtype=bf16)
    nan_st = torch.full((B, 64, 2), float("nan"), device=device)
    X, ST, WS, GB, CS, FX, Y, NS, s = _p(x), _p(st), _p(ws), _p(gb), _p(cs), _p(fx), _p(y), _p(nan_st), _s()

    def stats(**k):
        a = {**dict(x1=X, C1=C, x2=None, C2=0, B=B, rows=rows, G=G, st=NS, ws=WS, dt=0), **k}
        return L.seer_groupnorm_stats(a["x1"], a["C1"], a["x2"], a["C2"], a["B"], a["rows"], a["G"], a["st"], a["ws"], a["dt"], s)

    def apply(**k):
        a = {**dict(x1=X, C1=C, x2=None, C2=0, B=B, rows=rows, G=G, st=ST, count=160.0, gamma=GB, beta=GB, y=Y, dt=0), **k}
        return L.seer_groupnorm_apply(a["x1"], a["C1"], a["x2"], a["C2"], a["B"], a["rows"], a["G"], a["st"], a["count"], 1e-6, a["gamma"], a["beta"], 0,
                                      a["y"], a["dt"], s)

    def apply_cs(**k):
        a = {**dict(x1=X, C1=C, x2=None, C2=0, cs1=CS, ph1=1, t1=B, cs2=None, ph2=0, t2=0, B=B, rows=rows, G=G, count=160.0, gamma=GB, beta=GB, y=Y, dt=0), **k}
        return L.seer_groupnorm_apply_from_colsums(a["x1"], a["C1"], a["x2"], a["C2"], a["cs1"], a["ph1"], a["t1"], a["cs2"], a["ph2"], a["t2"], a["B"],
                                                   a["rows"], a["G"], a["count"], 1e-6, a["gamma"], a["beta"], 0, a["y"], a["dt"], s)

    def apply_fx(**k):
        a = {**dict(x1=X, C1=C, x2=None, C2=0, fx1=FX, r1=1, fx2=None, r2=0, B=B, rows=rows, G=G, count=160.0, gamma=GB, beta=GB, y=Y, dt=0), **k}
        return L.seer_groupnorm_apply_fx(a["x1"], a["C1"], a["x2"], a["C2"], a["fx1"], a["r1"], a["fx2"], a["r2"], a["B"], a["rows"], a["G"], a["count"], 1e-6,
                                         a["gamma"], a["beta"], 0, a["y"], None, a["dt"], s)

    def from_cs(**k):
        a = {**dict(cs1=CS, C1=C, ph1=1, t1=B, cs2=None, C2=0, ph2=0, t2=0, B=B, G=G, st=NS), **k}
        return L.seer_groupnorm_stats_from_colsums(a["cs1"], a["C1"], a["ph1"], a["t1"], a["cs2"], a["C2"], a["ph2"], a["t2"], a["B"], a["G"], a["st"], s)

    geometry = [("cpg 2", dict(C1=64, G=32)), ("cpg 5", dict(C1=160, G=32)), ("cpg 6", dict(C1=192, G=32)), ("groups 65", dict(C1=520, G=65)),
                ("C % groups", dict(C1=328, G=32)), ("C1 % 8", dict(C1=324, G=4)), ("groups 0", dict(G=0)), ("C2 % 8", dict(x2=X, C2=316, G=4))]
    common = [("x1 NULL", dict(x1=None)), ("batch 0", dict(B=0)), ("rows 0", dict(rows=0)), ("bad dtype", dict(dt=7))]
    for name, over in geometry + common + [("stats NULL", dict(st=None)), ("workspace NULL", dict(ws=None))]:
        assert stats(**over) == EINVAL, f"seer_groupnorm_stats {name}"
    for name, over in geometry + common + [("stats NULL", dict(st=None)), ("gamma NULL", dict(gamma=None)), ("beta NULL", dict(beta=None)),
                                           ("y NULL", dict(y=None)), ("count 0", dict(count=0.0))]:
        assert apply(**over) == EINVAL, f"seer_groupnorm_apply {name}"
    assert L.seer_groupnorm_workspace_floats(64, 2, 16, 32) == EINVAL
    one_launch = [("cpg 2: no slice of whole groups", dict(C1=64, G=32), ENOSYS), ("cpg 257", dict(C1=2056, G=8), ENOSYS),
                  ("groups 65", dict(C1=520, G=65), ENOSYS), ("x1 NULL", dict(x1=None), EINVAL), ("gamma NULL", dict(gamma=None), EINVAL),
                  ("beta NULL", dict(beta=None), EINVAL), ("y NULL", dict(y=None), EINVAL), ("count 0", dict(count=0.0), EINVAL), ("batch 0", dict(B=0), EINVAL),
                  ("rows 0", dict(rows=0), EINVAL), ("bad dtype", dict(dt=7), EINVAL)]
    for name, over, code in one_launch + [("cs1 NULL", dict(cs1=None), EINVAL), ("tiles % batch", dict(t1=3), EINVAL), ("phases 0", dict(ph1=0), EINVAL),
                                          ("tiles 0", dict(t1=0), EINVAL), ("cs2 NULL with C2", dict(x2=X, C2=320), EINVAL),
                                          ("tiles2 % batch", dict(x2=X, C2=320, cs2=CS, ph2=1, t2=3), EINVAL),
                                          ("more than 32 partials", dict(ph1=3, t1=B * 11), ENOSYS), ("33 partials in the second source", dict(x2=X, C2=320, cs2=CS, ph2=1, t2=B * 33), ENOSYS),
                                          ("a tensor above 4.2 M elements", dict(rows=13200), ENOSYS)]:
        assert apply_cs(**over) == code, f"seer_groupnorm_apply_from_colsums {name}"
    for name, over, code in one_launch + [("fx1 NULL", dict(fx1=None), EINVAL), ("reps 0", dict(r1=0), EINVAL), ("fx2 NULL with C2", dict(x2=X, C2=320), EINVAL),
                                          ("reps2 0", dict(x2=X, C2=320, fx2=FX, r2=0), EINVAL)]:
        assert apply_fx(**over) == code, f"seer_groupnorm_apply_fx {name}"
    for name, over in [("cs1 NULL", dict(cs1=None)), ("stats NULL", dict(st=None)), ("batch 0", dict(B=0)), ("groups 0", dict(G=0)), ("C1 0", dict(C1=0)),
                       ("phases 0", dict(ph1=0)), ("tiles 0", dict(t1=0)), ("tiles % batch", dict(t1=3)), ("C % groups", dict(C1=328)),
                       ("tiles2 % batch", dict(cs2=CS, C2=320, ph2=1, t2=3)), ("phases2 0", dict(cs2=CS, C2=320, ph2=0, t2=B))]:
        assert from_cs(**over) == EINVAL, f"seer_groupnorm_stats_from_colsums {name}"
    for name, args in [("x NULL", (None, C, B, rows, FX, 0)), ("fx NULL", (X, C, B, rows, None, 0)), ("C % 8", (X, 324, B, rows, FX, 0)), ("C 0", (X, 0, B, rows, FX, 0)),
                       ("batch 0", (X, C, 0, rows, FX, 0)), ("rows 0", (X, C, B, 0, FX, 0)), ("bad dtype", (X, C, B, rows, FX, 7))]:
        assert L.seer_groupnorm_stats_fx(*args, s) == EINVAL, f"seer_groupnorm_stats_fx {name}"
    torch.cuda.synchronize()
    assert bool(y.isnan().all()) and bool(nan_st.isnan().all()) and not bool(fx.any()), "a refused launch wrote"
    assert stats() == 0 and apply() == 0 and apply_cs() == 0 and apply_fx() == 0 and from_cs() == 0, "the unchanged arguments must launch"
