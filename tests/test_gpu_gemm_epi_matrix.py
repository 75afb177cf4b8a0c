"""The EPILOGUES of the tile kernel (csrc/gemm_tile_kernel.h, all 18 tile codes, plain / GEGLU / conv / split form), of its split-K second
pass (csrc/gemm_reduce.hip, three reduce kernels) and of the weight-stationary kernel (csrc/gemm_ws.hip), tested as the 256 x 320 kernel
is in tests/test_gpu_t320_matrix.py.  Every launch PROVES which kernel it ran: the descriptor handed to seer_gemm_bf16 is captured
(tests/gemm_spy.py) and seer_gemm_plan of it must read the intended [status, kernel, tile, K slices, reduce pass]; the plan is printed.
Four parts:

1. EXACT, zero tolerance.  The integer constructions of tests/t320_ref.py (operands in [-3, 3], terms in [-8, 8], every partial sum an
   integer below 2^24): the fp32 accumulator is exact whatever the order and the slice count, and the one rounding to the storage type
   is fully determined.  A, A2, the residual and the output are gapped views inside NaN-filled buffers; every launch runs twice and
   must repeat its bits, the gaps keep their NaN bits.  fp32 output, row statistics and accumulated column sums are integer equalities.
   The case table (tests/gemm_epi_ref.py) is chosen from the kernels' own conditions: tests/test_gemm_epi_ref_cpu.py asserts from
   body_of() that it reaches both epilogue bodies for every term on every representative tile.
2. PER OWN ROW against float64 for what integers cannot reach (GEGLU on N(0, 1) gates, rotary from seer_rotary_table, SiLU and
   quick-GELU -- unsplit and through the split-K second pass, plain and with both column-sum forms --, the folded LayerNorm with the
   producer's row statistics): the kernel's worst row within 2x the worst row of a float64
   emulation that rounds only where the kernels round (listed in gemm_epi_ref.py).  Nothing in the bound comes from the kernel.
3. THE BODIES AGREE: the same rows as full tiles (fast body), into an unstaged output (general body) and inside a ragged launch.
4. REFUSALS and fall-backs, decided on the host.

That the constructions can fail: tests/test_gemm_epi_ref_cpu.py (mutation table).  Measured values: profiles/gemm_epi_matrix.md."""
import pytest
import torch

from tests import gemm_epi_ref as R
from tests import t320_ref as T
from tests.gemm_spy import spy  # noqa: F401  (the fixture)
from tests.test_gpu_f16_matrix import _eq, _store
from tests.test_gpu_train_matrix import _gapped

pytestmark = pytest.mark.gpu

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")


def _dt(spec):
    return f16 if spec.get("dt") == "f16" else bf16


def _bits(t):
    return t.view(torch.int32 if t.dtype == f32 else torch.int16)


# =========================================================================================== operands as views
def _out_buffer(M, n, dev, dt, c0=8):
    """a NaN buffer [M + 1, n + 16] and its view [:M, c0:c0 + n]: c0 = 8 is 16-byte aligned, c0 = 4 only 8-byte aligned (unstaged)"""
    buf = torch.full((M + 1, n + 16), NAN, device=dev, dtype=dt)
    return buf, buf[:M, c0:c0 + n]


def _holds(buf, M, c0, n, what):
    """everything outside the view still holds the bits it was filled with"""
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:M, c0:c0 + n] = False
    fill = _bits(torch.full((1,), NAN, device=buf.device, dtype=buf.dtype))[0]
    bad = _bits(buf)[keep] != fill
    assert not bool(bad.any()), f"{what}: a store outside the slice ({int(bad.sum())} elements)"


def _wide(t, extra):
    buf, view = _gapped(torch.cat([t, torch.full((t.shape[0], extra), NAN, device=t.device, dtype=t.dtype)], 1))
    return view[:, :t.shape[1]]


def _res_view(res, kind):
    """the residual through t320_ref's three views: lds (ldr % 8 == 0 where the width allows, 16-byte aligned), ldr4 (a leading dimension
    4 off), base8 (a base that is 8- but not 16-byte aligned)"""
    M, N = res.shape
    if kind == "ldr4":
        v = _wide(res, 4)
    elif kind == "base8":
        buf = torch.full((M + 1, N + 16), NAN, device=res.device, dtype=res.dtype)
        v = buf[:M, 4:4 + N]
        v.copy_(res)
        assert v.data_ptr() % 16 == 8
    else:
        v = _gapped(res)[1]
        assert v.data_ptr() % 16 == 0
    return v


def _check_plan(spy, spec, what):
    want, got = R.planned(spec), spy.plans[-1]
    ok = all(w is None or w == g for w, g in zip(want, got))
    assert ok, f"{what}: planned {got}, meant {want}"


def _launch_kwargs(dev, spec, p, dt):
    """the keyword arguments of ops.gemm for a problem, the operands stored in `dt` as views with gaps"""
    N = p["w"].shape[0]
    kw, w = {}, p["w"]
    bias = p.get("bias")
    if p.get("a2") is not None:
        kw["a2"] = _wide(_store(p["a2"], dt), 8)
    if p.get("geglu"):
        order = R.interleave_order(N // 2, dev)
        w, bias = w[order], (None if bias is None else bias[order])
        kw["geglu"] = True
    if bias is not None:
        kw["bias"] = bias.float().contiguous()
    if p.get("rowvec") is not None:
        kw.update(rowvec=p["rowvec"].float(), rows_per_batch=p["rows_per_batch"])
    if p.get("res") is not None:
        kw["residual"] = _res_view(_store(p["res"], dt), spec.get("res"))
    if p.get("rot") is not None:
        r = p["rot"]
        kw["rotary"] = (r["table"], r["tokens"], r["off"], r["head_dim"], r["rot_dim"], r["cols"])
    if p.get("col_scale") is not None:
        kw["col_scale"] = p["col_scale"]
    for k, name in (("silu", "silu"), ("qgelu", "quick_gelu"), ("rowstat", "rowstat")):
        if p.get(k):
            kw[name] = True
    return _store(w, dt).contiguous(), kw


def _run_gemm(dev, spy, spec, p, c0=None, twice=True):
    """one ops.gemm launch of `p` as `spec` asks (tile, splits, storage type, fp32 output, column sums), twice; returns (output view, what)"""
    from seervideoldm_amd import ops
    dt = _dt(spec)
    M, N = p["a"].shape[0], p["w"].shape[0]
    n_out = N // 2 if p.get("geglu") else N
    what = "gemm_epi " + R.case_id(spec) + (f" M{M}" if M != spec.get("M") else "")
    c0 = (4 if spec.get("n_off") else 8) if c0 is None else c0
    a = _gapped(_store(p["a"], dt))[1]
    w16, kw = _launch_kwargs(dev, spec, p, dt)
    if kw.get("a2") is not None:
        assert kw["a2"].stride(0) != a.stride(0)
    buf, view = _out_buffer(M, n_out, dev, f32 if spec.get("f32") else dt, c0)
    spy.keep.append((a, w16, kw, buf))                                   # the captured descriptors point at these
    form = spec.get("colsum")
    B = M // spec["rpb"] if form else 0

    def launch():
        cb = (B, ops.FxArena(dev, 1 << 16)) if form == "fx" else B
        out = ops.gemm(a, w16, out=view, tile=spec["tile"], splits=spec.get("splits", 1), colsum_batch=cb, **kw)
        _check_plan(spy, spec, what)
        return out
    out = launch()
    if twice:
        first = buf.clone()
        view.fill_(NAN)
        out = launch()
        assert torch.equal(_bits(first), _bits(buf)), f"{what}: two launches differ"
    _holds(buf, M, c0, n_out, what)
    print(f"gemm_epi_matrix plan | {what} | {spy.plans[-1]}")
    return out, what


def _check_colsums(y, stored, spec, what):
    from seervideoldm_amd import ops
    M, gets = spec["M"], spec.get("gets", spec["colsum"])
    B = M // spec["rpb"]
    cs = y.colsums
    if gets is None:
        assert cs is None, f"{what}: column sums on partials that straddle batch elements"
    elif gets == "tiles":
        rows = 16 if M >= 2048 else 4
        assert isinstance(cs, ops.ColSums), f"{what}: no per-strip column sums"
        want = R.colsum_tiles(stored, rows)
        assert tuple(cs.buf.shape) == tuple(want.shape), (cs.buf.shape, want.shape)
        bad = cs.buf.to(f64) != want
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} partial sums differ, first at {bad.nonzero()[0].tolist()}"
    else:
        rows = 64 if M >= 1024 else 32
        assert isinstance(cs, ops.ColSumsFx), f"{what}: no accumulated column sums"
        want = R.colsum_fx(stored, rows, M // B, cs.reps)
        assert torch.equal(cs.buf, want), f"{what}: accumulated sums off by up to {(cs.buf - want).abs().max().item() / 2 ** 20}"


# =========================================================================================== 1. exact arithmetic
def _exact_case(dev, spy, spec):
    p = R.exact_problem(spec, dev)
    want = R.exact_reference(spec, p)
    out, what = _run_gemm(dev, spy, spec, p)
    _eq(out, want["pre"], _dt(spec), what)
    return p, want, out, what


@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.GEMM_EXACT if not s.get("trans")])
def test_exact_tile_epilogue(device, spy, spec):
    """every term alone and together at the edges of rows, columns, output alignment, row-vector batches, residual views, column scale,
    rotary, GEGLU, two sources, fp32 output, SiLU / quick-GELU and row statistics on the six representative tiles; all terms on all 18"""
    p, want, out, what = _exact_case(device, spy, spec)
    if spec.get("rowstat"):
        assert out.rowstats is not None, f"{what}: no row statistics"
        assert torch.equal(out.rowstats.buf, want["rowstat"]), f"{what}: row statistics differ in {int((out.rowstats.buf != want['rowstat']).any(1).sum())} rows"


@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.GEMM_EXACT if s.get("trans")])
def test_exact_transposed_output(device, spy, spec):
    """Ct[n * ldc + m], one and two batch elements with strideA / W / C (ops.gemm_batched), 16-bit and fp32; bias and column scale"""
    from seervideoldm_amd import ops
    dev, Bt, dt = device, spec["batch"], _dt(spec)
    M, N = spec["M"], spec["N"]
    ps = [R.exact_problem(dict(spec, seed=spec["seed"] + 500 * b), dev) for b in range(Bt)]
    for q in ps:
        q["bias"] = ps[0]["bias"]
    wants = [R.exact_reference(spec, q) for q in ps]
    a = torch.stack([_store(q["a"], dt) for q in ps]).contiguous()
    w = torch.stack([_store(q["w"], dt) for q in ps]).contiguous()
    buf = torch.full((Bt, N, M), NAN, device=dev, dtype=f32 if spec.get("f32") else dt)
    what = "gemm_epi " + R.case_id(spec)
    for _ in range(2):
        buf.fill_(NAN)
        ops.gemm_batched(a, w, trans_out=True, out=buf, bias=ps[0]["bias"].float(), tile=spec["tile"], col_scale=ps[0]["col_scale"])
        _check_plan(spy, spec, what)
        for b in range(Bt):
            _eq(buf[b], wants[b]["pre"], dt, f"{what} batch element {b}")
    print(f"gemm_epi_matrix plan | {what} | {spy.plans[-1]}")


@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.SPLIT_EXACT])
def test_exact_splitk_reduce(device, spy, spec):
    """seer_splitk_reduce_kernel behind the split forms of 64x64, G128x128_2, G64x64_3 and G96x160_2: the terms alone and together, two
    and three slices, ragged rows and column tiles, N = 68"""
    _exact_case(device, spy, spec)


@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.SPLIT_SUMS])
def test_exact_splitk_reduce_column_sums(device, spy, spec):
    """the reduce passes with per-strip and with accumulated column sums: sums of the STORED values with the terms applied, strip by
    strip / replica by replica; a partial that would straddle batch elements is not admitted and the output is exact all the same"""
    p, want, out, what = _exact_case(device, spy, spec)
    _check_colsums(out, want["out"], spec, what)


@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.WS_EXACT])
def test_exact_weight_stationary(device, spy, spec):
    """tile = 19 where the plan reads SEER_GEMM_KERNEL_WS: K = 320 / 640, a ragged row tail, N across one panel, bias, the column scale
    inside a wave's columns and past the first panel, GEGLU, two sources, both storage types"""
    _exact_case(device, spy, spec)


def test_exact_layout_invariant_request(device, spy):
    """SEER_TILE_AUTO_INVARIANT keeps every tile on the general body: 192 rows alone and as the first rows of 384 are the same bits, and
    both are the reference"""
    s384 = R.INV_EXACT[1]
    p = R.exact_problem(s384, device)
    want = R.exact_reference(s384, p)
    assert R.bodies_of(s384, 16) == {"general"}
    big, what = _run_gemm(device, spy, s384, p)
    _eq(big, want["pre"], bf16, what)
    small, what = _run_gemm(device, spy, dict(s384, M=192), R.head_rows(p, 192))
    _eq(small, want["pre"][:192], bf16, what)
    assert torch.equal(_bits(small), _bits(big[:192])), "the first 192 rows differ between the two launches"


@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.CONV_EXACT])
def test_exact_conv_epilogue(device, spy, spec):
    """bias + row vector + residual on the implicit-GEMM form at stride 1 / 2 and with pad_after_only, bias + column scale on the four
    phase convs, on G96x160_2 and 64x64; image boundaries inside a tile"""
    from seervideoldm_amd import ops
    from seervideoldm_amd import _lib
    from seervideoldm_amd.weights import pack_conv3x3, pack_conv3x3_up_phases
    dev = device
    p = R.exact_problem(spec, dev)
    want = R.exact_reference(spec, p)
    x, w = p["x"], p["w"]
    n, Ci, H, W = x.shape
    Co, M = w.shape[0], want["pre"].shape[0]
    what = "gemm_epi " + R.case_id(spec)
    x_cl = _store(x.permute(0, 2, 3, 1).reshape(-1, Ci).contiguous(), bf16)
    kw = {"bias": p["bias"].float()}
    if p.get("rowvec") is not None:
        kw.update(rowvec=p["rowvec"].float(), rows_per_batch=p["rows_per_batch"])
    if p.get("res") is not None:
        kw["residual"] = _res_view(_store(p["res"], bf16), spec["res"])
    if spec.get("up"):
        w4 = pack_conv3x3_up_phases(w.float())
        assert torch.equal(w4, w4.round())
        w16 = _store(w4.to(f64), bf16)
        scale, cols = p["col_scale"]

        def tweak(d):                                                    # (the wrapper has no column-scale argument)
            d.epilogue |= _lib.SEER_EPI_COLSCALE
            d.col_scale, d.col_scale_cols = scale, cols
        spy.tweak = tweak
    else:
        w16 = pack_conv3x3(_store(w, bf16))
    buf, view = _out_buffer(M, Co, dev, bf16)
    first = None
    for _ in range(2):
        view.fill_(NAN)
        if spec.get("up"):
            out = ops.conv_up2x(x_cl, w16, n, H, W, out=view, tile=spec["tile"], **kw)
        else:
            out = ops.conv3x3(x_cl, w16, n, H, W, stride=p["stride"], pad_after_only=p["pad_after"], out=view, tile=spec["tile"], **kw)
        _check_plan(spy, spec, what)
        assert first is None or torch.equal(_bits(first), _bits(buf)), f"{what}: two launches differ"
        first = buf.clone()
    print(f"gemm_epi_matrix plan | {what} | {spy.plans[-1]}")
    _eq(out, want["pre"], bf16, what)
    _holds(buf, M, 8, Co, what)


# =========================================================================================== 2. per own row against float64
def _seer_table(rows, rot_dim, dev):
    from seervideoldm_amd import ops
    freqs = (10000.0 ** (-torch.arange(0, rot_dim, 2, dtype=f32) / rot_dim)).to(dev)
    return ops.rotary_table(freqs, rows)


def _folded(w, gamma, beta, b):
    from seervideoldm_amd import ops
    return tuple(t.to(f64) for t in ops.fold_layernorm(_store(w, bf16), gamma.float(), beta.float(), b.float()))


def _producer(dev, spy, tile, M, amp):
    """the GEMM that leaves rows and row statistics; returns (stored rows of the REFERENCE as float64, the reference's statistics, the
    kernel's RowStats).  The kernel's rows are held to the row criterion, its statistics to the fp32 summation bound"""
    from seervideoldm_amd import ops
    pp = R.producer_problem(tile, M, amp, dev)
    ref = R.gemm(pp, tile=tile)
    spec = dict(tile=tile, M=M, N=R.LN_K, K=128, bias=True, res="lds", rowstat=True, seed=0)
    h, what = _run_gemm(dev, spy, spec, pp, twice=False)
    floor = T.row_floor(ref["pre"])
    ek, ee = T.row_err(h, ref["pre"], floor), T.row_err(ref["out"], ref["pre"], floor)
    assert ek <= 2 * ee, f"{what}: worst row {ek:.4g} above 2x the emulation's {ee:.4g}"
    assert h.rowstats is not None, f"{what}: no row statistics"
    # fp32 adds of N values (and K products behind each): |error| <= (N + K) 2^-23 sum |v| for the sum, likewise for the squares
    v = ref["pre"]
    tol = (R.LN_K + 128) * 2.0 ** -23
    got = h.rowstats.buf.to(f64) / float(1 << R.LN_SHIFT)
    assert bool(((got[:, 0] - v.sum(1)).abs() <= tol * v.abs().sum(1) + 2.0 ** -20).all()), f"{what}: row sums off"
    assert bool(((got[:, 1] - v.pow(2).sum(1)).abs() <= 2 * tol * v.pow(2).sum(1) + 2.0 ** -20).all()), f"{what}: row sums of squares off"
    return ref["out"], ref["rowstat"], h.rowstats


def _consumer(dev, spy, kind, tile, M, amp, x16, stats_ref, rs_kernel, rows=None):
    """the folded-LayerNorm launch on the first `rows` rows; returns (kernel output, emulation, reference, what)"""
    from seervideoldm_amd import ops
    rows = rows or M
    p, plain = R.consumer_problem(kind, tile, M, amp, x16, stats_ref, dev, make_table=_seer_table, folded=_folded)
    if rows != M:
        p = dict(R.head_rows(p, rows), ln=dict(p["ln"], stats=stats_ref[:rows]))
    emu, ref = R.gemm(p, tile=tile), R.ln_reference(p, plain)
    N = p["w"].shape[0]
    n_out = N // 2 if p.get("geglu") else N
    spec = dict(tile=tile, M=rows, N=N, K=R.LN_K, ln=True, geglu=bool(p.get("geglu")), rot=p.get("rot") is not None)
    what = f"gemm_epi {kind} {R.TILES[tile][0]} M{rows} x{amp:g}"
    a = _gapped(_store(p["a"], bf16))[1]
    w16, kw = _launch_kwargs(dev, spec, {k: v for k, v in p.items() if k != "ln"}, bf16)
    wsum = p["ln"]["wsum"]
    if p.get("geglu"):
        wsum = wsum[R.interleave_order(N // 2, dev)]
    buf, view = _out_buffer(rows, n_out, dev, bf16)
    out = ops.gemm(a, w16, out=view, tile=tile, ln=(ops.RowStats(rs_kernel.buf[:rows].contiguous()), wsum.float().contiguous(), 1e-5), **kw)
    assert out is not None, f"{what}: the host does not fold this launch"
    _check_plan(spy, spec, what)
    _holds(buf, rows, 8, n_out, what)
    assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    return out, emu, ref, what


@pytest.mark.parametrize("kind,tile,M,amp", [c for c in R.ROWS_CASES if c[0].startswith("ln")])
def test_rows_folded_layernorm(device, spy, kind, tile, M, amp):
    """norm -> projection, norm3 -> ff.net.0 (GEGLU), norm1 -> q | k | v (rotary + column scale): the producer's row statistics feed the
    consumer; rows N(b, 4^b) per batch element; full tiles (fast body) and a ragged last tile (general body)"""
    x16, stats_ref, rs = _producer(device, spy, tile, M, amp)
    out, emu, ref, what = _consumer(device, spy, kind, tile, M, amp, x16, stats_ref, rs)
    floor = T.row_floor(ref)
    ek, ee = T.row_err(out, ref, floor), T.row_err(emu["out"], ref, floor)
    bodies = sorted(R.bodies_of(dict(M=M, N=emu["pre"].shape[1] * (2 if kind == "ln_geglu" else 1), geglu=kind == "ln_geglu", rot=kind == "ln_rot", cs=kind == "ln_rot"), tile))
    print(f"gemm_epi_matrix rows | {kind} {R.TILES[tile][0]} M{M} x{amp:g} | bodies {bodies} | plan {spy.plans[-1]} | emulation {ee:.4g} | kernel {ek:.4g} | ratio {ek / ee:.3f}")
    assert ek <= 2 * ee, f"{what}: worst row {ek:.4g} above 2x the emulation's {ee:.4g}"


@pytest.mark.parametrize("tile", [5, 14])
def test_rows_ln_geglu_bodies_recorded(device, spy, tile):
    """the folded LayerNorm in front of a GEGLU is where the source says the two bodies differ in their last bits: the same rows as full
    tiles and inside a ragged launch, each within the bound; their difference is printed, bit equality is NOT asserted"""
    BM = R.TILES[tile][1]
    M = 2 * BM
    x16, stats_ref, rs = _producer(device, spy, tile, M, 1.0)
    full, emu, ref, _ = _consumer(device, spy, "ln_geglu", tile, M, 1.0, x16, stats_ref, rs)
    rag, emu_r, ref_r, what = _consumer(device, spy, "ln_geglu", tile, M, 1.0, x16, stats_ref, rs, rows=M - 27)
    floor = T.row_floor(ref)
    for o, e, r in ((full, emu, ref), (rag, emu_r, ref_r)):
        assert T.row_err(o, r, floor) <= 2 * T.row_err(e["out"], r, floor)
    d = full[BM:M - 27].to(f64) - rag[BM:].to(f64)
    worst = float((d.norm(dim=-1) / ref[BM:M - 27].norm(dim=-1).clamp_min(floor)).max())
    print(f"gemm_epi_matrix rows | ln_geglu {R.TILES[tile][0]} | fast body against general body on rows {BM} .. {M - 28}: worst row {worst:.4g}, "
          f"{int((d != 0).sum())} of {d.numel()} elements differ (recorded, not asserted)")


@pytest.mark.parametrize("kind,tile,M,amp", [c for c in R.ROWS_CASES if not c[0].startswith("ln")])
def test_rows_activations(device, spy, kind, tile, M, amp):
    """SiLU and quick-GELU behind bias and row vector, GEGLU on N(0, 1) gates, rotary from seer_rotary_table's own output: within 2x the
    once-rounded float64 result; SiLU / quick-GELU add 2x the error of a float32 CPU evaluation of the formula (expf)"""
    p = R.act_problem(kind, tile, M, amp, device, make_table=_seer_table)
    ref = R.gemm(p, tile=tile)
    N = p["w"].shape[0]
    spec = dict(tile=tile, M=M, N=N, K=192, geglu=kind == "geglu", rot=kind == "rot", silu=kind == "silu", qgelu=kind == "qgelu", seed=0)
    out, what = _run_gemm(device, spy, spec, p, twice=False)
    floor = T.row_floor(ref["pre"])
    ek, ee = T.row_err(out, ref["pre"], floor), T.row_err(ref["out"], ref["pre"], floor)
    e32 = R.act_f32_error(p, kind, ref["pre"]) if kind in ("silu", "qgelu") else 0.0
    print(f"gemm_epi_matrix rows | {kind} {R.TILES[tile][0]} M{M} x{amp:g} | plan {spy.plans[-1]} | emulation {ee:.4g} | float32 formula {e32:.4g} | "
          f"kernel {ek:.4g} | ratio {ek / ee:.3f}")
    assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    assert ek <= 2 * ee + 2 * e32, f"{what}: worst row {ek:.4g} above 2x the emulation's {ee:.4g} + 2x {e32:.4g}"


def _check_colsums_of_own_output(y, spec, what):
    """Part 2 has no exact sums: the column sums a reduce pass leaves are held to the float64 sums of the values IT stored, within the
    fp32 summation bound of a partial (rows adds: rows 2^-23 sum |v|) and, accumulated, the 2^-20 fixed-point step per partial"""
    from seervideoldm_amd import ops
    M, form = spec["M"], spec["colsum"]
    v = y.to(f64)
    if form == "tiles":
        rows = 16 if M >= 2048 else 4
        assert isinstance(y.colsums, ops.ColSums), f"{what}: no per-strip column sums"
        want, got = R.colsum_tiles(v, rows), y.colsums.buf.to(f64)
        mag = R.colsum_tiles(v.abs(), rows)
        tol = rows * 2.0 ** -23
        bad = (got - want).abs() > tol * torch.stack([mag[..., 0], 2 * mag[..., 1]], -1) + 2.0 ** -30
    else:
        rows, B = (64 if M >= 1024 else 32), 2
        assert isinstance(y.colsums, ops.ColSumsFx), f"{what}: no accumulated column sums"
        vb = v.reshape(B, M // B, -1)
        want, got = torch.stack([vb.sum(1), vb.pow(2).sum(1)], -1), y.colsums.totals()
        mag = torch.stack([vb.abs().sum(1), 2 * vb.pow(2).sum(1)], -1)
        bad = (got - want).abs() > rows * 2.0 ** -23 * mag + (M // B // rows) * 2.0 ** -20
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} column sums are not the sums of the stored values"


@pytest.mark.parametrize("kind,tile,M,N,K,S,form", R.ROWS_SPLIT)
def test_rows_splitk_activations(device, spy, kind, tile, M, N, K, S, form):
    """SiLU and quick-GELU in the split-K second pass (its own code, gemm_reduce.hip): bias + row vector in front, column scale +
    residual behind, two and three slices, the plain pass and both passes with column sums -- per own row as test_rows_activations"""
    spec, p = R.split_act_problem(kind, tile, M, N, K, S, form, device)
    ref = R.gemm(p, tile=tile)
    out, what = _run_gemm(device, spy, spec, p, twice=False)
    floor = T.row_floor(ref["pre"])
    ek, ee, e32 = T.row_err(out, ref["pre"], floor), T.row_err(ref["out"], ref["pre"], floor), R.act_f32_error(p, kind, ref["pre"])
    print(f"gemm_epi_matrix rows | split_{kind} {R.TILES[tile][0]} {M}x{N}x{K} S{S} sums {form} | plan {spy.plans[-1]} | emulation {ee:.4g} | "
          f"float32 formula {e32:.4g} | kernel {ek:.4g} | ratio {ek / ee:.3f}")
    assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    assert ek <= 2 * ee + 2 * e32, f"{what}: worst row {ek:.4g} above 2x the emulation's {ee:.4g} + 2x {e32:.4g}"
    if form:
        _check_colsums_of_own_output(out, spec, what)


# =========================================================================================== 3. the bodies agree
@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.bodies_cases()])
def test_bodies_agree(device, spy, spec):
    """the same rows as full tiles, into an output that is only 8-byte aligned (every block on the general body, unstaged) and as a
    launch whose second row tile is ragged (general body, staged): the same bits.  Which body each launch takes is asserted from body_of"""
    tile, BM, M = spec["tile"], R.TILES[spec["tile"]][1], spec["M"]
    p = R.exact_problem(spec, device)
    want = R.exact_reference(spec, p)
    term = next(k for k in ("geglu", "rot", "rpb") if spec.get(k))
    if "fast" in R.reachable("res" if spec.get("res") else term, tile) and "fast" in R.reachable(term, tile):
        assert R.bodies_of(spec, tile) == {"fast"}, R.bodies_of(spec, tile)
    assert R.bodies_of(dict(spec, n_off=4), tile) == {"general"} and "general" in R.bodies_of(dict(spec, M=M - 27), tile)
    full, what = _run_gemm(device, spy, spec, p)
    _eq(full, want["pre"], bf16, what)
    unstaged, _ = _run_gemm(device, spy, dict(spec, n_off=4), p)
    ragged, _ = _run_gemm(device, spy, dict(spec, M=M - 27), R.head_rows(p, M - 27))
    assert torch.equal(_bits(full), _bits(unstaged)), f"{what}: staged and unstaged launch differ"
    assert torch.equal(_bits(full[:M - 27]), _bits(ragged)), f"{what}: full-tile and ragged launch differ"
    print(f"gemm_epi_matrix bodies | {what} | full {sorted(R.bodies_of(spec, tile))} | unstaged ['general'] | ragged {sorted(R.bodies_of(dict(spec, M=M - 27), tile))}")


# =========================================================================================== 4. refusals and fall-backs
def _keeps_nan(buf):
    return bool((_bits(buf) == _bits(torch.full((1,), NAN, device=buf.device, dtype=buf.dtype))[0]).all())


def _base(dev, M=256, N=256, K=256, geglu=False):
    spec = R._c(5, M, N, K, bias=True, geglu=geglu, seed=3)
    return spec, R.exact_problem(spec, dev)


_REFUSED = ["geglu_colscale", "silu_quick_gelu", "rowstat_colsum_arg", "ln_misaligned_wsum", "colsum_geglu", "colsum_f32", "colsum_trans"]


@pytest.mark.parametrize("what", _REFUSED)
def test_requests_no_kernel_carries(device, spy, what):
    """SEER_EINVAL from the plan before any launch: the NaN-filled output keeps its bits"""
    from seervideoldm_amd import ops
    from seervideoldm_amd import _lib
    from seervideoldm_amd._lib import SeerHipError
    dev = device
    spec, p = _base(dev, geglu=what in ("geglu_colscale", "colsum_geglu"))
    a = _store(p["a"], bf16)
    w16, kw = _launch_kwargs(dev, spec, p, bf16)
    n_out = 128 if p.get("geglu") else 256
    buf, view = _out_buffer(256, n_out, dev, f32 if what == "colsum_f32" else bf16)
    seen = []
    sums = torch.zeros((64 * 256 * 2,), device=dev, dtype=f32)
    wsum = torch.zeros((260,), device=dev, dtype=f32)[1:257]             # 4 bytes off a 16-byte boundary
    stats = torch.zeros((256, 2), device=dev, dtype=torch.int64)

    def tweak(d):
        if what == "rowstat_colsum_arg":
            d.colsum = sums.data_ptr()
        elif what == "ln_misaligned_wsum":
            d.ln_rowstat, d.ln_wsum, d.ln_eps = stats.data_ptr(), wsum.data_ptr(), 1e-5
        elif what.startswith("colsum_"):
            d.colsum = sums.data_ptr()
            if what == "colsum_trans":
                d.epilogue |= _lib.SEER_EPI_TRANS_OUT
        seen.append(type(d).from_buffer_copy(d))
    spy.tweak = tweak
    if what == "geglu_colscale":
        kw["col_scale"] = (0.5, 64)
    elif what == "silu_quick_gelu":
        kw.update(silu=True, quick_gelu=True)
    elif what == "rowstat_colsum_arg":
        kw["rowstat"] = True
    assert wsum.data_ptr() % 16 == 4
    with pytest.raises(SeerHipError) as e:
        ops.gemm(a, w16, out=view, tile=5, **kw)
    # (refused by a size query in front of the launch, or by seer_gemm_bf16 itself from the plan: either way no kernel is started)
    assert "(-22)" in str(e.value) and all(pl == [-22, 0, 0, 0, 0] for pl in spy.plans) and spy.plan_of(seen[-1]) == [-22, 0, 0, 0, 0]
    assert _keeps_nan(buf), f"{what}: the call returned an error and still wrote"
    print(f"gemm_epi_matrix plan | {what} | [-22, 0, 0, 0, 0]: refused before any launch, the output keeps its bits")


@pytest.mark.parametrize("what", ["rowstat_geglu", "ln_a2_or_transposed", "ln_tile21", "ln_split", "ln_f32"])
def test_row_statistics_the_host_does_not_take(device, spy, what):
    """seer_gemm_rowstat_ok / seer_gemm_lnfold_ok say no on the host: a rowstat request launches without statistics (and is exact), a
    folded LayerNorm launches nothing (the caller runs layernorm() and the plain weights)"""
    from seervideoldm_amd import ops
    dev = device
    spec, p = _base(dev, geglu=what == "rowstat_geglu")
    want = R.exact_reference(spec, p)
    if what == "rowstat_geglu":
        out, w_ = _run_gemm(dev, spy, spec, dict(p, rowstat=True))
        assert out.rowstats is None
        _eq(out, want["pre"], bf16, w_)
        return
    a = _store(p["a"], bf16)
    w16, kw = _launch_kwargs(dev, spec, p, bf16)
    ln = (ops.RowStats(torch.zeros((256, 2), device=dev, dtype=torch.int64)), torch.zeros((256,), device=dev, dtype=f32), 1e-5)
    buf, view = _out_buffer(256, 256, dev, f32 if what == "ln_f32" else bf16)
    args = dict(tile=21 if what == "ln_tile21" else 5, splits=2 if what == "ln_split" else 1)
    if what == "ln_a2_or_transposed":
        # (ops.gemm asserts a2 is None with ln: the query is asked directly)
        from seervideoldm_amd import _lib
        import ctypes as C_
        d = _lib.GemmDesc()
        d.A, d.A2, d.W, d.C = a.data_ptr(), a.data_ptr(), w16.data_ptr(), view.data_ptr()
        d.M, d.N, d.K, d.K1, d.lda, d.lda2, d.ldc, d.mode, d.tile = 256, 256, 256, 128, 256, 256, view.stride(0), _lib.SEER_GEMM_PLAIN, 5
        d.ln_rowstat, d.ln_wsum, d.ln_eps = ln[0].buf.data_ptr(), ln[1].data_ptr(), 1e-5
        assert spy._real.seer_gemm_lnfold_ok(C_.byref(d)) == 0 and spy.plan_of(d)[0] == -22
        d.A2 = None
        d.K1 = 256
        assert spy._real.seer_gemm_lnfold_ok(C_.byref(d)) == 1, "the same descriptor without A2 folds"
        d.epilogue, d.ldc = _lib.SEER_EPI_TRANS_OUT, 256
        assert spy._real.seer_gemm_lnfold_ok(C_.byref(d)) == 0 and spy.plan_of(d)[0] == -22, "a transposed output does not fold"
        assert _keeps_nan(buf)
        return
    out = ops.gemm(a, w16, out=view, ln=ln, **args, **kw)
    if what == "ln_split":
        # a folded launch asked to slice K stays unsplit on the tile kernel
        assert out is not None and spy.plans[-1] == [0, R.K_TILE, 5, 1, 0], spy.plans
        return
    assert out is None and not spy.plans and _keeps_nan(buf), f"{what}: {spy.plans}"
    print(f"gemm_epi_matrix plan | {what} | the host does not fold: nothing launched")


@pytest.mark.parametrize("what", ["rotary", "rowvec", "residual", "m_below_1024", "k_384"])
def test_tile19_requests_that_fall_to_the_tile_kernel(device, spy, what):
    """a weight-stationary request the kernel is not eligible for runs on the tile kernel (the plan says so) and is exact"""
    dev = device
    M, K = (512 if what == "m_below_1024" else 1024), (384 if what == "k_384" else 320)
    terms = dict(bias=True)
    if what == "rotary":
        terms.update(rot=(40, 32, 96, 16, 200), cs=40)
    elif what == "rowvec":
        terms["rpb"] = 96
    elif what == "residual":
        terms["res"] = "lds"
    spec = R._c(R.WS, M, 264, K, seed=5, **terms)
    p = R.exact_problem(dict(spec, tile=5), dev)
    want = R.exact_reference(dict(spec, tile=5), p)
    from seervideoldm_amd import ops
    a = _gapped(_store(p["a"], bf16))[1]
    w16, kw = _launch_kwargs(dev, spec, p, bf16)
    buf, view = _out_buffer(M, 264, dev, bf16)
    out = ops.gemm(a, w16, out=view, tile=R.WS, **kw)
    plan = spy.plans[-1]
    assert plan[0] == 0 and plan[1] == R.K_TILE and plan[2] in R.TILES and plan[3:] == [1, 0], f"tile 19 with {what}: planned {plan}"
    print(f"gemm_epi_matrix plan | tile 19 with {what} | {plan}")
    _eq(out, want["pre"], bf16, f"tile 19 with {what}")
    _holds(buf, M, 8, 264, what)


@pytest.mark.parametrize("what", ["geglu", "rotary", "trans_out", "batch_2"])
def test_split_requests_the_planner_turns_unsplit(device, spy, what):
    """splits = 2 on a tile that has a split form, with a term the split form does not carry: one launch on the tile kernel, exact"""
    from seervideoldm_amd import ops
    dev = device
    if what in ("trans_out", "batch_2"):
        spec = R._c(5, 165, 136, 256, trans=what == "trans_out", batch=2 if what == "batch_2" else 1, bias=True, cs=20, seed=9)
        ps = [R.exact_problem(dict(spec, seed=9 + b), dev) for b in range(spec["batch"])]
        for q in ps:
            q["bias"] = ps[0]["bias"]
        a = torch.stack([_store(q["a"], bf16) for q in ps]).contiguous()
        w = torch.stack([_store(q["w"], bf16) for q in ps]).contiguous()
        buf = torch.full((len(ps), 136, 165) if what == "trans_out" else (len(ps), 165, 136), NAN, device=dev, dtype=bf16)

        def with_splits(dref, stream):                                   # (gemm_batched has no splits argument)
            dref._obj.splits = 2
            return type(spy).seer_gemm_bf16(spy, dref, stream)
        spy.seer_gemm_bf16 = with_splits
        ops.gemm_batched(a, w, trans_out=what == "trans_out", out=buf, bias=ps[0]["bias"].float(), tile=5, col_scale=ps[0]["col_scale"])
        assert spy.descs[-1].splits == 2 and spy.plans[-1] == [0, R.K_TILE, 5, 1, 0], spy.plans[-1]
        for b, q in enumerate(ps):
            _eq(buf[b], R.exact_reference(spec, q)["pre"], bf16, f"splits = 2 with {what}, batch element {b}")
    else:
        spec = R._c(5, 165, 288, 256, splits=2, seed=9, **(dict(geglu=True) if what == "geglu" else dict(bias=True, rot=(40, 32, 96, 16, 200), cs=40)))
        assert R.planned(spec) == [0, R.K_TILE, 5, 1, 0]
        _exact_case(dev, spy, spec)
    print(f"gemm_epi_matrix plan | splits = 2 with {what} | {spy.plans[-1]}")
