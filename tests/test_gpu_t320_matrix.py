"""The 256 x 320 tile GEMM / conv kernel (csrc/gemm_t320.hip, SEER_TILE_T256x320 = 22, plan kernel SEER_GEMM_KERNEL_T320) tested as the
other GEMM kernels are in tests/test_gpu_f16_matrix.py -- and every case PROVES it ran this kernel: tile = 22 silently falls back when
a launch is not eligible, so the descriptor ops._launch_gemm hands to seer_gemm_bf16 (workspace and sync filled in) is captured and
seer_gemm_plan of it must read [0, SEER_GEMM_KERNEL_T320, 22, S, 0] with the intended S.  Three parts:

1. EXACT, zero tolerance.  Integer operands in [-3, 3], bias / row vector / residual in [-8, 8]: every partial sum is an integer below
   2^24, the fp32 accumulator is exact whatever the order and the slice count, and the one rounding to bf16 is fully determined.  The
   activations, the residual and the output are row-strided views with a column offset inside NaN-filled buffers (W and a conv's input
   have no leading dimension in the descriptor: they are dense); the NaN pre-fill with exactness shows every element written, the gaps
   show none written outside.  Every launch runs twice and must repeat its bits; after a split launch the counters are zero.
2. PER OWN ROW against float64 for what integers cannot reach (GEGLU on N(0, 1) gates, rotary from the real table): the kernel's worst
   row within 2x the worst row of the float64 result rounded to bf16 once.  Nothing in the bound comes from the kernel.
3. REFUSALS and fall-backs, decided on the host.

References and the case table: tests/t320_ref.py (float64, no library).  That the constructions can fail: tests/test_t320_ref_cpu.py.
Measured values: profiles/t320_matrix.md."""
import ctypes as C_

import pytest
import torch

from tests import t320_ref as R
from tests.gemm_spy import spy  # noqa: F401  (the fixture)
from tests.test_gpu_f16_matrix import _eq, _ints, _store
from tests.test_gpu_t320 import _sync_is_zero
from tests.test_gpu_train_matrix import _gapped, _gaps_hold

pytestmark = pytest.mark.gpu

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
T320, K_T320 = R.T320, R.KERNEL_T320


# =========================================================================================== the plan of every launch
# (the `spy` fixture: tests/gemm_spy.py, shared with tests/test_gpu_gemm_epi_matrix.py)
def _ran_t320(spy, S, what):
    assert spy.plans[-1] == [0, K_T320, T320, S, 0], f"{what}: planned {spy.plans[-1]}, not the 256 x 320 kernel with {S} slice(s)"


def _ran_another(spy, what):
    assert spy.plans[-1][0] == 0 and spy.plans[-1][1] not in (0, K_T320), f"{what}: planned {spy.plans[-1]}"


# =========================================================================================== operands as views
def _nan_out(M, N, dev, dt=bf16):
    return _gapped(torch.full((M, N), NAN, device=dev, dtype=dt))


def _wide(t, extra):
    """_gapped with `extra` more spare columns behind the slice (a second leading dimension)"""
    buf, view = _gapped(torch.cat([t, torch.full((t.shape[0], extra), NAN, device=t.device, dtype=t.dtype)], 1))
    return view[:, :t.shape[1]]


def _res_view(res, kind):
    """the residual where the unsplit kernel takes it through LDS (ldr % 8 == 0, 16-byte aligned) and where it reads it directly"""
    M, N = res.shape
    if kind == "ldr4":
        v = _wide(res, 4)
        assert v.stride(0) % 8 == 4 and v.data_ptr() % 16 == 0
    elif kind == "base8":
        buf = torch.full((M + 1, N + 16), NAN, device=res.device, dtype=res.dtype)
        v = buf[:M, 4:4 + N]
        v.copy_(res)
        assert v.stride(0) % 8 == 0 and v.data_ptr() % 16 == 8
    else:
        v = _gapped(res)[1]
        assert v.stride(0) % 8 == 0 and v.data_ptr() % 16 == 0
    return v


def _epi_kwargs(p, spec):
    kw = {}
    if p.get("bias") is not None:
        kw["bias"] = p["bias"].float()
    if p.get("rowvec") is not None:
        kw.update(rowvec=p["rowvec"].float(), rows_per_batch=p["rows_per_batch"])
    if p.get("res") is not None:
        kw["residual"] = _res_view(_store(p["res"], bf16), spec.get("res"))
    return kw


def _twice(launch, buf, M, N, what, dev, split):
    """launch -> keep the buffer's bits -> NaN again -> launch: the same bits, nothing outside the slice, counters zero"""
    out = launch()
    first = buf.clone()
    buf[:M, 8:8 + N] = NAN
    out = launch()
    assert torch.equal(first.view(torch.int16), buf.view(torch.int16)), f"{what}: two launches differ"
    _gaps_hold(buf, M, N, what)
    if split:
        from seervideoldm_amd import ops
        assert ops._sync_buffers, f"{what}: a split launch without the counter buffer"
    assert _sync_is_zero(dev), f"{what}: the counters are not zero after the launch"
    return out


def _run_gemm(dev, spy, spec, p, colsum_batch=0):
    from seervideoldm_amd import ops
    M, N = p["a"].shape[0], p["w"].shape[0]
    n_out = N // 2 if p.get("geglu") else N
    what = "t320 " + R.case_id(spec)
    a = _gapped(_store(p["a"], bf16))[1]
    kw = _epi_kwargs(p, spec)
    w = p["w"]
    if p.get("a2") is not None:
        kw["a2"] = _wide(_store(p["a2"], bf16), 8)
        assert kw["a2"].stride(0) != a.stride(0)
    if p.get("geglu"):
        order = R.interleave_order(N // 2, dev)
        w, kw["bias"] = w[order], p["bias"][order].float().contiguous()
        kw["geglu"] = True
    if p.get("rot") is not None:
        r = p["rot"]
        kw["rotary"] = (r["table"], r["tokens"], r["off"], r["head_dim"], r["rot_dim"], r["cols"])
    if p.get("col_scale") is not None:
        kw["col_scale"] = p["col_scale"]
    w16 = _store(w, bf16).contiguous()
    buf, view = _nan_out(M, n_out, dev)
    S = R.planned_slices(p["w"].shape[1], spec.get("splits", 1))
    spy.keep.append((a, w16, kw, buf))                                   # the captured descriptors point at these

    def launch():
        arena = ops.FxArena(dev, 1 << 16) if isinstance(colsum_batch, tuple) else None
        out = ops.gemm(a, w16, out=view, tile=T320, splits=spec.get("splits", 1),
                       colsum_batch=(colsum_batch[0], arena) if arena is not None else colsum_batch, **kw)
        _ran_t320(spy, S, what)
        return out
    out = _twice(launch, buf, M, n_out, what, dev, S > 1)
    print(f"t320_matrix plan | {what} | {spy.plans[-1]}")
    return out, what


def _run_conv(dev, spy, spec, p, colsum_batch=0, tile=T320, expect="t320"):
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import pack_conv3x3, pack_conv3x3_up_phases
    x, w = p["x"], p["w"]
    n, Ci, H, W = x.shape
    Co = w.shape[0]
    what = "t320 conv " + R.case_id(spec)
    x_cl = _store(x.permute(0, 2, 3, 1).reshape(-1, Ci).contiguous(), bf16)
    kw = _epi_kwargs(p, spec)
    up = p.get("up")
    if up == "read_through":
        M = n * 4 * H * W
        w16 = pack_conv3x3(_store(w, bf16))
    elif up:
        M = n * 4 * H * W
        w4 = pack_conv3x3_up_phases(w.float())
        assert torch.equal(w4, w4.round()) and w4.abs().max() <= 12
        w16 = _store(w4.to(f64), bf16)
    else:
        pad = 1 if p["pad_after"] else 2
        M = n * ((H + pad - 3) // p["stride"] + 1) * ((W + pad - 3) // p["stride"] + 1)
        w16 = pack_conv3x3(_store(w, bf16))
    buf, view = _nan_out(M, Co, dev)
    S = R.planned_slices(9 * Ci, spec.get("splits", 1))

    def launch():
        arena = ops.FxArena(dev, 1 << 16) if isinstance(colsum_batch, tuple) else None
        cb = (colsum_batch[0], arena) if arena is not None else colsum_batch
        if up and up != "read_through":
            out = ops.conv_up2x(x_cl, w16, n, H, W, out=view, tile=tile, colsum_batch=cb, **kw)
        else:
            out = ops.conv3x3(x_cl, w16, n, H, W, stride=p["stride"], upsample=bool(up), pad_after_only=p["pad_after"], out=view, tile=tile,
                              splits=spec.get("splits", 1), colsum_batch=cb, **kw)
        if expect == "t320":
            _ran_t320(spy, 1 if up else S, what)
        else:
            _ran_another(spy, what)
        return out
    out = _twice(launch, buf, M, Co, what, dev, S > 1 and not up)
    print(f"t320_matrix plan | {what}{' upsample = 1' if up == 'read_through' else ''} | {spy.plans[-1]}")
    return out, what


# =========================================================================================== 1. exact arithmetic
@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.GEMM_EXACT])
def test_exact_gemm(device, spy, spec):
    """tile mapping, K loop and two sources, rounding, every epilogue term alone and together, rotary, in-launch split-K and its two clamps
    (the cases of t320_ref.GEMM_EXACT)"""
    p = R.exact_gemm(spec, device)
    want = R.gemm(p, exact=True)
    assert float(want["pre"].abs().max()) < 60000
    if spec.get("big"):
        assert float((want["out"] != want["pre"]).double().mean()) > 0.5, "the store must round most elements"
    out, what = _run_gemm(device, spy, spec, p)
    _eq(out, want["pre"], bf16, what)


@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.GEGLU_EXACT])
def test_exact_geglu(device, spy, spec):
    """value * gelu(gate) on the gate classes where gelu_erf_f is exact (0, and the integers from 8 up: test_gelu_premise of
    test_gpu_fused320_matrix.py); value and gate rows are drawn differently, so an exchanged group of 16 shows"""
    p = R.exact_gemm(spec, device)
    want = R.gemm(p, exact=True)
    assert float(want["pre"].abs().max()) < 60000 and float((want["out"] != want["pre"]).double().mean()) > 0.1
    out, what = _run_gemm(device, spy, spec, p)
    _eq(out, want["pre"], bf16, what)


@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.CONV_EXACT])
def test_exact_conv(device, spy, spec):
    """stride 1 / 2, pad_after_only, one image and three whose boundaries fall inside a tile, unsplit and two slices; bias + row vector +
    residual"""
    p = R.exact_conv(spec, device)
    want = R.conv(p, exact=True)
    assert float(want["pre"].abs().max()) < 60000
    out, what = _run_conv(device, spy, spec, p)
    _eq(out, want["pre"], bf16, what)


@pytest.mark.parametrize("spec", [pytest.param(s, id=R.case_id(s)) for s in R.UP_EXACT])
def test_exact_conv_up2x_phases(device, spy, spec):
    """the four phase convs on grid.z against F.interpolate + conv2d; integer taps keep the summed phase weights integer"""
    p = R.exact_conv(spec, device)
    want = R.conv(p, exact=True)
    assert float(want["pre"].abs().max()) < 60000
    out, what = _run_conv(device, spy, spec, p)
    _eq(out, want["pre"], bf16, what)


def test_exact_conv_upsample_forms_the_kernel_does_not_take(device, spy):
    """upsample = 1 (the nearest-2x read-through form) goes to another kernel; a phase launch that asks for K slices runs unsplit on this
    one.  Both as the plan says, both exact"""
    spec = dict(R.UP_EXACT[0])
    p = R.exact_conv(spec, device)
    want = R.conv(p, exact=True)
    out, what = _run_conv(device, spy, spec, dict(p, up="read_through", stride=1, pad_after=False), expect="another")
    _eq(out, want["pre"], bf16, what + " upsample = 1")
    spy.tweak = lambda d: setattr(d, "splits", 4)
    out, what = _run_conv(device, spy, spec, p)                          # asserts [0, T320, 22, 1, 0]
    assert spy.descs[-1].splits == 4 and spy.descs[-1].upsample == 2
    _eq(out, want["pre"], bf16, what + " splits = 4")


def _check_colsums(y, stored, B, rows, gemm_rows, form, what):
    from seervideoldm_amd import ops
    cs = y.colsums
    if form == "tiles":
        assert isinstance(cs, ops.ColSums), f"{what}: no per-tile column sums"
        want = R.colsum_tiles(stored, rows, gemm_rows)
        assert float(want.abs().max()) < 2 ** 24
        assert tuple(cs.buf.shape) == tuple(want.shape), (cs.buf.shape, want.shape)
        bad = cs.buf.to(f64) != want
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} partial sums differ, first at [z, partial, n, (sum | sq)] = {bad.nonzero()[0].tolist()}"
    else:
        assert isinstance(cs, ops.ColSumsFx), f"{what}: no accumulated column sums"
        M = gemm_rows.shape[1] if gemm_rows is not None else stored.shape[0]
        want = R.colsum_fx(stored, rows, M // B, cs.reps, gemm_rows)
        assert torch.equal(cs.buf, want), f"{what}: accumulated sums off by up to {(cs.buf - want).abs().max().item() / 2 ** 20}"
        if gemm_rows is None:
            v = stored.reshape(B, -1, stored.shape[1])
            assert torch.equal(cs.totals(), torch.stack([v.sum(1), v.pow(2).sum(1)], -1))


@pytest.mark.parametrize("form", ["tiles", "fx"])
@pytest.mark.parametrize("K,splits", [(320, 1), (768, 1), (768, 2), (768, 3)])
def test_exact_column_sums_gemm(device, spy, form, K, splits):
    """64-row partials unsplit, 16-row partials with K slices; sparse +-1 operands keep |C| <= 256, so the stored value is the fp32 value.
    Partial by partial in the layout [z][partial][N][2], and the accumulated fixed-point form replica by replica"""
    spec = R._c(512, 640, K, sums=True, splits=splits, bias=True, res="lds", seed=90)
    p = R.exact_gemm(spec, device)
    want = R.gemm(p, exact=True)
    assert float(want["pre"].abs().max()) <= 256
    y, what = _run_gemm(device, spy, spec, p, colsum_batch=2 if form == "tiles" else (2, None))
    _eq(y, want["pre"], bf16, what)
    _check_colsums(y, want["out"], 2, 16 if R.planned_slices(K, splits) > 1 else 64, None, form, what)


@pytest.mark.parametrize("form", ["tiles", "fx"])
@pytest.mark.parametrize("kind,splits", [("conv", 1), ("conv", 2), ("up", 1)])
def test_exact_column_sums_conv(device, spy, form, kind, splits):
    """conv: 8 images of 8 x 8, 64 -> 320; up-2x: 4 images of 8 x 8, whose partials cover rows of the SOURCE grid per phase"""
    spec = R._v(8, 8, 8, sums=True, splits=splits, bias=True, seed=91) if kind == "conv" else R._v(4, 8, 8, sums=True, up=True, bias=True, seed=92)
    p = R.exact_conv(spec, device)
    want = R.conv(p, exact=True)
    assert float(want["pre"].abs().max()) <= 256
    y, what = _run_conv(device, spy, spec, p, colsum_batch=2 if form == "tiles" else (2, None))
    _eq(y, want["pre"], bf16, what)
    rows = 16 if (kind == "conv" and splits > 1) else 64
    _check_colsums(y, want["out"], 2, rows, R.phase_rows(4, 8, 8, device) if kind == "up" else None, form, what)


def test_ragged_rows_leave_no_column_sums(device, spy):
    """M = 384: the partial layout would run past the rows -- no column sums, the output exact all the same"""
    spec = R._c(384, 640, 320, sums=True, bias=True, res="lds", seed=93)
    p = R.exact_gemm(spec, device)
    for cb in (2, (2, None)):
        y, what = _run_gemm(device, spy, spec, p, colsum_batch=cb)
        assert y.colsums is None
        _eq(y, R.gemm(p, exact=True)["pre"], bf16, what)


# =========================================================================================== 2. per own row against float64
def _seer_table(rows, rot_dim, dev):
    from seervideoldm_amd import ops
    freqs = (10000.0 ** (-torch.arange(0, rot_dim, 2, dtype=f32) / rot_dim)).to(dev)
    return ops.rotary_table(freqs, rows)


@pytest.mark.parametrize("kind,M,amp", R.ROWS_CASES)
def test_rows(device, spy, kind, M, amp):
    """GEGLU on N(0, 1) gates and rotary from seer_rotary_table's own output (a stored operand): the kernel's worst row, as
    |out - ref|_2 / max(|ref|_2, floor), within 2x the worst row of the float64 result rounded to bf16 once"""
    p = R.random_problem(kind, M, amp, device, make_table=_seer_table)
    ref = R.gemm(p)
    spec = dict(M=M, N=640, K=320, geglu=kind == "geglu", rot=kind == "rotary", seed=int(amp))
    out, what = _run_gemm(device, spy, spec, p)
    floor = R.row_floor(ref["pre"])
    ek, ee = R.row_err(out, ref["pre"], floor), R.row_err(ref["out"], ref["pre"], floor)
    print(f"t320_matrix rows | {kind} M{M} x{amp:g} | plan {spy.plans[-1]} | emulation {ee:.4g} | kernel {ek:.4g} | ratio {ek / ee:.3f}")
    assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    assert ek <= 2 * ee, f"{what}: worst row {ek:.4g} above 2x the emulation's {ee:.4g}"


# =========================================================================================== 3. refusals and fall-backs
def _keeps_nan(buf):
    return bool((buf.view(torch.int16) == 0x7FC0).all()) if buf.dtype == bf16 else bool(buf.isnan().all())


def _silu_problem(dev):
    """accumulators that silu and quick-GELU return unchanged in fp32: 0 (whole rows of zeros), or at least 20 (exp(-x) < 2^-25)"""
    a, w = _ints((256, 256), dev, 1, 0, 3), _ints((320, 256), dev, 2, 0, 3)
    a[::7] = 0.0
    acc = a @ w.t()
    assert bool(((acc == 0) | (acc >= 20)).all()) and bool((acc == 0).any()) and float(acc.max()) < 60000
    return a, w, acc


_FALLBACKS = ["f16", "out_f32", "trans_out", "silu", "quick_gelu", "n_not_320", "geglu_colscale", "rowstat", "ln"]


@pytest.mark.parametrize("what", _FALLBACKS)
def test_tile22_requests_the_kernel_refuses(device, spy, what):
    """a tile = 22 request the kernel is not eligible for plans another kernel and still gives the exact result.  GEGLU with a column
    scale is the one request no kernel carries (gemm.hip, validate): SEER_EINVAL before any launch, the output keeps its bits"""
    from seervideoldm_amd import ops
    from seervideoldm_amd._lib import SeerHipError
    dev = device
    M, N, K = 256, 320, 256
    a64, w64 = _ints((M, K), dev, 1), _ints((N, K), dev, 2)
    bias64 = _ints((N,), dev, 3, -8, 8)
    ref = a64 @ w64.t() + bias64
    dt, kw, n_out, out_dt = bf16, dict(bias=bias64.float()), N, bf16
    if what == "f16":
        dt = out_dt = f16
    elif what == "out_f32":
        out_dt = f32
    elif what in ("silu", "quick_gelu"):
        a64, w64, ref = _silu_problem(dev)
        kw = {what: True}
    elif what == "n_not_320":
        n_out = 328
        w64, bias64 = _ints((n_out, K), dev, 2), _ints((n_out,), dev, 3, -8, 8)
        ref, kw = a64 @ w64.t() + bias64, dict(bias=bias64.float())
    elif what == "geglu_colscale":
        spec = dict(R.GEGLU_EXACT[0], M=M)
        p = R.exact_gemm(spec, dev)
        p["col_scale"] = (0.5, 164)
        ref = R.gemm(p, exact=True)["pre"]
        order = R.interleave_order(320, dev)
        a64, w64, n_out = p["a"], p["w"][order], 320
        kw = dict(bias=p["bias"][order].float().contiguous(), geglu=True, col_scale=(0.5, 164))
    elif what == "ln":
        from tests.fused320_ref import balanced_rows
        # rows of +-1 with mean 0 and variance 1, gamma 1, beta 0, no bias: LN(x) W^T = rstd (x W^T) with rstd = 1 - 5e-6, which the
        # bf16 store returns to the integer x W^T (an exact 0 stays 0: 0 * rstd); a sparse W keeps |x W^T| <= 4
        K = 320
        a64 = balanced_rows(M, dev, 5)
        w64 = R.sparse_pm1((N, K), dev, 6, 4.0 / K)
        ref = a64 @ w64.t()
        assert float(ref.abs().max()) <= 256 and bool((ref == 0).any())
        wp, wsum, bp = ops.fold_layernorm(_store(w64, bf16), torch.ones(K, device=dev), torch.zeros(K, device=dev))
        stats = torch.zeros((M, 2), device=dev, dtype=torch.int64)
        stats[:, 1] = K << 24
        kw = dict(bias=bp, ln=(ops.RowStats(stats), wsum, 1e-5))
    elif what == "rowstat":
        kw["rowstat"] = True
    assert float(ref.abs().max()) < 60000
    a = _gapped(_store(a64, dt))[1]
    w = _store(w64, dt).contiguous()
    if what == "trans_out":
        buf = torch.full((1, N, M), NAN, device=dev, dtype=bf16)
        run = lambda: ops.gemm_batched(_store(a64, bf16)[None].contiguous(), w[None], trans_out=True, bias=bias64.float(), out=buf, tile=T320)[0]
        ref = ref.t().contiguous()
    else:
        buf, view = _nan_out(M, n_out, dev, out_dt)
        run = lambda: ops.gemm(a, w, out=view, tile=T320, **kw)
    seen = []
    spy.tweak = seen.append
    try:
        out = run()
    except SeerHipError as e:
        assert _keeps_nan(buf), f"{what}: the call returned an error and still wrote"
        if what != "geglu_colscale":
            raise
        assert "(-22)" in str(e) and not spy.plans and spy.plan_of(seen[-1]) == [-22, 0, 0, 0, 0]
        print("t320_matrix plan | tile 22 with geglu_colscale | [-22, 0, 0, 0, 0]: refused before any launch, the output keeps its bits")
        return
    assert what != "geglu_colscale", "GEGLU with a column scale is refused for every kernel"
    if out is None:                                                      # ln: the host says this launch cannot fold -- nothing launched
        assert what == "ln" and not spy.plans and _keeps_nan(buf)
        print("t320_matrix plan | tile 22 with ln | the host does not fold: nothing launched")
        return
    _ran_another(spy, f"tile 22 with {what}")
    print(f"t320_matrix plan | tile 22 with {what} | {spy.plans[-1]}")
    _eq(out, ref, dt, f"tile 22 with {what}")
    if what != "trans_out":
        _gaps_hold(buf, M, n_out, what)
    if what == "rowstat":
        assert out.rowstats is not None


@pytest.mark.parametrize("short", ["workspace NULL", "workspace one byte short", "sync NULL", "sync one byte short"])
def test_direct_call_without_room_to_split(device, spy, short):
    """seer_gemm_bf16 with tile = 22, splits = 4 and no room for the slabs or the counters: the plan of THAT descriptor says unsplit on
    this kernel, and the call does that -- exact"""
    from seervideoldm_amd import ops
    spec = R._c(300, 640, 1024, splits=4, bias=True, res="lds", seed=95)
    p = R.exact_gemm(spec, device)
    want = R.gemm(p, exact=True)
    out, what = _run_gemm(device, spy, spec, p)                          # the launch with room: four slices
    _eq(out, want["pre"], bf16, what)
    d = type(spy.descs[-1]).from_buffer_copy(spy.descs[-1])
    need = 2 * 2 * 4 * (8 * 40 * 64 * 16)                                 # tiles x slices x one slab of raw accumulators
    ws = torch.empty((need,), device=device, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    d.sync, d.sync_bytes = ops._sync_buffer(device).data_ptr(), 2 * 2 * 2 * 4
    assert spy.plan_of(d) == [0, K_T320, T320, 4, 0], "the descriptor with exactly enough room splits"
    if short == "workspace NULL":
        d.workspace, d.workspace_bytes = None, 0
    elif short == "workspace one byte short":
        d.workspace_bytes = need - 1
    elif short == "sync NULL":
        d.sync, d.sync_bytes = None, 0
    else:
        d.sync_bytes -= 1
    assert spy.plan_of(d) == [0, K_T320, T320, 1, 0], f"{short}: planned {spy.plan_of(d)}"
    buf, view = _nan_out(300, 640, device)
    d.C, d.ldc = view.data_ptr(), view.stride(0)
    assert spy._real.seer_gemm_bf16(C_.byref(d), torch.cuda.current_stream().cuda_stream) == 0
    _eq(view, want["pre"], bf16, f"direct call, {short}")
    _gaps_hold(buf, 300, 640, short)
    assert _sync_is_zero(device)
