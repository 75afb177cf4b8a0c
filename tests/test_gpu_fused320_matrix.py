"""The two hand-scheduled fused launches of the 320-channel level, seer_rowchain_c320 (csrc/rowchain.hip) and seer_ff_fused_c320
(csrc/ff_fused.hip), and their three pack entry points, tested exactly, per own row and at their edges: part 4 of the series after
test_gpu_f16_matrix.py, test_gpu_train_matrix.py and test_gpu_attn_fwd_matrix.py.  The older tests (test_gpu_rowchain.py,
test_ff_fused_c320* in test_gpu_kernels.py) read one relative L2 number over the whole tensor: the wrong batch element's GroupNorm
statistics in the few dozen rows of a straddling tile, one dropped K step in one wave's 80 columns, value and gate rows exchanged in
one group of 16 all pass there (tests/test_fused320_ref_cpu.py prints what they read on each).

0. The pack entry points bit for bit against a torch gather written from the index sentences of include/seer_hip.h, on random 16-bit
   words, into a guarded arena; seer_rowchain_pack also from a row-strided view (ld = 328).
1. EXACT, zero tolerance.  The fp32 accumulators are exact on small integers, every 16-bit store is one round-to-nearest-even of a
   known number, and at the three inexact spots (rsqrtf of GroupNorm and of LayerNorm, gelu_erf_f) the inputs are chosen so that the
   following 16-bit rounding absorbs the error (tests/fused320_ref.py asserts the preconditions on the float64 reference, case by
   case; a case whose preconditions fail is an error).  Every operand is a row-strided view with a column offset inside a NaN buffer,
   the gaps are checked after the launch, and every launch runs twice and must be bit-identical to itself.
2. PER OWN ROW against the float64 operator on N(0, 1) data at amplitudes 1 and 4, batch element b drawn as N(b, 4^b): the kernel's
   worst row must stay within 2x the worst row of the float64 emulation that rounds to the storage type exactly where the kernels
   round (fused320_ref.py lists the places).  Nothing in the bound comes from the kernel.
3. Every SEER_EINVAL / SEER_ENOSYS branch of the five entry points, one assertion each, decided on the host: the NaN-filled outputs
   keep their bits.

Arguments no other test passes, each in an assertion below: h == NULL with w2f set at M % 96 == 0 (the non-FULL instantiation that
drains where FULL counts), n2 = 2, rot_thirds 1 and 3, scale_thirds 0, 2 and 3, rot_pos_offset != 0, rot_tokens_per_batch that wraps
inside a tile, head dims 64, 80 and 160, groups = 8, gn_fx_reps 3 with uneven replicas, row-strided inp / res / h / out, M < 96, b1 == NULL,
ld > 320 in seer_rowchain_pack, fx_reps that wrap, batch boundaries inside a tile of the column sums.

Measured values, the instantiation each shape reaches, the mutation table and the file's run time: profiles/fused320_matrix.md."""
import ctypes as C_

import pytest
import torch

from tests import fused320_ref as R
from tests.test_gpu_f16_matrix import _eq, _exact_pre, _ints, _store
from tests.test_gpu_train_matrix import _gapped, _gaps_hold

pytestmark = pytest.mark.gpu

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTS = [pytest.param(bf16, id="bf16"), pytest.param(f16, id="f16")]
C, INNER = R.C, R.INNER
EINVAL, ENOSYS = -22, -38
GUARD = 64


def _lib():
    from seervideoldm_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _nan_view(rows, cols, dev, dt):
    return _gapped(torch.full((rows, cols), float("nan"), device=dev, dtype=dt))


def _f32(t):
    return None if t is None else t.to(f32).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


# =========================================================================================== 0. the pack entry points
def _words(shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16).to(dev)


def _arena(n, dev):
    """n 16-bit words of output in front of GUARD sentinel words, all of one allocation"""
    a = torch.full((n + GUARD,), 0x7FC0, device=dev, dtype=torch.int16)
    a[n:] = -7
    return a


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n_mats,ld", [(1, 320), (3, 320), (3, 328)])
def test_rowchain_pack_bit_for_bit(device, dt, n_mats, ld):
    """out[t][s][w][k32][j][lane][e] = W[320 t + 80 w + 16 j + (lane & 15)][64 s + 32 k32 + 8 (lane >> 4) + e], also from a row-strided view"""
    from seervideoldm_amd import ops
    buf = _words((n_mats * C, ld), device, 1)
    w = buf[:, :C]
    row, col = R.rowchain_pack_index(n_mats, device)
    want = w[row, col]
    arena = _arena(n_mats * C * C, device)
    rc = _lib().load().seer_rowchain_pack(w.data_ptr(), ld, n_mats, arena.data_ptr(), _stream())
    assert rc == 0
    assert torch.equal(arena[:n_mats * C * C], want), "seer_rowchain_pack: not the order of include/seer_hip.h"
    assert bool((arena[n_mats * C * C:] == -7).all()), "seer_rowchain_pack wrote behind its output"
    got = ops.rowchain_pack(w.view(dt))
    assert got.is_contiguous() and torch.equal(got.view(torch.int16).reshape(-1), want)


@pytest.mark.parametrize("dt", DTS)
def test_ff_pack_bit_for_bit(device, dt):
    from seervideoldm_amd import ops
    w1, wcat = _words((2 * INNER, C), device, 2), _words((C, C + INNER), device, 3)
    a1, a2 = _arena(w1.numel(), device), _arena(wcat.numel(), device)
    lib = _lib().load()
    assert lib.seer_ff_fused_pack_w1(w1.data_ptr(), a1.data_ptr(), _stream()) == 0
    assert lib.seer_ff_fused_pack_wcat(wcat.data_ptr(), a2.data_ptr(), _stream()) == 0
    r1, c1 = R.ff_pack_w1_index(device)
    r2, c2 = R.ff_pack_wcat_index(device)
    assert torch.equal(a1[:w1.numel()], w1[r1, c1]), "seer_ff_fused_pack_w1: not the order of include/seer_hip.h"
    assert torch.equal(a2[:wcat.numel()], wcat[r2, c2]), "seer_ff_fused_pack_wcat: not the order of include/seer_hip.h"
    assert bool((a1[w1.numel():] == -7).all()) and bool((a2[wcat.numel():] == -7).all()), "a pack kernel wrote behind its output"
    g1, g2 = ops.ff_fused_pack(w1.view(dt), wcat.view(dt))
    assert torch.equal(g1.view(torch.int16).reshape(-1), w1[r1, c1]) and torch.equal(g2.view(torch.int16).reshape(-1), wcat[r2, c2])


# =========================================================================================== launchers
class _Rc:
    """one seer_rowchain_c320 launch from a float64 problem of fused320_ref: every 16-bit operand a _gapped NaN view (row stride
    cols + 16, column offset 8), desc filled field by field.  .run() launches and returns (h, out) views; .check_gaps()"""

    def __init__(self, dev, dt, p, *, h_out=True, alias=False):
        from seervideoldm_amd import ops
        L = _lib()
        self.p, self.dt, self.dev = p, dt, dev
        M = self.M = p["inp"].shape[0]
        d = self.d = L.RowChainDesc()
        self.inp_buf, inp = _gapped(_store(p["inp"], dt))
        d.inp, d.ld_in, d.M, d.dtype = inp.data_ptr(), inp.stride(0), M, L.SEER_DT_F16 if dt == f16 else L.SEER_DT_BF16
        self.w1f = ops.rowchain_pack(_store(p["w1"], dt))
        d.w1f = self.w1f.data_ptr()
        if p.get("b1") is not None:
            self.b1 = _f32(p["b1"])
            d.b1 = self.b1.data_ptr()
        self.h_buf = self.h = self.res0 = None
        if p.get("res") is not None:
            self.res0 = _store(p["res"], dt)
            self.res_buf, self.res = _gapped(self.res0)
            d.res, d.ldr = self.res.data_ptr(), self.res.stride(0)
        if alias:
            assert h_out and self.res0 is not None
            self.h_buf, self.h = self.res_buf, self.res
        elif h_out:
            self.h_buf, self.h = _nan_view(M, C, dev, dt)
        if self.h is not None:
            d.h, d.ldh = self.h.data_ptr(), self.h.stride(0)
        gn = p.get("gn")
        if gn is not None:
            if gn["form"] == "stats":
                self.stats = _f32(gn["stats"])
                assert torch.equal(self.stats.to(f64), gn["stats"])
                d.gn_stats = self.stats.data_ptr()
            else:
                self.fx = gn["fx"].contiguous()
                d.gn_fx, d.gn_fx_reps = self.fx.data_ptr(), self.fx.shape[0]
            self.gg, self.gb = _f32(gn["gamma"]), _f32(gn["beta"])
            d.gn_count, d.gn_eps, d.gn_gamma, d.gn_beta = gn["count"], gn["eps"], self.gg.data_ptr(), self.gb.data_ptr()
            d.rows_per_batch, d.groups = gn["rows_pb"], gn["groups"]
        if p.get("ln") is not None:
            self.lg, self.lb = _f32(p["ln"][0]), _f32(p["ln"][1])
            d.ln_gamma, d.ln_beta, d.ln_eps = self.lg.data_ptr(), self.lb.data_ptr(), p["ln"][2]
        self.out_buf = self.out = None
        if p.get("w2") is not None:
            n2 = self.n2 = p["w2"].shape[0] // C
            self.w2f = ops.rowchain_pack(_store(p["w2"], dt))
            self.out_buf, self.out = _nan_view(M, n2 * C, dev, dt)
            d.w2f, d.n2, d.out, d.ldo = self.w2f.data_ptr(), n2, self.out.data_ptr(), self.out.stride(0)
            d.col_scale, d.scale_thirds = p.get("col_scale", 1.0), p.get("scale_thirds", 0)
            rot = p.get("rot")
            if rot is not None:
                self.table = rot["table"].to(f32).contiguous()
                assert self.table.shape[0] >= rot["tokens"] + rot["off"] and self.table.shape[1] * 2 == rot["rot_dim"]
                d.rot_table, d.rot_tokens_per_batch, d.rot_pos_offset = self.table.data_ptr(), rot["tokens"], rot["off"]
                d.rot_head_dim, d.rot_dim, d.rot_thirds = rot["head_dim"], rot["rot_dim"], rot["thirds"]

    def launch(self):
        return _lib().load().seer_rowchain_c320(C_.byref(self.d), _stream())

    def run(self):
        if self.res0 is not None:
            self.res.copy_(self.res0)                # (in place: the first run wrote h over it)
        rc = self.launch()
        assert rc == 0, f"seer_rowchain_c320 returned {rc}"
        return self.h, self.out

    def check_gaps(self, what):
        if self.h_buf is not None:
            _gaps_hold(self.h_buf, self.M, C, f"{what}: h")
        if self.out_buf is not None:
            _gaps_hold(self.out_buf, self.M, self.n2 * C, f"{what}: out")
        if self.res0 is not None and self.h is not self.res:
            assert torch.equal(_bits(self.res), _bits(self.res0)), f"{what}: res was written"


class _Ff:
    """one seer_ff_fused_c320 launch from a float64 problem: h, x, y, a as _gapped views; y may alias x"""

    def __init__(self, dev, dt, p, *, alias=False, fx=None, tiles=False):
        from seervideoldm_amd import ops
        self.p, self.dt = p, dt
        M = self.M = p["h"].shape[0]
        order = R.geglu_interleave_order(dev)
        self.w1f, self.wcf = ops.ff_fused_pack(_store(p["w1"], dt)[order].contiguous(), _store(p["wcat"], dt))
        self.b1 = _f32(p["b1"][order])
        self.gamma, self.beta, self.bcat = _f32(p["gamma"]), _f32(p["beta"]), _f32(p["bcat"])
        self.h_buf, self.h = _gapped(_store(p["h"], dt))
        self.x0 = _store(p["x"], dt)
        self.x_buf, self.x = _gapped(self.x0)
        if alias:
            self.y_buf, self.y = self.x_buf, self.x
        else:
            self.y_buf, self.y = _nan_view(M, C, dev, dt)
        self.a = self.wof = self.bo = None
        if p.get("pre") is not None:
            a, wo, bo = p["pre"]
            self.a_buf, self.a = _gapped(_store(a, dt))
            self.wof, self.bo = ops.rowchain_pack(_store(wo, dt)), _f32(bo)
        self.fx = self.tiles = None
        self.fx_rows = self.reps = 0
        if fx is not None:
            self.fx_rows, self.reps = fx
            self.fx = torch.zeros((self.reps, M // self.fx_rows, 2, C), device=dev, dtype=torch.int64)
        if tiles:
            self.tiles = torch.full((M // 96, C, 2), float("nan"), device=dev, dtype=f32)
        self.dtc = _lib().SEER_DT_F16 if dt == f16 else _lib().SEER_DT_BF16

    def launch(self, **over):
        k = dict(a=_ptr(self.a), lda=self.a.stride(0) if self.a is not None else 0, wof=_ptr(self.wof), bo=_ptr(self.bo), h=_ptr(self.h),
                 ldh=self.h.stride(0), x=_ptr(self.x), ldx=self.x.stride(0), y=_ptr(self.y), ldy=self.y.stride(0), M=self.M,
                 gamma=_ptr(self.gamma), beta=_ptr(self.beta), eps=self.p["eps"], w1f=_ptr(self.w1f), b1=_ptr(self.b1), wcf=_ptr(self.wcf),
                 bcat=_ptr(self.bcat), fx=_ptr(self.fx), fx_rows=self.fx_rows, reps=self.reps, tiles=_ptr(self.tiles), dtype=self.dtc)
        k.update(over)
        return _lib().load().seer_ff_fused_c320(k["a"], k["lda"], k["wof"], k["bo"], k["h"], k["ldh"], k["x"], k["ldx"], k["y"], k["ldy"], k["M"],
                                                k["gamma"], k["beta"], k["eps"], k["w1f"], k["b1"], k["wcf"], k["bcat"], k["fx"], k["fx_rows"],
                                                k["reps"], k["tiles"], k["dtype"], _stream())

    def run(self):
        self.x.copy_(self.x0)
        if self.fx is not None:
            self.fx.zero_()
        rc = self.launch()
        assert rc == 0, f"seer_ff_fused_c320 returned {rc}"
        return self.y

    def check_gaps(self, what):
        _gaps_hold(self.y_buf, self.M, C, f"{what}: y")
        if self.y is not self.x:
            assert torch.equal(_bits(self.x), _bits(self.x0)), f"{what}: x was written"
        assert torch.equal(_bits(self.h), _bits(_store(self.p["h"], self.dt))), f"{what}: h was written"


# =========================================================================================== 1. exact, zero tolerance
def test_gelu_premise(device):
    """the premise of the exact GEGLU construction, independent of ff_fused: the GEGLU epilogue's gelu_erf_f is exactly 0 at 0 and
    exactly x at the integers 8..64 (relu(x) - a 2^(..) with a clamped at 5.657 is x - 4.4e-8, which rounds to x in fp32 from 8 up)"""
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import interleave_geglu
    K = 64
    gate = torch.tensor([0.0] + [float(v) for v in range(8, 65)], device=device)
    a = torch.zeros((gate.numel(), K), device=device)
    a[:, 0], a[:, 1] = 1.0, gate
    w = torch.zeros((64, K), device=device)
    w[:32, 0], w[32:, 1] = 1.0, 1.0
    wi, bi = interleave_geglu(w.to(bf16), torch.zeros(64, device=device))
    out = ops.gemm(a.to(bf16), wi, bias=bi, geglu=True, out_f32=True)
    assert torch.equal(out, gate[:, None].expand(-1, 32).contiguous()), "gelu_erf_f is not the identity at 0 and at the integers from 8 up"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("spec", [pytest.param(s, id=R.rowchain_id(s)) for s in R.ROWCHAIN_EXACT])
def test_exact_rowchain(device, dt, spec):
    p = R.exact_rowchain(spec, dt, device)
    want = R.rowchain(p, dt, exact=True)                                   # asserts every precondition; never skipped
    share = R.rounded_share(want["out_pre"] if want["out"] is not None else want["h_pre"], dt)      # the FINAL store of the case
    assert share > 0.1, f"the final store of this case rounds {share:.3f} of its elements: too few to pin the rounding"
    what = R.rowchain_id(spec)
    rc = _Rc(device, dt, p, h_out=spec["h_out"], alias=spec["res"] == "alias")
    h, out = rc.run()
    if spec["h_out"]:
        _eq(h, want["h"], dt, f"{what}: h")
    if want["out"] is not None:
        _eq(out, want["out"], dt, f"{what}: out")
    rc.check_gaps(what)
    first = [None if t is None else t.clone() for t in (h, out)]
    h2, out2 = rc.run()
    for a, b in zip(first, (h2, out2)):
        assert a is None or torch.equal(_bits(a), _bits(b)), f"{what}: two launches differ"


def test_exact_rowchain_permutation_is_sharp(device):
    """the signed-permutation W1 as a fragment-order probe on its own: h[:, n] = s_n inp[:, perm(n)], inp distinct per column"""
    dt = bf16
    w1, perm, s = R.signed_permutation(device, 5)
    inp = (torch.arange(C, device=device, dtype=f64) % 251 - 125)[None, :] + _ints((97, 1), device, 6, 0, 2)
    _exact_pre(1, 127, 1)
    p = dict(inp=inp.contiguous(), w1=w1)
    rc = _Rc(device, dt, p)
    h, _ = rc.run()
    _eq(h, p["inp"][:, perm] * s, dt, "h through a signed permutation")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,pre,alias,colsum", R.FF_EXACT, ids=lambda v: str(v).replace(" ", ""))
def test_exact_ff_fused(device, dt, M, pre, alias, colsum):
    small = colsum is not None                                              # |y| <= 256 and integers: the column sums are exact
    p = R.exact_ff(dict(M=M, pre=pre, small=small), dt, device)
    info = {}
    want = R.ff(p, dt, exact=True, info=info)
    if small:
        assert float(want.abs().max()) <= 256 and bool((want == want.round()).all())
    else:
        share = R.rounded_share(info["y_pre"], dt)
        assert share > 0.3, f"the store of y rounds {share:.3f} of its elements"
    what = f"ff_fused M{M} pre{int(pre)} alias{int(alias)} {colsum}"
    ff = _Ff(device, dt, p, alias=alias, fx=colsum[1:] if isinstance(colsum, tuple) else None, tiles=colsum == "tiles")
    y = ff.run()
    _eq(y, want, dt, f"{what}: y")
    ff.check_gaps(what)
    if isinstance(colsum, tuple):
        want_fx = R.colsums_fx(want, colsum[1], colsum[2])
        assert torch.equal(ff.fx.sum(0), want_fx.sum(0)), f"{what}: colsum_fx totals are not the integer column sums of the stored y times 2^20"
        assert torch.equal(ff.fx, want_fx), f"{what}: a replica of colsum_fx holds another tile's sums"
    if colsum == "tiles":
        assert torch.equal(ff.tiles.to(f64), R.colsum_tiles(want)), f"{what}: colsum_tiles"
    first = (y.clone(), None if ff.fx is None else ff.fx.clone())
    y2 = ff.run()
    assert torch.equal(_bits(first[0]), _bits(y2)) and (ff.fx is None or torch.equal(first[1], ff.fx)), f"{what}: two launches differ"


# =========================================================================================== 2. per own row, derived allowance
def _seer_table(rows, rot_dim, dev):
    from seervideoldm_amd import ops
    freqs = (10000.0 ** (-torch.arange(0, rot_dim, 2, dtype=f32) / rot_dim)).to(dev)
    return ops.rotary_table(freqs, rows)


def _judge(tag, got, ref, emu):
    floor = R.row_floor(ref)
    ek, ee = R.row_err(got, ref, floor), R.row_err(emu, ref, floor)
    print(f"fused320_matrix rows | {tag} | emulation {ee:.4g} | kernel {ek:.4g} | ratio {ek / ee if ee > 0 else float('inf'):.3f}")
    assert bool(torch.isfinite(got.float()).all()), f"{tag}: non-finite output"
    assert ek <= 2 * ee, f"{tag}: worst row {ek:.4g} above 2x the emulation's {ee:.4g}"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("amp", [1.0, 4.0])
@pytest.mark.parametrize("gn,M,res,off", R.ROWCHAIN_ROWS, ids=lambda v: str(v).replace(" ", ""))
def test_rows_rowchain(device, dt, amp, gn, M, res, off):
    p = R.rows_rowchain_problem(dt, device, gn, M, res, off, amp, make_table=_seer_table)
    ref, emu = R.rowchain(p), R.rowchain(p, dt)
    rc = _Rc(device, dt, p, alias=res)
    h, out = rc.run()
    tag = f"rowchain {'f16' if dt == f16 else 'bf16'} {gn[0] if gn else 'plain'} M{M} off{off} x{amp:g}"
    _judge(tag + " h", h, ref["h"], emu["h"])
    _judge(tag + " out", out, ref["out"], emu["out"])
    rc.check_gaps(tag)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,rows_pb,amp", R.FX_STATS_CASES)
def test_rows_gn_fx_against_gn_stats(device, dt, B, rows_pb, amp):
    """the chain from the producer's accumulated fixed-point sums against the chain from (sum, sum of squares) per group, per row.  Both
    see the same x; they differ by the fp32 arithmetic of the statistics (stats form: mean and E[x^2] - mean^2 in fp32; fx form: one
    conversion per group in double), a relative 1e-7 in scale and shift that moves an output only where it flips a 16-bit rounding of
    GN(x) -- and that flip then moves its whole row of h, which flips further roundings.  The allowance is 2x
    fused320_ref.fx_stats_yardstick: the same difference between EMULATIONS that carry the fp32 statistics arithmetic, with the flip
    events sampled by moving the fp32 mean and variance by +-1 ulp, worst row over the cases of the storage type.  Nothing in it comes
    from a kernel"""
    ps, pf = R.fx_stats_problems(dt, device, B, rows_pb, amp, make_table=_seer_table)
    yard = R.fx_stats_yardstick(dt, device, make_table=_seer_table)
    ref = R.rowchain(ps)
    hs, os_ = [t.clone() for t in _Rc(device, dt, ps).run()]
    hf, of = _Rc(device, dt, pf).run()
    for name, a, b in (("h", hf, hs), ("out", of, os_)):
        dk = R.row_diff(a, b, ref[name])
        print(f"fused320_matrix fx-vs-stats | {'f16' if dt == f16 else 'bf16'} {B}x{rows_pb} x{amp:g} {name} | emulations' yardstick {yard[name]:.4g} | kernels {dk:.4g}")
        assert dk <= 2 * yard[name], f"{name}: the two forms differ by {dk:.4g} in their worst row, the emulations' yardstick is {yard[name]:.4g}"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("amp", [1.0, 4.0])
@pytest.mark.parametrize("M,pre", R.FF_ROWS)
def test_rows_ff_fused(device, dt, amp, M, pre):
    p = R.random_ff(dt, device, M=M, pre=pre, amp=amp, B=3 if M == 336 else 1, seed=int(amp) * 100 + M)
    ref, emu = R.ff(p), R.ff(p, dt)
    ff = _Ff(device, dt, p)
    y = ff.run()
    tag = f"ff_fused {'f16' if dt == f16 else 'bf16'} M{M} pre{int(pre)} x{amp:g}"
    _judge(tag, y, ref, emu)
    ff.check_gaps(tag)


# =========================================================================================== 3. refusals
def _refusal_chain(dev, dt=bf16):
    p = R.random_rowchain(dt, dev, M=192, gn=("stats", 2, 96, 32, 1), res=True, n2=3,
                          rot=dict(table=_seer_table(96, 32, dev), tokens=96, off=0, head_dim=40, rot_dim=32, thirds=2))
    return _Rc(dev, dt, p)


_RC_REFUSALS = [  # (name, {field: value or callable(desc)}, code)
    ("ld_in not a multiple of 8", dict(ld_in=332), EINVAL), ("ld_in below 320", dict(ld_in=312), EINVAL),
    ("ldh not a multiple of 8", dict(ldh=332), EINVAL), ("ldh below 320", dict(ldh=312), EINVAL),
    ("ldr not a multiple of 8", dict(ldr=332), EINVAL), ("ldr below 320", dict(ldr=312), EINVAL),
    ("ldo not a multiple of 8", dict(ldo=980), EINVAL), ("ldo below n2 * 320", dict(ldo=952), EINVAL),
    ("inp 8 bytes off", dict(inp=lambda d: d.inp + 8), EINVAL), ("w1f 8 bytes off", dict(w1f=lambda d: d.w1f + 8), EINVAL),
    ("h 8 bytes off", dict(h=lambda d: d.h + 8), EINVAL), ("res 8 bytes off", dict(res=lambda d: d.res + 8), EINVAL),
    ("w2f 8 bytes off", dict(w2f=lambda d: d.w2f + 8), EINVAL), ("out 8 bytes off", dict(out=lambda d: d.out + 8), EINVAL),
    ("n2 = 0", dict(n2=0), EINVAL), ("n2 = 4", dict(n2=4, ldo=1296), EINVAL), ("out NULL", dict(out=None), EINVAL),
    ("scale_thirds > n2", dict(scale_thirds=4), EINVAL), ("scale_thirds < 0", dict(scale_thirds=-1), EINVAL),
    ("rot_thirds > n2", dict(rot_thirds=4), EINVAL), ("rot_thirds above a smaller n2", dict(n2=1, rot_thirds=2), EINVAL),
    ("ln gamma only", dict(ln_beta=None), EINVAL), ("ln beta only", dict(ln_gamma=None), EINVAL),
    ("both statistics forms", dict(gn_fx=lambda d: d.gn_stats, gn_fx_reps=1), EINVAL),
    ("gn_fx_reps = 0", dict(gn_fx=lambda d: d.gn_stats, gn_stats=None, gn_fx_reps=0), EINVAL),
    ("gn gamma NULL", dict(gn_gamma=None), EINVAL), ("gn beta NULL", dict(gn_beta=None), EINVAL), ("gn_count 0", dict(gn_count=0.0), EINVAL),
    ("groups does not divide 320", dict(groups=7), EINVAL), ("groups 0", dict(groups=0), EINVAL),
    ("M % rows_per_batch", dict(rows_per_batch=100), EINVAL), ("rows_per_batch 0", dict(rows_per_batch=0), EINVAL),
    ("rows_per_batch 95", dict(rows_per_batch=95, M=190), ENOSYS),
    ("rot_dim > rot_head_dim", dict(rot_dim=48), EINVAL), ("rot_dim not a multiple of 4", dict(rot_dim=30), EINVAL),
    ("320 % rot_head_dim", dict(rot_head_dim=48), EINVAL), ("rot_head_dim not a multiple of 4", dict(rot_head_dim=10, rot_dim=8), EINVAL),
    ("rot_table NULL", dict(rot_table=None), EINVAL), ("rot_tokens_per_batch 0", dict(rot_tokens_per_batch=0), EINVAL),
    ("bad dtype", dict(dtype=7), EINVAL), ("bad dtype wins over ENOSYS", dict(dtype=7, rows_per_batch=95, M=190), EINVAL),
    ("neither h nor w2f", dict(h=None, w2f=None), EINVAL), ("M = 0", dict(M=0), EINVAL), ("inp NULL", dict(inp=None), EINVAL),
    ("w1f NULL", dict(w1f=None), EINVAL),
]


def test_rowchain_refusals(device):
    """every SEER_EINVAL / SEER_ENOSYS branch of seer_rowchain_c320, on valid device pointers: decided on the host, nothing launched"""
    L = _lib()
    rc = _refusal_chain(device)
    fields = [f[0] for f in L.RowChainDesc._fields_]
    saved = {f: getattr(rc.d, f) for f in fields}
    for name, change, code in _RC_REFUSALS:
        for f, v in saved.items():
            setattr(rc.d, f, v)
        for f, v in change.items():
            setattr(rc.d, f, v(rc.d) if callable(v) else v)
        assert rc.launch() == code, f"{name}: expected {code}"
    torch.cuda.synchronize()
    assert bool(rc.h.isnan().all()) and bool(rc.out.isnan().all()), "a refused launch wrote"
    rc.check_gaps("refusals")
    for f, v in saved.items():
        setattr(rc.d, f, v)
    assert rc.launch() == 0 and bool(torch.isfinite(rc.out.float()).all()), "the unchanged descriptor must launch"


def test_pack_refusals(device):
    lib = _lib().load()
    w = _words((C, 328), device, 1)
    arena = _arena(C * C + 8, device)
    before = arena.clone()
    W, O, s = w.data_ptr(), arena.data_ptr(), _stream()
    for name, args in [("ld below 320", (W, 312, 1, O)), ("ld not a multiple of 8", (W, 324, 1, O)), ("n_mats 0", (W, 328, 0, O)),
                       ("W 8 bytes off", (W + 8, 328, 1, O)), ("out 8 bytes off", (W, 328, 1, O + 8)), ("W NULL", (None, 328, 1, O)),
                       ("out NULL", (W, 328, 1, None))]:
        assert lib.seer_rowchain_pack(*args, s) == EINVAL, name
    for fn in (lib.seer_ff_fused_pack_w1, lib.seer_ff_fused_pack_wcat):
        for name, args in [("in 8 bytes off", (W + 8, O)), ("out 8 bytes off", (W, O + 8)), ("in NULL", (None, O)), ("out NULL", (W, None))]:
            assert fn(*args, s) == EINVAL, name
    torch.cuda.synchronize()
    assert torch.equal(arena, before), "a refused pack wrote"


def test_ff_fused_refusals(device):
    dt = bf16
    p = R.random_ff(dt, device, M=192, pre=True)
    ff = _Ff(device, dt, p, fx=(96, 2), tiles=True)
    p97 = R.random_ff(dt, device, M=97)
    ff97 = _Ff(device, dt, p97, tiles=False)
    tiles97 = torch.full((2, C, 2), float("nan"), device=device)
    cases = [
        ("lda not a multiple of 8", dict(lda=332)), ("lda below 320", dict(lda=312)), ("a without wof", dict(wof=None)), ("a without bo", dict(bo=None)),
        ("a 8 bytes off", dict(a=ff.a.data_ptr() + 8)), ("wof 8 bytes off", dict(wof=ff.wof.data_ptr() + 8)), ("bo 8 bytes off", dict(bo=ff.bo.data_ptr() + 8)),
        ("ldh not a multiple of 8", dict(ldh=332)), ("ldh below 320", dict(ldh=312)), ("ldx not a multiple of 8", dict(ldx=332)),
        ("ldx below 320", dict(ldx=312)), ("ldy not a multiple of 8", dict(ldy=332)), ("ldy below 320", dict(ldy=312)),
        ("h 8 bytes off", dict(h=ff.h.data_ptr() + 8)), ("x 8 bytes off", dict(x=ff.x.data_ptr() + 8)), ("y 8 bytes off", dict(y=ff.y.data_ptr() + 8)),
        ("w1f 8 bytes off", dict(w1f=ff.w1f.data_ptr() + 8)), ("wcf 8 bytes off", dict(wcf=ff.wcf.data_ptr() + 8)),
        ("b1 8 bytes off", dict(b1=ff.b1.data_ptr() + 8)), ("bcat 8 bytes off", dict(bcat=ff.bcat.data_ptr() + 8)),
        ("gamma 8 bytes off", dict(gamma=ff.gamma.data_ptr() + 8)), ("beta 8 bytes off", dict(beta=ff.beta.data_ptr() + 8)),
        ("h NULL", dict(h=None)), ("x NULL", dict(x=None)), ("y NULL", dict(y=None)), ("gamma NULL", dict(gamma=None)), ("beta NULL", dict(beta=None)),
        ("w1f NULL", dict(w1f=None)), ("b1 NULL", dict(b1=None)), ("wcf NULL", dict(wcf=None)), ("bcat NULL", dict(bcat=None)),
        ("M = 0", dict(M=0)), ("fx_rows 80", dict(fx_rows=80)), ("fx_rows 100", dict(fx_rows=100)), ("M % fx_rows", dict(fx_rows=112)),
        ("fx_reps 0", dict(reps=0)), ("bad dtype", dict(dtype=7)),
    ]
    for name, over in cases:
        assert ff.launch(**over) == EINVAL, name
    assert ff97.launch(tiles=tiles97.data_ptr()) == EINVAL, "colsum_tiles with M = 97"
    torch.cuda.synchronize()
    assert bool(ff.y.isnan().all()) and bool(ff97.y.isnan().all()) and bool(ff.tiles.isnan().all()) and bool(tiles97.isnan().all())
    assert not bool(ff.fx.any()), "a refused launch added to colsum_fx"
    ff.check_gaps("refusals")
    assert ff.launch() == 0 and bool(torch.isfinite(ff.y.float()).all()), "the unchanged arguments must launch"
