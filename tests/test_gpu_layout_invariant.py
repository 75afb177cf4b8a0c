"""Layout-invariant mode on a real MI355X: with SeerUNet(layout_invariant=True) the result for one batch element is the same BITS
whatever else is in the batch, however CFG is laid out (one batch, two calls, a half per rank) and however the frames are sharded;
with the switch off nothing changes.  Every comparison is torch.equal.

Kernel level: rows 0 .. M-1 of a launch with the SEER_TILE_AUTO_INVARIANT request equal rows 0 .. M-1 of a launch over 2 M and 3 M
rows (the extra rows hold other data), NaN sentinels behind the last output row stay NaN.  Model level: m(x[0:2]) against
cat(m(x[0:1]), m(x[1:2])), after asserting through seer_gemm_plan that the DEFAULT request plans the two layouts differently.
Sampler: the strict twin of tests/test_gpu_unet.py::test_unbatched_cfg_branch.  Processes: two ranks on one GPU over gloo."""
import ctypes as C
import math
import os
import sys
import time
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as Fn

from seervideoldm_amd import DDIMSampler, SeerUNet, _lib, ops, synth
from seervideoldm_amd.plms import PLMSSampler
from seervideoldm_amd.weights import geglu_row_order
from tests.test_dist_gpu import _backend, _free_port, _host_staged_gathers

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
INV = _lib.SEER_TILE_AUTO_INVARIANT
bf16, f16, f64 = torch.bfloat16, torch.float16, torch.float64
CFG_MINI = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)
CFG_WIDE = dict(block_out_channels=(320, 640, 1280, 1280), layers_per_block=1, cross_attention_dim=768, attention_head_dim=8)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- 1. kernel level ---------------------------------------------------------------------------------------------------------
def _out(rows, cols, dtype, device):
    """an output buffer with 8 NaN rows behind it"""
    full = torch.full((rows + 8, cols), float("nan"), device=device, dtype=dtype)
    return full, full[:rows]


def _eps(dt):
    """one rounding to the storage type, as the matrix tests bound it (tests/test_gpu_f16_matrix.py::_bound: 2^-11 for the 11
    significand bits of IEEE half; bf16 has 8)"""
    return 2.0 ** -11 if dt == f16 else 2.0 ** -8


def _within(got, ref, tol, what):
    err = (got.to(f64) - ref).abs()
    bad = err > tol
    print(f"[layout] {what}: worst err / bound {(err / tol).max().item():.3g}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} outside the bound, worst ratio {(err / tol).max().item():.3g}"


def _acc_bound(ref, absacc, K, dt):
    """tests/test_gpu_f16_matrix.py::_bound with the storage type's rounding: one rounding of the output, worst-case fp32
    accumulation of K products and the epilogue terms, subnormals"""
    return _eps(dt) * ref.abs() + (K + 4) * 2.0 ** -23 * absacc + 2.0 ** -25


def _sums_hold(got_i64, x, dim, scale_bits, dt, what):
    """integer (sum, sum of squares) statistics at scale 2^scale_bits against float64 sums of the STORED output x.  Bound: the
    statistic may be taken from the fp32 value before the store rounds it (eps |x| per element, 2 eps x^2 (1 + eps) per square),
    each addend is quantised to the scale once and squared in fp32 once."""
    x = x.to(f64)
    e, q = _eps(dt), x.shape[dim] * 2.0 ** -(scale_bits - 1)
    got = got_i64.to(f64) / float(1 << scale_bits)
    _within(got[0], x.sum(dim), e * x.abs().sum(dim) + q, what + " sums")
    _within(got[1], (x * x).sum(dim), (2 * e * (1 + e) + 2.0 ** -23) * (x * x).sum(dim) + q, what + " sums of squares")


def _rows_of_m_equal(run, M, what, check=None):
    """run(reps) -> (out over reps * M rows, sentinel rows, extras); rows 0 .. M-1 and the per-element extras of element 0 agree
    for every reps, and check(out rows, extras) holds them against a reference outside the mode"""
    base = None
    for reps in (1, 2, 3):
        out, guard, extra = run(reps)
        torch.cuda.synchronize()
        assert torch.isnan(guard).all(), f"{what}: wrote behind row {reps * M}"
        got = (out[:M].clone(), *[e.clone() for e in extra])
        assert torch.isfinite(got[0].float()).all(), what
        if base is None:
            base = got
            if check is not None:
                check(got[0], got[1:])
        else:
            for i, (a, b) in enumerate(zip(base, got)):
                assert torch.equal(a, b), f"{what}: rows 0..{M - 1} of a launch over {reps * M} rows differ from the launch over {M} rows " \
                                          f"(tensor {i}: {(a.float() - b.float()).abs().max().item():.3g})"


def _plain_case(device, dt, M, N, K, *, bias=True, residual=False, geglu=False, ln=False, a2=0, rotcs=False, rowstat=False, fx=False):
    a = _randn((3 * M, K - a2), 1).to(device, dt)
    a2t = _randn((3 * M, a2), 2).to(device, dt) if a2 else None
    w = _randn((N, K), 3, K ** -0.5).to(device, dt)
    n_out = N // 2 if geglu else N
    b = _randn((N,), 4).to(device) if bias else None
    res = _randn((3 * M, n_out), 5).to(device, dt) if residual else None
    kw = {}
    if rotcs:           # the temporal q|k|v projection: rotary on the q and k thirds, the softmax scale on q
        hd, tpb = N // 24, 256
        table = ops.rotary_table(torch.linspace(0.1, 1.0, 16, device=device), tpb)
        kw = dict(rotary=(table, tpb, 0, hd, 32, 2 * N // 3), col_scale=(0.3, N // 3))
    stats = wsum = None
    if ln:              # folded LayerNorm: the row statistics of a, as its producer would have left them
        af = a.double()
        stats = torch.stack([af.sum(1), (af * af).sum(1)], dim=1).mul(float(1 << 24)).round().to(torch.int64).contiguous()
        wsum = w.float().sum(1).contiguous()

    def run(reps):
        rows = reps * M
        full, out = _out(rows, n_out, dt, device)
        k = dict(kw)
        if ln:
            k["ln"] = (ops.RowStats(stats[:rows]), wsum, 1e-5)
        if fx:
            k["colsum_batch"] = (reps, ops.FxArena(device, 8 * reps * N * 2 + 16))
        y = ops.gemm(a[:rows], w, bias=b, residual=None if res is None else res[:rows], a2=None if a2t is None else a2t[:rows],
                     geglu=geglu, out=out, tile=INV, rowstat=rowstat, **k)
        assert y is not None, "the invariant plan folds the LayerNorm at every M"
        extra = []
        if rowstat:
            assert y.rowstats is not None
            extra.append(y.rowstats.buf[:M])
        if fx:
            assert isinstance(y.colsums, ops.ColSumsFx), "no accumulated column sums from this launch"
            extra.append(y.colsums.buf.sum(dim=0)[0])          # element 0: integers, equal per batch element
        return out, full[rows:], extra

    def check(out, extra):
        """float64 on the stored operands of rows 0 .. M-1"""
        what = f"gemm {M}x{N}x{K} {dt}"
        A = a[:M].to(f64) if a2t is None else torch.cat([a[:M], a2t[:M]], 1).to(f64)
        W = w.to(f64)
        tol_ln = None
        if ln:      # LN(a) W^T = rstd (a W^T - mean wsum): the fold of ops.fold_layernorm with gamma = 1, beta = 0
            A = Fn.layer_norm(A, (K,), eps=1e-5)
            tol_ln = 6e-3 if dt == f16 else 2e-2        # tests/test_gpu_f16_matrix.py::test_statistics_paths_over_magnitudes
        if geglu:   # the launch reads GEGLU.proj's rows in weights.geglu_row_order: undo it
            order = geglu_row_order(N // 2, device)
            Wo = torch.empty_like(W)
            Wo[order] = W
            bo = torch.zeros(N, device=device, dtype=f64)
            if b is not None:
                bo[order] = b.to(f64)
            W, bias64 = Wo, bo
        else:
            bias64 = b.to(f64) if b is not None else torch.zeros(N, device=device, dtype=f64)
        acc, ab = A @ W.t() + bias64, A.abs() @ W.abs().t() + bias64.abs()
        dacc = (K + 4) * 2.0 ** -23 * ab if tol_ln is None else tol_ln * (1 + acc.abs())
        if rotcs:   # tests/test_gpu_f16_matrix.py::test_f16_rotary_epilogue_and_col_scale: two accumulators meet in a rotated column
            Cq, Hh, rd = N // 3, 8, 32
            table, tpb = kw["rotary"][0], kw["rotary"][1]
            pos = torch.arange(M, device=device) % tpb
            c, s_ = table[pos, :, 0].to(f64)[:, None], table[pos, :, 1].to(f64)[:, None]
            t, tb = acc[:, :2 * Cq].reshape(M, 2 * Hh, hd).clone(), dacc[:, :2 * Cq].reshape(M, 2 * Hh, hd).clone()
            x0, x1, b0, b1 = t[..., 0:rd:2].clone(), t[..., 1:rd:2].clone(), tb[..., 0:rd:2].clone(), tb[..., 1:rd:2].clone()
            t[..., 0:rd:2], t[..., 1:rd:2] = x0 * c - x1 * s_, x1 * c + x0 * s_
            tb[..., 0:rd:2], tb[..., 1:rd:2] = b0 * c.abs() + b1 * s_.abs(), b1 * c.abs() + b0 * s_.abs()
            scv = torch.ones(N, device=device, dtype=f64)
            scv[:Cq] = float(torch.tensor(0.3, dtype=torch.float32))
            acc = torch.cat([t.reshape(M, 2 * Cq), acc[:, 2 * Cq:]], 1) * scv
            dacc = torch.cat([tb.reshape(M, 2 * Cq), dacc[:, 2 * Cq:]], 1) * scv + 3 * 2.0 ** -23 * acc.abs()
        if geglu:   # tests/test_gpu_f16_matrix.py::test_f16_geglu: both accumulators' error through the product, |gelu'| <= 1.13
            (val, gate), (dv, dg) = acc.chunk(2, dim=-1), dacc.chunk(2, dim=-1)
            gl = 0.5 * gate * (1 + torch.erf(gate / math.sqrt(2)))
            ref = val * gl
            tol = _eps(dt) * ref.abs() + dv * gl.abs() + (val.abs() + dv) * (1.13 * dg + 3.1e-7) + 2.0 ** -23 * ref.abs() + 2.0 ** -25
        else:
            r64 = res[:M].to(f64) if res is not None else 0
            ref = acc + r64
            tol = _eps(dt) * ref.abs() + dacc + 2.0 ** -23 * (r64.abs() if res is not None else 0) + 2.0 ** -25
        _within(out, ref, tol, what)
        extra = list(extra)
        if rowstat:
            _sums_hold(extra.pop(0).t(), out, 1, 24, dt, what + " rowstat")
        if fx:
            _sums_hold(extra.pop(0), out, 0, 20, dt, what + " colsum_fx")
    return run, check


PLAIN = {
    "768x1280x1280": dict(M=768, N=1280, K=1280),
    "512x2560x640": dict(M=512, N=2560, K=640),
    "192x5120x1280": dict(M=192, N=5120, K=1280),
    "96x320x320": dict(M=96, N=320, K=320),
    "1024x960x320_rotary_colscale": dict(M=1024, N=960, K=320, rotcs=True),
    "geglu_768x2560x320": dict(M=768, N=2560, K=320, geglu=True),
    "geglu_ln_768x2560x320": dict(M=768, N=2560, K=320, geglu=True, ln=True),
    # 192 rows on 128-row tiles: the ragged last tile of one launch is a full tile of the next (the two epilogue bodies of the kernel)
    "geglu_ln_192x2560x320_ragged_tile": dict(M=192, N=2560, K=320, geglu=True, ln=True),
    "ln_192x960x320_ragged_tile": dict(M=192, N=960, K=320, ln=True),
    "bias_residual_768x1280x1280": dict(M=768, N=1280, K=1280, residual=True),
    "a2_768x1280x6400_k_slices": dict(M=768, N=1280, K=6400, a2=5120, residual=True),
    "rowstat_768x1280x1280": dict(M=768, N=1280, K=1280, residual=True, rowstat=True),
    "rowstat_96x320x320": dict(M=96, N=320, K=320, rowstat=True),
    "colsum_fx_768x1280x1280": dict(M=768, N=1280, K=1280, fx=True),
    "colsum_fx_768x640x640": dict(M=768, N=640, K=640, fx=True),
    "ragged_462x1280x1280": dict(M=462, N=1280, K=1280),
    "ragged_462x320x1600": dict(M=462, N=320, K=1600, a2=1280),
}
PLAIN_F16 = ("768x1280x1280", "geglu_ln_768x2560x320", "geglu_ln_192x2560x320_ragged_tile", "a2_768x1280x6400_k_slices", "rowstat_768x1280x1280")


@pytest.mark.parametrize("name,dt", [(n, bf16) for n in PLAIN] + [(n, f16) for n in PLAIN_F16])
def test_gemm_rows_do_not_depend_on_the_rows_behind_them(device, name, dt):
    c = PLAIN[name]
    run, check = _plain_case(device, dt, **c)
    _rows_of_m_equal(run, c["M"], f"gemm {name} {dt}", check)


CONV = {
    # n_img, H, Cin, Cout, extras
    "48x1280x11520_k_slices": dict(n_img=3, H=4, Cin=1280, Cout=1280),
    "192x1280x11520_k_slices": dict(n_img=3, H=8, Cin=1280, Cout=1280, residual=True),
    "1024x640x2880": dict(n_img=4, H=16, Cin=320, Cout=640, rowvec=True),
    "768x640x5760_k_slices_colsum_fx": dict(n_img=3, H=16, Cin=640, Cout=640, fx=True),
    "768x320x2880_colsum_fx": dict(n_img=3, H=16, Cin=320, Cout=320, fx=True),
    "stride2_192x640x2880": dict(n_img=3, H=16, Cin=320, Cout=640, stride=2),
}


@pytest.mark.parametrize("name,dt", [(n, bf16) for n in CONV] + [("192x1280x11520_k_slices", f16)])
def test_conv_rows_do_not_depend_on_the_images_behind_them(device, name, dt):
    c = CONV[name]
    n_img, H, Cin, Cout, stride = c["n_img"], c["H"], c["Cin"], c["Cout"], c.get("stride", 1)
    Ho = (H - 1) // stride + 1
    M = n_img * Ho * Ho
    x = _randn((3 * n_img * H * H, Cin), 1).to(device, dt)
    w = _randn((Cout, 9 * Cin), 2, (9 * Cin) ** -0.5).to(device, dt)
    b = _randn((Cout,), 3).to(device)
    res = _randn((3 * M, Cout), 4).to(device, dt) if c.get("residual") else None
    rv = _randn((3, Cout), 5).to(device) if c.get("rowvec") else None

    def run(reps):
        full, out = _out(reps * M, Cout, dt, device)
        cb = (reps, ops.FxArena(device, 8 * reps * Cout * 2 + 16)) if c.get("fx") else 0
        y = ops.conv3x3(x[:reps * n_img * H * H], w, reps * n_img, H, H, stride=stride, bias=b, residual=None if res is None else res[:reps * M],
                        rowvec=None if rv is None else rv[:reps], rows_per_batch=M if rv is not None else 0, out=out, tile=INV,
                        colsum_batch=cb)
        extra = []
        if c.get("fx"):
            assert isinstance(y.colsums, ops.ColSumsFx), "no accumulated column sums from this launch"
            extra.append(y.colsums.buf.sum(dim=0)[0])
        return out, full[reps * M:], extra

    def check(out, extra):
        """float64 conv2d on the stored operands of the first n_img images"""
        x64 = x[:n_img * H * H].to(f64).reshape(n_img, H, H, Cin).permute(0, 3, 1, 2)
        w64 = w.to(f64).reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)          # (weights.pack_conv3x3: k = (ky * 3 + kx) * Ci + ci)
        acc = Fn.conv2d(x64, w64, b.to(f64), stride=stride, padding=1).permute(0, 2, 3, 1).reshape(M, Cout)
        ab = Fn.conv2d(x64.abs(), w64.abs(), b.to(f64).abs(), stride=stride, padding=1).permute(0, 2, 3, 1).reshape(M, Cout)
        for t in ([rv[0].to(f64)] if rv is not None else []) + ([res[:M].to(f64)] if res is not None else []):
            acc, ab = acc + t, ab + t.abs()
        _within(out, acc, _acc_bound(acc, ab, 9 * Cin, dt), f"conv {name} {dt}")
        if c.get("fx"):
            _sums_hold(extra[0], out, 0, 20, dt, f"conv {name} colsum_fx")
    _rows_of_m_equal(run, M, f"conv {name} {dt}", check)


# ---- 2. model level -------------------------------------------------------------------------------------------------------------
_models = {}


def _model(name, device, dtype=None, **kw):
    """a SeerUNet on closed-form weights; one per (config, storage type, switches) for the module"""
    key = (name, dtype, tuple(sorted(kw.items())))
    if key not in _models:
        cfg = dict(CFG_MINI if name == "mini" else CFG_WIDE)
        m = SeerUNet(**cfg, compute_dtype=dtype, **kw)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg)), strict=True)
        _models[key] = (cfg, m.to(device).eval())
    return _models[key]


class _Spy:
    """copies of the descriptors ops._launch_gemm is handed during one forward"""

    def __init__(self, monkeypatch):
        self.descs = []
        real = ops._launch_gemm

        def launch(d, *a, **k):
            self.descs.append(_lib.GemmDesc.from_buffer_copy(d))
            return real(d, *a, **k)
        monkeypatch.setattr(ops, "_launch_gemm", launch)

    def take(self):
        d, self.descs = self.descs, []
        return d


def _auto_plan(d):
    """the plan the DEFAULT request gives this launch, with the workspace it asks for"""
    lib = _lib.load()
    d = _lib.GemmDesc.from_buffer_copy(d)
    d.tile, d.workspace, d.workspace_bytes = _lib.SEER_TILE_AUTO, None, 0
    ws = lib.seer_gemm_workspace_bytes(C.byref(d))
    if ws > 0:
        d.workspace, d.workspace_bytes = 0x1000000, ws          # (the plan reads the size, nothing is launched)
    out = (C.c_int32 * 5)()
    assert lib.seer_gemm_plan(C.byref(d), out) == 0
    return tuple(out)


@pytest.mark.parametrize("name,dtype,Fr,H,W,cond", [
    ("wide", None, 3, 16, 16, 1),
    ("mini", None, 9, 32, 32, 0),         # 18 432 rows against 2 x 9 216: the threshold pair of the row-owner launches
    ("mini", None, 6, 8, 24, 0),          # non-square; 6 frames: at 2 the default request plans 384 and 768 rows alike (the guard below)
    ("mini", f16, 3, 16, 16, 1),
])
def test_a_batch_is_its_elements(device, monkeypatch, name, dtype, Fr, H, W, cond):
    cfg, m = _model(name, device, dtype, layout_invariant=True)
    D = cfg["cross_attention_dim"]
    x = _randn((2, 4, Fr, H, W), 11).to(device)
    ctx = _randn((2, Fr, 77, D), 12).to(device)         # two prompts
    t = torch.tensor([501, 37], device=device)           # two timesteps
    spy = _Spy(monkeypatch)
    pair = m(x, t, ctx, cond_frame=cond)
    d_pair = spy.take()
    e0 = m(x[0:1].contiguous(), t[0:1], ctx[0:1].contiguous(), cond_frame=cond)
    d_one = spy.take()
    e1 = m(x[1:2].contiguous(), t[1:2], ctx[1:2].contiguous(), cond_frame=cond)
    assert m._engine.inv and d_pair and all(d.tile == INV for d in d_pair + d_one)
    # the two layouts issue the same launches, and the default request would have planned at least one of them differently: without
    # that the comparison below holds for nothing
    def by_class(descs):
        out = {}
        for d in descs:
            out.setdefault((d.mode, d.epilogue, d.N, d.K, d.K1, d.stride, d.upsample), set()).add(_auto_plan(d))
        return out
    c_pair, c_one = by_class(d_pair), by_class(d_one)
    assert set(c_pair) == set(c_one)
    moved = sum(c_pair[k] != c_one[k] for k in c_pair)
    print(f"[layout] {name} F={Fr} {H}x{W}: AUTO plans {moved} of {len(c_pair)} launch classes differently for b = 2 and b = 1")
    assert moved >= 1
    assert torch.isfinite(pair).all()
    both = torch.cat([e0, e1])
    assert torch.equal(pair, both), f"max |pair - elements| = {(pair - both).abs().amax(dim=(1, 2, 3, 4)).tolist()}"


@pytest.mark.parametrize("name,dtype,Fr,H,cond", [
    ("wide", None, 3, 16, 0),
    ("wide", None, 3, 16, 1),
    ("mini", None, 9, 32, 0),           # the row-owner launches run (9 216 rows per element)
    ("mini", None, 9, 32, 2),           # ... and behind conditioning frames the temporal feed-forward runs per element, unfused
    ("mini", f16, 3, 16, 1),
])
def test_the_mode_computes_what_the_default_engine_computes(device, name, dtype, Fr, H, cond):
    """the comparisons around this one hold the mode against itself in another layout; this one holds it against the DEFAULT engine
    (which tests/test_gpu_unet.py holds against the reference), so a mistake the mode makes alike in every layout shows.  Bound: the
    3e-2 relative L2 that tests/test_gpu_unet.py::test_unbatched_cfg_branch allows between two kernel selections of one model."""
    cfg, inv = _model(name, device, dtype, layout_invariant=True)
    _, dflt = _model(name, device, dtype)
    x = _randn((2, 4, Fr, H, H), 11).to(device)
    ctx = _randn((2, Fr, 77, cfg["cross_attention_dim"]), 12).to(device)
    t = torch.tensor([501, 37], device=device)
    got, ref = inv(x, t, ctx, cond_frame=cond), dflt(x, t, ctx, cond_frame=cond)
    assert inv._engine.inv and not dflt._engine.inv
    assert torch.isfinite(got).all() and torch.isfinite(ref).all() and ref.abs().max() > 0
    norm = lambda v: torch.linalg.vector_norm(v.double(), dim=(1, 2, 3, 4))
    rel = (norm(got - ref) / norm(ref)).tolist()
    print(f"[layout] {name} {dtype} F={Fr} {H}x{H} cond_frame={cond}: relative L2 to the default engine, per element {rel}")
    assert max(rel) < 3e-2, rel


# ---- 3. sampler: the strict twin of test_unbatched_cfg_branch ---------------------------------------------------------------------
def _sampler_inputs(cfg, device):
    b, f1, Fp, H = 1, 1, 2, 16
    D = cfg["cross_attention_dim"]
    x0_emb, x = (_randn((b, 4, f1, H, H), 1) * 0.9).to(device), _randn((b, 4, Fp, H, H), 4).to(device)
    c = _randn((b, f1 + Fp, 77, D), 2).to(device)
    uc3 = _randn((b, 77, D), 3).to(device)                                  # no frame axis: the two-call branch
    uc4 = uc3.unsqueeze(1).expand(-1, f1 + Fp, -1, -1).contiguous()         # the same embedding per frame: the batched branch
    return b, f1, x0_emb, x, c, uc3, uc4


@pytest.mark.parametrize("use_graph", [False, True])
def test_the_two_cfg_branches_of_a_ddim_step_return_the_same_bits(device, use_graph):
    cfg, m = _model("mini", device, layout_invariant=True)
    b, f1, x0_emb, x, c, uc3, uc4 = _sampler_inputs(cfg, device)
    smp = DDIMSampler(device)
    smp.make_schedule(4, verbose=False)
    kw = dict(index=3, x0_emb=x0_emb, cond_frames=f1, unconditional_guidance_scale=7.5)
    m.use_graph = use_graph
    try:
        for rnd in range(2 if use_graph else 1):        # capture, then pure replay
            t = smp._t_table[3].expand(b)               # the schedule's own timestep: under use_graph the batched branch is ONE graph
            xa, pa = smp.p_sample_ddim(m, x, c, t, unconditional_conditioning=uc4, **kw)
            xb, pb = smp.p_sample_ddim(m, x, c, t, unconditional_conditioning=uc3, **kw)
            assert torch.isfinite(xa).all() and not torch.equal(xa, x)
            assert torch.equal(xa, xb) and torch.equal(pa, pb), (rnd, (xa - xb).abs().max().item(), (pa - pb).abs().max().item())
    finally:
        m.use_graph = False


@pytest.mark.parametrize("use_graph", [False, True])
def test_the_two_cfg_branches_of_a_later_plms_step_return_the_same_bits(device, use_graph):
    cfg, m = _model("mini", device, layout_invariant=True)
    b, f1, x0_emb, x, c, uc3, uc4 = _sampler_inputs(cfg, device)
    smp = PLMSSampler(device)
    smp.make_schedule(4, verbose=False)
    old = [_randn(tuple(x.shape), 9, 0.5).to(device)]     # one earlier eps: a second-order step
    kw = dict(index=2, x0_emb=x0_emb, cond_frames=f1, unconditional_guidance_scale=7.5)
    m.use_graph = use_graph
    try:
        for rnd in range(2 if use_graph else 1):
            t = smp._t_table[2].expand(b)
            ra = smp.p_sample_plms(m, x, c, t, unconditional_conditioning=uc4, old_eps=list(old), **kw)
            rb = smp.p_sample_plms(m, x, c, t, unconditional_conditioning=uc3, old_eps=list(old), **kw)
            for a, bb in zip(ra, rb):
                assert torch.isfinite(a).all() and torch.equal(a, bb), (rnd, (a - bb).abs().max().item())
    finally:
        m.use_graph = False


# ---- 4. processes: a CFG half per rank, then two frame shards -------------------------------------------------------------------------
def _worker(rank, world, port, batch_groups, B, Fr, H, cond_frame, out_path):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    backend, dev = _backend(rank, world)
    if backend == "nccl":
        torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        from seervideoldm_amd import SeerUNet, parallel, synth
        if backend == "gloo":
            _host_staged_gathers()
        m = SeerUNet(**CFG_MINI, layout_invariant=True).to(dev)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI), device=dev), strict=True)
        m.eval()
        g = torch.Generator().manual_seed(7)
        x = torch.randn((B, 4, Fr, H, H), generator=g).to(dev)
        ctx = torch.randn((B, Fr, 77, 256), generator=g).to(dev)
        t = torch.tensor([501, 37][:B], device=dev)
        ref = m(x, t, ctx, cond_frame=cond_frame).cpu()             # one process, the switch on
        shard = parallel.attach(m, world, rank, batch_groups=batch_groups)
        eager = m(x, t, ctx, cond_frame=cond_frame).cpu()
        m.use_graph = True
        rep1 = m(x, t, ctx, cond_frame=cond_frame).cpu()            # warm-up + capture + first replay
        rep2 = m(x, t, ctx, cond_frame=cond_frame).cpu()            # pure replay
        torch.save(dict(ref=ref, eager=eager, rep1=rep1, rep2=rep2, desc=shard.describe(), inv=bool(m._engine.inv),
                        chains=int(m._engine.rowchains)), f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


def _spawn_with_a_time_limit(worker, world, args, seconds=300):
    ctx = mp.spawn(worker, args=(world, _free_port(), *args), nprocs=world, join=False)
    deadline = time.monotonic() + seconds
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"the {world} ranks did not finish within {seconds} s")


@pytest.mark.parametrize("batch_groups,B,Fr,H,cond_frame", [
    (2, 2, 9, 32, 0),         # a CFG half per rank, 9 216 rows each: the row-owner launches run on both sides
    (1, 1, 10, 32, 0),        # two frame shards of 5 frames: exact statistics exchanged, the chain in front of q|k|v reads them
    (1, 2, 3, 16, 2),         # uneven shards (2 + 1) with conditioning frames across the boundary, below the row-owner threshold
])
def test_every_rank_returns_the_bits_of_one_process(tmp_path, batch_groups, B, Fr, H, cond_frame):
    out = tmp_path / "res"
    _spawn_with_a_time_limit(_worker, 2, (batch_groups, B, Fr, H, cond_frame, str(out)))
    for rank in range(2):
        r = torch.load(f"{out}.{rank}")
        assert r["inv"] and r["desc"].startswith(f"batch_groups{batch_groups}xframe_shards{2 // batch_groups}")
        assert torch.isfinite(r["ref"]).all()
        for k in ("eager", "rep1", "rep2"):
            assert torch.equal(r[k], r["ref"]), (rank, k, (r[k] - r["ref"]).abs().max().item())
        if H == 32:
            assert r["chains"] > 0, "the row-owner chains were meant to run in this case"


# ---- 5. off means off -------------------------------------------------------------------------------------------------------------------
def test_without_the_switch_the_engine_asks_for_auto_as_before(device, monkeypatch):
    monkeypatch.delenv("SEER_LAYOUT_INVARIANT", raising=False)
    cfg, plain = _model("mini", device)                         # built without the keyword
    _, off = _model("mini", device, layout_invariant=False)
    _, on = _model("mini", device, layout_invariant=True)
    x, ctx = _randn((2, 4, 3, 16, 16), 21).to(device), _randn((2, 3, 77, cfg["cross_attention_dim"]), 22).to(device)
    t = torch.tensor([501, 37], device=device)
    spy = _Spy(monkeypatch)
    y_plain = plain(x, t, ctx, cond_frame=1)
    d_plain = spy.take()
    y_off = off(x, t, ctx, cond_frame=1)
    d_off = spy.take()
    assert not plain._engine.inv and not off._engine.inv
    assert d_plain and all(d.tile == _lib.SEER_TILE_AUTO for d in d_plain + d_off)
    assert plain._engine.ops is ops and off._engine.ops is ops           # no wrapper in the way
    assert torch.equal(y_plain, y_off)
    # the environment switch turns it on for a model that does not say
    monkeypatch.setenv("SEER_LAYOUT_INVARIANT", "1")
    env = SeerUNet(**cfg)
    env.load_state_dict(plain.state_dict(), strict=True)
    env = env.to(device).eval()
    y_env = env(x, t, ctx, cond_frame=1)
    d_env = spy.take()
    assert env._engine.inv and all(d.tile == INV for d in d_env)
    assert torch.equal(y_env, on(x, t, ctx, cond_frame=1))
    # ... and an explicit False wins over it
    off._engine = None
    assert torch.equal(off(x, t, ctx, cond_frame=1), y_plain) and not off._engine.inv
