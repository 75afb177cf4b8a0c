"""TEST INFRASTRUCTURE ONLY -- a recording wrapper around tests/shape_ops_backend.py: every call the engine makes is written down as
(op, rows, details) before the shape-only stand-in answers it, and the launches of the GEMM family are kept as the fields of the
seer_gemm_desc the real wrapper (seervideoldm_amd.ops) would build: mode, epilogue flags, M, N, K, K1, stride / upsample, batch and
the optional outputs asked.  tests/test_layout_invariant_plan.py walks the full-size engine through it on torch's meta device.

Beyond the stand-in it answers the exact-statistics calls of the layout-invariant engine (FxArena, ColSumsFx, groupnorm_stats_fx,
groupnorm_apply_fx: shapes only), and it asks the PRODUCT's ff_fused_pays / rowchain_pays, so that a patched ops.device_cus is seen.
Never imported by the product package."""
from __future__ import annotations

import ctypes as C

import torch

from seervideoldm_amd import _lib
from seervideoldm_amd import ops as real_ops
from tests import shape_ops_backend as sob

bf16 = torch.bfloat16


class ColSumsFx:
    def __init__(self, batch, C_):
        self.batch, self.C, self.reduced = batch, C_, False


class FxArena:
    def __init__(self, device, int64_elems):
        self.n = int64_elems

    def reset(self):
        pass


class RecordingOps:
    def __init__(self, batch: int):
        self.B = batch              # rows are written down per batch element
        self.element = None         # set by the walker around a launch over ONE batch element's rows (the engine's per-element
                                    # feed-forward loop): its index; rows are then the launch's own, elements > 0 are not kept
        self.calls = []             # (op, rows per batch element or None, details)
        self.gemms = []             # dicts of seer_gemm_desc fields, one per launch of the GEMM family
        self.FxArena, self.ColSumsFx = FxArena, ColSumsFx

    def __getattr__(self, name):
        return getattr(sob, name)

    # ---- the two row-owner choices: the product's own rules (they read ops.device_cus) ----------------------------------
    def ff_fused_pays(self, rows, n_cu=None):
        return real_ops.ff_fused_pays(rows, n_cu)

    def rowchain_pays(self, rows, n_cu=None, products=4):
        return real_ops.rowchain_pays(rows, n_cu, products)

    def _pb(self, rows):
        if self.element is not None:
            return rows
        return rows // self.B if rows % self.B == 0 else ("ragged", rows)

    def _keep(self, call):
        if not self.element:        # (None: a launch over the whole batch; 0: batch element 0's own launch)
            self.calls.append(call)

    def _folds(self, M, N, K, epi, tile, dt):
        """seer_gemm_lnfold_ok of the library itself for the launch the real wrapper would build (addresses: aligned, never read)"""
        d = _lib.GemmDesc()
        d.A, d.W, d.C, d.bias = 0x100000, 0x300000, 0x700000, 0x400000
        d.M, d.N, d.K, d.K1, d.lda = M, N, K, K, K
        d.ldc = N // 2 if epi & _lib.SEER_EPI_GEGLU else N
        d.mode, d.epilogue, d.tile, d.batch = _lib.SEER_GEMM_PLAIN, epi | (_lib.SEER_EPI_F16 if dt == torch.float16 else 0), tile, 1
        d.ln_rowstat, d.ln_wsum, d.ln_eps = 0xC00000, 0xD00000, 1e-5
        return bool(_lib.load().seer_gemm_lnfold_ok(C.byref(d)))

    def _gemm_rec(self, op, **f):
        f = dict(op=op, stride=1, upsample=0, batch=1, K1=f["K"], colsum=False, colsum_fx=False, rowstat=False, ln=False, a2=False,
                 bias=False, residual=False, rowvec=False, rotary=False, colscale=False) | f
        self.gemms.append(f)
        self._keep((op, self._pb(f["M"]) if f["batch"] == 1 or op == "conv_up2x" else f["M"],
                           tuple(sorted((k, v) for k, v in f.items() if k not in ("M", "batch", "op")))))

    # ---- GEMM family -------------------------------------------------------------------------------------------------------
    def gemm(self, a, w, *, bias=None, residual=None, rowvec=None, rows_per_batch=0, a2=None, geglu=False, silu=False, out_f32=False,
             out=None, tile=0, splits=0, rotary=None, col_scale=None, colsum_batch=0, rowstat=False, ln=None):
        epi = (_lib.SEER_EPI_GEGLU if geglu else 0) | (_lib.SEER_EPI_SILU if silu else 0) | (_lib.SEER_EPI_OUT_F32 if out_f32 else 0) | \
              (_lib.SEER_EPI_ROTARY if rotary is not None else 0) | (_lib.SEER_EPI_COLSCALE if col_scale is not None else 0)
        if tile == _lib.SEER_TILE_AUTO_INVARIANT:
            # the stand-in models the default request's fold rule only: under the invariant request the library is asked
            if ln is not None and not self._folds(a.shape[0], w.shape[0], w.shape[1], epi, tile, a.dtype):
                return None
            y = sob.gemm(a, w, bias=bias, residual=residual, rowvec=rowvec, rows_per_batch=rows_per_batch, a2=a2, geglu=geglu, silu=silu,
                         out_f32=out_f32, out=out, tile=tile, splits=splits, rotary=rotary, col_scale=col_scale,
                         colsum_batch=colsum_batch, rowstat=rowstat)
        else:
            y = sob.gemm(a, w, bias=bias, residual=residual, rowvec=rowvec, rows_per_batch=rows_per_batch, a2=a2, geglu=geglu, silu=silu,
                         out_f32=out_f32, out=out, tile=tile, splits=splits, rotary=rotary, col_scale=col_scale,
                         colsum_batch=colsum_batch, rowstat=rowstat, ln=ln)
        if y is not None:
            self._gemm_rec("gemm", mode=_lib.SEER_GEMM_PLAIN, epilogue=epi, M=a.shape[0], N=w.shape[0], K=w.shape[1], K1=a.shape[1],
                           tile=tile, splits=splits, a2=a2 is not None, bias=bias is not None, residual=residual is not None,
                           rowvec=rowvec is not None, rotary=rotary is not None, colscale=col_scale is not None,
                           colsum_fx=isinstance(colsum_batch, tuple), colsum=bool(colsum_batch) and not isinstance(colsum_batch, tuple),
                           rowstat=bool(rowstat), ln=ln is not None)
        return y

    def gemm_batched(self, a, w, *, trans_out=False, out=None, bias=None, out_f32=False, tile=0, col_scale=None):
        epi = (_lib.SEER_EPI_TRANS_OUT if trans_out else 0) | (_lib.SEER_EPI_OUT_F32 if out_f32 else 0) | \
              (_lib.SEER_EPI_COLSCALE if col_scale is not None else 0)
        self._gemm_rec("gemm_batched", mode=_lib.SEER_GEMM_PLAIN, epilogue=epi, M=a.shape[1], N=w.shape[-2], K=a.shape[2], batch=a.shape[0],
                       tile=tile, splits=0, bias=bias is not None, colscale=col_scale is not None)
        return sob.gemm_batched(a, w, trans_out=trans_out, out=out, bias=bias, out_f32=out_f32, tile=tile, col_scale=col_scale)

    def conv3x3(self, x, w, n_img, Hin, Win, *, stride=1, upsample=False, bias=None, residual=None, rowvec=None, rows_per_batch=0,
                out=None, tile=0, splits=0, pad_after_only=False, colsum_batch=0):
        y = sob.conv3x3(x, w, n_img, Hin, Win, stride=stride, upsample=upsample, bias=bias, residual=residual, rowvec=rowvec,
                        rows_per_batch=rows_per_batch, out=out, tile=tile, splits=splits, pad_after_only=pad_after_only,
                        colsum_batch=colsum_batch)
        self._gemm_rec("conv3x3", mode=_lib.SEER_GEMM_CONV3X3, epilogue=0, M=y.shape[0], N=w.shape[0], K=w.shape[1], stride=stride,
                       tile=tile, splits=splits, bias=bias is not None, residual=residual is not None, rowvec=rowvec is not None,
                       colsum_fx=isinstance(colsum_batch, tuple), colsum=bool(colsum_batch) and not isinstance(colsum_batch, tuple))
        return y

    def conv_up2x(self, x, w4, n_img, Hin, Win, *, bias=None, out=None, tile=0, colsum_batch=0):
        self._gemm_rec("conv_up2x", mode=_lib.SEER_GEMM_CONV3X3, epilogue=0, M=x.shape[0], N=w4.shape[1], K=w4.shape[2], upsample=2,
                       batch=4, tile=tile, splits=1, bias=bias is not None,
                       colsum_fx=isinstance(colsum_batch, tuple), colsum=bool(colsum_batch) and not isinstance(colsum_batch, tuple))
        return sob.conv_up2x(x, w4, n_img, Hin, Win, bias=bias, out=out, tile=tile, colsum_batch=colsum_batch)

    def conv_out(self, x, w, bias, B, Fr, H, W, tile=0):
        if w.dtype in (bf16, torch.float16):        # the implicit-GEMM form (ops.conv_out): one GEMM per sample, transposed fp32 store
            self._gemm_rec("conv_out", mode=_lib.SEER_GEMM_CONV3X3, epilogue=_lib.SEER_EPI_TRANS_OUT | _lib.SEER_EPI_OUT_F32,
                           M=Fr * H * W, N=w.shape[0], K=w.shape[1], batch=B, tile=tile, splits=1, bias=True)
        else:
            self._keep(("conv_out", Fr * H * W, ()))
        return sob.conv_out(x, w, bias, B, Fr, H, W)

    # ---- everything else: the op, its rows per batch element, what selects a kernel ------------------------------------------
    def attention(self, q, k, v, out, **kw):
        kw = {k_: v_ for k_, v_ in kw.items() if k_ not in ("batch",)}
        self._keep(("attention", self._pb(q.shape[0]), tuple(sorted((k_, str(v_)) for k_, v_ in kw.items()))))
        return out

    def ff_fused(self, h, x, *a, **k):
        y = sob.ff_fused(h, x, *a, **k)
        if y is not None:
            self._keep(("ff_fused", self._pb(h.shape[0]), (("pre", k.get("pre") is not None), ("colsum", bool(k.get("colsum_batch"))))))
        return y

    def rowchain(self, inp, w1f, **k):
        r = sob.rowchain(inp, w1f, **k)
        if r is not None:
            self._keep(("rowchain", self._pb(inp.shape[0]), (("gn", k.get("gn") is not None), ("n2", None if k.get("w2f") is None else
                                                                                                      k["w2f"].numel() // (320 * 320)))))
        return r

    def layernorm(self, x, *a, **k):
        self._keep(("layernorm", self._pb(x.shape[0]), ()))
        return sob.layernorm(x, *a, **k)

    def groupnorm_stats(self, x1, x2, batch, groups, stats):
        self._keep(("groupnorm_stats", self._pb(x1.shape[0]), ()))
        return stats

    def groupnorm_apply(self, x1, x2, batch, groups, stats, *a, **k):
        self._keep(("groupnorm_apply", self._pb(x1.shape[0]), ()))
        return sob.groupnorm_apply(x1, x2, batch, groups, stats, *a, **k)

    def groupnorm_stats_fx(self, x, batch, arena=None):
        self._keep(("groupnorm_stats_fx", self._pb(x.shape[0]), ()))
        return ColSumsFx(batch, x.shape[1])

    def groupnorm_apply_fx(self, x1, x2, fx1, fx2, batch, groups, count, eps, gamma, beta, silu, out=None, stats_out=None):
        self._keep(("groupnorm_apply_fx", self._pb(x1.shape[0]), ()))
        return sob.groupnorm_apply(x1, x2, batch, groups, None, count, eps, gamma, beta, silu)

    def linear_smallm(self, x, w, bias, **k):
        self._keep(("linear_smallm", self._pb(x.shape[0]), (w.shape[0], w.shape[1])))
        return sob.linear_smallm(x, w, bias, **k)

    def conv_in(self, x, w, bias, **k):
        self._keep(("conv_in", x.shape[2] * x.shape[3] * x.shape[4], ()))
        return sob.conv_in(x, w, bias)
