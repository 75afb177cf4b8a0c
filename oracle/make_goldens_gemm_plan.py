"""Records what a built libseer_hip.so answers about GEMM launch plans -> tests/golden/gemm_plan_parent.npz.

    python -m oracle.make_goldens_gemm_plan PATH/libseer_hip.so [--plan-lib PATH/libseer_hip.so] [-o OUT.npz]

The fixture pins the host decisions of csrc/gemm.hip (which kernel, which tile, how many K slices, which reduce pass, and the six
queries seer_gemm_workspace_bytes / sync_bytes / colsum_rows / colsum_fx_layout / rowstat_ok / lnfold_ok) over a grid of
descriptors; tests/test_gemm_plan.py compares the library under test against it.  It is recorded from the PARENT of a change to
those rules, never from the code under test.  The six answers come from the first library; the five words of seer_gemm_plan come
from --plan-lib where that is given (a parent that predates seer_gemm_plan cannot report its launch decision: --plan-lib is
then a copy of it whose seer_gemm_bf16 records what it would have launched instead of launching), else from the first library.

Nothing here touches a GPU: the queries are host functions, every pointer is a fake aligned address and nothing is dereferenced.

Grid (a): every distinct GEMM-class call (gemm, gemm_batched, conv3x3, conv_up2x) of the meta-device schedule walk of
tests/test_roofline_accounting.py at CFG batch 2 and 1, 12 / 14 / 17 frames, the 64x64 latent, the Bridge configuration and a
rank's share of 3 and of 6 frames -- each without buffers and with the buffers the library asks for, with and without column sums
(per tile and accumulated), with and without the ln= / rowstat= the engine passes.
Grid (b): a seeded sample of the product of shapes, modes, epilogue flags, tile codes, split requests, batch counts, buffer
states (absent / exact / one byte short) and misaligned pointers listed below."""
from __future__ import annotations

import argparse
import ctypes as C
import itertools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from seervideoldm_amd import _lib  # noqa: E402

OUT = ROOT / "tests" / "golden" / "gemm_plan_parent.npz"

# the integer and pointer fields of seer_gemm_desc (col_scale and ln_eps, the two floats, decide nothing)
FIELDS = [n for n, t in _lib.GemmDesc._fields_ if t is not C.c_float]
ANSWERS = ["workspace_bytes", "sync_bytes", "colsum_rows", "colsum_fx_rows", "colsum_fx_reps", "rowstat_ok", "lnfold_ok"]
PLAN = ["status", "kernel", "tile", "splits", "reduce"]

# fake device addresses, 16-byte aligned
P = dict(A=0x10000, W=0x20000, C=0x30000, A2=0x40000, bias=0x50000, residual=0x60000, rowvec=0x70000, rot_table=0x80000,
         sync=0x90000, colsum=0xA0000, colsum_fx=0xB0000, rowstat=0xC0000, ln_rowstat=0xD0000, ln_wsum=0xE0000,
         workspace=0x100000)
GEGLU, OUT_F32, SILU, TRANS_OUT, ROTARY, COLSCALE, F16, QUICKGELU = 1, 2, 4, 8, 16, 32, 64, 128
TILE_CODES = list(range(0, 4)) + list(range(5, 23)) + [77]          # every code of the header and one that is none


def bind(path):
    """a parent's library, bound by this tree's header for the entry points it exports (one that predates seer_gemm_plan has none)"""
    return _lib.bind(C.CDLL(str(path)))


def to_struct(d: dict) -> _lib.GemmDesc:
    s = _lib.GemmDesc()
    for k, v in d.items():
        setattr(s, k, int(v))
    return s


def answers(lib, d: dict, fx_rpb: int):
    s = C.byref(to_struct(d))
    reps = C.c_int32(0)
    fx = lib.seer_gemm_colsum_fx_layout(s, fx_rpb, C.byref(reps))
    return [lib.seer_gemm_workspace_bytes(s), lib.seer_gemm_sync_bytes(s), lib.seer_gemm_colsum_rows(s), fx, reps.value,
            lib.seer_gemm_rowstat_ok(s), lib.seer_gemm_lnfold_ok(s)]


def plan(lib, d: dict):
    out = (C.c_int32 * 5)()
    rc = lib.seer_gemm_plan(C.byref(to_struct(d)), out)
    assert rc == 0, rc
    return list(out)


# ---- descriptors as ops.py builds them ------------------------------------------------------------------------------------------
def base(M, N, K, **kw):
    d = dict(A=P["A"], W=P["W"], C=P["C"], M=M, N=N, K=K, K1=K, lda=K, ldc=N, batch=1)
    d.update(kw)
    return d


def conv_desc(M, N, K, n_img, Hin, Win, Hout, Wout, stride=1, upsample=0, **kw):
    cin = K // (4 if upsample == 2 else 9)
    return base(M, N, K, lda=0, mode=1, Hin=Hin, Win=Win, Cin=cin, Hout=Hout, Wout=Wout, stride=stride, upsample=upsample,
                batch=4 if upsample == 2 else 1, splits=1 if upsample == 2 else 0, **kw)


class Recorder:
    """tests/shape_ops_backend with the GEMM-class calls written down as descriptors (the fields ops.py sets)"""

    def __init__(self, sob):
        self._sob = sob
        self.calls = []          # (descriptor, colsum batch or 0, ln?, rowstat?)

    def __getattr__(self, name):
        return getattr(self._sob, name)

    def gemm(self, a, w, *, bias=None, residual=None, rowvec=None, rows_per_batch=0, a2=None, geglu=False, silu=False, out_f32=False,
             out=None, tile=0, splits=0, rotary=None, col_scale=None, colsum_batch=0, rowstat=False, ln=None):
        M, K1 = a.shape
        N, K = w.shape
        d = base(M, N, K, K1=K1, lda=a.stride(0), tile=tile, splits=splits, ldc=out.stride(0) if out is not None else (N // 2 if geglu else N),
                 epilogue=(GEGLU if geglu else 0) | (SILU if silu else 0) | (OUT_F32 if out_f32 else 0))
        if a2 is not None:
            d.update(A2=P["A2"], lda2=a2.stride(0))
        if bias is not None:
            d.update(bias=P["bias"])
        if residual is not None:
            d.update(residual=P["residual"], ldr=residual.stride(0))
        if rowvec is not None:
            d.update(rowvec=P["rowvec"], rowvec_ld=rowvec.stride(0), rows_per_batch=rows_per_batch)
        if rotary is not None:
            _, tpb, pos_off, hd, rd, cols = rotary
            d.update(epilogue=d["epilogue"] | ROTARY, rot_table=P["rot_table"], rot_tokens_per_batch=tpb, rot_pos_offset=pos_off,
                     rot_head_dim=hd, rot_dim=rd, rot_cols=cols)
        if col_scale is not None:
            d.update(epilogue=d["epilogue"] | COLSCALE, col_scale_cols=int(col_scale[1]))
        self.calls.append((d, _cb(colsum_batch), ln is not None, bool(rowstat)))
        return self._sob.gemm(a, w, bias=bias, residual=residual, rowvec=rowvec, rows_per_batch=rows_per_batch, a2=a2, geglu=geglu,
                              silu=silu, out_f32=out_f32, out=out, tile=tile, splits=splits, rotary=rotary, col_scale=col_scale,
                              colsum_batch=colsum_batch, rowstat=rowstat, ln=ln)

    def gemm_batched(self, a, w, *, trans_out=False, out=None, bias=None, out_f32=False, tile=0, col_scale=None):
        Bt, M, K = a.shape
        N = w.shape[-2]
        d = base(M, N, K, ldc=M if trans_out else N, batch=Bt, strideA=M * K, strideW=N * K if w.dim() == 3 else 0, strideC=M * N,
                 tile=tile, epilogue=(TRANS_OUT if trans_out else 0) | (OUT_F32 if out_f32 else 0))
        if bias is not None:
            d.update(bias=P["bias"])
        if col_scale is not None:
            d.update(epilogue=d["epilogue"] | COLSCALE, col_scale_cols=int(col_scale[1]))
        self.calls.append((d, 0, False, False))
        return self._sob.gemm_batched(a, w, trans_out=trans_out, out=out, bias=bias, out_f32=out_f32, tile=tile, col_scale=col_scale)

    def conv3x3(self, x, w, n_img, Hin, Win, *, stride=1, upsample=False, bias=None, residual=None, rowvec=None, rows_per_batch=0,
                out=None, tile=0, splits=0, pad_after_only=False, colsum_batch=0):
        Hs, Ws = (2 * Hin, 2 * Win) if upsample else (Hin, Win)
        pad = 1 if pad_after_only else 2
        Ho, Wo = (Hs + pad - 3) // stride + 1, (Ws + pad - 3) // stride + 1
        N, K = w.shape
        d = conv_desc(n_img * Ho * Wo, N, K, n_img, Hin, Win, Ho, Wo, stride=stride, upsample=int(upsample), tile=tile,
                      pad_after_only=int(pad_after_only))
        d["splits"] = splits
        if bias is not None:
            d.update(bias=P["bias"])
        if residual is not None:
            d.update(residual=P["residual"], ldr=residual.stride(0))
        if rowvec is not None:
            d.update(rowvec=P["rowvec"], rowvec_ld=rowvec.stride(0), rows_per_batch=rows_per_batch)
        self.calls.append((d, _cb(colsum_batch), False, False))
        return self._sob.conv3x3(x, w, n_img, Hin, Win, stride=stride, upsample=upsample, bias=bias, residual=residual, rowvec=rowvec,
                                 rows_per_batch=rows_per_batch, out=out, tile=tile, splits=splits, pad_after_only=pad_after_only,
                                 colsum_batch=colsum_batch)

    def conv_up2x(self, x, w4, n_img, Hin, Win, *, bias=None, out=None, tile=0, colsum_batch=0):
        _, N, K = w4.shape
        d = conv_desc(n_img * Hin * Win, N, K, n_img, Hin, Win, 2 * Hin, 2 * Win, upsample=2, tile=tile)
        if bias is not None:
            d.update(bias=P["bias"])
        self.calls.append((d, _cb(colsum_batch), False, False))
        return self._sob.conv_up2x(x, w4, n_img, Hin, Win, bias=bias, out=out, tile=tile, colsum_batch=colsum_batch)


def _cb(colsum_batch):
    return int(colsum_batch[0] if isinstance(colsum_batch, tuple) else colsum_batch)


def walk(B, Fr, latent):
    """one evaluation of the full-size engine on the meta device (tests/test_roofline_accounting.py::_walk_config2)"""
    import torch
    from seervideoldm_amd import SeerUNet, synth
    from seervideoldm_amd.unet import _Engine
    from tests import shape_ops_backend as sob
    rec = Recorder(sob)
    eng = _Engine(SeerUNet(**dict(synth.SD15_UNET_CFG)).to("meta"), ops=rec)
    eng._rotary_table = lambda tb, T: sob.rotary_table(eng.w[tb + ".attn1.rotary_emb.freqs"], T)
    x = torch.empty((B, 4, Fr, latent, latent), device="meta")
    ctx = torch.empty((B, Fr, 77, 768), device="meta")
    eng._kv_key = None
    eng._context = lambda c: (torch.empty((B * Fr * 77, 768), dtype=torch.bfloat16, device="meta"), 77)
    eng.run(x, torch.empty((B,), dtype=torch.long, device="meta"), ctx, 0)
    return rec.calls, B


WALKS = [(2, 12, 32), (1, 12, 32), (2, 14, 32), (2, 17, 32), (2, 12, 64), (8, 16, 32), (2, 3, 32), (2, 6, 32)]


def grid_a():
    seen, out = set(), []
    for B, Fr, latent in WALKS:
        calls, batch = walk(B, Fr, latent)
        for d, cb, ln, rowstat in calls:
            cb = cb or batch                     # "with colsum_batch": the call's own, else the evaluation's batch
            for with_ln, with_rs in sorted({(False, False), (ln, False), (False, rowstat), (ln, rowstat)}):
                v = dict(d)
                if with_ln:
                    v.update(ln_rowstat=P["ln_rowstat"], ln_wsum=P["ln_wsum"])
                if with_rs:
                    v.update(rowstat=P["rowstat"])
                key = tuple(sorted(v.items())) + (cb,)
                if key not in seen:
                    seen.add(key)
                    out.append((v, cb))
    return out


# ---- grid (b) -------------------------------------------------------------------------------------------------------------------
MS = [64, 96, 256, 384, 768, 924, 1536, 3072, 6144, 12288, 24576, 28672, 131072]
NS = [64, 320, 640, 960, 1280, 1920, 2560, 3840, 5120]
KS = [64, 320, 640, 1280, 2880, 5760, 6400, 11520]
# output rows as images: M = n_img * H * W (H = W even, so that the nearest-2x read-through form has a source image)
IMAGES = {64: (1, 8), 96: (6, 4), 256: (1, 16), 384: (24, 4), 768: (12, 8), 924: (231, 2), 1536: (24, 8), 3072: (12, 16), 6144: (24, 16),
          12288: (12, 32), 24576: (24, 32), 28672: (28, 32), 131072: (128, 32)}
# the flags singly and in the pairs (triples) the engines use: q|k|v projections, the fp16 engine, the VAE's batched products
EPILOGUES = [0, GEGLU, OUT_F32, SILU, TRANS_OUT, ROTARY, COLSCALE, F16, QUICKGELU, ROTARY | COLSCALE, F16 | GEGLU, F16 | SILU,
             F16 | ROTARY | COLSCALE, TRANS_OUT | F16, OUT_F32 | COLSCALE, OUT_F32 | F16]
SPLITS = [0, 1, 2, 4, 16]
FEATURES = ["none", "colsum", "colsum_fx", "rowstat", "ln", "ln_wsum_misaligned"]
BUFFERS = ["absent", "exact", "short"]


def shape_desc(M, N, K, form):
    """form: plain | conv (3x3, stride 1) | conv_s2 | conv_up1 (nearest-2x read through) | conv_up2 (four phase convs)"""
    if form == "plain":
        return base(M, N, K)
    n_img, h = IMAGES[M]
    if form == "conv_up2":
        return conv_desc(M, N, K, n_img, h, h, 2 * h, 2 * h, upsample=2) if K % 256 == 0 else None
    if K % 576:
        return None
    if form == "conv":
        return conv_desc(M, N, K, n_img, h, h, h, h)
    if form == "conv_s2":
        return conv_desc(M, N, K, n_img, 2 * h, 2 * h, h, h, stride=2)
    return conv_desc(M, N, K, n_img, h // 2, h // 2, h, h, upsample=1)


def with_epilogue(d, epi):
    d = dict(d, epilogue=epi)
    N = d["N"]
    if epi & GEGLU:
        d["ldc"] = N // 2
    if epi & TRANS_OUT:
        d["ldc"] = d["M"]
    if epi & ROTARY:
        d.update(rot_table=P["rot_table"], rot_tokens_per_batch=12, rot_head_dim=64, rot_dim=32, rot_cols=max(64, N * 2 // 3 // 64 * 64))
    if epi & COLSCALE:
        d["col_scale_cols"] = max(4, N // 3 // 4 * 4)
    return d


def with_batch(d, batch):
    if batch > 1 and d.get("mode", 0) == 0:
        d = dict(d, batch=batch, strideA=d["M"] * d["K"], strideW=d["N"] * d["K"], strideC=d["M"] * d["N"])
    return d


def with_feature(d, feature):
    if feature == "rowstat":
        return dict(d, rowstat=P["rowstat"])
    if feature in ("ln", "ln_wsum_misaligned"):
        return dict(d, ln_rowstat=P["ln_rowstat"], ln_wsum=P["ln_wsum"] + (4 if feature == "ln_wsum_misaligned" else 0))
    return d                                     # column sums are added once the buffers are known: with_buffers


def grid_b(rng):
    out = []
    shapes = [(M, N, K, form) for M, N, K in itertools.product(MS, NS, KS)
              for form in ("plain", "conv", "conv_s2", "conv_up1", "conv_up2") if shape_desc(M, N, K, form) is not None]
    # every shape as AUTO hands it out, plain and with each kind of column sums, without buffers and with the ones asked for
    for M, N, K, form in shapes:
        d = shape_desc(M, N, K, form)
        for feature, buffers in itertools.product(("none", "colsum", "colsum_fx"), ("absent", "exact")):
            out.append((d, feature, buffers))
    # the 256 x 320 tile by name: slices by the cost model and by request, with and without room for them
    for M, N, K, form in shapes:
        if N % 320 == 0 and form in ("plain", "conv"):
            for splits, buffers in itertools.product((0, 4), BUFFERS):
                out.append((dict(shape_desc(M, N, K, form), tile=22, splits=splits), "colsum" if splits else "none", buffers))
    # a seeded sample of the rest of the product
    for M, N, K, form in shapes:
        for _ in range(6):
            d = with_epilogue(shape_desc(M, N, K, form), EPILOGUES[rng.integers(len(EPILOGUES))])
            d = with_batch(d, (1, 4)[rng.integers(2)])
            d.update(tile=TILE_CODES[rng.integers(len(TILE_CODES))] if rng.integers(3) else 0)
            if d.get("upsample", 0) != 2 or rng.integers(2):
                d["splits"] = SPLITS[rng.integers(len(SPLITS))]
            extra = rng.integers(8)
            if extra == 0 and d.get("mode", 0) == 0:
                d.update(A2=P["A2"], K1=max(64, d["K"] // 128 * 64), lda2=d["K"])
            elif extra == 1:
                d.update(residual=P["residual"], ldr=d["ldc"])
            elif extra == 2:
                d.update(rowvec=P["rowvec"], rowvec_ld=d["N"], rows_per_batch=d["M"] // 2)
            elif extra == 3:
                d["C"] = P["C"] + 8              # misaligned output
            feature = FEATURES[rng.integers(len(FEATURES))]
            out.append((with_feature(d, feature), feature, BUFFERS[rng.integers(len(BUFFERS))]))
    # descriptors the argument checks refuse, one per check
    ok = base(1536, 1280, 1280)
    for bad in (dict(M=0), dict(K=1300), dict(C=0), dict(N=1282), dict(ldc=1282), dict(lda=1284), dict(epilogue=SILU | QUICKGELU),
                dict(rowvec=P["rowvec"], rows_per_batch=0), dict(residual=P["residual"], ldr=1282), dict(mode=2),
                dict(epilogue=ROTARY), dict(epilogue=COLSCALE, col_scale_cols=0), dict(A2=P["A2"], K1=1344, lda2=8),
                dict(mode=1, Cin=128, Hin=8, Win=8, Hout=8, Wout=8, stride=1), dict(mode=1, Cin=320, Hin=8, Win=8, Hout=8, Wout=8, stride=3)):
        out.append((dict(ok, **bad), "none", "absent"))
    return out


# ---- buffers and column sums, as ops._launch_gemm provides them -------------------------------------------------------------------
def with_buffers(lib, d, buffers, colsum, cb):
    """the descriptor with the workspace / sync the library asks for (exact, or one byte short) and, where asked and possible,
    the column sums of `cb` batch elements: per tile ("colsum") or accumulated ("colsum_fx")"""
    d = dict(d)
    if buffers != "absent":
        s = C.byref(to_struct(d))
        short = 1 if buffers == "short" else 0
        ws, sy = lib.seer_gemm_workspace_bytes(s), lib.seer_gemm_sync_bytes(s)
        if ws > 0:
            d.update(workspace=P["workspace"], workspace_bytes=ws - short)
        if sy > 0:
            d.update(sync=P["sync"], sync_bytes=sy - short)
    if colsum == "colsum":
        d["colsum"] = P["colsum"]
    elif colsum == "colsum_fx":
        reps = C.c_int32(1)
        rpb = d["M"] // cb if cb and d["M"] % cb == 0 else d["M"]
        lib.seer_gemm_colsum_fx_layout(C.byref(to_struct(d)), rpb, C.byref(reps))
        d.update(colsum_fx=P["colsum_fx"], colsum_fx_rows=rpb, colsum_fx_reps=reps.value)
    return d


def build_grid(lib):
    rows = []                                    # (descriptor, rows per batch element for the colsum_fx_layout query)
    for d, cb in grid_a():
        for buffers, colsum in itertools.product(("absent", "exact"), ("none", "colsum", "colsum_fx")):
            rows.append((with_buffers(lib, d, buffers, colsum, cb), d["M"] // cb if d["M"] % cb == 0 else d["M"]))
    n_a = len(rows)
    for d, feature, buffers in grid_b(np.random.default_rng(20261018)):
        cb = 2 if d["M"] % 2 == 0 else 1
        rows.append((with_buffers(lib, d, buffers, feature if feature.startswith("colsum") else "none", cb), d["M"] // cb))
    seen, uniq, part = set(), [], []
    for i, (d, rpb) in enumerate(rows):
        key = tuple(int(d.get(f, 0)) for f in FIELDS) + (rpb,)
        if key not in seen:
            seen.add(key)
            uniq.append(key)
            part.append(0 if i < n_a else 1)
    return np.array(uniq, dtype=np.int64), np.array(part, dtype=np.int8)


def record(lib, plan_lib, out_path):
    grid, part = build_grid(lib)
    desc, fx_rpb = grid[:, :-1], grid[:, -1]
    ans = np.zeros((len(desc), len(ANSWERS)), dtype=np.int64)
    pl = np.zeros((len(desc), len(PLAN)), dtype=np.int32)
    for i, row in enumerate(desc):
        d = dict(zip(FIELDS, row))
        ans[i] = answers(lib, d, int(fx_rpb[i]))
        if plan_lib is not None:
            pl[i] = plan(plan_lib, d)
    null = C.POINTER(_lib.GemmDesc)()
    reps = C.c_int32(0)
    null_ans = np.array([lib.seer_gemm_workspace_bytes(null), lib.seer_gemm_sync_bytes(null), lib.seer_gemm_colsum_rows(null),
                         lib.seer_gemm_colsum_fx_layout(null, 64, C.byref(reps)), reps.value, lib.seer_gemm_rowstat_ok(null),
                         lib.seer_gemm_lnfold_ok(null)], dtype=np.int64)
    save = dict(fields=np.array(FIELDS), answer_names=np.array(ANSWERS), plan_names=np.array(PLAN), part=part,
                desc=desc, fx_rows_per_batch=fx_rpb.astype(np.int32), answers=ans, null_answers=null_ans)
    if plan_lib is not None:
        save["plan"] = pl
    np.savez_compressed(out_path, **save)
    return len(desc), int((part == 0).sum())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib", type=Path, help="the library whose six answers are recorded")
    ap.add_argument("--plan-lib", type=Path, default=None, help="the library whose seer_gemm_plan is recorded (default: the first)")
    ap.add_argument("-o", "--out", type=Path, default=OUT)
    a = ap.parse_args(argv)
    lib = bind(a.lib)
    plan_lib = bind(a.plan_lib) if a.plan_lib else (lib if hasattr(lib, "seer_gemm_plan") else None)
    n, n_a = record(lib, plan_lib, a.out)
    print(f"{a.out}: {n} descriptors ({n_a} from the schedule walks), {a.out.stat().st_size} bytes"
          + ("" if plan_lib is not None else "; no seer_gemm_plan in this library: plan words not recorded"))


if __name__ == "__main__":
    main()
