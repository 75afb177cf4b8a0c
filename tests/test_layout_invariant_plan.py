"""SEER_TILE_AUTO_INVARIANT on the host: the plan of csrc/gemm.hip under that request, and the answers of the queries derived from
it, do not move with the row count -- and the layout-invariant engine issues the same launches for one batch element whatever the
batch and the device.  Host functions only: no GPU, fake aligned addresses, nothing is dereferenced (as tests/test_gemm_plan.py).

The grid: every (mode, stride / upsample, epilogue, N, K, K1, batch > 1) the full-size engine issues at BASELINE config 2 (walked
on the meta device through tests/recording_ops_backend.py, default and invariant mode, with its 2 conditioning frames and with
none), each with every optional output asked that the launch form can carry, plus a 576-pair grid of plain products and 3x3 convs
at the UNet's widths; all crossed with 14 row counts from 16 to 98 304."""
import ctypes as C
import itertools

import pytest
import torch

from seervideoldm_amd import SeerUNet, _lib, synth
from seervideoldm_amd import ops as real_ops
from seervideoldm_amd.unet import _Engine, _LaunchPlan
from tests import shape_ops_backend as sob
from tests.recording_ops_backend import RecordingOps

INV, AUTO = _lib.SEER_TILE_AUTO_INVARIANT, _lib.SEER_TILE_AUTO
MS = (16, 48, 96, 192, 384, 768, 1536, 3072, 6144, 8192, 12288, 24576, 28672, 98304)
OUTPUTS = ("none", "colsum", "colsum_fx", "rowstat", "ln")
K_TILE, K_SPLITK = _lib.SEER_GEMM_KERNEL_TILE, _lib.SEER_GEMM_KERNEL_SPLITK
ADDR = dict(A=0x100000, A2=0x200000, W=0x300000, bias=0x400000, residual=0x500000, rowvec=0x600000, C=0x700000, rot=0x800000,
            ws=0x1000000, colsum=0x900000, colsum_fx=0xA00000, rowstat=0xB00000, ln_rowstat=0xC00000, ln_wsum=0xD00000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


COND_FRAMES = (0, 2)        # config 2 conditions on 2 frames (bench.py's workload); 0: every frame takes the feed-forward


def _walk(B, layout_invariant, cond_frame, Fr=12, H=32):
    """the launches of one evaluation of the full-size engine (SD-v1-5 widths) on the meta device"""
    model = SeerUNet(**dict(synth.SD15_UNET_CFG), layout_invariant=layout_invariant).to("meta")
    rec = RecordingOps(B)
    eng = _Engine(model, ops=rec)
    eng._rotary_table = lambda tb, T: sob.rotary_table(eng.w[tb + ".attn1.rotary_emb.freqs"], T)      # (meta buffers have no values to key on)
    eng._context = lambda c: (torch.empty((B * Fr * 77, 768), dtype=torch.bfloat16, device="meta"), 77)
    # the temporal feed-forward behind conditioning frames runs once per batch element, over that element's later frames: those
    # launches are written down with their own rows, and element 0's only.  (Told apart by their rows: (Fr - cond_frame) frames of a
    # power-of-two level against B * Fr frames of one -- with Fr = 12 only the second is a multiple of 3.)
    assert Fr % 3 == 0 and (cond_frame == 0 or (Fr - cond_frame) % 3 != 0)
    ff, seen = eng._ff, itertools.count()

    def one_element(tb, rows):
        if rows.shape[0] % Fr == 0:
            return ff(tb, rows)
        assert cond_frame > 0 and rows.shape[0] % (Fr - cond_frame) == 0
        rec.element = next(seen) % B        # (the engine's loop goes through the elements in order)
        try:
            return ff(tb, rows)
        finally:
            rec.element = None
    eng._ff = one_element
    x = torch.empty((B, 4, Fr, H, H), device="meta")
    eng.run(x, torch.empty((B,), dtype=torch.long, device="meta"), torch.empty((B, Fr, 77, 768), device="meta"), cond_frame)
    assert next(seen) % B == 0
    return rec


def _klass(g):
    """what the invariant plan may look at, of one recorded launch"""
    return (g["mode"], g["stride"], g["upsample"], g["epilogue"], g["N"], g["K"], g["K1"], g["batch"] > 1, g["splits"], g["a2"],
            g["rotary"], g["colscale"])


PAIRS_ROWS = tuple(r * f for r in (16, 64, 256, 1024) for f in (2, 3, 4))
PAIRS_PLAIN = [(n, k) for n in (320, 640, 960, 1280, 1920, 2560, 3840, 5120) for k in (320, 640, 1280)] + \
              [(320, 1600), (640, 3200), (1280, 6400), (640, 960), (1280, 1920), (1280, 2560)]
PAIRS_CONV = [(n, 9 * c) for n in (320, 640, 1280) for c in (320, 640, 960, 1280, 1920, 2560)]


def _pair_class(mode, n, k):
    return (mode, 1, 0, 0, n, k, k, False, 0, False, False, False)


@pytest.fixture(scope="module")
def classes(monkeypatch_module):
    monkeypatch_module.setattr(real_ops, "device_cus", lambda device=None: 256)
    ks = {_klass(g) for inv in (False, True) for cf in COND_FRAMES for g in _walk(2, inv, cf).gemms}
    # behind conditioning frames the temporal feed-forward leaves its fused and folded forms: these launches are in the grid only
    # because it was walked at cond_frame = 2
    geglu_320 = (_lib.SEER_GEMM_PLAIN, 1, 0, _lib.SEER_EPI_GEGLU, 2560, 320, 320, False, 0, False, False, False)
    assert {_pair_class(_lib.SEER_GEMM_PLAIN, 640, 2560), _pair_class(_lib.SEER_GEMM_PLAIN, 1280, 5120), geglu_320} <= ks
    ks |= {_pair_class(_lib.SEER_GEMM_PLAIN, n, k) for n, k in PAIRS_PLAIN}
    ks |= {_pair_class(_lib.SEER_GEMM_CONV3X3, n, k) for n, k in PAIRS_CONV}
    return sorted(ks)


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _desc(k, M, tile, output="none", rows_pb=None):
    mode, stride, upsample, epi, N, K, K1, batched, splits, a2, rotary, colscale = k
    d = _lib.GemmDesc()
    d.A, d.W, d.C, d.bias = ADDR["A"], ADDR["W"], ADDR["C"], ADDR["bias"]
    d.M, d.N, d.K, d.K1 = M, N, K, K1
    geglu = bool(epi & _lib.SEER_EPI_GEGLU)
    d.lda, d.ldc = K1, (M if epi & _lib.SEER_EPI_TRANS_OUT else (N // 2 if geglu else N))
    if a2:
        d.A2, d.lda2 = ADDR["A2"], K - K1
    d.mode, d.epilogue, d.tile, d.splits = mode, epi, tile, splits
    d.batch = 2 if batched else 1
    if batched:
        d.strideA, d.strideC = M * K, M * N
    if mode == _lib.SEER_GEMM_CONV3X3:
        d.Cin = K // (4 if upsample else 9)
        d.Hin = d.Win = 8 if stride == 2 else 4
        d.Hout = d.Wout = 8 if upsample else 4
        d.stride, d.upsample = stride, upsample
    if rotary:
        d.rot_table, d.rot_tokens_per_batch, d.rot_head_dim, d.rot_dim, d.rot_cols = ADDR["rot"], 16, N // 24, 32, 2 * N // 3
    if colscale:
        d.col_scale, d.col_scale_cols = 0.5, N // 3 // 4 * 4 or 4
    if output == "colsum":
        d.colsum = ADDR["colsum"]
    elif output == "colsum_fx":
        d.colsum_fx, d.colsum_fx_rows, d.colsum_fx_reps = ADDR["colsum_fx"], rows_pb or M, 8
    elif output == "rowstat":
        d.rowstat = ADDR["rowstat"]
    elif output == "ln":
        d.ln_rowstat, d.ln_wsum, d.ln_eps = ADDR["ln_rowstat"], ADDR["ln_wsum"], 1e-5
    return d


def _plan(lib, d):
    """(status, kernel, tile, K slices, reduce) of `d` given exactly the workspace the size query asks for, and that size"""
    ws = lib.seer_gemm_workspace_bytes(C.byref(d))
    if ws > 0:
        d.workspace, d.workspace_bytes = ADDR["ws"], ws
    out = (C.c_int32 * 5)()
    assert lib.seer_gemm_plan(C.byref(d), out) == 0
    return tuple(out), ws


def test_the_request_is_new_and_documented(lib):
    header = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "seer_hip.h").read_text()
    assert "#define SEER_TILE_AUTO_INVARIANT 23" in header and INV == 23
    # a tile code nobody defines is still refused
    d = _desc(_pair_class(_lib.SEER_GEMM_PLAIN, 1280, 1280), 768, 24)
    assert _plan(lib, d)[0][0] == -22
    assert _plan(lib, _desc(_pair_class(_lib.SEER_GEMM_PLAIN, 1280, 1280), 768, INV))[0][0] == 0


def test_the_plan_and_the_queries_do_not_move_with_the_rows(lib, classes):
    n_ok = n_split = n_refused = 0
    kernels, tiles = set(), set()
    for k, output in itertools.product(classes, OUTPUTS):
        # accumulated sums: a partial must not straddle two batch elements, so an element has to be whole row blocks (96- and
        # 128-row tiles, 32-row strips of the reduce pass): those descriptors are asked at the M that 384 divides
        ms = [m for m in MS if m % 384 == 0] if output == "colsum_fx" else MS
        plans, feats = [], []
        for M in ms:
            d = _desc(k, M, INV, output)
            plan, ws = _plan(lib, d)
            status, kernel, tile, splits, reduce = plan
            if status == 0:
                assert kernel in (K_TILE, K_SPLITK), (k, output, M, plan)
                assert lib.seer_gemm_sync_bytes(C.byref(d)) == 0
                assert ws == (splits * M * k[4] * 4 if splits > 1 else 0), (k, output, M, plan, ws)
                assert (kernel == K_SPLITK) == (splits > 1)
            plans.append(plan)
            # the four feature queries, asked of the launch without the optional output (they add their own)
            q = _desc(k, M, INV)
            q.workspace, q.workspace_bytes = ADDR["ws"], 1 << 40
            ln = _desc(k, M, INV, "ln")
            reps = C.c_int32(0)
            fx = lib.seer_gemm_colsum_fx_layout(C.byref(q), M, C.byref(reps))
            feats.append((lib.seer_gemm_colsum_rows(C.byref(q)), lib.seer_gemm_rowstat_ok(C.byref(q)), lib.seer_gemm_lnfold_ok(C.byref(ln)),
                          fx if M % 384 == 0 else None))
        assert len(set(plans)) == 1, (k, output, dict(zip(ms, plans)))
        assert len({f[:3] for f in feats}) == 1, (k, output, dict(zip(ms, feats)))
        # the row block of the accumulated sums is one number per plan; an element it does not divide is refused (0)
        assert len({f[3] for f in feats if f[3] is not None}) == 1, (k, output, dict(zip(ms, feats)))
        if plans[0][0] == 0:
            n_ok += 1
            n_split += plans[0][1] == K_SPLITK
            kernels.add(plans[0][1]); tiles.add(plans[0][2])
        else:
            n_refused += 1
    print(f"{len(classes)} classes x {len(OUTPUTS)} outputs: {n_ok} planned ({n_split} with K slices), {n_refused} refused at every M; "
          f"tiles {sorted(tiles)}")
    assert kernels == {K_TILE, K_SPLITK} and n_split >= 10 and len(tiles) >= 5


def test_k_slices_without_their_workspace_are_an_error_not_an_unsplit_launch(lib):
    k = _pair_class(_lib.SEER_GEMM_CONV3X3, 1280, 11520)
    out = (C.c_int32 * 5)()
    for M in (48, 384, 1536):
        d = _desc(k, M, INV)
        need = lib.seer_gemm_workspace_bytes(C.byref(d))
        assert need > 0
        assert lib.seer_gemm_plan(C.byref(d), out) == 0 and out[0] == -22            # no workspace
        d.workspace, d.workspace_bytes = ADDR["ws"], need - 4
        assert lib.seer_gemm_plan(C.byref(d), out) == 0 and out[0] == -22            # too small
        d.workspace_bytes = need
        assert lib.seer_gemm_plan(C.byref(d), out) == 0 and out[0] == 0 and out[1] == K_SPLITK
        # the default request, same descriptor, no workspace: planned, unsplit
        e = _desc(k, M, AUTO)
        assert lib.seer_gemm_plan(C.byref(e), out) == 0 and out[0] == 0 and out[1] == K_TILE


def test_the_default_request_does_move_with_the_rows(lib):
    """non-vacuity: on the 576-pair grid AUTO plans M rows and 2 M rows differently for many pairs (197 when this was written)"""
    moved = 0
    for mode, pairs in ((_lib.SEER_GEMM_PLAIN, PAIRS_PLAIN), (_lib.SEER_GEMM_CONV3X3, PAIRS_CONV)):
        for (n, kk), rows in itertools.product(pairs, PAIRS_ROWS):
            k = _pair_class(mode, n, kk)
            a, b = _plan(lib, _desc(k, rows, AUTO))[0], _plan(lib, _desc(k, 2 * rows, AUTO))[0]
            i, j = _plan(lib, _desc(k, rows, INV))[0], _plan(lib, _desc(k, 2 * rows, INV))[0]
            assert i == j and i[0] == 0, (k, rows, i, j)
            moved += a != b
    n = (len(PAIRS_PLAIN) + len(PAIRS_CONV)) * len(PAIRS_ROWS)
    print(f"AUTO: {moved} of {n} (rows, N, K) pairs planned differently for M and 2 M rows")
    assert n == 576 and moved >= 50
    # the GEGLU projection of the 32x32 level: AUTO folds its LayerNorm at 768 and 4096 rows and not from 8192 up; the invariant
    # request folds at every M
    gk = (_lib.SEER_GEMM_PLAIN, 1, 0, _lib.SEER_EPI_GEGLU, 2560, 320, 320, False, 0, False, False, False)
    assert [lib.seer_gemm_lnfold_ok(C.byref(_desc(gk, m, AUTO, "ln"))) for m in (768, 4096, 8192, 24576)] == [1, 1, 0, 0]
    assert [lib.seer_gemm_lnfold_ok(C.byref(_desc(gk, m, INV, "ln"))) for m in (768, 4096, 8192, 24576)] == [1, 1, 1, 1]


def _element0(rec):
    """the launch sequence as batch element 0 sees it: ops, per-element rows, tile request and everything else that selects a kernel"""
    return rec.calls


@pytest.mark.parametrize("cond_frame", COND_FRAMES)
def test_the_engine_walk_of_one_element_is_the_same_for_any_batch_and_device(monkeypatch, cond_frame):
    walks = {}
    for cus, B in itertools.product((32, 256), (1, 2)):
        monkeypatch.setattr(real_ops, "device_cus", lambda device=None, cus=cus: cus)
        walks[("inv", cus, B)] = _walk(B, True, cond_frame)
        walks[("default", cus, B)] = _walk(B, False, cond_frame)
    inv = [_element0(walks[("inv", c, b)]) for c in (32, 256) for b in (1, 2)]
    assert all(s == inv[0] for s in inv[1:]), next((x, y) for s in inv[1:] for x, y in zip(inv[0], s) if x != y)
    assert len(inv[0]) > 400
    # every launch of the GEMM family carries the invariant request; without the switch none does
    for key, rec in walks.items():
        want = INV if key[0] == "inv" else AUTO
        assert rec.gemms and all(g["tile"] == want for g in rec.gemms), key
        assert not any(g["colsum"] or g["colsum_fx"] for g in rec.gemms) or key[0] == "default"
    # the row-owner launches of the 320-channel level run in every invariant walk (12 288 rows per element)
    assert {"ff_fused", "rowchain", "groupnorm_stats_fx"} <= {c[0] for c in inv[0]}
    if cond_frame:
        # the temporal feed-forward of one element: its own launches over the 10 later frames, LayerNorm launched, GEGLU unfolded
        per_element = [c for c in inv[0] if c[0] == "gemm" and c[1] in (10 * 1024, 10 * 256, 10 * 64, 10 * 16)]
        assert len(per_element) >= 2 * 8 and any(dict(c[2])["epilogue"] & _lib.SEER_EPI_GEGLU and not dict(c[2])["ln"] for c in per_element)
    # non-vacuity: the default engine's walk of one element does change with the batch and with the device
    dflt = {k: _element0(v) for k, v in walks.items() if k[0] == "default"}
    assert dflt[("default", 256, 1)] != dflt[("default", 256, 2)]
    assert dflt[("default", 32, 1)] != dflt[("default", 256, 1)]       # (12 288 rows: the chain in front of q|k|v needs one round of the chip)


def test_a_clip_sharded_too_finely_is_refused_from_the_shard_table():
    """the GroupNorm -> q|k|v launch needs 96 rows of a batch element on every rank.  Whether the smallest shard has them is read from
    the shard table that every rank holds: a rank with enough rows of its own refuses too, before any exchange."""
    from types import SimpleNamespace
    model = SeerUNet(**dict(synth.SD15_UNET_CFG), layout_invariant=True).to("meta")
    eng = _Engine(model, ops=RecordingOps(1))
    # 64 rows per frame; this rank holds 2 frames (128 rows), the last rank 1 (64 rows); 9 280 rows over the clip: the launch pays
    # The refusal comes while the evaluation's plan is made (unet._LaunchPlan: B = 1, the rank's 2 frames of 8 x 8), before any launch.
    shard = dict(local_frames=2, exact_stats=True, local_cond_frames=lambda cond_frame: cond_frame)
    eng.shard = SimpleNamespace(total_frames=145, frame_counts=[2] * 72 + [1], **shard)
    with pytest.raises(RuntimeError, match="fewer frame shards"):
        _LaunchPlan(eng, 1, 2, 8, 8, 0)
    assert eng.ops.calls == []
    eng.shard = SimpleNamespace(total_frames=146, frame_counts=[2] * 73, **shard)
    plan = _LaunchPlan(eng, 1, 2, 8, 8, 0)
    assert plan.runs("chain", 320, 2 * 64) is True
    assert plan.runs("chain", 640, 2 * 64) is False
