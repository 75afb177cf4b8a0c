"""The constructions of tests/test_gpu_t320_matrix.py must be able to FAIL.  Here, without a GPU, the float64 references of
tests/t320_ref.py stand in for the 256 x 320 tile kernel:

1. every Part 1 case meets its preconditions on the reference alone: partial sums below 2^24, |C| < 60 000, the rounding cases round
   more than half of their elements, the column-sum cases stay within 256, the GEGLU gates are 0 or integers 8 .. 64; the spelled-out
   implicit GEMM agrees with F.conv2d; the planned slice counts are the intended ones;
2. the mutation table: each of t320_ref.MUTATIONS applied to the reference of one Part 1 (or Part 2) case is rejected by the new
   criterion -- a differing bit in Part 1, a worst row past 2x the once-rounded emulation's in Part 2.  For contrast the table prints
   what the older criterion (tests/test_gpu_t320.py::_close, atol = rtol = 2e-2) reads on that test's N(0, 1) data at the same shape;
   which mutations it lets through is recorded, not asserted.

The printed table (pytest -s) is copied into profiles/t320_matrix.md."""
import pytest
import torch
import torch.nn.functional as Fn

from tests import t320_ref as R

f64 = torch.float64
DEV = torch.device("cpu")


def _same(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def test_part1_preconditions():
    for spec in R.GEMM_EXACT + R.GEGLU_EXACT:
        p = R.exact_gemm(spec, DEV)
        r = R.gemm(p, exact=True)
        assert float(r["pre"].abs().max()) < 60000, R.case_id(spec)
        assert torch.equal(r["pre"].to(torch.float32).to(f64), r["pre"]), f"{R.case_id(spec)}: not exact in fp32"
        if spec.get("big"):
            assert float((r["out"] != r["pre"]).double().mean()) > 0.5, f"{R.case_id(spec)}: the store must round most elements"
    for spec in R.CONV_EXACT + R.UP_EXACT:
        r = R.conv(R.exact_conv(spec, DEV), exact=True)
        assert float(r["pre"].abs().max()) < 60000, R.case_id(spec)
    assert [R.planned_slices(K, S) for S, K in ((2, 512), (3, 768), (7, 1792), (16, 4096), (16, 1024), (2, 576), (3, 576), (2, 320))] == [2, 3, 7, 16, 4, 2, 2, 1]


def test_gather_is_the_conv():
    for spec in (R.CONV_EXACT[0], R.CONV_EXACT[10], R.CONV_EXACT[18]):
        p = R.exact_conv(spec, DEV)
        got = R.conv_gather(p["x"], p["w"], p["stride"], p["pad_after"])
        assert torch.equal(got, R.conv(p)["pre"]), R.case_id(spec)
    # the phase rows are a permutation of the output rows, phase z = 2 a + b at pixel (2 y + a, 2 x + b)
    rows = R.phase_rows(2, 3, 5, DEV)
    assert rows.reshape(-1).unique().numel() == 2 * 4 * 15 and int(rows[3, 0]) == 10 + 1 and int(rows[1, 1]) == 3


def test_colsum_layouts():
    y = R._ints((512, 320), DEV, 1, -9, 9)
    t = R.colsum_tiles(y, 64)
    assert t.shape == (1, 8, 320, 2) and torch.equal(t[0, 3, :, 0], y[192:256].sum(0)) and torch.equal(t[0, 3, :, 1], y[192:256].pow(2).sum(0))
    fx = R.colsum_fx(y, 16, 256, 3)
    assert fx.shape == (3, 2, 2, 320) and torch.equal(fx.sum(0)[1, 0], (y[256:].sum(0) * 2 ** 20).to(torch.int64))
    assert torch.equal(fx[1, 0, 1], (sum(y[16 * i:16 * i + 16].pow(2).sum(0) for i in range(1, 16, 3)) * 2 ** 20).to(torch.int64))


def _find(table, **want):
    hits = [s for s in table if all(s.get(k) == v for k, v in want.items()) and all(k in want or not s.get(k) for k in ("bias", "rpb", "cs", "res", "rot", "k1"))]
    assert hits, want
    return hits[0]


def _with_a2_buffers(p, gapped):
    """a2 as a view of a buffer, for a2_read_with_lda: row stride K2 + 24 behind a column offset of 8 next to lda = K1 + 16 (the gapped
    views of the GPU file), or both dense (the older test)"""
    a2 = p["a2"]
    M, K2 = a2.shape
    if gapped:
        buf = torch.full((M + 1, K2 + 24), float("nan"), dtype=f64)
        buf[:M, 8:8 + K2] = a2
        p.update(a2_buf=buf, a2_off=8, lda=p["a"].shape[1] + 16)
    else:
        p.update(a2_buf=a2, a2_off=0, lda=p["a"].shape[1])
    return p


# mutation -> (kind, the Part 1 case it is applied to)
_CASES = {
    "drop_kstep_one_wave": ("gemm", dict(M=256, N=320, K=3136)),
    "residual_row_clamped": ("gemm", dict(M=480, N=640, K=512, splits=1, res="lds")),
    "slice_last_twice": ("gemm", dict(M=300, N=320, K=1792, splits=7, bias=True, res="lds")),
    "slice0_skipped": ("gemm", dict(M=300, N=320, K=1792, splits=7, bias=True, res="lds")),
    "rowvec_batch_per_wave_tile": ("gemm", dict(M=480, N=640, K=512, splits=1, rpb=96)),
    "rot_no_modulo": ("gemm", dict(M=480, N=960, K=512, splits=1, rot=(40, 32, 96, 16, 640), cs=320)),
    "colscale_whole_fragment": ("gemm", dict(M=480, N=640, K=512, splits=1, cs=164)),
    "value_gate_exchanged_16": ("geglu", dict(M=300, N=640, K=64)),
    "pad_after_border_valid": ("conv", dict(n=3, H=16, W=24, stride=2, pad_after=True, splits=1)),
    "phases_swapped": ("up", dict(n=3, H=6, W=10, Co=320)),
    "a2_read_with_lda": ("gemm", dict(M=256, N=320, K=256, k1=192)),
    "truncating_stores": ("gemm", dict(M=300, N=320, K=768, big=True, splits=1)),
    "tile_twice_one_missing": ("gemm", dict(M=2100, N=640, K=64)),
}


def test_mutation_table():
    assert sorted(_CASES) == sorted(R.MUTATIONS) and len(R.MUTATIONS) == 13
    missed = []
    for mut in R.MUTATIONS:
        kind, want = _CASES[mut]
        if kind in ("gemm", "geglu"):
            spec = [s for s in (R.GEGLU_EXACT if kind == "geglu" else R.GEMM_EXACT) if all(s.get(k) == v for k, v in want.items())
                    and (kind == "geglu" or set(k for k in ("bias", "rpb", "cs", "res", "rot", "k1", "big") if s.get(k)) == set(want) - {"M", "N", "K", "splits"})][0]
            p = R.exact_gemm(spec, DEV)
            if p.get("a2") is not None:
                _with_a2_buffers(p, gapped=True)
            good, bad = R.gemm(p, exact=True), R.gemm(p, mut=mut)
            terms = {k: spec[k] for k in ("bias", "rpb", "cs", "res", "rot", "k1", "geglu") if spec.get(k)}
            po = R.old_problem(spec["M"], spec["N"], spec["K"], DEV, seed=7, S=p["S"], **terms)
            if po.get("a2") is not None:
                _with_a2_buffers(po, gapped=False)
            po["prefill"] = 0.0
            ref_o, bad_o = R.gemm(po), R.gemm(po, mut=mut)
        else:
            spec = [s for s in (R.UP_EXACT if kind == "up" else R.CONV_EXACT) if all(s.get(k) == v for k, v in want.items())][0]
            p = R.exact_conv(spec, DEV)
            good, bad = R.conv(p, exact=True), R.conv(p, mut=mut)
            po = R.old_conv_problem(spec["n"], spec["H"], spec["W"], spec["Ci"], spec["Co"], DEV, seed=7, stride=spec.get("stride", 1),
                                    pad_after=spec.get("pad_after", False), up=spec.get("up", False))
            ref_o, bad_o = R.conv(po), R.conv(po, mut=mut)
        assert bad is not None and bad_o is not None, f"{mut}: does not apply to its case {R.case_id(spec)}"
        seen = not _same(bad["out"], good["out"])
        differ = int(((bad["out"] != good["out"]) & ~(bad["out"].isnan() & good["out"].isnan())).sum())
        ok_old, reading = R.old_close(bad_o["out"], ref_o["pre"])
        base_old = R.old_close(ref_o["out"], ref_o["pre"])[1]
        print(f"t320_matrix mutations | part 1 | {mut} | {R.case_id(spec)} | new: {differ}/{good['out'].numel()} elements differ | "
              f"old criterion reads {reading:.3g} of its bound (unmutated {base_old:.3g}): {'PASSES, a miss' if ok_old else 'fails'}")
        if not seen:
            missed.append(mut)
    assert not missed, f"the exact criterion lets through: {missed}"


@pytest.mark.parametrize("mut,kind", [("value_gate_exchanged_16", "geglu"), ("rot_no_modulo", "rotary"), ("drop_kstep_one_wave", "geglu"),
                                      ("drop_kstep_one_wave", "rotary"), ("truncating_stores", "rotary")])
def test_part2_mutations(mut, kind):
    """the per-row criterion on the two places integers cannot reach"""
    for k, M, amp in R.ROWS_CASES:
        if k != kind:
            continue
        p = R.random_problem(kind, M, amp, DEV)
        ref = R.gemm(p)
        bad = R.gemm(p, mut=mut)
        floor = R.row_floor(ref["pre"])
        e0, e1 = R.row_err(ref["out"], ref["pre"], floor), R.row_err(bad["out"], ref["pre"], floor)
        ok_old, reading = R.old_close(bad["out"], ref["pre"])
        print(f"t320_matrix mutations | part 2 | {mut} | {kind} M{M} x{amp:g} | worst row {e1:.4g} against the emulation's {e0:.4g}: ratio {e1 / e0:.3g} | "
              f"old criterion reads {reading:.3g} of its bound: {'PASSES, a miss' if ok_old else 'fails'}")
        if mut != "truncating_stores":       # (a truncating store doubles the rounding error at most: Part 1's rounding cases pin it, not the rows)
            assert e1 > 2 * e0, (mut, kind, M, amp, e1, e0)


def test_unmutated_reference_is_the_operator():
    """the references against independent spellings: F.linear in float64, the GEGLU of attention.py on the interleaved rows, and the
    rotation written out for one element"""
    spec = _find(R.GEMM_EXACT, M=480, N=640, K=512, splits=1, bias=True, rpb=96, cs=484, res="lds")
    p = R.exact_gemm(spec, DEV)
    want = Fn.linear(p["a"], p["w"], p["bias"]) + p["rowvec"].repeat_interleave(96, 0)
    want[:, :484] *= 0.5
    assert torch.equal(R.gemm(p)["pre"], want + p["res"])
    p = R.exact_gemm(R.GEGLU_EXACT[0], DEV)
    order = R.interleave_order(320, DEV)
    h = Fn.linear(p["a"], p["w"][order], p["bias"][order]).reshape(300, 20, 2, 16)
    assert torch.equal(R.gemm(p, exact=True)["pre"], (h[:, :, 0] * h[:, :, 1]).reshape(300, 320))
    spec = _find(R.GEMM_EXACT, M=480, N=960, K=512, splits=1, rot=(80, 32, 96, 16, 640), cs=320)
    p = R.exact_gemm(spec, DEV)
    acc = p["a"] @ p["w"].t()
    m, n = 250, 320 + 80 * 2 + 6                                          # k block, head 2, pair 3
    c, s = p["rot"]["table"][m % 96 + 16, 3].to(f64)
    got = R.gemm(p)["pre"]
    assert got[m, n] == acc[m, n] * c - acc[m, n + 1] * s and got[m, n + 1] == acc[m, n + 1] * c + acc[m, n] * s
    assert got[m, 80 * 2 + 6] == (acc[m, 166] * c - acc[m, 167] * s) * 0.5 and got[m, 640 + 5] == acc[m, 645] and got[m, 320 + 40] == acc[m, 360]
