"""The constructions of tests/test_gpu_fused320_matrix.py must be able to FAIL.  Here, without a GPU, the float64 emulation of
tests/fused320_ref.py stands in for the kernels:

1. every Part 1 precondition holds on the reference alone (fused320_ref.rowchain / ff with exact=True assert them while they compute:
   partial sums below 2^24, every value rounded at an inexact spot within 2^-12 of a non-zero representable number, also with rstd
   moved by +-4 ulp in float32), the stores round a meaningful share of their elements, and the unmutated emulation -- which evaluates
   the kernels' own formulas, rsqrt(var + eps) and the erf GELU included -- gives the expected bits;
2. the index formulas of the three pack orders are permutations of their matrices;
3. the mutation table: every mutation of fused320_ref.MUTATIONS applied to the emulation changes a bit of a stored tensor in every
   Part 1 case it applies to, and pushes the worst row of every Part 2 case it applies to past 2x the unmutated emulation's.  For
   contrast the table prints what the older whole-tensor metric (relative L2 over the tensor: < 8e-3 bf16 / 1.2e-3 fp16 in
   test_gpu_rowchain.py, < 4e-3 / 6e-4 in test_ff_fused_c320*) reads on the same Part 2 case: "old passes" counts the cases it lets through.
   colsum_segment_to_first changes the column sums only: Part 1 holds their only assertions (they are exact), Part 2 has none.

The printed table (pytest -s) is copied into profiles/fused320_matrix.md."""
import pytest
import torch

from tests import fused320_ref as R

f16, bf16, f64 = torch.float16, torch.bfloat16, torch.float64
DEV = torch.device("cpu")
DTS = [pytest.param(bf16, id="bf16"), pytest.param(f16, id="f16")]
OLD_RC = {bf16: 8e-3, f16: 1.2e-3}          # tests/test_gpu_rowchain.py: _rel < tol
OLD_FF = {bf16: 4e-3, f16: 6e-4}            # tests/test_gpu_kernels.py::test_ff_fused_c320*: rel < tol


def _name(dt):
    return "f16" if dt == f16 else "bf16"


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _stored(spec, r):
    """the tensors a case stores"""
    return ([r["h"]] if spec["h_out"] else []) + ([r["out"]] if r["out"] is not None else [])


@pytest.mark.parametrize("dt", DTS)
def test_rowchain_preconditions_and_identity(dt):
    for spec in R.ROWCHAIN_EXACT:
        p = R.exact_rowchain(spec, dt, DEV)
        want = R.rowchain(p, dt, exact=True)
        share = R.rounded_share(want["out_pre"] if want["out"] is not None else want["h_pre"], dt)      # the FINAL store of the case
        assert share > 0.1, (R.rowchain_id(spec), share)
        emu = R.rowchain(p, dt)
        for a, b in zip(_stored(spec, emu), _stored(spec, want)):
            assert torch.equal(a, b), f"{R.rowchain_id(spec)}: the emulation (rsqrt(var + eps) and all) does not give the expected bits"
    assert len(R.ROWCHAIN_EXACT) >= 40


@pytest.mark.parametrize("dt", DTS)
def test_ff_preconditions_and_identity(dt):
    for M, pre, alias, colsum in R.FF_EXACT:
        small = colsum is not None
        p = R.exact_ff(dict(M=M, pre=pre, small=small), dt, DEV)
        info = {}
        want = R.ff(p, dt, exact=True, info=info)
        if small:
            assert float(want.abs().max()) <= 256 and bool((want == want.round()).all())
            if isinstance(colsum, tuple):
                fx = R.colsums_fx(want, colsum[1], colsum[2])
                yb = want.reshape(M // colsum[1], colsum[1], R.C)
                assert torch.equal(fx.sum(0)[:, 0], (yb.sum(1) * 2 ** 20).to(torch.int64)) and torch.equal(fx.sum(0)[:, 1], (yb.pow(2).sum(1) * 2 ** 20).to(torch.int64))
                assert float(yb.pow(2).sum(1).max()) < 2 ** 24
        else:
            assert R.rounded_share(info["y_pre"], dt) > 0.3
        assert torch.equal(R.ff(p, dt), want), f"ff M{M} pre{pre}: the emulation (erf GELU and all) does not give the expected bits"


def test_a_zero_is_not_absorbed():
    """the trap the constructions avoid: an exact LayerNorm value of 0 comes out as ~1e-5, and the precondition says so"""
    h = R.balanced_rows(4, DEV, 1)
    gamma, beta = torch.ones(R.C, dtype=f64), torch.ones(R.C, dtype=f64)      # |beta| = |gamma|: h = -1 gives 0
    with pytest.raises(AssertionError, match="exact value of 0"):
        R.assert_absorbed(h, torch.full((4, 1), (1 + 1e-5) ** -0.5, dtype=f64).expand(4, R.C), gamma.expand(4, R.C), beta.expand(4, R.C),
                          h * gamma + beta, bf16, "LN")


def test_pack_orders_are_permutations():
    for (row, col), shape in ((R.rowchain_pack_index(3, DEV), (960, 320)), (R.ff_pack_w1_index(DEV), (2560, 320)),
                              (R.ff_pack_wcat_index(DEV), (320, 1600))):
        flat = row * shape[1] + col
        assert flat.numel() == shape[0] * shape[1] and flat.unique().numel() == flat.numel() and int(row.max()) == shape[0] - 1
    order = R.geglu_interleave_order(DEV)
    assert order.unique().numel() == 2 * R.INNER and order[:16].tolist() == list(range(16)) and order[16:32].tolist() == list(range(1280, 1296))


@pytest.mark.parametrize("dt", DTS)
def test_part1_mutations(dt):
    table = {m: [0, 0] for m in R.MUTATIONS}
    fails = []
    for spec in R.ROWCHAIN_EXACT:
        p = R.exact_rowchain(spec, dt, DEV)
        want = R.rowchain(p, dt, exact=True)
        for mut in R.MUTATIONS:
            r = R.rowchain(p, dt, mut=mut)
            if r is None:
                continue
            seen = any(not torch.equal(a, b) for a, b in zip(_stored(spec, r), _stored(spec, want)))
            table[mut][0] += 1
            table[mut][1] += seen
            if not seen:
                fails.append(f"{R.rowchain_id(spec)}: {mut} leaves every stored bit in place")
    for M, pre, alias, colsum in R.FF_EXACT:
        p = R.exact_ff(dict(M=M, pre=pre, small=colsum is not None), dt, DEV)
        want = R.ff(p, dt, exact=True)
        for mut in R.MUTATIONS:
            if mut == "colsum_segment_to_first":
                if not isinstance(colsum, tuple):
                    continue
                fx = R.colsums_fx(want, colsum[1], colsum[2], mut=mut)
                if fx is None:
                    continue
                seen = not torch.equal(fx, R.colsums_fx(want, colsum[1], colsum[2]))
            else:
                y = R.ff(p, dt, mut=mut)
                if y is None:
                    continue
                seen = not torch.equal(y, want)
            table[mut][0] += 1
            table[mut][1] += seen
            if not seen:
                fails.append(f"ff M{M} pre{pre} {colsum}: {mut} leaves every stored bit in place")
    for mut, (n, hit) in table.items():
        print(f"fused320_matrix mutations | part 1 | {_name(dt)} | {mut} | applicable {n} | seen {hit}")
        assert n > 0, f"{mut}: applicable nowhere"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dt", DTS)
def test_part2_mutations(dt):
    table = {m: [0, 0, float("inf"), 0.0, 0, float("inf")] for m in R.MUTATIONS}      # applicable, past 2x, min ratio, max ratio, old passes, smallest old reading
    fails = []

    def note(mut, ratio, old, old_tol, what):
        t = table[mut]
        t[0] += 1
        t[1] += ratio > 2
        t[2], t[3] = min(t[2], ratio), max(t[3], ratio)
        t[4] += old < old_tol
        t[5] = min(t[5], old)
        if not ratio > 2:
            fails.append(f"{what}: {mut} ratio {ratio:.3g}")

    for amp in (1.0, 4.0):
        for gn, M, res, off in R.ROWCHAIN_ROWS:
            p = R.rows_rowchain_problem(dt, DEV, gn, M, res, off or 0, amp, table_rows=M + (off or 0))
            ref, emu = R.rowchain(p), R.rowchain(p, dt)
            floors = {k: R.row_floor(ref[k]) for k in ("h", "out")}
            e0 = {k: R.row_err(emu[k], ref[k], floors[k]) for k in ("h", "out")}
            for mut in R.MUTATIONS:
                r = R.rowchain(p, dt, mut=mut)
                if r is None:
                    continue
                ratio = max(R.row_err(r[k], ref[k], floors[k]) / e0[k] for k in ("h", "out"))
                old = max(_rel(r[k], ref[k]) for k in ("h", "out"))
                note(mut, ratio, old, OLD_RC[dt], f"rowchain {gn} M{M} x{amp:g}")
        for M, pre in R.FF_ROWS:
            p = R.random_ff(dt, DEV, M=M, pre=pre, amp=amp, B=3 if M == 336 else 1, seed=int(amp) * 100 + M)
            ref, emu = R.ff(p), R.ff(p, dt)
            floor = R.row_floor(ref)
            e0 = R.row_err(emu, ref, floor)
            for mut in R.MUTATIONS:
                y = R.ff(p, dt, mut=mut)
                if y is None:
                    continue
                note(mut, R.row_err(y, ref, floor) / e0, _rel(y, ref), OLD_FF[dt], f"ff M{M} pre{pre} x{amp:g}")
    for mut, (n, hit, lo, hi, old_pass, old_max) in table.items():
        if mut == "colsum_segment_to_first":
            print(f"fused320_matrix mutations | part 2 | {_name(dt)} | {mut} | no column-sum assertion in Part 2 (exact in Part 1)")
            continue
        print(f"fused320_matrix mutations | part 2 | {_name(dt)} | {mut} | applicable {n} | past 2x {hit} | ratio {lo:.3g} .. {hi:.3g} | "
              f"old passes {old_pass} | old reads from {old_max:.3g}")
        assert n > 0, f"{mut}: applicable nowhere"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dt", DTS)
def test_old_data_contrast(dt):
    """the hole the issue names first, on the older test's own data: every batch element drawn from ONE distribution (N(0.3, 1.5^2),
    B = 3, 1000 rows each, tests/test_gpu_rowchain.py).  Foreign statistics then move the rows behind a boundary by about 1 %: the
    whole-tensor metric reads far below its tolerance, the worst own row is tens of times the emulation's"""
    B, rows_pb = 3, 1000
    p = R.random_rowchain(dt, DEV, M=B * rows_pb, gn=("stats", B, rows_pb, 32, 1), n2=3, same_dist=True, seed=5)
    ref, emu = R.rowchain(p), R.rowchain(p, dt)
    for mut in ("gn_first_batch", "gn_group_plus1"):
        r = R.rowchain(p, dt, mut=mut)
        ratio = max(R.row_err(r[k], ref[k], R.row_floor(ref[k])) / R.row_err(emu[k], ref[k], R.row_floor(ref[k])) for k in ("h", "out"))
        old = max(_rel(r[k], ref[k]) for k in ("h", "out"))
        print(f"fused320_matrix mutations | old data | {_name(dt)} | {mut} | worst row / emulation {ratio:.3g} | old metric reads {old:.3g} "
              f"against {OLD_RC[dt]:g}: {'passes (a miss)' if old < OLD_RC[dt] else 'fails'}")
        assert ratio > 2


@pytest.mark.parametrize("dt", DTS)
def test_fx_stats_yardstick_samples_flips(dt):
    """the allowance of test_rows_gn_fx_against_gn_stats is not zero: moving the fp32 statistics by an ulp does flip roundings somewhere
    in the cases of either storage type, and stays far below one row's whole rounding error against float64 times ten"""
    y = R.fx_stats_yardstick(dt, DEV)
    print(f"fused320_matrix fx-vs-stats yardstick | {_name(dt)} | h {y['h']:.4g} | out {y['out']:.4g}")
    assert 0 < y["h"] < 2e-2 and 0 < y["out"] < 2e-2
