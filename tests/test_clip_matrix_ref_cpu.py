"""The constructions of tests/test_gpu_clip_matrix.py must be able to FAIL.  Here, without a GPU, the float64 emulation of
tests/clip_matrix_ref.py stands in for seer_attn_causal64:

1. every Part 1 precondition holds on the reference alone (the constructions assert them while they build: Q, K, V and the expected O
   exact in bf16, the score an integer below 2^24, two keys never holding the same V inside a 16-column tile, "a level column moves
   after rounding when n is off by one"); the unmutated emulation AND the fp32 oracle of the older tests
   (clip_oracle.attn_causal64_ref) give the expected O bit for bit in every run of every case; over the cases every key position is
   selected, ties occur, queries that see nothing come out as zeros and their neighbours do not;
2. the mutation table: every mutation of clip_matrix_ref.MUTATIONS applied to the emulation is caught by at least one part -- Part 1 when
   a (sample, head, query) row of a run is not the expected bits or not finite (the sentinel layout's assertion: a read of the NaN guard
   row), Part 2 when the worst own row exceeds 2x the unmutated emulation's.  The two numeric-only mutations (the denominator from the
   rounded P, P not rounded) are reported with their measured ratios, whatever they are.

The printed tables are copied into profiles/clip_matrix.md."""
import pytest
import torch

from tests import clip_matrix_ref as R
from tests import clip_oracle as CO
from tests.test_gpu_train_matrix import _row_err

bf16, f64 = torch.bfloat16, torch.float64
CASES = [(L, kind, b, h) for L in R.LENGTHS for kind in R.MASKS for b, h in R.layouts(L, kind)]


def test_masks_restate_the_older_kinds():
    from tests.test_gpu_clip_text import _mask
    for L in (1, 16, 17, 77, 128):
        for kind in ("null", "ones", "len1", "len20", "holes", "zero"):
            a, b = R.mask(kind, 2, L), _mask(kind, 2, L)
            assert (a is None and b is None) or torch.equal(a, b), (kind, L)
    m = R.mask("last", 3, 77)
    assert int((m == 0).sum()) == 3 and bool((m[:, 76] == 0).all())
    m = R.mask("tile", 3, 77)
    assert all(int((m[b] == 0).sum()) in (13, 16) and bool((m[b, 16 * ((b + 1) % 5):16 * ((b + 1) % 5) + 16] == 0).all()) for b in range(3))
    m = R.mask("even", 3, 97)                              # 7 tiles: pairs 0, 1, 2 have an odd tile
    assert all(bool((m[b, 32 * b:32 * b + 16] == 0).all()) and bool((m[b, 32 * b + 16:32 * b + 32] == 1).all()) for b in range(3))
    assert {lay for L in R.LENGTHS for lay in R.layouts(L, "null")} == {(1, 1), (2, 2), (3, 3), (1, 12)}
    assert all({R.layouts(L, k)[0] for k in R.MASKS} == set(R.LAYOUTS) for L in R.LENGTHS)


@pytest.mark.parametrize("L", R.LENGTHS)
def test_part1_identity_and_fp32_oracle(L):
    """the expected bits of every run, from the emulation and from clip_oracle.attn_causal64_ref in fp32 (with and without its P
    rounding: P is 0, 1/2 or 1); the coverage the issue asks of the targets"""
    ties = zero_rows = 0
    for kind in R.MASKS:
        for batch, heads in R.layouts(L, kind):
            vis = R.visible(R.mask(kind, batch, L), batch, L)
            for name, q4, k4, v4, want4, m in R.exact_runs(L, kind, batch, heads):
                what = f"L{L} {kind} b{batch} h{heads} {name}"
                r = R.emulate(q4, k4, v4, m)
                assert R.bad_rows(r.o, want4) == 0, f"{what}: the emulation does not give the expected O"
                q2, k2, v2 = (R.to2(t).to(bf16) for t in (q4, k4, v4))
                for round_p in (True, False):
                    o = CO.attn_causal64_ref(q2, k2, v2, batch=batch, heads=heads, L=L, key_mask=m, round_p=round_p)
                    assert torch.equal(o.to(bf16), R.to2(want4).to(bf16)), f"{what}: the fp32 oracle does not give the expected O"
                none = ~vis.any(-1)                                                     # [batch, L]
                zero_rows += int(none.sum())
                w = want4.transpose(1, 2)                                               # [batch, L, heads, 64]
                assert bool((w[none] == 0).all())
                if name == "uniform":
                    assert bool((w[~none].abs().sum(-1) > 0).all()), f"{what}: a query that sees a key expects zeros"
                if name == "selector ties":
                    ties += int((R.selector_sel(R.tie_targets(batch, heads, L, m), vis).sum(-1) > 1).sum())
                if name == "selector diag" and kind == "null":                          # every key position, by the only query that can: its own
                    sel = R.selector_sel(R.targets("diag", batch, heads, L), vis)
                    assert torch.equal(sel, torch.eye(L, dtype=f64).expand_as(sel))
                if name == "selector beyond" and kind == "null":
                    sel = R.selector_sel(R.targets("beyond", batch, heads, L), vis)
                    assert torch.equal(sel, torch.eye(L, dtype=f64).expand_as(sel))
    print(f"clip_matrix part1 | L {L} | tie rows {ties} | rows that see nothing {zero_rows}")
    assert zero_rows > 0 and (ties > 0 or L < 3)


def _caught(r, want4):
    return R.bad_rows(r.o, want4) > 0


def test_part1_mutations():
    """per mutation and construction: cases where it applies / cases where at least one row of O is not the expected bits.  Every structural
    mutation must be seen somewhere; the numeric ones change nothing here (every P is 0, 1/2 or 1)"""
    kinds = ("selector diag", "selector beyond", "selector spread", "selector ties", "uniform")
    table = {mut: {k: [0, 0] for k in kinds} for mut in R.MUTATIONS}
    for L, kind, batch, heads in CASES:
        if heads == 12:
            continue
        for name, q4, k4, v4, want4, m in R.exact_runs(L, kind, batch, heads):
            for mut in R.MUTATIONS:
                r = R.emulate(q4, k4, v4, m, mut=mut)
                if r is None:
                    continue
                hit = _caught(r, want4)
                table[mut][name][0] += 1
                table[mut][name][1] += hit
                if mut in R.NUMERIC_ONLY:
                    assert not hit, f"L{L} {kind} {name}: {mut} changed an exact construction"
    for mut, row in table.items():
        print(f"clip_matrix mutations | part 1 | {mut} | " + " | ".join(f"{k} {n} / {hit}" for k, (n, hit) in row.items()))
    for mut, row in table.items():
        if mut not in R.NUMERIC_ONLY:
            assert sum(hit for _, hit in row.values()) > 0, f"{mut}: no exact construction sees it"
    # what each construction is there for
    full = lambda mut, k: table[mut][k][0] > 0 and table[mut][k][0] == table[mut][k][1]
    assert full("drop_last", "uniform") and full("admit_masked", "uniform") and full("admit_clamped", "uniform")
    assert full("diag-1", "selector diag") and full("diag+1", "selector beyond") and full("diag+1", "uniform") and full("diag-1", "uniform")
    assert full("other_sample_v", "selector diag") and full("other_sample_v", "uniform")


def test_pos_swap_every_pair_of_a_block():
    """the selector sees ANY two keys of a 32-key block change places, not only the default pair: all pairs of CLIP's 77 keys"""
    L, batch, heads = 77, 1, 1
    runs = {name: rest for name, *rest in R.exact_runs(L, "null", batch, heads)}
    q4, k4, v4, want4, m = runs["selector diag"]
    for a in range(L):
        for b in range(a + 1, min(L, a // 32 * 32 + 32)):
            assert _caught(R.emulate(q4, k4, v4, m, mut="pos_swap", swap=(a, b)), want4), (a, b)


def test_part2_mutations():
    """N(0, 1) inputs (the GPU file's own, same seeds), q x 1 and q x 3: per mutation, the cases where it applies, where the worst row
    exceeds 2x the unmutated emulation's, and the range of that ratio.  Non-finite output counts as caught"""
    table = {m: [0, 0, float("inf"), 0.0] for m in R.MUTATIONS}
    for L in R.ROW_LENGTHS:
        for kind in R.ROW_MASKS:
            batch, heads = R.layouts(L, kind)[0]
            m = R.mask(kind, batch, L)
            for qamp in (1.0, 3.0):
                q4, k4, v4 = (R.to4(t.to(f64), batch, heads, L) for t in R.inputs(batch, heads, L, qamp))
                base = R.emulate(q4, k4, v4, m)
                floor = R.row_floor(base.o_ref)
                e0 = _row_err(base.o, base.o_ref, floor)
                for mut in R.MUTATIONS:
                    r = R.emulate(q4, k4, v4, m, mut=mut)
                    if r is None:
                        continue
                    e = _row_err(r.o, base.o_ref, floor) if bool(torch.isfinite(r.o).all()) else float("inf")
                    ratio = e / e0 if e0 > 0 else (float("inf") if e > 0 else 1.0)
                    t = table[mut]
                    t[0] += 1
                    t[1] += ratio > 2
                    t[2], t[3] = min(t[2], ratio), max(t[3], ratio)
    for mut, (n, hit, lo, hi) in table.items():
        print(f"clip_matrix mutations | part 2 | {mut} | applicable {n} | past 2x {hit} | ratio {lo:.3g} .. {hi:.3g}")
        assert n > 0, f"{mut}: applicable nowhere"
    for mut in R.MUTATIONS:
        if mut not in R.NUMERIC_ONLY:
            assert table[mut][1] > 0, f"{mut}: no Part 2 case sees it"


def test_embed_tables_and_reference():
    """the planted pairs are ties that round both ways, the tables hold no inf / NaN, and ids are clamped from both sides"""
    tok, pos = R.embed_tables(11, 77, 16)
    assert bool(torch.isfinite(tok.float()).all()) and bool(torch.isfinite(pos.float()).all())
    s = tok[:, 3].double()[:, None] + pos[:, 3].double()[None, :]
    lo, hi = s.to(bf16).double() < s, s.to(bf16).double() > s
    assert bool(lo.any()) and bool(hi.any())                               # not representable: rounded down here, up there
    ulp = 2.0 ** -7
    assert bool(((s.abs() / ulp * 2) % 2 == 1)[s.abs() > 1].all())          # exactly half an ulp past a bf16 number
    ids = torch.tensor([[0, 10, -1, 11, -2 ** 40, 2 ** 40]])
    ref = R.embed_ref(ids, tok, pos)
    want = (tok[[0, 10, 0, 10, 0, 10]].float() + pos[:6].float()).to(bf16)
    assert torch.equal(ref.view(torch.int16), want.view(torch.int16))
