"""The constructions of tests/test_gpu_norm_matrix.py and tests/test_gpu_edge_matrix.py must be able to FAIL.  Here, without a GPU, the
float64 emulation of tests/norm_edge_ref.py stands in for the kernels:

1. every Part 1 precondition holds on the reference alone (sums below 2^24, the absorption at +-4 ulp of rstd -- and of the mean and
   the rounded 1 / C for LayerNorm --, targets non-zero and representable), and the unmutated emulation, which evaluates the kernels'
   own formulas, gives the expected bits;
2. the unmutated emulation passes Part 2 with ratio 1 by construction, and the float32 emulation of the timestep embedding in the
   kernel's order uses at most half of its derived allowance;
3. the mutation table: every mutation of norm_edge_ref.MUTATIONS changes a bit in every Part 1 case it applies to and pushes the
   worst owner of every Part 2 case it applies to past 2x the unmutated emulation's (past the derived allowance for the fp32 step
   kernel).  For contrast the table prints what the oldest tests' _close (atol = rtol = 2e-2) reads on the same Part 2 case: "old
   passes" counts the cases in which it finds no element outside its tolerance.

The printed table (pytest -s) is copied into profiles/norm_edge_matrix.md."""
import pytest
import torch

from tests import fused320_ref as R
from tests import norm_edge_ref as N

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DEV = torch.device("cpu")
DTS = [pytest.param(bf16, id="bf16"), pytest.param(f16, id="f16")]
FORMS = [("stats", 1), ("cs", 1), ("cs", 12), ("cs", 32), ("fx", 1), ("fx", 3)]


def _name(dt):
    return "f16" if dt == f16 else "bf16"


class Table:
    def __init__(self, part):
        self.part, self.t, self.fails = part, {m: [0, 0, float("inf"), 0, 0] for m in N.MUTATIONS}, []

    def note(self, mut, seen, what, ratio=None, old_outside=None):
        t = self.t[mut]
        t[0] += 1
        t[1] += bool(seen)
        if ratio is not None:
            t[2] = min(t[2], ratio)
        if old_outside is not None:
            t[3] += 1
            t[4] += old_outside == 0
        if not seen:
            self.fails.append(f"{what}: {mut} is not seen" + (f" (ratio {ratio:.3g})" if ratio is not None else ""))

    def show(self, dt, need):
        for mut, (n, hit, lo, oldn, oldpass) in self.t.items():
            tail = f" | smallest ratio {lo:.3g} | old _close passes {oldpass} of {oldn}" if self.part == 2 and n and lo != float("inf") else ""
            print(f"norm_edge_matrix mutations | part {self.part} | {_name(dt)} | {mut} | applicable {n} | seen {hit}{tail}")
            assert n > 0 or mut not in need, f"{mut}: applicable nowhere in part {self.part}"
        assert not self.fails, "\n".join(self.fails)


def _last_block(C, B, rows):
    cpp, rows_par, rpb, nblk = N.gn_geom(C, B, rows)
    return (nblk - 1) * rpb


# =========================================================================================== 1. preconditions and identity
@pytest.mark.parametrize("dt", DTS)
def test_groupnorm_preconditions_and_identity(dt):
    low = {}
    for shape in N.GN_APPLY_SHAPES:
        B, rows, C1, C2, G = shape
        C = C1 + C2
        x, m = N.gn_exact_x(B, rows, C, G, DEV, 41 + rows)
        assert torch.equal(R.r16(x, dt), x)
        st = N.gn_sums(x, G)
        assert torch.equal(N.r32(st), st) and float(st.abs().max()) < 2 ** 24
        for form, n in FORMS:
            if form != "stats" and N.gn_cs_geom(C, G, B, rows) is None:
                continue
            gn = N.exact_gn(form, B, G, C, DEV, 41 + rows, reps=n, parts=n, m=m, splits=(C1, C2))
            want = N.gn_apply(x, gn, dt, exact=True)
            info = {}
            assert torch.equal(N.gn_apply(x, gn, dt, info=info), want), f"{N.gn_id(shape)} {form}{n}: the emulation (rsqrt(var + eps) and all) does not give the expected bits"
            share = float((info["pre"] != want).double().mean())                 # the store has something to absorb: rsqrt(1 + eps) is not 1
            low["gn"] = min(low.get("gn", 1.0), share)                            # (x = m lands on beta exactly: a seventh of the elements)
            assert share > 0.1, f"{N.gn_id(shape)} {form}{n}: the final store rounds only {share:.3f} of its elements (part 4 asks for 0.1)"
            assert want.unique().numel() >= 10
    print(f"norm_edge_matrix | GroupNorm apply {_name(dt)}: the store rounds at least {low['gn']:.3f} of a case's elements")
    # the layouts the one-launch forms refuse: exactly the one with 257 channels per group
    assert [s for s in N.GN_APPLY_SHAPES if N.gn_cs_geom(s[2] + s[3], s[4], s[0], s[1]) is None] == [(1, 5, 2056, 0, 8)]
    # the geometry the shapes are there for
    assert N.gn_geom(64, 1, 2100)[3] == 66 and N.gn_geom(2560, 1, 9)[0] == 256 and N.gn_geom(2056, 1, 5)[0] == 256 and N.gn_geom(320, 2, 100)[1] == 6
    assert N.gn_cs_geom(288, 32, 2, 61)[0] == 72 and N.gn_cs_geom(512, 32, 2, 40)[0] == 64
    # a ragged last row block and rows < rows_par occur in both launch geometries
    two = [N.gn_geom(s[2] + s[3], s[0], s[1]) for s in N.GN_APPLY_SHAPES]
    one = [N.gn_cs_geom(s[2] + s[3], s[4], s[0], s[1]) for s in N.GN_APPLY_SHAPES]
    assert sum(s[1] % g[2] != 0 for s, g in zip(N.GN_APPLY_SHAPES, two)) >= 4 and any(s[1] < g[1] for s, g in zip(N.GN_APPLY_SHAPES, two))
    assert sum(g is not None and s[1] % g[2] != 0 for s, g in zip(N.GN_APPLY_SHAPES, one)) >= 4 and any(g is not None and s[1] < g[1] for s, g in zip(N.GN_APPLY_SHAPES, one))


def test_colsum_and_fx_preconditions():
    for one, two in [((1, 1), None), ((4, 3), None), ((1, 40), (2, 17)), ((2, 17), (4, 3)), ((1, 1), (1, 40))]:
        C1, C2 = (640, 320) if two else (960, 0)
        srcs = [N.colsum_partials(one[0], one[1], 3, C1, 32, DEV, 21)] + ([N.colsum_partials(two[0], two[1], 3, C2, 32, DEV, 22)] if two else [])
        st = N.colsums_to_stats(srcs, 3, 32)                                # asserts the 2^24 bound
        assert st.reshape(-1, 2).unique(dim=0).shape[0] == 96, "the statistics of all (batch element, group) differ"
        for s in srcs:
            assert torch.equal(N.r32(s), s)
    for C, rows, B in N.FX_SHAPES:
        for mag in (1.0, 2.0 ** -12, 2.0 ** 7):
            x = (R.ints((B, rows, C), DEV, 31 + C) + (torch.arange(B, dtype=f64) - 1)[:, None, None]) * mag
            assert torch.equal(R.r16(x, bf16), x) and torch.equal(R.r16(x, f16), x)
            k = float(1 << 20)
            assert torch.equal(N.r32(x * k), x * k) and torch.equal(N.r32(x * x), x * x), "the products the kernel forms are exact in fp32"
            if mag < 1:
                assert bool(((x * x * k) != (x * x * k).round()).any()), "the squares at 2^-12 are there to be rounded"


@pytest.mark.parametrize("dt", DTS)
def test_layernorm_softmax_preconditions_and_identity(dt):
    low = 1.0
    for rows, C in [(r, c) for c in N.LN_CS for r in N.LN_ROWS] + N.LN_LONG:
        x, pm, m = N.ln_exact_x(rows, C, DEV, 51 + C)
        gamma, beta = N.ln_affine(C, DEV, 52 + C)
        want = N.ln_exact(x, pm, gamma, beta, 1e-5, dt)                      # +-4 ulp of mean and rstd with the rounded 1 / C
        if rows <= 1000:
            info = {}
            assert torch.equal(N.layernorm(x, gamma, beta, 1e-5, dt, info=info), want), f"layernorm rows{rows} C{C}: the emulation does not give the expected bits"
            share = float((info["pre"] != want).double().mean())
            low = min(low, share)
            assert share > 0.1, f"layernorm rows{rows} C{C}: the final store rounds only {share:.3f} of its elements (part 4 asks for 0.1)"
    print(f"norm_edge_matrix | LayerNorm {_name(dt)}: the store rounds at least {low:.3f} of a case's elements")
    for n in N.SM_NS:
        for rows in N.SM_ROWS:
            x, want = N.softmax_exact(rows, n, DEV, 61 + n + rows)
            assert torch.equal(R.r16(x, dt), x) and torch.equal(R.r16(want, dt), want) and bool((want.sum(-1) == 1).all())
            assert rows < 2 or want[:min(rows, 4)].max(-1).values.unique().numel() == min(rows, 4, int(torch.log2(torch.tensor(float(n)))) + 1), "k differs between neighbouring rows"
            for scale in (1.0, 0.25):
                assert torch.equal(N.softmax_rows(x, scale, dt), want), f"softmax n{n}: the emulation does not give the expected bits"


def test_edge_preconditions():
    for case in N.ROTARY_CASES:
        rows, heads, hd, rd, tokens, off, ld = case
        buf = R.ints((rows * ld + ld,), DEV, 101 + rows)
        want = N.rotary_inplace(buf, case, R.dyadic_table(max(rows, tokens) + off, rd, DEV, 102 + rows))
        assert torch.equal(R.r16(want, bf16), want) and N.ROT_COL0 + 2 * heads * hd <= ld
        changed = (want != buf).nonzero().reshape(-1)
        cols = changed % ld
        assert bool(((cols >= N.ROT_COL0) & (cols < N.ROT_COL0 + 2 * heads * hd)).all()) and bool(((cols - N.ROT_COL0) % hd < rd).all())
    assert any(2 * c[1] * c[3] // 8 > 64 for c in N.ROTARY_CASES), "a case with more than 64 items: the second pass of the item loop"
    for B, K, Nf in N.SMALLM_CASES:
        x, w, b = N.smallm_exact(B, K, Nf, DEV, 111 + K)
        y = N.linear_smallm(x, w, b)
        assert torch.equal(N.r32(y[:B * Nf]), y[:B * Nf]) and bool(y[B * Nf:].isnan().all())
    assert sum((c[0] * c[2] * c[3] * c[4]) % 32 != 0 for c in N.CONV_IN_CASES) >= 3, "pixel counts that are no multiple of 32"
    assert all(N.conv_in_lds_bytes(c[1], c[5]) <= 160 * 1024 for c in N.CONV_IN_CASES) and N.conv_in_lds_bytes(N.CONV_IN_REFUSED[1], N.CONV_IN_REFUSED[5]) > 160 * 1024
    assert sum(N.conv_in_lds_bytes(c[1], c[5]) > 64 * 1024 for c in N.CONV_IN_CASES) >= 3, "cases above the 64 KiB opt-in"
    for case in N.CFG_CASES:
        for cfg in (True, False):
            eps, x, noise = N.cfg_problem(case, cfg, DEV, 141 + case[4])
            for row in N.CFG_EXACT_COEF:
                xp, x0 = N.cfg_ddim(eps, x, noise, row, cfg, 7.5, case)
                assert torch.equal(N.r32(xp), xp) and torch.equal(N.r32(x0), x0) and bool(torch.isfinite(xp).all()), "exact in fp32, no NaN frame read"
            assert torch.equal(N.cfg_ddim(eps, x, noise, N.CFG_EXACT_COEF[0], cfg, 7.5, case)[0], N.cfg_ddim(eps, x, noise, N.CFG_EXACT_COEF[0], cfg, 7.5, case)[1])
            assert torch.equal(N.cfg_ddim(eps, x, noise, N.CFG_EXACT_COEF[2], cfg, 7.5, case)[0], noise)


def test_timestep_embedding_allowance_is_not_tight():
    """a float32 emulation in the kernel's order (torch's float32 exp, sin, cos) uses at most half of the derived allowance"""
    t = torch.tensor(N.TE_TS)
    worst = 0.0
    for dim in N.TE_DIMS:
        for flip in (0, 1):
            for shift in (0.0, 1.0):
                if dim == 2 and shift == 1.0:
                    continue
                want, arg, expo = N.timestep_embedding(t, dim, flip, shift)
                share = float(((N.timestep_embedding_f32(t, dim, flip, shift).to(f64) - want).abs() / N.timestep_allowance(arg, expo)).max())
                worst = max(worst, share)
    print(f"norm_edge_matrix | timestep embedding: the float32 emulation uses {worst:.3f} of the allowance")
    assert worst <= 0.5


# =========================================================================================== 3. the mutation table
@pytest.mark.parametrize("dt", DTS)
def test_part1_mutations(dt):
    T = Table(1)
    for shape in N.GN_STATS_SHAPES:                                          # the statistics kernels
        B, rows, C1, C2, G = shape
        C = C1 + C2
        x, m = N.gn_exact_x(B, rows, C, G, DEV, 11 + rows)
        want = N.gn_sums(x, G)
        for mut in N.MUTATIONS:
            got = N.gn_sums(x, G, mut, _last_block(C, B, rows))
            if got is not None:
                T.note(mut, not torch.equal(got, want), f"stats {N.gn_id(shape)}")
    for C, rows, B in N.FX_SHAPES:
        x = R.ints((B, rows, C), DEV, 31 + C) + (torch.arange(B, dtype=f64) - 1)[:, None, None]
        rpb = N.fx_rows_per_block(C, B, rows)
        for mut in N.MUTATIONS:
            got = N.fx_sums(x, mut, (-(-rows // rpb) - 1) * rpb)
            if got is not None:
                T.note(mut, not torch.equal(got, N.fx_sums(x)), f"stats_fx C{C} rows{rows}")
    for one, two in [((4, 3), None), ((1, 40), (2, 17)), ((2, 17), (4, 3)), ((1, 1), (1, 40))]:
        C1, C2 = (640, 320) if two else (960, 0)
        srcs = [N.colsum_partials(one[0], one[1], 3, C1, 32, DEV, 21)] + ([N.colsum_partials(two[0], two[1], 3, C2, 32, DEV, 22)] if two else [])
        for mut in N.MUTATIONS:
            got = N.colsums_to_stats(srcs, 3, 32, mut)
            if got is not None:
                T.note(mut, not torch.equal(got, N.colsums_to_stats(srcs, 3, 32)), f"stats_from_colsums {one} {two}")
    for shape in N.GN_APPLY_SHAPES:                                          # the apply kernels
        B, rows, C1, C2, G = shape
        C = C1 + C2
        x, m = N.gn_exact_x(B, rows, C, G, DEV, 41 + rows)
        for form, n in FORMS:
            if form != "stats" and N.gn_cs_geom(C, G, B, rows) is None:
                continue
            gn = N.exact_gn(form, B, G, C, DEV, 41 + rows, reps=n, parts=n, m=m, splits=(C1, C2))
            want = N.gn_apply(x, gn, dt)
            for mut in N.GN_MUTS:
                if mut == "skip_second_column_pass" and form != "stats":
                    continue
                got = N.gn_apply(x, gn, dt, mut=mut)
                if got is not None:
                    T.note(mut, not torch.equal(got.nan_to_num(nan=12345.0), want), f"apply {form}{n} {N.gn_id(shape)}")
    for rows, C in [(r, c) for c in N.LN_CS for r in (1, 5)] + [(1000, 520)]:
        x, pm, m = N.ln_exact_x(rows, C, DEV, 51 + C)
        gamma, beta = N.ln_affine(C, DEV, 52 + C)
        want = N.layernorm(x, gamma, beta, 1e-5, dt)
        for mut in ("ln_stats_miss_last_8", "ln_neighbour_row_stats"):
            got = N.layernorm(x, gamma, beta, 1e-5, dt, mut=mut)
            if got is not None:
                T.note(mut, not torch.equal(got, want), f"layernorm rows{rows} C{C}")
    for n in N.SM_NS:
        for rows in N.SM_ROWS:
            x, want = N.softmax_exact(rows, n, DEV, 61 + n + rows)
            for mut in ("softmax_sum_miss_chunk", "softmax_max_first_512"):
                got = N.softmax_rows(x, 1.0, dt, mut=mut)
                if got is not None:
                    T.note(mut, not torch.equal(got.nan_to_num(nan=-1.0), want), f"softmax rows{rows} n{n}")
    for case in N.ROTARY_CASES:
        rows, heads, hd, rd, tokens, off, ld = case
        buf, table = R.ints((rows * ld + ld,), DEV, 101 + rows), R.dyadic_table(max(rows, tokens) + off, rd, DEV, 102 + rows)
        want = N.rotary_inplace(buf, case, table)
        for mut in ("rot_no_offset", "rot_no_modulo", "rot_pair_plus1"):
            got = N.rotary_inplace(buf, case, table, mut)
            if got is not None:
                T.note(mut, not torch.equal(got, want), f"rotary {case}")
    for case in N.CFG_CASES:
        for cfg in (True, False):
            eps, x, noise = N.cfg_problem(case, cfg, DEV, 141 + case[4])
            for mut in ("cfg_offset_fp", "cfg_no_cond_f"):
                rows_ = [(N.cfg_ddim(eps, x, noise, row, cfg, 7.5, case), N.cfg_ddim(eps, x, noise, row, cfg, 7.5, case, mut)) for row in N.CFG_EXACT_COEF]
                if rows_[0][1] is not None:
                    T.note(mut, any(not torch.equal(g[0].nan_to_num(nan=1e9), w[0]) for w, g in rows_), f"cfg_ddim {case} cfg{int(cfg)}")
    for case in N.CONV_IN_CASES:
        B, Cin, F, H, W, Cout = case
        x, w, bias = R.ints((B, Cin, F, H, W), DEV, 121 + Cout), R.ints((3, 3, Cin, Cout), DEV, 122 + Cout, -2, 2), R.ints((Cout,), DEV, 123, -8, 8)
        got = N.conv_in(x, w, bias, "conv_in_frame_batch_exchanged")
        if got is not None:
            T.note("conv_in_frame_batch_exchanged", not torch.equal(got, N.conv_in(x, w, bias)), f"conv_in {case}")
    for B, K, Nf in N.SMALLM_CASES:
        x, w, b = N.smallm_exact(B, K, Nf, DEV, 111 + K)
        got = N.linear_smallm(x, w, b, mut="smallm_tail_row_stored")
        if got is not None:
            T.note("smallm_tail_row_stored", not torch.equal(got.nan_to_num(nan=1e9), N.linear_smallm(x, w, b).nan_to_num(nan=1e9)), f"linear_smallm B{B} K{K} N{Nf}")
    T.show(dt, set(N.MUTATIONS))


_GN_ROWS = [(2, 100, 320, 0, 32, None), (3, 45, 640, 320, 32, None), (1, 9, 2560, 0, 32, None), (2, 61, 288, 0, 32, None), (2, 100, 320, 0, 32, 8.0)]


def _ratio(got, ref, emu, err):
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return err(got, ref) / err(emu, ref)


@pytest.mark.parametrize("dt", DTS)
def test_part2_mutations(dt):
    T = Table(2)
    for amp in (1.0, 4.0):
        for B, rows, C1, C2, G, ratio in _GN_ROWS:
            C = C1 + C2
            cpg = C // G
            x16, gamma, beta = N.gn_random(B, rows, C, G, dt, DEV, 71 + rows, amp, ratio)
            err = lambda a, b: N.seg_err(a, b, cpg)
            for form in ("stats", "cs", "fx"):
                gn = dict(N.stats_of(x16, G, form, DEV, 72, reps=1), gamma=gamma, beta=beta)
                ref = N.gn_apply(x16, dict(gn, form="stats", stats=N.gn_sums(x16, G)))
                emu = N.gn_apply(x16, gn, dt)
                assert _ratio(emu, ref, emu, err) == 1.0
                what = f"groupnorm {form} B{B} r{rows} C{C} x{amp:g} ratio {ratio}"
                for mut in N.MUTATIONS:
                    got = None
                    if mut in ("stats_miss_last_row_block", "straddle_to_first_group") or (mut == "skip_second_column_pass" and form == "stats"):
                        if form == "stats":
                            st = N.gn_sums(x16, G, mut, _last_block(C, B, rows))
                            got = None if st is None else N.gn_apply(x16, dict(gn, stats=N.r32(st)), dt)
                            if got is not None and mut == "skip_second_column_pass":
                                got = N.gn_apply(x16, gn, dt, mut=mut)
                        elif form == "fx" and mut == "stats_miss_last_row_block":
                            rpb = N.fx_rows_per_block(C, B, rows)
                            got = N.gn_apply(x16, dict(gn, fx=[N.fx_sums(x16, mut, (-(-rows // rpb) - 1) * rpb)[None]]), dt)
                    elif mut in N.GN_MUTS and mut != "skip_second_column_pass":
                        got = N.gn_apply(x16, gn, dt, mut=mut)
                    if got is not None:
                        r = _ratio(got, ref, emu, err)
                        T.note(mut, r > 2, what, r, N.old_close(got, ref))
        for C in (320, 520, 1536):
            x16, gamma, beta = N.ln_random(37, C, dt, DEV, 81 + C, amp)
            ref, emu = N.layernorm(x16, gamma, beta, 1e-5), N.layernorm(x16, gamma, beta, 1e-5, dt)
            err = lambda a, b: R.row_err(a, b, R.row_floor(b))
            for mut in ("ln_stats_miss_last_8", "ln_neighbour_row_stats"):
                got = N.layernorm(x16, gamma, beta, 1e-5, dt, mut=mut)
                r = _ratio(got, ref, emu, err)
                T.note(mut, r > 2, f"layernorm C{C} x{amp:g}", r, N.old_close(got, ref))
    for n in (520, 2056, 4096):
        for spread in (1.0, 30.0):
            for in_dt in (f32, dt):
                x = N.softmax_random(13, n, spread, in_dt, DEV, 91 + n)
                ref, emu = N.softmax_rows(x, 0.125), N.softmax_rows(x, 0.125, dt)
                err = lambda a, b: R.row_err(a, b, R.row_floor(b))
                for mut in ("softmax_sum_miss_chunk",):      # (a maximum over a prefix is still a softmax until exp overflows: Part 1 only)
                    got = N.softmax_rows(x, 0.125, dt, mut=mut)
                    r = _ratio(got, ref, emu, err)
                    T.note(mut, r > 2, f"softmax n{n} spread {spread:g}", r, N.old_close(got, ref))
    row = [float(torch.tensor(v, dtype=f32)) for v in (0.4216, 0.5541, 0.31, (1 - 0.4216) ** 0.5)]
    for case in N.CFG_CASES:
        for cfg in (True, False):
            eps, x, noise = N.cfg_problem(case, cfg, DEV, 171 + case[4], exact=False)
            wp, w0 = N.cfg_ddim(eps, x, noise, row, cfg, 7.5, case)
            ap, a0 = N.cfg_ddim_allowance(eps, x, noise, row, cfg, 7.5, case)
            assert bool(((N.r32(wp) - wp).abs() <= ap).all())
            for mut in ("cfg_offset_fp", "cfg_no_cond_f"):
                got = N.cfg_ddim(eps, x, noise, row, cfg, 7.5, case, mut)
                if got is not None:
                    over = float(((got[0] - wp).abs() / ap).nan_to_num(nan=float("inf")).max())
                    T.note(mut, over > 1, f"cfg_ddim {case} cfg{int(cfg)}", over, N.old_close(got[0], wp))
    T.show(dt, {"stats_miss_last_row_block", "count_off_by_one_row", "neighbour_batch_stats", "neighbour_group_stats", "straddle_to_first_group",
                "skip_replica_or_phase", "skip_second_column_pass", "ln_stats_miss_last_8", "ln_neighbour_row_stats", "softmax_sum_miss_chunk",
                "cfg_offset_fp", "cfg_no_cond_f"})


@pytest.mark.parametrize("dt", DTS)
def test_old_data_contrast(dt):
    """the hole the issue names first, on the oldest test's own kind of data: N(0, 1) with one distribution in every batch element and
    group, (2, 768, 320), 32 groups.  Statistics that miss the last 6 rows, or a count wrong by one row, leave every element inside
    atol = rtol = 2e-2; printed next to what the per-segment judge reads on the same result"""
    B, rows, C, G = 2, 768, 320, 32
    x16 = R.r16(R._randn((B, rows, C), DEV, 7), dt)
    gamma, beta = N.r32(1.0 + 0.2 * R._randn((C,), DEV, 8)), N.r32(0.2 * R._randn((C,), DEV, 9))
    gn = dict(form="stats", count=float(rows * C // G), groups=G, eps=1e-6, shape=(B, G), gamma=gamma, beta=beta, stats=N.r32(N.gn_sums(x16, G)))
    ref, emu = N.gn_apply(x16, gn), N.gn_apply(x16, gn, dt)
    for name, got in (("statistics miss the last 6 rows", N.gn_apply(x16, dict(gn, stats=N.r32(N.gn_sums(x16[:, :rows - 6], G))), dt)),
                      ("count off by one row", N.gn_apply(x16, gn, dt, mut="count_off_by_one_row")),
                      ("neighbour batch element", N.gn_apply(x16, gn, dt, mut="neighbour_batch_stats")),
                      ("neighbour group", N.gn_apply(x16, gn, dt, mut="neighbour_group_stats"))):
        outside = N.old_close(got, ref)
        r = N.seg_err(got, ref, C // G) / N.seg_err(emu, ref, C // G)
        print(f"norm_edge_matrix mutations | old data | {_name(dt)} | {name} | old _close: {outside} of {ref.numel()} outside ({'passes: a miss' if outside == 0 else 'fails'})"
              f" | worst segment / emulation {r:.3g}")
    assert N.old_close(emu, ref) == 0
