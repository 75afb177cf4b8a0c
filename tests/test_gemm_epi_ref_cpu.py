"""The constructions of tests/test_gpu_gemm_epi_matrix.py must be able to FAIL, and its case table must reach what it claims.  Here,
without a GPU, the float64 references of tests/gemm_epi_ref.py stand in for the tile kernel, the split-K reduce pass and the
weight-stationary kernel:

1. every Part 1 case meets its preconditions on the reference alone (exact in fp32, |C| < 60 000, the GEGLU gate classes, the SiLU /
   quick-GELU class, column sums and row statistics exact, the rounding cases round more than half their elements) -- a case whose
   preconditions fail is an error, never a skip;
2. the tile table is the header's; body_of() reaches BOTH epilogue bodies for every term on every representative tile wherever the
   tile's compile-time class has both; every tile code has its all-terms case; the plan each case is meant to get is the plan the
   host planner answers for its descriptor (host function, fake aligned addresses, nothing dereferenced);
3. the mutation table: each mutation, at the tile's geometry, is rejected by the new criterion on at least one case -- a differing bit
   (or integer) in Part 1, a worst row past 2x the emulation's in Part 2.  For contrast the table prints what the older criterion
   (tests/test_gpu_kernels.py / test_gpu_f16.py: atol = rtol = 2e-2 on N(0, 1) data) reads at the same shape: recorded, not asserted.

The printed tables (pytest -s) are copied into profiles/gemm_epi_matrix.md.

Prerequisite of ONE test: test_planned_is_what_the_planner_answers asks the host planner itself, so it loads the built library
(build() of __graft_entry__.py; no GPU is touched).  Everything else here is plain torch."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from tests import gemm_epi_ref as R
from tests import t320_ref as T

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DEV = torch.device("cpu")
ROOT = Path(__file__).resolve().parent.parent


def _same(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


# =========================================================================================== 1. preconditions
def test_part1_preconditions():
    rounding = 0
    for spec in R.ALL_EXACT + R.bodies_cases():
        p = R.exact_problem(spec, DEV)
        r = R.exact_reference(spec, p)                                   # asserts exactness, |C| < 60 000, the activation / gate classes
        if spec.get("big"):
            rounding += 1
            assert float((r["out"] != r["pre"]).double().mean()) > 0.5, f"{R.case_id(spec)}: the store must round most elements"
        if spec.get("rowstat") and not spec.get("sums"):
            assert not torch.equal(R.rowstat_of(r["pre"]), R.rowstat_of(r["pre"], r["out"])), f"{R.case_id(spec)}: no element is rounded"
    assert rounding >= 2 * len(R.REPRESENTATIVE)
    print(f"gemm_epi_matrix cases | exact {len(R.ALL_EXACT)} (tile epilogue {len(R.GEMM_EXACT)}, reduce {len(R.SPLIT_EXACT)}, reduce with column sums "
          f"{len(R.SPLIT_SUMS)}, weight-stationary {len(R.WS_EXACT)}, layout-invariant {len(R.INV_EXACT)}, conv {len(R.CONV_EXACT)}) | per row "
          f"{len(R.ROWS_CASES)} | bodies {len(R.bodies_cases())}")


def test_part2_problems_are_what_they_say():
    """the folded form is the operator: on float64 statistics of the stored rows, unrounded, the folded GEMM equals LayerNorm + Linear"""
    x = R.r16x(R.batch_rows(200, 100, R.LN_K, DEV, 1, 1.0), bf16)
    stats = R.rowstat_of(x)
    p, plain = R.consumer_problem("ln", 5, 200, 1.0, x, stats, DEV)
    got, ref = R.gemm(p, tile=5)["pre"], R.ln_reference(p, plain)
    floor = T.row_floor(ref)
    assert T.row_err(got, ref, floor) < 2.0 ** -7                        # (W' and rstd are rounded: the 16-bit rounding of a weight)
    assert torch.equal(R.rowstat_of(x)[:, 0], (x.sum(1) * 2 ** 24).round().to(torch.int64))


# =========================================================================================== 2. tiles, bodies, plans
def test_tile_table_is_the_headers():
    codes = dict(re.findall(r"#define (SEER_TILE_\w+) (\d+)", (ROOT / "include" / "seer_hip.h").read_text()))
    rows = re.findall(r"X\((SEER_TILE_\w+), (\d+), (\d+), (\d+), (\d+), (\d+), (true|false), \d+\)", (ROOT / "seervideoldm_amd" / "csrc" / "gemm_tiles.h").read_text())
    assert len(rows) == 18
    table = {int(codes[n]): (n[len("SEER_TILE_"):], int(bm), int(bn), int(ns), int(wm), int(wn), sp == "true") for n, bm, bn, ns, wm, wn, sp in rows}
    assert table == R.TILES
    assert int(codes["SEER_TILE_WS"]) == R.WS and int(codes["SEER_TILE_AUTO_INVARIANT"]) == R.INVARIANT
    assert tuple(t for t in R.TILES if R.TILES[t][6]) == (2, 5, 8, 16) == R.SPLIT_TILES


def test_preload_classes_of_the_representative_tiles():
    """one tile per epilogue class, as read off the kernel: TM x TN and which loads exist before the K loop"""
    want = {2: (2, 2, True, True, True), 5: (4, 4, True, True, True), 12: (4, 5, False, False, False), 16: (3, 5, False, False, True),
            14: (4, 4, True, True, True), 21: (8, 4, False, False, False)}
    for t, (tm, tn, bias, rv, res) in want.items():
        s, pre = R.shape_of(t), R.preload_class(t)
        assert (s["TM"], s["TN"], pre["BIAS_PRE"], pre["RV_PRE"], pre["RES_PRE"]) == (tm, tn, bias, rv, res), t
        print(f"gemm_epi_matrix classes | {s['name']} | TM x TN {tm} x {tn} | BIAS_PRE {bias} RV_PRE {rv} RES_PRE {res} | GEGLU form {s['geglu_ok']} | ln_ok {R.ln_ok(t)}")
    assert [t for t in R.TILES if not R.ln_ok(t)] == [21] and [t for t in R.TILES if not R.shape_of(t)["geglu_ok"]] == [12, 13, 16, 17]


_TERMS = ("bias", "rpb", "res", "cs", "rot", "geglu", "k1", "rowstat", "silu", "qgelu", "f32")


def test_case_table_reaches_both_bodies():
    for t in R.REPRESENTATIVE:
        for term in _TERMS:
            got = set()
            for s in R.GEMM_EXACT:
                if s["tile"] == t and s.get(term):
                    got |= R.bodies_of(s, t)
            want = R.reachable("bias" if term == "k1" else term, t)
            assert got == want, f"{R.TILES[t][0]}: the cases with {term} reach {sorted(got)}, the kernel has {sorted(want)}"
            print(f"gemm_epi_matrix bodies | {R.TILES[t][0]} | {term} | {sorted(got) or 'no such form'}")
        # the row vector: a boundary on a fragment edge inside a tile, inside a 16-row fragment, and the preloaded one
        rpbs = {s["rpb"] for s in R.GEMM_EXACT if s["tile"] == t and s.get("rpb")}
        assert {96, 100, R.TILES[t][1]} <= rpbs
        assert {s.get("res") for s in R.GEMM_EXACT if s["tile"] == t} >= {"lds", "ldr4", "base8"}
        assert any(s["N"] % 8 == 4 for s in R.GEMM_EXACT if s["tile"] == t) and any(s.get("n_off") for s in R.GEMM_EXACT if s["tile"] == t)
        assert {s["M"] for s in R.GEMM_EXACT if s["tile"] == t} >= {1, R.TILES[t][1] - 1, R.TILES[t][1], R.TILES[t][1] + 1}
    for t in R.TILES:
        assert any(s["tile"] == t and all(s.get(k) for k in ("bias", "rpb", "res", "cs")) for s in R.GEMM_EXACT), f"no all-terms case on tile {t}"
    for s in R.INV_EXACT:
        assert R.bodies_of(s, s["runs"]) == {"general"}


def _desc(spec, lib_mod):
    """the descriptor the GPU file's launch of a GEMM case amounts to, with fake aligned addresses"""
    d = lib_mod.GemmDesc()
    M, N, K = spec["M"], spec["N"], spec["K"]
    n_out = N // 2 if spec.get("geglu") else N
    d.A, d.W, d.C = 0x10000, 0x20000, 0x30000 + (8 if spec.get("n_off") else 0)
    d.M, d.N, d.K, d.K1, d.lda, d.ldc = M, N, K, spec.get("k1") or K, K + 16, n_out + 16
    if spec.get("k1"):
        d.A2, d.lda2 = 0x40000, K - spec["k1"] + 24
    if spec.get("bias"):
        d.bias = 0x50000
    if spec.get("res"):
        d.residual, d.ldr = 0x60000 + (8 if spec["res"] == "base8" else 0), n_out + (20 if spec["res"] == "ldr4" else 16)
    if spec.get("rpb"):
        d.rowvec, d.rowvec_ld, d.rows_per_batch = 0x70000, N, spec["rpb"]
    e = lib_mod.SEER_EPI_F16 if spec.get("dt") == "f16" else 0
    for k, flag in (("geglu", lib_mod.SEER_EPI_GEGLU), ("silu", lib_mod.SEER_EPI_SILU), ("qgelu", lib_mod.SEER_EPI_QUICKGELU), ("f32", lib_mod.SEER_EPI_OUT_F32),
                    ("trans", lib_mod.SEER_EPI_TRANS_OUT), ("rot", lib_mod.SEER_EPI_ROTARY), ("cs", lib_mod.SEER_EPI_COLSCALE)):
        if spec.get(k):
            e |= flag
    d.epilogue = e
    if spec.get("rot"):
        hd, rd, tokens, off, cols = spec["rot"]
        d.rot_table, d.rot_tokens_per_batch, d.rot_pos_offset, d.rot_head_dim, d.rot_dim, d.rot_cols = 0x80000, tokens, off, hd, rd, cols
    if spec.get("cs"):
        d.col_scale, d.col_scale_cols = 0.5, spec["cs"]
    if spec.get("trans"):
        d.ldc, d.strideA, d.strideW, d.strideC = M, M * K, N * K, M * N
        d.lda = K
    d.batch = spec.get("batch", 1)
    d.mode, d.tile, d.splits = lib_mod.SEER_GEMM_PLAIN, spec["tile"], spec.get("splits", 1)
    if spec.get("rowstat"):
        d.rowstat = 0x90000
    if d.splits > 1:
        d.workspace, d.workspace_bytes = 0x1000000, 1 << 40
    gets = spec.get("gets", spec.get("colsum"))
    if gets == "tiles":
        d.colsum = 0xa0000
    elif gets == "fx":
        d.colsum_fx, d.colsum_fx_rows, d.colsum_fx_reps = 0xb0000, spec["rpb"], 1
    return d


def test_planned_is_what_the_planner_answers():
    """gemm_epi_ref.planned() restates gemm.hip for a tile asked for by name; here the host planner itself answers for every GEMM case"""
    from seervideoldm_amd import _lib
    lib = _lib.load()
    out = (C.c_int32 * 5)()
    reached = set()
    for spec in R.GEMM_EXACT + R.SPLIT_EXACT + R.SPLIT_SUMS + R.WS_EXACT + R.INV_EXACT + [R.split_act_spec(*c) for c in R.ROWS_SPLIT]:
        d = _desc(spec, _lib)
        assert lib.seer_gemm_plan(C.byref(d), out) == 0
        want, got = R.planned(spec), list(out)
        assert all(w is None or w == g for w, g in zip(want, got)), f"{R.case_id(spec)}: planned {got}, meant {want}"
        reached.add(tuple(got[1:]) if got[1] != R.K_WS else (got[1], "-", got[3], got[4]))
        if spec.get("rowstat"):
            assert lib.seer_gemm_rowstat_ok(C.byref(d)) == 1, R.case_id(spec)
    assert {r[0] for r in reached} == {R.K_TILE, R.K_SPLITK, R.K_WS} and {r[3] for r in reached} == {0, R.RED_PLAIN, R.RED_COLSUM, R.RED_FX32, R.RED_FX64}
    assert {r[1] for r in reached if r[0] == R.K_TILE} == set(R.TILES) and {r[1] for r in reached if r[0] == R.K_SPLITK} == set(R.SPLIT_TILES)
    print(f"gemm_epi_matrix plans | [kernel, tile, K slices, reduce] reached: {sorted(reached, key=str)}")


# =========================================================================================== 3. the mutation table
def _a2_buffers(p):
    """a2 as the GPU file lays it out, for a2_read_with_lda: row stride K2 + 24 behind a column offset of 8, next to lda = K1 + 16"""
    a2 = p["a2"]
    M, K2 = a2.shape
    buf = torch.full((M + 1, K2 + 24), float("nan"), dtype=f64)
    buf[:M, 8:8 + K2] = a2
    p.update(a2_buf=buf, a2_off=8, lda=p["a"].shape[1] + 16)
    return p


# mutation -> which cases of the table it is tried on (the first it applies to and that rejects it is printed)
_WHERE = {
    "drop_kstep_one_wave": lambda s: s in R.GEMM_EXACT and s.get("bias") and not s.get("rpb") and s["K"] == 192 and s["M"] > 2 * R.TILES[s["tile"]][1],
    "residual_row_clamped": lambda s: s in R.GEMM_EXACT and s.get("res") == "lds" and not s.get("bias"),
    "slice_last_twice": lambda s: s in R.SPLIT_EXACT and s.get("splits") == 3 and s.get("bias") and not s.get("big"),
    "slice0_skipped": lambda s: s in R.SPLIT_EXACT and s.get("splits") == 2 and s.get("res"),
    "rowvec_batch_per_wave_tile": lambda s: s in R.GEMM_EXACT and s.get("rpb") == 100,
    "rot_no_modulo": lambda s: s in R.GEMM_EXACT and s.get("rot"),
    "colscale_whole_fragment": lambda s: s in R.GEMM_EXACT and (s.get("cs") or 0) % 16 and not s.get("bias") and not s.get("rot"),
    "value_gate_exchanged_16": lambda s: s.get("geglu"),
    "pad_after_border_valid": lambda s: s.get("pad_after"),
    "phases_swapped": lambda s: s.get("up"),
    "a2_read_with_lda": lambda s: s in R.GEMM_EXACT and s.get("k1") and not s.get("silu") and not s.get("geglu"),
    "truncating_stores": lambda s: s.get("big") and not s.get("dt") and not s.get("splits"),
    "tile_twice_one_missing": lambda s: s in R.GEMM_EXACT and s.get("res") == "ldr4",
    "rowstat_after_rounding": lambda s: s.get("rowstat") and not s.get("sums"),
    "rowstat_ragged_row_counted": lambda s: s.get("rowstat") and s.get("sums"),
    "reduce_slice_order_irrelevant_but_slice_dropped": lambda s: s in R.SPLIT_EXACT and s.get("cs") and not s.get("silu"),
    "trans_out_ld_is_N": lambda s: s.get("trans"),
    "unstaged_tail_quad_skipped": lambda s: s in R.GEMM_EXACT and s["N"] % 8 == 4,
    "ws_colscale_whole_wave": lambda s: s["tile"] == R.WS and s.get("cs") == 164,
    "ws_panel_tail_from_previous_panel": lambda s: s["tile"] == R.WS and not s.get("geglu"),
    "activation_dropped": lambda s: s in R.SPLIT_EXACT and (s.get("silu") or s.get("qgelu")),
}
_PART2_ONLY = ("silu_before_bias", "ln_wsum_wrong_quad", "ln_mean_from_neighbour_row", "silu_qgelu_exchanged", "activation_after_colscale")
# (on the exact class SiLU and quick-GELU agree and commute with the scale of 0.5 only where both are the identity or 0: those two
#  mutations are held to the per-row criterion on the split cases, test_part2_split_activation_mutations)


def _old_reading(spec, mut, S):
    """what atol = rtol = 2e-2 reads on N(0, 1) data of the same shape under the same mutation (None: the older data has no such term)"""
    if "n" in spec:
        po = T.old_conv_problem(spec["n"], spec["H"], spec["W"], spec["Ci"], spec["Co"], DEV, seed=7, stride=spec.get("stride", 1),
                                pad_after=spec.get("pad_after", False), up=spec.get("up", False))
        ref, bad = T.conv(po), T.conv(po, mut=mut)
    else:
        terms = {k: spec[k] for k in ("bias", "rpb", "cs", "res", "rot", "k1", "geglu") if spec.get(k)}
        po = T.old_problem(spec["M"], spec["N"], spec["K"], DEV, seed=7, S=S, **terms)
        for k in ("f32", "trans", "rowstat"):
            if spec.get(k):
                po[k] = True
        if po.get("a2") is not None:
            _a2_buffers(po)
        po["prefill"] = 0.0
        tile = spec.get("runs", spec["tile"])
        ref, bad = R.gemm(po, tile=tile), R.gemm(po, mut=mut, tile=tile)
    if bad is None:
        return None
    ok, reading = T.old_close(bad["out"], ref["pre"])
    return ok, reading


def test_mutation_table():
    muts = [m for m in T.MUTATIONS + R.MUTATIONS if m not in _PART2_ONLY]
    assert sorted(muts) == sorted(_WHERE) and len(T.MUTATIONS) == 13 and len(R.MUTATIONS) == 13
    missed = []
    for mut in muts:
        seen = False
        for spec in R.ALL_EXACT:
            if not _WHERE[mut](spec):
                continue
            p = R.exact_problem(spec, DEV)
            tile = spec.get("runs", spec["tile"])
            store = f16 if spec.get("dt") == "f16" else bf16
            if "n" in spec:
                good, bad = R.conv(p, exact=True, geom=R.geom_of(tile)), R.conv(p, mut=mut, geom=R.geom_of(tile))
            else:
                if p.get("a2") is not None:
                    _a2_buffers(p)
                good, bad = R.exact_reference(spec, p), R.gemm(p, mut=mut, tile=tile, store=store)
            if bad is None:
                continue
            key = "rowstat" if mut.startswith("rowstat") else "out"
            differ = int(((bad[key] != good[key]) & ~((bad[key] != bad[key]) & (good[key] != good[key]))).sum()) if key == "out" else int((bad[key] != good[key]).sum())
            if not differ:
                continue
            old = _old_reading(spec, mut, p["S"])
            old_txt = "the older data has no such term" if old is None else f"old criterion reads {old[1]:.3g} of its bound: {'PASSES, a miss' if old[0] else 'fails'}"
            if key == "rowstat":
                old_txt = "the older tests compare the statistics' consumer at 2e-2"
            print(f"gemm_epi_matrix mutations | part 1 | {mut} | {R.case_id(spec)} | new: {differ}/{good[key].numel()} {'integers' if key == 'rowstat' else 'elements'} differ | {old_txt}")
            seen = True
            break
        if not seen:
            missed.append(mut)
    assert not missed, f"the exact criterion lets through: {missed}"


def _ln_case(kind, tile, M, amp):
    pp = R.producer_problem(tile, M, amp, DEV)
    prod = R.gemm(pp, tile=tile)
    return R.consumer_problem(kind, tile, M, amp, prod["out"], prod["rowstat"], DEV)


@pytest.mark.parametrize("mut,kind", [("silu_before_bias", "silu"), ("silu_before_bias", "qgelu"), ("ln_wsum_wrong_quad", "ln"), ("ln_mean_from_neighbour_row", "ln"),
                                      ("ln_mean_from_neighbour_row", "ln_geglu"), ("ln_wsum_wrong_quad", "ln_rot"), ("value_gate_exchanged_16", "geglu"),
                                      ("rot_no_modulo", "rot"), ("rot_no_modulo", "ln_rot"), ("drop_kstep_one_wave", "silu")])
def test_part2_mutations(mut, kind):
    """the per-row criterion on what integers cannot reach: every case of the kind must put the mutation past 2x the emulation"""
    cases = [c for c in R.ROWS_CASES if c[0] == kind]
    assert cases
    for _, tile, M, amp in cases:
        if kind.startswith("ln"):
            p, plain = _ln_case(kind, tile, M, amp)
            ref = R.ln_reference(p, plain)
            allow = 0.0
        else:
            p = R.act_problem(kind, tile, M, amp, DEV)
            if mut == "silu_before_bias":
                p = {k: v for k, v in p.items() if k not in ("rowvec", "rows_per_batch")}
            ref = R.gemm(p, tile=tile)["pre"]
            allow = 2 * R.act_f32_error(p, kind, ref) if kind in ("silu", "qgelu") and p.get("rowvec") is not None else 0.0
        good, bad = R.gemm(p, tile=tile), R.gemm(p, mut=mut, tile=tile)
        assert bad is not None, (mut, kind, tile, M)
        floor = T.row_floor(ref)
        e0, e1 = T.row_err(good["out"], ref, floor), T.row_err(bad["out"], ref, floor)
        ok_old, reading = T.old_close(bad["out"], ref)
        print(f"gemm_epi_matrix mutations | part 2 | {mut} | {kind} {R.TILES[tile][0]} M{M} x{amp:g} | worst row {e1:.4g} against the emulation's {e0:.4g}: "
              f"ratio {e1 / e0:.3g} | old criterion reads {reading:.3g} of its bound: {'PASSES, a miss' if ok_old else 'fails'}")
        assert e1 > 2 * e0 + allow, (mut, kind, tile, M, amp, e1, e0)


@pytest.mark.parametrize("mut", ["activation_dropped", "silu_qgelu_exchanged", "activation_after_colscale"])
def test_part2_split_activation_mutations(mut):
    """the split-K second pass has activation code of its own: EVERY split per-row case, both activations, the plain pass and both
    column-sum passes, must put each of the three past 2x the emulation (plus the float32 formula's allowance)"""
    for kind, tile, M, N, K, S, form in R.ROWS_SPLIT:
        spec, p = R.split_act_problem(kind, tile, M, N, K, S, form, DEV)
        assert R.planned(spec)[1] == R.K_SPLITK
        good, bad = R.gemm(p, tile=tile), R.gemm(p, mut=mut, tile=tile)
        assert bad is not None, (mut, kind, tile)
        ref = good["pre"]
        floor = T.row_floor(ref)
        e0, e1, e32 = T.row_err(good["out"], ref, floor), T.row_err(bad["out"], ref, floor), R.act_f32_error(p, kind, ref)
        ok_old, reading = T.old_close(bad["out"], ref)
        print(f"gemm_epi_matrix mutations | part 2 | {mut} | split_{kind} {R.TILES[tile][0]} {M}x{N}x{K} S{S} sums {form} | worst row {e1:.4g} against the "
              f"emulation's {e0:.4g}: ratio {e1 / e0:.3g} | old criterion reads {reading:.3g} of its bound: {'PASSES, a miss' if ok_old else 'fails'}")
        assert e1 > 2 * e0 + 2 * e32, (mut, kind, tile, M, S, form, e1, e0)


def test_unmutated_reference_is_the_operator():
    """the new terms against independent spellings"""
    import torch.nn.functional as Fn
    spec = next(s for s in R.GEMM_EXACT if s["tile"] == 5 and s.get("silu") and s.get("rpb"))
    p = R.exact_problem(spec, DEV)
    A = torch.cat([p["a"], p["a2"]], 1)
    x = Fn.linear(A, p["w"], p["bias"]) + p["rowvec"].repeat_interleave(96, 0)[:A.shape[0]]
    v = torch.where(x <= -104, torch.zeros_like(x), x)                   # float32 SiLU on the exact class: x, or -0 where expf overflows
    assert bool((Fn.silu(x.float()).double() == v).all()) and bool((x <= -104).any()) and bool((x >= 20).any())
    v[:, :p["col_scale"][1]] *= 0.5
    assert torch.equal(R.gemm(p, tile=5)["pre"], v + p["res"])
    _, q = R.split_act_problem("silu", 2, 101, 72, 256, 2, None, DEV)
    x = Fn.silu(Fn.linear(q["a"], q["w"], q["bias"]) + q["rowvec"].repeat_interleave(96, 0)[:101])
    x[:, :36] *= 0.125
    assert torch.allclose(R.gemm(q, tile=2)["pre"], x + q["res"], rtol=1e-13, atol=1e-15)
    q = R.act_problem("qgelu", 5, 100, 1.0, DEV)
    x = q["a"] @ q["w"].t() + q["bias"] + q["rowvec"][0]
    assert torch.allclose(R.gemm(q, tile=5)["pre"], x * torch.sigmoid(1.702 * x), rtol=1e-13, atol=0)
    spec = next(s for s in R.GEMM_EXACT if s.get("trans") and s.get("batch") == 1 and s["tile"] == 5)
    p = R.exact_problem(spec, DEV)
    r = R.gemm(p, tile=5)
    assert r["out"].shape == (spec["N"], spec["M"]) and r["pre"][7, 3] == (p["a"][3] @ p["w"][7] + p["bias"][7]) * 0.5
    x = T._ints((5, 8), DEV, 1, -9, 9) * 0.5
    rs = R.rowstat_of(x)
    assert rs.dtype == torch.int64 and int(rs[2, 0]) == int(x[2].sum() * 2 ** 24) and int(rs[2, 1]) == int((x[2] ** 2).sum() * 2 ** 24)
    # the layer norm from the integer totals: E[x^2] - mean^2 in double, rstd in fp32
    mr, r_ = R.ln_moments(rs, 8, 1e-5)
    d = x - x.mean(1, keepdim=True)
    want = (d.pow(2).mean(1) + 1e-5).rsqrt()
    assert torch.allclose(r_, want, rtol=2e-7) and torch.allclose(mr, x.mean(1) * want, rtol=3e-7, atol=1e-12)
