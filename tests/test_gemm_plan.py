"""The host decisions of csrc/gemm.hip -- which kernel, which tile, how many K slices, which reduce pass a descriptor gets
(seer_gemm_plan), and what the six queries derived from that plan answer -- against tests/golden/gemm_plan_parent.npz: the
answers of the PARENT of the change that put them behind one plan_gemm(), recorded by oracle/make_goldens_gemm_plan.py (grid and
recording described there).  Host functions only: no GPU, fake aligned addresses, nothing is dereferenced.

A rule of choose_split() / resolve_tile() / t320_plan() that is changed on purpose changes this fixture: record it again from the
library BEFORE the change and look at the difference."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from seervideoldm_amd import _lib

GOLDEN = Path(__file__).parent / "golden" / "gemm_plan_parent.npz"
WS, SYNC, CS_ROWS, FX_ROWS, FX_REPS, ROWSTAT_OK, LNFOLD_OK = range(7)
STATUS, KERNEL, TILE, SPLITS, REDUCE = range(5)
K_TILE, K_SPLITK, K_WS, K_T320 = (_lib.SEER_GEMM_KERNEL_TILE, _lib.SEER_GEMM_KERNEL_SPLITK, _lib.SEER_GEMM_KERNEL_WS,
                                  _lib.SEER_GEMM_KERNEL_T320)
T256x320 = 22


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert list(g["answer_names"]) == ["workspace_bytes", "sync_bytes", "colsum_rows", "colsum_fx_rows", "colsum_fx_reps", "rowstat_ok",
                                       "lnfold_ok"]
    assert list(g["plan_names"]) == ["status", "kernel", "tile", "splits", "reduce"]
    return g


def _structs(fields, desc):
    """the grid as an array of seer_gemm_desc, filled column by column"""
    arr = (_lib.GemmDesc * len(desc))()
    view = np.frombuffer(arr, dtype=np.dtype(_lib.GemmDesc))
    for j, f in enumerate(fields):
        view[str(f)] = desc[:, j]
    return arr


def _ask(lib, arr, fx_rpb):
    """(answers [n, 7], plan [n, 5]) of the library under test"""
    n = len(arr)
    ans, plan = np.zeros((n, 7), dtype=np.int64), np.zeros((n, 5), dtype=np.int32)
    out, reps = (C.c_int32 * 5)(), C.c_int32(0)
    for i in range(n):
        p = C.byref(arr[i])
        fx = lib.seer_gemm_colsum_fx_layout(p, int(fx_rpb[i]), C.byref(reps))
        ans[i] = (lib.seer_gemm_workspace_bytes(p), lib.seer_gemm_sync_bytes(p), lib.seer_gemm_colsum_rows(p), fx, reps.value,
                  lib.seer_gemm_rowstat_ok(p), lib.seer_gemm_lnfold_ok(p))
        assert lib.seer_gemm_plan(p, out) == 0
        plan[i] = out[:]
    return ans, plan


@pytest.fixture(scope="module")
def asked(lib, golden):
    return _ask(lib, _structs(golden["fields"], golden["desc"]), golden["fx_rows_per_batch"])


def _col(golden, name):
    return golden["desc"][:, list(golden["fields"]).index(name)]


def test_the_grid_reaches_every_branch_at_the_parent(golden):
    """a thinned grid must not hide a change: what the PARENT answered holds every value the rules can produce"""
    ans, plan, part = golden["answers"], golden["plan"], golden["part"]
    ok = plan[:, STATUS] == 0
    tile_in, mode = _col(golden, "tile"), _col(golden, "mode")
    assert (part == 0).sum() > 1500 and (part == 1).sum() > 20000
    assert set(plan[ok, KERNEL]) == {K_TILE, K_SPLITK, K_WS, K_T320}
    split = ok & (plan[:, KERNEL] == K_SPLITK)
    assert set(plan[split, TILE]) == {2, 8, 5, 16}                  # 64x64, G64x64_3, G128x128_2, G96x160_2
    auto = ok & (plan[:, KERNEL] == K_TILE) & np.isin(tile_in, (0, 19, 20, 22))
    # everything resolve_tile()'s AUTO branch returns: 96x160, 128x160, 128x128, 96x128, 128x64, 64x64 x 5 / x 3 stages, 64x64
    assert set(plan[auto, TILE]) == {16, 12, 5, 18, 7, 10, 8, 2}
    assert {1, 2, 4, 8} <= set(ans[ans[:, FX_ROWS] > 0, FX_REPS])
    assert {0, 4, 16, 64, 96, 128} <= set(ans[:, CS_ROWS])
    assert {3, 4} <= set(plan[split, REDUCE]) and {32, 64} <= set(ans[split, FX_ROWS])        # accumulated sums on 64- and 32-row blocks
    assert {1, 2} <= set(plan[split, REDUCE])
    ln = (_col(golden, "ln_rowstat") != 0) & (_col(golden, "ln_wsum") % 16 == 0) & (ans[:, WS] >= 0)
    assert set(ans[ln, LNFOLD_OK]) == {0, 1}
    # ... 0 because AUTO gives the launch without the fold to the weight-stationary kernel: the level-0 GEGLU projection
    ws_rule = ln & (tile_in == 0) & (_col(golden, "K") == 320) & (_col(golden, "N") == 2560) & (_col(golden, "M") >= 8192) & \
        (_col(golden, "epilogue") == 1) & (_col(golden, "colsum") == 0) & (_col(golden, "colsum_fx") == 0)
    assert ws_rule.any() and not ans[ws_rule, LNFOLD_OK].any()
    assert set(ans[ans[:, WS] >= 0, ROWSTAT_OK]) == {0, 1}
    # three different argument checks of validate(): no rows, K no multiple of 64, no output
    for bad in (_col(golden, "M") == 0, _col(golden, "K") % 64 != 0, _col(golden, "C") == 0):
        assert bad.any() and (ans[bad, WS] < 0).all() and (plan[bad, STATUS] < 0).all()
    t320 = ok & (plan[:, KERNEL] == K_T320)
    assert (plan[t320, SPLITS] > 1).any()
    # ... and asked for by name with slices but a `sync` one byte short: it runs unsplit
    short = t320 & (tile_in == T256x320) & (_col(golden, "sync") != 0) & (_col(golden, "sync_bytes") < ans[:, SYNC])
    assert short.any() and (plan[short, SPLITS] == 1).all()


def test_accepted_descriptors_answer_as_the_parent(golden, asked):
    ans, plan = asked
    acc = golden["answers"][:, WS] >= 0
    bad = np.flatnonzero(acc & ((ans != golden["answers"]).any(axis=1) | (plan != golden["plan"]).any(axis=1)))
    assert bad.size == 0, _show(golden, asked, bad)


def test_rejected_descriptors_return_the_parents_code_and_nothing_else(lib, golden, asked):
    ans, plan = asked
    rej = golden["answers"][:, WS] < 0
    assert rej.any()
    assert (ans[rej, WS] == golden["answers"][rej, WS]).all() and (plan[rej, STATUS] == golden["answers"][rej, WS]).all()
    assert not plan[rej, 1:].any()
    # the other five queries: what they answer for a NULL descriptor today -- nothing, and one replica
    assert not ans[rej][:, (SYNC, CS_ROWS, FX_ROWS, ROWSTAT_OK, LNFOLD_OK)].any() and (ans[rej, FX_REPS] == 1).all()
    differs = np.flatnonzero(rej & (ans != golden["answers"]).any(axis=1))
    print(f"{int(rej.sum())} rejected descriptors, {differs.size} of them answered differently by the parent:")
    print(_show(golden, asked, differs))
    null, reps, out = C.POINTER(_lib.GemmDesc)(), C.c_int32(0), (C.c_int32 * 5)()
    got = [lib.seer_gemm_workspace_bytes(null), lib.seer_gemm_sync_bytes(null), lib.seer_gemm_colsum_rows(null),
           lib.seer_gemm_colsum_fx_layout(null, 64, C.byref(reps)), reps.value, lib.seer_gemm_rowstat_ok(null), lib.seer_gemm_lnfold_ok(null)]
    assert got == list(golden["null_answers"]) and got[WS] < 0
    assert lib.seer_gemm_plan(null, out) == got[WS] and lib.seer_gemm_plan(null, None) == got[WS]


def test_plan_with_the_buffers_asked_for_agrees_with_the_size_queries(lib, golden, asked):
    """every accepted descriptor, given exactly the workspace and sync the size queries ask for: the plan's kernel and K slices are
    the ones those sizes were computed for.  No sync outside the 256 x 320 tile.  No workspace for an unsplit plan -- with the two
    exceptions the size query has always had and that this test pins: a launch with row statistics is kept unsplit after the size
    was answered for its split form, and where the 256 x 320 tile takes a shape unsplit that the smaller tiles would slice, the
    query leaves room for those ("room for both")."""
    ans, _ = asked
    fields = list(golden["fields"])
    acc = np.flatnonzero(ans[:, WS] >= 0)
    desc = golden["desc"][acc].copy()
    ws, sync = ans[acc, WS], ans[acc, SYNC]
    for name, val in (("workspace", np.where(ws > 0, 0x100000, 0)), ("workspace_bytes", ws), ("sync", np.where(sync > 0, 0x90000, 0)),
                      ("sync_bytes", sync)):
        desc[:, fields.index(name)] = val
    arr = _structs(golden["fields"], desc)
    out = (C.c_int32 * 5)()
    M, N = desc[:, fields.index("M")], desc[:, fields.index("N")]
    rows_ln = (desc[:, fields.index("rowstat")] != 0) | (desc[:, fields.index("ln_rowstat")] != 0)
    n_split = n_t320 = 0
    for i in range(len(acc)):
        p = C.byref(arr[i])
        # the sizes were asked of the descriptor as it was; with the buffers in place they do not move
        assert lib.seer_gemm_workspace_bytes(p) == ws[i] and lib.seer_gemm_sync_bytes(p) == sync[i]
        assert lib.seer_gemm_plan(p, out) == 0
        status, kernel, _, splits, _ = out[:]
        if status != 0:
            continue                             # a feature the launch cannot carry: the sizes are those of the launch without it
        if sync[i] > 0:
            assert kernel == K_T320 and splits > 1, (acc[i], out[:])
        if kernel == K_SPLITK:
            n_split += 1
            assert splits > 1 and ws[i] == splits * M[i] * N[i] * 4, (acc[i], out[:], ws[i])
        elif kernel == K_T320 and splits > 1:
            n_t320 += 1
            assert sync[i] > 0 and ws[i] > 0, (acc[i], out[:], ws[i], sync[i])
        elif ws[i] > 0:
            assert rows_ln[i] or kernel == K_T320, (acc[i], out[:], ws[i])
    assert n_split > 1000 and n_t320 > 50


def _show(golden, asked, idx, limit=12):
    ans, plan = asked
    fields = list(golden["fields"])
    lines = []
    for i in idx[:limit]:
        d = {f: int(v) for f, v in zip(fields, golden["desc"][i]) if v}
        lines.append(f"#{i} {d}\n   parent {list(golden['answers'][i])} {list(golden['plan'][i])}\n   now    {list(ans[i])} {list(plan[i])}")
    return f"{len(idx)} descriptors" + ("" if not len(idx) else ":\n" + "\n".join(lines))
