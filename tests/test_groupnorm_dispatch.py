"""Which GroupNorm form runs (seervideoldm_amd/groupnorm.py), checked without a GPU on a recording backend with fake column sums:
for every classification of the sources, WHICH primitives are called, in which order, and whether the statistics count as "from
column sums".  The expectations are the ladders the engine (`_Engine._gn`, `_gn_stats`) and the trainer (`SeerTrainer._gn_fwd`) carried
before the dispatch was written once; the CPU stand-in's producers leave accumulated sums or nothing, so the per-tile forms
(groupnorm_apply_from_colsums, groupnorm_stats_from_colsums) are selected nowhere else in the CPU suite."""
import pytest
import torch

from seervideoldm_amd.groupnorm import groupnorm, groupnorm_statistics
from seervideoldm_amd.parallel import FrameShard

G, B, ROWS_PB, EPS = 4, 2, 6, 1e-6


class _Fx:          # stand-ins of ops.ColSumsFx / ops.ColSums: the dispatch looks at the type only
    reduced = False


class _Tiles:
    pass


class _Backend:
    """records the primitives called; `refuse`: the one-launch forms that answer None (not supported for the shape)"""
    ColSumsFx = _Fx

    def __init__(self, refuse=()):
        self.calls, self.kw, self.refuse = [], {}, refuse

    def _rec(self, name, ret, **kw):
        self.calls.append(name)
        self.kw[name] = kw
        return None if name in self.refuse else ret

    def groupnorm_stats(self, x1, x2, batch, groups, stats):
        return self._rec("stats", stats)

    def groupnorm_stats_from_colsums(self, cs1, cs2, batch, groups, stats):
        return self._rec("stats_from_colsums", stats, cs=(cs1, cs2))

    def groupnorm_stats_from_fx(self, cs1, cs2, batch, groups, stats):
        return self._rec("stats_from_fx", stats, cs=(cs1, cs2))

    def groupnorm_stats_fx(self, x, batch, arena=None):
        return self._rec("stats_fx", _Fx(), x=x, arena=arena)

    def groupnorm_apply(self, x1, x2, batch, groups, stats, count, eps, gamma, beta, silu):
        return self._rec("apply", "y", count=count, stats=stats, eps=eps, silu=silu)

    def groupnorm_apply_from_colsums(self, x1, x2, cs1, cs2, batch, groups, count, eps, gamma, beta, silu):
        return self._rec("apply_from_colsums", "y", count=count, cs=(cs1, cs2), eps=eps, silu=silu)

    def groupnorm_apply_fx(self, x1, x2, cs1, cs2, batch, groups, count, eps, gamma, beta, silu, stats_out=None):
        return self._rec("apply_fx", "y", count=count, cs=(cs1, cs2), stats_out=stats_out, eps=eps, silu=silu)


class _Plain:
    """a backend that has the two-stage forms only (tests/shape_ops_backend.py)"""
    def __init__(self):
        self.calls = []

    def groupnorm_stats(self, *a):
        self.calls.append("stats")

    def groupnorm_stats_from_colsums(self, *a):
        self.calls.append("stats_from_colsums")

    def groupnorm_apply(self, *a):
        self.calls.append("apply")
        return "y"


def _x(kind, C=8):
    x = torch.zeros((B * ROWS_PB, C))
    x.colsums = {"fx": _Fx, "tiles": _Tiles, "none": lambda: None}[kind]()
    return x


def _run(ops, k1, k2=None, **kw):
    x1, x2 = _x(k1), (None if k2 is None else _x(k2))
    stats = torch.zeros((B, G, 2))
    y, from_colsums = groupnorm(ops, x1, x2, B, G, ROWS_PB, EPS, "gamma", "beta", True, stats=stats, **kw)
    assert y == "y"
    return from_colsums, x1, x2, stats


COUNT1, COUNT2 = ROWS_PB * (8 // G), ROWS_PB * (16 // G)

# (sources, keywords of the call, forms that answer None) -> (primitives in order, from column sums?)
ENGINE_CASES = [
    (("fx",), {}, (), ["apply_fx"], True),
    (("fx", "fx"), {}, (), ["apply_fx"], True),
    (("fx", "fx"), {"use_colsums": False, "fused": False}, (), ["apply_fx"], True),   # (producers leave none when the switch is off)
    (("fx",), {}, ("apply_fx",), ["apply_fx", "stats_from_fx", "apply"], True),
    (("fx", "tiles"), {}, (), ["stats", "apply"], False),
    (("tiles", "fx"), {}, (), ["stats", "apply"], False),
    (("fx", "none"), {}, (), ["stats", "apply"], False),
    (("tiles",), {}, (), ["apply_from_colsums"], True),
    (("tiles", "tiles"), {}, (), ["apply_from_colsums"], True),
    (("tiles", "tiles"), {}, ("apply_from_colsums",), ["apply_from_colsums", "stats_from_colsums", "apply"], True),
    (("tiles", "tiles"), {"fused": False}, (), ["stats_from_colsums", "apply"], True),
    (("tiles",), {"use_colsums": False}, (), ["stats", "apply"], False),
    (("tiles", "none"), {}, (), ["stats", "apply"], False),
    (("none", "tiles"), {}, (), ["stats", "apply"], False),
    (("none",), {}, (), ["stats", "apply"], False),
    (("none", "none"), {}, (), ["stats", "apply"], False),
]


@pytest.mark.parametrize("srcs,kw,refuse,calls,from_cs", ENGINE_CASES)
def test_form_selection(srcs, kw, refuse, calls, from_cs):
    ops = _Backend(refuse)
    got, x1, x2, stats = _run(ops, *srcs, **kw)
    assert ops.calls == calls and got is from_cs
    count = COUNT1 if len(srcs) == 1 else COUNT2
    last = ops.kw[calls[-1]]
    assert last["count"] == count and last["eps"] == EPS and last["silu"] is True
    if calls[-1] == "apply":
        assert last["stats"] is stats
    for name in ("apply_fx", "apply_from_colsums", "stats_from_colsums", "stats_from_fx"):
        if name in ops.kw:
            assert ops.kw[name]["cs"] == (x1.colsums, None if x2 is None else x2.colsums)
    if "apply_fx" in ops.kw:
        assert ops.kw["apply_fx"]["stats_out"] is None


def test_backend_without_the_newer_forms():
    ops = _Plain()
    assert _run(ops, "tiles", "tiles")[0] is True and ops.calls == ["stats_from_colsums", "apply"]
    ops = _Plain()
    assert _run(ops, "none")[0] is False and ops.calls == ["stats", "apply"]


def test_trainer_keeps_the_statistics():
    """want_stats: the one-launch fixed-point form writes (sum, sumsq) into `stats` (stats_out); fused=False: per-tile sums take the
    two launches -- the one-launch form leaves no statistics for the backward"""
    t = dict(want_stats=True, fused=False)
    ops = _Backend()
    got, _, _, stats = _run(ops, "fx", "fx", **t)
    assert ops.calls == ["apply_fx"] and got and ops.kw["apply_fx"]["stats_out"] is stats
    ops = _Backend(("apply_fx",))
    _run(ops, "fx", **t)
    assert ops.calls == ["apply_fx", "stats_from_fx", "apply"]
    for srcs, calls in ((("tiles", "tiles"), ["stats_from_colsums", "apply"]), (("fx", "tiles"), ["stats", "apply"]),
                        (("none",), ["stats", "apply"])):
        ops = _Backend()
        _, _, _, stats = _run(ops, *srcs, **t)
        assert ops.calls == calls and ops.kw["apply"]["stats"] is stats


def _shard(exact):
    sh = FrameShard(1, 0)
    sh.plan(1, 3)
    sh.force_exact_stats = exact
    return sh


def test_frame_shards_normalise_with_exact_sums():
    """force_exact_stats (what P > 1 frame shards run): a source without accumulated sums gets them from one pass
    (groupnorm_stats_fx), they stay with the tensor, and every GroupNorm is the fixed-point form with the exchanged count"""
    ops, sh, arena = _Backend(), _shard(True), object()
    synced = []
    got, x1, x2, _ = _run(ops, "tiles", "none", shard=sh, sync=synced.append, arena=arena)
    assert ops.calls == ["stats_fx", "stats_fx", "apply_fx"] and got is True
    assert isinstance(x1.colsums, _Fx) and isinstance(x2.colsums, _Fx) and ops.kw["stats_fx"]["arena"] is arena
    assert ops.kw["apply_fx"]["count"] == COUNT2 / sh.local_frames * sh.total_frames
    # the skip connection's second GroupNorm: its sums are there already
    ops2 = _Backend()
    stats = torch.zeros((B, G, 2))
    groupnorm(ops2, x1, None, B, G, ROWS_PB, EPS, "g", "b", False, stats=stats, shard=sh, arena=arena)
    assert ops2.calls == ["apply_fx"]
    # one source has them: only the other is passed over
    ops3 = _Backend()
    _run(ops3, "fx", "none", shard=sh, arena=arena)
    assert ops3.calls == ["stats_fx", "apply_fx"]
    # no arena (gn_fx off): the statistics tensor is exchanged between the two launches, no one-launch per-tile form
    ops4 = _Backend()
    assert _run(ops4, "tiles", shard=sh, arena=None)[0] is True and ops4.calls == ["stats_from_colsums", "apply"]
    ops5 = _Backend()
    assert _run(ops5, "none", shard=sh, arena=None)[0] is False and ops5.calls == ["stats", "apply"]


def test_batch_groups_keep_the_single_process_forms_but_the_fused_per_tile_one():
    ops, sh = _Backend(), _shard(False)
    assert _run(ops, "none", "tiles", shard=sh, arena=object())[0] is False and ops.calls == ["stats", "apply"]
    ops = _Backend()
    assert _run(ops, "fx", shard=sh, arena=object())[0] is True and ops.calls == ["apply_fx"]
    ops = _Backend()
    assert _run(ops, "tiles", shard=sh, arena=object())[0] is True and ops.calls == ["stats_from_colsums", "apply"]


@pytest.mark.parametrize("kind,use_colsums,calls,from_cs", [
    ("fx", True, [], True), ("fx", False, [], True), ("tiles", True, ["stats_from_colsums"], True),
    ("tiles", False, ["stats"], False), ("none", True, ["stats"], False)])
def test_statistics_for_a_launch_that_normalises_itself(kind, use_colsums, calls, from_cs):
    ops, x, stats = _Backend(), _x(kind), torch.zeros((B, G, 2))
    st, count, got = groupnorm_statistics(ops, x, B, G, ROWS_PB, stats=stats, use_colsums=use_colsums)
    assert ops.calls == calls and got is from_cs and count == COUNT1
    assert st is (x.colsums if kind == "fx" else stats)
