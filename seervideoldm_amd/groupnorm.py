"""Which form of GroupNorm runs -- decided here, once, for the inference engine (unet._Engine), the trainer (trainer.SeerTrainer)
and the VAE (vae.AutoencoderKL), over any ops backend (`ops`, profiler.ProfilingOps, the tests' stand-ins; the capability probes for
backends that lack a form live here and nowhere else).  By what the producers of the sources left next to them (`x.colsums`):
  every source ops.ColSumsFx (accumulated fixed point)  ->  groupnorm_apply_fx: one launch, no statistics launch;
  every source ops.ColSums (per tile)                   ->  groupnorm_apply_from_colsums: one launch (sharded engines, fused=False:
                                                            groupnorm_stats_from_colsums + groupnorm_apply);
  anything else (no sums, or one source of each kind)   ->  groupnorm_stats (a pass over the activations) + groupnorm_apply.
A one-launch form that answers None (not supported for this shape) falls to the two-launch form of the same sums."""
from __future__ import annotations


def _classify(ops, srcs, use_colsums):
    """'fx' / 'tiles' / None of the column sums of `srcs`"""
    FX = getattr(ops, "ColSumsFx", ())      # (): a stand-in backend without accumulated sums
    cs = [getattr(x, "colsums", None) for x in srcs]
    if any(isinstance(c, FX) for c in cs):
        return "fx" if all(isinstance(c, FX) for c in cs) else None
    return "tiles" if use_colsums and all(c is not None for c in cs) else None


def groupnorm(ops, x1, x2, batch, groups, rows_pb, eps, gamma, beta, silu, *, stats, use_colsums=True, fused=True, want_stats=False,
              shard=None, sync=None, arena=None, exact=False):
    """GroupNorm over the rows of x1 | x2 (rows_pb rows per batch element) -> (y, did the statistics come from column sums?).
    stats: [batch, groups, 2] fp32 scratch of the caller; want_stats (with fused=False: the one-launch per-tile form leaves none): it
    holds (sum, sumsq) on return.  shard, sync: parallel.FrameShard, the engine's sync_point; arena: the evaluation's ops.FxArena.
    exact: the exact-statistics form below whatever the shard layout (layout-invariant engines)."""
    srcs = [x1] if x2 is None else [x1, x2]
    count = rows_pb * (sum(x.shape[1] for x in srcs) // groups)
    if (exact or (shard is not None and shard.exact_stats)) and arena is not None and hasattr(ops, "groupnorm_stats_fx"):
        # frame shards (P > 1; batch groups alone exchange nothing and keep the forms below): EVERY GroupNorm normalises with exact
        # integer statistics -- a source whose producer left no accumulated sums (conv_in's output, tensors above the producers' row
        # limit) gets them from one pass over its rows; the sums stay with the tensor (a skip connection feeds a second GroupNorm
        # with the totals already exchanged)
        for x in srcs:
            if not isinstance(getattr(x, "colsums", None), ops.ColSumsFx):
                x.colsums = ops.groupnorm_stats_fx(x, batch, arena)
    kind = _classify(ops, srcs, use_colsums)
    cs1, cs2 = x1.colsums if kind else None, x2.colsums if kind and x2 is not None else None
    if kind == "fx":
        if shard is not None:
            # frame shards: the integer sums of all shards are added in place (exact: the statistics are the unsharded ones)
            count = shard.reduce_fx((cs1, cs2), count, sync=sync)
        y = ops.groupnorm_apply_fx(x1, x2, cs1, cs2, batch, groups, count, eps, gamma, beta, silu,
                                   **({"stats_out": stats} if want_stats else {}))
        if y is None:
            ops.groupnorm_stats_from_fx(cs1, cs2, batch, groups, stats)
            y = ops.groupnorm_apply(x1, x2, batch, groups, stats, count, eps, gamma, beta, silu)
        return y, True
    if kind == "tiles" and fused and shard is None and hasattr(ops, "groupnorm_apply_from_colsums"):
        # one launch: every apply block re-derives the statistics of its own groups from the column sums (no shards: a sharded run
        # all-reduces the statistics between the two steps)
        y = ops.groupnorm_apply_from_colsums(x1, x2, cs1, cs2, batch, groups, count, eps, gamma, beta, silu)
        if y is not None:
            return y, True
    _two_stage_stats(ops, kind, x1, x2, cs1, cs2, batch, groups, stats)
    if shard is not None:
        count = shard.reduce_gn_stats(stats, count, sync=sync)
    return ops.groupnorm_apply(x1, x2, batch, groups, stats, count, eps, gamma, beta, silu), kind == "tiles"


def groupnorm_statistics(ops, x, batch, groups, rows_pb, *, stats, use_colsums=True):
    """the statistics of the GroupNorm over x alone, for a launch that applies the normalisation itself (ops.rowchain) ->
    (statistics, count, from column sums?): the producer's accumulated fixed-point sums as they are (the chain reads them directly),
    else `stats` filled from its per-tile column sums or from a pass over x"""
    kind = _classify(ops, [x], use_colsums)
    count = rows_pb * (x.shape[1] // groups)
    if kind == "fx":
        return x.colsums, count, True
    _two_stage_stats(ops, kind, x, None, x.colsums if kind else None, None, batch, groups, stats)
    return stats, count, kind == "tiles"


def _two_stage_stats(ops, kind, x1, x2, cs1, cs2, batch, groups, stats):
    if kind == "tiles":
        ops.groupnorm_stats_from_colsums(cs1, cs2, batch, groups, stats)
    else:
        ops.groupnorm_stats(x1, x2, batch, groups, stats)
