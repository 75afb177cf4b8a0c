#!/usr/bin/env python
"""Record the sequence of `ops` calls of one forward, on CPU, one text file per scenario: the yes/no check of a host-side refactor
("same launches, same order, same arguments").  Run it on two commits and `diff -r` the two directories.

    python scripts/trace_ops.py OUT_DIR

A line is a call: name, the shapes of tensor arguments, the scalars / keywords that select a kernel.  Scenarios: the inference
engine at the tiny CPU-test config over tests/torch_ops_backend and at BASELINE config 2 on torch's meta device over
tests/shape_ops_backend (whose producers here leave fake per-tile ColSums / ColSumsFx, so all four GroupNorm forms appear), each with
every switch on and with gn_fx / gn_colsums / rowchain off; two frame shards over gloo; the trainer's forward + backward."""
import os
import socket
import sys
import types
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from seervideoldm_amd import FSTextTransformer, SeerUNet, ops as hip_ops, parallel, synth  # noqa: E402
from tests import shape_ops_backend as sob  # noqa: E402
from tests import torch_ops_backend as tob  # noqa: E402

MINI = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)
SWITCHES = (None, "gn_fx", "gn_colsums", "rowchain")


def _d(v):
    if torch.is_tensor(v):
        return f"T{tuple(v.shape)}:{str(v.dtype)[6:]}"
    if isinstance(v, hip_ops.ColSumsFx):
        return f"Fx{tuple(v.buf.shape)}" + ("r" if v.reduced else "")
    if isinstance(v, hip_ops.ColSums):
        return f"Cs[{v.C}]"
    if isinstance(v, (tuple, list)):
        return "(" + ",".join(_d(x) for x in v) + ")"
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    return type(v).__name__


class Rec:
    """any ops backend, every function call logged"""

    def __init__(self, base, post=None):
        self._base, self._post, self.lines = base, post, []

    def __getattr__(self, name):
        v = getattr(self._base, name)
        if not isinstance(v, types.FunctionType) or name.endswith("_pays"):      # (a question, not a launch)
            return v

        def call(*a, **k):
            r = v(*a, **k)
            if self._post is not None:
                r = self._post(name, r, k)
            self.lines.append(f"{name}({', '.join([_d(x) for x in a] + [f'{n}={_d(x)}' for n, x in k.items()])})"
                              + (" -> None" if r is None else ""))
            return r
        return call


class _ShapeFx(types.SimpleNamespace):
    """tests/shape_ops_backend plus what the library has around column sums: producers leave ColSumsFx for colsum_batch=(B, arena),
    per-tile ColSums for colsum_batch=B; the consumers are shape-only"""


def _shape_fx():
    ns = _ShapeFx(**{k: v for k, v in vars(sob).items() if not k.startswith("__")})
    ns.FxArena, ns.ColSumsFx, ns.ColSums = hip_ops.FxArena, hip_ops.ColSumsFx, hip_ops.ColSums
    y = lambda x1, x2: torch.empty((x1.shape[0], x1.shape[1] + (0 if x2 is None else x2.shape[1])), dtype=torch.bfloat16, device=x1.device)
    ns.groupnorm_apply_fx = lambda x1, x2, *a, **k: y(x1, x2)
    ns.groupnorm_apply_from_colsums = lambda x1, x2, *a, **k: y(x1, x2)
    ns.groupnorm_stats_from_colsums = lambda cs1, cs2, batch, groups, stats: stats
    ns.groupnorm_stats_from_fx = lambda cs1, cs2, batch, groups, stats: stats
    ns.groupnorm_stats_fx = lambda x, batch, arena=None: hip_ops.ColSumsFx(arena.take(1, batch, x.shape[1]), x.shape[1])

    def post(name, r, k):
        cb = k.get("colsum_batch", 0)
        if r is not None and torch.is_tensor(r) and cb:
            C = r.shape[1]
            r.colsums = hip_ops.ColSumsFx(cb[1].take(1, cb[0], C), C) if isinstance(cb, tuple) else hip_ops.ColSums(None, C, 1, 1)
        return r
    return ns, post


def _mini_model():
    m = SeerUNet(**MINI)
    m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(MINI)), strict=True)
    return m


def _engine(m, ops, off):
    from seervideoldm_amd.unet import _Engine
    if off:
        setattr(m, off, False)
    try:
        return _Engine(m, ops=ops)
    finally:
        if off:
            setattr(m, off, True) if off == "gn_colsums" else delattr(m, off)


def _write(out, name, rec, eng=None):
    tail = [] if eng is None else [f"# gn_from_colsums={eng.gn_from_colsums} rowchains={eng.rowchains} ln_folded={eng.ln_folded}"]
    (out / f"{name}.txt").write_text("\n".join(rec.lines + tail) + "\n")
    print(f"{name}: {len(rec.lines)} calls")


def tiny(out):
    m = _mini_model()
    g = torch.Generator().manual_seed(1)
    for B, Fr, H, cf in ((1, 2, 16, 0), (2, 3, 8, 1)):
        x, ctx, t = torch.randn((B, 4, Fr, H, H), generator=g), torch.randn((B, Fr, 77, 256), generator=g), torch.tensor([501] * B)
        for off in SWITCHES:
            rec = Rec(tob)
            eng = _engine(m, rec, off)
            with torch.no_grad():
                eng.run(x, t, ctx, cf)
            _write(out, f"tiny_B{B}F{Fr}H{H}_{off or 'all_on'}", rec, eng)


def config2(out):
    model = SeerUNet(**dict(synth.SD15_UNET_CFG)).to("meta")
    x = torch.empty((2, 4, 12, 32, 32), device="meta")
    ctx = torch.empty((2, 12, 77, 768), device="meta")
    t = torch.empty((2,), dtype=torch.long, device="meta")
    for label, (base, post) in (("shape", (sob, None)), ("shapefx", _shape_fx())):
        for off in SWITCHES:
            rec = Rec(base, post)
            eng = _engine(model, rec, off)
            eng._rotary_table = lambda tb, T, eng=eng: sob.rotary_table(eng.w[tb + ".attn1.rotary_emb.freqs"], T)
            eng._context = lambda c: (torch.empty((2 * 12 * 77, 768), dtype=torch.bfloat16, device="meta"), 77)
            eng.run(x, t, ctx, 0)
            _write(out, f"config2_{label}_{off or 'all_on'}", rec, eng)


def _shard_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = _mini_model()
        rec = Rec(tob)
        m._ops_backend = rec
        m.ln_fold = m.ff_fold = False       # as tests/test_dist_gloo.py
        sh = parallel.attach(m, world, rank, batch_groups=1)
        for name in ("reduce_fx", "reduce_gn_stats"):       # the exchanges and the counts they return belong to the record
            def logged(sums, count, sync=None, _f=getattr(sh, name), _n=name):
                r = _f(sums, count, sync=sync)
                rec.lines.append(f"shard.{_n}({_d(sums)}, {count!r}) -> {r!r}")
                return r
            setattr(sh, name, logged)
        g = torch.Generator().manual_seed(7)
        x, ctx = torch.randn((1, 4, 3, 16, 16), generator=g), torch.randn((1, 3, 77, 256), generator=g)
        m(x, torch.tensor([501]), ctx, cond_frame=1)
        _write(Path(out), f"shard2_rank{rank}", rec, m._engine)
    finally:
        dist.destroy_process_group()


def sharded(out):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_shard_worker, args=(2, port, str(out)), nprocs=2, join=True)
    # ... and the same code path on one rank (no exchange), every switch
    for off in SWITCHES:
        m = _mini_model()
        rec = Rec(tob)
        m._ops_backend = rec
        if off:
            setattr(m, off, False)
        parallel.attach(m, 1, 0).force_exact_stats = True
        g = torch.Generator().manual_seed(7)
        m(torch.randn((1, 4, 2, 16, 16), generator=g), torch.tensor([501]), torch.randn((1, 2, 77, 256), generator=g), cond_frame=0)
        _write(out, f"shard1_exact_{off or 'all_on'}", rec, m._engine)


def trainer(out):
    from seervideoldm_amd.trainer import SeerTrainer
    from tests import torch_train_ops_backend as ttob
    cfg = dict(MINI, cross_attention_dim=192)
    unet = SeerUNet(**cfg)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg)), strict=True)
    fst = FSTextTransformer(num_frames=16, in_channels=192, out_channels=192, n_heads=2, num_layers=1, cross_attention_dim=192)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(num_frames=16, num_layers=1, channels=192, n_heads=2,
                                                                         cross_attention_dim=192)), strict=True)
    g = torch.Generator().manual_seed(3)
    for B, Fr, cond, H in ((1, 3, 1, 8), (1, 2, 0, 16)):
        for fx in ("1", "0"):
            os.environ["SEER_GN_FX"] = fx
            try:
                fst.set_numframe(Fr)
                rec = Rec(tob)
                tr = SeerTrainer(unet, fst, ops=rec, tops=ttob, lr=1e-3, max_grad_norm=0.3)
                tr.forward_backward(torch.randn((B, 4, Fr, H, H), generator=g), torch.randn((B, 4, Fr - cond, H, H), generator=g),
                                    torch.tensor([417] * B), torch.randn((B, 77, 192), generator=g), cond)
            finally:
                del os.environ["SEER_GN_FX"]
            _write(out, f"trainer_B{B}F{Fr}H{H}_fx{fx}", rec)


if __name__ == "__main__":
    out = Path(sys.argv[1])
    out.mkdir(parents=True, exist_ok=True)
    for part in (tiny, config2, sharded, trainer):
        part(out)
