"""TEST INFRASTRUCTURE ONLY -- the launch traces of tests/test_engine_launch_trace.py and tests/make_launch_trace_golden.py: a generic
call recorder around an ops backend, and the walks both of them record.

A record is [op, shapes of the tensor arguments, repr of the arguments with every tensor written as "T", type names of `.colsums`
and `.rowstats` on the result].  Shapes and names only: a trace does not depend on the values, the machine or the thread count.
Never imported by the product package."""
from __future__ import annotations

import contextlib
import itertools

import torch

from seervideoldm_amd import FSTextTransformer, SeerUNet, synth
from seervideoldm_amd import ops as real_ops
from seervideoldm_amd.trainer import SeerTrainer
from seervideoldm_amd.unet import _Engine
from tests import freeu_ref, step_cache_ref
from tests import shape_ops_backend as sob
from tests import torch_ops_backend as tob
from tests import torch_train_ops_backend as ttob
from tests.recording_ops_backend import RecordingOps

SMALL_CFG = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)
SMALL_SHAPES = ((1, 2, 16, 0), (2, 3, 8, 1))                    # (B, Fr, H, cond_frame), as tests/test_engine_cpu.py
SWITCHES = ("gn_colsums", "gn_fused", "gn_fx", "ln_fold", "ff_fold", "ff_fused", "rowchain", "ff_pre")     # the table of _Engine.__init__
TRAIN_CFG = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=192, attention_head_dim=8)
TRAIN_FS = dict(num_frames=16, num_layers=1, channels=192, n_heads=2, cross_attention_dim=192)
TRAIN_HP = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=0.3)
TRAIN_SHAPES = ((1, 3, 1, 8), (2, 3, 2, 8), (1, 2, 0, 16))      # (B, Fr, cond, H), as tests/test_trainer_cpu.py
FULL_FR = 12


def _describe(v, shapes):
    if torch.is_tensor(v):
        shapes.append(list(v.shape))
        return "T"
    if isinstance(v, (tuple, list)):
        inner = ", ".join(_describe(e, shapes) for e in v)
        return f"({inner})" if isinstance(v, tuple) else f"[{inner}]"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {_describe(e, shapes)}" for k, e in v.items()) + "}"
    if v is None or isinstance(v, (bool, int, float, str, torch.dtype, torch.device)):
        return repr(v)
    return type(v).__name__             # arenas, statistics objects, hooks: what they are, not where they live


def _marks(r):
    return [[type(getattr(e, "colsums", None)).__name__, type(getattr(e, "rowstats", None)).__name__]
            for e in (r if isinstance(r, tuple) else (r,))]


class Recorder:
    """`backend` with every call of one of its functions written down in `calls`; constants and classes pass through"""

    def __init__(self, backend, calls=None):
        self._backend = backend
        self.calls = [] if calls is None else calls

    def __getattr__(self, name):
        v = getattr(self._backend, name)
        if not callable(v) or isinstance(v, type) or name.endswith("_pays"):        # (*_pays: host predicates, no launches)
            return v

        def call(*a, **k):
            shapes = []
            args = _describe(a, shapes) + " " + _describe(k, shapes)
            r = v(*a, **k)
            self.calls.append([name, shapes, args, _marks(r)])
            return r
        return call


@contextlib.contextmanager
def _device_cus(cus):
    was = real_ops.device_cus
    real_ops.device_cus = lambda device=None: cus
    try:
        yield
    finally:
        real_ops.device_cus = was


def full_size_walk(layout_invariant, B, cond_frame, H, cus):
    """one evaluation of the full-size engine (SD-v1-5 widths, 12 frames) on the meta device: (calls, engine)"""
    with _device_cus(cus):
        model = SeerUNet(**dict(synth.SD15_UNET_CFG), layout_invariant=layout_invariant).to("meta")
        rec = Recorder(RecordingOps(B))
        eng = _Engine(model, ops=rec)
        eng._rotary_table = lambda tb, T: sob.rotary_table(eng.w[tb + ".attn1.rotary_emb.freqs"], T)
        eng._context = lambda c: (torch.empty((B * FULL_FR * 77, 768), dtype=torch.bfloat16, device="meta"), 77)
        x = torch.empty((B, 4, FULL_FR, H, H), device="meta")
        del rec.calls[:]            # (the packing calls of the constructor are no launches of the walk)
        eng.run(x, torch.empty((B,), dtype=torch.long, device="meta"), torch.empty((B, FULL_FR, 77, 768), device="meta"), cond_frame)
    return rec.calls, eng


def full_size_walks():
    out, chains = {}, 0
    for inv, B, cf, H, cus in itertools.product((False, True), (1, 2), (0, 2), (16, 32), (256, 32)):
        calls, eng = full_size_walk(inv, B, cf, H, cus)
        out[f"full/{'inv' if inv else 'default'}/B{B}/cond{cf}/H{H}/cus{cus}"] = calls
        chains = max(chains, eng.rowchains)
    return out, chains


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _small_model(cfg=SMALL_CFG):
    m = SeerUNet(**cfg)
    m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg)), strict=True)
    return m


def _small_engine(m, backend, attrs=(), **kw):
    """an engine over Recorder(backend), built while the model carries `attrs` (its switches)"""
    for k, v in attrs:
        setattr(m, k, v)
    try:
        rec = Recorder(backend)
        eng = _Engine(m, ops=rec, **kw)
    finally:
        for k, _ in attrs:
            delattr(m, k)
    return rec, eng


def small_walks():
    """real values at the small 320-wide config: every form of the engine, at both shapes"""
    out, m = {}, _small_model()
    for B, Fr, H, cf in SMALL_SHAPES:
        x, ctx, t = _randn((B, 4, Fr, H, H), 1), _randn((B, Fr, 77, 256), 2), torch.tensor([501] * B)
        tag = f"small/B{B}F{Fr}H{H}c{cf}/"

        def walk(name, backend, attrs=(), setup=None, **kw):
            rec, eng = _small_engine(m, backend, attrs, **{k: v for k, v in kw.items() if k == "fold_ln"})
            if setup is not None:
                setup(eng)
            del rec.calls[:]
            with torch.no_grad():
                eng.run(x, t, ctx, cf, **{k: v for k, v in kw.items() if k != "fold_ln"})
            out[tag + name] = list(rec.calls)
            return rec, eng
        walk("plain", tob)
        walk("fold_ln=False", tob, fold_ln=False)
        for s in SWITCHES:
            walk(s + "=off", tob, attrs=((s, False),))
        walk("layout_invariant=on", step_cache_ref.TorchOpsWithStepCache(), attrs=(("layout_invariant", True),))
        walk("freeu", freeu_ref.TorchOpsWithFreeu(), setup=lambda e: e.set_freeu((0.9, 0.2, 1.2, 1.4)))
        walk("return_attn", tob, return_attn=True)
        for branch in range(SMALL_CFG["layers_per_block"] + 1):
            rec, eng = walk(f"cache/branch{branch}/phase0", step_cache_ref.TorchOpsWithStepCache(),
                            setup=lambda e: e.set_step_cache(branch), cache_phase=0)
            del rec.calls[:]
            with torch.no_grad():
                eng.run(x, t, ctx, cf, cache_phase=1, cache_weights=(1.0, 0.0, 0.0))
            out[tag + f"cache/branch{branch}/phase1"] = list(rec.calls)
    return out


def trainer_walks():
    """one forward_backward at each shape of tests/test_trainer_cpu.py: forward and backward in one trace, both backends"""
    out = {}
    unet = _small_model(TRAIN_CFG)
    fst = FSTextTransformer(num_frames=TRAIN_FS["num_frames"], in_channels=192, out_channels=192, n_heads=2, num_layers=1,
                            cross_attention_dim=192)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(**TRAIN_FS)), strict=True)
    for B, Fr, cond, H in TRAIN_SHAPES:
        fst.set_numframe(Fr)
        calls = []
        tr = SeerTrainer(unet, fst, ops=Recorder(tob, calls), tops=Recorder(ttob, calls), **TRAIN_HP)
        del calls[:]
        tr.forward_backward(_randn((B, 4, Fr, H, H), 1), _randn((B, 4, Fr - cond, H, H), 2), torch.tensor([417, 93][:B]),
                            _randn((B, 77, 192), 3), cond)
        out[f"trainer/B{B}F{Fr}c{cond}H{H}"] = list(calls)
    return out


def record_all():
    """every walk: ({name: calls}, the most ops.rowchain launches any full-size walk made)"""
    walks, chains = full_size_walks()
    walks.update(small_walks())
    walks.update(trainer_walks())
    return walks, chains
