"""SeerUNet -- host-side mirror of the reference's `seer.models.unet_3d_condition.SeerUNet` over libseer_hip.so.

Same constructor keywords, same `state_dict()` key layout (a reference `pytorch_model.bin` loads with strict=True), same
call: `unet(sample[B,4,F,h,w], timestep, context[B,F,77,ctx], cond_frame=0) -> Tensor[B,4,F,h,w]`
(seer/models/unet_3d_condition.py:64-84, 283-376).  The module tree only HOLDS parameters; the forward is executed by
`_Engine`, which repacks the weights once (bf16, channels-last GEMM layouts, fused q|k|v, interleaved GEGLU rows,
concatenated time-embedding projections) and then issues hand-written HIP kernels through the C ABI on torch's current
stream.  Activations are token-major bf16 [B*F*H*W, C] end to end; nothing is computed by torch ops.

There is no CPU path: calling forward with CPU tensors, or without the built library, raises.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import _lib
from . import ops as hip_ops
from . import synth
from .groupnorm import groupnorm, groupnorm_statistics
from .step_cache import RING_SLOTS, StepCachePolicy
from .weights import geglu_row_order, pack_conv1x1, pack_conv3x3, pack_conv3x3_up_phases

bf16 = torch.bfloat16
MAX_WIN_SIZE, MAX_RATIO, MIN_WIN_SIZE = 8, 4, 4      # seer/models/attention.py:31-33


class _Node(nn.Module):
    """parameter container: gives the state dict / named_modules() the reference's dotted names."""
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("container module: the forward pass lives in SeerUNet.forward")


def _build_tree(root: nn.Module, shapes: "OrderedDict[str, Tuple[int, ...]]"):
    for key, shape in shapes.items():
        parts = key.split(".")
        mod = root
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, _Node())
            mod = mod._modules[p]
        if key.endswith("rotary_emb.freqs"):
            mod.register_buffer(parts[-1], synth.synth_tensor(key, shape))
        else:
            mod.register_parameter(parts[-1], nn.Parameter(torch.zeros(shape), requires_grad=True))


class _Config(dict):
    __getattr__ = dict.get


class SeerUNet(nn.Module):
    _supports_gradient_checkpointing = True
    config_name = "config.json"

    def __init__(self, sample_size=None, in_channels=4, out_channels=4, center_input_sample=False,
                 flip_sin_to_cos=True, freq_shift=0,
                 down_block_types=("CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D"),
                 up_block_types=("UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D"),
                 block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, downsample_padding=1,
                 mid_block_scale_factor=1, act_fn="silu", norm_num_groups=32, norm_eps=1e-5,
                 cross_attention_dim=1280, attention_head_dim=8, compute_dtype=None, layout_invariant=None):
        super().__init__()
        # the reference overwrites the block types / downsample padding with constants (unet_3d_condition.py:90-92)
        if len(block_out_channels) != 4:
            raise ValueError("SeerUNet is hard-wired to 4 resolution levels (3 x CrossAttnDownBlock3D + DownBlock3D)")
        if act_fn != "silu":
            raise ValueError(f"act_fn {act_fn!r}: only 'silu' exists on this path")
        self.config = _Config(sample_size=sample_size, in_channels=in_channels, out_channels=out_channels,
                              center_input_sample=center_input_sample, flip_sin_to_cos=flip_sin_to_cos,
                              freq_shift=freq_shift, down_block_types=tuple(down_block_types),
                              up_block_types=tuple(up_block_types), block_out_channels=tuple(block_out_channels),
                              layers_per_block=layers_per_block, downsample_padding=1,
                              mid_block_scale_factor=mid_block_scale_factor, act_fn=act_fn,
                              norm_num_groups=norm_num_groups, norm_eps=norm_eps,
                              cross_attention_dim=cross_attention_dim, attention_head_dim=attention_head_dim)
        self.sample_size = sample_size
        self._shapes = synth.unet_param_shapes(self.config)
        _build_tree(self, self._shapes)
        self._engine: Optional[_Engine] = None
        self._slice_size = None
        self.use_graph = False
        self._shard = None              # parallel.FrameShard when attached (seervideoldm_amd/parallel.py)
        self.gn_colsums = True          # GroupNorm statistics from the producing GEMM's column sums (read by prepare())
        self._ops_backend = hip_ops     # tests may inject tests/torch_ops_backend.py to exercise the host logic on CPU
        self._ctx_slice = None
        # 16-bit storage type of activations and weights (fp32 accumulation and statistics either way): bf16 = the reference under
        # `mixed_precision: "bf16"` (BASELINE config 2), torch.float16 = under "fp16" (what every shipped yaml says:
        # configs/inference_base.yaml:16, eval.yaml:22, train.yaml:33).  Set here, by `unet.compute_dtype = ...`, or -- None --
        # taken from the autocast state of the call (accelerate's prepare() wraps forward in torch.autocast with the configured type).
        if compute_dtype not in (None, torch.bfloat16, torch.float16):
            raise ValueError(f"compute_dtype {compute_dtype!r}: torch.bfloat16 or torch.float16 (fp32 accumulation either way)")
        self.compute_dtype = compute_dtype
        # layout-invariant mode (off unless asked for): the output of one batch element depends on that element's inputs, the weights and
        # the storage type only -- not on the batch it came in, the CFG layout, the rank / frame-shard layout or the device's CU count.
        # True / False here or as an attribute before the first forward; None = the environment's SEER_LAYOUT_INVARIANT=1 (_Engine)
        self.layout_invariant = layout_invariant
        self._freeu: Optional[Tuple[float, float, float, float]] = None     # (s1, s2, b1, b2) while FreeU is on (enable_freeu)
        self._step_cache: Optional[StepCachePolicy] = None                  # the policy while step caching is on (enable_step_cache)

    # ---- construction / weights -------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path, subfolder=None, revision=None, low_cpu_mem_usage=False, **kw):
        """diffusers semantics (inference_img.py:74-79): read config.json, ignore unknown keys, load weights by name,
        non-strict (temporal keys are absent from an SD-v1-5 checkpoint)."""
        import inspect
        root = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(root, cls.config_name)) as f:
            cfg = json.load(f)
        allowed = set(inspect.signature(cls.__init__).parameters) - {"self"}
        model = cls(**{k: v for k, v in cfg.items() if k in allowed})
        for fname in ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin", "pytorch_model.bin"):
            fp = os.path.join(root, fname)
            if os.path.exists(fp):
                if fname.endswith(".safetensors"):
                    from safetensors.torch import load_file
                    sd = load_file(fp)
                else:
                    sd = torch.load(fp, map_location="cpu")
                model.load_state_dict(sd, strict=False)
                break
        else:
            raise FileNotFoundError(f"no weight file under {root}")
        return model

    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._engine = None
        return out

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    def _dtype_of_call(self):
        """the 16-bit storage type this forward runs in: compute_dtype, else the autocast type when the caller wrapped the call in
        torch.autocast (accelerate.prepare under mixed_precision fp16 / bf16), else bf16"""
        if self.compute_dtype is not None:
            return self.compute_dtype
        if torch.is_autocast_enabled():
            dt = torch.get_autocast_dtype("cuda")
            if dt in (torch.bfloat16, torch.float16):
                return dt
        return torch.bfloat16

    def prepare(self, dtype=None):
        """(re)build the packed device weights from the current parameters; call after editing parameters in place."""
        dtype = dtype or self._dtype_of_call()
        dev = next(self.parameters()).device.type
        with torch.autocast(device_type=dev if dev in ("cuda", "cpu") else "cuda", enabled=False):     # fp32 weight algebra stays fp32
            self._engine = _Engine(self, ops=self._ops_backend, shard=self._shard, dtype=dtype)
        self._engine.set_freeu(self._freeu)
        self._engine.set_step_cache(None if self._step_cache is None else self._step_cache.branch)
        return self

    # ---- toggles of the reference surface ---------------------------------------------------------
    def enable_xformers_memory_efficient_attention(self, *a, **k):
        return self     # the HIP flash kernels ARE the memory-efficient path (inference_img.py:85)

    def disable_xformers_memory_efficient_attention(self):
        return self

    def set_use_memory_efficient_attention_xformers(self, valid: bool = True):
        return self

    def set_attention_slice(self, slice_size):
        heads = self.config.attention_head_dim
        if isinstance(slice_size, int) and slice_size > heads:
            raise ValueError(f"size {slice_size} has to be smaller or equal to {heads}.")
        self._slice_size = slice_size      # attention never materialises S x S here: accepted, no effect

    def _set_gradient_checkpointing(self, module, value=False):
        pass

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """FreeU (Si et al., CVPR 2024), diffusers' name and argument order: in every resnet of up_blocks.0 (b1, s1) and up_blocks.1
        (b2, s2) the first half of the backbone's channels is scaled by b and the lowest spatial frequencies of the skip connection
        by s, in front of their concat (ops.freeu, one launch per resnet).  Inference only.  The four values live in a device buffer
        of the engine: calling this again with other values rewrites it in place and a captured step follows without a recapture;
        on <-> off selects another captured graph."""
        vals = tuple(float(v) for v in (s1, s2, b1, b2))
        for name, v in zip(("s1", "s2", "b1", "b2"), vals):
            if v != v or v in (float("inf"), float("-inf")):
                raise ValueError(f"enable_freeu: {name} = {v!r} is not finite")
        self._freeu = vals
        if self._engine is not None:
            self._engine.set_freeu(vals)
        return self

    def disable_freeu(self):
        self._freeu = None
        if self._engine is not None:
            self._engine.set_freeu(None)
        return self

    def enable_step_cache(self, interval: int = 3, branch: int = 1, order: int = 1):
        """Step caching (DeepCache, Ma et al., CVPR 2024; forecasting as in TaylorSeer, Liu et al., 2025): of a sampler's model
        evaluations every `interval`-th runs in full and keeps the feature that enters the last `branch` + 1 layers of the last up
        block; the others forecast that feature from the last full evaluations (order 0: reuse, 1: linear, 2: quadratic
        extrapolation) and run conv_in, the first `branch` layers of down_blocks.0 and those last layers only (step_cache.py, DESIGN.md
        "Step caching").  Inference only, off by default.  interval and order may change between samples without a recapture; branch
        and on <-> off select other captured graphs."""
        L = self.config.layers_per_block
        for name, v in (("interval", interval), ("branch", branch), ("order", order)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"enable_step_cache: {name} = {v!r} is not an integer")
        if interval < 2:
            raise ValueError(f"enable_step_cache: interval = {interval}: 2 or more (every interval-th evaluation runs in full)")
        if not 0 <= branch <= L:
            raise ValueError(f"enable_step_cache: branch = {branch}: 0 .. layers_per_block = {L}")
        if order not in (0, 1, 2):
            raise ValueError(f"enable_step_cache: order = {order}: 0 (reuse), 1 (linear) or 2 (quadratic) over the ring's {RING_SLOTS} slots")
        if self._shard is not None:
            raise ValueError("enable_step_cache: a sharded model (parallel.attach) keeps no step cache; detach it first")
        self._step_cache = StepCachePolicy(interval, branch, order)
        if self._engine is not None:
            self._engine.set_step_cache(int(branch))
        return self

    def disable_step_cache(self):
        self._step_cache = None
        if self._engine is not None:
            self._engine.set_step_cache(None)
        return self

    # ---- forward ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, sample: torch.Tensor, timestep: Union[torch.Tensor, float, int], context: torch.Tensor,
                cond_frame: int = 0, return_attn: bool = False, cache_phase: Optional[int] = None) -> torch.Tensor:
        """cache_phase (step caching, enable_step_cache): None = the evaluation as it always was, the cache untouched; 0 = the same
        evaluation, which also keeps its cut feature; d >= 1 = a cached evaluation, d evaluations after the last full one."""
        if not sample.is_cuda and self._ops_backend is hip_ops:
            raise hip_ops._lib.SeerHipError("SeerUNet.forward needs ROCm tensors: the HIP kernels are the only compute path")
        dt = self._dtype_of_call()
        # the caller's autocast state has said its piece (the storage type): everything below -- the host-side weight algebra of
        # prepare() included -- runs outside it (a torch matmul under autocast would hand back 16-bit biases)
        with torch.autocast(device_type=sample.device.type if sample.device.type in ("cuda", "cpu") else "cuda", enabled=False):
            return self._forward_impl(sample, timestep, context, cond_frame, return_attn, dt, cache_phase)

    def _cache_args(self, cache_phase, return_attn):
        """forward's cache_phase -> the engine's (phase, weights) keywords; the weights of a cached phase follow the policy and the
        engine's count of valid slots"""
        if self._step_cache is not None and self._shard is not None:
            raise ValueError("a sharded model (parallel.attach) keeps no step cache: call disable_step_cache(), or detach the model")
        if cache_phase is None:
            return {}
        if self._step_cache is None:
            raise ValueError("cache_phase: step caching is off (enable_step_cache)")
        if return_attn:
            raise ValueError("cache_phase with return_attn: the attention maps of the skipped blocks do not exist")
        d = int(cache_phase)
        if d < 0:
            raise ValueError(f"cache_phase = {cache_phase}: None, 0 (full, keep the feature) or d >= 1 (cached)")
        if d == 0:
            return {"cache_phase": 0}
        if self._engine.cache_valid < 1:
            raise ValueError(f"cache_phase = {d}: no full evaluation (cache_phase=0) has filled the cache since it was reset")
        return {"cache_phase": d, "cache_weights": self._step_cache.weights(d, self._engine.cache_valid)}

    def _forward_impl(self, sample, timestep, context, cond_frame, return_attn, dt, cache_phase=None):
        if self._engine is None or self._engine.device != sample.device or self._engine.dt != dt:
            self.prepare(dt)
        cache = self._cache_args(cache_phase, return_attn)
        if self.config.center_input_sample:
            sample = 2 * sample - 1.0
        t = timestep
        if not torch.is_tensor(t):
            t = torch.tensor([t], dtype=torch.long, device=sample.device)
        elif t.dim() == 0:
            t = t[None].to(sample.device)
        t = t.to(torch.long).broadcast_to((sample.shape[0],)).contiguous()
        if return_attn:
            # (out, attn_list): the text cross-attention scores of the last text block of every attention-bearing container
            # (unet_3d_condition.py:291-292,317-323,372-374) -- an analysis path: eager launches, one process
            if self._shard is not None:
                raise NotImplementedError("return_attn is not available on a sharded model")
            out, attn = self._engine.run(sample.float().contiguous(), t, context, int(cond_frame), return_attn=True)
            return out.to(sample.dtype), [a.to(sample.dtype) for a in attn]
        if self._shard is None:
            out = self._engine.run(sample.float().contiguous(), t, context, int(cond_frame), use_graph=self.use_graph, **cache)
            return out.to(sample.dtype)
        # sharded step: every rank holds the full inputs, computes its (batch rows, frames) block, all ranks get the full eps
        sh = self._shard
        B, _, Fr = sample.shape[:3]
        if context.dim() == 3:
            context = context[:, None].expand(-1, Fr, -1, -1)
        (b0, b1), (f0, f1) = sh.plan(B, Fr)
        sh.probe_frame_group(sample.device)
        key = (context.data_ptr(), context._version, tuple(context.shape), b0, b1, f0, f1)
        if self._ctx_slice is None or self._ctx_slice[0] != key:
            # the keyed tensor is kept alive with the slice: a recycled address must not look like the same context
            self._ctx_slice = (key, context[b0:b1, f0:f1].contiguous(), context)
        local = self._engine.run(sample[b0:b1, :, f0:f1].float().contiguous(), t[b0:b1].contiguous(),
                                 self._ctx_slice[1], int(cond_frame), use_graph=self.use_graph)
        return sh.gather_output(local, B, Fr).to(sample.dtype)


# =====================================================================================================================
FX_MAX_ROWS = 100_000        # rows at the finest level up to which the LayerNorms are folded (_LaunchPlan.ln_on)
FX_MAX_ROWS_PB = int(os.environ.get("SEER_FX_MAX_ROWS_PB", "4096"))        # rows per batch element up to which a GroupNorm's statistics are accumulated in fixed point (_LaunchPlan.colsum_batch)


def _switch(model, attr: str, env: Optional[str] = None, default: bool = True) -> bool:
    """an engine switch: the model's attribute if it is set, else the environment variable if the switch has one, else `default`
    (a switch that is on by default is turned off by "0", one that is off by default is turned on by "1")"""
    on = getattr(model, attr, None)
    if on is not None:
        return bool(on)
    val = os.environ.get(env) if env is not None else None
    return default if val is None else (val != "0" if default else val == "1")


def _tiled(name):
    """method of _InvariantOps: the backend's `name` with the layout-invariant tile request unless the caller names a tile"""
    def call(self, *a, **k):
        k.setdefault("tile", self.TILE)
        return getattr(self._ops, name)(*a, **k)
    call.__name__ = name
    return call


class _InvariantOps:
    """an ops backend as the layout-invariant engine calls it: every launch of the GEMM family goes out with SEER_TILE_AUTO_INVARIANT
    (a plan that does not look at the rows of the call or at the device, include/seer_hip.h), and the d = 40 attention kernel's
    query-block form -- which AUTO picks by the workgroups of the call -- is pinned to the 32-query form.  Everything else is the
    backend's own."""
    TILE = _lib.SEER_TILE_AUTO_INVARIANT

    def __init__(self, ops):
        self._ops = ops

    def __getattr__(self, name):
        return getattr(self._ops, name)

    gemm, gemm_batched, conv3x3 = _tiled("gemm"), _tiled("gemm_batched"), _tiled("conv3x3")
    conv_up2x, conv_out = _tiled("conv_up2x"), _tiled("conv_out")

    def attention(self, q, k, v, out, **kw):
        # (IEEE-half operands always run the tracked form; key sequences under 256 the generic kernel: neither looks at the batch)
        if kw.get("head_dim") == 40 and q.dtype == bf16 and kw.get("Sk", 0) >= 256:
            kw.setdefault("variant", 3)
        return self._ops.attention(q, k, v, out, **kw)


def fx_arena(ops, sample, need: int, arena, retired: list):
    """the ops.FxArena of one evaluation, zeroed: `arena` where it holds `need` int64 elements, else a new one -- the old one joins
    `retired` (captured steps of smaller shapes keep adding into theirs by address).  reset() = one fill over what the last
    evaluation took."""
    if arena is None or arena.buf.numel() < need:
        assert not (sample.is_cuda and torch.cuda.is_current_stream_capturing()), \
            "the accumulator arena must exist before a graph capture"
        if arena is not None:
            retired.append(arena)
        arena = ops.FxArena(sample.device, need)
    arena.reset()
    return arena


class Step(NamedTuple):
    kind: str               # resnet | text | temporal | push | down | up | gn_out; in a step-caching walk also cache_push | cache_forecast
    name: str = ""          # the module's path (down / up: the conv's)
    skip: bool = False      # resnet: takes the skip connection pushed last (unet_3d_blocks.py:596,712)
    feeds: bool = False     # resnet: a transformer follows -- the output's only GroupNorm is that transformer's


def block_sequence(boc, lpb):
    """THE block sequence of the UNet (unet_3d_condition.py:283-376), written once: the steps behind conv_in, in order.  _Engine walks
    it (whole, or the selection of a cached evaluation: _Engine._steps), SeerTrainer._unet_fwd walks it onto its tape; the text blocks,
    the GroupNorm count and the attention maps wanted are filters over it."""
    n = len(boc)

    def layer(p, j, skip, attn):
        yield Step("resnet", f"{p}.resnets.{j}", skip, attn)
        if attn:
            yield Step("text", f"{p}.attentions.{j}")
            yield Step("temporal", f"{p}.temporal_attentions.{j}")
    for i in range(n):
        for j in range(lpb):
            yield from layer(f"down_blocks.{i}", j, False, i < n - 1)
            yield Step("push")
        if i < n - 1:
            yield Step("down", f"down_blocks.{i}.downsamplers.0.conv")
            yield Step("push")
    yield from layer("mid_block", 0, False, True)
    yield Step("resnet", "mid_block.resnets.1")
    for i in range(n):
        for j in range(lpb + 1):
            yield from layer(f"up_blocks.{i}", j, True, i > 0)
        if i < n - 1:
            yield Step("up", f"up_blocks.{i}.upsamplers.0.conv")
    yield Step("gn_out", "conv_norm_out")


class _LaunchPlan:
    """the launch forms of ONE evaluation, decided once (at the top of _Engine._forward: nothing has been launched) and read by
    the block functions.  The mode is read HERE and nowhere below: a layout-invariant engine decides by _one_element_all_frames, every
    other by _rows_of_the_call.  The answers per (form, channel width, rows per batch element) are memoised: the producer of a tensor
    and its consumer read ONE answer.  Whether _pack made a block's fused weights stays with the blocks."""

    def __init__(self, eng, B, Fr, H, W, cond_frame):
        ops, sh = eng.ops, eng.shard
        self.ops, self.B, self.shard = ops, B, sh
        self.exact = eng.inv                    # GroupNorm statistics: exact integer sums of the stored activations (no producer sums)
        self._rule = self._one_element_all_frames if eng.inv else self._rows_of_the_call
        self._widths = {"chain": ops.ROWCHAIN_C, "chain2": ops.ROWCHAIN_C} if eng.rowchain else {}
        self._widths["ff_fused"] = getattr(ops, "FF_FUSED_C", -1)
        self._sums = eng.gn_colsums and not eng.inv
        self._memo: Dict[Tuple, bool] = {}
        self.arena = None                       # the evaluation's ops.FxArena while the GroupNorm sums are accumulated (_forward)
        # the folded LayerNorm trades a launch per norm for atomics in proportion to the rows: ahead up to ~100 k rows at the finest
        # level (config 2: 24 576 rows -0.19 ms; 64x64 latent, 98 304 rows: even; bridge, 131 072 rows: +0.15 ms --
        # profiles/r04_fx_ln_other_configs.log), off above
        self.ln_on = eng.ln_fold and (self._all_frames(Fr * H * W) if eng.inv else B * Fr * H * W) <= FX_MAX_ROWS
        self.fx_gn = bool((eng.gn_fx and eng.gn_colsums) or eng.inv)    # (per tensor: colsum_batch; frame shards all-reduce the integer sums: FrameShard.reduce_fx)
        # the temporal feed-forward skips the conditioning frames (attention.py:241-246).  ff_whole: every local row takes it, so it
        # runs in its folded / fused forms.  Layout-invariant engines decide on the CLIP's conditioning frames: a frame shard that
        # holds none of them must run the form the unsharded clip runs on those frames
        self.skip_frames = cond_frame if sh is None else sh.local_cond_frames(cond_frame)
        self.ff_whole = self.skip_frames <= 0 and not (eng.inv and cond_frame > 0)
        # every level's chain is asked now: a clip sharded too finely is refused before the first launch of the evaluation
        for C in eng.boc:
            self.runs("chain", C, Fr * H * W)
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1

    def _rows_of_the_call(self, form, rows_pb):
        """THE DEFAULT RULE: the rows of the call (B elements of this rank's frames) and the device's compute units.  Frame shards
        exchange the GroupNorm statistics between the two steps and keep the separate launches in front of q|k|v (batch groups alone run
        the single-process forms)."""
        ops, rows = self.ops, self.B * rows_pb
        if form == "chain":
            return (self.shard is None or not self.shard.exact_stats) and rows_pb >= ops.ROWCHAIN_ROWS and ops.rowchain_pays(rows)
        return ops.rowchain_pays(rows, products=2) if form == "chain2" else ops.ff_fused_pays(rows)

    def _all_frames(self, rows_pb):
        """rows per batch element over ALL frames of the clip (a frame shard holds local_frames of total_frames)"""
        sh = self.shard
        return rows_pb if sh is None or not sh.local_frames else rows_pb // sh.local_frames * sh.total_frames

    def _one_element_all_frames(self, form, rows_pb):
        """THE LAYOUT-INVARIANT RULE: ONE batch element over all its frames -- half of ops.FF_FUSED_MIN_ROWS, the rows from which a CFG
        pair takes the row-owner launches by default -- and nothing else: not the batch, not the shard's share, not the device."""
        ops, sh = self.ops, self.shard
        ok = self._all_frames(rows_pb) >= ops.FF_FUSED_MIN_ROWS // 2
        if form == "chain":         # (it reads exact sums, exchanged between frame shards first: _Engine._rc_in)
            ok = ok and hasattr(ops, "groupnorm_stats_fx")
            if ok and sh is not None and sh.local_frames:
                # the launch needs ROWCHAIN_ROWS rows of a batch element on EVERY rank; falling back on one of them would give other
                # bits than the unsharded clip.  Decided from the shard table every rank holds, before any launch: all refuse together
                least = rows_pb // sh.local_frames * min(sh.frame_counts)
                if least < ops.ROWCHAIN_ROWS:
                    raise RuntimeError(f"layout_invariant: {least} rows per batch element on the smallest of {len(sh.frame_counts)} frame "
                                       f"shards, the GroupNorm -> q|k|v launch needs {ops.ROWCHAIN_ROWS}: use fewer frame shards")
        return ok

    def runs(self, form, C, rows_pb):
        """does `form` run over [B * rows_pb, C]?  "chain": GroupNorm -> proj_in -> norm1 -> q|k|v as one launch (ops.rowchain) -- read by
        the consumer (_rc_in) and by the PRODUCER of its input, which then accumulates the column sums whatever the tensor's size
        (colsum_batch(feeds=)): the chain reads them directly and the statistics launch in front of it goes too; "chain2": behind a
        chain that ran, attn1.to_out + residual -> norm2 -> attn2.to_q as one launch; "ff_fused": the feed-forward + proj_out of a block
        that has the weights as the fused launch (ops.ff_fused)"""
        key = (form, C, rows_pb)
        if key not in self._memo:
            self._memo[key] = bool(C == self._widths.get(form) and self._rule(form, rows_pb))
        return self._memo[key]

    def colsum_batch(self, rows_pb, feeds=None):
        """`colsum_batch` of a launch whose output (rows_pb rows per batch element) feeds a GroupNorm: (B, arena) = accumulate in
        fixed point, B = per-tile sums, 0 = none.  feeds: the width of the transformer whose GroupNorm is the output's only one --
        accumulated where that one runs as a chain.  The accumulated form wins where the tensor is small (its apply launch owns slices
        of 64..128 channels: 160-byte pieces of a 640-byte row at the 32x32 level, ~20 % below the full-row kernel's bandwidth, and
        eight replicas to add per block): from the 16x16 level down 7.5 / 9.6 / 5.7 / 3.8 us against 8.4 / 12.1 / 7.6 / 5.7 for
        finalize + apply, at the 32x32 level 12.6 / 27.9 against 11.3 / 25.6 (profiles/r04_gn_fx_by_level.log)."""
        if not self._sums:
            return 0
        fx = self.arena is not None and (rows_pb <= FX_MAX_ROWS_PB or (feeds is not None and self.runs("chain", feeds, rows_pb)))
        return (self.B, self.arena) if fx else self.B


class _Engine:
    """packed weights + the kernel schedule of one SeerUNet forward."""

    def __init__(self, model: SeerUNet, ops=hip_ops, shard=None, fold_ln=True, dtype=bf16):
        self.ops = ops
        self.dt = dtype                 # 16-bit storage type of activations and packed weights (bf16, or IEEE half under fp16 autocast)
        self.cfg = model.config
        self.shard = shard              # parallel.FrameShard or None
        p0 = next(model.parameters())
        self.device = p0.device
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        self.boc = tuple(self.cfg.block_out_channels)
        self.lpb = self.cfg.layers_per_block
        self.heads = self.cfg.attention_head_dim
        self.G = self.cfg.norm_num_groups
        self.seq: Tuple[Step, ...] = tuple(block_sequence(self.boc, self.lpb))
        self.eps = self.cfg.norm_eps
        # The switches, resolved here and nowhere else (_switch: the model's attribute if set, else the environment variable, else
        # on), each with what it needs.  A/B runs and the tests run the older forms through them.
        # gn_colsums, gn_fused, gn_fx: GroupNorm statistics from the column sums the producers leave (per tile; derived inside the
        #   apply launch; accumulated in fixed point by the producers) instead of a pass over the activations: groupnorm.py
        # ln_fold:    LayerNorm folded into the consuming GEMM: the producers of the residual stream leave per-row (sum, sum of
        #   squares) next to it (ops.RowStats), the q|k|v / to_q / ff.net.0 GEMMs normalise in their epilogue -- no LayerNorm launch
        #   (fold_ln=False: the trainer's engine -- its weights move, it runs its own forward)
        # ff_fold:    ff.net.2 and proj_out as one two-source GEMM (off: two launches; see _pack)
        # ff_fused:   ... and, at 320 channels, the whole feed-forward with it as ONE launch
        # rowchain:   the row-local chains in front of the attention launches at 320 channels -- GroupNorm -> proj_in -> norm1 ->
        #   q|k|v, and attn1.to_out + residual -> norm2 -> attn2.to_q -- as ONE launch each (ops.rowchain, csrc/rowchain.hip)
        # ff_pre:     ... and the block's last to_out + residual as a prologue of the fused feed-forward
        self.gn_colsums = _switch(model, "gn_colsums")
        self.gn_fused = _switch(model, "gn_fused", "SEER_GN_FUSED")
        self.gn_fx = _switch(model, "gn_fx", "SEER_GN_FX")
        self.ln_fold = bool(fold_ln) and _switch(model, "ln_fold", "SEER_LN_FOLD") and hasattr(self.ops, "fold_layernorm")
        self.ff_fold = _switch(model, "ff_fold", "SEER_FF_FOLD")
        self.ff_fused = self.ff_fold and _switch(model, "ff_fused", "SEER_FF_FUSED")
        self.rowchain = _switch(model, "rowchain", "SEER_ROWCHAIN") and hasattr(self.ops, "rowchain")
        self.ff_pre = self.rowchain and self.ff_fused and _switch(model, "ff_pre", "SEER_FF_PRE")
        # layout_invariant (OFF unless asked for): every choice below that looks at the rows of the call, at the device or at the shard
        #   layout is made per batch element on the clip's whole frame count instead -- the invariant GEMM plan and the pinned attention
        #   form (_InvariantOps), exact integer GroupNorm statistics from the stored activations (no producer sums: their float partials
        #   follow the tiles), the 320-channel launches by _LaunchPlan._one_element_all_frames.  Same bits for any batch, CFG layout or shard layout; slower.
        #   (fold_ln=False: the trainer's engine ignores it, as it ignores ln_fold)
        self.inv = bool(fold_ln) and _switch(model, "layout_invariant", "SEER_LAYOUT_INVARIANT", default=False)
        if self.inv:
            self.ops = _InvariantOps(ops)
        self._fx_arena = None
        self._fx_retired: List[object] = []
        self._plan: Optional[_LaunchPlan] = None    # the launch forms of the running evaluation (_forward)
        self.ln_folded = 0
        self.rowchains = 0
        self._ffpre_bias: Dict[str, str] = {}
        self.gn_from_colsums = 0
        self.w: Dict[str, torch.Tensor] = {}
        self._pack(sd)
        self._rot_cache: Dict[Tuple, torch.Tensor] = {}
        self._kv_cache: Dict[str, torch.Tensor] = {}
        self._kv_key = None
        self._graphs: Dict[Tuple, object] = {}     # captured steps (whole-step graphs and sampler-step graphs), LRU: see graph_get / graph_put
        self._rec = None                # _SegmentRecorder while a segmented capture is running
        self._attn_list = None          # list that collects the text cross-attention scores of a return_attn forward
        # ... of the last text block of each container: the reference's containers overwrite attn_map layer by layer
        self._attn_wanted = set({st.name.rsplit(".", 1)[0]: st.name for st in self.seq if st.kind == "text"}.values())
        self.freeu_on = False           # FreeU (SeerUNet.enable_freeu): set_freeu
        self._freeu_buf = None          # fp32 (b1, s1, b2, s2) on the device, read by the seer_freeu launches
        self.cache_branch = None        # step caching (SeerUNet.enable_step_cache): the branch while it is on, set_step_cache
        self._cache_sets: Dict[Tuple[int, int], Dict[str, torch.Tensor]] = {}   # (rows, branch) -> ring, forecast and weight buffers
        self._cache_cur = None          # the set the last phase went to
        self.cache_valid = 0            # slots of that set's ring that hold a feature of the running chain

    # ---- step caching ---------------------------------------------------------------------------------------------------
    def set_step_cache(self, branch) -> None:
        """branch = 0 .. layers_per_block turns step caching on, None off.  Another branch is another cut: the count of valid slots
        starts over.  The buffer sets stay: captured graphs read them by address."""
        if branch != self.cache_branch:
            self.cache_valid = 0
        self.cache_branch = branch

    @property
    def step_cache_key(self) -> Tuple:
        """what step caching adds to the key of a captured sampler step: nothing while it is off, ("cache", branch) while it is on --
        interval and order are host policy and no part of it"""
        return () if self.cache_branch is None else ("cache", self.cache_branch)

    def cache_set(self, rows: int) -> Dict[str, torch.Tensor]:
        """the static buffers of the cut feature [rows, C] at the current branch, made on first use -- before any capture, like
        fx_arena: `ring` [3, n] (slot 0 the newest), `fc` [rows, C] the forecast, `w` fp32 [3] its weights on the device.  C is
        boc[0], the width of level 0 -- except at branch = layers_per_block, where the cut feature is the last upsampler's output and
        has the width of level 1"""
        key = (int(rows), self.cache_branch)
        S = self._cache_sets.get(key)
        if S is None:
            assert not (self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()), \
                "the step cache's buffers must exist before a graph capture"
            C = self.boc[1 if self.cache_branch == self.lpb else 0]
            n = (rows * C + 7) // 8 * 8          # a slot keeps 16-byte alignment
            S = dict(ring=torch.zeros((RING_SLOTS, n), device=self.device, dtype=self.dt),
                     fc=torch.zeros((rows, C), device=self.device, dtype=self.dt),
                     w=torch.tensor([1.0, 0.0, 0.0], dtype=torch.float32).to(self.device))
            self._cache_sets[key] = S
        return S

    def cache_begin(self) -> None:
        """a sampler begins a chain: nothing an earlier chain left in a ring is read"""
        self.cache_valid = 0

    def cache_note(self, rows: int, phase: int, weights=None) -> None:
        """the host's half of one evaluation with a phase, launched or replayed: the count of valid slots (reset when the feature's
        shape or the branch is not the last evaluation's), the refusal of a cold cached phase, and the weights of a cached one written
        into the set's device buffer -- the only host write of such a step"""
        if self.cache_branch is None:
            raise ValueError("cache_phase: step caching is off (SeerUNet.enable_step_cache)")
        S = self.cache_set(rows)
        if self._cache_cur is not S:
            self._cache_cur, self.cache_valid = S, 0
        if phase == 0:
            self.cache_valid = min(self.cache_valid + 1, RING_SLOTS)
            return
        if self.cache_valid < 1:
            raise ValueError(f"cache_phase = {phase}: no full evaluation (cache_phase=0) of this shape and branch has filled the cache "
                             "since it was reset")
        if weights is None or len(weights) != RING_SLOTS:
            raise ValueError(f"cache_phase = {phase}: a cached evaluation needs its {RING_SLOTS} forecast weights")
        S["w"].copy_(torch.tensor([float(v) for v in weights], dtype=torch.float32))

    # ---- FreeU ----------------------------------------------------------------------------------------------------------
    def set_freeu(self, vals) -> None:
        """vals = (s1, s2, b1, b2) turns FreeU on, None off.  The device buffer is made once and REWRITTEN in place afterwards: the
        captured steps read it by address."""
        self.freeu_on = vals is not None
        if vals is None:
            return
        s1, s2, b1, b2 = vals
        host = torch.tensor([b1, s1, b2, s2], dtype=torch.float32)
        if self._freeu_buf is None:
            self._freeu_buf = host.to(self.device)
        else:
            self._freeu_buf.copy_(host)

    @property
    def freeu_key(self) -> Tuple:
        """what FreeU adds to the key of a captured step: nothing while it is off (the keys are what they were), one word while it
        is on -- the values are no part of it"""
        return ("freeu",) if self.freeu_on else ()

    def _freeu_params(self, p):
        """the (b, s) pair of resnet `p` on the device, or None: FreeU is off, or `p` is outside up_blocks.0 / up_blocks.1"""
        if not self.freeu_on:
            return None
        if p.startswith("up_blocks.0."):
            return self._freeu_buf[0:2]
        return self._freeu_buf[2:4] if p.startswith("up_blocks.1.") else None

    # ---- captured graphs: ONE cache, ONE eviction policy ------------------------------------------------------------
    # Every entry owns a private graph memory pool with a full set of step activations, so the cache is small and evicts the
    # single least-recently-used entry (dict order = recency), never everything at once.
    MAX_GRAPHS = 6

    def graph_get(self, key):
        g = self._graphs.get(key)
        if g is not None:
            self._graphs[key] = self._graphs.pop(key)          # most recently used last
        return g

    def graph_put(self, key, g) -> None:
        self._graphs.pop(key, None)
        while len(self._graphs) >= self.MAX_GRAPHS:
            self._graphs.pop(next(iter(self._graphs)))         # the least recently used one
        self._graphs[key] = g

    # ---- weight packing ---------------------------------------------------------------------------------------
    def _pack(self, sd):
        w = self.w
        dev = self.device
        f32 = lambda t: t.to(dev, torch.float32).contiguous()
        b16 = lambda t: t.to(dev, torch.float32).to(self.dt).contiguous()
        self.resnets: List[str] = []
        self.temb_slices: Dict[str, Tuple[int, int]] = {}
        temb_w, temb_b, off = [], [], 0
        for k in sd:
            if k.endswith(".time_emb_proj.weight"):
                p = k[: -len(".time_emb_proj.weight")]
                n = sd[k].shape[0]
                self.temb_slices[p] = (off, n)
                temb_w.append(sd[k]); temb_b.append(sd[p + ".time_emb_proj.bias"])
                off += n
        w["temb_all.w"] = b16(torch.cat(temb_w, 0))
        w["temb_all.b"] = f32(torch.cat(temb_b, 0))
        for k, v in sd.items():
            if ".time_emb_proj." in k or k.endswith("rotary_emb.freqs"):
                if k.endswith("rotary_emb.freqs"):
                    w[k] = f32(v)
                continue
            if k in ("conv_in.weight",):
                w[k] = f32(v.permute(2, 3, 1, 0))                       # [3,3,Cin,Cout]
            elif k in ("conv_out.weight",):
                if v.shape[0] % 4 == 0:
                    w[k] = b16(pack_conv3x3(v))                         # [Cout, 9*C0]: MFMA implicit GEMM, transposed store
                else:
                    w[k] = f32(v.permute(0, 2, 3, 1))                   # [Cout,3,3,C0]: direct kernel
            elif k.endswith(".weight") and v.dim() == 4:
                w[k] = b16(pack_conv3x3(v) if v.shape[-1] == 3 else pack_conv1x1(v))
                if ".upsamplers." in k:
                    # the conv behind the nearest-2x upsample as four 2x2 phase convs (16 instead of 36 tap-products per
                    # source pixel); the 9-tap form stays for the fine-tuning backward (trainer.py)
                    w[k + "_up4"] = b16(pack_conv3x3_up_phases(v.to(torch.float32)))
            elif k.endswith(".weight") and v.dim() == 2:
                if k.endswith("ff.net.0.proj.weight"):
                    order = geglu_row_order(v.shape[0] // 2)
                    w[k] = b16(v[order])
                    w[k[:-6] + "bias"] = f32(sd[k[:-6] + "bias"][order])
                elif k.endswith((".to_q.weight", ".to_k.weight", ".to_v.weight")):
                    continue                                             # fused below
                else:
                    w[k] = b16(v)
            elif k.endswith("ff.net.0.proj.bias"):
                continue
            else:
                w[k] = f32(v)                                            # biases, norm affine
        for k in sd:
            if k.endswith(".attn1.to_q.weight"):
                p = k[: -len(".to_q.weight")]
                w[p + ".qkv"] = b16(torch.cat([sd[p + ".to_q.weight"], sd[p + ".to_k.weight"], sd[p + ".to_v.weight"]], 0))
            elif k.endswith(".attn2.to_q.weight"):
                p = k[: -len(".to_q.weight")]
                w[p + ".q"] = b16(sd[p + ".to_q.weight"])
                w[p + ".kv"] = b16(torch.cat([sd[p + ".to_k.weight"], sd[p + ".to_v.weight"]], 0))
        # ff.net.2 followed by proj_out (attention.py:742-747 then :126,141-145): two consecutive LINEAR maps with only the residual
        # add of the block between them -- x + proj_out(h + ff2(g)) = x + [Wp | Wp W2] [h | g] + (Wp b2 + bp) -- run as ONE two-source
        # GEMM over K = C + 4C (the same FLOPs: the second map's K = C rides in the first one's K loop).  The product Wp W2 is formed
        # once, in fp32, from the fp32 weights.  One launch and one round trip of the block's residual stream fewer per transformer
        # block, 32 per step.  The plain weights stay (row subsets under cond_frame > 0, return_attn, the training engine).
        if self.ff_fold:
            for k in sd:
                if not k.endswith(".proj_out.weight") or (".attentions." not in k and ".temporal_attentions." not in k):
                    continue
                pth = k[: -len(".proj_out.weight")]
                tb = pth + ".transformer_blocks.0"
                if (tb + ".ff.net.2.weight") not in sd:
                    continue
                wp = pack_conv1x1(sd[k]).to(dev, torch.float32)
                w2, b2 = f32(sd[tb + ".ff.net.2.weight"]), f32(sd[tb + ".ff.net.2.bias"])
                w[pth + ".ffproj.w"] = torch.cat([wp, wp @ w2], dim=1).to(self.dt).contiguous()           # [C, C + 4C]
                w[pth + ".ffproj.b"] = (wp @ b2 + f32(sd[pth + ".proj_out.bias"])).contiguous()
                # 320 channels: norm3, ff.net.0, GEGLU and this GEMM run as ONE launch (ops.ff_fused, csrc/ff_fused.hip), which reads
                # both matrices in its own fragment order
                if self.ff_fused and wp.shape[0] == getattr(self.ops, "FF_FUSED_C", -1) and (tb + ".norm3.weight") in sd:
                    w[pth + ".ff_fused.w1f"], w[pth + ".ff_fused.wcf"] = self.ops.ff_fused_pack(
                        w[tb + ".ff.net.0.proj.weight"], w[pth + ".ffproj.w"])
        # the chains of ops.rowchain read their 320 x 320 matrices in the kernel's fragment order
        if self.rowchain:
            RC = self.ops.ROWCHAIN_C
            for k in list(w):
                if k.endswith(".proj_in.weight") and w[k].shape == (RC, RC) and (k[:-len(".proj_in.weight")] + ".transformer_blocks.0.attn1.qkv") in w:
                    pth = k[: -len(".proj_in.weight")]
                    tb = pth + ".transformer_blocks.0"
                    w[pth + ".rc.proj_in"] = self.ops.rowchain_pack(w[k])
                    w[tb + ".rc.qkv"] = self.ops.rowchain_pack(w[tb + ".attn1.qkv"])
                    if (tb + ".attn2.q") in w:
                        w[tb + ".rc.to_out"] = self.ops.rowchain_pack(w[tb + ".attn1.to_out.0.weight"])
                        w[tb + ".rc.q"] = self.ops.rowchain_pack(w[tb + ".attn2.q"])
                    # the LAST to_out of the block (text: attn2, temporal: attn1) as the fused feed-forward's prologue (ops.ff_fused(pre=))
                    last = tb + (".attn2" if (tb + ".attn2.q") in w else ".attn1") + ".to_out.0"
                    if (pth + ".ff_fused.w1f") in w and self.ff_pre:
                        w[tb + ".ffpre.wo"] = self.ops.rowchain_pack(w[last + ".weight"])
                        self._ffpre_bias[tb] = last + ".bias"
        # LayerNorm folded into the GEMM that consumes it (ops.fold_layernorm): W' = gamma (.) W from the fp32 weights, its row
        # sums and beta W^T + b, next to the plain weights (a launch that cannot fold runs layernorm + the plain ones)
        self.wln: Dict[str, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        if self.ln_fold:
            fold = self.ops.fold_layernorm if self.dt == bf16 else (lambda *a: self.ops.fold_layernorm(*a, dtype=self.dt))
            for k in sd:
                if not k.endswith(".norm1.weight") or ".transformer_blocks." not in k:
                    continue
                tb = k[: -len(".norm1.weight")]
                g = lambda n: (f32(sd[f"{tb}.{n}.weight"]), f32(sd[f"{tb}.{n}.bias"]))
                qkv = torch.cat([sd[tb + ".attn1.to_q.weight"], sd[tb + ".attn1.to_k.weight"], sd[tb + ".attn1.to_v.weight"]], 0)
                self.wln[tb + ".attn1.qkv"] = fold(f32(qkv), *g("norm1"))
                if (tb + ".attn2.to_q.weight") in sd and (tb + ".norm2.weight") in sd:
                    self.wln[tb + ".attn2.q"] = fold(f32(sd[tb + ".attn2.to_q.weight"]), *g("norm2"))
                if (tb + ".norm3.weight") in sd:
                    v = sd[tb + ".ff.net.0.proj.weight"]
                    order = geglu_row_order(v.shape[0] // 2)
                    self.wln[tb + ".ff.net.0.proj.weight"] = fold(f32(v[order]), *g("norm3"), f32(sd[tb + ".ff.net.0.proj.bias"][order]))

    # ---- building blocks --------------------------------------------------------------------------------------
    def _gn(self, x1, x2, B, rows_pb, name, eps, silu):
        """GroupNorm over (C/G, F, H, W); which of its forms runs, and the cross-shard reduction: groupnorm.groupnorm"""
        self._stats_i += 1
        y, from_colsums = groupnorm(self.ops, x1, x2, B, self.G, rows_pb, eps, self.w[name + ".weight"], self.w[name + ".bias"], silu,
                                    stats=self._stats_arena[self._stats_i - 1], use_colsums=self.gn_colsums, fused=self.gn_fused,
                                    shard=self.shard, sync=self.sync_point, arena=self._plan.arena, exact=self._plan.exact)
        self.gn_from_colsums += from_colsums
        return y

    def _rc_in(self, p, tb, x, B, rows_pb, rotary, qs):
        """GroupNorm -> proj_in -> norm1 -> q|k|v of transformer `p` as one launch: (h, qkv), or None when this block / shape keeps
        the separate launches"""
        ops, w, plan = self.ops, self.w, self._plan
        if not plan.runs("chain", x.shape[1], rows_pb) or (p + ".rc.proj_in") not in w:
            return None
        if plan.exact:
            # exact integer sums of x's stored values, added over the frame shards: the statistics of the unsharded clip, bit for bit
            if not isinstance(getattr(x, "colsums", None), ops.ColSumsFx):
                x.colsums = ops.groupnorm_stats_fx(x, B, plan.arena)
            st, count, from_colsums = x.colsums, rows_pb * (x.shape[1] // self.G), False
            if self.shard is not None:
                count = self.shard.reduce_fx((st,), count, sync=self.sync_point)
        else:
            st, count, from_colsums = groupnorm_statistics(ops, x, B, self.G, rows_pb, stats=self._stats_arena[self._stats_i],
                                                           use_colsums=self.gn_colsums)
        r = ops.rowchain(x, w[p + ".rc.proj_in"], b1=w[p + ".proj_in.bias"],
                         gn=(st, count, 1e-6, w[p + ".norm.weight"], w[p + ".norm.bias"], rows_pb, self.G),
                         ln=(w[tb + ".norm1.weight"], w[tb + ".norm1.bias"], 1e-5), w2f=w[tb + ".rc.qkv"], col_scale=(qs, 1), rotary=rotary)
        if r is None:
            assert not plan.exact, "layout_invariant: the plan let a shape through that ops.rowchain refuses"
            return None
        self._stats_i += 1
        self.gn_from_colsums += from_colsums
        self.rowchains += 1
        return r

    def _resnet(self, p, x, skip, geo, feeds_transformer=False):
        """ResnetBlock3D (resnet.py:174-208); `skip` is the channel-concat partner of unet_3d_blocks.py:596,712.  feeds_transformer:
        the output's only GroupNorm is the next transformer's (see _LaunchPlan.runs)."""
        ops, w, plan = self.ops, self.w, self._plan
        B, Fr, H, W = geo
        rows_pb = Fr * H * W
        fu = self._freeu_params(p) if skip is not None else None
        if fu is not None:
            # FreeU, in front of everything the resnet does with its inputs: a new pair without column sums (norm1 takes its
            # statistics pass); per (frame, channel), so batch, CFG and frame-shard layouts are untouched
            x, skip = ops.freeu(x, skip, fu, H, W)
        h = self._gn(x, skip, B, rows_pb, p + ".norm1", self.eps, True)
        off, n = self.temb_slices[p]
        temb = self._temb[:, off:off + n]
        # (outputs that feed a GroupNorm leave their column sums behind)
        h = ops.conv3x3(h, w[p + ".conv1.weight"], B * Fr, H, W, bias=w[p + ".conv1.bias"], rowvec=temb,
                        rows_per_batch=rows_pb, colsum_batch=plan.colsum_batch(rows_pb))
        h = self._gn(h, None, B, rows_pb, p + ".norm2", self.eps, True)
        if (p + ".conv_shortcut.weight") in w:
            sc = ops.gemm(x, w[p + ".conv_shortcut.weight"], a2=skip, bias=w[p + ".conv_shortcut.bias"])
        else:
            assert skip is None
            sc = x
        w2 = w[p + ".conv2.weight"]
        return ops.conv3x3(h, w2, B * Fr, H, W, bias=w[p + ".conv2.bias"], residual=sc,
                           colsum_batch=plan.colsum_batch(rows_pb, feeds=w2.shape[0] if feeds_transformer else None))

    def _ln_gemm(self, h, tb, norm, wkey, bias_key=None, **kw):
        """LayerNorm `tb + norm` followed by the projection `wkey`: one GEMM when the producer of h left its row statistics and the
        launch can fold (ops.gemm(..., ln=)), else the layernorm kernel and the plain weights."""
        ops, w = self.ops, self.w
        rs = getattr(h, "rowstats", None)
        f = self.wln.get(wkey) if rs is not None else None
        if f is not None:
            y = ops.gemm(h, f[0], bias=f[2], ln=(rs, f[1], 1e-5), **kw)
            if y is not None:
                self.ln_folded += 1
                return y
        n = ops.layernorm(h, w[tb + norm + ".weight"], w[tb + norm + ".bias"])
        return ops.gemm(n, w[wkey], bias=(w[bias_key] if bias_key else None), **kw)

    def _rs(self):
        """extra arguments of a GEMM whose output rows feed a LayerNorm"""
        return {"rowstat": self._fx_arena if self._fx_arena is not None else True} if self._plan.ln_on else {}

    def _ff(self, tb, h_rows):
        ops, w = self.ops, self.w
        g = self._ln_gemm(h_rows, tb, ".norm3", tb + ".ff.net.0.proj.weight", tb + ".ff.net.0.proj.bias", geglu=True)
        ops.gemm(g, w[tb + ".ff.net.2.weight"], bias=w[tb + ".ff.net.2.bias"], residual=h_rows, out=h_rows)

    def _ff_forms(self, p, tb, C, rows_pb):
        """(fused, pre) of transformer `p` over all its rows: will _ff_proj_out run its feed-forward as the fused launch, and will the
        block's last to_out + residual ride in that launch (ops.ff_fused(pre=))?  The block's weights (_pack) and the plan"""
        fused = (p + ".ff_fused.w1f") in self.w and self._plan.runs("ff_fused", C, rows_pb)
        return fused, fused and (tb + ".ffpre.wo") in self.w

    def _ff_proj_out(self, p, tb, h, x, cb, fused, a=None):
        """the feed-forward of block `tb` and the transformer's proj_out + residual x: the fused launch where _ff_forms said so, else
        folded into one two-source GEMM when the block's weights were (see _pack), else ff.net.2 + residual and proj_out + residual
        as two launches.  `a` (only with _ff_forms' pre): the attention output whose to_out projection + residual h the fused launch
        computes itself."""
        ops, w = self.ops, self.w
        if fused:
            pre = None if a is None else (a, w[tb + ".ffpre.wo"], w[self._ffpre_bias[tb]])
            y = ops.ff_fused(h, x, w[tb + ".norm3.weight"], w[tb + ".norm3.bias"], w[p + ".ff_fused.w1f"],
                             w[tb + ".ff.net.0.proj.bias"], w[p + ".ff_fused.wcf"], w[p + ".ffproj.b"], colsum_batch=cb, pre=pre)
            if y is not None:
                return y
        assert a is None, "the to_out prologue exists only inside the fused feed-forward launch"
        if (p + ".ffproj.w") in w:
            g = self._ln_gemm(h, tb, ".norm3", tb + ".ff.net.0.proj.weight", tb + ".ff.net.0.proj.bias", geglu=True)
            return ops.gemm(h, w[p + ".ffproj.w"], a2=g, bias=w[p + ".ffproj.b"], residual=x, colsum_batch=cb)
        self._ff(tb, h)
        return ops.gemm(h, w[p + ".proj_out.weight"], bias=w[p + ".proj_out.bias"], residual=x, colsum_batch=cb)

    def _text_transformer(self, p, x, geo):
        """SpatialTransformer3D + BasicTextTransformerBlock3D (attention.py:129-145, 308-327)."""
        ops, w, plan = self.ops, self.w, self._plan
        B, Fr, H, W = geo
        C = x.shape[1]
        heads, d = self.heads, C // self.heads
        HW = H * W
        tb = p + ".transformer_blocks.0"
        fused, pre = self._ff_forms(p, tb, C, Fr * HW)
        # the q columns leave the projection as q * scale * log2(e) (one bf16 rounding): the attention kernels exponentiate
        # the raw dot products
        qs = ops.qk_prescale(d)
        rc = self._rc_in(p, tb, x, B, Fr * HW, None, qs)
        if rc is not None:
            h, qkv = rc
        else:
            hn = self._gn(x, None, B, Fr * HW, p + ".norm", 1e-6, False)
            h = ops.gemm(hn, w[p + ".proj_in.weight"], bias=w[p + ".proj_in.bias"], **self._rs())
            qkv = self._ln_gemm(h, tb, ".norm1", tb + ".attn1.qkv", col_scale=(qs, C))
        # self attention per frame
        a = torch.empty_like(h)
        ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], a, batch=B * Fr, heads=heads, head_dim=d,
                      Sq=HW, Sk=HW, q_prescaled=True)
        # text cross attention per frame (K/V depend on the context only: cached across DDIM steps)
        q = None
        if rc is not None and (tb + ".rc.q") in w and plan.runs("chain2", C, Fr * HW):
            # attn1.to_out + residual (over h) -> norm2 -> attn2.to_q, one launch
            r2 = ops.rowchain(a, w[tb + ".rc.to_out"], b1=w[tb + ".attn1.to_out.0.bias"], res=h, h_out=h,
                              ln=(w[tb + ".norm2.weight"], w[tb + ".norm2.bias"], 1e-5), w2f=w[tb + ".rc.q"], col_scale=(qs, 1))
            if r2 is not None:
                q = r2[1]
                self.rowchains += 1
        if q is None:
            ops.gemm(a, w[tb + ".attn1.to_out.0.weight"], bias=w[tb + ".attn1.to_out.0.bias"], residual=h, out=h, **self._rs())
            q = self._ln_gemm(h, tb, ".norm2", tb + ".attn2.q", col_scale=(qs, C))
        kv = self._kv_cache.get(tb)
        if kv is None:
            kv = ops.gemm(self._ctx, w[tb + ".attn2.kv"])
            self._kv_cache[tb] = kv
        L = self._ctx_len
        if self._attn_list is not None and p in self._attn_wanted:
            self._attn_list.append(self._cross_scores(q, kv[:, :C], B, Fr, H, W, heads, d, L))
        ops.attention(q, kv[:, :C], kv[:, C:], a, batch=B * Fr, heads=heads, head_dim=d, Sq=HW, Sk=L, q_prescaled=True)
        # (the output's only GroupNorm is the temporal transformer's: accumulated sums when that one runs as a chain)
        cb = plan.colsum_batch(Fr * HW, feeds=C)
        if pre:
            return self._ff_proj_out(p, tb, h, x, cb, fused, a=a)      # attn2.to_out + residual inside the fused feed-forward launch
        # (the fused feed-forward normalises its rows itself: no row statistics asked of their producer)
        ops.gemm(a, w[tb + ".attn2.to_out.0.weight"], bias=w[tb + ".attn2.to_out.0.bias"], residual=h, out=h,
                 **({} if fused else self._rs()))
        return self._ff_proj_out(p, tb, h, x, cb, fused)

    def _cross_scores(self, q, k, B, Fr, H, W, heads, d, L):
        """`attention_scores` of the text cross attention (attention.py:556-584: scale * Q K^T before the softmax) as
        [b, heads, f, h, w, L] (attention.py:320).  q carries scale * log2(e) (one bf16 rounding, as the attention kernel reads
        it): the scores are one batched MFMA GEMM over the head-split, zero-padded operands with 1 / log2(e) in its epilogue."""
        HW, Bt = H * W, B * Fr * heads
        dp, Lp = (d + 63) // 64 * 64, (L + 3) // 4 * 4
        qh = torch.zeros((Bt, HW, dp), device=q.device, dtype=q.dtype)
        kh = torch.zeros((Bt, Lp, dp), device=q.device, dtype=q.dtype)
        qh[:, :, :d] = q.reshape(B * Fr, HW, heads, d).permute(0, 2, 1, 3).reshape(Bt, HW, d)
        kh[:, :L, :d] = k.reshape(B * Fr, L, heads, d).permute(0, 2, 1, 3).reshape(Bt, L, d)
        s = self.ops.gemm_batched(qh, kh, out_f32=True, col_scale=(1.0 / self.ops.LOG2E, Lp))
        return s[:, :, :L].reshape(B, Fr, heads, H, W, L).permute(0, 2, 1, 3, 4, 5).contiguous()

    def _rotary_table(self, tb, T):
        freqs = self.w[tb + ".attn1.rotary_emb.freqs"]
        key = (freqs.data_ptr(), T)
        t = self._rot_cache.get(key)
        if t is None:
            fk = (tuple(freqs.tolist()), T)      # identical buffers share one table
            t = self._rot_cache.get(fk)
            if t is None:
                t = self.ops.rotary_table(freqs, T)
                self._rot_cache[fk] = t
            self._rot_cache[key] = t
        return t

    def _temporal_transformer(self, p, x, geo):
        """SpatialTransformer3D + BasicTransformerBlock3D(temporal) + WindowSTempAttention
        (attention.py:129-145, 231-248, 632-703)."""
        ops, w, plan = self.ops, self.w, self._plan
        B, Fr, H, W = geo
        C = x.shape[1]
        heads, d = self.heads, C // self.heads
        HW = H * W
        tb = p + ".transformer_blocks.0"
        F_all = Fr if self.shard is None else self.shard.total_frames
        f_off = 0 if self.shard is None else self.shard.frame_offset
        rot_dim = min(32, d)
        cs = self._rotary_table(tb, F_all * HW)
        rc = self._rc_in(p, tb, x, B, Fr * HW, (cs, Fr * HW, f_off * HW, d, rot_dim, 2), ops.qk_prescale(d))
        if rc is not None:
            h, qkv = rc
        else:
            hn = self._gn(x, None, B, Fr * HW, p + ".norm", 1e-6, False)
            h = ops.gemm(hn, w[p + ".proj_in.weight"], bias=w[p + ".proj_in.bias"], **self._rs())
            # q|k|v projection with the rotary embedding applied to the q and k columns in the GEMM epilogue
            qkv = self._ln_gemm(h, tb, ".norm1", tb + ".attn1.qkv", rotary=(cs, Fr * HW, f_off * HW, d, rot_dim, 2 * C),
                                col_scale=(ops.qk_prescale(d), C))
        a = torch.empty_like(h)
        if self.shard is not None:
            self.shard.temporal_attention(ops, qkv, a, B, heads, d, H, W, sync=self.sync_point)
        else:
            if H > MIN_WIN_SIZE:
                ws = MAX_WIN_SIZE if (H // MAX_WIN_SIZE) >= MAX_RATIO else MIN_WIN_SIZE
                ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], a, batch=B, heads=heads, head_dim=d,
                              Sq=Fr * ws * ws, Sk=Fr * ws * ws, causal=True, window=(ws, Fr, H, W), q_prescaled=True)
            else:
                ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], a, batch=B, heads=heads, head_dim=d,
                              Sq=Fr * HW, Sk=Fr * HW, causal=True, q_prescaled=True)
        # FF skips the conditioning frames (attention.py:241-246; _LaunchPlan.ff_whole); frames are the slow index inside a batch element
        skip_f, cb = plan.skip_frames, plan.colsum_batch(Fr * HW)
        fused, pre = self._ff_forms(p, tb, C, Fr * HW) if plan.ff_whole else (False, False)
        if pre:
            return self._ff_proj_out(p, tb, h, x, cb, fused, a=a)    # attn1.to_out + residual inside the fused feed-forward launch
        ops.gemm(a, w[tb + ".attn1.to_out.0.weight"], bias=w[tb + ".attn1.to_out.0.bias"], residual=h, out=h,
                 **({} if fused else self._rs()))
        if plan.ff_whole:
            return self._ff_proj_out(p, tb, h, x, cb, fused)
        elif skip_f < Fr:
            for b in range(B):
                self._ff(tb, h[b * Fr * HW + skip_f * HW:(b + 1) * Fr * HW])
        return ops.gemm(h, w[p + ".proj_out.weight"], bias=w[p + ".proj_out.bias"], residual=x, colsum_batch=cb)

    # ---- the schedule ---------------------------------------------------------------------------------------------
    def n_groupnorms(self):
        return sum({"resnet": 2, "text": 1, "temporal": 1, "gn_out": 1}.get(st.kind, 0) for st in self.seq)

    def _steps(self, cache_phase) -> Tuple[Step, ...]:
        """the steps of one evaluation (_forward): the sequence, or -- step caching -- the sequence around its cut, by position"""
        seq = self.seq
        if cache_phase is None:
            return seq
        cut = next(i for i, st in enumerate(seq) if st.name == f"up_blocks.{len(self.boc) - 1}.resnets.{self.lpb - self.cache_branch}")
        if not cache_phase:
            return seq[:cut] + (Step("cache_push"),) + seq[cut:]
        pushes = [i for i, st in enumerate(seq) if st.kind == "push"]
        head = seq[:pushes[self.cache_branch - 1] + 1] if self.cache_branch else ()
        return head + (Step("cache_forecast"),) + seq[cut:]

    def _forward(self, sample, t, ctx_bf16, ctx_len, cond_frame, return_attn=False, cache_phase=None):
        """cache_phase (step caching; the launches only -- the host's half is cache_note): None = the schedule as it always was;
        0 = the same, plus one cache_push of the cut feature, the backbone input of up_blocks.{n-1}.resnets.{lpb - branch}; d >= 1 =
        the cached walk: time embedding, conv_in, the first `branch` layers of down_blocks.0, one cache_forecast, the layers lpb -
        branch .. lpb of the last up block, conv_norm_out, conv_out (_steps)."""
        ops, w = self.ops, self.w
        B, Cin, Fr, H, W = sample.shape
        plan = self._plan = _LaunchPlan(self, B, Fr, H, W, cond_frame)          # (raises where it refuses: nothing is launched above this line)
        cache = None if cache_phase is None else self.cache_set(B * Fr * H * W)
        self._attn_list = [] if return_attn else None
        self._ctx, self._ctx_len = ctx_bf16, ctx_len
        self._stats_arena = torch.empty((self.n_groupnorms(), B, self.G, 2), device=sample.device, dtype=torch.float32)
        self._stats_i = 0
        self.gn_from_colsums = 0        # GroupNorms of this forward that took their statistics from column sums
        self.ln_folded = 0              # LayerNorms of this forward that ran inside the consuming GEMM
        self.rowchains = 0              # ops.rowchain launches of this forward
        if (plan.fx_gn or plan.ln_on) and hasattr(ops, "FxArena"):
            # fixed-point accumulators of the evaluation: a [reps, B, 2, C] slot per colsum producer, a [rows, 2] slot per producer
            # of LayerNorm rows
            need = (self.n_groupnorms() + 16) * B * 4 * max(self.boc) * 2 + 5 * 16 * B * Fr * H * W * 2
            self._fx_arena = fx_arena(ops, sample, need, self._fx_arena, self._fx_retired)
            plan.arena = self._fx_arena if plan.fx_gn else None
        emb = ops.timestep_embedding(t, self.boc[0], self.cfg.flip_sin_to_cos, self.cfg.freq_shift)
        emb = ops.linear_smallm(emb, w["time_embedding.linear_1.weight"], w["time_embedding.linear_1.bias"], silu_out=True)
        emb = ops.linear_smallm(emb, w["time_embedding.linear_2.weight"], w["time_embedding.linear_2.bias"])
        self._temb = ops.linear_smallm(emb, w["temb_all.w"], w["temb_all.b"], silu_in=True)
        # (on a side stream beside conv_in -- a fork / join in the step's graph -- this chain cost the step +0.35 ms:
        #  profiles/r06_temb_fork_rejected.log)

        x = ops.conv_in(sample, w["conv_in.weight"], w["conv_in.bias"]) if self.dt == bf16 else \
            ops.conv_in(sample, w["conv_in.weight"], w["conv_in.bias"], dtype=self.dt)
        skips = [x]
        geo = (B, Fr, H, W)
        for st in self._steps(cache_phase):
            kind = st.kind
            if kind == "resnet":
                x = self._resnet(st.name, x, skips.pop() if st.skip else None, geo, feeds_transformer=st.feeds)
            elif kind == "text":
                x = self._text_transformer(st.name, x, geo)
            elif kind == "temporal":
                x = self._temporal_transformer(st.name, x, geo)
            elif kind == "push":
                skips.append(x)
            elif kind == "down":
                Ho, Wo = (geo[2] - 1) // 2 + 1, (geo[3] - 1) // 2 + 1
                x = ops.conv3x3(x, w[st.name + ".weight"], B * Fr, geo[2], geo[3], stride=2, bias=w[st.name + ".bias"],
                                colsum_batch=plan.colsum_batch(Fr * Ho * Wo))
                geo = (B, Fr, Ho, Wo)
            elif kind == "up":
                x = ops.conv_up2x(x, w[st.name + ".weight_up4"], B * Fr, geo[2], geo[3], bias=w[st.name + ".bias"],
                                  colsum_batch=plan.colsum_batch(Fr * 4 * geo[2] * geo[3]))
                geo = (B, Fr, geo[2] * 2, geo[3] * 2)
            elif kind == "gn_out":
                x = self._gn(x, None, B, Fr * geo[2] * geo[3], st.name, self.eps, True)
            elif kind == "cache_push":
                ops.cache_push(x, cache["ring"])                # phase 0: the cut feature joins the ring; x itself is only read
            elif kind == "cache_forecast":
                # the forecast cut feature: a fresh view of the static buffer, without column sums -- norm1 takes its statistics
                # pass, as behind ops.freeu
                x = ops.cache_forecast(cache["ring"], cache["w"], cache["fc"])[:]
        out = ops.conv_out(x, w["conv_out.weight"], w["conv_out.bias"], B, Fr, geo[2], geo[3])
        if return_attn:
            attn, self._attn_list = self._attn_list, None
            return out, attn
        return out

    # ---- entry ---------------------------------------------------------------------------------------------------------
    def _context(self, context: torch.Tensor):
        """context [B, F, L, Dc] fp32 -> bf16 [B*F*L, Dc] plus the cross-attention K|V projections of the 16 text blocks, which
        depend on the context only: they run once per prompt instead of once per DDIM step.  A change is detected by the
        tensor's identity and version (the engine keeps the keyed tensor alive: a freed context's address handed to the next
        prompt must not look like a cache hit).  The bf16 context and the K|V tensors are STATIC buffers: a new prompt of the
        same shape is written into them in place, so the captured hipGraphs -- which read them by address -- stay valid and a
        new prompt costs 1 + 16 small launches, not a re-capture."""
        key = (context.data_ptr(), context._version, tuple(context.shape), context.dtype)
        if key != self._kv_key:     # (an engine is built per storage type: the cached K|V never mix types)
            c = context.reshape(-1, context.shape[-1])
            new = (self.ops.cast_bf16(c.float()) if self.dt == bf16 else self.ops.cast_bf16(c.float(), self.dt)) if c.dtype != self.dt else c
            old = getattr(self, "_ctx_bf16", None)
            if old is not None and old.shape == new.shape and self._kv_cache:
                old.copy_(new)
                for tb, kv in self._kv_cache.items():          # refresh in place, in the order the blocks first ran
                    self.ops.gemm(old, self.w[tb + ".attn2.kv"], out=kv)
            else:                                              # first prompt, or another context shape: start over
                self._ctx_bf16 = new.contiguous().clone() if new.data_ptr() == c.data_ptr() else new
                self._kv_cache = {}
                self._graphs.clear()
            self._kv_key = key
            self._kv_ctx_ref = context
        return self._ctx_bf16, context.shape[-2]

    def run(self, sample, t, context, cond_frame, use_graph=False, return_attn=False, cache_phase=None, cache_weights=None):
        """cache_phase / cache_weights: step caching (_forward, cache_note); None leaves the cache alone"""
        if cache_phase is not None and return_attn:
            raise ValueError("cache_phase with return_attn: the attention maps of the skipped blocks do not exist")
        if context.dim() == 3:      # [B, L, Dc] -> same text for every frame
            context = context[:, None].expand(-1, sample.shape[2], -1, -1)
        assert context.shape[0] == sample.shape[0] and context.shape[1] == sample.shape[2], \
            f"context {tuple(context.shape)} does not match sample {tuple(sample.shape)} (need [B, F, L, D])"
        H, W = sample.shape[-2:]
        if H % 8 or W % 8:
            raise ValueError("latent height/width must be multiples of 8 (three stride-2 levels + 4/8 windows)")
        ctx, L = self._context(context)
        if return_attn:
            return self._forward(sample, t, ctx, L, cond_frame, return_attn=True)
        if cache_phase is not None:
            if self.shard is not None:
                raise ValueError("cache_phase: a sharded engine keeps no step cache")
            B, _, Fr = sample.shape[:3]
            self.cache_note(B * Fr * H * W, cache_phase, cache_weights)
        if not use_graph or getattr(self, "_graph_broken", False):
            return self._forward(sample, t, ctx, L, cond_frame, cache_phase=cache_phase)
        return self._run_graph(sample, t, ctx, L, cond_frame, cache_phase)

    def sync_point(self, fn):
        """run `fn` -- a cross-rank exchange (all-reduce / all-gather on static buffers) -- at this point of the schedule.
        RCCL collectives are captured into the step's graph with everything else.  Backends that cannot be captured (gloo)
        get a segmented capture: the current hipGraph segment ends, `fn` is recorded as an eager replay step and the next
        segment opens."""
        rec = self._rec
        if rec is None or (self.shard is not None and self.shard.capture_collectives):
            fn()            # eager step, or an RCCL collective recorded into the graph being captured
            return
        rec.end_segment()
        fn()
        rec.steps.append(fn)
        rec.begin_segment()

    def _run_graph(self, sample, t, ctx, L, cond_frame, cache_phase=None):
        """hipGraph replay of the shape-static step: ~1.3k launches -> one graph launch, or -- frame-sharded -- one graph
        launch per stretch between two collectives (GroupNorm statistics / K|V exchanges stay eager torch.distributed
        calls on the same stream).  With a cache_phase the graph is the storing walk or the cached one of the current branch: the
        key takes that class and the branch, never the phase's number."""
        key = (tuple(sample.shape), L, cond_frame, tuple(ctx.shape), self.inv, *self.freeu_key,
               *(() if cache_phase is None else ("cached" if cache_phase else "store", self.cache_branch)))
        g = self.graph_get(key)
        if g is None:
            # warm up eagerly (fills the K/V and rotary caches, creates process groups, lets allocations settle), then capture
            s_in, t_in = sample.clone(), t.clone()
            # (the warm-up of a storing walk pushes, and the replay below pushes again: the ring is put back in between)
            ring = None if cache_phase is None else self.cache_set(sample.shape[0] * sample.shape[2] * sample.shape[3] * sample.shape[4])["ring"]
            ring_was = None if ring is None else ring.clone()
            self._forward(s_in, t_in, ctx, L, cond_frame, cache_phase=cache_phase)
            torch.cuda.synchronize()
            sharded = self.shard is not None and self.shard.world > 1
            err = None
            for attempt in range(2):
                rec = _SegmentRecorder()
                self._rec = rec
                try:
                    rec.begin_segment()
                    out = self._forward(s_in, t_in, ctx, L, cond_frame, cache_phase=cache_phase)
                    rec.end_segment()
                    err = None
                except Exception as e:      # noqa: BLE001  capture refused (driver / RCCL state)
                    rec.abort()
                    err = e
                finally:
                    self._rec = None
                if not sharded:
                    break
                # Sharded: the ranks decide TOGETHER.  While collectives are captured nothing is exchanged during capture, so a
                # rank whose capture failed has not left its peers waiting; everybody learns of the failure here and repeats
                # the capture with eager exchanges between graph segments (where a failure can only be symmetric).
                if self.shard.agree(err is None, self.device):
                    break
                if not self.shard.capture_collectives or attempt == 1:
                    raise err if err is not None else RuntimeError("hipGraph capture of the sharded step failed on another rank")
                self.shard.capture_collectives = False
                import warnings
                warnings.warn("capturing the RCCL exchanges into the step graph failed on at least one rank"
                              + (f" ({type(err).__name__}: {err})" if err is not None else "")
                              + "; all ranks fall back to eager exchanges between graph segments")
            if err is not None:             # single process: stay correct, run eagerly
                self._graph_broken = True
                import warnings
                warnings.warn(f"hipGraph capture of the denoising step failed ({type(err).__name__}: {err}); running eagerly")
                if ring is not None:
                    ring.copy_(ring_was)
                return self._forward(sample, t, ctx, L, cond_frame, cache_phase=cache_phase)
            if ring is not None:
                ring.copy_(ring_was)
            g = (rec, s_in, t_in, out)
            self.graph_put(key, g)
        rec, s_in, t_in, out = g
        s_in.copy_(sample)
        t_in.copy_(t)
        for step in rec.steps:
            step()
        # `out` is the graph's static output buffer: the caller gets its own copy (eps is only [B,4,F,h,w]); two replays of
        # one graph -- the unbatched CFG branch of p_sample_ddim calls uc then c -- must not alias each other's result
        return out.clone()


class _SegmentRecorder:
    """a step = a list of hipGraph segments (sharing one memory pool) interleaved with eager callables"""

    def __init__(self):
        self.steps = []
        self.pool = torch.cuda.graph_pool_handle()
        self._cur = None

    def begin_segment(self):
        g = torch.cuda.CUDAGraph()
        # thread_local: an RCCL watchdog thread polling its events must not invalidate this thread's capture
        ctx = torch.cuda.graph(g, pool=self.pool, capture_error_mode="thread_local")
        ctx.__enter__()
        self._cur = (g, ctx)

    def end_segment(self):
        g, ctx = self._cur
        self._cur = None
        ctx.__exit__(None, None, None)
        self.steps.append(g.replay)

    def abort(self):
        if self._cur is not None:
            g, ctx = self._cur
            self._cur = None
            try:
                ctx.__exit__(None, None, None)
            except Exception:
                pass
        self.steps = []

    @property
    def n_segments(self):
        return sum(1 for s in self.steps if getattr(s, "__self__", None).__class__ is torch.cuda.CUDAGraph)
