"""SlotSampler -- continuous batching of clips in ONE captured sampler step.

The engine is bound by fixed costs, not by its matrix units: a second clip in the same step costs a fraction of a step
("SlotSampler").  DDIMSampler cannot use that: it has one schedule index and one guidance scale for the whole batch,
the scale is frozen into the captured graph, and a batch starts and ends together.  Here a fixed number of SLOTS share one step:

    seer_slot_step_begin  ->  the UNet over [uc rows | c rows] of all slots  ->  seer_slot_cfg_ddim_step

With `plms=True` the sampler is chosen per request: the step is seer_slot_step_begin -> the UNet -> seer_slot_cfg_plms_step, and
every slot also has a phase word, a 3-entry ring of earlier eps and a provisional latent in device memory.  A DDIM clip (phase 0)
runs as above.  A PLMS clip of n schedule entries occupies its slot for n + 1 steps: its first step evaluates twice -- phase 1 at
(x, t) writes the provisional latent and keeps e, phase 2 evaluates at (x_prov, t_next) and applies the mean of the two to x --
and every later step (phase 3) is one evaluation of order 2, 3, 4 over the ring.  The kernels walk the phases themselves: the
host writes a slot's phase, like its counter, only when it fills the slot.

Each slot has its own schedule tables, step counter, guidance scale, prompt and conditioning frames, all in static device buffers, so
the step is captured ONCE per (slots, clip shape, context shape, engine mode) -- neither the scale nor a schedule is part of the key --
and a slot is refilled as soon as its clip is done.  The kernels count every slot's schedule down themselves; the host writes a
slot's counter only when it fills the slot, and it knows from its own count when the slot finishes: step() reads nothing back.

What a slot promises (INTEGRATION.md has the full list): under `SeerUNet(layout_invariant=True)` and scale != 1 the latent of a clip
is bit for bit the one DDIMSampler.sample -- PLMSSampler.sample for a PLMS clip -- returns for that clip alone (batch 1, eta = 0, the
same scale and start code), whatever the other slots hold, whichever sampler they run and whenever it was admitted.  At scale == 1 the solo sampler evaluates once without CFG, a slot evaluates the pair
and combines it with scale 1: not the same bits.  Without the invariant mode a slot is a row of a batch of `slots` clips: the same
kernels, results within the layout tolerance.  The captured step and the launch-by-launch step give the same bits in either mode.
The reference's per-step RNG draw (ddim_video.py:234) has no counterpart here: nothing consumes the device RNG stream.

With `stochastic=True` a request may carry eta > 0, a seed and a temperature: the step's last kernel is given the slots' seeds
and draws a slot's noise itself from (the slot's seed, its schedule index, the element) -- a counter-based generator (DESIGN.md,
"Seeded noise"), so nothing is drawn between launches, nothing is frozen into the graph and the noise of a clip does not depend on
its slot or its neighbours.  Each slot also has a seed pair and a temperature in device memory, and its coefficient rows carry the
sigma of its own eta.  The promise above then holds for a seeded clip against DDIMSampler.sample(..., eta=, seed=, x_T=None).

With `dpm=True` a request may choose DPM-Solver++ (submit's method="dpmpp", with order, lower_order_final and discretize as
DPMSolverSampler takes them): the step is seer_slot_step_begin -> the UNet -> seer_slot_cfg_dpm_step, and every slot also has a DPM
table and four state words in device memory -- history valid by index parity (twice), the slot's sampler (0 DDIM, 1 first order, 2
2M) and the final-step rule.  The history of a 2M clip is the slot's own pred_x0 rows.  A clip of n schedule entries occupies its slot
for n steps, one evaluation each, whichever sampler it runs: 2M at 25 steps is where DDIM is at 50 on the analytic model
(profiles/dpm_sampler.md), so the queue turns clips over twice as fast.  The host writes the four words only when it fills the slot --
(0, 0, sampler, rule): a clip's first step is first order and never reads the stale D of the slot's last clip -- and the kernel walks
the orders itself.  The promise above then reads: a "dpmpp" clip's latent is bit for bit DPMSolverSampler(order=, lower_order_final=,
discretize=).sample's for that clip alone, and a DDIM clip in such a queue has the bits it has in a plain one.

With `editing=True` a request may carry a mask with given latents, and a start level (submit's `mask`, `x0`, `t_start`): the step
opens with seer_slot_known_blend, which re-noises a slot's given latents to the level of the slot's next index from Philox stream 2 of
its seed and blends them in where the slot's mask says so.  A slot whose mask is all zero -- every plain clip -- is not touched by it,
so edited and plain clips share a queue, and a plain clip has the bits it has in a queue built without the keyword.

With `prediction_type="v_prediction"` (per sampler object, not per request: the parameterisation belongs to the model) the UNet's output
is the velocity v, and the step gains one launch between the model and the update, seer_slot_v_to_eps: every slot's rows become eps
with the slot's own coefficient row -- for a PLMS clip's second evaluation the row below and the provisional latent it was made at.
It holds in every mode above, under a key of its own, and the promise reads against the solo sampler built with the same keyword.

With `rescale=True` a request may carry guidance_rescale = phi in [0, 1] (submit): the step gains one node, seer_slot_cfg_rescale (two
launches), between the model and the v-conversion, which scales a slot's guided output to the std of its conditional row and writes it
to both of the slot's rows (DESIGN.md "Guidance rescale").  Each slot has its phi in device memory, like its scale; a slot with phi = 0
is not touched by the node, so rescaled and plain clips share a queue and a plain clip has the bits it has in a queue built without the
keyword.  It goes with every mode above, under a key of its own; the promise reads against the solo sampler's sample(guidance_rescale=phi).

Out of scope: PLMS with noise or with a mask, DPM-Solver++ with noise, with a mask or from a start level, PLMS and DPM-Solver++ in one
queue, slots of different clip shapes, frame-sharded models, a per-slot K/V refresh, resizing without a new
capture.
"""
from __future__ import annotations

from typing import Dict, Iterable, Iterator, List, Optional, Tuple

import torch

from . import ops as hip_ops
from . import step_cache
from .ddim import DDIMSampler, capture_step
from .dpm import DPMSolverSampler
from .step_graph import capture_engine, engine_on

MAX_SLOTS = 4           # the time-embedding MLP (seer_linear_smallm) takes up to 8 rows: the [uc | c] pair of 4 slots


class SlotSampler:
    """`slots` clips of one shape in one step.  shape = (C, F_pred, h, w) of a clip's latent, cond_frames = f1 conditioning latents
    in front of it (x0_emb), context_shape = (L, D) of one frame's text context.  `model_cond_frame` is the `cond_frame` the UNet is
    called with -- DDIMSampler.sample's `cond_frames` keyword, which ddim_sample leaves at 0.  `ops` is the backend of the two
    step-boundary kernels (tests inject a torch restatement to run the host logic on the CPU); a `unet` that is no SeerUNet is called
    as `unet(sample, t, context, cond_frame=...)`.  `plms=True` lets a request choose PLMS (submit's `method`): the step then runs
    the two kernels that carry a sampler per slot, over three more static buffers, and is captured under a key of its own; with
    False everything is as it was before that keyword existed.  `stochastic=True` lets a request carry eta, seed and temperature
    (submit): the step's last kernel then draws the noise per slot, over two more static buffers, again under a key of its own; it
    excludes plms=True (PLMS has no noise term).  `editing=True` lets a request carry mask, x0 and t_start (submit): the step then
    opens with the blend kernel, over per-slot mask, given-latent and seed buffers, under a key of its own once more (and another with
    stochastic=True); it excludes plms=True as well.  `dpm=True` lets a request choose DPM-Solver++ (submit's `method`, `order`,
    `lower_order_final`, `discretize`): the step's last kernel then carries a sampler per slot, DDIM or DPM-Solver++, over two more
    static buffers, under a key of its own; it excludes plms, stochastic and editing (the solo DPMSolverSampler has no seeded or masked
    form for a slot to be bit-equal to).  `prediction_type` "epsilon" (the default: nothing changes) or "v_prediction": what the
    UNet's output is (train.py:371-376; anything else is its ValueError), in every mode.  `rescale=True` lets a request carry
    guidance_rescale (submit): the step then has the rescale node behind the model, over a per-slot factor and a workspace, under a key
    of its own; it goes with every other keyword."""

    def __init__(self, unet, slots: int, shape, cond_frames: int, context_shape, max_steps: int = 64, device=None, ops=hip_ops,
                 model_cond_frame: int = 0, plms: bool = False, stochastic: bool = False, editing: bool = False,
                 dpm: bool = False, prediction_type: str = "epsilon", rescale: bool = False):
        self.prediction_type = hip_ops.check_prediction_type(prediction_type)
        step_cache.refuse(unet, "SlotSampler")
        C, Fp, h, w = (int(v) for v in shape)
        L, D = (int(v) for v in context_shape)
        f1 = int(cond_frames)
        if not 1 <= int(slots) <= MAX_SLOTS:
            raise ValueError(f"slots = {slots}: 1 .. {MAX_SLOTS} (the [uc | c] rows of all slots go through the 8-row time embedding)")
        if min(C, Fp, h, w, L, D) < 1 or f1 < 0 or int(max_steps) < 1:
            raise ValueError(f"shape {tuple(shape)}, cond_frames {cond_frames}, context_shape {tuple(context_shape)}, max_steps {max_steps}")
        if stochastic and plms:
            raise ValueError("stochastic=True with plms=True: PLMS is deterministic only, build one sampler for each")
        if editing and plms:
            raise ValueError("editing=True with plms=True: PLMS with a mask is not built, build one sampler for each")
        if dpm and plms:
            raise ValueError("dpm=True with plms=True: PLMS and DPM-Solver++ in one queue is not built, build one sampler for each")
        if stochastic and dpm:
            raise ValueError("stochastic=True with dpm=True: DPM-Solver++ is deterministic only, build one sampler for each")
        if editing and dpm:
            raise ValueError("editing=True with dpm=True: DPM-Solver++ with a mask is not built, build one sampler for each")
        if (stochastic or editing) and C * Fp * h * w >= 1 << 31:
            raise ValueError(f"shape {tuple(shape)}: a seeded clip has fewer than 2^31 elements")
        if device is None:
            p0 = next(unet.parameters(), None) if hasattr(unet, "parameters") else None
            device = p0.device if p0 is not None else "cpu"
        self.unet, self.ops, self.slots, self.max_steps = unet, ops, int(slots), int(max_steps)
        self.shape, self.f1, self.context_shape, self.model_cond_frame = (C, Fp, h, w), f1, (L, D), int(model_cond_frame)
        self.device = dev = torch.zeros((), device=device).device      # "cuda" -> the current device, with its index: what an engine reports
        n, f32 = self.slots, torch.float32
        # the static buffers of the step: everything the kernels and the UNet read, by address, for as long as this sampler lives
        self._x = torch.zeros((n, C, Fp, h, w), device=dev, dtype=f32)
        self._pred = torch.zeros_like(self._x)
        self._x0 = torch.zeros((n, C, f1, h, w), device=dev, dtype=f32) if f1 else None
        self._sample = torch.zeros((2 * n, C, f1 + Fp, h, w), device=dev, dtype=f32)
        self._t = torch.zeros((2 * n,), device=dev, dtype=torch.long)
        self._step = torch.full((n, 2), -1, device=dev, dtype=torch.int32)           # every slot idle
        self._coef = torch.zeros((n, self.max_steps, 4), device=dev, dtype=f32)
        self._coef[:, :, 0] = 1.0                    # a_t = 1 in the unused rows, as DDIMSampler's captured step keeps them
        self._ttab = torch.zeros((n, self.max_steps), device=dev, dtype=torch.long)
        self._scale = torch.ones((n,), device=dev, dtype=f32)
        self._context = torch.zeros((2 * n, f1 + Fp, L, D), device=dev, dtype=f32)    # uc rows, then c rows
        # The mode, decided here once: its buffers, the first word of its graph-cache key, the launches in front of the model call and the
        # update behind it (names in the backend with their arguments, for _body), and the buffers to zero when a slot retires (step).
        self.plms, self.stochastic, self.editing, self.dpm = bool(plms), bool(stochastic), bool(editing), bool(dpm)
        self._retire = [self._x] + ([self._x0] if f1 else [])
        if self.plms:
            self._state = torch.zeros((n, hip_ops.SLOT_STATE_WORDS), device=dev, dtype=torch.int32)    # phase 0, nothing in the ring
            self._ring = torch.zeros((n, 3, C, Fp, h, w), device=dev, dtype=f32)
            self._xprov = torch.zeros_like(self._x)
            self._retire.append(self._xprov)
            self._kind = "slots-plms"
            self._front = [("slot_plms_step_begin", (self._x0, self._x, self._xprov, self._ttab, self._step, self._state, 2, self._sample,
                                                     self._t))]
            self._update = ("slot_cfg_plms_step", (self._state, self._ring, self._xprov))
        elif self.dpm:
            self._dpm_coef = torch.zeros((n, self.max_steps, hip_ops.DPM_ROW_WORDS), device=dev, dtype=f32)
            self._dpm_state = torch.zeros((n, hip_ops.SLOT_DPM_STATE_WORDS), device=dev, dtype=torch.int32)   # every slot DDIM
            self._kind = "slots-dpm"
            self._front = [("slot_step_begin", (self._x0, self._x, self._ttab, self._step, 2, self._sample, self._t))]
            self._update = ("slot_cfg_dpm_step", (self._dpm_coef, self._dpm_state))
        else:
            self._kind = {(False, False): "slots", (False, True): "slots-rng", (True, False): "slots-edit",
                          (True, True): "slots-edit-rng"}[self.editing, self.stochastic]
            self._front = [("slot_step_begin", (self._x0, self._x, self._ttab, self._step, 2, self._sample, self._t))]
            self._update = ("slot_cfg_ddim_step", ())
        if self.stochastic or self.editing:
            self._seeds = torch.zeros((n, 2), device=dev, dtype=torch.int32)          # (lo, hi) words of a slot's uint64 seed
        if self.editing:
            self._mask = torch.zeros((n, Fp, h, w), device=dev, dtype=f32)            # all zero: the blend leaves the slot alone
            self._known = torch.zeros_like(self._x)
            self._retire += [self._mask, self._known]       # the next clip of a slot is a plain one until its submit says otherwise
            self._front.insert(0, ("slot_known_blend", (self._x, self._mask, self._known, self._coef, self._step, self._seeds)))
        if self.stochastic:
            self._temp = torch.ones((n,), device=dev, dtype=f32)
            self._update = ("slot_cfg_ddim_step_rng", (self._seeds, self._temp))
        self.rescale = bool(rescale)
        if self.rescale:
            self._phi = torch.zeros((n,), device=dev, dtype=f32)                      # 0: the rescale node leaves the slot alone
            self._rescale_ws = self.ops.cfg_rescale_workspace(n, C, f1 + Fp, f1, h * w, dev)
        self._left = [0] * n                          # steps a slot still has to run; 0 = free
        self._sched = DDIMSampler(dev)
        self._tables: Dict[Tuple[int, float], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._dpm_tables: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        self._capture_refused = False

    # ---- the queue's host side -----------------------------------------------------------------------------------------------
    def free_slots(self) -> List[int]:
        return [s for s, left in enumerate(self._left) if left == 0]

    def active(self) -> List[int]:
        return [s for s, left in enumerate(self._left) if left > 0]

    def pred_x0(self, slot: int) -> torch.Tensor:
        """a copy of the slot's pred_x0 of its last step (it stays readable after the slot retired, until the slot is refilled)"""
        return self._pred[slot:slot + 1].clone()

    def _schedule(self, S: int, eta: float = 0.):
        """DDIMSampler.make_schedule(S, ddim_eta=eta): the same tables bit for bit, made once per (S, eta)"""
        key = (S, float(eta))
        if key not in self._tables:
            self._sched.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=False)
            self._tables[key] = (self._sched.ddim_coef, self._sched._t_table)
        return self._tables[key]

    def _dpm_schedule(self, S: int, discretize: str):
        """DPMSolverSampler(discretize=).make_schedule(S): (ddim_coef, _t_table, dpm_coef), the same tables bit for bit, made once per
        (S, discretize)"""
        key = (S, discretize)
        if key not in self._dpm_tables:
            sched = DPMSolverSampler(self.device, discretize=discretize)
            sched.make_schedule(ddim_num_steps=S, ddim_eta=0., verbose=False)
            self._dpm_tables[key] = (sched.ddim_coef, sched._t_table, sched.dpm_coef)
        return self._dpm_tables[key]

    def _clip(self, t: Optional[torch.Tensor], want, what: str) -> torch.Tensor:
        if t is None or tuple(t.shape) not in (tuple(want), (1, *want)):
            raise ValueError(f"{what}: shape {None if t is None else tuple(t.shape)}, this sampler takes {tuple(want)} (with or without "
                             "a leading 1)")
        return t.reshape(want).to(device=self.device, dtype=torch.float32)

    @torch.no_grad()
    def submit(self, x_T, x0_emb, c, uc, S: int, scale: float, eta: float = 0., method: str = "ddim", seed: Optional[int] = None,
               temperature: float = 1., mask=None, x0=None, t_start: Optional[int] = None, order: int = 2,
               lower_order_final: bool = True, discretize: str = "uniform", guidance_rescale: float = 0.) -> int:
        """Admit one clip into a free slot and return the slot.  x_T [1 or none, C, F_pred, h, w] is the start code, x0_emb
        [.., C, f1, h, w] the conditioning latents (None when f1 == 0), c / uc [.., f1 + F_pred, L, D] the text context and the
        empty-prompt context, S the number of DDIM steps (DDIMSampler.make_schedule(S): the stride rule can give S + 1 entries),
        scale the guidance scale, method "ddim" or "plms" (a sampler built with plms=True only; the same schedule, and a clip of n
        entries then occupies its slot for n + 1 steps).  The clip's tables, scale, start index, latents and its two context rows are written into the
        slot's part of the static buffers; the engine's 16-bit context and the cross-attention K|V of the text blocks are then
        refreshed at the next step through the engine's own context path -- over ALL slots, not only the one that changed (1 + 16
        small launches per admission; a per-slot refresh is not built).
        A sampler built with stochastic=True also takes eta (the clip's tables then carry its sigma), seed (an unsigned 64-bit
        integer: the clip's noise is Philox stream 1 of it, and with x_T = None its start code is stream 0) and temperature; eta > 0
        needs a seed.  Without stochastic=True any of the three is a ValueError.
        A sampler built with editing=True also takes mask ([1 or none, 1 or none, F_pred, h, w], values in [0, 1]) with x0 (the given
        latents, shaped like x_T) -- in front of every step the slot's latent becomes q * mask + (1 - mask) * latent, q = x0 noised to
        the step's level with Philox stream 2 of `seed`, which it therefore needs -- and t_start = k (1 .. the schedule's entries):
        x_T is then the latent at level k, the slot's counter starts at k - 1 and the clip occupies its slot for k steps.  Without
        editing=True any of the three is a ValueError.
        A sampler built with dpm=True also takes method "dpmpp" with order (1 or 2: first order or 2M), lower_order_final (the final
        step of a schedule of fewer than 15 entries is first order) and discretize ("uniform", or "logsnr": the schedule can then
        have fewer than S entries) -- DPMSolverSampler's constructor keywords, with its defaults; the clip's tables are that sampler's
        make_schedule(S) and it occupies its slot for one step per entry.  The three keywords belong to "dpmpp": with another method
        anything but their defaults is a ValueError, as is "dpmpp" on a sampler built without dpm=True.
        A sampler built with rescale=True also takes guidance_rescale, a number in [0, 1]: the clip's guided model output is rescaled to
        the std of its conditional row and blended by that factor in every evaluation (0: the clip is a plain one).  Without
        rescale=True a non-zero value is a ValueError, as is a value outside [0, 1] anywhere.
        Raises RuntimeError when no slot is free, ValueError for a schedule longer than max_steps, a shape that is not the
        constructor's, eta != 0, a frame-sharded model, an unknown method, and "plms" or "dpmpp" on a sampler built without it."""
        C, Fp, h, w = self.shape
        F, (L, D) = self.f1 + Fp, self.context_shape
        phi = hip_ops.check_guidance_rescale(guidance_rescale)
        if phi != 0. and not self.rescale:
            raise ValueError("guidance_rescale needs a sampler built with rescale=True")
        if not self.editing and (mask is not None or x0 is not None or t_start is not None):
            raise ValueError("mask / x0 / t_start need a sampler built with editing=True")
        if (mask is None) != (x0 is None):
            raise ValueError("mask and x0 go together: the mask says where the latent is given, x0 what it is there")
        if mask is not None and seed is None:
            raise ValueError("mask needs a seed: a slot re-noises the given latents from the clip's own seed, not from torch's generator")
        if not self.stochastic:
            if eta != 0:
                raise ValueError(f"eta = {eta}: slots run the deterministic update only (eta = 0) unless built with stochastic=True")
            if (seed is not None and mask is None) or temperature != 1.:
                raise ValueError("seed / temperature need a sampler built with stochastic=True")
        elif eta < 0 or (eta != 0 and seed is None):
            raise ValueError(f"eta = {eta} needs a seed: a slot draws its noise from the clip's own seed, not from torch's generator")
        if seed is not None and not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"seed = {seed}: a seed is an unsigned 64-bit integer")
        if method not in ("ddim", "plms", "dpmpp"):
            raise ValueError(f"method = {method!r}: 'ddim', 'plms' or 'dpmpp'")
        if method == "plms" and not self.plms:
            raise ValueError("method = 'plms' needs a sampler built with plms=True")
        if method == "dpmpp" and not self.dpm:
            raise ValueError("method = 'dpmpp' needs a sampler built with dpm=True")
        if method != "dpmpp" and (order != 2 or not bool(lower_order_final) or discretize != "uniform"):
            raise ValueError(f"order / lower_order_final / discretize belong to method = 'dpmpp', not to {method!r}")
        if order not in (1, 2):
            raise ValueError(f"order = {order!r}: 1 (first order) or 2 (2M)")
        if discretize not in ("uniform", "logsnr"):
            raise ValueError(f"discretize = {discretize!r}: 'uniform' or 'logsnr'")
        if getattr(self.unet, "_shard", None) is not None:
            raise ValueError("a frame-sharded model cannot run slots: detach it (parallel.attach) first")
        if x_T is not None or seed is None or t_start is not None:
            x_T = self._clip(x_T, (C, Fp, h, w), "x_T")
        if mask is not None:
            mask = torch.as_tensor(mask)
            if tuple(mask.shape[-3:]) != (Fp, h, w) or any(d != 1 for d in mask.shape[:-3]) or mask.dim() > 5:
                raise ValueError(f"mask {tuple(mask.shape)}: this sampler takes {(1, Fp, h, w)}, one mask for a clip's channels")
            mask = mask.reshape(Fp, h, w).to(device=self.device, dtype=torch.float32)
            x0 = self._clip(x0, (C, Fp, h, w), "x0")
        if self.f1:
            x0_emb = self._clip(x0_emb, (C, self.f1, h, w), "x0_emb")
        elif x0_emb is not None:
            raise ValueError("x0_emb given to a sampler built with cond_frames = 0")
        c, uc = self._clip(c, (F, L, D), "c"), self._clip(uc, (F, L, D), "uc")
        dpm_coef = None
        if method == "dpmpp":
            coef, ttab, dpm_coef = self._dpm_schedule(int(S), discretize)
        else:
            coef, ttab = self._schedule(int(S), eta)
        n = int(coef.shape[0])
        if n > self.max_steps:
            raise ValueError(f"S = {S} makes a schedule of {n} entries, this sampler was built for max_steps = {self.max_steps}")
        start = n if t_start is None else int(t_start)
        if not 1 <= start <= n:
            raise ValueError(f"t_start = {t_start}: 1 .. {n}, the entries of the schedule of S = {S}")
        free = self.free_slots()
        if not free:
            raise RuntimeError(f"all {self.slots} slots are busy: step() until one finishes")
        s = free[0]
        self._coef[s, :n].copy_(coef)
        self._ttab[s, :n].copy_(ttab)
        self._scale[s:s + 1].fill_(float(scale))
        if self.rescale:
            self._phi[s:s + 1].fill_(phi)
        if x_T is None:                              # the start code of a seeded clip: stream 0 of its seed
            self.ops.philox_normal(int(seed), hip_ops.PHILOX_STREAM_START, 0, self._x[s].numel(), out=self._x[s])
        else:
            self._x[s].copy_(x_T)
        if self.stochastic or self.editing:
            self._seeds[s].copy_(hip_ops.seed_words([0 if seed is None else seed])[0])
        if self.stochastic:
            self._temp[s:s + 1].fill_(float(temperature))
        if mask is not None:
            self._mask[s].copy_(mask)
            self._known[s].copy_(x0)
        if self.f1:
            self._x0[s].copy_(x0_emb)
        self._context[s].copy_(uc)
        self._context[self.slots + s].copy_(c)
        self._step[s, :1].fill_(start - 1)           # the one host-written counter of the clip: the kernels count it down
        self._left[s] = start
        if self.plms:
            # the slot's sampler: phase 1 opens a PLMS clip, phase 0 is DDIM; (valid, newest) = (0, 2), an empty ring.  The first PLMS
            # step is two steps of the slot
            first = 1 if method == "plms" else 0
            self._state[s, :3].copy_(torch.tensor([first, 0, 2], dtype=torch.int32))
            self._left[s] = n + first
        if self.dpm:
            # the slot's sampler and its order rule, history invalid: the one host write of these words, the kernel walks the rest
            words = [0, 0, int(order), int(bool(lower_order_final) and n < 15)] if dpm_coef is not None else [0, 0, 0, 0]
            if dpm_coef is not None:
                self._dpm_coef[s, :n].copy_(dpm_coef)
            self._dpm_state[s].copy_(torch.tensor(words, dtype=torch.int32))
        return s

    # ---- the step ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self) -> List[Tuple[int, torch.Tensor]]:
        """One step of every active slot (one replay, or the same three calls launch by launch).  Returns (slot, latent
        [1, C, F_pred, h, w]) for the slots that finished with it: their latent is a copy, their buffers are zeroed and they are free
        again.  Does nothing when every slot is idle."""
        if not self.active():
            return []
        self._run_step()
        done = []
        for s in self.active():
            self._left[s] -= 1
            if self._left[s] == 0:
                done.append((s, self._x[s:s + 1].clone()))
                for buf in self._retire:             # an idle slot's rows stay finite (its counter is -1 by now: the kernels saw to it)
                    buf[s].zero_()
        return done

    def run(self, requests: Iterable[dict]) -> Iterator[Tuple[object, torch.Tensor]]:
        """Generator over an iterable of dict(x_T=, x0_emb=, c=, uc=, S=, scale=, tag=[, method=][, eta=, seed=, temperature=]
        [, mask=, x0=, t_start=][, order=, lower_order_final=, discretize=][, guidance_rescale=]): fills free slots in request order
        (a request is taken from the iterable only when a slot is free for it), steps, and yields (tag, latent) as clips finish, in
        finishing order."""
        it, tags, more = iter(requests), {}, True
        while True:
            while more and self.free_slots():
                r = next(it, None)
                if r is None:
                    more = False
                    break
                r = dict(r)
                tag = r.pop("tag", None)
                tags[self.submit(**r)] = tag
            if not self.active():
                return
            for s, lat in self.step():
                yield tags.pop(s), lat

    def _body(self, model) -> None:
        """the launches of the sampler's mode (__init__) around `model`, the UNet over the assembled [uc rows | c rows]"""
        for name, args in self._front:
            getattr(self.ops, name)(*args)
        eps = model()
        if self.rescale:                             # both rows of a slot with phi > 0 become its rescaled guided output, in place
            self.ops.slot_cfg_rescale(eps, self._scale, self._phi, self._coef, self._step, cond_f=self.f1, ws=self._rescale_ws)
        if self.prediction_type != "epsilon":        # v -> eps, in place on the model's output, per slot
            phases = dict(state=self._state, x_prov=self._xprov) if self.plms else {}
            self.ops.slot_v_to_eps(eps, self._x, self._coef, self._step, cond_f=self.f1, out=eps, **phases)
        name, args = self._update
        getattr(self.ops, name)(eps, self._x, self._scale, self._coef, self._step, *args, cond_f=self.f1, x_prev=self._x,
                                pred_x0=self._pred)

    def _run_step(self) -> None:
        from .unet import SeerUNet
        unet = self.unet
        step_cache.refuse(unet, "SlotSampler")       # (enabled since the sampler was built)
        if not isinstance(unet, SeerUNet):
            self._body(lambda: unet(self._sample, self._t, self._context, cond_frame=self.model_cond_frame).float().contiguous())
            return
        if unet._shard is not None or unet.config.center_input_sample:
            raise ValueError("slots run an unsharded model without center_input_sample")
        if self.shape[2] % 8 or self.shape[3] % 8:
            raise ValueError("latent height/width must be multiples of 8 (three stride-2 levels + 4/8 windows)")
        eng = engine_on(unet, self.device)           # the launch-by-launch step runs on the engine too
        ctx, L = eng._context(self._context)         # a new admission (or another caller's prompt since): refreshed in place, all slots
        model = lambda: eng._forward(self._sample, self._t, ctx, L, self.model_cond_frame)
        G = None
        if not self._capture_refused and capture_engine(unet, self.ops, self.device) is not None:
            key = (self._kind, self.slots, self.shape, self.f1, self.model_cond_frame, L, tuple(ctx.shape), eng.inv,
                   *(() if self.prediction_type == "epsilon" else (self.prediction_type,)), *(("rescale",) if self.rescale else ()),
                   *getattr(eng, "freeu_key", ()))
            G = eng.graph_get(key)
            if G is None or G["x"] is not self._x:   # (another SlotSampler of the same key owns that entry: this one captures its own)
                G = self._capture(eng, key, model)
        if G is None:
            self._body(model)
        else:
            G["graph"].replay()

    def _capture(self, eng, key, model):
        """the step as one hipGraph (ddim.capture_step: warm-up, capture, the engine's graph cache).  Warm-up and capture run with every
        slot idle -- the update kernel then writes nothing and the begin kernel only what the next step rewrites -- so admitted clips
        are where they were afterwards; the counters (and the sampler state words) are put back on the device, nothing is read back."""
        saved = self._step.clone()
        state = self._state.clone() if self.plms else None
        self._step.fill_(-1)
        G = capture_step(eng, key, dict(x=self._x, owner=self), lambda: self._body(model))
        self._step.copy_(saved)
        if state is not None:
            self._state.copy_(state)
        if G is None:
            self._capture_refused = True
        return G
