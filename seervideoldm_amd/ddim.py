"""DDIMSampler / ddim_sample -- host-side mirror of the reference's sampler surface
(ldm/models/diffusion/ddim_video.py:14-238, utils/ddim_sampling_utils.py:21-42).

Same names, keyword arguments and return values.  Differences that are not semantic:
  * the schedule tables are computed on the host exactly like the reference (float64 -> float32 values) and uploaded
    ONCE as a [S', 4] fp32 table; a step reads row `index` on the device, so there are no per-step host->device scalar
    copies (the reference does four `torch.full(numpy_scalar)` per step, ddim_video.py:219-222);
  * CFG combine + DDIM update are one fused HIP kernel (seer_cfg_ddim_step);
  * `register_buffer` does not hard-code "cuda" (SURVEY finding 5);
  * the batched-CFG inputs [uc, c] are concatenated once per `sample()` call, not once per step.
The reference draws `torch.randn(x.shape)` every step even when sigma == 0 (ddim_video.py:234); we keep the draw so a seeded
multi-sample run consumes the device RNG stream identically.

`sample(..., seed=)` (an int, or one int per batch row) replaces every draw by a counter-based generator inside the kernels (DESIGN.md,
"Seeded noise"): the start code is seer_philox_normal of the row's seed, the noise of a step is drawn by seer_cfg_ddim_step from
(seed, schedule index, element).  Nothing comes from torch's generator, the captured step is taken for eta > 0 too, and a row's
noise does not depend on the batch it is in.

`sample(..., mask=, x0=)`, `stochastic_encode` and `decode` follow the vendored CompVis sampler (ldm/models/diffusion/ddim.py:144-147,
207-241), whose mask blend ddim_video.py lost: kept regions are re-noised to each step's level and blended in in front of the step
(seer_known_blend; with a seed a node of the captured step, DESIGN.md "Editing"), a clip can be noised to a level of the schedule
(seer_q_sample) and denoised from there.

`encode` is DDIM inversion, the `encode()` CompVis added to ddim.py after the version the reference vendors: the probability-flow ODE
upward from a clip's latents to a level of the schedule with the model in the loop (seer_cfg_ddim_invert_step; as a captured step its
counter runs upward to a limit word in device memory, DESIGN.md "Editing"), so that decode comes back to the same clip.  Nothing is drawn.

`DDIMSampler(device, prediction_type="v_prediction")` samples a model fine-tuned on the velocity target (train.py:373-374): the UNet's
output is then v = sqrt(a) eps - sqrt(1 - a) x0, and ONE more elementwise kernel (seer_v_to_eps; in the captured step one more node,
seer_v_to_eps) turns it into eps = sqrt(a) v + sqrt(1 - a) x_t in front of the step's last kernel, with the coefficient row that
kernel reads.  Everything behind it -- CFG, eta > 0, seeds, mask / x0, decode, stochastic_encode -- acts on eps or on latents and is
unchanged.  `encode` is refused for such a model (see there).  With the default "epsilon" nothing new is launched or allocated.

`DDIMSampler(device, guidance_rescale=0.7)` -- or `guidance_rescale=` on sample, decode, encode, p_sample_ddim and p_invert_ddim, which
overrides the constructor's value for that call -- is guidance rescale (Lin et al. 2023, section 3.4; diffusers' rescale_noise_cfg), the
way v-models are sampled: the guided model output is scaled so that its std over a clip matches the conditional branch's and blended
with the unscaled one by that factor.  One node (two launches, seer_cfg_rescale) between the model and the conversion above overwrites
both rows of the [uc | c] pair with the result, and the update kernels behind it are unchanged (DESIGN.md "Guidance rescale").  A number
in [0, 1]; at 0 (the default), or where CFG is off, nothing is launched and the graph keys are what they were.  A sharded model is refused.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .step_cache import policy_of
from .step_graph import capture_engine, capture_step, changed, refresh      # capture_step: slots.py and callers import it from here


def _betas(n_train: int, beta_first: float, beta_last: float) -> np.ndarray:
    """The one noise schedule of this path: sqrt(beta) rises in n_train equal steps from sqrt(beta_first) to
    sqrt(beta_last); float64, like the reference's table (ldm/modules/diffusionmodules/util.py:23-26 under the name "linear")."""
    root = torch.linspace(float(beta_first) ** 0.5, float(beta_last) ** 0.5, int(n_train), dtype=torch.float64)
    return (root * root).numpy()


def _strided_timesteps(n_sample: int, n_train: int) -> np.ndarray:
    """Every (n_train // n_sample)-th training step, shifted by one: S = 50 -> 1, 21, ..., 981; S = 30 has stride 33 and
    therefore 31 entries (util.py:46-60, the "uniform" rule)."""
    stride = int(n_train) // int(n_sample)
    if stride < 1:
        raise ValueError(f"{n_sample} sampling steps do not fit into {n_train} training steps")
    return np.arange(0, int(n_train), stride, dtype=np.int64) + 1


class DDIMSampler(object):
    def __init__(self, device, timesteps=1000, schedule="linear", **kwargs):
        self.ddpm_num_timesteps = timesteps
        self.schedule = schedule
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        # the backend of the step's own kernels outside the captured step (tests inject a torch restatement to run this class on the
        # CPU; the captured step is taken with the HIP backend only)
        self.ops = kwargs.get("ops") or ops
        # what the UNet's output is (train.py:371-376): "epsilon", or "v_prediction" -- converted to eps in front of every update
        self.prediction_type = ops.check_prediction_type(kwargs.get("prediction_type", "epsilon"))
        # guidance rescale (Lin et al. 2023): the default blend factor of every call, 0 = off; a call's own keyword overrides it
        self.guidance_rescale = ops.check_guidance_rescale(kwargs.get("guidance_rescale", 0.))
        self.consume_rng_when_deterministic = True
        # p_sample_ddim under graph replay hands out its static latent buffers instead of copies of them: the next step
        # overwrites what the previous one returned.  ddim_sampling sets it for its own loop (and copies what it keeps).
        self.static_step_outputs = False
        self._capture_refused = False       # set when a capture of this sampler's step fails: it steps launch by launch from then on
        self._kept = {}                     # step_graph.changed's record of the (c, uc) pair behind _cfg_context

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, given_betas=None, beta_schedule="linear", timesteps=1000,
                      linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3, ddim_discretize="uniform", ddim_eta=0.,
                      verbose=True):
        """ddim_video.py:27-68.  Host arithmetic mirrors the reference's dtypes: cumprod in float64, stored float32."""
        if ddim_discretize != "uniform" or (given_betas is None and beta_schedule != "linear"):
            # the sampler scripts never ask for anything else (ddim_sampling_utils.py:29-36); the reference's other branches
            # are not on this path
            raise NotImplementedError(f"schedule {beta_schedule!r} / discretisation {ddim_discretize!r}: this path has the "
                                      "'linear' (sqrt-space) betas and the 'uniform' stride only")
        betas = np.asarray(given_betas, dtype=np.float64) if given_betas is not None else _betas(timesteps, linear_start, linear_end)
        alphas_cumprod = np.cumprod(1. - betas, axis=0)
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        ac32 = torch.tensor(alphas_cumprod, dtype=torch.float32)
        self.ddim_timesteps = self._sampling_timesteps(ddim_num_steps, ac32)
        if verbose:
            print(f"DDIM timesteps ({len(self.ddim_timesteps)}): {self.ddim_timesteps}")
        self.betas = torch.tensor(betas, dtype=torch.float32)
        self.alphas_cumprod = ac32
        self.alphas_cumprod_prev = torch.tensor(np.append(1., alphas_cumprod[:-1]), dtype=torch.float32)
        ts = self.ddim_timesteps
        a32 = ac32[ts].numpy()
        self.ddim_alphas = a32.astype(np.float64)
        self.ddim_alphas_prev = np.asarray([float(ac32[0])] + ac32[ts[:-1]].tolist())
        self.ddim_sigmas = ddim_eta * np.sqrt((1 - self.ddim_alphas_prev) / (1 - self.ddim_alphas) *
                                              (1 - self.ddim_alphas / self.ddim_alphas_prev))
        self.ddim_sqrt_one_minus_alphas = np.sqrt(np.float32(1.0) - a32).astype(np.float64)
        coef = np.stack([self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sigmas, self.ddim_sqrt_one_minus_alphas], 1)
        self.ddim_coef = torch.tensor(coef, dtype=torch.float32, device=self.device)     # ONE upload per schedule
        self._t_table = torch.tensor(ts, dtype=torch.long, device=self.device)

    def _sampling_timesteps(self, n_sample: int, alphas_cumprod: torch.Tensor) -> np.ndarray:
        """the training steps a schedule of n_sample steps visits, ascending: the reference's 'uniform' stride.  `alphas_cumprod` is
        the fp32 table of every training step, for a sampler that places its steps by noise level (dpm.py)."""
        return _strided_timesteps(n_sample, self.ddpm_num_timesteps)

    @torch.no_grad()
    def sample(self, unet, S, batch_size, shape, x0_emb=None, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, eta=0., mask=None, x0=None, cond_frames=0, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, null_cond_prob=None, is_3d=False,
               **kwargs):
        seeds = _row_seeds(kwargs.get("seed"), batch_size)
        size = self._sample_size(S, batch_size, shape, conditioning, eta, verbose, is_3d)
        return self.ddim_sampling(unet, conditioning, size, x0_emb=x0_emb, is_3d=is_3d, callback=callback,
                                  img_callback=img_callback, cond_frames=cond_frames, temperature=temperature,
                                  noise_dropout=noise_dropout, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, seeds=seeds, mask=mask, x0=x0,
                                  guidance_rescale=kwargs.get("guidance_rescale"))

    def _sample_size(self, S, batch_size, shape, conditioning, eta, verbose, is_3d):
        """how every sample() starts (ddim_video.py:84-98): the conditioning warning, the schedule of S steps, the latent's 5-D size"""
        if conditioning is not None and not isinstance(conditioning, dict):
            if conditioning.shape[0] != batch_size:
                print(f"Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        if not is_3d:
            raise NotImplementedError("the Seer hot path is 5-D (is_3d=True, ddim_sampling_utils.py:36)")
        C, Fr, H, W = shape
        return (batch_size, C, Fr, H, W)

    def _chain_start(self, unet, shape, x_T, x0_emb):
        """the latent a chain starts from -- x_T, or torch.randn(shape) -- in fp32 on the sampler's device, and x0_emb on that device.
        One clip sharded over several ranks (parallel.attach): every rank must denoise the SAME latent, so the start code and the
        conditioning latents (a per-rank posterior sample) come from rank 0, like any per-step noise.  A model with its step cache
        enabled begins a chain of evaluations here: the first one runs in full, and nothing an earlier chain kept is read."""
        _begin_cache_chain(unet)
        img = torch.randn(shape, device=self.device) if x_T is None else x_T.to(device=self.device, dtype=torch.float32)
        img = _from_rank0(unet, img)
        if x0_emb is not None:
            x0_emb = _from_rank0(unet, x0_emb.to(self.device))
        return img, x0_emb

    @torch.no_grad()
    def ddim_sampling(self, unet, cond, shape, is_3d, x0_emb=None, cond_frames=0, x_T=None, callback=None,
                      img_callback=None, log_every_t=100, temperature=1., noise_dropout=0.,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, seeds=None, mask=None, x0=None,
                      t_start=None, guidance_rescale=None, **kwargs):
        """`seeds`: None, or one uint64 per batch row (sample's `seed`): the start code (when x_T is None) and the noise of every step
        then come from the rows' Philox streams, nothing from torch's generator.  `mask` (broadcastable to [b, 1, F_pred, h, w], values
        in [0, 1]) with `x0` [b, C, F_pred, h, w]: in front of every step the latent becomes q * mask + (1 - mask) * latent, q = x0
        noised to that step's level (CompVis ddim.py:144-147); the final latent is not blended again.  `t_start` (decode): x_T is the
        latent at that level of the schedule, and the chain runs the indices t_start - 1 ... 0 only."""
        b = shape[0]
        if seeds is not None:
            _refuse_sharded(unet, "seed")
        known = self._known_pair(unet, mask, x0, shape)
        if seeds is not None:
            seeds = list(seeds)
            if len(seeds) != b:
                raise ValueError(f"seeds: {len(seeds)} for a batch of {b}")
            if x_T is None:
                x_T = torch.empty(shape, device=self.device, dtype=torch.float32)
                for row, s in zip(x_T, seeds):           # a row's start code: stream 0 of its own seed
                    self.ops.philox_normal(s, ops.PHILOX_STREAM_START, 0, row.numel(), out=row)
            seeds = ops.seed_words(seeds).to(self.device)
        img, x0_emb = self._chain_start(unet, shape, x_T, x0_emb)
        step = lambda img, index: self.p_sample_ddim(
            unet, img, cond, self._t_table[index].expand(b), index=index, is_3d=is_3d, x0_emb=x0_emb, cond_frames=cond_frames,
            temperature=temperature, noise_dropout=noise_dropout, unconditional_guidance_scale=unconditional_guidance_scale,
            unconditional_conditioning=unconditional_conditioning, seeds=seeds, known=known, guidance_rescale=guidance_rescale)
        return self._run_chain(img, self.ddim_timesteps.shape[0] if t_start is None else int(t_start), step, callback, img_callback,
                               log_every_t)

    def _run_chain(self, img, n_steps, step, callback=None, img_callback=None, log_every_t=100):
        """The loop of a sample: schedule indices n_steps - 1 ... 0 through `step(img, index) -> (img, pred_x0)`, starting from
        `img`, with the reference's callbacks and logged intermediates; returns (a copy of the last latent, the intermediates)."""
        total_steps = self.ddim_timesteps.shape[0]
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        # inside this loop a captured step may hand out its static buffers (nothing here keeps a step's output past the next
        # step without copying it)
        static_before, self.static_step_outputs = self.static_step_outputs, True
        try:
            for i, index in enumerate(reversed(range(n_steps))):
                img, pred_x0 = step(img, index)
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(pred_x0.clone(), i)
                if index % log_every_t == 0 or index == total_steps - 1:
                    intermediates["x_inter"].append(img.clone())
                    intermediates["pred_x0"].append(pred_x0.clone())
        finally:
            self.static_step_outputs = static_before
        return img.clone(), intermediates

    def _known_pair(self, unet, mask, x0, shape):
        """sample's `mask` / `x0` -> None, or (mask fp32 [b, F_pred, h, w], x0 fp32 [b, C, F_pred, h, w]) on the sampler's device, made
        once per call: the captured step keys its static copies on these two tensors"""
        if mask is None and x0 is None:
            return None
        if mask is None or x0 is None:
            raise ValueError("mask and x0 go together: the mask says where the latent is given, x0 what it is there")
        _refuse_sharded(unet, "mask")
        b, Cc, Fp, h, w = shape
        mask = torch.as_tensor(mask)
        if mask.dim() > 5 or (mask.dim() == 5 and mask.shape[1] != 1):
            raise ValueError(f"mask {tuple(mask.shape)}: a mask is shared by a clip's channels, [b, 1, F_pred, h, w] (per-channel masks "
                             "are not built)")
        try:
            mask = torch.broadcast_to(mask, (b, 1, Fp, h, w))
        except RuntimeError:
            raise ValueError(f"mask {tuple(mask.shape)} does not broadcast to {(b, 1, Fp, h, w)}") from None
        if tuple(x0.shape) != tuple(shape):
            raise ValueError(f"x0 {tuple(x0.shape)}: the given latents have the clip's shape {tuple(shape)}")
        return (mask.to(device=self.device, dtype=torch.float32).reshape(b, Fp, h, w).contiguous(),
                x0.to(device=self.device, dtype=torch.float32).contiguous())

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None, seed=None):
        """CompVis ddim.py:207-221 on the current schedule: sqrt(a_t) x0 + sqrt(1 - a_t) noise with t (an int, or an integer tensor
        [b]) indexing the DDIM tables.  `noise` as given; with `seed` (an int: row i takes seed + i, or one per row) Philox stream 2 of
        the row's seed at index t; with neither torch.randn_like(x0)."""
        if use_original_steps:
            raise NotImplementedError("only the DDIM-subsequence path that ddim_sample drives is built")
        if noise is not None and seed is not None:
            raise ValueError("stochastic_encode: `noise` or `seed`, not both")
        x0 = x0.to(device=self.device, dtype=torch.float32).contiguous()
        b, n = x0.shape[0], int(self.ddim_coef.shape[0])
        rows = [int(v) for v in t.reshape(-1).tolist()] if torch.is_tensor(t) else [int(t)]
        if len(rows) == 1:
            rows = rows * b
        if len(rows) != b or any(not 0 <= v < n for v in rows):
            raise ValueError(f"t = {t!r}: one index into the {n} entries of the current schedule, or one per row of {b}")
        index = torch.tensor(rows, dtype=torch.int32, device=self.device)
        if seed is not None:
            return self.ops.q_sample(x0, self.ddim_coef, index, seeds=ops.seed_words(_row_seeds(seed, b)).to(self.device))
        noise = torch.randn_like(x0) if noise is None else noise.to(device=self.device, dtype=torch.float32).contiguous()
        return self.ops.q_sample(x0, self.ddim_coef, index, noise=noise)

    @torch.no_grad()
    def decode(self, unet, x_latent, cond, t_start, unconditional_guidance_scale=1., unconditional_conditioning=None,
               use_original_steps=False, *, x0_emb=None, cond_frames=0, seed=None, temperature=1., mask=None, x0=None,
               guidance_rescale=None):
        """CompVis ddim.py:223-241 with the UNet first, as in sample: indices t_start - 1 ... 0 of the current schedule through
        p_sample_ddim, from x_latent taken as the latent at level t_start.  seed, mask and x0 as in sample."""
        if use_original_steps:
            raise NotImplementedError("only the DDIM-subsequence path that ddim_sample drives is built")
        n = int(self.ddim_timesteps.shape[0])
        if not 1 <= int(t_start) <= n:
            raise ValueError(f"t_start = {t_start}: 1 .. {n}, the entries of the current schedule")
        return self.ddim_sampling(unet, cond, tuple(x_latent.shape), True, x0_emb=x0_emb, cond_frames=cond_frames, x_T=x_latent,
                                  temperature=temperature, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning,
                                  seeds=_row_seeds(seed, x_latent.shape[0]), mask=mask, x0=x0, t_start=t_start,
                                  guidance_rescale=guidance_rescale)[0]

    @torch.no_grad()
    def encode(self, unet, x0, c, t_enc, use_original_steps=False, return_intermediates=None, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, callback=None, *, x0_emb=None, cond_frames=0, guidance_rescale=None):
        """DDIM inversion, CompVis ddim.py encode() on the current schedule with the UNet first, as in sample: the deterministic
        counterpart of stochastic_encode.  x0 [b, C, F_pred, h, w] is taken as the latent at the level of row 0's a_prev; the indices
        0 ... t_enc - 1 run UPWARD through p_invert_ddim, each evaluating the model at its own (the target level's) timestep, and
        the result is the latent at level t_enc: decode(t_start=t_enc) is the exact counterpart.  1 <= t_enc <= the schedule's entries.
        Returns (x_latent, {"x_inter": [...], "pred_x0": [...]}): with return_intermediates = k the lists hold copies of the latent
        and of pred_x0 after every k-th step (steps k - 1, 2k - 1, ...), otherwise they are empty.  callback(i) is called after
        step i.  Inversion is eta = 0 by definition: NO draw is made from torch's generator, which is left where it was.
        Refused (NotImplementedError) with prediction_type="v_prediction": encode evaluates the model at the TARGET level's timestep on
        a latent of the level below, so it is ambiguous which level's coefficients turn v into eps."""
        self._refuse_v_inversion()
        if use_original_steps:
            raise NotImplementedError("only the DDIM-subsequence path that ddim_sample drives is built")
        n = int(self.ddim_timesteps.shape[0])
        if not 1 <= int(t_enc) <= n:
            raise ValueError(f"t_enc = {t_enc}: 1 .. {n}, the entries of the current schedule")
        every = None if return_intermediates is None else int(return_intermediates)
        if every is not None and every < 1:
            raise ValueError(f"return_intermediates = {return_intermediates}: None, or keep every k-th latent with k >= 1")
        t_enc = int(t_enc)
        img, x0_emb = self._chain_start(unet, tuple(x0.shape), x0, x0_emb)
        b = img.shape[0]
        intermediates = {"x_inter": [], "pred_x0": []}
        static_before, self.static_step_outputs = self.static_step_outputs, True
        try:
            for index in range(t_enc):
                img, pred_x0 = self.p_invert_ddim(unet, img, c, self._t_table[index].expand(b), index, x0_emb=x0_emb,
                                                  cond_frames=cond_frames, unconditional_guidance_scale=unconditional_guidance_scale,
                                                  unconditional_conditioning=unconditional_conditioning, limit=t_enc,
                                                  guidance_rescale=guidance_rescale)
                if every is not None and (index + 1) % every == 0:
                    intermediates["x_inter"].append(img.clone())
                    intermediates["pred_x0"].append(pred_x0.clone())
                if callback:
                    callback(index)
        finally:
            self.static_step_outputs = static_before
        return img.clone(), intermediates

    @torch.no_grad()
    def p_invert_ddim(self, unet, x, c, t, index, x0_emb=None, cond_frames=0, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, limit=None, guidance_rescale=None):
        """One step of encode: x at the level of row `index`'s a_prev, the model evaluated at t (encode passes the row's own timestep)
        -> (x_next at the level of a_t, pred_x0).  Nothing is drawn.  `limit`: the number of rows the chain this step belongs to may
        use (encode's t_enc; the whole schedule when None) -- what the captured step's counter stops at.  Refused for a v-model, as
        encode is."""
        self._refuse_v_inversion()
        n = int(self.ddim_coef.shape[0])
        limit = n if limit is None else int(limit)
        if not 0 <= int(index) < limit <= n:
            raise ValueError(f"index = {index}, limit = {limit}: 0 <= index < limit <= {n}, the entries of the current schedule")
        x = x.to(torch.float32).contiguous()
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        # the captured step is gated as p_sample_ddim gates its own: batched CFG or none, and t the schedule table's own entry
        plain = uc is None or scale == 1.
        phi = self._rescale_factor(unet, guidance_rescale, plain)
        if ((plain or uc.shape[2] == c.shape[2]) and torch.is_tensor(t) and t.dtype == torch.long
                and t.data_ptr() == self._t_table.data_ptr() + 8 * int(index)):
            done = self._invert_graph_step(unet, x, c, None if plain else uc, int(index), x0_emb, 0 if plain else cond_frames, scale,
                                           limit, phi=phi)
            if done is not None:
                return done
        eps, cfg, cond_f = self._model_output(unet, x, c, t, x0_emb, cond_frames, uc, scale, cached=False)
        return self.ops.cfg_ddim_invert_step(self._rescaled(eps, scale, cond_f, phi), x, self.ddim_coef, int(index), cfg=cfg,
                                             scale=scale, cond_f=cond_f)

    def _refuse_v_inversion(self):
        if self.prediction_type != "epsilon":
            raise NotImplementedError("DDIM inversion (encode / p_invert_ddim) of a v-prediction model: the step evaluates the model at "
                                      "the target level's timestep on a latent of the level below, so it is ambiguous which level's "
                                      "coefficients convert v to eps")

    def _rescale_factor(self, unet, guidance_rescale, plain):
        """the blend factor phi of guidance rescale for one step: the call's own `guidance_rescale`, else the constructor's; 0 where CFG
        is off (`plain`: there is nothing to rescale).  phi > 0 on a sharded model is refused: a clip's elements, or its two rows, are on
        different ranks there, and the sums are not exchanged."""
        phi = self.guidance_rescale if guidance_rescale is None else ops.check_guidance_rescale(guidance_rescale)
        if plain or phi == 0.:
            return 0.
        _refuse_sharded(unet, "rescale")
        return phi

    def _rescaled(self, out, scale, cond_f, phi):
        """the model output `out` [2b, C, cond_f + F, h, w] as fp32, with guidance rescale applied when phi > 0 (_rescale_factor: CFG
        is on then): both rows of every clip become m * (the guided output), seer_cfg_rescale, in front of _as_eps -- for a v-model it
        is v that is rescaled, as in diffusers.  The rows are written on a tensor of this step's own, never on the model's."""
        res = out.float().contiguous()
        if phi == 0.:
            return res
        if res.data_ptr() == out.data_ptr():
            res = res.clone()
        return self.ops.cfg_rescale(res, scale=scale, rescale=phi, cond_f=cond_f)

    def _as_eps(self, out, x, index, cond_f):
        """the model output `out` [2b or b, C, cond_f + F, h, w] of an evaluation at x and at schedule entry `index`'s timestep, as fp32
        eps for the update kernel: itself, or -- a v-model -- through seer_v_to_eps with row `index` of the DDIM table"""
        out = out.float().contiguous()
        if self.prediction_type == "epsilon":
            return out
        return self.ops.v_to_eps(out, x, self.ddim_coef, int(index), cond_f=cond_f)

    @torch.no_grad()
    def p_sample_ddim(self, unet, x, c, t, index, is_3d=True, x0_emb=None, cond_frames=0, repeat_noise=False,
                      use_original_steps=False, temperature=1., noise_dropout=0., score_corrector=None,
                      corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                      null_cond_prob=None, seeds=None, known=None, guidance_rescale=None):
        """ddim_video.py:183-238.  `seeds` (int32 [b, 2] on x's device, ops.seed_words; not in the reference): the step's noise is
        drawn inside its last kernel from the rows' seeds and `index`, and torch's generator is left alone.  `known` (_known_pair's
        mask and given latents; not in the reference either): the mask blend of CompVis ddim.py:144-147 in front of the step, on a
        copy of x -- with seeds a node of the captured step, its noise stream 2 of the rows' seeds; without, a torch.randn drawn
        before the step's own draw, as CompVis orders them."""
        if use_original_steps or noise_dropout > 0. or repeat_noise:
            raise NotImplementedError("only the DDIM-subsequence path that ddim_sample drives is built")
        x = x.to(torch.float32).contiguous()
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        sigma = float(self.ddim_sigmas[index])
        if known is not None and seeds is None:
            x = self.ops.known_blend(x.clone(), known[0], known[1], self.ddim_coef, index, noise=torch.randn(x.shape, device=x.device))
            known = None
        # the whole step -- input assembly, CFG-batched UNet, CFG combine, DDIM update -- as ONE replayed hipGraph when the step is the
        # one ddim_sample drives: batched CFG or none, eta = 0 or a seed, and t = the schedule's own timestep of `index` (recognised by
        # its address: a view of the device timestep table).  Whether the model's steps may be captured at all is _step_graph's question.
        plain = uc is None or scale == 1.
        phi = self._rescale_factor(unet, guidance_rescale, plain)
        if ((sigma == 0. or seeds is not None) and (plain or uc.shape[2] == c.shape[2]) and torch.is_tensor(t) and t.dtype == torch.long
                and t.data_ptr() == self._t_table.data_ptr() + 8 * int(index)):
            done = self._graph_step(unet, x, c, None if plain else uc, index, x0_emb, 0 if plain else cond_frames, scale,
                                    seeds=seeds, temperature=temperature, known=known, phi=phi)
            if done is not None:
                return done
        if known is not None:
            x = self.ops.known_blend(x.clone(), known[0], known[1], self.ddim_coef, index, seeds=seeds)
        eps, cfg, cond_f = self._model_output(unet, x, c, t, x0_emb, cond_frames, uc, scale)
        eps = self._as_eps(self._rescaled(eps, scale, cond_f, phi), x, index, cond_f)
        if seeds is not None:
            return self.ops.cfg_ddim_step_rng(eps, x, self.ddim_coef, index, seeds, cfg=cfg, scale=scale,
                                              cond_f=cond_f, temperature=temperature)
        noise = None
        if sigma != 0. or self.consume_rng_when_deterministic:
            noise = torch.randn(x.shape, device=x.device) * temperature
            if sigma != 0.:
                noise = _from_rank0(unet, noise)
        return self.ops.cfg_ddim_step(eps, x, self.ddim_coef, index, cfg=cfg, scale=scale, cond_f=cond_f,
                                      noise=noise if sigma != 0. else None)

    def _model_output(self, unet, x, c, t, x0_emb, cond_frames, uc, scale, cached=True):
        """the model call of p_sample_ddim (ddim_video.py:187-207): x0_emb in front of x along frames, batched CFG when uc has c's
        frame count, two calls otherwise.  Returns (eps [2b or b, C, cond_f + F, h, w], cfg, cond_f): the CFG combine and the
        slicing off of the conditioning frames are the update kernel's.  For a v-model "eps" is v: the caller passes it through _as_eps.
        A SeerUNet with its step cache enabled is handed the phase of this evaluation (`cache_phase`, one next() of its policy) where
        the step makes ONE model call; the two calls of unbatched CFG, and inversion (cached=False), run in full and leave the cache
        alone.  Any other model is called as it always was."""
        cond_f = 0
        x_cat = x
        if x0_emb is not None:
            cond_f = x0_emb.shape[2]
            x_cat = torch.cat([x0_emb.to(x.dtype), x], dim=2)
        t = t.to(torch.long)
        pol = policy_of(unet) if cached and (uc is None or scale == 1. or uc.shape[2] == c.shape[2]) else None
        phase = {} if pol is None else {"cache_phase": pol.next()[0]}
        if uc is None or scale == 1.:
            eps = unet(x_cat, t, c, **phase)
            cfg = False
        elif uc.shape[2] == c.shape[2]:
            eps = unet(torch.cat([x_cat] * 2), torch.cat([t] * 2), self._cfg_context(c, uc), cond_frame=cond_frames, **phase)
            cfg = True
        else:
            e_uc = unet(x_cat, t, uc, cond_frame=cond_frames)
            e_c = unet(x_cat, t, c, cond_frame=cond_frames)
            eps = torch.cat([e_uc, e_c])
            cfg = True
        return eps, cfg, cond_f

    # ---- the captured step -----------------------------------------------------------------------------------------
    def _graph_step(self, unet, x, c, uc, index, x0_emb, cond_frames, scale, seeds=None, temperature=1., known=None, phi=0.):
        """One p_sample_ddim as a single hipGraph replay (seer_ddim_step_begin -> the UNet's kernels -> seer_cfg_ddim_step):
        no torch kernel between two UNet evaluations except the reference's per-step RNG draw, no host-written scalars -- the
        schedule index lives in device memory and the captured step counts it down itself.  Returns None when this step cannot
        take the path (sharded model, capture refused): the caller then runs the launches one by one.  With `seeds` the last kernel
        is the same entry point given seeds and the step draws nothing, at any eta.  With `known` (seeded only) seer_known_blend is the
        step's first node, over static copies of the mask and the given latents."""
        kind = "step" if seeds is None else "step-rng" if known is None else "step-mask"
        G = self._step_graph(unet, x, c, uc, x0_emb, cond_frames, scale, kind, None if seeds is None else float(temperature), phi=phi)
        if G is None:
            return None
        if seeds is not None:
            refresh(G["kept"], "seeds", (seeds,), (G["seeds"],))
        if known is not None:
            refresh(G["kept"], "known", known, (G["mask"], G["known"]))
        if G["expect"] != index:
            G["step"][:1].fill_(int(index))         # start of a chain (or a caller that jumps): the only host-written index
        return self._replay_step(G, x, index, draw=seeds is None)

    def _invert_graph_step(self, unet, x, c, uc, index, x0_emb, cond_frames, scale, limit, phi=0.):
        """One p_invert_ddim as a single hipGraph replay (seer_ddim_step_begin -> the UNet's kernels -> seer_cfg_ddim_invert_step).
        The captured step counts its index UPWARD and stops writing at the limit word of its static buffers; at the start of a chain
        the host writes those two words, step[0] and limit[0], and nothing after.  None when the step cannot be captured."""
        G = self._step_graph(unet, x, c, uc, x0_emb, cond_frames, scale, "invert", phi=phi)
        if G is None:
            return None
        if G["expect"] != index or G["limit_host"] != limit:
            G["step"][:1].fill_(index)
            G["limit"].fill_(limit)
            G["limit_host"] = limit
        return self._replay_step(G, x, index, draw=False, direction=1)

    def _replay_step(self, G, x, index, draw=True, direction=-1):
        """`direction`: where the captured step's last kernel leaves the counter, index - 1 for every sampling kind, index + 1 for
        "invert"; G["expect"] follows it, so that a chain's later steps find the index they need already in device memory."""
        if draw and self.consume_rng_when_deterministic:
            torch.randn(x.shape, device=x.device)   # ddim_video.py:234 draws every step, also at sigma = 0: keep the RNG stream
        (G["graph_cached"] if G.get("phase") else G["graph"]).replay()      # (_step_graph left this evaluation's phase there)
        G["expect"] = index + direction
        if self.static_step_outputs:
            return G["x"], G["pred"]
        return G["x"].clone(), G["pred"].clone()

    def _cfg_context(self, c, uc):
        """the batched-CFG context [uc, c]: ONE tensor per (c, uc) pair, because its identity keys the UNet's cross-attention K|V cache
        and graph.  Renewed when the caller brings another pair, as step_graph.refresh would: by a fresh concatenation, not a copy."""
        if changed(self._kept, "cfg", (c, uc)):
            self._cfg_cat = torch.cat([uc, c]).contiguous()
        return self._cfg_cat

    def _step_graph(self, unet, x, c, uc, x0_emb, cond_frames, scale, kind, temperature=None, phi=0.):
        """the captured step of this kind / shape / CFG / scale (captured on first use) with x and its read-by-address inputs
        refreshed; None when the step cannot be captured.  `kind` is the key's first word and an entry of STEP_KINDS.  A seeded kind
        comes with its temperature, the key's last field: like the guidance scale it is an argument of the last kernel and frozen
        into the capture; seeds, mask and given latents live in static buffers and are no part of the key.  A v-model's step has one
        more node and "v_prediction" as the key's last word of its own; the default's keys are what they were.  `phi` (_rescale_factor:
        0 unless CFG is on) > 0 is guidance rescale, one more node in front of that one and ("rescale", phi) as the key's trailing words:
        phi is a kernel argument frozen into the capture, like the guidance scale."""
        eng = None if self._capture_refused else capture_engine(unet, self.ops, x.device)
        if eng is None:
            return None
        cfg = uc is not None
        pol = None if kind == "invert" else policy_of(unet)      # step caching: inversion runs every step in full
        context = self._cfg_context(c, uc) if cfg else c
        b, Cc, Fp, h, w = x.shape
        f1 = 0 if x0_emb is None else x0_emb.shape[2]
        reps = 2 if cfg else 1
        if context.dim() == 3:
            context = context[:, None].expand(-1, f1 + Fp, -1, -1)
        if context.shape[0] != reps * b or context.shape[1] != f1 + Fp or h % 8 or w % 8:
            return None
        ctx, L = eng._context(context)          # new prompt: the static context / K|V buffers are refreshed in place
        # (the guidance scale is only part of a CFG step: a plain step at another scale is the same graph)
        key = (kind, (b, Cc, Fp, h, w), f1, cfg, int(cond_frames), float(scale) if cfg else None, L, tuple(ctx.shape), eng.inv,
               *(() if temperature is None else (float(temperature),)),
               *(() if self.prediction_type == "epsilon" else (self.prediction_type,)),
               *(("rescale", float(phi)) if cfg and phi > 0. else ()), *getattr(eng, "freeu_key", ()),
               *(() if pol is None else eng.step_cache_key))
        G = eng.graph_get(key)
        if G is None:
            G = self._capture_step(eng, key, x, x0_emb, reps, cfg, int(cond_frames), float(scale), temperature, ctx, L,
                                   phi=float(phi) if cfg else 0., cached=pol is not None)
            if G is None:
                return None
        n = self.ddim_coef.shape[0]
        if n > G["coef"].shape[0]:
            return None                             # a longer schedule than the one captured for: take the eager path
        # inputs that are read by address: refreshed in place when the caller brings new ones (once per sample / per schedule)
        if x0_emb is not None:
            refresh(G["kept"], "x0_emb", (x0_emb,), (G["x0"],))
        if refresh(G["kept"], "schedule", (self.ddim_coef, self._t_table), (G["coef"][:n], G["ttab"][:n])):
            G["expect"] = None
        if x is not G["x"] and x.data_ptr() != G["x"].data_ptr():
            G["x"].copy_(x)
        # step caching, last of all (from here on the caller replays): the phase of this evaluation picks the graph, and the host's
        # half of it -- the count of valid slots, a cached phase's weights into the device buffer -- is done as for a launched one
        G["phase"] = None
        if pol is not None:
            G["phase"], weights = pol.next()
            eng.cache_note(reps * b * (f1 + Fp) * h * w, G["phase"], weights)
        return G

    def _capture_step(self, eng, key, x, x0_emb, reps, cfg, cond_frames, scale, temperature, ctx, L, phi=0., cached=False):
        """the step of kind key[0] over fresh static buffers, captured and put under `key`; None when the capture is refused.  phi > 0:
        the rescale node sits behind the model and in front of the v-conversion, its workspace one more static buffer.  cached (step
        caching): TWO graphs over the one set of buffers, the step around a full evaluation that keeps its cut feature and the step
        around a cached one -- counter, solver state and latents are shared, the update kernels are the same.  Warm-up and capture
        may come in the middle of a chain (PLMS captures at its second step): the ring is put back afterwards."""
        dev = x.device
        b, Cc, Fp, h, w = x.shape
        f1 = 0 if x0_emb is None else x0_emb.shape[2]
        nsched = max(int(self.ddim_coef.shape[0]), 64)
        buffers, front, update = STEP_KINDS[key[0]]
        G = dict(x=torch.empty_like(x), pred=torch.empty_like(x),
                 x0=(torch.empty_like(x0_emb, dtype=torch.float32).contiguous() if x0_emb is not None else None),
                 sample=torch.empty((reps * b, Cc, f1 + Fp, h, w), device=dev, dtype=torch.float32),
                 t=torch.empty((reps * b,), device=dev, dtype=torch.long), step=torch.zeros((2,), device=dev, dtype=torch.int32),
                 coef=torch.zeros((nsched, 4), device=dev, dtype=torch.float32),
                 ttab=torch.zeros((nsched,), device=dev, dtype=torch.long), expect=None, **buffers(x),
                 kept={})                            # step_graph.refresh's record of what the static buffers were last filled from
        if phi > 0.:
            G["rescale_ws"] = ops.cfg_rescale_workspace(b, Cc, f1 + Fp, f1, h * w, dev)
        G["coef"][:, 0] = 1.0                        # a_t = 1 in the unused rows: the warm-up below must stay finite
        G["x"].copy_(x)
        if x0_emb is not None:
            G["x0"].copy_(x0_emb)

        def body(phase=0 if cached else None):
            for launch in front:
                launch(G)
            ops.ddim_step_begin(G["x0"], G["x"], G["ttab"], G["step"], reps, G["sample"], G["t"])
            eps = eng._forward(G["sample"], G["t"], ctx, L, cond_frames, cache_phase=phase)
            if phi > 0.:                                # in place, on the engine's output buffer, both rows of every clip
                ops.cfg_rescale(eps, scale=scale, rescale=phi, cond_f=f1, ws=G["rescale_ws"])
            if self.prediction_type != "epsilon":       # in place as well: nothing is allocated for it
                ops.v_to_eps_dev(eps, G["x"], G["coef"], G["step"], cond_f=f1, out=eps)
            update(G, eps, temperature, cfg=cfg, scale=scale, cond_f=f1)
        ring = eng.cache_set(G["sample"].numel() // Cc)["ring"] if cached else None
        ring_was = None if ring is None else ring.clone()
        done = capture_step(eng, key, G, body, **({"cached_body": lambda: body(1)} if cached else {}))
        if ring is not None:
            ring.copy_(ring_was)
        if done is None:
            self._capture_refused = True
            return None
        return G


# ---- the kinds of a captured step --------------------------------------------------------------------------------------------------
def _seed_buffers(x):
    return dict(seeds=torch.zeros((x.shape[0], 2), device=x.device, dtype=torch.int32))


def _mask_buffers(x):
    """an all-zero mask through warm-up and capture: the blend writes nothing there, whatever the step words hold; the caller's mask
    and latents are copied in by _graph_step afterwards"""
    b, _, Fp, h, w = x.shape
    return dict(_seed_buffers(x), mask=torch.zeros((b, Fp, h, w), device=x.device, dtype=torch.float32), known=torch.zeros_like(x))


def _blend(G):
    ops.known_blend(G["x"], G["mask"], G["known"], G["coef"], step=G["step"], seeds=G["seeds"])


def _ddim_update(G, eps, temperature, **kw):
    ops.cfg_ddim_step_dev(eps, G["x"], G["coef"], G["step"], x_prev=G["x"], pred_x0=G["pred"], **kw)


def _rng_update(G, eps, temperature, **kw):
    ops.cfg_ddim_step_rng_dev(eps, G["x"], G["coef"], G["step"], G["seeds"], temperature=temperature, x_prev=G["x"],
                              pred_x0=G["pred"], **kw)


def _limit_buffers(x):
    """the word the upward counter stops at.  It is 0 through warm-up and capture, so that they write no element: the unused rows of
    the static table hold a_prev = 0, which the inversion update divides by.  It lives in device memory because a replay's kernel
    arguments are frozen; _invert_graph_step writes it, with the start index, once per chain."""
    return dict(limit=torch.zeros((1,), device=x.device, dtype=torch.int32), limit_host=None)


def _invert_update(G, eps, temperature, **kw):
    ops.cfg_ddim_invert_step_dev(eps, G["x"], G["coef"], G["step"], G["limit"], x_next=G["x"], pred_x0=G["pred"], **kw)


# kind (the first word of the graph-cache key) -> (its static buffers, its launches in front of seer_ddim_step_begin, its last kernel).
# The step between the two is the same for every kind; plms.py adds "plms", dpm.py "dpm".
STEP_KINDS = {"step": (lambda x: {}, (), _ddim_update),
              "step-rng": (_seed_buffers, (), _rng_update),
              "step-mask": (_mask_buffers, (_blend,), _rng_update),
              "invert": (_limit_buffers, (), _invert_update)}


def _begin_cache_chain(unet) -> None:
    """a chain of model evaluations begins: the step cache's policy, and the engine's count of valid slots, start over"""
    pol = policy_of(unet)
    if pol is not None:
        pol.begin()
        if unet._engine is not None:
            unet._engine.cache_begin()


def _refuse_sharded(unet, what: str) -> None:
    """what one clip sharded over several ranks (parallel.attach) cannot do"""
    if getattr(unet, "_shard", None) is not None:
        raise ValueError({"seed": "seed: a frame-sharded model draws its noise on rank 0 (detach it, parallel.attach, to sample from a seed)",
                          "mask": "mask: a frame-sharded model cannot blend given latents (detach it, parallel.attach)",
                          "rescale": "guidance_rescale: a sharded model holds a clip's elements, or its two CFG rows, on different ranks, "
                                     "and the sums are not exchanged (detach it, parallel.attach, or sample with guidance_rescale=0)"}[what])


def _row_seeds(seed, batch_size: int):
    """sample()'s `seed` -> one uint64 per batch row, or None: an int s gives row i the seed s + i, a sequence is taken as it is"""
    if seed is None:
        return None
    if isinstance(seed, (int, np.integer)):
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"seed: {seed!r}: a seed is an unsigned 64-bit integer")
        seeds = [(int(seed) + i) & 0xffffffffffffffff for i in range(int(batch_size))]
    else:
        seeds = [int(s) for s in seed]
        if len(seeds) != int(batch_size):
            raise ValueError(f"seed: {len(seeds)} seeds for batch_size = {batch_size}")
    if any(not 0 <= s < 1 << 64 for s in seeds):
        raise ValueError(f"seed: {seed!r}: a seed is an unsigned 64-bit integer")
    return seeds


def _from_rank0(unet, t: torch.Tensor) -> torch.Tensor:
    """broadcast `t` from rank 0 when `unet` runs one clip sharded over several ranks; identity otherwise"""
    shard = getattr(unet, "_shard", None)
    if shard is None or shard.world <= 1:
        return t
    import torch.distributed as dist
    t = t.contiguous()
    dist.broadcast(t, src=0)
    return t


@torch.no_grad()
def ddim_sample(sampler, unet, vae, shape, c, start_code, x0_emb, ddim_steps=10, scale=1.0, uc=None):
    """utils/ddim_sampling_utils.py:21-42: sampler -> 1/0.18215 -> vae.decode -> clamp((x+1)/2, 0, 1)."""
    if scale == 1.0:
        uc = None
    samples_ddim, _ = sampler.sample(unet=unet, S=ddim_steps, conditioning=c, batch_size=shape[0], shape=shape[1:],
                                     x0_emb=x0_emb, verbose=False, unconditional_guidance_scale=scale,
                                     unconditional_conditioning=uc, eta=0.0, x_T=start_code, is_3d=True)
    return latents_to_clip(vae, samples_ddim)


def latents_to_clip(vae, latents: torch.Tensor) -> torch.Tensor:
    """latents [n, C, f, h, w] -> 1/0.18215 -> vae.decode of the n * f frames -> clip [n, 3, f, H, W], clamp((x + 1) / 2, 0, 1)"""
    n, ch, f, h, w = latents.shape
    z = (latents.permute(0, 2, 1, 3, 4).reshape(n * f, ch, h, w) * (1 / 0.18215)).contiguous()
    x = vae.decode(z).sample
    x = x.reshape(n, f, *x.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()
    return ops.clamp01_(x.float())


def frames_to_latents(vae, frames: torch.Tensor, generator=None) -> torch.Tensor:
    """frames [b, 3, f, H, W] in [-1, 1] -> vae.encode of the b * f frames, one draw of the posterior from `generator`, * 0.18215 ->
    latents [b, C, f, H/8, W/8] (inference_img.py:166-170)"""
    b, ch, f, H, W = frames.shape
    lat = vae.encode(frames.permute(0, 2, 1, 3, 4).reshape(b * f, ch, H, W)).latent_dist.sample(generator=generator) * 0.18215
    return lat.reshape(b, f, *lat.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()
