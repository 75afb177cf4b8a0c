"""DPMSolverSampler -- DPM-Solver++ (Lu et al. 2022), the second-order multistep solver "2M" and its first-order form, on the Seer
model call.  Not in the reference: its samplers are DDIM and PLMS.

The probability-flow ODE is integrated in lambda = log(alpha / sigma), half the log-SNR, with the data prediction D = (x - sigma eps)
/ alpha held constant (first order) or extrapolated linearly from the previous step's (2M) over a step, and the linear part solved
exactly.  One model evaluation per step at either order.  With alpha = sqrt(abar), sigma = sqrt(1 - abar), a step from the level s of
schedule entry i (ddim_alphas[i]) to the level t of ddim_alphas_prev[i], h_i = lambda_t - lambda_s:

    first order   x_prev = (sigma_t / sigma_s) x - alpha_t (exp(-h_i) - 1) D_i              (algebraically the eta = 0 DDIM update)
    2M            the same with D_i replaced by D_i + (D_i - D_(i+1)) / (2 r),  r = h_(i+1) / h_i

(entry i + 1 is the step before: a chain walks the indices downward).  A step is first order when it has no history -- the first of a
chain -- with order=1, and, under lower_order_final (the default, the rule of the original DPM-Solver code), as the final step of a
schedule of fewer than 15 entries.  The last step lands on alphas_cumprod[0] like DDIM's, where sigma is not 0: lambda is finite and
the step is like any other.

Same constructor arguments (plus order, lower_order_final, discretize), `sample(...)` keywords and return values as DDIMSampler, so
ddim_sample, pipeline.generate_clips, pipeline.evaluate_batch and pipeline.edit_clips(strength=) take it.  The tables are
DDIMSampler.make_schedule's, over the 'uniform' stride or -- discretize="logsnr" -- over training steps evenly spaced in lambda;
`encode` and `stochastic_encode` are DDIMSampler's as they are.  pred_x0 of a step is D_i, as for DDIM and PLMS.

Kernels: CFG combine + update are one fused HIP kernel (seer_cfg_dpm_step; include/seer_hip.h) that reads six host-computed words per
schedule entry and evaluates no exp or log.  With `unet.use_graph` on an unsharded SeerUNet EVERY step, the first included, is one
hipGraph replay -- seer_ddim_step_begin, the UNet, seer_cfg_dpm_step -- captured by DDIMSampler's machinery under the kind "dpm";
the history is the step's own pred_x0 buffer, and the kernel picks its order from words in device memory, so a chain of replays needs
no host-written scalar after its first step.

prediction_type="v_prediction" (DDIMSampler's keyword) converts the model's v with the DDIM coefficient rows of this sampler's own
timesteps, the log-SNR grid included, in front of either form of the step.  `guidance_rescale` (DDIMSampler's keyword; per call on
sample, decode and p_sample_dpm) rescales the guided model output in front of that, in either form of the step as well.

Only the deterministic solver is built: no mask / x0, no seed, no eta > 0 (the SDE variant), no noise_dropout, no order 3, no
singlestep (2S) form.  The per-step torch.randn draw of the reference's samplers is kept (consume_rng_when_deterministic), as in
PLMSSampler.  A queue of clips runs this solver through SlotSampler(dpm=True) (slots.py): submit(method="dpmpp") with this
constructor's order, lower_order_final and discretize, bit for bit this sampler's latent under the layout-invariant mode.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .ddim import STEP_KINDS, DDIMSampler
from .step_graph import refresh

BUILT = "DPMSolverSampler builds the deterministic DPM-Solver++ chain only (order 1 or 2M, eta = 0)"


def logsnr_timesteps(n_sample: int, alphas_cumprod: torch.Tensor) -> np.ndarray:
    """Training steps evenly spaced in lambda(t) = log(abar_t / (1 - abar_t)) / 2 over the fp32 table of every training step: n_sample
    targets from lambda(1) to lambda(last), each mapped to the nearest training step in 1 .. last, duplicates dropped, ascending.
    There may be fewer than n_sample (the targets crowd where lambda is steep)."""
    ac = alphas_cumprod.double().numpy()
    if int(n_sample) < 1 or ac.shape[0] < 2:
        raise ValueError(f"{n_sample} sampling steps over {ac.shape[0]} training steps")
    lam = 0.5 * np.log(ac / (1. - ac))
    steps = np.arange(1, ac.shape[0])
    targets = np.linspace(lam[1], lam[-1], int(n_sample))
    nearest = np.abs(lam[steps][None, :] - targets[:, None]).argmin(axis=1)
    return np.unique(steps[nearest]).astype(np.int64)


def dpm_table(alphas: np.ndarray, alphas_prev: np.ndarray) -> np.ndarray:
    """float64 [n, 6], a row per schedule entry (include/seer_hip.h, seer_cfg_dpm_step):
    (sigma_s, 1 / alpha_s, c_x, c_D1, c_D2, c_Dprev).  The top entry has no entry above it: its last two words are (c_D1, 0)."""
    a_s, a_t = np.asarray(alphas, dtype=np.float64), np.asarray(alphas_prev, dtype=np.float64)
    alpha_s, sigma_s, alpha_t, sigma_t = np.sqrt(a_s), np.sqrt(1. - a_s), np.sqrt(a_t), np.sqrt(1. - a_t)
    h = np.log(alpha_t / sigma_t) - np.log(alpha_s / sigma_s)
    c_d1 = -alpha_t * np.expm1(-h)
    half_inv_r = np.zeros_like(h)
    half_inv_r[:-1] = h[:-1] / (2. * h[1:])                       # 1 / (2 r_i), r_i = h_(i+1) / h_i
    return np.stack([sigma_s, 1. / alpha_s, sigma_t / sigma_s, c_d1, c_d1 * (1. + half_inv_r), -c_d1 * half_inv_r], 1)


class DPMSolverSampler(DDIMSampler):
    def __init__(self, device, timesteps=1000, schedule="linear", order=2, lower_order_final=True, discretize="uniform", **kwargs):
        super().__init__(device, timesteps=timesteps, schedule=schedule, **kwargs)
        if order not in (1, 2):
            raise NotImplementedError(f"order = {order!r}: {BUILT}")
        self.order = int(order)
        self.lower_order_final = bool(lower_order_final)
        self.discretize = discretize

    def make_schedule(self, ddim_num_steps, *args, ddim_eta=0., **kwargs):
        """DDIMSampler.make_schedule (over the 'uniform' stride or the log-SNR grid), then the DPM table: computed in float64, uploaded
        once per schedule as fp32 [entries, 6]"""
        if ddim_eta != 0:
            raise ValueError(f"ddim_eta = {ddim_eta}: {BUILT}")
        if self.discretize not in ("uniform", "logsnr"):
            raise NotImplementedError(f"discretize = {self.discretize!r}: 'uniform' (the reference's stride) or 'logsnr'")
        super().make_schedule(ddim_num_steps, *args, ddim_eta=ddim_eta, **kwargs)
        self.dpm_coef = torch.tensor(dpm_table(self.ddim_alphas, self.ddim_alphas_prev), dtype=torch.float32, device=self.device)

    def _sampling_timesteps(self, n_sample, alphas_cumprod):
        if self.discretize == "logsnr":
            return logsnr_timesteps(n_sample, alphas_cumprod)
        return super()._sampling_timesteps(n_sample, alphas_cumprod)

    def _final_first_order(self) -> bool:
        """lower_order_final: the final step (index 0) of a schedule of fewer than 15 entries is first order"""
        return self.lower_order_final and int(self.ddim_timesteps.shape[0]) < 15

    def step_order(self, index: int, has_history: bool) -> int:
        """the order of the step at schedule entry `index`, given whether the step before left its data prediction"""
        if not has_history or self.order == 1 or int(index) >= int(self.ddim_timesteps.shape[0]) - 1:
            return 1
        return 1 if int(index) == 0 and self._final_first_order() else 2

    @torch.no_grad()
    def sample(self, unet, S, batch_size, shape, x0_emb=None, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, eta=0., mask=None, x0=None, cond_frames=0, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, null_cond_prob=None, is_3d=False,
               **kwargs):
        if mask is not None or x0 is not None:
            raise NotImplementedError(f"mask / x0 (masked sampling): {BUILT}")
        if kwargs.get("seed") is not None:
            raise NotImplementedError(f"seed: nothing is drawn at eta = 0; {BUILT}")
        if eta != 0:
            raise ValueError(f"eta = {eta}: {BUILT}")
        if noise_dropout > 0.:
            raise NotImplementedError(f"noise_dropout: {BUILT}")
        size = self._sample_size(S, batch_size, shape, conditioning, eta, verbose, is_3d)
        return self.dpm_sampling(unet, conditioning, size, x0_emb=x0_emb, callback=callback, img_callback=img_callback,
                                 cond_frames=cond_frames, x_T=x_T, log_every_t=log_every_t,
                                 unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=unconditional_conditioning,
                                 guidance_rescale=kwargs.get("guidance_rescale"))

    @torch.no_grad()
    def dpm_sampling(self, unet, cond, shape, x0_emb=None, cond_frames=0, x_T=None, callback=None, img_callback=None,
                     log_every_t=100, unconditional_guidance_scale=1., unconditional_conditioning=None, t_start=None,
                     guidance_rescale=None, **kwargs):
        """the chain over the indices n - 1 ... 0 of the current schedule (t_start - 1 ... 0 with `t_start`: x_T is then the latent at
        that level), every step one captured replay where the step can be captured, launch by launch (p_sample_dpm) where not"""
        b = shape[0]
        img, x0_emb = self._chain_start(unet, shape, x_T, x0_emb)
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        plain = uc is None or scale == 1.
        batched = plain or uc.shape[2] == cond.shape[2]
        phi = self._rescale_factor(unet, guidance_rescale, plain)
        d_prev, chained = None, False

        def step(img, index):
            nonlocal d_prev, chained
            out = None
            if batched:
                out = self._dpm_graph_step(unet, img, cond, None if plain else uc, index, x0_emb, 0 if plain else cond_frames, scale,
                                           restart=not chained, phi=phi)
            chained = out is not None
            if out is None:
                out = self.p_sample_dpm(unet, img, cond, self._t_table[index].expand(b), index, x0_emb=x0_emb, cond_frames=cond_frames,
                                        unconditional_guidance_scale=scale, unconditional_conditioning=uc, d_prev=d_prev,
                                        guidance_rescale=phi)
            d_prev = out[1]
            return out
        return self._run_chain(img, self.ddim_timesteps.shape[0] if t_start is None else int(t_start), step, callback, img_callback,
                               log_every_t)

    @torch.no_grad()
    def p_sample_dpm(self, unet, x, c, t, index, is_3d=True, x0_emb=None, cond_frames=0, repeat_noise=False,
                     use_original_steps=False, quantize_denoised=False, temperature=1., noise_dropout=0., score_corrector=None,
                     corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None, d_prev=None,
                     guidance_rescale=None):
        """One step, launch by launch (seer_cfg_dpm_step) -> (x_prev, pred_x0).  `d_prev`: the pred_x0 the step at index + 1
        returned, None for the first step of a chain; the order follows from it (step_order)."""
        if use_original_steps or noise_dropout > 0. or repeat_noise or quantize_denoised or score_corrector is not None:
            raise NotImplementedError(BUILT + ", over the schedule's own entries")
        x = x.to(torch.float32).contiguous()
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        order = self.step_order(index, d_prev is not None)
        phi = self._rescale_factor(unet, guidance_rescale, uc is None or scale == 1.)
        eps, cfg, cond_f = self._model_output(unet, x, c, t, x0_emb, cond_frames, uc, scale)
        if self.consume_rng_when_deterministic:
            torch.randn(x.shape, device=x.device)       # the reference's samplers draw in every update, also at sigma = 0
        eps = self._as_eps(self._rescaled(eps, scale, cond_f, phi), x, index, cond_f)
        return self.ops.cfg_dpm_step(eps, x, self.dpm_coef, int(index), order, cfg=cfg, scale=scale, cond_f=cond_f,
                                     d_prev=d_prev.to(torch.float32).contiguous() if order == 2 else None)

    def p_sample_ddim(self, *args, **kwargs):
        raise NotImplementedError("DPMSolverSampler steps with p_sample_dpm")

    def ddim_sampling(self, *args, **kwargs):
        raise NotImplementedError("DPMSolverSampler samples with dpm_sampling")

    @torch.no_grad()
    def decode(self, unet, x_latent, cond, t_start, unconditional_guidance_scale=1., unconditional_conditioning=None,
               use_original_steps=False, *, x0_emb=None, cond_frames=0, seed=None, temperature=1., mask=None, x0=None,
               guidance_rescale=None):
        """SDEdit's downward half (DDIMSampler.decode) with this solver: indices t_start - 1 ... 0 of the current schedule from x_latent
        taken as the latent at level t_start, first order on its first step.  Nothing is drawn, so `seed` (what edit_clips hands
        every decode) and `temperature` have nothing to act on."""
        if use_original_steps:
            raise NotImplementedError(BUILT + ", over the schedule's own entries")
        if mask is not None or x0 is not None:
            raise NotImplementedError(f"mask / x0 (masked sampling): {BUILT}")
        n = int(self.ddim_timesteps.shape[0])
        if not 1 <= int(t_start) <= n:
            raise ValueError(f"t_start = {t_start}: 1 .. {n}, the entries of the current schedule")
        return self.dpm_sampling(unet, cond, tuple(x_latent.shape), x0_emb=x0_emb, cond_frames=cond_frames, x_T=x_latent,
                                 unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=unconditional_conditioning, t_start=t_start,
                                 guidance_rescale=guidance_rescale)[0]

    def _dpm_graph_step(self, unet, x, c, uc, index, x0_emb, cond_frames, scale, restart, phi=0.):
        """One step as a single replay.  `restart` (the first step of a chain), a counter that is not where this step needs it, or a
        new schedule: the host writes the index and the four state words -- history invalid, the order, the final-step rule -- and
        the step runs first order; these are the only host writes of a chain.  Returns None when the step cannot be captured."""
        G = self._step_graph(unet, x, c, uc, x0_emb, cond_frames, scale, "dpm", phi=phi)
        if G is None:
            return None
        n = self.dpm_coef.shape[0]
        if refresh(G["kept"], "dpm", (self.dpm_coef,), (G["dpm_coef"][:n],)):
            G["expect"] = None
        words = (self.order, int(self._final_first_order()))
        if restart or G["expect"] != index or G["dpm_words"] != words:
            G["step"][:1].fill_(int(index))
            G["dpm_state"].copy_(torch.tensor([0, 0, *words], dtype=torch.int32))
            G["dpm_words"] = words
        return self._replay_step(G, x, index)


# ---- the captured step: DDIMSampler's, with the DPM table and four state words, and seer_cfg_dpm_step as its last kernel -------------
def _dpm_buffers(x):
    """the table is made by the step's first run (the warm-up, outside the capture), where G["coef"], whose row count it shares, exists"""
    return dict(dpm_coef=None, dpm_state=torch.zeros((4,), device=x.device, dtype=torch.int32), dpm_words=None)


def _dpm_update(G, eps, temperature, **kw):
    if G["dpm_coef"] is None:
        # all zero through warm-up and capture: every D and latent they write is 0, whatever the step words hold
        G["dpm_coef"] = torch.zeros((G["coef"].shape[0], ops.DPM_ROW_WORDS), device=eps.device, dtype=torch.float32)
    ops.cfg_dpm_step_dev(eps, G["x"], G["dpm_coef"], G["step"], G["dpm_state"], x_prev=G["x"], d_hist=G["pred"], **kw)


STEP_KINDS["dpm"] = (_dpm_buffers, (), _dpm_update)
