"""PLMSSampler -- pseudo linear multistep sampling (ldm/models/diffusion/plms.py, the PNDM paper's PLMS) on the Seer model call.

The update is the reference's p_sample_plms: the first step evaluates twice (a provisional DDIM step to t_next, then the mean of
the two eps: improved Euler), every later step once, combining its eps with the last one, two or three earlier ones by the
Adams-Bashforth weights.  The model call is Seer's (ddim_video.py:187-207, DDIMSampler._model_output): x0_emb in front of the
latent along frames, batched or unbatched CFG by uc's frame count, cond_frame.  The reference's PLMSSampler drives a 4-D
`model.apply_model` and cannot run a SeerUNet.

Same constructor, `sample(...)` keywords and return values as DDIMSampler, so ddim_sample, pipeline.generate_clips and
pipeline.evaluate_batch take either sampler.  The schedule IS DDIMSampler.make_schedule (same tables, same 'uniform' stride), and
`encode` (DDIM inversion, first order by definition) is DDIMSampler's as it is.

Kernels: CFG combine + PLMS combination + DDIM update are one fused HIP kernel (seer_cfg_plms_step; include/seer_hip.h).  With
`unet.use_graph` on an unsharded SeerUNet every step after the first is ONE hipGraph replay -- seer_ddim_step_begin, the UNet,
seer_cfg_plms_step_dev -- captured once per shape / CFG / scale key by DDIMSampler's capture machinery; the eps history is a
3-slot ring in the graph's static buffers and the kernel walks it itself, so a chain of replays needs no host-written scalar.
The first step (two evaluations) runs launch by launch: a second captured graph would hold a second full set of step
activations in the engine's small graph cache for one step per sample.

The reference draws noise_like(x.shape) in every get_x_prev_and_pred_x0 call, also at sigma = 0 -- twice on the first step, once
on every later one (plms.py:212); those draws are kept (consume_rng_when_deterministic) so a seeded run leaves the device RNG
stream where the reference leaves it.

`guidance_rescale` (DDIMSampler's keyword; per call on sample and p_sample_plms) rescales the guided output of EVERY evaluation, both
of the first step included, in front of the combination: the history then holds rescaled eps.
"""
from __future__ import annotations

import torch

from . import ops
from .ddim import STEP_KINDS, DDIMSampler
from .step_graph import capture_engine


class PLMSSampler(DDIMSampler):
    def make_schedule(self, ddim_num_steps, *args, ddim_eta=0., **kwargs):
        """DDIMSampler.make_schedule; PLMS is deterministic only (plms.py:25-26)"""
        if ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")
        super().make_schedule(ddim_num_steps, *args, ddim_eta=ddim_eta, **kwargs)

    @torch.no_grad()
    def sample(self, unet, S, batch_size, shape, x0_emb=None, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, eta=0., mask=None, x0=None, cond_frames=0, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, null_cond_prob=None, is_3d=False,
               **kwargs):
        size = self._sample_size(S, batch_size, shape, conditioning, eta, verbose, is_3d)
        if noise_dropout > 0.:
            raise NotImplementedError("noise_dropout: only the deterministic PLMS path is built")
        return self.plms_sampling(unet, conditioning, size, x0_emb=x0_emb, is_3d=is_3d, callback=callback,
                                  img_callback=img_callback, cond_frames=cond_frames, temperature=temperature, x_T=x_T,
                                  log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning,
                                  guidance_rescale=kwargs.get("guidance_rescale"))

    @torch.no_grad()
    def plms_sampling(self, unet, cond, shape, is_3d=True, x0_emb=None, cond_frames=0, x_T=None, callback=None,
                      img_callback=None, log_every_t=100, temperature=1., unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, guidance_rescale=None, **kwargs):
        """plms.py:114-170 over the Seer model call"""
        b = shape[0]
        img, x0_emb = self._chain_start(unet, shape, x_T, x0_emb)
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        plain = uc is None or scale == 1.
        phi = self._rescale_factor(unet, guidance_rescale, plain)
        # a chain whose later steps are captured (batched CFG or none, and a model whose steps may be captured at all) runs the two
        # evaluations of its first step launch by launch, not as a UNet graph of their own
        graph = ((plain or uc.shape[2] == cond.shape[2]) and not self._capture_refused
                 and capture_engine(unet, self.ops, img.device) is not None)
        old_eps = []
        chained = False

        def step(img, index):
            nonlocal chained
            first, out = not old_eps, None
            if graph and not first:
                out = self._plms_graph_step(unet, img, cond, None if plain else uc, index, x0_emb, 0 if plain else cond_frames,
                                            scale, old_eps, restart=not chained, phi=phi)
            chained = out is not None
            if out is None:
                if first and graph:
                    unet.use_graph = False
                try:
                    # t_next = time_range[min(i + 1, n - 1)] (plms.py:145)
                    out = self.p_sample_plms(unet, img, cond, self._t_table[index].expand(b), index, x0_emb=x0_emb,
                                             cond_frames=cond_frames, temperature=temperature, unconditional_guidance_scale=scale,
                                             unconditional_conditioning=uc, old_eps=old_eps,
                                             t_next=self._t_table[max(index - 1, 0)].expand(b), guidance_rescale=phi)
                finally:
                    if first and graph:
                        unet.use_graph = True
            old_eps.append(out[2])
            if len(old_eps) >= 4:
                old_eps.pop(0)
            return out[:2]
        return self._run_chain(img, self.ddim_timesteps.shape[0], step, callback, img_callback, log_every_t)

    @torch.no_grad()
    def p_sample_plms(self, unet, x, c, t, index, is_3d=True, x0_emb=None, cond_frames=0, repeat_noise=False,
                      use_original_steps=False, quantize_denoised=False, temperature=1., noise_dropout=0.,
                      score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, old_eps=None, t_next=None, guidance_rescale=None):
        """plms.py:172-236 -> (x_prev, pred_x0, e_t); e_t is this step's (first) CFG-combined eps, the one old_eps keeps.
        Launch by launch (seer_cfg_plms_step; for a v-model seer_v_to_eps in front of each)."""
        if use_original_steps or noise_dropout > 0. or repeat_noise or quantize_denoised or score_corrector is not None:
            raise NotImplementedError("only the deterministic PLMS path over the DDIM subsequence is built")
        x = x.to(torch.float32).contiguous()
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        old_eps = [] if old_eps is None else old_eps
        history = [e.to(torch.float32).contiguous() for e in reversed(old_eps[-3:])]       # newest first
        phi = self._rescale_factor(unet, guidance_rescale, uc is None or scale == 1.)
        eps, cfg, cond_f = self._model_output(unet, x, c, t, x0_emb, cond_frames, uc, scale)
        kw = dict(cfg=cfg, scale=scale, cond_f=cond_f)
        as_eps = lambda out, at, row: self._as_eps(self._rescaled(out, scale, cond_f, phi), at, row, cond_f)
        if not history:
            # pseudo improved Euler: a provisional DDIM step to t_next, a second evaluation there, the mean of the two eps
            if t_next is None:
                raise ValueError("the first PLMS step (old_eps empty) needs t_next")
            self._consume_rng(x)
            x_prov, _, e_t = self.ops.cfg_plms_step(as_eps(eps, x, index), x, self.ddim_coef, index, 0, want_pred_x0=False, **kw)
            eps2, _, _ = self._model_output(unet, x_prov, c, t_next, x0_emb, cond_frames, uc, scale)
            self._consume_rng(x)
            # (a v-model's second evaluation was made at x_prov and at t_next = the timestep of entry max(index - 1, 0): that row)
            x_prev, pred_x0, _ = self.ops.cfg_plms_step(as_eps(eps2, x_prov, max(int(index) - 1, 0)), x, self.ddim_coef, index, 1,
                                                        history=[e_t], **kw)
        else:
            self._consume_rng(x)
            x_prev, pred_x0, e_t = self.ops.cfg_plms_step(as_eps(eps, x, index), x, self.ddim_coef, index, len(history) + 1,
                                                          history=history, **kw)
        return x_prev, pred_x0, e_t

    def _consume_rng(self, x):
        if self.consume_rng_when_deterministic:
            torch.randn(x.shape, device=x.device)    # plms.py:212 draws in every update, also at sigma = 0

    def p_sample_ddim(self, *args, **kwargs):
        raise NotImplementedError("PLMSSampler steps with p_sample_plms")

    def ddim_sampling(self, *args, **kwargs):
        raise NotImplementedError("PLMSSampler samples with plms_sampling")

    def _plms_graph_step(self, unet, x, c, uc, index, x0_emb, cond_frames, scale, old_eps, restart, phi=0.):
        """one later PLMS step as a single replay; `restart` (or a chain the graph did not run last) seeds the ring from old_eps and
        writes the step index and the ring state of that index: the only host writes of a chain.  Returns None when the step
        cannot be captured."""
        G = self._step_graph(unet, x, c, uc, x0_emb, cond_frames, scale, "plms", phi=phi)
        if G is None:
            return None
        if restart or G["expect"] != index or G["ring_host"] is None:
            hist = list(reversed(old_eps[-3:]))                         # newest first -> slots 0, 2, 1
            if hist:
                src = torch.stack([e.to(torch.float32) for e in hist])   # a copy: old_eps may be views of this very ring
                for k in range(len(hist)):
                    G["ring"][(3 - k) % 3].copy_(src[k])
            G["step"][:1].fill_(int(index))
            p = 2 * (int(index) & 1)
            G["ring_state"][p:p + 2].copy_(torch.tensor([len(hist), 0], dtype=torch.int32))
            G["ring_host"] = (len(hist), 0)
        valid, newest = G["ring_host"]
        slot = (newest + 1) % 3
        x_prev, pred_x0 = self._replay_step(G, x, index)
        G["ring_host"] = (min(valid + 1, 3), slot)
        e_t = G["ring"][slot]
        return x_prev, pred_x0, (e_t if self.static_step_outputs else e_t.clone())


# ---- the captured step: DDIMSampler's, with a 3-slot eps ring and seer_cfg_plms_step_dev as its last kernel ------------------------
def _ring_buffers(x):
    return dict(ring=torch.zeros((3, *x.shape), device=x.device, dtype=torch.float32),
                ring_state=torch.zeros((4,), device=x.device, dtype=torch.int32), ring_host=None)


def _plms_update(G, eps, temperature, **kw):
    ops.cfg_plms_step_dev(eps, G["x"], G["coef"], G["step"], G["ring"], G["ring_state"], x_prev=G["x"], pred_x0=G["pred"], **kw)


STEP_KINDS["plms"] = (_ring_buffers, (), _plms_update)
