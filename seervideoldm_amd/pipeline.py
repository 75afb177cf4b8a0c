"""The caller harness of the path -- our counterpart of `inference_img.py:164-187` over tensors.

The reference script loads an image and a prompt, runs CLIP, and then does exactly this with the results; the HF
downloads, PIL / GIF I/O and the CLIP tokenizer / text encoder are not reproduced (their outputs are the inputs here):

    x0_image  [b, 3, f1, H, W] in [-1, 1]  --vae.encode(.).latent_dist.sample() * 0.18215-->  x0_emb [b, 4, f1, H/8, W/8]
    text_emb  [b, 77, 768] (CLIP of the prompt)  --FSTextTransformer-->  c  [b, F, 77, 768]
    empty_emb [b, 77, 768] (CLIP of '')          --unsqueeze(1).expand-->  uc [b, F, 77, 768]   (same frame dim as c: the
                                                                           batched-CFG branch of ddim_video.py:200-204)
    noise = torch.randn(b, 4, F - f1, h, w) drawn on the CPU generator, then moved (inference_img.py:179), redrawn after
    every sample (:187);  `num_samples` sequential ddim_sample calls  ->  clips [b, 3, F - f1, H, W] in [0, 1]

Everything numeric runs in libseer_hip.so through SeerUNet / FSTextTransformer / AutoencoderKL / DDIMSampler.
"""
from __future__ import annotations

import itertools
from typing import Iterable, Iterator, List, Optional, Tuple

import torch

from . import ops
from .ddim import ddim_sample, frames_to_latents, latents_to_clip


@torch.no_grad()
def generate_clips(sunet, fstext_model, vae, sampler, x0_image: torch.Tensor, text_emb: torch.Tensor,
                   empty_emb: torch.Tensor, *, num_frames: int, cond_frames: int, ddim_steps: int = 30,
                   scale: float = 7.5, num_samples: int = 1, noise_generator: Optional[torch.Generator] = None,
                   latent_generator: Optional[torch.Generator] = None,
                   guidance_rescale: Optional[float] = None) -> List[torch.Tensor]:
    """x0_image: [b, 3, 1, H, W] (one image, repeated over the conditioning frames like inference_img.py:166) or
    [b, 3, cond_frames, H, W].  Returns `num_samples` clips [b, 3, num_frames - cond_frames, H, W] in [0, 1].
    `guidance_rescale` (None: the sampler's own) stands in for the sampler's default while these clips are sampled: ddim_sample keeps
    the reference's signature and has no keyword to carry it."""
    dev = x0_image.device
    f1, f2 = cond_frames, num_frames - cond_frames
    if x0_image.shape[2] == 1:
        x0_image = x0_image.expand(-1, -1, f1, -1, -1)
    assert x0_image.shape[2] == f1, "x0_image must hold one frame or cond_frames frames"
    x0_emb = frames_to_latents(vae, x0_image, latent_generator)
    b, c_l, _, h_l, w_l = x0_emb.shape

    fstext_model.set_numframe(num_frames)
    c = fstext_model(context=text_emb)
    uc = empty_emb.unsqueeze(1).expand(-1, c.shape[1], -1, -1).contiguous()

    clips = []
    own = getattr(sampler, "guidance_rescale", 0.)
    if guidance_rescale is not None:
        sampler.guidance_rescale = ops.check_guidance_rescale(guidance_rescale)
    try:
        for _ in range(num_samples):
            noise = torch.randn((b, c_l, f2, h_l, w_l), generator=noise_generator).to(dev)     # CPU draw, then moved (:179,187)
            clips.append(ddim_sample(sampler, sunet, vae, shape=(b, c_l, f2, h_l, w_l), c=c, start_code=noise, x0_emb=x0_emb,
                                     ddim_steps=ddim_steps, scale=scale, uc=uc))
    finally:
        if guidance_rescale is not None:
            sampler.guidance_rescale = own
    return clips


@torch.no_grad()
def generate_queue(sunet, fstext_model, vae, requests: Iterable[dict], *, slots: int, num_frames: int, cond_frames: int,
                   latent_generator: Optional[torch.Generator] = None, max_steps: int = 64,
                   plms: bool = False, stochastic: bool = False, editing: bool = False,
                   dpm: bool = False, prediction_type: str = "epsilon",
                   rescale: bool = False) -> Iterator[Tuple[object, torch.Tensor]]:
    """generate_clips over a queue of requests through a SlotSampler (slots.py): `slots` clips share one captured step and a
    finished clip's slot is refilled at once.  A request is dict(x0_image [1, 3, 1 or cond_frames, H, W], text_emb [1, 77, D],
    empty_emb [1, 77, D], ddim_steps, scale, noise [1, 4, num_frames - cond_frames, H/8, W/8] (the start code), tag, and
    optionally sampler = "ddim" (the default) or "plms").  `plms=True` builds the SlotSampler with plms=True, so that one captured
    step serves requests of either sampler; a request naming "plms" without it is a ValueError.  `stochastic=True` builds it with
    stochastic=True: a request may then carry seed, eta and temperature (SlotSampler.submit), and `noise` is optional when it has a
    seed -- the start code is then drawn from the seed; in a queue started without it those keys are a ValueError.  `editing=True`
    builds it with editing=True: a request may then carry mask with known (the given latents, SlotSampler.submit's x0; they need a
    seed) and t_start; in a queue started without it those keys are a ValueError as well.  `dpm=True`
    builds it with dpm=True: a request may then name sampler = "dpmpp" and carry order, lower_order_final and discretize
    (SlotSampler.submit); a request naming "dpmpp" without it is a ValueError.  `prediction_type="v_prediction"`
    builds it for a model fine-tuned on the velocity target: it belongs to the queue, not to a request.  `rescale=True` builds it with
    rescale=True: a request may then carry guidance_rescale (SlotSampler.submit); in a queue started without it a non-zero value is a
    ValueError.  The VAE encode
    (drawing from `latent_generator`, in admission order) and FSText run when a request is admitted -- it is taken from the iterable
    only when a slot is free -- and the VAE decode, 1/0.18215 and clamp01 when its clip finishes, as ddim_sample does them.  Yields
    (tag, clip [1, 3, num_frames - cond_frames, H, W] in [0, 1]) in finishing order.  Every request has the shape of the first."""
    from .slots import SlotSampler
    from .step_cache import refuse
    refuse(sunet, "generate_queue")
    f1, f2 = cond_frames, num_frames - cond_frames
    fstext_model.set_numframe(num_frames)
    sampler: List[SlotSampler] = []

    def admitted():
        for r in requests:
            method = r.get("sampler", "ddim")
            if method not in ("ddim", "plms", "dpmpp") or (method == "plms" and not plms) or (method == "dpmpp" and not dpm):
                raise ValueError(f"sampler = {method!r}: 'ddim', 'plms' in a queue started with plms=True, or 'dpmpp' in one started "
                                 "with dpm=True")
            x0_image = r["x0_image"]
            if x0_image.shape[2] == 1:
                x0_image = x0_image.expand(-1, -1, f1, -1, -1)
            assert x0_image.shape[0] == 1 and x0_image.shape[2] == f1, "x0_image must hold one clip of one frame or cond_frames frames"
            x0_emb = frames_to_latents(vae, x0_image, latent_generator)
            c = fstext_model(context=r["text_emb"])
            uc = r["empty_emb"].unsqueeze(1).expand(-1, c.shape[1], -1, -1).contiguous()
            if not sampler:
                _, c_l, _, h_l, w_l = x0_emb.shape
                sampler.append(SlotSampler(sunet, slots, shape=(c_l, f2, h_l, w_l), cond_frames=f1, context_shape=tuple(c.shape[2:]),
                                           max_steps=max_steps, device=x0_emb.device, plms=plms, stochastic=stochastic,
                                           **(dict(editing=True) if editing else {}), **(dict(dpm=True) if dpm else {}),
                                           **(dict(prediction_type=prediction_type) if prediction_type != "epsilon" else {}),
                                           **(dict(rescale=True) if rescale else {})))
            seeded = {k: r[k] for k in ("seed", "eta", "temperature") if k in r}
            edit = {k: r[k] for k in ("mask", "known", "t_start") if r.get(k) is not None}
            solver = {k: r[k] for k in ("order", "lower_order_final", "discretize", "guidance_rescale") if k in r}
            if solver.get("guidance_rescale") and not rescale:
                raise ValueError("guidance_rescale: a request carries it only in a queue started with rescale=True")
            if edit and not editing:
                raise ValueError(f"{sorted(edit)}: a request carries these only in a queue started with editing=True")
            if "known" in edit:
                edit["x0"] = edit.pop("known")
            if seeded and not stochastic and not (editing and "mask" in edit and set(seeded) == {"seed"}):
                raise ValueError(f"{sorted(seeded)}: a request carries these only in a queue started with stochastic=True")
            if r.get("noise") is None and seeded.get("seed") is None:
                raise ValueError("a request needs `noise` (its start code) or, in a queue started with stochastic=True, a `seed`")
            yield dict(x_T=r.get("noise"), x0_emb=x0_emb, c=c, uc=uc, S=r.get("ddim_steps", 30), scale=r.get("scale", 7.5),
                       tag=r.get("tag"), method=method, **seeded, **edit, **solver)

    reqs = admitted()
    first = next(reqs, None)
    if first is None:
        return
    for tag, lat in sampler[0].run(itertools.chain([first], reqs)):
        yield tag, latents_to_clip(vae, lat)


def edit_t_enc(strength: float, entries: int) -> int:
    """the level an edit of `strength` in (0, 1] starts from, out of a schedule of `entries`: max(1, int(strength * entries)), kept at
    or below entries - 1 because stochastic_encode indexes the schedule tables with it (CompVis ddim.py:207-221)"""
    if not 0. < float(strength) <= 1.:
        raise ValueError(f"strength = {strength}: in (0, 1]")
    if int(entries) < 2:
        raise ValueError(f"a schedule of {entries} entries leaves no level to edit from")
    return min(max(1, int(float(strength) * int(entries))), int(entries) - 1)


@torch.no_grad()
def edit_clips(sunet, fstext_model, vae, sampler, video: torch.Tensor, text_emb: torch.Tensor, empty_emb: torch.Tensor, *,
               cond_frames: int, ddim_steps: int = 30, scale: float = 7.5, strength: Optional[float] = None,
               keep_mask: Optional[torch.Tensor] = None, seed, latent_generator: Optional[torch.Generator] = None,
               invert: bool = False, source_emb: Optional[torch.Tensor] = None, source_scale: float = 1.0,
               guidance_rescale: Optional[float] = None) -> torch.Tensor:
    """Edit an existing clip.  `video` [b, 3, F, H, W] in [-1, 1] is VAE-encoded in one call (as evaluate_batch does; the posterior
    draw takes `latent_generator`); its first `cond_frames` latents condition the clip, the rest are the GIVEN latents.  Exactly one of
      strength   in (0, 1] (SDEdit): the given latents are noised to level t_enc = edit_t_enc(strength, schedule entries) by
                 sampler.stochastic_encode and denoised from there by sampler.decode(t_start=t_enc);
      keep_mask  [b, 1, F - cond_frames, H/8, W/8], 1 where the given latents are kept: masked sampling from a seeded start code.
    Every draw of the sampler comes from `seed` (an int, or one per row).  Returns the clips [b, 3, F - cond_frames, H, W] in [0, 1]
    like generate_clips.
    `invert=True` (with `strength`; `keep_mask` is refused) replaces the re-noising by DDIM inversion: sampler.encode carries the given
    latents up to t_enc with the model in the loop, under `source_emb` (the prompt that describes `video`; default `text_emb`) at
    guidance `source_scale` (its unconditional branch is `empty_emb` when that scale is not 1), and sampler.decode brings them back
    under `text_emb` at `scale`: the clip itself under the source prompt, a structure-preserving edit under another.  Nothing is
    drawn on this path, so `seed` may be None.  A sampler built with prediction_type="v_prediction" refuses it (NotImplementedError,
    DDIMSampler.encode), before anything is encoded.  `guidance_rescale` (None: the sampler's own) goes to every sample, encode and
    decode call made here."""
    gr = {} if guidance_rescale is None else dict(guidance_rescale=ops.check_guidance_rescale(guidance_rescale))
    if invert:
        if getattr(sampler, "prediction_type", "epsilon") != "epsilon":
            sampler._refuse_v_inversion()
        if keep_mask is not None:
            raise ValueError("edit_clips: invert=True inverts the whole clip; `keep_mask` belongs to masked sampling")
        if strength is None:
            raise ValueError("edit_clips: invert=True needs `strength`, the level the clip is inverted to")
    elif (strength is None) == (keep_mask is None):
        raise ValueError("edit_clips: exactly one of `strength` and `keep_mask`")
    b, _, F, H, W = video.shape
    f1 = int(cond_frames)
    if not 0 <= f1 < F:
        raise ValueError(f"cond_frames = {cond_frames} of a video of {F} frames")
    if strength is not None:
        sampler.make_schedule(ddim_num_steps=ddim_steps, ddim_eta=0.0, verbose=False)
        t_enc = edit_t_enc(strength, int(sampler.ddim_timesteps.shape[0]))
    lat = frames_to_latents(vae, video, latent_generator)
    x0_emb, given = (lat[:, :, :f1].contiguous() if f1 else None), lat[:, :, f1:].contiguous()
    fstext_model.set_numframe(F)
    c = fstext_model(context=text_emb)
    uc = None if scale == 1.0 else empty_emb.unsqueeze(1).expand(-1, c.shape[1], -1, -1).contiguous()
    if keep_mask is not None:
        samples, _ = sampler.sample(unet=sunet, S=ddim_steps, conditioning=c, batch_size=b, shape=given.shape[1:], x0_emb=x0_emb,
                                    verbose=False, unconditional_guidance_scale=scale, unconditional_conditioning=uc, eta=0.0,
                                    is_3d=True, seed=seed, mask=keep_mask, x0=given, **gr)
    elif invert:
        c_src = c if source_emb is None or source_emb is text_emb else fstext_model(context=source_emb)
        uc_src = None if source_scale == 1.0 else empty_emb.unsqueeze(1).expand(-1, c_src.shape[1], -1, -1).contiguous()
        noised, _ = sampler.encode(sunet, given, c_src, t_enc, unconditional_guidance_scale=source_scale,
                                   unconditional_conditioning=uc_src, x0_emb=x0_emb, **gr)
        samples = sampler.decode(sunet, noised, c, t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=uc,
                                 x0_emb=x0_emb, **gr)
    else:
        noised = sampler.stochastic_encode(given, t_enc, seed=seed)
        samples = sampler.decode(sunet, noised, c, t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=uc,
                                 x0_emb=x0_emb, seed=seed, **gr)
    return latents_to_clip(vae, samples)


def concat_all_gather(t: torch.Tensor, process_group=None) -> torch.Tensor:
    """eval.py's `concat_all_gather(accelerator, t)` (= accelerator.gather): the per-rank batches stacked in rank order"""
    import torch.distributed as dist
    # None = the default (WORLD) group, as accelerator.gather always gathers over WORLD (eval.py:226-231)
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(process_group) == 1:
        return t
    t = t.contiguous()
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size(process_group))]
    dist.all_gather(parts, t, group=process_group)
    return torch.cat(parts, 0)


@torch.no_grad()
def evaluate_batch(sunet, fstext_model, vae, sampler, video: torch.Tensor, text_emb: torch.Tensor, empty_emb: torch.Tensor, *,
                   cond_frames: int, ddim_steps: int = 30, scale: float = 7.5, process_group=None, gather: bool = True,
                   noise_generator: Optional[torch.Generator] = None, latent_generator: Optional[torch.Generator] = None,
                   guidance_rescale: Optional[float] = None):
    """The body of eval.py's validation loop (eval.py:186-231) for THIS rank's batch: the first `cond_frames` frames of
    `video` [b, 3, F, H, W] in [-1, 1] condition the rest; returns (pred, gt) = ([conditioning frames | sampled frames],
    ground truth), both [N*b, 3, F, H, W] in [0, 1] gathered over the ranks of `process_group` (None = every rank, as
    accelerator.gather does) in rank order.  N GPUs evaluate N batches with no communication until this final gather (the
    samples are the independent units of the path); gather=False returns this rank's batch only.  `guidance_rescale` (None: the
    sampler's own) is generate_clips' keyword."""
    x0 = video[:, :, :cond_frames]
    clip = generate_clips(sunet, fstext_model, vae, sampler, x0, text_emb, empty_emb, num_frames=video.shape[2],
                          cond_frames=cond_frames, ddim_steps=ddim_steps, scale=scale, num_samples=1,
                          noise_generator=noise_generator, latent_generator=latent_generator, guidance_rescale=guidance_rescale)[0]
    pred = torch.cat([(x0.float() + 1.0) / 2.0, clip], dim=2)
    gt = (video.float() + 1.0) / 2.0
    if not gather:
        return pred, gt
    return concat_all_gather(pred, process_group), concat_all_gather(gt, process_group)
