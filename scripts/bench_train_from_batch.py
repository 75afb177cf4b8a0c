"""What a real fine-tuning loop pays per step at BASELINE config 5 (b = 1, 2 + 12 frames of 256x256 pixels, full-size SeerUNet,
8-layer FSTextTransformer, SD VAE encoder, CLIP ViT-L/14 text tower; random-init weights, synthetic pixels and token ids):
    new     SeerTrainer.step_from_batch(use_graph=True)                                  train.py:330-387 in one call
    manual  text encoder, two vae.encode(...).latent_dist.sample() * 0.18215, torch.randn / randint, SeerTrainer.train_step
            (INTEGRATION.md 1a "what it does"; train_step's add_noise and concat are torch expressions)
plus the parts: the VAE encode (14 frames in one call; 12 + 2 in two), the text tower, and seer_train_inputs alone against the bytes
it moves.  Host clock around a synchronised block, 5 warm-up + 20 timed steps each.  Usage:
    python scripts/bench_train_from_batch.py new|manual|parts [steps] [warmup]          (one JSON line)"""
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from seervideoldm_amd import AutoencoderKL, synth, train_ops  # noqa: E402
from seervideoldm_amd.clip_text import CLIPTextEncoder  # noqa: E402
from seervideoldm_amd.trainer import SeerTrainer, ddpm_alphas_cumprod  # noqa: E402
from seervideoldm_amd.vae import ldm_to_diffusers_vae  # noqa: E402
from scripts.bench_train import build  # noqa: E402

B, F1, F2, PIX, LAT = 1, 2, 12, 256, 32


def frozen(device):
    vae = AutoencoderKL()
    vae.load_state_dict(ldm_to_diffusers_vae(synth.synth_state_dict(synth.vae_encoder_param_shapes()), 4), strict=True)
    g = torch.Generator().manual_seed(0)
    sd = {k: (0.02 * torch.randn(s, generator=g) if len(s) == 2 else
              0.1 * torch.randn(s, generator=g) + (1.0 if "norm" in k and k.endswith("weight") else 0.0))
          for k, s in synth.clip_text_param_shapes().items()}
    clip = CLIPTextEncoder()
    clip.load_state_dict(sd, strict=True)
    return vae.to(device), clip.to(device)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    mode = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    video = (torch.rand((B, 3, F1 + F2, PIX, PIX), generator=g) * 2 - 1).to(dev)
    ids = torch.randint(0, 49408, (B, 77), generator=g)
    mask = torch.ones((B, 77), dtype=torch.int64)
    acp = ddpm_alphas_cumprod().to(dev)
    vae, clip = frozen(dev)
    out = {"mode": mode, "steps": steps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
           "config": f"b={B} frames={F1}+{F2} pixels={PIX}x{PIX} (BASELINE config 5), bf16 UNet, fp16 VAE, hipGraph forward+backward"}
    if mode in ("new", "manual"):
        unet, fst = build(dev)
        fst.set_numframe(F1 + F2)
        tr = SeerTrainer(unet, fst, lr=1e-5, max_grad_norm=0.3)
        if mode == "new":
            def step():
                return tr.step_from_batch(video, ids, mask, vae=vae, text_encoder=clip, cond_frames=F1, alphas_cumprod=acp,
                                          use_graph=True)
        else:
            def step():
                text = clip(ids, attention_mask=mask)[0]
                x0 = video[:, :, :F1].permute(0, 2, 1, 3, 4).reshape(B * F1, 3, PIX, PIX)
                im = video[:, :, F1:].permute(0, 2, 1, 3, 4).reshape(B * F2, 3, PIX, PIX)
                lat = vae.encode(im).latent_dist.sample() * 0.18215
                lat0 = vae.encode(x0).latent_dist.sample() * 0.18215
                lat0 = lat0.view(B, F1, 4, LAT, LAT).permute(0, 2, 1, 3, 4)
                lat = lat.view(B, F2, 4, LAT, LAT).permute(0, 2, 1, 3, 4)
                noise = torch.randn(lat.shape).to(dev)
                t = torch.randint(0, 1000, (B,), device=dev)
                return tr.train_step(lat0, lat, noise, t, text, acp, use_graph=True)
        out["ms_per_step"] = timed(step, steps, warmup)
        out["loss_last"] = float(step())
        out["hipgraph"] = not getattr(tr, "_graph_broken", False)
    else:
        frames = video.permute(0, 2, 1, 3, 4).reshape(B * (F1 + F2), 3, PIX, PIX).contiguous()
        out["vae_encode_14_ms"] = timed(lambda: vae.encode(frames), steps, warmup)
        out["vae_encode_12_plus_2_ms"] = timed(lambda: (vae.encode(frames[F1:]), vae.encode(frames[:F1])), steps, warmup)
        out["clip_text_ms"] = timed(lambda: clip(ids, attention_mask=mask), steps, warmup)
        mom = vae.encode(frames).latent_dist.parameters
        eps = torch.randn((B * (F1 + F2), 4, LAT, LAT), device=dev)
        noise = torch.randn((B, 4, F2, LAT, LAT), device=dev)
        t = torch.tensor([500] * B, device=dev)
        x = torch.empty((B, 4, F1 + F2, LAT, LAT), device=dev)
        n = 200
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        call = lambda: train_ops.train_inputs(mom, eps, noise, t, acp, F1, out=x, _timesteps_in_range=True)
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):                          # back-to-back launches without the host's launch rate in between
            for _ in range(n):
                call()
        gr.replay()
        torch.cuda.synchronize()
        ev0.record()
        gr.replay()
        ev1.record()
        torch.cuda.synchronize()
        words = B * 4 * LAT * LAT * (3 * (F1 + F2) + F2 + (F1 + F2))   # mean, logvar, eps per element; noise; the output
        out["train_inputs_us"] = ev0.elapsed_time(ev1) * 1e3 / n
        out["train_inputs_bytes"] = 4 * words
        out["train_inputs_gb_per_s"] = 4 * words / (out["train_inputs_us"] * 1e-6) / 1e9
        # the torch expressions this launch stands for (sample, scale, rearranges, add_noise, cat), eager, same inputs
        def glue():
            z = train_ops.ops.gaussian_sample(mom, eps) * 0.18215
            z = z.view(B, F1 + F2, 4, LAT, LAT).permute(0, 2, 1, 3, 4)
            a = acp[t].reshape(-1, 1, 1, 1, 1)
            return torch.cat([z[:, :, :F1], a.sqrt() * z[:, :, F1:] + (1 - a).sqrt() * noise], 2)
        out["manual_glue_ms"] = timed(glue, 200, 20)
        out["train_inputs_eager_call_ms"] = timed(call, 200, 20)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
