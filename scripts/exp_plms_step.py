"""PLMS against DDIM at BASELINE config 2 (b = 1 with batched CFG, F = 12 with 2 conditioning frames, 32x32 latent, bf16, full-size
UNet with closed-form weights), S = 30, both samplers captured (unet.use_graph):

  * the steady captured step of each sampler, ms (median over the replayed steps of a sample; events recorded by `callback`);
  * the first PLMS step (two UNet evaluations, launch by launch) and the first DDIM step;
  * the wall time of a whole 30-step sample with each sampler.

    python scripts/exp_plms_step.py [--samples 3] [--steps 30]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    from seervideoldm_amd import DDIMSampler, PLMSSampler, SeerUNet, synth
    dev = torch.device("cuda:0")
    cfg = dict(synth.SD15_UNET_CFG)
    model = SeerUNet(**cfg).to(dev)
    model.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg), device=dev), strict=True)
    model.eval()
    model.use_graph = True
    g = torch.Generator().manual_seed(0)
    b, f1, F, h = 1, 2, 12, 32
    x_T = torch.randn((b, 4, F - f1, h, h), generator=g).to(dev)
    x0_emb = (torch.randn((b, 4, f1, h, h), generator=g) * 0.18215 * 5).to(dev)
    c = torch.randn((b, F, 77, 768), generator=g).to(dev)
    uc = torch.randn((b, 1, 77, 768), generator=g).expand(-1, F, -1, -1).contiguous().to(dev)

    def one_sample(sampler):
        events = []

        def cb(i):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            events.append(ev)
        torch.cuda.synchronize()
        start = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        lat, _ = sampler.sample(unet=model, S=args.steps, conditioning=c, batch_size=b, shape=(4, F - f1, h, h), x0_emb=x0_emb,
                                verbose=False, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0,
                                x_T=x_T, is_3d=True, callback=cb)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        marks = [start] + events
        per = [marks[i].elapsed_time(marks[i + 1]) for i in range(len(events))]
        assert torch.isfinite(lat).all()
        return wall, per

    res = {}
    for name, cls in (("ddim", DDIMSampler), ("plms", PLMSSampler)):
        sampler = cls(dev)
        one_sample(sampler)                        # capture + caches
        walls, firsts, steady = [], [], []
        for _ in range(args.samples):
            wall, per = one_sample(sampler)
            walls.append(wall)
            firsts.append(per[0])
            steady.append(statistics.median(per[1:]))
        res[name] = dict(steps=len(per), wall_ms=[round(v, 3) for v in walls], first_step_ms=[round(v, 3) for v in firsts],
                         steady_step_ms_median=[round(v, 3) for v in steady])
        print(f"{name}: {len(per)} steps/sample; wall {statistics.median(walls):.2f} ms; first step "
              f"{statistics.median(firsts):.3f} ms; steady step (median) {statistics.median(steady):.4f} ms", flush=True)
    d, p = (statistics.median(res[k]["steady_step_ms_median"]) for k in ("ddim", "plms"))
    res["plms_over_ddim_steady_step"] = round(p / d, 4)
    res["graph_keys"] = sorted({str(k[0]) for k in model._engine._graphs if isinstance(k, tuple) and k})
    print(f"steady PLMS step / DDIM step = {p / d:.4f} ({(p - d) * 1e3:+.1f} us)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
