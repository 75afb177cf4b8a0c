"""The eta > 0 DDIM step at BASELINE config 2 (b = 1 with batched CFG, F = 12 with 2 conditioning frames, 32x32 latent, bf16, full-size
UNet with closed-form weights), S = 30, unet.use_graph on:

  * unseeded, eta = 0.5: every step launch by launch around the UNet's own graph, a torch.randn between two UNet evaluations
    (what DDIMSampler did before `seed` existed, and still does without one);
  * seeded, eta = 0.5: ONE replay per step, the noise drawn inside seer_cfg_ddim_step (seeds, device index);
  * eta = 0, unseeded: the deterministic captured step, for scale.

The variants alternate inside one process; a step's time is the median over the steps of a sample after the first (device events
recorded by `callback`), a variant's figure the median over the samples, with the spread printed.

    python scripts/exp_stoch_step.py [--samples 5] [--steps 30]
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
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    from seervideoldm_amd import DDIMSampler, SeerUNet, synth
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
    variants = {"eta0.5_unseeded_eager": dict(eta=0.5), "eta0.5_seeded_captured": dict(eta=0.5, seed=1234), "eta0_captured": dict(eta=0.0)}
    samplers = {name: DDIMSampler(dev) for name in variants}

    def one_sample(name):
        events = []

        def cb(i):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            events.append(ev)
        torch.cuda.synchronize()
        start = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        lat, _ = samplers[name].sample(unet=model, S=args.steps, conditioning=c, batch_size=b, shape=(4, F - f1, h, h), x0_emb=x0_emb,
                                       verbose=False, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, x_T=x_T,
                                       is_3d=True, callback=cb, **variants[name])
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        marks = [start] + events
        per = [marks[i].elapsed_time(marks[i + 1]) for i in range(len(events))]
        assert torch.isfinite(lat).all()
        return wall, statistics.median(per[1:])

    for name in variants:
        one_sample(name)                               # capture + caches
    res = {name: dict(wall_ms=[], step_ms=[]) for name in variants}
    for _ in range(args.samples):
        for name in variants:                          # alternating: a drift of the machine hits every variant alike
            wall, step = one_sample(name)
            res[name]["wall_ms"].append(round(wall, 3))
            res[name]["step_ms"].append(round(step, 4))
    for name, r in res.items():
        s = r["step_ms"]
        print(f"{name}: step (median of {len(s)} samples) {statistics.median(s):.4f} ms, min {min(s):.4f}, max {max(s):.4f}; "
              f"sample wall {statistics.median(r['wall_ms']):.2f} ms", flush=True)
    e, s = (statistics.median(res[k]["step_ms"]) for k in ("eta0.5_unseeded_eager", "eta0.5_seeded_captured"))
    res["seeded_over_unseeded_step"] = round(s / e, 4)
    res["graph_keys"] = sorted({str(k[0]) for k in model._engine._graphs if isinstance(k, tuple) and k})
    print(f"seeded captured step / unseeded eager step = {s / e:.4f} ({(s - e) * 1e3:+.1f} us)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
