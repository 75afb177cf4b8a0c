"""The mask blend of an edited clip at BASELINE config 2 (b = 1 with batched CFG, F = 12 with 2 conditioning frames, 32x32 latent, bf16,
full-size UNet with closed-form weights), S = 30, eta = 0, unet.use_graph on:

  * one seer_known_blend launch on the config-2 latent [1, 4, 10, 32, 32] (40 960 elements, a mask that keeps half of them): 200
    launches captured into one graph, the replay timed by device events and divided by 200;
  * the captured step without a seed (the deterministic "step" graph: the path of bench.py), with a seed ("step-rng") and with a seed
    and a mask ("step-mask": the same graph with the blend as its first node).

The step variants alternate inside one process; a step's time is the median over the steps of a sample after the first (device events
recorded by `callback`), a variant's figure the median over the samples, with the spread printed.

    python scripts/exp_edit_step.py [--samples 5] [--steps 30]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def blend_launch_us(dev, shape, n=200, rounds=20):
    from seervideoldm_amd import DDIMSampler, ops
    b, Cc, Fp, h, w = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(shape, generator=g).to(dev)
    known = torch.randn(shape, generator=g).to(dev)
    mask = (torch.rand((b, Fp, h, w), generator=g) < 0.5).float().to(dev)
    seeds = ops.seed_words([1234] * b).to(dev)
    smp = DDIMSampler(dev)
    smp.make_schedule(30, verbose=False)
    step = torch.tensor([15, 15], dtype=torch.int32, device=dev)
    ops.known_blend(x, mask, known, smp.ddim_coef, step=step, seeds=seeds)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            ops.known_blend(x, mask, known, smp.ddim_coef, step=step, seeds=seeds)
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        e.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(e) * 1e3 / n)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    from seervideoldm_amd import DDIMSampler, SeerUNet, synth
    dev = torch.device("cuda:0")
    b, f1, F, h = 1, 2, 12, 32
    us = blend_launch_us(dev, (b, 4, F - f1, h, h))
    print(f"known_blend, one launch inside a graph of 200 ({4 * (F - f1) * h * h} elements, half kept): median {statistics.median(us):.3f} us, "
          f"min {min(us):.3f}, max {max(us):.3f} over {len(us)} replays", flush=True)
    cfg = dict(synth.SD15_UNET_CFG)
    model = SeerUNet(**cfg).to(dev)
    model.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg), device=dev), strict=True)
    model.eval()
    model.use_graph = True
    g = torch.Generator().manual_seed(0)
    x_T = torch.randn((b, 4, F - f1, h, h), generator=g).to(dev)
    x0_emb = (torch.randn((b, 4, f1, h, h), generator=g) * 0.18215 * 5).to(dev)
    c = torch.randn((b, F, 77, 768), generator=g).to(dev)
    uc = torch.randn((b, 1, 77, 768), generator=g).expand(-1, F, -1, -1).contiguous().to(dev)
    known = (torch.randn((b, 4, F - f1, h, h), generator=g) * 0.18215 * 5).to(dev)
    mask = (torch.rand((b, 1, F - f1, h, h), generator=g) < 0.5).float().to(dev)
    variants = {"eta0_captured": dict(), "eta0_seeded_captured": dict(seed=1234),
                "eta0_seeded_masked_captured": dict(seed=1234, mask=mask, x0=known)}
    samplers = {name: DDIMSampler(dev) for name in variants}

    def one_sample(name):
        events = []

        def cb(i):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            events.append(ev)
        torch.cuda.synchronize()
        start = torch.cuda.Event(enable_timing=True)
        start.record()
        lat, _ = samplers[name].sample(unet=model, S=args.steps, conditioning=c, batch_size=b, shape=(4, F - f1, h, h), x0_emb=x0_emb,
                                       verbose=False, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, x_T=x_T,
                                       is_3d=True, callback=cb, eta=0.0, **variants[name])
        torch.cuda.synchronize()
        marks = [start] + events
        per = [marks[i].elapsed_time(marks[i + 1]) for i in range(len(events))]
        assert torch.isfinite(lat).all()
        return statistics.median(per[1:])

    for name in variants:
        one_sample(name)                               # capture + caches
    res = {name: [] for name in variants}
    for _ in range(args.samples):
        for name in variants:                          # alternating: a drift of the machine hits every variant alike
            res[name].append(round(one_sample(name), 4))
    for name, s in res.items():
        print(f"{name}: step (median of {len(s)} samples) {statistics.median(s):.4f} ms, min {min(s):.4f}, max {max(s):.4f}", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print(f"masked - seeded = {(med['eta0_seeded_masked_captured'] - med['eta0_seeded_captured']) * 1e3:+.1f} us, "
          f"seeded - unseeded = {(med['eta0_seeded_captured'] - med['eta0_captured']) * 1e3:+.1f} us")
    keys = sorted({str(k[0]) for k in model._engine._graphs if isinstance(k, tuple) and k})
    print(json.dumps(dict(known_blend_us=[round(v, 3) for v in us], step_ms=res, graph_keys=keys)))


if __name__ == "__main__":
    main()
