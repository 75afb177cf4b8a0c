"""DDIM inversion at BASELINE config 2 (b = 1 with batched CFG, F = 12 with 2 conditioning frames, 32x32 latent, bf16, full-size UNet
with closed-form weights), guidance 7.5:

  * the captured DDIM step of `sample` (the deterministic "step" graph: the path of bench.py), the captured inversion step of `encode`
    ("invert": the same UNet graph with seer_cfg_ddim_invert_step in its device form as its last kernel) and `encode` launch by launch
    (unet.use_graph off).  The variants alternate inside one process; a step's time is the median over the steps of a chain after the
    first (device events recorded by `callback`), a variant's figure the median over the chains, with the spread printed;
  * the round trip encode -> decode on the mini UNet of the sampler tests (closed-form weights, no guidance, the whole schedule) at
    S = 10, 20, 50: rel-L2 of the returned latents to the given ones.

    python scripts/exp_invert_step.py [--samples 5] [--steps 30]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

CFG_MINI = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)


def round_trips(dev):
    from seervideoldm_amd import DDIMSampler, SeerUNet, synth
    m = SeerUNet(**CFG_MINI)
    m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI)), strict=True)
    m = m.to(dev).eval()
    m.use_graph = True
    g = torch.Generator().manual_seed(3)
    b, f1, Fp, H = 1, 1, 2, 16
    x0_emb = (torch.randn((b, 4, f1, H, H), generator=g) * 0.9).to(dev)
    c = torch.randn((b, f1 + Fp, 77, CFG_MINI["cross_attention_dim"]), generator=g).to(dev)
    x0 = (torch.randn((b, 4, Fp, H, H), generator=g) * 0.8).to(dev)
    out = {}
    for S in (10, 20, 50):
        smp = DDIMSampler(dev)
        smp.make_schedule(S, verbose=False)
        n = int(smp.ddim_timesteps.shape[0])
        up, _ = smp.encode(m, x0, c, n, x0_emb=x0_emb)
        down = smp.decode(m, up, c, n, x0_emb=x0_emb)
        noised = smp.stochastic_encode(x0, n - 1, seed=7)
        sde = smp.decode(m, noised, c, n, x0_emb=x0_emb)
        rel = lambda a: float((a.double() - x0.double()).norm() / x0.double().norm())
        out[S] = dict(entries=n, invert=rel(down), stochastic=rel(sde), finite=bool(torch.isfinite(down).all()))
        print(f"round trip on the mini UNet, S = {S} ({n} entries), no guidance: encode -> decode {out[S]['invert']:.4g}, "
              f"stochastic_encode -> decode {out[S]['stochastic']:.4g}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    from seervideoldm_amd import DDIMSampler, SeerUNet, synth
    dev = torch.device("cuda:0")
    quality = round_trips(dev)
    b, f1, F, h = 1, 2, 12, 32
    cfg = dict(synth.SD15_UNET_CFG)
    model = SeerUNet(**cfg).to(dev)
    model.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg), device=dev), strict=True)
    model.eval()
    g = torch.Generator().manual_seed(0)
    x_T = torch.randn((b, 4, F - f1, h, h), generator=g).to(dev)
    x0_emb = (torch.randn((b, 4, f1, h, h), generator=g) * 0.18215 * 5).to(dev)
    c = torch.randn((b, F, 77, 768), generator=g).to(dev)
    uc = torch.randn((b, 1, 77, 768), generator=g).expand(-1, F, -1, -1).contiguous().to(dev)
    given = (torch.randn((b, 4, F - f1, h, h), generator=g) * 0.18215 * 5).to(dev)
    sampler = DDIMSampler(dev)
    sampler.make_schedule(args.steps, verbose=False)
    n = int(sampler.ddim_timesteps.shape[0])
    finite = {}

    def ddim(cb):
        return sampler.sample(unet=model, S=args.steps, conditioning=c, batch_size=b, shape=(4, F - f1, h, h), x0_emb=x0_emb, verbose=False,
                              unconditional_guidance_scale=7.5, unconditional_conditioning=uc, x_T=x_T, is_3d=True, callback=cb, eta=0.0)[0]

    def invert(cb):
        return sampler.encode(model, given, c, n, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, callback=cb,
                              x0_emb=x0_emb)[0]
    variants = {"ddim_captured": (ddim, True), "invert_captured": (invert, True), "invert_launches": (invert, False)}

    def one_chain(name):
        run, graph = variants[name]
        events = []

        def cb(i):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            events.append(ev)
        model.use_graph = graph
        torch.cuda.synchronize()
        start = torch.cuda.Event(enable_timing=True)
        start.record()
        lat = run(cb)
        torch.cuda.synchronize()
        marks = [start] + events
        per = [marks[i].elapsed_time(marks[i + 1]) for i in range(len(events))]
        assert len(per) == n
        finite[name] = bool(torch.isfinite(lat).all())
        return statistics.median(per[1:])

    for name in variants:
        one_chain(name)                                # capture + caches
    res = {name: [] for name in variants}
    for _ in range(args.samples):
        for name in variants:                          # alternating: a drift of the machine hits every variant alike
            res[name].append(round(one_chain(name), 4))
    for name, s in res.items():
        print(f"{name}: step (median of {len(s)} chains of {n} steps) {statistics.median(s):.4f} ms, min {min(s):.4f}, max {max(s):.4f}, "
              f"finite {finite[name]}", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print(f"invert - ddim (captured) = {(med['invert_captured'] - med['ddim_captured']) * 1e3:+.1f} us; launches - captured = "
          f"{(med['invert_launches'] - med['invert_captured']) * 1e3:+.1f} us")
    keys = sorted({str(k[0]) for k in model._engine._graphs if isinstance(k, tuple) and k})
    print(json.dumps(dict(step_ms=res, finite=finite, graph_keys=keys, round_trip=quality)))


if __name__ == "__main__":
    main()
